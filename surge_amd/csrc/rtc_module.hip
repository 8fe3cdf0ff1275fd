// rtc_module.hip — the run-time compiled programs a process has loaded: one cache for every kind of program (the v1 flat
// and lane kernels of an op table, fold_v1_spec.hip; the v2 slot kernels of a schema, fold_slots.hip) and the one way a
// kernel of such a module is launched.  rtc.cpp turns a program's text into a code object (hiprtc, or the cache on disk);
// here the code object becomes a module of this process and its entry points functions.
#include <cstdlib>
#include <map>
#include <memory>
#include <mutex>

#include "replay_internal.h"

namespace surge {
namespace {

std::mutex g_mu;  // (one for all kinds: a compile runs under it, as it always has)
// key: the program's kind, what its text depends on, the device; entries live as long as the process (a handful of
// schemas per host; a module is a few tens of KB)
std::map<std::string, std::unique_ptr<RtcModule>> g_loaded;
std::map<std::string, std::string> g_failed;  // key -> why (never retried: the answer will not change)

}  // namespace

bool rtc_disabled(std::string* why) {
  const char* v = std::getenv("SURGE_REPLAY_RTC");
  if (!v || std::atoi(v) != 0) return false;
  *why = "disabled by SURGE_REPLAY_RTC=0";
  return true;
}

const RtcModule* rtc_module_acquire(const std::string& program_key, int device, const std::function<std::string()>& source,
                                    const std::vector<const char*>& entry_points, std::string* why) {
  if (rtc_disabled(why)) return nullptr;
  const std::string key = program_key + "@" + std::to_string(device);
  std::lock_guard<std::mutex> lk(g_mu);
  auto hit = g_loaded.find(key);
  if (hit != g_loaded.end()) return hit->second.get();
  auto miss = g_failed.find(key);
  if (miss != g_failed.end()) {
    *why = miss->second;
    return nullptr;
  }
  auto give_up = [&](const std::string& msg) -> const RtcModule* {
    g_failed[key] = msg;
    *why = msg;
    return nullptr;
  };
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess) return give_up("hipGetDeviceProperties failed");
  std::string arch = prop.gcnArchName;  // "gfx950:sramecc+:xnack-"
  const size_t colon = arch.find(':');
  if (colon != std::string::npos) arch.resize(colon);
  std::vector<char> code;
  std::string log;
  auto m = std::make_unique<RtcModule>();
  if (!rtc_compile(source(), arch.c_str(), &code, &log, &m->compile_ms)) return give_up(log);
  hipError_t e = hipModuleLoadData(&m->module, code.data());
  if (e != hipSuccess) return give_up(std::string("hipModuleLoadData: ") + hipGetErrorString(e));
  for (const char* name : entry_points) {
    hipFunction_t f = nullptr;
    e = hipModuleGetFunction(&f, m->module, name);
    if (e != hipSuccess) {
      (void)hipModuleUnload(m->module);
      return give_up(std::string("hipModuleGetFunction(") + name + "): " + hipGetErrorString(e));
    }
    m->fn.push_back(f);
  }
  return (g_loaded[key] = std::move(m)).get();
}

hipError_t launch_module_kernel(hipFunction_t fn, int64_t grid, unsigned lds, hipStream_t stream, const void* args, size_t args_bytes) {
  void* config[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, const_cast<void*>(args), HIP_LAUNCH_PARAM_BUFFER_SIZE, &args_bytes, HIP_LAUNCH_PARAM_END};
  return hipModuleLaunchKernel(fn, (unsigned)grid, 1, 1, kWave, 1, 1, lds, stream, nullptr, config);
}

}  // namespace surge
