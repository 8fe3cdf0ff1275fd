/*
 * surge_ingest.h — C ABI of the events-topic ingest: the step immediately BEFORE
 * the fold.  Kafka record batches of one partition of the events topic in, records in offset order with
 * their aggregate index out (ready for surge_replay_load_csr / surge_replay_append_events): entirely on
 * the host, or — "device decode" below — framed on the host and decoded on the GPU.
 *
 * What it restates (third party, NOT vendored under /root/reference: org.apache.kafka:kafka-clients 3.2.3,
 * message format v2 / KIP-98; LZ4 frame format — "parity unpinned"):
 *   - RecordBatch v2 framing, CRC-32C over [attributes .. end], zig-zag varint records
 *   - compression.type = lz4 (the reference's producer setting,
 *     modules/common/src/main/resources/reference.conf:112), snappy (raw blocks, alone or in snappy-java's framing: what a
 *     producer, broker or mirror configured for it writes) and none; gzip and zstd are refused
 *   - isolation.level = read_committed (modules/common/src/main/scala/surge/kafka/streams/
 *     SurgeStateStoreConsumer.scala:38): transactional batches are held back until their producer's
 *     COMMIT / ABORT control marker; aborted ones are dropped; nothing after an open transaction is
 *     delivered (last-stable-offset order); control batches are never delivered
 *   - the per-flush transaction the reference writes: events..., extra records, state
 *     (modules/command-engine/core/src/main/scala/surge/internal/kafka/KafkaProducerActorImpl.scala:421-453)
 *   - the producer's "flush" record, empty key and empty value (KafkaProducerActorImpl.scala:322-329), is skipped
 *   - aggregate id = record key up to the first ':' (PartitionStringUpToColon,
 *     modules/common/src/main/scala/surge/kafka/KafkaPartitioner.scala:38-42; event keys are "<id>:<seq>",
 *     TestBoundedContext.scala:122-124)
 */
#ifndef SURGE_INGEST_H
#define SURGE_INGEST_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SURGE_INGEST_READ_UNCOMMITTED 0
#define SURGE_INGEST_READ_COMMITTED   1

/* status codes are surge_replay.h's: 0 OK, -1 INVALID, -2 STATE, -3 DEVICE, -4 NOMEM, -5 UNSUPPORTED; plus: */
#define SURGE_E_CORRUPT (-7) /* bad magic / CRC mismatch / malformed varint / bad LZ4 stream */

typedef struct surge_ingest surge_ingest;

typedef struct surge_ingest_record {
  int64_t offset;      /* Kafka offset of the record                                   */
  int64_t agg_idx;     /* dense index of the aggregate id (key up to ':') in the key table */
  int64_t key_off;     /* span of the full key in the byte arena (surge_ingest_arena)   */
  int32_t key_len;     /* -1 = null key                                                */
  int32_t value_len;   /* -1 = null value (tombstone)                                  */
  int64_t value_off;
} surge_ingest_record;

int32_t surge_ingest_create(int32_t isolation_level, surge_ingest** out);
int32_t surge_ingest_destroy(surge_ingest* g);
const char* surge_ingest_last_error(const surge_ingest* g);

/* Feed bytes of consecutive record batches (a fetch response's record set / a log segment).  Whole
 * batches are consumed; *consumed_out tells how many bytes were (a trailing partial batch is left for
 * the next call, exactly like a fetch that cuts a batch).  Decoded records accumulate until drained.
 * On a failure in batch k (CRC, codec, malformed record) the status is returned with *consumed_out = the
 * byte offset of batch k: batches 0..k-1 of the buffer stay decoded and queued, so a caller must not feed
 * them again. */
int32_t surge_ingest_feed(surge_ingest* g, const uint8_t* data, int64_t len, int64_t* consumed_out);
/* Host threads that verify the CRC-32C of the batches of one feed (default 1; 1 .. 64).  A batch's checksum depends on
 * its own bytes only, so a feed of at least 1 MiB first verifies all its whole batches in parallel and then walks them
 * in order as before: same results, same errors at the same batches.  What it is for: uncompressed topics, where the
 * CRC over the fetch (11 GB/s per thread) is the longest stage between the wire and the GPU. */
int32_t surge_ingest_set_threads(surge_ingest* g, int32_t n_threads);

/* Records that are deliverable now (committed / non-transactional, before any open transaction). */
int64_t surge_ingest_ready(const surge_ingest* g);

/* Pops up to max deliverable records in offset order.  Spans point into the arena, valid until the next
 * feed/drain/destroy. */
int32_t surge_ingest_drain(surge_ingest* g, int64_t max, surge_ingest_record* out, int64_t* n_out);
const uint8_t* surge_ingest_arena(const surge_ingest* g);

/* Convenience for GPU-ready topics whose record value IS the 16-byte fixed event (surge_event16): pops
 * records straight into the arrays surge_replay_append_events / a CSR packer take.  A value of any other
 * length is an error (SURGE_E_INVALID). */
int32_t surge_ingest_drain_fixed16(surge_ingest* g, int64_t max, int64_t* agg_idx_out, void* events16_out,
                                   int64_t* offsets_out, int64_t* n_out);

/* ---- record VALUES as the reference's plugins write them: JSON text -> the 16-byte fixed event -----------------------
 * The reference's event writers are `Json.toJson(evt).toString().getBytes()` over play-json case-class formats
 * (TestBoundedContext.scala:42-49,122-124; BankAccountSurgeModel.scala:30-32): one flat JSON object per event, and for a
 * sealed family a discriminator field naming the case class.  A template tells the decoder which discriminator value is
 * which surge_event16.type and which fields carry the sequence number and the payload; field order, extra fields and
 * the spelling of numbers do not matter (play-json is not under /root/reference: its exact text is parity-unpinned, the
 * decoder does not depend on it).  The reference has no event READER at all (SurgeFormatting.scala:9-11 only writes):
 * this is additive, the mirror image of the GPU state encoders of surge_replay.h. */
#define SURGE_EVJ_MAX_TYPES 16
#define SURGE_EVJ_NAME      64
#define SURGE_EVJ_ARG_NONE  0
#define SURGE_EVJ_ARG_I32   1 /* JSON integer that fits a JVM Int -> payload low word (high word zero)              */
#define SURGE_EVJ_ARG_F64   2 /* JSON number -> IEEE double, correctly rounded (BigDecimal.doubleValue semantics) */
typedef struct surge_event_json_type {
  char     name[SURGE_EVJ_NAME];      /* discriminator value selecting this entry, NUL-terminated ("" if none)   */
  uint32_t event_type;                /* surge_event16.type to emit                                              */
  uint32_t arg_kind;                  /* SURGE_EVJ_ARG_*                                                         */
  char     seq_field[SURGE_EVJ_NAME]; /* integer field -> surge_event16.seq ("" = 0)                             */
  char     arg_field[SURGE_EVJ_NAME]; /* field -> payload ("" with SURGE_EVJ_ARG_NONE)                           */
} surge_event_json_type;
/* What lies around the JSON text in a record's value.  A multilanguage (SDK) application writes its events topic as the
 * protobuf message Event { string aggregateId = 1; bytes payload = 2; } (multilanguage-protocol.proto:17-20;
 * GenericSurgeCommandBusinessLogic.scala:30-34 stores Event(aggregateId, payload).toByteArray under the key aggregateId):
 * with SURGE_EVJ_ENVELOPE_PROTOBUF_EVENT a value is read as optionally field 1 (tag 0x0A, length varint, id bytes), then
 * optionally field 2 (tag 0x12, length varint, payload bytes) and nothing else — the grammar of the State envelope
 * (surge_replay.h): length varints of 1 - 5 bytes and at most 2^31 - 1, over-long spellings read, any other tag, order or
 * repetition refused — and the payload goes through the rules above exactly as a bare value (an absent or empty payload
 * is not a JSON object).  Where the record's key is known (surge_ingest_drain_json, surge_event_json_decode_keyed, every
 * push of a surge_device_decoder) field 1 must equal, byte for byte, the aggregate id the record is interned under: the
 * key up to the first ':'; an absent field 1 is the empty id.  Grammar errors are reported before a differing id. */
#define SURGE_EVJ_ENVELOPE_NONE           0 /* the value IS the JSON text (a zeroed field: what this field meant while it was reserved) */
#define SURGE_EVJ_ENVELOPE_PROTOBUF_EVENT 1
typedef struct surge_event_json_template {
  uint32_t n_types;
  uint32_t envelope;                      /* SURGE_EVJ_ENVELOPE_*; any other value is refused by surge_event_json_validate */
  char     discriminator[SURGE_EVJ_NAME]; /* e.g. "_type"; "" = every value is types[0]                            */
  surge_event_json_type types[SURGE_EVJ_MAX_TYPES];
} surge_event_json_template;
int32_t surge_event_json_validate(const surge_event_json_template* t);
/* One record value -> one 16-byte event.  0 or SURGE_E_CORRUPT (malformed JSON, unknown type, missing field, a number
 * that is not what the template says); the reason is in surge_event_json_last_error() (thread-local). */
int32_t surge_event_json_decode(const surge_event_json_template* t, const uint8_t* value, int64_t len, void* event16_out);
/* The same, and with an enveloped template the envelope's aggregateId is compared with key[0 .. key_len): the caller passes
 * the aggregate id, i.e. the record key already cut at its first ':'.  key_len < 0: no comparison — what
 * surge_event_json_decode does.  A template without an envelope ignores the key. */
int32_t surge_event_json_decode_keyed(const surge_event_json_template* t, const uint8_t* key, int64_t key_len, const uint8_t* value, int64_t len,
                                      void* event16_out);
const char* surge_event_json_last_error(void);
/* A JSON number -> the bits of the nearest IEEE double, ties to even (what BigDecimal(text).doubleValue gives play-json):
 * the Eisel-Lemire algorithm (surge_amd/csrc/f64_parse.h — the same code decodes Doubles on the device), with strtod
 * for the values it reports as undecidable.  0: decided by the fast path; 1: decided by strtod; SURGE_E_CORRUPT: not a
 * JSON number. */
int32_t surge_parse_f64_json(const uint8_t* text, int64_t len, uint64_t* bits_out);
/* Like surge_ingest_drain_fixed16 for topics whose values are JSON events: pops up to max deliverable records and
 * decodes each value through the template — no per-record work in the host language.  Nothing is popped when a value
 * does not decode (SURGE_E_CORRUPT; surge_ingest_last_error names the record's offset and the reason).  Enveloped values
 * (tmpl->envelope) are decoded with surge_event_json_decode_keyed against the record's aggregate id. */
int32_t surge_ingest_drain_json(surge_ingest* g, int64_t max, const surge_event_json_template* tmpl, int64_t* agg_idx_out,
                                void* events16_out, int64_t* offsets_out, int64_t* n_out);

/* ---- device decode (N1 on the GPU) ---------------------------------------------------------------------------------------
 * Per-record work — parsing the varint-framed records, interning the aggregate ids, decoding the event values — is what
 * the host decoder above spends its time on (about 90 ns per record and thread for 16-byte values, 640 ns for JSON), in
 * front of a fold that takes 3 ps per event.  In FRAMES mode the host keeps only what is sequential and cheap per byte —
 * walking the 61-byte batch headers, the CRC-32C, read_committed, LZ4 — and hands the records SECTIONS of the
 * deliverable batches over as they are; a surge_device_decoder turns them into device-resident (aggregate index,
 * 16-byte event, offset) arrays and a device key table: what surge_replay_append_events_device / a CSR build take.
 *   g = surge_ingest_create(isolation | SURGE_INGEST_FRAMES, ..)   feed as usual
 *   surge_ingest_drain_sections(g, ..)  ->  surge_device_decoder_push(d, surge_ingest_arena(g), sections, n)
 * Same results as surge_ingest_drain_fixed16 / _json on the same bytes (tests/test_ingest_gpu.py): same records in the
 * same order, aggregate ids numbered in first-delivered order, flush records skipped, the same values rejected. */
#define SURGE_INGEST_FRAMES     0x100 /* OR into surge_ingest_create's isolation_level */
#define SURGE_INGEST_DEVICE_LZ4 0x200 /* FRAMES, and lz4 batches keep their LZ4 frame: the device decoder decodes the blocks on the
                                         GPU (one wave per 64 KiB block, assembled in LDS); frames kafka-clients would not write —
                                         blocks above 64 KiB, dependent blocks — it decompresses on the host.  snappy batches keep
                                         their chunks the same way (section codec 2): one wave parses a chunk, the LZ4 stage's second
                                         pass applies its copies; chunks above 64 KiB or off the 16-byte grid go through the host    */
#define SURGE_INGEST_DEVICE_DECOMPRESS SURGE_INGEST_DEVICE_LZ4 /* the same bit by the name of what it has come to mean                */
#define SURGE_INGEST_DEVICE_CRC 0x400 /* FRAMES, and a data batch's CRC-32C is verified ON THE DEVICE: the host checksums only the 40
                                         header bytes the CRC covers in front of the records section (the state of the CRC register
                                         after them travels with the section), the device decoder continues over the section's bytes
                                         where they already are and fails the push (SURGE_E_CORRUPT, nothing delivered, no key kept)
                                         when the result is not the batch's CRC.  The per-byte host work of framing is then gone:
                                         what remains per batch is the header walk and the transaction bookkeeping.  Control batches
                                         (78 bytes) are still verified on the host.  Sections of such a framer carry
                                         SURGE_SECTION_CRC_PENDING in `codec` and are only good for a surge_device_decoder.
                                         The price of verifying late: the framer has already acted on the batch's header (its
                                         transaction bookkeeping) when the device finds the mismatch — like kafka-clients'
                                         CorruptRecordException the failure ends this consumer's pass over the partition: discard
                                         framer and decoder, start again from the last good offsets.                               */
#define SURGE_SECTION_CRC_PENDING 0x100 /* in surge_batch_section.codec: the 8 bytes in front of byte_off hold {the batch's CRC-32C,
                                           the CRC register after the covered header bytes}, little-endian u32 each                  */
#define SURGE_SECTION_CRC_WIRE    0x200 /* ... (in-place framing) the 44 bytes in front of byte_off are the batch's own crc field (big-endian)
                                           and the 40 header bytes it covers, as received: the device runs the whole CRC             */
#define SURGE_SECTION_FLOORED     0x400 /* ... the section straddles the framer's start offset (below): records of it lie below the start     */
typedef struct surge_batch_section {
  int64_t byte_off;    /* the batch's records section inside the arena (surge_ingest_arena)            */
  int64_t byte_len;
  int64_t base_offset; /* Kafka offset of the batch's first record                                     */
  int32_t n_records;
  int32_t codec;       /* low byte 0: the records themselves; 3: one LZ4 frame that holds them, 2: snappy chunks or one raw
                          snappy block (SURGE_INGEST_DEVICE_LZ4);
                          | SURGE_SECTION_CRC_PENDING                                                             */
} surge_batch_section;
/* Pops up to max deliverable batches (committed / non-transactional, before any open transaction), in offset order.
 * SURGE_E_STATE on a decoder that was not created in FRAMES mode.
 * Lifetime of the spans: a FRAMES decoder rotates through six arenas, one per feed, so the sections handed out here
 * (and the address surge_ingest_arena returned right after this drain) stay valid THROUGH the next five feeds — host
 * threads can frame fetches i + 1 .. i + 5 (feed, drain_sections, surge_ingest_arena) while a device decoder's pushes of
 * fetch i .. i + 4 are still in flight (surge_device_decoder_push_async).  The handle itself is for one thread at a
 * time; what the other threads touch is only the arena memory.  Batches still queued at a feed (open transactions) move to
 * the new arena with it. */
int32_t surge_ingest_drain_sections(surge_ingest* g, int64_t max_sections, surge_batch_section* out, int64_t* n_out);

/* ---- start offsets and positions: resuming inside a partition ------------------------------------------------------------
 * A consumer that seeks to offset o (SurgeStateStoreConsumer.scala:33-46,57-76: the restore consumer of the reference starts
 * from the offsets committed with its store) is sent the whole batch that contains o and drops the records in front of o,
 * record by record, behind the decompression.  surge_ingest_set_start_offset(g, o) — before the first feed, SURGE_E_STATE
 * afterwards; o <= 0: no start — makes the framer do the same: a record is delivered only if its offset is >= o.
 *   - Transactions are read exactly as without a start: batches below it open and close transactions, markers are read, a
 *     transaction that straddles the start commits or aborts as a whole.
 *   - The rule applies where a batch would be handed out.  A batch whose last offset (baseOffset + lastOffsetDelta) lies below
 *     the start is discarded there (surge_ingest_below_start counts it).  surge_ingest_drain, _drain_fixed16 and _drain_json
 *     pass over the records below the start: they count as neither decoded nor delivered, their keys are not interned, their
 *     values are never decoded (a value that would not decode does not fail the drain); a flush record below the start is
 *     dropped as one of them.  surge_ingest_drain_sections hands the ONE batch that straddles the start out with
 *     SURGE_SECTION_FLOORED in `codec` — its records below the start are dropped where records are parsed, on the device
 *     (surge_device_decoder_push_parts_floored_async) — and names it in the floors list.
 *   - Once a batch that reaches the start has been handed out the start is inert: at most one floored section per partition
 *     over the framer's life.
 * The floors list travels beside the sections: take_floors fills it for the sections the last surge_ingest_drain_sections /
 * surge_ingest_group_feed handed out (valid until the next one; SURGE_E_INVALID with the count in *n_out when `max` is too
 * small).  `section` indexes that call's section array; `part` is the partition the floor belongs to (0 from a single handle).
 * surge_ingest_position: the offset a consumer would resume from — behind the last batch the framer has decided (delivered,
 * aborted, control or discarded), in front of an open transaction and of anything still queued for a drain, never below the
 * start: what a publisher commits with a snapshot.  A fresh framer started there delivers exactly what this one has not. */
typedef struct surge_section_floor {
  int32_t part, reserved;
  int64_t section;
  int64_t first_offset;
} surge_section_floor;
int32_t surge_ingest_set_start_offset(surge_ingest* g, int64_t first_offset);
int32_t surge_ingest_take_floors(surge_ingest* g, int64_t max, surge_section_floor* out, int64_t* n_out);
int64_t surge_ingest_position(const surge_ingest* g);
/* [0] batches discarded below the start, [1] records dropped below it (host drains: one by one; FRAMES: the discarded batches'
 * recordCount — what the device drops of the floored section is in surge_device_decoder_below_floor).  In FRAMES mode the
 * framer cannot see into the floored section: its whole recordCount stays in surge_ingest_counters' "records decoded" and
 * "records delivered" (handed to the device); subtract surge_device_decoder_below_floor for the records that were decoded and
 * delivered in the issue's sense (surge_amd/store.py does for its tail_* counts). */
int32_t surge_ingest_below_start(const surge_ingest* g, int64_t out[2]);

/* A consumer that is assigned several partitions gets, per fetch response, the next bytes of each of them; transactions,
 * last stable offsets and cut batches are per partition, so each partition needs a framer of its own.  A group owns n
 * FRAMES handles and, instead of an arena per handle, six rotating SLABS; a feed lays partition 0's records sections,
 * then partition 1's ... out in the next slab (every partition's slice is sized for the feed up front; batches a
 * partition still holds — open transactions — move along), so what comes back is one array of sections, partition after
 * partition, whose spans index one buffer: one part of surge_device_decoder_push_parts_async, one host-to-device copy.
 * A slab stays as it is through the next five feeds.  data[p] / len[p]: partition p's bytes of this fetch response (len
 * 0: nothing, the partition is only carried along); consumed_out (nullable, n entries); sections_out holds up to
 * max_sections entries: the total of len[] / 61 + surge_ingest_group_queued_sections() is always enough (a feed also
 * delivers what earlier feeds left queued — a transaction whose COMMIT marker arrives in this one).  `threads` host
 * threads frame the partitions side by side: the calling thread + a pool the group keeps for its lifetime.
 * SURGE_INGEST_DEVICE_LZ4 / isolation level as in surge_ingest_create (FRAMES is implied; without DEVICE_LZ4 the host
 * decompresses lz4 batches into the slab, sized by trial).
 * A feed is ALL OR NOTHING: when a partition fails (its status is returned, its message in
 * surge_ingest_group_last_error) or sections_out is too small (SURGE_E_INVALID with the count the feed delivers in
 * *n_sections_out), every partition's framer is put back exactly as it was before the call — nothing consumed, nothing
 * drained, consumed_out all 0 — so the caller can feed again (a larger table; without the failing partition's bytes). */
typedef struct surge_ingest_group surge_ingest_group;
int32_t surge_ingest_group_create(int32_t n_partitions, int32_t isolation_level, surge_ingest_group** out);
int32_t surge_ingest_group_destroy(surge_ingest_group* g);
const char* surge_ingest_group_last_error(const surge_ingest_group* g);
int32_t surge_ingest_group_feed(surge_ingest_group* g, const uint8_t* const* data, const int64_t* len, int32_t threads, int64_t* consumed_out,
                                int64_t max_sections, surge_batch_section* sections_out, int64_t* n_sections_out, const uint8_t** slab_out);
/* Framing IN PLACE: where the consumer can choose where a fetch response lands (a socket read, a JNI direct buffer), it
 * receives straight into the group's next page-locked slab: receive_buffer returns room for `bytes` bytes there (behind the few
 * sections the partitions carry over — open transactions); the feed that follows, with every data[p] inside that room,
 * copies NOTHING: the sections it hands out are the received bytes themselves.  With SURGE_INGEST_DEVICE_LZ4 |
 * SURGE_INGEST_DEVICE_CRC the host then reads a batch's 61-byte header and not one byte more (sections carry
 * SURGE_SECTION_CRC_WIRE: the device runs the whole CRC-32C over the header bytes and the section as received).  A feed whose
 * data lies elsewhere frames by copy as before.  lz4 batches need SURGE_INGEST_DEVICE_LZ4 in place. */
int32_t surge_ingest_group_receive_buffer(surge_ingest_group* g, int64_t bytes, uint8_t** buf_out);
/* ... and for a host whose fetch responses already lie somewhere else: receive_buffer for the sum of len[], then the one copy the
 * socket read would have made — partition after partition, on `threads` threads — placed_out[p] = where partition p's bytes
 * now are (NULL for len[p] == 0): what the in-place feed takes as data[p]. */
int32_t surge_ingest_group_receive_copy(surge_ingest_group* g, const uint8_t* const* data, const int64_t* len, int32_t threads, const uint8_t** placed_out);
/* What the group's host threads have cost so far, as thread CPU time (not wall): out[0] seconds inside receive_copy's copies,
 * out[1] seconds framing (surge_ingest_group_feed's per-partition work: headers, transactions — and the sections' copy and
 * CRC-32C where those still run on the host). */
int32_t surge_ingest_group_cpu_seconds(const surge_ingest_group* g, double out[2]);
/* The group's six slabs: bytes allocated so far, and whether they come from an allocator the host set
 * (surge_ingest_group_use_pinned_slabs: page-locked memory — the footprint a host has to budget per consumer). */
int32_t surge_ingest_group_slab_bytes(const surge_ingest_group* g, int64_t* bytes_out, int32_t* custom_allocator_out);
int64_t surge_ingest_group_queued_sections(const surge_ingest_group* g); /* batches the partitions hold from earlier feeds (upper bound of what the next feed delivers beyond its own) */
int32_t surge_ingest_group_counters(const surge_ingest_group* g, int64_t out[8]); /* surge_ingest_counters, summed */
/* The calls of "start offsets and positions" above for a group: one entry per partition (a value <= 0: that partition has no start) */
int32_t surge_ingest_group_set_start_offsets(surge_ingest_group* g, const int64_t* first_offset);
int32_t surge_ingest_group_take_floors(surge_ingest_group* g, int64_t max, surge_section_floor* out, int64_t* n_out);
int32_t surge_ingest_group_positions(const surge_ingest_group* g, int64_t* out);
int32_t surge_ingest_group_below_start(const surge_ingest_group* g, int64_t out[2]); /* surge_ingest_below_start, summed */
int32_t surge_ingest_group_set_allocator(surge_ingest_group* g, void* (*alloc)(size_t), void (*release)(void*));
int32_t surge_ingest_group_use_pinned_slabs(surge_ingest_group* g); /* page-locked slabs (SURGE_E_DEVICE without a HIP runtime) */

/* Where the arena's memory comes from (before the first feed; NULL / NULL = malloc / free).  surge_ingest_use_pinned_arena
 * makes it page-locked host memory of the HIP runtime: a device decoder then copies the sections to the GPU straight out
 * of the arena (no staging copy).  SURGE_E_DEVICE without a usable HIP runtime. */
int32_t surge_ingest_set_allocator(surge_ingest* g, void* (*alloc)(size_t), void (*release)(void*));
int32_t surge_ingest_use_pinned_arena(surge_ingest* g);

typedef struct surge_device_decoder surge_device_decoder;
/* (Calls on the same decoder must not overlap, with one exception made for throughput: ONE thread may enqueue pushes
 * (push_async / push_parts_async / push_records_async) while ONE other thread finishes them and consumes the results (push_finish*, result,
 * clear, surge_replay_append_decoded*): the host work of framing tables and launches of fetch i + depth then runs beside
 * the interning and the fold of fetch i.) */
/* tmpl == NULL: record values are 16-byte surge_event16; otherwise the reference's JSON event text, decoded by the
 * template with surge_event_json_decode's rules (Doubles correctly rounded on the device — f64_parse.h — the rare value
 * its fast path cannot decide is re-parsed on the host).  tmpl->envelope travels with the template: every push of such a
 * decoder — push, push_async / push_parts_async, push_records — reads the protobuf Event envelope in front of the JSON text
 * and compares its aggregateId with the record's aggregate id; a value that is no such envelope, or names another id, fails
 * the push like every bad record.  hip_stream: the stream the decoder works on (NULL = default). */
int32_t surge_device_decoder_create(int32_t device_id, void* hip_stream, const surge_event_json_template* tmpl, surge_device_decoder** out);
/* STATE MODE: a decoder for the compacted STATE topic (what SurgeStateStoreConsumer.scala:57-76 reads, records written by
 * SurgeModel.scala:57-65).  Every other entry point works on it unchanged — push, push_async / push_parts_async,
 * push_finish[_async], push_records, reserve, keys, key_table, counters, stats, clear — with these differences per record:
 *   - the aggregate id is the WHOLE key (the state topic's key is the id itself; "a:b" and "a" are two ids);
 *   - a null value is a TOMBSTONE and is delivered (value length 0); a null key fails the push; so does an empty, non-null
 *     value under a non-empty key (writeState never writes one, and the loader could not tell it from a tombstone) —
 *     SURGE_E_CORRUPT naming the record's offset, nothing of the push delivered, like every bad record;
 *   - empty key AND empty value is still the producer's flush record (KafkaProducerActorImpl.scala:322-329 writes it on the
 *     state topic): skipped and counted; record headers (stateHeaders) are skipped;
 *   - no value is decoded: the delivered records' value bytes are gathered, in delivery order, into one device buffer behind
 *     what earlier pushes delivered (a push's staged bytes are reused by the next push, so the values move);
 *   - push_records: an EMPTY value is the tombstone (ConsumerRecord.value() == null: a JVM caller maps null to empty).
 * The result is read with surge_device_decoder_state_result and handed over with surge_device_decoder_load_states;
 * surge_device_decoder_result, surge_replay_append_decoded[_async] and surge_replay_stage_decoded return SURGE_E_STATE. */
int32_t surge_device_decoder_create_states(int32_t device_id, void* hip_stream, surge_device_decoder** out);
/* A state decoder goes on as the EVENTS decoder of the same aggregates: fold(prev snapshot, new events) on one key table.  The
 * restore consumer of the reference reads the state topic and then serves (SurgeStateStoreConsumer.scala:33-46,57-76); a store that
 * resumes from a snapshot reads the events behind it as well, and the dense ids the state decoder interned are the resident
 * state's row numbers — the events' ids have to be the same numbers.  Both modes hash an id's bytes alike, so the table is good
 * for both.  Allowed on a state decoder with no push pending and every delivered record loaded or cleared (SURGE_E_STATE
 * otherwise, and on an events decoder: the switch is one-way); a template that fails surge_event_json_validate: SURGE_E_INVALID,
 * nothing changed.  The key table — slots, arena, offsets, hashes, seed, key count, reserve — stays where it is, nothing is
 * copied; the value buffers of state mode are released; the template is set up as surge_device_decoder_create does (NULL:
 * 16-byte fixed events; tmpl->envelope honoured).  From then on the decoder is an events decoder in every respect: ids are the
 * key up to the first ':', new ids are numbered from the key count on, state-only calls return SURGE_E_STATE,
 * surge_replay_append_decoded[_async] and surge_replay_stage_decoded work.  The one exception: string columns kept with
 * surge_device_decoder_keep_strings stay readable through surge_device_decoder_state_strings until clear or destroy.
 *   - A state id that contains a colon ("a:b") stays in the table, and keeps its row, but can never be named by an event: the
 *     event key "a:b:7" is the id "a".
 *   - A re-seed of the hash function after the switch re-hashes the state-era keys from the arena like any others. */
int32_t surge_device_decoder_continue_as_events(surge_device_decoder* d, const surge_event_json_template* tmpl);
int32_t surge_device_decoder_destroy(surge_device_decoder* d);
const char* surge_device_decoder_last_error(const surge_device_decoder* d);
/* Decodes the sections (spans of `bytes`, a HOST buffer) and APPENDS their records to the device-resident result.  A
 * record that does not decode fails the whole push (SURGE_E_CORRUPT, the message names the record's offset): nothing of
 * the push is appended.  Synchronous. */
int32_t surge_device_decoder_push(surge_device_decoder* d, const uint8_t* bytes, const surge_batch_section* sections, int64_t n_sections);
/* The two halves of a push, for a consumer that keeps the GPU busy across fetches.  push_async enqueues everything of a
 * push that does not touch the key table — the copy to the device, the LZ4 blocks, chaining / parsing the records and
 * decoding their values — on a stream of its own and returns; push_finish interns the keys of the OLDEST unfinished
 * push, appends its records to the result and returns what surge_device_decoder_push would have returned.  Up to five
 * pushes may be unfinished at a time (SURGE_E_STATE beyond that, and from push / push_records while any is), so the
 * copy engine, the latency-bound LZ4 kernels and the compute-bound decode of consecutive fetches overlap on the chip:
 *     push_async(fetch 0) ... push_async(fetch 3);
 *     loop i: push_finish() -> surge_replay_append_decoded_async (fold of fetch i, no host wait); push_async(fetch i + 4)
 * (what surge_amd/store.py and bench.py --workload e2e do; 8.9 - 9.2e8 events/s on a 10^7-aggregate topic).
 * Stage 1 rotates over three LOW-priority streams: the runtime maps streams onto four hardware queues per priority, a queue
 * runs in order, and a stage-1 stream that shares the queue of the decoder's own stream puts a push's interning behind a
 * later push's whole stage 1 — low-priority streams come out of another pool of queues than the decoder's stream and the
 * fold's (SURGE_INGEST_PUSH_PRIORITY, SURGE_INGEST_PUSH_STREAMS: INTEGRATION.md).
 * `bytes` and `sections` must stay valid until the matching push_finish.  push_parts_async takes the sections of
 * several arenas — e.g. one per partition of a fetch response, framed on as many host threads — as ONE push: part p's
 * sections index bytes[p]; records are delivered part after part.  A push_async that fails occupies no slot. */
int32_t surge_device_decoder_push_async(surge_device_decoder* d, const uint8_t* bytes, const surge_batch_section* sections, int64_t n_sections);
int32_t surge_device_decoder_push_parts_async(surge_device_decoder* d, int32_t n_parts, const uint8_t* const* bytes,
                                              const surge_batch_section* const* sections, const int64_t* n_sections);
/* The same with the floors of the push's sections (surge_ingest_take_floors / surge_ingest_group_take_floors; "start offsets and
 * positions" above): floors[i].section counts through the push's sections in push order — part p's follow part p - 1's; with one
 * part, what every framer here fills, it is the index take_floors wrote — and `part` is not read.  A record of such a section
 * whose offset (base_offset + its offset delta) lies below first_offset is passed over where records are parsed, right behind its
 * offset delta: its key is not hashed or interned, its value is never looked at — a value that would not decode is not refused, a
 * Double the device cannot decide is not handed back to the host — and it is not delivered; it counts in
 * surge_device_decoder_below_floor, not as a flush record.  A record that is malformed fails the push on either side of the floor,
 * as it fails the host framer's feed.  The host drains are the pin (tests/test_resume_tail_gpu.py).  Events decoders only
 * (SURGE_E_STATE on a state decoder: the state topic is read from its beginning); push_records takes no floors — a consumer
 * that has sought never hands over a record below its position.  n_floors == 0: exactly push_parts_async, the same kernels;
 * a push that carries a floor launches instantiations of the record stage of its own (section_kernel's kFloor), so every other
 * push runs the code it ran before.  push_floored: the synchronous form, as surge_device_decoder_push is push_async's. */
int32_t surge_device_decoder_push_parts_floored_async(surge_device_decoder* d, int32_t n_parts, const uint8_t* const* bytes,
                                                      const surge_batch_section* const* sections, const int64_t* n_sections, int64_t n_floors,
                                                      const surge_section_floor* floors);
int32_t surge_device_decoder_push_floored(surge_device_decoder* d, const uint8_t* bytes, const surge_batch_section* sections, int64_t n_sections, int64_t n_floors,
                                          const surge_section_floor* floors);
int32_t surge_device_decoder_below_floor(const surge_device_decoder* d, int64_t* n_out); /* records passed over below a floor so far */
/* Stage 1 of a push of records that are ALREADY FRAMED (surge_device_decoder_push_records below: a KafkaConsumer's poll — key
 * bytes, value bytes and an offset per record), enqueued on the next free slot: the copy to the device and the record stage —
 * the key cut at its ':' and hashed, the value decoded — run on a stream of their own, and the call returns.  Arguments and
 * refusals are push_records' (spans that run backwards and n >= 2^32 - 1 are refused before any launch; a NULL decoder).  It
 * takes one of the five slots: wire pushes and records pushes may be in flight in any mix (a sixth: SURGE_E_STATE), and
 * push_finish / push_finish_async finish the OLDEST push whatever its kind, with what the synchronous call would have returned;
 * results are appended in push order.  UNLIKE push_async, which reads `bytes` and `sections` until the matching push_finish,
 * this call copies keys, key_off, values, value_off and offsets into the slot's page-locked staging before it returns: the
 * caller's arrays may be reused or freed as soon as it has returned (a JVM caller releases its pinned arrays right behind the
 * call).  n == 0 returns SURGE_OK and occupies no slot — there is nothing to finish —, and so does a call that fails.  Works on
 * every kind of decoder as push_records does: events (bare, enveloped and 16-byte values, kept event strings), states (the id
 * is the whole key, an empty value is the tombstone, the values are gathered at the finish) and a state decoder that continued
 * as an events decoder.  No floors, as push_records:
 *     loop over the polls: push_records_async(poll i + 4); push_finish_async() -> surge_replay_append_decoded_async (poll i) */
int32_t surge_device_decoder_push_records_async(surge_device_decoder* d, const uint8_t* keys, const int64_t* key_off, const uint8_t* values,
                                                const int64_t* value_off, const int64_t* offsets, int64_t n);
int32_t surge_device_decoder_push_finish(surge_device_decoder* d);
/* push_finish without its closing wait for the device: the results are complete in the order of the decoder's stream
 * (hand them over with surge_replay_append_decoded_async, or synchronise that stream before reading them).  The one
 * wait that remains is the one in the middle of the call — errors, new keys, the record count: what the host decides on. */
int32_t surge_device_decoder_push_finish_async(surge_device_decoder* d);
int32_t surge_device_decoder_pending(const surge_device_decoder* d); /* pushes enqueued and not finished */
/* Optional capacity hint — e.g. the aggregate count of the store's last snapshot: room for n_keys aggregate ids of
 * key_bytes bytes in all (hash table, key arena, offsets), so a recovery does not grow them step by step (every step
 * allocates, copies and frees device memory: tens of milliseconds at 10^7 keys).  Growing beyond it still works. */
int32_t surge_device_decoder_reserve(surge_device_decoder* d, int64_t n_keys, int64_t key_bytes);
/* The same for records that arrive already framed — what a JVM's KafkaConsumer hands over (ConsumerRecord key / value
 * bytes and offset): record i's key is keys[key_off[i] .. key_off[i+1]), its value values[value_off[i] .. value_off[i+1]),
 * offsets nullable (then 0, 1, 2 ..).  A record with an empty key AND an empty value is the producer's flush record and
 * is skipped, as in the wire path.  Synchronous: push_records_async, then push_finish, when nothing is pending (SURGE_E_STATE
 * while a push is). */
int32_t surge_device_decoder_push_records(surge_device_decoder* d, const uint8_t* keys, const int64_t* key_off, const uint8_t* values,
                                          const int64_t* value_off, const int64_t* offsets, int64_t n);
/* Everything appended since the last clear: device arrays of n_records entries (valid until the next push / clear). */
int32_t surge_device_decoder_result(surge_device_decoder* d, int64_t* n_records, const int64_t** d_agg_idx, const void** d_events16,
                                    const int64_t** d_offsets, int64_t* n_keys);
/* The same of a state decoder (SURGE_E_STATE on any other): record r names aggregate d_agg_idx[r], its value is
 * d_values[d_value_off[r] .. d_value_off[r+1]) (empty: a tombstone), its Kafka offset d_offsets[r] (log compaction leaves
 * gaps); d_value_off has n_records + 1 entries, d_value_off[0] = 0.  The values buffer ends at least 64 bytes behind its last
 * value.  Valid until the next push_finish / clear / load_states. */
int32_t surge_device_decoder_state_result(surge_device_decoder* d, int64_t* n_records, const int64_t** d_agg_idx, const uint8_t** d_values,
                                          const int64_t** d_value_off, const int64_t** d_offsets, int64_t* n_keys);
int32_t surge_device_decoder_clear(surge_device_decoder* d); /* drops the records, keeps the key table */
/* Folds everything decoded since the last clear onto the replay handle's resident state and clears it: grows the
 * state for aggregate ids seen for the first time (surge_replay_grow), device group-by + fold
 * (surge_replay_append_events_device), synchronises.  The handle must hold a bound / restored state (an empty one will
 * do: load a CSR of zero aggregates and fold).  *n_events_out / *n_keys_out (nullable): what was folded / the key count. */
struct surge_replay_handle;
int32_t surge_replay_append_decoded(struct surge_replay_handle* h, surge_device_decoder* d, int64_t* n_events_out, int64_t* n_keys_out);
/* The same without a host wait: the handle's stream waits (event) for the decoder's, group-by + fold are enqueued, the
 * decoder is cleared; the next push_finish* waits (event, on the device) for the group-by's last read of the result
 * arrays before it writes them again.  With the handle on a stream of its own (surge_replay_set_stream, non-blocking),
 * interning of fetch i + 1 overlaps the fold of fetch i — and the decoder then rotates its stage 1 over two streams instead
 * of three (the handle's stream is one more for the four hardware queues); on the decoder's stream (the default of both) the
 * host thread simply does not wait for the fold, which measured the same or better.  Errors of the fold surface at the next
 * surge_replay_synchronize. */
int32_t surge_replay_append_decoded_async(struct surge_replay_handle* h, surge_device_decoder* d, int64_t* n_events_out, int64_t* n_keys_out);
/* For a recovery that ends with ONE fold of the whole topic (surge_replay_pack_staged in surge_replay.h): instead of
 * folding, everything decoded since the last clear is appended to the handle's staging log (surge_replay_stage_events_device)
 * and the decoder is cleared.  No host wait: the hand-over is ordered by events exactly like append_decoded_async's.
 * When the topic ends: surge_replay_pack_staged(h, <the decoder's key count>) and one surge_replay_fold. */
int32_t surge_replay_stage_decoded(struct surge_replay_handle* h, surge_device_decoder* d, int64_t* n_events_out, int64_t* n_keys_out);
/* A state decoder's hand-over (SURGE_E_STATE on an events decoder): everything delivered since the last clear goes into the
 * handle's resident state, as a KTable restore applies the records it is handed (SurgeStateStoreConsumer.scala:69).  The
 * state grows for ids seen for the first time (as in surge_replay_append_decoded: the handle must hold a bound / restored
 * state), the handle's stream waits (event) for the decoder's, and surge_replay_decode_json_states (surge_replay.h) runs over
 * the decoder's own arrays WITH its key table — a value's KEY string must be the interned id — writing
 * surge_replay_device_state: per aggregate the last record wins, a tombstone makes the row 64 zero bytes.  tmpl: the model's
 * serialized state (struct surge_json_template).  counts_out: that decode's four counts for this call {rows written,
 * tombstones, winners refused, Doubles re-parsed on the host}.
 * The call returns when the rows are written, so the next push_finish may write the result arrays again (stage 1 of later
 * pushes overlaps on its own streams all the while).  The decoder's records are cleared whether or not a winner was refused:
 * then SURGE_E_CORRUPT is returned after everything else was loaded, and the message gives the TOPIC offset of the first
 * refused record.  Keep-last ACROSS calls follows from calling in delivery order: a later call overwrites or zeroes what an
 * earlier one wrote.  What the bytes the template does not name hold stays the caller's business
 * (surge_replay_set_decode_base).  ABI v2 handles: SURGE_E_UNSUPPORTED (the decode's; nothing is cleared). */
struct surge_json_template;
int32_t surge_device_decoder_load_states(surge_device_decoder* d, struct surge_replay_handle* h, const struct surge_json_template* tmpl, int64_t counts_out[4]);
/* surge_device_decoder_load_states for a state topic a multilanguage (SDK) application wrote: every value is the protobuf
 * State message around the text payload_tmpl describes (surge_replay_decode_protobuf_states in surge_replay.h; the reference
 * reads them with protobuf.State.parseFrom, GenericSurgeCommandBusinessLogic.scala:25-27).  The same hand-over, the same
 * naming of the first refused record by its topic offset, the same merge of kept strings. */
int32_t surge_device_decoder_load_protobuf_states(surge_device_decoder* d, struct surge_replay_handle* h, const struct surge_json_template* payload_tmpl,
                                                  int64_t counts_out[4]);
/* The STR fields of the loaded states, kept on the device (off by default: load_states then behaves exactly as described
 * above).  surge_device_decoder_keep_strings(d, 1) — state decoders only (SURGE_E_STATE otherwise), before the first
 * load_states — makes every load_states also reserve a span buffer for the decode and, for every column a SURGE_JP_STR part
 * of tmpl names, run surge_replay_merge_state_strings (surge_replay.h) over the load's records with the decoder's own
 * previous column, n_agg = the decoder's key count: the column of a decoder that has loaded the whole topic holds, per
 * aggregate, the string of the record that won — empty for a tombstoned id, the earlier string where a later winner was
 * refused (a load that returns SURGE_E_CORRUPT has merged everything else).  The decoder owns the buffers (two per column,
 * used in turn; they grow with room to spare), the merges run on the handle's stream behind the decode.
 * surge_device_decoder_state_strings: column's CSR column (n_agg + 1 offsets) — the form surge_replay_set_encode_strings
 * takes — valid until the next load_states, clear or destroy; *d_off == NULL (and *n_agg == 0) for a column no load has
 * named. */
int32_t surge_device_decoder_keep_strings(surge_device_decoder* d, int32_t on);
int32_t surge_device_decoder_state_strings(surge_device_decoder* d, int32_t column, const uint8_t** d_utf8, const int64_t** d_off, int64_t* n_agg);

/* ---- the STRING fields of events -------------------------------------------------------------------------------------------
 * A 16-byte event carries a type, a sequence number and one numeric argument; an event class may also carry strings the state
 * keeps (BankAccountCreated: accountOwner, securityCode — BankAccountSurgeModel.scala:14-17).  surge_event_strings names them:
 * up to SURGE_EVS_MAX entries {type name, field name, column}.  type_name is the discriminator value of the class, as in
 * surge_event_json_type.name ("" for a template without a discriminator); column is the side string column
 * (0 .. SURGE_JSON_STRING_COLUMNS - 1 of surge_replay.h) the string lands in.  surge_event_json_template is untouched.
 * THE RULE (one text for host and device, surge_amd/csrc/event_strings_parse.h):
 *   - the record's class is the one surge_event_json_decode chooses;
 *   - for every column that class names, the string is the FIRST string-valued field of that name among the first 24 top-level
 *     fields with unescaped names (the rule surge_event_json_decode applies to its numeric fields): a numeric field of the same
 *     name in front does not count, a field with an escaped name does not count, the field at position 25 does not count;
 *   - its contents (the bytes between the quotes) must pass surge_unescape_json_string's rules (surge_replay.h); the bytes kept
 *     are that routine's output;
 *   - a class that names a column, in a record without such a field or with a string that is refused, REFUSES THE RECORD.
 * Which event wins: per aggregate and column the last event in topic order whose class names the column; an aggregate without
 * such an event keeps what it had, an aggregate new to the table has empty strings. */
#define SURGE_EVS_MAX 16
#define SURGE_EVENT_STRING_OK      0   /* == SURGE_STATE_DECODE_OK: the span is the column's string                             */
#define SURGE_EVENT_STRING_MISSING 12  /* refusal: the class names the column and the record has no string-valued field of that name */
#define SURGE_EVENT_STRING_RECORD  13  /* refusal: the value is not an event the template decodes (not the object, unknown class, bad envelope) */
#define SURGE_EVENT_STRING_ABSENT  254 /* not a refusal: the record's class does not name this column                          */
/* (the other refusals are surge_unescape_json_string's: SURGE_STATE_DECODE_STRING, _ESCAPE, _SURROGATE) */
typedef struct surge_event_string_field {
  char     type_name[SURGE_EVJ_NAME]; /* NUL-terminated */
  char     field[SURGE_EVJ_NAME];     /* NUL-terminated, not empty */
  uint32_t column;
  uint32_t reserved;
} surge_event_string_field;
typedef struct surge_event_strings {
  uint32_t n;
  uint32_t reserved;
  surge_event_string_field entry[SURGE_EVS_MAX];
} surge_event_strings;
/* 0, or -1 with the reason in surge_event_json_last_error(): a template that fails surge_event_json_validate, n outside
 * [1, SURGE_EVS_MAX], a name that is not NUL-terminated, a type name the template does not have, a column out of range, the
 * same (type, column) named twice, an empty field name. */
int32_t surge_event_strings_validate(const surge_event_json_template* tmpl, const surge_event_strings* strings);
/* The rule for ONE record value on the host (thread-safe, no device).  spans_out: 2 x SURGE_JSON_STRING_COLUMNS int64 {offset
 * into value, length} of the still-escaped bytes between the quotes — with an enveloped template offsets into the VALUE, of the
 * payload's text; status_out: one byte per column, SURGE_EVENT_STRING_OK, _ABSENT or the refusal.  Returns 0 when no column is
 * refused, SURGE_E_CORRUPT when one is (a value that is no event of the template refuses every column with _RECORD), -1 for a
 * bad argument or strings that do not validate. */
int32_t surge_event_json_string_spans(const surge_event_json_template* tmpl, const surge_event_strings* strings, const uint8_t* value, int64_t len,
                                      int64_t* spans_out, uint8_t* status_out);
/* Arms an events decoder (created with a template; SURGE_E_STATE on a state decoder and on a 16-byte-event decoder) BEFORE ITS
 * FIRST PUSH — a decoder that went through surge_device_decoder_continue_as_events: before its first EVENTS push — anywhere
 * else SURGE_E_STATE; strings that do not validate against the decoder's template: SURGE_E_INVALID.  From then on every push,
 * behind its interning, selects the delivered records whose class names a column, validates their strings by the rule (a
 * refusal fails the push with SURGE_E_CORRUPT naming the record's offset, nothing delivered, no key kept, the columns as they
 * were) and keeps those records' values on the device; the columns are merged (surge_replay_merge_state_strings' kernels, the
 * last naming event wins) when surge_device_decoder_state_strings asks for them or when more than SURGE_INGEST_EVENT_STRINGS_PENDING
 * (environment, default 1048576) records are pending.  A continued decoder that kept the state topic's strings
 * (surge_device_decoder_keep_strings) goes on merging into the SAME columns.  surge_device_decoder_clear drops what is pending
 * and not yet merged.  A decoder that was never armed launches exactly what it launched before.
 * On an armed decoder what surge_device_decoder_state_strings answered is valid only until the next push_finish[_async], clear
 * or destroy: a push that crosses the pending bound merges at its end — with its host waits, also when the push was finished
 * without its closing wait — and a merge writes the column's other buffer, which may have moved. */
int32_t surge_device_decoder_keep_event_strings(surge_device_decoder* d, const surge_event_strings* strings);
/* What an armed decoder holds until the next merge (SURGE_E_STATE on any other): out[0] records pending, out[1] their value
 * bytes, out[2] the capacity of the values buffer, out[3] merges that have run; d_values / d_value_off (out[0] + 1 offsets) /
 * d_rows (nullable): where the pending values, their CSR offsets and their aggregate rows lie on the device — complete in the order
 * of the decoder's stream, valid until the next push_finish, merge or clear.  For tests and for sizing the bound. */
int32_t surge_device_decoder_event_strings_pending(surge_device_decoder* d, int64_t out[4], const uint8_t** d_values, const int64_t** d_value_off, const int64_t** d_rows);
/* Where the NEXT merge of an armed decoder writes column `column` (SURGE_E_STATE on any other decoder): the call makes the
 * reservation that merge would make for what is pending now — the column's other buffer, room for the column's bytes so far plus
 * the pending values' and for key count + 1 offsets — and reports out[0] the capacity of the bytes buffer, out[1] of the offsets
 * buffer (bytes), out[2] the key count; *d_utf8 / *d_off: the buffers.  A merge that follows with nothing pushed in between
 * writes exactly these buffers — surge_device_decoder_state_strings then answers the same addresses — and nothing in them
 * behind the column's total bytes and behind its key count + 1 offsets.  A column the next merge would not write (not named, or
 * already up to date with nothing pending): out[0] = out[1] = 0, NULL.  For tests. */
int32_t surge_device_decoder_event_strings_next_column(surge_device_decoder* d, int32_t column, int64_t out[3], uint8_t** d_utf8, int64_t** d_off);
/* The key table (aggregate ids in first-delivered order): to the host (NULL / NULL = size query), or where it lives on
 * the device (n_keys + 1 offsets; what the GPU state encoders and the UTF-8 shard map,
 * surge_replay_partition_hash_utf8_device, take — K4 itself hashes UTF-16 code units and does not). */
int32_t surge_device_decoder_keys(surge_device_decoder* d, uint8_t* utf8_out, int64_t utf8_capacity, int64_t* key_off_out, int64_t* n_keys_out,
                                  int64_t* utf8_bytes_out);
int32_t surge_device_decoder_key_table(surge_device_decoder* d, const uint8_t** d_utf8, const int64_t** d_key_off);
/* The key table, read: which row is this id.  Query i is the id ids_utf8[id_off[i] .. id_off[i+1]) (n + 1 offsets that do not
 * decrease); idx_out[i] receives its dense index — the id's position in first-delivered order, the row of the resident state a
 * hand-over of this decoder wrote — or -1 when the table does not hold it.  One thread per query hashes the id under the hash
 * function in use (the new one after a re-seed), probes linearly from its home slot, wrapping at the table's end, and compares
 * length and bytes with the key arena: only byte equality is a hit, an equal 64-bit hash over other bytes goes on probing, an
 * empty slot is a miss.  The table is only read (no atomics), so nothing a later push sees changes.
 *   - The id is compared as it stands, in every mode: there is no cut at ':'.  A state decoder's id "a:b" is found as "a:b", also
 *     after surge_device_decoder_continue_as_events; an events decoder holds the key up to its first ':', so that is what is asked
 *     for.  An id whose last record was a tombstone resolves (its row is None: that is not a miss).  The empty id is an id.
 *   - Events decoders, state decoders and continued ones alike.  SURGE_E_STATE while a push is unfinished (its keys have no ids
 *     yet) and on a decoder a device error poisoned.  n == 0: SURGE_OK, nothing read.  A decoder that has interned nothing
 *     answers -1 to everything.  SURGE_E_INVALID for a NULL argument with n > 0, a negative n, offsets that decrease (host form).
 *   - surge_device_decoder_lookup takes HOST buffers: ids and offsets are staged to the device (with the slack below), the device
 *     form runs on the decoder's stream, the indices are copied back; it returns when they are there.
 *   - surge_device_decoder_lookup_device takes DEVICE buffers and only enqueues on the decoder's stream: d_idx_out is complete in
 *     that stream's order (surge_replay_set_stream the consumer onto it, or synchronize it).  d_ids_utf8 must be readable 16 bytes
 *     behind the end of its last id, as the key arena is: ids are compared four bytes a load.  Offsets that do not describe a
 *     length in [0, 2^31) make their query a miss.
 * One caller at a time per decoder (the host form stages into buffers the decoder owns). */
int32_t surge_device_decoder_lookup(surge_device_decoder* d, const uint8_t* ids_utf8, const int64_t* id_off, int64_t n, int64_t* idx_out);
int32_t surge_device_decoder_lookup_device(surge_device_decoder* d, const uint8_t* d_ids_utf8, const int64_t* d_id_off, int64_t n, int64_t* d_idx_out);
/* The key table, read IN KEY ORDER.  The decoder keeps a permutation of the dense indices sorted by the ids' bytes as unsigned
 * bytes, a proper prefix in front of the longer id ("a" < "a\0" < "a\x01"): the order of Kafka's Bytes comparator — a
 * KeyValueStore's range / all — and, for valid UTF-8, of the code points.  It is built on the device on first use and whenever
 * the table has grown since (a push that interns a new id leaves it stale; clear and a re-seed of the hash function do not):
 * passes over four bytes of every id, most significant first, until every id stands alone — *passes_out of the last build.  It
 * costs 8 bytes per id; more than 2^29 ids are SURGE_E_UNSUPPORTED.
 *   - surge_device_decoder_range_device: the rows whose id k satisfies from <= k <= to, both ends inclusive, ascending, to the
 *     DEVICE array d_rows_out; the bounds are HOST bytes.  from == NULL: unbounded below; to == NULL: unbounded above (NULL, NULL =
 *     every id); a zero-length bound with a non-NULL pointer is the empty id.  *n_out is always the number of matches; when that is
 *     more than `capacity`: SURGE_E_RANGE, nothing written.  from > to: SURGE_OK, 0 rows.  An id whose last record was a tombstone
 *     is in the order (its row reads SURGE_READ_NONE).  Two binary searches on the device, 16 bytes back, one copy.
 *   - surge_device_decoder_gather_keys_device: the ids of a DEVICE row list, back to back: id q =
 *     d_utf8_out[d_off_out[q] .. d_off_out[q+1]) (n + 1 offsets).  A row outside [0, n_keys): SURGE_E_INVALID; more bytes than
 *     utf8_capacity: SURGE_E_RANGE with *total_bytes_out set — both found before anything is written.
 *   - surge_device_decoder_key_order: where the order lives (n_keys entries, the decoder's: valid until the next push that interns
 *     an id, or destroy; NULL for an empty table); builds it if stale.
 * Events decoders, state decoders and continued ones alike; a decoder that has interned nothing answers 0 rows.  SURGE_E_STATE
 * while a push is unfinished and on a poisoned decoder; SURGE_E_INVALID for a NULL decoder, a negative length or capacity.  The
 * calls run on the decoder's stream and return when their results are there.  One caller at a time per decoder. */
int32_t surge_device_decoder_range_device(surge_device_decoder* d, const uint8_t* from_utf8, int64_t from_len, const uint8_t* to_utf8, int64_t to_len,
                                          int64_t* d_rows_out, int64_t capacity, int64_t* n_out);
int32_t surge_device_decoder_gather_keys_device(surge_device_decoder* d, const int64_t* d_rows, int64_t n, uint8_t* d_utf8_out, int64_t utf8_capacity,
                                                int64_t* d_off_out, int64_t* total_bytes_out);
int32_t surge_device_decoder_key_order(surge_device_decoder* d, const int64_t** d_order, int64_t* n_keys_out, int64_t* passes_out);
/* [0] records seen, [1] delivered, [2] flush records skipped, [3] Double values re-parsed on the host */
int32_t surge_device_decoder_counters(const surge_device_decoder* d, int64_t out[4]);
/* [0..3] the counters above, [4] re-seeds of the key table's hash function — two different aggregate ids with the same
 * 64-bit hash are detected (every record's key is compared byte for byte with the key its slot stands for) and handled:
 * nothing of the push is committed, the table gets another hash function (every known key re-hashed from the key arena) and
 * the push runs again; after four functions in a row the push fails with SURGE_E_UNSUPPORTED — [5] slots of the key table,
 * [6] pushes that delivered, [7] the hash function in use (0 = the first). */
int32_t surge_device_decoder_stats(const surge_device_decoder* d, int64_t out[8]);
/* What stands behind those eight (their positions do not move, and a caller's array of eight is never overrun): the routes
 * compressed sections took — [0] snappy chunks decoded on the device, [1] snappy sections decompressed on the host (a chunk
 * above 64 KiB, a chunk but the last that is no multiple of 16 bytes, a raw block above 64 KiB), both of the pushes that
 * delivered. */
int32_t surge_device_decoder_route_stats(const surge_device_decoder* d, int64_t out[2]);

/* Key table: aggregate ids in first-DELIVERED order (a key is interned when its record is drained, so the
 * keys of aborted or still-open transactions never appear). */
int64_t surge_ingest_key_count(const surge_ingest* g);
int32_t surge_ingest_key(const surge_ingest* g, int64_t idx, const char** utf8_out, int64_t* len_out);

/* Counters: [0] batches, [1] records decoded, [2] records delivered, [3] records dropped (aborted),
 * [4] control batches, [5] flush records skipped, [6] bytes decompressed, [7] open transactions. */
int32_t surge_ingest_counters(const surge_ingest* g, int64_t out[8]);

/* Exposed for tests / other bindings. */
uint32_t surge_crc32c(const uint8_t* data, int64_t len);          /* SSE4.2 CRC32 instruction when the CPU has it */
uint32_t surge_crc32c_portable(const uint8_t* data, int64_t len); /* table walk; must always agree with the above */
/* LZ4 frame -> bytes.  Returns the decompressed size, or a negative status (-6: dst too small, -7: not a valid
 * frame, which includes a wrong header checksum — kafka-clients rejects those for message format v2 as well). */
int64_t surge_lz4_frame_decompress(const uint8_t* src, int64_t src_len, uint8_t* dst, int64_t dst_cap);
/* bytes -> LZ4 frame as kafka-clients writes it (version 01, block independence, 64 KiB blocks, header checksum).
 * dst_cap must be at least surge_lz4_frame_bound(n); returns the frame size or a negative status. */
int64_t surge_lz4_frame_bound(int64_t n);
int64_t surge_lz4_frame_compress(const uint8_t* src, int64_t n, uint8_t* dst, int64_t dst_cap);
/* XXH32 (the frame's header checksum is its second byte over the descriptor). */
uint32_t surge_xxh32(const uint8_t* data, int64_t len, uint32_t seed);
/* snappy, reading only (surge_amd/csrc/snappy_block.h).  One raw block: its preamble's length, and the block into dst.  A
 * records section — snappy-java's framing (magic, version pair, [int32 BE length][raw block] chunks) or, without the magic,
 * one raw block: the sum of its preambles (nothing decoded), and the section into dst.  Each returns the size, or -1 (bad
 * argument), -6 (dst too small) or SURGE_E_CORRUPT; *status_out (nullable) then says which refusal it was, by the number
 * surge_snappy_status_name gives a text for (0 = none). */
int64_t surge_snappy_uncompressed_length(const uint8_t* src, int64_t src_len, int32_t* status_out);
int64_t surge_snappy_uncompress(const uint8_t* src, int64_t src_len, uint8_t* dst, int64_t dst_cap, int32_t* status_out);
int64_t surge_snappy_frame_bound(const uint8_t* src, int64_t src_len, int32_t* status_out);
int64_t surge_snappy_frame_decompress(const uint8_t* src, int64_t src_len, uint8_t* dst, int64_t dst_cap, int32_t* status_out);
const char* surge_snappy_status_name(int32_t status);

#ifdef __cplusplus
}
#endif
#endif /* SURGE_INGEST_H */
