"""``surge_amd.ingest`` is the import point of the ingest, its code lies in units of their own: every name that could be
imported from it before the split still can and is the unit's own object, every unit imports alone, and ``_native`` names
every export of the library once."""
import inspect
import os
import subprocess
import sys

import pytest

from surge_amd import _native

# what ``surge_amd.ingest`` offered before it was split (commit 3b6d423), by the module that holds each name now
SURFACE = {
    "surge_amd.ingest_types": (
        "READ_UNCOMMITTED", "READ_COMMITTED", "FRAMES", "DEVICE_LZ4", "DEVICE_CRC",
        "SECTION_CRC_PENDING", "SECTION_CRC_WIRE", "SECTION_FLOORED",
        "SECTION_DTYPE", "FLOOR_DTYPE", "NO_FLOORS", "RECORD_DTYPE", "COUNTER_NAMES",
        "EVJ_NAME", "EVJ_MAX_TYPES", "ARG_NONE", "ARG_I32", "ARG_F64", "EVJ_ENVELOPES",
        "CEventJsonTemplate", "EVS_MAX", "EVENT_STRING_OK", "EVENT_STRING_MISSING", "EVENT_STRING_RECORD", "EVENT_STRING_ABSENT", "CEventStrings",
        "EventStrings", "EventJsonTemplate", "IngestError"),
    "surge_amd.host_framer": ("EventsTopicIngest",),
    "surge_amd.framing": ("Framed", "FramedFetches", "PartitionedFramedFetches", "pushes_in_flight", "PushPipeline"),
    "surge_amd.device_decoder": ("DeviceDecoder",),
}
NAMES = [(module, name) for module, names in SURFACE.items() for name in names]
MODULES = ("surge_amd.ingest",) + tuple(SURFACE)


def test_the_surface_lists_each_of_its_thirty_six_names_once():
    assert len(NAMES) == 36 and len({name for _, name in NAMES}) == 36


@pytest.mark.parametrize("module,name", NAMES)
def test_a_name_of_the_surface_is_its_units_own_object(module, name):
    import importlib

    import surge_amd.ingest as surface

    here, there = getattr(surface, name), getattr(importlib.import_module(module), name)
    assert here is there
    if inspect.isclass(here) or inspect.isfunction(here):  # defined in that unit, not passed through it
        assert here.__module__ == module


@pytest.mark.parametrize("module", MODULES)
def test_a_unit_imports_alone_in_a_fresh_interpreter(module):
    code = f"import {module} as m, sys; assert 'surge_amd.ingest_types' in sys.modules; print('alone', m.__name__)"
    res = subprocess.run([sys.executable, "-c", code], cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), capture_output=True, text=True)
    assert res.returncode == 0 and res.stdout.strip() == f"alone {module}", res.stdout + res.stderr


def test_native_names_every_export_once():
    tuples = (_native.EXPORTS, _native.INGEST_EXPORTS, _native.SNAPSHOT_EXPORTS, _native.STATE_EXPORTS, _native.EVENT_STRINGS_EXPORTS)
    names = [n for t in tuples for n in t]
    assert all(isinstance(t, tuple) and t for t in tuples)
    assert len(names) == len(set(names))  # disjoint and free of duplicates
    tables = (_native.REPLAY_H, _native.INGEST_H, _native.SNAPSHOT_H)
    keys = [n for table in tables for n in table]
    assert len(keys) == len(set(keys)) and set(keys) == set(names)
    for table in tables:
        for name, (argtypes, restype) in table.items():
            assert isinstance(argtypes, list), name
