"""Events-topic ingest: Kafka record batches -> records in offset order with their aggregate index, through
the C ABI in ``include/surge_ingest.h``.  This module is the import point; the code lies in four units:

``ingest_types``    flags, record layouts, ``EventJsonTemplate`` / ``EventStrings``, ``IngestError`` — what the others share
``host_framer``     ``EventsTopicIngest``: one partition's batches framed and decoded on the host (no GPU)
``framing``         ``FramedFetches`` / ``PartitionedFramedFetches`` (framing one fetch ahead), ``pushes_in_flight``, ``PushPipeline``
``device_decoder``  ``DeviceDecoder``: records sections -> device-resident events or state values and a device key table
"""
from .device_decoder import DeviceDecoder  # noqa: F401
from .framing import Framed, FramedFetches, PartitionedFramedFetches, PushPipeline, pushes_in_flight  # noqa: F401
from .host_framer import EventsTopicIngest  # noqa: F401
from .ingest_types import (  # noqa: F401
    ARG_F64, ARG_I32, ARG_NONE, COUNTER_NAMES, DEVICE_CRC, DEVICE_LZ4, EVENT_STRING_ABSENT, EVENT_STRING_MISSING, EVENT_STRING_OK, EVENT_STRING_RECORD,
    EVJ_ENVELOPES, EVJ_MAX_TYPES, EVJ_NAME, EVS_MAX, FLOOR_DTYPE, FRAMES, NO_FLOORS, READ_COMMITTED, READ_UNCOMMITTED, RECORD_DTYPE, SECTION_CRC_PENDING,
    SECTION_CRC_WIRE, SECTION_DTYPE, SECTION_FLOORED, CEventJsonTemplate, CEventStrings, EventJsonTemplate, EventStrings, IngestError)
