"""crdt_amd — MI355X-native MapCrdt merge hot path (drop-in for Dart ``crdt`` v4.0.2).

Public names mirror the reference barrel ``lib/crdt.dart:3-7``.
"""
from .crdt import Crdt, GroupDiff, MapCrdt, ReplicaDiff, Watch
from .crdt_json import CrdtJson
from .device import CrdtNativeError, DeviceTable, Export
from .hlc import ClockDriftException, DuplicateNodeException, Hlc, OverflowException
from .record import Record

__all__ = ["Crdt", "GroupDiff", "MapCrdt", "ReplicaDiff", "Watch", "CrdtJson", "DeviceTable", "Export", "CrdtNativeError", "Hlc",
           "Record", "ClockDriftException", "DuplicateNodeException", "OverflowException"]
