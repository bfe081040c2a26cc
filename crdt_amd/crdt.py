"""``Crdt`` / ``MapCrdt`` — drop-in mirror of ``lib/src/crdt.dart`` and
``lib/src/map_crdt.dart`` whose storage and merge live on an MI355X.

The public surface keeps the reference's names and argument meanings
(``put``, ``putAll``, ``delete``, ``get``, ``merge``, ``mergeJson``,
``canonicalTime``, ``refreshCanonicalTime``, ``toJson``, ``recordMap``,
``watch``, ...).  Every clock read takes an optional ``wall`` (ms since epoch);
by default ``self.clock()`` = the host wall clock, as ``DateTime.now()`` is in
the reference.  ``mergeAll`` is the batched extension: R sequential merges in
one device call (the hot path of the benchmark).
"""
from __future__ import annotations

import weakref

import numpy as np

from . import _capi
from .crdt_json import CrdtJson
from .device import CrdtNativeError, DeviceTable
from .hlc import (ClockDriftException, DuplicateNodeException, Hlc, OverflowException, now_millis)
from .intern import NULL_HANDLE, KeyIndex, NodeRanks, ValueStore
from .record import Record


class Watch:
    """A subscription to change events (``Stream<MapEntry<K, V?>>``, map_crdt.dart:47-49)."""

    def __init__(self, key=None, has_key=False):
        self.key = key
        self._has_key = has_key
        self.events: list = []

    def _offer(self, key, value):
        if not self._has_key or key == self.key:
            self.events.append((key, value))

    def __iter__(self):
        return iter(self.events)

    def __len__(self):
        return len(self.events)


class ReplicaDiff:
    """What ``MapCrdt.diff`` found: the number of keys on which this map holds the winning record
    (``ahead``), on which the other does (``behind``), and on which both hold one Hlc with different values
    (``conflicts``: no merge heals those).  With ``keys=True`` also the three key lists (else None)."""

    __slots__ = ("ahead", "behind", "conflicts", "ahead_keys", "behind_keys", "conflict_keys")

    def __init__(self, ahead: int, behind: int, conflicts: int, ahead_keys=None, behind_keys=None,
                 conflict_keys=None):
        self.ahead, self.behind, self.conflicts = int(ahead), int(behind), int(conflicts)
        self.ahead_keys, self.behind_keys, self.conflict_keys = ahead_keys, behind_keys, conflict_keys

    @property
    def converged(self) -> bool:
        return self.ahead == 0 and self.behind == 0 and self.conflicts == 0

    def __repr__(self):
        return f"ReplicaDiff(ahead={self.ahead}, behind={self.behind}, conflicts={self.conflicts})"


class GroupDiff:
    """What ``MapCrdt.groupDiff`` found among ``maps = [self, *replicas]``: per map, in ``maps`` order, the number
    of keys on which it lacks the group's winning record (``behind``) and on which it alone holds it (``sole``:
    news nobody else has); the number of keys on which some map is behind (``disputed``) and on which two holders
    of the winning Hlc carry different values (``conflicts``: no merge heals those).  With ``keys=True`` also
    ``behind_keys[j]`` per map and ``conflict_keys`` (else None)."""

    __slots__ = ("behind", "sole", "disputed", "conflicts", "behind_keys", "conflict_keys")

    def __init__(self, behind, sole, disputed: int, conflicts: int, behind_keys=None, conflict_keys=None):
        self.behind, self.sole = [int(x) for x in behind], [int(x) for x in sole]
        self.disputed, self.conflicts = int(disputed), int(conflicts)
        self.behind_keys, self.conflict_keys = behind_keys, conflict_keys

    @property
    def converged(self) -> bool:
        return self.disputed == 0 and self.conflicts == 0

    def __repr__(self):
        return (f"GroupDiff(behind={self.behind}, sole={self.sole}, disputed={self.disputed}, "
                f"conflicts={self.conflicts})")


def _any_two_differ(values: list) -> bool:
    return any(a != b for i, a in enumerate(values) for b in values[i + 1:])


FILL_LT = -0x7F7F7F7F7F7F7F80     # lt of a never-written row (bytes 0x80: DESIGN.md §2), outside the clock domain


class _ReplicaGroup:
    """The id space several ``MapCrdt``s of one device share (``MapCrdt.replica``): one key index, one
    node ranking and one value store, which is what every table-to-table form asks of its ctxs.  Members are
    held weakly; a ``MapCrdt`` that never calls ``replica()`` is a group of one."""

    def __init__(self):
        self.keys = KeyIndex()
        self.nodes = NodeRanks()
        self.values = ValueStore()
        self._members: list = []

    def add(self, member):
        self._members.append(weakref.ref(member))

    def members(self) -> list:
        live = [(r, m) for r, m in ((r, r()) for r in self._members) if m is not None]
        self._members = [r for r, _ in live]
        return [m for _, m in live]

    def register(self, node_ids):
        """New node ids for every member: a shift of ranks re-ranks every member's rows, and every member's
        local rank and rank bound follow."""
        lut = self.nodes.register(node_ids)
        members = self.members()
        if lut is not None:
            for m in members:
                m._reserve()
                m._table.remap_ranks(len(self.keys), lut)
                m._table.local_rank = self.nodes.rank(m.nodeId)
        for m in members:
            if len(self.nodes) != m._rank_bound:      # ranks are dense: 0 .. len - 1
                m._rank_bound = len(self.nodes)
                m._table.set_rank_bound(m._rank_bound)


class Crdt:
    """Abstract ``Crdt<K, V>`` (crdt.dart:7-170): the API over a storage SPI."""

    # ---- views (crdt.dart:13-29) ----
    @property
    def isEmpty(self) -> bool:
        return len(self.map) == 0

    @property
    def length(self) -> int:
        return len(self.map)

    @property
    def map(self) -> dict:
        return {k: r.value for k, r in self.recordMap().items() if not r.isDeleted}

    @property
    def keys(self) -> list:
        return list(self.map.keys())

    @property
    def values(self) -> list:
        return list(self.map.values())

    def get(self, key):                                                 # crdt.dart:36
        r = self.getRecord(key)
        return None if r is None else r.value

    def delete(self, key, wall: int | None = None):                     # crdt.dart:58
        self.put(key, None, wall=wall)

    def isDeleted(self, key):                                           # crdt.dart:62
        r = self.getRecord(key)
        return None if r is None else r.isDeleted

    def clear(self, purge: bool = False, wall: int | None = None):      # crdt.dart:67-73
        if purge:
            self.purge()
        else:
            self.putAll({k: None for k in self.map}, wall=wall)

    def mergeJson(self, js: str, keyDecoder=None, valueDecoder=None, wall: int | None = None):
        wall = self._wall(wall)                                         # crdt.dart:100-109
        if keyDecoder is None and valueDecoder is None and self._native_ingest():
            from . import hostlib
            n0 = len(self._keys)
            try:
                dec = hostlib.decode(js, self._keys.native)             # libcrdt_host.so
            except (hostlib.Fallback, ValueError):
                dec = None                                              # the restatement decides
            if dec is not None:
                self.last_ingest = "native"
                return self._merge_decoded(dec, n0, wall)
        self.last_ingest = "python"
        m = CrdtJson.decode(js, self.canonicalTime, keyDecoder=keyDecoder, valueDecoder=valueDecoder,
                            millis=wall)
        self.merge(m, wall=wall)

    def _native_ingest(self) -> bool:
        return False

    def toJson(self, modifiedSince: Hlc | None = None, keyEncoder=None, valueEncoder=None) -> str:
        return CrdtJson.encode(self.recordMap(modifiedSince=modifiedSince),           # crdt.dart:127-135
                               keyEncoder=keyEncoder, valueEncoder=valueEncoder)

    def __str__(self):
        return str(self.recordMap())

    def _wall(self, wall):
        return self.clock() if wall is None else int(wall)


class MapCrdt(Crdt):
    """``MapCrdt<K, V>`` (map_crdt.dart:9-53) with its map on the GPU.

    ``MapCrdt(nodeId, seed)`` keeps the reference's constructor quirk: the
    canonical clock is refreshed on the still-empty map (crdt.dart:31-33) before
    the seed is added (map_crdt.dart:16-18), so it starts at 0.
    """

    def __init__(self, nodeId, seed: dict | None = None, *, device: int = 0, capacity: int = 1024,
                 clock=None, _group: _ReplicaGroup | None = None):
        self.nodeId = nodeId
        self.clock = clock or now_millis
        self._group = _group or _ReplicaGroup()
        self._keys = self._group.keys
        self._nodes = self._group.nodes
        self._values = self._group.values
        self._hlc_override: dict = {}     # key id -> Hlc not in canonical (millis, counter) form
        self._mod_override: dict = {}     # key id -> modified Hlc with a foreign node / odd form
        self._watches: list = []
        self._rank_bound = 0
        self.last_sync = None             # "table" | "object": how the last replica sync into this map ran
        self.last_sync_winners = None     # winner records it fetched from the device (None: no export ran)
        self.last_diff = None             # "table" | "object": how this map's last diff() / groupDiff() ran
        self.last_clear = None            # "table": the last clear() ran on the device table
        self.last_purge = None            # "table" | "object": how this map's last purgeDeleted() ran
        self._purged = False              # purgeDeleted() dropped a key here: its id stays, its row is the fill
        self._group.register([nodeId])    # (a shift of ranks reaches the members there are)
        self._table = DeviceTable(device, local_rank=self._nodes.rank(nodeId), capacity=capacity)
        self._table.set_rank_bound(len(self._nodes))
        self._rank_bound = len(self._nodes)
        self._group.add(self)
        self.refreshCanonicalTime()
        if seed:
            self._store(list(seed.items()), notify=False)

    def replica(self, nodeId, seed: dict | None = None, *, capacity: int | None = None, clock=None) -> "MapCrdt":
        """A new ``MapCrdt`` on this one's device that shares its key ids, node ranks and value handles, with
        a table, canonical clock, node id, watches and overrides of its own: the replicas of one group sync on
        the device (``mergeFrom``, ``syncWith``, ``mergeFromAll``, ``broadcastTo``).  A node id equal to a
        sibling's is allowed (a merge between the two then raises ``DuplicateNodeException``, as the
        reference's does).  A group iterates its keys in the order the GROUP first saw them."""
        cap = self._table.capacity if capacity is None else int(capacity)
        return MapCrdt(nodeId, seed, device=self._table.device, capacity=cap, clock=clock or self.clock,
                       _group=self._group)

    # ------------------------------------------------------------ internals
    def _register_nodes(self, node_ids):
        self._group.register(node_ids)

    def _shared(self) -> bool:
        """Whether this map has live siblings (a group of one answers as a plain ``MapCrdt`` always has)."""
        return len(self._group.members()) > 1

    def _sparse(self) -> bool:
        """Whether an interned key may have no record here: a sibling interned it, or purgeDeleted() dropped
        it (either way its row holds the never-written fill, ``FILL_LT``)."""
        return self._purged or self._shared()

    def _reserve(self):
        if len(self._keys) > self._table.capacity:
            self._table.reserve(len(self._keys))

    def _emit(self, key, value):
        for w in self._watches:
            w._offer(key, value)

    def _note_overrides(self, kid: int, hlc: Hlc, modified: Hlc | None):
        if hlc.is_canonical_form:
            self._hlc_override.pop(kid, None)
        else:
            self._hlc_override[kid] = hlc
        if modified is None or (modified.nodeId == self.nodeId and modified.is_canonical_form):
            self._mod_override.pop(kid, None)
        else:
            self._mod_override[kid] = modified

    def _store(self, items, notify: bool):
        """putRecord(s) (map_crdt.dart:27-39): rows stored verbatim."""
        if not items:
            return
        self._register_nodes([r.hlc.nodeId for _, r in items])
        n = len(items)
        kid = np.empty(n, np.uint32)
        lt = np.empty(n, np.int64)
        rank = np.empty(n, np.uint32)
        val = np.empty(n, np.uint32)
        mod = np.empty(n, np.int64)
        for i, (k, r) in enumerate(items):
            kid[i] = self._keys.intern(k)
            lt[i] = r.hlc.logicalTime
            rank[i] = self._nodes.rank(r.hlc.nodeId)
            val[i] = self._values.put(r.value)
            mod[i] = r.modified.logicalTime
            self._note_overrides(int(kid[i]), r.hlc, r.modified)
        self._reserve()
        self._table.put_rows(kid, lt, rank, val, mod)
        if notify:
            for k, r in items:
                self._emit(k, r.value)
        self._maybe_compact()

    def _maybe_compact(self):
        if len(self._values) > 2 * max(4096, len(self._keys)):
            ids = np.arange(len(self._keys), dtype=np.uint32)
            live = []
            for m in self._group.members():             # several tables may hold one handle
                m._reserve()
                val = m._table.read_rows(ids)[2]
                live.append(val[val != NULL_HANDLE])
            self._values.compact(live[0] if len(live) == 1 else np.concatenate(live))

    def _raise_for(self, res: dict):
        st = res["status"]
        if st == _capi.CRDT_CLOCK_DRIFT:
            raise ClockDriftException(res["drift_ms"], 0)
        if st == _capi.CRDT_DUPLICATE_NODE:
            raise DuplicateNodeException(str(self.nodeId))
        if st == _capi.CRDT_OVERFLOW:
            raise OverflowException(res["counter"])

    def _make_record(self, kid: int, lt: int, rank: int, val: int, mod: int) -> Record:
        hlc = self._hlc_override.get(kid) or Hlc.fromLogicalTime(int(lt), self._nodes.node(int(rank)))
        modified = self._mod_override.get(kid) or Hlc.fromLogicalTime(int(mod), self.nodeId)
        return Record(hlc, self._values.get(int(val)), modified)

    # ------------------------------------------------------------ views
    @property
    def length(self) -> int:                                            # crdt.dart:20 (map.length)
        """Live records counted on the device (crdt_count_since): no Record is built."""
        self._reserve()
        return self._table.count_since(len(self._keys), 0)[1]

    @property
    def isEmpty(self) -> bool:                                          # crdt.dart:17
        return self.length == 0

    def _live_columns(self):
        """(key ids, value handles) of the live records in id order (crdt_export_live), as lists."""
        self._reserve()
        ex = self._table.export_live(len(self._keys))
        if ex.n == 0:
            return [], []
        ids, _, _, val, _ = ex.columns()
        return ids.tolist(), val.tolist()

    @property
    def map(self) -> dict:                                              # crdt.dart:22-24
        """The live records' values, compacted on the device: no Record and no Hlc is built."""
        ids, val = self._live_columns()
        names, get = self._keys.keys, self._values.get
        return {names[i]: get(v) for i, v in zip(ids, val)}

    @property
    def keys(self) -> list:                                             # crdt.dart:26
        names = self._keys.keys
        return [names[i] for i in self._live_columns()[0]]

    @property
    def values(self) -> list:                                           # crdt.dart:29
        get = self._values.get
        return [get(v) for v in self._live_columns()[1]]

    # ------------------------------------------------------------ SPI
    def containsKey(self, key) -> bool:                                 # map_crdt.dart:21
        kid = self._keys.get(key)
        if kid is None or not self._sparse():
            return kid is not None
        self._reserve()                                 # (a sibling may have interned the key)
        return int(self._table.read_rows(np.array([kid], np.uint32))[0][0]) != FILL_LT

    def getRecord(self, key):                                           # map_crdt.dart:24
        kid = self._keys.get(key)
        if kid is None:
            return None
        shared = self._sparse()
        if shared:
            self._reserve()
        lt, rank, val, mod = self._table.read_rows(np.array([kid], np.uint32))
        if shared and int(lt[0]) == FILL_LT:            # known to the group, never written here
            return None
        return self._make_record(kid, lt[0], rank[0], val[0], mod[0])

    def putRecord(self, key, record: Record):                           # map_crdt.dart:27-30
        self._store([(key, record)], notify=True)

    def putRecords(self, records: dict):                                # map_crdt.dart:33-39
        self._store(list(records.items()), notify=True)

    def recordMap(self, modifiedSince: Hlc | None = None) -> dict:      # map_crdt.dart:42-45
        since = modifiedSince.logicalTime if modifiedSince is not None else 0
        self._reserve()
        ex = self._table.export_since(len(self._keys), since)       # one device compaction of all columns
        if ex.n == 0:
            return {}
        ids, lt, rank, val, mod = ex.columns()
        keys = self._keys.keys
        return {keys[int(i)]: self._make_record(int(i), lt[x], rank[x], val[x], mod[x])
                for x, i in enumerate(ids)}

    def toJson(self, modifiedSince: Hlc | None = None, keyEncoder=None, valueEncoder=None) -> str:
        """crdt.dart:127-135 over recordMap (map_crdt.dart:42-45).  String keys and no encoders:
        the rows come from the device compaction (crdt_modified_since) and the document is
        assembled natively (hostlib.encode) — keys from the native table, Hlc.toString of the
        columns, raw input values reused when already in dumps form — so no Record is built.
        Anything else, or a Fallback from the native side, runs the restatement."""
        if keyEncoder is None and valueEncoder is None and self._keys.native is not None:
            from . import hostlib
            try:
                return self._native_export(modifiedSince)
            except hostlib.Fallback:
                pass
        self.last_export = "python"
        return super().toJson(modifiedSince, keyEncoder=keyEncoder, valueEncoder=valueEncoder)

    def _native_export(self, modifiedSince: Hlc | None) -> str:
        import json

        from . import hostlib
        from .crdt_json import _default
        since = modifiedSince.logicalTime if modifiedSince is not None else 0
        self._reserve()
        ex = self._table.export_since(len(self._keys), since)
        if ex.n == 0:
            self.last_export = "native"
            return "{}"
        ids, lt, rank, val, _ = ex.columns()
        hlc_text = None
        if self._hlc_override:
            pos = {int(k): x for x, k in enumerate(ids.tolist())} if len(self._hlc_override) > 64 else None
            for kid, h in self._hlc_override.items():
                row = pos.get(kid) if pos is not None else (
                    int(np.searchsorted(ids, kid)) if kid <= int(ids[-1]) else None)
                if row is not None and row < len(ids) and int(ids[row]) == kid:
                    hlc_text = hlc_text or {}
                    hlc_text[row] = str(h)

        def dumps(objs):
            return json.dumps(objs, separators=(",", ":"), ensure_ascii=False, default=_default)

        ptr, ln, keep = self._values.texts(val, dumps)
        nodes = [self._nodes.node(r) for r in range(len(self._nodes))]
        out = hostlib.encode(self._keys.native, ids, lt, rank, nodes, ptr, ln, hlc_text)
        del keep
        self.last_export = "native"
        return out

    def watch(self, key=None, **kw) -> Watch:                           # map_crdt.dart:47-49
        w = Watch(key, has_key=("key" in kw) or key is not None)
        self._watches.append(w)
        return w

    def purge(self):                                                    # map_crdt.dart:52
        self._reserve()
        self._table.clear_rows(0, len(self._keys))
        if not self._shared():                          # (a member clears its own rows and overrides only)
            self._keys.clear()
            self._values.clear()
            self._purged = False                        # (no key id is left without a record)
        self._hlc_override.clear()
        self._mod_override.clear()

    # ------------------------------------------------------------ clock
    @property
    def canonicalTime(self) -> Hlc:                                     # crdt.dart:11
        return Hlc.fromLogicalTime(self._table.canonical, self.nodeId)

    def refreshCanonicalTime(self):                                     # crdt.dart:114-121
        self._reserve()
        self._table.refresh_canonical(len(self._keys))

    # ------------------------------------------------------------ writes
    def put(self, key, value, wall: int | None = None):                 # crdt.dart:39-43
        self.putAll({key: value}, wall=wall)

    def putAll(self, values: dict, wall: int | None = None):          # crdt.dart:46-54
        if not values:
            return
        wall = self._wall(wall)
        n0 = len(self._keys)
        items = list(values.items())
        kid = np.array([self._keys.intern(k) for k, _ in items], np.uint32)
        handles = np.array([self._values.put(v) for _, v in items], np.uint32)
        self._reserve()
        res = self._table.put_stamped(kid, handles, wall)
        if res["status"] != 0:
            self._keys.truncate(n0)
            for h in handles:
                self._values.release(int(h))
            self._raise_for(res)
        for i in kid:
            self._hlc_override.pop(int(i), None)
            self._mod_override.pop(int(i), None)
        for k, v in items:
            self._emit(k, v)
        self._maybe_compact()

    def clear(self, purge: bool = False, wall: int | None = None):      # crdt.dart:67-73
        """``putAll`` of ``None`` over ``self.map``, decided and stored on the table (crdt_tombstone_live): one
        ``Hlc.send``, every live record becomes a tombstone, and nothing moves when there is none.  The ids
        of the cleared keys are fetched (crdt_export_flagged on this map's own table) only for a map that has
        a watch or keeps an Hlc / modified on the host.  In a replica group a key that only siblings have
        written is not live here and stays unwritten."""
        if purge:
            return self.purge()
        wall = self._wall(wall)
        self._reserve()
        n = len(self._keys)
        res, flags = self._table.tombstone_live(n, wall, row_flags=self._wants_winners())
        self.last_clear = "table"
        self._raise_for(res)
        if res["n_won"] and flags is not None:
            ids = self._table.export_flagged(n, flags, 1).columns()[0].tolist()
            for k in ids:                               # canonical-form Hlc, modified by this node
                self._hlc_override.pop(k, None)
                self._mod_override.pop(k, None)
            if self._watches:
                keys = self._keys.keys
                for k in ids:                           # id order: the order self.map iterates
                    self._emit(keys[k], None)
        self._maybe_compact()

    def purgeDeleted(self, before: Hlc | None = None, replicas=()) -> int:
        """Tombstone collection: drop the deletions that this map and every one of ``replicas`` hold alike.
        Let P be the keys k that every map m of ``[self, *replicas]`` holds in ``m.recordMap()`` (a record with a
        negative ``modified`` is not seen by it, as it is not by ``merge``), each such record ``isDeleted`` and
        with the Hlc that ``self``'s has, that Hlc's ``logicalTime`` below ``before.logicalTime``
        (``before=None``: no bound).  Every key of P is removed from the storage of every
        one of those maps, and ``len(P)`` is returned.  A replica that has not seen the deletion blocks it in
        all of them: it could still hand the older live record back.  No watch event is emitted, no clock
        moves, ``last_sync`` is untouched and nothing is interned.

        Between up to ``_capi.PURGE_MAX`` members of one group that keep no Hlc on the host it runs on the
        device tables (``crdt_purge_tombstones``, ``last_purge == "table"``); the purged ids are fetched
        (``crdt_export_flagged``) only when a participant keeps a ``modified`` on the host, whose entries of the
        purged keys are dropped.  Anything else runs the definition on the ``recordMap()``s and clears the rows
        one by one (``last_purge == "object"``): maps of different groups, an Hlc kept on the host, and more
        than ``PURGE_MAX`` maps (one call purges what its members agree on at once, so a second chunk could
        not take back what a ninth map blocks).

        A purged key keeps its key id: a later ``put`` or ``merge`` of it stores it again at its old place in
        the iteration order (the group's "first seen" order rule), and a map that has purged anything answers
        ``containsKey`` / ``getRecord`` / ``isDeleted`` / ``get`` through the never-written check that group
        members use, until ``purge()`` on an unshared map resets it."""
        maps, table = self._members(replicas, _capi.PURGE_MAX, "purge together")
        if not table:
            self.last_purge = "object"
            return self._purge_objects(maps, before)
        self.last_purge = "table"
        n = len(self._keys)
        for m in maps:
            m._reserve()
        keyed = any(m._mod_override for m in maps)
        before_lt = before.logicalTime if before is not None else (1 << 63) - 1
        res, flags = self._table.purge_tombstones([m._table for m in maps[1:]], n, before_lt, row_flags=keyed)
        if res["n_purged"]:
            if keyed:
                ids = self._table.export_flagged(n, flags, 1).columns()[0].tolist()
            for m in maps:
                m._purged = True
                if m._mod_override:
                    for k in ids:
                        m._mod_override.pop(k, None)
        return res["n_purged"]

    def _members(self, replicas, limit: int, cannot: str):
        """``[self, *replicas]`` de-duplicated by identity, and whether an operation over them runs on the device
        tables: at most ``limit`` members, all of one group, none keeping an Hlc on the host.  ``cannot``: what
        replicas of different devices are refused with."""
        maps = [self]
        for m in replicas:
            if not any(m is x for x in maps):
                maps.append(m)
        if any(m._table.device != self._table.device for m in maps):
            raise ValueError(f"replicas of different devices cannot {cannot}")
        return maps, (len(maps) <= limit and all(m._group is self._group for m in maps)
                      and not any(m._hlc_override for m in maps))

    @staticmethod
    def _purge_objects(maps, before: Hlc | None) -> int:
        """The definition itself, on the maps' recordMap()s."""
        first, rest = maps[0].recordMap(), [m.recordMap() for m in maps[1:]]
        purged = []
        for k, r in first.items():
            if not r.isDeleted or (before is not None and not r.hlc.logicalTime < before.logicalTime):
                continue
            others = [rm.get(k) for rm in rest]
            if all(o is not None and o.isDeleted and o.hlc == r.hlc for o in others):
                purged.append(k)
        for m in maps:
            for k in purged:
                kid = m._keys.get(k)
                m._table.clear_rows(kid, 1)
                m._hlc_override.pop(kid, None)
                m._mod_override.pop(kid, None)
            m._purged = m._purged or bool(purged)
        return len(purged)

    # ------------------------------------------------------------ merge
    def _native_ingest(self) -> bool:
        return self._keys.native is not None and self._nodes.kind in (None, "str")

    def _merge_decoded(self, dec: dict, n0: int, wall: int):
        """merge() of one natively decoded CrdtJson document (crdt.dart:77-94 on columns):
        keys already interned (ids >= n0 are new), values still raw JSON text."""
        kid, lt, nodes = dec["key_id"], dec["lt"], dec["nodes"]
        n = len(kid)
        self._register_nodes(nodes)
        lut = np.array([self._nodes.rank(x) for x in nodes], np.uint32)
        rank = lut[dec["node"]] if n else np.zeros(0, np.uint32)
        val = self._values.put_raw(dec["buf"], dec["val_off"], dec["val_len"])
        self._reserve()
        res, flags = self._table.merge(kid, lt, rank, val, np.array([0, n], np.uint64), wall)
        won = flags[:n].astype(bool) if res["n_stored"] else np.zeros(n, bool)
        if not res["n_stored"]:
            self._keys.truncate(n0)                    # keys of an unstored changeset never entered
        self._values.release_many(val[~won & (val != NULL_HANDLE)])
        if won.any() and (self._hlc_override or self._mod_override):
            for k in kid[won].tolist():                 # canonical-form Hlc, modified by this node
                self._hlc_override.pop(k, None)
                self._mod_override.pop(k, None)
        if won.any() and self._watches:
            keys = self._keys.keys
            for x in np.flatnonzero(won).tolist():
                self._emit(keys[int(kid[x])], self._values.get(int(val[x])))
        self._maybe_compact()
        self._raise_for(res)
        return res

    def merge(self, remoteRecords: dict, wall: int | None = None):    # crdt.dart:77-94
        self.mergeAll([remoteRecords], wall=wall)

    def mergeAllBulk(self, changesets, wall: int | None = None):
        """The catch-up form of ``mergeAll``: the same R sequential merges (rows, canonical clock,
        exceptions), but the merged maps are not cut down to their winners (``removeWhere``,
        crdt.dart:80-85) and no ``watch()`` event is emitted, so no per-record outcome is needed and
        the device may take the sorted path's order-free form.  Mirrors
        ``GpuMapCrdt.mergeAllBulk`` (dart/lib/src/gpu_map_crdt.dart).  A batch that needs per-record
        host bookkeeping — an Hlc outside the (millis << 16) + counter form, or a key whose stored
        Hlc / modified is kept on the host — runs as ``mergeAll``."""
        wall = self._wall(wall)
        changesets = list(changesets)
        R = len(changesets)
        if R == 0:
            return
        if self._hlc_override or self._mod_override or any(
                not r.hlc.is_canonical_form for cs in changesets for r in cs.values()):
            keyed = set(self._hlc_override) | set(self._mod_override)
            if any(not r.hlc.is_canonical_form for cs in changesets for r in cs.values()) or any(
                    self._keys.get(k) in keyed for cs in changesets for k in cs):
                self.mergeAll([dict(cs) for cs in changesets], wall=wall)   # (copies: maps untouched)
                return
        self._register_nodes([r.hlc.nodeId for cs in changesets for r in cs.values()])
        n_total = sum(len(cs) for cs in changesets)
        kid = np.empty(n_total, np.uint32)
        lt = np.empty(n_total, np.int64)
        rank = np.empty(n_total, np.uint32)
        val = np.empty(n_total, np.uint32)
        offsets = np.zeros(R + 1, np.uint64)
        newid_start = []
        i = 0
        for j, cs in enumerate(changesets):
            newid_start.append(len(self._keys))
            for key, rec in cs.items():
                kid[i] = self._keys.intern(key)
                lt[i] = rec.hlc.logicalTime
                rank[i] = self._nodes.rank(rec.hlc.nodeId)
                val[i] = self._values.put(rec.value)
                i += 1
            offsets[j + 1] = i
        newid_start.append(len(self._keys))
        self._reserve()
        self._table.set_counts(False)
        try:
            res, _ = self._table.merge(kid, lt, rank, val, offsets, wall, win_flags=False)
        except CrdtNativeError:
            self._keys.truncate(newid_start[0])
            self._values.release_many(val)
            raise
        finally:
            self._table.set_counts(True)
        stop = res["n_stored"]
        self._keys.truncate(newid_start[stop])
        self._values.release_many(val[int(offsets[stop]):])       # changesets never stored
        # the stored changesets' losing handles are unknown here: the next compaction frees them
        self._maybe_compact()
        self._raise_for(res)
        return res

    def mergeAll(self, changesets, wall: int | None = None):
        """``for m in changesets: merge(m)`` as ONE device call (R sequential merges)."""
        wall = self._wall(wall)
        changesets = list(changesets)
        R = len(changesets)
        if R == 0:
            return
        self._register_nodes([r.hlc.nodeId for cs in changesets for r in cs.values()])
        n_total = sum(len(cs) for cs in changesets)
        kid = np.empty(n_total, np.uint32)
        lt = np.empty(n_total, np.int64)
        rank = np.empty(n_total, np.uint32)
        val = np.empty(n_total, np.uint32)
        odd = []                  # (index, Hlc.millis) of Hlcs outside the (millis << 16) + counter form
        offsets = np.zeros(R + 1, np.uint64)
        newid_start = []
        items = []
        i = 0
        for j, cs in enumerate(changesets):
            newid_start.append(len(self._keys))
            for key, rec in cs.items():
                h = rec.hlc
                kid[i] = self._keys.intern(key)
                lt[i] = h.logicalTime
                rank[i] = self._nodes.rank(h.nodeId)
                val[i] = self._values.put(rec.value)
                if not h.is_canonical_form:
                    odd.append((i, h.millis))
                items.append((key, rec))
                i += 1
            offsets[j + 1] = i
        newid_start.append(len(self._keys))
        millis = None
        if odd:                   # built from the COMPLETE lt column, then the odd Hlcs patched in
            millis = lt >> 16
            for x, ms in odd:
                millis[x] = ms
        self._reserve()
        try:
            res, flags = self._table.merge(kid, lt, rank, val, offsets, wall, millis=millis)
        except CrdtNativeError:
            # the library refused the call (nothing stored on a single context, include/crdt_merge.h):
            # forget the keys and value handles this batch interned
            self._keys.truncate(newid_start[0])
            for x in range(n_total):
                self._values.release(int(val[x]))
            raise
        stop = res["n_stored"]
        # keys first seen in changesets that were not stored never entered the map
        self._keys.truncate(newid_start[stop])
        stored_end = int(offsets[stop])
        for x in range(n_total):
            if x >= stored_end or not flags[x]:
                self._values.release(int(val[x]))
        # the reference mutates each merged Map to its winners (removeWhere, crdt.dart:80-85)
        for j in range(stop):
            cs = changesets[j]
            b = int(offsets[j])
            for x, key in enumerate(list(cs.keys())):
                if not flags[b + x]:
                    del cs[key]
            for key, rec in cs.items():
                k = self._keys.get(key)
                self._note_overrides(k, rec.hlc, None)
                self._emit(key, rec.value)
        self._maybe_compact()
        self._raise_for(res)
        return res

    # ------------------------------------------------------------ replica sync
    # Each member below is DEFINED as a composition of merge() and recordMap() calls and leaves exactly what
    # that composition leaves on every replica.  Between members of one group it runs as a table-to-table
    # form on the device (include/crdt_merge.h); the records a merge stored are fetched (crdt_export_flagged
    # on the SOURCE table, with the merge's row flags) only for a storing replica that has a watch or keeps
    # an Hlc / modified on the host.  The object route is the composition itself: it is taken when a source
    # keeps an Hlc outside the (millis << 16) + counter form (its millis is not lt >> 16, which the tables
    # cannot see) or the replicas do not share a group.

    @staticmethod
    def _since_lt(h: Hlc | None) -> int:
        return h.logicalTime if h is not None else 0

    @staticmethod
    def _sinces_for(sinces, replicas, method: str, noun: str) -> list:
        """One ``modifiedSince`` per replica (None: none for any), or ValueError."""
        sinces = [None] * len(replicas) if sinces is None else list(sinces)
        if len(sinces) != len(replicas):
            raise ValueError(f"{method}: {len(replicas)} {noun} but {len(sinces)} sinces")
        return sinces

    def _table_route(self, sources, others=()) -> bool:
        """Whether a sync among self, ``sources`` and ``others`` runs on the device tables."""
        everyone = [self, *sources, *others]
        if any(m._table.device != self._table.device for m in everyone):
            raise ValueError("replicas of different devices cannot sync")
        return all(m._group is self._group for m in everyone) and not any(m._hlc_override for m in sources)

    def _wants_winners(self) -> bool:
        return bool(self._watches or self._hlc_override or self._mod_override)

    def _took(self, src: "MapCrdt", n_rows: int, flags, bit: int):
        """Bookkeeping of one stored table merge into self: the winners, read from src's table."""
        self.last_sync = "table"
        if flags is None:
            return
        ex = src._table.export_flagged(n_rows, flags, 1 << bit)
        self.last_sync_winners = (self.last_sync_winners or 0) + ex.n
        if ex.n == 0:
            return
        ids, _, _, val, _ = ex.columns()
        if self._hlc_override or self._mod_override:
            for k in ids.tolist():                      # canonical-form Hlc, modified by this node
                self._hlc_override.pop(k, None)
                self._mod_override.pop(k, None)
        if self._watches:
            keys, values = self._keys.keys, self._values
            for k, v in zip(ids.tolist(), val.tolist()):
                self._emit(keys[k], values.get(v))

    def _sync_rows(self, *replicas) -> int:
        n = len(self._keys)
        for m in replicas:
            m._reserve()
            m.last_sync_winners = None
        return n

    def mergeFrom(self, src: "MapCrdt", modifiedSince: Hlc | None = None, wall: int | None = None):
        """``self.merge(src.recordMap(modifiedSince=modifiedSince), wall=wall)``."""
        wall = self._wall(wall)
        if not self._table_route([src]):
            self.last_sync, self.last_sync_winners = "object", None
            return self.merge(src.recordMap(modifiedSince=modifiedSince), wall=wall)
        n = self._sync_rows(self, src)
        res, flags = self._table.merge_table(src._table, n, self._since_lt(modifiedSince), wall,
                                             row_flags=self._wants_winners())
        self.last_sync = "table"
        if res["n_stored"]:
            self._took(src, n, flags, 0)
        self._maybe_compact()
        self._raise_for(res)

    def syncWith(self, other: "MapCrdt", sinceSelf: Hlc | None = None, sinceOther: Hlc | None = None,
                 wall: int | None = None):
        """``self.merge(other.recordMap(modifiedSince=sinceOther))`` then, unless that raised,
        ``other.merge(self.recordMap(modifiedSince=sinceSelf))``, one ``wall`` for both.  The reference's
        ``_sync(local, remote)`` is ``t = local.canonicalTime; remote.syncWith(local, sinceSelf=t)``."""
        wall = self._wall(wall)
        if not self._table_route([other, self]):
            self.last_sync, self.last_sync_winners = "object", None
            self.merge(other.recordMap(modifiedSince=sinceOther), wall=wall)
            other.last_sync, other.last_sync_winners = "object", None
            return other.merge(self.recordMap(modifiedSince=sinceSelf), wall=wall)
        n = self._sync_rows(self, other)
        (res_a, fl_a), (res_b, fl_b) = self._table.sync_tables(
            other._table, n, self._since_lt(sinceSelf), self._since_lt(sinceOther), wall,
            row_flags=(self._wants_winners(), other._wants_winners()))
        self.last_sync = "table"
        if res_a["n_stored"]:
            self._took(other, n, fl_a, 0)               # other's copy of what self took is unchanged (a tie)
        if res_a["status"] == 0:
            other.last_sync = "table"
            if res_b["n_stored"]:
                other._took(self, n, fl_b, 0)           # self is not written after its own merge
        self._maybe_compact()
        self._raise_for(res_a)
        other._raise_for(res_b)

    def mergeFromAll(self, srcs, sinces=None, wall: int | None = None):
        """``for s, t in zip(srcs, sinces): self.merge(s.recordMap(modifiedSince=t))``, ending at the first
        that raises."""
        wall = self._wall(wall)
        srcs = list(srcs)
        sinces = self._sinces_for(sinces, srcs, "mergeFromAll", "sources")
        if not self._table_route(srcs):
            self.last_sync, self.last_sync_winners = "object", None
            for s, t in zip(srcs, sinces):
                self.merge(s.recordMap(modifiedSince=t), wall=wall)
            return
        n = self._sync_rows(self, *srcs)
        try:
            for c in range(0, len(srcs), _capi.FANIN_MAX):      # a sequence: consecutive chunks are exact
                part = srcs[c:c + _capi.FANIN_MAX]
                res, mask = self._table.merge_tables([s._table for s in part], n,
                                                     [self._since_lt(t) for t in sinces[c:c + len(part)]], wall,
                                                     win_mask=self._wants_winners())
                self.last_sync = "table"
                for j, s in enumerate(part):
                    if res[j]["n_stored"]:
                        self._took(s, n, mask, j)
                    self._raise_for(res[j])
        finally:
            self._maybe_compact()

    def broadcastTo(self, dsts, sinces=None, wall: int | None = None):
        """``for d, t in zip(dsts, sinces): d.merge(self.recordMap(modifiedSince=t))``, ending at the first
        that raises."""
        wall = self._wall(wall)
        dsts = list(dsts)
        sinces = self._sinces_for(sinces, dsts, "broadcastTo", "destinations")
        if not self._table_route([self], dsts):
            for d, t in zip(dsts, sinces):
                d.last_sync, d.last_sync_winners = "object", None
                d.merge(self.recordMap(modifiedSince=t), wall=wall)
            return
        n = self._sync_rows(self, *dsts)
        try:
            for c in range(0, len(dsts), _capi.FANOUT_MAX):
                part = dsts[c:c + _capi.FANOUT_MAX]
                res, mask = self._table.fanout_tables([d._table for d in part], n,
                                                      [self._since_lt(t) for t in sinces[c:c + len(part)]], wall,
                                                      win_mask=any(d._wants_winners() for d in part))
                for j, d in enumerate(part):
                    d.last_sync = "table"                   # (a later destination is never reached after a raise)
                    if res[j]["n_stored"]:
                        d._took(self, n, mask if d._wants_winners() else None, j)
                    d._raise_for(res[j])
        finally:
            self._maybe_compact()

    # ------------------------------------------------------------ replica comparison (read-only)
    # diff() is DEFINED as the comparison of self.recordMap() with other.recordMap(): per key, a map is ahead
    # when it alone holds a record or its record's Hlc is greater (the win rule of crdt.dart:83-84), and the
    # key is a conflict when both hold one Hlc with values that differ (Record ==, record.dart:34-35).  Between
    # members of one group that keep no Hlc on the host it runs on the two device tables (crdt_diff_tables):
    # no Record is built and the flag bytes stay on the device.  None of these members emits a watch event,
    # moves a clock, touches last_sync, or interns or compacts anything.

    def diff(self, other: "MapCrdt", keys: bool = False) -> ReplicaDiff:
        """Where this map and ``other`` stand: ``ahead`` (this map holds the winning record), ``behind``,
        ``conflicts`` and ``converged``; ``keys=True`` adds the three key lists, in the group's key order."""
        if other._group is not self._group or self._hlc_override or other._hlc_override:
            self.last_diff = "object"
            return self._diff_objects(other, keys)
        self.last_diff = "table"
        n = len(self._keys)
        self._reserve()
        other._reserve()
        d, flags = self._table.diff_table(other._table, n, flags=keys)
        n_conf, conf_ids = d["n_conflict"], None
        if n_conf:
            # the tables compare values by handle, and equal values may sit under two handles (the same
            # record stored on both sides by putRecord or merge()): the definition compares the values
            if flags is None:
                d, flags = self._table.diff_table(other._table, n, flags=True)
            ids, _, _, va, _ = self._table.export_flagged(n, flags, _capi.DIFF_CONFLICT).columns()
            vb = other._table.export_flagged(n, flags, _capi.DIFF_CONFLICT).columns()[3]
            get = self._values.get
            real = np.fromiter((a != b and get(a) != get(b) for a, b in zip(va.tolist(), vb.tolist())), bool, len(ids))
            conf_ids, n_conf = ids[real], int(real.sum())
        if not keys:
            return ReplicaDiff(d["n_a_ahead"], d["n_b_ahead"], n_conf)
        names = self._keys.keys

        def listed(bit, count):
            if not count:
                return []
            return [names[i] for i in self._table.export_flagged(n, flags, bit).columns()[0].tolist()]

        return ReplicaDiff(d["n_a_ahead"], d["n_b_ahead"], n_conf, listed(_capi.DIFF_A_AHEAD, d["n_a_ahead"]),
                           listed(_capi.DIFF_B_AHEAD, d["n_b_ahead"]),
                           [names[i] for i in conf_ids.tolist()] if n_conf else [])

    def _diff_objects(self, other: "MapCrdt", keys: bool) -> ReplicaDiff:
        """The definition itself, on the two recordMap()s."""
        ra, rb = self.recordMap(), other.recordMap()
        order = list(ra) + [k for k in rb if k not in ra]
        if other._group is self._group:
            order.sort(key=self._keys.get)
        ahead, behind, conflicts = [], [], []
        for k in order:
            a, b = ra.get(k), rb.get(k)
            if b is None or (a is not None and a.hlc > b.hlc):
                ahead.append(k)
            elif a is None or b.hlc > a.hlc:
                behind.append(k)
            elif a.value != b.value:
                conflicts.append(k)
        if not keys:
            return ReplicaDiff(len(ahead), len(behind), len(conflicts))
        return ReplicaDiff(len(ahead), len(behind), len(conflicts), ahead, behind, conflicts)

    def convergedWith(self, other: "MapCrdt") -> bool:
        """Whether ``self.recordMap() == other.recordMap()`` under ``Record ==`` (``diff(other).converged``)."""
        return self.diff(other).converged

    # groupDiff() is DEFINED on the recordMap()s of maps = [self, *replicas] (de-duplicated by identity): per key
    # of their union, the holders are the maps whose record has the greatest Hlc, every other map (one without a
    # record included) is behind, and the key is a conflict iff two holders' values differ under !=.

    def groupDiff(self, replicas, keys: bool = False) -> GroupDiff:
        """Where this map and ``replicas`` stand as a group (``GroupDiff``); ``keys=True`` adds the key lists, in
        the group's key order.  Up to ``_capi.GROUP_MAX`` members of one group that keep no Hlc on the host are
        compared on the device tables in one pass (``crdt_diff_group``, ``last_diff == "table"``); anything else
        runs the definition on the ``recordMap()``s (``last_diff == "object"``)."""
        maps, table = self._members(replicas, _capi.GROUP_MAX, "be compared")
        if not table:
            self.last_diff = "object"
            return self._group_objects(maps, keys)
        self.last_diff = "table"
        n, k = len(self._keys), len(maps)
        for m in maps:
            m._reserve()
        others = [m._table for m in maps[1:]]
        d, behind, hold, conflict = self._table.diff_group(others, n, masks=keys)
        n_conf, conf_ids = d["n_conflict"], None
        if n_conf:
            # the tables compare values by handle, and equal values may sit under two handles: the definition
            # compares the values of the holders, whose bits the hold bytes of the conflict rows carry
            if conflict is None:
                d, behind, hold, conflict = self._table.diff_group(others, n, masks=True)
            ids = self._table.export_flagged(n, conflict, 1).columns()[0]
            vals = [m._table.export_flagged(n, conflict, 1).columns()[3].tolist() for m in maps]
            import torch
            held = hold[torch.from_numpy(ids.astype(np.int64)).to(hold.device)].cpu().tolist()
            get = self._values.get
            real = np.zeros(len(ids), bool)
            for r, h in enumerate(held):
                handles = {vals[j][r] for j in range(k) if (h >> j) & 1}
                real[r] = len(handles) > 1 and _any_two_differ([get(v) for v in handles])
            conf_ids, n_conf = ids[real], int(real.sum())
        if not keys:
            return GroupDiff(d["n_behind"][:k], d["n_sole"][:k], d["n_disputed"], n_conf)
        names = self._keys.keys
        behind_keys = [[names[i] for i in self._table.export_flagged(n, behind, 1 << j).columns()[0].tolist()]
                       if d["n_behind"][j] else [] for j in range(k)]
        return GroupDiff(d["n_behind"][:k], d["n_sole"][:k], d["n_disputed"], n_conf, behind_keys,
                         [names[i] for i in conf_ids.tolist()] if n_conf else [])

    def _group_objects(self, maps, keys: bool) -> GroupDiff:
        """The definition itself, on the maps' recordMap()s."""
        rms = [m.recordMap() for m in maps]
        order = list(dict.fromkeys(k for rm in rms for k in rm))
        if all(m._group is self._group for m in maps):
            order.sort(key=self._keys.get)
        k = len(maps)
        behind, sole, disputed, conflicts = [[] for _ in range(k)], [0] * k, 0, []
        for key in order:
            recs = [rm.get(key) for rm in rms]
            top = None
            for r in recs:
                if r is not None and (top is None or r.hlc > top):
                    top = r.hlc
            holders = [j for j, r in enumerate(recs) if r is not None and r.hlc == top]
            for j in range(k):
                if j not in holders:
                    behind[j].append(key)
            disputed += len(holders) < k
            if len(holders) == 1:
                sole[holders[0]] += 1
            if _any_two_differ([recs[j].value for j in holders]):
                conflicts.append(key)
        counts = [len(b) for b in behind]
        if not keys:
            return GroupDiff(counts, sole, disputed, len(conflicts))
        return GroupDiff(counts, sole, disputed, len(conflicts), behind, conflicts)

    def convergedAll(self, replicas) -> bool:
        """Whether every map of ``[self, *replicas]`` has the same ``recordMap()`` under ``Record ==``
        (``groupDiff(replicas).converged``)."""
        return self.groupDiff(replicas).converged

    def stateDigest(self, block_rows: int = 1 << 20) -> np.ndarray:
        """One uint64 word per ``block_rows`` key ids of what ``recordMap()`` holds under ``Record ==``
        (``DeviceTable.digest_rows(state=True)``).  Members of one group whose ``diff`` reports nothing on
        the device tables have equal words; values enter by their handle in the group's value store."""
        self._reserve()
        return self._table.digest_rows(len(self._keys), block_rows, state=True)
