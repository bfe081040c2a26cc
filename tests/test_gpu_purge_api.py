"""MapCrdt.purgeDeleted on the device tables against its definition run on the object-level oracle's maps
(tests/_purge_cases.purge_definition over oracle/crdt_oracle.py MapCrdts, which delete from ``_map``), after the
same seeded histories of puts, deletes, syncs and clears.  Everything is exact.  A group iterates its keys in the
order the GROUP first saw them, the oracle's maps each in their own, so the contents are compared key by key."""
import json
import random

import pytest

from crdt_amd import Hlc, MapCrdt, Record, _capi
from oracle import crdt_oracle as O
from tests import _purge_cases as pc
from tests._cases import WALL

pytestmark = pytest.mark.gpu

KEYS = [f"k{i}" for i in range(12)]


class Net:
    """n GPU MapCrdts (one replica group unless ``grouped`` is False) and their oracle mirrors, all watched."""

    def __init__(self, n: int, grouped: bool = True):
        nodes = [f"n{j}" for j in range(n)]
        self.g = [MapCrdt(nodes[0], clock=lambda: WALL)]
        for node in nodes[1:]:
            self.g.append(self.g[0].replica(node) if grouped else MapCrdt(node, clock=lambda: WALL))
        self.o = [O.MapCrdt(node) for node in nodes]
        self.w = [g.watch() for g in self.g]
        self.wall = WALL

    def tick(self) -> int:
        self.wall += 1
        return self.wall

    def put(self, j, values: dict):
        w = self.tick()
        self.g[j].putAll(dict(values), wall=w)
        self.o[j].put_all(dict(values), w)

    def ordered(self, d: dict) -> dict:
        """In the order the GROUP first saw the keys, which is how a member iterates (a purged key that is
        stored again keeps its old place; the oracle's map appends it)."""
        ids = self.g[0]._keys
        return {k: d[k] for k in sorted(d, key=ids.get)}

    def clear(self, j):
        w = self.tick()
        self.g[j].clear(wall=w)
        self.o[j].put_all({k: None for k in self.ordered(self.o[j].map)}, w)     # crdt.dart:67-73

    def sync(self, i, j):
        """g[i].syncWith(g[j]): i takes j's records, then j takes i's."""
        w = self.tick()
        self.g[i].syncWith(self.g[j], wall=w)
        self.o[i].merge(self.ordered(self.o[j].record_map()), w)
        self.o[j].merge(self.ordered(self.o[i].record_map()), w)

    def converge(self):
        for j in range(1, len(self.g)):
            self.sync(0, j)
        for j in range(1, len(self.g)):
            self.sync(0, j)

    def history(self, rng: random.Random, steps: int):
        n = len(self.g)
        for _ in range(steps):
            j, op = rng.randrange(n), rng.random()
            if op < 0.40:
                self.put(j, {rng.choice(KEYS): rng.randrange(100) for _ in range(rng.randint(1, 3))})
            elif op < 0.70:
                self.put(j, {rng.choice(KEYS): None for _ in range(rng.randint(1, 3))})
            elif op < 0.95 and n > 1:
                i = rng.randrange(n - 1)
                self.sync(j, i if i < j else i + 1)
            elif op >= 0.95:
                self.clear(j)

    def purge(self, members, before_wall=None, route="table") -> int:
        """purgeDeleted on g[members[0]] with the others as replicas, and the definition on the oracles."""
        gs, os_ = [self.g[j] for j in members], [self.o[j] for j in members]
        before = None if before_wall is None else Hlc(before_wall, 0, "zz")
        canon = [g.canonicalTime.logicalTime for g in self.g]
        syncs = [g.last_sync for g in self.g]
        n_keys = len(self.g[0]._keys)
        want = pc.purge_definition(os_, None if before is None else before.logicalTime)
        serial = getattr(gs[0]._table, "_export_serial", 0)
        got = gs[0].purgeDeleted(before, gs[1:])
        self.exports = getattr(gs[0]._table, "_export_serial", 0) - serial    # exports the purge itself ran
        assert got == len(want) and gs[0].last_purge == route, (got, want, gs[0].last_purge)
        assert [g.canonicalTime.logicalTime for g in self.g] == canon and [g.last_sync for g in self.g] == syncs
        assert len(self.g[0]._keys) == n_keys                    # a purged key keeps its id; nothing is interned
        for k in want:
            for g in gs:
                assert not g.containsKey(k) and g.getRecord(k) is None and g.isDeleted(k) is None and g.get(k) is None
        self.check(("purge", members, before_wall))
        return got

    def check(self, tag=None):
        for j, (g, o, w) in enumerate(zip(self.g, self.o, self.w)):
            rm_g, rm_o = g.recordMap(), o.record_map()
            assert sorted(rm_g) == sorted(rm_o), (tag, j)
            for k, r in rm_o.items():
                d = rm_g[k]
                assert (d.hlc.logicalTime, d.hlc.nodeId, d.value, d.modified.logicalTime, d.modified.nodeId) == \
                    (r.hlc.logical_time, r.hlc.node_id, r.value, r.modified.logical_time, r.modified.node_id), (tag, j, k)
            assert g.map == o.map and g.length == o.length and g.isEmpty == o.is_empty, (tag, j)
            assert json.loads(g.toJson()) == json.loads(o.to_json()), (tag, j)
            assert (g.canonicalTime.logicalTime, g.canonicalTime.nodeId) == \
                (o.canonical_time.logical_time, o.canonical_time.node_id), (tag, j)
            assert w.events == o.events, (tag, j)
            for k in KEYS:
                assert g.containsKey(k) == o.contains_key(k), (tag, j, k)


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("n", [1, 2, 9])
def test_random_histories(gpu_device, n, seed):
    rng = random.Random(100 * n + seed)
    net = Net(n)
    net.history(rng, 30 + 10 * n)
    net.check("history")
    everyone = list(range(n))
    route = "table" if n <= _capi.PURGE_MAX else "object"        # more maps than one call takes: the definition
    net.purge(everyone, before_wall=(WALL + net.wall) // 2, route=route)      # unconverged: some are blocked
    net.put(0, {"k0": None, "k1": None})
    net.converge()
    net.check("converged")
    dead = [k for k, r in net.o[0].record_map().items() if r.is_deleted]
    bounded = net.purge(everyone, before_wall=(WALL + net.wall) // 2, route=route)
    rest = net.purge(everyone, route=route)                      # converged and unbounded: every deletion goes
    assert bounded + rest == len(dead) >= 2
    assert all(not r.is_deleted for o in net.o for r in o.record_map().values())
    assert net.purge(everyone, route=route) == 0
    if n > _capi.PURGE_MAX:                                      # a subset that one call takes runs on the tables
        net.put(0, {"k0": None, "k1": None})
        net.converge()
        assert net.purge(everyone[:_capi.PURGE_MAX], route="table") == 2     # the ninth map is not asked ...
        assert net.g[n - 1].isDeleted("k0") is True and net.purge([0, n - 1], route="table") == 0
        assert net.purge([n - 1], route="table") == 2                        # ... and keeps them until it collects
    net.history(rng, 20)                                         # the maps go on living: purged keys come back
    net.check("after")
    net.converge()
    net.check("converged again")


def test_purged_key_of_a_map_without_siblings(gpu_device):
    net = Net(1)
    g, o = net.g[0], net.o[0]
    net.put(0, {"a": 1, "b": 2, "c": 3})
    net.put(0, {"b": None})
    assert g.containsKey("b") and g.isDeleted("b") is True
    assert net.purge([0]) == 1
    assert not g.containsKey("b") and g.getRecord("b") is None and g.isDeleted("b") is None and g.get("b") is None
    assert g.containsKey("a") and g.get("a") == 1 and not g.containsKey("never seen")
    assert list(g.recordMap()) == ["a", "c"] and g.length == 2
    net.put(0, {"b": "again"})
    net.check("put again")
    assert g.containsKey("b") and g.get("b") == "again"
    assert list(g.map) == ["a", "b", "c"] and list(o.map) == ["a", "c", "b"]     # its old place: "first seen" order
    net.put(0, {"c": None})
    assert net.purge([0]) == 1 and g._purged
    g.purge()                                                    # purge(all) on an unshared map resets the check
    o.purge()
    assert not g._purged and not g.containsKey("a") and g.recordMap() == {}
    net.put(0, {"z": 1})
    assert g.containsKey("z") and list(g.recordMap()) == ["z"]


def test_a_replica_that_has_not_synced_the_deletion_blocks_it(gpu_device):
    net = Net(2)
    net.put(0, {"x": 1, "y": 2})
    net.sync(0, 1)
    net.put(0, {"x": None})                                      # only map 0 has seen the deletion
    assert net.purge([0, 1]) == 0
    assert net.g[0].isDeleted("x") is True and net.g[1].get("x") == 1
    assert net.purge([1, 0]) == 0
    net.sync(1, 0)
    assert net.g[1].isDeleted("x") is True
    assert net.purge([0, 1]) == 1
    assert all(not g.containsKey("x") and g.get("y") == 2 for g in net.g)
    net.put(1, {"y": None})
    assert net.purge([1]) == 1                                   # alone, map 1 collects what map 0 has not seen ...
    net.sync(0, 1)
    assert net.g[0].get("y") == 2 and net.g[1].get("y") == 2     # ... and is handed the older live record back
    net.check("handed back")


def test_a_mod_override_is_dropped_with_its_key(gpu_device):
    net = Net(2)
    net.put(0, {"x": 1, "y": 2})
    net.sync(0, 1)
    lt = net.g[0].canonicalTime.logicalTime + 5
    for g, o in zip(net.g, net.o):                               # one tombstone, its modified kept on the host
        g.putRecord("x", Record(Hlc.fromLogicalTime(lt, "n0"), None, Hlc(WALL, 0, "elsewhere")))
        o.put_record("x", O.Record(O.Hlc.from_logical_time(lt, "n0"), None, O.Hlc(WALL, 0, "elsewhere")))
        g.putRecord("y", Record(Hlc.fromLogicalTime(lt, "n0"), 7, Hlc(WALL, 0, "elsewhere")))
        o.put_record("y", O.Record(O.Hlc.from_logical_time(lt, "n0"), 7, O.Hlc(WALL, 0, "elsewhere")))
    assert all(len(g._mod_override) == 2 and not g._hlc_override for g in net.g)
    assert net.g[0].getRecord("x").modified.nodeId == "elsewhere"
    assert net.purge([0, 1]) == 1 and net.exports == 1           # the purged ids were fetched once
    kx, ky = net.g[0]._keys.get("x"), net.g[0]._keys.get("y")
    assert all(kx not in g._mod_override and ky in g._mod_override for g in net.g)
    net.put(1, {"x": "back"})
    net.check("back")
    assert net.g[1].getRecord("x").modified.nodeId == "n1"
    plain = Net(1)                                               # no override anywhere: no export runs
    plain.put(0, {"a": None})
    assert plain.purge([0]) == 1 and plain.exports == 0


def test_other_groups_and_host_kept_hlcs_take_the_object_route(gpu_device):
    net = Net(2, grouped=False)                                  # two maps, two id spaces
    net.put(0, {"x": 1, "y": 2, "z": 3})
    net.put(0, {"x": None, "z": None})
    w = net.tick()
    net.g[1].merge(net.g[0].recordMap(), wall=w)
    net.o[1].merge(dict(net.o[0].record_map()), w)
    net.put(1, {"z": None})                                      # map 1 deleted z again: another Hlc
    net.check("before")
    assert net.purge([0, 1], route="object") == 1
    assert all(not g.containsKey("x") and g.isDeleted("z") is True for g in net.g)
    assert net.purge([0], route="table") == 1 and net.purge([1], route="table") == 1
    grp = Net(2)                                                 # one group, an Hlc outside the canonical form
    grp.put(0, {"a": 1})
    grp.sync(0, 1)
    for g, o in zip(grp.g, grp.o):
        g.putRecord("odd", Record(Hlc(WALL + 4, 0x10005, "n5"), None, Hlc(WALL + 4, 0, g.nodeId)))
        o.put_record("odd", O.Record(O.Hlc(WALL + 4, 0x10005, "n5"), None, O.Hlc(WALL + 4, 0, o.node_id)))
    grp.put(0, {"a": None})
    grp.sync(0, 1)
    assert all(g._hlc_override for g in grp.g)
    assert grp.purge([0, 1], before_wall=WALL + 4, route="object") == 1      # a; odd's logical time is not below it
    assert all(g.isDeleted("odd") is True and g._hlc_override for g in grp.g)
    assert grp.purge([0, 1], route="object") == 1
    assert not any(g._hlc_override for g in grp.g)
    grp.put(0, {"a": None})
    assert grp.purge([0], route="table") == 1                    # no Hlc is kept on the host any more
