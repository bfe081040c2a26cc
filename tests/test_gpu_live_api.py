"""MapCrdt.clear() and the live views map / keys / values on the device table, against the object-level oracle
(oracle/crdt_oracle.py, the restatement of crdt.dart:13-29 and 67-73) driven with the same puts, deletes and
merges.  Everything is exact."""
import pytest

from crdt_amd import ClockDriftException, Hlc, MapCrdt, Record
from oracle import crdt_oracle as O
from tests._cases import WALL

pytestmark = pytest.mark.gpu


class Pair:
    """A GPU MapCrdt and its oracle mirror, each with a watch on everything and one on ``watched``."""

    def __init__(self, node="n1", watched="k2", gpu=None):
        self.g = gpu if gpu is not None else MapCrdt(node, clock=lambda: WALL)
        self.o = O.MapCrdt(node)
        self.watched = watched
        self.w_all, self.w_key = self.g.watch(), self.g.watch(key=watched)

    def both(self, gpu_call, ora_call):
        e1 = e2 = None
        try:
            gpu_call()
        except Exception as ex:  # noqa: BLE001
            e1 = (type(ex).__name__, str(ex))
        try:
            ora_call()
        except Exception as ex:  # noqa: BLE001
            e2 = (type(ex).__name__, str(ex))
        assert e1 == e2, (e1, e2)
        return e1 and e1[0]

    def put_all(self, values, wall):
        return self.both(lambda: self.g.putAll(dict(values), wall=wall), lambda: self.o.put_all(dict(values), wall))

    def delete(self, key, wall):
        return self.both(lambda: self.g.delete(key, wall=wall), lambda: self.o.delete(key, wall))

    def merge(self, recs, wall):
        """An external changeset {key: (millis, counter, node, value)}."""
        cs_d = {k: Record(Hlc(ms, c, n), v, Hlc(0, 0, "ext")) for k, (ms, c, n, v) in recs.items()}
        cs_o = {k: O.Record(O.Hlc(ms, c, n), v, O.Hlc(0, 0, "ext")) for k, (ms, c, n, v) in recs.items()}
        return self.both(lambda: self.g.merge(cs_d, wall=wall), lambda: self.o.merge(cs_o, wall))

    def clear(self, wall):
        self.g.last_clear = None
        out = self.both(lambda: self.g.clear(wall=wall), lambda: self.o.clear(wall))
        assert self.g.last_clear == "table"
        return out

    def check(self, tag=None):
        g, o = self.g, self.o
        rm_d, rm_o = g.recordMap(), o.record_map()
        assert list(rm_d) == list(rm_o), tag
        for k, r in rm_o.items():
            d = rm_d[k]
            assert (d.hlc.logicalTime, d.hlc.nodeId, d.value, d.modified.logicalTime, d.modified.nodeId) == \
                (r.hlc.logical_time, r.hlc.node_id, r.value, r.modified.logical_time, r.modified.node_id), (tag, k)
        assert (g.canonicalTime.logicalTime, g.canonicalTime.nodeId) == \
            (o.canonical_time.logical_time, o.canonical_time.node_id), tag
        assert g.map == o.map and list(g.map.items()) == list(o.map.items()), tag
        assert g.keys == o.keys and g.values == o.values, tag
        assert g.length == o.length and g.isEmpty == o.is_empty, tag
        assert self.w_all.events == o.events, tag
        assert self.w_key.events == [e for e in o.events if e[0] == self.watched], tag


def filled() -> Pair:
    p = Pair()
    p.put_all({f"k{i}": i for i in range(6)}, WALL)
    p.delete("k1", WALL + 1)
    p.merge({"k2": (WALL + 2, 0, "n9", "remote"), "k7": (WALL + 2, 1, "n0", [1, 2]), "k8": (WALL + 2, 2, "n0", None)},
            WALL + 3)
    p.check("filled")
    return p


def test_clear_against_the_oracle(gpu_device):
    p = filled()
    c0 = p.g.canonicalTime.logicalTime
    assert p.clear(WALL + 10) is None
    p.check("cleared")
    assert p.g.isEmpty and p.g.map == {} and p.g.keys == [] and p.g.canonicalTime.logicalTime > c0
    assert p.w_all.events[-6:] == [(k, None) for k in ("k0", "k2", "k3", "k4", "k5", "k7")]
    p.put_all({"k3": "again", "new": 1}, WALL + 11)          # the cleared map goes on living
    p.check("after")
    assert p.g.map == {"k3": "again", "new": 1}
    assert p.clear(WALL + 12) is None
    p.check("cleared again")


def test_clear_without_a_watch_fetches_nothing(gpu_device):
    g, o = MapCrdt("n1", clock=lambda: WALL), O.MapCrdt("n1")
    for m, put in ((g, lambda v, w: g.putAll(v, wall=w)), (o, lambda v, w: o.put_all(v, w))):
        put({"a": 1, "b": 2, "c": 3}, WALL)
        put({"b": None}, WALL + 1)
    serial = getattr(g._table, "_export_serial", 0)
    g.clear(wall=WALL + 5)
    o.clear(WALL + 5)
    assert g.last_clear == "table" and getattr(g._table, "_export_serial", 0) == serial   # no export ran
    assert g.canonicalTime.logicalTime == o.canonical_time.logical_time and g.map == o.map == {}
    assert {k: (r.hlc.logicalTime, r.modified.logicalTime) for k, r in g.recordMap().items()} == \
        {k: (r.hlc.logical_time, r.modified.logical_time) for k, r in o.record_map().items()}


def test_clear_of_an_empty_map_and_of_only_tombstones(gpu_device):
    p = Pair()
    assert p.clear(WALL) is None
    p.check("empty")
    assert p.g.canonicalTime.logicalTime == 0 and p.w_all.events == []
    p.put_all({"x": 1, "y": 2}, WALL)
    p.put_all({"x": None, "y": None}, WALL + 1)
    c, n_events = p.g.canonicalTime.logicalTime, len(p.w_all.events)
    assert p.clear(WALL + 2) is None
    assert p.clear(WALL - 70000) is None                     # no live record: no Hlc.send, so no drift either
    p.check("only tombstones")
    assert p.g.canonicalTime.logicalTime == c and len(p.w_all.events) == n_events


def test_drift_raise_changes_nothing(gpu_device):
    p = filled()
    c, n_events = p.g.canonicalTime.logicalTime, len(p.w_all.events)
    assert p.clear(WALL - 60001) == "ClockDriftException"
    with pytest.raises(ClockDriftException):
        p.g.clear(wall=WALL - 60001)
    p.check("after the raise")
    assert p.g.canonicalTime.logicalTime == c and len(p.w_all.events) == n_events and p.g.length == 6


def test_clear_drops_the_overrides(gpu_device):
    p = filled()
    odd = Hlc(WALL + 4, 0x10005, "n5")                       # a counter above 0xFFFF: not (millis << 16) + counter
    assert not odd.is_canonical_form
    p.g.putRecord("k4", Record(odd, "odd", Hlc(WALL + 4, 0, "elsewhere")))
    p.o.put_record("k4", O.Record(O.Hlc(WALL + 4, 0x10005, "n5"), "odd", O.Hlc(WALL + 4, 0, "elsewhere")))
    r = p.g.getRecord("k4")
    assert (r.hlc.millis, r.hlc.counter, r.modified.nodeId) == (WALL + 4, 0x10005, "elsewhere")
    assert p.g._hlc_override and p.g._mod_override
    assert p.clear(WALL + 20) is None
    p.check("cleared")
    assert not p.g._hlc_override and not p.g._mod_override
    r, c = p.g.getRecord("k4"), p.g.canonicalTime
    assert r.value is None and r.hlc.nodeId == r.modified.nodeId == "n1"
    assert r.hlc.logicalTime == r.modified.logicalTime == c.logicalTime and r.hlc.is_canonical_form


def test_clear_in_a_replica_group(gpu_device):
    a = Pair("a")
    b = Pair("b", gpu=a.g.replica("b"))
    a.put_all({"shared": 1, "only_a": 2}, WALL)
    b.put_all({"shared": 10, "only_b": 20}, WALL + 1)        # (the group saw b's keys in this order too)
    assert b.clear(WALL + 2) is None
    b.check("b cleared")
    a.check("a untouched")
    assert not b.g.containsKey("only_a") and b.g.getRecord("only_a") is None
    assert b.w_all.events[-2:] == [("shared", None), ("only_b", None)]
    # a takes b's tombstones where they win
    rm = b.o.record_map()
    a.both(lambda: a.g.mergeFrom(b.g, wall=WALL + 3), lambda: a.o.merge({k: rm[k] for k in ("shared", "only_b")}, WALL + 3))
    a.check("a merged")
    assert a.g.last_sync == "table" and a.g.map == {"only_a": 2} and a.g.isDeleted("shared") and a.g.isDeleted("only_b")


def test_map_of_10000_keys_half_deleted(gpu_device):
    g, o = MapCrdt("n1", clock=lambda: WALL), O.MapCrdt("n1")
    values = {f"key{i}": (i if i % 3 else f"s{i}") for i in range(10000)}
    dead = {f"key{i}": None for i in range(0, 10000, 2)}
    g.putAll(dict(values), wall=WALL)
    o.put_all(dict(values), WALL)
    g.putAll(dict(dead), wall=WALL + 1)
    o.put_all(dict(dead), WALL + 1)
    m = g.map
    assert len(m) == 5000 and list(m.items()) == list(o.map.items())
    assert g.keys == o.keys and g.values == o.values and g.length == o.length == 5000
    g.clear(wall=WALL + 2)
    o.clear(WALL + 2)
    assert g.map == o.map == {} and g.canonicalTime.logicalTime == o.canonical_time.logical_time
    assert g.last_clear == "table"
