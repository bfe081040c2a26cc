"""MapCrdt.diff / convergedWith / stateDigest against their definition: the comparison of the two recordMap()s
under the win rule of crdt.dart:83-84 and Record == (record.dart:34-35), computed here from the maps.  The
table route (members of one group) and the object route (other groups, an Hlc kept on the host) must both
give it; none of the calls may emit a watch event or move a clock."""
import numpy as np
import pytest

from crdt_amd import Hlc, MapCrdt, Record
from tests._cases import WALL

pytestmark = pytest.mark.gpu


def definition(a: MapCrdt, b: MapCrdt, order) -> tuple:
    """(ahead, behind, conflicts) key lists of a against b, in ``order``."""
    ra, rb = a.recordMap(), b.recordMap()
    ahead, behind, conflicts = [], [], []
    for k in order:
        x, y = ra.get(k), rb.get(k)
        if x is None and y is None:
            continue
        if y is None or (x is not None and x.hlc.compareTo(y.hlc) > 0):
            ahead.append(k)
        elif x is None or y.hlc.compareTo(x.hlc) > 0:
            behind.append(k)
        elif x.value != y.value:
            conflicts.append(k)
    return ahead, behind, conflicts


def assert_diff(a: MapCrdt, b: MapCrdt, order, route: str, tag=None):
    ahead, behind, conflicts = definition(a, b, order)
    d = a.diff(b, keys=True)
    assert a.last_diff == route, tag
    if a._group is not b._group:                         # (no key order is shared: each map's own, then the other's)
        for ks in (d.ahead_keys, d.behind_keys, d.conflict_keys):
            ks.sort(key=order.index)
    assert (d.ahead_keys, d.behind_keys, d.conflict_keys) == (ahead, behind, conflicts), tag
    assert (d.ahead, d.behind, d.conflicts) == (len(ahead), len(behind), len(conflicts)), tag
    assert d.converged is (not (ahead or behind or conflicts)), tag
    c = a.diff(b)                                        # the counts alone: no key list is built
    assert (c.ahead, c.behind, c.conflicts, c.ahead_keys, c.behind_keys, c.conflict_keys) == \
        (d.ahead, d.behind, d.conflicts, None, None, None), tag
    assert a.convergedWith(b) is d.converged, tag
    r = b.diff(a, keys=True)                             # seen from the other side
    assert [sorted(ks, key=order.index) for ks in (r.ahead_keys, r.behind_keys, r.conflict_keys)] == \
        [behind, ahead, conflicts], tag
    return d


def scenario(make_peers):
    """Three members with puts on each, a sync, a planted conflict; ``make_peers(first)`` builds the other two.
    Returns what the diffs reported, step by step (the routes must agree on it)."""
    a = MapCrdt("na", clock=lambda: WALL)
    b, c = make_peers(a)
    maps = (a, b, c)
    watches = [m.watch() for m in maps]
    a.putAll({f"k{i}": i for i in range(40)}, wall=WALL)
    b.putAll({f"k{i}": 100 + i for i in range(30, 70)}, wall=WALL + 1)
    b.delete("k35", wall=WALL + 2)
    c.putAll({f"k{i}": 200 + i for i in range(60, 90)}, wall=WALL + 3)
    c.put("k5", "late", wall=WALL + 4)
    order = [f"k{i}" for i in range(90)]
    events = [list(w.events) for w in watches]
    clocks = [m.canonicalTime for m in maps]
    syncs = [(m.last_sync, m.last_sync_winners) for m in maps]
    route = "table" if b._group is a._group else "object"
    log = []
    for x, y in ((a, b), (a, c), (b, c)):
        d = assert_diff(x, y, order, route, "before")
        assert d.ahead and d.behind and not d.conflicts
        log.append((d.ahead_keys, d.behind_keys, d.conflict_keys))
    digests = [m.stateDigest(2048) for m in maps]
    assert all(len(g) == 1 and g.dtype == np.uint64 for g in digests)
    if route == "table":
        assert len({int(g[0]) for g in digests}) == 3
    # none of that emitted an event, moved a clock or touched the sync bookkeeping
    assert [list(w.events) for w in watches] == events
    assert [m.canonicalTime for m in maps] == clocks
    assert [(m.last_sync, m.last_sync_winners) for m in maps] == syncs
    a.syncWith(b, wall=WALL + 10)
    d = assert_diff(a, b, order, route, "synced")
    assert d.converged and a.convergedWith(b) and b.convergedWith(a)
    if route == "table":
        assert np.array_equal(a.stateDigest(2048), b.stateDigest(2048))
        assert not np.array_equal(a.stateDigest(2048), c.stateDigest(2048))
    assert not a.convergedWith(c)
    # a conflict: the same Hlc under another value, stored verbatim on one side only
    r = a.getRecord("k7")
    b.putRecord("k7", Record(r.hlc, "other", r.modified))
    d = assert_diff(a, b, order, route, "conflict")
    assert (d.ahead, d.behind, d.conflict_keys) == (0, 0, ["k7"]) and not a.convergedWith(b)
    log.append((d.ahead_keys, d.behind_keys, d.conflict_keys))
    a.syncWith(b, wall=WALL + 20)                        # no merge heals it: equal keeps local on both sides
    d = assert_diff(a, b, order, route, "conflict after a sync")
    assert d.conflict_keys == ["k7"] and (a.get("k7"), b.get("k7")) == (7, "other")
    # the same record stored again under a handle of its own is no conflict (Record == compares values)
    b.putRecord("k7", Record(r.hlc, 7, r.modified))
    assert assert_diff(a, b, order, route, "healed by hand").converged
    clocks = [m.canonicalTime for m in maps]
    events = [list(w.events) for w in watches]
    for x, y in ((a, c), (c, b)):
        d = assert_diff(x, y, order, route, "after")
        log.append((d.ahead_keys, d.behind_keys, d.conflict_keys))
    assert [m.canonicalTime for m in maps] == clocks and [list(w.events) for w in watches] == events
    return log, maps


def test_three_member_group_takes_the_table_route(gpu_device):
    log, (a, b, c) = scenario(lambda first: (first.replica("nb"), first.replica("nc")))
    assert a.last_diff == b.last_diff == c.last_diff == "table"
    assert a.diff(a).converged and a.last_diff == "table"
    # a member that has stored nothing is behind on every key the others hold
    d = a.replica("nd")
    got = d.diff(a, keys=True)
    assert d.last_diff == "table" and (got.ahead, got.conflicts) == (0, 0) and got.behind == len(a.recordMap())
    assert got.behind_keys == list(a.recordMap())


def test_object_route_between_groups_gives_the_same(gpu_device):
    table_log, _ = scenario(lambda first: (first.replica("nb"), first.replica("nc")))
    object_log, (a, b, c) = scenario(lambda first: (MapCrdt("nb", clock=lambda: WALL), MapCrdt("nc", clock=lambda: WALL)))
    assert a.last_diff == b.last_diff == c.last_diff == "object"
    assert object_log == table_log


def test_object_route_with_an_hlc_kept_on_the_host(gpu_device):
    a = MapCrdt("na", clock=lambda: WALL)
    b = a.replica("nb")
    a.putAll({f"k{i}": i for i in range(20)}, wall=WALL)
    b.mergeFrom(a, wall=WALL + 1)
    b.putAll({"k3": "b's", "x": 1}, wall=WALL + 2)
    order = [f"k{i}" for i in range(20)] + ["x"]
    want = assert_diff(a, b, order, "table", "canonical")
    assert (want.ahead_keys, want.behind_keys, want.conflict_keys) == ([], ["k3", "x"], [])
    # a counter past 0xFFFF: the Hlc's millis is not lt >> 16, so the map keeps it on the host
    wide = Hlc(WALL + 1, 0x1FFFF, "zz")
    a.putRecord("k9", Record(wide, "wide", Hlc(WALL, 0, "na")))
    assert a._hlc_override
    clocks = a.canonicalTime, b.canonicalTime
    d = assert_diff(a, b, order, "object", "override")
    assert (d.ahead_keys, d.behind_keys, d.conflict_keys) == (["k9"], ["k3", "x"], [])
    assert b.diff(a).behind == 1 and b.last_diff == "object"
    b.putRecord("k9", Record(wide, "wide", Hlc(WALL, 0, "nb")))
    d = assert_diff(a, b, order, "object", "override on both")
    assert (d.ahead_keys, d.behind_keys) == ([], ["k3", "x"])
    assert (a.canonicalTime, b.canonicalTime) == clocks
