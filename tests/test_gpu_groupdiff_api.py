"""MapCrdt.groupDiff / convergedAll against their definition: per key of the union of the maps' recordMap()s the
holders are the maps whose record has the greatest Hlc, every other map is behind, and the key is a conflict iff
two holders' values differ, computed here from the maps.  The table route (up to GROUP_MAX members of one group)
and the object route (a member of another group, an Hlc kept on the host, nine maps) must both give it; none of
the calls may emit a watch event, move a clock, touch the sync bookkeeping or intern anything."""
import pytest

from crdt_amd import GroupDiff, Hlc, MapCrdt, Record, _capi
from tests._cases import WALL

pytestmark = pytest.mark.gpu


def definition(maps: list, order) -> tuple:
    """(behind key lists per map, sole counts, disputed, conflict keys), the keys in ``order``."""
    rms = [m.recordMap() for m in maps]
    behind, sole, disputed, conflicts = [[] for _ in maps], [0] * len(maps), 0, []
    for k in order:
        recs = [rm.get(k) for rm in rms]
        held = [r for r in recs if r is not None]
        if not held:
            continue
        top = held[0].hlc
        for r in held[1:]:
            if r.hlc.compareTo(top) > 0:
                top = r.hlc
        holders = [j for j, r in enumerate(recs) if r is not None and r.hlc.compareTo(top) == 0]
        for j in range(len(maps)):
            if j not in holders:
                behind[j].append(k)
        disputed += len(holders) < len(maps)
        if len(holders) == 1:
            sole[holders[0]] += 1
        if any(recs[x].value != recs[y].value for x in holders for y in holders):
            conflicts.append(k)
    return behind, sole, disputed, conflicts


def assert_group(maps: list, order, route: str, tag=None) -> GroupDiff:
    behind, sole, disputed, conflicts = definition(maps, order)
    first = maps[0]
    g = first.groupDiff(maps[1:], keys=True)
    assert isinstance(g, GroupDiff) and first.last_diff == route, tag
    if any(m._group is not first._group for m in maps):  # (no key order is shared: first seen over the maps)
        for ks in (*g.behind_keys, g.conflict_keys):
            ks.sort(key=order.index)
    assert (g.behind_keys, g.conflict_keys) == (behind, conflicts), tag
    assert (g.behind, g.sole, g.disputed, g.conflicts) == ([len(b) for b in behind], sole, disputed, len(conflicts)), tag
    assert g.converged is (disputed == 0 and not conflicts), tag
    c = first.groupDiff(maps[1:])                        # the counts alone: no key list is built
    assert (c.behind, c.sole, c.disputed, c.conflicts, c.behind_keys, c.conflict_keys) == \
        (g.behind, g.sole, g.disputed, g.conflicts, None, None), tag
    assert first.convergedAll(maps[1:]) is g.converged and first.last_diff == route, tag
    return g


def snapshot(maps, watches):
    return ([list(w.events) for w in watches], [m.canonicalTime for m in maps],
            [(m.last_sync, m.last_sync_winners) for m in maps], [(len(m._keys), len(m._values)) for m in maps])


def scenario(make_peers):
    """Four maps, the last one empty: puts on three, a hub sync, a conflict among the holders of a newer Hlc while
    the others are behind.  Returns what the group diffs reported, step by step (the routes must agree on it)."""
    a = MapCrdt("na", clock=lambda: WALL)
    b, c, d = make_peers(a)
    maps = [a, b, c, d]
    watches = [m.watch() for m in maps]
    a.putAll({f"k{i}": i for i in range(40)}, wall=WALL)
    b.putAll({f"k{i}": 100 + i for i in range(30, 70)}, wall=WALL + 1)
    b.delete("k35", wall=WALL + 2)
    c.putAll({f"k{i}": 200 + i for i in range(60, 90)}, wall=WALL + 3)
    c.put("k5", "late", wall=WALL + 4)
    order = [f"k{i}" for i in range(90)]
    route = "table" if all(m._group is a._group for m in maps) else "object"
    log = []

    def note(g):
        log.append((g.behind, g.sole, g.disputed, g.conflicts, g.behind_keys, g.conflict_keys))
        return g

    before = snapshot(maps, watches)
    g = note(assert_group(maps, order, route, "before"))
    assert all(g.behind) and g.behind[3] == g.disputed == 90 and g.sole[3] == 0 and all(g.sole[:3]) and not g.conflicts
    note(assert_group([c, a, b], order, route if c._group is a._group and b._group is a._group else "object", "three"))
    g = assert_group([b], order, "table", "alone")       # one map: it holds everything it sees, alone
    assert g.converged and g.behind == [0] and g.sole == [len(b.recordMap())]
    assert b.groupDiff([b, b]).sole == g.sole            # (de-duplicated by identity)
    assert snapshot(maps, watches) == before             # no event, clock, last_sync or intern change
    a.mergeFromAll([b, c], wall=WALL + 10)
    a.broadcastTo([b, c, d], wall=WALL + 11)
    g = note(assert_group(maps, order, route, "synced"))
    assert g.converged and g.behind == g.sole == [0] * 4 and a.convergedAll([b, c, d]) and d.convergedAll([a])
    # a newer Hlc on two members under two values, the other two behind: a conflict among the holders
    h = Hlc(WALL + 50, 0, "na")
    a.putRecord("k7", Record(h, "x", h))
    b.putRecord("k7", Record(h, "y", h))
    g = note(assert_group(maps, order, route, "conflict"))
    assert (g.behind, g.sole, g.disputed, g.conflict_keys) == ([0, 0, 1, 1], [0] * 4, 1, ["k7"])
    assert g.behind_keys == [[], [], ["k7"], ["k7"]] and not a.convergedAll([b])
    c.putRecord("k7", Record(h, "x", h))                 # three holders, the first and the last agree
    g = note(assert_group(maps, order, route, "three holders"))
    assert (g.behind, g.conflict_keys) == ([0, 0, 0, 1], ["k7"])
    g = note(assert_group([a, c, b, d], order, route, "the last holder differs"))
    assert (g.behind, g.conflict_keys) == ([0, 0, 0, 1], ["k7"])
    # a member above all of them overrules the conflict
    d.putRecord("k7", Record(Hlc(WALL + 60, 0, "nd"), "z", Hlc(WALL + 60, 0, "nd")))
    g = note(assert_group(maps, order, route, "overruled"))
    assert (g.behind, g.sole, g.conflicts) == ([1, 1, 1, 0], [0, 0, 0, 1], 0)
    # the same value stored again under a handle of its own is no conflict (the definition compares values)
    d.putRecord("k7", Record(h, "x", h))
    b.putRecord("k7", Record(h, "x", h))
    before = snapshot(maps, watches)
    g = note(assert_group(maps, order, route, "healed by hand"))
    assert g.converged and snapshot(maps, watches) == before
    return log, maps


def test_a_group_takes_the_table_route(gpu_device):
    log, maps = scenario(lambda first: (first.replica("nb"), first.replica("nc"), first.replica("nd")))
    assert maps[0].last_diff == "table" and len(log) == 8


def test_object_route_with_a_member_of_another_group_gives_the_same(gpu_device):
    table_log, _ = scenario(lambda first: (first.replica("nb"), first.replica("nc"), first.replica("nd")))
    object_log, maps = scenario(lambda first: (first.replica("nb"), MapCrdt("nc", clock=lambda: WALL), first.replica("nd")))
    assert maps[0].last_diff == "object" and maps[2]._group is not maps[0]._group
    assert object_log == table_log


def test_object_route_with_an_hlc_kept_on_the_host(gpu_device):
    a = MapCrdt("na", clock=lambda: WALL)
    b, c = a.replica("nb"), a.replica("nc")
    a.putAll({f"k{i}": i for i in range(20)}, wall=WALL)
    b.mergeFrom(a, wall=WALL + 1)
    b.putAll({"k3": "b's", "x": 1}, wall=WALL + 2)
    order = [f"k{i}" for i in range(20)] + ["x"]
    want = assert_group([a, b, c], order, "table", "canonical")
    assert (want.behind, want.sole) == ([2, 0, 21], [0, 2, 0])
    # a counter past 0xFFFF: the Hlc's millis is not lt >> 16, so the map keeps it on the host
    wide = Hlc(WALL + 1, 0x1FFFF, "zz")
    a.putRecord("k9", Record(wide, "wide", Hlc(WALL, 0, "na")))
    assert a._hlc_override
    clocks = [m.canonicalTime for m in (a, b, c)]
    g = assert_group([a, b, c], order, "object", "override")
    assert (g.behind, g.sole) == ([2, 1, 21], [1, 2, 0]) and g.behind_keys[1] == ["k9"]
    assert c.groupDiff([b, a]).behind == [21, 1, 2] and c.last_diff == "object"
    assert_group([b, c], order, "table", "the two without one")
    assert [m.canonicalTime for m in (a, b, c)] == clocks


def test_nine_maps_take_the_object_route(gpu_device):
    a = MapCrdt("n0", clock=lambda: WALL)
    maps = [a] + [a.replica(f"n{j}") for j in range(1, 9)]
    order = [f"k{i}" for i in range(12)]
    for j, m in enumerate(maps):
        m.putAll({f"k{i}": 10 * j + i for i in range(j, j + 4)}, wall=WALL + j)
    assert len(maps) == _capi.GROUP_MAX + 1
    nine = assert_group(maps, order, "object", "nine")
    eight = assert_group(maps[:8], order, "table", "eight")
    assert nine.sole == [1] * 8 + [4] and eight.sole == [1] * 7 + [4] and nine.disputed == eight.disputed + 1 == 12
    assert nine.behind[:7] == [b + 1 for b in eight.behind[:7]]


def test_a_purged_key_and_a_key_only_a_sibling_wrote_are_not_held(gpu_device):
    a = MapCrdt("na", clock=lambda: WALL)
    b, c = a.replica("nb"), a.replica("nc")
    a.putAll({"gone": 1, "kept": 2}, wall=WALL)
    a.delete("gone", wall=WALL + 1)
    a.broadcastTo([b, c], wall=WALL + 2)
    assert a.purgeDeleted(replicas=[b, c]) == 1 and a.last_purge == "table"
    b.put("only_b", 5, wall=WALL + 3)                    # a and c have its key id and no record
    order = ["gone", "kept", "only_b"]
    g = assert_group([a, b, c], order, "table", "purged")
    assert g.behind_keys == [["only_b"], [], ["only_b"]] and (g.sole, g.disputed, g.conflicts) == ([0, 1, 0], 1, 0)
    g = assert_group([a, c], order, "table", "nobody holds either")
    assert g.converged and g.behind == [0, 0]
    c.put("gone", "back", wall=WALL + 4)                 # stored again at its old place in the key order
    g = assert_group([a, b, c], order, "table", "stored again")
    assert g.behind_keys == [["gone", "only_b"], ["gone"], ["only_b"]] and g.sole == [0, 1, 1]


def test_replicas_of_different_devices_are_refused(gpu_device):
    a = MapCrdt("na", clock=lambda: WALL)
    b = a.replica("nb")
    a.put("k", 1, wall=WALL)
    b._table.device = 1                                  # (as if it had been created on another GPU)
    try:
        with pytest.raises(ValueError):
            a.groupDiff([b])
        with pytest.raises(ValueError):
            a.convergedAll([b])
    finally:
        b._table.device = 0
    assert not a.convergedAll([b]) and a.groupDiff([b]).sole == [1, 0]
