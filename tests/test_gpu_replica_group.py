"""Replica groups (MapCrdt.replica) and the MapCrdt-level syncs mergeFrom / syncWith / mergeFromAll /
broadcastTo against the object-level oracle: every GPU replica is mirrored by one oracle MapCrdt, driven through
the members' DEFINING compositions of merge() and recordMap() with the same wall.  A group iterates its keys in
the order the group first saw them, so the oracle's changesets are handed over in that order (the reference's
own order is each map's insertion order, which replicas with stores of their own need not share).  After every
step every replica's recordMap (hlc, value, modified with node ids), canonicalTime, length, map and watch
events are compared.  Everything is exact."""
import numpy as np
import pytest

from crdt_amd import Hlc, MapCrdt, Record, _capi
from oracle import crdt_oracle as O
from tests._cases import WALL
from tests.test_gpu_api import _random_ops_vs_oracle

pytestmark = pytest.mark.gpu

T = _capi.TABLE_TILE


def o_hlc(h):
    return None if h is None else O.Hlc.from_logical_time(h.logicalTime, h.nodeId)


class Net:
    """GPU replicas of one group and their oracle mirrors."""

    def __init__(self, node_ids, watched=None, capacity=None):
        first = MapCrdt(node_ids[0], clock=lambda: WALL)
        self.gpu = [first] + [first.replica(n, capacity=capacity) for n in node_ids[1:]]
        self.ora = [O.MapCrdt(n) for n in node_ids]
        watched = range(len(node_ids)) if watched is None else watched
        self.watch = {i: self.gpu[i].watch() for i in watched}

    # ---- the compositions on the oracle
    def ordered(self, record_map: dict) -> dict:
        ids = self.gpu[0]._keys
        return {k: record_map[k] for k in sorted(record_map, key=ids.get)}

    def o_merge_from(self, dst, src, since, wall):
        self.ora[dst].merge(self.ordered(self.ora[src].record_map(o_hlc(since))), wall)

    def both(self, gpu_call, ora_call):
        """Run the GPU member and the oracle composition; the exceptions must agree.  Returns its name."""
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

    def merge_from(self, dst, src, since=None, wall=WALL):
        return self.both(lambda: self.gpu[dst].mergeFrom(self.gpu[src], modifiedSince=since, wall=wall),
                         lambda: self.o_merge_from(dst, src, since, wall))

    def sync_with(self, a, b, since_self=None, since_other=None, wall=WALL):
        def ora():
            self.o_merge_from(a, b, since_other, wall)
            self.o_merge_from(b, a, since_self, wall)
        return self.both(lambda: self.gpu[a].syncWith(self.gpu[b], sinceSelf=since_self, sinceOther=since_other,
                                                      wall=wall), ora)

    def merge_from_all(self, hub, srcs, sinces, wall=WALL):
        def ora():
            for s, t in zip(srcs, sinces):
                self.o_merge_from(hub, s, t, wall)
        return self.both(lambda: self.gpu[hub].mergeFromAll([self.gpu[s] for s in srcs], sinces, wall=wall), ora)

    def broadcast_to(self, hub, dsts, sinces, wall=WALL):
        def ora():
            for d, t in zip(dsts, sinces):
                self.o_merge_from(d, hub, t, wall)
        return self.both(lambda: self.gpu[hub].broadcastTo([self.gpu[d] for d in dsts], sinces, wall=wall), ora)

    def put_all(self, i, values, wall):
        return self.both(lambda: self.gpu[i].putAll(dict(values), wall=wall),
                         lambda: self.ora[i].put_all(dict(values), wall))

    def merge(self, i, recs, wall):
        """An external changeset {key: (millis, counter, node, value)}."""
        cs_d = {k: Record(Hlc(ms, c, n), v, Hlc(0, 0, "ext")) for k, (ms, c, n, v) in recs.items()}
        cs_o = {k: O.Record(O.Hlc(ms, c, n), v, O.Hlc(0, 0, "ext")) for k, (ms, c, n, v) in recs.items()}
        return self.both(lambda: self.gpu[i].merge(cs_d, wall=wall), lambda: self.ora[i].merge(cs_o, wall))

    # ---- the comparison
    def check(self, tag=None):
        for i, (g, o) in enumerate(zip(self.gpu, self.ora)):
            rm_d, rm_o = g.recordMap(), o.record_map()
            assert set(rm_d) == set(rm_o), (tag, i)
            for k, r in rm_o.items():
                d = rm_d[k]
                assert (d.hlc.logicalTime, d.hlc.nodeId, d.value, d.modified.logicalTime, d.modified.nodeId) == \
                    (r.hlc.logical_time, r.hlc.node_id, r.value, r.modified.logical_time, r.modified.node_id), (tag, i, k)
            assert g.canonicalTime.logicalTime == o.canonical_time.logical_time, (tag, i)
            assert g.canonicalTime.nodeId == o.canonical_time.node_id, (tag, i)
            assert g.length == o.length and g.map == o.map, (tag, i)
            if i in self.watch:
                assert self.watch[i].events == o.events, (tag, i)


# ------------------------------------------------------------------ 1. the reference's delta sync group
@pytest.mark.parametrize("order", ["in", "reverse"])
def test_delta_sync_group(gpu_device, order):
    """map_crdt_test.dart's 'Delta sync' group: _sync(local, remote) is t = local.canonicalTime;
    remote.merge(local.recordMap()); local.merge(remote.recordMap(modifiedSince: t))."""
    net = Net(["a", "b", "c"])
    a, b, c = 0, 1, 2

    def sync(local, remote, wall):
        t = net.gpu[local].canonicalTime
        assert net.sync_with(remote, local, since_self=t, wall=wall) is None
        net.check((order, local, remote))

    net.put_all(a, {"x": 1}, WALL)
    net.put_all(b, {"x": 2}, WALL + 100)
    net.check("puts")
    if order == "in":
        sync(a, c, WALL + 200)
        sync(b, c, WALL + 200)
        assert [net.gpu[i].get("x") for i in (a, b, c)] == [1, 2, 2]
    else:
        sync(b, c, WALL + 200)
        sync(a, c, WALL + 200)
        sync(b, c, WALL + 200)
        assert [net.gpu[i].get("x") for i in (a, b, c)] == [2, 2, 2]
    assert all(g.last_sync == "table" for g in net.gpu)


# ------------------------------------------------------------------ 2. random schedules
def _pick_since(net, rng, src, other, wall0, wall):
    kind = int(rng.integers(0, 4))
    if kind == 0:
        return None
    if kind == 1:
        return Hlc((wall0 + wall) // 2, 0, "s")
    if kind == 2:
        return net.gpu[src].canonicalTime                          # the latest
    return net.gpu[other].canonicalTime                            # a sibling's canonical


@pytest.mark.parametrize("seed", range(4))
def test_random_schedules(gpu_device, seed):
    rng = np.random.default_rng(8800 + seed)
    n_members = 3 + seed % 2
    nodes = ["n2", "n5", "n7", "n9"][:n_members]
    net = Net(nodes, watched=range(0, n_members, 2), capacity=64 if seed % 2 else None)
    wall = WALL
    n_keys = T + 300 if seed < 3 else 2 * T + 40                   # more than one tile of keys (at most 3)
    key = lambda i: f"k{i}"  # noqa: E731
    net.put_all(0, {key(i): i for i in range(n_keys)}, wall)       # one member holds every key
    net.check("fill")
    ext_nodes = ["x1", "n6", "zz", "!first"]
    peers_cycle = [1, 3, 9]
    for step in range(40):
        wall += int(rng.integers(0, 3))
        op = int(rng.integers(0, 10))
        i = int(rng.integers(0, n_members))
        others = [m for m in range(n_members) if m != i]
        j = int(rng.choice(others))
        small = lambda n: [key(int(k)) for k in rng.choice(n_keys + 50, n, replace=False)]  # noqa: E731
        if op == 0:
            what = ("put", net.put_all(i, {small(1)[0]: int(rng.integers(0, 1000))}, wall))
        elif op == 1:
            what = ("putAll", net.put_all(i, {k: int(rng.integers(0, 1000)) for k in small(int(rng.integers(1, 40)))}, wall))
        elif op == 2:
            what = ("delete", net.put_all(i, {small(1)[0]: None}, wall))
        elif op == 3 and step % 3 == 0:
            what = ("clear", net.both(lambda: net.gpu[i].clear(wall=wall), lambda: net.ora[i].clear(wall)))
        elif op in (3, 4):
            what = ("mergeFrom", net.merge_from(i, j, _pick_since(net, rng, j, i, WALL, wall), wall))
        elif op == 5:
            what = ("syncWith", net.sync_with(i, j, _pick_since(net, rng, i, j, WALL, wall),
                                              _pick_since(net, rng, j, i, WALL, wall), wall))
        elif op in (6, 7):
            n_peers = peers_cycle[step % 3]
            peers = [int(p) for p in rng.choice(others, n_peers)]
            sinces = [_pick_since(net, rng, p if op == 6 else i, i if op == 6 else p, WALL, wall) for p in peers]
            if op == 6:
                what = ("mergeFromAll", n_peers, net.merge_from_all(i, peers, sinces, wall))
            else:
                what = ("broadcastTo", n_peers, net.broadcast_to(i, peers, sinces, wall))
        else:
            node = ext_nodes[int(rng.integers(0, len(ext_nodes)))]
            recs = {k: (wall + int(rng.integers(-40, 3)), int(rng.integers(0, 3)), node,
                        None if rng.random() < 0.2 else int(rng.integers(0, 1000))) for k in small(int(rng.integers(1, 30)))}
            what = ("merge", net.merge(i, recs, wall))
        net.check((seed, step, what))
    # the chunked forms ran on the tables
    assert any(g.last_sync == "table" for g in net.gpu)


def test_hub_forms_with_1_3_and_9_peers(gpu_device):
    """Lists longer than eight run in consecutive chunks; a peer may appear more than once."""
    net = Net(["h", "p1", "p2", "p3"])
    wall = WALL
    for i in range(4):
        wall += 1
        net.put_all(i, {f"k{i}_{x}": x for x in range(T // 2 + 7)}, wall)
        net.put_all(i, {"shared": i}, wall)
    for n_peers in (1, 3, 9):
        wall += 1
        peers = [1 + x % 3 for x in range(n_peers)]
        before = len(net.watch[0].events)
        assert net.merge_from_all(0, peers, [None] * n_peers, wall) is None
        net.check(("fan-in", n_peers))
        assert net.gpu[0].last_sync == "table" and net.gpu[0]._table.last_plan()["table"]
        assert net.gpu[0].last_sync_winners == len(net.watch[0].events) - before
        wall += 1
        net.put_all(0, {f"hub{n_peers}": n_peers, "shared": 10 + n_peers}, wall)
        assert net.broadcast_to(0, peers, [None] * n_peers, wall) is None
        net.check(("fan-out", n_peers))
        assert all(net.gpu[p].last_sync == "table" for p in set(peers))


# ------------------------------------------------------------------ 3. routes and what they fetch
def test_plain_merge_from_runs_on_the_tables_and_fetches_nothing(gpu_device):
    net = Net(["a", "b", "c"], watched=[2])
    net.put_all(0, {f"k{i}": i for i in range(T + 9)}, WALL)
    net.put_all(0, {"k3": None}, WALL + 1)
    assert net.merge_from(1, 0, wall=WALL + 2) is None
    b = net.gpu[1]
    assert b.last_sync == "table" and b._table.last_plan()["table"]
    assert b.last_sync_winners is None                              # no watch, no override: no export ran
    net.check("no watch")
    n_events = len(net.ora[2].events)
    assert net.merge_from(2, 0, wall=WALL + 3) is None              # c has a watch: the winners are fetched
    c = net.gpu[2]
    stored = len(net.ora[2].events) - n_events
    assert c.last_sync == "table" and c.last_sync_winners == stored == T + 9
    net.check("watch")
    assert net.merge_from(2, 0, wall=WALL + 4) is None              # again: every record ties, nothing stored
    assert c.last_sync_winners == 0
    net.check("ties")
    # an override on the storing replica is dropped by a winner: the export runs without a watch
    assert net.merge(1, {"k5": (WALL + 3, 0x1FFFF, "zz", "wide")}, WALL + 5) is None
    assert net.gpu[1]._hlc_override
    net.put_all(0, {"k5": "newer"}, WALL + 20000)
    assert net.merge_from(1, 0, net.gpu[0].canonicalTime, wall=WALL + 20000) is None
    assert b.last_sync == "table" and b.last_sync_winners == 1 and not b._hlc_override
    net.check("override dropped")


def test_source_with_a_wide_counter_takes_the_object_route(gpu_device):
    net = Net(["a", "b"])
    net.put_all(0, {f"k{i}": i for i in range(50)}, WALL)
    assert net.merge(0, {"k7": (WALL + 1, 0x1FFFF, "zz", "wide"), "new": (WALL + 1, 0x10002, "zz", 5)}, WALL + 10) is None
    assert net.gpu[0]._hlc_override
    assert net.merge_from(1, 0, wall=WALL + 11) is None
    assert net.gpu[1].last_sync == "object" and net.gpu[1].last_sync_winners is None
    net.check("object route")
    assert net.gpu[1].getRecord("k7").hlc.counter == 0x1FFFF
    assert net.sync_with(1, 0, wall=WALL + 12) is None
    assert net.gpu[0].last_sync == "object"
    net.check("object sync")
    # replicas of different groups: the object route too
    lone, olone = MapCrdt("lone", clock=lambda: WALL), O.MapCrdt("lone")
    lone.mergeFrom(net.gpu[1], wall=WALL + 13)
    olone.merge(net.ora[1].record_map(), WALL + 13)
    assert lone.last_sync == "object" and lone.map == olone.map
    assert lone.canonicalTime.logicalTime == olone.canonical_time.logical_time


# ------------------------------------------------------------------ 4. exceptions
def test_duplicate_node_between_members(gpu_device):
    net = Net(["a", "a", "c", "d"])                                 # two members with one node id
    net.put_all(0, {"x": 1, "y": 2}, WALL + 5)
    net.put_all(2, {"z": 3}, WALL)
    assert net.merge_from(1, 0, wall=WALL) == "DuplicateNodeException"
    net.check("mergeFrom")
    # the second half of a syncWith is not run: a's canonical does not move
    c0 = net.gpu[0].canonicalTime.logicalTime
    assert net.sync_with(1, 0, wall=WALL + 6) == "DuplicateNodeException"
    assert net.gpu[0].canonicalTime.logicalTime == c0
    net.check("syncWith")
    # later hub steps are not run
    c2 = net.gpu[2].canonicalTime.logicalTime
    assert net.broadcast_to(0, [2, 1, 2], [None, None, None], WALL + 7) == "DuplicateNodeException"
    assert net.gpu[2].canonicalTime.logicalTime == (WALL + 7) << 16 != c2      # the first step ran, once
    net.check("broadcastTo")
    net.put_all(3, {"w": 4}, WALL + 8)                              # (d holds no record of node "a")
    net.put_all(0, {"x": 5}, WALL + 20)                             # above what b's clock reaches in step 0
    assert net.merge_from_all(1, [3, 0, 3], [None, None, None], WALL + 9) == "DuplicateNodeException"
    assert net.gpu[1].get("w") == 4 and net.gpu[1].get("x") is None
    net.check("mergeFromAll")


def test_clock_drift_from_a_far_ahead_put(gpu_device):
    net = Net(["a", "b", "c"])
    net.put_all(0, {"x": 1}, WALL + 100_000)                        # far ahead of the others' wall
    net.put_all(1, {"y": 2}, WALL)
    assert net.merge_from(2, 0, wall=WALL + 1) == "ClockDriftException"
    net.check("mergeFrom")
    assert net.sync_with(2, 0, wall=WALL + 2) == "ClockDriftException"
    net.check("syncWith")
    assert net.merge_from_all(2, [1, 0, 1], [None] * 3, WALL + 3) == "ClockDriftException"
    assert net.gpu[2].get("y") == 2 and net.gpu[2].get("x") is None
    net.check("mergeFromAll")
    assert net.broadcast_to(0, [1, 2], [None, None], WALL + 4) == "ClockDriftException"
    assert net.gpu[2].get("x") is None
    net.check("broadcastTo")


# ------------------------------------------------------------------ 5. the shared id space
def test_node_id_that_sorts_before_all_others(gpu_device):
    net = Net(["m", "p", "t"])
    for i in range(3):
        net.put_all(i, {f"k{i}_{x}": x for x in range(40)}, WALL + i)
    net.merge_from(0, 1, wall=WALL + 3)
    net.merge_from(2, 0, wall=WALL + 4)
    net.check("before")
    ranks = {n: net.gpu[0]._nodes.rank(n) for n in ("m", "p", "t")}
    assert net.merge(1, {"k1_0": (WALL + 5, 0, "!first", "early"), "fresh": (WALL + 5, 1, "!first", 1)}, WALL + 6) is None
    assert net.gpu[0]._nodes.rank("!first") == 0
    assert {n: net.gpu[0]._nodes.rank(n) for n in ranks} == {n: r + 1 for n, r in ranks.items()}
    assert [g._table.local_rank for g in net.gpu] == [1, 2, 3]
    net.check("ranks moved")                                        # every member's records name the right nodes
    assert net.sync_with(0, 1, wall=WALL + 7) is None
    assert net.merge_from_all(2, [0, 1], [None, None], WALL + 8) is None
    net.check("after")
    assert net.gpu[2].getRecord("fresh").hlc.nodeId == "!first"


def test_a_key_of_one_member_only_and_purge(gpu_device):
    net = Net(["a", "b", "c"])
    net.put_all(0, {"mine": 1, "both": 2}, WALL)
    net.put_all(1, {"both": 3}, WALL + 1)
    a, b, c = net.gpu
    assert a.containsKey("mine") and not b.containsKey("mine") and not c.containsKey("mine")
    assert b.getRecord("mine") is None and b.get("mine") is None and b.isDeleted("mine") is None
    assert (a.length, b.length, c.length) == (2, 1, 0) and not b.containsKey("nobody's")
    net.check("one member")
    net.merge_from(2, 0, wall=WALL + 2)
    net.merge_from(1, 0, wall=WALL + 3)
    net.check("merged")
    b.purge()
    net.ora[1].purge()
    assert b.length == 0 and not b.containsKey("both") and b.getRecord("mine") is None
    assert a.get("mine") == 1 and c.get("mine") == 1 and c.get("both") == 2     # siblings intact, values too
    net.check("purged")
    net.put_all(1, {"again": 5}, WALL + 4)
    net.merge_from(1, 2, wall=WALL + 5)
    net.check("after purge")


def test_value_handles_survive_a_compaction(gpu_device):
    """Over 2 x 4096 handles churned through one member: the compaction takes the live set from every
    member's table, so a sibling's values (shared handles and its own) survive."""
    net = Net(["a", "b"], watched=[])
    net.put_all(0, {f"k{i}": f"a{i}" for i in range(100)}, WALL)
    net.put_all(1, {f"own{i}": f"b{i}" for i in range(50)}, WALL)
    net.merge_from(1, 0, wall=WALL + 1)                             # b now holds a's handles
    values = net.gpu[0]._values
    sizes = [len(values)]
    for r in range(90):                                             # 9000 handles, of which 100 stay live in a
        net.put_all(0, {f"k{i}": f"r{r}_{i}" for i in range(100)}, WALL + 2 + r)
        sizes.append(len(values))
    drops = [x for x in range(1, len(sizes)) if sizes[x] < sizes[x - 1]]
    assert len(drops) == 1 and sizes[drops[0] - 1] + 100 > 2 * 4096        # one compaction, at the threshold
    assert sizes[drops[0]] == 100 + 100 + 50                        # a's live rows, and b's: shared and own
    net.check("after the churn")
    assert net.gpu[1].get("k7") == "a7" and net.gpu[1].get("own7") == "b7"
    net.merge_from(1, 0, wall=WALL + 200)
    net.check("merged")


def test_a_small_member_syncs_from_a_large_sibling(gpu_device):
    net = Net(["a", "b"], capacity=16)
    n = 2 * T + 33
    net.put_all(0, {f"k{i}": i for i in range(n)}, WALL)
    b = net.gpu[1]
    assert b._table.capacity == 16 and b.length == 0 and b.recordMap() == {} and not b.containsKey("k5")
    b.refreshCanonicalTime()
    net.ora[1].refresh_canonical_time()
    assert net.merge_from(1, 0, wall=WALL + 1) is None
    assert b._table.capacity >= n and b.length == n and b.last_sync_winners == n
    net.check("grown")


@pytest.mark.parametrize("seed", [21])
def test_a_solitary_mapcrdt_is_a_group_of_one(gpu_device, seed):
    _random_ops_vs_oracle(seed)
    c = MapCrdt("solo", clock=lambda: WALL)
    c.put("x", 1, wall=WALL)
    assert c._shared() is False and c.last_sync is None and c.last_sync_winners is None
    c._keys.intern("known, never written")                          # (as a failed call's leftover would be)
    assert c.containsKey("known, never written")                    # today's answer
