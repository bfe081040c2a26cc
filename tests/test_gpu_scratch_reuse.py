"""Scratch reuse on one long-lived context: every merge form after every other, with the context's scratch
buffers fresh from hipMalloc or filled with 0x5A bytes (CRDT_POISON_ALLOC=1, read at each allocation).

A kernel that reads scratch no kernel of the same call wrote gets zeroes from a fresh allocation (often the
value that hides it), the previous call's bytes on a reused context and 0x5A5A... under the poison; the
catalogue and the runner are tests/_ctx_sequence.py.  Everything is integer data: every comparison is exact."""
import numpy as np
import pytest

from tests import _ctx_sequence as seq
from tests._cases import ABSENT_MOD, NULL, WALL

pytestmark = pytest.mark.gpu


def _env(monkeypatch, poison: bool, **more):
    monkeypatch.setenv("CRDT_ENV_DYNAMIC", "1")               # (read when a table is created)
    monkeypatch.setenv("CRDT_POISON_ALLOC", "1" if poison else "0")
    for k, v in more.items():
        monkeypatch.setenv(k, v)


@pytest.mark.parametrize("step", seq.CATALOGUE, ids=lambda s: s.name)
def test_step_alone_poisoned(gpu_device, monkeypatch, step):
    """Each catalogue step on a fresh context whose every scratch allocation holds 0x5A bytes: the suite's
    single-call coverage without whatever hipMalloc returned; names the failing form directly."""
    from crdt_amd import DeviceTable
    _env(monkeypatch, True)
    phase = step.phases[0]
    t = DeviceTable(0, local_rank=0, capacity=seq.PHASE1_CAP if phase == 1 else seq.PHASE2_CAP)
    try:
        if seq.run_step(t, step, phase, monkeypatch.setenv):
            seq.check_views(t, step)
    finally:
        t.close()


KV_WINDOW_SEED = 2                  # this seed's context splits host batches into 777-record windows


@pytest.mark.parametrize("poison", [False, True], ids=["plain", "poison"])
@pytest.mark.parametrize("seed", range(4))
def test_sequence(gpu_device, monkeypatch, seed, poison):
    """One context runs a seeded permutation of the whole catalogue forwards and backwards, in one partition
    level and, after one reserve, in two: larger before smaller and every form before and after every other.
    After every successful step the export, the id list, the counts and refresh_canonical on the rows it
    left; after every fourth a merge_table into a second long-lived table; merge_from once from each side."""
    more = {"CRDT_KV_WINDOW": "777"} if seed == KV_WINDOW_SEED else {}
    _env(monkeypatch, poison, **more)
    seq.run_sequence(seed, monkeypatch.setenv)


LOOP_G, LOOP_K, LOOP_R = 4, 1 << 23, 64          # shards of 2^21 slots (route_l1 needs > 2^20), 64 changesets (auto
                                                 # routing takes the fan-in ways from 64 on)
# records of the two jobs: route_l1 cuts pieces from 2^20 home records on (a quarter of the job is rank 0's), so
# the small job sits exactly there and the other is half as large again (at 512,000 records one piece is reported)
LOOP_TOTALS = (4 << 20, 6 << 20)
# way: (CRDT_COMBINE, CRDT_ROUTE_L1, CRDT_RL1_SPLIT, pieces reported)
LOOP_WAYS = {"pieces1": ("0", "1", "0", 1), "pieces2": ("0", "1", "1", 2), "pieces4": ("0", "1", "4", 4),
             "head": ("0", "2", "1", 2), "headall": ("0", "3", "1", 2), "route": ("0", "0", "1", 0),
             "fold": ("2", "1", "1", 0)}


@pytest.mark.parametrize("poison", [False, True], ids=["plain", "poison"])
def test_loopback_sequence(gpu_device, monkeypatch, poison):
    """One sharded context (rank 0 of 4 through the loopback communicator of tests/_loopback.py) alternates the
    routing ways of test_loopback_route_ways_same_rows — route_l1 in 1, 2 and 4 pieces, with the head fold and
    with every digit folded, record routing, the map-side fold — over two fan-in jobs of different sizes, every
    way on both jobs and every call after a call of the other size: rows against _loopback_winners (its tie
    slots excepted for the value), the plan bits of each way, and the bytes handed to the communicator."""
    from crdt_amd import DeviceTable
    from crdt_amd.workload import gen_fanin
    from tests._loopback import LoopbackComm
    from tests.test_gpu_parity import _loopback_winners
    _env(monkeypatch, poison)
    G = LOOP_G
    jobs = [gen_fanin(total=total, R=LOOP_R, K=LOOP_K, n_local=1 << 20, s=0.8, device="cuda", rank=0, world=G,
                      route=True, seed=0xC0FFEE04 + i) for i, total in enumerate(LOOP_TOTALS)]
    cap = jobs[0]["capacity"]
    assert cap == jobs[1]["capacity"] > (1 << 20)
    want = [_loopback_winners(wl, G, cap) for wl in jobs]
    t = DeviceTable(0, local_rank=0, capacity=cap)
    t.set_counts(False)
    comm = LoopbackComm(G)
    t.comm_init_ops(G, 0, comm)
    mods = [None, None]
    ran = set()
    names = list(LOOP_WAYS)
    assert len(names) % 2 == 1
    for k, name in enumerate(names + names):
        job = k % 2                                            # alternating; an odd number of ways, so the second
                                                               # pass takes each way on the other job
        comb, rl1, split, pieces = LOOP_WAYS[name]
        monkeypatch.setenv("CRDT_COMBINE", comb)
        monkeypatch.setenv("CRDT_ROUTE_L1", rl1)
        monkeypatch.setenv("CRDT_RL1_SPLIT", split)
        wl = jobs[job]
        home, loc = wl["home"], wl["local"]
        t.clear_rows(0, cap)
        t.put_rows(loc["slot"], loc["lt"], loc["rank"], loc["val"], loc["mod"])
        t.canonical = wl["c0"]
        res, _ = t.merge(home["key"], home["lt"], home["rank"], home["val"], wl["home_offsets"], wl["wall"],
                         win_flags=False)
        tag = (k, name, job)
        assert res["status"] == 0 and comm.error is None, (tag, res, comm.error)
        assert t.timing()["sent_bytes"] == comm.exchange_bytes() > 0, tag
        plan = t.last_plan()
        assert plan["route_l1"] == (pieces > 0) and plan["rl1_pieces"] == pieces, (tag, plan)
        assert plan["combined"] == (name == "fold"), (tag, plan)
        assert plan["rl1_head"] == name.startswith("head"), (tag, plan)
        lt, rank, val, mod = t.read_rows(np.arange(cap, dtype=np.uint32))
        w_lt, w_rank, w_val, present, tie = want[job]
        assert np.array_equal(mod != ABSENT_MOD, present), tag
        assert np.array_equal(lt[present], w_lt[present]) and np.array_equal(rank[present], w_rank[present]), tag
        keep = present & ~tie
        assert np.array_equal(val[keep], w_val[keep]), tag
        if mods[job] is None:
            mods[job] = mod
        assert np.array_equal(mod, mods[job]), tag              # every way stamps the same rows alike
        ran.add((name, job))
    comm.exchange_ms()
    t.close()
    assert ran == {(n, j) for n in names for j in (0, 1)}


def _put_stamped_both(t, o, key, val, wall):
    """put_stamped on the table and on its oracle mirror; a refused call's status, else the result fields."""
    from crdt_amd import CrdtNativeError
    want = o.put_stamped(key, val, wall).as_dict()
    try:
        got = t.put_stamped(key, val, wall)
    except CrdtNativeError as e:
        return e.status, want
    for f in seq.RESULT_FIELDS:
        assert got[f] == want[f], (f, got[f], want[f])
    return got, want


@pytest.mark.parametrize("poison", [False, True], ids=["plain", "poison"])
def test_put_stamped_reused_context(gpu_device, monkeypatch, poison):
    """put_stamped on a context whose staging buffers earlier merges sized and filled: a send() that fails on
    drift and on counter overflow and a key at the capacity (status and fields as oracle_c.send_scalar and
    OracleTable.put_stamped give them, rows and canonical unchanged), then 600,000 keys — more than the
    2048 x 256 threads of the put grid, so its grid-stride loop runs — every row, and refresh_canonical over
    them with invisible rows (mod < 0) holding the largest lt."""
    from crdt_amd import DeviceTable, _capi
    from oracle.oracle_c import OracleTable, send_scalar
    _env(monkeypatch, poison)
    cap = 700_001
    t = DeviceTable(0, local_rank=0, capacity=cap)
    by_name = {s.name: s for s in seq.CATALOGUE}
    for name in ("gather_300k_one_changeset", "free_edges", "flagged_split_bucket"):
        assert seq.run_step(t, by_name[name], 1, monkeypatch.setenv)
    c = seq.case("fused0")
    seq.reset(t, c)
    t.local_rank = 3
    o = OracleTable(cap, 3, c["c0"])
    loc = c["local"]
    o.put_rows(np.arange(c["n_local"], dtype=np.uint32), loc["lt"], loc["rank"], loc["val"], loc["mod"])

    def same(tag):
        seq.rows_equal(t, o.rows, cap, tag)
        assert t.canonical == o.canonical, tag

    same("start")
    key = np.array([5, 4999, cap - 1], np.uint32)
    val = np.array([1, NULL, 7], np.uint32)
    # drift: the canonical's millis more than 60 s above the wall
    for tag, canon, status in (("drift", (WALL + 60_001) << 16, _capi.CRDT_CLOCK_DRIFT),
                               ("overflow", (WALL << 16) | 0xFFFF, _capi.CRDT_OVERFLOW)):
        t.canonical = o.canonical = canon
        got, want = _put_stamped_both(t, o, key, val, WALL)
        st, _, drift, counter = send_scalar(canon, WALL)
        assert got["status"] == want["status"] == st == status, (tag, got, want, st)
        assert (got["drift_ms"], got["counter"]) == (drift, counter), (tag, got, drift, counter)
        assert got["canonical_lt"] == canon and got["n_won"] == 0, (tag, got)
        same(tag)
    # a key at the capacity: nothing of the call is stored
    t.canonical = o.canonical = c["c0"]
    got, want = _put_stamped_both(t, o, np.array([5, cap, 9], np.uint32), val, WALL)
    assert got == _capi.CRDT_E_KEY_RANGE, got
    same("key at the capacity")
    # 600,000 keys: the grid-stride loop
    rng = np.random.default_rng(600_000)
    key = rng.permutation(cap)[:600_000].astype(np.uint32)
    val = rng.integers(0, 1 << 20, len(key)).astype(np.uint32)
    val[rng.random(len(key)) < 0.1] = NULL
    got, want = _put_stamped_both(t, o, key, val, WALL)
    assert got["status"] == 0 and got["n_won"] == len(key) and got["canonical_lt"] == o.canonical
    same("600,000 keys")
    # invisible rows with the largest lt must not count in refreshCanonicalTime
    hid = rng.choice(cap, 1000, replace=False).astype(np.uint32)
    top = np.full(len(hid), o.canonical + (5 << 16), np.int64) + np.arange(len(hid))
    cols = (hid, top, np.full(len(hid), 4, np.uint32), np.zeros(len(hid), np.uint32),
            np.where(np.arange(len(hid)) % 2 == 0, -(1 << 20), ABSENT_MOD).astype(np.int64))
    t.put_rows(*cols)
    o.put_rows(*cols)
    same("hidden rows")
    assert (o.rows["lt"][o.rows["mod"] < 0].max()) > o.rows["lt"][o.rows["mod"] >= 0].max()
    assert t.refresh_canonical(cap) == o.refresh(cap) == int(o.rows["lt"][o.rows["mod"] >= 0].max())
    t.close()
