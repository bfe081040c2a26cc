"""crdt_sync_tables (DeviceTable.sync_tables): the two-replica exchange a.merge(b.recordMap(since_b)) then
b.merge(a.recordMap(since_a)), fused into one clock pass and one apply pass over the two tables, against its
contract: the composition of two table merges on the C restatement (oracle_merge_table of
tests/test_gpu_table_merge.py applied twice, the second only after a clean first).  Where the numpy model of
tests/_sync_cases.py says the fused conditions hold, both contexts must report the plan table|sync, and
nowhere else.  Everything is integer data: every comparison is exact."""
import numpy as np
import pytest

import tests.test_gpu_table_merge as gt
from crdt_amd import CrdtNativeError, DeviceTable, _capi
from oracle.oracle_c import OracleTable, new_table
from tests import _sync_cases as sc
from tests import _table_cases as tc

pytestmark = pytest.mark.gpu

T = _capi.TABLE_TILE
GRID = _capi.SYNC_CLOCK_GRID
I64_MIN = tc.I64_MIN
U64_MAX = (1 << 64) - 1
MW = tc.MERGE_WALL
RESULT_FIELDS = gt.RESULT_FIELDS
STRIDES = gt.STRIDES
COLS = ("lt", "rank", "val", "mod")


def load_pair(a_rows, b_rows, cap, strides=(24, 24), c_a=None, c_b=sc.C_B):
    a, oa = gt.load(a_rows, cap, strides[0], local_rank=sc.A_RANK, canonical=sc.canon0() if c_a is None else c_a)
    b, ob = gt.load(b_rows, cap, strides[1], local_rank=sc.B_RANK, canonical=c_b)
    return a, oa, b, ob


def close(*tables):
    for t in tables:
        t.close()


oracle_sync = tc.oracle_sync                          # (the contract on the oracle: tests/_table_cases.py)


def check_sync(a, oa, b, ob, n_rows, since_a, since_b, wall, tag, fused="model", row_flags=True):
    """One sync_tables against the oracle: both results field by field, both tables' rows and canonicals,
    both flag arrays, and the plan of both contexts.  ``fused``: "model" -> what the numpy model says of
    the tables as they are; True / False -> that; None -> not checked.  Returns (model, results)."""
    m = sc.model({k: oa.rows[k].copy() for k in COLS}, {k: ob.rows[k].copy() for k in COLS}, n_rows, since_a,
                 since_b, oa.canonical, ob.canonical, wall, a.local_rank, b.local_rank)
    (ores_a, ofl_a), (ores_b, ofl_b) = oracle_sync(oa, ob, n_rows, since_a, since_b, wall)
    if a is not b and not (m["may_raise_1"] or m["may_raise_2"]) and m["status_1"] == 0:
        # the model is exact here: it must agree with the oracle before either judges the library
        assert np.array_equal(ofl_a != 0, m["win_a"]) and np.array_equal(ofl_b != 0, m["win_b"]), tag
        assert (oa.canonical, ob.canonical) == (m["canon_a"], m["canon_b"]), tag
    (res_a, fl_a), (res_b, fl_b) = a.sync_tables(b, n_rows, since_a, since_b, wall, row_flags=row_flags)
    for side, res, ores in (("a", res_a, ores_a), ("b", res_b, ores_b)):
        for f in RESULT_FIELDS:
            assert res[f] == ores[f], (tag, side, f, res[f], ores[f])
    gt.assert_rows(a, oa, (tag, "a"))
    gt.assert_rows(b, ob, (tag, "b"))
    if row_flags is not False:
        for side, fl, ofl in (("a", fl_a, ofl_a), ("b", fl_b, ofl_b)):
            got = fl.cpu().numpy() if hasattr(fl, "cpu") else np.asarray(fl)
            assert len(got) >= n_rows and np.array_equal(got[:n_rows], ofl), (tag, side, "flags")
    if fused == "model":
        fused = m["fused"] and a is not b
    if fused is not None:
        for side, t in (("a", a), ("b", b)):
            plan = t.last_plan()
            assert plan["sync"] is fused, (tag, side, plan)
            if fused:
                assert plan["table"] and not any(v for k, v in plan.items() if k not in ("table", "sync")), (tag, plan)
                assert t.last_path() == "gather"
    return m, (res_a, ofl_a, res_b, ofl_b)


# ------------------------------------------------------------------ 1. shapes
def run_shapes(n_rows, strides, fused="model"):
    a_rows, b_rows = sc.pair(n_rows, seed=3000 + n_rows)
    n_fused = 0
    for since_a, since_b in sc.since_pairs():
        a, oa, b, ob = load_pair(a_rows, b_rows, max(n_rows, 16), strides)
        m, _ = check_sync(a, oa, b, ob, n_rows, since_a, since_b, MW, (n_rows, strides, since_a, since_b), fused=fused)
        assert m["fused"] == (not m["ra_below_since_a"])
        n_fused += m["fused"]
        if n_rows >= tc.PLANT_FROM and (since_a, since_b) == (0, I64_MIN):
            assert m["both"].any()                              # rows stored on both sides
        close(a, b)
    assert n_fused >= 6                                         # (the two since_a above TOP fall back, from 63 rows on
                                                                #  only TOP + 1)


@pytest.mark.parametrize("strides", STRIDES)
@pytest.mark.parametrize("n_rows", sc.shapes())
def test_shapes(gpu_device, n_rows, strides):
    run_shapes(n_rows, strides)


@pytest.mark.parametrize("kind", ["host", "device_views", "one_side", "none"])
def test_flags_memory(gpu_device, kind):
    """Host arrays, caller's device tensors at odd alignments (nothing outside [0, n_rows) written), flags of
    one side only, and no flags at all: the same results."""
    import torch
    n_rows = 3 * T + 17
    a_rows, b_rows = sc.pair(n_rows, seed=3000 + n_rows)
    for since_a, since_b in [(0, 0), (tc.TOP + 1, sc.mid()), (sc.mid(), tc.TOP + 1)]:   # fused, fallback, sparse
        a, oa, b, ob = load_pair(a_rows, b_rows, n_rows)
        tag = (kind, since_a, since_b)
        if kind == "host":
            fl = (np.full(n_rows, 9, np.uint8), np.full(n_rows, 9, np.uint8))
            check_sync(a, oa, b, ob, n_rows, since_a, since_b, MW, tag, row_flags=fl)
        elif kind == "device_views":
            bufs = [torch.full((off + n_rows + 16,), 9, dtype=torch.uint8, device="cuda:0") for off in (1, 8)]
            fl = tuple(buf[off:off + n_rows] for buf, off in zip(bufs, (1, 8)))
            check_sync(a, oa, b, ob, n_rows, since_a, since_b, MW, tag, row_flags=fl)
            for buf, off in zip(bufs, (1, 8)):
                got = buf.cpu().numpy()
                assert np.all(got[:off] == 9) and np.all(got[off + n_rows:] == 9), tag
        elif kind == "one_side":
            (ra, fa), (rb, fb) = a.sync_tables(b, n_rows, since_a, since_b, MW, row_flags=(False, True))
            (ores_a, _), (ores_b, ofl_b) = oracle_sync(oa, ob, n_rows, since_a, since_b, MW)
            assert fa is None and np.array_equal(fb.cpu().numpy(), ofl_b), tag
            assert ra == ores_a and rb == ores_b, tag
            gt.assert_rows(a, oa, tag)
            gt.assert_rows(b, ob, tag)
        else:
            check_sync(a, oa, b, ob, n_rows, since_a, since_b, MW, tag, row_flags=False)
        close(a, b)


# ------------------------------------------------------------------ 2. tile skipping
@pytest.mark.parametrize("pattern", list(sc.patterns(T, 5 * T + 9)))
def test_tile_skipping(gpu_device, pattern):
    n_rows = 5 * T + 9
    sel_a, sel_b = sc.patterns(T, n_rows)[pattern]
    lo, hi = int(tc.STAMPS[2]), int(tc.STAMPS[30])
    a_rows = sc.select_pattern(n_rows, 21, sel_a, lo, hi)
    b_rows = sc.select_pattern(n_rows, 22, sel_b, lo, hi)
    # a's canonical at the top stamp: R_a >= since_a = hi whatever b selects, so the fused form runs
    a, oa, b, ob = load_pair(a_rows, b_rows, n_rows, c_a=tc.TOP)
    m, (res_a, ofl_a, res_b, ofl_b) = check_sync(a, oa, b, ob, n_rows, hi, hi, MW, pattern, fused=True)
    assert m["fused"]
    assert np.array_equal(m["sel_b"], sel_b) and np.array_equal(m["sel_a"], sel_a | m["win_a"])
    assert res_a["status"] == 0 and res_b["status"] == 0 and res_a["n_stored"] == res_b["n_stored"] == 1
    if pattern == "none":                # still one merge() call each: the closing sends advance both canonicals
        assert res_a["n_won"] == res_b["n_won"] == 0 and not ofl_a.any() and not ofl_b.any()
        assert a.canonical == b.canonical == MW << 16 > tc.TOP
    else:
        if sel_b.any():
            assert 0 < res_a["n_won"] == int(ofl_a.sum())
        if sel_a.any():
            assert 0 < res_b["n_won"] == int(ofl_b.sum())
    close(a, b)


# ------------------------------------------------------------------ 3. more tiles than the clock pass's grid
def test_more_tiles_than_the_clock_grid(gpu_device):
    n_rows = (GRID + 3) * T + 17
    a_rows, b_rows = sc.pair(n_rows, seed=5)
    a, oa, b, ob = load_pair(a_rows, b_rows, n_rows)
    m, (res_a, _, res_b, _) = check_sync(a, oa, b, ob, n_rows, 0, 0, MW, "grid", fused=True)
    assert res_a["n_won"] > n_rows // 4 and res_b["n_won"] > n_rows // 4
    close(a, b)


# ------------------------------------------------------------------ 4. fallbacks
N_EXC = 3 * T + 17
ABOVE = gt.ABOVE                                             # an lt above every stamp
DRIFT_LT = gt.DRIFT_LT


def exc_pair(plant_a=None, plant_b=None, c_a=None, c_b=sc.C_B):
    a_rows, b_rows = sc.pair(N_EXC, seed=41)
    for rows, planted in ((a_rows, plant_a), (b_rows, plant_b)):
        for k, (lt, rank, mod) in (planted or {}).items():
            tc._plant(rows, {k: (lt, rank, 77, mod)})
    return load_pair(a_rows, b_rows, N_EXC, c_a=c_a, c_b=c_b)


def written_ids(which: str):
    a_rows, b_rows = sc.pair(N_EXC, seed=41)
    d = tc.dense(a_rows if which == "a" else b_rows, N_EXC)
    return np.flatnonzero(d["mod"] >= 0)


def test_duplicate_node_in_direction_1(gpu_device):
    at = int(written_ids("b")[T + 3])
    a, oa, b, ob = exc_pair(plant_b={at: (ABOVE, sc.A_RANK, tc.TOP)})
    b_before, cb = gt.read_all(b), b.canonical
    m, (res_a, ofl_a, res_b, ofl_b) = check_sync(a, oa, b, ob, N_EXC, 0, 0, MW, "dup 1", fused=False)
    assert m["may_raise_1"] and res_a["status"] == _capi.CRDT_DUPLICATE_NODE and res_a["n_stored"] == 0
    assert res_b == {"status": 0, "n_stored": 0, "exc_changeset": 0, "exc_index": U64_MAX, "canonical_lt": cb,
                     "drift_ms": 0, "counter": 0, "n_present": 0, "n_won": 0}
    assert not ofl_a.any() and not ofl_b.any() and b.canonical == cb
    for x, y in zip(b_before, gt.read_all(b)):
        assert np.array_equal(x, y)                          # b untouched
    close(a, b)


def test_duplicate_node_in_direction_2_only(gpu_device):
    """A row of a carries b's node id above b's canonical and is not replaced by step 1: a merges, b's recv()
    raises at it and stores nothing."""
    at = int(written_ids("a")[2 * T + 9])
    a, oa, b, ob = exc_pair(plant_a={at: (ABOVE, sc.B_RANK, tc.TOP)})
    b_before = gt.read_all(b)
    m, (res_a, ofl_a, res_b, ofl_b) = check_sync(a, oa, b, ob, N_EXC, 0, 0, MW, "dup 2", fused=False)
    assert not m["may_raise_1"] and m["may_raise_2"] and not m["win_a"][at]
    assert res_a["status"] == 0 and res_a["n_won"] == int(ofl_a.sum()) > 0
    assert res_b["status"] == _capi.CRDT_DUPLICATE_NODE and res_b["n_stored"] == 0 and not ofl_b.any()
    for x, y in zip(b_before, gt.read_all(b)):
        assert np.array_equal(x, y)
    close(a, b)


def test_duplicate_node_in_direction_2_from_a_row_that_won_into_a(gpu_device):
    """b holds a row with its OWN node id above its canonical (a raw put_rows).  It wins into a, comes back in
    step 2 and raises there: the direction-2 candidate bit has to see step 1's winners."""
    at = int(written_ids("b")[T - 5])
    a, oa, b, ob = exc_pair(plant_b={at: (ABOVE, sc.B_RANK, tc.TOP)})
    m, (res_a, ofl_a, res_b, ofl_b) = check_sync(a, oa, b, ob, N_EXC, 0, 0, MW, "dup 2 via a", fused=False)
    assert not m["may_raise_1"] and m["may_raise_2"] and m["win_a"][at]
    assert res_a["status"] == 0 and ofl_a[at] == 1
    assert res_b["status"] == _capi.CRDT_DUPLICATE_NODE and res_b["n_stored"] == 0 and not ofl_b.any()
    close(a, b)


def test_drift_on_a_selected_row(gpu_device):
    at = int(written_ids("b")[T + 3])
    a, oa, b, ob = exc_pair(plant_b={at: (DRIFT_LT, 2, tc.TOP)})
    m, (res_a, _, res_b, ofl_b) = check_sync(a, oa, b, ob, N_EXC, 0, 0, MW, "drift", fused=False)
    assert res_a["status"] == _capi.CRDT_CLOCK_DRIFT and res_a["drift_ms"] == 60001 and res_a["n_stored"] == 0
    assert res_b["status"] == 0 and res_b["n_stored"] == 0 and not ofl_b.any()
    close(a, b)


@pytest.mark.parametrize("kind", ["drift", "overflow"])
def test_send_fails_after_step_1s_store(gpu_device, kind):
    c1 = (MW + 60001) << 16 if kind == "drift" else ((MW + 5) << 16) | 0xFFFF
    a, oa, b, ob = exc_pair(c_a=c1)
    b_before, cb = gt.read_all(b), b.canonical
    m, (res_a, ofl_a, res_b, ofl_b) = check_sync(a, oa, b, ob, N_EXC, 0, 0, MW, kind, fused=False)
    want = _capi.CRDT_CLOCK_DRIFT if kind == "drift" else _capi.CRDT_OVERFLOW
    assert m["status_1"] == want == res_a["status"] and res_a["exc_index"] == U64_MAX
    assert res_a["n_stored"] == 1 and res_a["n_won"] == int(ofl_a.sum()) > 0 and a.canonical == c1
    assert res_b["n_stored"] == 0 and res_b["canonical_lt"] == cb == b.canonical and not ofl_b.any()
    for x, y in zip(b_before, gt.read_all(b)):
        assert np.array_equal(x, y)
    close(a, b)


def test_send_overflows_after_step_2s_store_and_stays_fused(gpu_device):
    c2 = ((MW + 5) << 16) | 0xFFFF
    a, oa, b, ob = exc_pair(c_b=c2)
    m, (res_a, ofl_a, res_b, ofl_b) = check_sync(a, oa, b, ob, N_EXC, 0, 0, MW, "overflow 2", fused=True)
    assert m["fused"] and m["status_2"] == _capi.CRDT_OVERFLOW
    assert res_a["status"] == 0 and res_a["n_won"] > 0
    assert (res_b["status"], res_b["exc_index"], res_b["counter"]) == (_capi.CRDT_OVERFLOW, U64_MAX, 0x10000)
    assert res_b["n_stored"] == 1 and res_b["n_won"] == int(ofl_b.sum()) > 0 and b.canonical == c2
    assert np.all(gt.read_all(b)[3][np.flatnonzero(ofl_b)] == c2)       # b's winners carry mod = R_b
    close(a, b)


def test_a_is_b(gpu_device):
    rows, _ = sc.pair(N_EXC, seed=91)
    t, o = gt.load(rows, N_EXC, local_rank=sc.A_RANK, canonical=sc.canon0())
    m, (res_a, _, res_b, _) = check_sync(t, o, t, o, N_EXC, 0, 0, MW, "self", fused=False)
    assert res_a["status"] == res_b["status"] == 0 and res_a["n_won"] == res_b["n_won"] == 0
    assert res_a["n_present"] == res_b["n_present"] > 0
    t.close()


@pytest.mark.parametrize("which", ["a", "b"])
def test_a_ctx_pinned_to_sorted(gpu_device, which):
    a, oa, b, ob = exc_pair()
    (a if which == "a" else b).set_merge_path("sorted")
    m, (res_a, _, res_b, _) = check_sync(a, oa, b, ob, N_EXC, 0, 0, MW, ("sorted", which), fused=False)
    assert m["fused"] and res_a["n_won"] > 0 and res_b["n_won"] > 0     # (only the pin kept it from the fused form)
    close(a, b)


def test_switch_takes_the_composition(gpu_device, monkeypatch):
    monkeypatch.setenv("CRDT_TABLE_MERGE", "0")              # read when the tables are created
    run_shapes(3 * T + 17, (24, 32), fused=False)


def test_n_rows_above_one_capacity_is_invalid(gpu_device):
    a_rows, b_rows = sc.pair(N_EXC, seed=41)
    small, _ = sc.pair(T + 5, seed=43)
    for a_cap, b_cap in ((N_EXC, T + 5), (T + 5, N_EXC)):
        a, oa = gt.load(a_rows if a_cap == N_EXC else small, a_cap, local_rank=sc.A_RANK, canonical=sc.canon0())
        b, ob = gt.load(b_rows if b_cap == N_EXC else small, b_cap, local_rank=sc.B_RANK, canonical=sc.C_B)
        assert min(a.capacity, b.capacity) == T + 5
        with pytest.raises(CrdtNativeError) as e:
            a.sync_tables(b, T + 6, 0, 0, MW, row_flags=True)
        assert e.value.status == _capi.CRDT_E_INVALID
        gt.assert_rows(a, oa, "a untouched")
        gt.assert_rows(b, ob, "b untouched")
        check_sync(a, oa, b, ob, T + 5, 0, 0, MW, "at the smaller capacity", fused=True)
        close(a, b)


def test_other_device_is_refused(gpu_device):
    a, b = DeviceTable(0, capacity=16), DeviceTable(0, capacity=16)
    b.device = 1                                              # (as if it had been created on another GPU)
    with pytest.raises(ValueError):
        a.sync_tables(b, 16, 0, 0, MW)
    b.device = 0
    close(a, b)


# ------------------------------------------------------------------ 5. idempotence, convergence
def test_second_sync_stores_nothing(gpu_device):
    n_rows = 3 * T + 17
    a_rows, b_rows = sc.pair(n_rows, seed=3000 + n_rows)
    a, oa, b, ob = load_pair(a_rows, b_rows, n_rows)
    m, (res_a, _, res_b, _) = check_sync(a, oa, b, ob, n_rows, 0, 0, MW, "first", fused=True)
    assert res_a["n_won"] > 0 and res_b["n_won"] > 0
    m, (res_a, ofl_a, res_b, ofl_b) = check_sync(a, oa, b, ob, n_rows, 0, 0, MW + 1, "second")
    assert res_a["n_won"] == res_b["n_won"] == 0 and not ofl_a.any() and not ofl_b.any()
    ra, rb = gt.read_all(a), gt.read_all(b)
    vis = ra[3] >= 0
    assert np.array_equal(vis, rb[3] >= 0) and vis.any()
    for name, x, y in zip(("lt", "rank"), ra, rb):
        assert np.array_equal(x[vis], y[vis]), ("the visible rows of the two tables are equal", name)
    # The values too, except where the generator gave both replicas the SAME (lt, rank) with different values
    # (planted row 0 and a few chance ties): equal keeps local on both sides (crdt.dart:83-90), so each keeps
    # its own.  Taken from the generated rows, not from what the library left.
    A0, B0 = tc.dense(a_rows, n_rows), tc.dense(b_rows, n_rows)
    tie = (A0["lt"] == B0["lt"]) & (A0["rank"] == B0["rank"]) & (A0["mod"] >= 0) & (B0["mod"] >= 0)
    assert tie[0] and 0 < int(tie.sum()) < n_rows // 100
    keep = vis & ~tie
    assert np.array_equal(ra[2][keep], rb[2][keep]), ("the visible rows of the two tables are equal", "val")
    close(a, b)


# ------------------------------------------------------------------ 6. scratch reuse on one pair of contexts
def reset(t: DeviceTable, rows: dict, canonical: int) -> OracleTable:
    """The long-lived table cleared and refilled; returns its new oracle mirror."""
    cap = t.capacity
    t.clear_rows(0, cap)
    o = OracleTable(cap, t.local_rank, canonical)
    cols = tuple(rows[k] for k in ("ids", "lt", "rank", "val", "mod"))
    if len(cols[0]):
        t.put_rows(*cols)
        o.put_rows(*cols)
    first, count = rows.get("clear", (0, 0))
    if count:
        t.clear_rows(first, count)
        o.rows[first:first + count] = new_table(count)
    t.canonical = canonical
    return o


def check_merge(t, o, n_rows, seed, tag):
    """A two-changeset host merge into the long-lived table, against the oracle."""
    rng = np.random.default_rng(seed)
    n = max(n_rows // 2, 1)
    key = np.concatenate([rng.permutation(max(n_rows, 1))[:n], rng.permutation(max(n_rows, 1))[:n]]).astype(np.uint32)
    lt = tc.STAMPS[rng.integers(0, tc.N_STAMPS, 2 * n)].astype(np.int64)
    rank = rng.integers(0, 6, 2 * n).astype(np.uint32)
    val = rng.integers(0, 1 << 20, 2 * n).astype(np.uint32)
    offs = np.array([0, n, 2 * n], np.uint64)
    ores, oflags = o.merge(key, lt, rank, val, offs, MW)
    res, flags = t.merge(key, lt, rank, val, offs, MW)
    for f in RESULT_FIELDS:
        assert res[f] == ores.as_dict()[f], (tag, "merge", f)
    assert np.array_equal(np.asarray(flags), oflags), (tag, "merge flags")
    gt.assert_rows(t, o, (tag, "merge"))


@pytest.mark.parametrize("poison", [False, True], ids=["plain", "poison"])
def test_scratch_reuse(gpu_device, monkeypatch, poison):
    """One pair of contexts alternates merge, merge_table and sync_tables at shrinking and growing n_rows, its
    scratch fresh from hipMalloc or filled with 0x5A bytes: every call matches the oracle."""
    monkeypatch.setenv("CRDT_ENV_DYNAMIC", "1")               # (read when a table is created)
    monkeypatch.setenv("CRDT_POISON_ALLOC", "1" if poison else "0")
    cap = 5 * T + 9
    a = DeviceTable(0, local_rank=sc.A_RANK, capacity=cap)
    b = DeviceTable(0, local_rank=sc.B_RANK, capacity=cap)
    pairs = sc.since_pairs()
    for step, n_rows in enumerate([3 * T + 17, 65, 5 * T + 9, T, 1, 2 * T + 1, 0, 4 * T - 1, 63]):
        a_rows, b_rows = sc.pair(n_rows, seed=7000 + step)
        since_a, since_b = pairs[step % len(pairs)]
        oa, ob = reset(a, a_rows, sc.canon0()), reset(b, b_rows, sc.C_B)
        tag = (step, n_rows, since_a, since_b)
        check_sync(a, oa, b, ob, n_rows, since_a, since_b, MW, tag)
        check_merge(a, oa, n_rows, 100 + step, tag)
        gt.check(b, ob, a, oa, n_rows, since_a, MW + 1, (tag, "merge_table"), table=None)
        check_sync(a, oa, b, ob, n_rows, 0, 0, MW + 2, (tag, "again"))
        check_merge(b, ob, n_rows, 200 + step, tag)
    close(a, b)
