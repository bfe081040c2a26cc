"""crdt_fanin_tables (DeviceTable.merge_tables): up to eight replicas merged into one table, decided on one
read of it, against its contract: the sequence of table merges on the C restatement (oracle_merge_table of
tests/test_gpu_table_merge.py applied source by source, ending at the first step that raises).  Where the
numpy model of tests/_fanin_cases.py says the fused conditions hold, dst must report the plan table|fanin,
and nowhere else.  Everything is integer data: every comparison is exact."""
import numpy as np
import pytest

import tests.test_gpu_sync_tables as gs
import tests.test_gpu_table_merge as gt
from crdt_amd import CrdtNativeError, DeviceTable, _capi
from tests import _fanin_cases as fc
from tests import _sync_cases as sc
from tests import _table_cases as tc

pytestmark = pytest.mark.gpu

T = _capi.TABLE_TILE
GRID = _capi.TABLE_CLOCK_GRID
I64_MIN = tc.I64_MIN
U64_MAX = (1 << 64) - 1
MW = tc.MERGE_WALL
RESULT_FIELDS = gt.RESULT_FIELDS
COLS = fc.COLS
DRIFT_LT = gt.DRIFT_LT
DUP_LT = (MW + 10) << 16                 # above every running canonical of a call at MW, within the drift bound
CLEARED = tc.CLEARED


def close(*tables):
    for t in {id(t): t for t in tables}.values():
        t.close()


def load_sources(rows_list, cap, strides=None):
    out = [gt.load(rows, cap, (strides or [24] * len(rows_list))[j], local_rank=1 + j % 5, canonical=100 + j)
           for j, rows in enumerate(rows_list)]
    return [t for t, _ in out], [o for _, o in out]


def load_dst(rows, cap, stride=24, canonical=None):
    return gt.load(rows, cap, stride, local_rank=fc.DST_RANK, canonical=sc.canon0() if canonical is None else canonical)


oracle_fanin = tc.oracle_fanin                        # (the contract on the oracle: tests/_table_cases.py)


def check_fanin(dst, odst, srcs, osrcs, n_rows, sinces, wall, tag, fused="model", win_mask=True):
    """One merge_tables against the oracle: every result field by field, dst's rows and canonical, the mask,
    every source untouched, and the plan.  ``fused``: "model" -> what the numpy model says of the tables as
    they are; True / False -> that; None -> not checked.  Returns (model, results, mask)."""
    own = any(s is dst for s in srcs)
    m = fc.model({k: odst.rows[k].copy() for k in COLS}, [{k: o.rows[k].copy() for k in COLS} for o in osrcs],
                 n_rows, sinces, odst.canonical, wall, dst.local_rank, dst_cap=dst.capacity)
    before = [(o.rows.copy(), o.canonical) for o in osrcs]
    ores, omask, stop = oracle_fanin(odst, osrcs, n_rows, sinces, wall)
    if not own and not m["may_raise"] and not m["out_of_range"]:
        # the model is exact here: it must agree with the oracle before either judges the library
        assert np.array_equal(omask, m["mask"]) and odst.canonical == m["canonical"], tag
        assert [r["n_present"] for r in ores[:len(m["n_present"])]] == m["n_present"], tag
    res, mask = dst.merge_tables(srcs, n_rows, sinces, wall, win_mask=win_mask)
    assert len(res) == len(srcs)
    for j, (r, o) in enumerate(zip(res, ores)):
        for f in RESULT_FIELDS:
            assert r[f] == o[f], (tag, j, f, r[f], o[f])
    gt.assert_rows(dst, odst, tag)
    if win_mask is not False:
        got = mask.cpu().numpy() if hasattr(mask, "cpu") else np.asarray(mask)
        assert len(got) >= n_rows and np.array_equal(got[:n_rows], omask), (tag, "mask")
        if stop is not None:
            assert not (omask >> (stop + 1)).any(), (tag, "no bit above the stop")
    if not own:
        for j, (s, o, (rows, canon)) in enumerate(zip(srcs, osrcs, before)):
            assert np.array_equal(o.rows, rows) and o.canonical == canon
            gt.assert_rows(s, o, (tag, "source untouched", j))
    if fused == "model":
        fused = m["fused"] and not own
    if fused is not None:
        plan = dst.last_plan()
        assert plan["fanin"] is (fused and len(srcs) > 1), (tag, plan)
        if fused:
            assert plan["table"] and not any(v for k, v in plan.items() if k not in ("table", "fanin")), (tag, plan)
            assert dst.last_path() == "gather"
    return m, res, omask


# ------------------------------------------------------------------ 1. shapes
def run_shapes(n_rows, n_src, fused="model"):
    cap = max(n_rows, 16)
    strides = [24 if j % 2 else 32 for j in range(n_src)]            # row strides mixed between dst and sources
    srcs, osrcs = load_sources([fc.source_rows(n_rows, j) for j in range(n_src)], cap, strides)
    for name, sinces in fc.since_vectors(n_src).items():
        dst, odst = load_dst(fc.dst_rows(n_rows), cap, 32 if name in ("mid", "mixed") else 24)
        c0 = dst.canonical
        m, res, omask = check_fanin(dst, odst, srcs, osrcs, n_rows, sinces, MW, (n_rows, n_src, name), fused=fused)
        assert m["fused"] and [r["status"] for r in res] == [0] * n_src
        if n_rows >= 63 and name != "mixed":
            assert (m["stores"] > 1).any()                           # rows stored more than once in the call
        # an empty selection is still one merge() call: every step's send moves the canonical
        canons = [c0] + [r["canonical_lt"] for r in res]
        assert all(x < y for x, y in zip(canons, canons[1:])) and all(r["n_stored"] == 1 for r in res)
        dst.close()
    close(*srcs)


@pytest.mark.parametrize("n_src", [2, 8])
@pytest.mark.parametrize("n_rows", fc.shapes())
def test_shapes(gpu_device, n_rows, n_src):
    run_shapes(n_rows, n_src)


def test_shapes_three_sources(gpu_device):
    run_shapes(3 * T + 17, 3)


def test_one_source_is_merge_table(gpu_device):
    n_rows = 3 * T + 17
    srcs, osrcs = load_sources([fc.source_rows(n_rows, 0)], n_rows)
    dst, odst = load_dst(fc.dst_rows(n_rows), n_rows)
    m, res, omask = check_fanin(dst, odst, srcs, osrcs, n_rows, [0], MW, "one", fused=None)
    plan = dst.last_plan()
    assert plan["table"] and not plan["fanin"] and res[0]["n_won"] == int(omask.sum()) > 0
    close(dst, *srcs)


def test_switch_takes_the_composition(gpu_device, monkeypatch):
    monkeypatch.setenv("CRDT_TABLE_MERGE", "0")              # read when the tables are created
    run_shapes(3 * T + 17, 3, fused=False)


# ------------------------------------------------------------------ 2. planted rows: the sequence rules
def test_planted_rows(gpu_device):
    n_rows = 3 * T + 17
    s10, s20, s30, s35 = (int(tc.STAMPS[k]) for k in (10, 20, 30, 35))
    NULL = 0xFFFFFFFF
    a, b, c = 1000, 2 * T - 1, 3 * T + 16                    # outside every cleared range (checked by _plant)
    rows = [fc.source_rows(n_rows, j) for j in range(2)]
    drows = fc.dst_rows(n_rows)
    # a: source 0 wins, source 1 carries the same (lt, rank): equal keeps local
    # b: dst invisible; an older source 0 wins; an even older source 1 then loses
    # c: a tombstone wins, then a newer live row wins
    tc._plant(drows, {a: (s10, 2, 31, s10), b: (s30, 5, 32, -(1 << 20)), c: (s10, 1, 33, s10)})
    tc._plant(rows[0], {a: (s20, 3, 41, tc.TOP), b: (s20, 2, 42, tc.TOP), c: (s20, 4, NULL, tc.TOP)})
    tc._plant(rows[1], {a: (s20, 3, 51, tc.TOP), b: (s10, 2, 52, tc.TOP), c: (s35, 0, 53, tc.TOP)})
    srcs, osrcs = load_sources(rows, n_rows, [24, 32])
    dst, odst = load_dst(drows, n_rows)
    m, res, omask = check_fanin(dst, odst, srcs, osrcs, n_rows, [0, 0], MW, "planted", fused=True)
    assert (omask[a], omask[b], omask[c]) == (1, 1, 3)
    lt, rank, val, mod = dst.read_rows(np.array([a, b, c], np.uint32))
    assert list(val) == [41, 42, 53] and list(mod) == [m["stamps"][0], m["stamps"][0], m["stamps"][1]]
    # n_present of row b alone: 0, then 1, then 1 (dst, then one source at a time, selecting only that row)
    for t in (dst, *srcs):
        t.close()
    only = lambda r: {k: (v[r["ids"] == b] if k != "clear" else (0, 0)) for k, v in r.items() if k != "n_rows"}  # noqa: E731
    srcs, osrcs = load_sources([only(rows[0]), only(rows[1]), only(rows[1])], n_rows)
    dst, odst = load_dst(only(drows), n_rows)
    m, res, omask = check_fanin(dst, odst, srcs, osrcs, n_rows, [0, 0, 0], MW, "row b", fused=True)
    assert [r["n_present"] for r in res] == [0, 1, 1] and [r["n_won"] for r in res] == [1, 0, 0]
    close(dst, *srcs)


def test_same_source_twice(gpu_device):
    n_rows = 3 * T + 17
    srcs, osrcs = load_sources([fc.source_rows(n_rows, 0), fc.source_rows(n_rows, 1)], n_rows)
    dst, odst = load_dst(fc.dst_rows(n_rows), n_rows)
    order = [0, 1, 0]
    m, res, omask = check_fanin(dst, odst, [srcs[k] for k in order], [osrcs[k] for k in order], n_rows,
                                [0, 0, 0], MW, "twice", fused=True)
    assert res[0]["n_won"] > 0 and res[1]["n_won"] > 0 and res[2]["n_won"] == 0 and not (omask & 4).any()
    assert res[2]["n_present"] > 0
    close(dst, *srcs)


# ------------------------------------------------------------------ 3. tile skipping
@pytest.mark.parametrize("pattern", list(fc.tile_patterns(T, 5 * T + 9)))
def test_tile_skipping(gpu_device, pattern):
    n_rows = 5 * T + 9
    sels = fc.tile_patterns(T, n_rows)[pattern]
    lo, hi = int(tc.STAMPS[2]), int(tc.STAMPS[30])
    srcs, osrcs = load_sources([sc.select_pattern(n_rows, 31 + j, sel, lo, hi) for j, sel in enumerate(sels)], n_rows)
    dst, odst = load_dst(sc.select_pattern(n_rows, 30, np.zeros(n_rows, bool), lo, hi), n_rows)
    m, res, omask = check_fanin(dst, odst, srcs, osrcs, n_rows, [hi] * len(sels), MW, pattern, fused=True)
    for j, sel in enumerate(sels):
        assert res[j]["n_present"] == int(sel.sum()) and res[j]["n_stored"] == 1
        assert not ((omask >> j) & 1)[~sel].any()
        if sel.any():
            assert 0 < res[j]["n_won"] == int(((omask >> j) & 1).sum())
    if pattern == "none":
        assert not omask.any() and dst.canonical == (MW << 16) + len(sels) - 1
    close(dst, *srcs)


def test_sources_with_different_high_water_marks(gpu_device):
    """Sources written up to different rows (their clock passes cover different tile counts) in tables of one
    capacity, into a dst written further than some and less far than others."""
    w = T + 5
    cap = 4 * w
    widths = [3 * w, 0, w, 2 * w + 1]
    srcs, osrcs = load_sources([fc.source_rows(x, j) for j, x in enumerate(widths)], cap)
    for since in (0, I64_MIN):                               # (I64_MIN selects the never-written rows too)
        dst, odst = load_dst(fc.dst_rows(2 * w), cap)
        m, res, omask = check_fanin(dst, odst, srcs, osrcs, cap, [since, since, since, 0], MW, ("marks", since),
                                    fused=True)
        assert res[0]["n_won"] > 0 and res[2]["n_won"] > 0 and omask[2 * w:3 * w].any()
        assert res[1]["n_present"] == res[1]["n_won"] == 0 or since == I64_MIN   # (the never-written source)
        gt.check_export_equals(dst, odst, cap, 0)            # dst's own mark covers every stored row
        gt.check_export_equals(dst, odst, cap, I64_MIN)
        dst.close()
    close(*srcs)


# ------------------------------------------------------------------ 4. a negative first stamp
def test_negative_first_stamp(gpu_device):
    """dst's canonical is negative and source 0's selection lies below it: R_0 = C_0 < 0, so step 0's winners
    are stored INVISIBLE, and source 1 wins every one of those rows whatever its clock."""
    n_rows = 2 * T + 9
    c0 = -(1 << 40)
    rng = np.random.default_rng(5)
    ids = np.arange(n_rows, dtype=np.uint32)
    mk = lambda lt, mod: {"ids": ids, "lt": lt.astype(np.int64), "rank": rng.integers(0, 6, n_rows).astype(np.uint32),  # noqa: E731
                          "val": rng.integers(0, 1 << 20, n_rows).astype(np.uint32),
                          "mod": np.full(n_rows, mod, np.int64)}
    drows = mk(c0 - (1 << 30) - rng.integers(0, 1000, n_rows), 5)
    s0 = mk(c0 - (1 << 20) - rng.integers(0, 1000, n_rows), 5)          # newer than dst, below C_0
    s1 = mk(c0 - (1 << 35) - rng.integers(0, 1000, n_rows), 5)          # older than both
    s0["mod"][::3] = -7                                                  # (not selected by since 0)
    srcs, osrcs = load_sources([s0, s1], n_rows, [32, 24])
    dst, odst = load_dst(drows, n_rows, canonical=c0)
    m, res, omask = check_fanin(dst, odst, srcs, osrcs, n_rows, [0, 0], MW, "negative stamp", fused=True)
    assert m["stamps"][0] == c0 < 0 < m["stamps"][1] == MW << 16
    sel0 = s0["mod"] >= 0
    assert np.array_equal(omask, np.where(sel0, 3, 0).astype(np.uint8))   # lost where dst stayed visible
    assert res[0]["n_won"] == res[1]["n_won"] == int(sel0.sum()) and res[1]["n_present"] == int((~sel0).sum())
    close(dst, *srcs)


# ------------------------------------------------------------------ 5. fallbacks
N_EXC = 3 * T + 17


def exc_tables(n_src, planted=None, canonical=None):
    """``planted`` = {source index: {id: (lt, rank)}}: rows selected by since = 0."""
    rows = [fc.source_rows(N_EXC, j) for j in range(n_src)]
    for j, p in (planted or {}).items():
        for k, (lt, rank) in p.items():
            tc._plant(rows[j], {k: (lt, rank, 77, tc.TOP)})
    srcs, osrcs = load_sources(rows, N_EXC)
    dst, odst = load_dst(fc.dst_rows(N_EXC), N_EXC, canonical=canonical)
    return srcs, osrcs, dst, odst


def written_id(j, pos):
    d = tc.dense(fc.source_rows(N_EXC, j), N_EXC)
    return int(np.flatnonzero(d["mod"] >= 0)[pos])


@pytest.mark.parametrize("k", [0, 2])
@pytest.mark.parametrize("kind", ["duplicate", "drift"])
def test_a_row_raises_in_source_k(gpu_device, k, kind):
    at = written_id(k, T + 3)
    row = (DUP_LT, fc.DST_RANK) if kind == "duplicate" else (DRIFT_LT, 2)
    srcs, osrcs, dst, odst = exc_tables(5, {k: {at: row}})
    m, res, omask = check_fanin(dst, odst, srcs, osrcs, N_EXC, [0] * 5, MW, (kind, k), fused=False)
    want = _capi.CRDT_DUPLICATE_NODE if kind == "duplicate" else _capi.CRDT_CLOCK_DRIFT
    assert m["may_raise"] and [r["status"] for r in res] == [0] * k + [want] + [0] * (4 - k)
    assert res[k]["n_stored"] == 0 and res[k]["exc_index"] < U64_MAX and res[k]["n_won"] == 0
    for j in range(k):
        assert res[j]["n_won"] == int(((omask >> j) & 1).sum()) > 0      # the steps before stay merged
    for j in range(k + 1, 5):
        assert res[j] == dict(CLEARED, canonical_lt=dst.canonical)
    assert not (omask >> k).any()
    close(dst, *srcs)


def test_candidate_against_c0_that_no_step_raises(gpu_device):
    """A row of dst's own node id just above C_0 in source 2: by then the running canonical has passed it, so
    recv() returns early and nothing raises — but the kernels' rule is taken against C_0: the composition."""
    at = written_id(2, 2 * T + 1)
    srcs, osrcs, dst, odst = exc_tables(4, {2: {at: (sc.canon0() + 1, fc.DST_RANK)}})
    m, res, omask = check_fanin(dst, odst, srcs, osrcs, N_EXC, [0] * 4, MW, "candidate", fused=False)
    assert m["may_raise"] and [r["status"] for r in res] == [0] * 4 and all(r["n_won"] > 0 for r in res)
    close(dst, *srcs)


def test_selected_id_beyond_dst_capacity(gpu_device):
    dcap = 2 * T + 5
    rows = [fc.source_rows(N_EXC, j) for j in range(3)]
    lo, hi = int(tc.STAMPS[2]), int(tc.STAMPS[30])
    for j, r in enumerate(rows):                             # only source 1 selects a row at or above dst's capacity
        r["clear"] = (0, 0)
        above = r["ids"] >= dcap
        r["mod"] = np.where(above, lo, np.where(r["mod"] >= 0, hi, r["mod"])).astype(np.int64)
        if j == 1:
            r["mod"][np.flatnonzero(above)[3]] = hi
    srcs, osrcs = load_sources(rows, N_EXC)
    dst, odst = load_dst(fc.dst_rows(dcap), dcap)
    assert dst.capacity == dcap
    _, flags0, _ = gt.oracle_merge_table(odst, osrcs[0], N_EXC, hi, MW)     # step 0 stays merged
    mask = np.full(N_EXC, 9, np.uint8)
    with pytest.raises(CrdtNativeError) as e:
        dst.merge_tables(srcs, N_EXC, [hi] * 3, MW, win_mask=mask)
    assert e.value.status == _capi.CRDT_E_KEY_RANGE
    gt.assert_rows(dst, odst, "step 0 merged, step 1 stored nothing")
    assert np.array_equal(mask, flags0) and flags0.any() and not dst.last_plan()["fanin"]
    close(dst, *srcs)


def test_middle_send_overflows(gpu_device):
    """C_0 = (wall + 5 ms, counter 0xFFFE): step 0's send reaches 0xFFFF, step 1's overflows after its store."""
    c0 = ((MW + 5) << 16) | 0xFFFE
    srcs, osrcs, dst, odst = exc_tables(4, canonical=c0)
    m, res, omask = check_fanin(dst, odst, srcs, osrcs, N_EXC, [0] * 4, MW, "overflow", fused=False)
    assert m["statuses"] == [0, 3] and [r["status"] for r in res] == [0, _capi.CRDT_OVERFLOW, 0, 0]
    assert res[1]["n_stored"] == 1 and res[1]["counter"] == 0x10000 and res[1]["exc_index"] == U64_MAX
    assert res[1]["n_won"] == int(((omask >> 1) & 1).sum()) > 0 and dst.canonical == c0 + 1
    assert res[2] == res[3] == dict(CLEARED, canonical_lt=c0 + 1) and not (omask >> 2).any()
    close(dst, *srcs)


def test_dst_among_its_sources(gpu_device):
    srcs, osrcs, dst, odst = exc_tables(2)
    m, res, omask = check_fanin(dst, odst, [srcs[0], dst, srcs[1]], [osrcs[0], odst, osrcs[1]], N_EXC, [0, 0, 0], MW,
                                "self", fused=False)
    assert [r["status"] for r in res] == [0, 0, 0] and res[1]["n_won"] == 0 and res[1]["n_present"] > 0
    assert res[0]["n_won"] > 0 and res[2]["n_won"] > 0
    close(dst, *srcs)


def test_dst_pinned_to_sorted(gpu_device):
    srcs, osrcs, dst, odst = exc_tables(3)
    dst.set_merge_path("sorted")
    m, res, omask = check_fanin(dst, odst, srcs, osrcs, N_EXC, [0, 0, 0], MW, "sorted", fused=False)
    assert m["fused"] and all(r["n_won"] > 0 for r in res)  # (only the pin kept it from the fused form)
    close(dst, *srcs)


# ------------------------------------------------------------------ 6. mask memory
@pytest.mark.parametrize("kind", ["host", "device_view", "none"])
def test_mask_memory(gpu_device, kind):
    import torch
    n_rows = 3 * T + 17
    srcs, osrcs = load_sources([fc.source_rows(n_rows, j) for j in range(3)], n_rows)
    for sinces, fused in (([0, 0, 0], True), ([tc.TOP + 1, tc.TOP, tc.TOP + 1], True), ([0, 0, 0], False)):
        dst, odst = load_dst(fc.dst_rows(n_rows), n_rows)
        if not fused:
            dst.set_merge_path("sorted")                     # the composition fills the mask the same way
        tag = (kind, sinces, fused)
        if kind == "host":
            check_fanin(dst, odst, srcs, osrcs, n_rows, sinces, MW, tag, fused=fused, win_mask=np.full(n_rows, 9, np.uint8))
        elif kind == "device_view":
            buf = torch.full((1 + n_rows + 16,), 9, dtype=torch.uint8, device="cuda:0")
            check_fanin(dst, odst, srcs, osrcs, n_rows, sinces, MW, tag, fused=fused, win_mask=buf[1:1 + n_rows])
            got = buf.cpu().numpy()
            assert got[0] == 9 and np.all(got[1 + n_rows:] == 9), tag     # nothing outside [0, n_rows) written
        else:
            check_fanin(dst, odst, srcs, osrcs, n_rows, sinces, MW, tag, fused=fused, win_mask=False)
        dst.close()
    close(*srcs)


# ------------------------------------------------------------------ 7. more tiles than the clock pass's grid
def test_more_tiles_than_the_clock_grid(gpu_device):
    n_rows = (GRID + 1) * T + 5
    srcs, osrcs = load_sources([fc.source_rows(n_rows, j) for j in range(2)], n_rows)
    dst, odst = load_dst(fc.dst_rows(n_rows), n_rows)
    m, res, omask = check_fanin(dst, odst, srcs, osrcs, n_rows, [0, 0], MW, "grid", fused=True)
    assert res[0]["n_won"] > n_rows // 4 and res[1]["n_won"] > n_rows // 8 and (omask == 3).any()
    close(dst, *srcs)


# ------------------------------------------------------------------ 8. scratch reuse on one dst ctx
def test_scratch_reuse(gpu_device):
    cap = 3 * T + 17
    dst = DeviceTable(0, local_rank=fc.DST_RANK, capacity=cap)
    other = DeviceTable(0, local_rank=sc.B_RANK, capacity=cap)
    srcs, osrcs = load_sources([fc.source_rows(cap, j) for j in range(8)], cap)
    small, osmall = load_sources([fc.source_rows(T - 1, j) for j in range(2)], cap)
    c0 = sc.canon0()
    odst = gs.reset(dst, fc.dst_rows(cap), c0)
    check_fanin(dst, odst, srcs, osrcs, cap, [0] * 8, MW, "fan-in of 8", fused=True)
    odst = gs.reset(dst, fc.dst_rows(cap), c0)
    gt.check(dst, odst, srcs[3], osrcs[3], cap, 0, MW, "merge_table")
    odst = gs.reset(dst, fc.dst_rows(cap), c0)
    oother = gs.reset(other, fc.source_rows(cap, 9), sc.C_B)
    gs.check_sync(dst, odst, other, oother, cap, 0, 0, MW, "sync_tables", fused=True)
    odst = gs.reset(dst, fc.dst_rows(T - 1), c0)
    check_fanin(dst, odst, small, osmall, T - 1, [0, sc.mid()], MW, "fan-in of 2", fused=True)
    odst = gs.reset(dst, fc.dst_rows(cap), c0)
    check_fanin(dst, odst, srcs, osrcs, cap, fc.since_vectors(8)["mixed"], MW, "fan-in of 8 again", fused=True)
    close(dst, other, *srcs, *small)


# ------------------------------------------------------------------ 9. refusals
def test_refusals(gpu_device):
    n_rows = T + 5
    srcs, osrcs = load_sources([fc.source_rows(n_rows, j) for j in range(2)], n_rows)
    dst, odst = load_dst(fc.dst_rows(n_rows), n_rows)
    mask = np.full(n_rows + 1, 9, np.uint8)

    def refused(tables, n, sinces):
        with pytest.raises(CrdtNativeError) as e:
            dst.merge_tables(tables, n, sinces, MW, win_mask=mask)
        assert e.value.status == _capi.CRDT_E_INVALID
        gt.assert_rows(dst, odst, "dst untouched")
        for s, o in zip(srcs, osrcs):
            gt.assert_rows(s, o, "source untouched")
        assert np.all(mask == 9)

    refused([], n_rows, [])
    refused([srcs[j % 2] for j in range(9)], n_rows, [0] * 9)
    big = DeviceTable(0, local_rank=3, capacity=2 * n_rows)          # n_rows above ONE source's capacity
    refused([big, srcs[0]], n_rows + 1, [0, 0])
    refused([srcs[0], big, srcs[1]], n_rows + 1, [0, 0, 0])
    from tests._loopback import LoopbackComm
    joined = DeviceTable(0, local_rank=4, capacity=n_rows)
    joined.comm_init_ops(2, 0, LoopbackComm(2))                      # rank 0 of a loopback communicator
    refused([srcs[0], joined], n_rows, [0, 0])
    other = DeviceTable(0, capacity=16)
    other.device = 1                                                 # (as if it had been created on another GPU)
    with pytest.raises(ValueError):
        dst.merge_tables([srcs[0], other], 16, [0, 0], MW)
    other.device = 0
    with pytest.raises(ValueError):
        dst.merge_tables(srcs, n_rows, [0], MW)
    check_fanin(dst, odst, srcs, osrcs, n_rows, [0, 0], MW, "after the refusals", fused=True)
    close(dst, big, joined, other, *srcs)
