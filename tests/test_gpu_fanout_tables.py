"""crdt_fanout_tables (DeviceTable.fanout_tables, called on the source): one replica merged into up to eight
tables, decided on one read of it, against its contract: the sequence of table merges on the C restatement
(oracle_fanout of tests/_fanout_cases.py, ending at the first step that raises).  Where the numpy model of
tests/_fanout_cases.py says the fused conditions hold, EVERY destination must report the plan table|fanout, and
nowhere else.  Everything is integer data: every comparison is exact."""
import numpy as np
import pytest

import tests.test_gpu_fanin_tables as gf
import tests.test_gpu_sync_tables as gs
import tests.test_gpu_table_merge as gt
from crdt_amd import CrdtNativeError, DeviceTable, _capi
from tests import _fanin_cases as fc
from tests import _fanout_cases as fo
from tests import _sync_cases as sc
from tests import _table_cases as tc
from tests._cases import NULL

pytestmark = pytest.mark.gpu

T = _capi.TABLE_TILE
GRID = _capi.TABLE_CLOCK_GRID
I64_MIN = tc.I64_MIN
U64_MAX = (1 << 64) - 1
MW = tc.MERGE_WALL
RESULT_FIELDS = gt.RESULT_FIELDS
COLS = fo.COLS
DRIFT_LT = gt.DRIFT_LT
DUP_LT = (MW + 10) << 16                 # above every canonical of a call at MW, within the drift bound
CLEARED = tc.CLEARED


def close(*tables):
    for t in {id(t): t for t in tables}.values():
        t.close()


def load_src(rows, cap, stride=24):
    return gt.load(rows, cap, stride, local_rank=fo.SRC_RANK, canonical=100)


def load_dsts(rows_list, caps, strides=None, setting="mid", canons=None):
    n = len(rows_list)
    caps = [caps] * n if isinstance(caps, int) else caps
    canons = [fo.canonical(setting, j) for j in range(n)] if canons is None else canons
    out = [gt.load(rows, caps[j], (strides or [24] * n)[j], local_rank=fo.dst_rank(j), canonical=canons[j])
           for j, rows in enumerate(rows_list)]
    return [t for t, _ in out], [o for _, o in out]


def check_fanout(src, osrc, dsts, odsts, n_rows, sinces, wall, tag, fused="model", win_mask=True):
    """One fanout_tables against the oracle: every result field by field, every destination's rows and
    canonical, the mask, the source's rows / canonical / plan / export view untouched, and the plan of every
    destination.  ``fused``: "model" -> what the numpy model says of the tables as they are; True / False ->
    that; None -> not checked.  Returns (model, results, mask)."""
    own = any(d is src for d in dsts)
    twice = len({id(d) for d in dsts}) < len(dsts)
    m = fo.model({k: osrc.rows[k].copy() for k in COLS}, [{k: o.rows[k].copy() for k in COLS} for o in odsts],
                 n_rows, sinces, [o.canonical for o in odsts], wall, ranks=[d.local_rank for d in dsts],
                 caps=[d.capacity for d in dsts])
    before = (osrc.rows.copy(), osrc.canonical)
    view, view_ids, src_plan = None, None, None
    if not own:
        if n_rows:
            view_ids = osrc.modified_since(n_rows, 0)
            view = src.export_since(n_rows, 0)
        src_plan = src.last_plan()
    ores, omask, stop = fo.oracle_fanout(osrc, odsts, n_rows, sinces, wall)
    if not own and not twice and not any(m["may_raise"]) and not any(m["out_of_range"]):
        # the model is exact here (up to the stop): it must agree with the oracle before either judges the library
        upto = len(dsts) if stop is None else stop + 1
        keep = np.uint8((1 << upto) - 1)
        assert np.array_equal(omask, m["mask"] & keep), tag
        assert [r["n_present"] for r in ores[:upto]] == m["n_present"][:upto], tag
        assert [r["status"] for r in ores[:upto]] == m["statuses"][:upto], tag
        assert all(o.canonical == c for o, c, st in zip(odsts[:upto], m["canonical"], m["statuses"]) if st == 0), tag
    res, mask = src.fanout_tables(dsts, n_rows, sinces, wall, win_mask=win_mask)
    assert len(res) == len(dsts)
    for j, (r, o) in enumerate(zip(res, ores)):
        for f in RESULT_FIELDS:
            assert r[f] == o[f], (tag, j, f, r[f], o[f])
    for j, (d, o) in enumerate(zip(dsts, odsts)):
        gt.assert_rows(d, o, (tag, "destination", j))
    if win_mask is not False:
        got = mask.cpu().numpy() if hasattr(mask, "cpu") else np.asarray(mask)
        assert len(got) >= n_rows and np.array_equal(got[:n_rows], omask), (tag, "mask")
        if stop is not None:
            assert not (omask >> (stop + 1)).any(), (tag, "no bit above the stop")
    if not own:
        assert np.array_equal(osrc.rows, before[0]) and osrc.canonical == before[1]
        gt.assert_rows(src, osrc, (tag, "source untouched"))
        assert src.last_plan() == src_plan, (tag, "the source's plan")
        if view is not None:                                   # its export view, taken before the call, still reads
            key, lt, rank, val, mod = view.columns()
            assert np.array_equal(key, view_ids), (tag, "view")
            for name, got in (("lt", lt), ("rank", rank), ("val", val), ("mod", mod)):
                assert np.array_equal(got, osrc.rows[name][view_ids]), (tag, "view", name)
    if fused == "model":
        fused = m["fused"] and not own and not twice
    if fused is not None:
        for j, d in enumerate(dsts):
            plan = d.last_plan()
            assert plan["fanout"] is (fused and len(dsts) > 1), (tag, j, plan)
            if fused:
                assert plan["table"] and not any(v for k, v in plan.items() if k not in ("table", "fanout")), (tag, j, plan)
                assert d.last_path() == "gather"
    return m, res, omask


# ------------------------------------------------------------------ 1. shapes
def run_shapes(n_rows, n_dst, fused="model"):
    cap = max(n_rows, 16)
    srcs = {stride: load_src(fo.source_rows(n_rows), cap, stride) for stride in (24, 32)}
    for setting in fo.CANON_SETTINGS:
        for name, sinces in fo.since_vectors(n_dst).items():
            s_stride, d_strides = fo.strides(n_dst, flip=name in ("mid", "mixed"))
            src, osrc = srcs[s_stride]
            dsts, odsts = load_dsts([fo.dst_rows(n_rows, j) for j in range(n_dst)], cap, d_strides, setting)
            canons = [d.canonical for d in dsts]
            tag = (n_rows, n_dst, setting, name)
            m, res, omask = check_fanout(src, osrc, dsts, odsts, n_rows, sinces, MW, tag, fused=fused)
            assert m["fused"] and [r["status"] for r in res] == [0] * n_dst
            # an empty selection is still one merge() call on that destination: its send moves its canonical
            assert all(r["canonical_lt"] > c and r["n_stored"] == 1 for r, c in zip(res, canons)), tag
            if n_rows >= 63 and name == "zero":
                assert all(r["n_won"] > 0 for r in res)
                assert any(not np.array_equal(m["wins"][0], w) for w in m["wins"][1:])    # the verdicts differ
            close(*dsts)
    close(*(t for t, _ in srcs.values()))


@pytest.mark.parametrize("n_dst", [2, 8])
@pytest.mark.parametrize("n_rows", fo.shapes())
def test_shapes(gpu_device, n_rows, n_dst):
    run_shapes(n_rows, n_dst)


def test_shapes_three_destinations(gpu_device):
    run_shapes(3 * T + 17, 3)


def test_one_destination_is_merge_table(gpu_device):
    n_rows = 3 * T + 17
    src, osrc = load_src(fo.source_rows(n_rows), n_rows)
    dsts, odsts = load_dsts([fo.dst_rows(n_rows, 0)], n_rows)
    m, res, omask = check_fanout(src, osrc, dsts, odsts, n_rows, [0], MW, "one", fused=None)
    plan = dsts[0].last_plan()
    assert plan["table"] and not plan["fanout"] and res[0]["n_won"] == int(omask.sum()) > 0
    assert not any(v for k, v in plan.items() if k != "table")
    close(src, *dsts)


def test_switch_takes_the_composition(gpu_device, monkeypatch):
    monkeypatch.setenv("CRDT_TABLE_MERGE", "0")              # read when the tables are created
    run_shapes(3 * T + 17, 3, fused=False)


# ------------------------------------------------------------------ 2. planted rows: one source row, several verdicts
def test_planted_rows(gpu_device):
    n_rows = 3 * T + 17
    s10, s20, s30, s35 = (int(tc.STAMPS[k]) for k in (10, 20, 30, 35))
    a, b, c, d = 1000, 2 * T - 1, 3 * T + 16, 5              # outside every cleared range (checked by _plant)
    srows = fo.source_rows(n_rows)
    drows = [fo.dst_rows(n_rows, j) for j in range(8)]
    # a: equal (lt, rank) at destination 0 (keeps local), older there at destination 1 (the source wins)
    # b: newer and visible at destination 0 (the source loses), newer but INVISIBLE at destination 1 (it wins)
    # c: a source tombstone: wins over destination 0's older row, loses to destination 1's newer one
    # d: newer than every destination's row: wins at all 8
    tc._plant(srows, {a: (s20, 3, 41, tc.TOP), b: (s20, 2, 42, tc.TOP), c: (s20, 4, NULL, tc.TOP), d: (s35, 5, 44, tc.TOP)})
    tc._plant(drows[0], {a: (s20, 3, 31, s10), b: (s30, 5, 32, s10), c: (s10, 1, 33, s10), d: (s10, 0, 34, s10)})
    tc._plant(drows[1], {a: (s10, 2, 51, s10), b: (s30, 5, 52, -(1 << 20)), c: (s30, 1, 53, s10), d: (s10, 0, 54, s10)})
    for j in range(2, 8):
        tc._plant(drows[j], {d: (s10, 0, 60 + j, s10)})
    src, osrc = load_src(srows, n_rows, 32)
    dsts, odsts = load_dsts(drows, n_rows, fo.strides(8)[1], "top")
    m, res, omask = check_fanout(src, osrc, dsts, odsts, n_rows, [0] * 8, MW, "planted", fused=True)
    assert (omask[a] & 3, omask[b] & 3, omask[c] & 3, omask[d]) == (2, 2, 1, 0xFF)
    ids = np.array([a, b, c, d], np.uint32)
    lt, rank, val, mod = dsts[0].read_rows(ids)
    assert list(val) == [31, 32, NULL, 44] and list(mod) == [s10, s10, m["stamps"][0], m["stamps"][0]]
    lt, rank, val, mod = dsts[1].read_rows(ids)
    assert list(val) == [41, 42, 53, 44] and list(mod) == [m["stamps"][1], m["stamps"][1], s10, m["stamps"][1]]
    for j in range(2, 8):                                    # every destination stamps with its OWN canonical
        lt, rank, val, mod = dsts[j].read_rows(ids[3:])
        assert (int(val[0]), int(mod[0])) == (44, tc.TOP + 1 + j)
    close(src, *dsts)


# ------------------------------------------------------------------ 3. tile patterns, nested selections
@pytest.mark.parametrize("pattern", list(fo.nested_patterns(T, 5 * T + 9)))
def test_tile_patterns(gpu_device, pattern):
    n_rows = 5 * T + 9
    sels = fo.nested_patterns(T, n_rows)[pattern]
    lo, hi = int(tc.STAMPS[2]), int(tc.STAMPS[30])
    srows = sc.select_pattern(n_rows, 41, sels[0], lo, hi)
    srows["mod"], sinces = fo.nested_mods(sels, tc.STAMPS)
    src, osrc = load_src(srows, n_rows)
    dsts, odsts = load_dsts([sc.select_pattern(n_rows, 50 + j, np.zeros(n_rows, bool), lo, hi) for j in range(len(sels))],
                            n_rows, fo.strides(len(sels))[1], "top")
    m, res, omask = check_fanout(src, osrc, dsts, odsts, n_rows, sinces, MW, pattern, fused=True)
    for j, sel in enumerate(sels):
        assert res[j]["n_present"] == int(sel.sum()) and res[j]["n_stored"] == 1
        assert not ((omask >> j) & 1)[~sel].any()
        if sel.any():
            assert 0 < res[j]["n_won"] == int(((omask >> j) & 1).sum())
        assert dsts[j].canonical == MW << 16                 # every destination's own send, selection or not
    if pattern == "none":
        assert not omask.any()
    close(src, *dsts)


def test_mixed_row_bounds(gpu_device):
    """One destination's since is I64_MIN, which selects the never-written fill above the source's high-water
    mark too, the others' 0: the clock pass covers the largest bound, each destination's bits end at its own."""
    w = T + 5
    cap = 4 * w
    src, osrc = load_src(fo.source_rows(2 * w + 1), cap)
    for sinces in ([0, I64_MIN, 0], [I64_MIN, 0, -1]):
        dsts, odsts = load_dsts([fo.dst_rows(x, j) for j, x in enumerate([w, 3 * w, 2 * w])], cap, [24, 32, 24])
        m, res, omask = check_fanout(src, osrc, dsts, odsts, cap, sinces, MW, ("bounds", sinces), fused=True)
        for j, since in enumerate(sinces):
            bit = (omask >> j) & 1
            assert res[j]["n_won"] == int(bit.sum()) > 0
            if since == I64_MIN:
                assert res[j]["n_present"] + res[j]["n_won"] >= cap - 3 * w     # (the fill rows count as selected)
            else:
                assert not bit[2 * w + 1:].any()             # nothing selected above the source's mark
            gt.check_export_equals(dsts[j], odsts[j], cap, 0)        # its own mark covers every stored row
            gt.check_export_equals(dsts[j], odsts[j], cap, I64_MIN)
        close(*dsts)
    src.close()


def test_more_tiles_than_the_clock_grid(gpu_device):
    """k_fo_clock strides a grid of TABLE_CLOCK_GRID workgroups: a sparse selection in the first tile, a middle
    one, the tiles that the first workgroups take on their second round, and the last row."""
    n_rows = (GRID + 3) * T + 5
    z = lambda: np.zeros(n_rows, bool)  # noqa: E731
    wide, narrow = z(), z()
    for first in (3, (GRID // 2) * T + 7, GRID * T + 1, (GRID + 1) * T + 900, n_rows - 5):
        wide[first:first + 4] = True
    narrow[(GRID // 2) * T + 8] = narrow[GRID * T + 2] = narrow[n_rows - 1] = True
    lo, hi = int(tc.STAMPS[2]), int(tc.STAMPS[30])
    srows = sc.select_pattern(n_rows, 43, wide, lo, hi)
    srows["mod"], sinces = fo.nested_mods([wide | narrow, narrow], tc.STAMPS)
    src, osrc = load_src(srows, n_rows)
    dsts, odsts = load_dsts([sc.select_pattern(n_rows, 60 + j, z(), lo, int(tc.STAMPS[0])) for j in range(2)], n_rows,
                            [32, 24], "top")
    m, res, omask = check_fanout(src, osrc, dsts, odsts, n_rows, sinces, MW, "grid", fused=True)
    assert [r["n_present"] for r in res] == [int((wide | narrow).sum()), 3]
    assert res[0]["n_won"] == int((omask & 1).sum()) > 0 and not omask[~(wide | narrow)].any()
    close(src, *dsts)


# ------------------------------------------------------------------ 4. fallbacks
N_EXC = 3 * T + 17


def exc_tables(n_dst, planted=None, canons=None, caps=None):
    """``planted`` = {id: (lt, rank)}: source rows selected by since = 0."""
    srows = fo.source_rows(N_EXC)
    for k, (lt, rank) in (planted or {}).items():
        tc._plant(srows, {k: (lt, rank, 77, tc.TOP)})
    src, osrc = load_src(srows, N_EXC)
    caps = caps or [N_EXC] * n_dst
    dsts, odsts = load_dsts([fo.dst_rows(min(N_EXC, caps[j]), j) for j in range(n_dst)], caps, canons=canons)
    return src, osrc, dsts, odsts


def written_id(pos):
    d = tc.dense(fo.source_rows(N_EXC), N_EXC)
    return int(np.flatnonzero(d["mod"] >= 0)[pos])


def test_duplicate_node_at_destination_1(gpu_device):
    """A source row of destination 1's own node id above its canonical: its recv() raises.  Destination 0 (for
    which the row is an ordinary one) stays merged, destination 2 is untouched."""
    at = written_id(T + 3)
    src, osrc, dsts, odsts = exc_tables(3, {at: (DUP_LT, fo.dst_rank(1))})
    c2 = dsts[2].canonical
    m, res, omask = check_fanout(src, osrc, dsts, odsts, N_EXC, [0] * 3, MW, "duplicate", fused=False)
    assert m["may_raise"] == [False, True, False]
    assert [r["status"] for r in res] == [0, _capi.CRDT_DUPLICATE_NODE, 0]
    assert res[0]["n_won"] == int((omask & 1).sum()) > 0 and omask[at] == 1
    assert res[1]["n_stored"] == 0 and res[1]["exc_index"] < U64_MAX and res[1]["n_won"] == 0
    assert res[2] == dict(CLEARED, canonical_lt=c2) and dsts[2].canonical == c2
    assert not (omask >> 1).any()
    close(src, *dsts)


def test_clock_drift_at_destination_0(gpu_device):
    at = written_id(2 * T + 1)
    src, osrc, dsts, odsts = exc_tables(3, {at: (DRIFT_LT, 2)})
    canons = [d.canonical for d in dsts]
    m, res, omask = check_fanout(src, osrc, dsts, odsts, N_EXC, [0] * 3, MW, "drift", fused=False)
    assert all(m["may_raise"]) and [r["status"] for r in res] == [_capi.CRDT_CLOCK_DRIFT, 0, 0]
    assert res[0]["n_stored"] == 0 and res[0]["n_won"] == 0 and not omask.any()
    assert [res[k] for k in (1, 2)] == [dict(CLEARED, canonical_lt=canons[k]) for k in (1, 2)]
    assert [d.canonical for d in dsts[1:]] == canons[1:]      # nothing merged after the stop
    close(src, *dsts)


def test_selected_id_beyond_destination_1(gpu_device):
    dcap = 2 * T + 5
    src, osrc, dsts, odsts = exc_tables(3, caps=[N_EXC, dcap, N_EXC])
    assert [d.capacity for d in dsts] == [N_EXC, dcap, N_EXC]
    _, flags0, ids = gt.oracle_merge_table(odsts[0], osrc, N_EXC, 0, MW)    # step 0 stays merged
    assert ids.max() >= dcap
    mask = np.full(N_EXC, 9, np.uint8)
    with pytest.raises(CrdtNativeError) as e:
        src.fanout_tables(dsts, N_EXC, [0] * 3, MW, win_mask=mask)
    assert e.value.status == _capi.CRDT_E_KEY_RANGE
    for j, (d, o) in enumerate(zip(dsts, odsts)):
        gt.assert_rows(d, o, ("step 0 merged, step 1 stored nothing, step 2 not run", j))
    gt.assert_rows(src, osrc, "source untouched")
    assert np.array_equal(mask, flags0) and flags0.any() and not any(d.last_plan()["fanout"] for d in dsts)
    close(src, *dsts)


def test_send_overflows_at_destination_1(gpu_device):
    """Destination 1's canonical is (wall + 5 ms, counter 0xFFFF): its send overflows after its store, and the
    sequence ends there as the composition's does."""
    c1 = ((MW + 5) << 16) | 0xFFFF
    canons = [fo.canonical("mid", 0), c1, fo.canonical("mid", 2)]
    src, osrc, dsts, odsts = exc_tables(3, canons=canons)
    m, res, omask = check_fanout(src, osrc, dsts, odsts, N_EXC, [0] * 3, MW, "overflow", fused=False)
    assert m["statuses"] == [0, 3, 0] and not any(m["may_raise"])
    assert [r["status"] for r in res] == [0, _capi.CRDT_OVERFLOW, 0]
    assert res[1]["n_stored"] == 1 and res[1]["counter"] == 0x10000 and res[1]["exc_index"] == U64_MAX
    assert res[1]["n_won"] == int(((omask >> 1) & 1).sum()) > 0 and dsts[1].canonical == c1
    assert res[2] == dict(CLEARED, canonical_lt=canons[2]) and not (omask >> 2).any()
    close(src, *dsts)


def test_source_among_the_destinations(gpu_device):
    src, osrc, dsts, odsts = exc_tables(2)
    m, res, omask = check_fanout(src, osrc, [dsts[0], src, dsts[1]], [odsts[0], osrc, odsts[1]], N_EXC, [0, 0, 0], MW,
                                 "self", fused=False)
    assert [r["status"] for r in res] == [0, 0, 0] and res[1]["n_won"] == 0 and res[1]["n_present"] > 0
    assert res[0]["n_won"] > 0 and res[2]["n_won"] > 0 and not (omask & 2).any()
    close(src, *dsts)


def test_destination_listed_twice(gpu_device):
    src, osrc, dsts, odsts = exc_tables(2)
    c0 = dsts[0].canonical
    order = [0, 1, 0]
    m, res, omask = check_fanout(src, osrc, [dsts[k] for k in order], [odsts[k] for k in order], N_EXC, [0, 0, 0], MW,
                                 "twice", fused=False)
    assert res[0]["n_won"] > 0 and res[1]["n_won"] > 0 and res[2]["n_won"] == 0 and not (omask & 4).any()
    assert res[2]["n_present"] > res[0]["n_present"] and c0 < res[0]["canonical_lt"] < res[2]["canonical_lt"]
    close(src, *dsts)


def test_destination_pinned_to_sorted(gpu_device):
    src, osrc, dsts, odsts = exc_tables(3)
    dsts[1].set_merge_path("sorted")
    m, res, omask = check_fanout(src, osrc, dsts, odsts, N_EXC, [0, 0, 0], MW, "sorted", fused=False)
    assert m["fused"] and all(r["n_won"] > 0 for r in res)   # (only the pin kept it from the fused form)
    assert dsts[0].last_plan()["table"] and not dsts[1].last_plan()["table"]    # each its own merge_table's plan
    close(src, *dsts)


# ------------------------------------------------------------------ 5. mask memory
def test_mask_memory(gpu_device):
    import torch
    n_rows = 3 * T + 17
    src, osrc = load_src(fo.source_rows(n_rows), n_rows)
    for sinces, fused in (([0, 0, 0], True), ([tc.TOP + 1, tc.TOP, tc.TOP + 1], True), ([0, 0, 0], False)):
        seen = []
        for kind in ("host", "device_view", "none"):
            dsts, odsts = load_dsts([fo.dst_rows(n_rows, j) for j in range(3)], n_rows, [24, 32, 24])
            if not fused:
                dsts[2].set_merge_path("sorted")             # the composition fills the mask the same way
            tag = (kind, sinces, fused)
            if kind == "host":
                arr = np.full(n_rows, 9, np.uint8)
                m, res, omask = check_fanout(src, osrc, dsts, odsts, n_rows, sinces, MW, tag, fused=fused, win_mask=arr)
                seen.append(arr.copy())
            elif kind == "device_view":
                buf = torch.full((1 + n_rows + 16,), 9, dtype=torch.uint8, device="cuda:0")
                m, res, omask = check_fanout(src, osrc, dsts, odsts, n_rows, sinces, MW, tag, fused=fused,
                                             win_mask=buf[1:1 + n_rows])
                got = buf.cpu().numpy()
                assert got[0] == 9 and np.all(got[1 + n_rows:] == 9), tag     # nothing outside [0, n_rows) written
                seen.append(got[1:1 + n_rows])
            else:                                            # (check_fanout compares the rows it leaves with the oracle's)
                m, res, omask = check_fanout(src, osrc, dsts, odsts, n_rows, sinces, MW, tag, fused=fused, win_mask=False)
            seen.append(res)
            close(*dsts)
        assert np.array_equal(seen[0], seen[2]) and seen[1] == seen[3] == seen[4], (sinces, fused)
        assert seen[0].any() or sinces[0] != 0
    src.close()


# ------------------------------------------------------------------ 6. scratch reuse on one dsts[0] ctx
@pytest.mark.parametrize("order", ["fanin_first", "fanout_first"])
def test_scratch_reuse(gpu_device, order):
    """crdt_fanin_tables into a table and crdt_fanout_tables with that table first share its t_words / t_sel /
    t_mask (and the count words): either order leaves the oracle's rows."""
    cap = 3 * T + 17
    d0 = DeviceTable(0, local_rank=fc.DST_RANK, capacity=cap)
    od0 = gs.reset(d0, fc.dst_rows(cap), sc.canon0())
    ins, oins = gf.load_sources([fc.source_rows(cap, j) for j in range(8)], cap)
    src, osrc = load_src(fo.source_rows(cap), cap, 32)
    others, oothers = load_dsts([fo.dst_rows(cap, j) for j in range(1, 4)], cap, [32, 24, 32], "top",
                                canons=[fo.canonical("top", j) for j in range(1, 4)])

    def fanin(tag):
        gf.check_fanin(d0, od0, ins, oins, cap, fc.since_vectors(8)["mixed"], MW, tag, fused=True)

    def fanout(tag):
        check_fanout(src, osrc, [d0] + others, [od0] + oothers, cap, [0, sc.mid(), 0, -1], MW, tag, fused=True)

    for step in ((fanin, fanout, fanin) if order == "fanin_first" else (fanout, fanin, fanout)):
        step((order, step.__name__))
    close(d0, src, *ins, *others)


# ------------------------------------------------------------------ 7. refusals
def test_refusals(gpu_device):
    n_rows = T + 5
    src, osrc = load_src(fo.source_rows(n_rows), n_rows)
    dsts, odsts = load_dsts([fo.dst_rows(n_rows, j) for j in range(2)], 2 * n_rows)
    mask = np.full(2 * n_rows, 9, np.uint8)

    def refused(tables, n, sinces):
        with pytest.raises(CrdtNativeError) as e:
            src.fanout_tables(tables, n, sinces, MW, win_mask=mask)
        assert e.value.status == _capi.CRDT_E_INVALID
        gt.assert_rows(src, osrc, "source untouched")
        for d, o in zip(dsts, odsts):
            gt.assert_rows(d, o, "destination untouched")
        assert np.all(mask == 9)

    refused([], n_rows, [])
    refused([dsts[j % 2] for j in range(9)], n_rows, [0] * 9)
    refused(dsts, src.capacity + 1, [0, 0])                  # n_rows above the SOURCE's capacity
    from tests._loopback import LoopbackComm
    joined = DeviceTable(0, local_rank=4, capacity=n_rows)
    joined.comm_init_ops(2, 0, LoopbackComm(2))              # rank 0 of a loopback communicator
    refused([dsts[0], joined], n_rows, [0, 0])
    other = DeviceTable(0, capacity=16)
    other.device = 1                                         # (as if it had been created on another GPU)
    with pytest.raises(ValueError):
        src.fanout_tables([dsts[0], other], 16, [0, 0], MW)
    other.device = 0
    with pytest.raises(ValueError):
        src.fanout_tables(dsts, n_rows, [0], MW)
    check_fanout(src, osrc, dsts, odsts, n_rows, [0, 0], MW, "after the refusals", fused=True)
    close(src, joined, other, *dsts)
