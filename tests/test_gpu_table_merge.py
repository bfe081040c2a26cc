"""crdt_merge_table (DeviceTable.merge_table): dst.merge(src.recordMap(modifiedSince)) between two tables
of one device in two streaming passes, against the composition on the C restatement: the oracle's
modified_since, then its merge of that one changeset, the win flags carried to their row ids.
Everything is integer data: every comparison is exact."""
import numpy as np
import pytest

import tests.test_gpu_export as gx
from crdt_amd import CrdtNativeError, DeviceTable, _capi
from oracle.oracle_c import OracleTable, new_table
from tests import _table_cases as tc
from tests._cases import NULL, WALL

pytestmark = pytest.mark.gpu

T = _capi.TABLE_TILE                    # rows per workgroup of both passes
GRID = _capi.TABLE_CLOCK_GRID           # workgroups of the clock pass: more tiles than this and each strides
I64_MIN = tc.I64_MIN
U64_MAX = (1 << 64) - 1
MW = tc.MERGE_WALL
RESULT_FIELDS = gx.RESULT_FIELDS
STRIDES = [(24, 24), (24, 32), (32, 24), (32, 32)]


def load(rows: dict, capacity: int, row_bytes: int = 24, local_rank: int = 0, canonical: int = 0):
    """The rows in a DeviceTable and in its OracleTable mirror."""
    t = DeviceTable(0, local_rank=local_rank, capacity=capacity)
    if row_bytes != 24:
        t.set_row_bytes(row_bytes)
    o = OracleTable(t.capacity, local_rank, canonical)
    cols = tuple(rows[k] for k in ("ids", "lt", "rank", "val", "mod"))
    if len(cols[0]):
        t.put_rows(*cols)
        o.put_rows(*cols)
    first, count = rows.get("clear", (0, 0))
    if count:
        t.clear_rows(first, count)
        o.rows[first:first + count] = new_table(count)
    t.canonical = canonical
    return t, o


def read_all(t: DeviceTable):
    return t.read_rows(np.arange(t.capacity, dtype=np.uint32))


def assert_rows(t: DeviceTable, o: OracleTable, tag):
    for name, a in zip(("lt", "rank", "val", "mod"), read_all(t)):
        assert np.array_equal(a, o.rows[name]), (tag, name)
    assert t.canonical == o.canonical, tag


oracle_merge_table = tc.oracle_merge_table         # (the contract on the oracle: tests/_table_cases.py)


def check(dst, odst, src, osrc, n_rows, since, wall, tag, table=True, row_flags=True):
    """One merge_table against the oracle: every result field, dst's rows and canonical, the row flags,
    src untouched, and the plan."""
    src_before, src_canon = osrc.rows.copy(), osrc.canonical
    ores, oflags, ids = oracle_merge_table(odst, osrc, n_rows, since, wall)
    res, flags = dst.merge_table(src, n_rows, since, wall, row_flags=row_flags)
    for f in RESULT_FIELDS:
        assert res[f] == ores[f], (tag, f, res[f], ores[f])
    assert_rows(dst, odst, tag)
    if row_flags is True:
        assert str(flags.device) == "cuda:0" and len(flags) == n_rows, tag
        assert np.array_equal(flags.cpu().numpy(), oflags), tag
    if src is not dst:
        assert np.array_equal(osrc.rows, src_before) and osrc.canonical == src_canon
        assert_rows(src, osrc, (tag, "src untouched"))
    if table is not None:
        plan = dst.last_plan()
        assert plan["table"] is table, (tag, plan)
        if table:
            assert not any(v for k, v in plan.items() if k != "table"), (tag, plan)
            assert dst.last_path() == "gather"
    return res, oflags, ids


def canon0() -> int:
    return int(np.sort(tc.STAMPS)[tc.N_STAMPS // 2]) + 1      # some selected lts above it, some below


# ------------------------------------------------------------------ 1. shapes
def run_shapes(n_rows, strides, table):
    sb, db = strides
    srows, drows = tc.gen_pair(n_rows, seed=3000 + n_rows)
    src, osrc = load(srows, max(n_rows, 16), sb, local_rank=1, canonical=123)
    for since in tc.sinces():
        if n_rows >= tc.PLANT_FROM and since <= tc.TOP:        # computed from the rows alone (also on the CPU:
            got = tc.decisions(srows, drows, n_rows, since)     # tests/test_table_merge_cpu.py)
            assert all(v > 0 for v in got.values()), (n_rows, since, got)
        dst, odst = load(drows, max(n_rows, 16), db, local_rank=tc.DST_RANK, canonical=canon0())
        check(dst, odst, src, osrc, n_rows, since, MW, (n_rows, strides, since), table=table)
        dst.close()
    src.close()


@pytest.mark.parametrize("strides", STRIDES)
@pytest.mark.parametrize("n_rows", [0, 1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 17])
def test_shapes(gpu_device, n_rows, strides):
    run_shapes(n_rows, strides, table=True)


# ------------------------------------------------------------------ 2. tile skipping
def pattern_rows(pattern: str, n_rows: int, seed: int):
    sel = np.zeros(n_rows, bool)
    if pattern == "all":
        sel[:] = True
    elif pattern == "alternating":
        sel[::2] = True
    elif pattern == "tile_ends":                         # exactly the first and the last row of a tile
        sel[2 * T] = sel[3 * T - 1] = True
    elif pattern == "run_across_boundary":               # a dense run over a tile boundary, empty tiles around it
        sel[2 * T - 300:2 * T + 500] = True
    else:
        assert pattern == "none"
    lo, hi = int(tc.STAMPS[2]), int(tc.STAMPS[30])
    rng = np.random.default_rng(seed)
    rows = {"ids": np.arange(n_rows, dtype=np.uint32), "mod": np.where(sel, hi, lo).astype(np.int64)}
    rows["lt"] = tc.STAMPS[rng.integers(0, tc.N_STAMPS, n_rows)].astype(np.int64)
    rows["rank"] = rng.integers(0, 6, n_rows).astype(np.uint32)
    rows["val"] = rng.integers(0, 1 << 20, n_rows).astype(np.uint32)
    rows["val"][rng.random(n_rows) < 0.2] = NULL
    return rows, sel, hi


@pytest.mark.parametrize("pattern", ["all", "none", "alternating", "tile_ends", "run_across_boundary"])
def test_tile_skipping(gpu_device, pattern):
    n_rows = 5 * T + 9
    srows, sel, hi = pattern_rows(pattern, n_rows, seed=11)
    _, drows = tc.gen_pair(n_rows, seed=12)
    src, osrc = load(srows, n_rows, local_rank=1)
    dst, odst = load(drows, n_rows, local_rank=tc.DST_RANK, canonical=canon0())
    c0 = dst.canonical
    res, oflags, ids = check(dst, odst, src, osrc, n_rows, hi, MW, pattern)
    assert np.array_equal(ids, np.flatnonzero(sel))
    assert res["status"] == 0 and res["n_stored"] == 1
    if pattern == "none":                # still one merge() call: the closing send advances the canonical
        assert res["n_won"] == 0 and not oflags.any() and dst.canonical == MW << 16 > c0
    else:
        assert 0 < res["n_won"] == int(oflags.sum())
    src.close()
    dst.close()


# ------------------------------------------------------------------ 3. more tiles than the clock pass's grid
@pytest.mark.parametrize("which", ["sparse", "full"])
def test_more_tiles_than_the_clock_grid(gpu_device, which):
    n_rows = (GRID + 3) * T + 17
    srows, drows = tc.gen_pair(n_rows, seed=5)
    src, osrc = load(srows, n_rows, local_rank=1)
    dst, odst = load(drows, n_rows, local_rank=tc.DST_RANK, canonical=canon0())
    since = tc.TOP if which == "sparse" else 0
    res, oflags, ids = check(dst, odst, src, osrc, n_rows, since, MW, which)
    assert res["status"] == 0 and res["n_won"] > 0
    assert len(ids) < n_rows // 20 if which == "sparse" else len(ids) > n_rows // 2
    src.close()
    dst.close()


# ------------------------------------------------------------------ 4. exceptions
N_EXC = 3 * T + 17


def exc_tables(planted: dict):
    """Every written src row selected by since = 0; ``planted`` = {id: (lt, rank)} rows that may raise."""
    srows, drows = tc.gen_pair(N_EXC, seed=41)
    for k, (lt, rank) in planted.items():
        tc._plant(srows, {k: (lt, rank, 77, tc.TOP)})
    src, osrc = load(srows, N_EXC, local_rank=1)
    dst, odst = load(drows, N_EXC, local_rank=tc.DST_RANK, canonical=canon0())
    return src, osrc, dst, odst


def selected_ids():
    srows, _ = tc.gen_pair(N_EXC, seed=41)
    s = tc.dense(srows, N_EXC)
    return np.flatnonzero(s["mod"] >= 0)


def check_raise(planted, status, at_id, tag):
    src, osrc, dst, odst = exc_tables(planted)
    before = read_all(dst)
    c0 = dst.canonical
    res, oflags, ids = check(dst, odst, src, osrc, N_EXC, 0, MW, tag, table=None)
    pos = int(np.searchsorted(ids, at_id))
    assert ids[pos] == at_id
    assert (res["status"], res["exc_changeset"], res["exc_index"]) == (status, 0, pos), (tag, res)
    assert res["n_stored"] == 0 and res["n_won"] == 0 and not oflags.any()
    # the canonical is the running max before the failing record (crdt.dart:82): lts below the record's
    lts = osrc.rows["lt"][ids[:pos]]
    assert dst.canonical == res["canonical_lt"] == max(c0, int(lts.max(initial=c0)))
    for x, y in zip(before, read_all(dst)):
        assert np.array_equal(x, y), tag                     # nothing of the changeset is stored
    src.close()
    dst.close()
    return res


ABOVE = tc.TOP + (1 << 16)                                   # an lt above every stamp (and dst's canonical)
DRIFT_LT = (MW + 60001) << 16                                # (lt >> 16) - wall == 60001


@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_duplicate_node_raises(gpu_device, where):
    sel = selected_ids()
    at = int({"first": sel[0], "middle": sel[len(sel) // 2], "last": sel[-1]}[where])
    res = check_raise({at: (ABOVE, tc.DST_RANK)}, _capi.CRDT_DUPLICATE_NODE, at, where)
    assert res["drift_ms"] == 0


def test_drift_raises(gpu_device):
    at = int(selected_ids()[T + 3])
    res = check_raise({at: (DRIFT_LT, 2)}, _capi.CRDT_CLOCK_DRIFT, at, "drift")
    assert res["drift_ms"] == 60001


@pytest.mark.parametrize("first", ["dup", "drift"])
def test_first_in_id_order_decides(gpu_device, first):
    sel = selected_ids()
    a, b = int(sel[T - 5]), int(sel[2 * T + 9])
    dup, drift = (ABOVE + 5, tc.DST_RANK), (DRIFT_LT, 2)
    if first == "dup":
        check_raise({a: dup, b: drift}, _capi.CRDT_DUPLICATE_NODE, a, first)
    else:
        check_raise({a: drift, b: dup}, _capi.CRDT_CLOCK_DRIFT, a, first)


def test_candidate_that_does_not_raise(gpu_device):
    """A row with dst's node id above dst's canonical, behind an earlier selected row that already lifted
    the running canonical to its lt: recv() returns early (hlc.dart:85), the merge stores."""
    sel = selected_ids()
    a, b = int(sel[7]), int(sel[2 * T + 1])
    src, osrc, dst, odst = exc_tables({a: (ABOVE, 2), b: (ABOVE, tc.DST_RANK)})
    res, oflags, _ = check(dst, odst, src, osrc, N_EXC, 0, MW, "no raise", table=None)
    assert res["status"] == 0 and res["n_stored"] == 1 and res["n_won"] > 0 and oflags[a] == 1
    assert res["exc_index"] == U64_MAX
    src.close()
    dst.close()


# ------------------------------------------------------------------ 5. send() failures after the store
@pytest.mark.parametrize("kind", ["drift", "overflow"])
def test_send_fails_after_the_store(gpu_device, kind):
    n_rows = 3 * T + 17
    srows, drows = tc.gen_pair(n_rows, seed=51)
    c1 = (MW + 60001) << 16 if kind == "drift" else ((MW + 5) << 16) | 0xFFFF
    src, osrc = load(srows, n_rows, local_rank=1)
    dst, odst = load(drows, n_rows, local_rank=tc.DST_RANK, canonical=c1)
    res, oflags, ids = check(dst, odst, src, osrc, n_rows, 0, MW, kind, table=None)
    want = _capi.CRDT_CLOCK_DRIFT if kind == "drift" else _capi.CRDT_OVERFLOW
    assert (res["status"], res["exc_changeset"], res["exc_index"]) == (want, 0, U64_MAX)
    assert res["n_stored"] == 1 and res["n_won"] == int(oflags.sum()) > 0
    assert res["canonical_lt"] == dst.canonical == c1
    if kind == "drift":
        assert res["drift_ms"] == 60001
    else:
        assert res["counter"] == 0x10000
    mod = read_all(dst)[3]
    assert np.all(mod[np.flatnonzero(oflags)] == c1)          # the winners carry mod = C1
    src.close()
    dst.close()


# ------------------------------------------------------------------ 6. capacity
def capacity_tables(selected_above: bool):
    n_rows, dcap = 3 * T + 17, 2 * T + 5
    lo, hi = int(tc.STAMPS[2]), int(tc.STAMPS[30])
    srows, _ = tc.gen_pair(n_rows, seed=61)
    srows["clear"] = (0, 0)
    above = srows["ids"] >= dcap
    srows["mod"] = np.where(above, lo, np.where(srows["mod"] >= 0, hi, srows["mod"])).astype(np.int64)
    bad = int(srows["ids"][above][3])
    if selected_above:
        srows["mod"][srows["ids"] == bad] = hi
    _, drows = tc.gen_pair(dcap, seed=62)
    src, osrc = load(srows, n_rows, local_rank=1)
    dst, odst = load(drows, dcap, local_rank=tc.DST_RANK, canonical=canon0())
    assert dst.capacity == dcap < n_rows
    return src, osrc, dst, odst, n_rows, hi


def test_capacity_smaller_than_n_rows(gpu_device):
    src, osrc, dst, odst, n_rows, hi = capacity_tables(False)
    res, oflags, ids = check(dst, odst, src, osrc, n_rows, hi, MW, "below dst's capacity")
    assert res["status"] == 0 and res["n_won"] > 0 and ids.max() < dst.capacity
    src.close()
    dst.close()


def test_selected_id_at_or_above_dst_capacity(gpu_device):
    src, osrc, dst, odst, n_rows, hi = capacity_tables(True)
    before, c0 = read_all(dst), dst.canonical
    with pytest.raises(CrdtNativeError) as e:
        dst.merge_table(src, n_rows, hi, MW, row_flags=True)
    assert e.value.status == _capi.CRDT_E_KEY_RANGE
    for x, y in zip(before, read_all(dst)):
        assert np.array_equal(x, y)
    assert dst.canonical == c0
    assert_rows(src, osrc, "src untouched")
    with pytest.raises(CrdtNativeError) as e:
        dst.merge_table(src, src.capacity + 1, hi, MW)
    assert e.value.status == _capi.CRDT_E_INVALID
    assert dst.canonical == c0
    src.close()
    dst.close()


# ------------------------------------------------------------------ 7. high-water marks
def check_export_equals(t: DeviceTable, o: OracleTable, n_rows: int, since: int):
    ids = o.modified_since(n_rows, since)
    key, lt, rank, val, mod = t.export_since(n_rows, since).columns()
    assert np.array_equal(key, ids), since
    for name, got in (("lt", lt), ("rank", rank), ("val", val), ("mod", mod)):
        assert np.array_equal(got, o.rows[name][ids]), (name, since)


@pytest.mark.parametrize("since", [0, I64_MIN])
@pytest.mark.parametrize("case", ["src_above_dst_mark", "src_mark_below_n_rows"])
def test_high_water_marks(gpu_device, case, since):
    w = T + 5
    cap = 8 * w
    ws, wd = (3 * w, w) if case == "src_above_dst_mark" else (w, 3 * w)
    srows, _ = tc.gen_pair(ws, seed=71)
    _, drows = tc.gen_pair(wd, seed=72)
    src, osrc = load(srows, cap, local_rank=1)
    dst, odst = load(drows, cap, local_rank=tc.DST_RANK, canonical=canon0())
    assert src.capacity == dst.capacity == cap
    res, oflags, ids = check(dst, odst, src, osrc, cap, since, MW, (case, since))
    assert res["status"] == 0
    assert len(ids) == cap if since == I64_MIN else ids.max() < ws
    if case == "src_above_dst_mark":
        assert oflags[wd:ws].any()                           # rows stored above dst's mark
    check_export_equals(dst, odst, cap, 0)
    check_export_equals(dst, odst, cap, I64_MIN)
    src.close()
    dst.close()


# ------------------------------------------------------------------ 8. convergence
def test_converges_like_merge_from(gpu_device):
    CAP = gx.CAP
    A, oA, B, oB, stamp = gx._pair("gather")
    for t in (A, B):
        t.set_merge_path("auto")
    res, oflags, ids = check(B, oB, A, oA, CAP, 0, WALL + 1, "A->B")
    assert res["status"] == 0 and len(ids) > gx.N_LOCAL // 2 and 0 < res["n_won"] < len(ids)
    res, oflags, ids2 = check(A, oA, B, oB, CAP, stamp, WALL + 2, "B->A")
    assert res["status"] == 0 and 0 < len(ids2) < len(ids) and res["n_won"] > 0
    ra, rb = read_all(A), read_all(B)
    for name, x, y in zip(("lt", "rank", "val"), ra, rb):
        assert np.array_equal(x, y), ("convergence", name)
    # a twin pair synced by the export + merge route ends in the same rows
    A2, _, B2, _, stamp2 = gx._pair("gather")
    B2.merge_from(A2, CAP, 0, WALL + 1)
    A2.merge_from(B2, CAP, stamp2, WALL + 2)
    for t, t2 in ((A, A2), (B, B2)):
        for name, x, y in zip(("lt", "rank", "val", "mod"), read_all(t), read_all(t2)):
            assert np.array_equal(x, y), ("twin", name)
        assert t.canonical == t2.canonical
    for t in (A, B, A2, B2):
        t.close()


# ------------------------------------------------------------------ 9. the switch
@pytest.mark.parametrize("strides", STRIDES)
def test_switch_takes_the_composition(gpu_device, monkeypatch, strides):
    monkeypatch.setenv("CRDT_TABLE_MERGE", "0")              # read when the tables are created
    run_shapes(3 * T + 17, strides, table=False)


# ------------------------------------------------------------------ 10. flags memory, src is dst, devices
def test_host_flags_equal_device_flags(gpu_device):
    import torch
    n_rows = 3 * T + 17
    srows, drows = tc.gen_pair(n_rows, seed=3000 + n_rows)
    src, osrc = load(srows, n_rows, local_rank=1)
    got = []
    for kind in ("device", "host", "given"):
        dst, odst = load(drows, n_rows, local_rank=tc.DST_RANK, canonical=canon0())
        if kind == "host":
            arr = np.full(n_rows, 9, np.uint8)
        elif kind == "given":
            arr = torch.full((n_rows,), 9, dtype=torch.uint8, device="cuda:0")
        else:
            arr = True
        res, oflags, _ = check(dst, odst, src, osrc, n_rows, 0, MW, kind, row_flags=arr)
        if kind == "device":
            got.append(oflags)                                # (check compared the returned tensor with them)
        else:
            got.append(arr.copy() if kind == "host" else arr.cpu().numpy())
            assert np.array_equal(got[-1], oflags), kind      # filled in place, every entry written
            arr[:] = 9                                        # an empty selection writes every entry too: zeros
            res, oflags, ids = check(dst, odst, src, osrc, n_rows, tc.TOP + 1, MW + 1, (kind, "empty"), row_flags=arr)
            assert len(ids) == 0 and not (arr if kind == "host" else arr.cpu().numpy()).any()
        dst.close()
    assert np.array_equal(got[0], got[1]) and np.array_equal(got[0], got[2]) and got[0].any()
    # without flags: the same result
    dst, odst = load(drows, n_rows, local_rank=tc.DST_RANK, canonical=canon0())
    check(dst, odst, src, osrc, n_rows, 0, MW, "no flags", row_flags=False)
    dst.close()
    src.close()


@pytest.mark.parametrize("offset", [0, 1, 8])
def test_given_flags_tensor_at_any_alignment(gpu_device, offset):
    """Tiles that select nothing zero their flags with wide stores where the tensor allows it: a view that
    starts at an odd byte gets the same flags, and nothing outside [0, n_rows) is written."""
    import torch
    n_rows = 5 * T + 9
    srows, sel, hi = pattern_rows("run_across_boundary", n_rows, seed=11)
    _, drows = tc.gen_pair(n_rows, seed=12)
    src, osrc = load(srows, n_rows, local_rank=1)
    dst, odst = load(drows, n_rows, local_rank=tc.DST_RANK, canonical=canon0())
    buf = torch.full((offset + n_rows + 16,), 9, dtype=torch.uint8, device="cuda:0")
    arr = buf[offset:offset + n_rows]
    res, oflags, _ = check(dst, odst, src, osrc, n_rows, hi, MW, offset, row_flags=arr)
    got = buf.cpu().numpy()
    assert np.array_equal(got[offset:offset + n_rows], oflags) and oflags.any()
    assert np.all(got[:offset] == 9) and np.all(got[offset + n_rows:] == 9)
    src.close()
    dst.close()


def test_src_is_dst(gpu_device):
    n_rows = 3 * T + 17
    srows, _ = tc.gen_pair(n_rows, seed=91)
    t, o = load(srows, n_rows, local_rank=tc.DST_RANK, canonical=canon0())
    res, oflags, ids = check(t, o, t, o, n_rows, 0, MW, "self", table=None)
    assert res["status"] == 0 and res["n_won"] == 0 and res["n_present"] == len(ids) > 0
    t.close()


def test_other_device_is_refused(gpu_device):
    a, b = DeviceTable(0, capacity=16), DeviceTable(0, capacity=16)
    b.device = 1                                              # (as if it had been created on another GPU)
    with pytest.raises(ValueError):
        a.merge_table(b, 16, 0, WALL)
    b.device = 0
    a.close()
    b.close()
