"""crdt_tombstone_live / crdt_export_live (DeviceTable.tombstone_live, export_live) on the GPU against the model
of tests/_live_cases.py (the composition on the C restatement), against the existing composition on a twin
table, and against the existing calls as oracle for what the new stamp selects.  Everything is integer data:
every comparison is exact."""
import ctypes

import numpy as np
import pytest
import torch

import tests.test_gpu_table_merge as gt
from crdt_amd import DeviceTable, _capi
from oracle.oracle_c import send_scalar
from tests import _live_cases as lc
from tests import _table_cases as tc
from tests._cases import ABSENT_MOD, NULL

pytestmark = pytest.mark.gpu

T = lc.T
RESULT_FIELDS = gt.RESULT_FIELDS
ABOVE_FILL = int(ABSENT_MOD) + 1


def load_live(n_rows: int, seed: int, row_bytes: int = 24, canonical: int = lc.C0, extra: int = 37, rows=None):
    """(table, oracle mirror) of gen_live's rows, the capacity above n_rows (a live row sits at n_rows)."""
    rows = lc.gen_live(n_rows, seed) if rows is None else rows
    return gt.load(rows, max(n_rows, 16) + extra, row_bytes, local_rank=lc.LOCAL_RANK, canonical=canonical)


def check(t, o, n_rows: int, wall: int, tag, row_flags=True):
    """One tombstone_live against the model: every result field, the rows, the canonical and the flags."""
    ores, oflags = lc.model_tombstone(o, n_rows, wall)
    res, flags = t.tombstone_live(n_rows, wall, row_flags=row_flags)
    for f in RESULT_FIELDS:
        assert res[f] == ores[f], (tag, f, res[f], ores[f])
    gt.assert_rows(t, o, tag)
    if row_flags is True:
        assert str(flags.device) == "cuda:0" and flags.dtype == torch.uint8 and len(flags) == n_rows, tag
        assert np.array_equal(flags.cpu().numpy(), oflags), tag
    return res, flags, oflags


def composition(t: DeviceTable, n_rows: int, wall: int) -> dict:
    """The existing calls: export_since at 0, a torch filter on val, put_stamped with device ids."""
    key, _, _, val, _ = t.export_since(n_rows, 0).columns()
    kd = torch.from_numpy(key.view(np.int32)).to("cuda:0")
    vd = torch.from_numpy(val.view(np.int32)).to("cuda:0")
    ids = kd[vd != -1].contiguous()
    return t.put_stamped(ids, torch.full_like(ids, -1), wall)


# ------------------------------------------------------------------ 1. shapes
@pytest.mark.parametrize("row_bytes", [24, 32])
@pytest.mark.parametrize("n_rows", lc.SHAPES)
def test_shapes(gpu_device, n_rows, row_bytes):
    rows = lc.gen_live(n_rows, 500 + n_rows)
    t, o = load_live(n_rows, 0, row_bytes, rows=rows)
    twin, _ = load_live(n_rows, 0, row_bytes, rows=rows)
    n_live = int(lc.live_mask(o.rows, n_rows).sum())
    res, _, oflags = check(t, o, n_rows, lc.WALL, (n_rows, row_bytes))
    want_c = send_scalar(lc.C0, lc.WALL)[1] if n_live else lc.C0
    assert (res["status"], res["n_won"], res["canonical_lt"]) == (0, n_live, want_c)
    if n_rows >= lc.PLANT_FROM:
        assert n_live >= n_rows // 4 and oflags[0] == oflags[n_rows - 1] == 1 and not oflags[1:4].any()
    cres = composition(twin, n_rows, lc.WALL)
    for f in RESULT_FIELDS:
        assert res[f] == cres[f], (n_rows, row_bytes, f)
    assert twin.canonical == t.canonical
    for a, b in zip(gt.read_all(t), gt.read_all(twin)):
        assert np.array_equal(a, b), (n_rows, row_bytes)
    assert np.array_equal(t.digest_rows(t.capacity, T), twin.digest_rows(twin.capacity, T))
    t.close()
    twin.close()


# ------------------------------------------------------------------ 2. more tiles than workgroups
def test_more_tiles_than_workgroups(gpu_device):
    n = lc.LARGE
    assert n > lc.GRID * T
    t, o = load_live(n, 7, 24, extra=3)
    res, _, oflags = check(t, o, n, lc.WALL, "large")
    assert oflags[-1] == 1 and res["n_won"] == int(oflags.sum()) > n // 4
    t.close()


# ------------------------------------------------------------------ 3. the no-op
@pytest.mark.parametrize("row_bytes", [24, 32])
def test_no_live_row_is_a_noop_even_where_send_would_raise(gpu_device, row_bytes):
    assert send_scalar(lc.C0, lc.DRIFT_WALL)[0] == 1
    n = 3 * T + 17
    t, o = load_live(n, 0, row_bytes, rows=lc.gen_dead(n, 31))
    for wall in (lc.DRIFT_WALL, lc.WALL):
        res, flags, _ = check(t, o, n, wall, ("dead", wall))
        assert (res["status"], res["n_won"], res["canonical_lt"]) == (0, 0, lc.C0) and not flags.any().item()
    t.close()
    t, o = load_live(n, 32, row_bytes)                     # live rows, but none below n_rows == 0
    for wall in (lc.DRIFT_WALL, lc.WALL):
        res, flags, _ = check(t, o, 0, wall, ("n_rows 0", wall))
        assert (res["status"], res["n_won"], t.canonical) == (0, 0, lc.C0) and len(flags) == 0
    t.close()


# ------------------------------------------------------------------ 4. Hlc.send raises and there is a live row
@pytest.mark.parametrize("row_bytes", [24, 32])
def test_a_raise_with_live_rows_keeps_everything(gpu_device, row_bytes):
    n = 2 * T + 9
    millis = lc.C0 >> 16
    over = (millis << 16) | 0xFFFF
    cases = [("drift", lc.C0, lc.DRIFT_WALL, 1), ("overflow at the wall", over, millis, 3),
             ("overflow above the wall", over, millis - 10, 3)]
    for name, canonical, wall, status in cases:
        t, o = load_live(n, 41, row_bytes, canonical=canonical)
        before = o.rows.copy()
        st, _, drift, counter = send_scalar(canonical, wall)
        res, flags, _ = check(t, o, n, wall, name)
        assert st == status == res["status"], name
        assert (res["drift_ms"], res["counter"], res["canonical_lt"], res["n_won"]) == (drift, counter, canonical, 0), name
        assert (drift > 60000) if status == 1 else (counter == 0x10000), name
        assert not flags.any().item() and np.array_equal(o.rows, before) and t.canonical == canonical, name
        t.close()


# ------------------------------------------------------------------ 5. what the new stamp selects
@pytest.mark.parametrize("row_bytes", [24, 32])
def test_the_new_stamp_selects_the_tombstones(gpu_device, row_bytes):
    n = 5 * T + 9
    rows = lc.gen_live(n, 55)
    t, o = load_live(n, 0, row_bytes, rows=rows)
    visible = t.count_since(n, 0)[0]
    res, flags, oflags = check(t, o, n, lc.WALL, "clear")
    c, want_ids = res["canonical_lt"], np.flatnonzero(oflags)
    ex = t.export_since(n, c)
    assert ex.n == res["n_won"] == len(want_ids) and ex.n_live == 0
    key, lt, rank, val, mod = ex.columns()
    assert np.array_equal(key, want_ids) and np.all(lt == c) and np.all(mod == c)
    assert np.all(rank == lc.LOCAL_RANK) and np.all(val == NULL)
    assert np.array_equal(t.export_flagged(n, flags, 1).columns()[0], want_ids)
    assert t.count_since(n, 0) == (visible, 0)
    # a sibling holding the rows as they were takes exactly those tombstones
    sib, osib = gt.load(rows, t.capacity, 24, local_rank=3, canonical=lc.C0)
    ores, orf, _ = tc.oracle_merge_table(osib, o, n, c, lc.WALL + 1)
    sres, rf = sib.merge_table(t, n, c, lc.WALL + 1, row_flags=True)
    for f in RESULT_FIELDS:
        assert sres[f] == ores[f], f
    assert sres["n_won"] == res["n_won"] and np.array_equal(orf, oflags) and torch.equal(rf, flags)
    gt.assert_rows(sib, osib, "sibling")
    gt.assert_rows(t, o, "the cleared table is the merge's source: untouched")
    t.close()
    sib.close()


# ------------------------------------------------------------------ 6. left alone
@pytest.mark.parametrize("row_bytes", [24, 32])
def test_left_alone(gpu_device, row_bytes):
    n = 2 * T + 5
    t, o = load_live(n, 66, row_bytes, extra=3 * T)
    plan, path_rows = t.last_plan(), o.rows[n].copy()
    view = t.export_since(n, int(tc.STAMPS[20]))
    cols = view.columns()
    assert view.n > 0
    res, _, _ = check(t, o, n, lc.WALL, "clear", row_flags=False)
    assert res["n_won"] > 0
    for a, b in zip(view.columns(), cols):               # the view taken before the call reads back its old columns
        assert np.array_equal(a, b)
    assert t.last_plan() == plan
    lt, rank, val, mod = t.read_rows(np.array([n], np.uint32))
    assert (lt[0], rank[0], val[0], mod[0]) == tuple(path_rows[k] for k in ("lt", "rank", "val", "mod"))
    assert val[0] != NULL and mod[0] >= 0                # the live row at n_rows survives
    # the high-water mark is where it was: an export above the fill's mod selects no fill row
    assert np.array_equal(t.export_since(t.capacity, ABOVE_FILL).columns()[0], o.modified_since(t.capacity, ABOVE_FILL))
    t.close()


# ------------------------------------------------------------------ 7. where the flags live
def test_flags_in_host_and_device_memory_and_unaligned(gpu_device):
    n = 3 * T + 17
    rows = lc.gen_live(n, 77)
    t, o = load_live(n, 0, 24, rows=rows)
    _, _, want = check(t, o, n, lc.WALL, "device flags")
    want_rows = gt.read_all(t)
    t.close()
    t, _ = load_live(n, 0, 24, rows=rows)
    host = np.full(n + 9, 0x5A, np.uint8)
    res, got = t.tombstone_live(n, lc.WALL, row_flags=host)
    assert got is host and np.array_equal(host[:n], want) and np.all(host[n:] == 0x5A)
    t.close()
    for off in (1, 3):
        t, _ = load_live(n, 0, 24, rows=rows)
        base = torch.full((off + n + 9,), 0x5A, dtype=torch.uint8, device="cuda:0")
        res, _ = t.tombstone_live(n, lc.WALL, row_flags=base[off:])
        got = base.cpu().numpy()
        assert res["n_won"] == int(want.sum()) and np.array_equal(got[off:off + n], want), off
        assert np.all(got[:off] == 0x5A) and np.all(got[off + n:] == 0x5A), off
        t.close()
    for m in (n - 1, T + 64, 63):                        # fewer rows than the table holds: nothing past them is written
        t, o = load_live(n, 0, 32, rows=rows)
        base = torch.full((n,), 0x5A, dtype=torch.uint8, device="cuda:0")
        check(t, o, m, lc.WALL, ("partial", m), row_flags=base)
        got = base.cpu().numpy()
        assert np.array_equal(got[:m], want[:m]) and np.all(got[m:] == 0x5A), m
        t.close()
    t, o = load_live(n, 0, 24, rows=rows)
    res, none = t.tombstone_live(n, lc.WALL)             # without flags: the same rows
    assert none is None and res["n_won"] == int(want.sum())
    for a, b in zip(gt.read_all(t), want_rows):
        assert np.array_equal(a, b)
    t.close()


# ------------------------------------------------------------------ 8. refused calls
def test_refused_calls_touch_nothing(gpu_device):
    n = T + 9
    t, o = load_live(n, 88)
    lib, E, D, H = t._lib, _capi.CRDT_E_INVALID, _capi.CRDT_MEM_DEVICE, _capi.CRDT_MEM_HOST
    out = _capi.CrdtResult()
    ctypes.memset(ctypes.byref(out), 0x5A, ctypes.sizeof(out))
    poisoned = bytes(out)
    dflags = torch.full((t.capacity + 8,), 0x5A, dtype=torch.uint8, device="cuda:0")
    hflags = np.full(t.capacity + 8, 0x5A, np.uint8)
    torch.cuda.synchronize()
    dp, hp = ctypes.c_void_p(dflags.data_ptr()), hflags.ctypes.data_as(ctypes.c_void_p)
    from tests._loopback import LoopbackComm
    joined = DeviceTable(0, local_rank=4, capacity=n)
    joined.put_stamped(np.arange(8, dtype=np.uint32), np.arange(8, dtype=np.uint32), lc.WALL)
    joined.comm_init_ops(2, 0, LoopbackComm(2))          # rank 0 of a loopback communicator
    call = lib.crdt_tombstone_live
    refused = [
        call(None, n, lc.WALL, dp, D, ctypes.byref(out)), call(t._ctx, n, lc.WALL, dp, D, None),
        call(t._ctx, t.capacity + 1, lc.WALL, dp, D, ctypes.byref(out)),
        call(t._ctx, n, lc.WALL, dp, 7, ctypes.byref(out)), call(t._ctx, n, lc.WALL, hp, -1, ctypes.byref(out)),
        call(joined._ctx, 8, lc.WALL, dp, D, ctypes.byref(out)), call(joined._ctx, 8, lc.WALL, hp, H, ctypes.byref(out)),
    ]
    assert refused == [E] * len(refused)
    assert bytes(out) == poisoned and np.all(hflags == 0x5A) and torch.all(dflags == 0x5A).item()
    gt.assert_rows(t, o, "untouched")
    assert joined.count_since(8, 0) == (8, 8)
    view = _capi.CrdtExport()
    live = lib.crdt_export_live
    assert [live(None, n, ctypes.byref(view)), live(t._ctx, n, None),
            live(t._ctx, t.capacity + 1, ctypes.byref(view))] == [E] * 3
    ores, _ = lc.model_tombstone(o, n, lc.WALL)          # (a bad flags_mem without a pointer is unused)
    assert call(t._ctx, n, lc.WALL, None, 7, ctypes.byref(out)) == 0 and out.n_won == ores["n_won"] > 0
    gt.assert_rows(t, o, "stored")
    t.close()
    joined.close()


# ------------------------------------------------------------------ 9. export_live
@pytest.mark.parametrize("row_bytes", [24, 32])
@pytest.mark.parametrize("n_rows", lc.SHAPES)
def test_export_live(gpu_device, n_rows, row_bytes):
    t, o = load_live(n_rows, 900 + n_rows, row_bytes)
    want = lc.model_live(o.rows, n_rows)
    ex = t.export_live(n_rows)
    assert ex.n == ex.n_live == len(want["key"]) == t.count_since(n_rows, 0)[1]
    for name, col in zip(("key", "lt", "rank", "val", "mod"), ex.columns()):     # export_read on the current view
        assert col.dtype == want[name].dtype and np.array_equal(col, want[name]), (n_rows, row_bytes, name)
    if ex.n > 10:
        part = ex.columns(3, 5)
        assert np.array_equal(part[0], want["key"][3:8]) and np.array_equal(part[3], want["val"][3:8])
    full = t.export_since(n_rows, 0)                     # the next export ends it, and holds the tombstones again
    assert full.n == len(o.modified_since(n_rows, 0)) and full.n_live == len(want["key"])
    with pytest.raises(Exception):
        ex.columns()
    gt.assert_rows(t, o, "read-only")
    t.close()
