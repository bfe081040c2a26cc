"""crdt_purge_tombstones (DeviceTable.purge_tombstones) on the GPU against the model of tests/_purge_cases.py, against
the composition the call is held to run with the existing calls on a twin set of tables (export_since of every
member, the intersection on the host, clear_rows(i, 1) per purged id), and with the existing calls around it.
Everything is integer data: every comparison is exact."""
import ctypes

import numpy as np
import pytest
import torch

import tests.test_gpu_table_merge as gt
from crdt_amd import CrdtNativeError, DeviceTable, _capi
from tests import _purge_cases as pc
from tests import _table_cases as tc
from tests._cases import ABSENT_MOD, NULL

pytestmark = pytest.mark.gpu

T = pc.T
B = pc.BEFORE
ABOVE_FILL = int(ABSENT_MOD) + 1
STRIDES = {"24": (24,), "32": (32,), "mixed": (24, 32, 24)}
assert T == _capi.TABLE_TILE and pc.GRID == _capi.PURGE_GRID and max(pc.MEMBERS) == _capi.PURGE_MAX


def load_group(members: list, n_rows: int, strides=(24,), extra: int = 37):
    """(tables, oracle mirrors): member j with row size strides[j % len], local rank 8 + j (above the rows' ranks),
    canonical 100 + j and a capacity of its own above n_rows (an agreed tombstone sits at n_rows)."""
    pairs = [gt.load(m, max(n_rows, 16) + extra + 11 * j, strides[j % len(strides)], local_rank=8 + j, canonical=100 + j)
             for j, m in enumerate(members)]
    return [t for t, _ in pairs], [o for _, o in pairs]


def close(*groups):
    for g in groups:
        for t in g:
            t.close()


def check(ts, os_, n_rows: int, before: int, tag, row_flags=True):
    """One purge_tombstones against the model: the counts, every member's rows and canonical, the flags."""
    want, wflags = pc.model_purge(os_, n_rows, before)
    res, flags = ts[0].purge_tombstones(ts[1:], n_rows, before, row_flags=row_flags)
    assert res == want, (tag, res, want)
    for j, (t, o) in enumerate(zip(ts, os_)):
        gt.assert_rows(t, o, (tag, "member", j))
    if row_flags is True:
        assert str(flags.device) == "cuda:0" and flags.dtype == torch.uint8 and len(flags) == n_rows, tag
        assert np.array_equal(flags.cpu().numpy(), wflags), tag
    return res, flags, wflags


def composition(ts, n_rows: int, before: int) -> np.ndarray:
    """The existing calls: export_since at 0 of every member, the intersection on the host, clear_rows per id."""
    cols = [t.export_since(n_rows, 0).columns() for t in ts]
    key0, lt0, rank0, val0, _ = cols[0]
    ids = key0[(val0 == NULL) & (lt0 < before)]
    for key, lt, rank, val, _ in cols[1:]:
        held = {int(k): (int(a), int(r)) for k, a, r, v in zip(key, lt, rank, val) if v == NULL}
        mine = dict(zip(key0.tolist(), zip(lt0.tolist(), rank0.tolist())))
        ids = np.array([i for i in ids.tolist() if held.get(i) == mine[i]], np.uint32)
    for t in ts:
        for i in ids.tolist():
            t.clear_rows(i, 1)
    return ids


# ------------------------------------------------------------------ 1. shapes
@pytest.mark.parametrize("strides", list(STRIDES))
@pytest.mark.parametrize("n_members", pc.MEMBERS)
@pytest.mark.parametrize("n_rows", pc.SHAPES)
def test_shapes(gpu_device, n_rows, n_members, strides):
    members = pc.gen_group(n_rows, n_members, 700 + n_rows + n_members)
    ts, os_ = load_group(members, n_rows, STRIDES[strides])
    twins, _ = load_group(members, n_rows, STRIDES[strides])
    assert len({t.capacity for t in ts}) == n_members
    res, _, wflags = check(ts, os_, n_rows, B, (n_rows, n_members, strides))
    if n_rows >= pc.PLANT_FROM:
        assert res["n_purged"] >= n_rows // 8 and wflags[0] == wflags[n_rows - 1] == 1
        assert res["n_candidates"] - res["n_purged"] >= (n_rows // 8 if n_members > 1 else 0)
        lt, _, val, mod = ts[-1].read_rows(np.array([n_rows], np.uint32))
        assert val[0] == NULL and mod[0] >= 0 and lt[0] < B       # the agreed tombstone at n_rows survives
    ids = composition(twins, n_rows, B)
    assert np.array_equal(ids, np.flatnonzero(wflags))
    for t, twin in zip(ts, twins):
        for a, b in zip(gt.read_all(t), gt.read_all(twin)):
            assert np.array_equal(a, b), (n_rows, n_members, strides)
        assert np.array_equal(t.digest_rows(t.capacity, T), twin.digest_rows(twin.capacity, T))
        assert t.canonical == twin.canonical
    close(ts, twins)


# ------------------------------------------------------------------ 2. more tiles than workgroups
def test_more_tiles_than_workgroups(gpu_device):
    n = pc.LARGE
    assert n > pc.GRID * T
    ts, os_ = load_group(pc.gen_group(n, 2, 7), n, (24, 32), extra=3)
    res, _, wflags = check(ts, os_, n, B, "large")
    assert wflags[-1] == 1 and res["n_purged"] == int(wflags.sum()) > n // 8
    close(ts)


# ------------------------------------------------------------------ 3. degenerate inputs
@pytest.mark.parametrize("strides", ["24", "mixed"])
def test_nothing_to_purge_and_everything_agreed(gpu_device, strides):
    n = 3 * T + 17
    ts, os_ = load_group(pc.gen_no_tombstone(n, 3, 31), n, STRIDES[strides])
    res, flags, _ = check(ts, os_, n, pc.I64_MAX, "no tombstone")
    assert res == {"n_candidates": 0, "n_purged": 0} and not flags.any().item()
    close(ts)
    ts, os_ = load_group(pc.gen_group(n, 3, 32), n, STRIDES[strides])
    res, flags, _ = check(ts, os_, n, pc.I64_MIN, "before = INT64_MIN")
    assert res == {"n_candidates": 0, "n_purged": 0} and not flags.any().item()
    res, flags, _ = check(ts, os_, 0, pc.I64_MAX, "n_rows 0")
    assert res == {"n_candidates": 0, "n_purged": 0} and len(flags) == 0
    close(ts)
    ts, os_ = load_group(pc.gen_blocked(n, 3, 33), n, STRIDES[strides])
    res, flags, _ = check(ts, os_, n, B, "all blocked")
    assert res["n_candidates"] > n // 8 and res["n_purged"] == 0 and not flags.any().item()
    close(ts)
    ts, os_ = load_group(pc.gen_agreed(n, 3, 34), n, STRIDES[strides])
    res, flags, _ = check(ts, os_, n, B, "all agreed")
    assert res["n_candidates"] == res["n_purged"] == int(flags.sum().item()) > n // 8
    assert check(ts, os_, n, B, "again")[0] == {"n_candidates": 0, "n_purged": 0}
    close(ts)


def test_a_second_call_purges_nothing_and_counts_the_blocked_again(gpu_device):
    n = 2 * T + 9
    ts, os_ = load_group(pc.gen_group(n, 3, 35), n, STRIDES["mixed"])
    first, _, _ = check(ts, os_, n, B, "first")
    second, flags, _ = check(ts, os_, n, B, "second")
    assert first["n_purged"] > 0 and first["n_candidates"] > first["n_purged"]
    assert second == {"n_candidates": first["n_candidates"] - first["n_purged"], "n_purged": 0}
    assert not flags.any().item()
    alone, _, _ = check(ts[:1], os_[:1], n, B, "member 0 alone")        # nobody blocks: it collects its own
    assert alone["n_purged"] == alone["n_candidates"] == second["n_candidates"]
    close(ts)


# ------------------------------------------------------------------ 4. where the flags live
def test_flags_in_host_and_device_memory_and_unaligned(gpu_device):
    n = 3 * T + 17
    members = pc.gen_group(n, 2, 77)
    ts, os_ = load_group(members, n)
    _, _, want = check(ts, os_, n, B, "device flags")
    want_rows = [gt.read_all(t) for t in ts]
    close(ts)
    ts, _ = load_group(members, n)
    host = np.full(n + 9, 0x5A, np.uint8)
    res, got = ts[0].purge_tombstones(ts[1:], n, B, row_flags=host)
    assert got is host and np.array_equal(host[:n], want) and np.all(host[n:] == 0x5A)
    close(ts)
    for off in (1, 3, 8):
        ts, _ = load_group(members, n)
        base = torch.full((off + n + 9,), 0x5A, dtype=torch.uint8, device="cuda:0")
        res, _ = ts[0].purge_tombstones(ts[1:], n, B, row_flags=base[off:])
        got = base.cpu().numpy()
        assert res["n_purged"] == int(want.sum()) and np.array_equal(got[off:off + n], want), off
        assert np.all(got[:off] == 0x5A) and np.all(got[off + n:] == 0x5A), off
        close(ts)
    for m in (n - 1, T + 64, 63):                        # fewer rows than the tables hold: nothing past them is written
        ts, os_ = load_group(members, n, (32, 24))
        base = torch.full((n,), 0x5A, dtype=torch.uint8, device="cuda:0")
        check(ts, os_, m, B, ("partial", m), row_flags=base)
        got = base.cpu().numpy()
        assert np.array_equal(got[:m], want[:m]) and np.all(got[m:] == 0x5A), m
        close(ts)
    ts, os_ = load_group(members, n)
    res, none = ts[0].purge_tombstones(ts[1:], n, B)     # without flags: the same rows
    assert none is None and res["n_purged"] == int(want.sum())
    for t, rows in zip(ts, want_rows):
        for a, b in zip(gt.read_all(t), rows):
            assert np.array_equal(a, b)
    close(ts)


# ------------------------------------------------------------------ 5. left alone
@pytest.mark.parametrize("strides", ["24", "32"])
def test_left_alone(gpu_device, strides):
    n = 2 * T + 5
    ts, os_ = load_group(pc.gen_group(n, 3, 66), n, STRIDES[strides], extra=3 * T)
    plans = [(t.last_plan(), t.last_path(), t.timing()) for t in ts]
    beyond = [o.rows[n:].copy() for o in os_]
    views = [t.export_since(n, int(tc.STAMPS[20])) for t in ts]
    cols = [v.columns() for v in views]
    assert all(v.n > 0 for v in views)
    res, _, _ = check(ts, os_, n, B, "purge", row_flags=False)          # (assert_rows compares every canonical)
    assert res["n_purged"] > 0
    for t, o, v, c, p, rest in zip(ts, os_, views, cols, plans, beyond):
        for a, b in zip(v.columns(), c):                 # the view taken before the call reads back its old columns
            assert np.array_equal(a, b)
        assert (t.last_plan(), t.last_path(), t.timing()) == p
        assert np.array_equal(o.rows[n:], rest) and t.canonical == o.canonical
        # the high-water mark is where it was: an export above the fill's mod selects no fill row
        assert np.array_equal(t.export_since(t.capacity, ABOVE_FILL).columns()[0], o.modified_since(t.capacity, ABOVE_FILL))
    close(ts)


# ------------------------------------------------------------------ 6. refused calls
def test_refused_calls_touch_nothing(gpu_device):
    n = T + 9
    ts, os_ = load_group(pc.gen_group(n, 3, 88), n, STRIDES["mixed"])
    a, b, c = ts
    lib, E, D, H = a._lib, _capi.CRDT_E_INVALID, _capi.CRDT_MEM_DEVICE, _capi.CRDT_MEM_HOST
    out = _capi.CrdtPurge()
    ctypes.memset(ctypes.byref(out), 0x5A, ctypes.sizeof(out))
    poisoned = bytes(out)
    dflags = torch.full((c.capacity + 8,), 0x5A, dtype=torch.uint8, device="cuda:0")
    hflags = np.full(c.capacity + 8, 0x5A, np.uint8)
    torch.cuda.synchronize()
    dp, hp, po = ctypes.c_void_p(dflags.data_ptr()), hflags.ctypes.data_as(ctypes.c_void_p), ctypes.byref(out)
    from tests._loopback import LoopbackComm
    joined = DeviceTable(0, local_rank=4, capacity=n)
    joined.comm_init_ops(2, 0, LoopbackComm(2))          # rank 0 of a loopback communicator
    assert a.capacity < b.capacity < c.capacity

    def arr(*tables):
        return (ctypes.c_void_p * max(len(tables), 1))(*(t._ctx.value if t is not None else None for t in tables))

    call = lib.crdt_purge_tombstones
    more = [DeviceTable(0, capacity=16) for _ in range(6)]
    refused = [
        call(None, 1, n, B, dp, D, po), call(arr(a, b), 2, n, B, dp, D, None),
        call(arr(a, None, b), 3, n, B, dp, D, po), call(arr(None), 1, n, B, dp, D, po),
        call(arr(a), 0, n, B, dp, D, po), call(arr(a, b, c, *more), 9, 16, B, dp, D, po),
        call(arr(a, b, a), 3, n, B, dp, D, po), call(arr(a, a), 2, n, B, dp, D, po),
        call(arr(b, a), 2, a.capacity + 1, B, dp, D, po),                # above a's capacity, inside b's
        call(arr(a, b), 2, a.capacity + 1, B, dp, D, po),
        call(arr(a, b), 2, n, B, dp, 7, po), call(arr(a, b), 2, n, B, hp, -1, po),
        call(arr(a, joined), 2, n, B, dp, D, po), call(arr(joined, a), 2, n, B, hp, H, po),
    ]
    assert refused == [E] * len(refused)
    assert bytes(out) == poisoned and np.all(hflags == 0x5A) and torch.all(dflags == 0x5A).item()
    other = DeviceTable(0, capacity=16)
    other.device = 1                                     # (as if it had been created on another GPU)
    with pytest.raises(ValueError):
        a.purge_tombstones([b, other], 16, B)
    other.device = 0
    with pytest.raises(CrdtNativeError) as e:
        a.purge_tombstones([other], other.capacity + 1, B)
    assert e.value.status == E
    for j, (t, o) in enumerate(zip(ts, os_)):
        gt.assert_rows(t, o, ("untouched", j))
    want, _ = pc.model_purge(os_, n, B)                  # (a bad flags_mem without a pointer is unused)
    assert call(arr(a, b, c), 3, n, B, None, 7, po) == 0
    assert (out.n_candidates, out.n_purged) == (want["n_candidates"], want["n_purged"]) and want["n_purged"] > 0
    for j, (t, o) in enumerate(zip(ts, os_)):
        gt.assert_rows(t, o, ("stored", j))
    close(ts, more, [joined, other])


# ------------------------------------------------------------------ 7. with the calls around it
@pytest.mark.parametrize("strides", ["24", "mixed"])
def test_interplay(gpu_device, strides):
    n = 5 * T + 9
    members = pc.gen_agreed(n, 3, 91)
    ts, os_ = load_group(members, n, STRIDES[strides])
    third, othird = gt.load(members[0], ts[0].capacity, 24, local_rank=6, canonical=5)   # it keeps the tombstones
    digest_before = [t.digest_rows(n, T, state=True) for t in ts]
    assert all(np.array_equal(d, digest_before[0]) for d in digest_before)
    listed_before = ts[0].export_since(n, 0).columns()[0]
    res, flags, wflags = check(ts, os_, n, B, "purge")
    ids = np.flatnonzero(wflags).astype(np.uint32)
    assert res["n_purged"] == len(ids) > n // 8
    for t in ts[1:]:                                     # converged before, converged after
        d, _ = ts[0].diff_table(t, n)
        assert (d["n_a_ahead"], d["n_b_ahead"], d["n_conflict"]) == (0, 0, 0)
    digest_after = [t.digest_rows(n, T, state=True) for t in ts]
    assert all(np.array_equal(d, digest_after[0]) for d in digest_after)
    assert not np.array_equal(digest_after[0], digest_before[0])
    for t in ts:
        listed = t.export_since(n, 0).columns()[0]
        assert not np.isin(ids, listed).any() and np.array_equal(np.union1d(listed, ids), listed_before)
        key, lt, _, val, mod = t.export_flagged(n, flags, 1).columns()
        assert np.array_equal(key, ids) and np.all(mod == ABSENT_MOD) and np.all(val == 0x80808080)
    # a replica that still holds the tombstones hands them back
    ores, orf, _ = tc.oracle_merge_table(os_[0], othird, n, 0, tc.MERGE_WALL)
    mres, rf = ts[0].merge_table(third, n, 0, tc.MERGE_WALL, row_flags=True)
    for f in gt.RESULT_FIELDS:
        assert mres[f] == ores[f], f
    assert mres["n_won"] == len(ids) and np.array_equal(rf.cpu().numpy(), wflags) and np.array_equal(orf, wflags)
    gt.assert_rows(ts[0], os_[0], "stored again")
    lt, rank, val, _ = ts[0].read_rows(ids)
    assert np.all(val == NULL) and np.array_equal(lt, othird.rows["lt"][ids]) and np.array_equal(rank, othird.rows["rank"][ids])
    close(ts, [third])
