"""crdt_diff_tables / crdt_digest_rows (DeviceTable.diff_table, digest_rows) on the GPU against the numpy model
of tests/_diff_cases.py, and against the existing merge as oracle: diff bit 0 is merge_table's row flags,
n_a_ahead its n_won, export_flagged of the diff's flags the records it stores, and the STATE digests are equal
exactly where the diff is zero.  Everything is integer data: every comparison is exact."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import tests.test_gpu_table_merge as gt
from crdt_amd import CrdtNativeError, DeviceTable, _capi
from tests import _diff_cases as dc
from tests import _table_cases as tc
from tests._cases import ABSENT_MOD

pytestmark = pytest.mark.gpu

T = dc.T
MW = tc.MERGE_WALL
SHAPES = (0, 1, T - 1, T, T + 1, 5 * T + 9)
STRIDES = [(24, 24), (32, 32), (24, 32)]
ABOVE_FILL = int(ABSENT_MOD) + 1


def below(rows: dict, limit: int) -> dict:
    """The rows with an id under ``limit``: the table's high-water mark ends up under it too."""
    keep = rows["ids"] < limit
    return {k: (v[keep] if k in ("ids", "lt", "rank", "val", "mod") else v) for k, v in rows.items()}


def load_pair(n_rows: int, seed: int, strides=(24, 24), caps=(37, 64), clip_b=True):
    """(a, oracle mirror of a, b, mirror of b): both capacities above n_rows, b written below n_rows only."""
    ra, rb = dc.gen_diff_pair(n_rows, seed)
    if clip_b:
        rb = below(rb, n_rows - n_rows // 8)
    c0 = dc.max_lt(ra, rb)
    a, oa = gt.load(ra, max(n_rows, 16) + caps[0], strides[0], local_rank=6, canonical=c0)
    b, ob = gt.load(rb, max(n_rows, 16) + caps[1], strides[1], local_rank=tc.DST_RANK, canonical=c0)
    return a, oa, b, ob


def assert_untouched(t: DeviceTable, o, plan, tag):
    gt.assert_rows(t, o, tag)                            # the rows and the canonical
    assert t.last_plan() == plan, tag
    # the high-water mark is where it was: an export above the fill's mod selects no fill row
    assert np.array_equal(t.export_since(t.capacity, ABOVE_FILL).columns()[0], o.modified_since(t.capacity, ABOVE_FILL)), tag


def check_diff(a, oa, b, ob, n_rows: int, tag, flags=True):
    want_flags, want = dc.model_diff(oa.rows, ob.rows, n_rows)
    d, got = a.diff_table(b, n_rows, flags=flags)
    assert d == want, (tag, d, want)
    if flags is True:
        assert str(got.device) == "cuda:0" and got.dtype == torch.uint8 and len(got) == n_rows, tag
        assert np.array_equal(got.cpu().numpy(), want_flags), tag
    return d, got, want_flags


# ------------------------------------------------------------------ 1. shapes
@pytest.mark.parametrize("strides", STRIDES)
@pytest.mark.parametrize("n_rows", SHAPES)
def test_diff_shapes(gpu_device, n_rows, strides):
    a, oa, b, ob = load_pair(n_rows, 100 + n_rows, strides)
    plans = a.last_plan(), b.last_plan()
    d, _, want_flags = check_diff(a, oa, b, ob, n_rows, (n_rows, strides))
    if n_rows >= dc.PLANT_FROM:
        assert d["n_a_ahead"] and d["n_b_ahead"] and d["n_conflict"] and d["first_diff"] == 0
        assert np.mean(want_flags == 0) >= 0.40
    if n_rows == 0:
        assert d == dict(zip(dc.FIELDS, (0, 0, 0, 0, 0, dc.NONE)))
    # the other way round: the two bits swap; and without flags: the same struct
    ds, _, _ = check_diff(b, ob, a, oa, n_rows, (n_rows, strides, "swapped"))
    assert (ds["n_a_ahead"], ds["n_b_ahead"], ds["n_conflict"]) == (d["n_b_ahead"], d["n_a_ahead"], d["n_conflict"])
    assert a.diff_table(b, n_rows)[0] == d and a.diff_table(b, n_rows)[1] is None
    assert_untouched(a, oa, plans[0], (n_rows, strides, "a"))
    assert_untouched(b, ob, plans[1], (n_rows, strides, "b"))
    a.close()
    b.close()


@functools.lru_cache(maxsize=1)
def large_rows():
    return dc.gen_diff_pair(dc.LARGE, 7)


@pytest.fixture(scope="module")
def large(gpu_device):
    """The shape with more tiles than workgroups, loaded once (the tests below only read the two tables)."""
    ra, rb = large_rows()
    c0 = dc.max_lt(ra, rb)
    a, oa = gt.load(ra, dc.LARGE + 3, 24, local_rank=6, canonical=c0)
    b, ob = gt.load(rb, dc.LARGE + 11, 32, local_rank=tc.DST_RANK, canonical=c0)
    yield a, oa, b, ob
    a.close()
    b.close()


def test_diff_more_tiles_than_workgroups(large):
    a, oa, b, ob = large
    assert dc.LARGE > _capi.DIFF_GRID * T
    d, _, want_flags = check_diff(a, oa, b, ob, dc.LARGE, "large")
    assert want_flags[-1] == dc.A_AHEAD and d["first_diff"] == 0 and d["n_conflict"] > 1000


def test_first_diff_in_the_last_row_then_in_row_0(large):
    a, oa, _, _ = large
    n = dc.LARGE
    twin, otwin = gt.load(large_rows()[0], n, 24, local_rank=6, canonical=a.canonical)
    assert a.diff_table(twin, n)[0] == dict(zip(dc.FIELDS, (0, 0, 0, *[len(oa.modified_since(n, 0))] * 2, dc.NONE)))
    last = np.array([n - 1], np.uint32)
    lt, rank, val, mod = (c.copy() for c in twin.read_rows(last))
    twin.put_rows(last, lt + 1, rank, val, mod)          # the only difference: the last row, twin ahead
    d, flags = a.diff_table(twin, n, flags=True)
    assert (d["n_a_ahead"], d["n_b_ahead"], d["n_conflict"], d["first_diff"]) == (0, 1, 0, n - 1)
    assert torch.count_nonzero(flags).item() == 1 and flags[n - 1].item() == dc.B_AHEAD
    first = np.array([0], np.uint32)
    lt, rank, val, mod = (c.copy() for c in twin.read_rows(first))
    twin.put_rows(first, lt, rank, val + 1, mod)         # ... and row 0, a conflict
    d, flags = a.diff_table(twin, n, flags=True)
    assert (d["n_a_ahead"], d["n_b_ahead"], d["n_conflict"], d["first_diff"]) == (0, 1, 1, 0)
    assert flags[0].item() == dc.CONFLICT and torch.count_nonzero(flags).item() == 2
    twin.close()


# ------------------------------------------------------------------ 2. where the flags live
def test_flags_in_host_and_device_memory_and_unaligned(gpu_device):
    n = 3 * T + 17
    a, oa, b, ob = load_pair(n, 41)
    want_flags, want = dc.model_diff(oa.rows, ob.rows, n)
    host = np.full(n + 9, 0x5A, np.uint8)
    d, got = a.diff_table(b, n, flags=host)
    assert got is host and d == want
    assert np.array_equal(host[:n], want_flags) and np.all(host[n:] == 0x5A)
    for off in (0, 1, 7):
        base = torch.full((off + n + 9,), 0x5A, dtype=torch.uint8, device="cuda:0")
        d, got = a.diff_table(b, n, flags=base[off:])
        got = base.cpu().numpy()
        assert d == want and np.array_equal(got[off:off + n], want_flags), off
        assert np.all(got[:off] == 0x5A) and np.all(got[off + n:] == 0x5A), off
    # whole runs of equal rows (their zeros go out as wider stores where the bytes are aligned): a against a table
    # that differs from it in three rows, at every alignment and with a partial last run
    twin, _ = gt.load(dc.gen_diff_pair(n, 41)[0], a.capacity, 32, local_rank=6, canonical=a.canonical)
    odd = np.array([0, T + 63, n - 1], np.uint32)
    lt, rank, val, mod = twin.read_rows(odd)
    twin.put_rows(odd, lt + 1, rank, val, np.abs(mod))
    sparse = np.zeros(n, np.uint8)
    sparse[odd] = dc.B_AHEAD
    for off in (0, 1, 4, 7, 8):
        for m in (n, n - 1, n - 17, T + 64, 64, 63):
            base = torch.full((off + n + 9,), 0x5A, dtype=torch.uint8, device="cuda:0")
            d, _ = a.diff_table(twin, m, flags=base[off:])
            got = base.cpu().numpy()
            assert np.array_equal(got[off:off + m], sparse[:m]) and d["n_b_ahead"] == int(sparse[:m].sum()) // 2, (off, m)
            assert np.all(got[:off] == 0x5A) and np.all(got[off + m:] == 0x5A), (off, m)
    twin.close()
    for m in (n - 1, 2 * T, T + 1, 5, 0):                # fewer rows than the tables hold: nothing past them is written
        base = torch.full((n,), 0x5A, dtype=torch.uint8, device="cuda:0")
        d, _ = a.diff_table(b, m, flags=base)
        wf, w = dc.model_diff(oa.rows, ob.rows, m)
        got = base.cpu().numpy()
        assert d == w and np.array_equal(got[:m], wf) and np.all(got[m:] == 0x5A), m
    a.close()
    b.close()


# ------------------------------------------------------------------ 3. the diff predicts the merge
@pytest.mark.parametrize("strides", [(24, 24), (24, 32)])
@pytest.mark.parametrize("n_rows", [T + 1, 5 * T + 9])
def test_diff_predicts_merge_table(gpu_device, n_rows, strides):
    a, oa, b, ob = load_pair(n_rows, 55 + n_rows, strides, clip_b=False)
    d, flags, want_flags = check_diff(a, oa, b, ob, n_rows, "before")
    # the changeset b lacks, fetched before the merge
    key, lt, rank, val, _ = a.export_flagged(n_rows, flags, _capi.DIFF_A_AHEAD).columns()
    assert len(key) == d["n_a_ahead"] > 0 and np.array_equal(key, np.flatnonzero(want_flags & 1))
    ores, oflags, _ = tc.oracle_merge_table(ob, oa, n_rows, 0, MW)
    res, rf = b.merge_table(a, n_rows, 0, MW, row_flags=True)
    assert res["status"] == ores["status"] == 0 and b.last_plan()["table"]
    assert res["n_won"] == d["n_a_ahead"] == ores["n_won"]
    assert torch.equal(rf, flags & 1) and np.array_equal(oflags, want_flags & 1)
    gt.assert_rows(b, ob, "merged")
    got = b.read_rows(key)                               # exactly the records b stored
    assert np.array_equal(got[0], lt) and np.array_equal(got[1], rank) and np.array_equal(got[2], val)
    assert np.array_equal(got[3], ob.rows["mod"][key])
    plan = b.last_plan()
    d2, flags2, _ = check_diff(a, oa, b, ob, n_rows, "after")
    assert (d2["n_a_ahead"], d2["n_b_ahead"], d2["n_conflict"]) == (0, d["n_b_ahead"], d["n_conflict"])
    assert torch.equal(flags2, flags & 6)
    assert b.last_plan() == plan and b.last_path() == "gather"
    a.close()
    b.close()


def test_a_table_against_itself(gpu_device):
    n = 2 * T + 5
    a, oa, b, ob = load_pair(n, 77)
    d, flags = a.diff_table(a, n, flags=True)
    vis = len(oa.modified_since(n, 0))
    assert d == dict(zip(dc.FIELDS, (0, 0, 0, vis, vis, dc.NONE))) and not flags.any().item()
    gt.assert_rows(a, oa, "self")
    a.close()
    b.close()


# ------------------------------------------------------------------ 4. refused calls
def test_refused_calls_touch_nothing(gpu_device):
    n = T + 9
    a, oa, b, ob = load_pair(n, 88, caps=(37, 64))
    lib, E, D, H = a._lib, _capi.CRDT_E_INVALID, _capi.CRDT_MEM_DEVICE, _capi.CRDT_MEM_HOST
    out = _capi.CrdtDiff()
    ctypes.memset(ctypes.byref(out), 0x5A, ctypes.sizeof(out))
    poisoned = bytes(out)
    dflags = torch.full((b.capacity + 8,), 0x5A, dtype=torch.uint8, device="cuda:0")
    hflags = np.full(b.capacity + 8, 0x5A, np.uint8)
    torch.cuda.synchronize()
    dp, hp = ctypes.c_void_p(dflags.data_ptr()), hflags.ctypes.data_as(ctypes.c_void_p)
    from tests._loopback import LoopbackComm
    joined = DeviceTable(0, local_rank=4, capacity=n)
    joined.comm_init_ops(2, 0, LoopbackComm(2))          # rank 0 of a loopback communicator
    assert a.capacity < b.capacity
    call = lib.crdt_diff_tables
    refused = [
        call(None, b._ctx, n, dp, D, ctypes.byref(out)), call(a._ctx, None, n, dp, D, ctypes.byref(out)),
        call(a._ctx, b._ctx, n, dp, D, None),
        call(a._ctx, b._ctx, a.capacity + 1, dp, D, ctypes.byref(out)),      # above a's capacity, inside b's
        call(b._ctx, a._ctx, a.capacity + 1, dp, D, ctypes.byref(out)),
        call(a._ctx, b._ctx, n, dp, 7, ctypes.byref(out)), call(a._ctx, b._ctx, n, hp, -1, ctypes.byref(out)),
        call(a._ctx, joined._ctx, n, dp, D, ctypes.byref(out)), call(joined._ctx, a._ctx, n, hp, H, ctypes.byref(out)),
    ]
    assert refused == [E] * len(refused)
    assert bytes(out) == poisoned and np.all(hflags == 0x5A) and torch.all(dflags == 0x5A).item()
    assert call(a._ctx, b._ctx, n, None, 7, ctypes.byref(out)) == 0          # (a bad flags_mem without a pointer is unused)
    assert {f: getattr(out, f) for f in dc.FIELDS} == dc.model_diff(oa.rows, ob.rows, n)[1]
    words = np.full(4, 0x5A5A, np.uint64)
    wp = words.ctypes.data_as(ctypes.c_void_p)
    dig = lib.crdt_digest_rows
    refused = [dig(None, n, T, 0, wp, H), dig(a._ctx, n, T, 0, None, H), dig(a._ctx, a.capacity + 1, 1 << 20, 0, wp, H),
               dig(a._ctx, n, T // 2, 0, wp, H), dig(a._ctx, n, 3 * T, 0, wp, H), dig(a._ctx, n, 0, 0, wp, H),
               dig(a._ctx, n, T, 2, wp, H), dig(a._ctx, n, T, -1, wp, H), dig(a._ctx, n, T, 0, wp, 2),
               dig(joined._ctx, n, T, 0, wp, H)]
    assert refused == [E] * len(refused) and np.all(words == 0x5A5A)
    assert dig(a._ctx, 0, T, 1, None, H) == 0
    other = DeviceTable(0, capacity=16)
    other.device = 1                                     # (as if it had been created on another GPU)
    with pytest.raises(ValueError):
        a.diff_table(other, 16)
    other.device = 0
    with pytest.raises(CrdtNativeError) as e:
        a.diff_table(other, other.capacity + 1)
    assert e.value.status == E
    with pytest.raises(CrdtNativeError) as e:
        a.digest_rows(n, block_rows=1000)
    assert e.value.status == E
    gt.assert_rows(a, oa, "a untouched")
    gt.assert_rows(b, ob, "b untouched")
    for t in (a, b, joined, other):
        t.close()


# ------------------------------------------------------------------ 5. digests
@pytest.mark.parametrize("row_bytes", [24, 32])
@pytest.mark.parametrize("n_rows", [0, 1, T + 1, 5 * T + 9])
def test_rows_digest(gpu_device, n_rows, row_bytes):
    """Every row as stored, the fill above the high-water mark included, at bench's block and at one tile."""
    rows = below(dc.gen_diff_pair(n_rows, 300 + n_rows)[0], n_rows - n_rows // 4)
    t, o = gt.load(rows, max(n_rows, 16) + 5, row_bytes, canonical=9)
    plan = t.last_plan()
    for block in (1 << 20, T, 1 << 40):
        for state in (False, True):
            got = t.digest_rows(n_rows, block, state=state)
            assert got.dtype == np.uint64 and np.array_equal(got, dc.model_digest(o.rows, n_rows, block, state)), (block, state)
    if n_rows > T:
        assert not np.array_equal(t.digest_rows(n_rows, T), t.digest_rows(n_rows, T, state=True))
    assert_untouched(t, o, plan, "digest")
    t.close()


def test_digests_more_tiles_than_workgroups_and_into_device_memory(large):
    a, oa, b, ob = large
    n = dc.LARGE
    for t, o in ((a, oa), (b, ob)):
        for block, state in ((1 << 20, False), (T, False), (1 << 20, True), (4 * T, True)):
            want = dc.model_digest(o.rows, n, block, state)
            assert len(want) == -(-n // block) > 1
            assert np.array_equal(t.digest_rows(n, block, state=state), want), (block, state)
    words = torch.full((-(-n // T) + 3,), 0x5A5A, dtype=torch.int64, device="cuda:0")   # the words left on the device
    torch.cuda.synchronize()
    st = a._lib.crdt_digest_rows(a._ctx, n, T, _capi.DIGEST_ROWS, ctypes.c_void_p(words.data_ptr()), _capi.CRDT_MEM_DEVICE)
    got = words.cpu().numpy().view(np.uint64)
    assert st == 0 and np.array_equal(got[:-3], dc.model_digest(oa.rows, n, T, False)) and np.all(got[-3:] == 0x5A5A)


def test_state_digests_follow_the_diff(gpu_device):
    """Equal visible state in a 24-B and a 32-B table of different capacities gives equal STATE words; between
    the pair's two tables the words differ in exactly the blocks the diff's flags mark."""
    n = 5 * T + 9
    a, oa, b, ob = load_pair(n, 99, strides=(24, 32), caps=(5, 3 * T))
    _, flags, _ = check_diff(a, oa, b, ob, n, "pair")
    blocks = np.zeros(-(-n // T), bool)
    blocks[torch.nonzero(flags).cpu().numpy().ravel() // T] = True
    sa, sb = a.digest_rows(n, T, state=True), b.digest_rows(n, T, state=True)
    assert blocks.any() and np.array_equal(sa != sb, blocks)
    # a third table takes a's visible records under stamps of its own, and garbage where a is invisible
    ids = oa.modified_since(n, 0)
    c, oc = gt.load({"ids": ids, "lt": oa.rows["lt"][ids], "rank": oa.rows["rank"][ids], "val": oa.rows["val"][ids],
                     "mod": np.arange(len(ids), dtype=np.int64), "clear": (0, 0)}, 4 * n, 32, canonical=5)
    hidden = np.setdiff1d(np.arange(n, dtype=np.uint32), ids)[::3]
    c.put_rows(hidden, np.full(len(hidden), 77, np.int64), np.zeros(len(hidden), np.uint32),
               np.full(len(hidden), 5, np.uint32), np.full(len(hidden), -9, np.int64))
    d, _ = a.diff_table(c, n)
    assert (d["n_a_ahead"], d["n_b_ahead"], d["n_conflict"], d["first_diff"]) == (0, 0, 0, dc.NONE)
    for block in (T, 1 << 20):
        assert np.array_equal(a.digest_rows(n, block, state=True), c.digest_rows(n, block, state=True))
    assert not np.array_equal(a.digest_rows(n, T), c.digest_rows(n, T))
    for t in (a, b, c):
        t.close()
