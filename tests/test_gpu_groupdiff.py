"""crdt_diff_group (DeviceTable.diff_group) on the GPU against the numpy model of tests/_group_cases.py, against the
pairwise crdt_diff_tables, the STATE digests and crdt_export_flagged as the header relates them, and with the
fan-in and fan-out around it.  Everything is integer data: every comparison is exact."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import tests.test_gpu_table_merge as gt
from crdt_amd import CrdtNativeError, DeviceTable, _capi
from tests import _group_cases as gc
from tests import _table_cases as tc
from tests._cases import ABSENT_MOD

pytestmark = pytest.mark.gpu

T = gc.T
MW = tc.MERGE_WALL
ABOVE_FILL = int(ABSENT_MOD) + 1
STRIDES = {"24": (24,), "32": (32,), "mixed": (24, 32, 24)}
ZERO = {"n_held": 0, "n_disputed": 0, "n_conflict": 0, "first_diff": gc.NONE, "n_visible": [0] * 8,
        "n_behind": [0] * 8, "n_sole": [0] * 8}
assert T == _capi.TABLE_TILE and gc.GRID == _capi.DIFF_GRID and max(gc.MEMBERS) == _capi.GROUP_MAX == gc.GROUP_MAX


def load_group(members: list, n_rows: int, strides=(24,), extra: int = 37):
    """(tables, oracle mirrors): member j with row size strides[j % len], local rank 8 + j (above the rows' ranks),
    a canonical above every lt and a capacity of its own above n_rows."""
    c0 = gc.max_lt(members)
    pairs = [gt.load(m, max(n_rows, 16) + extra + 11 * j, strides[j % len(strides)], local_rank=8 + j, canonical=c0)
             for j, m in enumerate(members)]
    return [t for t, _ in pairs], [o for _, o in pairs]


def close(*groups):
    for g in groups:
        for t in g:
            t.close()


def check(ts, os_, n_rows: int, tag, masks=True):
    """One diff_group against the model: the counts and, with masks=True, the three arrays."""
    wb, wh, wc, want = gc.model_group([o.rows for o in os_], n_rows)
    d, behind, hold, conflict = ts[0].diff_group(ts[1:], n_rows, masks=masks)
    assert d == want, (tag, d, want)
    if masks is True:
        for got, w, name in ((behind, wb, "behind"), (hold, wh, "hold"), (conflict, wc, "conflict")):
            assert str(got.device) == "cuda:0" and got.dtype == torch.uint8 and len(got) == n_rows, (tag, name)
            assert np.array_equal(got.cpu().numpy(), w), (tag, name)
    return d, (behind, hold, conflict), (wb, wh, wc)


def state_of(ts):
    return [(t.last_plan(), t.last_path(), t.timing()) for t in ts]


def assert_untouched(ts, os_, state, tag):
    for j, (t, o, s) in enumerate(zip(ts, os_, state)):
        gt.assert_rows(t, o, (tag, j))                   # the rows and the canonical
        assert (t.last_plan(), t.last_path(), t.timing()) == s, (tag, j)
        # the high-water mark is where it was: an export above the fill's mod selects no fill row
        assert np.array_equal(t.export_since(t.capacity, ABOVE_FILL).columns()[0],
                              o.modified_since(t.capacity, ABOVE_FILL)), (tag, j)


# ------------------------------------------------------------------ 1. shapes
@pytest.mark.parametrize("strides", list(STRIDES))
@pytest.mark.parametrize("n_ctx", gc.MEMBERS)
@pytest.mark.parametrize("n_rows", gc.SHAPES)
def test_shapes(gpu_device, n_rows, n_ctx, strides):
    members = gc.gen_group(n_rows, n_ctx, 100 + n_rows + n_ctx)
    ts, os_ = load_group(members, n_rows, STRIDES[strides])
    assert len({t.capacity for t in ts}) == n_ctx
    state = state_of(ts)
    views = [t.export_since(n_rows, int(tc.STAMPS[20])) for t in ts]
    cols = [v.columns() for v in views]
    tag = (n_rows, n_ctx, strides)
    d, _, (wb, wh, wc) = check(ts, os_, n_rows, tag)
    assert not np.any(wb & wh)
    if n_rows >= gc.PLANT_FROM:
        assert np.mean((wb == 0) & (wc == 0)) >= 0.40 and d["n_held"] > n_rows // 2
        if n_ctx >= 2:
            assert d["n_disputed"] and d["n_conflict"] and d["first_diff"] == 0 and all(d["n_behind"][:n_ctx])
        if n_ctx >= 3:
            assert wc[gc.OVERRULED] == 0 and wh[gc.OVERRULED] == 4
    if n_rows == 0:
        assert d == ZERO
    if n_ctx == 1:                                       # one member: hold is what it sees
        assert d["n_disputed"] == d["n_conflict"] == 0 and d["n_sole"][0] == d["n_visible"][0] == d["n_held"]
    none = ts[0].diff_group(ts[1:], n_rows)              # without the arrays: the same struct
    assert none[0] == d and none[1:] == (None, None, None)
    for v, c in zip(views, cols):                        # the views taken before the calls read back their old columns
        for a, b in zip(v.columns(), c):
            assert np.array_equal(a, b)
    assert_untouched(ts, os_, state, tag)
    close(ts)


@functools.lru_cache(maxsize=1)
def large_rows():
    return gc.gen_group(gc.LARGE, 3, 7)


def bare(rows: dict, capacity: int, row_bytes: int = 24, canonical: int = 0) -> DeviceTable:
    """The rows in a DeviceTable without a mirror."""
    t = DeviceTable(0, local_rank=9, capacity=capacity)
    if row_bytes != 24:
        t.set_row_bytes(row_bytes)
    t.put_rows(*(rows[k] for k in ("ids", "lt", "rank", "val", "mod")))
    first, count = rows["clear"]
    if count:
        t.clear_rows(first, count)
    t.canonical = canonical
    return t


@pytest.fixture(scope="module")
def large(gpu_device):
    """The shape with more tiles than workgroups, loaded once (the tests below only read the three tables)."""
    ts, os_ = load_group(large_rows(), gc.LARGE, STRIDES["mixed"], extra=3)
    yield ts, os_
    close(ts)


def test_more_tiles_than_workgroups(large):
    ts, os_ = large
    assert gc.LARGE > _capi.DIFF_GRID * T
    d, _, (wb, _, wc) = check(ts, os_, gc.LARGE, "large")
    assert d["first_diff"] == 0 and d["n_conflict"] > 1000 and wb[-1] != 0 and min(d["n_sole"][:3]) > 1000


def test_first_diff_in_the_last_row_then_in_row_0(large):
    ts, os_ = large
    n, a = gc.LARGE, ts[0]
    twins = [bare(large_rows()[0], n + j, rb, a.canonical) for j, rb in ((0, 32), (5, 24))]
    vis = len(os_[0].modified_since(n, 0))
    d = a.diff_group(twins, n)[0]
    assert d == dict(ZERO, n_held=vis, n_visible=[vis] * 3 + [0] * 5)
    last = np.array([n - 1], np.uint32)
    lt, rank, val, mod = (c.copy() for c in twins[1].read_rows(last))
    twins[1].put_rows(last, lt + 1, rank, val, np.abs(mod))      # the only difference: the last row, member 2 ahead
    d, behind, hold, conflict = a.diff_group(twins, n, masks=True)
    assert (d["n_disputed"], d["n_conflict"], d["first_diff"]) == (1, 0, n - 1)
    assert d["n_behind"][:3] == [1, 1, 0] and d["n_sole"][:3] == [0, 0, 1]
    assert torch.count_nonzero(behind).item() == 1 and (behind[n - 1].item(), hold[n - 1].item()) == (3, 4)
    assert not conflict.any().item()
    first = np.array([0], np.uint32)
    lt, rank, val, mod = (c.copy() for c in twins[0].read_rows(first))
    twins[0].put_rows(first, lt, rank, val + 1, mod)             # ... and row 0, a conflict
    d, behind, hold, conflict = a.diff_group(twins, n, masks=True)
    assert (d["n_disputed"], d["n_conflict"], d["first_diff"]) == (1, 1, 0)
    assert torch.count_nonzero(conflict).item() == 1 and (conflict[0].item(), behind[0].item()) == (1, 0)
    assert hold[0].item() == 7
    close(twins)


# ------------------------------------------------------------------ 2. where the arrays live
def test_arrays_in_host_and_device_memory_unaligned_alone_and_none(gpu_device):
    n = 3 * T + 17
    ts, os_ = load_group(gc.gen_group(n, 3, 41), n, STRIDES["mixed"])
    wb, wh, wc, want = gc.model_group([o.rows for o in os_], n)
    wants = (wb, wh, wc)
    host = [np.full(n + 9, 0x5A, np.uint8) for _ in range(3)]
    d, *got = ts[0].diff_group(ts[1:], n, masks=tuple(host))
    assert d == want and all(g is h for g, h in zip(got, host))
    for h, w in zip(host, wants):
        assert np.array_equal(h[:n], w) and np.all(h[n:] == 0x5A)
    for off in (1, 3, 8):
        base = [torch.full((off + n + 9,), 0x5A, dtype=torch.uint8, device="cuda:0") for _ in range(3)]
        d = ts[0].diff_group(ts[1:], n, masks=tuple(b[off + k:] for k, b in enumerate(base)))[0]
        assert d == want
        for k, (b, w) in enumerate(zip(base, wants)):
            g, o = b.cpu().numpy(), off + k
            assert np.array_equal(g[o:o + n], w) and np.all(g[:o] == 0x5A) and np.all(g[o + n:] == 0x5A), (off, k)
    for k in range(3):                                   # each array alone, in device and in host memory
        for make in (lambda: torch.full((n + 9,), 0x5A, dtype=torch.uint8, device="cuda:0"),
                     lambda: np.full(n + 9, 0x5A, np.uint8)):
            arr = make()
            masks = [None, None, None]
            masks[k] = arr
            d, *got = ts[0].diff_group(ts[1:], n, masks=tuple(masks))
            g = arr.cpu().numpy() if torch.is_tensor(arr) else arr
            assert d == want and np.array_equal(g[:n], wants[k]) and np.all(g[n:] == 0x5A), k
            assert [x is None for x in got] == [j != k for j in range(3)]
    with pytest.raises(ValueError):                      # one memory for the arrays that are passed
        ts[0].diff_group(ts[1:], n, masks=(host[0], torch.zeros(n, dtype=torch.uint8, device="cuda:0"), None))
    # whole runs of equal bytes go out as wider stores where aligned: converged tables that differ in three rows,
    # at every alignment and with a partial last run
    members = gc.gen_group(n, 1, 42) * 3
    cs, _ = load_group(members, n, STRIDES["mixed"])
    odd = np.array([0, T + 63, n - 1], np.uint32)
    lt, rank, val, mod = cs[2].read_rows(odd)
    cs[2].put_rows(odd, lt + 1, rank, val, np.abs(mod))
    seen = np.zeros(cs[0].capacity, bool)
    seen[cs[0].export_since(n, 0).columns()[0]] = True
    seen[odd] = True
    sparse_b, sparse_h = np.zeros(n, np.uint8), np.where(seen[:n], 7, 0).astype(np.uint8)
    sparse_b[odd], sparse_h[odd] = 3, 4
    for off in (0, 1, 4, 7, 8):
        for m in (n, n - 1, n - 17, T + 64, 64, 63):
            base = [torch.full((off + n + 9,), 0x5A, dtype=torch.uint8, device="cuda:0") for _ in range(3)]
            d = cs[0].diff_group(cs[1:], m, masks=tuple(b[off:] for b in base))[0]
            assert d["n_disputed"] == int(np.count_nonzero(sparse_b[:m])) and d["n_conflict"] == 0, (off, m)
            for b, w in zip(base, (sparse_b, sparse_h, np.zeros(n, np.uint8))):
                g = b.cpu().numpy()
                assert np.array_equal(g[off:off + m], w[:m]), (off, m)
                assert np.all(g[:off] == 0x5A) and np.all(g[off + m:] == 0x5A), (off, m)
    close(ts, cs)


# ------------------------------------------------------------------ 3. refused calls
def test_refused_calls_touch_nothing(gpu_device):
    n = T + 9
    ts, os_ = load_group(gc.gen_group(n, 3, 88), n, STRIDES["mixed"])
    a, b, c = ts
    state = state_of(ts)
    lib, E, D, H = a._lib, _capi.CRDT_E_INVALID, _capi.CRDT_MEM_DEVICE, _capi.CRDT_MEM_HOST
    out = _capi.CrdtGroupDiff()
    ctypes.memset(ctypes.byref(out), 0x5A, ctypes.sizeof(out))
    poisoned = bytes(out)
    dflags = torch.full((3 * (c.capacity + 8),), 0x5A, dtype=torch.uint8, device="cuda:0")
    hflags = np.full(3 * (c.capacity + 8), 0x5A, np.uint8)
    torch.cuda.synchronize()
    step = c.capacity + 8
    dp = [ctypes.c_void_p(dflags.data_ptr() + k * step) for k in range(3)]
    hp = [ctypes.c_void_p(hflags.ctypes.data + k * step) for k in range(3)]
    po = ctypes.byref(out)
    from tests._loopback import LoopbackComm
    joined = DeviceTable(0, local_rank=4, capacity=n)
    joined.comm_init_ops(2, 0, LoopbackComm(2))          # rank 0 of a loopback communicator
    assert a.capacity < b.capacity < c.capacity

    def arr(*tables):
        return (ctypes.c_void_p * max(len(tables), 1))(*(t._ctx.value if t is not None else None for t in tables))

    call = lib.crdt_diff_group
    more = [DeviceTable(0, capacity=16) for _ in range(6)]
    refused = [
        call(None, 1, n, *dp, D, po), call(arr(a, b), 2, n, *dp, D, None),
        call(arr(a, None, b), 3, n, *dp, D, po), call(arr(None), 1, n, *dp, D, po),
        call(arr(a), 0, n, *dp, D, po), call(arr(a, b, c, *more), 9, 16, *dp, D, po),
        call(arr(a, b, a), 3, n, *dp, D, po), call(arr(a, a), 2, n, *dp, D, po),
        call(arr(b, a), 2, a.capacity + 1, *dp, D, po),                  # above a's capacity, inside b's
        call(arr(a, b), 2, a.capacity + 1, *dp, D, po),
        call(arr(a, b), 2, n, *dp, 7, po), call(arr(a, b), 2, n, *hp, -1, po),
        call(arr(a, b), 2, n, dp[0], None, None, 7, po), call(arr(a, b), 2, n, None, dp[1], None, 7, po),
        call(arr(a, b), 2, n, None, None, hp[2], 9, po),                 # a bad flags_mem with any one array
        call(arr(a, joined), 2, n, *dp, D, po), call(arr(joined, a), 2, n, *hp, H, po),
    ]
    assert refused == [E] * len(refused)
    assert bytes(out) == poisoned and np.all(hflags == 0x5A) and torch.all(dflags == 0x5A).item()
    other = DeviceTable(0, capacity=16)
    other.device = 1                                     # (as if it had been created on another GPU)
    with pytest.raises(ValueError):
        a.diff_group([b, other], 16)
    other.device = 0
    with pytest.raises(CrdtNativeError) as e:
        a.diff_group([other], other.capacity + 1)
    assert e.value.status == E
    with pytest.raises(CrdtNativeError) as e:
        a.diff_group([b] + more + [other], 16)           # nine members
    assert e.value.status == E
    assert call(arr(a, b, c), 3, n, None, None, None, 7, po) == 0       # (a bad flags_mem without a pointer is unused)
    want = gc.model_group([o.rows for o in os_], n)[3]
    assert _capi.CrdtGroupDiff.as_dict(out) == want and want["n_disputed"] > 0
    assert_untouched(ts, os_, state, "refused")
    close(ts, more, [joined, other])


# ------------------------------------------------------------------ 4. the header's identities
@pytest.mark.parametrize("strides", ["24", "mixed"])
def test_two_members_are_diff_tables(gpu_device, strides):
    n = 3 * T + 17
    ts, os_ = load_group(gc.gen_group(n, 2, 51), n, STRIDES[strides])
    d, (behind, hold, conflict), _ = check(ts, os_, n, "pair")
    p, flags = ts[0].diff_table(ts[1], n, flags=True)
    assert torch.equal((behind >> 1) & 1, flags & _capi.DIFF_A_AHEAD)
    assert torch.equal(behind & 1, (flags & _capi.DIFF_B_AHEAD) >> 1)
    assert torch.equal(conflict, (flags & _capi.DIFF_CONFLICT) >> 2)
    assert (d["first_diff"], d["n_visible"][0], d["n_visible"][1], d["n_conflict"]) == \
        (p["first_diff"], p["n_visible_a"], p["n_visible_b"], p["n_conflict"])
    assert d["n_behind"][:2] == [p["n_b_ahead"], p["n_a_ahead"]] and p["n_a_ahead"] and p["n_b_ahead"]
    close(ts)


def test_a_holder_against_every_member_is_diff_tables(gpu_device):
    n = 2 * T + 9
    ts, os_ = load_group(gc.gen_group(n, 4, 52), n, STRIDES["mixed"])
    _, (behind, hold, _), _ = check(ts, os_, n, "four")
    for h in range(4):
        rows = ((hold >> h) & 1).bool()
        assert rows.any().item()
        for j in range(4):
            flags = ts[h].diff_table(ts[j], n, flags=True)[1]
            assert torch.equal((flags & _capi.DIFF_A_AHEAD)[rows], ((behind >> j) & 1)[rows]), (h, j)
    close(ts)


def test_state_digests_are_equal_where_nothing_is_disputed(gpu_device):
    n = 5 * T + 9
    ts, os_ = load_group(gc.gen_group(n, 1, 53) * 4, n, STRIDES["mixed"], extra=3 * T)
    seen = os_[0].modified_since(n, 0)
    newer, other = seen[seen > T][:1], seen[seen > 4 * T][:1]    # a row of block 1 and a row of block 4
    for t, o in zip(ts[2:], os_[2:]):
        lt, rank, val, mod = t.read_rows(newer)
        for x in (t, o):
            x.put_rows(newer, lt + 1, rank, val, mod)            # members 2 and 3 are ahead there
    lt, rank, val, mod = ts[3].read_rows(other)
    for x in (ts[3], os_[3]):
        x.put_rows(other, lt, rank, val + 1, mod)                # member 3 holds another value there
    d, (behind, _, conflict), _ = check(ts, os_, n, "four")
    assert (d["n_disputed"], d["n_conflict"], d["n_behind"][:4]) == (1, 1, [1, 1, 0, 0])
    digests = [t.digest_rows(n, T, state=True) for t in ts]
    blocks = np.zeros(-(-n // T), bool)
    blocks[torch.nonzero(behind | conflict).cpu().numpy().ravel() // T] = True
    differ = np.zeros(len(blocks), bool)
    for x in digests[1:]:
        differ |= x != digests[0]
    assert np.array_equal(np.flatnonzero(blocks), [1, 4]) and np.array_equal(differ, blocks)
    # members that hold one visible state under stamps, capacities and row sizes of their own, with garbage where
    # it is invisible: nothing disputed, nothing in conflict, and the same STATE words
    ids = os_[0].modified_since(n, 0)
    same = []
    for j in range(3):
        rows = {"ids": ids, "lt": os_[0].rows["lt"][ids], "rank": os_[0].rows["rank"][ids], "val": os_[0].rows["val"][ids],
                "mod": np.arange(len(ids), dtype=np.int64) + j, "clear": (0, 0)}
        t = bare(rows, n + 100 * j + 16, (24, 32, 24)[j], 5)
        hidden = np.setdiff1d(np.arange(n, dtype=np.uint32), ids)[j::3]
        t.put_rows(hidden, np.full(len(hidden), 77 + j, np.int64), np.zeros(len(hidden), np.uint32),
                   np.full(len(hidden), 5 + j, np.uint32), np.full(len(hidden), -9 - j, np.int64))
        same.append(t)
    d = same[0].diff_group(same[1:], n)[0]
    assert (d["n_disputed"], d["n_conflict"], d["first_diff"], d["n_held"]) == (0, 0, gc.NONE, len(ids))
    assert d["n_sole"] == d["n_behind"] == [0] * 8
    words = [t.digest_rows(n, T, state=True) for t in same]
    assert all(np.array_equal(w, words[0]) for w in words[1:])
    close(ts, same)


def test_the_arrays_feed_export_flagged(gpu_device):
    n = 3 * T + 17
    ts, os_ = load_group(gc.gen_group(n, 3, 54), n, STRIDES["mixed"])
    d, (behind, hold, conflict), (wb, wh, wc) = check(ts, os_, n, "three")
    for j in range(3):                                   # the keys member j is behind on, read against any member
        for t in ts:
            key = t.export_flagged(n, behind, 1 << j).columns()[0]
            assert np.array_equal(key, np.flatnonzero(wb & (1 << j))) and len(key) == d["n_behind"][j] > 0
    for h in range(3):                                   # the winners member h holds
        ids = np.flatnonzero(wh & (1 << h))
        key, lt, rank, val, _ = ts[h].export_flagged(n, hold, 1 << h).columns()
        assert np.array_equal(key, ids) and np.array_equal(lt, os_[h].rows["lt"][ids])
        assert np.array_equal(rank, os_[h].rows["rank"][ids]) and np.array_equal(val, os_[h].rows["val"][ids])
    ids = np.flatnonzero(wc)
    vals = []
    for t, o in zip(ts, os_):                            # every member's records of the rows in conflict
        key, _, _, val, _ = t.export_flagged(n, conflict, 1).columns()
        assert np.array_equal(key, ids) and np.array_equal(val, o.rows["val"][ids]) and len(ids) == d["n_conflict"] > 0
        vals.append(val)
    held = wh[ids]
    for r in range(len(ids)):                            # two holders of such a row differ
        assert len({int(vals[j][r]) for j in range(3) if (held[r] >> j) & 1}) > 1
    close(ts)


# ------------------------------------------------------------------ 5. with the fan-in and the fan-out around it
@pytest.mark.parametrize("n_ctx,strides", [(3, "24"), (8, "mixed")])
def test_fanin_then_fanout_leaves_nothing_disputed(gpu_device, n_ctx, strides):
    """Member 0 merges every other member, then every other member merges member 0, all at since 0 and under a
    canonical above every lt (nothing raises).  A tie keeps local, so a conflict at the top would stay one: the
    members' values are made a function of their hlc first."""
    n = 2 * T + 9
    members = gc.gen_group(n, n_ctx, 60 + n_ctx)
    for m in members:
        m["val"] = (((m["lt"] >> 16) ^ m["rank"]) & 0xFFFFF).astype(np.uint32)
    ts, os_ = load_group(members, n, STRIDES[strides])
    before = check(ts, os_, n, "before", masks=False)[0]
    assert before["n_disputed"] > n // 8 and before["n_conflict"] == 0 and all(before["n_sole"][:n_ctx])
    res, _ = ts[0].merge_tables(ts[1:], n, [0] * (n_ctx - 1), MW)
    assert all(r["status"] == 0 for r in res)
    res, _ = ts[0].fanout_tables(ts[1:], n, [0] * (n_ctx - 1), MW)
    assert all(r["status"] == 0 for r in res)
    d, behind, hold, conflict = ts[0].diff_group(ts[1:], n, masks=True)
    assert (d["n_disputed"], d["n_conflict"], d["first_diff"]) == (0, 0, gc.NONE)
    assert d["n_held"] == before["n_held"] and d["n_visible"][:n_ctx] == [d["n_held"]] * n_ctx
    assert d["n_behind"] == d["n_sole"] == [0] * 8
    assert not behind.any().item() and not conflict.any().item()
    assert torch.all((hold == 0) | (hold == (1 << n_ctx) - 1)).item()
    words = [t.digest_rows(n, T, state=True) for t in ts]
    assert all(np.array_equal(w, words[0]) for w in words[1:])
    close(ts)
