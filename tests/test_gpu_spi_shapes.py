"""The storage calls at their grid edges: k_put_stamped and k_refresh run capped grids of 2048 x 256
threads with a stride loop, k_key_check reads 16-B vectors between a scalar head and tail.  put_stamped
and refresh_canonical at one row, around a wave (64), a block (256), the whole grid (524288) and into the
loop's second trip (1048581), for both row sizes, against the C restatement; a key at the capacity seen by
k_key_check's head, body and tail; remap_ranks and a clear_rows that straddles the high-water mark.
Everything is integer data: every comparison is exact."""
import functools

import numpy as np
import pytest

import tests.test_gpu_export as gx
from crdt_amd import CrdtNativeError, DeviceTable, _capi
from oracle.oracle_c import OracleTable, new_table
from tests._cases import NULL, WALL

pytestmark = pytest.mark.gpu

GRID = 2048 * 256                                    # threads of the capped put / refresh grids
SIZES = [0, 1, 63, 64, 65, 255, 256, 257, GRID - 1, GRID, GRID + 1, 2 * GRID + 5]
I64_MIN = -(1 << 63)
LOCAL_RANK = 3
C0 = ((WALL - 5) << 16) + 7                          # the canonical before the put
COLS = ("lt", "rank", "val", "mod")
RESULT_FIELDS = gx.RESULT_FIELDS


def extra_rows(n):
    """Three rows above the ids a call writes: they must come through it unchanged."""
    ids = np.arange(n, n + 3, dtype=np.uint32)
    return (ids, np.array([5 << 16, 6 << 16, 7 << 16], np.int64), np.array([1, 2, 9], np.uint32),
            np.array([11, NULL, 13], np.uint32), np.array([5 << 16, -(1 << 20), 7 << 16], np.int64))


def fresh(n, row_bytes):
    t = DeviceTable(0, local_rank=LOCAL_RANK, capacity=n + 3)
    if row_bytes != 24:
        t.set_row_bytes(row_bytes)
    t.put_rows(*extra_rows(n))
    t.canonical = C0
    return t


def read_all(t):
    return t.read_rows(np.arange(t.capacity, dtype=np.uint32))


def dev(a):
    import torch
    return torch.from_numpy(np.array(a.view(np.int32) if a.dtype == np.uint32 else a)).to("cuda:0")


@functools.lru_cache(maxsize=None)
def put_case(n):
    """(keys, values, the restatement's result, its rows, its canonical) of one put_stamped of n shuffled ids."""
    rng = np.random.default_rng(n)
    key = rng.permutation(n).astype(np.uint32)
    val = rng.integers(0, 1 << 20, n).astype(np.uint32)
    val[rng.random(n) < 0.15] = NULL
    o = OracleTable(max(n + 3, 16), LOCAL_RANK, C0)
    o.put_rows(*extra_rows(n))
    res = o.put_stamped(key, val, WALL).as_dict()
    for a in (key, val, o.rows):
        a.setflags(write=False)
    return key, val, res, o.rows, o.canonical


@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("row_bytes", [24, 32])
@pytest.mark.parametrize("n", SIZES)
def test_put_stamped_sizes(gpu_device, n, row_bytes, mem):
    key, val, want, rows, canon = put_case(n)
    t = fresh(n, row_bytes)
    got = t.put_stamped(dev(key) if mem == "device" else key, dev(val) if mem == "device" else val, WALL)
    for f in RESULT_FIELDS:
        assert got[f] == want[f], (f, got[f], want[f])
    assert got["n_won"] == n and t.canonical == canon == (C0 if n == 0 else WALL << 16)
    for name, a in zip(COLS, read_all(t)):
        assert np.array_equal(a, rows[name]), name
    if n:                                            # the mark follows the put: the export reads every row written
        o = OracleTable(1, LOCAL_RANK, canon)
        o.rows = rows
        gx.check_export(t, o, t.capacity, 0)
    t.close()


N_BAD = GRID + 1


@pytest.mark.parametrize("offset", [0, 1, 3])
@pytest.mark.parametrize("where", ["first", "last", "middle"])
@pytest.mark.parametrize("row_bytes", [24, 32])
def test_put_stamped_key_at_the_capacity(gpu_device, row_bytes, where, offset):
    """One id >= capacity among 524289, at the ends and at an odd index, in a tensor that starts 0, 4 and 12
    bytes into a 16-B line: k_key_check's head, body and tail each see it.  Nothing of the call is stored."""
    import torch
    key, val, _, _, _ = put_case(N_BAD)
    at = {"first": 0, "last": N_BAD - 1, "middle": N_BAD // 2 + 1 - (N_BAD // 2) % 2}[where]
    assert where != "middle" or (at % 2 == 1 and 256 < at < N_BAD - 256)
    t = fresh(N_BAD, row_bytes)
    before = read_all(t)
    buf = torch.zeros(offset + N_BAD, dtype=torch.int32, device="cuda:0")
    dkey = buf[offset:]
    dkey.copy_(dev(key))
    dkey[at] = t.capacity                            # (= N_BAD + 3, the first id outside the table)
    assert dkey.data_ptr() % 16 == 4 * offset % 16 and dkey.is_contiguous()
    with pytest.raises(CrdtNativeError) as e:
        t.put_stamped(dkey, dev(val), WALL)
    assert e.value.status == _capi.CRDT_E_KEY_RANGE
    assert t.canonical == C0
    for name, a, b in zip(COLS, before, read_all(t)):
        assert np.array_equal(a, b), name
    # and the same keys without the bad one are stored
    dkey[at] = int(key[at])
    assert t.put_stamped(dkey, dev(val), WALL)["n_won"] == N_BAD
    t.close()


@functools.lru_cache(maxsize=None)
def refresh_case(n_rows, top_at_end):
    """Rows [0, n_rows) all invisible (mod < 0) with large lts, but one visible row with a small lt at one end;
    three visible rows with the largest lts of all lie at n_rows and above."""
    big = (WALL + 1000) << 16
    ids = np.arange(n_rows + 3, dtype=np.uint32)
    lt = big + np.arange(n_rows + 3, dtype=np.int64)
    mod = np.full(n_rows + 3, -(1 << 20), np.int64)
    mod[1::7] = I64_MIN // 3                         # (other negative mods too)
    mod[n_rows:] = 5
    want = 0
    if n_rows:
        at = n_rows - 1 if top_at_end else 0
        lt[at], mod[at] = (WALL << 16) + 3, 9
        want = int(lt[at])
    rank = (ids % 7).astype(np.uint32)
    val = ids.copy()
    o = OracleTable(max(n_rows + 3, 16), LOCAL_RANK, 0)
    o.put_rows(ids, lt, rank, val, mod)
    assert o.refresh(n_rows) == want
    return (ids, lt, rank, val, mod), want


@pytest.mark.parametrize("top_at_end", [True, False], ids=["last_row", "row_0"])
@pytest.mark.parametrize("row_bytes", [24, 32])
@pytest.mark.parametrize("n_rows", SIZES)
def test_refresh_canonical_sizes(gpu_device, n_rows, row_bytes, top_at_end):
    cols, want = refresh_case(n_rows, top_at_end)
    t = DeviceTable(0, local_rank=LOCAL_RANK, capacity=n_rows + 3)
    if row_bytes != 24:
        t.set_row_bytes(row_bytes)
    t.put_rows(*cols)
    t.canonical = 12345
    assert t.refresh_canonical(n_rows) == want == t.canonical
    t.close()


@pytest.mark.parametrize("row_bytes", [24, 32])
def test_remap_then_clear_across_the_mark(gpu_device, row_bytes):
    """remap_ranks over more rows than were written, then a clear_rows that starts below the high-water
    mark and ends above it: the export at since 0 (bounded by the mark) and at INT64_MIN (every row) still
    equal the restatement's, and a put above the lowered mark raises it again."""
    n = 3 * 2048 + 17
    cap = 2 * n
    t, o = gx.build_pair(n, cap, row_bytes, seed=4242)
    assert t.capacity == cap
    lut = np.array([0, 2, 3, 4, 5, 6, 7], np.uint32)         # a node id interned between ranks 0 and 1
    t.remap_ranks(cap, lut)
    r = o.rows["rank"]
    m = r < len(lut)
    r[m] = lut[r[m]]
    for since in (0, I64_MIN):
        gx.check_export(t, o, cap, since)
    t.clear_rows(n - 100, 300)
    o.rows[n - 100:n + 200] = new_table(300)
    for since in (0, I64_MIN):
        gx.check_export(t, o, cap, since)
    for name, a in zip(COLS, read_all(t)):
        assert np.array_equal(a, o.rows[name]), name
    ids = np.array([n - 50, n + 150, n + 500], np.uint32)
    vals = np.array([1, NULL, 3], np.uint32)
    o.canonical = t.canonical
    want = o.put_stamped(ids, vals, WALL).as_dict()
    got = t.put_stamped(ids, vals, WALL)
    assert got["canonical_lt"] == want["canonical_lt"] and got["n_won"] == 3
    for since in (0, I64_MIN, want["canonical_lt"]):
        gx.check_export(t, o, cap, since)
    t.close()
