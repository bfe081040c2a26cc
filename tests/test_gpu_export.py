"""Device-resident changeset export (crdt_export_since / crdt_count_since) and the
replica-to-replica merge built on it (DeviceTable.merge_from), against the C restatement.
Everything is integer data: every comparison is exact."""
import ctypes

import numpy as np
import pytest

from crdt_amd import CrdtJson, CrdtNativeError, DeviceTable, Hlc, MapCrdt, Record, _capi
from crdt_amd.crdt import Crdt
from oracle.oracle_c import OracleTable, new_table
from tests._cases import ABSENT_MOD, NULL, WALL, make_case
from tests._table_cases import oracle_merge_from as _oracle_merge_from   # (the contract on the oracle)

pytestmark = pytest.mark.gpu

T = _capi.EXPORT_TILE                  # rows per workgroup of the export's two passes
SCAN_STEP = _capi.EXPORT_SCAN_STEP     # tile counts the scan takes per iteration of its loop
COUNT_GRID = _capi.EXPORT_COUNT_GRID   # workgroups of the count pass: more tiles than this and each strides
I64_MIN = -(1 << 63)
N_STAMPS = 40
STAMPS = ((WALL + 7 * np.arange(N_STAMPS, dtype=np.int64)) << 16) + np.arange(N_STAMPS, dtype=np.int64) % 5
RESULT_FIELDS = ("status", "n_stored", "exc_changeset", "exc_index", "canonical_lt", "drift_ms", "counter",
                 "n_present", "n_won")


def sinces():
    s = np.sort(STAMPS)
    return [0, int(s[0]), int(s[len(s) // 2]), int(s[-1]), int(s[-1]) + 1, -1, I64_MIN]


def oracle_clear(o: OracleTable, first: int, count: int):
    o.rows[first:first + count] = new_table(count)


def build_pair(n_rows: int, capacity: int, row_bytes: int, seed: int):
    """The same rows in a DeviceTable and an OracleTable: mods over N_STAMPS stamps, ~20 % tombstones,
    ~10 % never-written holes, ~5 % negative mods, and a cleared range in the second third."""
    rng = np.random.default_rng(seed)
    t = DeviceTable(0, local_rank=0, capacity=capacity)
    if row_bytes != 24:
        t.set_row_bytes(row_bytes)
    o = OracleTable(t.capacity, 0)
    ids = np.flatnonzero(rng.random(n_rows) >= 0.10).astype(np.uint32)
    n = len(ids)
    mod = STAMPS[rng.integers(0, N_STAMPS, n)]
    neg = rng.random(n) < 0.05
    mod[neg] = -(1 << 20) - rng.integers(0, 1000, int(neg.sum()))
    lt = mod - rng.integers(0, 1 << 18, n)
    rank = rng.integers(0, 6, n).astype(np.uint32)
    val = rng.integers(0, 1 << 20, n).astype(np.uint32)
    val[rng.random(n) < 0.20] = NULL
    if n:
        t.put_rows(ids, lt, rank, val, mod)
        o.put_rows(ids, lt, rank, val, mod)
    first, count = n_rows // 3, n_rows // 10
    if count:
        t.clear_rows(first, count)
        oracle_clear(o, first, count)
    return t, o


def check_export(t: DeviceTable, o: OracleTable, n_rows: int, since: int):
    ids = o.modified_since(n_rows, since)
    rows = o.rows[ids]
    n_live = int(np.count_nonzero(rows["val"] != NULL))
    ex = t.export_since(n_rows, since)
    key, lt, rank, val, mod = ex.columns()
    what = (n_rows, since)
    assert ex.n == len(ids), what
    assert np.array_equal(key, ids), what
    for name, got in (("lt", lt), ("rank", rank), ("val", val), ("mod", mod)):
        assert np.array_equal(got, rows[name]), (name,) + what
    assert ex.n_live == n_live, what
    assert t.count_since(n_rows, since) == (len(ids), n_live), what
    assert np.array_equal(t.modified_since(n_rows, since), ids), what      # the id-only SPI call still agrees
    return ex


# ------------------------------------------------------------------ 1. parity against the oracle
@pytest.mark.parametrize("row_bytes", [24, 32])
@pytest.mark.parametrize("n_rows", [0, 1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 17])
def test_export_parity_shapes(gpu_device, row_bytes, n_rows):
    t, o = build_pair(n_rows, max(n_rows, 16), row_bytes, seed=1000 + n_rows)
    for since in sinces():
        check_export(t, o, n_rows, since)
    if n_rows > 2:                       # a prefix of the table: n_rows is the caller's, not the capacity
        check_export(t, o, n_rows - 2, int(np.sort(STAMPS)[N_STAMPS // 2]))
    t.close()


@pytest.mark.parametrize("row_bytes", [24, 32])
def test_export_high_water(gpu_device, row_bytes):
    """Capacity 8x the written rows: the rows above the high-water mark are fill, selected by
    since = INT64_MIN (mod 0x8080808080808080 is not below it) and by no since above the fill's mod."""
    w = T + 5
    t, o = build_pair(w, 8 * w, row_bytes, seed=77)
    cap = t.capacity
    assert cap == 8 * w
    ex = check_export(t, o, cap, I64_MIN)
    assert ex.n == cap
    check_export(t, o, cap, 0)
    check_export(t, o, cap, int(ABSENT_MOD))            # the fill's own mod: still every row
    check_export(t, o, cap, int(ABSENT_MOD) + 1)        # one above: no fill row
    # a clear that reaches the mark lowers it; a put above it raises it again
    t.clear_rows(w - 7, 10)
    oracle_clear(o, w - 7, 10)
    for since in (I64_MIN, 0):
        check_export(t, o, cap, since)
    k = np.array([5 * w + 3], np.uint32)
    one = (k, np.array([int(STAMPS[3])]), np.array([2], np.uint32), np.array([9], np.uint32), np.array([int(STAMPS[9])]))
    t.put_rows(*one)
    o.put_rows(*one)
    for since in (I64_MIN, 0, int(STAMPS[9]), int(STAMPS[9]) + 1):
        check_export(t, o, cap, since)
    t.close()


@pytest.mark.parametrize("row_bytes", [24, 32])
def test_export_more_tiles_than_one_scan_step(gpu_device, row_bytes):
    # the scan's loop runs three times, with a carry, and the count pass's workgroups stride over the tiles
    n_rows = (max(SCAN_STEP, COUNT_GRID) + 3) * T + 17
    t, o = build_pair(n_rows, n_rows, row_bytes, seed=5)
    for since in (int(np.sort(STAMPS)[N_STAMPS // 2]), int(np.sort(STAMPS)[-1]), I64_MIN):
        check_export(t, o, n_rows, since)
    t.close()


def _pattern(name: str, n_rows: int) -> np.ndarray:
    sel = np.zeros(n_rows, bool)
    if name == "all":
        sel[:] = True
    elif name == "alternating":
        sel[::2] = True
    elif name == "tile_ends":                            # exactly the first and the last row of a tile
        sel[2 * T] = sel[3 * T - 1] = True
    elif name == "run_across_boundary":                  # a dense run over a tile boundary, empty tiles around it
        sel[2 * T - 300:2 * T + 500] = True
    else:
        assert name == "none"
    return sel


@pytest.mark.parametrize("row_bytes", [24, 32])
@pytest.mark.parametrize("pattern", ["all", "none", "alternating", "tile_ends", "run_across_boundary"])
def test_export_selection_patterns(gpu_device, row_bytes, pattern):
    n_rows = 5 * T + 9
    sel = _pattern(pattern, n_rows)
    lo, hi = int(STAMPS[2]), int(STAMPS[30])
    rng = np.random.default_rng(11)
    ids = np.arange(n_rows, dtype=np.uint32)
    mod = np.where(sel, hi, lo).astype(np.int64)
    lt = mod - rng.integers(0, 1000, n_rows)
    rank = rng.integers(0, 6, n_rows).astype(np.uint32)
    val = rng.integers(0, 1 << 20, n_rows).astype(np.uint32)
    val[rng.random(n_rows) < 0.2] = NULL
    t = DeviceTable(0, capacity=n_rows)
    if row_bytes != 24:
        t.set_row_bytes(row_bytes)
    o = OracleTable(t.capacity, 0)
    t.put_rows(ids, lt, rank, val, mod)
    o.put_rows(ids, lt, rank, val, mod)
    ex = check_export(t, o, n_rows, hi)
    assert ex.n == int(sel.sum())
    key = ex.columns()[0]
    assert np.array_equal(key, np.flatnonzero(sel))
    if ex.n > 3:                                         # a window of the view
        part = ex.columns(first=2, count=ex.n - 3)
        assert np.array_equal(part[0], key[2:ex.n - 1])
    t.close()


def test_export_argument_checks(gpu_device):
    t = DeviceTable(0, capacity=64)
    lib, E = t._lib, _capi.CRDT_E_INVALID
    view = _capi.CrdtExport()
    n, live = ctypes.c_uint64(), ctypes.c_uint64()
    assert lib.crdt_export_since(t._ctx, 16, 0, None) == E
    assert lib.crdt_export_since(t._ctx, t.capacity + 1, 0, ctypes.byref(view)) == E
    assert lib.crdt_count_since(t._ctx, 16, 0, None, ctypes.byref(live)) == E
    assert lib.crdt_count_since(t._ctx, 16, 0, ctypes.byref(n), None) == E
    assert lib.crdt_count_since(t._ctx, t.capacity + 1, 0, ctypes.byref(n), ctypes.byref(live)) == E
    assert lib.crdt_export_read(t._ctx, 0, 0, None, None, None, None, None) == E      # no view yet
    ex = t.export_since(t.capacity, 0)                   # nothing written: an empty view
    assert (ex.n, ex.n_live) == (0, 0) and all(len(c) == 0 for c in ex.columns())
    assert lib.crdt_export_read(t._ctx, 0, 1, None, None, None, None, None) == E      # past its end
    t.close()


# ------------------------------------------------------------------ 2. replica-to-replica merge
CAP = (1 << 16) + 3
N_LOCAL = 40000


def _replica(case, path):
    """A DeviceTable and its OracleTable mirror: the case's local rows, then its changesets merged."""
    t = DeviceTable(0, local_rank=case["local_rank"], capacity=CAP)
    o = OracleTable(CAP, case["local_rank"], case["c0"])
    loc = case["local"]
    keep = loc["mod"] != ABSENT_MOD
    ids = np.arange(case["n_local"], dtype=np.uint32)[keep]
    cols = (ids, loc["lt"][keep], loc["rank"][keep], loc["val"][keep], loc["mod"][keep])
    t.put_rows(*cols)
    o.put_rows(*cols)
    t.canonical = case["c0"]
    t.set_merge_path(path)
    return t, o


def _diverge(t, o, case):
    batch = (case["key"], case["lt"], case["rank"], case["val"], case["offsets"], case["wall"])
    res, _ = t.merge(*batch)
    ores, _ = o.merge(*batch)
    assert res["status"] == ores.status == 0
    assert res["canonical_lt"] == o.canonical


def _check_rows(t: DeviceTable, o: OracleTable, tag):
    got = t.read_rows(np.arange(CAP, dtype=np.uint32))
    for name, a in zip(("lt", "rank", "val", "mod"), got):
        assert np.array_equal(a, o.rows[name]), (tag, name)
    assert t.canonical == o.canonical, tag
    return got


def _check_merge_from(dst, odst, src, osrc, since, wall, tag):
    res, flags = dst.merge_from(src, CAP, since, wall)
    ores, oflags, n = _oracle_merge_from(odst, osrc, CAP, since, wall)
    for f in RESULT_FIELDS:
        assert res[f] == ores[f], (tag, f, res[f], ores[f])
    assert str(flags.device) == "cuda:0" and len(flags) == n
    assert np.array_equal(flags.cpu().numpy(), oflags), tag
    _check_rows(dst, odst, tag)
    return res, n


def _pair(path):
    """A (rank 0) and B (rank 1) start from the SAME local rows and canonical, then merge different
    random changesets: every row on which they differ carries a mod above the shared starting
    canonical, so a delta taken since that stamp holds all of a replica's divergence."""
    a_case = make_case(seed=101, n_local=N_LOCAL, n_new=CAP - N_LOCAL, R=3, per_cs=6000, local_rank=0,
                       n_ranks=6, tomb_frac=0.2, absent_frac=0.1, neg_mod_frac=0.05)
    b_case = make_case(seed=202, n_local=N_LOCAL, n_new=CAP - N_LOCAL, R=4, per_cs=5000, local_rank=1,
                       n_ranks=6, tomb_frac=0.2)
    b_case["local"], b_case["c0"] = a_case["local"], a_case["c0"]
    # an Hlc names one write: the two replicas' changesets come from disjoint nodes, so no record of
    # one ties on (lt, rank) with a different value of the other (which no merge order could settle)
    a_case["rank"] = (2 + a_case["rank"] % 2).astype(np.uint32)
    b_case["rank"] = (4 + b_case["rank"] % 2).astype(np.uint32)
    A, oA = _replica(a_case, path)
    B, oB = _replica(b_case, path)
    stamp = B.canonical                                    # taken before B's merges (= A's: the shared start)
    _diverge(A, oA, a_case)
    _diverge(B, oB, b_case)
    return A, oA, B, oB, stamp


@pytest.mark.parametrize("path", ["gather", "sorted"])
def test_merge_from_converges(gpu_device, path):
    A, oA, B, oB, stamp = _pair(path)
    # B.merge(A.recordMap()): every visible row of A as one device changeset
    res, n = _check_merge_from(B, oB, A, oA, 0, WALL + 1, "A->B")
    assert res["status"] == 0 and n > N_LOCAL // 2 and 0 < res["n_won"] < n
    assert B.last_path() == path
    # A.merge(B.recordMap(modifiedSince: stamp)): the reference's changeset pattern
    res, n2 = _check_merge_from(A, oA, B, oB, stamp, WALL + 2, "B->A")
    assert res["status"] == 0 and 0 < n2 < n and res["n_won"] > 0
    assert A.last_path() == path
    ra = A.read_rows(np.arange(CAP, dtype=np.uint32))
    rb = B.read_rows(np.arange(CAP, dtype=np.uint32))
    for name, x, y in zip(("lt", "rank", "val"), ra, rb):
        assert np.array_equal(x, y), ("convergence", name)
    A.close()
    B.close()


def test_merge_from_duplicate_node(gpu_device):
    """A holds a record stamped with B's node id above B's canonical: B's merge raises
    DuplicateNodeException at that record (hlc.dart:88-90) and stores nothing of the changeset."""
    A, oA, B, oB, _ = _pair("gather")
    k = np.array([N_LOCAL // 2], np.uint32)
    bad = (k, np.array([(WALL + 5000) << 16]), np.array([1], np.uint32), np.array([77], np.uint32),
           np.array([int(A.canonical)]))
    A.put_rows(*bad)
    oA.put_rows(*bad)
    before = _check_rows(B, oB, "before")
    res, n = _check_merge_from(B, oB, A, oA, 0, WALL + 1, "dup")
    assert res["status"] == _capi.CRDT_DUPLICATE_NODE and res["n_stored"] == 0 and res["n_won"] == 0
    pos = int(np.searchsorted(oA.modified_since(CAP, 0), k[0]))
    assert (res["exc_changeset"], res["exc_index"]) == (0, pos)
    after = B.read_rows(np.arange(CAP, dtype=np.uint32))
    for x, y in zip(before, after):
        assert np.array_equal(x, y)
    A.close()
    B.close()


def test_merge_from_empty_selection(gpu_device):
    """An empty changeset is still one merge() call: the closing Hlc.send advances the canonical
    (crdt.dart:93) and no row changes."""
    A, oA, B, oB, _ = _pair("gather")
    c0 = B.canonical
    res, n = _check_merge_from(B, oB, A, oA, int(A.canonical) + 1, WALL + 9, "empty")
    assert n == 0 and res["status"] == 0 and res["n_stored"] == 1 and res["n_won"] == 0
    assert B.canonical == (WALL + 9) << 16 and B.canonical > c0
    A.close()
    B.close()


def test_merge_from_other_device_is_refused(gpu_device):
    a, b = DeviceTable(0, capacity=16), DeviceTable(0, capacity=16)
    b.device = 1                                          # (as if it had been created on another GPU)
    with pytest.raises(ValueError):
        a.merge_from(b, 16, 0, WALL)
    b.device = 0
    a.close()
    b.close()


# ------------------------------------------------------------------ 3. view lifetime
def test_view_lifetime(gpu_device):
    A, oA, B, oB, stamp = _pair("gather")
    exA = A.export_since(CAP, 0)
    first = exA.columns()
    assert exA.n == len(first[0]) > 0
    # other ctxs, and merges / puts on the same ctx, leave the view alone
    B.merge(first[0][:100], first[1][:100], first[2][:100], first[3][:100], [0, 100], WALL + 1)
    exB = B.export_since(CAP, stamp)
    A.put_stamped(np.arange(500, dtype=np.uint32), np.arange(500, dtype=np.uint32), WALL + 3)
    extra = make_case(seed=9, n_local=N_LOCAL, n_new=CAP - N_LOCAL, R=2, per_cs=3000, local_rank=0, n_ranks=6)
    A.merge(extra["key"], extra["lt"], extra["rank"], extra["val"], extra["offsets"], WALL + 4)
    again = exA.columns()
    for x, y in zip(first, again):
        assert np.array_equal(x, y)
    assert exB.n == len(exB.columns()[0])
    # a second export on A replaces the view: the old handle is refused, the new one differs
    ex2 = A.export_since(CAP, 0)
    with pytest.raises(CrdtNativeError) as e:
        exA.columns()
    assert e.value.status == _capi.CRDT_E_INVALID
    assert not np.array_equal(ex2.columns()[4], first[4])  # (mods of the rows put since)
    A.export_release()
    with pytest.raises(CrdtNativeError) as e:
        ex2.columns()
    assert e.value.status == _capi.CRDT_E_INVALID
    assert A._lib.crdt_export_read(A._ctx, 0, 0, None, None, None, None, None) == _capi.CRDT_E_INVALID
    assert exB.n == len(exB.columns()[0])                 # B's view is B's
    A.export_since(CAP, 0).columns()                      # and A exports again after a release
    A.close()
    B.close()


# ------------------------------------------------------------------ 4. MapCrdt views
def _check_views(c: MapCrdt, hs):
    m = c.map
    assert c.length == len(m)
    assert c.isEmpty == (len(m) == 0)
    full = c.recordMap()
    for h in hs:
        since = 0 if h is None else h.logicalTime
        want = {k: r for k, r in full.items() if r.modified.logicalTime >= since}      # map_crdt.dart:42-45
        got = c.recordMap(modifiedSince=h)
        assert got == want and list(got) == list(want), h
    assert c.toJson() == Crdt.toJson(c)
    for h in hs:
        assert c.toJson(modifiedSince=h) == Crdt.toJson(c, modifiedSince=h)


def test_mapcrdt_views(gpu_device):
    h0 = Hlc(WALL - 50, 0, "abc")
    c = MapCrdt("abc", {f"s{i}": Record(Hlc(WALL - 50 + i, 0, "abc"), i, Hlc(WALL - 50 + i, 0, "abc"))
                        for i in range(20)}, clock=lambda: WALL)
    hs = [None, Hlc(0, 0, "abc"), h0, Hlc(WALL - 40, 0, "abc"), Hlc(WALL, 0, "abc"), Hlc(WALL + 1, 1, "abc"),
          Hlc(WALL + 50, 0, "abc")]
    _check_views(c, hs)
    c.putAll({f"p{i}": {"v": i} for i in range(30)}, wall=WALL)
    c.put("s3", "again", wall=WALL + 1)
    _check_views(c, hs)
    for k in ("s1", "p2", "p29"):
        c.delete(k, wall=WALL + 2)
    _check_views(c, hs)
    assert c.length == 47
    remote = CrdtJson.encode({f"p{i}": Record(Hlc(WALL + 3, i, "xyz"), None if i % 3 == 0 else i * 10, None)
                              for i in range(25, 40)})
    c.mergeJson(remote, wall=WALL + 4)
    _check_views(c, hs + [c.canonicalTime])
    c.purge()
    _check_views(c, hs)
    assert c.isEmpty and c.length == 0
    c.putAll({"x": 1, "y": None}, wall=WALL + 5)
    _check_views(c, hs)
    assert c.length == 1
