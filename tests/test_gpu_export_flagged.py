"""Flag-predicated export (crdt_export_flagged / DeviceTable.export_flagged) against the numpy model of
tests/_flagged_cases.py over the C restatement's rows, and, after real table merges, against the records the
oracle composition stored.  Everything is integer data: every comparison is exact."""
import ctypes

import numpy as np
import pytest
import torch

import tests.test_gpu_table_merge as gt
from crdt_amd import CrdtNativeError, DeviceTable, _capi
from tests import _fanin_cases as fc
from tests import _fanout_cases as fo
from tests import _flagged_cases as fl
from tests import _sync_cases as sc
from tests import _table_cases as tc
from tests._cases import ABSENT_MOD, NULL
from tests.test_gpu_export import build_pair

pytestmark = pytest.mark.gpu

T = _capi.EXPORT_TILE
MW = tc.MERGE_WALL
COLS = fl.COLS


def dev(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8)).to("cuda:0")


def check_flagged(t: DeviceTable, rows, n_rows: int, flags: np.ndarray, bits: int, tag, dflags=None):
    """One export_flagged against the model: n, n_live, the five columns."""
    m = fl.model(rows, n_rows, flags, bits)
    ex = t.export_flagged(n_rows, dev(flags) if dflags is None else dflags, bits)
    key, lt, rank, val, mod = ex.columns()
    assert (ex.n, ex.n_live) == (m["n"], m["n_live"]), tag
    assert np.array_equal(key, m["key"]), tag
    for name, got in (("lt", lt), ("rank", rank), ("val", val), ("mod", mod)):
        assert np.array_equal(got, m[name]), (tag, name)
    return ex, m


# ------------------------------------------------------------------ 1. shapes, patterns, bits
@pytest.mark.parametrize("row_bytes", [24, 32])
@pytest.mark.parametrize("n_rows", fl.SHAPES)
def test_flagged_parity_shapes(gpu_device, row_bytes, n_rows):
    """Every pattern under every bits value, over mask bytes with other bits set, on a table with holes,
    tombstones, a cleared range and a capacity above the written rows; the table is unchanged by the calls."""
    written = n_rows - n_rows // 4                       # the last quarter lies above the high-water mark
    t, o = build_pair(written, max(n_rows, 16), row_bytes, seed=3000 + n_rows)
    canon = t.canonical
    for name, sel in fl.patterns(n_rows, high_water=written).items():
        for bits in fl.BITS:
            flags = fl.mask_bytes(sel, bits)
            ex, m = check_flagged(t, o.rows, n_rows, flags, bits, (n_rows, name, bits))
            assert m["n"] == (int(sel.sum()) if bits else 0)
    gt.assert_rows(t, o, "rows untouched")
    assert t.canonical == canon
    above_fill = int(ABSENT_MOD) + 1                     # the high-water mark is where it was: no fill row selected
    assert np.array_equal(t.export_since(t.capacity, above_fill).columns()[0], o.modified_since(t.capacity, above_fill))
    t.close()


@pytest.mark.parametrize("row_bytes", [24, 32])
def test_flagged_fill_rows_and_high_water_mark(gpu_device, row_bytes):
    """Flagged rows at or above the high-water mark come out with their fill contents (no clipping), and the
    mark itself is where it was: an export_since above the fill's mod still selects no fill row."""
    w = T + 5
    t, o = build_pair(w, 4 * w, row_bytes, seed=78)
    cap = t.capacity
    sel = np.arange(cap) >= w - 3
    ex, m = check_flagged(t, o.rows, cap, sel.astype(np.uint8), 1, "fill")
    assert m["n"] == cap - (w - 3) and np.all(m["mod"][3:] == ABSENT_MOD)
    assert np.all(m["lt"][3:] == ABSENT_MOD) and np.all(m["val"][3:] == 0x80808080)
    since = int(ABSENT_MOD) + 1
    ids = o.modified_since(cap, since)
    assert len(ids) and ids.max() < w
    assert np.array_equal(t.export_since(cap, since).columns()[0], ids)
    assert t.count_since(cap, since)[0] == len(ids)
    t.close()


@pytest.mark.parametrize("n_rows", fl.LARGE_SHAPES)
def test_flagged_more_tiles_than_one_scan_step_or_grid(gpu_device, n_rows):
    t, o = build_pair(n_rows, n_rows, 24, seed=6)
    pats = fl.patterns(n_rows)
    for name, bits in (("one_percent", 0x05), ("last_row_of_each_tile", 0x80), ("half", 0xFF), ("last_row", 0x01)):
        check_flagged(t, o.rows, n_rows, fl.mask_bytes(pats[name], bits), bits, (n_rows, name))
    t.close()


def test_flags_longer_than_n_rows_and_unaligned(gpu_device):
    """Ones beyond n_rows must not appear; a flags tensor that starts at an odd byte reads the same; a bool
    tensor is taken as bytes; columns(first, count) windows."""
    n = 3 * T + 17
    t, o = build_pair(n, n, 24, seed=8)
    sel = fl.patterns(n)["half"]
    for n_rows in (n, n - 2, 2 * T, T + 1, 5):
        flags = np.concatenate([fl.mask_bytes(sel[:n_rows], 0x05), np.full(n + 9 - n_rows, 0xFF, np.uint8)])
        check_flagged(t, o.rows, n_rows, flags, 0x05, ("longer", n_rows))
        for shift in (1, 3, 7):
            base = dev(np.concatenate([np.full(shift, 0xFF, np.uint8), flags]))
            check_flagged(t, o.rows, n_rows, flags, 0x05, ("unaligned", n_rows, shift), dflags=base[shift:])
    ex, m = check_flagged(t, o.rows, n, sel.astype(np.uint8), 0xFF, "bool", dflags=torch.from_numpy(sel).to("cuda:0"))
    assert ex.n > 10
    for first, count in ((0, 0), (0, 1), (2, ex.n - 3), (ex.n - 1, 1), (ex.n, 0)):
        part = ex.columns(first=first, count=count)
        assert np.array_equal(part[0], m["key"][first:first + count])
        for name, got in zip(COLS, part[1:]):
            assert np.array_equal(got, m[name][first:first + count]), (first, count, name)
    with pytest.raises(CrdtNativeError):
        ex.columns(first=ex.n, count=1)
    t.close()


# ------------------------------------------------------------------ 2. the view, and refused calls
def test_view_replacement(gpu_device):
    n = 2 * T + 9
    t, o = build_pair(n, n, 24, seed=12)
    sel = fl.patterns(n)["one_percent"]
    since_view = t.export_since(n, 0)
    assert since_view.n > 0
    fx, m = check_flagged(t, o.rows, n, sel.astype(np.uint8), 1, "first")
    with pytest.raises(CrdtNativeError) as e:            # an export_since view ends at the call
        since_view.columns()
    assert e.value.status == _capi.CRDT_E_INVALID
    assert np.array_equal(fx.columns()[0], m["key"])
    later = t.export_since(n, 0)                         # a later export_since ends the flagged view
    with pytest.raises(CrdtNativeError) as e:
        fx.columns()
    assert e.value.status == _capi.CRDT_E_INVALID
    assert np.array_equal(later.columns()[0], o.modified_since(n, 0))
    fx2 = t.export_flagged(n, dev(sel), 1)
    t.export_release()
    with pytest.raises(CrdtNativeError):
        fx2.columns()
    assert t._lib.crdt_export_read(t._ctx, 0, 0, None, None, None, None, None) == _capi.CRDT_E_INVALID
    # an empty selection, bits == 0 and n_rows == 0 are valid empty views
    for n_rows, flags, bits in ((n, np.zeros(n, np.uint8), 0xFF), (n, np.ones(n, np.uint8), 0), (0, np.ones(4, np.uint8), 1)):
        ex = t.export_flagged(n_rows, dev(flags), bits)
        assert (ex.n, ex.n_live) == (0, 0) and all(len(c) == 0 for c in ex.columns())
        assert t._lib.crdt_export_read(t._ctx, 0, 1, None, None, None, None, None) == _capi.CRDT_E_INVALID
    t.close()


def test_refused_calls_keep_the_earlier_view(gpu_device):
    n = T + 9
    t, o = build_pair(n, n, 24, seed=13)
    sel = fl.patterns(n)["half"]
    ex, m = check_flagged(t, o.rows, n, sel.astype(np.uint8), 1, "view")
    dflags = dev(np.ones(t.capacity + 8, np.uint8))
    with pytest.raises(CrdtNativeError) as e:            # host-memory flags
        t.export_flagged(n, np.ones(n, np.uint8), 1)
    assert e.value.status == _capi.CRDT_E_INVALID
    with pytest.raises(CrdtNativeError) as e:            # more rows than the table has
        t.export_flagged(t.capacity + 1, dflags, 1)
    assert e.value.status == _capi.CRDT_E_INVALID
    view = _capi.CrdtExport()
    lib, E, D = t._lib, _capi.CRDT_E_INVALID, _capi.CRDT_MEM_DEVICE
    p = ctypes.c_void_p(dflags.data_ptr())
    assert lib.crdt_export_flagged(t._ctx, n, p, D, 1, None) == E
    assert lib.crdt_export_flagged(t._ctx, n, None, D, 1, ctypes.byref(view)) == E
    assert lib.crdt_export_flagged(t._ctx, n, p, _capi.CRDT_MEM_HOST, 1, ctypes.byref(view)) == E
    assert lib.crdt_export_flagged(t._ctx, n, p, 7, 1, ctypes.byref(view)) == E
    key = ex.columns()[0]                                # the earlier view still reads
    assert np.array_equal(key, m["key"])
    gt.assert_rows(t, o, "rows untouched")
    t.close()


# ------------------------------------------------------------------ 3. after real table merges
def stored(osrc_rows, flags: np.ndarray, bit: int) -> dict:
    """The records a merge stored, from the oracle: the source's rows where the oracle's flags have the bit."""
    return fl.model(osrc_rows, len(flags), flags, 1 << bit)


def assert_export(src: DeviceTable, n_rows: int, dflags, bit: int, want: dict, tag):
    ex = src.export_flagged(n_rows, dflags, 1 << bit)
    key, lt, rank, val, _ = ex.columns()
    assert (ex.n, ex.n_live) == (want["n"], want["n_live"]), tag
    assert np.array_equal(key, want["key"]), tag
    for name, got in (("lt", lt), ("rank", rank), ("val", val)):
        assert np.array_equal(got, want[name]), (tag, name)
    return ex


@pytest.mark.parametrize("strides", [(24, 24), (32, 24), (24, 32)])
@pytest.mark.parametrize("n_rows", [65, T + 1, 3 * T + 17])
def test_winners_of_merge_table(gpu_device, n_rows, strides):
    srows, drows = tc.gen_pair(n_rows, 4000 + n_rows)
    src, osrc = gt.load(srows, max(n_rows, 16), strides[0], local_rank=0, canonical=100)
    dst, odst = gt.load(drows, max(n_rows, 16), strides[1], local_rank=tc.DST_RANK, canonical=sc.canon0())
    for step, since in enumerate((sc.mid(), 0)):
        src_before = osrc.rows.copy()
        ores, oflags, _ = tc.oracle_merge_table(odst, osrc, n_rows, since, MW)
        res, flags = dst.merge_table(src, n_rows, since, MW, row_flags=True)
        assert res["status"] == ores["status"] == 0 and res["n_won"] == ores["n_won"]
        want = stored(src_before, oflags, 0)
        assert want["n"] == ores["n_won"] and (step or want["n"] > 0)
        assert_export(src, n_rows, flags, 0, want, (n_rows, since))
        # what dst holds at those ids is the exported {lt, rank, val}, under dst's own stamp
        lt, rank, val, mod = dst.read_rows(want["key"])
        assert np.array_equal(lt, want["lt"]) and np.array_equal(rank, want["rank"]) and np.array_equal(val, want["val"])
        assert np.array_equal(mod, odst.rows["mod"][want["key"]])
    gt.assert_rows(src, osrc, "source untouched")
    src.close()
    dst.close()


def test_winners_of_sync_tables(gpu_device):
    n_rows = 3 * T + 17
    arows, brows = sc.pair(n_rows, 4100)
    a, oa = gt.load(arows, n_rows, 24, local_rank=sc.A_RANK, canonical=sc.canon0())
    b, ob = gt.load(brows, n_rows, 32, local_rank=sc.B_RANK, canonical=sc.C_B)
    b_before = ob.rows.copy()
    (ra, fa), (rb, fb) = tc.oracle_sync(oa, ob, n_rows, 0, 0, MW)
    (ga, da), (gb, db) = a.sync_tables(b, n_rows, 0, 0, MW, row_flags=True)
    assert ga["status"] == ra["status"] == 0 and gb["status"] == rb["status"] == 0
    assert np.array_equal(da.cpu().numpy(), fa) and np.array_equal(db.cpu().numpy(), fb)
    assert fa.any() and fb.any()
    # a stored b's rows as they were; b stored a's rows as they were after a's merge (= oa.rows now)
    assert_export(b, n_rows, da, 0, stored(b_before, fa, 0), "a's winners, read from b")
    assert_export(a, n_rows, db, 0, stored(oa.rows, fb, 0), "b's winners, read from a")
    # b's copy of what a took is unchanged by the second merge (a tie keeps local)
    took = np.flatnonzero(fa)
    for name in ("lt", "rank", "val"):
        assert np.array_equal(ob.rows[name][took], b_before[name][took]), name
    a.close()
    b.close()


@pytest.mark.parametrize("n_src", [3, 8])
def test_winners_of_merge_tables(gpu_device, n_src):
    """Bit j against srcs[j] is merge j's stored records, even where a later merge overwrote the row in dst."""
    n_rows = 2 * T + 17
    cap = max(n_rows, 16)
    drows = fc.dst_rows(n_rows)
    srows = [fc.source_rows(n_rows, j) for j in range(n_src)]
    # two sources win row 5 in turn: source 1's record beats dst's, source 2's beats source 1's
    tc._plant(drows, {5: (int(tc.STAMPS[2]), 0, 600, int(tc.STAMPS[2]))})
    for j in (1, 2):
        tc._plant(srows[j], {5: (int(tc.STAMPS[10 * j]), j, 700 + j, tc.TOP)})
    for j in range(n_src):
        if j not in (1, 2):                              # (no other source holds a newer row 5)
            tc._plant(srows[j], {5: (int(tc.STAMPS[1]), 0, 800 + j, tc.TOP)})
    dst, odst = gt.load(drows, cap, 24, local_rank=tc.DST_RANK, canonical=sc.canon0())
    loaded = [gt.load(r, cap, 24 if j % 2 else 32, local_rank=j % 6, canonical=100) for j, r in enumerate(srows)]
    srcs, osrcs = [t for t, _ in loaded], [o for _, o in loaded]
    sinces = [0] * n_src
    ores, omask, stop = tc.oracle_fanin(odst, osrcs, n_rows, sinces, MW)
    res, mask = dst.merge_tables(srcs, n_rows, sinces, MW, win_mask=True)
    assert stop is None and [r["status"] for r in res] == [0] * n_src
    assert np.array_equal(mask.cpu().numpy(), omask)
    assert (omask[5] >> 1) & 1 and (omask[5] >> 2) & 1                       # both won row 5, in turn
    overwritten = 0
    for j in range(n_src):
        want = stored(osrcs[j].rows, omask, j)
        assert want["n"] == ores[j]["n_won"]
        assert_export(srcs[j], n_rows, mask, j, want, ("fanin", j))
        overwritten += int(np.count_nonzero(odst.rows["lt"][want["key"]] != want["lt"]))
    assert overwritten > 0                                                   # dst alone could not have told
    for t in srcs + [dst]:
        t.close()


@pytest.mark.parametrize("n_dst", [3, 8])
def test_winners_of_fanout_tables(gpu_device, n_dst):
    n_rows = 2 * T + 17
    cap = max(n_rows, 16)
    src, osrc = gt.load(fo.source_rows(n_rows), cap, 32, local_rank=fo.SRC_RANK, canonical=100)
    loaded = [gt.load(fo.dst_rows(n_rows, j), cap, 24 if j % 2 else 32, local_rank=fo.dst_rank(j),
                      canonical=fo.canonical("mid", j)) for j in range(n_dst)]
    dsts, odsts = [t for t, _ in loaded], [o for _, o in loaded]
    sinces = fo.since_vectors(n_dst)["mixed"]
    ores, omask, stop = fo.oracle_fanout(osrc, odsts, n_rows, sinces, MW)
    res, mask = src.fanout_tables(dsts, n_rows, sinces, MW, win_mask=True)
    assert stop is None and np.array_equal(mask.cpu().numpy(), omask)
    for j in range(n_dst):
        want = stored(osrc.rows, omask, j)
        assert want["n"] == ores[j]["n_won"] == res[j]["n_won"]
        assert_export(src, n_rows, mask, j, want, ("fanout", j))
    union = fl.model(osrc.rows, n_rows, omask, 0xFF)                          # every destination's at once
    ex = src.export_flagged(n_rows, mask)
    assert ex.n == union["n"] and np.array_equal(ex.columns()[0], union["key"])
    assert union["n_live"] == int(np.count_nonzero(union["val"] != NULL)) == ex.n_live
    for t in dsts + [src]:
        t.close()
