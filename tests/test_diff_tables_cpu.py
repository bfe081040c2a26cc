"""crdt_diff_tables / crdt_digest_rows without a GPU: the numpy model of tests/_diff_cases.py against the
existing merge on the C restatement (diff bit 0 is the merge's row flags, n_a_ahead its n_won; a sync leaves
nothing ahead and every conflict in place), the digests against bench.row_digests and against the diff, and
the C surface: the header, the binding, the struct layout, the refused calls."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import bench
from crdt_amd import DeviceTable, _capi
from oracle.oracle_c import OracleTable, new_table
from tests import _diff_cases as dc
from tests import _table_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = dc.T
SHAPES = (1, 63, 64, T - 1, T, T + 1, 5 * T + 9)
SEEDS = (11, 12, 13)
MW = tc.MERGE_WALL


def oracle_of(rows: dict, capacity: int, local_rank: int, canonical: int) -> OracleTable:
    o = OracleTable(capacity, local_rank, canonical)
    if len(rows["ids"]):
        o.put_rows(*(rows[k] for k in ("ids", "lt", "rank", "val", "mod")))
    first, count = rows["clear"]
    if count:
        o.rows[first:first + count] = new_table(count)
    return o


def pair(n_rows: int, seed: int):
    ra, rb = dc.gen_diff_pair(n_rows, seed)
    c0 = dc.max_lt(ra, rb)
    return ra, rb, oracle_of(ra, max(n_rows, 16), 6, c0), oracle_of(rb, max(n_rows, 16), tc.DST_RANK, c0)


def clone(o: OracleTable) -> OracleTable:
    c = OracleTable(len(o.rows), o.local_rank, o.canonical)
    c.rows[:] = o.rows
    return c


# ------------------------------------------------------------------ 1. the diff against the merge
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("n_rows", SHAPES)
def test_bit0_is_the_merge_and_a_sync_converges(n_rows, seed):
    ra, rb, oa, ob = pair(n_rows, seed)
    flags, d = dc.model_diff(oa.rows, ob.rows, n_rows)
    assert np.array_equal(flags, dc.model_diff(tc.dense(ra, n_rows), tc.dense(rb, n_rows), n_rows)[0])
    # b.merge(a.recordMap()) stores exactly the A_AHEAD rows, a.merge(b.recordMap()) the B_AHEAD ones
    res, rf, _ = tc.oracle_merge_table(clone(ob), oa, n_rows, 0, MW)
    assert res["status"] == 0 and res["n_won"] == d["n_a_ahead"]
    assert np.array_equal(rf, flags & 1)
    res, rf, _ = tc.oracle_merge_table(clone(oa), ob, n_rows, 0, MW)
    assert res["status"] == 0 and res["n_won"] == d["n_b_ahead"]
    assert np.array_equal(rf, (flags >> 1) & 1)
    assert d["n_visible_a"] == len(oa.modified_since(n_rows, 0)) and d["n_visible_b"] == len(ob.modified_since(n_rows, 0))
    # swapping the sides swaps the two bits and keeps the conflicts
    sw, ds = dc.model_diff(ob.rows, oa.rows, n_rows)
    assert np.array_equal(sw, ((flags & 1) << 1) | ((flags >> 1) & 1) | (flags & 4))
    assert (ds["n_a_ahead"], ds["n_b_ahead"], ds["n_conflict"]) == (d["n_b_ahead"], d["n_a_ahead"], d["n_conflict"])
    # after the two-way sync nothing is ahead, and every conflict is where it was
    before = dc.model_digest(ob.rows, n_rows, T, True)
    (r1, _), (r2, _) = tc.oracle_sync(oa, ob, n_rows, 0, 0, MW)
    assert r1["status"] == 0 and r2["status"] == 0
    after, da = dc.model_diff(oa.rows, ob.rows, n_rows)
    assert (da["n_a_ahead"], da["n_b_ahead"], da["n_conflict"]) == (0, 0, d["n_conflict"])
    assert np.array_equal(after, flags & 4)
    assert da["n_visible_a"] == da["n_visible_b"]
    # ... so the STATE digests agree exactly outside the blocks that hold a conflict
    sa, sb = dc.model_digest(oa.rows, n_rows, T, True), dc.model_digest(ob.rows, n_rows, T, True)
    blocks = np.zeros(len(sa), bool)
    blocks[np.flatnonzero(after) // T] = True
    assert np.array_equal(sa != sb, blocks)
    assert d["n_a_ahead"] == 0 or not np.array_equal(before, sb)          # b took a's rows: its state moved


def test_no_conflict_means_equal_state_digests_after_a_sync():
    """The same pairs with the conflict rows made equal: the synced tables' STATE digests are equal, though
    their capacities, stamps and never-written rows differ."""
    for n_rows in (64, T + 1, 5 * T + 9):
        ra, rb, oa, _ = pair(n_rows, 21)
        ob = oracle_of(rb, 2 * n_rows + 7, tc.DST_RANK, oa.canonical)
        conf = np.flatnonzero(dc.model_diff(oa.rows, ob.rows, n_rows)[0] & 4)
        ob.rows["val"][conf] = oa.rows["val"][conf]
        tc.oracle_merge_table(oa, ob, n_rows, 0, MW)
        tc.oracle_merge_table(ob, oa, n_rows, 0, MW)
        flags, d = dc.model_diff(oa.rows, ob.rows, n_rows)
        assert not flags.any() and d["first_diff"] == dc.NONE
        assert not np.array_equal(oa.rows["mod"][:n_rows], ob.rows["mod"][:n_rows])
        for block in (T, 1 << 20):
            assert np.array_equal(dc.model_digest(oa.rows, n_rows, block, True), dc.model_digest(ob.rows, n_rows, block, True))
        assert not np.array_equal(dc.model_digest(oa.rows, n_rows, T, False), dc.model_digest(ob.rows, n_rows, T, False))


def test_first_diff_and_the_classes():
    ra, rb = dc.gen_diff_pair(5 * T + 9, 11)
    assert set(ra["classes"]) == set(dc.CLASSES) | {"planted"}
    assert ra["classes"]["planted"].tolist() == list(range(8)) + [5 * T + 8]
    flags, d = dc.model_diff(tc.dense(ra, 5 * T + 9), tc.dense(rb, 5 * T + 9), 5 * T + 9)
    assert d["first_diff"] == 0 and flags[5 * T + 8] == dc.A_AHEAD and set(np.unique(flags)) == {0, 1, 2, 4}
    same = tc.dense(ra, 5 * T + 9)
    assert dc.model_diff(same, same, 5 * T + 9)[1] == dict(zip(dc.FIELDS, (0, 0, 0, d["n_visible_a"], d["n_visible_a"], dc.NONE)))
    assert dc.model_diff(same, same, 0)[1]["first_diff"] == dc.NONE


# ------------------------------------------------------------------ 2. the digests
@pytest.mark.parametrize("n_rows", [0, 1, T + 1, (1 << 20) + 5, 3 << 20])
def test_rows_digest_is_bench_row_digests(n_rows):
    rows = tc.dense(tc.gen_rows(n_rows, 31), n_rows + 3)
    want = bench.row_digests(rows["lt"][:n_rows], rows["rank"][:n_rows], rows["val"][:n_rows], rows["mod"][:n_rows], 0)
    got = dc.model_digest(rows, n_rows, bench.DIGEST_BLOCK, False)
    assert got.dtype == np.uint64 and np.array_equal(got, want)
    assert [int(x) for x in dc.P] == [int(x) for x in bench._DIG_P]
    if n_rows > T:                                       # finer blocks add up to the coarser ones
        fine = dc.model_digest(rows, n_rows, T, False)
        with np.errstate(over="ignore"):
            assert np.array_equal(np.add.reduceat(fine, np.arange(0, len(fine), bench.DIGEST_BLOCK // T)), got)


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("n_rows", SHAPES)
def test_state_digests_differ_in_exactly_the_differing_blocks(n_rows, seed):
    """No collision on the fixed seeds: a block's STATE word differs iff the block holds a non-zero diff byte."""
    ra, rb = dc.gen_diff_pair(n_rows, seed)
    a, b = tc.dense(ra, n_rows), tc.dense(rb, n_rows + 9)
    flags = dc.model_diff(a, b, n_rows)[0]
    sa, sb = dc.model_digest(a, n_rows, T, True), dc.model_digest(b, n_rows, T, True)
    assert len(sa) == -(-n_rows // T)
    blocks = np.zeros(len(sa), bool)
    blocks[np.flatnonzero(flags) // T] = True
    assert np.array_equal(sa != sb, blocks)


# ------------------------------------------------------------------ 3. header and library
def _header() -> str:
    return open(os.path.join(ROOT, "include", "crdt_merge.h")).read()


def _params(name: str) -> list:
    decl = re.search(rf"^int {name}\(([^;]*)\);", _header(), flags=re.M | re.S)
    assert decl, f"the header does not declare {name}"
    return [" ".join(p.split()) for p in re.sub(r"/\*.*?\*/", "", decl.group(1), flags=re.S).split(",")]


def test_header_binding_and_library_agree():
    lib = _capi.load()
    out = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True).stdout
    assert {"crdt_diff_tables", "crdt_digest_rows"} <= set(re.findall(r" T (crdt_\w+)", out))
    P, U64, I32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int32
    assert _capi.SIGNATURES["crdt_diff_tables"] == (ctypes.c_int, [P, P, U64, P, I32, P])
    assert _capi.SIGNATURES["crdt_digest_rows"] == (ctypes.c_int, [P, U64, U64, I32, P, I32])
    for name in ("crdt_diff_tables", "crdt_digest_rows"):
        assert getattr(lib, name).argtypes == _capi.SIGNATURES[name][1]
    assert _params("crdt_diff_tables") == ["crdt_ctx* a", "crdt_ctx* b", "uint64_t n_rows", "uint8_t* diff_flags",
                                           "int32_t flags_mem", "crdt_diff* out"]
    assert _params("crdt_digest_rows") == ["crdt_ctx* ctx", "uint64_t n_rows", "uint64_t block_rows", "int32_t kind",
                                           "uint64_t* out_words", "int32_t mem"]
    txt = _header()
    assert re.search(r"#define\s+CRDT_ABI_VERSION\s+5\b", txt) and lib.crdt_abi_version() == _capi.ABI_VERSION == 5
    assert re.search(r"enum crdt_diff_bits \{ CRDT_DIFF_A_AHEAD = 1, CRDT_DIFF_B_AHEAD = 2, CRDT_DIFF_CONFLICT = 4 \}", txt)
    assert re.search(r"enum crdt_digest_kind \{ CRDT_DIGEST_ROWS = 0, CRDT_DIGEST_STATE = 1 \}", txt)
    assert (_capi.DIFF_A_AHEAD, _capi.DIFF_B_AHEAD, _capi.DIFF_CONFLICT) == (dc.A_AHEAD, dc.B_AHEAD, dc.CONFLICT) == (1, 2, 4)
    assert (_capi.DIGEST_ROWS, _capi.DIGEST_STATE, _capi.DIFF_NONE) == (0, 1, dc.NONE)
    assert "CRDT_DIFF_A_AHEAD" in txt[txt.index("Call it on the table the merged records CAME FROM"):txt.index("int crdt_export_flagged(")]


def test_struct_layout_matches_the_header(tmp_path):
    src = tmp_path / "sz.c"
    lines = ['#include "crdt_merge.h"', "#include <stdio.h>", "#include <stddef.h>", "int main(void){",
             'printf("crdt_diff %zu\\n", sizeof(crdt_diff));']
    for f, _ in _capi.CrdtDiff._fields_:
        lines.append(f'printf("{f} %zu\\n", offsetof(crdt_diff, {f}));')
    lines.append("return 0;}")
    src.write_text("\n".join(lines))
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got["crdt_diff"]) == ctypes.sizeof(_capi.CrdtDiff) == 48
    assert [f for f, _ in _capi.CrdtDiff._fields_] == list(dc.FIELDS)
    for f, _ in _capi.CrdtDiff._fields_:
        assert int(got[f]) == getattr(_capi.CrdtDiff, f).offset, f


def test_kernel_file_is_included_and_its_constants_are_the_models():
    src = open(os.path.join(ROOT, "crdt_amd", "csrc", "crdt_merge.hip")).read()
    assert src.index('#include "table_merge.inc"') < src.index('#include "table_diff.inc"')
    inc = open(os.path.join(ROOT, "crdt_amd", "csrc", "table_diff.inc")).read()
    assert re.search(r"kDfGrid = (\d+)", inc).group(1) == str(dc.GRID) == str(_capi.DIFF_GRID)
    assert dc.T == _capi.TABLE_TILE and "std::min(nb, kDfGrid), kTmThreads" in src
    for p in dc.P:
        assert f"0x{int(p):016X}ull" in inc
    assert dc.LARGE > dc.GRID * dc.T and dc.LARGE % T


def test_null_arguments_are_invalid_before_any_ctx_is_read():
    lib = _capi.load()
    out = _capi.CrdtDiff()
    ctypes.memset(ctypes.byref(out), 0x5A, ctypes.sizeof(out))
    before = bytes(out)
    fake = ctypes.create_string_buffer(1 << 20)          # (never read as a ctx: the checks below come first)
    flags = (ctypes.c_uint8 * 32)(*([0x5A] * 32))
    words = (ctypes.c_uint64 * 4)(*([0x5A5A] * 4))
    E, D = _capi.CRDT_E_INVALID, _capi.CRDT_MEM_DEVICE
    assert lib.crdt_diff_tables(None, fake, 32, flags, D, ctypes.byref(out)) == E
    assert lib.crdt_diff_tables(fake, None, 32, flags, D, ctypes.byref(out)) == E
    assert lib.crdt_diff_tables(fake, fake, 32, flags, D, None) == E
    assert lib.crdt_diff_tables(None, None, 0, None, D, None) == E
    assert lib.crdt_digest_rows(None, 32, 2048, 0, words, _capi.CRDT_MEM_HOST) == E
    assert lib.crdt_digest_rows(None, 0, 2048, 0, None, _capi.CRDT_MEM_HOST) == E
    assert bytes(out) == before and bytes(flags) == b"\x5A" * 32 and list(words) == [0x5A5A] * 4
    assert bytes(fake) == bytes(1 << 20)


def test_binding_refuses_another_device_and_short_flags():
    t, u = DeviceTable.__new__(DeviceTable), DeviceTable.__new__(DeviceTable)   # (no ctx: the checks come first)
    t.device, t._ctx, u.device, u._ctx = 0, ctypes.c_void_p(), 1, ctypes.c_void_p()
    with pytest.raises(ValueError):
        t.diff_table(u, 16)
    u.device = 0
    with pytest.raises(ValueError):
        t.diff_table(u, 16, flags=np.zeros(8, np.uint8))
