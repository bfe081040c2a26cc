"""crdt_sync_tables' C surface without a GPU: the library exports it, the binding declares it with the
header's signature, the ABI stays 5, the plan flag and the clock grid are the header's and the kernels' own,
the call refuses null arguments before it touches a device, and a numpy model of the contract
(tests/_sync_cases.py) shows that the cases of tests/test_gpu_sync_tables.py contain what those tests are
about."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from crdt_amd import DeviceTable, _capi
from tests import _sync_cases as sc
from tests import _table_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = _capi.TABLE_TILE


def _header() -> str:
    return open(os.path.join(ROOT, "include", "crdt_merge.h")).read()


def test_library_exports_the_symbol():
    _capi.load()
    out = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True).stdout
    assert "crdt_sync_tables" in set(re.findall(r" T (crdt_\w+)", out))


def test_capi_declares_it_and_abi_stays_5():
    lib = _capi.load()
    res, args = _capi.SIGNATURES["crdt_sync_tables"]
    assert lib.crdt_sync_tables.argtypes == args and lib.crdt_sync_tables.restype == res
    P, U64, I64, I32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int64, ctypes.c_int32
    assert (res, args) == (ctypes.c_int, [P, P, U64, I64, I64, I64, P, P, I32, P, P])
    assert lib.crdt_abi_version() == _capi.ABI_VERSION == 5
    txt = _header()
    assert re.search(r"#define\s+CRDT_ABI_VERSION\s+5\b", txt)
    decl = re.search(r"^int crdt_sync_tables\(([^;]*)\);", txt, flags=re.M | re.S)
    assert decl, "the header does not declare crdt_sync_tables"
    params = [" ".join(p.split()) for p in decl.group(1).split(",")]
    assert params == ["crdt_ctx* a", "crdt_ctx* b", "uint64_t n_rows", "int64_t since_a", "int64_t since_b",
                      "int64_t wall_millis", "uint8_t* flags_a", "uint8_t* flags_b", "int32_t flags_mem",
                      "crdt_result* out_a", "crdt_result* out_b"]


def test_plan_flag_is_the_headers():
    m = re.search(r"CRDT_PLAN_SYNC\s*=\s*(\d+)", _header())
    assert m and int(m.group(1)) == DeviceTable.PLAN_FLAGS["sync"] == 4194304
    others = [b for k, b in DeviceTable.PLAN_FLAGS.items() if k != "sync"]
    assert all(b & 4194304 == 0 for b in others) and (7 << 15) & 4194304 == 0      # (bits 15-17: rl1_pieces)
    enum = re.search(r"enum crdt_plan_flags \{(.*?)\};", re.sub(r"/\*.*?\*/", "", _header(), flags=re.S), flags=re.S)
    values = {k: int(v) for k, v in re.findall(r"(CRDT_PLAN_\w+)\s*=\s*(\d+)", enum.group(1))}
    for k, v in values.items():
        if k not in ("CRDT_PLAN_SYNC", "CRDT_PLAN_RL1_PIECES_SHIFT"):
            assert v & 4194304 == 0, k


def test_clock_grid_matches_the_kernels():
    """The clock-grid case of tests/test_gpu_sync_tables.py comes from this: it must be the kernels' own,
    and the sync kernels keep crdt_merge_table's tile."""
    src = open(os.path.join(ROOT, "crdt_amd", "csrc", "table_merge.inc")).read()
    grid = int(re.search(r"constexpr unsigned kSyClockGrid = (\d+);", src).group(1))
    assert grid == _capi.SYNC_CLOCK_GRID
    assert re.search(r"k_sy_clock<<<std::min\(nb, kSyClockGrid\), kTmThreads,",
                     open(os.path.join(ROOT, "crdt_amd", "csrc", "crdt_merge.hip")).read())
    assert sc.SHAPES_T == T


def test_null_ctxs_and_null_outs_are_invalid():
    lib = _capi.load()
    ra, rb = _capi.CrdtResult(), _capi.CrdtResult()
    for r in (ra, rb):
        ctypes.memset(ctypes.byref(r), 0x5A, ctypes.sizeof(r))
    before = bytes(ra)
    fa = (ctypes.c_uint8 * 32)(*([7] * 32))
    fb = (ctypes.c_uint8 * 32)(*([7] * 32))
    fake = ctypes.create_string_buffer(1 << 20)          # (never read: the null checks come first)
    E, H = _capi.CRDT_E_INVALID, _capi.CRDT_MEM_HOST
    oa, ob = ctypes.byref(ra), ctypes.byref(rb)
    assert lib.crdt_sync_tables(None, None, 0, 0, 0, 0, None, None, H, oa, ob) == E
    assert lib.crdt_sync_tables(None, None, 32, 0, 0, 0, fa, fb, H, oa, ob) == E
    assert lib.crdt_sync_tables(None, fake, 32, 0, 0, 0, fa, fb, H, oa, ob) == E
    assert lib.crdt_sync_tables(fake, None, 32, 0, 0, 0, fa, fb, H, oa, ob) == E
    assert lib.crdt_sync_tables(None, None, 32, 0, 0, 0, fa, fb, H, None, ob) == E
    assert lib.crdt_sync_tables(None, None, 32, 0, 0, 0, fa, fb, H, oa, None) == E
    assert lib.crdt_sync_tables(None, None, 32, 0, 0, 0, fa, fb, H, None, None) == E
    assert bytes(ra) == before and bytes(rb) == before                     # nothing written on a refused call
    assert bytes(fa) == bytes([7] * 32) and bytes(fb) == bytes([7] * 32)
    assert bytes(fake) == bytes(1 << 20)


# ---- the cases of the GPU tests, checked where no GPU is needed
def _model(n, since_a, since_b):
    a, b = sc.pair(n, seed=3000 + n)
    cap = max(n, 16)
    return sc.model(tc.dense(a, cap), tc.dense(b, cap), n, since_a, since_b, sc.canon0(), sc.C_B, tc.MERGE_WALL)


def test_case_list_is_the_issues():
    top, m = tc.TOP, sc.mid()
    assert sc.shapes() == [0, 1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 17]
    assert sc.since_pairs() == [(0, 0), (m, m), (0, sc.I64_MIN), (sc.I64_MIN, 0), (-1, top), (m, top + 1),
                                (top, 0), (top + 1, m)]
    assert 0 < m < top and (sc.A_RANK, sc.B_RANK, sc.C_B) == (7, 6, 123)


@pytest.mark.parametrize("n_rows", [n for n in sc.shapes() if n >= tc.PLANT_FROM])
def test_generated_cases_hold_what_the_gpu_tests_are_about(n_rows):
    m = _model(n_rows, 0, 0)
    assert m["fused"] and m["win_a"].any() and m["win_b"].any() and m["ties_kept"].any(), n_rows
    assert not (m["win_a"] & m["win_b"]).any()
    m = _model(n_rows, 0, sc.I64_MIN)                    # b's invisible rows selected: they win into a and come
    assert m["fused"] and m["both"].any(), n_rows        # back visible
    if n_rows == 63:
        assert int(m["both"].sum()) == 7
    if n_rows == 3 * T + 17:
        assert int(m["both"].sum()) == 366
    # since_a above every lt and both canonicals: R_a < since_a whatever b's selection holds (the fallback).
    # since_a == TOP is the boundary: some selected row of b carries lt == TOP from 63 rows on, so R_a == TOP,
    # step 1's winners (mod = TOP) are selected again and the fused form runs.
    m = _model(n_rows, tc.TOP + 1, sc.mid())
    assert m["ra_below_since_a"] and not m["fused"] and m["win_a"].any() and not m["win_b"].any()
    m = _model(n_rows, tc.TOP, 0)
    assert m["r_a"] == tc.TOP and not m["ra_below_since_a"] and m["fused"]
    assert (m["win_a"] & m["sel_a"]).sum() == m["win_a"].sum() > 0


@pytest.mark.parametrize("n_rows", sc.shapes())
def test_generated_cases_cannot_raise_in_either_direction(n_rows):
    """Neither replica's rows carry the other's local rank (0..5 against 7 and 6; the fill's is 0x80808080),
    no stamp is more than 60000 ms above the wall, and no closing send() raises."""
    a, b = sc.pair(n_rows, seed=3000 + n_rows)
    cap = max(n_rows, 16)
    A, B = tc.dense(a, cap), tc.dense(b, cap)
    for rows in (A, B):
        assert not np.any((rows["rank"] == sc.A_RANK) | (rows["rank"] == sc.B_RANK))
        assert int((rows["lt"] >> 16).max()) - tc.MERGE_WALL <= sc.MAX_DRIFT
    for since_a, since_b in sc.since_pairs():
        m = sc.model(A, B, n_rows, since_a, since_b, sc.canon0(), sc.C_B, tc.MERGE_WALL)
        assert not m["may_raise_1"] and not m["may_raise_2"], (n_rows, since_a, since_b)
        assert m["status_1"] == 0 and m["status_2"] == 0
        assert m["fused"] == (not m["ra_below_since_a"])


def test_tile_patterns_select_what_their_names_say():
    n = 5 * T + 9
    pats = sc.patterns(T, n)
    tiles = lambda s: set(np.flatnonzero(s) // T)  # noqa: E731
    assert pats["only_a"][0].any() and not pats["only_a"][1].any()
    assert pats["only_b"][1].any() and not pats["only_b"][0].any()
    sa, sb = pats["disjoint_tiles"]
    assert tiles(sa) and tiles(sb) and not (tiles(sa) & tiles(sb))
    sa, sb = pats["same_tile"]
    assert tiles(sa) == tiles(sb) == {2} and (sa & sb).any() and (sa & ~sb).any() and (sb & ~sa).any()
    sa, sb = pats["tile_ends"]
    assert sa[2 * T] and sb[3 * T - 1] and sa[4 * T - 1] and sb[4 * T - 1] and sb[4 * T]
    sa, sb = pats["run_across_boundary"]
    assert tiles(sa) == {1, 2} and tiles(sb) == {3, 4}
    assert not pats["none"][0].any() and not pats["none"][1].any()
