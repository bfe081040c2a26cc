"""crdt_merge_table's C surface without a GPU: the library exports it, the binding declares it with the
header's signature, the plan flag and the tile constants are the header's and the kernels' own, the call
refuses null arguments before it touches a device, and the generator of the GPU tests' cases really
produces the four decisions those tests are about."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from crdt_amd import DeviceTable, _capi
from tests import _table_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = _capi.TABLE_TILE


def _header() -> str:
    return open(os.path.join(ROOT, "include", "crdt_merge.h")).read()


def test_library_exports_the_symbol():
    _capi.load()
    out = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True).stdout
    assert "crdt_merge_table" in set(re.findall(r" T (crdt_\w+)", out))


def test_capi_declares_it_and_abi_stays_5():
    lib = _capi.load()
    res, args = _capi.SIGNATURES["crdt_merge_table"]
    assert lib.crdt_merge_table.argtypes == args and lib.crdt_merge_table.restype == res
    P, U64, I64, I32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int64, ctypes.c_int32
    assert (res, args) == (ctypes.c_int, [P, P, U64, I64, I64, P, I32, P])
    assert lib.crdt_abi_version() == _capi.ABI_VERSION == 5
    txt = _header()
    assert re.search(r"#define\s+CRDT_ABI_VERSION\s+5\b", txt)
    decl = re.search(r"^int crdt_merge_table\(([^;]*)\);", txt, flags=re.M | re.S)
    assert decl, "the header does not declare crdt_merge_table"
    params = [" ".join(p.split()) for p in decl.group(1).split(",")]
    assert params == ["crdt_ctx* dst", "crdt_ctx* src", "uint64_t n_rows", "int64_t since_lt", "int64_t wall_millis",
                      "uint8_t* row_flags", "int32_t flags_mem", "crdt_result* out"]


def test_plan_flag_is_the_headers():
    m = re.search(r"CRDT_PLAN_TABLE\s*=\s*(\d+)", _header())
    assert m and int(m.group(1)) == DeviceTable.PLAN_FLAGS["table"] == 2097152
    others = [b for k, b in DeviceTable.PLAN_FLAGS.items() if k != "table"]
    assert all(b & 2097152 == 0 for b in others) and (7 << 15) & 2097152 == 0      # (bits 15-17: rl1_pieces)


def test_tile_constants_match_the_kernels():
    """The shapes of tests/test_gpu_table_merge.py come from these: they must be the kernels' own."""
    src = open(os.path.join(ROOT, "crdt_amd", "csrc", "table_merge.inc")).read()
    threads = int(re.search(r"constexpr int kTmThreads = (\d+);", src).group(1))
    items = int(re.search(r"constexpr int kTmItems = (\d+);", src).group(1))
    assert re.search(r"constexpr int kTmTile = kTmThreads \* kTmItems;", src)
    grid = int(re.search(r"constexpr unsigned kTmClockGrid = (\d+);", src).group(1))
    assert (threads * items, grid) == (_capi.TABLE_TILE, _capi.TABLE_CLOCK_GRID)
    main = open(os.path.join(ROOT, "crdt_amd", "csrc", "crdt_merge.hip")).read()
    assert '#include "table_merge.inc"' in main


def test_null_ctxs_and_null_out_are_invalid():
    lib = _capi.load()
    res = _capi.CrdtResult()
    ctypes.memset(ctypes.byref(res), 0x5A, ctypes.sizeof(res))
    before = bytes(res)
    flags = (ctypes.c_uint8 * 32)(*([7] * 32))
    fake = ctypes.create_string_buffer(1 << 20)          # (never read: the null checks come first)
    E = _capi.CRDT_E_INVALID
    out = ctypes.byref(res)
    assert lib.crdt_merge_table(None, None, 0, 0, 0, None, _capi.CRDT_MEM_HOST, out) == E
    assert lib.crdt_merge_table(None, None, 32, 0, 0, flags, _capi.CRDT_MEM_HOST, out) == E
    assert lib.crdt_merge_table(None, fake, 32, 0, 0, flags, _capi.CRDT_MEM_HOST, out) == E
    assert lib.crdt_merge_table(fake, None, 32, 0, 0, flags, _capi.CRDT_MEM_HOST, out) == E
    assert lib.crdt_merge_table(None, None, 32, 0, 0, flags, _capi.CRDT_MEM_HOST, None) == E
    assert bytes(res) == before and bytes(flags) == bytes([7] * 32)       # nothing written on a refused call
    assert bytes(fake) == bytes(1 << 20)


# ---- the cases of the GPU tests (tests/_table_cases.py), checked where no GPU is needed
SHAPES = [0, 1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 17]


@pytest.mark.parametrize("n_rows", SHAPES)
def test_generated_cases_hold_the_four_decisions(n_rows):
    src, dst = tc.gen_pair(n_rows, seed=3000 + n_rows)
    for since in tc.sinces():
        got = tc.decisions(src, dst, n_rows, since)
        if n_rows >= tc.PLANT_FROM and since <= tc.TOP:
            assert all(v > 0 for v in got.values()), (n_rows, since, got)
    if n_rows >= T - 1:                       # and not from the planted rows alone
        got = tc.decisions(src, dst, n_rows, 0)
        assert got["tie_keeps_local"] > 1 and got["equal_lt_rank_wins"] > 1 and got["tombstone_wins"] > 1, got
        assert got["older_wins_invisible"] > 1, got


def test_generated_cases_cannot_raise_in_recv():
    """No source rank is the destination's, and no stamp is more than 60000 ms above the wall: the
    selection holds no candidate, whatever the destination's canonical."""
    src, dst = tc.gen_pair(3 * T + 17, seed=3000 + 3 * T + 17)
    assert not np.any(src["rank"] == tc.DST_RANK)
    assert int((src["lt"] >> 16).max()) - tc.MERGE_WALL <= 60000
    s = tc.dense(src, 3 * T + 17)
    assert not np.any(s["rank"] == tc.DST_RANK)                # (the fill's rank is 0x80808080)
    assert int((s["lt"] >> 16).max()) - tc.MERGE_WALL <= 60000
