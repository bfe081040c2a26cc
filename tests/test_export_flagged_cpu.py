"""crdt_export_flagged's C surface without a GPU: the library exports it, the binding declares it with the
header's signature, the ABI stays 5, the call refuses null arguments before it touches a device, and the numpy
model of the contract (tests/_flagged_cases.py) agrees with a row-by-row loop on the patterns the GPU tests use."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from crdt_amd import DeviceTable, _capi
from tests import _flagged_cases as fl
from tests._cases import NULL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header() -> str:
    return open(os.path.join(ROOT, "include", "crdt_merge.h")).read()


def test_library_exports_the_symbol():
    _capi.load()
    out = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True).stdout
    assert "crdt_export_flagged" in set(re.findall(r" T (crdt_\w+)", out))


def test_capi_declares_it_and_abi_stays_5():
    lib = _capi.load()
    res, args = _capi.SIGNATURES["crdt_export_flagged"]
    assert lib.crdt_export_flagged.argtypes == args and lib.crdt_export_flagged.restype == res
    P, U8, U64, I32 = ctypes.c_void_p, ctypes.c_uint8, ctypes.c_uint64, ctypes.c_int32
    assert (res, args) == (ctypes.c_int, [P, U64, P, I32, U8, P])
    assert lib.crdt_abi_version() == _capi.ABI_VERSION == 5
    txt = _header()
    assert re.search(r"#define\s+CRDT_ABI_VERSION\s+5\b", txt)
    decl = re.search(r"^int crdt_export_flagged\(([^;]*)\);", txt, flags=re.M | re.S)
    assert decl, "the header does not declare crdt_export_flagged"
    params = [" ".join(p.split()) for p in re.sub(r"/\*.*?\*/", "", decl.group(1), flags=re.S).split(",")]
    assert params == ["crdt_ctx* ctx", "uint64_t n_rows", "const uint8_t* flags", "int32_t flags_mem",
                      "uint8_t bits", "crdt_export* out"]


def test_tile_constants_are_the_kernels():
    assert (fl.T, fl.SCAN_STEP, fl.COUNT_GRID) == (_capi.EXPORT_TILE, _capi.EXPORT_SCAN_STEP, _capi.EXPORT_COUNT_GRID)
    src = open(os.path.join(ROOT, "crdt_amd", "csrc", "crdt_merge.hip")).read()
    assert "k_xf_count<<<std::min(nb, kExCountGrid), kExThreads" in src       # the capped, striding grids
    assert "k_xf_write<<<std::min(nb, kExCountGrid), kExThreads" in src
    assert fl.LARGE_SHAPES[0] > fl.SCAN_STEP * fl.T and fl.LARGE_SHAPES[1] > fl.COUNT_GRID * fl.T


def test_null_arguments_are_invalid():
    lib = _capi.load()
    view = _capi.CrdtExport()
    ctypes.memset(ctypes.byref(view), 0x5A, ctypes.sizeof(view))
    before = bytes(view)
    fake = ctypes.create_string_buffer(1 << 20)          # (never read: the checks below come first)
    flags = (ctypes.c_uint8 * 32)(*([1] * 32))
    E, D = _capi.CRDT_E_INVALID, _capi.CRDT_MEM_DEVICE
    call = lib.crdt_export_flagged
    assert call(None, 32, flags, D, 1, ctypes.byref(view)) == E
    assert call(None, 0, None, D, 0, None) == E
    assert call(fake, 32, flags, D, 1, None) == E
    assert call(fake, 32, None, D, 1, ctypes.byref(view)) == E               # rows, but no flags
    assert bytes(view) == before                                              # nothing written on a refused call
    assert bytes(fake) == bytes(1 << 20)


def test_binding_refuses_short_flags_and_bad_bits():
    class Flags:                                         # (stands in for a CUDA tensor: the checks come first)
        __module__ = "torch"
        is_cuda = True

        def numel(self):
            return 8
    Flags.__module__ = "torch"
    t = DeviceTable.__new__(DeviceTable)                 # (no ctx: both checks come before the library is called)
    t.device, t._ctx = 0, ctypes.c_void_p()
    with pytest.raises(ValueError):
        t.export_flagged(16, Flags())
    with pytest.raises(ValueError):
        t.export_flagged(16, np.zeros(8, np.uint8))
    with pytest.raises(ValueError):
        t.export_flagged(8, np.zeros(8, np.uint8), bits=0x100)


def _rows(n: int, seed: int) -> dict:
    rng = np.random.default_rng(seed)
    val = rng.integers(0, 1 << 20, n).astype(np.uint32)
    val[rng.random(n) < 0.2] = NULL
    return {"lt": rng.integers(0, 1 << 50, n), "rank": rng.integers(0, 6, n).astype(np.uint32), "val": val,
            "mod": rng.integers(-(1 << 20), 1 << 50, n)}


@pytest.mark.parametrize("n_rows", [0, 1, fl.T - 1, fl.T + 1, 3 * fl.T + 9])
def test_model_agrees_with_a_loop(n_rows):
    rows = _rows(n_rows + 5, n_rows)
    for name, sel in fl.patterns(n_rows, high_water=n_rows // 2).items():
        for bits in fl.BITS:
            flags = np.concatenate([fl.mask_bytes(sel, bits), np.full(5, 0xFF, np.uint8)])   # ones beyond n_rows
            m, b = fl.model(rows, n_rows, flags, bits), fl.brute_force(rows, n_rows, flags, bits)
            assert m["n"] == b["n"] == (int(sel.sum()) if bits else 0), (name, bits)
            assert m["n_live"] == b["n_live"], (name, bits)
            assert np.array_equal(m["key"], np.array(b["key"], np.uint32)), (name, bits)
            for c in fl.COLS:
                assert np.array_equal(m[c], np.array(b[c], m[c].dtype)), (name, bits, c)
            if bits:
                assert np.array_equal(m["key"], np.flatnonzero(sel)), (name, bits)


def test_patterns_are_the_issues():
    n = 5 * fl.T + 9
    p = fl.patterns(n, high_water=4 * fl.T)
    tiles = lambda s: sorted(set(np.flatnonzero(s) // fl.T))  # noqa: E731
    assert not p["none"].any() and p["all"].all()
    assert 0.45 < p["half"].mean() < 0.55 and 0.005 < p["one_percent"].mean() < 0.02
    for name, lane in (("lane0_of_each_tile", 0), ("lane63_of_each_tile", 63), ("last_row_of_each_tile", fl.T - 1)):
        ids = np.flatnonzero(p[name])
        assert np.all(ids % fl.T == lane) and len(ids) == len(tiles(p[name])) >= 5, name
    assert np.flatnonzero(p["last_row"]).tolist() == [n - 1]
    assert np.flatnonzero(p["above_high_water"]).min() == 4 * fl.T
    assert tiles(p["empty_tile_between_full"]) == [0, 2] and int(p["empty_tile_between_full"].sum()) == 2 * fl.T
    assert set(fl.SHAPES) == {0, 1, 2047, 2048, 2049, 5 * 2048 + 9} and set(fl.BITS) == {0x01, 0x80, 0x05, 0xFF, 0}
