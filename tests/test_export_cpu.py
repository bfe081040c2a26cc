"""The changeset export's C surface without a GPU: the built library exports the new entry
points, the ctypes binding declares them with the header's layout, and every one of them refuses
a null ctx (and null out pointers) before it touches a device."""
import ctypes
import os
import re
import subprocess

from crdt_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("crdt_export_since", "crdt_export_read", "crdt_export_release", "crdt_count_since")


def test_library_exports_the_export_symbols():
    _capi.load()
    out = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (crdt_\w+)", out))
    assert set(NEW) <= exported, set(NEW) - exported


def test_capi_declares_them_and_abi_stays_5():
    lib = _capi.load()
    for name in NEW:
        assert name in _capi.SIGNATURES, name
        assert getattr(lib, name).argtypes == _capi.SIGNATURES[name][1]
    assert lib.crdt_abi_version() == _capi.ABI_VERSION == 5
    txt = open(os.path.join(ROOT, "include", "crdt_merge.h")).read()
    assert re.search(r"#define\s+CRDT_ABI_VERSION\s+5\b", txt)
    for name in NEW:
        assert re.search(rf"^int {name}\(", txt, flags=re.M), name


def test_export_struct_layout_matches_header(tmp_path):
    src = tmp_path / "sz.c"
    lines = ['#include "crdt_merge.h"', "#include <stdio.h>", "#include <stddef.h>", "int main(void){",
             'printf("size %zu\\n", sizeof(crdt_export));']
    for f, _ in _capi.CrdtExport._fields_:
        lines.append(f'printf("{f} %zu\\n", offsetof(crdt_export, {f}));')
    lines.append("return 0;}")
    src.write_text("\n".join(lines))
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == ctypes.sizeof(_capi.CrdtExport)
    for f, _ in _capi.CrdtExport._fields_:
        assert int(got[f]) == getattr(_capi.CrdtExport, f).offset, f


def test_null_ctx_and_null_outs_are_invalid():
    lib = _capi.load()
    view = _capi.CrdtExport()
    n, live = ctypes.c_uint64(7), ctypes.c_uint64(7)
    key = (ctypes.c_uint32 * 4)()
    assert lib.crdt_export_since(None, 0, 0, ctypes.byref(view)) == _capi.CRDT_E_INVALID
    assert lib.crdt_export_since(None, 16, 0, None) == _capi.CRDT_E_INVALID
    assert lib.crdt_count_since(None, 0, 0, ctypes.byref(n), ctypes.byref(live)) == _capi.CRDT_E_INVALID
    assert lib.crdt_count_since(None, 16, 0, None, None) == _capi.CRDT_E_INVALID
    assert (n.value, live.value) == (7, 7)                      # nothing written on a refused call
    assert lib.crdt_export_read(None, 0, 4, key, None, None, None, None) == _capi.CRDT_E_INVALID
    assert lib.crdt_export_read(None, 0, 0, None, None, None, None, None) == _capi.CRDT_E_INVALID
    assert lib.crdt_export_release(None) == _capi.CRDT_E_INVALID


def test_tile_constants_match_the_kernels():
    """The shapes of tests/test_gpu_export.py come from these: they must be the kernels' own."""
    src = open(os.path.join(ROOT, "crdt_amd", "csrc", "crdt_merge.hip")).read()
    threads = int(re.search(r"constexpr int kExThreads = (\d+);", src).group(1))
    items = int(re.search(r"constexpr int kExItems = (\d+);", src).group(1))
    step = int(re.search(r"constexpr int kExScanStep = (\d+);", src).group(1))
    assert re.search(r"constexpr int kExTile = kExThreads \* kExItems;", src)
    grid = int(re.search(r"constexpr unsigned kExCountGrid = (\d+);", src).group(1))
    assert (threads * items, step, grid) == (_capi.EXPORT_TILE, _capi.EXPORT_SCAN_STEP, _capi.EXPORT_COUNT_GRID)
