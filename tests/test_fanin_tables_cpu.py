"""crdt_fanin_tables' C surface without a GPU: the library exports it, the binding declares it with the
header's signature, the ABI stays 5, the plan flag and the source bound are the header's, the call refuses
null arguments and a bad source count before it touches a device, and a numpy model of the contract
(tests/_fanin_cases.py) shows that the cases of tests/test_gpu_fanin_tables.py contain what those tests are
about: rows stored more than once in one call, under stamps that differ from step to step."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from crdt_amd import DeviceTable, _capi
from tests import _fanin_cases as fc
from tests import _sync_cases as sc
from tests import _table_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = _capi.TABLE_TILE
FANIN = 8388608


def _header() -> str:
    return open(os.path.join(ROOT, "include", "crdt_merge.h")).read()


def test_library_exports_the_symbol():
    _capi.load()
    out = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True).stdout
    assert "crdt_fanin_tables" in set(re.findall(r" T (crdt_\w+)", out))


def test_capi_declares_it_and_abi_stays_5():
    lib = _capi.load()
    res, args = _capi.SIGNATURES["crdt_fanin_tables"]
    assert lib.crdt_fanin_tables.argtypes == args and lib.crdt_fanin_tables.restype == res
    P, U32, U64, I64, I32 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int64, ctypes.c_int32
    assert (res, args) == (ctypes.c_int, [P, P, P, U32, U64, I64, P, I32, P])
    assert lib.crdt_abi_version() == _capi.ABI_VERSION == 5
    txt = _header()
    assert re.search(r"#define\s+CRDT_ABI_VERSION\s+5\b", txt)
    decl = re.search(r"^int crdt_fanin_tables\(([^;]*)\);", txt, flags=re.M | re.S)
    assert decl, "the header does not declare crdt_fanin_tables"
    params = [" ".join(p.split()) for p in re.sub(r"/\*.*?\*/", "", decl.group(1), flags=re.S).split(",")]
    assert params == ["crdt_ctx* dst", "crdt_ctx* const* srcs", "const int64_t* since_lt", "uint32_t n_src",
                      "uint64_t n_rows", "int64_t wall_millis", "uint8_t* win_mask", "int32_t mask_mem",
                      "crdt_result* out"]


def test_source_bound_is_the_headers():
    m = re.search(r"#define\s+CRDT_FANIN_MAX\s+(\d+)", _header())
    assert m and int(m.group(1)) == _capi.FANIN_MAX == fc.FANIN_MAX == 8        # one mask bit per source in a byte
    src = open(os.path.join(ROOT, "crdt_amd", "csrc", "table_merge.inc")).read()
    assert re.search(r"constexpr int kFanMax = 8;", src) and "kFanMax == CRDT_FANIN_MAX" in src
    assert fc.SHAPES_T == T


def test_plan_flag_is_the_headers():
    m = re.search(r"CRDT_PLAN_FANIN\s*=\s*(\d+)", _header())
    assert m and int(m.group(1)) == DeviceTable.PLAN_FLAGS["fanin"] == FANIN
    others = [b for k, b in DeviceTable.PLAN_FLAGS.items() if k != "fanin"]
    assert all(b & FANIN == 0 for b in others) and (7 << 15) & FANIN == 0        # (bits 15-17: rl1_pieces)
    enum = re.search(r"enum crdt_plan_flags \{(.*?)\};", re.sub(r"/\*.*?\*/", "", _header(), flags=re.S), flags=re.S)
    values = {k: int(v) for k, v in re.findall(r"(CRDT_PLAN_\w+)\s*=\s*(\d+)", enum.group(1))}
    assert values["CRDT_PLAN_FANIN"] == FANIN
    for k, v in values.items():
        if k not in ("CRDT_PLAN_FANIN", "CRDT_PLAN_RL1_PIECES_SHIFT"):
            assert v & FANIN == 0, k


def test_null_arguments_and_bad_source_counts_are_invalid():
    lib = _capi.load()
    n_out = 9
    out = (_capi.CrdtResult * n_out)()
    ctypes.memset(out, 0x5A, ctypes.sizeof(out))
    before = bytes(out)
    mask = (ctypes.c_uint8 * 32)(*([7] * 32))
    fake = ctypes.create_string_buffer(1 << 20)          # (never read: the checks below come first)
    fake_p = ctypes.cast(fake, ctypes.c_void_p).value
    since = (ctypes.c_int64 * 9)()
    srcs = (ctypes.c_void_p * 9)(*([fake_p] * 9))
    with_null = (ctypes.c_void_p * 3)(fake_p, None, fake_p)
    E, H = _capi.CRDT_E_INVALID, _capi.CRDT_MEM_HOST
    call = lib.crdt_fanin_tables
    assert call(None, srcs, since, 2, 32, 0, mask, H, out) == E
    assert call(fake, None, since, 2, 32, 0, mask, H, out) == E
    assert call(fake, srcs, None, 2, 32, 0, mask, H, out) == E
    assert call(fake, srcs, since, 2, 32, 0, mask, H, None) == E
    assert call(fake, with_null, since, 3, 32, 0, mask, H, out) == E
    assert call(None, None, None, 0, 0, 0, None, H, None) == E
    assert call(fake, srcs, since, 0, 32, 0, mask, H, out) == E              # no source
    assert call(fake, srcs, since, 9, 32, 0, mask, H, out) == E              # more than CRDT_FANIN_MAX
    assert call(fake, srcs, since, 0xFFFFFFFF, 32, 0, mask, H, out) == E
    assert bytes(out) == before                                              # nothing written on a refused call
    assert bytes(mask) == bytes([7] * 32)
    assert bytes(fake) == bytes(1 << 20)


def test_binding_refuses_unequal_lengths_and_other_devices():
    class Stub:
        device = 0
        _ctx = ctypes.c_void_p(0)
    t = DeviceTable.__new__(DeviceTable)                 # (no ctx: both checks come before the library is called)
    t.device, t._ctx = 0, ctypes.c_void_p()
    with pytest.raises(ValueError):
        t.merge_tables([Stub(), Stub()], 16, [0], 0)
    other = Stub()
    other.device = 1
    with pytest.raises(ValueError):
        t.merge_tables([Stub(), other], 16, [0, 0], 0)


# ---- the cases of the GPU tests, checked where no GPU is needed
def test_case_list_is_the_issues():
    assert fc.shapes() == [0, 1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 17]
    assert fc.DST_RANK == 7 and 0 < sc.mid() < tc.TOP
    for n_src in (2, 3, 8):
        v = fc.since_vectors(n_src)
        assert v["zero"] == [0] * n_src and v["mid"] == [sc.mid()] * n_src and v["min"] == [fc.I64_MIN] * n_src
        assert len(v["mixed"]) == n_src and tc.TOP + 1 in v["mixed"][:-1] and v["mixed"][-1] == -1
    # the generators are the issue's: checked on one seed against a direct call
    a, b = fc.source_rows(65, 4), tc.gen_rows(65, 5000 + 65 + 404, clear_at=2 / 4)
    assert all(np.array_equal(a[k], b[k]) for k in ("ids", "lt", "rank", "val", "mod")) and a["clear"] == b["clear"]
    a, b = fc.dst_rows(65), tc.gen_rows(65, 5000 + 65 + 7919, clear_at=2 / 3)
    assert all(np.array_equal(a[k], b[k]) for k in ("ids", "lt", "rank", "val", "mod")) and a["clear"] == b["clear"]


@pytest.mark.parametrize("n_src", [2, 3, 8])
@pytest.mark.parametrize("n_rows", [n for n in fc.shapes() if n >= 63])
def test_generated_cases_hold_rows_stored_more_than_once(n_rows, n_src):
    dst, srcs = fc.case(n_rows, n_src)
    most = 0
    for since in (0, sc.mid(), fc.I64_MIN):
        m = fc.model(dst, srcs, n_rows, [since] * n_src, sc.canon0(), tc.MERGE_WALL)
        multi = int((m["stores"] > 1).sum())
        assert multi >= 1, (n_rows, n_src, since)
        if since == 0:
            assert multi >= 6, (n_rows, n_src)
        if (n_rows, n_src, since) == (63, 2, sc.mid()):
            assert multi == 1                                    # the fewest of all cases
        most = max(most, int(m["stores"].max()))
        # a row stamped with another step's R would be caught: the stamps of one call are all different
        assert len(m["stamps"]) == n_src == len(set(m["stamps"])), (n_rows, n_src, since)
        assert m["statuses"] == [0] * n_src and not m["may_raise"] and m["fused"]
        # the mask is the steps' winners, and the last winner's stamp is the row's mod
        for j, win in enumerate(m["wins"]):
            assert np.array_equal((m["mask"] >> j) & 1, win.astype(np.uint8))
        stored = m["mask"] != 0
        last = np.zeros(n_rows, np.int64)
        for j, win in enumerate(m["wins"]):
            last[win] = m["stamps"][j]
        assert np.array_equal(m["rows"]["mod"][stored], last[stored])
        assert np.array_equal(m["rows"]["mod"][~stored], dst["mod"][:n_rows][~stored])
    assert most == n_src if n_src < 8 else most >= 4
    if (n_rows, n_src) == (3 * T + 17, 8):
        assert most == 7


@pytest.mark.parametrize("n_rows", fc.shapes())
def test_generated_cases_cannot_raise(n_rows):
    """No source row carries dst's local rank (0..5 against 7; the fill's is 0x80808080), no stamp is more than
    60000 ms above the wall, and no closing send() raises: every since vector runs the fused form."""
    dst, srcs = fc.case(n_rows, 8)
    for rows in srcs:
        assert not np.any(rows["rank"] == fc.DST_RANK)
        assert int((rows["lt"] >> 16).max()) - tc.MERGE_WALL <= sc.MAX_DRIFT
    for n_src in (2, 8):
        for name, sinces in fc.since_vectors(n_src).items():
            m = fc.model(dst, srcs[:n_src], n_rows, sinces, sc.canon0(), tc.MERGE_WALL, dst_cap=max(n_rows, 16))
            assert m["fused"] and len(m["statuses"]) == n_src, (n_rows, n_src, name)


def test_model_steps_are_single_merges():
    """The model's step is tests/_sync_cases.model's direction 1, the merge the other GPU tests trust."""
    n = 3 * T + 17
    dst, srcs = fc.case(n, 3)
    m = fc.model(dst, srcs, n, [0, 0, 0], sc.canon0(), tc.MERGE_WALL)
    one = sc.model(dst, srcs[0], n, tc.TOP + 1, 0, sc.canon0(), 0, tc.MERGE_WALL)
    assert np.array_equal(one["win_a"], m["wins"][0]) and one["r_a"] == m["stamps"][0]
    assert m["canonical"] == (tc.MERGE_WALL << 16) + 2           # the wall, then one counter step per later send


def test_model_knows_the_fallbacks():
    n = 3 * T + 17
    dst, srcs = fc.case(n, 3)
    c0, wall = sc.canon0(), tc.MERGE_WALL
    written = np.flatnonzero(srcs[1]["mod"] >= 0)
    at = int(written[len(written) // 2])
    s1 = {k: v.copy() for k, v in srcs[1].items()}
    s1["lt"][at], s1["rank"][at] = tc.TOP + (1 << 16), fc.DST_RANK
    assert fc.model(dst, [srcs[0], s1, srcs[2]], n, [0, 0, 0], c0, wall)["may_raise"]
    # a candidate against C_0 that the running canonical has passed by step 1: still a fallback
    s1["lt"][at] = c0 + 1
    m = fc.model(dst, [srcs[0], s1, srcs[2]], n, [0, 0, 0], c0, wall)
    assert m["may_raise"] and not m["fused"] and m["stamps"][0] > c0 + 1
    assert fc.model(dst, srcs, n, [0, 0, 0], c0, wall, dst_cap=n - 5)["out_of_range"]
    m = fc.model(dst, srcs, n, [0, 0, 0], ((wall + 5) << 16) | 0xFFFF, wall)
    assert m["statuses"] == [3] and not m["fused"]              # the sequence ends at the send() that overflows


def test_tile_patterns_select_what_their_names_say():
    n = 5 * T + 9
    pats = fc.tile_patterns(T, n)
    tiles = lambda s: set(np.flatnonzero(s) // T)  # noqa: E731
    assert [tiles(s) for s in pats["own_tiles"]] == [{0}, {1}, {2}, {3}]
    assert all(tiles(s) == {2} for s in pats["same_tile"])
    a, b, c = pats["same_tile"]
    assert (a & b).any() and (b & c).any() and (a & ~b & ~c).any()
    run, ends = pats["run_across_boundary"]
    assert tiles(run) == {1, 2} and tiles(ends) == {1, 2, 3, 5} and ends[n - 1]
    assert not any(s.any() for s in pats["none"])
