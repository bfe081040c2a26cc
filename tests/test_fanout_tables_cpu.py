"""crdt_fanout_tables' C surface without a GPU: the library exports it, the binding declares it with the
header's signature, the ABI stays 5, the plan flag and the destination bound are the header's, the call refuses
null arguments and a bad destination count before it touches a device, and a numpy model of the contract
(tests/_fanout_cases.py) shows that the cases of tests/test_gpu_fanout_tables.py contain what those tests are
about: destinations that decide differently on the same source rows, under stamps of their own."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from crdt_amd import DeviceTable, _capi
from tests import _fanout_cases as fo
from tests import _sync_cases as sc
from tests import _table_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = _capi.TABLE_TILE
FANOUT = 16777216
MW = tc.MERGE_WALL


def _header() -> str:
    return open(os.path.join(ROOT, "include", "crdt_merge.h")).read()


def test_library_exports_the_symbol():
    _capi.load()
    out = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True).stdout
    assert "crdt_fanout_tables" in set(re.findall(r" T (crdt_\w+)", out))


def test_capi_declares_it_and_abi_stays_5():
    lib = _capi.load()
    res, args = _capi.SIGNATURES["crdt_fanout_tables"]
    assert lib.crdt_fanout_tables.argtypes == args and lib.crdt_fanout_tables.restype == res
    P, U32, U64, I64, I32 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int64, ctypes.c_int32
    assert (res, args) == (ctypes.c_int, [P, P, P, U32, U64, I64, P, I32, P])
    assert lib.crdt_abi_version() == _capi.ABI_VERSION == 5
    txt = _header()
    assert re.search(r"#define\s+CRDT_ABI_VERSION\s+5\b", txt)
    decl = re.search(r"^int crdt_fanout_tables\(([^;]*)\);", txt, flags=re.M | re.S)
    assert decl, "the header does not declare crdt_fanout_tables"
    params = [" ".join(p.split()) for p in re.sub(r"/\*.*?\*/", "", decl.group(1), flags=re.S).split(",")]
    assert params == ["crdt_ctx* src", "crdt_ctx* const* dsts", "const int64_t* since_lt", "uint32_t n_dst",
                      "uint64_t n_rows", "int64_t wall_millis", "uint8_t* win_mask", "int32_t mask_mem",
                      "crdt_result* out"]


def test_destination_bound_is_the_headers():
    m = re.search(r"#define\s+CRDT_FANOUT_MAX\s+(\d+)", _header())
    assert m and int(m.group(1)) == _capi.FANOUT_MAX == fo.FANOUT_MAX == 8    # one mask bit per destination in a byte
    src = open(os.path.join(ROOT, "crdt_amd", "csrc", "table_merge.inc")).read()
    assert re.search(r"constexpr int kFoMax = 8;", src) and "kFoMax == CRDT_FANOUT_MAX" in src
    assert fo.SHAPES_T == T
    grid = re.search(r"constexpr unsigned kFoClockGrid = (\d+);", src)      # the GPU test's strided-grid case
    assert grid and int(grid.group(1)) == _capi.TABLE_CLOCK_GRID


def test_plan_flag_is_the_headers():
    m = re.search(r"CRDT_PLAN_FANOUT\s*=\s*(\d+)", _header())
    assert m and int(m.group(1)) == DeviceTable.PLAN_FLAGS["fanout"] == FANOUT
    others = [b for k, b in DeviceTable.PLAN_FLAGS.items() if k != "fanout"]
    assert all(b & FANOUT == 0 for b in others) and (7 << 15) & FANOUT == 0       # (bits 15-17: rl1_pieces)
    enum = re.search(r"enum crdt_plan_flags \{(.*?)\};", re.sub(r"/\*.*?\*/", "", _header(), flags=re.S), flags=re.S)
    values = {k: int(v) for k, v in re.findall(r"(CRDT_PLAN_\w+)\s*=\s*(\d+)", enum.group(1))}
    assert values["CRDT_PLAN_FANOUT"] == FANOUT
    for k, v in values.items():
        if k not in ("CRDT_PLAN_FANOUT", "CRDT_PLAN_RL1_PIECES_SHIFT"):
            assert v & FANOUT == 0, k


def test_null_arguments_and_bad_destination_counts_are_invalid():
    lib = _capi.load()
    n_out = 9
    out = (_capi.CrdtResult * n_out)()
    ctypes.memset(out, 0x5A, ctypes.sizeof(out))
    before = bytes(out)
    mask = (ctypes.c_uint8 * 32)(*([7] * 32))
    fake = ctypes.create_string_buffer(1 << 20)          # (never read: the checks below come first)
    fake_p = ctypes.cast(fake, ctypes.c_void_p).value
    since = (ctypes.c_int64 * 9)()
    dsts = (ctypes.c_void_p * 9)(*([fake_p] * 9))
    with_null = (ctypes.c_void_p * 3)(fake_p, None, fake_p)
    E, H = _capi.CRDT_E_INVALID, _capi.CRDT_MEM_HOST
    call = lib.crdt_fanout_tables
    assert call(None, dsts, since, 2, 32, 0, mask, H, out) == E
    assert call(fake, None, since, 2, 32, 0, mask, H, out) == E
    assert call(fake, dsts, None, 2, 32, 0, mask, H, out) == E
    assert call(fake, dsts, since, 2, 32, 0, mask, H, None) == E
    assert call(fake, with_null, since, 3, 32, 0, mask, H, out) == E
    assert call(None, None, None, 0, 0, 0, None, H, None) == E
    assert call(fake, dsts, since, 0, 32, 0, mask, H, out) == E              # no destination
    assert call(fake, dsts, since, 9, 32, 0, mask, H, out) == E              # more than CRDT_FANOUT_MAX
    assert call(fake, dsts, since, 0xFFFFFFFF, 32, 0, mask, H, out) == E
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
        t.fanout_tables([Stub(), Stub()], 16, [0], 0)
    other = Stub()
    other.device = 1
    with pytest.raises(ValueError):
        t.fanout_tables([Stub(), other], 16, [0, 0], 0)


# ---- the cases of the GPU tests, checked where no GPU is needed
def test_case_list_is_the_issues():
    assert fo.shapes() == [0, 1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 17]
    assert [fo.dst_rank(j) for j in range(8)] == list(range(7, 15)) and 0 < sc.mid() < tc.TOP
    for n_dst in (2, 3, 8):
        v = fo.since_vectors(n_dst)
        assert v["zero"] == [0] * n_dst and v["mid"] == [sc.mid()] * n_dst and v["min"] == [fo.I64_MIN] * n_dst
        assert len(v["mixed"]) == n_dst and tc.TOP + 1 in v["mixed"][:-1] and v["mixed"][-1] == -1
        assert [fo.canonical("top", j) for j in range(n_dst)] == [tc.TOP + 1 + j for j in range(n_dst)]
        assert [fo.canonical("mid", j) for j in range(n_dst)] == [sc.canon0() + j for j in range(n_dst)]
        s, d = fo.strides(n_dst)
        assert (s, d[:2]) == (32, [24, 32]) and set(d) == {24, 32}
        s, d = fo.strides(n_dst, flip=True)
        assert (s, d[:2]) == (24, [32, 24])
    # the generators are the issue's: checked on one seed against a direct call
    same = lambda a, b: all(np.array_equal(a[k], b[k]) for k in ("ids", "lt", "rank", "val", "mod")) and a["clear"] == b["clear"]  # noqa: E731
    assert same(fo.source_rows(65), tc.gen_rows(65, 6000 + 65, clear_at=1 / 3))
    assert same(fo.dst_rows(65, 4), tc.gen_rows(65, 6000 + 65 + 7919 + 404, clear_at=2 / 4))


@pytest.mark.parametrize("setting", fo.CANON_SETTINGS)
@pytest.mark.parametrize("n_dst", [2, 3, 8])
@pytest.mark.parametrize("n_rows", [n for n in fo.shapes() if n >= 63])
def test_generated_cases_hold_destinations_that_decide_differently(n_rows, n_dst, setting):
    src, dsts = fo.case(n_rows, n_dst)
    canons = [fo.canonical(setting, j) for j in range(n_dst)]
    for name, sinces in fo.since_vectors(n_dst).items():
        m = fo.model(src, dsts, n_rows, sinces, canons, MW, caps=[max(n_rows, 16)] * n_dst)
        assert m["fused"] and m["statuses"] == [0] * n_dst and not any(m["may_raise"]), (n_rows, n_dst, name)
        # the mask is the destinations' winners, and a winner's mod is its own destination's stamp
        for j, win in enumerate(m["wins"]):
            assert np.array_equal((m["mask"] >> j) & 1, win.astype(np.uint8))
            assert np.all(m["rows"][j]["mod"][win] == m["stamps"][j])
            assert np.array_equal(m["rows"][j]["mod"][~win], dsts[j]["mod"][:n_rows][~win])
        if setting == "top":
            # a row stamped with another destination's R would be caught: every stamp is its own canonical
            assert m["stamps"] == canons and len(set(m["stamps"])) == n_dst
        if name == "zero":
            assert all(int(w.sum()) >= 1 for w in m["wins"]), (n_rows, n_dst)
            differ = sum(not np.array_equal(m["wins"][0], w) for w in m["wins"][1:])
            assert differ >= 1, (n_rows, n_dst)
    if setting == "mid":                                     # some selected lts lie above the canonical
        assert (src["lt"][:n_rows][src["mod"][:n_rows] >= 0] > canons[0]).any()
        m = fo.model(src, dsts, n_rows, [0] * n_dst, canons, MW)
        assert all(r > c for r, c in zip(m["stamps"], canons))


@pytest.mark.parametrize("n_rows", fo.shapes())
def test_generated_cases_cannot_raise(n_rows):
    """No source row carries a destination's local rank (0..5 against 7..14; the fill's is 0x80808080), no stamp
    is more than 60000 ms above the wall, and no closing send() raises: every since vector runs the fused form."""
    src, dsts = fo.case(n_rows, 8)
    assert not np.any(np.isin(src["rank"], [fo.dst_rank(j) for j in range(8)]))
    assert int((src["lt"] >> 16).max()) - MW <= sc.MAX_DRIFT
    for setting in fo.CANON_SETTINGS:
        for n_dst in (2, 8):
            canons = [fo.canonical(setting, j) for j in range(n_dst)]
            for name, sinces in fo.since_vectors(n_dst).items():
                m = fo.model(src, dsts[:n_dst], n_rows, sinces, canons, MW, caps=[max(n_rows, 16)] * n_dst)
                assert m["fused"] and len(m["statuses"]) == n_dst, (n_rows, n_dst, name)


def test_model_steps_are_single_merges():
    """The model's step is tests/_sync_cases.model's direction 1, the merge the other GPU tests trust."""
    n = 3 * T + 17
    src, dsts = fo.case(n, 3)
    canons = [fo.canonical("mid", j) for j in range(3)]
    m = fo.model(src, dsts, n, [0, sc.mid(), 0], canons, MW)
    for j, since in enumerate([0, sc.mid(), 0]):
        one = sc.model(dsts[j], src, n, tc.TOP + 1, since, canons[j], 0, MW, rank_a=fo.dst_rank(j))
        assert np.array_equal(one["win_a"], m["wins"][j]) and one["r_a"] == m["stamps"][j]
        assert one["canon_a"] == m["canonical"][j] == MW << 16     # every destination's own send: the wall, counter 0


def test_model_knows_the_fallbacks():
    n = 3 * T + 17
    src, dsts = fo.case(n, 3)
    canons = [fo.canonical("mid", j) for j in range(3)]
    written = np.flatnonzero(src["mod"] >= 0)
    at = int(written[len(written) // 2])
    # a candidate for destination 1 only: its own rank above its canonical
    s = {k: v.copy() for k, v in src.items()}
    s["lt"][at], s["rank"][at] = tc.TOP + (1 << 16), fo.dst_rank(1)
    m = fo.model(s, dsts, n, [0, 0, 0], canons, MW)
    assert m["may_raise"] == [False, True, False] and not m["fused"]
    assert fo.model(s, dsts, n, [0, tc.TOP + 1, 0], canons, MW)["fused"]        # (not selected for it: fused)
    # an id out of one destination's range
    m = fo.model(src, dsts, n, [0, 0, 0], canons, MW, caps=[n, n - 5, n])
    assert m["out_of_range"] == [False, True, False] and not m["fused"]
    # a send that overflows, at one destination
    m = fo.model(src, dsts, n, [0, 0, 0], [canons[0], canons[1], ((MW + 5) << 16) | 0xFFFF], MW)
    assert m["statuses"] == [0, 0, 3] and not m["fused"]


def test_nested_patterns_select_what_their_names_say():
    n = 5 * T + 9
    pats = fo.nested_patterns(T, n)
    tiles = lambda s: set(np.flatnonzero(s) // T)  # noqa: E731
    assert [tiles(s) for s in pats["own_tiles"]] == [{0, 1, 2, 3}, {1, 2, 3}, {2, 3}, {3}]
    assert all(tiles(s) == {2} for s in pats["same_tile"])
    a, b, c = pats["same_tile"]
    assert (a & ~b).any() and (b & ~c).any() and c.any()
    run, ends = pats["run_across_boundary"]
    assert tiles(run) == {1, 2, 3, 5} and tiles(ends) == {1, 2, 3, 5} and ends[n - 1] and int(ends.sum()) == 4
    assert not any(s.any() for s in pats["none"])
    for name, sels in pats.items():
        mod, sinces = fo.nested_mods(sels, tc.STAMPS)
        assert sinces == sorted(sinces) and mod.min() >= 0
        for sel, since in zip(sels, sinces):
            assert np.array_equal(~(mod < since), sel), name
