"""The model of crdt_purge_tombstones (tests/_purge_cases.py) against MapCrdt.purgeDeleted's object-level
definition run on the oracle's MapCrdts, which delete from ``_map``, on small mirrored maps; the generator's
self-checks at every shape the GPU tests use; and the header's declaration.  No GPU, no library."""
import os
import re

import numpy as np
import pytest

from oracle import crdt_oracle as O
from oracle.oracle_c import OracleTable
from tests import _purge_cases as pc
from tests import _table_cases as tc
from tests._cases import NULL, WALL

NODES = ["a", "b", "c", "d"]              # ranks are their positions (already in compareTo order)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def mirror(maps: list):
    """One OracleTable per map over the group's key ids (first-seen order over the maps); (tables, names)."""
    names = []
    for m in maps:
        names += [k for k in m._map if k not in names]
    tables = []
    for m in maps:
        o = OracleTable(len(names) + 3, NODES.index(m.node_id), m.canonical_time.logical_time)
        for i, k in enumerate(names):
            r = m._map.get(k)
            if r is not None:
                val = NULL if r.value is None else 1000 + i + 17 * len(str(r.value))
                o.put_rows([i], [r.hlc.logical_time], [NODES.index(r.hlc.node_id)], [val], [r.modified.logical_time])
        tables.append(o)
    return tables, names


def run_both(maps: list, before_lt):
    """The definition on the maps and the model on their mirrors; compares everything; returns the purged keys."""
    tables, names = mirror(maps)
    n = len(names)
    canon = [m.canonical_time.logical_time for m in maps]
    for m in maps:
        m.events.clear()
    bound = pc.I64_MAX if before_lt is None else before_lt
    want_cand = [k for k, r in maps[0].record_map().items() if r.is_deleted and r.hlc.logical_time < bound]
    purged = pc.purge_definition(maps, before_lt)
    res, flags = pc.model_purge(tables, n, bound)
    assert [names[i] for i in np.flatnonzero(flags)] == sorted(purged, key=names.index)
    assert res == {"n_candidates": len(want_cand), "n_purged": len(purged)}
    for m, o, c in zip(maps, tables, canon):
        assert not m.events and m.canonical_time.logical_time == o.canonical == c
        for i, k in enumerate(names):
            r, row = m._map.get(k), o.rows[i]
            if r is None:
                assert np.all(o.rows[i:i + 1].view(np.uint8) == 0x80), k      # the never-written row
            else:
                assert (int(row["lt"]), NODES[row["rank"]], int(row["mod"]), row["val"] == NULL) == \
                    (r.hlc.logical_time, r.hlc.node_id, r.modified.logical_time, r.value is None), k
        assert np.all(o.rows["mod"][n:] < 0)
    return purged


def single(wall=WALL) -> O.MapCrdt:
    m = O.MapCrdt("b")
    m.put_all({"k0": 0, "k1": 1, "k2": 2, "k3": 3}, wall)
    m.delete("k1", wall + 5)
    m.delete("k3", wall + 9)
    m.put_record("k4", O.Record(O.Hlc(wall, 0, "a"), None, O.Hlc.from_logical_time(-7, "b")))    # invisible tombstone
    m.put_record("k5", O.Record(O.Hlc.from_logical_time(-(9 << 16), "c"), None, O.Hlc(wall, 0, "b")))   # negative lt
    return m


def trio(wall=WALL):
    """Three replicas: converged on k1's deletion, c behind on k3's, b with k5 under another node."""
    a, b, c = O.MapCrdt("a"), O.MapCrdt("b"), O.MapCrdt("c")
    a.put_all({"k0": 0, "k1": 1, "k2": 2, "k3": 3, "k6": 6}, wall)
    a.delete("k1", wall + 5)
    for m in (b, c):
        m.merge(dict(a.record_map()), wall + 6)
    a.delete("k3", wall + 9)
    a.delete("k6", wall + 9)
    b.merge(dict(a.record_map()), wall + 10)                     # c has not seen k3's and k6's deletion
    c.put("k6", None, wall + 9)                                  # ... and deleted k6 itself: another Hlc
    t = O.Hlc(wall + 2, 1, "a")
    a.put_record("k5", O.Record(t, None, t))
    b.put_record("k5", O.Record(O.Hlc(wall + 2, 1, "d"), None, t))    # same lt, another node
    c.put_record("k5", O.Record(t, None, t))
    c.put_record("k7", O.Record(t, None, t))                     # only c holds it
    return [a, b, c]


@pytest.mark.parametrize("before", [None, "at", "above", "below", "min"])
def test_single_map(before):
    m = single()
    at = m._map["k1"].hlc.logical_time
    bound = {None: None, "at": at, "above": at + 1, "below": at - 1, "min": pc.I64_MIN}[before]
    purged = run_both([m], bound)
    want = {None: ["k1", "k3", "k5"], "at": ["k5"], "above": ["k1", "k5"], "below": ["k5"], "min": []}[before]
    assert purged == want
    assert "k4" in m._map and m.get_record("k0").value == 0
    assert run_both([m], bound) == []                            # nothing left to collect


@pytest.mark.parametrize("before", [None, "at", "above", "below"])
def test_three_members(before):
    maps = trio()
    at = maps[0]._map["k1"].hlc.logical_time
    bound = {None: None, "at": at, "above": at + 1, "below": at - 1}[before]
    purged = run_both(maps, bound)
    assert purged == ([] if before in ("at", "below") else ["k1"])
    for m in maps[:2]:
        assert m._map["k3"].is_deleted and m._map["k5"].is_deleted      # blocked: c is behind, b differs
    assert maps[2]._map["k3"].value == 3 and "k7" in maps[2]._map
    left = ["k1"] if before in ("at", "below") else []
    assert run_both(maps[:2], None) == left + ["k3", "k6"]       # the two that have synced agree on them


def test_member_order_decides_the_candidates_only():
    maps = trio()
    assert run_both([maps[2], maps[0], maps[1]], None) == ["k1"]      # k7 is a candidate of c's, blocked by a


@pytest.mark.parametrize("n_members", pc.MEMBERS)
@pytest.mark.parametrize("n_rows", pc.SHAPES + (pc.T + 9, 2 * pc.T + 5, 3 * pc.T + 17))
def test_generator_self_checks(n_rows, n_members):
    members = pc.gen_group(n_rows, n_members, 700 + n_rows + n_members)
    assert len(members) == n_members
    if n_rows >= pc.PLANT_FROM:
        got = pc.self_check(members, n_rows, pc.BEFORE)
        assert all(got[k] > 0 for k in (pc.KINDS if n_members > 1 else ("lt_at_before", "first_last"))), got
        for gen, all_purged in ((pc.gen_agreed, True), (pc.gen_blocked, False), (pc.gen_no_tombstone, False)):
            group = gen(n_rows, max(n_members, 2), 800 + n_rows)
            cand, purged = pc.masks([tc.dense(m, n_rows + 1) for m in group], n_rows, pc.BEFORE)
            assert cand.any() == (gen is not pc.gen_no_tombstone)
            assert np.array_equal(purged, cand) if all_purged else not purged.any()


def test_generator_self_checks_large():
    members = pc.gen_group(pc.LARGE, 2, 7)
    assert pc.LARGE > pc.GRID * pc.T and pc.self_check(members, pc.LARGE, pc.BEFORE)["first_last"]


def test_model_writes_the_never_written_row():
    members = pc.gen_group(pc.T + 9, 3, 11)
    tables = []
    for j, m in enumerate(members):
        o = OracleTable(pc.T + 9 + 5 + j, j, 77)
        o.put_rows(*(m[k] for k in ("ids", "lt", "rank", "val", "mod")))
        first, count = m["clear"]
        o.rows[first:first + count].view(np.uint8)[:] = 0x80
        tables.append(o)
    before = [o.rows.copy() for o in tables]
    res, flags = pc.model_purge(tables, pc.T + 9, pc.BEFORE)
    ids = np.flatnonzero(flags)
    assert res["n_purged"] == len(ids) > 0 and res["n_candidates"] > res["n_purged"]
    for o, b in zip(tables, before):
        assert np.all(o.rows[ids].view(np.uint8) == 0x80) and o.canonical == 77
        rest = np.ones(len(b), bool)
        rest[ids] = False
        assert np.array_equal(o.rows[rest], b[rest])
    assert pc.model_purge(tables, pc.T + 9, pc.BEFORE)[0] == {"n_candidates": res["n_candidates"] - len(ids),
                                                              "n_purged": 0}


def test_header_declares_the_call_and_the_abi_stays():
    import ctypes

    from crdt_amd import _capi
    text = open(os.path.join(ROOT, "include", "crdt_merge.h")).read()
    assert re.search(r"#define\s+CRDT_ABI_VERSION\s+5\b", text) and _capi.ABI_VERSION == 5
    assert re.search(r"#define\s+CRDT_PURGE_MAX\s+8\b", text) and _capi.PURGE_MAX == 8
    assert re.search(r"typedef struct crdt_purge \{ uint64_t n_candidates, n_purged; \} crdt_purge;", text)
    decl = re.search(r"int crdt_purge_tombstones\(([^;]*)\);", text).group(1)
    assert re.sub(r"\s+", " ", decl) == ("crdt_ctx* const* ctxs, uint32_t n_ctx, uint64_t n_rows, int64_t before_lt, "
                                         "uint8_t* row_flags, int32_t flags_mem, crdt_purge* out")
    P, U32, U64, I64, I32 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int64, ctypes.c_int32
    assert _capi.SIGNATURES["crdt_purge_tombstones"] == (ctypes.c_int, [P, U32, U64, I64, P, I32, P])
    assert ctypes.sizeof(_capi.CrdtPurge) == 16
    assert "crdt_purge_tombstones(ctxs, .., row_flags)" in text          # crdt_export_flagged's list
    assert '#include "table_purge.inc"' in open(os.path.join(ROOT, "crdt_amd", "csrc", "crdt_merge.hip")).read()
