"""The model of crdt_diff_group (tests/_group_cases.py) against a per-key restatement of the definition in plain
Python, against the pairwise model for two members, and under permutation of the members; the generator's
self-checks at every shape the GPU tests use; and the header's declaration.  No GPU, no library."""
import os
import re

import numpy as np
import pytest

from tests import _diff_cases as dc
from tests import _group_cases as gc
from tests import _table_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def brute(tables: list, n_rows: int):
    """The definition, one row and one member at a time, on Python ints and tuples."""
    m = len(tables)
    behind, hold, conflict = np.zeros(n_rows, np.uint8), np.zeros(n_rows, np.uint8), np.zeros(n_rows, np.uint8)
    cols = [[t[k][:n_rows].tolist() for k in ("lt", "rank", "val", "mod")] for t in tables]
    for i in range(n_rows):
        seen = {j: (cols[j][0][i], cols[j][1][i]) for j in range(m) if cols[j][3][i] >= 0}
        if not seen:
            continue
        top = max(seen.values())
        holders = [j for j, h in seen.items() if h == top]
        hold[i] = sum(1 << j for j in holders)
        behind[i] = sum(1 << j for j in range(m) if j not in holders)
        conflict[i] = len({cols[j][2][i] for j in holders}) > 1
    pad = [0] * (gc.GROUP_MAX - m)
    nz = [i for i in range(n_rows) if behind[i] or conflict[i]]
    counts = {"n_held": int(np.count_nonzero(hold)), "n_disputed": int(np.count_nonzero(behind)),
              "n_conflict": int(conflict.sum()), "first_diff": nz[0] if nz else gc.NONE,
              "n_visible": [sum(x >= 0 for x in cols[j][3]) for j in range(m)] + pad,
              "n_behind": [sum((int(b) >> j) & 1 for b in behind) for j in range(m)] + pad,
              "n_sole": [sum(int(h) == 1 << j for h in hold) for j in range(m)] + pad}
    return behind, hold, conflict, counts


def dense_group(n_rows: int, m: int, seed: int) -> list:
    return [tc.dense(r, n_rows) for r in gc.gen_group(n_rows, m, seed)]


@pytest.mark.parametrize("m", gc.MEMBERS)
@pytest.mark.parametrize("n_rows", [0, 1, 63, 64, 65, gc.T + 1])
def test_model_against_the_definition(n_rows, m):
    tables = dense_group(n_rows, m, 900 + n_rows + m)
    got, want = gc.model_group(tables, n_rows), brute(tables, n_rows)
    for g, w in zip(got[:3], want[:3]):
        assert g.dtype == np.uint8 and np.array_equal(g, w)
    assert got[3] == want[3]
    behind, hold, _, counts = got
    assert not np.any(hold & behind)
    assert np.all((hold | behind)[hold != 0] == (1 << m) - 1) and not np.any(behind[hold == 0])
    assert counts["n_visible"][m:] == counts["n_behind"][m:] == counts["n_sole"][m:] == [0] * (gc.GROUP_MAX - m)
    if n_rows == 0:
        assert counts == {"n_held": 0, "n_disputed": 0, "n_conflict": 0, "first_diff": gc.NONE,
                          "n_visible": [0] * 8, "n_behind": [0] * 8, "n_sole": [0] * 8}


@pytest.mark.parametrize("n_rows", [1, 64, gc.T + 1, 3 * gc.T + 17])
def test_two_members_are_the_pairwise_diff(n_rows):
    pairs = [[tc.dense(r, n_rows) for r in dc.gen_diff_pair(n_rows, 31 + n_rows)], dense_group(n_rows, 2, 32 + n_rows)]
    for a, b in pairs:
        flags, d = dc.model_diff(a, b, n_rows)
        behind, hold, conflict, c = gc.model_group([a, b], n_rows)
        assert np.array_equal((behind >> 1) & 1, flags & dc.A_AHEAD)                  # b is behind: a is ahead
        assert np.array_equal(behind & 1, (flags & dc.B_AHEAD) >> 1)
        assert np.array_equal(conflict, (flags & dc.CONFLICT) >> 2)
        assert c["first_diff"] == d["first_diff"] and c["n_conflict"] == d["n_conflict"]
        assert c["n_visible"][:2] == [d["n_visible_a"], d["n_visible_b"]]
        assert c["n_behind"][:2] == [d["n_b_ahead"], d["n_a_ahead"]]
        assert np.array_equal(hold != 0, (a["mod"][:n_rows] >= 0) | (b["mod"][:n_rows] >= 0))


def test_one_member_holds_what_it_sees():
    n = gc.T + 9
    (t,) = dense_group(n, 1, 5)
    behind, hold, conflict, c = gc.model_group([t], n)
    assert not behind.any() and not conflict.any() and np.array_equal(hold, (t["mod"] >= 0).astype(np.uint8))
    assert c["n_sole"][0] == c["n_visible"][0] == c["n_held"] and c["first_diff"] == gc.NONE


@pytest.mark.parametrize("m", [2, 3, 8])
def test_permuting_the_members_permutes_the_bits(m):
    n = gc.T + 9
    tables = dense_group(n, m, 77 + m)
    behind, hold, conflict, c = gc.model_group(tables, n)
    perm = np.random.default_rng(m).permutation(m)               # the new member k is the old member perm[k]
    pb, ph, pconf, pc_ = gc.model_group([tables[j] for j in perm], n)

    def moved(x):
        return sum((((x >> int(old)) & 1) << new) for new, old in enumerate(perm)).astype(np.uint8)

    assert np.array_equal(pb, moved(behind)) and np.array_equal(ph, moved(hold)) and np.array_equal(pconf, conflict)
    for f in ("n_held", "n_disputed", "n_conflict", "first_diff"):
        assert pc_[f] == c[f]
    for f in ("n_visible", "n_behind", "n_sole"):
        assert pc_[f][:m] == [c[f][j] for j in perm]


@pytest.mark.parametrize("m", gc.MEMBERS)
@pytest.mark.parametrize("n_rows", gc.SHAPES)
def test_generator_self_checks(n_rows, m):
    """The seeds of tests/test_gpu_groupdiff.py: every class the member count allows, the planted rows, the share."""
    members = gc.gen_group(n_rows, m, 100 + n_rows + m)
    assert len(members) == m
    if n_rows < gc.PLANT_FROM:
        return
    classes = members[0]["classes"]
    for name, least in {**gc.CLASSES, **gc.RANGES}.items():
        assert (name in classes and len(classes[name]) > 0) == (m >= least), (name, m)
    assert len(classes["planted"]) == 3 * len(gc.COMPARISONS) + 1
    if int(n_rows * gc.SHARE) >= m:                              # every member is singled out by every class
        behind = gc.model_group([tc.dense(r, n_rows) for r in members], n_rows)[0]
        for name in ("one_behind_lt", "one_behind_rank", "negative_mod", "never_written"):
            if name in classes:
                assert set(behind[classes[name]].tolist()) == {1 << j for j in range(m)}, (name, m)


def test_generator_self_checks_large():
    members = gc.gen_group(gc.LARGE, 3, 7)
    assert gc.LARGE > gc.GRID * gc.T and len(members[0]["classes"]["conflict_with_behind"]) > 1000


def test_the_overruled_conflict_clears():
    tables = dense_group(64, 3, 3)
    behind, hold, conflict, _ = gc.model_group(tables, 64)
    k = gc.OVERRULED
    assert tables[0]["val"][k] != tables[1]["val"][k] and (tables[0]["lt"][k], tables[0]["rank"][k]) == \
        (tables[1]["lt"][k], tables[1]["rank"][k])
    assert (behind[k], hold[k], conflict[k]) == (3, 4, 0)
    assert gc.model_group(tables[:2], 64)[2][k] == 1             # without the third member it is one


def test_header_declares_the_call_and_the_abi_stays():
    import ctypes

    from crdt_amd import _capi
    text = open(os.path.join(ROOT, "include", "crdt_merge.h")).read()
    assert re.search(r"#define\s+CRDT_ABI_VERSION\s+5\b", text) and _capi.ABI_VERSION == 5
    assert re.search(r"#define\s+CRDT_GROUP_MAX\s+8\b", text) and _capi.GROUP_MAX == gc.GROUP_MAX == 8
    decl = re.search(r"int crdt_diff_group\(([^;]*)\);", text).group(1)
    assert re.sub(r"\s+", " ", decl) == ("crdt_ctx* const* ctxs, uint32_t n_ctx, uint64_t n_rows, uint8_t* behind_mask, "
                                         "uint8_t* hold_mask, uint8_t* conflict_flags, int32_t flags_mem, "
                                         "crdt_group_diff* out")
    P, U32, U64, I32 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int32
    assert _capi.SIGNATURES["crdt_diff_group"] == (ctypes.c_int, [P, U32, U64, P, P, P, I32, P])
    assert ctypes.sizeof(_capi.CrdtGroupDiff) == 8 * (4 + 3 * 8)
    assert tuple(f for f, _ in _capi.CrdtGroupDiff._fields_) == gc.FIELDS
    assert "crdt_diff_group(ctxs, .., behind_mask, hold_mask, conflict_flags)" in text   # crdt_export_flagged's list
    hip = open(os.path.join(ROOT, "crdt_amd", "csrc", "crdt_merge.hip")).read()
    assert hip.index('#include "table_purge.inc"') < hip.index('#include "table_group.inc"')
