"""Replica groups and the numpy model for the group diff (crdt_diff_group), pure numpy (test helper; nothing here
imports the library).

``gen_group`` starts every member from one ``tests/_table_cases.gen_rows`` table, as converged replicas do, and
perturbs disjoint random subsets of its rows, one subset per way a group can come to differ (``CLASSES``); the
member a class singles out rotates over the members with the row, so that from ``take >= m`` rows on every member
is singled out by every class.  Even members clear one range and odd members another, and the last member is
written only below ``n_rows - n_rows // 32`` (its high-water mark lies under the call's rows).  From 64 rows on it
plants the rows that hold the comparisons a kernel can get wrong (``planted``).  The generator asserts that every
class that the member count allows occurs with the bytes it was built for, and that at least 40 % of the rows are
undisputed and conflict-free.

The budget behind that bound, at the smallest planted shape (64 rows, 8 members): 13 planted rows, 11 disputed
class rows, 2 + 2 cleared rows and 2 rows above the last member's high-water mark are 30 of 64; from 2048 rows on
the classes take 1.5 % of the rows each and the ranges 3/32 together, about a quarter in all.

Member j holds row i visibly iff mod >= 0; hlc = (lt, rank), signed lt then unsigned rank; the holders of a row are
the visible members with the greatest hlc, every other member is behind on a row somebody holds, and the row is a
conflict iff two holders' val differ."""
from __future__ import annotations

import numpy as np

from tests import _table_cases as tc
from tests._cases import ABSENT_MOD, NULL

T = 2048                                  # rows per tile of the pass (table_group.inc: kTmTile)
GRID = 2048                               # its capped grid (kDfGrid)
LARGE = (GRID + 1) * T + 5                # more tiles than workgroups, a partial last tile
GROUP_MAX = 8
SHAPES = (0, 1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 17)
MEMBERS = (1, 2, 3, 8)
NONE = (1 << 64) - 1                      # first_diff when nothing differs
PLANT_FROM = 64
SHARE = 0.015                             # of the rows, per random class
I64_MIN = -(1 << 63)
FIELDS = ("n_held", "n_disputed", "n_conflict", "first_diff", "n_visible", "n_behind", "n_sole")

# the random classes: name -> the fewest members it needs
CLASSES = {"one_behind_lt": 2, "one_behind_rank": 2, "sole_leader": 2, "two_tied_leaders": 3, "all_different": 2,
           "negative_mod": 2, "never_written": 2, "all_invisible": 1, "mod_only": 2, "conflict_with_behind": 3,
           "last_holder_differs": 3, "conflict_repeated": 4, "live_against_tombstone": 2}
RANGES = {"cleared": 2, "above_high_water": 2}     # the classes the ranges make

_X = int(tc.STAMPS[0]) & ~(1 << 31)       # an lt with bit 31 clear; with it set, 32768 ms later
_S5 = int(tc.STAMPS[5])
# (low, high) of the four comparisons, as (lt, rank)
COMPARISONS = (((_X, 2), (_X | (1 << 31), 2)),               # lts that differ only in bit 31
               ((_X | -(1 << 63), 2), (_X, 2)),              # ... only in bit 63: lt is signed
               ((_S5, 0x7FFFFFFF), (_S5, 0x80000000)),       # rank is unsigned
               ((-(5 << 16), 3), (5 << 16, 3)))              # a negative lt against a positive one
OVERRULED = 3 * len(COMPARISONS)          # the id of the conflict between members 0 and 1 that member 2 overrules


def positions(m: int) -> tuple:
    """The first, a middle and the last member."""
    return (0, m // 2, m - 1)


def planted(m: int) -> dict:
    """id -> ([(lt, rank, val, mod) per member], hold byte, conflict)."""
    out = {}
    for c, (low, high) in enumerate(COMPARISONS):
        for p, at in enumerate(positions(m)):
            k = 3 * c + p
            out[k] = ([((high if j == at else low) + (10 + k, _S5)) for j in range(m)], 1 << at, 0)
    rows = [(_S5, 4, 30 + (j == 1), _S5) for j in range(m)]          # members 0 and 1: one hlc, two values
    if m >= 3:
        rows[2] = (_S5 + (1 << 16), 1, 40, _S5)                      # ... and member 2 above both: no conflict
    out[OVERRULED] = (rows, 4 if m >= 3 else (1 << m) - 1, int(m == 2))
    return out


def _rows_of(d: dict, written: np.ndarray, clear) -> dict:
    ids = np.flatnonzero(written).astype(np.uint32)
    return {"n_rows": len(written), "ids": ids, "lt": d["lt"][ids], "rank": d["rank"][ids], "val": d["val"][ids],
            "mod": d["mod"][ids], "clear": clear}


def gen_group(n_rows: int, m: int, seed: int) -> list:
    """The members' rows in tests/_table_cases' form ({ids, lt, rank, val, mod, clear}), member 0 first;
    ``members[0]["classes"]`` maps every class (and "planted") to its row ids."""
    base = tc.gen_rows(n_rows, seed)
    rng = np.random.default_rng(seed + 15485863)
    written = np.zeros(n_rows, bool)
    written[base["ids"]] = True
    d = {k: np.zeros(n_rows, base[k].dtype) for k in ("lt", "rank", "val", "mod")}
    for k in d:
        d[k][base["ids"]] = base[k]
    mem = [{k: v.copy() for k, v in d.items()} for _ in range(m)]
    wr = [written.copy() for _ in range(m)]
    span = n_rows // 32
    clears = [(n_rows // 3, span) if j % 2 == 0 else (2 * n_rows // 3, span) for j in range(m)]
    top = n_rows - span if m > 1 else n_rows                     # the last member is written below it only
    taken = np.zeros(n_rows, bool)
    for first, count in set(clears):
        taken[first:first + count] = True
    taken[top:] = True
    plants = planted(m) if n_rows >= PLANT_FROM else {}
    taken[list(plants)] = True
    free = rng.permutation(np.flatnonzero(written & (d["mod"] >= 0) & ~taken))   # visible in every member so far
    take = max(1, int(n_rows * SHARE))
    classes, hold = {}, {}
    full = (1 << m) - 1
    for name, least in CLASSES.items():
        if m < least:
            continue
        classes[name], free = np.sort(free[:take]), free[take:]
    for name, ids in classes.items():
        want = np.zeros(len(ids), np.int64)
        for r, i in enumerate(ids.tolist()):
            a, b = r % m, (r + 1) % m                            # the members this row singles out
            rows = [mem[j] for j in range(m)]
            if name == "one_behind_lt":
                rows[a]["lt"][i] -= 1 << 16
                want[r] = full & ~(1 << a)
            elif name == "one_behind_rank":
                for j in range(m):
                    rows[j]["rank"][i] += j != a
                want[r] = full & ~(1 << a)
            elif name == "sole_leader":
                rows[a]["lt"][i] += 3 << 16
                want[r] = 1 << a
            elif name == "two_tied_leaders":
                rows[a]["lt"][i] += 2 << 16
                rows[b]["lt"][i] += 2 << 16
                want[r] = (1 << a) | (1 << b)
            elif name == "all_different":
                for j in range(m):
                    rows[j]["lt"][i] += ((j + r) % m) << 16
                want[r] = 1 << ((m - 1 - r) % m)
            elif name == "negative_mod":
                rows[a]["mod"][i] = -1 - (r % 3) * (1 << 20)
                want[r] = full & ~(1 << a)
            elif name == "never_written":
                wr[a][i] = False
                want[r] = full & ~(1 << a)
            elif name == "all_invisible":                        # different garbage under negative mods
                for j in range(m):
                    rows[j]["mod"][i] = -2 - j
                    rows[j]["lt"][i] += (99 * j) << 16
                    rows[j]["val"][i] = 0x12345 + j
            elif name == "mod_only":
                rows[a]["mod"][i] = int(tc.STAMPS[r % tc.N_STAMPS]) + 1
                want[r] = full
            elif name == "conflict_with_behind":                 # a is behind; b and its neighbour disagree
                rows[a]["lt"][i] -= 1 << 16
                rows[b]["val"][i] = rows[(b + 1) % m]["val"][i] ^ 0x40000
                want[r] = (full & ~(1 << a)) | 0x100
            elif name == "last_holder_differs":                  # every member holds the top; only the last differs
                rows[m - 1]["val"][i] ^= 0x40000
                want[r] = full | 0x100
            elif name == "conflict_repeated":                    # ... and where the members after the second repeat it
                for j in range(2, m):
                    rows[j]["val"][i] = rows[0]["val"][i] ^ 0x40000
                want[r] = full | 0x100
            elif name == "live_against_tombstone":
                for j in range(m):
                    rows[j]["val"][i] = NULL if j == a else 7
                want[r] = full | 0x100
        hold[name] = want
    for k, (rows, _, _) in plants.items():
        for j in range(m):
            wr[j][k] = True
            for f, name in enumerate(("lt", "rank", "val", "mod")):
                mem[j][name][k] = rows[j][f]
    if m > 1:
        wr[m - 1][top:] = False
    members = [_rows_of(mem[j], wr[j], clears[j]) for j in range(m)]
    dense = [tc.dense(r, n_rows) for r in members]
    someone = np.zeros(n_rows, bool)
    for x in dense:
        someone |= x["mod"] >= 0
    inside = np.zeros(n_rows, bool)
    for first, count in set(clears):
        inside[first:first + count] = True
    if m >= 2:
        classes["cleared"] = np.flatnonzero(inside & someone)
        classes["above_high_water"] = np.flatnonzero((np.arange(n_rows) >= top) & someone)
    classes["planted"] = np.array(sorted(plants), np.int64)
    if n_rows >= PLANT_FROM:                                     # what every such shape has to show
        behind, hd, conflict, _ = model_group(dense, n_rows)
        assert np.mean((behind == 0) & (conflict == 0)) >= 0.40, (n_rows, m, np.mean((behind == 0) & (conflict == 0)))
        for name, want in hold.items():
            ids = classes[name]
            assert len(ids) > 0, (n_rows, m, name)
            assert np.array_equal(hd[ids], want & 0xFF) and np.array_equal(conflict[ids], want >> 8), (n_rows, m, name)
            assert np.array_equal(behind[ids], np.where(want & 0xFF, full & ~(want & 0xFF), 0)), (n_rows, m, name)
        for name in RANGES:
            if m >= RANGES[name]:
                ids = classes[name]
                assert len(ids) > 0 and np.all(behind[ids] != 0), (n_rows, m, name)
        for k, (_, h, c) in plants.items():
            assert (hd[k], behind[k], conflict[k]) == (h, full & ~h, c), (n_rows, m, k)
    members[0]["classes"] = classes
    return members


def max_lt(members: list) -> int:
    """The largest lt any member holds: a canonical at or above it keeps every recv() quiet."""
    return max([int(r["lt"].max()) for r in members if len(r["lt"])] + [0])


def model_group(tables: list, n_rows: int):
    """(behind bytes, hold bytes, conflict bytes, dict of the crdt_group_diff fields) of the members' dense
    tables ({lt, rank, val, mod} arrays, or an OracleTable's rows)."""
    m = len(tables)
    lt = np.stack([np.asarray(t["lt"][:n_rows], np.int64) for t in tables]) if m else np.zeros((0, n_rows), np.int64)
    rank = np.stack([np.asarray(t["rank"][:n_rows]).astype(np.int64) for t in tables])
    val = np.stack([np.asarray(t["val"][:n_rows]).astype(np.int64) for t in tables])
    vis = np.stack([np.asarray(t["mod"][:n_rows]) >= 0 for t in tables])
    held = vis.any(axis=0)
    top_lt = np.where(vis, lt, I64_MIN).max(axis=0)
    at_lt = vis & (lt == top_lt)
    top_rank = np.where(at_lt, rank, -1).max(axis=0)
    holds = at_lt & (rank == top_rank)
    bits = (1 << np.arange(m, dtype=np.int64))[:, None]
    hold = (holds * bits).sum(axis=0)
    full = (1 << m) - 1
    behind = np.where(held, full & ~hold, 0)
    conflict = held & (np.where(holds, val, 1 << 40).min(axis=0) != np.where(holds, val, -1).max(axis=0))
    nz = np.flatnonzero((behind != 0) | conflict)
    pad = [0] * (GROUP_MAX - m)
    counts = {"n_held": int(held.sum()), "n_disputed": int((behind != 0).sum()), "n_conflict": int(conflict.sum()),
              "first_diff": int(nz[0]) if len(nz) else NONE,
              "n_visible": [int(vis[j].sum()) for j in range(m)] + pad,
              "n_behind": [int(((behind >> j) & 1).sum()) for j in range(m)] + pad,
              "n_sole": [int((hold == (1 << j)).sum()) for j in range(m)] + pad}
    return behind.astype(np.uint8), hold.astype(np.uint8), conflict.astype(np.uint8), counts


def group_definition(maps: list):
    """MapCrdt.groupDiff's definition on ``oracle.crdt_oracle.MapCrdt``s: per key of the union of the maps'
    record_map()s, in first-seen order over the maps: (behind keys per map, sole counts, disputed, conflict keys)."""
    rms = [m.record_map() for m in maps]
    order = list(dict.fromkeys(k for rm in rms for k in rm))
    behind, sole, disputed, conflicts = [[] for _ in maps], [0] * len(maps), 0, []
    for k in order:
        recs = [rm.get(k) for rm in rms]
        top = max(r.hlc for r in recs if r is not None)
        holders = [j for j, r in enumerate(recs) if r is not None and r.hlc == top]
        for j in range(len(maps)):
            if j not in holders:
                behind[j].append(k)
        disputed += len(holders) < len(maps)
        if len(holders) == 1:
            sole[holders[0]] += 1
        if any(recs[a].value != recs[b].value for a in holders for b in holders):
            conflicts.append(k)
    return behind, sole, disputed, conflicts


assert ABSENT_MOD < 0
