"""Replica groups and the model for tombstone collection on the device tables (crdt_purge_tombstones): pure numpy
plus the C restatement's table type (test helper; nothing here imports the library).

``gen_group`` makes the members of one group as ``tests/_table_cases.gen_rows`` tables over ids [0, n_rows] (one
row past the call's n_rows).  The members start as copies of one table, as converged replicas do; a share of the
visible rows is forced to tombstones whose lt lies on both sides of ``BEFORE``; then every member j > 0 is
perturbed on planted and on random rows, and the odd members clear another range than member 0.  From 64 rows on
the generator asserts that every kind of row a purge can get wrong occurs (``KINDS``) and that the purged rows
and the blocked candidates are each at least 1/8 of the rows.

Member j holds row i visibly iff mod >= 0 and as a tombstone iff, besides, its val is NULL.  Row i is a candidate
iff member 0 holds a tombstone with lt < before, and purged iff, besides, every member holds a tombstone of member
0's (lt, rank).  The model sets the purged rows of every member's ``OracleTable`` to the never-written row."""
from __future__ import annotations

import numpy as np

from oracle.oracle_c import new_table
from tests import _table_cases as tc
from tests._cases import ABSENT_MOD, NULL

T = 2048                                  # rows per tile of the pass (table_purge.inc: kTmTile)
GRID = 2048                               # its capped grid (kPgGrid)
LARGE = (GRID + 1) * T + 5                # more tiles than workgroups, a partial last tile
SHAPES = (0, 1, T - 1, T, T + 1, 5 * T + 9)
MEMBERS = (1, 2, 3, 8)
PLANT_FROM = 64
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
_S = np.sort(tc.STAMPS)
BEFORE = int(_S[tc.N_STAMPS // 2])        # stamps on both sides of it
_LOW = [int(s) for s in _S[:tc.N_STAMPS // 2]]
NEG_LT = -(9 << 16)
KINDS = ("live_higher", "other_rank", "mod_negative", "never_written", "cleared", "live_value", "mod_differs",
         "lt_at_before", "lt_below_before", "negative_lt", "member0_invisible", "at_n_rows", "first_last")


def masks(cols: list, n_rows: int, before: int):
    """(candidate, purged) of rows [0, n_rows); ``cols``: per member, dense columns or an OracleTable's rows."""
    c0 = {k: np.asarray(cols[0][k][:n_rows]) for k in ("lt", "rank", "val", "mod")}
    cand = (c0["mod"] >= 0) & (c0["val"] == NULL) & (c0["lt"] < before)
    purged = cand.copy()
    for c in cols[1:]:
        purged &= (np.asarray(c["mod"][:n_rows]) >= 0) & (np.asarray(c["val"][:n_rows]) == NULL) & \
                  (np.asarray(c["lt"][:n_rows]) == c0["lt"]) & (np.asarray(c["rank"][:n_rows]) == c0["rank"])
    return cand, purged


def _copy(rows: dict) -> dict:
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in rows.items()}


def _planted(n_rows: int, before: int):
    """(id -> row of every member, id -> row of the LAST member where it differs; None: never written)."""
    lo, lo2 = _LOW[3], _LOW[5]
    tomb = lambda lt, rank=2, mod=_LOW[7]: (lt, rank, NULL, mod)  # noqa: E731
    every = {
        0: tomb(lo), 1: tomb(lo), 2: tomb(lo, 3), 3: tomb(lo2), 4: tomb(lo2, 1), 5: tomb(lo), 6: tomb(lo2, 4),
        7: tomb(before, 0), 8: tomb(before - 1, 0), 9: tomb(NEG_LT, 5), 10: tomb(lo, 1),
        n_rows - 1: tomb(lo2, 0), n_rows: tomb(lo, 2),
    }
    last = {
        1: (lo + (1 << 16), 2, 11, int(tc.TOP)),                 # live with a higher Hlc
        2: tomb(lo, 4),                                          # same lt, other rank
        3: tomb(lo2, 2, -3),                                     # same Hlc, but mod < 0
        4: None,                                                 # never written
        5: (lo, 2, 12, _LOW[7]),                                 # same Hlc with a live value
        6: tomb(lo2, 4, int(tc.TOP)),                            # agreed, another mod: it purges
    }
    first = {10: (lo, 1, NULL, -(1 << 40))}                      # member 0 invisible with a NULL val
    return every, last, first


def gen_group(n_rows: int, n_members: int, seed: int, before: int = BEFORE, agree: float = 0.6) -> list:
    """The members' rows in tests/_table_cases' form over ids [0, n_rows]; member 0 first."""
    rng = np.random.default_rng(seed)
    base = tc.gen_rows(n_rows, seed, clear_at=1 / 3)
    vis = np.flatnonzero(base["mod"] >= 0)
    force = vis[rng.random(len(vis)) < 0.7]
    base["val"][force] = NULL
    pool = np.array(_LOW * 2 + [int(s) for s in _S[tc.N_STAMPS // 2:]] + [before - 1, NEG_LT], np.int64)
    base["lt"][force] = pool[rng.integers(0, len(pool), len(force))]
    if n_rows >= PLANT_FROM:
        every, last, first = _planted(n_rows, before)
        tc._plant(base, every)
    members = []
    for j in range(n_members):
        m = _copy(base)
        if j % 2 == 1:
            m["clear"] = (int(n_rows * 2 / 3), n_rows // 10)
        members.append(m)
    cand0 = masks([tc.dense(base, n_rows + 1)], n_rows, before)[0]
    cand_ids = np.flatnonzero(cand0)
    if n_rows >= PLANT_FROM:
        cand_ids = cand_ids[~np.isin(cand_ids, list(every))]     # (the planted rows are perturbed as planned only)
    cand_pos = np.searchsorted(base["ids"], cand_ids)
    p = 1 - agree ** (1 / max(n_members - 1, 1))
    for j in range(1, n_members):
        m = members[j]
        pos = cand_pos[rng.random(len(cand_pos)) < p]
        kind = rng.integers(0, 6, len(pos))
        a, b, c, d, e, f = (pos[kind == k] for k in range(6))
        m["lt"][a] += 1 << 16
        m["val"][a] = 5
        m["mod"][a] = int(tc.TOP)
        m["rank"][b] = (m["rank"][b] + 1) % 6
        m["mod"][c] = -3
        m["val"][e] = 7
        m["mod"][f] = int(tc.TOP) - 1                            # (another stamp: the row still purges)
        keep = np.ones(len(m["ids"]), bool)
        keep[d] = False                                          # never written here
        for k in ("ids", "lt", "rank", "val", "mod"):
            m[k] = m[k][keep]
    if n_rows >= PLANT_FROM:
        if n_members > 1:
            m = members[-1]
            tc._plant(m, {k: v for k, v in last.items() if v is not None})
            keep = ~np.isin(m["ids"], [k for k, v in last.items() if v is None])
            for k in ("ids", "lt", "rank", "val", "mod"):
                m[k] = m[k][keep]
        if n_members > 1:
            tc._plant(members[0], first)
        self_check(members, n_rows, before)
    return members


def self_check(members: list, n_rows: int, before: int) -> dict:
    """Asserts that every kind of KINDS occurs in the group; returns the rows counted per kind."""
    n = len(members)
    d = [tc.dense(m, n_rows + 1) for m in members]
    cand, purged = masks(d, n_rows, before)
    d0 = {k: v[:n_rows] for k, v in d[0].items()}
    tomb0 = (d0["mod"] >= 0) & (d0["val"] == NULL)
    got = {k: 0 for k in KINDS}
    got["lt_at_before"] = int(np.count_nonzero(tomb0 & (d0["lt"] == before) & ~purged))
    got["lt_below_before"] = int(np.count_nonzero(purged & (d0["lt"] == before - 1)))
    got["negative_lt"] = int(np.count_nonzero(purged & (d0["lt"] < 0)))
    both = masks([{k: v[:n_rows + 1] for k, v in x.items()} for x in d], n_rows + 1, before)[1]
    got["at_n_rows"] = int(both[n_rows])
    got["first_last"] = int(purged[0] and purged[n_rows - 1])
    for j in range(1, n):
        dj = {k: v[:n_rows] for k, v in d[j].items()}
        written = np.zeros(n_rows + 1, bool)
        written[members[j]["ids"]] = True
        first, count = members[j]["clear"]
        cleared = np.zeros(n_rows, bool)
        cleared[first:first + count] = True
        visj = dj["mod"] >= 0
        same = (dj["lt"] == d0["lt"]) & (dj["rank"] == d0["rank"])
        got["live_higher"] += int(np.count_nonzero(cand & visj & (dj["val"] != NULL) & (dj["lt"] > d0["lt"])))
        got["other_rank"] += int(np.count_nonzero(cand & visj & (dj["val"] == NULL) & (dj["lt"] == d0["lt"]) & ~same))
        got["mod_negative"] += int(np.count_nonzero(cand & ~visj & same & written[:n_rows] & ~cleared))
        got["never_written"] += int(np.count_nonzero(cand & ~written[:n_rows] & ~cleared))
        got["cleared"] += int(np.count_nonzero(cand & written[:n_rows] & cleared))
        got["live_value"] += int(np.count_nonzero(cand & visj & same & (dj["val"] != NULL)))
        got["mod_differs"] += int(np.count_nonzero(purged & (dj["mod"] != d0["mod"])))
        got["member0_invisible"] += int(np.count_nonzero(~(d0["mod"] >= 0) & (d0["val"] == NULL) & visj & same &
                                                         (dj["val"] == NULL)))
    alone = ("lt_at_before", "lt_below_before", "negative_lt", "at_n_rows", "first_last")
    for k in (alone if n == 1 else KINDS):
        assert got[k] > 0, (n_rows, n, k, got)
    assert purged.mean() >= 1 / 8, (n_rows, n, purged.mean())
    if n > 1:
        assert (cand & ~purged).mean() >= 1 / 8, (n_rows, n, (cand & ~purged).mean())
    else:
        assert np.array_equal(cand, purged)
    return got


def gen_agreed(n_rows: int, n_members: int, seed: int) -> list:
    """Every member a copy of one table: every candidate is agreed."""
    base = gen_group(n_rows, 1, seed)[0]
    return [_copy(base) for _ in range(n_members)]


def gen_blocked(n_rows: int, n_members: int, seed: int) -> list:
    """Copies of one table whose LAST member holds every row of [0, n_rows) under another rank: all blocked."""
    members = gen_agreed(n_rows, n_members, seed)
    members[-1]["rank"] = (members[-1]["rank"] + 1).astype(np.uint32)
    return members


def gen_no_tombstone(n_rows: int, n_members: int, seed: int) -> list:
    """Copies of one table without a visible tombstone."""
    base = tc.gen_rows(n_rows, seed)
    base["val"] = np.where((base["mod"] >= 0) & (base["val"] == NULL), 9, base["val"]).astype(np.uint32)
    return [_copy(base) for _ in range(n_members)]


def model_purge(tables: list, n_rows: int, before: int):
    """The contract on the members' OracleTables (which it updates): the intersection, then the never-written
    row over each purged id of every member.  Returns ({"n_candidates", "n_purged"}, flag bytes by ROW id)."""
    cand, purged = masks([o.rows for o in tables], n_rows, before)
    ids = np.flatnonzero(purged)
    for o in tables:
        o.rows[ids] = new_table(1)[0]
    return {"n_candidates": int(cand.sum()), "n_purged": int(purged.sum())}, purged.astype(np.uint8)


def purge_definition(maps: list, before_lt: int | None = None) -> list:
    """MapCrdt.purgeDeleted's definition on ``oracle.crdt_oracle.MapCrdt``s (maps[0] is self): the keys every map
    holds in its record_map() as a deleted record of maps[0]'s Hlc, that Hlc's logical time below ``before_lt``,
    are deleted from every map's storage.  Returns them in maps[0]'s order; no event, no clock."""
    rms = [m.record_map() for m in maps]
    purged = []
    for k, r in rms[0].items():
        if not r.is_deleted or (before_lt is not None and not r.hlc.logical_time < before_lt):
            continue
        if all(k in rm and rm[k].is_deleted and rm[k].hlc == r.hlc for rm in rms[1:]):
            purged.append(k)
    for m in maps:
        for k in purged:
            del m._map[k]
    return purged


assert ABSENT_MOD < 0 and 0x80808080 != NULL     # the never-written fill: invisible, its val not NULL
