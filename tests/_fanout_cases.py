"""The table fan-out (crdt_fanout_tables) as a numpy model of its contract, pure numpy plus the C oracle
(test helper).

    for j in 0 .. N-1:
        s_j = dsts[j].merge(src.recordMap(modifiedSince: sinces[j]))
        if s_j raised: stop

``oracle_fanout`` is that loop on OracleTable objects (every value a GPU test compares comes from it).
``model`` runs the merges on dense columns and reports what the tests need to know about a case before they
trust it: per destination its selection, winners, stamp R_j, send status, whether a selected row may raise in
ITS recv() (against its canonical and rank, the kernels' conservative rule) and whether a selected id lies
outside IT — and from those whether the library's fused form runs.

Cases: the source ``tc.gen_rows(n, 6000 + n, clear_at=1/3)``, destination j ``tc.gen_rows(n, 6000 + n + 7919 +
101 j, clear_at=(j % 3 + 1) / 4)`` with local rank 7 + j (the source's ranks are 0..5), the wall MERGE_WALL, and
two canonical settings: "top" = TOP + 1 + j (every R_j is the destination's own, distinct canonical: a row
stamped with another destination's R is caught) and "mid" = canon0() + j (some selected lts lie above it)."""
from __future__ import annotations

import numpy as np

from tests import _fanin_cases as fc
from tests import _sync_cases as sc
from tests import _table_cases as tc

I64_MIN = tc.I64_MIN
FANOUT_MAX = 8
SHAPES_T = sc.SHAPES_T
COLS = ("lt", "rank", "val", "mod")
CANON_SETTINGS = ("top", "mid")
SRC_RANK = 6                                         # the source table's own local rank (its rows' ranks are 0..5)


def shapes():
    return sc.shapes()


def source_rows(n: int) -> dict:
    return tc.gen_rows(n, 6000 + n, clear_at=1 / 3)


def dst_rows(n: int, j: int) -> dict:
    return tc.gen_rows(n, 6000 + n + 7919 + 101 * j, clear_at=(j % 3 + 1) / 4)


def dst_rank(j: int) -> int:
    return 7 + j


def canonical(setting: str, j: int) -> int:
    return tc.TOP + 1 + j if setting == "top" else sc.canon0() + j


def strides(n_dst: int, flip: bool = False):
    """(the source's stride, the destinations'): 24 / 32 alternating across the destinations, the source's the
    other way round from destination 0's."""
    first = 32 if flip else 24
    return 56 - first, [first if j % 2 == 0 else 56 - first for j in range(n_dst)]


since_vectors = fc.since_vectors                     # all 0, all mid, all I64_MIN, mixed (an empty selection, a -1)


def oracle_fanout(osrc, odsts, n_rows, sinces, wall):
    """crdt_fanout_tables' contract on the oracle: (results, mask, index of the step that stopped the sequence
    or None).  A destination after the stop is untouched and reports its own canonical."""
    results, mask, stop = [], np.zeros(n_rows, np.uint8), None
    for j, (odst, since) in enumerate(zip(odsts, sinces)):
        if stop is not None:
            results.append(dict(tc.CLEARED, canonical_lt=odst.canonical))
            continue
        res, flags, _ = tc.oracle_merge_table(odst, osrc, n_rows, since, wall)
        results.append(res)
        mask |= (flags << j).astype(np.uint8)
        if res["status"] != 0:
            stop = j
    return results, mask, stop


def _padded(d: dict, n: int) -> dict:
    cur = {k: d[k][:n].copy() for k in COLS}
    if len(cur["lt"]) < n:                           # a smaller destination: the rows it lacks count as never written
        empty = {"ids": np.zeros(0, np.uint32), "clear": (0, 0), **{k: np.zeros(0, cur[k].dtype) for k in COLS}}
        fill = tc.dense(empty, n - len(cur["lt"]))
        cur = {k: np.concatenate([cur[k], fill[k]]) for k in COLS}
    return cur


def model(src: dict, dsts: list, n: int, sinces: list, canons: list, wall: int, ranks: list | None = None,
          caps: list | None = None) -> dict:
    """The merges on dense columns {lt, rank, val, mod} (first n rows of each); the destinations are independent,
    so every one is computed, whatever an earlier one's send() does.  Exact only where no recv() raises and no
    selected id lies outside its destination; the tests use it for the plan and for what a case contains, the C
    oracle for every compared value."""
    ranks = [dst_rank(j) for j in range(len(dsts))] if ranks is None else ranks
    s = {k: src[k][:n] for k in COLS}
    out = {k: [] for k in ("sel", "wins", "stamps", "statuses", "canonical", "n_present", "may_raise",
                           "out_of_range", "rows")}
    mask = np.zeros(n, np.uint8)
    for j, (d, since, c, rank) in enumerate(zip(dsts, sinces, canons, ranks)):
        cur = _padded(d, n)
        sel = ~(s["mod"] < since)
        vis = cur["mod"] >= 0
        win = sel & (~vis | sc._newer(s, cur))
        r = max(c, int(s["lt"][sel].max())) if sel.any() else c
        st, c_after = sc.send(r, wall)
        for k in ("lt", "rank", "val"):
            cur[k] = np.where(win, s[k], cur[k])
        cur["mod"] = np.where(win, np.int64(r), cur["mod"])
        mask |= (win.astype(np.uint8) << j).astype(np.uint8)
        out["sel"].append(sel)
        out["wins"].append(win)
        out["stamps"].append(r)
        out["statuses"].append(st)
        out["canonical"].append(c_after)
        out["n_present"].append(int((sel & vis).sum()))
        out["may_raise"].append(sc._may_raise(s["lt"], s["rank"], sel, c, rank, wall))
        out["out_of_range"].append(bool(caps is not None and sel.any() and int(np.flatnonzero(sel).max()) >= caps[j]))
        out["rows"].append(cur)
    out["mask"] = mask
    out["fused"] = not (any(out["may_raise"]) or any(out["out_of_range"]) or any(out["statuses"]))
    return out


def case(n: int, n_dst: int):
    """(the source's dense columns, the destinations' dense columns) of the generated case, at capacity
    max(n, 16)."""
    cap = max(n, 16)
    return tc.dense(source_rows(n), cap), [tc.dense(dst_rows(n, j), cap) for j in range(n_dst)]


def nested_patterns(T: int, n_rows: int) -> dict:
    """Tile patterns over 5T+9 rows: name -> one selection per destination, NESTED (selection j + 1 is a subset
    of selection j, as the rows with !(mod < since_j) are for growing since_j).  ``nested_mods`` turns them into
    the source's mods and the sinces that select them."""
    z = lambda: np.zeros(n_rows, bool)  # noqa: E731
    out = {}
    extra = [z() for _ in range(4)]                  # each destination's extra rows in a tile of its own; tile 4 empty
    for j, s in enumerate(extra):
        s[j * T + 5 + 40 * j:j * T + 300] = True
    out["own_tiles"] = [np.logical_or.reduce(extra[j:]) for j in range(4)]
    extra = [z() for _ in range(3)]                  # all in one tile
    extra[0][2 * T + 10:2 * T + 500:3] = True
    extra[1][2 * T + 11:2 * T + 900:2] = True
    extra[2][2 * T + 12:2 * T + 700:5] = True
    for j in (1, 2):                                 # (disjoint extras: a row belongs to the deepest level that has it)
        for k in range(j):
            extra[k] &= ~extra[j]
    out["same_tile"] = [np.logical_or.reduce(extra[j:]) for j in range(3)]
    run, ends = z(), z()                             # a run across a tile boundary, and tile ends inside and outside it
    run[2 * T - 300:2 * T + 500] = True
    ends[2 * T - 1] = ends[2 * T] = ends[4 * T - 1] = ends[5 * T + 8] = True
    out["run_across_boundary"] = [run | ends, ends]
    out["none"] = [z() for _ in range(3)]
    return out


def nested_mods(sels: list, stamps: np.ndarray):
    """(the source's mod column, the sinces): level = how many of the nested selections hold the row; mod =
    stamps[level], since_j = stamps[j + 1], so !(mod < since_j) is exactly selection j."""
    level = np.zeros(len(sels[0]), np.int64)
    for j, s in enumerate(sels):
        assert j == 0 or not (s & ~sels[j - 1]).any(), "the selections are nested"
        level += s
    st = np.sort(np.asarray(stamps, np.int64))[:len(sels) + 1]
    assert len(set(st.tolist())) == len(sels) + 1
    return st[level], [int(st[j + 1]) for j in range(len(sels))]
