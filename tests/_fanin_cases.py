"""The table fan-in (crdt_fanin_tables) as a numpy model of its contract, pure numpy (test helper).

    for j in 0 .. N-1:
        s_j = dst.merge(srcs[j].recordMap(modifiedSince: sinces[j]))
        if s_j raised: stop

``model`` runs that sequence on dense columns and reports what the tests need to know about a case before
they trust it: each step's winners, the mask (bit j where step j stored the row), the stamps R_j, the send
statuses, whether a selected row may raise in a recv() (against C_0, the kernels' conservative rule), whether
a selected id lies outside dst — and from those whether the library's fused form runs.

Cases: source j = ``tc.gen_rows(n, 5000 + n + 101 j, clear_at=(j % 3 + 1) / 4)``, the destination
``tc.gen_rows(n, 5000 + n + 7919, clear_at=2 / 3)``, dst's local rank 7, C_0 = canon0(), the wall MERGE_WALL."""
from __future__ import annotations

import numpy as np

from tests import _sync_cases as sc
from tests import _table_cases as tc

I64_MIN = tc.I64_MIN
DST_RANK = tc.DST_RANK
FANIN_MAX = 8
SHAPES_T = sc.SHAPES_T
COLS = ("lt", "rank", "val", "mod")


def shapes():
    return sc.shapes()


def source_rows(n: int, j: int) -> dict:
    return tc.gen_rows(n, 5000 + n + 101 * j, clear_at=(j % 3 + 1) / 4)


def dst_rows(n: int) -> dict:
    return tc.gen_rows(n, 5000 + n + 7919, clear_at=2 / 3)


def since_vectors(n_src: int):
    """name -> the sinces of the sources: all 0, all mid, all I64_MIN, and a mixed one with an empty selection
    in the middle (TOP + 1) and a -1."""
    mixed = [0, sc.mid(), I64_MIN, tc.TOP, 0, sc.mid(), 0, I64_MIN][:n_src]
    mixed[n_src // 2 if n_src > 2 else 0] = tc.TOP + 1
    mixed[-1] = -1
    return {"zero": [0] * n_src, "mid": [sc.mid()] * n_src, "min": [I64_MIN] * n_src, "mixed": mixed}


def model(dst: dict, srcs: list, n: int, sinces: list, c0: int, wall: int, dst_rank: int = DST_RANK,
          dst_cap: int | None = None) -> dict:
    """The sequence on dense columns {lt, rank, val, mod} (first n rows of each).  Exact only where no
    recv() raises and no selected id lies outside dst; the tests use it for the plan and for what a case
    contains, the C oracle for every compared value.  Steps after a send() that raises are not run."""
    cur = {k: dst[k][:n].copy() for k in COLS}
    if len(cur["lt"]) < n:                           # a smaller dst: the rows it lacks count as never written
        fill = tc.dense({"ids": np.zeros(0, np.uint32), "clear": (0, 0), **{k: np.zeros(0, cur[k].dtype) for k in COLS}},
                        n - len(cur["lt"]))
        cur = {k: np.concatenate([cur[k], fill[k]]) for k in COLS}
    wins, stamps, statuses, present = [], [], [], []
    mask = np.zeros(n, np.uint8)
    stores = np.zeros(n, np.int64)
    may_raise = out_of_range = False
    c = c0
    # what the clock passes see: every source's selection, known before anything is stored
    for s, since in zip(srcs, sinces):
        sel = ~(s["mod"][:n] < since)
        may_raise |= sc._may_raise(s["lt"][:n], s["rank"][:n], sel, c0, dst_rank, wall)
        if dst_cap is not None and sel.any():
            out_of_range |= int(np.flatnonzero(sel).max()) >= dst_cap
    for j, (s, since) in enumerate(zip(srcs, sinces)):
        s = {k: s[k][:n] for k in COLS}
        sel = ~(s["mod"] < since)
        vis = cur["mod"] >= 0
        win = sel & (~vis | sc._newer(s, cur))
        r = max(c, int(s["lt"][sel].max())) if sel.any() else c
        st, c = sc.send(r, wall)
        for k in ("lt", "rank", "val"):
            cur[k] = np.where(win, s[k], cur[k])
        cur["mod"] = np.where(win, np.int64(r), cur["mod"])
        mask |= (win.astype(np.uint8) << j).astype(np.uint8)
        stores += win
        wins.append(win)
        stamps.append(r)
        statuses.append(st)
        present.append(int((sel & vis).sum()))
        if st != 0:
            break
    return {"wins": wins, "mask": mask, "stamps": stamps, "statuses": statuses, "n_present": present,
            "stores": stores, "canonical": c, "rows": cur, "may_raise": bool(may_raise),
            "out_of_range": bool(out_of_range),
            "fused": not (may_raise or out_of_range or any(statuses))}


def case(n: int, n_src: int):
    """(dst's dense columns, the sources' dense columns) of the generated case, at capacity max(n, 16)."""
    cap = max(n, 16)
    return tc.dense(dst_rows(n), cap), [tc.dense(source_rows(n, j), cap) for j in range(n_src)]


def tile_patterns(T: int, n_rows: int) -> dict:
    """Tile-skipping patterns over 5T+9 rows: name -> one selection per source."""
    z = lambda: np.zeros(n_rows, bool)  # noqa: E731
    out = {}
    own = [z() for _ in range(4)]                    # each source selects in a tile of its own; tile 4 is empty
    for j, s in enumerate(own):
        s[j * T + 5 + 40 * j:j * T + 300] = True
    out["own_tiles"] = own
    same = [z() for _ in range(3)]                   # several sources select in one tile
    same[0][2 * T + 10:2 * T + 500:3] = True
    same[1][2 * T + 11:2 * T + 900:2] = True
    same[2][2 * T + 12:2 * T + 700:5] = True
    out["same_tile"] = same
    run = [z() for _ in range(2)]                    # a run across a tile boundary, tile ends
    run[0][2 * T - 300:2 * T + 500] = True
    run[1][2 * T - 1] = run[1][2 * T] = run[1][4 * T - 1] = run[1][5 * T + 8] = True
    out["run_across_boundary"] = run
    out["none"] = [z() for _ in range(3)]
    return out
