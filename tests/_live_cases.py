"""Row sets and the model for the live view on the device table (crdt_tombstone_live, crdt_export_live): pure
numpy plus the C restatement (test helper; nothing here imports the library).

``gen_live`` is a ``tests/_table_cases.gen_rows`` table over ids [0, n_rows] (one row past the call's n_rows).
From 64 rows on it plants the rows a liveness test can get wrong and asserts that every kind of row occurs and
that at least a quarter of [0, n_rows) is live and at least a quarter is not.  A row is visible iff mod >= 0 and
live iff it is visible and its val is not NULL.

The model is the composition the call is held to, on an ``OracleTable``: the live ids of rows [0, n_rows), then
``put_stamped(ids, NULL, wall)``, skipped when there are none."""
from __future__ import annotations

import numpy as np

from tests import _table_cases as tc
from tests._cases import ABSENT_MOD, NULL

T = 2048                                  # rows per tile of the pass (table_live.inc: kTmTile)
GRID = 2048                               # its capped grid (kLvGrid)
LARGE = (GRID + 1) * T + 5                # more tiles than workgroups, a partial last tile
SHAPES = (0, 1, T - 1, T, T + 1, 5 * T + 9)
PLANT_FROM = 64
LOCAL_RANK = 7                            # gen_rows' ranks are 0..5: a stored tombstone shows its rank
_S = [int(s) for s in tc.STAMPS]
C0 = tc.TOP                               # a canonical at the largest stamp
WALL = tc.MERGE_WALL                      # above every stamp's millis: Hlc.send moves the clock to it
DRIFT_WALL = (C0 >> 16) - 60001           # the canonical's millis is 60001 ms ahead of it: Hlc.send raises drift


def planted(n_rows: int) -> dict:
    """id -> ((lt, rank, val, mod), live) of the planted rows."""
    return {
        0: ((_S[3], 2, 100, _S[4]), True),                       # live, the first row
        1: ((_S[5], 1, NULL, _S[6]), False),                     # a tombstone
        2: ((_S[7], 3, 101, -5), False),                         # invisible with a live-looking val
        3: ((_S[8], 4, NULL, -(1 << 40)), False),                # invisible and NULL
        4: ((_S[9], 5, 102, 0), True),                           # a mod of exactly 0 is visible
        5: ((-(9 << 16), 0, 103, 1), True),                      # a negative lt under a visible mod
        n_rows - 1: ((_S[10], 0, 104, _S[11]), True),            # live, the last row
        n_rows: ((_S[12], 2, 105, _S[13]), True),                # live, but past n_rows: it survives
    }


def gen_live(n_rows: int, seed: int) -> dict:
    """Rows in tests/_table_cases' form over ids [0, n_rows]; ``rows["n_rows"]`` is the call's n_rows."""
    rows = tc.gen_rows(n_rows, seed)
    if n_rows < PLANT_FROM:
        return rows
    plan = planted(n_rows)
    tc._plant(rows, {k: v for k, (v, _) in plan.items()})
    d = tc.dense(rows, n_rows + 1)
    live = live_mask(d, n_rows + 1)
    for k, (_, want) in plan.items():
        assert bool(live[k]) is want, (n_rows, seed, k)
    inside, vis = live[:n_rows], d["mod"][:n_rows] >= 0
    written = np.zeros(n_rows + 1, bool)
    written[rows["ids"]] = True
    first, count = rows["clear"]
    cleared = np.zeros(n_rows, bool)
    cleared[first:first + count] = True
    assert count > 0 and not inside[cleared].any() and written[:n_rows][cleared].any(), (n_rows, seed, "cleared")
    assert np.any(~written[:n_rows] & ~cleared), (n_rows, seed, "never written")
    assert np.any(vis & (d["val"][:n_rows] == NULL)), (n_rows, seed, "tombstones")
    assert np.any(~vis & written[:n_rows] & ~cleared & (d["val"][:n_rows] != NULL)), (n_rows, seed, "invisible, live val")
    assert np.any(~vis & written[:n_rows] & ~cleared & (d["val"][:n_rows] == NULL)), (n_rows, seed, "invisible, NULL")
    assert np.any(inside & (d["mod"][:n_rows] == 0)), (n_rows, seed, "mod == 0")
    assert inside.mean() >= 0.25 and (~inside).mean() >= 0.25, (n_rows, seed, inside.mean())
    return rows


def gen_dead(n_rows: int, seed: int) -> dict:
    """The same kinds of rows with no live one: every visible row is a tombstone."""
    rows = tc.gen_rows(n_rows, seed)
    rows["val"] = np.where(rows["mod"] >= 0, NULL, rows["val"]).astype(np.uint32)
    return rows


def live_mask(rows, n_rows: int) -> np.ndarray:
    """Which of rows [0, n_rows) are live; ``rows``: dense columns or an OracleTable's structured rows."""
    return (np.asarray(rows["mod"][:n_rows]) >= 0) & (np.asarray(rows["val"][:n_rows]) != NULL)


def model_tombstone(o, n_rows: int, wall: int):
    """The composition on an OracleTable (which it updates); returns (result dict, flag bytes by ROW id)."""
    ids = np.flatnonzero(live_mask(o.rows, n_rows)).astype(np.uint32)
    flags = np.zeros(n_rows, np.uint8)
    if len(ids) == 0:
        return dict(tc.CLEARED, canonical_lt=o.canonical), flags
    res = o.put_stamped(ids, np.full(len(ids), NULL, np.uint32), wall).as_dict()
    if res["status"] == 0:
        flags[ids] = 1
    return res, flags


def model_live(rows, n_rows: int) -> dict:
    """The columns crdt_export_live gives for rows [0, n_rows)."""
    ids = np.flatnonzero(live_mask(rows, n_rows)).astype(np.uint32)
    return {"key": ids, **{k: np.asarray(rows[k][:n_rows])[ids] for k in ("lt", "rank", "val", "mod")}}


assert ABSENT_MOD < 0 and 0x80808080 != NULL      # the never-written fill: invisible, its val not NULL
