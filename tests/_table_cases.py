"""Row sets for the table-to-table merge tests (crdt_merge_table), pure numpy (test helper).

A source and a destination replica are generated independently over one id space: mods and lts
come from a small shared stamp set, so ties on lt (and on (lt, rank)) are frequent; ~20 % of the
rows are tombstones, ~10 % are never written, ~5 % carry a negative mod, and a range is cleared.
The source's ranks are 0..5 and the destination's local rank is 7, and the wall clock lies just
above the stamps: no selected row can raise in recv() (hlc.dart:85-94), so the fused form runs.

From 63 rows on, rows 0..3 are planted (with the highest stamp as the source's mod, so every
``since`` up to it selects them) to hold the four decisions a merge has to get right:
  row 0  equal (lt, rank) on both sides          -> keeps local
  row 1  equal lt, the source's rank greater     -> the source wins
  row 2  an OLDER source row, dst's row invisible -> the source wins
  row 3  a newer source tombstone                -> the tombstone wins
``decisions`` computes, from the rows alone, which of the four a case contains."""
from __future__ import annotations

import numpy as np

from tests._cases import ABSENT_MOD, NULL, WALL

I64_MIN = -(1 << 63)
N_STAMPS = 40
STAMPS = ((WALL + 7 * np.arange(N_STAMPS, dtype=np.int64)) << 16) + np.arange(N_STAMPS, dtype=np.int64) % 5
TOP = int(STAMPS.max())
MERGE_WALL = WALL + 300                   # above every stamp's millis: no drift, and send() moves the clock to it
DST_RANK = 7
PLANT_FROM = 63                           # the smallest table the four planted rows go into


def sinces():
    s = np.sort(STAMPS)
    return [0, int(s[0]), int(s[len(s) // 2]), int(s[-1]), int(s[-1]) + 1, -1, I64_MIN]


def gen_rows(n_rows: int, seed: int, clear_at: float = 1 / 3) -> dict:
    """Columns of the written rows of one replica and the range cleared after they are put."""
    rng = np.random.default_rng(seed)
    ids = np.flatnonzero(rng.random(n_rows) >= 0.10).astype(np.uint32)
    n = len(ids)
    mod = STAMPS[rng.integers(0, N_STAMPS, n)]
    neg = rng.random(n) < 0.05
    mod[neg] = -(1 << 20) - rng.integers(0, 1000, int(neg.sum()))
    lt = STAMPS[rng.integers(0, N_STAMPS, n)]
    rank = rng.integers(0, 6, n).astype(np.uint32)
    val = rng.integers(0, 1 << 20, n).astype(np.uint32)
    val[rng.random(n) < 0.20] = NULL
    return {"n_rows": n_rows, "ids": ids, "lt": lt.astype(np.int64), "rank": rank, "val": val,
            "mod": mod.astype(np.int64), "clear": (int(n_rows * clear_at), n_rows // 10)}


def _plant(rows: dict, planted: dict):
    """Replace / add the rows of ``planted`` ({id: (lt, rank, val, mod)}); none lies in the cleared range."""
    keep = ~np.isin(rows["ids"], np.fromiter(planted, np.uint32))
    ids = np.concatenate([np.fromiter(planted, np.uint32), rows["ids"][keep]])
    order = np.argsort(ids, kind="stable")
    cols = {"ids": ids[order]}
    for j, name in enumerate(("lt", "rank", "val", "mod")):
        head = np.array([p[j] for p in planted.values()], rows[name].dtype)
        cols[name] = np.concatenate([head, rows[name][keep]])[order]
    rows.update(cols)
    first, count = rows["clear"]
    assert not any(first <= k < first + count for k in planted)


def gen_pair(n_rows: int, seed: int) -> tuple[dict, dict]:
    """(source rows, destination rows) over ids [0, n_rows)."""
    src = gen_rows(n_rows, seed, clear_at=1 / 3)
    dst = gen_rows(n_rows, seed + 7919, clear_at=2 / 3)
    if n_rows >= PLANT_FROM:
        s10, s20, s30 = int(STAMPS[10]), int(STAMPS[20]), int(STAMPS[30])
        _plant(src, {0: (s20, 3, 11, TOP), 1: (s20, 4, 12, TOP), 2: (s10, 2, 13, TOP), 3: (s30, 1, NULL, TOP)})
        _plant(dst, {0: (s20, 3, 21, s20), 1: (s20, 2, 22, s20), 2: (s30, 5, 23, -(1 << 20)), 3: (s20, 5, 24, s20)})
    return src, dst


def dense(rows: dict, capacity: int) -> dict:
    """The table the rows make, as dense columns of ``capacity`` rows (never-written rows hold the fill)."""
    fill = np.frombuffer(b"\x80" * 8, dtype="<i8")[0]
    out = {"lt": np.full(capacity, fill, np.int64), "rank": np.full(capacity, 0x80808080, np.uint32),
           "val": np.full(capacity, 0x80808080, np.uint32), "mod": np.full(capacity, ABSENT_MOD, np.int64)}
    for name in out:
        out[name][rows["ids"]] = rows[name]
    first, count = rows["clear"]
    for name, v in (("lt", fill), ("rank", 0x80808080), ("val", 0x80808080), ("mod", ABSENT_MOD)):
        out[name][first:first + count] = v
    return out


def decisions(src: dict, dst: dict, n_rows: int, since: int) -> dict:
    """Which of the four decisions the merge of src's selection into dst contains (counts of rows)."""
    s, d = dense(src, n_rows), dense(dst, n_rows)
    sel = ~(s["mod"] < since)
    vis = d["mod"] >= 0
    newer = (s["lt"] > d["lt"]) | ((s["lt"] == d["lt"]) & (s["rank"] > d["rank"]))
    return {
        "tie_keeps_local": int(np.count_nonzero(sel & vis & (s["lt"] == d["lt"]) & (s["rank"] == d["rank"]))),
        "equal_lt_rank_wins": int(np.count_nonzero(sel & vis & (s["lt"] == d["lt"]) & (s["rank"] > d["rank"]))),
        "older_wins_invisible": int(np.count_nonzero(sel & ~vis & ~newer)),
        "tombstone_wins": int(np.count_nonzero(sel & (s["val"] == NULL) & (~vis | newer))),
    }


# ------------------------------------------------------------------ the contracts on the C restatement
# The compositions that crdt_merge_table, crdt_sync_tables, crdt_fanin_tables and merge_from are held to,
# on OracleTable objects (oracle/oracle_c.py; nothing here imports the library).  Every value a GPU test
# compares comes from these.
RESULT_FIELDS = ("status", "n_stored", "exc_changeset", "exc_index", "canonical_lt", "drift_ms", "counter",
                 "n_present", "n_won")
U64_MAX = (1 << 64) - 1
CLEARED = {"status": 0, "n_stored": 0, "exc_changeset": 0, "exc_index": U64_MAX, "drift_ms": 0, "counter": 0,
           "n_present": 0, "n_won": 0}


def oracle_merge_from(dst, src, n_rows: int, since: int, wall: int):
    """dst.merge(src.recordMap(modifiedSince)); returns (result dict, flags by RECORD, records)."""
    ids = src.modified_since(n_rows, since)
    rows = src.rows[ids]
    res, flags = dst.merge(ids, rows["lt"].copy(), rows["rank"].copy(), rows["val"].copy(),
                           np.array([0, len(ids)], np.uint64), wall)
    return res.as_dict(), flags, len(ids)


def oracle_merge_table(odst, osrc, n_rows: int, since: int, wall: int):
    """The composition on the oracle; returns (result dict, flags by ROW id, selected ids)."""
    ids = osrc.modified_since(n_rows, since)
    rows = osrc.rows[ids]
    res, flags = odst.merge(ids, rows["lt"].copy(), rows["rank"].copy(), rows["val"].copy(),
                            np.array([0, len(ids)], np.uint64), wall)
    row_flags = np.zeros(n_rows, np.uint8)
    row_flags[ids[flags != 0]] = 1
    return res.as_dict(), row_flags, ids


def oracle_sync(oa, ob, n_rows, since_a, since_b, wall):
    """crdt_sync_tables' contract on the oracle: ((result a, flags a), (result b, flags b))."""
    res_a, fl_a, _ = oracle_merge_table(oa, ob, n_rows, since_b, wall)
    if res_a["status"] == 0:
        res_b, fl_b, _ = oracle_merge_table(ob, oa, n_rows, since_a, wall)
    else:
        res_b = {f: 0 for f in RESULT_FIELDS}
        res_b["exc_index"] = U64_MAX
        res_b["canonical_lt"] = ob.canonical
        fl_b = np.zeros(n_rows, np.uint8)
    return (res_a, fl_a), (res_b, fl_b)


def oracle_fanin(odst, osrcs, n_rows, sinces, wall):
    """crdt_fanin_tables' contract on the oracle: (results, mask, index of the step that stopped the
    sequence or None)."""
    results, mask, stop = [], np.zeros(n_rows, np.uint8), None
    for j, (osrc, since) in enumerate(zip(osrcs, sinces)):
        if stop is not None:
            results.append(dict(CLEARED, canonical_lt=odst.canonical))
            continue
        res, flags, _ = oracle_merge_table(odst, osrc, n_rows, since, wall)
        results.append(res)
        mask |= (flags << j).astype(np.uint8)
        if res["status"] != 0:
            stop = j
    return results, mask, stop
