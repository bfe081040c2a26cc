"""The two-way table sync (crdt_sync_tables) as a numpy model of its contract, pure numpy (test helper).

    s1 = a.merge(b.recordMap(modifiedSince: since_b))
    if s1 raised nothing: b.merge(a.recordMap(modifiedSince: since_a))      # a as step 1 left it

``model`` runs that composition on dense columns and reports what the tests need to know about a case
before they trust it: the winners of each direction, the rows stored on both sides, the ties kept, whether
a row may raise in either recv() (k_scan's conservative rule, the one the kernels use), whether step 1's
send() raises, whether R_a < since_a — and from those whether the library's fused form runs.

Cases: ``tests/_table_cases.gen_pair(n, seed)`` as (b's rows, a's rows), a's local rank 7, b's 6, the wall
MERGE_WALL, C_a = canon0(), C_b = 123."""
from __future__ import annotations

import numpy as np

from tests import _table_cases as tc

I64_MIN = tc.I64_MIN
A_RANK, B_RANK = tc.DST_RANK, 6
C_B = 123
MAX_DRIFT = 60000
SHAPES_T = 2048                                   # (= _capi.TABLE_TILE; the CPU test checks it)


def canon0() -> int:
    return int(np.sort(tc.STAMPS)[tc.N_STAMPS // 2]) + 1      # some selected lts above it, some below


def mid() -> int:
    return int(np.sort(tc.STAMPS)[tc.N_STAMPS // 2])


def since_pairs():
    """(since_a, since_b): a selects since_a from ITS rows for b, and takes b's rows since since_b."""
    m, top = mid(), tc.TOP
    return [(0, 0), (m, m), (0, I64_MIN), (I64_MIN, 0), (-1, top), (m, top + 1), (top, 0), (top + 1, m)]


def shapes():
    T = SHAPES_T
    return [0, 1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 17]


def send(c: int, wall: int):
    """Hlc.send at a fixed wall (hlc.dart:51-74): (status, canonical after)."""
    m, cnt = c >> 16, c & 0xFFFF
    mn = max(m, wall)
    cn = cnt + 1 if mn == m else 0
    if mn - wall > MAX_DRIFT:
        return 1, c
    if cn > 0xFFFF:
        return 3, c
    return 0, (mn << 16) + cn


def _newer(x, y):
    return (x["lt"] > y["lt"]) | ((x["lt"] == y["lt"]) & (x["rank"] > y["rank"]))


def _may_raise(lt, rank, sel, canon, local_rank, wall):
    return bool(np.any(sel & (lt > canon) & ((rank == local_rank) | ((lt >> 16) - wall > MAX_DRIFT))))


def model(a: dict, b: dict, n: int, since_a: int, since_b: int, c_a: int, c_b: int, wall: int,
          rank_a: int = A_RANK, rank_b: int = B_RANK) -> dict:
    """The composition on dense columns {lt, rank, val, mod} of a and b (first n rows).  Exact only where
    no recv() raises (``may_raise_*`` False); the tests use it for the plan and for what a case contains,
    the C oracle for every compared value."""
    a = {k: v[:n] for k, v in a.items()}
    b = {k: v[:n] for k, v in b.items()}
    sel_b = ~(b["mod"] < since_b)
    vis_a = a["mod"] >= 0
    win_a = sel_b & (~vis_a | _newer(b, a))
    r_a = max(c_a, int(b["lt"][sel_b].max())) if sel_b.any() else c_a
    st1, canon_a = send(r_a, wall)
    raise1 = _may_raise(b["lt"], b["rank"], sel_b, c_a, rank_a, wall)
    a2 = {k: np.where(win_a, b[k], a[k]) for k in ("lt", "rank", "val")}
    a2["mod"] = np.where(win_a, np.int64(r_a), a["mod"])
    sel_a = ~(a2["mod"] < since_a)
    vis_b = b["mod"] >= 0
    win_b = sel_a & (~vis_b | _newer(a2, b))
    r_b = max(c_b, int(a2["lt"][sel_a].max())) if sel_a.any() else c_b
    st2, canon_b = send(r_b, wall)
    # the rows the fused form's direction-2 words are taken over: step 1's winners counted as selected
    sel_a_assumed = win_a | ~(a["mod"] < since_a)
    raise2 = _may_raise(a2["lt"], a2["rank"], sel_a_assumed, c_b, rank_b, wall)
    tie = (a["lt"] == b["lt"]) & (a["rank"] == b["rank"])
    out = {
        "win_a": win_a, "win_b": win_b, "sel_a": sel_a, "sel_b": sel_b, "r_a": r_a, "r_b": r_b,
        "both": win_a & win_b, "status_1": st1, "status_2": st2, "canon_a": canon_a, "canon_b": canon_b,
        "ties_kept": sel_b & sel_a & vis_a & vis_b & tie & ~win_a & ~win_b,
        "may_raise_1": raise1, "may_raise_2": raise2, "ra_below_since_a": r_a < since_a,
    }
    out["fused"] = not (raise1 or raise2 or st1 != 0 or r_a < since_a)
    return out


def pair(n: int, seed: int):
    """(a's written rows, b's written rows) of the generator: gen_pair's (source, destination) = (b, a)."""
    b, a = tc.gen_pair(n, seed)
    return a, b


def select_pattern(n_rows: int, seed: int, sel: np.ndarray, lo: int, hi: int) -> dict:
    """Every row written; mod = hi where ``sel`` else lo, so ``since = hi`` selects exactly ``sel``."""
    rng = np.random.default_rng(seed)
    rows = {"ids": np.arange(n_rows, dtype=np.uint32), "mod": np.where(sel, hi, lo).astype(np.int64)}
    rows["lt"] = tc.STAMPS[rng.integers(0, tc.N_STAMPS, n_rows)].astype(np.int64)
    rows["rank"] = rng.integers(0, 6, n_rows).astype(np.uint32)
    rows["val"] = rng.integers(0, 1 << 20, n_rows).astype(np.uint32)
    rows["val"][rng.random(n_rows) < 0.2] = 0xFFFFFFFF
    return rows


def patterns(T: int, n_rows: int) -> dict:
    """Tile-skipping patterns over 5T+9 rows: name -> (rows of a selected, rows of b selected)."""
    z = lambda: np.zeros(n_rows, bool)  # noqa: E731
    out = {}
    s = z(); s[T + 5:T + 300] = True
    out["only_a"] = (s, z())
    out["only_b"] = (z(), s.copy())
    sa, sb = z(), z()
    sa[T // 2:T // 2 + 100] = True
    sb[3 * T + 7:3 * T + 400] = True
    out["disjoint_tiles"] = (sa, sb)
    sa, sb = z(), z()
    sa[2 * T + 10:2 * T + 500:3] = True
    sb[2 * T + 11:2 * T + 900:2] = True
    out["same_tile"] = (sa, sb)
    sa, sb = z(), z()
    sa[2 * T] = sb[3 * T - 1] = True
    sa[4 * T - 1] = sb[4 * T - 1] = True
    sb[4 * T] = True
    out["tile_ends"] = (sa, sb)
    sa, sb = z(), z()
    sa[2 * T - 300:2 * T + 500] = True
    sb[4 * T - 100:4 * T + 50] = True
    out["run_across_boundary"] = (sa, sb)
    out["none"] = (z(), z())
    return out
