"""The flag-predicated export's contract (crdt_export_flagged) as a numpy model, and the case list of
tests/test_gpu_export_flagged.py, pure numpy (test helper): nothing here imports the library.

The export of a table under (n_rows, flags, bits) is the rows ``ids = flatnonzero(flags[:n_rows] & bits)``
as they are in the table, ascending by id; n_live counts those whose val is not the tombstone handle."""
from __future__ import annotations

import numpy as np

from tests._cases import NULL

T = 2048                                  # (= _capi.EXPORT_TILE; the CPU test checks it)
SCAN_STEP = 1024                          # (= _capi.EXPORT_SCAN_STEP)
COUNT_GRID = 2048                         # (= _capi.EXPORT_COUNT_GRID)
COLS = ("lt", "rank", "val", "mod")
BITS = (0x01, 0x80, 0x05, 0xFF, 0)
SHAPES = (0, 1, T - 1, T, T + 1, 5 * T + 9)
LARGE_SHAPES = ((SCAN_STEP + 1) * T + 3,  # the scan's loop runs a second time, with a carry
                (COUNT_GRID + 1) * T + 5)  # more tiles than workgroups: the count and write grids stride


def model(rows, n_rows: int, flags: np.ndarray, bits: int) -> dict:
    """``rows``: a structured array (or dict of columns) with lt, rank, val, mod, indexed by row id."""
    ids = np.flatnonzero(flags[:n_rows] & np.uint8(bits)).astype(np.uint32)
    out = {"key": ids, "n": len(ids)}
    for name in COLS:
        out[name] = np.asarray(rows[name])[ids]
    out["n_live"] = int(np.count_nonzero(out["val"] != NULL))
    return out


def brute_force(rows, n_rows: int, flags, bits: int) -> dict:
    """The same, one row at a time."""
    out = {"key": [], **{name: [] for name in COLS}}
    live = 0
    for i in range(n_rows):
        if int(flags[i]) & bits:
            out["key"].append(i)
            for name in COLS:
                out[name].append(int(rows[name][i]))
            live += int(rows["val"][i]) != NULL
    out["n"], out["n_live"] = len(out["key"]), live
    return out


def patterns(n_rows: int, high_water: int | None = None, seed: int = 0) -> dict:
    """name -> which rows are flagged (bool[n_rows]).  ``high_water``: the first never-written row."""
    rng = np.random.default_rng(9000 + n_rows + seed)
    idx = np.arange(n_rows)
    p = {"none": np.zeros(n_rows, bool), "all": np.ones(n_rows, bool),
         "half": rng.random(n_rows) < 0.5, "one_percent": rng.random(n_rows) < 0.01,
         "lane0_of_each_tile": idx % T == 0, "lane63_of_each_tile": idx % T == 63,
         "last_row_of_each_tile": idx % T == T - 1}
    last = np.zeros(n_rows, bool)
    if n_rows:
        last[-1] = True
    p["last_row"] = last
    if high_water is not None:
        p["above_high_water"] = idx >= high_water
    if n_rows >= 3 * T:
        p["empty_tile_between_full"] = (idx < T) | ((idx >= 2 * T) & (idx < 3 * T))
    return p


def mask_bytes(sel: np.ndarray, bits: int, seed: int = 0) -> np.ndarray:
    """Mask bytes whose ``& bits`` is non-zero exactly where ``sel``: a selected row carries a random non-empty
    subset of ``bits``, and every row random bits outside them."""
    rng = np.random.default_rng(77 + seed + bits)
    n = len(sel)
    other = rng.integers(0, 256, n).astype(np.uint8) & np.uint8(~bits & 0xFF)
    if bits == 0:
        return other
    own = rng.integers(0, 256, n).astype(np.uint8) & np.uint8(bits)
    lowest = np.uint8(bits & -bits)
    own = np.where(own == 0, lowest, own).astype(np.uint8)
    return np.where(sel, own | other, other).astype(np.uint8)
