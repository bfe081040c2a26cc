#!/usr/bin/env python3
"""The two-replica exchange on one GPU: two table merges (DeviceTable.merge_table a <- b, then b <- a, the
route before crdt_sync_tables) against the fused two-way sync (DeviceTable.sync_tables), in one process on
one pair of tables.

    python tools/sync2_bench.py [--rows-log2 27] [--row-bytes 24] [--repeats 7] [--out FILE]

Both replicas' rows carry one of three mod stamps, so one pair of tables serves every selected fraction:
since = S1 selects every row of a side, S2 about 1 %, S3 about 0.01 %; both directions use the same since.
The replicas are generated independently (about half of the selected rows win) and their canonicals sit at
the top stamp, as a replica's does above its own rows' stamps, so step 1's winners are selected by step 2
and the fused form runs.  Both tables are put back to the same rows and canonicals before every call, timed
or not, from column tensors kept on the device.  Each call is synchronous, so a host clock around it is the
call's time.  Per fraction and flags setting the two routes are warmed once (and must leave the same rows,
canonicals, results and flags), then alternate inside each of the repeats; median, min and max are reported.

"model_bytes" is the pass model of DESIGN.md §6e, from byte counts in the code (rows of 24 B; "touched" =
rows of the tiles that hold a row selected in a direction, or in either for the fused form):
  composed  per direction: 24 B x rows (clock pass) + rows / 8 B (its bits) + touched / 8 B + of both tables
            the lines of the selected rows, 2 x 128 B x selected but at most 48 B x touched
            + 24 B x winners (+ 1 B x rows with flags)
  fused     48 B x rows (clock pass over both tables) + rows / 4 B (its bits) + touched / 4 B + the same
            lines once for the rows selected either way + 24 B x winners of both sides (+ 2 B x rows with flags)
and "model_tbps" is that over the median.  Prints one JSON line."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WALL = 1_700_000_000_000
S1, S2, S3 = (WALL << 16), ((WALL + 10) << 16), ((WALL + 20) << 16)
FRACTIONS = ((1.0, S1), (0.01, S2), (0.0001, S3))
MERGE_WALL = WALL + 100
CANON = S3                                   # >= every row's mod and lt on both sides


def columns(n_rows: int, seed: int, chunk: int = 1 << 24):
    """One replica's rows as device columns (key, lt, rank, val, mod), generated chunk by chunk."""
    import torch
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    key = torch.arange(n_rows, dtype=torch.int32, device="cuda")
    lt = torch.empty(n_rows, dtype=torch.int64, device="cuda")
    mod = torch.empty(n_rows, dtype=torch.int64, device="cuda")
    rank = torch.empty(n_rows, dtype=torch.int32, device="cuda")
    val = torch.empty(n_rows, dtype=torch.int32, device="cuda")
    for first in range(0, n_rows, chunk):
        m = min(chunk, n_rows - first)
        s = slice(first, first + m)
        u = torch.rand(m, device="cuda", generator=g)
        md = torch.full((m,), S1, dtype=torch.int64, device="cuda")
        md[u < 0.01] = S2
        md[u < 0.0001] = S3
        mod[s] = md
        lt[s] = md - torch.randint(0, 1 << 16, (m,), device="cuda", generator=g)
        rank[s] = torch.randint(0, 6, (m,), device="cuda", generator=g, dtype=torch.int32)
        v = torch.randint(0, 1 << 20, (m,), device="cuda", generator=g, dtype=torch.int32)
        v[torch.rand(m, device="cuda", generator=g) < 0.2] = -1          # CRDT_NULL_VALUE
        val[s] = v
    return key, lt, rank, val, mod


def put(table, cols, chunk: int = 1 << 24):
    n = len(cols[0])
    for first in range(0, n, chunk):
        table.put_rows(*(c[first:first + chunk] for c in cols))
    table.canonical = CANON


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows-log2", type=int, default=27)
    ap.add_argument("--row-bytes", type=int, choices=[24, 32], default=24)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()

    import torch

    from crdt_amd import DeviceTable, _capi
    if _capi.device_count() < 1:
        sys.exit("sync2_bench: no gfx950 device (these figures cannot be taken without one)")
    n_rows = 1 << args.rows_log2
    rb = args.row_bytes
    tile = _capi.TABLE_TILE
    a = DeviceTable(0, local_rank=7, capacity=n_rows)
    b = DeviceTable(0, local_rank=6, capacity=n_rows)
    a.set_row_bytes(rb)
    b.set_row_bytes(rb)
    cols_a, cols_b = columns(n_rows, args.seed), columns(n_rows, args.seed + 1000)

    def tiles_of(sel):
        pad = (-len(sel)) % tile
        if pad:
            sel = torch.cat([sel, torch.zeros(pad, dtype=torch.bool, device="cuda")])
        return int(sel.view(-1, tile).any(dim=1).sum())

    def reset():
        put(a, cols_a)
        put(b, cols_b)

    def composed(since, flags):
        ra, fa = a.merge_table(b, n_rows, since, MERGE_WALL, row_flags=flags)
        if ra["status"] != 0:
            return (ra, fa), (None, None)
        return (ra, fa), b.merge_table(a, n_rows, since, MERGE_WALL, row_flags=flags)

    def fused(since, flags):
        return a.sync_tables(b, n_rows, since, since, MERGE_WALL, row_flags=flags)

    routes = (("composed", composed), ("fused", fused))
    probe = np.arange(0, n_rows, max(n_rows >> 16, 1), dtype=np.uint32)     # rows compared between the routes
    legs = []
    for frac, since in FRACTIONS:
        sel_a0, sel_b = cols_a[4] >= since, cols_b[4] >= since
        counts = None                            # (taken in the flagged leg, which runs first: it needs the flags)
        for flags in (True, False):
            # warm-up: both routes from the same tables, and they must agree before either is timed
            seen = {}
            for name, fn in routes:
                reset()
                (ra, fa), (rbt, fb) = fn(since, flags)
                seen[name] = (ra, rbt, a.read_rows(probe), b.read_rows(probe), a.canonical, b.canonical, fa, fb)
            x, y = seen["composed"], seen["fused"]
            assert x[0] == y[0] and x[1] == y[1] and x[4:6] == y[4:6], (x[:2], y[:2])
            assert x[0]["status"] == 0 and x[1]["status"] == 0
            assert all((p == q).all() for p, q in zip(x[2] + x[3], y[2] + y[3]))
            if flags:
                assert torch.equal(x[6], y[6]) and torch.equal(x[7], y[7])
                assert int(x[6].sum()) == x[0]["n_won"] and int(x[7].sum()) == x[1]["n_won"]
                # step 2's selection: a's own selected rows and step 1's winners (stamped above since)
                sel_a = sel_a0 | (y[6] != 0)
                n_b, n_a, n_u = int(sel_b.sum()), int(sel_a.sum()), int((sel_b | sel_a).sum())
                counts = (n_b, n_a, n_u) + tuple(min(tiles_of(s) * tile, n_rows) for s in (sel_b, sel_a, sel_b | sel_a))
                del sel_a
            won_a, won_b = x[0]["n_won"], x[1]["n_won"]
            del seen, x, y
            times = {name: [] for name, _ in routes}
            plan = None
            for _ in range(args.repeats):
                for name, fn in routes:
                    reset()
                    torch.cuda.synchronize()
                    ms, out = timed(lambda: fn(since, flags))
                    del out
                    times[name].append(ms)
                    if name == "fused":
                        plan = a.last_plan()
            row = {"fraction": frac, "flags": flags, "selected_b": int(sel_b.sum()), "selected_a0": int(sel_a0.sum()),
                   "won_a": won_a, "won_b": won_b, "fused_ran_sync_form": bool(plan["table"] and plan["sync"])}
            n_b, n_a, n_u, t_b, t_a, t_u = counts
            lines = lambda t, n: min(2 * rb * t, 2 * 128 * n)  # noqa: E731
            fbytes = 2 * n_rows if flags else 0
            model = {
                "composed": 2 * (rb * n_rows + n_rows // 8) + (t_b + t_a) // 8 + lines(t_b, n_b) + lines(t_a, n_a)
                            + rb * (won_a + won_b) + fbytes,
                "fused": 2 * rb * n_rows + n_rows // 4 + t_u // 4 + lines(t_u, n_u) + rb * (won_a + won_b) + fbytes,
            }
            row.update(selected_a=n_a, selected_either=n_u)
            for name, _ in routes:
                med = statistics.median(times[name])
                row[f"{name}_ms"] = round(med, 3)
                row[f"{name}_min_ms"] = round(min(times[name]), 3)
                row[f"{name}_max_ms"] = round(max(times[name]), 3)
                row[f"{name}_model_bytes"] = model[name]
                row[f"{name}_model_tbps"] = round(model[name] / (med * 1e-3) / 1e12, 3)
            row["speedup"] = round(row["composed_ms"] / row["fused_ms"], 3)
            legs.append(row)
    out = {"bench": "sync2", "rows": n_rows, "row_bytes": rb, "table_bytes": n_rows * rb, "repeats": args.repeats,
           "tile_rows": tile, "legs": legs}
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    a.close()
    b.close()


if __name__ == "__main__":
    main()
