#!/usr/bin/env python3
"""Replica-to-replica sync on one GPU: the export + merge composition (DeviceTable.merge_from, the
route before crdt_merge_table) against the fused table merge (DeviceTable.merge_table), in one
process on one pair of tables.

    python tools/sync_bench.py [--rows-log2 27] [--row-bytes 24] [--repeats 7] [--out FILE]

The source's rows carry one of three mod stamps, so one table serves every selected fraction:
since = S1 selects every row, S2 about 1 %, S3 about 0.01 %.  The destination is generated
independently (so about half of the selected rows win) and is reset to the same rows and canonical
before every call, timed or not.  Each call is synchronous, so a host clock around it is the call's
time.  Per fraction and flags setting the two routes are warmed once (and must leave the same rows,
result and flags), then alternate inside each of the repeats; median, min and max are reported.

"model_bytes" is the pass model of DESIGN.md §6d, from byte counts in the code (rows of 24 B):
  composed  24 B x rows (count pass) + 24 B x rows in tiles holding a selected row (write pass)
            + (28 + 12 + 28 + 24) B x selected (export columns written, scan, apply's reads, its row
            gathers) + 24 B x winners (+ 1 B x selected with flags)
  fused     24 B x rows (clock pass) + rows / 8 B (its selection bits) + the apply pass: the bits of the
            tiles holding a selected row, and of src and dst the lines of the selected rows, 2 x 128 B
            x selected but at most 48 B x rows in those tiles, + 24 B x winners (+ 1 B x rows with flags)
and "model_tbps" is that over the median.  Device memory in use is taken with torch.cuda.mem_get_info
around the first 100 % call of each route.  Prints one JSON line."""
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
DST_CANON = S1 - (1 << 20)


def fill(table, n_rows: int, seed: int, tile: int, chunk: int = 1 << 24, count: bool = True):
    """Rows generated on the device, chunk by chunk (no host copy of the table).  Returns, per
    fraction, (selected rows, tiles holding a selected row)."""
    import torch
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    stats = [[0, 0] for _ in FRACTIONS]
    for first in range(0, n_rows, chunk):
        m = min(chunk, n_rows - first)
        u = torch.rand(m, device="cuda", generator=g)
        mod = torch.full((m,), S1, dtype=torch.int64, device="cuda")
        mod[u < 0.01] = S2
        mod[u < 0.0001] = S3
        key = torch.arange(first, first + m, dtype=torch.int32, device="cuda")
        lt = mod - torch.randint(0, 1 << 16, (m,), device="cuda", generator=g)
        rank = torch.randint(0, 6, (m,), device="cuda", generator=g, dtype=torch.int32)
        val = torch.randint(0, 1 << 20, (m,), device="cuda", generator=g, dtype=torch.int32)
        val[torch.rand(m, device="cuda", generator=g) < 0.2] = -1          # CRDT_NULL_VALUE
        table.put_rows(key, lt, rank, val, mod)
        for k, (_, since) in enumerate(FRACTIONS if count else ()):
            sel = mod >= since
            stats[k][0] += int(sel.sum())
            pad = (-m) % tile
            if pad:
                sel = torch.cat([sel, torch.zeros(pad, dtype=torch.bool, device="cuda")])
            stats[k][1] += int(sel.view(-1, tile).any(dim=1).sum())
    return stats


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
        sys.exit("sync_bench: no gfx950 device (these figures cannot be taken without one)")
    n_rows = 1 << args.rows_log2
    rb = args.row_bytes
    tile = _capi.TABLE_TILE
    assert tile == _capi.EXPORT_TILE                     # (one "tiles holding a selected row" count serves both)
    src = DeviceTable(0, local_rank=1, capacity=n_rows)
    dst = DeviceTable(0, local_rank=7, capacity=n_rows)
    src.set_row_bytes(rb)
    dst.set_row_bytes(rb)
    sel_stats = fill(src, n_rows, args.seed, tile)

    def reset():
        fill(dst, n_rows, args.seed + 1000, tile, count=False)
        dst.canonical = DST_CANON

    def used():
        torch.cuda.synchronize()
        free, total = torch.cuda.mem_get_info(0)
        return total - free

    def composed(since, flags):
        return dst.merge_from(src, n_rows, since, MERGE_WALL, win_flags=flags)

    def fused(since, flags):
        return dst.merge_table(src, n_rows, since, MERGE_WALL, row_flags=flags)

    routes = (("composed", composed), ("fused", fused))
    probe = np.arange(0, n_rows, max(n_rows >> 16, 1), dtype=np.uint32)     # rows compared between the routes
    memory = {}
    legs = []
    for k, (frac, since) in enumerate(FRACTIONS):
        n_sel, tiles_sel = sel_stats[k]
        touched = min(tiles_sel * tile, n_rows)
        for flags in (False, True):
            # warm-up: both routes from the same destination, and they must agree before either is timed
            seen = {}
            for name, fn in reversed(routes):            # (fused first: its memory figure is taken before the
                reset()                                  # composition has grown its export buffers)
                before = used()
                res, fl = fn(since, flags)
                after = used()
                if frac == 1.0 and not flags:
                    memory[name] = {"before_bytes": before, "after_bytes": after, "growth_bytes": after - before}
                rows = dst.read_rows(probe)
                # (per-record flags on one route, per-row flags on the other: both mark the winners)
                seen[name] = (res, rows, int(fl.sum()) if flags else None, dst.canonical)
                del fl
            a, b = seen["composed"], seen["fused"]
            assert a[0] == b[0] and a[3] == b[3], (a[0], b[0])
            assert all((x == y).all() for x, y in zip(a[1], b[1]))
            assert a[2] == b[2] and (a[2] is None or a[2] == a[0]["n_won"])
            n_won = a[0]["n_won"]
            del seen, a, b
            times = {name: [] for name, _ in routes}
            plan_table = None
            for _ in range(args.repeats):
                for name, fn in routes:
                    reset()
                    torch.cuda.synchronize()
                    ms, out = timed(lambda: fn(since, flags))
                    del out
                    times[name].append(ms)
                    if name == "fused":
                        plan_table = dst.last_plan()["table"]
            model = {
                "composed": rb * n_rows + rb * touched + (28 + 12 + 28 + 24) * n_sel + rb * n_won
                            + (n_sel if flags else 0),
                "fused": rb * n_rows + n_rows // 8 + touched // 8 + min(2 * rb * touched, 2 * 128 * n_sel)
                         + rb * n_won + (n_rows if flags else 0),
            }
            row = {"fraction": frac, "flags": flags, "selected": n_sel, "won": n_won,
                   "tiles_selected": tiles_sel, "fused_ran_table_form": plan_table}
            for name, _ in routes:
                med = statistics.median(times[name])
                row[f"{name}_ms"] = round(med, 3)
                row[f"{name}_min_ms"] = round(min(times[name]), 3)
                row[f"{name}_max_ms"] = round(max(times[name]), 3)
                row[f"{name}_model_bytes"] = model[name]
                row[f"{name}_model_tbps"] = round(model[name] / (med * 1e-3) / 1e12, 3)
            row["speedup"] = round(row["composed_ms"] / row["fused_ms"], 3)
            legs.append(row)
    out = {"bench": "sync", "rows": n_rows, "row_bytes": rb, "table_bytes": n_rows * rb, "repeats": args.repeats,
           "tile_rows": tile, "memory_full_sync": memory, "legs": legs}
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    src.close()
    dst.close()


if __name__ == "__main__":
    main()
