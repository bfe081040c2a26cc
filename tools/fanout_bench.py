#!/usr/bin/env python3
"""The hub's outbound half on one GPU: one table merged into N tables by N table merges
(DeviceTable.merge_table once per destination, the route before crdt_fanout_tables) against the fused fan-out
(DeviceTable.fanout_tables), in one process on one set of tables.

    python tools/fanout_bench.py [--rows-log2 27] [--row-bytes 24] [--repeats 7] [--dests 2 4 8] [--out FILE]

The source's rows carry one of three mod stamps (tools/sync2_bench.py's generator), so one table serves every
selected fraction: since = S1 selects every row, S2 about 1 %, S3 about 0.01 %; all destinations of a leg use
the same since.  The replicas are generated independently, and every destination's canonical sits at the top
stamp, so no selected row is a candidate and the fused form runs.  The source is never written; the
destinations of a leg are put back to the same rows and canonical before every call, timed or not, from column
tensors kept on the device.  Each call is synchronous, so a host clock around it is the call's time.  Per leg
(destinations, fraction, mask or not) the two routes are warmed once (and must leave the same canonicals,
results and mask, compared in full, and the same rows on a probe of 2^16 evenly spaced rows of every
destination; the composition's mask is the OR of its steps' row flags, shifted), then alternate inside
each of the repeats; median, min and max are reported.  With the mask, the composition writes one preallocated
flag array per step and the fused form one preallocated mask.

"model_bytes" is the byte model of DESIGN.md §6g (rows of 24 B, 20 B of a row read by a clock pass; N rows, S_j
selected for destination j, W_j winners there, U selected for any):
  composed  sum over j of 20 N + 40 S_j + 24 W_j (+ N with flags)
  fused     20 N + 24 U + sum over j of 16 S_j + 24 W_j (+ N with the mask)
"within_spread": the fused median is not above the composition's by more than the larger of the two routes'
min-max spreads; "ranges_overlap": the two routes' [min, max] intervals intersect.
Prints one JSON line."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from sync2_bench import FRACTIONS, MERGE_WALL, columns, put, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows-log2", type=int, default=27)
    ap.add_argument("--row-bytes", type=int, choices=[24, 32], default=24)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--dests", type=int, nargs="+", default=[2, 4, 8])
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()

    import torch

    from crdt_amd import DeviceTable, _capi
    if _capi.device_count() < 1:
        sys.exit("fanout_bench: no gfx950 device (these figures cannot be taken without one)")
    n_rows = 1 << args.rows_log2
    rb = args.row_bytes
    n_max = max(args.dests)
    assert 2 <= min(args.dests) and n_max <= _capi.FANOUT_MAX
    src = DeviceTable(0, local_rank=6, capacity=n_rows)
    src.set_row_bytes(rb)
    cols = columns(n_rows, args.seed)
    put(src, cols)                               # the source is read-only: put once, only its mods kept
    src_mod = cols[4]
    del cols
    dsts, cols_d = [], []
    for j in range(n_max):
        d = DeviceTable(0, local_rank=7 + j, capacity=n_rows)
        d.set_row_bytes(rb)
        dsts.append(d)
        cols_d.append(columns(n_rows, args.seed + 1000 * (j + 1)))
    step_flags = [torch.zeros(n_rows, dtype=torch.uint8, device="cuda") for _ in range(n_max)]
    mask_buf = torch.zeros(n_rows, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def reset(n_dst):
        for j in range(n_dst):
            put(dsts[j], cols_d[j])              # (sets the canonical too)

    def composed(n_dst, since, mask):
        out = []
        for j in range(n_dst):
            res, _ = dsts[j].merge_table(src, n_rows, since, MERGE_WALL, row_flags=step_flags[j] if mask else False)
            out.append(res)
            if res["status"] != 0:
                break
        return out

    def fused(n_dst, since, mask):
        return src.fanout_tables(dsts[:n_dst], n_rows, [since] * n_dst, MERGE_WALL,
                                 win_mask=mask_buf if mask else False)[0]

    routes = (("composed", composed), ("fused", fused))
    probe = np.arange(0, n_rows, max(n_rows >> 16, 1), dtype=np.uint32)     # rows compared between the routes
    legs = []
    for n_dst in args.dests:
        for frac, since in FRACTIONS:
            selected = int((src_mod >= since).sum())          # the same since for every destination: U = S_j
            for mask in (True, False):
                # warm-up: both routes from the same tables, and they must agree before either is timed
                seen = {}
                for name, fn in routes:
                    reset(n_dst)
                    res = fn(n_dst, since, mask)
                    seen[name] = (res, [d.read_rows(probe) for d in dsts[:n_dst]], [d.canonical for d in dsts[:n_dst]])
                x, y = seen["composed"], seen["fused"]
                assert x[0] == y[0] and x[2] == y[2], (x[0], y[0])
                assert all(r["status"] == 0 for r in x[0]) and len(x[0]) == n_dst
                assert all((p == q).all() for a, b in zip(x[1], y[1]) for p, q in zip(a, b))
                if mask:
                    want = torch.zeros(n_rows, dtype=torch.uint8, device="cuda")
                    for j in range(n_dst):
                        want |= step_flags[j] << j
                    assert torch.equal(want, mask_buf)
                    assert [int(f.sum()) for f in step_flags[:n_dst]] == [r["n_won"] for r in x[0]]
                    del want
                won = [r["n_won"] for r in x[0]]
                del seen, x, y
                times = {name: [] for name, _ in routes}
                plans = None
                for _ in range(args.repeats):
                    for name, fn in routes:
                        reset(n_dst)
                        torch.cuda.synchronize()
                        ms, out = timed(lambda: fn(n_dst, since, mask))
                        del out
                        times[name].append(ms)
                        if name == "fused":
                            plans = [d.last_plan() for d in dsts[:n_dst]]
                row = {"dests": n_dst, "fraction": frac, "mask": mask, "selected": selected, "won": won,
                       "fused_ran_fanout_form": all(p["table"] and p["fanout"] for p in plans)}
                model = {
                    "composed": sum(20 * n_rows + 40 * selected + 24 * w + (n_rows if mask else 0) for w in won),
                    "fused": 20 * n_rows + 24 * selected + sum(16 * selected + 24 * w for w in won)
                             + (n_rows if mask else 0),
                }
                for name, _ in routes:
                    med = statistics.median(times[name])
                    row[f"{name}_ms"] = round(med, 3)
                    row[f"{name}_min_ms"] = round(min(times[name]), 3)
                    row[f"{name}_max_ms"] = round(max(times[name]), 3)
                    row[f"{name}_model_bytes"] = model[name]
                    row[f"{name}_model_tbps"] = round(model[name] / (med * 1e-3) / 1e12, 3)
                row["speedup"] = round(row["composed_ms"] / row["fused_ms"], 3)
                row["model_bytes_ratio"] = round(model["composed"] / model["fused"], 3)
                spread = max(max(times[name]) - min(times[name]) for name, _ in routes)
                row["within_spread"] = bool(statistics.median(times["fused"]) <=
                                            statistics.median(times["composed"]) + spread)
                row["ranges_overlap"] = bool(min(times["fused"]) <= max(times["composed"]) and
                                             min(times["composed"]) <= max(times["fused"]))
                legs.append(row)
                print(json.dumps(row), file=sys.stderr, flush=True)
    out = {"bench": "fanout", "rows": n_rows, "row_bytes": rb, "table_bytes": n_rows * rb, "repeats": args.repeats,
           "tile_rows": _capi.TABLE_TILE, "legs": legs}
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    src.close()
    for d in dsts:
        d.close()


if __name__ == "__main__":
    main()
