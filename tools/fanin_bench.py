#!/usr/bin/env python3
"""The hub on one GPU: N table merges into one table (DeviceTable.merge_table once per source, the route
before crdt_fanin_tables) against the fused fan-in (DeviceTable.merge_tables), in one process on one set of
tables.

    python tools/fanin_bench.py [--rows-log2 27] [--row-bytes 24] [--repeats 7] [--sources 2 4 8] [--out FILE]

Every replica's rows carry one of three mod stamps (tools/sync2_bench.py's generator), so one set of tables
serves every selected fraction: since = S1 selects every row of a source, S2 about 1 %, S3 about 0.01 %; all
sources of a leg use the same since.  The replicas are generated independently, and dst's canonical sits at the
top stamp, so no selected row is a candidate and the fused form runs.  The sources are never written; dst is
put back to the same rows and canonical before every call, timed or not, from column tensors kept on the
device.  Each call is synchronous, so a host clock around it is the call's time.  Per leg (sources, fraction,
mask or not) the two routes are warmed once (and must leave the same rows, canonical, results and mask: the
composition's mask is the OR of its steps' row flags, shifted), then alternate inside each of the repeats;
median, min and max are reported.  With the mask, the composition writes one preallocated flag array per
step and the fused form one preallocated mask.

"model_bytes" is the byte model of DESIGN.md §6f (rows of 24 B, 20 B of a row read by a clock pass):
  composed  per source: 20 B x rows + 40 B x selected + 24 B x winners (+ 1 B x rows with flags)
  fused     per source: 20 B x rows + 24 B x selected; once: 16 B x rows selected by any + 24 B x rows stored
            (+ 1 B x rows with the mask)
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

from sync2_bench import CANON, FRACTIONS, MERGE_WALL, columns, put, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows-log2", type=int, default=27)
    ap.add_argument("--row-bytes", type=int, choices=[24, 32], default=24)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--sources", type=int, nargs="+", default=[2, 4, 8])
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()

    import torch

    from crdt_amd import DeviceTable, _capi
    if _capi.device_count() < 1:
        sys.exit("fanin_bench: no gfx950 device (these figures cannot be taken without one)")
    n_rows = 1 << args.rows_log2
    rb = args.row_bytes
    n_max = max(args.sources)
    assert 2 <= min(args.sources) and n_max <= _capi.FANIN_MAX
    dst = DeviceTable(0, local_rank=7, capacity=n_rows)
    dst.set_row_bytes(rb)
    cols_d = columns(n_rows, args.seed)
    srcs, src_mod = [], []
    for j in range(n_max):                       # the sources are read-only: put once, only their mods kept
        s = DeviceTable(0, local_rank=6, capacity=n_rows)
        s.set_row_bytes(rb)
        cols = columns(n_rows, args.seed + 1000 * (j + 1))
        put(s, cols)
        src_mod.append(cols[4])
        del cols
        srcs.append(s)
    step_flags = [torch.zeros(n_rows, dtype=torch.uint8, device="cuda") for _ in range(n_max)]
    mask_buf = torch.zeros(n_rows, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def reset():
        put(dst, cols_d)                         # (sets the canonical too)

    def composed(n_src, since, mask):
        out = []
        for j in range(n_src):
            res, _ = dst.merge_table(srcs[j], n_rows, since, MERGE_WALL, row_flags=step_flags[j] if mask else False)
            out.append(res)
            if res["status"] != 0:
                break
        return out

    def fused(n_src, since, mask):
        return dst.merge_tables(srcs[:n_src], n_rows, [since] * n_src, MERGE_WALL,
                                win_mask=mask_buf if mask else False)[0]

    routes = (("composed", composed), ("fused", fused))
    probe = np.arange(0, n_rows, max(n_rows >> 16, 1), dtype=np.uint32)     # rows compared between the routes
    legs = []
    for n_src in args.sources:
        for frac, since in FRACTIONS:
            selected = [int((src_mod[j] >= since).sum()) for j in range(n_src)]
            any_sel = torch.zeros(n_rows, dtype=torch.bool, device="cuda")
            for j in range(n_src):
                any_sel |= src_mod[j] >= since
            n_any = int(any_sel.sum())
            del any_sel
            stored = None                        # (taken in the mask leg, which runs first: it needs the mask)
            for mask in (True, False):
                # warm-up: both routes from the same dst, and they must agree before either is timed
                seen = {}
                for name, fn in routes:
                    reset()
                    res = fn(n_src, since, mask)
                    seen[name] = (res, dst.read_rows(probe), dst.canonical)
                x, y = seen["composed"], seen["fused"]
                assert x[0] == y[0] and x[2] == y[2], (x[0], y[0])
                assert all(r["status"] == 0 for r in x[0]) and len(x[0]) == n_src
                assert all((p == q).all() for p, q in zip(x[1], y[1]))
                if mask:
                    want = torch.zeros(n_rows, dtype=torch.uint8, device="cuda")
                    for j in range(n_src):
                        want |= step_flags[j] << j
                    assert torch.equal(want, mask_buf)
                    assert [int(f.sum()) for f in step_flags[:n_src]] == [r["n_won"] for r in x[0]]
                    stored = int((mask_buf != 0).sum())
                    del want
                won = [r["n_won"] for r in x[0]]
                del seen, x, y
                times = {name: [] for name, _ in routes}
                plan = None
                for _ in range(args.repeats):
                    for name, fn in routes:
                        reset()
                        torch.cuda.synchronize()
                        ms, out = timed(lambda: fn(n_src, since, mask))
                        del out
                        times[name].append(ms)
                        if name == "fused":
                            plan = dst.last_plan()
                row = {"sources": n_src, "fraction": frac, "mask": mask, "selected": selected, "selected_any": n_any,
                       "won": won, "stored": stored, "fused_ran_fanin_form": bool(plan["table"] and plan["fanin"])}
                fbytes = n_rows if mask else 0
                model = {
                    "composed": sum(20 * n_rows + 40 * s + 24 * w + fbytes for s, w in zip(selected, won)),
                    "fused": sum(20 * n_rows + 24 * s for s in selected) + 16 * n_any + 24 * stored + fbytes,
                }
                for name, _ in routes:
                    med = statistics.median(times[name])
                    row[f"{name}_ms"] = round(med, 3)
                    row[f"{name}_min_ms"] = round(min(times[name]), 3)
                    row[f"{name}_max_ms"] = round(max(times[name]), 3)
                    row[f"{name}_model_bytes"] = model[name]
                    row[f"{name}_model_tbps"] = round(model[name] / (med * 1e-3) / 1e12, 3)
                row["speedup"] = round(row["composed_ms"] / row["fused_ms"], 3)
                legs.append(row)
                print(json.dumps(row), file=sys.stderr, flush=True)
    out = {"bench": "fanin", "rows": n_rows, "row_bytes": rb, "table_bytes": n_rows * rb, "repeats": args.repeats,
           "tile_rows": _capi.TABLE_TILE, "legs": legs}
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    dst.close()
    for s in srcs:
        s.close()


if __name__ == "__main__":
    main()
