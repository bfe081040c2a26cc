#!/usr/bin/env python3
"""Changeset export on one GPU: the id-only compaction plus a row gather to the host
(crdt_modified_since + crdt_read_rows) against the fused device-resident export
(crdt_export_since), with and without its host copy, in one process on one table.

    python tools/export_bench.py [--rows-log2 27] [--row-bytes 24] [--repeats 7] [--out FILE]

The table's rows carry one of three mod stamps, so one table serves every selection fraction:
since = S1 selects every row, S2 about 1 %, S3 about 0.01 %.  Each call is synchronous (it ends
in a stream synchronise), so a host clock around it is the call's time.  Every leg is warmed
once per fraction, then the legs alternate inside each repeat; the median and the minimum of the
repeats are reported.  "table GB/s" is the table's bytes over the call's time — how fast the call
gets through the table, not the bytes it moved (the export reads the table about twice).
Prints one JSON line."""
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


def fill(table, n_rows: int, seed: int, chunk: int = 1 << 24):
    """Rows generated on the device, chunk by chunk (no host copy of the table)."""
    import torch
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
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

    from crdt_amd import DeviceTable, _capi
    if _capi.device_count() < 1:
        sys.exit("export_bench: no gfx950 device (these figures cannot be taken without one)")
    n_rows = 1 << args.rows_log2
    t = DeviceTable(0, capacity=n_rows)
    t.set_row_bytes(args.row_bytes)
    fill(t, n_rows, args.seed)
    table_bytes = n_rows * args.row_bytes

    def parent(since):
        ids = t.modified_since(n_rows, since)
        return (ids,) + tuple(t.read_rows(ids))

    def export(since):
        return t.export_since(n_rows, since)

    def export_columns(since):
        return t.export_since(n_rows, since).columns()

    legs = (("parent", parent), ("export", export), ("export_columns", export_columns))
    results = []
    for frac, since in FRACTIONS:
        # warm-up, and the three routes must agree before any of them is timed
        ref = parent(since)
        got = export_columns(since)
        ex = export(since)
        assert ex.n == len(ref[0]) == len(got[0])
        for a, b in zip(ref, (got[0], got[1], got[2], got[3], got[4])):
            assert np.array_equal(a, b)
        n_sel = ex.n
        del ref, got
        times = {name: [] for name, _ in legs}
        for _ in range(args.repeats):
            for name, fn in legs:
                ms, out = timed(lambda: fn(since))
                del out
                times[name].append(ms)
        row = {"fraction": frac, "selected": n_sel}
        for name, _ in legs:
            med, best = statistics.median(times[name]), min(times[name])
            row[f"{name}_ms"] = round(med, 3)
            row[f"{name}_min_ms"] = round(best, 3)
            row[f"{name}_table_gbps"] = round(table_bytes / (med * 1e-3) / 1e9, 1)
        results.append(row)
    count_ms = [timed(lambda: t.count_since(n_rows, S2))[0] for _ in range(args.repeats + 1)][1:]
    out = {"bench": "export", "rows": n_rows, "row_bytes": args.row_bytes, "table_bytes": table_bytes,
           "repeats": args.repeats, "tile_rows": _capi.EXPORT_TILE,
           "count_since_ms": round(statistics.median(count_ms), 3),
           "count_since_table_gbps": round(table_bytes / (statistics.median(count_ms) * 1e-3) / 1e9, 1),
           "legs": results}
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    t.close()


if __name__ == "__main__":
    main()
