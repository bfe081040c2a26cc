#!/usr/bin/env python3
"""The read-only replica diff and the block digests on one GPU against the routes there were before them,
unchanged code timed in the same process on the same two tables.

    python tools/diff_bench.py [--rows-log2 27] [--row-bytes 24] [--repeats 7] [--out FILE]

Diff legs: 0 % / 0.01 % / 1 % / 100 % of the rows differ (a third of them newer in b, a third newer in a, a
third a conflict), each with and without device flags.  The yardstick is the host route: read_rows of both
tables in 2^25-row chunks and the numpy comparison of tests/_diff_cases.model_diff per chunk.  Every call is
synchronous, so a host clock around it is the call's time.  Per leg both routes run once as a warm-up and must
agree (the six counts, and the flag bytes where they are taken); then they alternate inside each repeat and
the median, minimum and maximum are reported.  Accepted: the device diff's median is not above the host
route's by more than the larger min-max spread.

Also reported, without a bound: the diff's achieved bytes per second (2 * row_bytes * N read + N flag bytes
written) against the streaming-read ceiling of profiles/r06_ubench_stream.txt; count_since on each of the two
tables (an existing pass that touches every line of a table once: the sum of the two is what one streaming
read of both costs here); digest_rows against bench.shard_digests.
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
FRACTIONS = (0.0, 0.0001, 0.01, 1.0)
POOL = 1024
CHUNK = 1 << 25                              # rows per read_rows of the host route
READ_CEILING_GBS = 6929                      # profiles/r06_ubench_stream.txt: the fastest read leg


def rows_of(key):
    """The table's row of each key id (a torch int64 tensor on the device): a function of the id alone, so a
    perturbed row can be rebuilt from it."""
    import torch
    mod = torch.full_like(key, WALL << 16)
    lt = mod - (key * 40503 % 65536)
    val = (key * 2654435761 % POOL).to(torch.int32)
    val[key % 5 == 0] = -1                   # CRDT_NULL_VALUE
    return lt, torch.zeros_like(val), val, mod


def fill(table, n_rows: int, chunk: int = 1 << 24):
    import torch
    for first in range(0, n_rows, chunk):
        key = torch.arange(first, min(first + chunk, n_rows), dtype=torch.int64, device="cuda")
        lt, rk, val, mod = rows_of(key)
        table.put_rows(key.to(torch.int32), lt, rk, val, mod)


def perturb(table, ids, chunk: int = 1 << 24):
    """b's rows of these ids: id % 3 == 0 newer than a's, 1 older, 2 the same hlc under another value."""
    import torch
    for first in range(0, int(ids.numel()), chunk):
        key = ids[first:first + chunk].to(torch.int64)
        lt, rk, val, mod = rows_of(key)
        kind = key % 3
        lt = lt + (kind == 0) * (1 << 16) - (kind == 1) * (1 << 16)
        val = torch.where(kind == 2, (val + 1) % POOL, val)
        table.put_rows(key.to(torch.int32), lt, rk, val, mod)


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def summary(ms: list) -> dict:
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows-log2", type=int, default=27)
    ap.add_argument("--row-bytes", type=int, choices=[24, 32], default=24)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()

    import torch

    import bench
    from crdt_amd import DeviceTable, _capi
    from tests import _diff_cases as dc
    if _capi.device_count() < 1:
        sys.exit("diff_bench: no gfx950 device (these figures cannot be taken without one)")
    n_rows = 1 << args.rows_log2
    a, b = DeviceTable(0, local_rank=0, capacity=n_rows), DeviceTable(0, local_rank=1, capacity=n_rows)
    if args.row_bytes != 24:
        a.set_row_bytes(args.row_bytes)
        b.set_row_bytes(args.row_bytes)
    fill(a, n_rows)
    fill(b, n_rows)
    g = torch.Generator(device="cuda")
    g.manual_seed(args.seed)
    u = torch.rand(n_rows, device="cuda", generator=g)
    dflags = torch.zeros(n_rows, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def device_route(with_flags: bool):
        return a.diff_table(b, n_rows, flags=dflags if with_flags else False)

    def host_route(with_flags: bool):
        total = dict.fromkeys(dc.FIELDS, 0)
        total["first_diff"] = dc.NONE
        parts = []
        for first in range(0, n_rows, CHUNK):
            ids = np.arange(first, min(first + CHUNK, n_rows), dtype=np.uint32)
            ra = dict(zip(("lt", "rank", "val", "mod"), a.read_rows(ids)))
            rb = dict(zip(("lt", "rank", "val", "mod"), b.read_rows(ids)))
            flags, d = dc.model_diff(ra, rb, len(ids))
            for f in dc.FIELDS[:5]:
                total[f] += d[f]
            if d["first_diff"] != dc.NONE and total["first_diff"] == dc.NONE:
                total["first_diff"] = first + d["first_diff"]
            if with_flags:
                parts.append(flags)
        return total, (np.concatenate(parts) if with_flags else None)

    legs = []
    prev = 0.0
    for frac in FRACTIONS:
        if frac > prev:
            perturb(b, torch.nonzero((u >= prev) & (u < frac)).flatten())
            prev = frac
        for with_flags in (False, True):
            (d, fl), (want, want_fl) = device_route(with_flags), host_route(with_flags)   # warm-up: the routes agree
            assert d == want, (frac, d, want)
            if with_flags:
                assert np.array_equal(fl.cpu().numpy(), want_fl), frac
            del fl, want_fl
            times = {"diff_table": [], "host": []}
            for _ in range(args.repeats):
                for name, fn in (("diff_table", device_route), ("host", host_route)):
                    ms, out = timed(lambda: fn(with_flags))
                    del out
                    times[name].append(ms)
            row = {"fraction": frac, "device_flags": with_flags, "differing": d["n_a_ahead"] + d["n_b_ahead"] + d["n_conflict"],
                   "diff_table": summary(times["diff_table"]), "host": summary(times["host"])}
            new, old = row["diff_table"], row["host"]
            spread = max(new["max_ms"] - new["min_ms"], old["max_ms"] - old["min_ms"])
            row["accepted"] = new["median_ms"] <= old["median_ms"] + spread
            moved = n_rows * (2 * args.row_bytes + (1 if with_flags else 0))
            row["diff_gbs"] = round(moved / new["median_ms"] / 1e6, 1)
            row["of_read_ceiling"] = round(row["diff_gbs"] / READ_CEILING_GBS, 3)
            legs.append(row)

    # ---- one streaming read of each table with an existing pass, in this process
    counts = {}
    for name, t in (("a", a), ("b", b)):
        t.count_since(n_rows, 0)
        counts[f"count_since_{name}"] = summary([timed(lambda: t.count_since(n_rows, 0))[0] for _ in range(args.repeats)])

    # ---- the block digests against bench.shard_digests (read_rows of the table + bench.row_digests)
    got, want = a.digest_rows(n_rows), bench.shard_digests(a, n_rows)
    assert got.dtype == want.dtype and np.array_equal(got, want)
    dig = {"digest_rows": [], "shard_digests": []}
    for _ in range(min(args.repeats, 3)):
        dig["digest_rows"].append(timed(lambda: a.digest_rows(n_rows))[0])
        dig["shard_digests"].append(timed(lambda: bench.shard_digests(a, n_rows))[0])
    digest = {k: summary(v) for k, v in dig.items()}
    digest["state"] = summary([timed(lambda: a.digest_rows(n_rows, state=True))[0] for _ in range(args.repeats)])
    digest["digest_gbs"] = round(n_rows * args.row_bytes / digest["digest_rows"]["median_ms"] / 1e6, 1)

    out = {"bench": "diff", "rows": n_rows, "row_bytes": args.row_bytes, "table_bytes": n_rows * args.row_bytes,
           "repeats": args.repeats, "tile_rows": _capi.TABLE_TILE, "host_chunk_rows": CHUNK,
           "read_ceiling_gbs": READ_CEILING_GBS, "legs": legs, "accepted": all(r["accepted"] for r in legs),
           **counts, "digest": digest,
           "not_measured": ["32-B rows", "flags in host memory", "tables of different row sizes"]}
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
