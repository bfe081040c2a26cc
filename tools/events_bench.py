#!/usr/bin/env python3
"""The winners of a table merge as a list, on one GPU: the flag-predicated export
(crdt_export_flagged + its host copy) against the route there was before it (the row flags copied
to the host, np.flatnonzero, crdt_read_rows), in one process on one table; then MapCrdt.mergeFrom
on a two-member replica group, with and without a watch, against DeviceTable.merge_table alone.

    python tools/events_bench.py [--rows-log2 27] [--row-bytes 24] [--repeats 7] [--out FILE]

Flags are set for 100 % / 1 % / 0.01 % of the rows.  Each call is synchronous (it ends in a stream
synchronise), so a host clock around it is the call's time.  For every fraction both routes run once
as a warm-up and must return identical columns; then they alternate inside each repeat, and the
median, minimum and maximum of the repeats are reported.

The merge legs: before every timed call the source takes newer rows for the same ~1 % of the ids
(outside the timed region), so every call stores that many winners.  At this size the group's keys
are the integer ids themselves, installed once and outside the timed region (no 2^27-entry host
index is built), and the values come from a small pool of handles.
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
FRACTIONS = (1.0, 0.01, 0.0001)
POOL = 1024                                  # value handles of the merge legs


def fill(table, n_rows: int, seed: int, rank: int, chunk: int = 1 << 24):
    """Rows generated on the device, chunk by chunk (no host copy of the table)."""
    import torch
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    for first in range(0, n_rows, chunk):
        m = min(chunk, n_rows - first)
        key = torch.arange(first, first + m, dtype=torch.int32, device="cuda")
        mod = torch.full((m,), WALL << 16, dtype=torch.int64, device="cuda")
        lt = mod - torch.randint(0, 1 << 16, (m,), device="cuda", generator=g)
        rk = torch.full((m,), rank, dtype=torch.int32, device="cuda")
        val = torch.randint(0, POOL, (m,), device="cuda", generator=g, dtype=torch.int32)
        val[torch.rand(m, device="cuda", generator=g) < 0.2] = -1          # CRDT_NULL_VALUE
        table.put_rows(key, lt, rk, val, mod)


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def summary(ms: list) -> dict:
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}


def int_key_group(n_rows: int, row_bytes: int):
    """Two replicas of one group whose keys are the ids 0 .. n_rows - 1."""
    from crdt_amd import MapCrdt
    a = MapCrdt("a", capacity=n_rows, clock=lambda: WALL)
    b = a.replica("b")
    if row_bytes != 24:
        for r in (a, b):
            r._table.set_row_bytes(row_bytes)
    keys = a._keys
    keys._to_python()
    keys._list = range(n_rows)               # id -> key; nothing in these legs looks a key up
    for v in range(POOL):
        a._values.put(v)
    return a, b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows-log2", type=int, default=27)
    ap.add_argument("--row-bytes", type=int, choices=[24, 32], default=24)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()

    import torch
    from crdt_amd import _capi
    if _capi.device_count() < 1:
        sys.exit("events_bench: no gfx950 device (these figures cannot be taken without one)")
    n_rows = 1 << args.rows_log2
    a, b = int_key_group(n_rows, args.row_bytes)
    t = a._table
    fill(t, n_rows, args.seed, rank=0)
    fill(b._table, n_rows, args.seed, rank=0)            # the same rows: only the deltas below win
    g = torch.Generator(device="cuda")
    g.manual_seed(args.seed + 1)
    u = torch.rand(n_rows, device="cuda", generator=g)

    # ---- 1. the winners of given flags: export_flagged + columns() against flags -> host -> read_rows
    def new_route(flags):
        return t.export_flagged(n_rows, flags, 1).columns()

    def parent_route(flags):
        ids = np.flatnonzero(flags.cpu().numpy()).astype(np.uint32)
        return (ids,) + tuple(t.read_rows(ids))

    legs = (("export_flagged", new_route), ("parent", parent_route))
    results = []
    for frac in FRACTIONS:
        flags = (u < frac).to(torch.uint8)
        torch.cuda.synchronize()
        got, ref = new_route(flags), parent_route(flags)  # warm-up: the routes must agree before either is timed
        assert len(got[0]) == len(ref[0])
        for x, y in zip(got, ref):
            assert np.array_equal(x, y)
        row = {"fraction": frac, "flagged": int(len(ref[0]))}
        del got, ref
        times = {name: [] for name, _ in legs}
        for _ in range(args.repeats):
            for name, fn in legs:
                ms, out = timed(lambda: fn(flags))
                del out
                times[name].append(ms)
        for name, _ in legs:
            row[name] = summary(times[name])
        new, old = row["export_flagged"], row["parent"]
        spread = max(new["max_ms"] - new["min_ms"], old["max_ms"] - old["min_ms"])
        row["accepted"] = new["median_ms"] <= old["median_ms"] + spread
        row["tie"] = abs(new["median_ms"] - old["median_ms"]) <= spread
        results.append(row)
        del flags
    t.export_release()

    # ---- 2. mergeFrom on the group against merge_table alone
    ids = torch.nonzero(u < 0.01).flatten().to(torch.int32)
    m = int(ids.numel())
    rk = torch.zeros(m, dtype=torch.int32, device="cuda")
    val = torch.randint(0, POOL, (m,), device="cuda", generator=g, dtype=torch.int32)
    tick = [0]

    def delta():
        """Newer rows for the ~1 % ids in a; returns (since, wall) of the merge that takes them."""
        tick[0] += 1
        wall = WALL + 100 * tick[0]
        stamp = torch.full((m,), wall << 16, dtype=torch.int64, device="cuda")
        t.put_rows(ids, stamp, rk, val, stamp)
        return wall << 16, wall

    from crdt_amd import Hlc

    def table_alone(since, wall):
        return b._table.merge_table(t, n_rows, since, wall)

    def merge_from(since, wall):
        return b.mergeFrom(a, modifiedSince=Hlc.fromLogicalTime(since, "a"), wall=wall)

    def merge_from_watched(since, wall):
        w = b.watch()
        try:
            b.mergeFrom(a, modifiedSince=Hlc.fromLogicalTime(since, "a"), wall=wall)
        finally:
            b._watches.remove(w)                         # (the other legs run without a watch)
        return w

    mlegs = (("merge_table", table_alone), ("mergeFrom", merge_from), ("mergeFrom_watched", merge_from_watched))
    mtimes = {name: [] for name, _ in mlegs}
    for rep in range(args.repeats + 1):                  # the first round is the warm-up
        for name, fn in mlegs:
            since, wall = delta()
            ms, got = timed(lambda: fn(since, wall))
            if name == "mergeFrom_watched":
                assert b.last_sync == "table" and b.last_sync_winners == len(got.events) == m
            elif name == "mergeFrom":
                assert b.last_sync == "table" and b.last_sync_winners is None
            else:
                assert got[0]["status"] == 0 and got[0]["n_won"] == m
            del got
            if rep:
                mtimes[name].append(ms)
    merge = {"winners": m}
    for name, _ in mlegs:
        merge[name] = summary(mtimes[name])

    out = {"bench": "events", "rows": n_rows, "row_bytes": args.row_bytes, "table_bytes": n_rows * args.row_bytes,
           "repeats": args.repeats, "tile_rows": _capi.EXPORT_TILE, "legs": results, "merge": merge}
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
