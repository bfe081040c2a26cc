#!/usr/bin/env python3
"""Tombstone collection on the device tables (crdt_purge_tombstones) on one GPU, beside the existing passes it is
measured against, timed in the same process on the same tables.

    python tools/purge_bench.py [--rows-log2 27] [--row-bytes 24] [--repeats 5] [--out FILE]

Legs: 1, 2 and 8 members x 1 % / 50 % / 100 % of the rows candidates, every candidate agreed (so every one is
purged in every member), and one leg with 50 % candidates all blocked by the LAST member (another rank on every
row), which writes nothing.  A purge consumes its input, so the members are rebuilt before every timed call,
outside the timed region; the blocked leg is not rebuilt.  Every call is synchronous, so a host clock around it
is the call's time.  Per leg one warm-up call, whose counts and the members' ROWS digests must be what the fill
implies (purged rows hold the never-written fill in every member: equal digests across members); then the
repeats, reported as median, minimum and maximum.

Yardsticks, not enforced: ``digest_rows`` of each member (one full read of one table, existing code) in the same
process; the spread between its repeats is the margin.  The pass reads no table more than once, so the blocked
leg should not exceed the sum of the members' digest times by more than that spread ("within_digest_sum"); and
the 1-member, 1 % leg sits beside ``tombstone_live`` at 1 % live (the same loads, the same kind of stores).
Prints one JSON line."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WALL = 1_700_000_000_000
BEFORE = WALL << 16                       # every tombstone's lt lies below it
MEMBERS = (1, 2, 8)
SHARES = (0.01, 0.5, 1.0)
POOL = 1024


def fill(table, u, share: float, n_rows: int, rank: int = 0, tomb: bool = True, chunk: int = 1 << 24):
    """Row i: a tombstone (tomb) or a live row (not tomb) iff u[i] < share, else the other; every row visible."""
    import torch
    for first in range(0, n_rows, chunk):
        key = torch.arange(first, min(first + chunk, n_rows), dtype=torch.int64, device="cuda")
        mod = torch.full_like(key, WALL << 16)
        lt = mod - 1 - (key * 40503 % 65536)
        val = (key * 2654435761 % POOL).to(torch.int32)
        picked = u[first:first + len(key)] < share
        val[picked if tomb else ~picked] = -1                # CRDT_NULL_VALUE
        table.put_rows(key.to(torch.int32), lt, torch.full_like(val, rank), val, mod)


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
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()

    import torch

    from crdt_amd import DeviceTable, _capi
    if _capi.device_count() < 1:
        sys.exit("purge_bench: no gfx950 device (these figures cannot be taken without one)")
    n_rows, rb = 1 << args.rows_log2, args.row_bytes
    tables = []
    for j in range(max(MEMBERS)):
        t = DeviceTable(0, local_rank=8 + j, capacity=n_rows)
        if rb != 24:
            t.set_row_bytes(rb)
        tables.append(t)
    g = torch.Generator(device="cuda")
    g.manual_seed(args.seed)
    u = torch.rand(n_rows, device="cuda", generator=g)
    dflags = torch.zeros(n_rows, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def rebuilt(ts, share, last_rank=0):
        for j, t in enumerate(ts):
            fill(t, u, share, n_rows, rank=last_rank if j == len(ts) - 1 else 0)
        torch.cuda.synchronize()

    def digests(ts) -> tuple[list, float]:
        """(per member summary of digest_rows, the largest min-max spread among them)."""
        out = []
        for t in ts:
            t.digest_rows(n_rows)
            out.append(summary([timed(lambda: t.digest_rows(n_rows))[0] for _ in range(args.repeats)]))
        return out, max(s["max_ms"] - s["min_ms"] for s in out)

    legs = []
    for m in MEMBERS:
        ts = tables[:m]
        for share in SHARES:
            rebuilt(ts, share)
            dg, sp = digests(ts)
            res, _ = ts[0].purge_tombstones(ts[1:], n_rows, BEFORE, row_flags=dflags)      # warm-up, checked
            n_cand = int((u < share).sum().item())
            assert res == {"n_candidates": n_cand, "n_purged": n_cand}, (m, share, res, n_cand)
            assert int(dflags.sum().item()) == n_cand
            first = ts[0].digest_rows(n_rows).tolist()
            assert all(t.digest_rows(n_rows).tolist() == first for t in ts[1:])
            assert ts[0].purge_tombstones(ts[1:], n_rows, BEFORE)[0] == {"n_candidates": 0, "n_purged": 0}
            times = {"purge": [], "purge_flags": []}
            for _ in range(args.repeats):
                for name, rf in (("purge", False), ("purge_flags", dflags)):
                    rebuilt(ts, share)
                    times[name].append(timed(lambda: ts[0].purge_tombstones(ts[1:], n_rows, BEFORE, row_flags=rf))[0])
            row = {"members": m, "share_candidates": share, "purged_rows": n_cand,
                   **{k: summary(v) for k, v in times.items()},
                   "digest_rows": dg, "digest_sum_ms": round(sum(s["median_ms"] for s in dg), 3),
                   "digest_spread_ms": round(sp, 3)}
            # member 0 read whole, the others at the candidates' lines (at most whole), the purged rows stored
            moved = n_rows * rb + (m - 1) * min(n_cand * 128, n_rows * rb) + m * n_cand * rb
            row["purge_gbs"] = round(moved / row["purge"]["median_ms"] / 1e6, 1)
            legs.append(row)

    # ---- 50 % candidates, all blocked by the last member: nothing is written, so nothing is rebuilt
    blocked = []
    for m in (2, 8):
        ts = tables[:m]
        rebuilt(ts, 0.5, last_rank=1)
        dg, sp = digests(ts)
        before = [t.digest_rows(n_rows).tolist() for t in ts]
        n_cand = int((u < 0.5).sum().item())
        res, _ = ts[0].purge_tombstones(ts[1:], n_rows, BEFORE, row_flags=dflags)
        assert res == {"n_candidates": n_cand, "n_purged": 0} and int(dflags.sum().item()) == 0, res
        assert [t.digest_rows(n_rows).tolist() for t in ts] == before
        ms = [timed(lambda: ts[0].purge_tombstones(ts[1:], n_rows, BEFORE))[0] for _ in range(args.repeats)]
        row = {"members": m, "share_candidates": 0.5, "purged_rows": 0, "purge": summary(ms), "digest_rows": dg,
               "digest_sum_ms": round(sum(s["median_ms"] for s in dg), 3), "digest_spread_ms": round(sp, 3)}
        row["within_digest_sum"] = row["purge"]["median_ms"] <= row["digest_sum_ms"] + row["digest_spread_ms"]
        blocked.append(row)

    # ---- beside the 1-member, 1 % leg: tombstone_live at 1 % live on the same table
    t = tables[0]
    live = []
    for _ in range(args.repeats + 1):                    # (the first round is the warm-up)
        fill(t, u, 0.01, n_rows, tomb=False)
        t.canonical = (WALL << 16) + 7
        torch.cuda.synchronize()
        ms, (res, _) = timed(lambda: t.tombstone_live(n_rows, WALL + 5))
        assert res["n_won"] == int((u < 0.01).sum().item())
        live.append(ms)
    for t in tables:
        t.close()

    out = {"bench": "purge", "rows": n_rows, "row_bytes": rb, "table_bytes": n_rows * rb, "repeats": args.repeats,
           "tile_rows": _capi.TABLE_TILE, "agreed": legs, "blocked": blocked,
           "tombstone_live_1pct": summary(live[1:]),
           "not_measured": ["32-B rows" if rb == 24 else "24-B rows", "mixed row sizes", "flags in host memory",
                            "candidates partly blocked", "MapCrdt.purgeDeleted"]}
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
