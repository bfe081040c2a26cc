#!/usr/bin/env python3
"""The group diff on the device tables (crdt_diff_group) on one GPU, beside the existing passes it is measured
against, timed in the same process on the same tables.

    python tools/groupdiff_bench.py [--rows-log2 27] [--row-bytes 24] [--repeats 5] [--out FILE]

Legs: 2, 4 and 8 members, converged and with 1 % of the rows disputed (on such a row one member, rotating with the
row id, holds an lt one millisecond lower), each without and with the three arrays (device memory).  The call
writes no table, so nothing is rebuilt between the repeats.  Every call is synchronous, so a host clock around it
is the call's time.  Per leg one warm-up call, whose counts must be what the fill implies; then the repeats,
reported as median, minimum and maximum.

Yardsticks, not enforced: the sum of the members' ``digest_rows`` times (one full read of every table, existing
code, the bytes the pass moves without its arrays); the spread between the digest repeats is the margin
("within_digest_sum").  And ``n - 1`` ``diff_table`` calls against member 0, which read ``2 (n - 1)`` tables and
answer less.  Prints one JSON line."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WALL = 1_700_000_000_000
MEMBERS = (2, 4, 8)
SHARES = (0.0, 0.01)
POOL = 1024


def fill(table, u, share: float, n_rows: int, member: int, members: int, chunk: int = 1 << 24):
    """Every row visible and the same in every member, but where u[i] < share: there member i % members holds an
    lt 65536 lower (one millisecond)."""
    import torch
    for first in range(0, n_rows, chunk):
        key = torch.arange(first, min(first + chunk, n_rows), dtype=torch.int64, device="cuda")
        mod = torch.full_like(key, WALL << 16)
        lt = mod - 1 - (key * 40503 % 65536)
        val = (key * 2654435761 % POOL).to(torch.int32)
        lt[(u[first:first + len(key)] < share) & (key % members == member)] -= 65536
        table.put_rows(key.to(torch.int32), lt, torch.zeros_like(val), val, mod)


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
        sys.exit("groupdiff_bench: no gfx950 device (these figures cannot be taken without one)")
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
    ids = torch.arange(n_rows, dtype=torch.int64, device="cuda")
    arrays = tuple(torch.zeros(n_rows, dtype=torch.uint8, device="cuda") for _ in range(3))
    torch.cuda.synchronize()

    legs = []
    for share in SHARES:
        for m in MEMBERS:
            ts = tables[:m]
            for j, t in enumerate(ts):
                fill(t, u, share, n_rows, j, m)
            torch.cuda.synchronize()
            dg = []
            for t in ts:
                t.digest_rows(n_rows)
                dg.append(summary([timed(lambda: t.digest_rows(n_rows))[0] for _ in range(args.repeats)]))
            spread = max(s["max_ms"] - s["min_ms"] for s in dg)
            # warm-up, checked: the counts and the arrays the fill implies
            d, behind, hold, conflict = ts[0].diff_group(ts[1:], n_rows, masks=arrays)
            picked = u < share
            per = [int((picked & (ids % m == j)).sum().item()) for j in range(m)]
            pad = [0] * (_capi.GROUP_MAX - m)
            sole = [per[1], per[0]] if m == 2 else [0] * m
            want = {"n_held": n_rows, "n_disputed": sum(per), "n_conflict": 0, "n_visible": [n_rows] * m + pad,
                    "n_behind": per + pad, "n_sole": sole + pad}
            assert {k: d[k] for k in want} == want, (m, share, d, want)
            assert (d["first_diff"] == _capi.DIFF_NONE) == (sum(per) == 0)
            assert int(torch.count_nonzero(behind).item()) == sum(per) and not conflict.any().item()
            assert torch.equal((hold | behind), torch.full_like(hold, (1 << m) - 1))
            assert ts[0].diff_group(ts[1:], n_rows)[0] == d
            plain = [timed(lambda: ts[0].diff_group(ts[1:], n_rows))[0] for _ in range(args.repeats)]
            masks = [timed(lambda: ts[0].diff_group(ts[1:], n_rows, masks=arrays))[0] for _ in range(args.repeats)]
            for t in ts[1:]:
                ts[0].diff_table(t, n_rows)
            pairs = [sum(timed(lambda: ts[0].diff_table(t, n_rows))[0] for t in ts[1:]) for _ in range(args.repeats)]
            row = {"members": m, "share_disputed": share, "disputed_rows": sum(per), "diff_group": summary(plain),
                   "diff_group_masks": summary(masks), "digest_rows": dg,
                   "digest_sum_ms": round(sum(s["median_ms"] for s in dg), 3), "digest_spread_ms": round(spread, 3),
                   "pairwise_diff_table": summary(pairs)}
            row["within_digest_sum"] = row["diff_group"]["median_ms"] <= row["digest_sum_ms"] + row["digest_spread_ms"]
            row["diff_group_gbs"] = round(m * n_rows * rb / row["diff_group"]["median_ms"] / 1e6, 1)
            row["diff_group_masks_gbs"] = round((m * rb + 3) * n_rows / row["diff_group_masks"]["median_ms"] / 1e6, 1)
            legs.append(row)
    for t in tables:
        t.close()

    out = {"bench": "groupdiff", "rows": n_rows, "row_bytes": rb, "table_bytes": n_rows * rb, "repeats": args.repeats,
           "tile_rows": _capi.TABLE_TILE, "legs": legs,
           "not_measured": ["32-B rows" if rb == 24 else "24-B rows", "mixed row sizes", "arrays in host memory",
                            "conflicts", "invisible rows", "MapCrdt.groupDiff"]}
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
