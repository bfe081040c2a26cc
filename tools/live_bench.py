#!/usr/bin/env python3
"""clear() and the live view on the device table on one GPU, against the routes there were before them, timed
in the same process on the same table.

    python tools/live_bench.py [--rows-log2 27] [--row-bytes 24] [--repeats 5] [--api-keys-log2 17] [--out FILE]

Tombstone legs: 100 % / 50 % / 1 % of the rows live.  The call consumes its input, so the table is rebuilt and
its canonical reset before every timed call, outside the timed region.  Routes:
  tombstone_live        the fused call without flags
  tombstone_live_flags  ... with device flags
  composition           (a) export_since(0), a torch filter on val, put_stamped with device ids
Every call is synchronous, so a host clock around it is the call's time (the composition's torch filter is
followed by a device synchronise inside put_stamped's hand-over).  Per leg every route runs once as a warm-up
and the routes must agree (result, canonical and the ROWS digest of the whole table); then they alternate
inside each repeat and the median, minimum and maximum are reported.  Expected, not enforced: the fused call
beats the composition at every share by more than the larger min-max spread ("beats_composition").

  (b) what MapCrdt.clear() did before this call existed, Crdt.clear's putAll over the Record-built map, at
  2^api-keys-log2 string keys (nothing is extrapolated from it), beside the new clear() on the same map.

Live-view legs: export_live against export_since(0) at the same three shares (the table is only read), each in
a block of repeats of its own after one call that sizes the ctx's column buffers.
Beside them, the read-only passes of this process on the same table: count_since and digest_rows.
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
SHARES = (1.0, 0.5, 0.01)
POOL = 1024


class _DevPtr:
    """A device column of an export as torch sees it (no copy): the CUDA array interface over its pointer."""

    def __init__(self, ptr: int, n: int, typestr: str):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": typestr, "data": (int(ptr), False), "version": 2}


def fill(table, u, share: float, n_rows: int, chunk: int = 1 << 24):
    """Row i: live iff u[i] < share, else a tombstone; every row visible, stamped below the canonical."""
    import torch
    for first in range(0, n_rows, chunk):
        key = torch.arange(first, min(first + chunk, n_rows), dtype=torch.int64, device="cuda")
        mod = torch.full_like(key, WALL << 16)
        lt = mod - (key * 40503 % 65536)
        val = (key * 2654435761 % POOL).to(torch.int32)
        val[u[first:first + len(key)] >= share] = -1         # CRDT_NULL_VALUE
        table.put_rows(key.to(torch.int32), lt, torch.zeros_like(val), val, mod)


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def summary(ms: list) -> dict:
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}


def spread(*s) -> float:
    return max(x["max_ms"] - x["min_ms"] for x in s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows-log2", type=int, default=27)
    ap.add_argument("--row-bytes", type=int, choices=[24, 32], default=24)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--api-keys-log2", type=int, default=17)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()

    import torch

    from crdt_amd import DeviceTable, MapCrdt, _capi
    from crdt_amd.crdt import Crdt
    if _capi.device_count() < 1:
        sys.exit("live_bench: no gfx950 device (these figures cannot be taken without one)")
    n_rows = 1 << args.rows_log2
    t = DeviceTable(0, local_rank=3, capacity=n_rows)
    if args.row_bytes != 24:
        t.set_row_bytes(args.row_bytes)
    g = torch.Generator(device="cuda")
    g.manual_seed(args.seed)
    u = torch.rand(n_rows, device="cuda", generator=g)
    dflags = torch.zeros(n_rows, dtype=torch.uint8, device="cuda")
    c0, wall = (WALL << 16) + 7, WALL + 5
    torch.cuda.synchronize()

    def composition():
        ex = t.export_since(n_rows, 0)
        if ex.n == 0:
            return t.put_stamped(np.zeros(0, np.uint32), np.zeros(0, np.uint32), wall)
        key = torch.as_tensor(_DevPtr(ex._view.key_id, ex.n, "<i4"), device="cuda")
        val = torch.as_tensor(_DevPtr(ex._view.val, ex.n, "<i4"), device="cuda")
        ids = key[val != -1]
        return t.put_stamped(ids, torch.full_like(ids, -1), wall)

    routes = {"tombstone_live": lambda: t.tombstone_live(n_rows, wall)[0],
              "tombstone_live_flags": lambda: t.tombstone_live(n_rows, wall, row_flags=dflags)[0],
              "composition": composition}

    def rebuilt(share):
        fill(t, u, share, n_rows)
        t.canonical = c0
        torch.cuda.synchronize()

    legs, views = [], []
    for share in SHARES:
        # ---- warm-up: every route once, and they agree
        seen = {}
        for name, fn in routes.items():
            rebuilt(share)
            res = fn()
            seen[name] = (res, t.canonical, t.digest_rows(n_rows).tolist())
        first = seen["composition"]
        assert all(v == first for v in seen.values()), (share, {k: v[:2] for k, v in seen.items()})
        n_live = first[0]["n_won"]
        assert int(dflags.sum().item()) == n_live
        times = {name: [] for name in routes}
        for _ in range(args.repeats):
            for name, fn in routes.items():
                rebuilt(share)
                ms, out = timed(fn)
                del out
                times[name].append(ms)
        row = {"share_live": share, "live_rows": n_live, **{k: summary(v) for k, v in times.items()}}
        for name in ("tombstone_live", "tombstone_live_flags"):
            sp = spread(row[name], row["composition"])
            row[f"{name}_beats_composition"] = row[name]["median_ms"] + sp < row["composition"]["median_ms"]
            moved = n_rows * args.row_bytes + n_live * args.row_bytes + (n_rows if name.endswith("flags") else 0)
            row[f"{name}_gbs"] = round(moved / row[name]["median_ms"] / 1e6, 1)
        legs.append(row)

        # ---- the live view on the rebuilt table (read-only legs)
        rebuilt(share)
        assert t.export_live(n_rows).n == n_live and t.export_since(n_rows, 0).n == n_rows
        # the two exports in blocks of their own, after one call that sizes the column buffers: alternated, a
        # small export gives the large one's buffers back and the large one allocates them again, every time
        vt = {"export_live": [], "export_since_0": [], "count_since": [], "digest_rows": []}
        for name, fn in (("export_live", lambda: t.export_live(n_rows)), ("export_since_0", lambda: t.export_since(n_rows, 0))):
            fn()
            vt[name] = [timed(fn)[0] for _ in range(args.repeats)]
        for _ in range(args.repeats):
            vt["count_since"].append(timed(lambda: t.count_since(n_rows, 0))[0])
            vt["digest_rows"].append(timed(lambda: t.digest_rows(n_rows))[0])
        t.export_release()
        views.append({"share_live": share, "live_rows": n_live, **{k: summary(v) for k, v in vt.items()}})
    t.close()
    del u, dflags

    # ---- (b) the MapCrdt-level clear() as it was (Crdt.clear over the Record-built map) and as it is
    n_keys = 1 << args.api_keys_log2
    values = {f"key{i:08d}": i for i in range(n_keys)}
    dead = {f"key{i:08d}": None for i in range(0, n_keys, 2)}
    api = {"keys": n_keys, "live_keys": n_keys - len(dead)}

    def fresh():
        m = MapCrdt("bench", capacity=n_keys, clock=lambda: WALL)
        m.putAll(values, wall=WALL)
        m.putAll(dead, wall=WALL + 1)
        return m

    def old_clear(m):
        m.putAll({k: None for k in Crdt.map.fget(m)}, wall=WALL + 2)

    at = {"old_clear": [], "clear": [], "old_map": [], "map": []}
    for rep in range(min(args.repeats, 3) + 1):          # (the first round is the warm-up)
        mo, mn = fresh(), fresh()
        m_old, m_new = timed(lambda: Crdt.map.fget(mo))[0], timed(lambda: mn.map)[0]
        c_old, c_new = timed(lambda: old_clear(mo))[0], timed(lambda: mn.clear(wall=WALL + 2))[0]
        assert mo.canonicalTime.logicalTime == mn.canonicalTime.logicalTime and mo.length == mn.length == 0
        assert mo._table.digest_rows(n_keys).tolist() == mn._table.digest_rows(n_keys).tolist()
        if rep:
            for k, v in (("old_clear", c_old), ("clear", c_new), ("old_map", m_old), ("map", m_new)):
                at[k].append(v)
        mo._table.close()
        mn._table.close()
    api.update({k: summary(v) for k, v in at.items()})

    out = {"bench": "live", "rows": n_rows, "row_bytes": args.row_bytes, "table_bytes": n_rows * args.row_bytes,
           "repeats": args.repeats, "tile_rows": _capi.TABLE_TILE, "tombstone": legs, "views": views, "api": api,
           "not_measured": ["32-B rows" if args.row_bytes == 24 else "24-B rows", "flags in host memory",
                            "the MapCrdt-level clear() above 2^%d keys" % args.api_keys_log2]}
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
