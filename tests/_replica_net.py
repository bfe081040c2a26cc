"""A replica network played as a seeded schedule of every table operation (test helper; numpy and the C
restatement only, nothing here imports the library).

Four replicas (local ranks 0..3) share one id space of K = 5 tiles + 9 rows in tables of different capacities
and row sizes.  ``schedule(seed)`` yields a list of plain-data ops: stamped puts, the three table forms
(merge_table / sync_tables / merge_tables) at delta, zero and INT64_MIN sinces, external batches (some with a
record that raises), range clears, wipes (a restored replica that kept its node id), refresh_canonical, rank
remaps, and the per-context settings that change which form a later call takes.  ``Net`` plays the list on
``OracleReplica`` objects (the model: every compared value comes from the compositions of
tests/_table_cases.py) and, in lockstep, on any second list of replicas with the same method names
(tests/test_gpu_replica_net.py wraps DeviceTable); ``Net.check`` is the comparison hook.  From the model's
state alone ``Net`` predicts whether each table-form call runs fused (the header's conditions, through
tests/_sync_cases.model and tests/_fanin_cases.model).

A failure is replayed with ``replay(seed, upto)``: the model's state after ops[0 .. upto).

Rules that make convergence a property of the reference (tests/test_replica_net_cpu.py measures them):
  - an external record's value is a fixed function of (key, lt, rank): equal clocks never carry different values;
  - a wipe advances the wall by 10 ms (external clocks run at most 7 ms ahead), so a wiped node's new stamps
    never equal its old ones; for the same reason the wall moves on after the echo scenario and before the
    closing puts;
  - every replica closes with one put (it lifts a wiped replica's canonical past its old stamps).

The echo scenario.  A step j > 0 of a merge_tables call can raise only on a row of dst's own node id above the
canonical that step j - 1's Hlc.send left, and send lifts the canonical to the wall: after a wipe (10 ms) no such
row exists, so the op forced after a wipe stops at step 0 or not at all.  The scenario builds the case from
ordinary ops at one wall value: X puts twice in one window, Y merges X, X clears the window and refreshes its
canonical (purge + refreshCanonicalTime), then X merges [Z, Y, ...]: Z's rows are older than the wall, step 0's
send leaves (wall, 0), and Y returns X's second stamp (wall, 1): DuplicateNode at step 1."""
from __future__ import annotations

import numpy as np

from oracle.oracle_c import OracleTable, new_table
from tests import _fanin_cases as fc
from tests import _sync_cases as sc
from tests import _table_cases as tc
from tests._cases import NULL, WALL

N = 4
T = sc.SHAPES_T
K = 5 * T + 9
CAPS = (K, K + 777, 2 * K, K + 1)
ROW_BYTES = (24, 32, 24, 24)
N_EXT = 5                                  # external node ids, ranks N .. N + 4 at the start
I64_MIN = tc.I64_MIN
U64_MAX = tc.U64_MAX
COLS = fc.COLS
FILL_RANK = 0x80808080                     # the rank of a never-written row (an INT64_MIN since selects those)
SEEDS = tuple(range(8))
N_OPS = 160
PATHS = ("auto", "gather", "sorted")
FLAG_KINDS = ("host", "device", "none")
TABLE_FORMS = ("merge_table", "sync_tables", "merge_tables")

WEIGHTS = {"put": 0.245, "merge_table": 0.20, "sync_tables": 0.20, "merge_tables": 0.10, "merge": 0.13,
           "clear_rows": 0.02, "wipe": 0.035, "refresh_canonical": 0.01, "remap_ranks": 0.01,
           "set_row_bytes": 0.0125, "reserve": 0.0125, "set_merge_path": 0.0125, "set_counts": 0.0125}
ECHO_AFTER_WIPE = 0.3                      # how often the echo scenario follows a wipe's forced op


def ext_val(key, lt, rank):
    """The value of an external record: a fixed function of (key, lt, rank), ~15 % tombstones."""
    h = (key.astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)) ^ (lt.astype(np.uint64) * np.uint64(0xC2B2AE3D27D4EB4F))
    h ^= rank.astype(np.uint64) * np.uint64(0x165667B19E3779F9)
    h ^= h >> np.uint64(29)
    h *= np.uint64(0xBF58476D1CE4E5B9)
    h ^= h >> np.uint64(32)
    val = (h & np.uint64(0xFFFFF)).astype(np.uint32)
    val[(h >> np.uint64(40)) % np.uint64(100) < np.uint64(15)] = NULL
    return val


# ------------------------------------------------------------------ the schedule
class _Gen:
    def __init__(self, seed: int):
        self.rng = np.random.default_rng([seed, 0x5EED])
        self.wall = WALL
        self.local = list(range(N))                    # live rank of each replica
        self.ext = list(range(N, N + N_EXT))           # live ranks of the external nodes
        self.caps = list(CAPS)
        self.row_bytes = list(ROW_BYTES)
        self.path = [0] * N
        self.counts_off = [False] * N
        self.reserved = [False] * N
        self.remaps = 0
        self.leaked = False                            # an INT64_MIN since has made the fill's rank a live one
        self.calls = 0                                 # flag-memory cycle
        self.tables = 0                                # merge_table calls (every fifth goes through merge_from)
        self.merges = 0                                # external batches (host / device columns alternate)
        self.puts = 0
        self.ops = []

    # -- pieces
    def tick(self, lo=0, hi=3):
        self.wall += int(self.rng.integers(lo, hi))
        return self.wall

    def flags(self):
        self.calls += 1
        return FLAG_KINDS[self.calls % 3]

    def others(self, r):
        return [x for x in range(N) if x != r]

    def bound(self):
        return FILL_RANK + 1 if self.leaked else max(self.local + self.ext) + 1

    def bounds(self):
        """The rank bound the host keeps promised on the replicas whose counts are off."""
        return [self.bound() if off else None for off in self.counts_off]

    def emit(self, op, **kw):
        self.ops.append(dict(op=op, wall=self.wall, **kw))

    # -- ops
    def put(self, r=None, window=None, base=None):
        rng = self.rng
        r = int(rng.integers(N)) if r is None else r
        if window is None:
            window = rng.random() < 0.5
        if window:
            base = int(rng.integers(0, K - 300)) if base is None else base
            ids = base + rng.permutation(300)[:int(rng.integers(1, 200))]
        else:
            ids = rng.permutation(K)[:int(rng.integers(1, 500))]
        val = rng.integers(0, 1 << 20, len(ids)).astype(np.uint32)
        val[rng.random(len(ids)) < 0.15] = NULL
        self.puts += 1
        self.emit("put", r=r, ids=ids.astype(np.uint32), val=val, mem=("host", "device")[self.puts % 2])

    def merge_table(self, dst=None, src=None, since=None, via=None):
        rng = self.rng
        dst = int(rng.integers(N)) if dst is None else dst
        src = int(rng.choice(self.others(dst))) if src is None else src
        if since is None:
            since = ("mark", 0, I64_MIN)[int(rng.choice(3, p=[0.6, 0.3, 0.1]))]
        self.tables += 1
        kw = {}
        if since == I64_MIN and not self.leaked:
            self.leaked = True
            kw["bounds"] = self.bounds()               # (before the call: its changeset holds the fill's rank)
        self.emit("merge_table", dst=dst, src=src, since=since, flags=self.flags(),
                  via=via or ("from" if self.tables % 5 == 0 else "table"), **kw)

    def sync_tables(self, a=None, b=None, since=None):
        rng = self.rng
        a = int(rng.integers(N)) if a is None else a
        b = int(rng.choice(self.others(a))) if b is None else b
        if since is None:
            since = "mark" if rng.random() < 0.6 else 0
        self.emit("sync_tables", a=a, b=b, since=since, flags=self.flags())

    def merge_tables(self, dst=None, srcs=None, zero=False):
        rng = self.rng
        dst = int(rng.integers(N)) if dst is None else dst
        if srcs is None:
            srcs = [int(x) for x in rng.choice(self.others(dst), int(rng.integers(2, 9)))]
        sinces = [0 if zero or rng.random() < 0.5 else "mark" for _ in srcs]
        self.emit("merge_tables", dst=dst, srcs=srcs, since=sinces, flags=self.flags())

    def merge(self):
        rng = self.rng
        dst = int(rng.integers(N))
        keys, lts, ranks, offsets = [], [], [], [0]
        for _ in range(int(rng.integers(1, 4))):
            n = int(rng.integers(0, 400))
            keys.append(rng.permutation(K)[:n].astype(np.uint32))
            lts.append(((self.wall + rng.integers(-50, 8, n)) << 16) + rng.integers(0, 3, n))
            ranks.append(np.asarray(self.ext, np.uint32)[rng.integers(0, N_EXT, n)])
            offsets.append(offsets[-1] + n)
        bad = None
        if rng.random() < 0.1 and offsets[-1] > 0:
            bad = ("dup" if rng.random() < 0.5 else "drift", int(rng.integers(offsets[-1])))
        self.merges += 1
        self.emit("merge", dst=dst, key=np.concatenate(keys), lt=np.concatenate(lts).astype(np.int64),
                  rank=np.concatenate(ranks), offsets=np.array(offsets, np.uint64), bad=bad,
                  mem=("host", "device")[self.merges % 2], flags=self.flags())

    def clear_rows(self, r=None, first=None, count=None):
        rng = self.rng
        r = int(rng.integers(N)) if r is None else r
        if first is None:
            count = int(rng.integers(1, 3001))
            first = int(rng.integers(0, K - count + 1))
        self.emit("clear_rows", r=r, first=first, count=count)

    def wipe(self):
        rng = self.rng
        w = int(rng.integers(N))
        self.emit("wipe", r=w)
        self.wall += 10
        # the next op: a table form into the wiped replica at since 0 (the reference's DuplicateNode case)
        self.tick()
        form = int(rng.integers(3))
        if form == 0:
            self.merge_table(dst=w, since=0, via="table")
        elif form == 1:
            self.sync_tables(a=w, since=0)
        else:
            self.merge_tables(dst=w, zero=True)
        if rng.random() < ECHO_AFTER_WIPE:
            self.echo(w)

    def echo(self, w):
        """See the module docstring.  Y is not the wiped replica (it may be unable to merge yet)."""
        rng = self.rng
        self.tick()
        x = int(rng.integers(N))
        y = int(rng.choice([r for r in self.others(x) if r != w]))
        z = int(rng.choice([r for r in self.others(x) if r != y]))
        base = int(rng.integers(0, K - 300))
        self.put(r=x, window=True, base=base)
        self.put(r=x, window=True, base=base)
        self.merge_table(dst=y, src=x, since=0)
        self.clear_rows(r=x, first=base, count=300)
        self.emit("refresh_canonical", r=x)
        extra = [int(s) for s in rng.choice(self.others(x), int(rng.integers(0, 3)))]
        self.merge_tables(dst=x, srcs=[z, y] + extra, zero=True)
        self.wall += 1                                 # X's later stamps lie above the ones it no longer knows

    def remap_ranks(self):
        if self.remaps >= 2:
            return self.put()
        self.remaps += 1
        n_ranks = max(self.local + self.ext) + 1
        p = int(self.rng.integers(0, N + 6))
        lut = np.arange(n_ranks, dtype=np.uint32)
        lut[lut >= p] += 1
        self.local = [int(lut[r]) for r in self.local]
        self.ext = [int(lut[r]) for r in self.ext]
        self.emit("remap_ranks", lut=lut, local=list(self.local), bounds=self.bounds())

    def setting(self, kind):
        rng = self.rng
        r = int(rng.integers(N))
        if kind == "reserve" and self.reserved[r]:
            kind = "set_row_bytes"                     # (a table doubles at most once: the read-backs stay small)
        if kind == "set_row_bytes":
            self.row_bytes[r] = 56 - self.row_bytes[r]
            self.emit("set_row_bytes", r=r, row_bytes=self.row_bytes[r])
        elif kind == "reserve":
            want = self.caps[r] + int(rng.integers(1, 4097))
            self.caps[r] = max(want, 2 * self.caps[r])
            self.reserved[r] = True
            self.emit("reserve", r=r, capacity=want, new_capacity=self.caps[r])
        elif kind == "set_merge_path":
            self.path[r] = (self.path[r] + 1) % 3
            self.emit("set_merge_path", r=r, path=PATHS[self.path[r]])
        else:
            self.counts_off[r] = not self.counts_off[r]
            self.emit("set_counts", r=r, exact=not self.counts_off[r],
                      bound=self.bound() if self.counts_off[r] else 0)

    def run(self, n_ops):
        names = list(WEIGHTS)
        p = np.array([WEIGHTS[k] for k in names])
        p /= p.sum()
        while len(self.ops) < n_ops:
            self.tick()
            kind = names[int(self.rng.choice(len(names), p=p))]
            if kind.startswith("set_") or kind == "reserve":
                self.setting(kind)
            elif kind == "refresh_canonical":
                self.emit("refresh_canonical", r=int(self.rng.integers(N)))
            else:
                getattr(self, kind)()
        n_walk = len(self.ops)
        # quiescence: one put each, then two rounds of all ordered pairs at since 0
        self.wall += 1
        for r in range(N):
            self.put(r=r)
        for _ in range(2):
            for dst in range(N):
                for src in self.others(dst):
                    self.merge_table(dst=dst, src=src, since=0)
        return self.ops, n_walk


def schedule(seed: int, n_ops: int = N_OPS):
    """(ops, n_walk): the op list of a seed; ops[n_walk:] is the quiescence."""
    return _Gen(seed).run(n_ops)


# ------------------------------------------------------------------ the model's replica
class OracleReplica(OracleTable):
    """An OracleTable under the method names the runner calls (the DeviceTable adapter has the same)."""

    def __init__(self, capacity: int, local_rank: int):
        super().__init__(capacity, local_rank, 0)

    @property
    def capacity(self):
        return len(self.rows)

    def all_rows(self):
        return tuple(self.rows[k] for k in COLS)

    def do_put(self, ids, val, wall, mem):
        return self.put_stamped(ids, val, wall).as_dict()

    def do_merge_table(self, src, since, wall, flags):
        res, row_flags, _ = tc.oracle_merge_table(self, src, K, since, wall)
        return res, row_flags

    def do_merge_from(self, src, since, wall):
        res, rec_flags, _ = tc.oracle_merge_from(self, src, K, since, wall)
        return res, rec_flags

    def do_sync_tables(self, other, since_self, since_other, wall, flags):
        (ra, fa), (rb, fb) = tc.oracle_sync(self, other, K, since_self, since_other, wall)
        return (ra, fa), (rb, fb)

    def do_merge_tables(self, srcs, sinces, wall, flags):
        res, mask, _ = tc.oracle_fanin(self, srcs, K, sinces, wall)
        return res, mask

    def do_merge(self, key, lt, rank, val, offsets, wall, mem, flags):
        res, rec_flags = self.merge(key, lt, rank, val, offsets, wall)
        return res.as_dict(), rec_flags

    def do_clear_rows(self, first, count):
        self.rows[first:first + count] = new_table(count)

    def do_refresh_canonical(self):
        self.canonical = self.refresh(K)
        return self.canonical

    def do_remap_ranks(self, lut, local_rank, bound):
        r = self.rows["rank"][:K]
        m = r < len(lut)
        r[m] = lut[r[m]]
        self.local_rank = local_rank

    def do_reserve(self, capacity, new_capacity):
        grown = new_table(new_capacity)
        grown[:len(self.rows)] = self.rows
        self.rows = grown

    def do_setting(self, op):                          # row size, merge path, counts, rank bound: the library's own
        pass


# ------------------------------------------------------------------ the runner
def _dense(o, n=K):
    return {k: o.rows[k][:n].copy() for k in COLS}


class Net:
    """Plays ops on the model (``self.model``) and, if given, on ``self.other`` in lockstep.  After each op
    ``check(step, op, outcome of the model, outcome of the other, replicas written, replicas read)`` is called."""

    def __init__(self, other=None, check=None):
        self.model = [OracleReplica(CAPS[r], r) for r in range(N)]
        self.other = other
        self.check = check
        self.marks = [[0] * N for _ in range(N)]       # marks[dst][src]: src's canonical at dst's last clean merge of it
        self.pinned = [False] * N                      # merge path pinned to sorted
        self.counts_off = [False] * N
        self.stats = {"kinds": {}, "fused": {f: 0 for f in TABLE_FORMS}, "composed": {f: 0 for f in TABLE_FORMS},
                      "fanin_stops": 0, "select_nothing": 0, "sync_both": 0, "ext_raises": 0, "raises": 0}
        self.log = []                                  # (step, what the call was, predicted fused or None)

    # -- what an op means on the state as it is
    def since(self, s, dst, src):
        return self.marks[dst][src] if s == "mark" else int(s)

    def batch(self, op):
        """The external batch's columns: the op's, with its raising record (if any) made against dst's state."""
        key, lt, rank = op["key"], op["lt"].copy(), op["rank"].copy()
        if op["bad"] is not None:
            kind, i = op["bad"]
            dst = self.model[op["dst"]]
            if kind == "dup":                          # dst's node id, above its canonical and every record of the batch
                rank[i] = dst.local_rank
                lt[i] = (max(dst.canonical >> 16, op["wall"] + 8) + 1) << 16
            else:
                lt[i] = (op["wall"] + 60008) << 16
        return key, lt, rank, ext_val(key, lt, rank)

    def predict(self, op):
        """Does this table-form call run fused?  The header's conditions on the model's state."""
        m, wall = self.model, op["wall"]
        kind = op["op"]
        if kind == "merge_table":
            if op["via"] != "table":
                return None
            dst, src = m[op["dst"]], m[op["src"]]
            since = self.since(op["since"], op["dst"], op["src"])
            s = _dense(src)
            sel = ~(s["mod"] < since)
            cand = sc._may_raise(s["lt"], s["rank"], sel, dst.canonical, dst.local_rank, wall)
            return not (cand or self.pinned[op["dst"]] or op["dst"] == op["src"])
        if kind == "sync_tables":
            a, b = op["a"], op["b"]
            mod = sc.model(_dense(m[a]), _dense(m[b]), K, self.since(op["since"], b, a), self.since(op["since"], a, b),
                           m[a].canonical, m[b].canonical, wall, m[a].local_rank, m[b].local_rank)
            return bool(mod["fused"]) and not (self.pinned[a] or self.pinned[b] or a == b)
        if kind == "merge_tables":
            d = op["dst"]
            sinces = [self.since(s, d, j) for s, j in zip(op["since"], op["srcs"])]
            mod = fc.model(_dense(m[d]), [_dense(m[j]) for j in op["srcs"]], K, sinces, m[d].canonical, wall,
                           m[d].local_rank, dst_cap=m[d].capacity)
            return bool(mod["fused"]) and not (self.pinned[d] or d in op["srcs"])
        return None

    # -- one op on one list of replicas
    def apply(self, op, reps, cols=None):
        """Returns (outcome, written replica indices, read-only replica indices)."""
        kind, wall = op["op"], op["wall"]
        if op.get("bounds"):
            for r, b in enumerate(op["bounds"]):
                if b is not None:
                    reps[r].do_setting({"op": "set_rank_bound", "bound": b})
        if kind == "put":
            return reps[op["r"]].do_put(op["ids"], op["val"], wall, op["mem"]), [op["r"]], []
        if kind == "merge_table":
            d, s = op["dst"], op["src"]
            since = self.since(op["since"], d, s)
            if op["via"] == "from":
                return reps[d].do_merge_from(reps[s], since, wall), [d], [s]
            return reps[d].do_merge_table(reps[s], since, wall, op["flags"]), [d], [s]
        if kind == "sync_tables":
            a, b = op["a"], op["b"]
            out = reps[a].do_sync_tables(reps[b], self.since(op["since"], b, a), self.since(op["since"], a, b), wall,
                                         op["flags"])
            return out, [a, b], []
        if kind == "merge_tables":
            d = op["dst"]
            sinces = [self.since(s, d, j) for s, j in zip(op["since"], op["srcs"])]
            out = reps[d].do_merge_tables([reps[j] for j in op["srcs"]], sinces, wall, op["flags"])
            return out, [d], sorted(set(op["srcs"]))
        if kind == "merge":
            return reps[op["dst"]].do_merge(*cols, op["offsets"], wall, op["mem"], op["flags"]), [op["dst"]], []
        if kind == "clear_rows":
            return reps[op["r"]].do_clear_rows(op["first"], op["count"]), [op["r"]], []
        if kind == "wipe":
            r = reps[op["r"]]
            r.do_clear_rows(0, r.capacity)
            return r.do_refresh_canonical(), [op["r"]], []
        if kind == "refresh_canonical":
            return reps[op["r"]].do_refresh_canonical(), [op["r"]], []
        if kind == "remap_ranks":
            for r, rep in enumerate(reps):
                rep.do_remap_ranks(op["lut"], op["local"][r], None)
            return None, list(range(N)), []
        if kind == "reserve":
            return reps[op["r"]].do_reserve(op["capacity"], op["new_capacity"]), [op["r"]], []
        return reps[op["r"]].do_setting(op), [op["r"]], []

    # -- bookkeeping from the model's outcome
    def settle(self, op, out, canon_before, fused):
        kind, st = op["op"], self.stats
        st["kinds"][kind] = st["kinds"].get(kind, 0) + 1
        if fused is not None:
            st["fused" if fused else "composed"][kind] += 1
        if kind == "merge_table":
            res = out[0]
            if res["status"] == 0:
                self.marks[op["dst"]][op["src"]] = canon_before[op["src"]]
            else:
                st["raises"] += 1
            if op["via"] == "table" and res["status"] == 0 and res["n_present"] == 0 and res["n_won"] == 0 \
                    and not out[1].any():
                # nothing selected: no record present, none stored (a selected record is one or the other)
                st["select_nothing"] += 1
        elif kind == "sync_tables":
            (ra, _), (rb, _) = out
            a, b = op["a"], op["b"]
            if ra["status"] == 0:
                self.marks[a][b] = canon_before[b]
                if rb["status"] == 0:
                    self.marks[b][a] = canon_before[a]
            st["raises"] += int(ra["status"] != 0 or rb["status"] != 0)
            st["sync_both"] += int(ra["n_won"] > 0 and rb["n_won"] > 0)
        elif kind == "merge_tables":
            results = out[0]
            stop = next((j for j, r in enumerate(results) if r["status"] != 0), None)
            for j, (r, s) in enumerate(zip(results, op["srcs"])):
                if (stop is None or j < stop) and r["status"] == 0:
                    self.marks[op["dst"]][s] = canon_before[s]
            st["raises"] += int(stop is not None)
            st["fanin_stops"] += int(stop is not None and stop > 0)
        elif kind == "merge":
            st["ext_raises"] += int(out[0]["status"] != 0)
        elif kind == "wipe":
            self.marks[op["r"]] = [0] * N
        elif kind == "set_merge_path":
            self.pinned[op["r"]] = op["path"] == "sorted"
        elif kind == "set_counts":
            self.counts_off[op["r"]] = not op["exact"]

    def step(self, i, op):
        cols = self.batch(op) if op["op"] == "merge" else None
        fused = self.predict(op)
        canon_before = [m.canonical for m in self.model]
        want, written, read = self.apply(op, self.model, cols)
        if self.other is not None:
            got, _, _ = self.apply(op, self.other, cols)
            if self.check is not None:
                self.check(i, op, want, got, written, read, fused)
        self.settle(op, want, canon_before, fused)
        self.log.append((i, op["op"], fused, want))
        return want

    def run(self, ops, first=0):
        for i, op in enumerate(ops, first):
            self.step(i, op)
        return self


def replay(seed: int, upto: int | None = None, n_ops: int = N_OPS) -> Net:
    """The model after ops[0 .. upto) of the seed's schedule (all of it, the quiescence included, by default)."""
    ops, _ = schedule(seed, n_ops)
    return Net().run(ops[:upto])


def brief(op) -> str:
    """An op in one line (arrays by their length)."""
    parts = []
    for k, v in op.items():
        if k == "op":
            continue
        parts.append(f"{k}=<{len(v)}>" if isinstance(v, np.ndarray) else f"{k}={v}")
    return f"{op['op']}({', '.join(parts)})"


def converged(model) -> list:
    """The differences between the replicas' visible rows of [0, K): empty when they converged."""
    bad = []
    first = _dense(model[0])
    vis0 = first["mod"] >= 0
    for r in range(1, N):
        d = _dense(model[r])
        vis = d["mod"] >= 0
        if not np.array_equal(vis, vis0):
            bad.append((r, "visible", int(np.count_nonzero(vis != vis0))))
            continue
        for k in ("lt", "rank", "val"):
            if not np.array_equal(d[k][vis], first[k][vis0]):
                bad.append((r, k, int(np.count_nonzero(d[k][vis] != first[k][vis0]))))
    return bad
