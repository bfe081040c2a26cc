"""The replica network of tests/_replica_net.py on DeviceTables: four contexts play a seeded schedule of
every table operation in lockstep with four replicas on the C restatement, and after EVERY op the call's
results, flags, plan, every row of every table involved and the canonicals must equal the model's.  What
one call leaves for a different call on a different context (high-water marks, canonical chains,
per-context settings, rows written from another context's stream, shared scratch) is what this walk sees
and the one-call tests cannot.  tests/test_replica_net_cpu.py checks the schedule itself.

A failure names (seed, step, op) and the last five ops; ``tests._replica_net.replay(seed, step)`` rebuilds
the model's state before the failing op.  Everything is integer data: every comparison is exact."""
import numpy as np
import pytest

import tests.test_gpu_export as gx
from crdt_amd import CrdtNativeError, DeviceTable
from tests import _replica_net as rn

pytestmark = pytest.mark.gpu

K = rn.K
U64_MAX = rn.U64_MAX
RESULT_FIELDS = rn.tc.RESULT_FIELDS
CHECK_EVERY = 8


def _host(a):
    if a is None:
        return None
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def _dev(a):
    """A numpy column as a tensor on the GPU (uint32 columns travel as int32: the same bits)."""
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to("cuda:0")


class DeviceReplica:
    """A DeviceTable under the method names of tests/_replica_net.OracleReplica."""

    def __init__(self, r: int):
        self.t = DeviceTable(0, local_rank=r, capacity=rn.CAPS[r])
        if rn.ROW_BYTES[r] != 24:
            self.t.set_row_bytes(rn.ROW_BYTES[r])
        assert self.t.capacity == rn.CAPS[r]
        self.counts_off = False

    capacity = property(lambda self: self.t.capacity)
    canonical = property(lambda self: self.t.canonical)

    def all_rows(self):
        return self.t.read_rows(np.arange(self.t.capacity, dtype=np.uint32))

    def _flags_arg(self, kind):
        return {"host": np.full(K, 9, np.uint8), "device": True, "none": False}[kind]

    def _counted(self) -> bool:
        """Did the last crdt_merge on this context report per-record counts?  (crdt_set_counts: not when
        its order-free sorted form ran.)"""
        plan = self.t.last_plan()
        return not (self.counts_off and plan["sorted"] and not plan["flagged"])

    def do_put(self, ids, val, wall, mem):
        if mem == "device":
            ids, val = _dev(ids), _dev(val)
        return self.t.put_stamped(ids, val, wall)

    def do_merge_table(self, src, since, wall, flags):
        res, fl = self.t.merge_table(src.t, K, since, wall, row_flags=self._flags_arg(flags))
        return res, _host(fl)

    def do_merge_from(self, src, since, wall):
        res, fl = self.t.merge_from(src.t, K, since, wall)
        return res, _host(fl)

    def do_sync_tables(self, other, since_self, since_other, wall, flags):
        (ra, fa), (rb, fb) = self.t.sync_tables(other.t, K, since_self, since_other, wall,
                                                row_flags=(self._flags_arg(flags), self._flags_arg(flags)))
        return (ra, _host(fa)), (rb, _host(fb))

    def do_merge_tables(self, srcs, sinces, wall, flags):
        res, mask = self.t.merge_tables([s.t for s in srcs], K, sinces, wall, win_mask=self._flags_arg(flags))
        return res, _host(mask)

    def do_merge(self, key, lt, rank, val, offsets, wall, mem, flags):
        if mem == "device":
            key, lt, rank, val = _dev(key), _dev(lt), _dev(rank), _dev(val)
        res, fl = self.t.merge(key, lt, rank, val, offsets, wall, win_flags=flags != "none")
        return res, _host(fl)

    def do_clear_rows(self, first, count):
        self.t.clear_rows(first, count)

    def do_refresh_canonical(self):
        return self.t.refresh_canonical(K)

    def do_remap_ranks(self, lut, local_rank, bound):
        self.t.remap_ranks(K, lut)
        self.t.local_rank = local_rank

    def do_reserve(self, capacity, new_capacity):
        self.t.reserve(capacity)
        assert self.t.capacity == new_capacity

    def do_setting(self, op):
        kind = op["op"]
        if kind == "set_row_bytes":
            self.t.set_row_bytes(op["row_bytes"])
        elif kind == "set_merge_path":
            self.t.set_merge_path(op["path"])
        elif kind == "set_rank_bound":
            self.t.set_rank_bound(op["bound"])
        else:
            assert kind == "set_counts"
            self.t.set_counts(op["exact"])
            self.t.set_rank_bound(op["bound"])
            self.counts_off = not op["exact"]


class Walk:
    def __init__(self, seed: int, ops=None):
        self.seed = seed
        self.ops, self.n_walk = rn.schedule(seed) if ops is None else (ops, len(ops))
        self.dev = [DeviceReplica(r) for r in range(rn.N)]
        self.net = rn.Net(self.dev, self.compare)
        self.rng = np.random.default_rng([seed, 0xC4EC])
        self.reported = {f: 0 for f in rn.TABLE_FORMS}            # calls the library reports as fused
        self.uncounted = 0                                        # results whose counts had to be 2^64 - 1

    def close(self):
        for d in self.dev:
            d.t.close()

    # -- comparisons
    def same_result(self, got, want, counted, tag):
        for f in RESULT_FIELDS:
            w = want[f]
            if f in ("n_present", "n_won") and counted is not True:
                if counted is False:
                    w = U64_MAX
                    self.uncounted += 1
                else:                                             # (either: see merge_tables below)
                    assert got[f] in (w, U64_MAX) and (got["n_present"] == U64_MAX) == (got["n_won"] == U64_MAX), \
                        (tag, f, got[f], w)
                    continue
            assert got[f] == w, (tag, f, got[f], w)

    def same_table(self, r, tag):
        d, m = self.dev[r], self.net.model[r]
        assert d.capacity == m.capacity, (tag, r, "capacity")
        for name, a, b in zip(rn.COLS, d.all_rows(), m.all_rows()):
            assert np.array_equal(a, b), (tag, "replica", r, name, np.flatnonzero(a != b)[:8])
        assert d.canonical == m.canonical, (tag, "replica", r, "canonical", d.canonical, m.canonical)

    def same_flags(self, got, want, kind, tag):
        if kind == "none":
            assert got is None, tag
        else:
            assert got is not None and len(got) >= len(want) and np.array_equal(got[:len(want)], want), (tag, "flags")

    def compare(self, i, op, want, got, written, read, fused):
        kind = op["op"]
        dev = self.dev
        if kind == "put":
            self.same_result(got, want, True, kind)
        elif kind == "merge_table":
            d = dev[op["dst"]]
            if op["via"] == "from":
                self.same_result(got[0], want[0], d._counted(), kind)
                self.same_flags(got[1], want[1], "device", kind)
            else:
                plan = d.t.last_plan()
                assert plan["table"] is fused, (kind, "fused", fused, plan)
                self.reported[kind] += plan["table"]
                self.same_result(got[0], want[0], plan["table"] or d._counted(), kind)
                self.same_flags(got[1], want[1], op["flags"], kind)
        elif kind == "sync_tables":
            for side, r in ((0, op["a"]), (1, op["b"])):
                # composed: each context ran one merge of its own, unless step 1 raised: b is untouched then,
                # its plan still that of its last call
                ran = side == 0 or want[0][0]["status"] == 0
                plan = dev[r].t.last_plan()
                if ran:
                    assert plan["sync"] is fused, (kind, "ab"[side], "fused", fused, plan)
                self.same_result(got[side][0], want[side][0], not ran or plan["table"] or dev[r]._counted(),
                                 (kind, "ab"[side]))
                self.same_flags(got[side][1], want[side][1], op["flags"], (kind, "ab"[side]))
            self.reported[kind] += dev[op["a"]].t.last_plan()["sync"]
        elif kind == "merge_tables":
            d = dev[op["dst"]]
            plan = d.t.last_plan()
            assert plan["fanin"] is fused, (kind, "fused", fused, plan)
            self.reported[kind] += plan["fanin"]
            last = max((j for j, r in enumerate(want[0]) if r["n_stored"] or r["status"]), default=-1)
            for j, (g, w) in enumerate(zip(got[0], want[0])):
                # composed on a context whose counts are off: each step's crdt_merge reports counts or not by
                # the path IT took; the context remembers only the last step's
                counted = True if plan["fanin"] or not d.counts_off or j > last else (d._counted() if j == last else None)
                if not plan["fanin"] and plan["table"] and j == last:
                    counted = True                                # (the last step ran the fused merge_table)
                self.same_result(g, w, counted, (kind, "step", j))
            self.same_flags(got[1], want[1], op["flags"], kind)
        elif kind == "merge":
            self.same_result(got[0], want[0], dev[op["dst"]]._counted(), kind)
            self.same_flags(got[1], want[1], op["flags"], kind)
        elif kind in ("wipe", "refresh_canonical"):
            assert got == want, (kind, got, want)
        for r in written:
            self.same_table(r, (kind, "written"))
        for r in read:
            self.same_table(r, (kind, "source untouched"))

    # -- the periodic checks on a random replica
    def periodic(self, tag):
        r = int(self.rng.integers(rn.N))
        d, m = self.dev[r], self.net.model[r]
        mark = self.net.marks[r][int(self.rng.integers(rn.N))]
        for since in (0, mark, rn.I64_MIN):
            gx.check_export(d.t, m, K, since)
        c = d.canonical
        assert d.t.refresh_canonical(K) == m.refresh(K), (tag, "refresh_canonical", r)
        d.t.canonical = c

    def view_before(self):
        """An export view of a random replica and the model's snapshot of the same rows."""
        r = int(self.rng.integers(rn.N))
        m = self.net.model[r]
        ex = gx.check_export(self.dev[r].t, m, K, 0)
        ids = m.modified_since(K, 0)
        snap = (ids,) + tuple(m.rows[k][ids].copy() for k in rn.COLS)
        return r, ex, snap

    def view_after(self, op, view):
        """The view survives every call but a merge_from out of its table (that call exports again)."""
        r, ex, snap = view
        if op["op"] == "merge_table" and op["via"] == "from" and op["src"] == r:
            with pytest.raises(CrdtNativeError):
                ex.columns()
            return
        for name, a, b in zip(("key",) + rn.COLS, ex.columns(), snap):
            assert np.array_equal(a, b), ("export view read after the op", "replica", r, name)

    def run(self):
        ops = self.ops
        for i, op in enumerate(ops):
            try:
                view = self.view_before() if i % CHECK_EVERY == CHECK_EVERY - 1 else None
                self.net.step(i, op)
                if view is not None:
                    self.view_after(op, view)
                    self.periodic((i, "periodic"))
            except (AssertionError, CrdtNativeError) as e:
                last = "\n  ".join(f"{j}: {rn.brief(o)}" for j, o in list(enumerate(ops))[max(i - 4, 0):i + 1])
                raise AssertionError(f"seed {self.seed}, step {i} ({'walk' if i < self.n_walk else 'quiescence'}), "
                                     f"op {op['op']}: {e!r}\nlast ops:\n  {last}\n"
                                     f"replay: tests._replica_net.replay({self.seed}, {i})") from e
        for r in range(rn.N):
            self.same_table(r, "end")
        self.periodic("at the end")
        return self


def run_walk(seed):
    import time
    t0 = time.perf_counter()
    w = Walk(seed)
    try:
        w.run()
    finally:
        w.close()
    assert rn.converged(w.net.model) == []
    st = w.net.stats
    predicted = {f: st["fused"][f] for f in rn.TABLE_FORMS}
    assert w.reported == predicted, (w.reported, predicted)
    print(f"\nreplica net seed {seed}: {len(w.ops)} ops {dict(sorted(st['kinds'].items()))} "
          f"predicted fused {predicted} composed {st['composed']} reported fused {w.reported} "
          f"fanin_stops {st['fanin_stops']} in {time.perf_counter() - t0:.2f} s")


@pytest.mark.parametrize("seed", rn.SEEDS)
def test_replica_net(gpu_device, seed):
    run_walk(seed)


@pytest.mark.parametrize("seed", rn.SEEDS[:2])
def test_replica_net_poisoned_scratch(gpu_device, monkeypatch, seed):
    """The same walk with every scratch allocation of its contexts filled with 0x5A bytes."""
    monkeypatch.setenv("CRDT_ENV_DYNAMIC", "1")               # (read when a table is created)
    monkeypatch.setenv("CRDT_POISON_ALLOC", "1")
    run_walk(seed)


def test_counts_off_on_the_sorted_path(gpu_device):
    """No seed above has a destination whose counts are off AND whose merges are pinned to the sorted path in
    a call without flags (the settings are drawn independently); this hand-written schedule does, through the
    same runner: the composed merge_table, an external batch and the composed fan-in's last step must report
    n_present = n_won = 2^64 - 1, with every row as the model has it."""
    g = rn._Gen(100)
    for r in (1, 2, 0, 1):
        g.tick()
        g.put(r=r)
    g.counts_off[0] = True
    g.emit("set_counts", r=0, exact=False, bound=g.bound())
    g.emit("set_merge_path", r=0, path="sorted")
    for call in ("merge_table", "merge", "merge_tables"):
        g.tick()
        g.calls = 1                                               # (the next call's flags: none)
        if call == "merge_table":
            g.merge_table(dst=0, src=1, since=0, via="table")
        elif call == "merge":
            g.merge()
            g.ops[-1].update(dst=0, bad=None)
        else:
            g.merge_tables(dst=0, srcs=[2, 1, 2], zero=True)
        assert g.ops[-1]["flags"] == "none"
    w = Walk(100, g.ops)
    try:
        w.run()
    finally:
        w.close()
    assert w.uncounted == 2 * 3 and w.net.stats["composed"] == {"merge_table": 1, "sync_tables": 0, "merge_tables": 1}
