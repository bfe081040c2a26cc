"""The key-sharded merge over a device-ordered transport with real peers (tests/_thread_comm.py): the
CRDT_MEM_DEVICE branch of comm_path.inc, the one RCCL takes, where a callback only enqueues work on the ctx
stream and correctness rests on the library's own stream and event dependencies.  G ranks are G threads of
this process, every rank holds its own part of the job, the transport lands its data late (lag) behind
poisoned receive ranges, and every row of every shard, the result fields and the win flags are compared with
the C oracle's unsharded merge.  A consumer that does not wait for its exchange reads poison here; under a
host-synchronous transport (dist.GlooComm) it would read correct bytes."""
import collections
import ctypes

import numpy as np
import pytest

from tests._cases import ABSENT_MOD, CASE_SPECS, oracle_run
from tests.test_gpu_parity import _make_injected, check_shards

pytestmark = pytest.mark.gpu

NOMEM = -3


# ------------------------------------------------------------------ a. the transport's own tests
def _bare(G=3, **kw):
    """A ThreadComm, one stream per rank and each rank's callback table (no library involved)."""
    import torch

    from tests._thread_comm import ThreadComm
    comm = ThreadComm(G, **kw)
    streams = [torch.cuda.Stream() for _ in range(G)]
    return comm, streams, [comm.rank(r).ops() for r in range(G)]


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _finish(comm):
    import torch
    torch.cuda.synchronize()
    assert comm.error is None, comm.error
    comm.close()


@pytest.mark.parametrize("n", [1, 1000])
@pytest.mark.parametrize("op", [0, 1, 2], ids=["sum", "max", "min"])
def test_transport_all_reduce(gpu_device, op, n):
    """SUM (wrapping past 2^63 as int64), signed MAX and MIN, in place, twice in a row on each stream (the
    second collective reuses the events and the scratch) against numpy."""
    import torch

    from tests._thread_comm import run_ranks
    G = 3
    comm, streams, ops = _bare(G)
    rng = np.random.default_rng(100 + 10 * op + n)
    lo, hi = np.iinfo(np.int64).min, np.iinfo(np.int64).max
    vals = [rng.integers(lo, hi, (G, n), dtype=np.int64, endpoint=True) for _ in range(2)]
    vals[0][:, 0] = (hi, hi, 5)                           # 2 * (2^63 - 1) + 5 wraps to 3
    vals[1][:, 0] = (lo, -1, hi)
    words = [[_dev(v[r]) for r in range(G)] for v in vals]
    torch.cuda.synchronize()

    def rank(r):
        for w in words:
            assert ops[r].all_reduce_i64(None, w[r].data_ptr(), n, op, streams[r].cuda_stream) == 0
    run_ranks(G, rank, comm)
    _finish(comm)
    with np.errstate(over="ignore"):
        want = [(np.sum, np.max, np.min)[op](v, axis=0) for v in vals]
    if op == 0:
        assert want[0][0] == 3
    for w, e in zip(words, want):
        for r in range(G):
            assert np.array_equal(w[r].cpu().numpy(), e), (r, op, n)


@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("n", [1, 17])
def test_transport_all_gather(gpu_device, n, in_place):
    import torch

    from tests._thread_comm import run_ranks
    G = 3
    comm, streams, ops = _bare(G)
    rng = np.random.default_rng(200 + n)
    vals = rng.integers(-1 << 62, 1 << 62, (G, n), dtype=np.int64)
    recv = [_dev(np.full(G * n, -7, np.int64)) for _ in range(G)]
    send = []
    for r in range(G):
        if in_place:
            recv[r][r * n:(r + 1) * n] = _dev(vals[r])
            send.append(recv[r][r * n:(r + 1) * n])
        else:
            send.append(_dev(vals[r]))
    torch.cuda.synchronize()

    def rank(r):
        assert send[r].data_ptr() == recv[r].data_ptr() + r * n * 8 or not in_place
        assert ops[r].all_gather_i64(None, send[r].data_ptr(), recv[r].data_ptr(), n, streams[r].cuda_stream) == 0
    run_ranks(G, rank, comm)
    _finish(comm)
    for r in range(G):
        assert np.array_equal(recv[r].cpu().numpy(), vals.reshape(-1)), r


SENTINEL = 0xA5


def _a2a_args(cols_send, cols_recv, eb, sc, sd, rc, rd):
    n = len(eb)
    return (n, (ctypes.c_void_p * n)(*[t.data_ptr() for t in cols_send]),
            (ctypes.c_void_p * n)(*[t.data_ptr() for t in cols_recv]), (ctypes.c_uint32 * n)(*eb),
            (ctypes.c_uint64 * len(sc))(*sc), (ctypes.c_uint64 * len(sc))(*sd), (ctypes.c_uint64 * len(sc))(*rc),
            (ctypes.c_uint64 * len(sc))(*rd))


def test_transport_all_to_all_v(gpu_device):
    """Three columns of 1-, 4- and 8-byte elements, ragged counts with zeros in both directions,
    displacements that are no multiple of 16 bytes, and an own-rank range (non-zero own counts, as a general
    all-to-all would pass) whose sentinel bytes must survive with every byte outside the peers' ranges."""
    import torch

    from tests._thread_comm import run_ranks
    G, eb = 3, (1, 4, 8)
    comm, streams, ops = _bare(G)
    rng = np.random.default_rng(300)
    cnt = np.array([[5, 0, 33], [7, 3, 1], [0, 129, 2]])         # cnt[s][d]: elements s sends d
    gap = (3, 1, 5)                                              # elements skipped before each range
    sd = [[int(sum(cnt[s][:d]) + sum(gap[:d + 1])) for d in range(G)] for s in range(G)]
    rd = [[int(sum(cnt[:s, d]) + sum(gap[:s + 1]) + 2) for s in range(G)] for d in range(G)]
    ns = [sd[s][-1] + int(cnt[s][-1]) + 4 for s in range(G)]
    nr = [rd[d][-1] + int(cnt[-1][d]) + 4 for d in range(G)]
    assert any((sd[s][d] * e) % 16 for s in range(G) for d in range(G) for e in eb)
    send_h = [[rng.integers(0, 200, ns[s] * e, dtype=np.uint8) for e in eb] for s in range(G)]
    send = [[_dev(c) for c in cols] for cols in send_h]
    recv = [[_dev(np.full(nr[d] * e, SENTINEL, np.uint8)) for e in eb] for d in range(G)]
    torch.cuda.synchronize()

    def rank(r):
        a = _a2a_args(send[r], recv[r], eb, [int(c) for c in cnt[r]], sd[r], [int(c) for c in cnt[:, r]], rd[r])
        assert ops[r].all_to_all_v(None, *a, streams[r].cuda_stream) == 0
    run_ranks(G, rank, comm)
    _finish(comm)
    for d in range(G):
        for k, e in enumerate(eb):
            want = np.full(nr[d] * e, SENTINEL, np.uint8)
            for s in range(G):
                if s != d:
                    want[rd[d][s] * e:(rd[d][s] + cnt[s][d]) * e] = send_h[s][k][sd[s][d] * e:(sd[s][d] + cnt[s][d]) * e]
            assert np.array_equal(recv[d][k].cpu().numpy(), want), (d, k)


def test_lag_and_poison_expose_an_unordered_reader(gpu_device):
    """What the parity tests rely on: after an all_to_all_v with lag, a copy of the receive range taken on a
    stream that has no dependency on the collective's stream shows old bytes or poison (it differs from what
    was sent), and the same copy on a stream that waits for an event recorded after the collective shows the
    data.  Only valid buffers are read.

    The HIP runtime multiplexes its streams on a few hardware queues (4 by default here), and two streams that
    share one run in submission order whatever their dependencies: measured on an MI355X, an unordered reader
    on such a stream saw the complete data behind a lag of 400 fills (15 ms) as behind one of 100, while the
    readers on other queues saw only old bytes behind 27.  That is the hardware's order, not a dependency the
    lag could outlast, so the unordered copy is taken on READERS streams created one after the other (the
    runtime spreads them over its queues) and the mechanism must show on at least one of them; which ones
    saw the data is in the failure message."""
    import torch

    from tests import _thread_comm as tc
    G, n, READERS = 3, 1 << 16, 8
    comm, streams, ops = _bare(G)
    rng = np.random.default_rng(400)
    sent = [rng.integers(1, 1 << 62, G * n, dtype=np.int64) for _ in range(G)]      # [to d] chunks of n words
    send = [_dev(s) for s in sent]
    recv = [_dev(np.zeros(G * n, np.int64)) for _ in range(G)]                      # the old bytes: zeros
    early = [_dev(np.zeros(2 * n, np.int64)) for _ in range(READERS)]
    late = _dev(np.zeros(2 * n, np.int64))
    s_free, s_dep = [torch.cuda.Stream() for _ in range(READERS)], torch.cuda.Stream()
    assert len({s.cuda_stream for s in s_free + streams + [s_dep]}) == READERS + G + 1
    ev = tc._event()
    for s, e in zip(s_free + [s_dep], early + [late]):          # (every stream has run before)
        tc._copy(e.data_ptr(), e.data_ptr() + 64, 8, s.cuda_stream)
    torch.cuda.synchronize()
    cnt, dis = [n] * G, [d * n for d in range(G)]

    def rank(r):
        a = _a2a_args([send[r]], [recv[r]], (8,), cnt, dis, cnt, dis)
        assert ops[r].all_to_all_v(None, *a, streams[r].cuda_stream) == 0
        if r == 0:                                              # rank 0's peers' ranges: [n, 3 n)
            for s, e in zip(s_free, early):
                tc._copy(e.data_ptr(), recv[0].data_ptr() + n * 8, 2 * n * 8, s.cuda_stream)
            tc._ok(tc.hip.hipEventRecord(ev, streams[0].cuda_stream), "hipEventRecord")
            tc._ok(tc.hip.hipStreamWaitEvent(s_dep.cuda_stream, ev, 0), "hipStreamWaitEvent")
            tc._copy(late.data_ptr(), recv[0].data_ptr() + n * 8, 2 * n * 8, s_dep.cuda_stream)
    tc.run_ranks(G, rank, comm)
    _finish(comm)
    want = np.concatenate([sent[1][:n], sent[2][:n]])
    assert np.array_equal(late.cpu().numpy(), want)
    saw_data = [bool(np.array_equal(e.cpu().numpy(), want)) for e in early]
    print("unordered readers that saw the data:", saw_data)
    assert not all(saw_data), "every unordered reader saw the data: the lag is too short"
    for e, d in zip(early, saw_data):                           # what differs is old bytes or poison
        if not d:
            got = e.cpu().numpy()
            assert np.isin(got[got != want], (0, -1)).all()
    assert np.array_equal(recv[0].cpu().numpy()[:n], np.zeros(n, np.int64))        # the own range: untouched


# ------------------------------------------------------------------ b. parity against the C oracle
_REF = collections.OrderedDict()       # (case, G, kind) -> the oracle's unsharded merge, kept for the tests
_REF_RECORDS = 24_000_000              # ... that share it (the least recently used leave past this many records)


def _reference(kw, G, kind):
    """The job in the layout's iteration order, every rank's (rows, offsets) and the oracle's merge of it."""
    from tests.test_dist_cpu import layout
    key = (repr(sorted(kw.items())), G, kind)
    if key in _REF:
        _REF.move_to_end(key)
        return _REF[key]
    base = _make_injected(kw)
    parts = [layout(base, G, r, kind) for r in range(G)]
    case = parts[0][0]
    ref = (case, [(sel, offs) for _, sel, offs in parts], oracle_run(case))
    _REF[key] = ref
    while len(_REF) > 1 and sum(len(v[0]["key"]) + v[0]["n_ids"] for v in _REF.values()) > _REF_RECORDS:
        _REF.popitem(last=False)
    return ref


class Shards:
    """G ranks of one replica on device 0, each a thread with its own DeviceTable joined over a ThreadComm:
    _shard_gpu_worker (tests/test_gpu_parity.py) with threads for processes.  Environment switches are set
    (monkeypatch) before this is built: they are process-wide, which is what every rank must see anyway."""

    def __init__(self, kw, G, kind="routed", path="sorted", counts=False, poison=True, lag=True):
        from tests import _thread_comm as tc
        self.G, self.kind, self.path, self.counts = G, kind, path, counts
        self.case, self.parts, self.oracle = _reference(kw, G, kind)
        self.comm = tc.ThreadComm(G, poison=poison, lag_fills=tc.LAG_FILLS if lag else 0)
        self.cap = -(-self.case["n_ids"] // G)
        self.want_flags = path in ("gather", "sorted+flags")
        self.tables, self.cols, self.flags = [None] * G, [None] * G, [None] * G
        tc.run_ranks(G, self._setup, self.comm)

    def _setup(self, r):
        import torch

        from crdt_amd import DeviceTable
        from tests._thread_comm import DEADLINE_MS
        case, (sel, _) = self.case, self.parts[r]
        t = self.tables[r] = DeviceTable(0, local_rank=case["local_rank"], capacity=self.cap)
        t.set_merge_path("sorted" if self.path == "sorted+flags" else self.path)
        t.set_counts(self.counts)
        self.reset(r)
        t.comm_init_ops(self.G, r, self.comm.rank(r))
        t.set_comm_timeout(DEADLINE_MS)
        assert t.comm_info() == (self.G, r)
        t.set_presharded(self.kind == "presharded")
        key = case["key"][sel]
        if self.kind == "presharded":
            key = key // self.G
        dev = lambda a: None if a is None else torch.from_numpy(  # noqa: E731
            np.ascontiguousarray(a.view(np.int32) if a.dtype == np.uint32 else a)).cuda()
        millis = None if case["millis"] is None else dev(case["millis"][sel])
        self.flags[r] = torch.zeros(max(len(sel), 1), dtype=torch.uint8, device="cuda") if self.want_flags else False
        self.cols[r] = (dev(key.astype(np.uint32)), dev(case["lt"][sel]), dev(case["rank"][sel]),
                        dev(case["val"][sel]), millis)

    def reset(self, r):
        case, t, G = self.case, self.tables[r], self.G
        loc = case["local"]
        ids = np.arange(case["n_local"])
        mine = (ids % G == r) & (loc["mod"] != ABSENT_MOD)
        t.clear_rows(0, self.cap)
        if mine.any():
            t.put_rows((ids[mine] // G).astype(np.uint32), loc["lt"][mine], loc["rank"][mine], loc["val"][mine],
                       loc["mod"][mine])
        t.canonical = case["c0"]

    def merge(self, reset=False, may_fail=False):
        """One collective crdt_merge on every rank; returns run_shard_gpu's per-rank tuples (may_fail: a
        CrdtNativeError's status instead)."""
        from crdt_amd.device import CrdtNativeError
        from tests._thread_comm import run_ranks

        def rank(r):
            t, (sel, offs) = self.tables[r], self.parts[r]
            if reset:
                self.reset(r)
            *cols, millis = self.cols[r]
            try:
                res, _ = t.merge(*cols, offs, self.case["wall"], millis=millis, win_flags=self.flags[r])
            except CrdtNativeError as e:
                if not may_fail:
                    raise
                return e.status
            res["path"] = t.last_path()
            res["plan"] = t.last_plan()
            lt, rk, val, mod = t.read_rows(np.arange(self.cap, dtype=np.uint32))
            fl = self.flags[r][:len(sel)].cpu().numpy() if self.want_flags else None
            return (r, res, lt, rk, val, mod, sel, fl)
        outs = run_ranks(self.G, rank, self.comm)
        assert self.comm.error is None, self.comm.error
        return outs

    def check(self, outs):
        check_shards(self.case, outs, self.G, self.kind, self.path, self.counts, *self.oracle)

    def close(self):
        for t in self.tables:
            if t is not None:
                t.close()
        self.comm.close()


def run_shard_threads(kw, G, kind="routed", path="sorted", counts=False, again=False, **comm_kw):
    """run_shard_gpu over the device-ordered transport: one call (again: a second on the same ctxs, after the
    same reset) and the comparison with the oracle; returns the last call's per-rank tuples."""
    sh = Shards(kw, G, kind, path, counts, **comm_kw)
    try:
        outs = sh.merge()
        if again:
            sh.check(outs)
            outs = sh.merge(reset=True)
        sh.check(outs)
        assert all(n > 0 for n in sh.comm.collectives), sh.comm.collectives
        return outs
    finally:
        sh.close()


PATHS = {"gather": ("gather", True), "sorted": ("sorted", True), "sorted-nocounts": ("sorted", False),
         "sorted+flags": ("sorted+flags", True)}
SMALL = ["r4_ties", "r8_tombstones", "drift_late", "dup_node", "send_overflow", "explicit_millis",
         "empty_changesets"]


@pytest.mark.parametrize("G", [2, 3])
@pytest.mark.parametrize("kind", ["routed", "parts", "presharded"])
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("name", SMALL)
def test_record_routing(gpu_device, name, path, kind, G):
    """Record routing (and the presharded form, no exchange) of the small golden cases in three layouts on 2
    and 3 ranks: gather receivers with win flags, sorted receivers with exact counts, the order-free form, and
    the flagged form whose flags travel back to the senders."""
    p, counts = PATHS[path]
    run_shard_threads(dict(CASE_SPECS)[name], G, kind, path=p, counts=counts)


@pytest.mark.parametrize("name", ["drift_late", "dup_node", "r8_tombstones"])
def test_eight_rank_record_routing(gpu_device, name):
    """G = 8: 7 peers, route_bits(8), sorted receivers in the order-free form."""
    outs = run_shard_threads(dict(CASE_SPECS)[name], 8, "routed", path="sorted", counts=False)
    assert all(o[1]["path"] in ("sorted", "gather") for o in outs)


def test_record_routing_without_lag(gpu_device):
    """The timing RCCL on a fast link gives: the data lands at once (poison still first)."""
    run_shard_threads(dict(CASE_SPECS)["r8_tombstones"], 3, "parts", path="sorted+flags", counts=True, again=True,
                      lag=False)


FRAME = dict(millis_span=1 << 12, counter_span=16, n_ranks=65, tomb_frac=0.1)     # the global frame fits
PACKED = dict(seed=808, R=16, per_cs=20_000, n_local=150_000, n_new=60_000, **FRAME)
AT = (9, 12_345)                       # where an injected record raises: it exists in every case below


def _injected(kw, inject):
    return dict(kw, inject=inject, inject_at=AT) if inject else dict(kw)


def _check_stop(outs, inject):
    for rank, res, *_ in outs:
        assert res["status"] == {None: 0, "drift": 1, "dup": 2}[inject], (rank, res)
        if inject:
            assert (res["exc_changeset"], res["exc_index"]) == AT, (rank, res)


@pytest.mark.parametrize("inject", [None, "drift", "dup"])
def test_packed_wire_own_chunk_in_place(gpu_device, monkeypatch, inject):
    """4 ranks, 16-B packed wire records, sorted receivers; the second call on each ctx scatters the own chunk
    straight into the receive columns while the peers' ranges are poisoned and filled by the exchange."""
    monkeypatch.setenv("CRDT_COMBINE", "0")
    outs = run_shard_threads(_injected(PACKED, inject), 4, "routed", path="sorted", counts=False, again=True)
    for rank, res, *_ in outs:
        assert res["path"] == "sorted" and res["plan"]["wire_packed"], (rank, res["plan"])
        assert res["plan"]["own_in_place"] and not res["plan"]["combined"], (rank, res["plan"])
    _check_stop(outs, inject)


@pytest.mark.parametrize("G", [2, 4])
def test_map_side_combine(gpu_device, monkeypatch, G):
    monkeypatch.setenv("CRDT_COMBINE", "2")
    outs = run_shard_threads(PACKED, G, "routed", path="sorted", counts=False, again=True)
    for rank, res, *_ in outs:
        assert res["plan"]["combined"] and res["plan"]["wire_packed"], (rank, res["plan"])


CAP1 = (1 << 20) + 13                  # a shard just above 2^20 slots: route_l1 with one level-1 digit per owner
HOME = (1 << 20) + 4224                # a rank's home records in the pieces cases: above route_l1's threshold


def _one_piece_kw(G):
    return dict(seed=821, R=8, per_cs=20_000, n_local=200_000, n_new=G * CAP1 - 200_000, **FRAME)


def _pieces_kw(G, R=16, cap=CAP1, seed=822):
    """Every rank's home part (changeset j whole on rank j % G) holds HOME >= 2^20 records."""
    assert G * HOME % R == 0 and R % G == 0
    return dict(seed=seed, R=R, per_cs=G * HOME // R, n_local=400_000, n_new=G * cap - 400_000, **FRAME)


def _rl1_env(monkeypatch, route_l1="1", split="1"):
    monkeypatch.setenv("CRDT_COMBINE", "0")
    monkeypatch.setenv("CRDT_ROUTE_L1", route_l1)
    monkeypatch.setenv("CRDT_RL1_SPLIT", split)


@pytest.mark.parametrize("G", [2, 8])
def test_route_l1_one_piece(gpu_device, monkeypatch, G):
    _rl1_env(monkeypatch)
    outs = run_shard_threads(_one_piece_kw(G), G, "routed", path="sorted", counts=False)
    for rank, res, *_ in outs:
        assert res["plan"]["route_l1"] and res["plan"]["rl1_pieces"] == 1, (rank, res["plan"])
        assert not res["plan"]["rl1_head"] and not res["plan"]["combined"], (rank, res["plan"])


@pytest.mark.parametrize("split,pieces", [("1", 2), ("3", 3), ("4", 4)])
@pytest.mark.parametrize("G", [2, 4])
def test_route_l1_pipelined_pieces(gpu_device, monkeypatch, G, split, pieces):
    """Piece q crosses the exchange on the ctx stream while q + 1 is partitioned on the side stream and the
    owner resolves q - 1 on the owner stream: each owner pass must wait for its piece's (late) exchange."""
    _rl1_env(monkeypatch, split=split)
    outs = run_shard_threads(_pieces_kw(G), G, "routed", path="sorted", counts=False, again=True)
    for rank, res, *_ in outs:
        assert res["plan"]["route_l1"] and res["plan"]["rl1_pieces"] == pieces, (rank, res["plan"])


def test_route_l1_pieces_without_lag(gpu_device, monkeypatch):
    _rl1_env(monkeypatch)
    outs = run_shard_threads(_pieces_kw(2), 2, "routed", path="sorted", counts=False, again=True, lag=False)
    assert all(o[1]["plan"]["rl1_pieces"] == 2 for o in outs)


def test_route_l1_two_digits_per_owner(gpu_device, monkeypatch):
    """Shards of 2^21 + 5 slots: two level-1 digits per owner, two pieces."""
    _rl1_env(monkeypatch)
    outs = run_shard_threads(_pieces_kw(2, cap=(1 << 21) + 5, seed=823), 2, "routed", path="sorted", counts=False)
    for rank, res, *_ in outs:
        assert res["plan"]["route_l1"] and res["plan"]["rl1_pieces"] == 2, (rank, res["plan"])


@pytest.mark.parametrize("inject", [None, "dup"])
@pytest.mark.parametrize("route_l1", ["2", "3"], ids=["head", "every-digit"])
@pytest.mark.parametrize("G", [2, 4])
def test_route_l1_head_fold(gpu_device, monkeypatch, G, route_l1, inject):
    """The head fold runs behind the partition on the side stream, crosses in an exchange of its own and is
    resolved as soon as that exchange is done, beside the pieces' owner work."""
    _rl1_env(monkeypatch, route_l1=route_l1)
    outs = run_shard_threads(_injected(_pieces_kw(G), inject), G, "routed", path="sorted", counts=False, again=True)
    for rank, res, *_ in outs:
        assert res["plan"]["route_l1"] and res["plan"]["rl1_head"], (rank, res["plan"])
        assert res["plan"]["rl1_pieces"] == 2, (rank, res["plan"])
    _check_stop(outs, inject)


def test_route_tune(gpu_device, monkeypatch):
    """The routing tuner left on: 12 calls at the pieces shape with 64 changesets take each way twice and then
    the fastest; every call leaves the oracle's rows and both ranks report the same decision."""
    for k in ("CRDT_COMBINE", "CRDT_ROUTE_L1", "CRDT_ROUTE_TUNE", "CRDT_RL1_SPLIT"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("CRDT_ENV_DYNAMIC", "1")
    sh = Shards(_pieces_kw(2, R=64, seed=824), 2, "routed", "sorted", False)
    try:
        ways = ("route_l1", "combine", "route_l1_4", "route_l1_1", "route_l1_head")
        for i in range(12):
            outs = sh.merge(reset=i > 0)
            sh.check(outs)
            tunes = [t.route_tune() for t in sh.tables]
            assert tunes[0] == tunes[1], (i, tunes)
            way = tunes[0]["best"] if i >= 10 else ways[i // 2]
            for rank, res, *_ in outs:
                plan = res["plan"]
                assert res["path"] == "sorted" and plan["route_tuned"], (rank, i, plan)
                assert plan["combined"] == (way == "combine") and plan["route_l1"] == (way != "combine"), (i, plan)
                assert plan["rl1_head"] == (way == "route_l1_head"), (rank, i, plan)
                if way != "combine":
                    assert plan["rl1_pieces"] == {"route_l1_4": 4, "route_l1_1": 1}.get(way, 2), (rank, i, plan)
        tune = sh.tables[0].route_tune()
        assert tune["best"] in ways and all(tune[f"{w}_ms"] > 0 for w in ways), tune
        assert tune["best"] == min(ways, key=lambda w: tune[f"{w}_ms"]), tune
    finally:
        sh.close()


@pytest.mark.parametrize("fail_rank", [0, 1])
@pytest.mark.parametrize("route,point", [("route_l1", 1), ("route_l1", 2), ("route_l1", 3), ("route_l1", 4),
                                         ("route_l1", 6), ("records", 1), ("records", 3), ("records", 4)])
def test_agreed_local_failure(gpu_device, monkeypatch, route, point, fail_rank):
    """An injected status (CRDT_TEST_FAIL, no GPU fault) on one rank: every rank returns CRDT_E_NOMEM, and a
    clean call on the same ctxs then equals the oracle (point 6, after the last exchange: on top of the stopped
    call's rows, the canonical having stood)."""
    _rl1_env(monkeypatch, route_l1="1" if route == "route_l1" else "0")
    monkeypatch.setenv("CRDT_ENV_DYNAMIC", "1")
    monkeypatch.setenv("CRDT_TEST_FAIL", f"{fail_rank}:{point}")
    sh = Shards(_one_piece_kw(2), 2, "routed", "sorted", False)
    try:
        assert sh.merge(may_fail=True) == [NOMEM, NOMEM]
        monkeypatch.setenv("CRDT_TEST_FAIL", "-1:0")      # (no rank is inside the library here)
        if point == 6:
            assert all(t.canonical == sh.case["c0"] for t in sh.tables)
        outs = sh.merge(reset=point != 6)
        sh.check(outs)
        for rank, res, *_ in outs:
            assert res["plan"]["route_l1"] == (route == "route_l1"), (rank, res["plan"])
    finally:
        sh.close()
