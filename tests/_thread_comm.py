"""An in-process, device-ordered crdt_comm_ops (CRDT_MEM_DEVICE) for G ranks with real peers: the ranks are G
Python threads of one process, each with its own DeviceTable on device 0 joined with
``comm_init_ops(G, r, comm.rank(r))``, and every rank holds its own data.  A callback only enqueues work on the
stream the library hands it and returns, as RCCL does; it never synchronises the host with the device, so
the library's own stream and event dependencies (stream / sstream / ostream in comm_path.inc) are all that
orders a consumer behind an exchange.  Test infrastructure (tests/test_gpu_device_ordered.py).

Protocol (pull model; every collective of the library goes on the ctx stream, so a rank has one order of
collectives and one rendezvous per collective is enough):

  1. rank r records ``ready[r]`` on its stream (its send buffers are final) and publishes its pointers, counts
     and displacements in ``slots[r]``;
  2. host barrier;
  3. rank r makes its stream wait on every peer's ``ready[p]``, enqueues the lag, the poison and then device
     copies (hipMemcpyAsync) from the peers' send ranges into its own receive ranges, and records ``done[r]``;
  4. host barrier;
  5. rank r makes its stream wait on every peer's ``done[p]``: a send buffer stays busy until every reader has
     read it (RCCL's contract; the library may reuse it right after).

One ``ready`` / ``done`` pair per rank serves every collective.  That is safe because a wait is always enqueued
before the barrier that lets the event's owner record it again: hipStreamWaitEvent captures the record that is
current when it is called, the waits on ``ready[p]`` are enqueued before barrier 4 and p records ``ready[p]``
again only after it passed barrier 4 of this collective; the waits on ``done[p]`` are enqueued before barrier 2
of the next collective and p records ``done[p]`` again only after that barrier.  The same argument covers the
slots: they are read in step 3 and rewritten after barrier 4.

Two knobs make a missing dependency visible (both on in the parity tests):

  * ``poison``: the receive ranges about to be written are first filled with 0xFF bytes on the stream (receive
    contents are undefined until the collective completes, so this is within the contract);
  * ``lag_fills``: before the poison and the copies the stream runs a bounded piece of ordinary device work,
    ``lag_fills`` fills (hipMemsetAsync) of a LAG_BYTES scratch buffer, so the data lands well after anything the
    library queued on its other streams.  Measured on an MI355X with HIP events around the lag alone (the loop
    at the bottom of this file, ``python -m tests._thread_comm``): one fill of 256 MiB takes 38.4 us, and the
    smallest count that gives at least 1 ms is LAG_FILLS = 27 (1.033 ms; 26 fills: 0.996 ms).  With G ranks'
    lags running at once each takes longer, never shorter.

all_to_all_v touches only ``[recv_displs[d], + recv_counts[d])`` for d != me (the library writes its own chunk
itself, possibly from another stream at the same time); all_gather copies the own row only when the pointers
differ (in place is legal); all_reduce pulls the G word vectors into a per-rank scratch tensor [G, n] by steps
3 to 5 and then reduces it with torch on ``torch.cuda.ExternalStream(stream)`` (SUM wraps as int64, MAX and
MIN are signed) and copies the result over the words.

Failure: every host barrier has a timeout (BARRIER_S, far above any test's run time and below the ctx deadline
the harness sets); a timeout or any exception sets ``comm.error``, breaks the barrier so the other ranks
return at once too, and the callback returns 1, which the library turns into CRDT_E_COMM.
"""
import ctypes
import threading

from crdt_amd import _capi

_capi.load()                    # (first: it brings in the one HIP runtime of the process, _capi.load's rule)
hip = ctypes.CDLL("libamdhip64.so.7")
_P, _SZ, _U = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint
hip.hipMemcpyAsync.argtypes = [_P, _P, _SZ, ctypes.c_int, _P]
hip.hipMemsetAsync.argtypes = [_P, ctypes.c_int, _SZ, _P]
hip.hipEventCreateWithFlags.argtypes = [ctypes.POINTER(_P), _U]
hip.hipEventCreate.argtypes = [ctypes.POINTER(_P)]
hip.hipEventDestroy.argtypes = [_P]
hip.hipEventRecord.argtypes = [_P, _P]
hip.hipStreamWaitEvent.argtypes = [_P, _P, _U]
hip.hipEventSynchronize.argtypes = [_P]
hip.hipEventElapsedTime.argtypes = [ctypes.POINTER(ctypes.c_float), _P, _P]
D2D = 3
EVENT_DISABLE_TIMING = 2

BARRIER_S = 30.0                # every host barrier's timeout
DEADLINE_MS = 60_000            # the ctx deadline the harness sets on every rank (crdt_set_comm_timeout)
JOIN_S = 120.0                  # run_ranks joins every rank's thread within this
LAG_BYTES = 256 << 20           # the lag's scratch buffer (one per rank)
# The smallest fill count whose lag alone took at least 1 ms on an MI355X, HIP events around it, the minimum of
# 5 runs on an idle device (measure_lag below): 38.4 us a fill, 26 fills 0.996 ms, 27 fills 1.033 ms
LAG_FILLS = 27

REDUCE_SUM, REDUCE_MAX, REDUCE_MIN = 0, 1, 2


def _ok(st, what):
    if st != 0:
        raise RuntimeError(f"{what} failed with HIP status {st}")


def _event(timing=False):
    e = _P()
    if timing:
        _ok(hip.hipEventCreate(ctypes.byref(e)), "hipEventCreate")
    else:
        _ok(hip.hipEventCreateWithFlags(ctypes.byref(e), EVENT_DISABLE_TIMING), "hipEventCreateWithFlags")
    return e


def _copy(dst, src, nbytes, stream):
    if nbytes:
        _ok(hip.hipMemcpyAsync(dst, src, nbytes, D2D, stream), "hipMemcpyAsync")


def _fill(dst, byte, nbytes, stream):
    if nbytes:
        _ok(hip.hipMemsetAsync(dst, byte, nbytes, stream), "hipMemsetAsync")


class _Rank:
    """What DeviceTable.comm_init_ops takes for one rank: ``ops()`` and the group's ``error``."""

    def __init__(self, comm, r):
        self.comm, self.r = comm, r
        self._ops = None

    @property
    def error(self):
        return self.comm.error

    def ops(self):
        if self._ops is None:
            self._ops = self.comm._ops(self.r)
        return self._ops


class ThreadComm:
    """G ranks in one process; ``rank(r)`` is rank r's crdt_comm_ops (device memory)."""

    def __init__(self, G, poison=True, lag_fills=LAG_FILLS):
        import torch
        self.G, self.poison, self.lag_fills = G, poison, lag_fills
        self.error = None
        self.barrier = threading.Barrier(G, timeout=BARRIER_S)
        self.slots = [None] * G
        self.ready = [_event() for _ in range(G)]
        self.done = [_event() for _ in range(G)]
        self.keep = []                                 # tensors and callbacks kept alive until the test ends
        self.lag = [torch.empty(LAG_BYTES, dtype=torch.uint8, device="cuda") if lag_fills else None
                    for _ in range(G)]
        self.scratch = [torch.empty((G, 1024), dtype=torch.int64, device="cuda") for _ in range(G)]
        self.result = [torch.empty(1024, dtype=torch.int64, device="cuda") for _ in range(G)]
        self.collectives = [0] * G                     # per rank, for the tests
        torch.cuda.synchronize()                       # (the constructor is test code, not a callback)
        self._ranks = [_Rank(self, r) for r in range(G)]

    def rank(self, r):
        return self._ranks[r]

    def close(self):
        for e in self.ready + self.done:
            hip.hipEventDestroy(e)
        self.ready = self.done = []

    def fail(self, e):
        if self.error is None:
            self.error = e
        self.barrier.abort()

    # ---- the rendezvous ---------------------------------------------------------------------------------
    def _collective(self, r, stream, slot, pull):
        """Steps 1 to 5 for rank r: ``slot`` is what the peers read of r, ``pull(p, slots[p])`` the copies
        (destination, source, bytes) r makes from rank p's send ranges."""
        G = self.G
        _ok(hip.hipEventRecord(self.ready[r], stream), "hipEventRecord")
        self.slots[r] = slot
        self.barrier.wait()
        for p in range(G):
            if p != r:
                _ok(hip.hipStreamWaitEvent(stream, self.ready[p], 0), "hipStreamWaitEvent")
        for i in range(self.lag_fills):
            _fill(self.lag[r].data_ptr(), i & 0xFF, LAG_BYTES, stream)
        plans = [pull(p, self.slots[p]) for p in range(G)]
        if self.poison:
            for plan in plans:
                for dst, _, nb in plan:
                    _fill(dst, 0xFF, nb, stream)
        for plan in plans:
            for dst, src, nb in plan:
                _copy(dst, src, nb, stream)
        _ok(hip.hipEventRecord(self.done[r], stream), "hipEventRecord")
        self.barrier.wait()
        for p in range(G):
            if p != r:
                _ok(hip.hipStreamWaitEvent(stream, self.done[p], 0), "hipStreamWaitEvent")
        self.collectives[r] += 1

    # ---- the three operations (device pointers as integers) -----------------------------------------
    def all_gather(self, r, send, recv, n, stream):
        nb = n * 8
        if recv + r * nb != send:                        # (in place is legal: then the own row is there already)
            _copy(recv + r * nb, send, nb, stream)
        self._collective(r, stream, (send, n), lambda p, s: [] if p == r else [(recv + p * nb, s[0], nb)])

    def all_to_all_v(self, r, cols, sc, sd, rc, rd, stream):
        """cols: [(send pointer, receive pointer, element bytes)]; from peer p: its elements
        [sd_p[r], + sc_p[r]) into [rd[p], + rc[p]) of every column.  The own-rank range is never touched."""
        def pull(p, s):
            if p == r:
                return []
            pcols, psc, psd = s
            if psc[r] != rc[p]:
                raise RuntimeError(f"all_to_all_v: rank {p} sends rank {r} {psc[r]} elements, it expects {rc[p]}")
            return [(mine[1] + rd[p] * mine[2], theirs[0] + psd[r] * theirs[2], rc[p] * mine[2])
                    for mine, theirs in zip(cols, pcols) if rc[p]]
        self._collective(r, stream, (cols, sc, sd), pull)

    def all_reduce(self, r, words, n, op, stream):
        import torch
        G = self.G
        if self.scratch[r].shape[1] < n:                 # grown only when too small; the old ones stay alive
            self.keep += [self.scratch[r], self.result[r]]
            self.scratch[r] = torch.empty((G, n), dtype=torch.int64, device="cuda")
            self.result[r] = torch.empty(n, dtype=torch.int64, device="cuda")
        scr, res = self.scratch[r], self.result[r]
        row = scr.shape[1] * 8

        def pull(p, s):
            if s[1:] != (n, op):
                raise RuntimeError(f"all_reduce: rank {p} posted (n, op) = {s[1:]}, rank {r} {(n, op)}")
            return [(scr.data_ptr() + p * row, s[0], n * 8)]
        self._collective(r, stream, (words, n, op), pull)
        with torch.cuda.stream(torch.cuda.ExternalStream(stream)):
            v = scr[:, :n]
            if op == REDUCE_SUM:
                torch.sum(v, dim=0, out=res[:n])         # (int64: wraps)
            elif op == REDUCE_MAX:
                torch.amax(v, dim=0, out=res[:n])
            elif op == REDUCE_MIN:
                torch.amin(v, dim=0, out=res[:n])
            else:
                raise RuntimeError(f"all_reduce: op {op}")
        _copy(words, res.data_ptr(), n * 8, stream)

    # ---- the C table --------------------------------------------------------------------------------------
    def _ops(self, r):
        G = self.G

        def guard(fn):
            def call(*a):
                try:
                    fn(*a)
                    return 0
                except Exception as e:  # noqa: BLE001 -- the library reports CRDT_E_COMM
                    self.fail(e)
                    return 1
            return call

        def _ar(user, words, n, op, stream):
            self.all_reduce(r, words, int(n), int(op), stream)

        def _ag(user, send, recv, n, stream):
            self.all_gather(r, send, recv, int(n), stream)

        def _a2a(user, n_cols, send, recv, eb, sc, sd, rc, rd, stream):
            cols = [(send[k] or 0, recv[k] or 0, int(eb[k])) for k in range(n_cols)]
            self.all_to_all_v(r, cols, [int(sc[d]) for d in range(G)], [int(sd[d]) for d in range(G)],
                              [int(rc[d]) for d in range(G)], [int(rd[d]) for d in range(G)], stream)

        cbs = (_capi.ALL_REDUCE_FN(guard(_ar)), _capi.ALL_GATHER_FN(guard(_ag)), _capi.ALL_TO_ALL_FN(guard(_a2a)))
        self.keep.append(cbs)
        return _capi.CrdtCommOps(None, _capi.CRDT_MEM_DEVICE, 0, *cbs)


def run_ranks(G, fn, comm=None, timeout=JOIN_S):
    """fn(r) on G threads (one per rank); joins each within ``timeout`` s and re-raises the first worker
    exception (a worker that raises breaks ``comm``'s barrier, so its peers return at once).  Returns the
    ranks' results in rank order."""
    out, errs = [None] * G, []

    def work(r):
        try:
            out[r] = fn(r)
        except BaseException as e:  # noqa: BLE001 -- re-raised on the calling thread
            errs.append((r, e))
            if comm is not None:
                comm.fail(e)

    ts = [threading.Thread(target=work, args=(r,), daemon=True) for r in range(G)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout)
    hung = [r for r, t in enumerate(ts) if t.is_alive()]
    if errs:
        r, e = min(errs, key=lambda x: x[0])
        raise RuntimeError(f"rank {r} failed: {e!r}") from e
    assert not hung, f"ranks {hung} did not finish within {timeout} s"
    return out


def measure_lag(fills, runs=5):
    """The lag alone, ``fills`` fills on one stream of an idle device, HIP events around it: ms, the minimum
    of ``runs``."""
    import torch
    buf = torch.empty(LAG_BYTES, dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    a, b = _event(True), _event(True)
    best = None
    for k in range(runs + 1):                            # (the first run warms up)
        torch.cuda.synchronize()
        _ok(hip.hipEventRecord(a, s.cuda_stream), "hipEventRecord")
        for i in range(fills):
            _fill(buf.data_ptr(), i & 0xFF, LAG_BYTES, s.cuda_stream)
        _ok(hip.hipEventRecord(b, s.cuda_stream), "hipEventRecord")
        _ok(hip.hipEventSynchronize(b), "hipEventSynchronize")
        ms = ctypes.c_float()
        _ok(hip.hipEventElapsedTime(ctypes.byref(ms), a, b), "hipEventElapsedTime")
        if k:
            best = ms.value if best is None else min(best, ms.value)
    return best


if __name__ == "__main__":                               # the smallest fill count whose lag is >= 1 ms
    per = measure_lag(64) / 64
    print(f"one fill of {LAG_BYTES >> 20} MiB: {per * 1e3:.1f} us")
    n = max(1, int(0.5 / per))
    while True:
        ms = measure_lag(n)
        print(f"fills {n}: {ms:.3f} ms")
        if ms >= 1.0:
            break
        n += 1
    print(f"LAG_FILLS = {n}  ({ms:.3f} ms)")
