// comm_path.inc — a key-sharded replica: the collectives of a multi-GPU merge run inside
// the ctx (included by crdt_merge.hip, after the single-GPU phases it reuses).
//
// SURVEY §8(b) ("Threading": one HIP stream and one RCCL communicator per device inside
// the ctx) and §8(e) steps 1-6.  The reference has no transport at all
// (example/crdt_example.dart:21-25); the contract is that R sequential Crdt.merge calls
// (crdt.dart:77-94) against the union of the shards give exactly the rows, canonical and
// exception the single-GPU call gives.
//
// Backends.  RCCL: librccl.so.1 is opened on first use (a process that already loaded
// PyTorch's copy gets that one: same SONAME), so single-GPU users never load it; every
// collective is enqueued on the ctx stream.  crdt_comm_ops: a caller's transport;
// CRDT_MEM_HOST tables are called synchronously on staged host copies.
// (<dlfcn.h> and <rccl/rccl.h> — types and prototypes only, the symbols are resolved with
// dlsym — are included at the top of crdt_merge.hip; this file sits inside its anonymous
// namespace and leaves it open again at its end.)

struct RcclApi {
    void* handle = nullptr;
    decltype(&ncclGetUniqueId) get_unique_id = nullptr;
    decltype(&ncclCommInitRank) comm_init_rank = nullptr;
    decltype(&ncclCommDestroy) comm_destroy = nullptr;
    decltype(&ncclAllReduce) all_reduce = nullptr;
    decltype(&ncclAllGather) all_gather = nullptr;
    decltype(&ncclSend) send = nullptr;
    decltype(&ncclRecv) recv = nullptr;
    decltype(&ncclGroupStart) group_start = nullptr;
    decltype(&ncclGroupEnd) group_end = nullptr;
    decltype(&ncclCommAbort) comm_abort = nullptr;             // the call's deadline (below)
    decltype(&ncclCommGetAsyncError) get_async_error = nullptr;
};

RcclApi g_rccl;

int rccl_load() {
    if (g_rccl.handle) return CRDT_OK;
    void* h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!h) h = dlopen("/opt/rocm/lib/librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!h) {
        fprintf(stderr, "crdt: cannot open librccl.so.1: %s\n", dlerror());
        return CRDT_E_COMM;
    }
    RcclApi a;
    a.handle = h;
#define CRDT_SYM(field, name)                                              \
    a.field = reinterpret_cast<decltype(a.field)>(dlsym(h, name));         \
    if (!a.field) { fprintf(stderr, "crdt: librccl lacks %s\n", name); return CRDT_E_COMM; }
    CRDT_SYM(get_unique_id, "ncclGetUniqueId");
    CRDT_SYM(comm_init_rank, "ncclCommInitRank");
    CRDT_SYM(comm_destroy, "ncclCommDestroy");
    CRDT_SYM(all_reduce, "ncclAllReduce");
    CRDT_SYM(all_gather, "ncclAllGather");
    CRDT_SYM(send, "ncclSend");
    CRDT_SYM(recv, "ncclRecv");
    CRDT_SYM(group_start, "ncclGroupStart");
    CRDT_SYM(group_end, "ncclGroupEnd");
    CRDT_SYM(comm_abort, "ncclCommAbort");
    CRDT_SYM(get_async_error, "ncclCommGetAsyncError");
#undef CRDT_SYM
    g_rccl = a;
    return CRDT_OK;
}

// ---- the RCCL backend as a crdt_comm_ops table (user = the ctx) --------------------------
int rccl_all_reduce(void* user, int64_t* w, uint64_t n, int32_t op, void* stream) {
    crdt_ctx* c = static_cast<crdt_ctx*>(user);
    const ncclRedOp_t o = op == CRDT_REDUCE_SUM ? ncclSum : op == CRDT_REDUCE_MAX ? ncclMax : ncclMin;
    return g_rccl.all_reduce(w, w, n, ncclInt64, o, static_cast<ncclComm_t>(c->rccl_comm),
                             static_cast<hipStream_t>(stream)) == ncclSuccess ? 0 : 1;
}

int rccl_all_gather(void* user, const int64_t* send, int64_t* recv, uint64_t n, void* stream) {
    crdt_ctx* c = static_cast<crdt_ctx*>(user);
    return g_rccl.all_gather(send, recv, n, ncclInt64, static_cast<ncclComm_t>(c->rccl_comm),
                             static_cast<hipStream_t>(stream)) == ncclSuccess ? 0 : 1;
}

// One group: every column to / from every peer (RCCL runs the peers' transfers concurrently
// over their xGMI links; per-column calls outside a group would serialise).
int rccl_all_to_all_v(void* user, uint32_t n_cols, const void* const* send_cols, void* const* recv_cols,
                      const uint32_t* eb, const uint64_t* sc, const uint64_t* sd, const uint64_t* rc,
                      const uint64_t* rd, void* stream) {
    crdt_ctx* c = static_cast<crdt_ctx*>(user);
    const ncclComm_t comm = static_cast<ncclComm_t>(c->rccl_comm);
    const hipStream_t s = static_cast<hipStream_t>(stream);
    if (g_rccl.group_start() != ncclSuccess) return 1;
    bool ok = true;
    for (uint32_t d = 0; d < c->n_ranks && ok; ++d) {
        if (d == c->rank) continue;
        for (uint32_t k = 0; k < n_cols && ok; ++k) {
            if (sc[d])
                ok = g_rccl.send(static_cast<const char*>(send_cols[k]) + sd[d] * eb[k], sc[d] * eb[k], ncclUint8,
                                 (int)d, comm, s) == ncclSuccess;
            if (ok && rc[d])
                ok = g_rccl.recv(static_cast<char*>(recv_cols[k]) + rd[d] * eb[k], rc[d] * eb[k], ncclUint8,
                                 (int)d, comm, s) == ncclSuccess;
        }
    }
    const bool ended = g_rccl.group_end() == ncclSuccess;
    return ok && ended ? 0 : 1;
}

// ---- the call's deadline (crdt_set_comm_timeout; VERDICT r5 item 1) ----------------------------------------
// A peer that died, hung or faulted never posts its side of a collective.  On RCCL the collective's kernels
// then spin on this device, and the host would wait at the call's next synchronisation forever.  So every host
// wait of a sharded call polls (comm_wait) against the call's deadline — crdt_set_comm_timeout ms after the
// call's entry (default 300 s; 0 = none) — and against RCCL's asynchronous error.  Past the deadline the
// communicator is aborted (ncclCommAbort: its kernels in flight exit), the ctx's streams drain (bounded) and the
// call returns CRDT_E_COMM; every surviving rank does the same at its own deadline.  The ctx then refuses
// sharded merges (CRDT_E_COMM at once) until it joins a communicator again; the rows of its shard touched by the
// failed call are undefined (re-sync the shard).  Host transports (CRDT_MEM_HOST) block inside their callbacks,
// so they bound each operation themselves (dist.GlooComm: its timeout); a callback that fails, or returns past
// the deadline, fails the call and the communicator the same way.  crdt_comm_state reports where the call was
// (c->comm_phase), also from another thread while the call runs (a watchdog's report).
inline int64_t now_ns() {
    return std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch())
        .count();
}
inline void set_phase(crdt_ctx* c, const char* p) { c->comm_phase.store(p, std::memory_order_relaxed); }

// wait for s (or e) with a bound of its own, whatever the call's deadline: true if it drained
bool wait_bounded(hipStream_t s, hipEvent_t e, int64_t ns) {
    const int64_t end = now_ns() + ns;
    for (;;) {
        const hipError_t q = e ? hipEventQuery(e) : hipStreamQuery(s);
        if (q != hipErrorNotReady) return q == hipSuccess;
        if (now_ns() > end) return false;
        std::this_thread::sleep_for(std::chrono::microseconds(200));
    }
}

constexpr int64_t kDrainNs = 30ll * 1000 * 1000 * 1000;   // after an abort the ctx's streams get 30 s to drain
constexpr int64_t kSpinNs = 50ll * 1000 * 1000;           // a wait spins (yielding) this long, then sleeps

int comm_abort(crdt_ctx* c, const char* why, int state) {
    int expected = 0;
    if (!c->comm_state.compare_exchange_strong(expected, state)) return CRDT_E_COMM;
    fprintf(stderr, "crdt: rank %u of %u: %s in '%s' (deadline %u ms after the call's start): communicator "
            "aborted\n", c->rank, c->n_ranks, why, c->comm_phase.load(), c->comm_timeout_ms);
    fflush(stderr);
    if (c->rccl_comm && g_rccl.comm_abort) {
        g_rccl.comm_abort(static_cast<ncclComm_t>(c->rccl_comm));
        c->rccl_comm = nullptr;
    }
    for (hipStream_t s : {c->stream, c->sstream, c->ostream})
        if (s && !wait_bounded(s, nullptr, kDrainNs))
            fprintf(stderr, "crdt: rank %u: a stream did not drain within 30 s of the abort\n", c->rank);
    return CRDT_E_COMM;
}

int comm_wait(crdt_ctx* c, hipStream_t s, hipEvent_t e) {
    const bool polled = c->has_comm && c->ops.mem == CRDT_MEM_DEVICE && c->comm_deadline_ns;
    if (!polled) return (e ? hipEventSynchronize(e) : hipStreamSynchronize(s)) == hipSuccess ? CRDT_OK : CRDT_E_HIP;
    const int64_t t0 = now_ns();
    for (uint32_t it = 0;; ++it) {
        const hipError_t q = e ? hipEventQuery(e) : hipStreamQuery(s);
        if (q == hipSuccess) return CRDT_OK;
        if (q != hipErrorNotReady) return CRDT_E_HIP;
        const int64_t t = now_ns();
        if (t > c->comm_deadline_ns) return comm_abort(c, "deadline passed", 1);
        if ((it & 255) == 255 && c->rccl_comm && g_rccl.get_async_error) {
            ncclResult_t ae = ncclSuccess;
            if (g_rccl.get_async_error(static_cast<ncclComm_t>(c->rccl_comm), &ae) == ncclSuccess &&
                ae != ncclSuccess && ae != ncclInProgress)
                return comm_abort(c, "RCCL asynchronous error", 2);
        }
        if (t - t0 < kSpinNs)
            std::this_thread::yield();
        else
            std::this_thread::sleep_for(std::chrono::microseconds(100));
    }
}

// a host transport's callback returned rc: its failure, or a return past the deadline, fails the call
int host_done(crdt_ctx* c, int rc) {
    if (rc) return comm_abort(c, "transport error", 2);
    if (c->comm_deadline_ns && now_ns() > c->comm_deadline_ns) return comm_abort(c, "deadline passed", 1);
    return CRDT_OK;
}

// CRDT_TEST_STALL="rank:point:ms[:d]": the named rank stalls at `point` (kStall*): a host sleep, or (:d) a
// device spin of ms on the ctx stream (bounded by the wall clock); ms < 0: the process exits there.
enum : int { kStallGather = 1, kStallCounts = 2, kStallRecords = 3, kStallFinish = 4, kStallReadback = 5 };
__global__ void k_test_spin(unsigned long long ticks) {
    const unsigned long long t0 = wall_clock64();
    while ((unsigned long long)wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(64);
}
void test_stall(crdt_ctx* c, int point) {
    if (c->stall_at != point || c->stall_rank != (int)c->rank) return;
    if (c->stall_ms < 0) {
        fprintf(stderr, "crdt: rank %u: CRDT_TEST_STALL: exiting at point %d\n", c->rank, point);
        fflush(stderr);
        _exit(17);
    }
    if (c->stall_dev) {
        int khz = 0;
        if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, c->device) != hipSuccess || khz <= 0)
            khz = 100000;
        k_test_spin<<<1, 64, 0, c->stream>>>((unsigned long long)khz * (unsigned long long)c->stall_ms);
    } else {
        std::this_thread::sleep_for(std::chrono::milliseconds(c->stall_ms));
    }
}

// ---- collectives as the merge calls them (host-staged for CRDT_MEM_HOST tables) ----------
int comm_all_reduce(crdt_ctx* c, long long* d, uint64_t n, int32_t op) {
    if (c->comm_state.load()) return CRDT_E_COMM;
    if (!n) return CRDT_OK;
    if (c->ops.mem == CRDT_MEM_DEVICE)
        return c->ops.all_reduce_i64(c->ops.user, reinterpret_cast<int64_t*>(d), n, op, c->stream)
                   ? comm_abort(c, "transport error", 2) : CRDT_OK;
    HIPCHK(hipStreamSynchronize(c->stream));             // a pending copy may still read h_stage
    HIPALLOC(c->h_stage.ensure(n * 8));
    HIPCHK(hipMemcpyAsync(c->h_stage.p, d, n * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    int st = host_done(c, c->ops.all_reduce_i64(c->ops.user, reinterpret_cast<int64_t*>(c->h_stage.p), n, op, nullptr));
    if (st) return st;
    HIPCHK(hipMemcpyAsync(d, c->h_stage.p, n * 8, hipMemcpyHostToDevice, c->stream));
    return CRDT_OK;
}

int comm_all_gather(crdt_ctx* c, const long long* send, long long* recv, uint64_t n) {
    if (c->comm_state.load()) return CRDT_E_COMM;
    if (c->ops.mem == CRDT_MEM_DEVICE)
        return c->ops.all_gather_i64(c->ops.user, reinterpret_cast<const int64_t*>(send),
                                     reinterpret_cast<int64_t*>(recv), n, c->stream)
                   ? comm_abort(c, "transport error", 2) : CRDT_OK;
    const uint64_t tot = n * (1 + (uint64_t)c->n_ranks);
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPALLOC(c->h_stage.ensure(tot * 8));
    int64_t* h = reinterpret_cast<int64_t*>(c->h_stage.p);
    HIPCHK(hipMemcpyAsync(h, send, n * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    int st = host_done(c, c->ops.all_gather_i64(c->ops.user, h, h + n, n, nullptr));
    if (st) return st;
    HIPCHK(hipMemcpyAsync(recv, h + n, n * c->n_ranks * 8, hipMemcpyHostToDevice, c->stream));
    return CRDT_OK;
}

// ns / nr: lengths of the send / receive columns (host-staged tables copy them whole).
int comm_all_to_all(crdt_ctx* c, uint32_t n_cols, const void* const* send, void* const* recv, const uint32_t* eb,
                    const uint64_t* sc, const uint64_t* sd, const uint64_t* rc, const uint64_t* rd, uint64_t ns,
                    uint64_t nr) {
    if (c->comm_state.load()) return CRDT_E_COMM;
    uint32_t rec_bytes = 0;                              // (crdt_timing.sent_bytes)
    for (uint32_t k = 0; k < n_cols; ++k) rec_bytes += eb[k];
    for (uint32_t d = 0; d < c->n_ranks; ++d)
        if (d != c->rank) c->sent_bytes += sc[d] * rec_bytes;
    if (c->ops.mem == CRDT_MEM_DEVICE)
        return c->ops.all_to_all_v(c->ops.user, n_cols, send, recv, eb, sc, sd, rc, rd, c->stream)
                   ? comm_abort(c, "transport error", 2) : CRDT_OK;
    uint64_t bytes = 0;
    for (uint32_t k = 0; k < n_cols; ++k) bytes += (ns + nr) * eb[k];
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPALLOC(c->h_stage.ensure(bytes ? bytes : 1));
    std::vector<const void*> hs(n_cols);
    std::vector<void*> hr(n_cols);
    uint8_t* p = c->h_stage.p;
    for (uint32_t k = 0; k < n_cols; ++k) {
        hs[k] = p;
        if (ns) HIPCHK(hipMemcpyAsync(p, send[k], ns * eb[k], hipMemcpyDeviceToHost, c->stream));
        p += ns * eb[k];
        hr[k] = p;
        p += nr * eb[k];
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    int st = host_done(c, c->ops.all_to_all_v(c->ops.user, n_cols, hs.data(), hr.data(), eb, sc, sd, rc, rd, nullptr));
    if (st) return st;
    // this rank's own chunk is not in the exchange: copy only the peers' ranges back
    for (uint32_t k = 0; k < n_cols; ++k)
        for (uint32_t s = 0; s < c->n_ranks; ++s)
            if (s != c->rank && rc[s])
                HIPCHK(hipMemcpyAsync(static_cast<uint8_t*>(recv[k]) + rd[s] * eb[k],
                                      static_cast<const uint8_t*>(hr[k]) + rd[s] * eb[k], rc[s] * eb[k],
                                      hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));            // the staging buffer is reused next call
    return CRDT_OK;
}

// ---- failures agreed over the ranks ---------------------------------------------------------------------
// A sharded merge is a fixed sequence of collectives; a rank that returned early on a local failure (an
// allocation, a bad argument of its own batch) would leave its peers blocked in the next one.  So every
// local failure is carried to a point where all ranks learn of it and fail the call alike:
//   * before the gather: the rank still posts the gather and the clock phase's two reductions, its gather row
//     carrying the status (k_fail_row -> k_shard_combine -> Misc::shard_status), and the MAX reduction a word
//     for failures after the gather — read back with the shape words at the clock phase's one synchronisation;
//   * route_l1's preparation: a status word reduced beside the count exchange, read back with the counts;
//   * before each record exchange: comm_agree, one MAX all-reduce of the status (a host synchronisation);
//   * in the owners' apply: finish_apply's SUM reduction, with one word per failure code.
// The buffers these collectives use are allocated when the ctx joins its communicator (comm_attach) or at the
// call's start, before any local work.  What stays rank-local: a failing transport (CRDT_E_COMM) and a rank
// that cannot allocate the O(R) words of the gather itself.
enum : int { kFailLocal = 1, kFailRoutePrep = 2, kFailRecv = 3, kFailOwner = 4, kFailCombine = 5, kFailApply = 6 };
inline bool inject_fail(const crdt_ctx* c, int point) {
    return c->fail_at == point && c->fail_rank == (int)c->rank;
}

// Every rank's status (0 or -CRDT_E_*) -> the same on every rank: 0 if all are 0, else the largest code.
// A HIP error of the word's own upload (the device failing a copy) is folded into the word the rank sends
// where it can be (the host-staged form) and otherwise returned after the reduction was posted: the peers
// then fail at their deadline (the rank-local errors of include/crdt_merge.h).
int comm_agree(crdt_ctx* c, int st) {
    if (c->comm_state.load()) return CRDT_E_COMM;
    const long long w = st < 0 ? -(long long)st : 0;
    c->h_agree.p[0] = w;
    if (c->ops.mem == CRDT_MEM_HOST) {                  // (a host backend reduces the pinned word in place)
        const int e = host_done(c, c->ops.all_reduce_i64(c->ops.user, reinterpret_cast<int64_t*>(c->h_agree.p), 1,
                                                         CRDT_REDUCE_MAX, nullptr));
        if (e) return e;
        c->h_agree.p[1] = c->h_agree.p[0];
    } else {
        int lst = CRDT_OK;
        HIPLST(hipMemcpyAsync(c->d_agree.p, c->h_agree.p, 8, hipMemcpyHostToDevice, c->stream));
        if (c->ops.all_reduce_i64(c->ops.user, reinterpret_cast<int64_t*>(c->d_agree.p), 1, CRDT_REDUCE_MAX,
                                  c->stream))
            return comm_abort(c, "transport error", 2);
        if (lst) return lst;
        HIPCHK(hipMemcpyAsync(c->h_agree.p + 1, c->d_agree.p, 8, hipMemcpyDeviceToHost, c->stream));
        SYNCHK(c, c->stream);
    }
    return c->h_agree.p[1] ? -(int)c->h_agree.p[1] : CRDT_OK;
}

// Leaving a call on an agreed failure: the side streams' queued work reads this call's buffers.
int drain_side(crdt_ctx* c, int st) {
    for (hipStream_t s : {c->sstream, c->ostream, c->stream}) {
        if (!s) continue;
        const int w = comm_wait(c, s);
        if (w == CRDT_E_COMM) return w;                  // (aborted: comm_abort drained them, bounded)
    }
    return st;
}

// ---- map-side combine (order-free sharded merges): route one packed maximum per distinct key ----------
// Owner offsets of the emit items: off[item][o] = entries of owner o in the items before, tot[o] = all.
// Three passes over chunks of 1024 items (sums per chunk and owner; a scan of the chunk sums per owner;
// the items' offsets) — one workgroup per owner scanning every item serially took 0.17 ms at N = 8.
constexpr uint32_t kCombChunk = 1024;
__global__ __launch_bounds__(256) void k_comb_chunk_sum(const uint32_t* __restrict__ ocount, uint32_t n_items,
                                                        uint32_t G, unsigned long long* __restrict__ csum)
{
    __shared__ unsigned long long s_sum[kRouteMaxRanks];
    const uint32_t ch = blockIdx.x, i0 = ch * kCombChunk, i1 = std::min<uint32_t>(n_items, i0 + kCombChunk);
    for (uint32_t o = threadIdx.x; o < G; o += 256) s_sum[o] = 0;
    __syncthreads();
    const uint64_t j1 = (uint64_t)i1 * G;                    // (item, owner) pairs, consecutive in memory
    for (uint64_t j = (uint64_t)i0 * G + threadIdx.x; j < j1; j += 256)
        atomicAdd(&s_sum[j % G], (unsigned long long)ocount[j]);
    __syncthreads();
    for (uint32_t o = threadIdx.x; o < G; o += 256) csum[(uint64_t)ch * G + o] = s_sum[o];
}

__global__ __launch_bounds__(256) void k_comb_chunk_scan(unsigned long long* __restrict__ csum, uint32_t n_chunks,
                                                         uint32_t G, unsigned long long* __restrict__ tot)
{
    for (uint32_t o = blockIdx.x * 256 + threadIdx.x; o < G; o += gridDim.x * 256) {
        unsigned long long run = 0;
        for (uint32_t ch = 0; ch < n_chunks; ++ch) {
            const unsigned long long x = csum[(uint64_t)ch * G + o];
            csum[(uint64_t)ch * G + o] = run;
            run += x;
        }
        tot[o] = run;
    }
}

// One workgroup per chunk, one wave per owner group: the chunk's items in order (a wave-wide scan of
// 64 items at a time).
__global__ __launch_bounds__(256) void k_comb_offsets(const uint32_t* __restrict__ ocount, uint32_t n_items,
                                                      uint32_t G, const unsigned long long* __restrict__ csum,
                                                      uint64_t* __restrict__ off)
{
    const uint32_t ch = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint32_t i0 = ch * kCombChunk, i1 = std::min<uint32_t>(n_items, i0 + kCombChunk);
    for (uint32_t o = w; o < G; o += 4) {
        unsigned long long run = csum[(uint64_t)ch * G + o];
        for (uint32_t b = i0; b < i1; b += 64) {
            const uint32_t i = b + lane;
            const unsigned long long v = i < i1 ? ocount[(uint64_t)i * G + o] : 0ull;
            unsigned long long inc = v;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const unsigned long long u = __shfl_up(inc, d, 64);
                if ((int)lane >= d) inc += u;
            }
            if (i < i1) off[(uint64_t)i * G + o] = run + inc - v;
            run += __shfl(inc, 63, 64);
        }
    }
}

// One workgroup per emit item: its entries go owner-major — slot = key / G, the packed key in the lt
// column — to obase[o] + off[item][o] + (LDS cursor); this rank's own keys straight into the receive
// columns (obase[me] is a receive-column position).
__global__ __launch_bounds__(256) void k_comb_scatter(const uint32_t* __restrict__ ekey, const uint64_t* __restrict__ epk,
                                                      const uint32_t* __restrict__ eval,
                                                      const uint32_t* __restrict__ icount,
                                                      const uint32_t* __restrict__ ibase, const uint64_t* __restrict__ off,
                                                      const unsigned long long* __restrict__ obase, uint32_t G, uint32_t me,
                                                      uint32_t* __restrict__ s_slot, int64_t* __restrict__ s_pk,
                                                      uint32_t* __restrict__ s_val, uint32_t* __restrict__ r_slot,
                                                      int64_t* __restrict__ r_pk, uint32_t* __restrict__ r_val)
{
    __shared__ unsigned long long cur[kRouteMaxRanks];
    const uint32_t item = blockIdx.x;
    const uint32_t n = icount[item];
    if (!n) return;
    for (uint32_t o = threadIdx.x; o < G; o += 256) cur[o] = obase[o] + off[(uint64_t)item * G + o];
    __syncthreads();
    const uint64_t base = ibase[item];
    for (uint32_t e = threadIdx.x; e < n; e += 256) {
        const uint32_t k = ekey[base + e];
        const uint32_t o = k % G;
        const unsigned long long pos = atomicAdd(&cur[o], 1ull);
        if (o == me) {
            r_slot[pos] = k / G;
            r_pk[pos] = (int64_t)epk[base + e];
            r_val[pos] = eval[base + e];
        } else {
            s_slot[pos] = k / G;
            s_pk[pos] = (int64_t)epk[base + e];
            s_val[pos] = eval[base + e];
        }
    }
}

// ---- the routed level-1 partition (order-free sharded merges; VERDICT r3 item 1) --------------------
// Routing records and partitioning them again at their owner reads and writes every record twice.  Here
// each rank partitions its home records ONCE, by (owner, owner's level-1 digit) — KeyMap: digit =
// owner << dsh | slot >> 20, G x 2^dsh <= 256 digits, one 8-bit pass — writing the owners' 14-B level-1
// records (12-B payload packed against the all-gathered frame + 2-B key column) owner-major into one
// buffer.  The peers' parts cross the exchange as they are; the own part is not moved.  Each owner then
// starts at level 2: its level-1 bucket d is the G pieces (d, source s) — its own piece in the send area,
// the peers' in the receive area behind it — which level 2 tiles as G x 2^dsh segments (no tile straddles
// one), numbered digit by digit, so every final bucket still comes out contiguous.  Per record: the
// single-GPU path's bytes (20 B read + 14 B written at the sender, level 2 and the resolve at the owner)
// plus 14 B over the link (DESIGN.md §7).
inline uint32_t route_l1_dsh(uint64_t cap) {          // an owner's level-1 digits: 2^dsh buckets of 2^20 slots
    uint32_t d = 0;
    while ((1ull << (d + 20)) < cap) ++d;
    return d;
}

bool route_l1_ok(const crdt_ctx* c) {
    const uint32_t G = c->n_ranks;
    return c->route_l1 && G > 1 && (G & (G - 1)) == 0 && c->cap > (1ull << 20) && c->cap <= kSortedMaxCap &&
           ((uint64_t)G << route_l1_dsh(c->cap)) <= kDigits && !(c->form_off & (kFormNoKey8 | kFormNoKey16));
}

// cnt[o][p][d] = this rank's applied records of piece p for owner o's level-1 digit d (sums of the routed
// partition's per-chunk digit counts over the piece's chunks); the own rows also into the received matrix.
__global__ __launch_bounds__(256) void k_rl1_counts(const uint32_t* __restrict__ part, const uint32_t* __restrict__ cbase,
                                                    uint32_t P, uint32_t GD, uint32_t dsh, uint32_t me,
                                                    unsigned long long* __restrict__ scnt,
                                                    unsigned long long* __restrict__ rcnt)
{
    const uint32_t p = blockIdx.x, D = 1u << dsh;
    const uint32_t c0 = cbase[p], c1 = cbase[p + 1];
    for (uint32_t x = threadIdx.x; x < GD; x += 256) {
        unsigned long long v = 0;
        for (uint32_t ch = c0; ch < c1; ++ch) v += part[(uint64_t)ch * kDigits + x];
        const uint32_t o = x >> dsh, d = x & (D - 1);
        const uint64_t i = ((uint64_t)o * P + p) * D + d;
        scnt[i] = v;
        if (o == me) rcnt[i] = v;
    }
}

// Level 2 of route_l1's level-1 records over ngrp groups of nsrc segments each — segment x = g * nsrc + s holds
// [beg[x], beg[x] + len[x]) of c->rl_rec / c->rl_k16 — tiled segment by segment, group-major, so every final
// bucket (group g, level-2 digit) comes out contiguous in os.rec2 / os.kj2: the host plan and the buffers.
int l2_prep(crdt_ctx* c, Rl1Scratch& os, uint32_t ngrp, uint32_t nsrc, const uint64_t* beg, const uint64_t* len) {
    const size_t nsg = (size_t)ngrp * nsrc;
    const size_t u32w = ((nsg + 1) + 2 * ((size_t)ngrp + 1) + 1) / 2;   // tb2 [nsg + 1], stb [ngrp + 1], scb [ngrp + 1]
    const size_t pw = 2 * nsg + u32w + ngrp;                            // + spos [ngrp]
    HIPALLOC(os.hplan.ensure(pw));
    HIPALLOC(os.plan.ensure(pw));
    uint64_t* g_beg = os.hplan.p;
    uint64_t* g_end = g_beg + nsg;
    uint32_t* tb2 = reinterpret_cast<uint32_t*>(g_end + nsg);
    uint32_t* stb = tb2 + nsg + 1;
    uint32_t* scb = stb + ngrp + 1;
    uint64_t* spos = os.hplan.p + 2 * nsg + u32w;
    const uint32_t ts2 = (uint32_t)kPTile2;
    uint32_t nt2 = 0, nc2 = 0;
    uint64_t pos = 0;
    for (uint32_t g = 0; g < ngrp; ++g) {
        stb[g] = nt2;
        scb[g] = nc2;
        spos[g] = pos;
        for (uint32_t s = 0; s < nsrc; ++s) {
            const size_t x = (size_t)g * nsrc + s;
            g_beg[x] = beg[x];
            g_end[x] = beg[x] + len[x];
            pos += len[x];
            tb2[x] = nt2;
            nt2 += (uint32_t)((len[x] + ts2 - 1) / ts2);
        }
        nc2 += (nt2 - stb[g] + kChunkTiles - 1) / kChunkTiles;
    }
    tb2[nsg] = nt2;
    stb[ngrp] = nt2;
    scb[ngrp] = nc2;
    os.pw = pw;
    os.u32w = u32w;
    os.nt2 = nt2;
    os.nc2 = nc2;
    os.ngrp = ngrp;
    os.nsg = nsg;
    os.nw = pos;
    HIPALLOC(os.hist.ensure((size_t)std::max<uint32_t>(nt2, 1) * kDigits));
    HIPALLOC(os.toff.ensure((size_t)std::max<uint32_t>(nt2, 1) * kDigits));
    HIPALLOC(os.part.ensure((size_t)std::max<uint32_t>(nc2, 1) * kDigits));
    HIPALLOC(os.choff.ensure((size_t)std::max<uint32_t>(nc2, 1) * kDigits));
    HIPALLOC(os.dstart2.ensure((size_t)ngrp * kDigits + 1));
    HIPALLOC(os.tseg.ensure(std::max<uint32_t>(nt2, 1)));
    HIPALLOC(os.rec2.ensure((3 * pos + 3) / 4 + kPartPad));             // 12-B payloads
    HIPALLOC(os.kj2.ensure(pos / 4 + 1 + kPartPad));                      // 1-B key column
    // the packed resolve's work items and split buckets' part states
    const ItemGeom g = item_geom(ngrp * kDigits, pos);
    HIPALLOC(os.ibase.ensure(g.ibase_units));
    HIPALLOC(os.kslt.ensure(g.ksn));
    HIPALLOC(os.ksu32.ensure(g.ksn));
    HIPALLOC(os.ibucket.ensure(g.max_items));
    return CRDT_OK;
}

// The level-2 kernels of a plan l2_prep made (its plan copied to the device first), on `stream`.
int l2_launch(crdt_ctx* c, Rl1Scratch& os, hipStream_t stream) {
    const uint32_t ngrp = os.ngrp, nt2 = os.nt2, nc2 = os.nc2;
    const size_t nsg = os.nsg;
    HIPCHK(hipMemcpyAsync(os.plan.p, os.hplan.p, os.pw * sizeof(uint64_t), hipMemcpyHostToDevice, stream));
    const uint64_t* d_gbeg = os.plan.p;
    const uint64_t* d_gend = os.plan.p + nsg;
    const uint32_t* d_tb2 = reinterpret_cast<const uint32_t*>(os.plan.p + 2 * nsg);
    const uint32_t* d_stb = d_tb2 + nsg + 1;
    const uint32_t* d_scb = d_stb + ngrp + 1;
    const uint64_t* d_spos = os.plan.p + 2 * nsg + os.u32w;
    const TileMap tm2{d_gbeg, d_gend, d_tb2, os.tseg.p, nullptr, (uint32_t)nsg, (uint32_t)kPTile2};
    const ScanMap sm2{d_stb, d_scb, d_spos, ngrp};
    if (nt2) {
        k_seg_index<<<std::min<uint32_t>(grid_for(nt2, 256), 4096), 256, 0, stream>>>(d_tb2, (uint32_t)nsg, nt2,
                                                                                     os.tseg.p);
        // (the compact form: 1-B level-2 digits beside the 12-B records)
        launch_l2_hist(c->rl1_cmp ? kH2Digit8 : kH2Wide8K, c->rl_k16.p, tm2, nt2, c, os.hist.p, stream);
        k_scan_part<<<nc2, 256, 0, stream>>>(os.hist.p, sm2, os.part.p);
    }
    k_scan_seg<<<ngrp, 256, 0, stream>>>(os.part.p, sm2, os.choff.p, os.dstart2.p, nullptr);
    if (nt2) {
        k_scan_tiles<<<nc2, 256, 0, stream>>>(os.hist.p, os.choff.p, sm2, os.dstart2.p, os.toff.p);
        launch_scatter2(false, true, c->rl1_cmp, true, true, c->rl_rec.p, c->rl_k16.p, tm2, nt2, os.toff.p, os.rec2.p,
                               os.kj2.p, c->xcd_map, form_reverse(c) ? os.hist.p : nullptr, stream);
    }
    HIPCHK(hipGetLastError());
    return CRDT_OK;
}

// The owner's level 2 + packed resolve of piece q (route_l1) with the scratch set os: its level-1 bucket d is
// the G pieces (d, source s) — counts h_r[s][q][d], the source's part starting at prd[q][s] (the own part in
// the send area) — tiled as G x D segments, digit-major, so every final bucket comes out contiguous.
// rl1_owner_prep: the host plan and every buffer (before the record exchanges: its failures are agreed);
// rl1_owner_launch: the kernels on `stream`; rows at or above hw are the fill.  timed: windows 2 / 3.
int rl1_owner_prep(crdt_ctx* c, Rl1Scratch& os, uint32_t q, uint32_t P, const uint64_t* h_r,
                   const std::vector<uint64_t>& prd) {
    const uint32_t G = c->n_ranks, dsh = route_l1_dsh(c->cap), D = 1u << dsh;
    std::vector<uint64_t> beg((size_t)D * G), len((size_t)D * G);
    std::vector<uint64_t> run(prd.begin() + (size_t)q * G, prd.begin() + (size_t)(q + 1) * G);
    for (uint32_t d = 0; d < D; ++d)
        for (uint32_t s = 0; s < G; ++s) {
            const size_t x = (size_t)d * G + s;
            len[x] = h_r[((size_t)s * P + q) * D + d];
            beg[x] = run[s];
            run[s] += len[x];
        }
    return l2_prep(c, os, D, G, beg.data(), len.data());
}

int rl1_owner_launch(crdt_ctx* c, Rl1Scratch& os, const PackFrame& pf, hipStream_t stream, uint64_t hw, bool timed) {
    const uint64_t nw = os.nw;
    if (timed) ev_record(c, ev_window(2, false));
    int st = l2_launch(c, os, stream);
    if (st) return st;
    if (timed) ev_record(c, ev_window(2, true));
    const ItemGeom g = item_geom(os.ngrp * kDigits, nw, os.ibase.p);
    const PackedItems a{os.dstart2.p, g, os.ibucket.p, reinterpret_cast<const Rec12*>(os.rec2.p), os.kj2.p, c->table,
                        c->cap, c->d_Rj.p, reinterpret_cast<uint64_t*>(os.kslt.p), os.ksu32.p, pf, c->d_misc};
    if (timed) ev_record(c, ev_window(3, false));
    k_bucket_items<<<(g.nb + 1023) / 1024, 1024, 0, stream>>>(a.bst, g.nb, g.ib, g.hb, g.hot, c->d_misc);
    k_seg_index<<<std::min<uint32_t>(grid_for(g.max_items, 256), 4096), 256, 0, stream>>>(g.ib, g.nb, g.max_items,
                                                                                        os.ibucket.p);
    launch_packed_fold(a, c->rl1_cmp, true, g.max_items, stream, hw, 0, nullptr);
    k_part_carry_packed<false><<<dim3(kSKeys / 256, g.max_hot), 256, 0, stream>>>(
        g.hot, g.ib, g.hb, c->table, c->cap, hw, a.ps_key, a.ps_val, c->d_Rj.p, 0, pf, c->d_misc);
    launch_packed_dense(a, c->rl1_cmp, true, true, g.max_items, stream, hw, 0, nullptr, c->sparse_t, false);
    if (timed) ev_record(c, ev_window(3, true));
    HIPCHK(hipGetLastError());
    return CRDT_OK;
}

// ---- route_l1's head fold (the tuner's fifth way; CRDT_ROUTE_L1=2) ---------------------------------------
// A Zipf fan-in's hot keys sit in every owner's first level-1 digits (digit d: slots [d << 20, (d + 1) << 20);
// digit 0 alone holds 49 % of the 1B fan-in's records at G = 8) and repeat across a rank's home changesets,
// so every rank folds the records of the first Dh digits to one packed maximum per key before sending.  Dh
// comes from the job's records per digit (summed over owners, pieces and ranks beside the count exchange,
// so every rank picks the same): the leading digits whose records per rank per slot reach kHeadDensity.
// The fold: level 2 over the groups (owner o, digit d) — the runs of every piece in the send area — the
// map-side combine's emitting resolve (an absent table, bucket rows numbered (o * Dh + d) << 20 | low slot
// bits: EmitOut::osh = 20, one emit "owner" per group), and k_head_scatter writing each group's maxima back
// as 14-B level-1 records, owner-major and digit-minor — the peers' into the head send buffers, the own
// into its place in the receive area.  The pieces then carry digits Dh .. D-1 only, and the folded head
// crosses the exchange after them as one more piece (its per-digit counts first: the fold decides them).
// The fold is a maximum and the packed key carries the changeset (order-free form), so folding changes
// nothing but the bytes; the head's keys are disjoint from every piece's, so the owners apply it in any
// order relative to the pieces.
constexpr double kHeadDensity = 1.0;    // records per rank per slot of a digit worth folding at the sender

// per-digit records of this rank (summed over owners and pieces): dt[d], then SUM-reduced over the ranks
__global__ void k_rl1_dtot(const unsigned long long* __restrict__ scnt, uint32_t P, uint32_t G, uint32_t D,
                           unsigned long long* __restrict__ dt)
{
    for (uint32_t d = threadIdx.x; d < D; d += blockDim.x) {
        unsigned long long v = 0;
        for (uint32_t o = 0; o < G; ++o)
            for (uint32_t p = 0; p < P; ++p) v += scnt[((uint64_t)o * P + p) * D + d];
        dt[d] = v;
    }
}

// Bases of the folded entries per group g = o * Dh + d: the peers' runs back to back in the head send buffers
// (owner-major, digit-minor), the own runs from own_pos of the receive area; the send counts (Dh words per
// peer) and the own counts (Dh words).
__global__ void k_head_bases(const unsigned long long* __restrict__ tot, uint32_t G, uint32_t Dh, uint32_t me,
                             unsigned long long own_pos, unsigned long long* __restrict__ obase,
                             unsigned long long* __restrict__ scnt, unsigned long long* __restrict__ own)
{
    if (threadIdx.x != 0) return;
    unsigned long long run = 0, orun = own_pos;
    for (uint32_t g = 0; g < G * Dh; ++g) {
        if (g / Dh == me) {
            obase[g] = orun;
            orun += tot[g];
            scnt[g] = 0;
            own[g - me * Dh] = tot[g];
        } else {
            obase[g] = run;
            scnt[g] = tot[g];
            run += tot[g];
        }
    }
}

// One workgroup per emit item (every item's entries belong to one group: its bucket's): entry e of the item
// goes to obase[g] + off[item][g] + e as a level-1 record — 12-B payload {packed key lo, packed key hi | slot
// bits [0, 4) << 28, value handle} and the 2-B key column (slot bits [4, 20)), the form k_part_scatter1 writes
// (the digit is the run's).
__global__ __launch_bounds__(256) void k_head_scatter(const uint32_t* __restrict__ ekey, const uint64_t* __restrict__ epk,
                                                      const uint32_t* __restrict__ eval,
                                                      const uint32_t* __restrict__ icount,
                                                      const uint32_t* __restrict__ ibase, const uint64_t* __restrict__ off,
                                                      const unsigned long long* __restrict__ obase, uint32_t GD,
                                                      uint32_t Dh, uint32_t me, uint32_t* __restrict__ srec,
                                                      uint16_t* __restrict__ sk16, uint32_t* __restrict__ rrec,
                                                      uint16_t* __restrict__ rk16, uint32_t cmp)
{
    const uint32_t item = blockIdx.x;
    const uint32_t n = icount[item];
    if (!n) return;
    const uint64_t base = ibase[item];
    const uint32_t g = ekey[base] >> 20;
    const uint64_t at = obase[g] + off[(uint64_t)item * GD + g];
    uint32_t* __restrict__ rec = g / Dh == me ? rrec : srec;
    uint16_t* __restrict__ k16 = g / Dh == me ? rk16 : sk16;
    for (uint32_t e = threadIdx.x; e < n; e += 256) {
        const uint32_t sl = ekey[base + e] & 0xFFFFFu;
        const uint64_t pk = epk[base + e];
        const uint64_t pos = at + e;
        rec[3 * pos] = (uint32_t)pk;
        rec[3 * pos + 2] = eval[base + e];
        if (cmp) {              // the compact form: the slot in the word, the level-2 digit in a 1-B column
            rec[3 * pos + 1] = (uint32_t)(pk >> 32) | (sl << (kCKeyShift - 32));
            reinterpret_cast<uint8_t*>(k16)[pos] = (uint8_t)(sl >> 12);
        } else {
            rec[3 * pos + 1] = (uint32_t)(pk >> 32) | ((sl & 15u) << 28);
            k16[pos] = (uint16_t)(sl >> 4);
        }
    }
}

// The fold's plan and buffers (before the record exchanges: a failure is agreed there).  Segment (g, q), group
// g = o * Dh + d: this rank's records of owner o's digit d in piece q, hs0[g * P + q] of them at hb[g * P + q]
// of the send area.  send_cap: the folded entries bound for the peers, at most (records, 2^20 keys per group).
int rl1_head_prep(crdt_ctx* c, uint32_t P, uint32_t Dh, const std::vector<uint64_t>& hb,
                  const std::vector<uint64_t>& hs0, uint64_t send_cap) {
    const uint32_t G = c->n_ranks, GD = G * Dh;
    int st = l2_prep(c, c->rl_hf, GD, P, hb.data(), hs0.data());
    if (st) return st;
    const uint64_t nw = c->rl_hf.nw;
    const uint32_t nb = GD * kDigits;
    const ItemGeom g = item_geom(nb, nw);
    const uint32_t n_items = g.max_items + g.max_hot * (kSKeys / 256);
    const size_t slots = (size_t)std::min<uint64_t>(nw, (uint64_t)nb * kSKeys) + 1;
    HIPALLOC(c->e_bbase.ensure(nb));
    HIPALLOC(c->e_key.ensure(slots));
    HIPALLOC(c->e_pk.ensure(slots));
    HIPALLOC(c->e_val.ensure(slots));
    HIPALLOC(c->e_icnt.ensure((size_t)n_items * (2 + GD)));
    HIPALLOC(c->e_off.ensure(((size_t)n_items + 1) * GD));
    HIPALLOC(c->e_csum.ensure((size_t)((n_items + kCombChunk - 1) / kCombChunk) * GD));
    HIPALLOC(c->e_cnt.ensure(2 * (size_t)GD + 2));
    HIPALLOC(c->e_cur.ensure(GD));
    HIPALLOC(c->rl_hrec.ensure(3 * send_cap + 3));
    HIPALLOC(c->rl_hk16.ensure(send_cap + 1));
    HIPALLOC(c->rl_hcnt.ensure(2 * (size_t)GD + Dh));
    HIPALLOC(c->h_hcnt.ensure(2 * (size_t)GD + Dh));
    if (!c->rl_evh) HIPCHK(hipEventCreateWithFlags(&c->rl_evh, hipEventDisableTiming));
    return CRDT_OK;
}

// The fold's kernels on `stream` (behind every piece's partition): level 2, the emitting resolve, the groups'
// offsets, the send counts (c->rl_hcnt: [G][Dh] sent, [G][Dh] received (the exchange fills them), [Dh] own)
// and the level-1 records; the own runs go to own_pos of the receive area.
int rl1_head_launch(crdt_ctx* c, const PackFrame& pf, uint32_t Dh, uint64_t own_pos, hipStream_t stream) {
    Rl1Scratch& hf = c->rl_hf;
    const uint32_t G = c->n_ranks, me = c->rank, GD = G * Dh;
    int st = l2_launch(c, hf, stream);
    if (st) return st;
    const ItemGeom g = item_geom(GD * kDigits, hf.nw, hf.ibase.p);
    const uint32_t n_items = g.max_items + g.max_hot * (kSKeys / 256);
    EmitOut eo{};
    eo.G = GD;                                          // one emit "owner" per group (o, d)
    eo.osh = 20;
    eo.key = c->e_key.p;
    eo.pk = c->e_pk.p;
    eo.val = c->e_val.p;
    eo.bbase = c->e_bbase.p;
    eo.icount = c->e_icnt.p;
    eo.ibase = c->e_icnt.p + n_items;
    eo.ocount = c->e_icnt.p + 2 * (size_t)n_items;
    eo.item0 = g.max_items;
    eo.n_items = n_items;
    HIPCHK(hipMemsetAsync(c->e_icnt.p, 0, (size_t)n_items * (2 + GD) * sizeof(uint32_t), stream));
    const uint64_t hcap = (uint64_t)GD << 20;           // rows g << 20 | low slot bits, all absent (hw = 0: no table)
    const PackedItems a{hf.dstart2.p, g, hf.ibucket.p, reinterpret_cast<const Rec12*>(hf.rec2.p), hf.kj2.p, c->table,
                        hcap, c->d_Rj.p, reinterpret_cast<uint64_t*>(hf.kslt.p), hf.ksu32.p, pf, c->d_misc};
    k_bucket_items<<<(g.nb + 1023) / 1024, 1024, 0, stream>>>(a.bst, g.nb, g.ib, g.hb, g.hot, c->d_misc, c->e_bbase.p);
    k_seg_index<<<std::min<uint32_t>(grid_for(g.max_items, 256), 4096), 256, 0, stream>>>(g.ib, g.nb, g.max_items,
                                                                                        hf.ibucket.p);
    launch_packed_fold(a, c->rl1_cmp, true, g.max_items, stream, 0, 0, nullptr);
    launch_packed_emit(a, c->rl1_cmp, true, g.max_items, stream, 0, eo);
    k_part_carry_packed<true><<<dim3(kSKeys / 256, g.max_hot), 256, 0, stream>>>(
        g.hot, g.ib, g.hb, c->table, hcap, 0, a.ps_key, a.ps_val, c->d_Rj.p, 0, pf, c->d_misc, eo);
    unsigned long long* d_tot = c->e_cnt.p + 2;
    const uint32_t nch = (n_items + kCombChunk - 1) / kCombChunk;
    k_comb_chunk_sum<<<nch, 256, 0, stream>>>(eo.ocount, n_items, GD, c->e_csum.p);
    k_comb_chunk_scan<<<std::max<uint32_t>(1, (GD + 255) / 256), 256, 0, stream>>>(c->e_csum.p, nch, GD, d_tot);
    k_comb_offsets<<<nch, 256, 0, stream>>>(eo.ocount, n_items, GD, c->e_csum.p, c->e_off.p);
    k_head_bases<<<1, 64, 0, stream>>>(d_tot, G, Dh, me, own_pos, c->e_cur.p, c->rl_hcnt.p, c->rl_hcnt.p + 2 * GD);
    k_head_scatter<<<n_items, 256, 0, stream>>>(eo.key, eo.pk, eo.val, eo.icount, eo.ibase, c->e_off.p, c->e_cur.p, GD,
                                                Dh, me, c->rl_hrec.p, c->rl_hk16.p, c->rl_rec.p, c->rl_k16.p,
                                                c->rl1_cmp ? 1u : 0u);
    HIPCHK(hipGetLastError());
    return CRDT_OK;
}

// The routed partition and the owners' level 2 + resolve (the order-free packed form, one window of
// changesets, the global frame pf).  Called by merge_sharded after the clock phase; ends with finish_apply.
// The home changesets go in P pieces of about equal records (c->rl1_call_pieces: 2 by default, 4 as the
// tuner's third way, 1 with CRDT_RL1_SPLIT=0), partitioned in order on a side stream; piece q crosses the
// exchange on the ctx stream (every collective stays there, in the same order on every rank) while piece
// q+1 is partitioned and the owner resolves piece q-1 on a third stream; the last piece's owner work follows
// on the ctx stream.  Failures: the preparation's beside the count exchange, the receive area's and the
// owners' buffers' by comm_agree before the first record exchange (the header of this file).
int route_l1(crdt_ctx* c, const Cols& cols, const uint64_t* offsets, int64_t wall, const PackFrame& pf_in,
             crdt_result* out) {
    // the compact form (round 6; sorted_path.inc PackFrame::cb) on the all-gathered frame and counter maximum
    // (the same on every rank): 12-B level-1 records + a 1-B digit column — 13 B per record over the links
    PackFrame pf = pf_in;
    c->rl1_cmp = false;
    if (!(c->form_off & (kFormNoCompact | kFormNoVecLoads))) {
        const PackFrame cf = compact_frame(pf_in, (uint32_t)std::min<unsigned long long>(c->h_misc->fr_cmax, 0xFFFFull),
                                           c->plan_R);
        if (cf.cb) {
            pf = cf;
            c->rl1_cmp = true;
        }
    }
    c->last_compact = c->rl1_cmp;
    const uint32_t kcol = c->rl1_cmp ? 1u : 2u;      // the level-1 key column's bytes per record
    const uint32_t R = c->plan_R, G = c->n_ranks, me = c->rank;
    const uint32_t dsh = route_l1_dsh(c->cap), D = 1u << dsh, GD = G << dsh;
    const KeyMap km{route_bits(G), dsh};
    const uint64_t n = offsets[R];
    int st, lst = CRDT_OK;
    // the stop point first: the partition leaves out the changesets >= stop (k_part_hist / scatter1)
    k_resolve<<<1, 64, 0, c->stream>>>(c->d_event.p, R, wall, c->canonical, c->d_Rj.p, c->d_Cj.p, c->d_misc);
    c->resolved = false;
    c->windows.clear();
    c->apply_total = 1;
    const bool ph = c->timing;
    if (ph) ev_record(c, ev_window(0, false));
    c->last_sorted = c->last_packed = c->last_key8 = c->last_key16 = true;
    c->last_ordered = c->last_flagged = c->last_combined = false;
    c->last_hw = c->hw_read < c->cap;
    c->sorted_phases = false;
    c->key_end_valid = true;
    // piece q = changesets [pj[q], pj[q + 1]): cut at the changesets nearest to q / P of the records
    uint32_t pj[kRl1MaxPieces + 1], P = 0;
    pj[0] = 0;
    const uint32_t want = std::min<uint32_t>(std::max<uint32_t>(c->rl1_call_pieces, 1u), kRl1MaxPieces);
    if (want > 1 && R >= 2 && n >= (1u << 20)) {
        uint32_t j = 0;
        for (uint32_t k = 1; k < want; ++k) {
            const uint64_t target = n * k / want;
            while (j < R && offsets[j] < target) ++j;
            if (j > pj[P] && j < R) pj[++P] = j;
        }
    }
    pj[++P] = R;
    c->last_rl1_pieces = P;
    const size_t cw = (size_t)GD * P;                   // per-(owner, piece, digit) counts, each direction

    // ---- sender: level-1 tiles over the home changesets (one tiling; a scan segment per piece)
    const uint32_t nseg = R;
    const size_t u32_words = (2 * (size_t)nseg + 2) / 2;         // seg_j [nseg] + tb [nseg + 1]
    const size_t words = 2 * (size_t)nseg + u32_words + 2 * (size_t)P + 1;   // + tbase/cbase [P + 1], seg_pos [P]
    const size_t tail = 2 * (size_t)nseg + u32_words;
    uint32_t nt1 = 0, nc1 = 0;
    std::vector<uint32_t> tb(nseg + 1);
    for (uint32_t s = 0; s <= nseg; ++s) {
        tb[s] = nt1;
        if (s < nseg) nt1 += (uint32_t)((offsets[s + 1] - offsets[s] + l1_plan_tile(c) - 1) / l1_plan_tile(c));
    }
    for (uint32_t q = 0; q < P; ++q) nc1 += (tb[pj[q + 1]] - tb[pj[q]] + kChunkTiles - 1) / kChunkTiles;
    // the preparation's buffers (a failure: this rank's status word, reduced beside the count exchange)
    auto prep = [&]() -> int {
        HIPALLOC(c->h_pplan.ensure(words));
        HIPALLOC(c->p_plan.ensure(words));
        HIPALLOC(c->p_hist.ensure((size_t)std::max<uint32_t>(nt1, 1) * kDigits));
        HIPALLOC(c->p_toff.ensure((size_t)std::max<uint32_t>(nt1, 1) * kDigits));
        HIPALLOC(c->p_part.ensure((size_t)std::max<uint32_t>(nc1, 1) * kDigits));
        HIPALLOC(c->p_choff.ensure((size_t)std::max<uint32_t>(nc1, 1) * kDigits));
        HIPALLOC(c->p_dstart1.ensure((size_t)P * kDigits + 1));
        HIPALLOC(c->p_tseg.ensure(std::max<uint32_t>(nt1, 1)));
        // the partition buffer: the send area [0, n), the peers' parts behind it (room for as many again + 25 %;
        // grown below, keeping the send area, when a call receives more)
        if (c->rl_cap < 2 * n + n / 4 + 1) {
            const uint64_t w = 2 * n + n / 4 + 1;
            HIPALLOC(c->rl_rec.ensure(3 * w));
            HIPALLOC(c->rl_k16.ensure(w));
            c->rl_cap = w;
        }
        if (!c->sstream) HIPCHK(hipStreamCreateWithFlags(&c->sstream, hipStreamNonBlocking));
        if (!c->ostream) HIPCHK(hipStreamCreateWithFlags(&c->ostream, hipStreamNonBlocking));
        for (uint32_t q = 0; q < kRl1MaxPieces; ++q) {
            if (!c->rl_evs[q]) HIPCHK(hipEventCreateWithFlags(&c->rl_evs[q], hipEventDisableTiming));
            if (!c->rl_evx[q]) HIPCHK(hipEventCreateWithFlags(&c->rl_evx[q], hipEventDisableTiming));
        }
        if (!c->rl_evo) HIPCHK(hipEventCreateWithFlags(&c->rl_evo, hipEventDisableTiming));
        if (!c->route_ev) HIPCHK(hipEventCreateWithFlags(&c->route_ev, hipEventDisableTiming));
        return inject_fail(c, kFailRoutePrep) ? CRDT_E_NOMEM : CRDT_OK;
    };
    lst = prep();
    unsigned long long* d_cnt = c->d_rl1cnt.p;          // [send cw][recv cw][status] (comm_attach)
    const uint32_t* hist1 = c->p_hist.p;
    const uint32_t* d_tb1 = nullptr;
    TileMap tm1{};
    // the plan's upload and the counting kernels (a HIP failure here: this rank's status, carried by the
    // status word beside the count exchange, with zero counts)
    auto counts = [&]() -> int {
        uint64_t* h_beg = c->h_pplan.p;
        uint64_t* h_end = c->h_pplan.p + nseg;
        uint32_t* h_sj = reinterpret_cast<uint32_t*>(c->h_pplan.p + 2 * (size_t)nseg);
        uint32_t* h_tb = h_sj + nseg;
        for (uint32_t s = 0; s <= nseg; ++s) {
            h_tb[s] = tb[s];
            if (s < nseg) { h_beg[s] = offsets[s]; h_end[s] = offsets[s + 1]; h_sj[s] = s; }
        }
        uint32_t* sm_t = reinterpret_cast<uint32_t*>(c->h_pplan.p + tail);          // [P + 1]
        uint32_t* sm_c = sm_t + (P + 1);                                             // [P + 1]
        uint64_t* sm_p = c->h_pplan.p + tail + (P + 1);                              // [P]
        uint32_t cc = 0;
        for (uint32_t q = 0; q < P; ++q) {
            sm_t[q] = tb[pj[q]];
            sm_c[q] = cc;
            sm_p[q] = offsets[pj[q]];                   // piece q's part of the send area starts here
            cc += (tb[pj[q + 1]] - tb[pj[q]] + kChunkTiles - 1) / kChunkTiles;
        }
        sm_t[P] = nt1;
        sm_c[P] = nc1;
        HIPCHK(hipMemcpyAsync(c->p_plan.p, c->h_pplan.p, words * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
        const uint64_t* d_beg = c->p_plan.p;
        const uint64_t* d_end = c->p_plan.p + nseg;
        const uint32_t* d_sj = reinterpret_cast<const uint32_t*>(c->p_plan.p + 2 * (size_t)nseg);
        d_tb1 = d_sj + nseg;
        if (nt1)
            k_seg_index<<<std::min<uint32_t>(grid_for(nt1, 256), 4096), 256, 0, c->stream>>>(d_tb1, nseg, nt1, c->p_tseg.p);
        tm1 = TileMap{d_beg, d_end, d_tb1, c->p_tseg.p, d_sj, nseg, l1_plan_tile(c)};
        const uint32_t* d_smt = reinterpret_cast<const uint32_t*>(c->p_plan.p + tail);
        const ScanMap sm1{d_smt, d_smt + (P + 1), c->p_plan.p + tail + (P + 1), P};
        // the level-1 histogram: counted by the scan with this key map (phase_scan's route_km; the tiles of the
        // changesets >= stop cleared now) or here
        const bool h1 = c->hist1_fused && c->hist1_routed && c->hist1_key == cols.key && nt1 == c->plan_ptiles;
        hist1 = h1 ? c->p_hist1.p : c->p_hist.p;
        c->last_hist1_fused = h1;
        if (nt1) {
            if (h1)
                k_hist_trim<<<256, 256, 0, c->stream>>>(c->p_hist1.p, c->d_ptb, R, c->d_misc);
            else
                k_part_hist<true><<<nt1, kHThreads, 0, c->stream>>>(cols.key, tm1, 0, c->d_misc, c->cap, 20u, c->p_hist.p, km);
            k_scan_part<<<nc1, 256, 0, c->stream>>>(hist1, sm1, c->p_part.p);
        } else {
            HIPCHK(hipMemsetAsync(c->p_part.p, 0, kDigits * sizeof(uint32_t), c->stream));
        }
        k_scan_seg<<<P, 256, 0, c->stream>>>(c->p_part.p, sm1, c->p_choff.p, c->p_dstart1.p, nullptr);
        if (nt1) k_scan_tiles<<<nc1, 256, 0, c->stream>>>(hist1, c->p_choff.p, sm1, c->p_dstart1.p, c->p_toff.p);
        k_rl1_counts<<<P, 256, 0, c->stream>>>(c->p_part.p, d_smt + (P + 1), P, GD, dsh, me, d_cnt, d_cnt + cw);
        HIPCHK(hipGetLastError());
        return CRDT_OK;
    };
    if (!lst) lst = counts();
    if (lst) HIPLST(hipMemsetAsync(d_cnt, 0, 2 * cw * sizeof(uint64_t), c->stream));
    // owner o's P x D count words go to it; every rank's status beside them (MAX)
    std::vector<uint64_t> sc(G), sd(G), rcn(G), rd(G);
    for (uint32_t d = 0; d < G; ++d) {
        sc[d] = rcn[d] = d == me ? 0 : (uint64_t)P * D;
        sd[d] = rd[d] = (uint64_t)d * P * D;
    }
    test_stall(c, kStallCounts);
    set_phase(c, "route_l1: count exchange");
    {
        const void* s1[1] = {d_cnt};
        void* r1[1] = {d_cnt + cw};
        const uint32_t e8 = 8;
        if ((st = comm_all_to_all(c, 1, s1, r1, &e8, sc.data(), sd.data(), rcn.data(), rd.data(), cw, cw))) return st;
    }
    c->h_agree.p[0] = lst < 0 ? -(long long)lst : 0;
    HIPLST(hipMemcpyAsync(d_cnt + 2 * cw, c->h_agree.p, 8, hipMemcpyHostToDevice, c->stream));
    if ((st = comm_all_reduce(c, reinterpret_cast<long long*>(d_cnt + 2 * cw), 1, CRDT_REDUCE_MAX))) return st;
    // the head fold: the job's records per digit (every rank the same sums: the same folded digits)
    const bool head = c->rl1_call_head;
    if (head) {
        k_rl1_dtot<<<1, 256, 0, c->stream>>>(d_cnt, P, G, D, d_cnt + 2 * cw + 1);
        if ((st = comm_all_reduce(c, reinterpret_cast<long long*>(d_cnt + 2 * cw + 1), D, CRDT_REDUCE_SUM))) return st;
    }
    HIPCHK(hipMemcpyAsync(c->h_rl1cnt.p, d_cnt, (2 * cw + 1 + (head ? D : 0)) * 8, hipMemcpyDeviceToHost, c->stream));
    if (lst) {                                          // (no partition was launched)
        SYNCHK(c, c->stream);
        return c->h_rl1cnt.p[2 * cw] ? -(int)c->h_rl1cnt.p[2 * cw] : lst;
    }
    HIPCHK(hipEventRecord(c->route_ev, c->stream));
    // every piece partitioned on the side stream, in order, behind the scans (the ctx stream stays free for
    // the collectives)
    const bool rev = form_reverse(c);
    HIPCHK(hipEventRecord(c->rl_evo, c->stream));
    HIPCHK(hipStreamWaitEvent(c->sstream, c->rl_evo, 0));
    for (uint32_t q = 0; q < P; ++q) {
        if (ph && q == 0 && ev_window(1, true) < c->events.size())
            HIPCHK(hipEventRecord(c->events[ev_window(1, false)], c->sstream));
        const uint32_t t0 = tb[pj[q]], ntq = tb[pj[q + 1]] - t0;
        if (ntq) {
            TileMap tq = tm1;
            tq.nseg = pj[q + 1];
            tq.tile0 = t0;
            const uint32_t xper = c->xcd_map ? (ntq + kXcds - 1) / kXcds : 0;
            if (c->rl1_cmp)
                k_part_scatter1<true, false, true, kL1Items, true, true, false, true>
                    <<<xcd_grid(ntq, c->xcd_map), kPThreads, 0, c->sstream>>>(
                    cols.key, cols.lt, cols.rank, cols.val, tq, 0, c->d_misc, c->cap, 20u, c->p_toff.p, c->rl_rec.p,
                    c->rl_k16.p, xper, pf, rev ? hist1 : nullptr, nullptr, nullptr, km);
            else
                k_part_scatter1<true, false, true, kL1Items, true><<<xcd_grid(ntq, c->xcd_map), kPThreads, 0, c->sstream>>>(
                    cols.key, cols.lt, cols.rank, cols.val, tq, 0, c->d_misc, c->cap, 20u, c->p_toff.p, c->rl_rec.p,
                    c->rl_k16.p, xper, pf, rev ? hist1 : nullptr, nullptr, nullptr, km);
        }
        if (ph && q == 0 && ev_window(1, true) < c->events.size())
            HIPCHK(hipEventRecord(c->events[ev_window(1, true)], c->sstream));
        HIPCHK(hipEventRecord(c->rl_evs[q], c->sstream));
    }
    HIPLST(hipGetLastError());                          // (a failed launch: agreed by comm_agree below)
    if ((st = comm_wait(c, nullptr, c->route_ev))) return st;   // the counts and the status (the partition runs on)
    if (c->h_rl1cnt.p[2 * cw]) return drain_side(c, -(int)c->h_rl1cnt.p[2 * cw]);
    const uint64_t* h_s = c->h_rl1cnt.p;                // [G][P][D] records this rank sends owner o
    const uint64_t* h_r = c->h_rl1cnt.p + cw;           // [G][P][D] records source s sends here (own: own)
    auto cnt = [&](const uint64_t* m, uint32_t o, uint32_t q, uint32_t d) { return m[((size_t)o * P + q) * D + d]; };
    // the head fold: every owner's first Dh digits leave the pieces (their exchanges and owner passes start at
    // digit Dh) and are folded on the side stream behind the partition, then sent as one more piece.  Dh: the
    // leading digits whose records per rank per slot (the job's, over G owners x G ranks x 2^20 slots) reach
    // kHeadDensity (the same on every rank: the sums were reduced), at least 1
    uint32_t Dh = 0;
    if (head) {
        const uint64_t* dt = c->h_rl1cnt.p + 2 * cw + 1;
        Dh = 1;
        while (Dh < D && (c->rl1_call_all || (double)dt[Dh] >= kHeadDensity * (double)G * G * (double)(1u << 20)))
            ++Dh;
    }
    c->last_rl1_head = head;
    c->last_rl1_head_digits = Dh;
    auto h0 = [&](const uint64_t* m, uint32_t o, uint32_t q) -> uint64_t {
        uint64_t v = 0;
        for (uint32_t d = 0; d < Dh; ++d) v += cnt(m, o, q, d);
        return v;
    };
    // send area: piece q from offsets[pj[q]], owner-major; receive area behind the send area, piece-major
    std::vector<uint64_t> psd((size_t)P * G), psc((size_t)P * G), prd((size_t)P * G), prc((size_t)P * G);
    std::vector<uint64_t> hb((size_t)G * Dh * P), hs0((size_t)G * Dh * P);   // head: [o][d][q] runs (send area)
    uint64_t ro = n, p0 = 0;
    for (uint32_t q = 0; q < P && !lst; ++q) {
        uint64_t at = offsets[pj[q]];
        for (uint32_t o = 0; o < G; ++o) {
            uint64_t a = 0, b = 0;
            for (uint32_t d = 0; d < D; ++d) { a += cnt(h_s, o, q, d); b += cnt(h_r, o, q, d); }
            const uint64_t sh = h0(h_s, o, q), rh = h0(h_r, o, q);
            uint64_t hd = at;
            for (uint32_t d = 0; d < Dh; ++d) {
                hb[((size_t)o * Dh + d) * P + q] = hd;
                hs0[((size_t)o * Dh + d) * P + q] = cnt(h_s, o, q, d);
                hd += cnt(h_s, o, q, d);
            }
            psd[(size_t)q * G + o] = at + sh;
            psc[(size_t)q * G + o] = a - sh;
            at += a;
            if (q == 0) p0 += a;
            prc[(size_t)q * G + o] = b - rh;
            prd[(size_t)q * G + o] = o == me ? psd[(size_t)q * G + o] : ro;   // the own part stays put
            if (o != me) ro += b - rh;
        }
        if (at > offsets[pj[q + 1]]) lst = CRDT_E_INVALID;     // (digit starts cover applied records only)
    }
    // head: the folded runs' receive area behind the pieces' — the own runs (each digit at most its records or
    // 2^20 keys), then each peer's at its bound; the owners' counts of the pieces without the head digits
    const uint64_t ro_tail = ro;
    std::vector<uint64_t> hrb((size_t)G * Dh, 0), hprd(G, 0);
    std::vector<uint64_t> hr_t(h_r, h_r + cw);
    uint64_t hsend = 0, hin = 0;
    if (head) {
        for (uint32_t s = 0; s < G; ++s)
            for (uint32_t d = 0; d < Dh; ++d) {
                uint64_t b = 0, x = 0;
                for (uint32_t q = 0; q < P; ++q) {
                    b += s == me ? cnt(h_s, me, q, d) : cnt(h_r, s, q, d);
                    x += cnt(h_s, s, q, d);
                    hr_t[((size_t)s * P + q) * D + d] = 0;
                }
                hrb[(size_t)s * Dh + d] = std::min<uint64_t>(b, 1ull << 20);
                hin += x;
                if (s != me) hsend += std::min<uint64_t>(x, 1ull << 20);
            }
        auto run_of = [&](uint32_t s) {
            uint64_t v = 0;
            for (uint32_t d = 0; d < Dh; ++d) v += hrb[(size_t)s * Dh + d];
            return v;
        };
        hprd[me] = ro;
        ro += run_of(me);
        for (uint32_t s = 0; s < G; ++s)
            if (s != me) { hprd[s] = ro; ro += run_of(s); }
    }
    // the receive area (grown, keeping the send area the scatters wrote) and every piece's owner buffers
    if (!lst && inject_fail(c, kFailRecv)) lst = CRDT_E_NOMEM;
    if (!lst && ro > c->rl_cap) {
        const uint64_t w = ro + ro / 4;
        DBuf<uint32_t> nrec;
        DBuf<uint16_t> nk;
        if (nrec.ensure(3 * w) != hipSuccess || nk.ensure(w) != hipSuccess) {
            nrec.release();
            nk.release();
            lst = CRDT_E_NOMEM;
        } else {
            HIPLST(hipStreamWaitEvent(c->stream, c->rl_evs[P - 1], 0));    // every piece partitioned
            if (n && !lst) {
                HIPLST(hipMemcpyAsync(nrec.p, c->rl_rec.p, n * 12, hipMemcpyDeviceToDevice, c->stream));
                HIPLST(hipMemcpyAsync(nk.p, c->rl_k16.p, n * kcol, hipMemcpyDeviceToDevice, c->stream));
            }
            if (!lst) lst = comm_wait(c, c->stream);
            if (lst) {                                  // (kept the old buffers: the call fails at comm_agree)
                nrec.release();
                nk.release();
            } else {
            c->rl_rec.release();
            c->rl_k16.release();
            c->rl_rec = nrec; nrec.p = nullptr; nrec.n = 0;
            c->rl_k16 = nk; nk.p = nullptr; nk.n = 0;
            c->rl_cap = w;
            }
        }
    }
    for (uint32_t q = 0; q < P && !lst; ++q) lst = rl1_owner_prep(c, c->rl_os[q], q, P, hr_t.data(), prd);
    Rl1Scratch& hos = c->rl_os[kRl1MaxPieces];         // the owner's pass over the folded head
    std::vector<uint64_t> hr1((size_t)G * D, 0);
    if (head && !lst) {
        lst = rl1_head_prep(c, P, Dh, hb, hs0, hsend);
        for (uint32_t s = 0; s < G; ++s)
            for (uint32_t d = 0; d < Dh; ++d) hr1[(size_t)s * D + d] = hrb[(size_t)s * Dh + d];
        if (!lst) lst = rl1_owner_prep(c, hos, 0, 1, hr1.data(), hprd);   // at the bounds (exact after the fold)
    }
    if (!lst && inject_fail(c, kFailOwner)) lst = CRDT_E_NOMEM;
    test_stall(c, kStallRecords);
    set_phase(c, "route_l1: agreement before the record exchange");
    if ((st = comm_agree(c, lst))) return drain_side(c, st);
    // from here every HIP failure stays in lst: the exchanges are posted all the same and finish_apply's
    // reduction carries the failure to every rank
    if (head) {                                         // the fold, behind every piece's partition
        lst = rl1_head_launch(c, pf, Dh, ro_tail, c->sstream);
        HIPLST(hipEventRecord(c->rl_evh, c->sstream));
    }
    // the peers' parts, piece by piece (payload and key column in one grouped exchange each), and the owner's
    // level 2 + resolve of each piece as soon as it is complete: pieces 0 .. P-2 on the owner stream, in
    // order, while the next pieces cross the exchange; the last on the ctx stream after them (with the head
    // fold: every piece on the owner stream, the folded head last on the ctx stream).  P passes over the table
    // are one fold: the order-free result is a maximum, and every changeset of piece q precedes those of q + 1,
    // so a row an earlier piece stored keeps a tie against a later piece exactly as the table's own rows do
    // (pack_local); the folded head's keys are in no piece.
    set_phase(c, "route_l1: record exchange");
    for (uint32_t q = 0; q < P; ++q) {
        HIPLST(hipStreamWaitEvent(c->stream, c->rl_evs[q], 0));
        std::vector<uint64_t> sc0(psc.begin() + (size_t)q * G, psc.begin() + (size_t)(q + 1) * G);
        std::vector<uint64_t> rc0(prc.begin() + (size_t)q * G, prc.begin() + (size_t)(q + 1) * G);
        std::vector<uint64_t> sd0(psd.begin() + (size_t)q * G, psd.begin() + (size_t)(q + 1) * G);
        std::vector<uint64_t> rd0(prd.begin() + (size_t)q * G, prd.begin() + (size_t)(q + 1) * G);
        sc0[me] = rc0[me] = 0;
        const void* s2[2] = {c->rl_rec.p, c->rl_k16.p};
        void* r2[2] = {c->rl_rec.p, c->rl_k16.p};
        const uint32_t e2[2] = {12, kcol};
        if ((st = comm_all_to_all(c, 2, s2, r2, e2, sc0.data(), sd0.data(), rc0.data(), rd0.data(), n, ro)))
            return drain_side(c, st);
        if ((q + 1 < P || head) && !lst) {              // (rows stored by an earlier piece lie anywhere: hw = cap)
            HIPLST(hipEventRecord(c->rl_evx[q], c->stream));
            HIPLST(hipStreamWaitEvent(c->ostream, c->rl_evx[q], 0));
            if (!lst) lst = rl1_owner_launch(c, c->rl_os[q], pf, c->ostream, q == 0 ? c->hw_read : c->cap, false);
        }
    }
    if (head) {
        // the folded head: its counts (Dh words per peer; a rank whose fold did not launch sends none), then its
        // records into the receive positions planned at the bounds (each source's digits back to back)
        unsigned long long* hc = c->rl_hcnt.p;          // [G][Dh] sent, [G][Dh] received, [Dh] own
        const size_t GD = (size_t)G * Dh, hw_words = 2 * GD + Dh;
        set_phase(c, "route_l1: head exchange");
        HIPLST(hipStreamWaitEvent(c->stream, c->rl_evh, 0));
        if (lst) HIPLST(hipMemsetAsync(hc, 0, hw_words * sizeof(unsigned long long), c->stream));
        std::vector<uint64_t> sc1(G), sd1(G), rc1(G), rd1(G);
        for (uint32_t d = 0; d < G; ++d) {
            sc1[d] = rc1[d] = d == me ? 0 : Dh;
            sd1[d] = (uint64_t)d * Dh;
            rd1[d] = GD + (uint64_t)d * Dh;
        }
        {
            const void* s1[1] = {hc};
            void* r1[1] = {hc};
            const uint32_t e8 = 8;
            if ((st = comm_all_to_all(c, 1, s1, r1, &e8, sc1.data(), sd1.data(), rc1.data(), rd1.data(), hw_words,
                                      hw_words)))
                return drain_side(c, st);
        }
        HIPCHK(hipMemcpyAsync(c->h_hcnt.p, hc, hw_words * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
        SYNCHK(c, c->stream);
        const unsigned long long* hh = c->h_hcnt.p;
        std::vector<uint64_t> sch(G, 0), sdh(G), rch(G, 0);
        uint64_t so = 0, hout = 0;
        for (uint32_t o = 0; o < G; ++o) {
            for (uint32_t d = 0; d < Dh; ++d) {
                const uint64_t sent = o == me ? 0 : hh[(size_t)o * Dh + d];
                const uint64_t got = o == me ? hh[2 * GD + d] : hh[GD + (size_t)o * Dh + d];
                sch[o] += sent;
                if (o != me) rch[o] += got;
                hout += o == me ? got : sent;
                hr1[(size_t)o * D + d] = got;
                if (got > hrb[(size_t)o * Dh + d] && !lst) lst = CRDT_E_INVALID;   // (cannot happen: fold <= bound)
            }
            sdh[o] = so;
            so += sch[o];
        }
        c->last_rl1_head_in = hin;
        c->last_rl1_head_out = hout;
        const void* s2[2] = {c->rl_hrec.p, c->rl_hk16.p};
        void* r2[2] = {c->rl_rec.p, c->rl_k16.p};
        const uint32_t e2[2] = {12, kcol};
        if ((st = comm_all_to_all(c, 2, s2, r2, e2, sch.data(), sdh.data(), rch.data(), hprd.data(), so, ro)))
            return drain_side(c, st);
        if (!lst) lst = rl1_owner_prep(c, hos, 0, 1, hr1.data(), hprd);    // exact (within the bounds' buffers)
    }
    ev_record(c, kEvApply);                             // route_ms: partition + the exchanges
    if (!lst && inject_fail(c, kFailApply)) lst = CRDT_E_NOMEM;    // (after the last exchange)
    // the folded head's level 2 + resolve as soon as its exchange is done, beside the pieces' owner work still
    // on the owner stream (round 6: its keys — digits < Dh — are in no piece, its buckets, rows and scratch are
    // its own); the last piece (no head) after the others, in piece order (a later piece must see the rows an
    // earlier one stored)
    if (head && !lst) lst = rl1_owner_launch(c, hos, pf, c->stream, c->cap, ph);
    if (P > 1 || head) {
        HIPLST(hipEventRecord(c->rl_evo, c->ostream));
        HIPLST(hipStreamWaitEvent(c->stream, c->rl_evo, 0));
    }
    if (!head && !lst)
        lst = rl1_owner_launch(c, c->rl_os[P - 1], pf, c->stream, P == 1 ? c->hw_read : c->cap, ph);
    if (ph && !lst) {
        c->sorted_phases = true;
        c->p1_records = p0;                             // the records piece 0's partition (window 1) read and wrote
        ev_record(c, ev_window(0, true));
        c->windows.push_back(1u);
    }
    c->hw_read = c->cap;
    // (a launch that failed after the agreement: finish_apply's reduction carries it to every rank)
    st = finish_apply(c, nullptr, nullptr, 0, true, out, lst);
    return st < 0 ? drain_side(c, st) : st;
}

// The settings of this process that decide the shape of a sharded merge's collectives after the clock
// phase (record exchange or map-side combine, wire columns, flags coming back): all-gathered with the part
// maxima, so ranks that disagree (an environment variable set on one of them, win flags passed by some)
// all fail the call with CRDT_E_INVALID instead of posting mismatched exchanges.
long long shard_cfg_word(const crdt_ctx* c, bool flags) {
    return (long long)((c->presharded ? 1u : 0u) | (flags ? 2u : 0u) | (c->counts ? 4u : 0u) |
                       (c->packed_resolve ? 8u : 0u) | ((uint32_t)c->merge_path << 4) | ((uint32_t)c->combine << 6) |
                       (c->frame_on ? 256u : 0u) | (c->route_l1 ? 512u : 0u) | (c->rl1_pieces << 10) |
                       ((uint32_t)(c->tune_mode + 1) << 13) | ((uint32_t)(c->route_l1 >= 2 ? c->route_l1 - 1 : 0) << 16) |
                       ((c->form_off & (kFormNoCompact | kFormNoVecLoads)) ? 1u << 19 : 0u));   // (route_l1's wire)
}

// ---- RouteTune: which way a sharded order-free fan-in moves its records, measured ----------------------
// Every way leaves the same rows (the fold is a maximum; tests/test_gpu_parity.py); they differ in bytes
// over the links (route_l1 14 B per home record, the combine ~3.4x fewer at ~1.7x the local work, DESIGN.md
// §7) and in how much of the exchange hides behind the partition and the owner work (route_l1 in 2 or 4
// pipelined pieces), so the best one depends on the links' rate, which only the run can tell.  A ctx whose
// calls could take any (the auto settings: CRDT_COMBINE=1, CRDT_ROUTE_L1=1) runs kTrials calls each way
// (0: route_l1 in 2 pieces, 1: the combine, 2: route_l1 in 4 pieces, 3: in one, 4: in 2 pieces with the
// head fold), times each call on the
// host (entry to the final synchronisation) and MAX-all-reduces the last one of each way (the step is as
// slow as its slowest rank); from then on every call with the same (R, G, capacity) takes the fastest.  The schedule
// depends only on the call sequence and the reduced times, so every rank takes the same way in every call
// (the way is in the collective-shape word, checked after the gather).
constexpr uint32_t kTrials = 2;         // the first call of a way may allocate its buffers: the second is timed
constexpr int kTuneWays = 5;

int route_tune_mode(crdt_ctx* c, const crdt_batch* batch) {
    const uint32_t R = batch->n_changesets, G = c->n_ranks;
    const bool tunable = c->route_tune && c->combine == 1 && c->route_l1 == 1 && !c->presharded && R >= 64 &&
                         c->packed_resolve && c->merge_path != 1 && c->canonical >= 0 && !c->counts &&
                         route_l1_ok(c) && (uint64_t)G * c->cap <= kSortedMaxCap;
    if (!tunable) return -1;
    const uint64_t shape = ((uint64_t)R << 40) ^ ((uint64_t)G << 32) ^ c->cap;
    if (c->rt.shape != shape) c->rt = crdt_ctx::RouteTune{shape, 0, -1, {-1, -1, -1, -1, -1}};
    if (c->rt.best >= 0) return c->rt.best;
    return (int)std::min<uint32_t>(c->rt.trial / kTrials, kTuneWays - 1);
}

// after a call that took the tuner's way with both ways open: this rank's time, max over ranks
int route_tune_record(crdt_ctx* c, double ms) {
    const uint32_t t = c->rt.trial++;
    if ((t + 1) % kTrials) return CRDT_OK;              // not the timed call of its way
    HIPALLOC(c->d_tune.ensure(1));
    HIPALLOC(c->h_tune.ensure(2));
    c->h_tune.p[0] = (long long)(ms * 1e3);
    HIPCHK(hipMemcpyAsync(c->d_tune.p, c->h_tune.p, 8, hipMemcpyHostToDevice, c->stream));
    int st = comm_all_reduce(c, c->d_tune.p, 1, CRDT_REDUCE_MAX);
    if (st) return st;
    HIPCHK(hipMemcpyAsync(c->h_tune.p + 1, c->d_tune.p, 8, hipMemcpyDeviceToHost, c->stream));
    SYNCHK(c, c->stream);
    const int way = (int)(t / kTrials);
    c->rt.us[way] = c->h_tune.p[1];
    if (way == kTuneWays - 1) {
        int b = 0;
        for (int w = 1; w < kTuneWays; ++w) b = c->rt.us[w] < c->rt.us[b] ? w : b;
        c->rt.best = b;
    }
    return CRDT_OK;
}

// =========================================================================================
// crdt_merge on a sharded ctx (include/crdt_merge.h, "key-sharded multi-GPU").
// =========================================================================================
int merge_sharded_call(crdt_ctx* c, const crdt_batch* batch, int64_t wall, uint8_t* win_flags, crdt_result* out) {
    const uint32_t R = batch->n_changesets, G = c->n_ranks, me = c->rank;
    const uint64_t n = batch->offsets[R];
    int st;
    c->finish_posted = false;
    // The O(R) buffers of the clock phase's collectives first: with them a rank whose local work fails below
    // still posts the gather and the two reductions, its gather row carrying the status (k_fail_row), and
    // every rank fails the call at the clock phase's synchronisation (this file's header).
    const uint64_t grow = 2ull * R + kGatherExtra;                // all-gather row: maxima, counts, frame, words
    HIPALLOC(c->d_gsend.ensure(grow));
    HIPALLOC(c->d_grecv.ensure(grow * G));
    HIPALLOC(c->d_M.ensure(R));
    HIPALLOC(c->d_pbase.ensure(R));
    HIPALLOC(c->d_ibase.ensure(R));
    HIPALLOC(c->d_Cprev.ensure(R + 1));
    HIPALLOC(c->d_Rj.ensure(R + 1));
    HIPALLOC(c->d_Cj.ensure(R + 1));
    const long long cfg = shard_cfg_word(c, win_flags != nullptr);
    // local work: every column of a host batch staged now (the exchange reads them all), the scan
    Cols cols;
    crdt_batch dev = *batch;
    uint8_t* dflags = nullptr;
    auto local = [&]() -> int {
        int e;
        if ((e = stage_apply_cols(c, batch, &cols))) return e;
        if ((e = stage(c, c->s_millis, batch->millis, n, batch->mem, &cols.millis))) return e;
        dev.key_id = cols.key; dev.lt = cols.lt; dev.rank = cols.rank; dev.val = cols.val; dev.millis = cols.millis;
        dev.mem = CRDT_MEM_DEVICE;
        if (win_flags) {
            if (batch->mem == CRDT_MEM_HOST) {
                HIPALLOC(c->s_flags.ensure(n ? n : 1));
                dflags = c->s_flags.p;
            } else {
                dflags = win_flags;
            }
        }
        if (c->timing) HIPCHK(ensure_events(c, events_for((size_t)R * G)));
        ev_record(c, kEvStart);
        // 1: per-part scan (the record frame rides along whenever the sorted path's packed form may run on
        // this rank; it also serves the receivers' ordered form — win flags or exact counts on the sorted path
        // — but only the order-free form takes packed wire records: pack_ok)
        const bool frame = c->packed_resolve && c->merge_path != 1 && c->canonical >= 0;
        const bool pack_ok = !win_flags && !c->counts;
        // the routed level-1 partition is likely (route_l1 below; the frame decides for sure after the
        // gather): its level-1 histogram rides on the scan (keys read with lt and rank)
        const bool rl1_likely = frame && pack_ok && c->packed_resolve && c->merge_path != 1 && !c->presharded &&
                                route_l1_ok(c) && (c->merge_path == 2 || R >= 64) &&
                                (c->tune_mode >= 0 ? c->tune_mode != 1
                                                   : c->combine != 2 && !(c->combine == 1 && G == 2 && R >= 64));
        const KeyMap rkm{route_bits(G), route_l1_dsh(c->cap)};
        if ((e = phase_scan(c, &dev, wall, c->d_gsend.p, false, frame, false, false, rl1_likely ? &rkm : nullptr)))
            return e;
        return inject_fail(c, kFailLocal) ? CRDT_E_NOMEM : CRDT_OK;
    };
    set_phase(c, "scan");
    int lst = local();
    if (!lst) {
        k_part_counts<<<grid_for(R, 256), 256, 0, c->stream>>>(c->d_offs, R, c->d_misc, c->d_gsend.p, cfg, 0);
        HIPLST(hipGetLastError());
    }
    if (lst) {                                          // this rank posts the clock phase's collectives only
        HIPLST(hipMemsetAsync(c->d_misc, 0, sizeof(Misc), c->stream));
        k_fail_row<<<std::max<uint32_t>(1, std::min<uint32_t>(grid_for(R, 256), 1024)), 256, 0, c->stream>>>(
            c->d_gsend.p, R, cfg, -(long long)lst);
    }
    ev_record(c, kEvScan);
    // 2-3: all-gather of the part maxima and counts; clock recurrence and the exception scan from each part's
    // predecessors; the first event and its details (and, MAX-reduced in d_event[4], a local failure after
    // the gather)
    test_stall(c, kStallGather);
    set_phase(c, "clock phase: gather of the part maxima");
    if ((st = comm_all_gather(c, c->d_gsend.p, c->d_grecv.p, grow))) return st;
    k_shard_combine<<<grid_for(R, 256), 256, 0, c->stream>>>(c->d_grecv.p, G, me, R, c->d_M.p, c->d_pbase.p,
                                                             c->d_ibase.p, c->d_misc);
    if (!lst) lst = phase_clock(c, &dev, wall, c->d_M.p, c->d_event.p, c->d_pbase.p, c->d_ibase.p);
    if (lst) k_event_init<<<1, 64, 0, c->stream>>>(c->d_event.p);
    if ((st = comm_all_reduce(c, c->d_event.p, 1, CRDT_REDUCE_MIN))) return st;
    if (!lst) lst = phase_resolve(c, c->d_event.p);
    k_fill_i64<<<1, 64, 0, c->stream>>>(c->d_event.p + 4, 1, lst < 0 ? -(long long)lst : 0);
    if ((st = comm_all_reduce(c, c->d_event.p + 1, 4, CRDT_REDUCE_MAX))) return st;
    HIPCHK(hipGetLastError());
    ev_record(c, kEvClock);
    // the gathered frame and the ranks' collective-shape words and failures (k_shard_combine): every rank
    // reads the same words, so every rank takes the same branch below — or fails here, before any exchange.
    // (A HIP failure of this read-back is rank-local: without the agreed words the rank cannot post what its
    // peers post next, and they fail at their deadline.)
    HIPCHK(hipMemcpyAsync(c->h_misc, c->d_misc, sizeof(Misc), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(c->h_agree.p + 1, c->d_event.p + 4, 8, hipMemcpyDeviceToHost, c->stream));
    SYNCHK(c, c->stream);
    const unsigned long long fail = std::max<unsigned long long>(c->h_misc->shard_status,
                                                                 (unsigned long long)c->h_agree.p[1]);
    if (fail) return -(int)fail;
    if (c->h_misc->route_own & 4) return CRDT_E_INVALID;
    const bool frame = c->frame_on;
    const bool pack_ok = !win_flags && !c->counts;

    // 4: route every record to its owner (key % G, slot key / G) in one grouped exchange
    Cols rc = cols;
    uint64_t nr = n;
    uint8_t* rflags = dflags;
    PackFrame pf{};
    bool wire_pk = false;
    c->last_wire_pk = false;
    c->last_own_in_place = false;
    std::vector<uint64_t> sc(G), sd(G), rcn(G), rd(G);
    // map-side combine (order-free form, one window, the global frame fits the packed key): every rank
    // folds its home records into one packed maximum per distinct key (apply_sorted's emit mode, the
    // key range G x slots, an absent table) and routes those instead of the records — the order-free
    // fold is a maximum and the packed key carries the changeset, so folding before routing changes
    // nothing but the bytes (DESIGN.md §7)
    bool comb = false;
    c->last_combined = false;
    // (auto: many-changeset fan-ins only — a key repeats at most once per changeset, so a few changesets
    // fold to about as many keys as records and the fold would be pure overhead; CRDT_COMBINE=2 forces it)
    // auto (CRDT_COMBINE=1): a many-changeset fan-in on TWO ranks, whose one link carries every routed byte
    // (the fold sends ~3.4x fewer); from four ranks on the routed level-1 partition (route_l1) is cheaper in
    // local work and the exchange spreads over G - 1 links (DESIGN.md §7)
    const bool rl1_possible = frame && pack_ok && c->packed_resolve && c->merge_path != 1 && !c->presharded &&
                              route_l1_ok(c);
    if (frame) pf = frame_of(c);                                       // the all-gathered frame
    const bool comb_ok = !c->presharded && frame && pack_ok && c->packed_resolve && c->merge_path != 1 &&
                         (uint64_t)G * c->cap <= kSortedMaxCap && pf.ok && R <= pf.jwin;
    const bool rl1_ok = rl1_possible && pf.ok && pf.key4 && R <= pf.jwin && (c->merge_path == 2 || R >= 64) &&
                        c->canonical >= 0;
    // (every input: the same on every rank, checked by shard_cfg_word above)
    c->tune_trial = c->tune_mode >= 0 && comb_ok && rl1_ok;
    c->rl1_call_pieces = !c->tune_trial ? c->rl1_pieces : c->tune_mode == 2 ? kRl1MaxPieces : c->tune_mode == 3 ? 1u : 2u;
    c->rl1_call_head = c->tune_trial ? c->tune_mode == 4 : c->route_l1 >= 2;
    c->rl1_call_all = !c->tune_trial && c->route_l1 == 3;
    if (c->tune_trial)
        comb = c->tune_mode == 1;
    else if (c->combine && (c->combine == 2 || (R >= 64 && (G == 2 || !rl1_possible))))
        comb = comb_ok;
    c->last_route_l1 = false;
    if (!comb && rl1_ok) {
        c->last_route_l1 = true;
        c->last_wire_pk = true;
        c->last_own_in_place = true;
        st = route_l1(c, cols, batch->offsets, wall, pf, out);
        if (st == CRDT_E_COMM) return st;
        if (c->timing) ev_record(c, kEvEnd);
        SYNCHK(c, c->stream);
        collect_timing(c);
        return st;
    }
    if (comb) {
        EmitOut eo{};
        eo.G = G;
        uint32_t n_items = 0;
        unsigned long long* d_own = nullptr;
        // the home fold and the counts' buffers (a failure: agreed before the counts' exchange)
        auto fold = [&]() -> int {
            HIPALLOC(c->e_cnt.ensure(2 * (size_t)G + 2));
            HIPALLOC(c->d_rcnt.ensure(2 * (size_t)G));
            HIPALLOC(c->h_rcnt.ensure(2 * (size_t)G + 1));
            d_own = c->e_cnt.p + 2;                                 // [G] emitted entries per owner
            Segs hs;
            hs.from_offsets(batch->offsets, R);
            // the stop point first (the fold applies changesets < stop only); the owners' apply reuses it
            k_resolve<<<1, 64, 0, c->stream>>>(c->d_event.p, R, wall, c->canonical, c->d_Rj.p, c->d_Cj.p, c->d_misc);
            c->resolved = true;
            const uint64_t cap0 = c->cap, hw0 = c->hw_read;
            c->cap = (uint64_t)G * cap0;                            // global key ids, every row absent
            c->hw_read = 0;
            int e = apply_sorted(c, cols, hs, wall, c->d_event.p, nullptr, nullptr, &eo);
            c->cap = cap0;
            c->hw_read = hw0;
            if (e) return e;
            n_items = eo.n_items;                                   // 0: nothing applied here
            HIPALLOC(c->e_off.ensure(((size_t)n_items + 1) * G));
            if (n_items) {
                const uint32_t nch = (n_items + kCombChunk - 1) / kCombChunk;
                HIPALLOC(c->e_csum.ensure((size_t)nch * G));
                k_comb_chunk_sum<<<nch, 256, 0, c->stream>>>(eo.ocount, n_items, G, c->e_csum.p);
                k_comb_chunk_scan<<<std::max<uint32_t>(1, (G + 255) / 256), 256, 0, c->stream>>>(c->e_csum.p, nch, G,
                                                                                                d_own);
                k_comb_offsets<<<nch, 256, 0, c->stream>>>(eo.ocount, n_items, G, c->e_csum.p, c->e_off.p);
            } else {
                HIPCHK(hipMemsetAsync(d_own, 0, G * sizeof(unsigned long long), c->stream));
            }
            return inject_fail(c, kFailCombine) ? CRDT_E_NOMEM : CRDT_OK;
        };
        set_phase(c, "combine: agreement after the fold");
        if ((st = comm_agree(c, fold()))) return st;
        // per-owner counts -> host; the counts' exchange (one word per peer; a HIP failure of the copies: zero
        // counts sent, the failure agreed before the record exchange; lst is 0 here: the clock phase agreed it)
        HIPLST(hipMemcpyAsync(c->d_rcnt.p, d_own, G * sizeof(unsigned long long), hipMemcpyDeviceToDevice,
                              c->stream));
        HIPLST(hipMemcpyAsync(c->d_rcnt.p + G + me, d_own + me, sizeof(unsigned long long), hipMemcpyDeviceToDevice,
                              c->stream));
        if (lst) HIPLST(hipMemsetAsync(c->d_rcnt.p, 0, 2 * (size_t)G * sizeof(unsigned long long), c->stream));
        for (uint32_t d = 0; d < G; ++d) {
            sc[d] = rcn[d] = d == me ? 0 : 1;
            sd[d] = d;
            rd[d] = G + d;
        }
        test_stall(c, kStallCounts);
        set_phase(c, "combine: count exchange");
        {
            const void* s1[1] = {c->d_rcnt.p};
            void* r1[1] = {c->d_rcnt.p};
            const uint32_t e8 = 8;
            if ((st = comm_all_to_all(c, 1, s1, r1, &e8, sc.data(), sd.data(), rcn.data(), rd.data(), 2 * (size_t)G,
                                      2 * (size_t)G)))
                return st;
        }
        HIPCHK(hipMemcpyAsync(c->h_rcnt.p, c->d_rcnt.p, 2 * G * sizeof(unsigned long long), hipMemcpyDeviceToHost,
                              c->stream));
        SYNCHK(c, c->stream);
        const uint64_t* h_send = c->h_rcnt.p;                        // records I send to d
        const uint64_t* h_recv = c->h_rcnt.p + G;                    // records s sends me
        uint64_t so = 0, ro = 0;
        for (uint32_t d = 0; d < G; ++d) {
            sc[d] = h_send[d];
            rcn[d] = h_recv[d];
            sd[d] = so;
            rd[d] = ro;
            so += sc[d];
            ro += rcn[d];
        }
        nr = ro;
        auto bufs = [&]() -> int {                          // (agreed before the record exchange)
            HIPALLOC(c->r_skey.ensure(so ? so : 1)); HIPALLOC(c->r_slt.ensure(so ? so : 1));
            HIPALLOC(c->r_sval.ensure(so ? so : 1));
            HIPALLOC(c->r_key.ensure(nr ? nr : 1)); HIPALLOC(c->r_lt.ensure(nr ? nr : 1));
            HIPALLOC(c->r_val.ensure(nr ? nr : 1));
            HIPALLOC(c->h_ebase.ensure(G));
            HIPALLOC(c->e_cur.ensure(G));
            return inject_fail(c, kFailRecv) ? CRDT_E_NOMEM : CRDT_OK;
        };
        if (!lst) lst = bufs();
        test_stall(c, kStallRecords);
        set_phase(c, "combine: agreement before the record exchange");
        if ((st = comm_agree(c, lst))) return st;
        lst = CRDT_OK;
        c->recv_cap = std::min({(uint64_t)c->r_key.n, (uint64_t)c->r_lt.n, (uint64_t)c->r_rank.n, (uint64_t)c->r_val.n});
        // the owners' bases through pinned staging (read by the copy after this returns: no wait here;
        // the staging is rewritten only by the next call, after this call's final synchronisation)
        for (uint32_t d = 0; d < G; ++d) c->h_ebase.p[d] = d == me ? rd[me] : sd[d];
        HIPLST(hipMemcpyAsync(c->e_cur.p, c->h_ebase.p, G * sizeof(unsigned long long), hipMemcpyHostToDevice,
                              c->stream));
        if (n_items && !lst)
            k_comb_scatter<<<n_items, 256, 0, c->stream>>>(eo.key, eo.pk, eo.val, eo.icount, eo.ibase, c->e_off.p, c->e_cur.p, G,
                                                           me, c->r_skey.p, c->r_slt.p, c->r_sval.p, c->r_key.p,
                                                           c->r_lt.p, c->r_val.p);
        HIPLST(hipGetLastError());
        set_phase(c, "combine: record exchange");
        std::vector<uint64_t> sc0(sc), rc0(rcn);
        sc0[me] = rc0[me] = 0;
        const void* s3[3] = {c->r_skey.p, c->r_slt.p, c->r_sval.p};
        void* r3[3] = {c->r_key.p, c->r_lt.p, c->r_val.p};
        const uint32_t e3[3] = {4, 8, 4};
        if ((st = comm_all_to_all(c, 3, s3, r3, e3, sc0.data(), sd.data(), rc0.data(), rd.data(), so, nr)))
            return st;
        // the owners' batch: one segment per source, all in the window's first changeset (the packed keys
        // carry each record's own)
        Segs& sg = c->segs;
        sg.beg.clear(); sg.end.clear(); sg.j.clear();
        for (uint32_t s = 0; s < G; ++s)
            if (rcn[s]) { sg.beg.push_back(rd[s]); sg.end.push_back(rd[s] + rcn[s]); sg.j.push_back(0); }
        rc.key = c->r_key.p; rc.lt = c->r_lt.p; rc.rank = nullptr; rc.val = c->r_val.p;
        rc.packed_in = true;
        wire_pk = true;
        c->last_wire_pk = true;
        c->last_combined = true;
    } else if (c->presharded) {
        c->segs.from_offsets(batch->offsets, R);
    } else {
        // The route plan runs on the device: counts, their exchange, and the cursors (k_route_plan)
        // feed the scatter directly.  Only the SIZES of the record exchange must reach the host (RCCL's
        // send / receive take host counts): they are copied back behind the plan and the host waits for
        // that copy alone (an event) while the scatter runs, so the device never idles on it.  The own
        // chunk is scattered straight into the receive columns (no device-to-device copy) whenever they
        // already hold every record this rank receives (win flags: the copy, as their perm is in send order).
        const size_t cells = (size_t)G * R;
        auto prep = [&]() -> int {                          // (agreed before the counts' exchange)
            HIPALLOC(c->d_rcnt.ensure(cells));
            HIPALLOC(c->d_rrecv.ensure(cells));
            HIPALLOC(c->d_rcur.ensure(cells));
            HIPALLOC(c->h_rcnt.ensure(2 * cells));
            HIPALLOC(c->r_skey.ensure(n)); HIPALLOC(c->r_slt.ensure(n));
            HIPALLOC(c->r_srank.ensure(n)); HIPALLOC(c->r_sval.ensure(n));
            if (dflags) {
                HIPALLOC(c->r_perm.ensure(n));
                HIPALLOC(c->r_sflags.ensure(n ? n : 1));
            }
            if (!c->route_ev) HIPCHK(hipEventCreateWithFlags(&c->route_ev, hipEventDisableTiming));
            return CRDT_OK;
        };
        set_phase(c, "record routing: agreement before the counts");
        if ((st = comm_agree(c, prep()))) return st;
        // (a HIP failure from here to the count exchange: zero counts sent, the failure agreed before the
        // record exchange)
        HIPLST(hipMemsetAsync(c->d_rcnt.p, 0, cells * sizeof(uint64_t), c->stream));
        if (c->plan_tiles && !lst) {
            const uint32_t gx = std::max<uint32_t>(1, std::min<uint32_t>(c->plan_mt, std::max<uint32_t>(1, 65536u / R)));
            for (uint32_t jb = 0; jb < R; jb += 65535)
                if (c->form_off & kFormNoVecRoute)
                    k_route_count<<<dim3(gx, std::min<uint32_t>(65535, R - jb)), kScanThreads, 0, c->stream>>>(
                        cols.key, c->d_offs, c->d_tstart, jb, R, G, c->d_rcnt.p);
                else
                    k_route_count_v<<<dim3(gx, std::min<uint32_t>(65535, R - jb)), kScanThreads, 0, c->stream>>>(
                        cols.key, c->d_offs, c->d_tstart, jb, R, G, route_bits(G), c->d_rcnt.p);
        }
        // counts: row d of every rank's [G][R] matrix goes to rank d
        HIPLST(hipGetLastError());
        HIPLST(hipMemcpyAsync(c->d_rrecv.p + (size_t)me * R, c->d_rcnt.p + (size_t)me * R, R * sizeof(uint64_t),
                              hipMemcpyDeviceToDevice, c->stream));
        if (lst) HIPLST(hipMemsetAsync(c->d_rcnt.p, 0, cells * sizeof(uint64_t), c->stream));
        for (uint32_t d = 0; d < G; ++d) {
            sc[d] = rcn[d] = d == me ? 0 : R;
            sd[d] = rd[d] = (uint64_t)d * R;
        }
        test_stall(c, kStallCounts);
        set_phase(c, "record routing: count exchange");
        {
            const void* s1[1] = {c->d_rcnt.p};
            void* r1[1] = {c->d_rrecv.p};
            const uint32_t e8 = 8;
            if ((st = comm_all_to_all(c, 1, s1, r1, &e8, sc.data(), sd.data(), rcn.data(), rd.data(), cells, cells)))
                return st;
        }
        const bool own_req = !dflags && !(c->form_off & kFormNoOwnInPlace);
        k_route_plan<<<1, 1024, 0, c->stream>>>(c->d_rcnt.p, c->d_rrecv.p, G, R, me, own_req ? 1u : 0u,
                                                c->recv_cap, n, c->d_rcur.p, c->d_misc);
        uint64_t* h_send = c->h_rcnt.p;                      // [G][R] records I send to d, per changeset
        uint64_t* h_recv = c->h_rcnt.p + cells;              // [G][R] records s sends me
        HIPCHK(hipMemcpyAsync(h_send, c->d_rcnt.p, cells * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(h_recv, c->d_rrecv.p, cells * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(c->h_misc, c->d_misc, sizeof(Misc), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipEventRecord(c->route_ev, c->stream));
        // the receive columns as they stand (recv_cap records; k_route_plan checked the fit)
        const RouteCols send{c->r_skey.p, c->r_slt.p, c->r_srank.p, c->r_sval.p};
        const RouteCols own = c->recv_cap ? RouteCols{c->r_key.p, c->r_lt.p, c->r_rank.p, c->r_val.p}
                                          : RouteCols{nullptr, nullptr, nullptr, nullptr};
        const uint32_t fr_on = c->frame_on && pack_ok ? 1u : 0u;      // the scatter packs under the frame
        if (c->plan_tiles && !lst) {
            const uint32_t gx = std::max<uint32_t>(1, std::min<uint32_t>(c->plan_mt, std::max<uint32_t>(1, 65536u / R)));
            for (uint32_t jb = 0; jb < R; jb += 65535) {
                const dim3 grid(gx, std::min<uint32_t>(65535, R - jb));
                if (c->form_off & kFormNoVecRoute)
                    k_route_scatter<<<grid, kScanThreads, 0, c->stream>>>(
                        cols.key, cols.lt, cols.rank, cols.val, c->d_offs, c->d_tstart, jb, R, G, c->d_rcur.p,
                        send, own, me, dflags ? c->r_perm.p : nullptr, c->d_misc, fr_on);
                else                    // vector loads + wave-aggregated slots (tools/ubench_route.hip)
                    k_route_scatter_v<<<grid, kScanThreads, 0, c->stream>>>(
                        cols.key, cols.lt, cols.rank, cols.val, c->d_offs, c->d_tstart, jb, R, G, route_bits(G),
                        c->d_rcur.p, send, own, me, dflags ? c->r_perm.p : nullptr, c->d_misc, fr_on);
            }
            HIPLST(hipGetLastError());
        }
        if ((st = comm_wait(c, nullptr, c->route_ev))) return st;   // the counts only: the scatter runs on
        // wire format: 16-B packed records when the global frame fits the sorted path's key (the
        // same decision on every rank and in the scatter: the frame was all-gathered)
        pf = frame_of(c);
        wire_pk = c->frame_on && pf.ok && pack_ok;
        c->last_wire_pk = wire_pk;
        const bool own_in = (c->h_misc->route_own & 1) != 0;
        // plan (host, O(G R)): send columns owner-major then changeset order; receive columns
        // source-major; the apply reads changeset j as one segment per source
        uint64_t so = 0, ro = 0;
        for (uint32_t d = 0; d < G; ++d) {
            sd[d] = so;
            rd[d] = ro;
            uint64_t a = 0, b = 0;
            for (uint32_t j = 0; j < R; ++j) {
                a += h_send[(size_t)d * R + j];
                b += h_recv[(size_t)d * R + j];
            }
            sc[d] = a;
            rcn[d] = b;
            so += a;
            ro += b;
        }
        // every record has an owner (else the scatter, told by k_route_plan, wrote nothing); the receive
        // columns and the flags' buffers — a failure of any of these on any rank fails every rank here
        if (!lst && (so != n || (c->h_misc->route_own & 2))) lst = CRDT_E_INVALID;
        nr = ro;
        Segs& sg = c->segs;
        sg.beg.clear(); sg.end.clear(); sg.j.clear();
        std::vector<uint64_t> run(rd);
        for (uint32_t j = 0; j < R; ++j)
            for (uint32_t s = 0; s < G; ++s) {
                const uint64_t k = h_recv[(size_t)s * R + j];
                if (!k) continue;
                sg.beg.push_back(run[s]);
                sg.end.push_back(run[s] + k);
                sg.j.push_back(j);
                run[s] += k;
            }
        auto grow_recv = [&]() -> int {
            if (inject_fail(c, kFailRecv)) return CRDT_E_NOMEM;
            if (dflags) HIPALLOC(c->r_flags.ensure(nr ? nr : 1));
            if (own_in) return CRDT_OK;
            // the receive columns grow (a reallocation waits for the device) and the own chunk, left
            // in the send columns by the scatter, is copied over; the next calls scatter it in place
            HIPALLOC(c->r_key.ensure(nr)); HIPALLOC(c->r_lt.ensure(nr));
            HIPALLOC(c->r_rank.ensure(nr)); HIPALLOC(c->r_val.ensure(nr));
            c->recv_cap = std::min({(uint64_t)c->r_key.n, (uint64_t)c->r_lt.n, (uint64_t)c->r_rank.n,
                                    (uint64_t)c->r_val.n});
            if (own_req && c->recv_cap < nr + nr / 4) {      // headroom for the next calls' spread
                const uint64_t want = nr + nr / 4;
                HIPALLOC(c->r_key.ensure(want)); HIPALLOC(c->r_lt.ensure(want));
                HIPALLOC(c->r_rank.ensure(want)); HIPALLOC(c->r_val.ensure(want));
                c->recv_cap = want;
            }
            return CRDT_OK;
        };
        if (!lst) lst = grow_recv();
        test_stall(c, kStallRecords);
        set_phase(c, "record routing: agreement before the record exchange");
        if ((st = comm_agree(c, lst))) return st;
        // (from here a HIP failure stays in lst: the exchange is posted, finish_apply's reduction carries it)
        if (!own_in) {
            const uint64_t owned = sc[me];
            if (owned) {
                HIPLST(hipMemcpyAsync(c->r_key.p + rd[me], c->r_skey.p + sd[me], owned * 4, hipMemcpyDeviceToDevice,
                                      c->stream));
                HIPLST(hipMemcpyAsync(c->r_lt.p + rd[me], c->r_slt.p + sd[me], owned * 8, hipMemcpyDeviceToDevice,
                                      c->stream));
                if (!wire_pk)
                    HIPLST(hipMemcpyAsync(c->r_rank.p + rd[me], c->r_srank.p + sd[me], owned * 4,
                                          hipMemcpyDeviceToDevice, c->stream));
                HIPLST(hipMemcpyAsync(c->r_val.p + rd[me], c->r_sval.p + sd[me], owned * 4, hipMemcpyDeviceToDevice,
                                      c->stream));
            }
        }
        set_phase(c, "record routing: record exchange");
        c->last_own_in_place = own_in;
        std::vector<uint64_t> sc0(sc), rc0(rcn);
        sc0[me] = rc0[me] = 0;
        // one grouped exchange: {slot, lt, rank, val} (20 B) or {slot, packed, val} (16 B)
        const void* s4[4] = {c->r_skey.p, c->r_slt.p, c->r_sval.p, c->r_srank.p};
        void* r4[4] = {c->r_key.p, c->r_lt.p, c->r_val.p, c->r_rank.p};
        const uint32_t e4[4] = {4, 8, 4, 4};
        if ((st = comm_all_to_all(c, wire_pk ? 3 : 4, s4, r4, e4, sc0.data(), sd.data(), rc0.data(), rd.data(), n,
                                  nr)))
            return st;
        rc.key = c->r_key.p; rc.lt = c->r_lt.p; rc.rank = c->r_rank.p; rc.val = c->r_val.p;
        rc.packed_in = wire_pk;
        if (wire_pk && !use_sorted(c, c->segs, R, dflags)) {         // the gather path reads (lt, rank)
            if (nr) k_unpack_routed<<<grid_for(nr, 256), 256, 0, c->stream>>>(c->r_lt.p, c->r_rank.p, nr, pf);
            rc.packed_in = false;
        }
        if (dflags) rflags = c->r_flags.p;
    }
    HIPLST(hipGetLastError());
    test_stall(c, kStallFinish);
    set_phase(c, "owners' apply and the final reduction");

    // 5-6: apply what this rank owns; finish_apply SUM-reduces the counts, the error word and a failure of
    // any rank's apply (a rank that failed before its finish_apply posts that reduction here)
    if (inject_fail(c, kFailOwner) || inject_fail(c, kFailApply)) {
        st = CRDT_E_NOMEM;
    } else if (lst) {
        st = lst;
    } else if (comb) {                            // packed keys carry their changesets: the sorted path only
        c->last_sorted = true;
        c->last_flagged = false;
        st = apply_sorted(c, rc, c->segs, wall, c->d_event.p, out);
    } else {
        st = apply_segs(c, rc, nr, CRDT_MEM_DEVICE, wall, c->d_event.p, rflags, out, true);
    }
    if (st < 0 && !c->finish_posted) st = finish_apply(c, nullptr, nullptr, 0, c->last_sorted, out, st);
    if (st < 0) return drain_side(c, st);
    if (dflags && !c->presharded) {                          // win flags back to the senders (r_sflags: prep)
        if (sc[me])
            HIPLST(hipMemcpyAsync(c->r_sflags.p + sd[me], c->r_flags.p + rd[me], sc[me], hipMemcpyDeviceToDevice,
                                  c->stream));
        set_phase(c, "win flags back to their senders");
        std::vector<uint64_t> back_s(rcn), back_r(sc);
        back_s[me] = back_r[me] = 0;
        const void* s1[1] = {c->r_flags.p};
        void* r1[1] = {c->r_sflags.p};
        const uint32_t e1 = 1;
        int cs = comm_all_to_all(c, 1, s1, r1, &e1, back_s.data(), rd.data(), back_r.data(), sd.data(), nr, n);
        if (cs) return cs;
        if (lst) return drain_side(c, lst);            // (rank-local: the exchange was posted)
        if (n) k_flags_back<<<grid_for(n, 256), 256, 0, c->stream>>>(c->r_sflags.p, c->r_perm.p, n, dflags);
        HIPCHK(hipGetLastError());
    }
    if (c->timing) ev_record(c, kEvEnd);
    if (win_flags && batch->mem == CRDT_MEM_HOST && n)
        HIPCHK(hipMemcpyAsync(win_flags, dflags, n, hipMemcpyDeviceToHost, c->stream));
    SYNCHK(c, c->stream);
    collect_timing(c);
    return st;
}

int merge_sharded(crdt_ctx* c, const crdt_batch* batch, int64_t wall, uint8_t* win_flags, crdt_result* out) {
    if (c->comm_state.load()) return CRDT_E_COMM;       // aborted: join a communicator again first
    c->tune_mode = win_flags ? -1 : route_tune_mode(c, batch);
    c->tune_trial = false;
    const auto t0 = std::chrono::steady_clock::now();
    c->comm_deadline_ns = c->comm_timeout_ms ? now_ns() + (int64_t)c->comm_timeout_ms * 1000000 : 0;
    int st = merge_sharded_call(c, batch, wall, win_flags, out);   // (ends with a stream synchronisation)
    set_phase(c, st == CRDT_E_COMM ? "aborted" : "idle");
    if (st == CRDT_E_COMM) {                            // rank-local: the schedule may differ across ranks now
        c->rt = crdt_ctx::RouteTune{};
        return st;
    }
    // a failed call (an agreed status, the same on every rank: this file's header) restarts its way's trials,
    // on every rank
    if (st < 0 && c->tune_trial && c->rt.best < 0) c->rt.trial -= c->rt.trial % kTrials;
    if (st || !c->tune_trial || c->rt.best >= 0) return st;
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return route_tune_record(c, ms);
}

int comm_attach(crdt_ctx* c, uint32_t n_ranks, uint32_t rank, const crdt_comm_ops& ops) {
    if (n_ranks == 0 || rank >= n_ranks || n_ranks > (uint32_t)kRouteMaxRanks) return CRDT_E_INVALID;
    if (!ops.all_reduce_i64 || !ops.all_gather_i64 || !ops.all_to_all_v) return CRDT_E_INVALID;
    if (ops.mem != CRDT_MEM_HOST && ops.mem != CRDT_MEM_DEVICE) return CRDT_E_INVALID;
    // the buffers of the collectives that carry failures (every call posts them, a failing rank too)
    HIPALLOC(c->d_sum.ensure(kSumWords + kSumCodes));
    HIPALLOC(c->h_sum.ensure(kSumWords + kSumCodes));
    HIPALLOC(c->d_agree.ensure(2));
    HIPALLOC(c->h_agree.ensure(2));
    HIPALLOC(c->d_rl1cnt.ensure(2ull * kDigits * kRl1MaxPieces + 2 + kDigits));
    HIPALLOC(c->h_rl1cnt.ensure(2ull * kDigits * kRl1MaxPieces + 2 + kDigits));
    c->ops = ops;
    c->n_ranks = n_ranks;
    c->rank = rank;
    c->has_comm = true;
    c->comm_state.store(0);
    set_phase(c, "idle");
    c->rt = crdt_ctx::RouteTune{};
    for (int i = 1; i < crdt_ctx::kPlaceMax; ++i) {      // a sharded ctx partitions elsewhere (route_l1, the
        c->pc_rec[i].release();                          // fold): no placement trials, no candidate buffers
        c->pc_kj[i].release();
    }
    c->place_k = 0;
    c->place_trial = 0;
    c->place_best = -1;
    return CRDT_OK;
}

void comm_release(crdt_ctx* c) {
    if (c->rccl_comm && g_rccl.comm_destroy) g_rccl.comm_destroy(static_cast<ncclComm_t>(c->rccl_comm));
    c->rccl_comm = nullptr;
    c->has_comm = false;
    c->n_ranks = 1;
    c->rank = 0;
    c->ops = crdt_comm_ops{};
}

}  // namespace

extern "C" {

int crdt_comm_unique_id(uint8_t* id) {
    if (!id) return CRDT_E_INVALID;
    int st = rccl_load();
    if (st) return st;
    ncclUniqueId u;
    static_assert(sizeof(u) == CRDT_COMM_ID_BYTES, "ncclUniqueId is 128 bytes");
    if (g_rccl.get_unique_id(&u) != ncclSuccess) return CRDT_E_COMM;
    memcpy(id, &u, sizeof(u));
    return CRDT_OK;
}

int crdt_comm_init_rccl(crdt_ctx* c, uint32_t n_ranks, uint32_t rank, const uint8_t* id) {
    if (!c || !id || n_ranks == 0 || rank >= n_ranks) return CRDT_E_INVALID;
    int st = rccl_load();
    if (st) return st;
    HIPCHK(hipSetDevice(c->device));
    comm_release(c);
    ncclUniqueId u;
    memcpy(&u, id, sizeof(u));
    ncclComm_t comm = nullptr;
    if (g_rccl.comm_init_rank(&comm, (int)n_ranks, u, (int)rank) != ncclSuccess) return CRDT_E_COMM;
    c->rccl_comm = comm;
    crdt_comm_ops ops{};
    ops.user = c;
    ops.mem = CRDT_MEM_DEVICE;
    ops.all_reduce_i64 = rccl_all_reduce;
    ops.all_gather_i64 = rccl_all_gather;
    ops.all_to_all_v = rccl_all_to_all_v;
    st = comm_attach(c, n_ranks, rank, ops);
    if (st) comm_release(c);
    return st;
}

int crdt_comm_init_ops(crdt_ctx* c, uint32_t n_ranks, uint32_t rank, const crdt_comm_ops* ops) {
    if (!c || !ops) return CRDT_E_INVALID;
    comm_release(c);
    return comm_attach(c, n_ranks, rank, *ops);
}

int crdt_comm_info(const crdt_ctx* c, uint32_t* n_ranks, uint32_t* rank) {
    if (!c || !n_ranks || !rank) return CRDT_E_INVALID;
    *n_ranks = c->n_ranks;
    *rank = c->rank;
    return CRDT_OK;
}

int crdt_comm_free(crdt_ctx* c) {
    if (!c) return CRDT_E_INVALID;
    hipSetDevice(c->device);
    if (c->stream) hipStreamSynchronize(c->stream);
    comm_release(c);
    return CRDT_OK;
}

int crdt_set_comm_timeout(crdt_ctx* c, uint32_t ms) {
    if (!c) return CRDT_E_INVALID;
    c->comm_timeout_ms = ms;
    return CRDT_OK;
}

int crdt_comm_state(const crdt_ctx* c, int32_t* state, const char** phase) {
    if (!c || !state || !phase) return CRDT_E_INVALID;
    *state = c->comm_state.load();
    *phase = c->comm_phase.load(std::memory_order_relaxed);
    return CRDT_OK;
}

int crdt_set_presharded(crdt_ctx* c, int presharded) {
    if (!c || (presharded != 0 && presharded != 1)) return CRDT_E_INVALID;
    c->presharded = presharded != 0;
    return CRDT_OK;
}

}  // extern "C"

namespace {
