// table_purge.inc — crdt_purge_tombstones: the tombstones a group of replicas agrees on, dropped from every
// one of them (DESIGN §6k).  Included from crdt_merge.hip inside its anonymous namespace, after table_live.inc;
// the tile (kTmTile rows, a thread's rows tm_row(base, q)) is table_merge.inc's, the flag store table_live.inc's.
// Member j holds row i visibly iff its mod >= 0 (the sign of mod_hi) and as a tombstone iff, besides, its val is
// CRDT_NULL_VALUE (crdt_tombstone_live's predicates).  Row i is a candidate iff member 0 holds a tombstone with
// lt < before (signed, strict) and purged iff, besides, every member holds a tombstone of member 0's (lt, rank);
// mod is never compared (replicas stamp their own).
//   k_pg_purge   one streaming pass, a capped grid striding over the tiles.  A thread loads {lt, rank, mod_hi}
//                and val of its kTmItems rows of member 0 (every 128-B line of its table once), rows past n
//                clamped to row n - 1 and masked, and forms the 8-bit mask of its candidate rows.  Members 1 ..
//                n_ctx - 1 are visited member-outer, rows-inner: a member's row is loaded only where the bit is
//                still set, all of a thread's loads of one member in flight together, and a wave whose ballot
//                of remaining bits is zero skips the members that are left (wave-uniform: no barrier sits in the
//                loop).  So a table with few tombstones costs one stream of member 0 plus the lines its
//                candidates touch in the others.  The rows that survived every member are then stored in every
//                member as the never-written fill, kFill in every word of the stride (crdt_clear_rows' 0x80
//                memset: 16 + 8 B, or one aligned 32-B store whose padding is fill too, not store_hc's zeros);
//                the members may mix 24-B and 32-B rows.  Every row of every table belongs to one thread, which
//                reads it before it writes it, and reads nothing after its first store.
//                flags[row] (optional) = 1 where the row was purged, else 0, every row of [0, n): lv_store_flags.
//                Candidates and purged rows are counted in two registers over the workgroup's tiles, reduced by
//                wave shuffle, handed through LDS to thread 0: one atomicAdd per workgroup and word onto
//                words[0] (candidates) and words[1] (purged), none where the value is zero.
constexpr int kPgMax = 8;                        // CRDT_PURGE_MAX
constexpr unsigned kPgGrid = 2048;               // as kLvGrid: 256 CUs x 8 resident workgroups
static_assert(kPgMax == CRDT_PURGE_MAX, "the header's bound");
static_assert(kTmItems <= 8, "a thread's candidate rows are one byte of bits");

struct PgArgs { Table t[kPgMax]; };              // by value: the members' tables

// Row k of t as crdt_clear_rows leaves it: every byte of the stride 0x80.
__device__ inline void pg_store_fill(const Table& t, uint64_t k)
{
    constexpr uint32_t f = 0x80808080u;
    char* p = row_ptr(t, k);
    if (t.stride == 32) {                        // one aligned 32-B store
        u32x8a a;
        a.s0 = f; a.s1 = f; a.s2 = f; a.s3 = f; a.s4 = f; a.s5 = f; a.s6 = f; a.s7 = f;
        *reinterpret_cast<u32x8a*>(p) = a;
        return;
    }
    u32x4u a;
    a.x = f; a.y = f; a.z = f; a.w = f;
    *reinterpret_cast<u32x4u*>(p) = a;
    u32x2u b;
    b.x = f; b.y = f;
    *reinterpret_cast<u32x2u*>(p + 16) = b;
}

__global__ __launch_bounds__(kTmThreads) void k_pg_purge(PgArgs a, uint32_t n_ctx, uint64_t n, uint32_t nb,
                                                         int64_t before, uint8_t* __restrict__ flags,
                                                         unsigned long long* __restrict__ words)
{
    __shared__ uint32_t s_cnt[2][4];             // per wave: candidates, purged
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // (wave-uniform)
    uint32_t ncand = 0, npurged = 0;             // (a thread sees at most 8 rows of each of its tiles)
    for (uint32_t tile = blockIdx.x; tile < nb; tile += gridDim.x) {
        const uint64_t base = (uint64_t)tile * kTmTile;
        const Table t0 = a.t[0];
        uint4 h[kTmItems];
        uint32_t v[kTmItems];
#pragma unroll
        for (int q = 0; q < kTmItems; ++q) {
            const uint64_t i = tm_row(base, q);
            const uint64_t ic = i < n ? i : n - 1;
            h[q] = load_hot(t0, ic);
            v[q] = *reinterpret_cast<const uint32_t*>(row_ptr(t0, ic) + 20);
        }
        uint32_t m = 0;                          // bit q: row q is a candidate no member has blocked yet
#pragma unroll
        for (int q = 0; q < kTmItems; ++q) {
            const bool cand = tm_row(base, q) < n && (int32_t)h[q].w >= 0 && v[q] == CRDT_NULL_VALUE &&
                              hot_lt(h[q]) < before;
            m |= (uint32_t)cand << q;
        }
        ncand += (uint32_t)__popc(m);
#pragma unroll 1
        for (uint32_t j = 1; j < n_ctx; ++j) {
            if (__ballot(m != 0) == 0) break;    // (the whole wave: nothing left to confirm)
            const Table t = a.t[j];
            uint4 g[kTmItems];
            uint32_t u[kTmItems];
#pragma unroll
            for (int q = 0; q < kTmItems; ++q) {
                g[q] = make_uint4(0u, 0u, 0u, 0x80000000u);   // (not loaded: invisible, and its bit is clear)
                u[q] = 0u;
                if ((m >> q) & 1u) {
                    const uint64_t i = tm_row(base, q);
                    g[q] = load_hot(t, i);
                    u[q] = *reinterpret_cast<const uint32_t*>(row_ptr(t, i) + 20);
                }
            }
            uint32_t ok = 0;
#pragma unroll
            for (int q = 0; q < kTmItems; ++q) {
                const bool same = (int32_t)g[q].w >= 0 && u[q] == CRDT_NULL_VALUE && g[q].x == h[q].x &&
                                  g[q].y == h[q].y && g[q].z == h[q].z;
                ok |= (uint32_t)same << q;
            }
            m &= ok;
        }
        // every load of this thread's rows is done: the agreed rows become the fill in every member
#pragma unroll 1
        for (uint32_t j = 0; j < n_ctx; ++j) {
            if (__ballot(m != 0) == 0) break;    // (the whole wave)
            const Table t = a.t[j];
#pragma unroll
            for (int q = 0; q < kTmItems; ++q)
                if ((m >> q) & 1u) pg_store_fill(t, tm_row(base, q));
        }
        npurged += (uint32_t)__popc(m);
        if (flags) {
#pragma unroll
            for (int q = 0; q < kTmItems; ++q)
                lv_store_flags(flags, base + (uint64_t)q * kTmThreads + (uint64_t)w * 64, n, lane, (m >> q) & 1u);
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        ncand += __shfl_xor(ncand, off, 64);
        npurged += __shfl_xor(npurged, off, 64);
    }
    if (lane == 0) { s_cnt[0][w] = ncand; s_cnt[1][w] = npurged; }
    __syncthreads();
    if (threadIdx.x != 0) return;
    const unsigned long long c = (unsigned long long)s_cnt[0][0] + s_cnt[0][1] + s_cnt[0][2] + s_cnt[0][3];
    const unsigned long long p = (unsigned long long)s_cnt[1][0] + s_cnt[1][1] + s_cnt[1][2] + s_cnt[1][3];
    if (c) atomicAdd(&words[0], c);
    if (p) atomicAdd(&words[1], p);
}
