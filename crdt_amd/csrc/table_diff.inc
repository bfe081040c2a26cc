// table_diff.inc — crdt_diff_tables: the read-only comparison of two replicas of one device and one id space
// ("are they converged, and if not, who is ahead on which rows?"), and crdt_digest_rows: one 64-bit word per
// block of rows of one table (DESIGN §6i).  Included from crdt_merge.hip inside its anonymous namespace,
// after table_merge.inc, whose tile (kTmTile rows, a thread's rows tm_row(base, q)) and hlc_gt both kernels
// reuse.  Neither kernel writes a table; their scratch is the result words.
//   k_df_diff    one streaming pass over both tables, a capped grid striding over the tiles.  A thread loads
//                both halves of its kTmItems rows of BOTH tables before it uses any (every 128-B line of a
//                24-B or 32-B table holds part of a decision half, so the val half adds no HBM traffic),
//                rows past n clamped to row n - 1 and masked.  Per row, with va / vb the visibility (mod >= 0):
//                  A_AHEAD  va && (!vb || hlc_a > hlc_b)      (the win rule of b.merge(a's record), crdt.dart:83-84)
//                  B_AHEAD  the same with the sides swapped
//                  CONFLICT va && vb && hlc_a == hlc_b && val_a != val_b
//                The byte goes to flags[row] (optional) from the thread that owns the row; the 64 zero bytes of a
//                wave-instruction whose rows all agree go out as eight 8-B stores where whole and aligned.  The
//                five counts (rows carrying each bit, visible rows of each side) and the smallest row id with a
//                non-zero byte are kept in registers over the workgroup's tiles, reduced by wave shuffle, handed
//                through LDS to thread 0: at most five atomicAdd and one atomicMin per workgroup onto words[0..5],
//                none where the value is zero or unset.
//   k_df_digest  word k = the wrapping sum over rows i of block k of mix(i, row_i), mix being bench.py's
//                row_digests (constants included).  A capped grid strides over the tiles; block_rows is a power
//                of two >= kTmTile, so a tile lies in one block: the tile's sum is reduced in the workgroup and
//                one atomicAdd goes onto words[tile >> shift] (integer sums commute: the words do not depend
//                on scheduling).  kState: an invisible row contributes 0 and a visible one leaves mod out, the
//                digest of what Record == sees (record.dart:34-35).
constexpr unsigned kDfGrid = 2048;               // as kTmClockGrid: 256 CUs x 8 resident workgroups
constexpr int kDfWords = 6;                      // n_a_ahead, n_b_ahead, n_conflict, n_visible_a, n_visible_b, first_diff
static_assert(CRDT_DIFF_A_AHEAD == 1 && CRDT_DIFF_B_AHEAD == 2 && CRDT_DIFF_CONFLICT == 4, "the header's bits");
static_assert(sizeof(crdt_diff) == kDfWords * sizeof(uint64_t), "the words are the struct's fields, in order");

__global__ __launch_bounds__(kTmThreads) void k_df_diff(Table ta, Table tb, uint64_t n, uint32_t nb,
                                                        uint8_t* __restrict__ flags,
                                                        unsigned long long* __restrict__ words)
{
    __shared__ uint32_t s_cnt[5][4];             // per wave
    __shared__ unsigned long long s_first[4];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // (wave-uniform)
    uint32_t na = 0, nbh = 0, nc = 0, va_n = 0, vb_n = 0;   // (a thread sees at most 8 rows of each of its tiles)
    unsigned long long first = ~0ull;
    for (uint32_t tile = blockIdx.x; tile < nb; tile += gridDim.x) {
        const uint64_t base = (uint64_t)tile * kTmTile;
        uint4 ha[kTmItems], hb[kTmItems];
        uint2 xa[kTmItems], xb[kTmItems];
        unsigned long long bytes = 0;            // byte q: the flag byte of row q
#pragma unroll
        for (int q = 0; q < kTmItems; ++q) {
            const uint64_t i = tm_row(base, q);
            const uint64_t ic = i < n ? i : n - 1;
            ha[q] = load_hot(ta, ic);
            xa[q] = load_cold(ta, ic);
            hb[q] = load_hot(tb, ic);
            xb[q] = load_cold(tb, ic);
        }
#pragma unroll
        for (int q = 0; q < kTmItems; ++q) {
            const uint64_t i = tm_row(base, q);
            const bool in = i < n;
            const bool va = in && (int32_t)ha[q].w >= 0, vb = in && (int32_t)hb[q].w >= 0;
            const bool agt = hlc_gt(ha[q], hb[q]), bgt = hlc_gt(hb[q], ha[q]);
            const bool a_ahead = va && (!vb || agt), b_ahead = vb && (!va || bgt);
            const bool conflict = va && vb && !agt && !bgt && xa[q].y != xb[q].y;
            const uint32_t byte = (a_ahead ? CRDT_DIFF_A_AHEAD : 0) | (b_ahead ? CRDT_DIFF_B_AHEAD : 0) |
                                  (conflict ? CRDT_DIFF_CONFLICT : 0);
            na += a_ahead;
            nbh += b_ahead;
            nc += conflict;
            va_n += va;
            vb_n += vb;
            if (byte && i < first) first = i;
            bytes |= (unsigned long long)byte << (8 * q);
        }
        if (!flags) continue;
#pragma unroll
        for (int q = 0; q < kTmItems; ++q) {
            // a wave-instruction's 64 rows are 64 consecutive bytes: where none of them differs (the usual case)
            // and the segment is whole and 8-B aligned, eight lanes store its zeros, 8 B each
            const uint32_t byte = (uint32_t)(bytes >> (8 * q)) & 0xFFu;
            const uint64_t seg = base + (uint64_t)q * kTmThreads + (uint64_t)w * 64;
            if (__ballot(byte != 0) == 0 && seg + 64 <= n && (reinterpret_cast<uintptr_t>(flags + seg) & 7u) == 0) {
                if (lane < 8) reinterpret_cast<unsigned long long*>(flags + seg)[lane] = 0ull;
            } else if (seg + lane < n) {
                flags[seg + lane] = (uint8_t)byte;
            }
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        na += __shfl_xor(na, off, 64);
        nbh += __shfl_xor(nbh, off, 64);
        nc += __shfl_xor(nc, off, 64);
        va_n += __shfl_xor(va_n, off, 64);
        vb_n += __shfl_xor(vb_n, off, 64);
        const unsigned long long f = __shfl_xor(first, off, 64);
        first = f < first ? f : first;
    }
    if (lane == 0) {
        s_cnt[0][w] = na; s_cnt[1][w] = nbh; s_cnt[2][w] = nc; s_cnt[3][w] = va_n; s_cnt[4][w] = vb_n;
        s_first[w] = first;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int k = 0; k < 5; ++k) {
        const unsigned long long t = (unsigned long long)s_cnt[k][0] + s_cnt[k][1] + s_cnt[k][2] + s_cnt[k][3];
        if (t) atomicAdd(&words[k], t);
    }
    for (int ww = 0; ww < 4; ++ww) first = s_first[ww] < first ? s_first[ww] : first;
    if (first != ~0ull) atomicMin(&words[5], first);
}

// bench.py row_digests' constants
constexpr unsigned long long kDgP0 = 0x9E3779B97F4A7C15ull, kDgP1 = 0xC2B2AE3D27D4EB4Full,
                             kDgP2 = 0x165667B19E3779F9ull, kDgP3 = 0xD6E8FEB86659FD93ull,
                             kDgP4 = 0xFF51AFD7ED558CCDull;

template <bool kState>
__global__ __launch_bounds__(kTmThreads) void k_df_digest(Table t, uint64_t n, uint32_t nb, uint32_t shift,
                                                          unsigned long long* __restrict__ words)
{
    __shared__ unsigned long long s_sum[2][4];   // per wave; one buffer per tile parity
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint32_t par = 0;
    for (uint32_t tile = blockIdx.x; tile < nb; tile += gridDim.x, par ^= 1u) {
        const uint64_t base = (uint64_t)tile * kTmTile;
        uint4 h[kTmItems];
        uint2 x[kTmItems];
#pragma unroll
        for (int q = 0; q < kTmItems; ++q) {
            const uint64_t i = tm_row(base, q);
            const uint64_t ic = i < n ? i : n - 1;
            h[q] = load_hot(t, ic);
            x[q] = load_cold(t, ic);
        }
        unsigned long long sum = 0;
#pragma unroll
        for (int q = 0; q < kTmItems; ++q) {
            const uint64_t i = tm_row(base, q);
            const unsigned long long lt = ((unsigned long long)h[q].y << 32) | h[q].x;
            const unsigned long long mod = ((unsigned long long)h[q].w << 32) | x[q].x;
            const unsigned long long rv = ((unsigned long long)h[q].z << 32) | x[q].y;
            unsigned long long m = lt * kDgP0 ^ rv * kDgP2 ^ i * kDgP3;
            if (!kState) m ^= mod * kDgP1;
            m ^= m >> 29;
            m *= kDgP4;
            m ^= m >> 32;
            const bool take = i < n && (!kState || (int32_t)h[q].w >= 0);
            sum += take ? m : 0ull;
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off, 64);
        if (lane == 0) s_sum[par][w] = sum;
        __syncthreads();                         // (the next tile writes the other buffer)
        if (threadIdx.x == 0) {
            const unsigned long long total = s_sum[par][0] + s_sum[par][1] + s_sum[par][2] + s_sum[par][3];
            if (total) atomicAdd(&words[tile >> shift], total);
        }
    }
}
