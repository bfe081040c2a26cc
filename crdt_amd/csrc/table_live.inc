// table_live.inc — crdt_tombstone_live: Crdt.clear() (crdt.dart:67-73, putAll of null over the live view) on
// the table itself (DESIGN §6j).  Included from crdt_merge.hip inside its anonymous namespace, after
// table_diff.inc; the tile (kTmTile rows, a thread's rows tm_row(base, q)) is table_merge.inc's.
// A row is live iff it is visible (mod >= 0, the sign of mod_hi) and its val is not CRDT_NULL_VALUE.
//   k_lv_tombstone  one streaming pass, a capped grid striding over the tiles.  A thread loads the 12 B
//                {mod_hi, mod_lo, val} of its kTmItems rows (k_ex_count's load: every 128-B line of a 24-B or
//                32-B table once), rows past n clamped to row n - 1 and masked, and stores the whole row
//                {lt = stamp, rank = local_rank, mod = stamp, val = CRDT_NULL_VALUE} over its LIVE rows only
//                (store_hc: 16 + 8 B, or one aligned 32-B store with the zero padding).  Every row belongs to
//                one thread, which reads it before it writes it.  The host has already taken Hlc.send, so the
//                stamp is final; whether the canonical moves is decided by the count.
//                flags[row] (optional) = 1 where the row was tombstoned, else 0, every row of [0, n): a
//                wave-instruction's 64 rows are 64 consecutive bytes, the wave's ballot; where the segment is
//                whole and 8-B aligned eight lanes store 8 B of it each (lv_spread8), else each lane its byte.
//                The live rows are counted in a register over the workgroup's tiles, reduced by wave shuffle,
//                handed through LDS to thread 0: one atomicAdd per workgroup onto *word, none where zero.
constexpr unsigned kLvGrid = 2048;               // as kDfGrid: 256 CUs x 8 resident workgroups

// Bit k of b (k < 8) as byte k of the result, 0 or 1.
__device__ inline unsigned long long lv_spread8(uint32_t b)
{
    const unsigned long long y = ((unsigned long long)(b & 0xFFu) * 0x0101010101010101ull) & 0x8040201008040201ull;
    return ((y + 0x7F7F7F7F7F7F7F7Full) >> 7) & 0x0101010101010101ull;   // (a byte is at most 0x80: no carry out)
}

// One wave-instruction's flag bytes: the 64 consecutive rows from seg on, this lane's row seg + lane carrying
// bit.  Every lane of the wave calls it (it takes the ballot); shared with k_pg_purge (table_purge.inc).
__device__ inline void lv_store_flags(uint8_t* __restrict__ flags, uint64_t seg, uint64_t n, int lane, bool bit)
{
    const unsigned long long b = __ballot(bit);
    if (seg + 64 <= n && (reinterpret_cast<uintptr_t>(flags + seg) & 7u) == 0) {
        if (lane < 8)
            reinterpret_cast<unsigned long long*>(flags + seg)[lane] = lv_spread8((uint32_t)(b >> (8 * lane)));
    } else if (seg + lane < n) {
        flags[seg + lane] = (uint8_t)bit;
    }
}

__global__ __launch_bounds__(kTmThreads) void k_lv_tombstone(Table t, uint64_t n, uint32_t nb, int64_t stamp,
                                                             uint32_t local_rank, uint8_t* __restrict__ flags,
                                                             unsigned long long* __restrict__ word)
{
    __shared__ uint32_t s_live[4];               // per wave
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // (wave-uniform)
    const uint32_t st_lo = (uint32_t)stamp, st_hi = (uint32_t)((uint64_t)stamp >> 32);
    const uint4 th = make_uint4(st_lo, st_hi, local_rank, st_hi);
    const uint2 tx = make_uint2(st_lo, CRDT_NULL_VALUE);
    uint32_t live = 0;                           // (a thread sees at most 8 rows of each of its tiles)
    for (uint32_t tile = blockIdx.x; tile < nb; tile += gridDim.x) {
        const uint64_t base = (uint64_t)tile * kTmTile;
        u32x3u v[kTmItems];
#pragma unroll
        for (int q = 0; q < kTmItems; ++q) {
            const uint64_t i = tm_row(base, q);
            v[q] = *reinterpret_cast<const u32x3u*>(row_ptr(t, i < n ? i : n - 1) + 12);
        }
#pragma unroll
        for (int q = 0; q < kTmItems; ++q) {
            const uint64_t i = tm_row(base, q);
            const bool is_live = i < n && (int32_t)v[q].x >= 0 && v[q].z != CRDT_NULL_VALUE;
            if (is_live) store_hc(t, i, th, tx);
            live += is_live;
            if (flags) lv_store_flags(flags, base + (uint64_t)q * kTmThreads + (uint64_t)w * 64, n, lane, is_live);
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) live += __shfl_xor(live, off, 64);
    if (lane == 0) s_live[w] = live;
    __syncthreads();
    if (threadIdx.x != 0) return;
    const unsigned long long total = (unsigned long long)s_live[0] + s_live[1] + s_live[2] + s_live[3];
    if (total) atomicAdd(word, total);
}
