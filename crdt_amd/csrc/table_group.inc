// table_group.inc — crdt_diff_group: the read-only comparison of up to 8 replicas of one device and one id space
// ("are they all converged, who lacks the winning record, who holds news nobody else has?", DESIGN §6l).
// Included from crdt_merge.hip inside its anonymous namespace, after table_purge.inc; the tile (kTmTile rows, a
// thread's rows tm_row(base, q)) and hlc_gt are table_merge.inc's, the capped grid table_diff.inc's, the flag
// store of the conflict bytes table_live.inc's.  The kernel writes no table; its scratch is the result words.
// Member j holds row i visibly iff its mod >= 0 (the sign of mod_hi); hlc = (lt, rank), signed lt then unsigned
// rank; mod is never compared and values are compared by handle (crdt_diff_tables' predicates).  Per row:
//   hold    bit j: member j is visible and its hlc is the greatest among the visible members
//   behind  bit j (j < n_ctx): bit j of hold is clear, on a row some member holds; 0 where nobody holds it
//   conflict 1: two members of hold carry different val
//   k_gd_diff    one streaming pass, a capped grid striding over the tiles, members outer and rows inner (as
//                k_pg_purge visits its members).  A thread loads both halves of its kTmItems rows of ONE member,
//                all in flight together (every 128-B line of a 24-B or 32-B table once), rows past n clamped to
//                row n - 1 and masked, and folds them into five registers per row: the top (lt lo, lt hi, rank),
//                the top's val, and one state word {hold byte, conflict bit, visible byte}.  A visible record
//                above the top (or the first visible one) replaces it, makes hold its own bit and clears the
//                conflict; an equal one joins hold and sets the conflict where its val is not the kept one (all
//                holders equal to the kept val, or the conflict is already set: one kept val is enough); an
//                invisible one changes nothing.  No member's rows outlive its fold, so eight members cost the
//                registers of one; there is no early exit, every row of every member is read once; the members
//                may mix 24-B and 32-B rows.
//                The three bytes go to behind[row], hold[row], conflict[row] (each optional) from the wave that
//                owns the 64 consecutive rows: where all 64 bytes are equal (the converged run: behind 0, hold
//                all members) and the segment is whole and 8-B aligned eight lanes store 8 B each, else each
//                lane its byte; the conflict bytes through lv_store_flags.
//                Counts: rows held, disputed and in conflict and the smallest such row id in four registers as
//                k_df_diff keeps its six; the per-member counts (visible, holding, sole holder) as byte-sliced
//                sums, bit j of a row's byte adding 1 to byte j of a 64-bit register (lv_spread8), at most 8 per
//                tile and flushed every kGdFlush tiles (248 <= 255) by wave shuffle into the wave's LDS words.
//                Thread 0 adds the four waves' words, forms behind_j = held - holding_j for j < n_ctx, and issues
//                at most one atomicAdd per non-zero word and one atomicMin per workgroup onto words[0..27].
constexpr int kGdMax = 8;                        // CRDT_GROUP_MAX
constexpr int kGdWords = 4 + 3 * kGdMax;         // crdt_group_diff's fields, in order
constexpr int kGdFlush = 31;                     // tiles between two flushes of the byte-sliced sums: 31 * 8 <= 255
static_assert(kGdMax == CRDT_GROUP_MAX, "the header's bound");
static_assert(sizeof(crdt_group_diff) == kGdWords * sizeof(uint64_t), "the words are the struct's fields, in order");
static_assert(kTmItems * kGdFlush <= 255, "a byte of the sliced sums holds the rows between two flushes");

struct GdArgs { Table t[kGdMax]; };              // by value: the members' tables

// The eight byte sums of x, each reduced over the wave, added onto the wave's eight LDS words; x restarts at 0.
// Every lane of the wave calls it.
__device__ inline void gd_flush(unsigned long long& x, uint32_t* __restrict__ slot, int lane)
{
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        uint32_t v = (uint32_t)(x >> (8 * k)) & 0xFFu;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
        if (lane == 0) slot[k] += v;
    }
    x = 0;
}

// One wave-instruction's mask bytes: the 64 consecutive rows from seg on, this lane's row seg + lane carrying byte.
// Every lane of the wave calls it (it takes the ballot).
__device__ inline void gd_store_bytes(uint8_t* __restrict__ out, uint64_t seg, uint64_t n, int lane, uint32_t byte)
{
    const uint32_t b0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)byte);
    if (__ballot(byte != b0) == 0 && seg + 64 <= n && (reinterpret_cast<uintptr_t>(out + seg) & 7u) == 0) {
        if (lane < 8) reinterpret_cast<unsigned long long*>(out + seg)[lane] = b0 * 0x0101010101010101ull;
    } else if (seg + lane < n) {
        out[seg + lane] = (uint8_t)byte;
    }
}

__global__ __launch_bounds__(kTmThreads) void k_gd_diff(GdArgs a, uint32_t n_ctx, uint64_t n, uint32_t nb,
                                                        uint8_t* __restrict__ behind, uint8_t* __restrict__ hold,
                                                        uint8_t* __restrict__ conflict,
                                                        unsigned long long* __restrict__ words)
{
    __shared__ uint32_t s_cnt[4][3 + 3 * kGdMax];    // per wave: held, disputed, conflict; visible, holding, sole
    __shared__ unsigned long long s_first[4];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // (wave-uniform)
    for (int k = threadIdx.x; k < 4 * (3 + 3 * kGdMax); k += kTmThreads) (&s_cnt[0][0])[k] = 0u;
    __syncthreads();
    const uint32_t full = (1u << n_ctx) - 1u;
    uint32_t n_held = 0, n_disp = 0, n_conf = 0;     // (a thread sees at most 8 rows of each of its tiles)
    unsigned long long first = ~0ull;
    unsigned long long vis_s = 0, hold_s = 0, sole_s = 0;   // byte j: rows carrying member j's bit since the last flush
    uint32_t pending = 0;
    for (uint32_t tile = blockIdx.x; tile < nb; tile += gridDim.x) {
        const uint64_t base = (uint64_t)tile * kTmTile;
        uint32_t tx[kTmItems], ty[kTmItems], tz[kTmItems], tv[kTmItems];   // the top's lt lo, lt hi, rank; its val
        uint32_t st[kTmItems];                       // bits 0-7 hold, bit 8 conflict, bits 16-23 visible
#pragma unroll
        for (int q = 0; q < kTmItems; ++q) { tx[q] = ty[q] = tz[q] = tv[q] = 0u; st[q] = 0u; }
#pragma unroll 1
        for (uint32_t j = 0; j < n_ctx; ++j) {
            const Table t = a.t[j];
            uint4 g[kTmItems];
            uint2 x[kTmItems];
#pragma unroll
            for (int q = 0; q < kTmItems; ++q) {
                const uint64_t i = tm_row(base, q);
                const uint64_t ic = i < n ? i : n - 1;
                g[q] = load_hot(t, ic);
                x[q] = load_cold(t, ic);
            }
            const uint32_t bit = 1u << j;
#pragma unroll
            for (int q = 0; q < kTmItems; ++q) {
                const bool vis = tm_row(base, q) < n && (int32_t)g[q].w >= 0;
                const uint4 top = make_uint4(tx[q], ty[q], tz[q], 0u);
                const bool take = vis && ((st[q] & 0xFFu) == 0u || hlc_gt(g[q], top));
                const bool same = vis && !take && g[q].x == tx[q] && g[q].y == ty[q] && g[q].z == tz[q];
                tx[q] = take ? g[q].x : tx[q];
                ty[q] = take ? g[q].y : ty[q];
                tz[q] = take ? g[q].z : tz[q];
                uint32_t s = st[q];
                s = take ? ((s & 0xFFFF0000u) | bit) : s;                      // hold = its bit, conflict cleared
                s |= same ? (bit | (x[q].y != tv[q] ? 0x100u : 0u)) : 0u;
                s |= vis ? (bit << 16) : 0u;
                tv[q] = take ? x[q].y : tv[q];
                st[q] = s;
            }
        }
#pragma unroll
        for (int q = 0; q < kTmItems; ++q) {
            const uint64_t i = tm_row(base, q);
            const uint32_t h = st[q] & 0xFFu, c = (st[q] >> 8) & 1u;
            const uint32_t bh = h ? (~h & full) : 0u;                          // nobody holds the row: all zero
            n_held += h != 0u;
            n_disp += bh != 0u;
            n_conf += c;
            if ((bh | c) && i < first) first = i;
            vis_s += lv_spread8(st[q] >> 16);
            hold_s += lv_spread8(h);
            sole_s += lv_spread8((h & (h - 1u)) == 0u ? h : 0u);
            const uint64_t seg = base + (uint64_t)q * kTmThreads + (uint64_t)w * 64;
            if (behind) gd_store_bytes(behind, seg, n, lane, bh);
            if (hold) gd_store_bytes(hold, seg, n, lane, h);
            if (conflict) lv_store_flags(conflict, seg, n, lane, c != 0u);
        }
        if (++pending == kGdFlush) {                 // (the same tile count in every thread of the workgroup)
            gd_flush(vis_s, &s_cnt[w][3], lane);
            gd_flush(hold_s, &s_cnt[w][3 + kGdMax], lane);
            gd_flush(sole_s, &s_cnt[w][3 + 2 * kGdMax], lane);
            pending = 0;
        }
    }
    gd_flush(vis_s, &s_cnt[w][3], lane);
    gd_flush(hold_s, &s_cnt[w][3 + kGdMax], lane);
    gd_flush(sole_s, &s_cnt[w][3 + 2 * kGdMax], lane);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        n_held += __shfl_xor(n_held, off, 64);
        n_disp += __shfl_xor(n_disp, off, 64);
        n_conf += __shfl_xor(n_conf, off, 64);
        const unsigned long long f = __shfl_xor(first, off, 64);
        first = f < first ? f : first;
    }
    if (lane == 0) {
        s_cnt[w][0] = n_held; s_cnt[w][1] = n_disp; s_cnt[w][2] = n_conf;
        s_first[w] = first;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    const auto total = [&](int k) {                  // (LDS, indexed: no per-thread array)
        return (unsigned long long)s_cnt[0][k] + s_cnt[1][k] + s_cnt[2][k] + s_cnt[3][k];
    };
    const unsigned long long held = total(0);
    for (int k = 0; k < 3; ++k) {
        const unsigned long long t = total(k);
        if (t) atomicAdd(&words[k], t);
    }
    for (int ww = 0; ww < 4; ++ww) first = s_first[ww] < first ? s_first[ww] : first;
    if (first != ~0ull) atomicMin(&words[3], first);
    for (int j = 0; j < (int)n_ctx; ++j) {
        const unsigned long long v = total(3 + j), hd = total(3 + kGdMax + j), so = total(3 + 2 * kGdMax + j);
        if (v) atomicAdd(&words[4 + j], v);
        if (held - hd) atomicAdd(&words[4 + kGdMax + j], held - hd);           // behind: held, but not by j
        if (so) atomicAdd(&words[4 + 2 * kGdMax + j], so);
    }
}
