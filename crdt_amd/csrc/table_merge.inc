// table_merge.inc — crdt_merge_table: dst.merge(src.recordMap(modifiedSince)) between two tables of one
// device and one id space, without an export (crdt.dart:77-94 on the changeset of crdt.dart:157-160),
// crdt_sync_tables, the two-way exchange on one read of both tables, crdt_fanin_tables, up to eight
// sources merged into one table on one read of it, and crdt_fanout_tables, one source merged into up to
// eight tables on one read of it (all further down).
// Included from crdt_merge.hip inside its anonymous namespace, beside the export kernels.
//
// Key k lives in row k of BOTH tables, so the merge is an element-wise pass over two aligned arrays:
// nothing is compacted, gathered, partitioned or sorted, and the only scratch is one count per tile and
// one bit per row (n_rows / 8 bytes), whatever the selection.
// Tiles are kTmTile rows; a thread takes rows tm_row(base, q) = base + q * 256 + tid, q < kTmItems, as the
// export does (a wave-instruction covers 64 consecutive rows, all of a thread's loads are in flight
// together, rows past n are clamped to row n - 1 and masked).
//   k_tm_clock  20 B of every src row ({lt, rank, mod}: every line of the table once) -> each tile's
//               selected rows into sel[tile], one bit per row into mask[] (the ballot of each
//               wave-instruction's 64 consecutive rows), and over the whole table words[0] = max ord64(lt)
//               of the selected rows, [1] = 1 + the largest selected id, [2] = 1 when a selected row may
//               raise in recv() (recv_candidate, k_scan's rule: lt > C_0 and rank == local or millis - wall
//               > 60000; hlc.dart:85-94), [3] = the selected rows.  A capped grid strides over the tiles; a
//               thread keeps the four in a TmClock, whose publish() makes the atomics on words[], at most
//               four per workgroup (same-address atomics serialise).
//   k_tm_apply  one workgroup per tile; a tile that selected nothing returns before any row load.  Else
//               a thread takes its rows' bits from mask[] and loads, for its SELECTED rows, the src row
//               (both halves) and dst's decision half; its other lanes read row 0 instead (no branch, one
//               hot line), so all of a thread's loads are in flight before the first is used.  (A dense
//               tile reads every line of both tables; a sparse one only the lines of the selected rows:
//               loading every row of every tile that holds a selected one measured 1.89 ms against the
//               composition's 1.45 ms at 1 % selected, where every tile holds ~20.)
//               A selected row wins iff dst's row is invisible or (lt, rank)_src > (lt, rank)_dst
//               strictly (hlc_gt, k_apply's rule: equal keeps local, crdt.dart:83-90), and a winner is
//               stored {lt, rank, val, mod = stamp}.  Every row belongs to one thread.  n_present / n_won:
//               one pair of atomics per workgroup into the striped counter slots (tm_add_counts).  flags
//               (optional, by ROW id): every row of [0, n) gets its byte from the thread that owns it, zeros
//               included (a tile that selected nothing writes its zeros, tm_zero_flags, and returns).
//   k_tm_flags_scatter  the fallback (the export + crdt_merge composition): its per-record win flags
//               carried to their row ids.
constexpr int kTmThreads = 256;
constexpr int kTmItems = 8;
constexpr int kTmTile = kTmThreads * kTmItems;   // 2048 rows: 48 KB of 24-B src rows + 32 KB of dst halves
constexpr int kTmMaskWords = kTmTile / 64;       // 64-bit selection words per tile: word q * 4 + wave
constexpr unsigned kTmClockGrid = 2048;          // 256 CUs x 8 resident workgroups
constexpr int kTmWords = 4;                      // clock words of one merge direction
static_assert(kTmThreads == 4 * 64, "the epilogues hand four waves' partial results to thread 0");

// ---- what the k_tm_* and k_sy_* kernels share
__device__ inline int64_t hot_lt(uint4 h) { return (int64_t)(((uint64_t)h.y << 32) | h.x); }
__device__ inline int64_t hot_mod(uint4 h, uint32_t lo) {   // lo: the low word of mod, first of the cold half
    return (int64_t)(((uint64_t)h.w << 32) | lo);
}
__device__ inline bool hlc_gt(uint4 p, uint4 q) {   // (lt, rank) of p strictly above q's
    const int64_t pl = hot_lt(p), ql = hot_lt(q);
    return pl > ql || (pl == ql && p.z > q.z);
}
// A row that may raise in Hlc.recv (hlc.dart:85-94) on a replica of this canonical and rank: it is above
// the canonical, and of the replica's own node or drifted past the wall.
__device__ inline bool recv_candidate(uint4 h, int64_t canonical, uint32_t local_rank, int64_t wall) {
    const int64_t lt = hot_lt(h);
    return lt > canonical && (h.z == local_rank || wsub(lt >> kShift, wall) > kMaxDrift);
}
__device__ inline uint64_t tm_row(uint64_t base, int q) { return base + (uint64_t)q * kTmThreads + threadIdx.x; }

// The zero flags of a tile that selected nothing (every thread of the workgroup; flags may be null).
__device__ inline void tm_zero_flags(uint8_t* __restrict__ flags, uint64_t base, uint64_t n) {
    if (!flags) return;
    uint8_t* f = flags + base;                   // the tile's kTmTile bytes: 8 per thread where whole and aligned
    if (base + kTmTile <= n && (reinterpret_cast<uintptr_t>(f) & 7u) == 0) {
        static_assert(kTmItems == 8, "one 8-B store per thread zeroes the tile's flags");
        reinterpret_cast<unsigned long long*>(f)[threadIdx.x] = 0ull;
    } else {
#pragma unroll
        for (int q = 0; q < kTmItems; ++q) {
            const uint64_t i = tm_row(base, q);
            if (i < n) flags[i] = 0;
        }
    }
}

// One merge direction's clock words, as a thread gathers them over its selected rows.
struct TmClockLds { unsigned long long mx[4], id[4]; uint32_t cnt[4], cand[4]; };   // per wave
struct TmClock {
    unsigned long long mx = 0, id = 0;           // max ord64(lt), max row id + 1
    uint32_t cnt = 0;
    unsigned long long cand = 0;                 // the wave's lanes that met a candidate: wave-uniform, no VGPR
    // Row i (hot half h), selected or not (sel) into a replica of this canonical and rank.  Every lane of
    // the wave calls it, for the ballot.
    __device__ void add(bool sel, uint4 h, uint64_t i, int64_t canonical, uint32_t local_rank, int64_t wall) {
        cnt += sel;
        bool c = false;
        if (sel) {                               // (a wave with no selected row skips all of it)
            const unsigned long long o = ord64(hot_lt(h));
            mx = o > mx ? o : mx;
            id = i + 1 > id ? i + 1 : id;
            c = recv_candidate(h, canonical, local_rank, wall);
        }
        cand |= __ballot(c);
    }
    // The workgroup's rows into words[0..3]: wave reduction, LDS hand-off to thread 0, at most four
    // atomics, none where nothing was selected.  Every thread calls it (it has a barrier); s is its own.
    __device__ void publish(TmClockLds& s, unsigned long long* __restrict__ words) {
        const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const unsigned long long a = __shfl_xor(mx, off, 64), b = __shfl_xor(id, off, 64);
            mx = a > mx ? a : mx;
            id = b > id ? b : id;
            cnt += __shfl_xor(cnt, off, 64);
        }
        if (lane == 0) { s.mx[w] = mx; s.id[w] = id; s.cnt[w] = cnt; s.cand[w] = cand ? 1u : 0u; }
        __syncthreads();
        if (threadIdx.x != 0) return;
        unsigned long long total = 0;
        uint32_t cd = 0;
        for (int ww = 0; ww < 4; ++ww) {
            mx = s.mx[ww] > mx ? s.mx[ww] : mx;
            id = s.id[ww] > id ? s.id[ww] : id;
            total += s.cnt[ww];
            cd |= s.cand[ww];
        }
        if (!total) return;
        atomicMax(&words[0], mx);
        atomicMax(&words[1], id);
        if (cd) atomicMax(&words[2], 1ull);
        atomicAdd(&words[3], total);
    }
};

// The workgroup's sums of these per-thread counts onto *present / *won (Misc's striped present[slot] /
// won[slot] in the second form): one pair of atomics.
// Every thread calls it (it has a barrier); s is its own.
__device__ inline void tm_add_counts(int npres, int nwon, int (&s)[2][4], unsigned long long* __restrict__ present,
                                     unsigned long long* __restrict__ won) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        npres += __shfl_xor(npres, off, 64);
        nwon += __shfl_xor(nwon, off, 64);
    }
    if (lane == 0) { s[0][w] = npres; s[1][w] = nwon; }
    __syncthreads();
    if (threadIdx.x != 0) return;
    npres = s[0][0] + s[0][1] + s[0][2] + s[0][3];
    nwon = s[1][0] + s[1][1] + s[1][2] + s[1][3];
    if (npres) atomicAdd(present, (unsigned long long)npres);
    if (nwon) atomicAdd(won, (unsigned long long)nwon);
}
__device__ inline void tm_add_counts(int npres, int nwon, int (&s)[2][4], Misc* __restrict__ misc, int slot) {
    tm_add_counts(npres, nwon, s, &misc->present[slot], &misc->won[slot]);
}

__global__ __launch_bounds__(kTmThreads) void k_tm_clock(Table src, uint64_t n, int64_t since, uint32_t nb,
                                                         int64_t c0, int64_t wall, uint32_t local_rank,
                                                         uint32_t* __restrict__ sel,
                                                         unsigned long long* __restrict__ mask,
                                                         unsigned long long* __restrict__ words)
{
    __shared__ uint32_t s_cnt[2][4];             // per wave: selected rows; one buffer per tile parity
    __shared__ TmClockLds s_clock;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    TmClock clock;
    uint32_t par = 0;
    for (uint32_t tile = blockIdx.x; tile < nb; tile += gridDim.x, par ^= 1u) {
        const uint64_t base = (uint64_t)tile * kTmTile;
        uint4 h[kTmItems];
        uint32_t ml[kTmItems];
#pragma unroll
        for (int q = 0; q < kTmItems; ++q) {
            const uint64_t i = tm_row(base, q);
            const uint64_t ic = i < n ? i : n - 1;
            h[q] = load_hot(src, ic);
            ml[q] = *reinterpret_cast<const uint32_t*>(row_ptr(src, ic) + 16);
        }
        uint32_t cnt = 0;                        // (wave-uniform: summed from the ballots)
#pragma unroll
        for (int q = 0; q < kTmItems; ++q) {
            const uint64_t i = tm_row(base, q);
            const bool keep = i < n && !(hot_mod(h[q], ml[q]) < since);
            const unsigned long long b = __ballot(keep);
            if (lane == 0) mask[(uint64_t)tile * kTmMaskWords + q * 4 + w] = b;
            cnt += (uint32_t)__popcll(b);
            clock.add(keep, h[q], i, c0, local_rank, wall);
        }
        if (lane == 0) s_cnt[par][w] = cnt;
        __syncthreads();                         // (the next tile writes the other buffer)
        if (threadIdx.x == 0) sel[tile] = s_cnt[par][0] + s_cnt[par][1] + s_cnt[par][2] + s_cnt[par][3];
    }
    clock.publish(s_clock, words);
}

__global__ __launch_bounds__(kTmThreads) void k_tm_apply(Table src, Table dst, uint64_t n, uint64_t dcap,
                                                         const uint32_t* __restrict__ sel,
                                                         const unsigned long long* __restrict__ mask,
                                                         int64_t stamp, Misc* __restrict__ misc,
                                                         uint8_t* __restrict__ flags)
{
    __shared__ int s_pw[2][4];
    const uint64_t base = (uint64_t)blockIdx.x * kTmTile;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (sel[blockIdx.x] == 0) {                  // the whole workgroup: nothing selected in this tile
        tm_zero_flags(flags, base, n);
        return;
    }
    uint4 h[kTmItems], d[kTmItems];
    uint2 x[kTmItems];
    unsigned long long mb[kTmItems];
#pragma unroll
    for (int q = 0; q < kTmItems; ++q) mb[q] = mask[(uint64_t)blockIdx.x * kTmMaskWords + q * 4 + w];
    uint32_t keep = 0;
#pragma unroll
    for (int q = 0; q < kTmItems; ++q) {
        const uint64_t i = tm_row(base, q);
        // (the clock pass set bits of rows < n only; the host sent a call with a selected id >= dcap elsewhere)
        const bool k = ((mb[q] >> lane) & 1ull) && i < n && i < dcap;
        keep |= (uint32_t)k << q;
        const uint64_t ic = k ? i : 0;           // an unselected lane reads row 0 (one hot line for all of them):
        h[q] = load_hot(src, ic);                // always a valid address and no branch, so the 24 loads of a
        x[q] = load_cold(src, ic);               // thread issue back to back
        d[q] = load_hot(dst, ic);
    }
    const uint32_t st_hi = (uint32_t)((uint64_t)stamp >> 32), st_lo = (uint32_t)stamp;
    int npres = 0, nwon = 0;
#pragma unroll
    for (int q = 0; q < kTmItems; ++q) {
        const uint64_t i = tm_row(base, q);
        const bool k = (keep >> q) & 1u;
        const bool present = (int32_t)d[q].w >= 0;
        const bool win = k && (!present || hlc_gt(h[q], d[q]));
        npres += k && present;
        nwon += win;
        if (win) store_hc(dst, i, make_uint4(h[q].x, h[q].y, h[q].z, st_hi), make_uint2(st_lo, x[q].y));
        if (flags && i < n) flags[i] = win ? 1 : 0;
    }
    tm_add_counts(npres, nwon, s_pw, misc, blockIdx.x & (kCounterSlots - 1));
}

__global__ __launch_bounds__(256) void k_tm_flags_scatter(const uint32_t* __restrict__ key,
                                                          const uint8_t* __restrict__ win, uint64_t n,
                                                          uint64_t n_rows, uint8_t* __restrict__ row_flags)
{
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        if (!win[i]) continue;
        const uint32_t k = key[i];
        if (k < n_rows) row_flags[k] = 1;
    }
}

// ---- crdt_sync_tables: the two-replica exchange a.merge(b.recordMap(since_b)); b.merge(a.recordMap(since_a))
// on ONE read of the two rows (DESIGN §6e).  The win decision of crdt.dart:83-84 reads no canonical clock,
// so step 1's winners (winA) are known in the clock pass already, and with them the changeset step 2 will
// select from a as step 1 leaves it: the winners (stamped mod = R_a >= since_a, the host checks that) and
// the rows of a that since_a selects and step 1 does not replace.  Same tiles and thread shape as k_tm_*,
// and the same pieces: one TmClock and one tm_add_counts per direction, tm_zero_flags per side.
//   k_sy_clock  {lt, rank, mod} of every row of BOTH tables -> sel[tile] = rows selected in either
//               direction, two ballots per wave-instruction into mask[] (word 2 * (q * 4 + wave): selB =
//               !(b.mod < since_b); + 1: selA0 = !(a.mod < since_a)), and eight words:
//                 [0..3] direction 1 as k_tm_clock's (max ord64(lt) over selB, 1 + its largest id, the
//                        candidate bit against C_a / a's rank / the wall, its count);
//                 [4..7] direction 2 over {winA: b's row} U {selA0 && !winA: a's row}, against C_b and b's
//                        rank.  A row of b that wins into a comes back to b and may raise there (b's own
//                        rank above C_b after a raw put): its (lt, rank) are b's, so the bit covers it.
//               At most eight atomics per workgroup.
//   k_sy_apply  one workgroup per tile; a tile with no selection writes its zero flags (both arrays) and
//               returns.  Else, for the rows with either bit set (the others read row 0), both rows in
//               full; a' = winA ? {b's lt, rank, val; mod = R_a} : a in registers, selA = winA || selA0,
//               winB = selA && (b invisible || hlc(a') > hlc(b)) — the plain rule on a' — and the winners
//               stored on each side (a row can be stored on BOTH: b's invisible row, selected by a negative
//               since_b, wins into a and comes back visible).  Every row belongs to one thread, so one
//               pass writes both tables.  Counts: direction 1 into slots [0, 32) of Misc's striped
//               counters, direction 2 into [32, 64).
//               The rows are taken kSyBatch items at a time (12 VGPRs of loads per row against
//               k_tm_apply's 10), see DESIGN §6e for the register counts.
constexpr int kSyBatch = 4;                      // rows of a thread in flight together in k_sy_apply
constexpr unsigned kSyClockGrid = 2048;          // as kTmClockGrid
constexpr int kSyWords = 2 * kTmWords;
static_assert(kTmItems % kSyBatch == 0, "k_sy_apply takes a thread's rows in whole batches");
static_assert(kCounterSlots == 64, "k_sy_apply halves the striped counter slots between the directions");

__global__ __launch_bounds__(kTmThreads) void k_sy_clock(Table ta, Table tb, uint64_t n, int64_t since_a,
                                                         int64_t since_b, uint32_t nb, int64_t ca, int64_t cb,
                                                         int64_t wall, uint32_t rank_a, uint32_t rank_b,
                                                         uint32_t* __restrict__ sel,
                                                         unsigned long long* __restrict__ mask,
                                                         unsigned long long* __restrict__ words)
{
    __shared__ uint32_t s_cnt[2][4];             // per wave: rows selected either way; one buffer per tile parity
    __shared__ TmClockLds s_clock[2];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    TmClock clock1, clock2;                      // b's rows into a; a's rows, as step 1 leaves them, into b
    uint32_t par = 0;
    for (uint32_t tile = blockIdx.x; tile < nb; tile += gridDim.x, par ^= 1u) {
        const uint64_t base = (uint64_t)tile * kTmTile;
        uint32_t cnt = 0;                        // (wave-uniform: summed from the ballots)
#pragma unroll 1
        for (int g = 0; g < kTmItems; g += kSyBatch) {
            uint4 ha[kSyBatch], hb[kSyBatch];
            uint32_t la[kSyBatch], lb[kSyBatch];
#pragma unroll
            for (int q = 0; q < kSyBatch; ++q) {
                const uint64_t i = tm_row(base, g + q);
                const uint64_t ic = i < n ? i : n - 1;
                hb[q] = load_hot(tb, ic);
                lb[q] = *reinterpret_cast<const uint32_t*>(row_ptr(tb, ic) + 16);
                ha[q] = load_hot(ta, ic);
                la[q] = *reinterpret_cast<const uint32_t*>(row_ptr(ta, ic) + 16);
            }
#pragma unroll
            for (int q = 0; q < kSyBatch; ++q) {
                const uint64_t i = tm_row(base, g + q);
                // (both mods before the tests: inside the && the compiler kept 2 more VGPRs)
                const int64_t mod_b = hot_mod(hb[q], lb[q]), mod_a = hot_mod(ha[q], la[q]);
                const bool selB = i < n && !(mod_b < since_b);
                const bool selA0 = i < n && !(mod_a < since_a);
                const unsigned long long bb = __ballot(selB), ba = __ballot(selA0);
                if (lane == 0) {
                    unsigned long long* m = mask + ((uint64_t)tile * kTmMaskWords + (g + q) * 4 + w) * 2;
                    m[0] = bb;
                    m[1] = ba;
                }
                cnt += (uint32_t)__popcll(bb | ba);
                const bool winA = selB && ((int32_t)ha[q].w < 0 || hlc_gt(hb[q], ha[q]));
                clock1.add(selB, hb[q], i, ca, rank_a, wall);
                clock2.add(winA || selA0, winA ? hb[q] : ha[q], i, cb, rank_b, wall);
            }
        }
        if (lane == 0) s_cnt[par][w] = cnt;
        __syncthreads();                         // (the next tile writes the other buffer)
        if (threadIdx.x == 0) sel[tile] = s_cnt[par][0] + s_cnt[par][1] + s_cnt[par][2] + s_cnt[par][3];
    }
    clock1.publish(s_clock[0], words);
    clock2.publish(s_clock[1], words + kTmWords);
}

__global__ __launch_bounds__(kTmThreads) void k_sy_apply(Table ta, Table tb, uint64_t n,
                                                         const uint32_t* __restrict__ sel,
                                                         const unsigned long long* __restrict__ mask,
                                                         int64_t stamp_a, int64_t stamp_b,
                                                         Misc* __restrict__ misc, uint8_t* __restrict__ flags_a,
                                                         uint8_t* __restrict__ flags_b)
{
    __shared__ int s_pw[2][2][4];
    const uint64_t base = (uint64_t)blockIdx.x * kTmTile;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (sel[blockIdx.x] == 0) {                  // the whole workgroup: nothing selected in this tile, either way
        tm_zero_flags(flags_a, base, n);
        tm_zero_flags(flags_b, base, n);
        return;
    }
    const uint32_t sa_hi = (uint32_t)((uint64_t)stamp_a >> 32), sa_lo = (uint32_t)stamp_a;
    const uint32_t sb_hi = (uint32_t)((uint64_t)stamp_b >> 32), sb_lo = (uint32_t)stamp_b;
    int np1 = 0, nw1 = 0, np2 = 0, nw2 = 0;
#pragma unroll 1
    for (int g = 0; g < kTmItems; g += kSyBatch) {
        uint4 ha[kSyBatch], hb[kSyBatch];
        uint2 xa[kSyBatch], xb[kSyBatch];
        uint32_t kb = 0, ka = 0;
#pragma unroll
        for (int q = 0; q < kSyBatch; ++q) {
            const uint64_t i = tm_row(base, g + q);
            const unsigned long long* m = mask + ((uint64_t)blockIdx.x * kTmMaskWords + (g + q) * 4 + w) * 2;
            // (the clock pass set bits of rows < n only, and n is within both capacities)
            const bool b1 = ((m[0] >> lane) & 1ull) && i < n, a1 = ((m[1] >> lane) & 1ull) && i < n;
            kb |= (uint32_t)b1 << q;
            ka |= (uint32_t)a1 << q;
            const uint64_t ic = (b1 || a1) ? i : 0;   // a lane selected neither way reads row 0 (one hot line)
            hb[q] = load_hot(tb, ic);
            xb[q] = load_cold(tb, ic);
            ha[q] = load_hot(ta, ic);
            xa[q] = load_cold(ta, ic);
        }
#pragma unroll
        for (int q = 0; q < kSyBatch; ++q) {
            const uint64_t i = tm_row(base, g + q);
            const bool selB = (kb >> q) & 1u, selA0 = (ka >> q) & 1u;
            const bool pres_a = (int32_t)ha[q].w >= 0, pres_b = (int32_t)hb[q].w >= 0;
            const bool winA = selB && (!pres_a || hlc_gt(hb[q], ha[q]));
            // a as step 1 leaves it: step 2 selects a winner by its new mod = R_a (>= since_a, host-checked)
            const bool selA = winA || selA0;
            const bool winB = selA && (!pres_b || (!winA && hlc_gt(ha[q], hb[q])));
            np1 += selB && pres_a;
            nw1 += winA;
            np2 += selA && pres_b;
            nw2 += winB;
            if (winA) store_hc(ta, i, make_uint4(hb[q].x, hb[q].y, hb[q].z, sa_hi), make_uint2(sa_lo, xb[q].y));
            if (winB) {
                const uint4 h = winA ? hb[q] : ha[q];
                store_hc(tb, i, make_uint4(h.x, h.y, h.z, sb_hi), make_uint2(sb_lo, winA ? xb[q].y : xa[q].y));
            }
            if (i < n) {
                if (flags_a) flags_a[i] = winA ? 1 : 0;
                if (flags_b) flags_b[i] = winB ? 1 : 0;
            }
        }
    }
    const int slot = blockIdx.x & (kCounterSlots / 2 - 1);
    tm_add_counts(np1, nw1, s_pw[0], misc, slot);
    tm_add_counts(np2, nw2, s_pw[1], misc, kCounterSlots / 2 + slot);
}

// ---- crdt_fanin_tables: the hub, for j < n_src: dst.merge(srcs[j].recordMap(since_j)), n_src <= kFanMax, on
// ONE read of dst's row (DESIGN §6f).  The win decision reads no canonical clock and the call writes no
// source, so every source's selection and clock words are known before anything is stored: k_tm_clock runs
// as it is once per source (source j's counts in sel[j * nb ..], its bits in mask[j * nb * kTmMaskWords ..],
// its words in words[4 j ..], every launch over all nb tiles with the source's own row bound and dst's
// canonical at entry for the candidate bit), the host chains R_j = max(C_{j-1}, max lt of selection j),
// C_j = Hlc.send(R_j), and
//   k_fan_apply one workgroup per tile; a tile no source selected writes its zero mask bytes and returns.
//               Else a thread takes its selection bits of every source that selected in the tile (eight bits
//               a source, kept in one 64-bit word: the loop below issues no dependent mask load), loads dst's
//               decision half for its rows that ANY source selected (the others read row 0) and keeps the
//               running row {lt, rank, mod, val} in registers.  The sources follow
//               in call order, a runtime loop with one source's loads in flight at a time (a source that
//               selected nothing in the tile is skipped): its selected rows' decision half and val, the plain
//               rule on the running row (wins iff that is invisible or hlc_gt(src, running); the visibility
//               of a row stored earlier in the call is the sign of its stamp R_i, as the next
//               crdt_merge_table would read it), and a winner replaces the running {lt, rank, val}, takes
//               mod = R_j and sets bit j of the row's outcome byte.  After the loop a row whose byte is
//               non-zero is stored ONCE; the byte goes to win_mask[row] (optional) in any case.
//               n_present / n_won per source, in words of the call's own (counts[]: source j's present in
//               [128 j, 128 j + 64), its won in the 64 after them, striped by tile as Misc's are: eight slots
//               a source of Misc's 64 would put 8192 tiles' atomics of a 2^27-row call on one address).
constexpr int kFanMax = 8;                       // CRDT_FANIN_MAX: one outcome bit per source in a byte
constexpr int kFanCounts = kFanMax * 2 * kCounterSlots;   // words of counts[]
static_assert(kFanMax == CRDT_FANIN_MAX, "the header's bound");
static_assert(kFanMax <= 8, "one mask bit per source");
static_assert(kTmItems * 8 <= 64, "a thread's outcome bytes travel in one 64-bit word");

struct FanArgs {                                 // by value: the sources' tables, row bounds and stamps R_j
    Table src[kFanMax];
    uint64_t rows[kFanMax];
    int64_t stamp[kFanMax];
};

__global__ __launch_bounds__(kTmThreads) void k_fan_apply(FanArgs a, uint32_t n_src, Table dst, uint64_t n,
                                                          uint32_t nb, const uint32_t* __restrict__ sel,
                                                          const unsigned long long* __restrict__ mask,
                                                          unsigned long long* __restrict__ counts,
                                                          uint8_t* __restrict__ flags)
{
    __shared__ int s_pw[kFanMax][2][4];
    const uint32_t tile = blockIdx.x;
    const uint64_t base = (uint64_t)tile * kTmTile;
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // (wave-uniform: the mask words load as scalars)
    // the sources that selected in this tile (the counts load together), then this thread's selection bits of
    // each of them, kept for the loop below: bit 8 j + q = source j selected row q
    uint32_t active = 0;
#pragma unroll
    for (int j = 0; j < kFanMax; ++j) {
        const uint32_t cnt = sel[(uint64_t)((uint32_t)j < n_src ? j : 0) * nb + tile];   // (always inside sel[])
        active |= (uint32_t)((uint32_t)j < n_src && cnt != 0) << j;
    }
    if (active == 0) {                           // the whole workgroup: no source selected in this tile
        tm_zero_flags(flags, base, n);
        return;
    }
    unsigned long long bits = 0;
    for (uint32_t j = 0; j < n_src; ++j) {
        if (!((active >> j) & 1u)) continue;     // (its words may never have been written)
        const unsigned long long* m = mask + ((uint64_t)j * nb + tile) * kTmMaskWords;
        uint32_t b = 0;
#pragma unroll
        for (int q = 0; q < kTmItems; ++q) b |= (uint32_t)((m[q * 4 + w] >> lane) & 1ull) << q;
        bits |= (unsigned long long)b << (8 * j);
    }
    uint32_t any = (uint32_t)bits | (uint32_t)(bits >> 32);   // the rows any source selected
    any |= any >> 16;
    any |= any >> 8;
    uint4 r[kTmItems];                           // the running row: {lt, rank, mod_hi}
    uint32_t rl[kTmItems], rv[kTmItems];         // its mod_lo and val (of a winner; a row that never wins is not stored)
#pragma unroll
    for (int q = 0; q < kTmItems; ++q) {
        // (the host sent a call with a selected id >= dst's capacity elsewhere; an unselected lane reads row 0)
        r[q] = load_hot(dst, (any >> q) & 1u ? tm_row(base, q) : 0);
        rl[q] = rv[q] = 0;
    }
    unsigned long long won = 0;                  // byte q: the outcome byte of row q
#pragma unroll 1
    for (uint32_t j = 0; j < n_src; ++j) {
        if (!((active >> j) & 1u)) continue;     // (the whole workgroup)
        const Table src = a.src[j];
        const uint64_t nj = a.rows[j];
        const uint32_t mine = (uint32_t)(bits >> (8 * j));
        uint4 h[kTmItems];
        uint32_t v[kTmItems];
        uint32_t keep = 0;
#pragma unroll
        for (int q = 0; q < kTmItems; ++q) {
            const uint64_t i = tm_row(base, q);
            const bool k = ((mine >> q) & 1u) && i < nj;       // (the clock pass set bits of rows < nj only)
            keep |= (uint32_t)k << q;
            const uint64_t ic = k ? i : 0;
            h[q] = load_hot(src, ic);
            v[q] = *reinterpret_cast<const uint32_t*>(row_ptr(src, ic) + 20);
        }
        const uint32_t st_hi = (uint32_t)((uint64_t)a.stamp[j] >> 32), st_lo = (uint32_t)a.stamp[j];
        int npres = 0, nwon = 0;
#pragma unroll
        for (int q = 0; q < kTmItems; ++q) {
            const bool k = (keep >> q) & 1u;
            const bool present = (int32_t)r[q].w >= 0;
            const bool win = k && (!present || hlc_gt(h[q], r[q]));
            npres += k && present;
            nwon += win;
            if (win) {
                r[q] = make_uint4(h[q].x, h[q].y, h[q].z, st_hi);
                rl[q] = st_lo;
                rv[q] = v[q];
            }
            won |= (unsigned long long)win << (q * 8 + j);
        }
        unsigned long long* c = counts + (2 * j * kCounterSlots + (tile & (kCounterSlots - 1)));
        tm_add_counts(npres, nwon, s_pw[j], c, c + kCounterSlots);
    }
#pragma unroll
    for (int q = 0; q < kTmItems; ++q) {
        const uint64_t i = tm_row(base, q);
        const uint32_t b = (uint32_t)(won >> (q * 8)) & 0xFFu;
        if (b) store_hc(dst, i, r[q], make_uint2(rl[q], rv[q]));
        if (flags && i < n) flags[i] = (uint8_t)b;
    }
}

// ---- crdt_fanout_tables: the hub's outbound half, for j < n_dst: dsts[j].merge(src.recordMap(since_j)),
// n_dst <= kFoMax, on ONE read of src (DESIGN §6g).  The win decision reads no canonical clock, src is never
// written and the destinations are independent, so the n_dst clock passes of the composition are the same
// read of src done n_dst times, and so are its apply passes' reads of src's selected rows.  Scratch in
// crdt_fanin_tables' layout with j the destination: sel[j * nb + tile], mask[(j * nb + tile) * kTmMaskWords
// ..], words[4 j ..], counts[128 j ..].
//   k_fo_clock  {lt, rank, mod} of every row of src below the largest of the destinations' row bounds, each
//               line once whatever n_dst is; from the loaded rows, per destination j (a runtime loop, its
//               arguments held one destination a lane and read with v_readlane): the selection ballot
//               !(mod < since_j) of its rows below ITS bound into its mask words, its tile count, and its
//               clock words (the candidate bit against destination j's canonical and rank).  A wave's count
//               and largest id come from the ballots; a wave that selected for j folds them, its candidate
//               bit and each thread's max ord64(lt) into LDS (eight TmClocks in registers, the loop unrolled,
//               spilled SGPRs).  At the end each destination's LDS state goes through one TmClock::publish:
//               at most four atomics per destination per workgroup.
//   k_fo_apply  one workgroup per tile; a tile that no destination selected writes its zero mask bytes and
//               returns.  Else a thread takes its selection bits of every destination that selected in the
//               tile (one 64-bit word, as k_fan_apply), loads src's row in full ONCE for its rows that ANY
//               destination selected (the others read row 0) and keeps them in registers.  The destinations
//               follow in call order, a runtime loop with one destination's loads in flight at a time (one
//               that selected nothing in the tile is skipped): the decision half of its selected rows, the
//               plain rule (src wins iff the destination's row is invisible or hlc_gt(src, dst)), the winners
//               stored {lt, rank, val, mod = R_j} with that destination's stride, bit j of the row's outcome
//               byte, n_present / n_won into counts[] (as k_fan_apply's).  The byte goes to win_mask[row]
//               once, after the loop.  Every row belongs to one thread.
constexpr int kFoMax = 8;                        // CRDT_FANOUT_MAX: one outcome bit per destination in a byte
constexpr unsigned kFoClockGrid = 2048;          // as kTmClockGrid
static_assert(kFoMax == CRDT_FANOUT_MAX, "the header's bound");
static_assert(kFoMax <= 8, "one mask bit per destination");
static_assert(kFoMax == kFanMax, "counts[] is crdt_fanin_tables' (kFanCounts words)");

struct FoArgs {                                  // by value: what the two kernels know of each destination
    Table dst[kFoMax];
    uint64_t rows[kFoMax];                       // its row bound: ex_rows(src, n_rows, since_j)
    uint64_t cap[kFoMax];
    int64_t since[kFoMax];
    int64_t canonical[kFoMax];                   // at entry (k_fo_clock's candidate bit)
    int64_t stamp[kFoMax];                       // R_j (k_fo_apply)
    uint32_t rank[kFoMax];
};

__device__ inline unsigned long long fo_lane64(unsigned long long v, uint32_t l) {   // lane l's v (l wave-uniform)
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, (int)l);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), (int)l);
    return ((unsigned long long)hi << 32) | lo;
}

__global__ __launch_bounds__(kTmThreads) void k_fo_clock(FoArgs a, uint32_t n_dst, Table src, uint64_t n,
                                                         uint32_t nb, int64_t wall, uint32_t* __restrict__ sel,
                                                         unsigned long long* __restrict__ mask,
                                                         unsigned long long* __restrict__ words)
{
    __shared__ uint32_t s_cnt[2][kFoMax][4];     // per destination and wave: selected rows; one buffer per tile parity
    __shared__ TmClockLds s_clock[kFoMax];
    __shared__ unsigned long long s_mx[kFoMax][kTmThreads];   // per destination and thread: max ord64(lt) so far
    __shared__ unsigned long long s_id[kFoMax][4];            // per destination and wave: 1 + its largest selected id,
    __shared__ uint32_t s_sum[kFoMax][4], s_cand[kFoMax][4];  // its selected rows, whether it met a candidate
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (uint32_t j = 0; j < n_dst; ++j) {       // (a thread's own slots, and lane 0 its wave's: no barrier)
        s_mx[j][threadIdx.x] = 0;
        if (lane == 0) { s_id[j][w] = 0; s_sum[j][w] = 0; s_cand[j][w] = 0; }
    }
    // Lane l keeps destination (l & 7)'s arguments; the loop below takes destination j's from lane j
    // (v_readlane: scalar loads of FoArgs inside the tile loop put their latency on every (tile, j) step).
    const int al = lane & (kFoMax - 1);
    const unsigned long long v_since = (unsigned long long)a.since[al], v_canon = (unsigned long long)a.canonical[al];
    const unsigned long long v_rows = a.rows[al];
    const uint32_t v_rank = a.rank[al];
    uint32_t par = 0;
    for (uint32_t tile = blockIdx.x; tile < nb; tile += gridDim.x, par ^= 1u) {
        const uint64_t base = (uint64_t)tile * kTmTile;
        uint4 h[kTmItems];
        uint32_t ml[kTmItems];
#pragma unroll
        for (int q = 0; q < kTmItems; ++q) {
            const uint64_t i = tm_row(base, q);
            const uint64_t ic = i < n ? i : n - 1;
            h[q] = load_hot(src, ic);
            ml[q] = *reinterpret_cast<const uint32_t*>(row_ptr(src, ic) + 16);
        }
#pragma unroll 1
        for (uint32_t j = 0; j < n_dst; ++j) {
            const int64_t since = (int64_t)fo_lane64(v_since, j), cj = (int64_t)fo_lane64(v_canon, j);
            const uint64_t nj = fo_lane64(v_rows, j);
            const uint32_t rj = (uint32_t)__builtin_amdgcn_readlane((int)v_rank, (int)j);
            unsigned long long mine = 0;         // lane q < 8: the ballot of wave-instruction q (one store for the eight)
            unsigned long long* m = mask + ((uint64_t)j * nb + tile) * kTmMaskWords;
            uint32_t cnt = 0;                    // (wave-uniform, as top: from the ballots)
            unsigned long long top = 0, mx = 0;  // 1 + the wave's largest selected id; this thread's max ord64(lt)
            bool c = false;
#pragma unroll
            for (int q = 0; q < kTmItems; ++q) {
                const uint64_t i = tm_row(base, q);
                const bool keep = i < nj && !(hot_mod(h[q], ml[q]) < since);
                const unsigned long long b = __ballot(keep);
                mine = lane == q ? b : mine;
                cnt += (uint32_t)__popcll(b);
                // (bit l of b is row base + q * 256 + w * 64 + l; q ascends, so the last assignment is the largest)
                if (b) top = base + (uint64_t)q * kTmThreads + (uint64_t)w * 64 + (64 - __clzll((long long)b));
                if (keep) {
                    const unsigned long long o = ord64(hot_lt(h[q]));
                    mx = o > mx ? o : mx;
                    c |= recv_candidate(h[q], cj, rj, wall);
                }
            }
            if (lane < kTmItems) m[lane * 4 + w] = mine;
            if (lane == 0) s_cnt[par][j][w] = cnt;
            if (cnt) {                           // (the whole wave)
                const unsigned long long old = s_mx[j][threadIdx.x];
                s_mx[j][threadIdx.x] = mx > old ? mx : old;
                const bool cd = __ballot(c) != 0;
                if (lane == 0) {
                    s_id[j][w] = top > s_id[j][w] ? top : s_id[j][w];
                    s_sum[j][w] += cnt;
                    s_cand[j][w] |= cd ? 1u : 0u;
                }
            }
        }
        __syncthreads();                         // (the next tile writes the other buffer)
        if (threadIdx.x < n_dst) {
            const uint32_t* t = s_cnt[par][threadIdx.x];
            sel[(uint64_t)threadIdx.x * nb + tile] = t[0] + t[1] + t[2] + t[3];
        }
    }
#pragma unroll 1
    for (uint32_t j = 0; j < n_dst; ++j) {       // each destination's words through a TmClock: lane 0 carries its wave's
        TmClock clock;
        clock.mx = s_mx[j][threadIdx.x];
        clock.id = lane == 0 ? s_id[j][w] : 0;
        clock.cnt = lane == 0 ? s_sum[j][w] : 0;
        clock.cand = s_cand[j][w];
        clock.publish(s_clock[j], words + j * kTmWords);
    }
}

__global__ __launch_bounds__(kTmThreads) void k_fo_apply(FoArgs a, uint32_t n_dst, Table src, uint64_t n,
                                                         uint32_t nb, const uint32_t* __restrict__ sel,
                                                         const unsigned long long* __restrict__ mask,
                                                         unsigned long long* __restrict__ counts,
                                                         uint8_t* __restrict__ flags)
{
    __shared__ int s_pw[kFoMax][2][4];
    const uint32_t tile = blockIdx.x;
    const uint64_t base = (uint64_t)tile * kTmTile;
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // (wave-uniform: the mask words load as scalars)
    // the destinations that selected in this tile (the counts load together), then this thread's selection bits
    // of each of them, kept for the loop below: bit 8 j + q = destination j selected row q
    uint32_t active = 0;
#pragma unroll
    for (int j = 0; j < kFoMax; ++j) {
        const uint32_t cnt = sel[(uint64_t)((uint32_t)j < n_dst ? j : 0) * nb + tile];   // (always inside sel[])
        active |= (uint32_t)((uint32_t)j < n_dst && cnt != 0) << j;
    }
    if (active == 0) {                           // the whole workgroup: no destination selected in this tile
        tm_zero_flags(flags, base, n);
        return;
    }
    unsigned long long bits = 0;
    for (uint32_t j = 0; j < n_dst; ++j) {
        if (!((active >> j) & 1u)) continue;
        const unsigned long long* m = mask + ((uint64_t)j * nb + tile) * kTmMaskWords;
        uint32_t b = 0;
#pragma unroll
        for (int q = 0; q < kTmItems; ++q) b |= (uint32_t)((m[q * 4 + w] >> lane) & 1ull) << q;
        bits |= (unsigned long long)b << (8 * j);
    }
    uint32_t any = (uint32_t)bits | (uint32_t)(bits >> 32);   // the rows any destination selected
    any |= any >> 16;
    any |= any >> 8;
    uint4 h[kTmItems];                           // src's rows, read once for all destinations
    uint32_t v[kTmItems];
#pragma unroll
    for (int q = 0; q < kTmItems; ++q) {
        // (the clock pass set bits of rows < n only; an unselected lane reads row 0: one hot line)
        const uint64_t ic = (any >> q) & 1u ? tm_row(base, q) : 0;
        h[q] = load_hot(src, ic);
        v[q] = load_cold(src, ic).y;
    }
    unsigned long long won = 0;                  // byte q: the outcome byte of row q
#pragma unroll 1
    for (uint32_t j = 0; j < n_dst; ++j) {
        if (!((active >> j) & 1u)) continue;     // (the whole workgroup)
        const Table dst = a.dst[j];
        const uint64_t nj = a.rows[j], dcap = a.cap[j];
        const uint32_t mine = (uint32_t)(bits >> (8 * j));
        uint4 d[kTmItems];
        uint32_t keep = 0;
#pragma unroll
        for (int q = 0; q < kTmItems; ++q) {
            const uint64_t i = tm_row(base, q);
            // (the clock pass set bits of rows < nj only; the host sent a call with a selected id >= dcap elsewhere)
            const bool k = ((mine >> q) & 1u) && i < nj && i < dcap;
            keep |= (uint32_t)k << q;
            d[q] = load_hot(dst, k ? i : 0);
        }
        const uint32_t st_hi = (uint32_t)((uint64_t)a.stamp[j] >> 32), st_lo = (uint32_t)a.stamp[j];
        int npres = 0, nwon = 0;
#pragma unroll
        for (int q = 0; q < kTmItems; ++q) {
            const bool k = (keep >> q) & 1u;
            const bool present = (int32_t)d[q].w >= 0;
            const bool win = k && (!present || hlc_gt(h[q], d[q]));
            npres += k && present;
            nwon += win;
            if (win) store_hc(dst, tm_row(base, q), make_uint4(h[q].x, h[q].y, h[q].z, st_hi), make_uint2(st_lo, v[q]));
            won |= (unsigned long long)win << (q * 8 + j);
        }
        unsigned long long* c = counts + (2 * j * kCounterSlots + (tile & (kCounterSlots - 1)));
        tm_add_counts(npres, nwon, s_pw[j], c, c + kCounterSlots);
    }
    if (!flags) return;
#pragma unroll
    for (int q = 0; q < kTmItems; ++q) {
        const uint64_t i = tm_row(base, q);
        if (i < n) flags[i] = (uint8_t)(won >> (q * 8));
    }
}

// The composition's mask: step j's row flags into bit j.
__global__ __launch_bounds__(256) void k_fan_or_flags(const uint8_t* __restrict__ step, uint64_t n, uint32_t j,
                                                      uint8_t* __restrict__ win_mask)
{
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
        if (step[i]) win_mask[i] |= (uint8_t)(1u << j);
}
