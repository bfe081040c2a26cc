// table_merge.inc — crdt_merge_table: dst.merge(src.recordMap(modifiedSince)) between two tables of one
// device and one id space, without an export (crdt.dart:77-94 on the changeset of crdt.dart:157-160).
// Included from crdt_merge.hip inside its anonymous namespace, beside the export kernels.
//
// Key k lives in row k of BOTH tables, so the merge is an element-wise pass over two aligned arrays:
// nothing is compacted, gathered, partitioned or sorted, and the only scratch is one count per tile and
// one bit per row (n_rows / 8 bytes), whatever the selection.
// Tiles are kTmTile rows; a thread takes rows base + q * 256 + tid, q < kTmItems, as the export does (a
// wave-instruction covers 64 consecutive rows, all of a thread's loads are in flight together, rows past
// n are clamped to row n - 1 and masked).
//   k_tm_clock  20 B of every src row ({lt, rank, mod}: every line of the table once) -> each tile's
//               selected rows into sel[tile], one bit per row into mask[] (the ballot of each
//               wave-instruction's 64 consecutive rows), and over the whole table words[0] = max ord64(lt)
//               of the selected rows, [1] = 1 + the largest selected id, [2] = 1 when a selected row may
//               raise in recv() (k_scan's rule: lt > C_0 and rank == local or millis - wall > 60000;
//               hlc.dart:85-94), [3] = the selected rows.  A capped grid strides over the tiles; the
//               atomics on words[] are at most four per workgroup (same-address atomics serialise).
//   k_tm_apply  one workgroup per tile; a tile that selected nothing returns before any row load.  Else
//               a thread takes its rows' bits from mask[] and loads, for its SELECTED rows, the src row
//               (both halves) and dst's decision half; its other lanes read row 0 instead (no branch, one
//               hot line), so all of a thread's loads are in flight before the first is used.  (A dense
//               tile reads every line of both tables; a sparse one only the lines of the selected rows:
//               loading every row of every tile that holds a selected one measured 1.89 ms against the
//               composition's 1.45 ms at 1 % selected, where every tile holds ~20.)
//               A selected row wins iff dst's row is invisible or (lt, rank)_src > (lt, rank)_dst
//               strictly (k_apply's rule: equal keeps local, crdt.dart:83-90), and a winner is stored
//               {lt, rank, val, mod = stamp}.  Every row belongs to one thread.  n_present / n_won: one
//               pair of atomics per workgroup into the striped counter slots.  flags (optional, by ROW
//               id): every row of [0, n) gets its byte from the thread that owns it, zeros included (a
//               tile that selected nothing writes its zeros and returns).
//   k_tm_flags_scatter  the fallback (the export + crdt_merge composition): its per-record win flags
//               carried to their row ids.
constexpr int kTmThreads = 256;
constexpr int kTmItems = 8;
constexpr int kTmTile = kTmThreads * kTmItems;   // 2048 rows: 48 KB of 24-B src rows + 32 KB of dst halves
constexpr int kTmMaskWords = kTmTile / 64;       // 64-bit selection words per tile: word q * 4 + wave
constexpr unsigned kTmClockGrid = 2048;          // 256 CUs x 8 resident workgroups

__global__ __launch_bounds__(kTmThreads) void k_tm_clock(Table src, uint64_t n, int64_t since, uint32_t nb,
                                                         int64_t c0, int64_t wall, uint32_t local_rank,
                                                         uint32_t* __restrict__ sel,
                                                         unsigned long long* __restrict__ mask,
                                                         unsigned long long* __restrict__ words)
{
    __shared__ uint32_t s_cnt[2][4];             // per wave: selected rows; one buffer per tile parity
    __shared__ unsigned long long s_mx[4], s_id[4];
    __shared__ uint32_t s_cand[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    unsigned long long mx = 0, mid = 0, total = 0;   // (total: thread 0's)
    bool cand = false;
    uint32_t par = 0;
    for (uint32_t tile = blockIdx.x; tile < nb; tile += gridDim.x, par ^= 1u) {
        const uint64_t base = (uint64_t)tile * kTmTile;
        uint4 h[kTmItems];
        uint32_t ml[kTmItems];
#pragma unroll
        for (int q = 0; q < kTmItems; ++q) {
            const uint64_t i = base + q * kTmThreads + threadIdx.x;
            const uint64_t ic = i < n ? i : n - 1;
            h[q] = load_hot(src, ic);
            ml[q] = *reinterpret_cast<const uint32_t*>(row_ptr(src, ic) + 16);
        }
        uint32_t cnt = 0;                        // (wave-uniform: summed from the ballots)
#pragma unroll
        for (int q = 0; q < kTmItems; ++q) {
            const uint64_t i = base + q * kTmThreads + threadIdx.x;
            const int64_t mod = (int64_t)(((uint64_t)h[q].w << 32) | ml[q]);
            const int64_t lt = (int64_t)(((uint64_t)h[q].y << 32) | h[q].x);
            const bool keep = i < n && !(mod < since);
            const unsigned long long b = __ballot(keep);
            if (lane == 0) mask[(uint64_t)tile * kTmMaskWords + q * 4 + w] = b;
            cnt += (uint32_t)__popcll(b);
            if (keep) {
                const unsigned long long o = ord64(lt);
                mx = o > mx ? o : mx;
                mid = i + 1 > mid ? i + 1 : mid;
                cand |= lt > c0 && (h[q].z == local_rank || wsub(lt >> kShift, wall) > kMaxDrift);
            }
        }
        if (lane == 0) s_cnt[par][w] = cnt;
        __syncthreads();                         // (the next tile writes the other buffer)
        if (threadIdx.x == 0) {
            cnt = s_cnt[par][0] + s_cnt[par][1] + s_cnt[par][2] + s_cnt[par][3];
            sel[tile] = cnt;
            total += cnt;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long a = __shfl_xor(mx, off, 64), b = __shfl_xor(mid, off, 64);
        mx = a > mx ? a : mx;
        mid = b > mid ? b : mid;
    }
    const bool wcand = __any(cand);
    if (lane == 0) { s_mx[w] = mx; s_id[w] = mid; s_cand[w] = wcand ? 1u : 0u; }
    __syncthreads();
    if (threadIdx.x == 0 && total) {
        uint32_t cd = 0;
        for (int ww = 0; ww < 4; ++ww) {
            mx = s_mx[ww] > mx ? s_mx[ww] : mx;
            mid = s_id[ww] > mid ? s_id[ww] : mid;
            cd |= s_cand[ww];
        }
        atomicMax(&words[0], mx);
        atomicMax(&words[1], mid);
        if (cd) atomicMax(&words[2], 1ull);
        atomicAdd(&words[3], total);
    }
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
        if (flags) {
            uint8_t* f = flags + base;           // the tile's kTmTile bytes: 8 per thread where whole and aligned
            if (base + kTmTile <= n && (reinterpret_cast<uintptr_t>(f) & 7u) == 0) {
                static_assert(kTmItems == 8, "one 8-B store per thread zeroes the tile's flags");
                reinterpret_cast<unsigned long long*>(f)[threadIdx.x] = 0ull;
            } else {
#pragma unroll
                for (int q = 0; q < kTmItems; ++q) {
                    const uint64_t i = base + q * kTmThreads + threadIdx.x;
                    if (i < n) flags[i] = 0;
                }
            }
        }
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
        const uint64_t i = base + q * kTmThreads + threadIdx.x;
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
        const uint64_t i = base + q * kTmThreads + threadIdx.x;
        const int64_t lt = (int64_t)(((uint64_t)h[q].y << 32) | h[q].x);
        const int64_t dlt = (int64_t)(((uint64_t)d[q].y << 32) | d[q].x);
        const bool k = (keep >> q) & 1u;
        const bool present = (int32_t)d[q].w >= 0;
        const bool win = k && (!present || lt > dlt || (lt == dlt && h[q].z > d[q].z));
        npres += k && present;
        nwon += win;
        if (win) store_hc(dst, i, make_uint4(h[q].x, h[q].y, h[q].z, st_hi), make_uint2(st_lo, x[q].y));
        if (flags && i < n) flags[i] = win ? 1 : 0;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        npres += __shfl_xor(npres, off, 64);
        nwon += __shfl_xor(nwon, off, 64);
    }
    if (lane == 0) { s_pw[0][w] = npres; s_pw[1][w] = nwon; }
    __syncthreads();
    if (threadIdx.x == 0) {
        npres = s_pw[0][0] + s_pw[0][1] + s_pw[0][2] + s_pw[0][3];
        nwon = s_pw[1][0] + s_pw[1][1] + s_pw[1][2] + s_pw[1][3];
        const int slot = blockIdx.x & (kCounterSlots - 1);
        if (npres) atomicAdd(&misc->present[slot], (unsigned long long)npres);
        if (nwon) atomicAdd(&misc->won[slot], (unsigned long long)nwon);
    }
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
// the rows of a that since_a selects and step 1 does not replace.  Same tiles and thread shape as k_tm_*.
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
constexpr int kSyWords = 8;
static_assert(kTmItems % kSyBatch == 0, "k_sy_apply takes a thread's rows in whole batches");
static_assert(kCounterSlots == 64, "k_sy_apply halves the striped counter slots between the directions");

__device__ inline bool hlc_gt(uint4 p, uint4 q) {   // (lt, rank) of p strictly above q's
    const int64_t pl = (int64_t)(((uint64_t)p.y << 32) | p.x), ql = (int64_t)(((uint64_t)q.y << 32) | q.x);
    return pl > ql || (pl == ql && p.z > q.z);
}

__global__ __launch_bounds__(kTmThreads) void k_sy_clock(Table ta, Table tb, uint64_t n, int64_t since_a,
                                                         int64_t since_b, uint32_t nb, int64_t ca, int64_t cb,
                                                         int64_t wall, uint32_t rank_a, uint32_t rank_b,
                                                         uint32_t* __restrict__ sel,
                                                         unsigned long long* __restrict__ mask,
                                                         unsigned long long* __restrict__ words)
{
    __shared__ uint32_t s_cnt[2][4];             // per wave: rows selected either way; one buffer per tile parity
    __shared__ unsigned long long s_w[4][6];     // per wave: max lt, max id, count of each direction
    __shared__ uint32_t s_cand[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    unsigned long long mx1 = 0, id1 = 0, mx2 = 0, id2 = 0;
    uint32_t c1 = 0, c2 = 0;                     // this thread's rows of each direction (at most 8 per tile)
    bool cand1 = false, cand2 = false;
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
                const uint64_t i = base + (uint64_t)(g + q) * kTmThreads + threadIdx.x;
                const uint64_t ic = i < n ? i : n - 1;
                hb[q] = load_hot(tb, ic);
                lb[q] = *reinterpret_cast<const uint32_t*>(row_ptr(tb, ic) + 16);
                ha[q] = load_hot(ta, ic);
                la[q] = *reinterpret_cast<const uint32_t*>(row_ptr(ta, ic) + 16);
            }
#pragma unroll
            for (int q = 0; q < kSyBatch; ++q) {
                const uint64_t i = base + (uint64_t)(g + q) * kTmThreads + threadIdx.x;
                const int64_t mod_b = (int64_t)(((uint64_t)hb[q].w << 32) | lb[q]);
                const int64_t mod_a = (int64_t)(((uint64_t)ha[q].w << 32) | la[q]);
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
                const bool selA = winA || selA0;
                c1 += selB;
                c2 += selA;
                if (selB) {
                    const int64_t lt = (int64_t)(((uint64_t)hb[q].y << 32) | hb[q].x);
                    const unsigned long long o = ord64(lt);
                    mx1 = o > mx1 ? o : mx1;
                    id1 = i + 1 > id1 ? i + 1 : id1;
                    cand1 |= lt > ca && (hb[q].z == rank_a || wsub(lt >> kShift, wall) > kMaxDrift);
                }
                if (selA) {
                    const uint4 h = winA ? hb[q] : ha[q];
                    const int64_t lt = (int64_t)(((uint64_t)h.y << 32) | h.x);
                    const unsigned long long o = ord64(lt);
                    mx2 = o > mx2 ? o : mx2;
                    id2 = i + 1 > id2 ? i + 1 : id2;
                    cand2 |= lt > cb && (h.z == rank_b || wsub(lt >> kShift, wall) > kMaxDrift);
                }
            }
        }
        if (lane == 0) s_cnt[par][w] = cnt;
        __syncthreads();                         // (the next tile writes the other buffer)
        if (threadIdx.x == 0) sel[tile] = s_cnt[par][0] + s_cnt[par][1] + s_cnt[par][2] + s_cnt[par][3];
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long a = __shfl_xor(mx1, off, 64), b = __shfl_xor(id1, off, 64);
        const unsigned long long c = __shfl_xor(mx2, off, 64), d = __shfl_xor(id2, off, 64);
        mx1 = a > mx1 ? a : mx1;
        id1 = b > id1 ? b : id1;
        mx2 = c > mx2 ? c : mx2;
        id2 = d > id2 ? d : id2;
        c1 += __shfl_xor(c1, off, 64);
        c2 += __shfl_xor(c2, off, 64);
    }
    const bool wc1 = __any(cand1), wc2 = __any(cand2);
    if (lane == 0) {
        s_w[w][0] = mx1; s_w[w][1] = id1; s_w[w][2] = c1;
        s_w[w][3] = mx2; s_w[w][4] = id2; s_w[w][5] = c2;
        s_cand[w] = (wc1 ? 1u : 0u) | (wc2 ? 2u : 0u);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t cd = 0;
        unsigned long long n1 = 0, n2 = 0;
        for (int ww = 0; ww < 4; ++ww) {
            mx1 = s_w[ww][0] > mx1 ? s_w[ww][0] : mx1;
            id1 = s_w[ww][1] > id1 ? s_w[ww][1] : id1;
            n1 += s_w[ww][2];
            mx2 = s_w[ww][3] > mx2 ? s_w[ww][3] : mx2;
            id2 = s_w[ww][4] > id2 ? s_w[ww][4] : id2;
            n2 += s_w[ww][5];
            cd |= s_cand[ww];
        }
        if (n1) {
            atomicMax(&words[0], mx1);
            atomicMax(&words[1], id1);
            if (cd & 1u) atomicMax(&words[2], 1ull);
            atomicAdd(&words[3], n1);
        }
        if (n2) {
            atomicMax(&words[4], mx2);
            atomicMax(&words[5], id2);
            if (cd & 2u) atomicMax(&words[6], 1ull);
            atomicAdd(&words[7], n2);
        }
    }
}

__global__ __launch_bounds__(kTmThreads) void k_sy_apply(Table ta, Table tb, uint64_t n,
                                                         const uint32_t* __restrict__ sel,
                                                         const unsigned long long* __restrict__ mask,
                                                         int64_t stamp_a, int64_t stamp_b,
                                                         Misc* __restrict__ misc, uint8_t* __restrict__ flags_a,
                                                         uint8_t* __restrict__ flags_b)
{
    __shared__ int s_pw[4][4];
    const uint64_t base = (uint64_t)blockIdx.x * kTmTile;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (sel[blockIdx.x] == 0) {                  // the whole workgroup: nothing selected in this tile, either way
#pragma unroll
        for (int side = 0; side < 2; ++side) {
            uint8_t* flags = side ? flags_b : flags_a;
            if (!flags) continue;
            uint8_t* f = flags + base;           // the tile's kTmTile bytes: 8 per thread where whole and aligned
            if (base + kTmTile <= n && (reinterpret_cast<uintptr_t>(f) & 7u) == 0) {
                static_assert(kTmItems == 8, "one 8-B store per thread zeroes the tile's flags");
                reinterpret_cast<unsigned long long*>(f)[threadIdx.x] = 0ull;
            } else {
#pragma unroll
                for (int q = 0; q < kTmItems; ++q) {
                    const uint64_t i = base + q * kTmThreads + threadIdx.x;
                    if (i < n) flags[i] = 0;
                }
            }
        }
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
            const uint64_t i = base + (uint64_t)(g + q) * kTmThreads + threadIdx.x;
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
            const uint64_t i = base + (uint64_t)(g + q) * kTmThreads + threadIdx.x;
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
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        np1 += __shfl_xor(np1, off, 64);
        nw1 += __shfl_xor(nw1, off, 64);
        np2 += __shfl_xor(np2, off, 64);
        nw2 += __shfl_xor(nw2, off, 64);
    }
    if (lane == 0) { s_pw[0][w] = np1; s_pw[1][w] = nw1; s_pw[2][w] = np2; s_pw[3][w] = nw2; }
    __syncthreads();
    if (threadIdx.x == 0) {
        np1 = s_pw[0][0] + s_pw[0][1] + s_pw[0][2] + s_pw[0][3];
        nw1 = s_pw[1][0] + s_pw[1][1] + s_pw[1][2] + s_pw[1][3];
        np2 = s_pw[2][0] + s_pw[2][1] + s_pw[2][2] + s_pw[2][3];
        nw2 = s_pw[3][0] + s_pw[3][1] + s_pw[3][2] + s_pw[3][3];
        const int slot = blockIdx.x & (kCounterSlots / 2 - 1);
        if (np1) atomicAdd(&misc->present[slot], (unsigned long long)np1);
        if (nw1) atomicAdd(&misc->won[slot], (unsigned long long)nw1);
        if (np2) atomicAdd(&misc->present[kCounterSlots / 2 + slot], (unsigned long long)np2);
        if (nw2) atomicAdd(&misc->won[kCounterSlots / 2 + slot], (unsigned long long)nw2);
    }
}
