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
