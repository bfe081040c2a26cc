// sorted_path.inc — the key-partitioned merge path (included by crdt_merge.hip).
//
// The gather path (K2 k_apply) reads every record's row at a random address:
// one 128-B line per record, ~31 G records/s on a 2^28-row table — the random
// request ceiling of the chip (tools/ubench_gather.hip), 13 % of HBM peak in
// algorithmic bytes.  This path instead groups the batch by key so that each
// table row is read and written once, coalesced, and resolves every key's
// records in LDS:
//
//   KP1  k_part_hist / k_scan_* / k_part_scatter1, level 1: an 8-bit radix
//        partition of the applied records (changesets < stop) on key bits
//        [shift1, shift1 + 8).  Tiles never straddle a changeset, so changesets keep
//        their order inside every bucket while a tile's own records (one changeset,
//        distinct keys) take LDS-atomic slots in any order.  Output record: 16 B
//        {lt, rank, val} (one dwordx4) + a 4-B kj column, kj = key bits [0, 20) |
//        (changeset - window base) << 20 (the next level's histogram reads kj alone).
//   KP2  k_part_hist / k_scan_* / k_part_scatter2, level 2: inside every level-1
//        bucket on key bits [12, 20) -> 2^16 final buckets of 4096 consecutive keys
//        (only when the capacity exceeds 2^20 keys; below that one level gives the
//        final buckets).  Its tiles span changesets, so it ranks stably (ballot
//        multisplit): every final bucket holds its records in (changeset, position) order.
//   KR   k_resolve: one workgroup per 4096-key bucket (part).  The bucket's
//        4096 rows are read once (coalesced) into LDS state; its records are
//        consumed in global order, 2048 per chunk; inside a chunk, records of the
//        same key are linked through an LDS list (head[key], tagged per chunk) and
//        each record finds the maximum of the same-key records before it —
//        the exact sequential semantics of R back-to-back Crdt.merge calls
//        (crdt.dart:83-90): a record wins iff it beats the row as left by every
//        earlier record; n_present / n_won are counted per record as in K2.
//        Winner rows are written once at the end, with mod = R_j of the winning
//        record's changeset.  Buckets over 65,536 records are split into parts
//        (k_resolve<true> folds, k_part_carry carries) so a Zipf head runs in parallel.
//
// Preconditions (checked on the host, otherwise the gather path runs):
// canonical C_0 >= 0 (so every stamp R_j >= 0 and rows written by one changeset are
// visible to the next, as a sequential fold assumes), capacity <= 2^28, < 2^31 records
// per window of 4096 changesets; with per-record win flags also a batch frame that fits the
// packed key (the flagged form, "win flags" at the end of this file; a sharded ctx's receivers run
// it on the all-gathered global frame, their records routed unpacked — only the order-free form
// takes packed wire records).
//
// Forms: the packed order-free form (counts off, no flags: one ds_max_u64 per record), the
// ordered packed form (flags and / or exact counts: changeset-ordered level 2 and an ordered
// resolve), the wide list form and the round-1 counted form (frames over 64 bits).

constexpr int kSBits = 12;                        // 4096 keys per final bucket
constexpr uint32_t kSKeys = 1u << kSBits;
constexpr uint32_t kDigits = 256;                 // 8-bit digits per level
constexpr int kJShift = 20;
constexpr uint32_t kKeyLoMask = (1u << kJShift) - 1;
constexpr uint32_t kWindow = 1u << (32 - kJShift);   // changesets per window (4096)
constexpr int kHThreads = 1024;                   // histogram workgroup
constexpr int kPThreads = 1024;                   // scatter workgroup (119 KB LDS; 512-thread
constexpr int kPWaves = kPThreads / 64;           // workgroups two per CU measured 15 % slower)
constexpr int kPItems = 4;
constexpr int kPSub = kPThreads * kPItems;        // 4096 records per LDS sub-tile
constexpr int kPTile = 28672;                     // the largest level-1 partition tile (records): seven scan
                                                  // tiles, exactly four 7168-record sub-tiles of the level-1
                                                  // scatter; the tile in use is l1_plan_tile() (28672 or 14336,
                                                  // both counted by the scan).  32768 left a ragged fifth
                                                  // sub-tile whose short digit runs are mostly partial lines
                                                  // (profiles/r04_l1tile_ab.txt)
constexpr int kPTile2 = 8192;                     // level-2 tiles of the packed form: one 8192-record
                                                  // sub-tile each (32K: +0.95 ms, 16K: +0.55 ms per step)
constexpr int kPGroups = kPItems * kPWaves;       // 64 ordered (item, wave) groups
#ifndef CRDT_FREE_ITEMS
#define CRDT_FREE_ITEMS 7
#endif
#ifndef CRDT_L1_ITEMS
#define CRDT_L1_ITEMS 7
#endif
constexpr int kFreeItems = CRDT_FREE_ITEMS;       // order-free level-2 scatter: records per thread
constexpr int kL1Items = CRDT_L1_ITEMS;           // level-1 scatter: records per thread
constexpr int kPLanes = kPThreads / 256;          // lanes scanning one digit's groups
static_assert(kPGroups / kPLanes == 16, "group scan: 16 groups per lane");
constexpr uint32_t kChunkTiles = 128;             // tiles per scan chunk
constexpr int kRThreads = 1024;
constexpr int kRItems = 2;
constexpr int kRChunk = kRThreads * kRItems;      // 2048 records per resolve chunk
constexpr uint32_t kRefLocal = 0xFFFFFFFFu;
constexpr uint32_t kRefAbsent = 0xFFFFFFFEu;
constexpr uint64_t kSortedMaxCap = 1ull << 28;

// Tiling of a record range into partition tiles that never straddle a segment
// (level 1: changeset segments — a changeset routed in from several ranks is one segment
// per source, listed in changeset order — whose changeset becomes kj's high bits;
// level 2: level-1 buckets, contiguous, so seg_end = seg_beg + 1).
struct TileMap {
    const uint64_t* seg_beg;   // [nseg] first record of segment s
    const uint64_t* seg_end;   // [nseg] one past its last record
    const uint32_t* tbase;     // [nseg + 1] tile prefix
    const uint32_t* tile_seg;  // [tiles] segment of each tile (k_seg_index), so a workgroup
    const uint32_t* seg_j;     // starts with two independent loads, not a search
    uint32_t nseg;             // seg_j [nseg]: global changeset of segment s (level 1 only)
    uint32_t tsize;            // records per tile: kPTile, or kPTile2 for level 2 of the packed form
    uint32_t tile0 = 0;        // k_part_scatter1: the launch covers tiles [tile0, tbase[nseg]) (route_l1's
                               // two launches over one tiling)
};

// Scan segments: tiles whose digit offsets are numbered together (level 1: all
// tiles of the window; level 2: the tiles of one level-1 bucket).
struct ScanMap {
    const uint32_t* tbase;     // [nseg + 1]
    const uint32_t* cbase;     // [nseg + 1] chunk prefix
    const uint64_t* seg_pos;   // [nseg] first output position of the segment
    uint32_t nseg;
};

__device__ inline uint32_t seg_of(const uint32_t* base, uint32_t n, uint32_t x) {
    uint32_t lo = 0, hi = n;                       // largest s < n with base[s] <= x
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (base[mid] <= x) lo = mid; else hi = mid;
    }
    return lo;
}

// idx[x] = largest s < n with base[s] <= x, for every x < base[n] (grid-stride): the
// segment lookup of tiles / resolve items done once, massively parallel.
__global__ __launch_bounds__(256) void k_seg_index(const uint32_t* __restrict__ base, uint32_t n, uint32_t max_x,
                                                   uint32_t* __restrict__ idx)
{
    const uint32_t total = std::min<uint32_t>(base[n], max_x);
    for (uint32_t x = blockIdx.x * 256 + threadIdx.x; x < total; x += gridDim.x * 256) idx[x] = seg_of(base, n, x);
}

__device__ inline void tile_info(const TileMap& m, uint32_t t, uint32_t* seg, uint64_t* beg, uint32_t* len) {
    const uint32_t s = m.tile_seg[t];
    const uint64_t b = m.seg_beg[s] + (uint64_t)(t - m.tbase[s]) * m.tsize;
    const uint64_t e = m.seg_end[s];
    *seg = s;
    *beg = b;
    *len = (uint32_t)(e > b ? std::min<uint64_t>(m.tsize, e - b) : 0);
}

// XCD-aware tile order for the scatters.  Workgroups are dispatched round-robin over the
// 8 XCDs (workgroup i runs on XCD i % 8); mapped this way XCD x works through the contiguous
// tiles [x * per, (x + 1) * per), so the output runs of consecutive tiles — adjacent in every
// bucket — meet in the same L2, and a line split between two tiles is completed there
// before it is written back.  The grid is padded to 8 * per workgroups; tiles >= n exit.
constexpr uint32_t kXcds = 8;
__device__ inline uint32_t xcd_tile(uint32_t i, uint32_t per, bool on) {
    return on ? (i % kXcds) * per + i / kXcds : i;
}
inline uint32_t xcd_grid(uint32_t n, bool on) { return on ? ((n + kXcds - 1) / kXcds) * kXcds : n; }

// Lanes of the wave that are active and carry the same 8-bit digit as this lane.
__device__ inline unsigned long long match_digit(uint32_t d, bool active) {
    unsigned long long m = __ballot(active);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        const bool bit = (d >> b) & 1u;
        const unsigned long long bb = __ballot(active && bit);
        m &= bit ? bb : ~bb;
    }
    return m;
}

// 256-thread exclusive scan helper (threads 0..255 = 4 waves); returns exclusive prefix,
// *total = sum of all 256.
__device__ inline uint32_t scan256_excl(uint32_t v, uint32_t* s_w /*[4]*/, uint32_t* total) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t u = __shfl_up(inc, off, 64);
        if (lane >= off) inc += u;
    }
    if (tid < 256 && lane == 63) s_w[w] = inc;
    __syncthreads();
    uint32_t wp = 0;
    for (int k = 0; k < w && k < 4; ++k) wp += s_w[k];
    *total = s_w[0] + s_w[1] + s_w[2] + s_w[3];
    return wp + inc - v;
}


// -------------------------------------------------------------------- histogram
// hist[t][d] = records of tile t with digit d (0 for tiles of changesets >= stop).
// keyw: level 1 the user key column, level 2 the kj column of level 1.
// k16: level 2 over the 2-B key column of k_part_scatter1<.., kK16>.
template <bool kLevel1, bool k16 = false>
__global__ __launch_bounds__(kHThreads) void k_part_hist(
    const void* __restrict__ keyw, TileMap tm, uint32_t jbase, const Misc* __restrict__ misc,
    uint64_t cap, uint32_t shift, uint32_t* __restrict__ hist, KeyMap km = KeyMap{0u, 8u})
{
    constexpr int kQ = kPTile / kHThreads;       // 32 records per thread
    __shared__ uint32_t h[kDigits];
    const uint32_t t = blockIdx.x;
    if (t >= tm.tbase[tm.nseg]) return;
    uint32_t seg, len;
    uint64_t beg;
    tile_info(tm, t, &seg, &beg, &len);
    if (kLevel1 && misc && tm.seg_j[seg] >= misc->stop) len = 0;   // (misc null: every changeset)
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid < (int)kDigits) h[tid] = 0;
    uint32_t k[kQ];
#pragma unroll
    for (int q = 0; q < kQ; ++q) {                // every load in flight before the first use
        const uint32_t i = q * kHThreads + tid;
        k[q] = i >= len ? 0u
             : k16 ? (uint32_t)__builtin_nontemporal_load(static_cast<const uint16_t*>(keyw) + beg + i)
                   : __builtin_nontemporal_load(static_cast<const uint32_t*>(keyw) + beg + i);
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < kQ; ++q) {               // counts are order-free: one LDS atomic per record
        const uint32_t i = q * kHThreads + tid;  // (2.2x the ballot-match rate, ubench_hist), one
        const bool act = i < len && (!kLevel1 || (k[q] >> km.gsh) < cap);   // per wave when it holds one digit
        const uint32_t d = kLevel1 ? km_digit(km, k[q], shift) : (k[q] >> shift) & (kDigits - 1);
        digit_count(h, d, act, lane);
    }
    __syncthreads();
    if (tid < (int)kDigits) hist[(uint64_t)t * kDigits + tid] = h[tid];
}

// Level-2 histogram over the 2-B key column (k_part_scatter1<.., kK16>'s; digit = key16 >> shift):
// the column read as whole 16-B blocks (8 keys per load instead of one 2-B load each; the blocks
// at a tile's two ends are shared with its neighbours and their outside keys masked), each wave
// counting into its own 256 bins with no-return LDS adds (no same-bin serialisation between
// waves, no ballot fast path: level-2 digits inside a tile are spread), the copies summed.  kT threads for
// tiles of at most kTile records: the 8192-record level-2 tiles take 256 (4 KB of bins, five 16-B loads per
// thread, many workgroups per CU: the tile's fixed work — zeroing, summing and writing the bins — is a
// quarter of the 1024-thread form's); the 32K tiles keep 1024.
// kD8 (the compact form): the column is k_part_scatter1<.., kC>'s 1-B level-2 digits, 16 per 16-B block.
template <int kT = kHThreads, int kTile = kPTile, bool kD8 = false>
__global__ __launch_bounds__(kT) void k_part_hist16w(
    const uint16_t* __restrict__ key16, TileMap tm, uint32_t shift, uint32_t* __restrict__ hist)
{
    constexpr uint32_t kE = kD8 ? 16u : 8u, kEsh = kD8 ? 4u : 3u;   // column entries per 16-B block
    constexpr int kWv = kT / 64;
    __shared__ uint32_t hw[kWv][kDigits];          // 4 / 16 KB
    const uint32_t t = blockIdx.x;
    if (t >= tm.tbase[tm.nseg]) return;
    uint32_t seg, len;
    uint64_t beg;
    tile_info(tm, t, &seg, &beg, &len);
    const int tid = threadIdx.x, w = tid >> 6;
    for (int i = tid; i < kWv * (int)kDigits; i += kT) (&hw[0][0])[i] = 0;
    const uint64_t end = beg + len;
    const uint64_t b0 = beg >> kEsh, nblk = len ? ((end + kE - 1) >> kEsh) - b0 : 0;   // 16-B blocks touched
    constexpr int kB = ((int)(kTile / kE) + 1 + kT - 1) / kT;                    // per thread at most
    u32x4 v[kB];
#pragma unroll
    for (int q = 0; q < kB; ++q) {                // every load in flight before the first use
        const uint64_t b = (uint64_t)q * kT + tid;
        v[q] = b < nblk ? __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(key16) + b0 + b)
                        : u32x4{0u, 0u, 0u, 0u};
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < kB; ++q) {
        const uint64_t b = (uint64_t)q * kT + tid;
        if (b >= nblk) continue;
        const uint64_t e0 = (b0 + b) << kEsh;     // column index of the block's first key
        const uint32_t wd[4] = {v[q].x, v[q].y, v[q].z, v[q].w};
#pragma unroll
        for (int x = 0; x < (int)kE; ++x) {
            const uint64_t e = e0 + x;
            const uint32_t k = kD8 ? (wd[x >> 2] >> ((x & 3) * 8)) & 0xFFu : (wd[x >> 1] >> ((x & 1) * 16)) & 0xFFFFu;
            if (e >= beg && e < end) atomicAdd(&hw[w][kD8 ? k : (k >> shift) & (kDigits - 1)], 1u);
        }
    }
    __syncthreads();
    for (int d = tid; d < (int)kDigits; d += kT) {
        uint32_t s = 0;
#pragma unroll
        for (int x = 0; x < kWv; ++x) s += hw[x][d];
        hist[(uint64_t)t * kDigits + d] = s;
    }
}

// Tiles of the changesets >= stop hold no records to apply: their rows of a histogram the scan
// counted (k_scan<.., kHist>, before stop was known) are cleared.  stop == R: nothing to do.
__global__ __launch_bounds__(256) void k_hist_trim(uint32_t* __restrict__ hist, const uint32_t* __restrict__ ptb,
                                                   uint32_t R, const Misc* __restrict__ misc)
{
    const uint32_t stop = misc->stop;
    if (stop >= R) return;
    const uint64_t a = (uint64_t)ptb[stop] * kDigits, b = (uint64_t)ptb[R] * kDigits;
    for (uint64_t x = a + (uint64_t)blockIdx.x * 256 + threadIdx.x; x < b; x += (uint64_t)gridDim.x * 256)
        hist[x] = 0;
}
// The scan's hot bins (k_scan's ScanHot) for a form that does not take them: back into digit 0, so that hist is
// what it is without them.  One wave per tile (grid-stride).
__global__ __launch_bounds__(64) void k_hot_fold(uint32_t* __restrict__ hist, const uint32_t* __restrict__ hhist,
                                                 uint32_t tiles)
{
    for (uint32_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const uint32_t* h = hhist + (uint64_t)t * kDigits;
        uint32_t s = h[threadIdx.x] + h[64 + threadIdx.x] + h[128 + threadIdx.x] + h[192 + threadIdx.x];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
        if (threadIdx.x == 0) hist[(uint64_t)t * kDigits] += s;
    }
}

// Final bucket starts of the hot buckets (filled by level 1, HotL1): level 2's scan left bstart[b] = the hot total
// for the b < hot (empty there); their starts are the hot scan's.
__global__ __launch_bounds__(256) void k_hot_starts(uint32_t* __restrict__ bstart, const uint32_t* __restrict__ hstart,
                                                    uint32_t hot)
{
    if (threadIdx.x < hot) bstart[threadIdx.x] = hstart[threadIdx.x];
}
static_assert(kHotShift == (uint32_t)kSBits && kHotMax == kDigits, "a hot bin is a final bucket of level-1 digit 0");
static_assert(kPTile == (int)kHistSub * kTile && (kPTile / 2) % 1024 == 0,
              "the largest level-1 tile is kHistSub scan tiles; half of it splits on the scan's 1024-record groups");
static_assert(kDigits == 256, "k_scan<.., kHist> counts 256 digits");

// ------------------------------------------------------------------------- scan
// S1: per chunk of <= kChunkTiles tiles (inside one scan segment), digit sums.
__global__ __launch_bounds__(256) void k_scan_part(const uint32_t* __restrict__ hist, ScanMap sm,
                                                   uint32_t* __restrict__ part)
{
    const uint32_t c = blockIdx.x;
    if (c >= sm.cbase[sm.nseg]) return;
    const uint32_t s = seg_of(sm.cbase, sm.nseg, c);
    const uint32_t t0 = sm.tbase[s] + (c - sm.cbase[s]) * kChunkTiles;
    const uint32_t t1 = std::min<uint32_t>(t0 + kChunkTiles, sm.tbase[s + 1]);
    const uint32_t d = threadIdx.x;
    uint32_t sum = 0;
#pragma unroll 8
    for (uint32_t t = t0; t < t1; ++t) sum += hist[(uint64_t)t * kDigits + d];
    part[(uint64_t)c * kDigits + d] = sum;
}

// S2: one workgroup per scan segment: exclusive chunk offsets inside the segment,
// then the segment's digit starts (= output position of bucket (segment, digit)).
// dstart[s][d] (u32) and, optionally, dstart64 (u64, [nseg*256 + 1]).
__global__ __launch_bounds__(256) void k_scan_seg(const uint32_t* __restrict__ part, ScanMap sm,
                                                  uint32_t* __restrict__ choff, uint32_t* __restrict__ dstart,
                                                  uint64_t* __restrict__ dstart64)
{
    __shared__ uint32_t s_w[4];
    const uint32_t s = blockIdx.x, d = threadIdx.x;
    const uint32_t c0 = sm.cbase[s], c1 = sm.cbase[s + 1];
    uint32_t run = 0;
#pragma unroll 8
    for (uint32_t c = c0; c < c1; ++c) {
        const uint32_t v = part[(uint64_t)c * kDigits + d];
        choff[(uint64_t)c * kDigits + d] = run;
        run += v;
    }
    uint32_t total;
    const uint32_t ex = scan256_excl(run, s_w, &total);
    const uint64_t pos = sm.seg_pos[s] + ex;
    dstart[(uint64_t)s * kDigits + d] = (uint32_t)pos;
    if (dstart64) {
        dstart64[(uint64_t)s * kDigits + d] = pos;
        if (s + 1 == sm.nseg && d == kDigits - 1) dstart64[(uint64_t)sm.nseg * kDigits] = sm.seg_pos[s] + total;
    }
    if (s + 1 == sm.nseg && d == kDigits - 1) dstart[(uint64_t)sm.nseg * kDigits] = (uint32_t)(sm.seg_pos[s] + total);
}

// S3: tile offsets toff[t][d] = first output position of tile t's digit-d records.
__global__ __launch_bounds__(256) void k_scan_tiles(const uint32_t* __restrict__ hist,
                                                    const uint32_t* __restrict__ choff, ScanMap sm,
                                                    const uint32_t* __restrict__ dstart,
                                                    uint32_t* __restrict__ toff)
{
    const uint32_t c = blockIdx.x;
    if (c >= sm.cbase[sm.nseg]) return;
    const uint32_t s = seg_of(sm.cbase, sm.nseg, c);
    const uint32_t t0 = sm.tbase[s] + (c - sm.cbase[s]) * kChunkTiles;
    const uint32_t t1 = std::min<uint32_t>(t0 + kChunkTiles, sm.tbase[s + 1]);
    const uint32_t d = threadIdx.x;
    uint32_t run = dstart[(uint64_t)s * kDigits + d] + choff[(uint64_t)c * kDigits + d];
    // eight tiles' counts in flight per thread (a chunk's walk is ~128 dependent steps, on few workgroups: cfg3's
    // level 1 has 32 chunks)
    for (uint32_t t = t0; t < t1; t += 8) {
        uint32_t h[8];
#pragma unroll
        for (uint32_t u = 0; u < 8; ++u) h[u] = t + u < t1 ? hist[(uint64_t)(t + u) * kDigits + d] : 0u;
#pragma unroll
        for (uint32_t u = 0; u < 8; ++u) {
            if (t + u < t1) toff[(uint64_t)(t + u) * kDigits + d] = run;
            run += h[u];
        }
    }
}

// Level-2 tiling and scan segments from the level-1 bucket starts (one workgroup).
__global__ __launch_bounds__(256) void k_l2_plan(const uint64_t* __restrict__ l1_beg, uint32_t* __restrict__ tbase,
                                                 uint32_t* __restrict__ cbase, uint32_t tsize)
{
    __shared__ uint32_t s_w[4];
    const uint32_t s = threadIdx.x;
    const uint64_t n = l1_beg[s + 1] - l1_beg[s];
    const uint32_t nt = (uint32_t)((n + tsize - 1) / tsize);
    const uint32_t nc = (nt + kChunkTiles - 1) / kChunkTiles;
    uint32_t tt, tc;
    const uint32_t et = scan256_excl(nt, s_w, &tt);
    __syncthreads();
    const uint32_t ec = scan256_excl(nc, s_w, &tc);
    tbase[s] = et;
    cbase[s] = ec;
    if (s == 255) { tbase[256] = tt; cbase[256] = tc; }
}

// ------------------------------------------------------------ packed order-free resolve
// The order-free form (no per-record counts) needs only each key's best record: max over the
// local row and the bucket's records of (lt, rank), ties to the earlier changeset and the
// local row before all (crdt.dart:83-84 applied in changeset order).  When the records' lt and
// rank spans fit (the frame k_part_scatter1 reduced), that order is one unsigned 64-bit key
//     ((lt - lt_min) << (K + J)) | ((rank - rank_min) << J) | (W - window changeset)
// with W changesets per window and J = the bits of W + 1 (W = min(R, 4096): 11 bits for the
// 1024-replica fan-in; narrower windows when the lt span needs the bits), and a bucket resolves with ONE LDS 64-bit atomic max per record (ds_max_u64) plus a compare
// after the chunk's barrier that lets the record equal to the new max store its value handle —
// no same-key lists.  The local row enters clamped: below the frame it loses to every record
// (key 0, also "absent"), above it it beats every record (all ones); inside it, changeset
// field W + 1 keeps it ahead of an equal record, and a rank outside the frame is clamped with
// changeset field 0 below / rank field span + 1 above.  A state whose changeset field is in
// [1, W] is a record's and is written back with mod = R_j.  Frames that do not fit 64 bits even
// with 1022-changeset windows (an lt span over ~2^(54 - K)) take the wide records and the list form.  The frame comes from the scan (k_scan<*, *, true>); the host reads it once per
// call and picks the form, so each window launches one form's kernels only.
struct PackFrame {
    int64_t lt0;       // frame minimum lt
    uint64_t lt_span;  // max - min (wrapping difference of the int64 bounds)
    uint32_t rk0, rk_span;
    uint32_t jb;       // J: bits of the changeset field
    uint32_t jwin;     // W: changesets per window (field values 1 .. W; 0 and W + 1 for the local row)
    uint32_t sh;       // K + J
    uint64_t rk_mask;  // (1 << K) - 1
    uint32_t rk_limit; // ranks must be below (a declared bound; UINT32_MAX: frame from the data)
    bool ok;
    bool key4;         // the key uses <= 60 bits: a record's key bits [0, 4) ride in bits [60, 64)
    // the compact lt field (round 6; cb > 0): lt = hi * 2^16 + lo (hi = lt >> 16), and every record's lo is at
    // most 2^cb - 2, so the field ((hi - m0) << cb) | lo orders records exactly as lt does in L = bitlen(hi span)
    // + cb bits instead of bitlen(lt span) — the 1B fan-in's clocks (2^16 ms, counters < 16) take 21 bits, not 32,
    // and a record's whole 20-bit level-1 key then rides in its 64-bit word (kCKeyShift: 12-B partition records,
    // no key column).  A local row whose lo is over 2^cb - 2 packs with lo = 2^cb - 1: above every record of its
    // hi, below those of hi + 1 (no record has its exact lt, so no tie is decided by the lower fields).
    uint32_t cb;       // 0: the plain lt field (lt - lt0)
    int64_t m0;        // hi of the frame's minimum lt (cb > 0)
};

// The compact form's 12-B partition record: the packed key in bits [0, 44) of its 64-bit word (frame bits
// L + K + J <= 44) and the key's low 20 bits (its level-1 bucket slot) in bits [44, 64); level 2 moves the
// record as it is (its digit: key bits [12, 20) = word bits [56, 64)), and the resolve takes the key's low 12
// bits from word bits [44, 56).
constexpr uint32_t kCKeyShift = 44;
constexpr uint64_t kCPkMask = (1ull << kCKeyShift) - 1;

// the lt field of a packed key (a record's lt inside the frame) and its inverse
__host__ __device__ inline uint64_t pack_ltf(const PackFrame& f, int64_t lt) {
    if (!f.cb) return (uint64_t)lt - (uint64_t)f.lt0;
    return ((uint64_t)((lt >> 16) - f.m0) << f.cb) | ((uint64_t)lt & 0xFFFFull);
}
__host__ __device__ inline int64_t pack_lt(const PackFrame& f, uint64_t x) {
    const uint64_t lf = x >> f.sh;
    if (!f.cb) return (int64_t)((uint64_t)f.lt0 + lf);
    return (int64_t)(((uint64_t)((int64_t)(lf >> f.cb) + f.m0) << 16) | (lf & ((1ull << f.cb) - 1)));
}

__host__ __device__ inline int bitlen64(uint64_t x) {
    int b = 0;
    while (b < 64 && (x >> b) != 0) ++b;
    return b;
}

// The changeset field of a frame whose lt / rank fields take L + K bits, for R changesets: W = min(R,
// 4096) changesets per window in J = bitlen(W + 1) bits when they fit beside L + K, else the widest
// window that does (at least 1022 changesets: more windows would each re-read the table).
__host__ __device__ inline bool frame_window(int L, int K, uint32_t R, uint32_t* jb, uint32_t* jwin) {
    const uint32_t want = R < 1u ? 1u : (R > kWindow ? kWindow : R);
    int J = bitlen64((uint64_t)want + 1);
    if (L + K + J > 64) {
        J = 64 - L - K;
        if (J < 10) return false;
    }
    *jb = (uint32_t)J;
    *jwin = std::min<uint32_t>(want, (1u << J) - 2);
    return true;
}

// From the scan's max-accumulators (Misc::fr_*; all zero: no record) and the call's changesets.
__host__ __device__ inline PackFrame make_frame(unsigned long long acc_lo, unsigned long long acc_hi,
                                                uint32_t acc_rlo, uint32_t acc_rhi, uint32_t R) {
    PackFrame f;
    f.rk_limit = UINT32_MAX;
    f.cb = 0;
    f.m0 = 0;
    f.jb = 13;
    f.jwin = kWindow;
    if (acc_lo == 0 && acc_hi == 0) {                  // no record: anything goes
        f.lt0 = 0; f.lt_span = 0; f.rk0 = 0; f.rk_span = 0; f.rk_mask = 1; f.key4 = true;
        f.ok = frame_window(0, 1, R, &f.jb, &f.jwin);
        f.sh = 1 + f.jb;
        return f;
    }
    f.lt0 = (int64_t)(~acc_lo ^ (1ull << 63));
    const uint64_t lt_max = acc_hi ^ (1ull << 63);
    f.lt_span = lt_max - (uint64_t)f.lt0;
    f.rk0 = ~acc_rlo;
    f.rk_span = acc_rhi - f.rk0;
    // the lt field holds 0 .. span (a local row above the frame packs to all ones); the rank field
    // 0 .. span + 1 (a local rank above the frame clamps to span + 1)
    const int K = bitlen64((uint64_t)f.rk_span + 1), L = bitlen64(f.lt_span);
    f.rk_mask = K >= 64 ? ~0ull : (1ull << K) - 1;
    f.ok = L + K <= 54 && frame_window(L, K, R, &f.jb, &f.jwin);
    f.sh = (uint32_t)K + f.jb;
    f.key4 = f.ok && L + K + (int)f.jb <= 60;
    return f;
}

// kCmp: the frame is compact (cb > 0) — decided at compile time, so the partition kernels of the plain frame
// keep their register budget (the level-1 scatter sits at 128 VGPRs)
template <bool kCmp = false>
__host__ __device__ inline uint64_t pack_record(const PackFrame& f, int64_t lt, uint32_t rank, uint32_t jw) {
    const uint64_t lf = kCmp ? ((uint64_t)((lt >> 16) - f.m0) << f.cb) | ((uint64_t)lt & 0xFFFFull)
                             : (uint64_t)lt - (uint64_t)f.lt0;
    return (lf << f.sh) | ((uint64_t)(rank - f.rk0) << f.jb) | (uint64_t)(f.jwin - jw);
}

// The compact frame (PackFrame::cb) of a frame f = make_frame(..) whose records' largest lt & 0xFFFF is cmax:
// ok when its packed key fits kCKeyShift bits; else f unchanged (cb = 0).
__host__ __device__ inline PackFrame compact_frame(PackFrame f, uint32_t cmax, uint32_t R) {
    if (!f.ok || cmax > 0xFFFDu) return f;
    const int64_t m0 = f.lt0 >> 16, m1 = (int64_t)((uint64_t)f.lt0 + f.lt_span) >> 16;
    const int cb = bitlen64((uint64_t)cmax + 1);
    const int L = bitlen64((uint64_t)(m1 - m0)) + cb, K = bitlen64((uint64_t)f.rk_span + 1);
    uint32_t jb, jwin;
    if (L + K > 54 || !frame_window(L, K, R, &jb, &jwin) || L + K + (int)jb > (int)kCKeyShift) return f;
    PackFrame c = f;
    c.cb = (uint32_t)cb;
    c.m0 = m0;
    c.jb = jb;
    c.jwin = jwin;
    c.sh = (uint32_t)K + jb;
    c.key4 = true;
    return c;
}
__host__ __device__ inline uint64_t pack_jmask(const PackFrame& f) { return (1ull << f.jb) - 1; }
// the window changeset of a record's packed key, and its rank
__host__ __device__ inline uint32_t pack_jw(const PackFrame& f, uint64_t x) {
    return f.jwin - (uint32_t)(x & pack_jmask(f));
}
__host__ __device__ inline uint32_t pack_rank(const PackFrame& f, uint64_t x) {
    return f.rk0 + (uint32_t)((x >> f.jb) & f.rk_mask);
}

// local row (lt, rank), present (visible to merge); absent -> 0
__device__ inline uint64_t pack_local(const PackFrame& f, bool present, int64_t lt, uint32_t rank) {
    if (!present || lt < f.lt0) return 0;
    if ((uint64_t)lt - (uint64_t)f.lt0 > f.lt_span) return UINT64_MAX;
    const uint64_t lo = (uint64_t)lt & 0xFFFFull, top = (1ull << f.cb) - 1;   // (cb > 0: lo over the records')
    const uint64_t hi = (f.cb && lo > top ? pack_ltf(f, (int64_t)(((uint64_t)lt & ~0xFFFFull) | top))
                                          : pack_ltf(f, lt)) << f.sh;
    if (rank < f.rk0) return hi;                                   // rank field 0, changeset field 0
    if (rank - f.rk0 > f.rk_span) return hi | ((uint64_t)(f.rk_span + 1) << f.jb);
    return hi | ((uint64_t)(rank - f.rk0) << f.jb) | (uint64_t)(f.jwin + 1);
}

__device__ inline bool pack_is_record(const PackFrame& f, uint64_t st) {
    const uint32_t jf = (uint32_t)(st & pack_jmask(f));
    return st != UINT64_MAX && jf >= 1u && jf <= f.jwin;
}

// ---------------------------------------------------------------------- records
// A partition record is a payload plus its kj word (kept apart: the level-2 histogram reads kj
// alone).  Wide payload (16 B, one dwordx4): {lt lo, lt hi, rank, val}.  Packed payload (12 B,
// one dwordx3), when the batch's frame fits the resolve's 64-bit key (PackFrame below):
// {key lo, key hi, val} with key = the packed (lt, rank, changeset) — the records then cost
// 16 B instead of 20 in every partition pass and the resolve reads its key ready-made.
struct __attribute__((aligned(4))) Rec12 { uint32_t a, b, c; };

template <bool kPk>
__device__ inline void load_payload(const void* __restrict__ base, uint64_t i, uint32_t (&w)[kPk ? 3 : 4]) {
    if constexpr (kPk) {
        const Rec12 r = static_cast<const Rec12*>(base)[i];
        w[0] = r.a; w[1] = r.b; w[2] = r.c;
    } else {
        const u32x4 r = __builtin_nontemporal_load(static_cast<const u32x4*>(base) + i);
        w[0] = r.x; w[1] = r.y; w[2] = r.z; w[3] = r.w;
    }
}

template <bool kPk>
__device__ inline void store_payload(void* __restrict__ base, uint64_t i, const uint32_t (&w)[kPk ? 3 : 4]) {
    if constexpr (kPk) {
        Rec12 r; r.a = w[0]; r.b = w[1]; r.c = w[2];
        static_cast<Rec12*>(base)[i] = r;
    } else {
        u32x4 r; r.x = w[0]; r.y = w[1]; r.z = w[2]; r.w = w[3];
        static_cast<u32x4*>(base)[i] = r;
    }
}

// ---------------------------------------------------------------------- scatter
// Partition of one tile: sub-tiles of kS records, each ranked in LDS, staged in digit order
// (payload words SoA) and written as contiguous runs at the tile's running digit cursors.
// kStable (level 2 with exact counts): ballot multisplit per wave, 64 ordered (item, wave)
// groups scanned per digit by 4 lanes of 16 groups each, so records keep (changeset, position)
// order.  Otherwise (order-free sorted path): ranks from one LDS atomic per record, as level 1.
// kK8 (packed, PackFrame::key4): the output keeps a record's key bits [4, 12) in a 1-B column
// and bits [0, 4) in its packed key's top 4 bits (13 B per final record instead of 16).
// kIn16: the input is k_part_scatter1<.., kK16>'s (2-B key column of key bits [4, 20), bits [0, 4)
// already in the packed key), so kK8 too.
// kStable && kPk: the flagged form (packed records kept in changeset order for the ordered resolve);
// pos_out (stable only) then receives, at each record's level-1 index, its offset inside its tile's
// digit run (level-2 position - toff[t][digit]; < 2^16: tiles hold at most kPTile records).
// The packed order-free form takes 8 records per thread: one 8192-record sub-tile per level-2 tile, 131 KB
// of LDS (4 per thread, two 4096-record sub-tiles and two workgroups per CU: measured +0.39 ms, DESIGN §5.2).
// kC (the compact form): 12-B records in and out, unchanged (the digit is word bits [56, 64): key bits [12,
// 20)); no key column is read or written.
template <bool kStable, bool kPk, bool kK8 = false, bool kIn16 = false, bool kDigKj = kIn16, bool kC = false>
__global__ __launch_bounds__(kPThreads) void k_part_scatter2(
    const void* __restrict__ irec, const void* __restrict__ ikj, TileMap tm, uint32_t shift,
    const uint32_t* __restrict__ toff, void* __restrict__ orec, void* __restrict__ okj, uint32_t xper,
    const uint32_t* __restrict__ thist, uint16_t* __restrict__ pos_out = nullptr)
{
    static_assert(!kK8 || kPk, "1-B key column: packed records only");
    static_assert(kPTile <= 65536, "run offsets in 16 bits");
    static_assert(!kIn16 || kK8, "2-B key input gives 1-B key output");
    static_assert(!kDigKj || kIn16, "digit recomputed from the staged 16-bit key: 2-B key input only");
    static_assert(!kC || (kPk && !kStable && kDigKj), "compact: the order-free packed form");
    constexpr int kW = kPk ? 3 : 4;                       // payload words
    constexpr int kI = kStable ? kPItems : kPk ? 8 : kFreeItems;   // records per thread per sub-tile
    constexpr int kS = kPThreads * kI;                    // records per LDS sub-tile
    __shared__ uint32_t cur[kDigits];
    __shared__ uint32_t dst[kDigits + 1];
    __shared__ uint32_t tot_s[kDigits];
    __shared__ uint32_t s_w[4];
    __shared__ uint16_t gcnt[kStable ? kDigits * kPGroups : 2];   // [digit][group], 32 KB
    // payload staging: wide = one dwordx4 per record (64 KB at 4 per thread .. 112 KB at 7),
    // packed = 3 dword arrays (96 KB at 8 per thread)
    __shared__ u32x4 s_rec[kPk ? 1 : kS];
    __shared__ uint32_t s_pay[kPk ? kW : 1][kPk ? kS : 1];
    __shared__ uint32_t s_kj[kC ? 1 : kS];            // 28-32 KB (kC: the staged word 1 is the key word)
    __shared__ uint8_t s_dig[kDigKj ? 1 : kS];        //   7-8 KB (kDigKj: the digit is recomputed from s_kj)
    const uint32_t t = xcd_tile(blockIdx.x, xper, xper != 0);
    if (t >= tm.tbase[tm.nseg]) return;
    uint32_t seg, len;
    uint64_t beg;
    tile_info(tm, t, &seg, &beg, &len);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const unsigned long long below = (1ull << lane) - 1;
    // order-free form: odd tiles fill their ranges downwards (k_part_scatter1: neighbours' shared
    // lines written at the same time)
    const bool rev = !kStable && thist && (t & 1u);
    if (tid < (int)kDigits)
        cur[tid] = toff[(uint64_t)t * kDigits + tid] + (rev ? thist[(uint64_t)t * kDigits + tid] : 0u);
    // register double buffer: sub-tile sb + kS is loaded while sb is ranked and written
    uint32_t nrec[kI][kW];
    uint32_t nv[kI];
    auto load_sub = [&](uint32_t sb) {
#pragma unroll
        for (int q = 0; q < kI; ++q) {
            const uint32_t i = sb + q * kPThreads + tid;
            const uint64_t gi = beg + (i < len ? i : 0);
            load_payload<kPk>(irec, gi, nrec[q]);
            nv[q] = kC ? 0u
                  : kIn16 ? (uint32_t)__builtin_nontemporal_load(static_cast<const uint16_t*>(ikj) + gi)
                          : __builtin_nontemporal_load(static_cast<const uint32_t*>(ikj) + gi);
        }
    };
    load_sub(0);
    for (uint32_t sb = 0; sb < len; sb += kS) {
        if (kStable) {
            u32x4* g4 = reinterpret_cast<u32x4*>(gcnt);
            const u32x4 z = {0u, 0u, 0u, 0u};
            for (int i = tid; i < (int)(kDigits * kPGroups / 8); i += kPThreads) g4[i] = z;
        } else if (tid < (int)kDigits) {
            tot_s[tid] = 0;
        }
        uint32_t rec[kI][kW];
        uint32_t v[kI], d[kI], rk[kI];
        bool act[kI];
#pragma unroll
        for (int q = 0; q < kI; ++q) {
            act[q] = sb + q * kPThreads + tid < len;
#pragma unroll
            for (int x = 0; x < kW; ++x) rec[q][x] = nrec[q][x];
            v[q] = kC ? nrec[q][kC ? 1 : 0] : nv[q];      // (kC: shift = 24, the word's top byte)
        }
        if (sb + kS < len) load_sub(sb + kS);
        __syncthreads();                                 // gcnt zeroed; previous sub-tile's cursors final
        if (!kStable) {                                  // order-free: rank = LDS atomic slot
#pragma unroll
            for (int q = 0; q < kI; ++q) {
                d[q] = (v[q] >> shift) & (kDigits - 1);
                rk[q] = digit_count(tot_s, d[q], act[q], lane);
            }
            __syncthreads();
        } else {
#pragma unroll
        for (int q = 0; q < kI; ++q) {
            d[q] = (v[q] >> shift) & (kDigits - 1);
            const unsigned long long m = match_digit(d[q], act[q]);
            rk[q] = (uint32_t)__popcll(m & below);
            if (act[q] && rk[q] == 0) gcnt[d[q] * kPGroups + q * kPWaves + w] = (uint16_t)__popcll(m);
        }
        __syncthreads();
        {   // per digit, exclusive scan over its groups: kPLanes adjacent lanes, 16 groups each
            const uint32_t dg = tid / kPLanes, part = tid % kPLanes;
            u32x4* p4 = reinterpret_cast<u32x4*>(gcnt + dg * kPGroups + part * 16);
            u32x4 a = p4[0], b = p4[1];
            uint32_t c[16] = {a.x & 0xFFFF, a.x >> 16, a.y & 0xFFFF, a.y >> 16, a.z & 0xFFFF, a.z >> 16,
                              a.w & 0xFFFF, a.w >> 16, b.x & 0xFFFF, b.x >> 16, b.y & 0xFFFF, b.y >> 16,
                              b.z & 0xFFFF, b.z >> 16, b.w & 0xFFFF, b.w >> 16};
            uint32_t sum = 0;
#pragma unroll
            for (int g = 0; g < 16; ++g) sum += c[g];
            uint32_t inc = sum;                          // inclusive over the 4 parts of this digit
#pragma unroll
            for (int off = 1; off < kPLanes; off <<= 1) {
                const uint32_t u = __shfl_up(inc, off, 64);
                if ((int)part >= off) inc += u;
            }
            uint32_t run = inc - sum;
#pragma unroll
            for (int g = 0; g < 16; ++g) { const uint32_t x = c[g]; c[g] = run; run += x; }
            a.x = c[0] | (c[1] << 16); a.y = c[2] | (c[3] << 16); a.z = c[4] | (c[5] << 16); a.w = c[6] | (c[7] << 16);
            b.x = c[8] | (c[9] << 16); b.y = c[10] | (c[11] << 16); b.z = c[12] | (c[13] << 16);
            b.w = c[14] | (c[15] << 16);
            p4[0] = a;
            p4[1] = b;
            if (part == kPLanes - 1) tot_s[dg] = inc;
        }
        __syncthreads();
        }
        uint32_t all;
        const uint32_t tv = tid < (int)kDigits ? tot_s[tid] : 0u;
        const uint32_t ex = scan256_excl(tv, s_w, &all);
        if (tid < (int)kDigits) {
            dst[tid] = ex;
            if (tid == kDigits - 1) dst[kDigits] = ex + tv;
            if (rev) cur[tid] -= tv;
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < kI; ++q) {
            if (act[q]) {
                const uint32_t pos = dst[d[q]] + (kStable ? gcnt[d[q] * kPGroups + q * kPWaves + w] : 0u) + rk[q];
                if constexpr (kPk) {
#pragma unroll
                    for (int x = 0; x < kW; ++x) s_pay[x][pos] = rec[q][x];
                } else {
                    u32x4 r4; r4.x = rec[q][0]; r4.y = rec[q][1]; r4.z = rec[q][2]; r4.w = rec[q][kW - 1];
                    s_rec[pos] = r4;
                }
                if (!kC) s_kj[kC ? 0 : pos] = v[q];
                if (!kDigKj) s_dig[kDigKj ? 0 : pos] = (uint8_t)d[q];
                if (kStable && pos_out)
                    pos_out[beg + sb + q * kPThreads + tid] =
                        (uint16_t)(cur[d[q]] - toff[(uint64_t)t * kDigits + d[q]] + (pos - dst[d[q]]));
            }
        }
        __syncthreads();
        const uint32_t staged = dst[kDigits];
#pragma unroll
        for (int q = 0; q < kI; ++q) {
            const uint32_t s = q * kPThreads + tid;
            if (s < staged) {
                if constexpr (kC) {                      // the digit from the staged record's own word 1
                    uint32_t o[kW];
#pragma unroll
                    for (int x = 0; x < kW; ++x) o[x] = s_pay[x][s];
                    const uint32_t dd = (o[1] >> shift) & (kDigits - 1);
                    store_payload<kPk>(orec, (uint64_t)cur[dd] + (s - dst[dd]), o);
                    continue;
                }
                const uint32_t dd = kDigKj ? (s_kj[s] >> shift) & (kDigits - 1) : s_dig[kDigKj ? 0 : s];
                const uint64_t g = (uint64_t)cur[dd] + (s - dst[dd]);
                if constexpr (kPk) {
                    uint32_t o[kW];
#pragma unroll
                    for (int x = 0; x < kW; ++x) o[x] = s_pay[x][s];
                    const uint32_t kj = s_kj[kC ? 0 : s];
                    if (kK8 && !kIn16 && !kC) o[1] |= (kj & 15u) << 28;
                    store_payload<kPk>(orec, g, o);
                    if (kC) {
                    } else if (kK8) {
                        static_cast<uint8_t*>(okj)[g] = (uint8_t)(kIn16 ? kj : kj >> 4);
                    } else {
                        static_cast<uint32_t*>(okj)[g] = kj;
                    }
                } else {
                    static_cast<u32x4*>(orec)[g] = s_rec[s];
                    static_cast<uint32_t*>(okj)[g] = s_kj[s];
                }
            }
        }
        __syncthreads();
        if (tid < (int)kDigits && !rev) cur[tid] += dst[tid + 1] - dst[tid];
    }
}

// The flagged form's level-2 scatter (packed records).  Final buckets must keep changeset order
// (the ordered resolve walks them in it).  A level-2 tile's records (level-1 order) already come in
// changeset order, and the records of one changeset have distinct keys, so only the changeset has
// to order records of a digit, not their positions: a sub-tile takes the records from its start
// whose changeset lies within kSegs of the start's (at most kS of them, a prefix), ranks them by
// (digit, changeset - first) with one LDS atomic per record (digit_count) and stages them
// digit-major, changeset-minor — the order-free scatter's cost, where the ballot multisplit
// (k_part_scatter2<true, ..>) pays nine ballots per record.  Changesets of fewer than kS / kSegs
// records in a tile just take more sub-tiles.  pos_out: each record's index in its tile's digit-major
// staging order (the tile's records of lower digits, from phist[t][*], plus its offset inside its
// digit run), at its level-1 index (16 bits) — what k_flags_back reads, with no digit needed.
// kC (the compact form): 12-B records in and out unchanged, the digit = the word's top byte (shift 24), no
// key column.
template <bool kK8, bool kIn16, bool kC = false>
__global__ __launch_bounds__(kPThreads) void k_part_scatter2_seg(
    const Rec12* __restrict__ irec, const void* __restrict__ ikj, TileMap tm, uint32_t shift,
    const uint32_t* __restrict__ toff, Rec12* __restrict__ orec, void* __restrict__ okj, uint32_t xper,
    uint32_t jmask, uint16_t* __restrict__ pos_out, const uint32_t* __restrict__ phist)
{
    static_assert(!kIn16 || kK8, "2-B key input gives 1-B key output");
    constexpr int kI = 8;
    constexpr uint32_t kS = kPThreads * kI;               // 8192 records per sub-tile at most
    constexpr uint32_t kSegs = 16, kCnt = kDigits * kSegs;
    static_assert(kCnt == 4 * kPThreads, "scan: 4 counters per thread");
    __shared__ uint32_t cnt[kCnt];                        // 16 KB: [changeset][digit] counts -> starts
    __shared__ uint32_t cur[kDigits];
    __shared__ uint32_t t0[kDigits];
    __shared__ uint32_t s_w[kPWaves];
    __shared__ uint32_t s_pay[3][kS];                     // 96 KB
    __shared__ uint32_t s_kj[kC ? 1 : kS];                // 32 KB (kC: the staged word 1 is the key word)
    const uint32_t t = xcd_tile(blockIdx.x, xper, xper != 0);
    if (t >= tm.tbase[tm.nseg]) return;
    uint32_t seg, len;
    uint64_t beg;
    tile_info(tm, t, &seg, &beg, &len);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    {   // t0[d] = toff[t][d] - (the tile's records of digits < d): cur[d] - t0[d] is a staging index
        uint32_t all;
        const uint32_t hv = pos_out && tid < (int)kDigits ? phist[(uint64_t)t * kDigits + tid] : 0u;
        const uint32_t ex = scan256_excl(hv, s_w, &all);
        if (tid < (int)kDigits) {
            cur[tid] = toff[(uint64_t)t * kDigits + tid];
            t0[tid] = cur[tid] - ex;
        }
    }
    for (uint32_t sb = 0; sb < len;) {
        uint32_t rec[kI][3], v[kI], idx[kI], slot[kI];
        bool act[kI];
        const uint32_t f0 = irec[beg + sb].a & jmask;    // the sub-tile's first changeset field
#pragma unroll
        for (int q = 0; q < kI; ++q) {
            const uint32_t i = sb + q * kPThreads + tid;
            const bool in = i < len;
            const uint64_t gi = beg + (in ? i : sb);
            const Rec12 r = irec[gi];
            rec[q][0] = r.a; rec[q][1] = r.b; rec[q][2] = r.c;
            v[q] = kC ? r.b
                 : kIn16 ? (uint32_t)__builtin_nontemporal_load(static_cast<const uint16_t*>(ikj) + gi)
                         : __builtin_nontemporal_load(static_cast<const uint32_t*>(ikj) + gi);
            const uint32_t sg = f0 - (r.a & jmask);      // fields fall as changesets rise
            act[q] = in && sg < kSegs;
            idx[q] = (sg & (kSegs - 1)) * kDigits + ((v[q] >> shift) & (kDigits - 1));   // bank = digit
        }
        for (uint32_t x = tid; x < kCnt; x += kPThreads) cnt[x] = 0;
        __syncthreads();
#pragma unroll
        for (int q = 0; q < kI; ++q) slot[q] = digit_count(cnt, idx[q], act[q], lane);
        __syncthreads();
        // exclusive scan of the 4096 counters in digit-major, changeset-minor order: thread t takes
        // digit t / 4, changesets 4 (t % 4) .. + 3
        const uint32_t sd = (uint32_t)tid >> 2, s4 = ((uint32_t)tid & 3u) * 4u;
        uint32_t c0 = cnt[s4 * kDigits + sd], c1 = cnt[(s4 + 1) * kDigits + sd];
        uint32_t c2 = cnt[(s4 + 2) * kDigits + sd], c3 = cnt[(s4 + 3) * kDigits + sd];
        const uint32_t sum = c0 + c1 + c2 + c3;
        uint32_t inc = sum;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t u = __shfl_up(inc, off, 64);
            if (lane >= off) inc += u;
        }
        if (lane == 63) s_w[w] = inc;
        __syncthreads();
        uint32_t wp = 0, n = 0;
#pragma unroll
        for (int k = 0; k < kPWaves; ++k) {
            const uint32_t x = s_w[k];
            wp += k < w ? x : 0u;
            n += x;
        }
        uint32_t run = wp + inc - sum;                    // (each thread rewrites the four counts it read)
        cnt[s4 * kDigits + sd] = run; run += c0;
        cnt[(s4 + 1) * kDigits + sd] = run; run += c1;
        cnt[(s4 + 2) * kDigits + sd] = run; run += c2;
        cnt[(s4 + 3) * kDigits + sd] = run;
        __syncthreads();
#pragma unroll
        for (int q = 0; q < kI; ++q) {
            if (!act[q]) continue;
            const uint32_t pos = cnt[idx[q]] + slot[q];
            s_pay[0][pos] = rec[q][0];
            s_pay[1][pos] = rec[q][1];
            s_pay[2][pos] = rec[q][2];
            if (!kC) s_kj[kC ? 0 : pos] = v[q];
            const uint32_t d = idx[q] & (kDigits - 1);
            if (pos_out) pos_out[beg + sb + q * kPThreads + tid] = (uint16_t)(cur[d] - t0[d] + (pos - cnt[d]));
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < kI; ++q) {
            const uint32_t s2 = q * kPThreads + tid;
            if (s2 >= n) continue;
            Rec12 o;
            o.a = s_pay[0][s2];
            o.b = s_pay[1][s2];
            o.c = s_pay[2][s2];
            const uint32_t kj = kC ? o.b : s_kj[kC ? 0 : s2];
            const uint32_t dd = (kj >> shift) & (kDigits - 1);
            const uint64_t g = (uint64_t)cur[dd] + (s2 - cnt[dd]);
            if (kK8 && !kIn16 && !kC) o.b |= (kj & 15u) << 28;
            orec[g] = o;
            if (kC) {
            } else if (kK8) {
                static_cast<uint8_t*>(okj)[g] = (uint8_t)(kIn16 ? kj : kj >> 4);
            } else {
                static_cast<uint32_t*>(okj)[g] = kj;
            }
        }
        __syncthreads();
        if (tid < (int)kDigits) cur[tid] += (tid + 1 < (int)kDigits ? cnt[tid + 1] : n) - cnt[tid];
        sb += n;
        __syncthreads();
    }
}

// Level 1 fast form: a level-1 tile never straddles a changeset and keys are distinct inside
// a changeset, so where a tile's records land inside one bucket is free — ranks come from one
// LDS atomic per record (digit_count), not from the stable ballot multisplit level 2 needs.
// kPk: payloads packed against the frame pf (the packed order-free form).  kPkIn: the input
// records are already packed (routed in by a sharded merge): lt holds the packed key, no rank.
// kK16 (packed, PackFrame::key4, two levels): the output key column holds key bits [4, 20) in 2 B
// and bits [0, 4) ride in the packed key's top 4 bits (14 B per level-1 record instead of 16).
// kVec: a thread's records come as 4 consecutive ones (one 16-B load per 4-B column, two for lt:
// 1 KB per wave instruction instead of 256 B), then 2 consecutive ones (8-B loads), the rest strided;
// a sub-tile's records are ranked order-free, so which thread holds which record does not matter.
// kPos (the flagged form, §"win flags" below): each record's level-1 position is also written at its
// input index as its index in the tile's digit-major staging order — the tile's records of lower digits
// (the exclusive prefix of phist[t][*]) plus its offset inside its digit run (output position -
// toff[t][digit]); < 2^16 — so the win flags can be carried back without the digit (k_flags_back).
// kC (the compact form, PackFrame::cb): the record's whole 20-bit bucket slot rides in its 64-bit word (bits
// [44, 64): kCKeyShift) and the key column holds only its level-2 digit (key bits [12, 20)) in 1 B — 13 B per
// level-1 record, and level 2 reads the 1-B column for its histogram only.
// kPT (with kPos, kVec; one window): the positions tile-strided — tile t's at pos_out[t * kPTile + i], i its record
// inside the tile — so a thread stores its records' positions straight from registers, 8-B / 4-B aligned (four
// consecutive records, a pair, a single), with no LDS staging pass; k_flags_back_pre<.., kPT> reads them so.
// kHot (the compact order-free form, two levels, one window; HotL1): the records of the first h.hot final buckets
// (slot >> 12 < h.hot) take level-1 digits of their own, 256 + (slot >> 12), whose output ranges come first —
// h.toff[t][b] from the scan of the hot tile histogram h.thist, starting at position 0 — and are written to
// h.orec, the level-2 record buffer, at those positions: they are in their final bucket after this one pass.  The
// ordinary digits' positions start at the hot total (level 2 writes nothing below it) and digit 0 holds only its
// slots >= h.hot * 4096.  Hot records write no digit column.
struct HotL1 {
    uint32_t hot = 0;                  // hot final buckets (<= 256)
    const uint32_t* toff = nullptr;    // [tiles][256] first position of the tile's records of hot bucket b
    const uint32_t* thist = nullptr;   // [tiles][256] their counts
    void* orec = nullptr;              // the level-2 record buffer
};

// exclusive scan over threads 0..511 (8 waves; every thread of the workgroup calls it); *total = the sum
__device__ inline uint32_t scan512_excl(uint32_t v, uint32_t* s_w /*[8]*/, uint32_t* total) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t u = __shfl_up(inc, off, 64);
        if (lane >= off) inc += u;
    }
    if (tid < 512 && lane == 63) s_w[w] = inc;
    __syncthreads();
    uint32_t x = lane < 8 ? s_w[lane] : 0u;              // the 8 wave sums, scanned by every wave's first lanes
#pragma unroll
    for (int off = 1; off < 8; off <<= 1) {
        const uint32_t u = __shfl_up(x, off, 64);
        if (lane >= off) x += u;
    }
    const int wu = __builtin_amdgcn_readfirstlane(w);
    *total = (uint32_t)__builtin_amdgcn_readlane((int)x, 7);
    const uint32_t wp = wu == 0 ? 0u : wu <= 8 ? (uint32_t)__builtin_amdgcn_readlane((int)x, wu - 1) : *total;
    return wp + inc - v;
}

// digit_count (crdt_merge.hip) with the wave's shared values read across lanes into scalars and the lane's rank
// inside the matching lanes counted by mbcnt: no lane id or lane mask kept in vector registers (the hot-bucket
// level 1 runs at its register cap).  The first lane of the match mask is the first active lane.
__device__ inline uint32_t digit_count_s(uint32_t* bins, uint32_t d, bool act) {
    const unsigned long long a = __ballot(act);
    if (!a) return 0;
    const int L = __ffsll((long long)a) - 1;
    const uint32_t d0 = (uint32_t)__builtin_amdgcn_readlane((int)d, L);
    const bool same = act && d == d0;
    const unsigned long long m = __ballot(same);
    const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
    uint32_t base = 0;
    if (same && below == 0) base = atomicAdd(&bins[d0], (uint32_t)__popcll(m));
    base = (uint32_t)__builtin_amdgcn_readlane((int)base, L);
    if (same) return base + below;
    return act ? atomicAdd(&bins[d], 1u) : 0u;
}

template <bool kPk, bool kPkIn, bool kK16, int kItems, bool kVec, bool kDigKj, bool kPos, bool kC, bool kPT, bool kHot>
__device__ __forceinline__ void part_scatter1_body(
    const uint32_t* __restrict__ keyw, const int64_t* __restrict__ lt, const uint32_t* __restrict__ rank,
    const uint32_t* __restrict__ val, TileMap tm, uint32_t jbase, Misc* __restrict__ misc, uint64_t cap,
    uint32_t shift, const uint32_t* __restrict__ toff, void* __restrict__ orec, void* __restrict__ okj,
    uint32_t xper, PackFrame pf, const uint32_t* __restrict__ thist,
    uint16_t* __restrict__ pos_out, const uint32_t* __restrict__ phist, KeyMap km, HotL1 hl)
{
    static_assert(!kK16 || kPk, "2-B key column: packed records only");
    static_assert(!kDigKj || kK16, "digit beside the 16-bit key: 2-B key columns only");
    static_assert(!kC || (kK16 && kDigKj && !kPkIn), "compact: one ctx's packed forms");
    static_assert(!kPT || (kPos && kVec && (kPThreads * kItems) % 8 == 0), "tile-strided positions: kVec groups");
    static_assert(!kHot || (kC && !kPos && kPThreads >= 512), "hot buckets: the compact order-free form");
    constexpr int kW = kPk ? 3 : 4;
    constexpr int kI = kItems;                            // records per thread per sub-tile
    constexpr int kS = kPThreads * kI;                    // records per LDS sub-tile
    constexpr int kND = kHot ? 2 * (int)kDigits : (int)kDigits;   // digits: the ordinary 256 (+ 256 hot ones)
    __shared__ uint32_t cur[kND];
    __shared__ uint32_t cnt[kND];
    __shared__ uint32_t dst[kND + 1];
    __shared__ uint32_t s_w[kHot ? 8 : 4];
    __shared__ u32x4 s_rec[kPk ? 1 : kS];             // wide: 112 KB (7 per thread)
    __shared__ uint32_t s_pay[kPk ? kW : 1][kPk ? kS : 1];   // packed: 84 KB
    __shared__ uint32_t s_kj[kS];                     //  28 KB
    __shared__ uint8_t s_dig[kDigKj ? 1 : kS];        //   7-8 KB (kDigKj: the digit rides in s_kj's top half)
    __shared__ uint32_t s_t0[kPos ? kDigits : 1];    // kPos: staging start - toff[t][*] of each digit
    __shared__ uint16_t s_pos[kPos && !kPT ? kS : 1];   // kPos: the sub-tile's positions in input order (14 KB)
    const uint32_t t = tm.tile0 + xcd_tile(blockIdx.x, xper, xper != 0);
    if (t >= tm.tbase[tm.nseg]) return;
    uint32_t seg, len;
    uint64_t beg;
    tile_info(tm, t, &seg, &beg, &len);
    const uint32_t jw = tm.seg_j[seg];                   // global changeset of this tile
    if (jw >= misc->stop) return;
    const int tid = threadIdx.x, lane = tid & 63;
    // thist (the tile histogram) given: odd tiles fill each digit's range from its end downwards,
    // so both lines a tile shares with its neighbours (which run beside it on the same XCD) are
    // written by the two tiles at about the same time — both at their first sub-tile or both at
    // their last — and meet in that XCD's L2 instead of reaching HBM as two partial writes
    const bool rev = thist && (t & 1u);
    if (tid < (int)kDigits)
        cur[tid] = toff[(uint64_t)t * kDigits + tid] + (rev ? thist[(uint64_t)t * kDigits + tid] : 0u);
    else if (kHot && tid < kND)
        cur[tid] = hl.toff[(uint64_t)t * kDigits + tid - kDigits] +
                   (rev ? hl.thist[(uint64_t)t * kDigits + tid - kDigits] : 0u);
    if constexpr (kPos) {                                // (a barrier precedes every read of s_t0)
        uint32_t all;
        const uint32_t hv = tid < (int)kDigits ? phist[(uint64_t)t * kDigits + tid] : 0u;
        const uint32_t ex = scan256_excl(hv, s_w, &all);
        if (tid < (int)kDigits) s_t0[kPos ? tid : 0] = ex - toff[(uint64_t)t * kDigits + tid];
    }
    bool bad = false, over = false;             // over: a rank at or above pf.rk_limit
    int64_t nl[kI];
    uint32_t nr[kI], nvl[kI], nk[kI];
    static_assert(!kVec || kI >= 4, "kVec: 4 consecutive records per thread");
    // kVec: records in groups of 4 consecutive ones per thread (16-B loads), then a group of 2
    // (8-B loads) and a single one as the item count leaves them
    constexpr int kG4 = kVec ? kI / 4 : 0, kP2 = kVec && kI % 4 >= 2 ? 1 : 0;
    // record index (inside the tile) of a thread's q-th record in the sub-tile at sb
    auto rec_index = [&](uint32_t sb, int q) -> uint32_t {
        if (q < 4 * kG4) return sb + (uint32_t)(q >> 2) * (4u * kPThreads) + (uint32_t)tid * 4u + (uint32_t)(q & 3);
        const uint32_t b2 = sb + 4u * kG4 * kPThreads;
        if (kP2 && q < 4 * kG4 + 2) return b2 + (uint32_t)tid * 2u + (uint32_t)(q - 4 * kG4);
        return kVec ? b2 + 2u * kP2 * kPThreads + (uint32_t)(q - 4 * kG4 - 2 * kP2) * kPThreads + tid
                    : sb + (uint32_t)q * kPThreads + tid;
    };
    auto load1 = [&](uint32_t sb, int q) {
        const uint32_t i = rec_index(sb, q);
        const uint64_t gi = beg + (i < len ? i : 0);
        nl[q] = __builtin_nontemporal_load(lt + gi);
        nr[q] = kPkIn ? 0u : __builtin_nontemporal_load(rank + gi);
        nvl[q] = __builtin_nontemporal_load(val + gi);
        nk[q] = __builtin_nontemporal_load(keyw + gi);
    };
    auto load_sub = [&](uint32_t sb) {
#pragma unroll
        for (int g4 = 0; g4 < kG4; ++g4) {
            const int q = 4 * g4;
            const uint32_t i0 = rec_index(sb, q);
            if (i0 + 4u <= len) {                        // whole group in range: vector loads
                const uint64_t g = beg + i0;
                const u32x4u kv = *reinterpret_cast<const u32x4u*>(keyw + g);
                const u32x4u vv = *reinterpret_cast<const u32x4u*>(val + g);
                const u32x4u l0 = *reinterpret_cast<const u32x4u*>(lt + g);
                const u32x4u l1 = *reinterpret_cast<const u32x4u*>(lt + g + 2);
                nk[q] = kv.x; nk[q + 1] = kv.y; nk[q + 2] = kv.z; nk[q + 3] = kv.w;
                nvl[q] = vv.x; nvl[q + 1] = vv.y; nvl[q + 2] = vv.z; nvl[q + 3] = vv.w;
                nl[q] = (int64_t)(((uint64_t)l0.y << 32) | l0.x); nl[q + 1] = (int64_t)(((uint64_t)l0.w << 32) | l0.z);
                nl[q + 2] = (int64_t)(((uint64_t)l1.y << 32) | l1.x); nl[q + 3] = (int64_t)(((uint64_t)l1.w << 32) | l1.z);
                if constexpr (!kPkIn) {
                    const u32x4u rv = *reinterpret_cast<const u32x4u*>(rank + g);
                    nr[q] = rv.x; nr[q + 1] = rv.y; nr[q + 2] = rv.z; nr[q + 3] = rv.w;
                } else {
                    nr[q] = nr[q + 1] = nr[q + 2] = nr[q + 3] = 0u;
                }
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) load1(sb, q + j);
            }
        }
        if constexpr (kP2 != 0) {
            const int q = 4 * kG4;
            const uint32_t i0 = rec_index(sb, q);
            if (i0 + 2u <= len) {                        // a pair: 8-B loads (16 B for lt)
                const uint64_t g = beg + i0;
                const u32x2u kv = *reinterpret_cast<const u32x2u*>(keyw + g);
                const u32x2u vv = *reinterpret_cast<const u32x2u*>(val + g);
                const u32x4u l0 = *reinterpret_cast<const u32x4u*>(lt + g);
                nk[q] = kv.x; nk[q + 1] = kv.y;
                nvl[q] = vv.x; nvl[q + 1] = vv.y;
                nl[q] = (int64_t)(((uint64_t)l0.y << 32) | l0.x); nl[q + 1] = (int64_t)(((uint64_t)l0.w << 32) | l0.z);
                if constexpr (!kPkIn) {
                    const u32x2u rv = *reinterpret_cast<const u32x2u*>(rank + g);
                    nr[q] = rv.x; nr[q + 1] = rv.y;
                } else {
                    nr[q] = nr[q + 1] = 0u;
                }
            } else {
                load1(sb, q);
                load1(sb, q + 1);
            }
        }
#pragma unroll
        for (int q = 4 * kG4 + 2 * kP2; q < kI; ++q) load1(sb, q);
    };
    load_sub(0);
    for (uint32_t sb = 0; sb < len; sb += kS) {
        if (tid < kND) cnt[tid] = 0;
        uint32_t rec[kI][kW];
        uint32_t k[kI], d[kI], slot[kI];
        bool act[kI];
#pragma unroll
        for (int q = 0; q < kI; ++q) {
            act[q] = rec_index(sb, q) < len;
            // a rank at or over the declared bound (flagged before the rank register is reused;
            // a record whose key is also out of range fails the call either way)
            if (kPk && !kPkIn) over |= act[q] && nr[q] >= pf.rk_limit;
            if constexpr (kPk) {
                int64_t lq = nl[q];
                uint64_t pk;
                pk = kPkIn ? (uint64_t)nl[q] : pack_record<kC>(pf, lq, nr[q], jw - jbase);
                rec[q][0] = (uint32_t)pk;
                rec[q][1] = (uint32_t)(pk >> 32);
                rec[q][kW - 1] = nvl[q];
            } else {
                rec[q][0] = (uint32_t)nl[q];
                rec[q][1] = (uint32_t)((uint64_t)nl[q] >> 32);
                rec[q][2] = nr[q];
                rec[q][kW - 1] = nvl[q];
            }
            k[q] = nk[q];
        }
        if (sb + kS < len) load_sub(sb + kS);
        __syncthreads();                                 // cnt zeroed; previous sub-tile written out
#pragma unroll
        for (int q = 0; q < kI; ++q) {
            const uint32_t sl = k[q] >> km.gsh;          // the key's slot (its id on one ctx)
            bad |= act[q] && sl >= cap;
            act[q] = act[q] && sl < cap;
            d[q] = km_digit(km, k[q], shift);
            if (kHot) d[q] = (sl >> kSBits) < hl.hot ? kDigits + (sl >> kSBits) : d[q];
            if (kC) {
                rec[q][1] |= (sl & 0xFFFFFu) << (kCKeyShift - 32);
                k[q] = (sl >> 12) & 0xFFu;
                if (kHot) k[q] |= d[q] << 16;            // (the staged word already: d[] is not kept in registers)
            } else if (kK16) {
                rec[q][1] |= (sl & 15u) << 28;
                k[q] = (sl >> 4) & 0xFFFFu;
            } else {
                k[q] = (sl & kKeyLoMask) | ((jw - jbase) << kJShift);
            }
            slot[q] = kHot ? digit_count_s(cnt, d[q], act[q]) : digit_count(cnt, d[q], act[q], lane);
        }
        __syncthreads();
        uint32_t all;
        const uint32_t tv = tid < kND ? cnt[tid] : 0u;
        const uint32_t ex = kHot ? scan512_excl(tv, s_w, &all) : scan256_excl(tv, s_w, &all);
        if (tid < kND) {
            dst[tid] = ex;
            if (tid == kND - 1) dst[kND] = ex + tv;
            if (rev) cur[tid] -= tv;                     // this sub-tile's chunk ends where the last began
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < kI; ++q) {
            if (act[q]) {
                const uint32_t pos = dst[kHot ? k[q] >> 16 : d[q]] + slot[q];
                if constexpr (kPk) {
#pragma unroll
                    for (int x = 0; x < kW; ++x) s_pay[x][pos] = rec[q][x];
                } else {
                    u32x4 r4; r4.x = rec[q][0]; r4.y = rec[q][1]; r4.z = rec[q][2]; r4.w = rec[q][kW - 1];
                    s_rec[pos] = r4;
                }
                if (kHot) {
                    s_kj[pos] = k[q];
                } else if (kDigKj) {
                    s_kj[pos] = k[q] | (d[q] << 16);            // one LDS write for key and digit
                } else {
                    s_kj[pos] = k[q];
                    s_dig[kDigKj ? 0 : pos] = (uint8_t)d[q];
                }
                // kPos: staging index = tile prefix + cur[d] + slot - toff[t][d] (cur final here), staged in
                // input order and written below as 16-B vectors
                if constexpr (kPos && !kPT)
                    s_pos[kPos && !kPT ? rec_index(sb, q) - sb : 0] =
                        (uint16_t)(cur[d[q]] + slot[q] + s_t0[kPos ? d[q] : 0]);
            }
        }
        if constexpr (kPT) {         // tile-strided positions straight from registers
            uint32_t pp[kI];
#pragma unroll
            for (int q = 0; q < kI; ++q) pp[q] = act[q] ? (cur[d[q]] + slot[q] + s_t0[kPos ? d[q] : 0]) & 0xFFFFu : 0u;
            uint16_t* __restrict__ po = pos_out + (uint64_t)t * kPTile;
#pragma unroll
            for (int g4 = 0; g4 < kG4; ++g4) {
                const int q = 4 * g4;
                const uint32_t i0 = rec_index(sb, q);
                if (i0 + 4u <= len) {
                    u32x2u v;
                    v.x = pp[q] | (pp[q + 1] << 16);
                    v.y = pp[q + 2] | (pp[q + 3] << 16);
                    *reinterpret_cast<u32x2u*>(po + i0) = v;
                } else {
#pragma unroll
                    for (int u = 0; u < 4; ++u)
                        if (i0 + u < len) po[i0 + u] = (uint16_t)pp[q + u];
                }
            }
            if constexpr (kP2 != 0) {
                const int q = 4 * kG4;
                const uint32_t i0 = rec_index(sb, q);
                if (i0 + 2u <= len) *reinterpret_cast<uint32_t*>(po + i0) = pp[q] | (pp[q + 1] << 16);
                else if (i0 < len) po[i0] = (uint16_t)pp[q];
            }
#pragma unroll
            for (int q = 4 * kG4 + 2 * kP2; q < kI; ++q) {
                const uint32_t i = rec_index(sb, q);
                if (i < len) po[i] = (uint16_t)pp[q];
            }
        }
        __syncthreads();
        const uint32_t staged = dst[kND];
        if constexpr (kPos && !kPT) {   // the sub-tile's positions: 8 per 16-B store on the aligned body
            const uint32_t ns = std::min<uint32_t>((uint32_t)kS, len - sb);
            uint16_t* __restrict__ po = pos_out + beg + sb;
            const uint32_t head = std::min<uint32_t>(ns, (8u - (uint32_t)(((uintptr_t)po >> 1) & 7u)) & 7u);
            const uint32_t nv = (ns - head) / 8u;
            if ((uint32_t)tid < head) po[tid] = s_pos[kPos ? tid : 0];
            for (uint32_t i = tid; i < nv; i += kPThreads) {
                const uint32_t b = head + i * 8u;
                u32x4 v;
                v.x = (uint32_t)s_pos[kPos ? b : 0] | ((uint32_t)s_pos[kPos ? b + 1 : 0] << 16);
                v.y = (uint32_t)s_pos[kPos ? b + 2 : 0] | ((uint32_t)s_pos[kPos ? b + 3 : 0] << 16);
                v.z = (uint32_t)s_pos[kPos ? b + 4 : 0] | ((uint32_t)s_pos[kPos ? b + 5 : 0] << 16);
                v.w = (uint32_t)s_pos[kPos ? b + 6 : 0] | ((uint32_t)s_pos[kPos ? b + 7 : 0] << 16);
                *reinterpret_cast<u32x4*>(po + b) = v;
            }
            const uint32_t tl = head + nv * 8u;
            if (tl + (uint32_t)tid < ns) po[tl + tid] = s_pos[kPos ? tl + tid : 0];
        }
#pragma unroll
        for (int q = 0; q < kI; ++q) {
            const uint32_t s = q * kPThreads + tid;
            if (s < staged) {
                const uint32_t kw = s_kj[s];
                const uint32_t dd = kDigKj ? kw >> 16 : s_dig[kDigKj ? 0 : s];
                const uint64_t g = (uint64_t)cur[dd] + (s - dst[dd]);
                if constexpr (kPk) {
                    uint32_t o[kW];
#pragma unroll
                    for (int x = 0; x < kW; ++x) o[x] = s_pay[x][s];
                    store_payload<kPk>(kHot && dd >= kDigits ? hl.orec : orec, g, o);
                } else {
                    static_cast<u32x4*>(orec)[g] = s_rec[s];
                }
                if (kHot && dd >= kDigits) continue;     // a final record: no digit column
                if (kC) static_cast<uint8_t*>(okj)[g] = (uint8_t)kw;
                else if (kK16) static_cast<uint16_t*>(okj)[g] = (uint16_t)kw;
                else static_cast<uint32_t*>(okj)[g] = kw;
            }
        }
        __syncthreads();
        if (tid < kND && !rev) cur[tid] += dst[tid + 1] - dst[tid];
    }
    // (kHot: the first lane from the exec mask here, so that no lane id stays in a register through the loop)
    const unsigned long long em = kHot ? __ballot(true) : 0ull;
    const bool l0 = kHot ? __builtin_amdgcn_mbcnt_hi((uint32_t)(em >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)em, 0u)) == 0u
                         : lane == 0;
    if (__any(bad) && l0) atomicOr(&misc->err, 1u);
    if (kPk && __any(over) && l0) atomicOr(&misc->err, 2u);
}

template <bool kPk, bool kPkIn = false, bool kK16 = false, int kItems = kL1Items, bool kVec = false,
          bool kDigKj = kK16, bool kPos = false, bool kC = false, bool kPT = false>
__global__ __launch_bounds__(kPThreads) void k_part_scatter1(
    const uint32_t* __restrict__ keyw, const int64_t* __restrict__ lt, const uint32_t* __restrict__ rank,
    const uint32_t* __restrict__ val, TileMap tm, uint32_t jbase, Misc* __restrict__ misc, uint64_t cap,
    uint32_t shift, const uint32_t* __restrict__ toff, void* __restrict__ orec, void* __restrict__ okj,
    uint32_t xper, PackFrame pf, const uint32_t* __restrict__ thist,
    uint16_t* __restrict__ pos_out = nullptr, const uint32_t* __restrict__ phist = nullptr,
    KeyMap km = KeyMap{0u, 8u})
{
    part_scatter1_body<kPk, kPkIn, kK16, kItems, kVec, kDigKj, kPos, kC, kPT, false>(
        keyw, lt, rank, val, tm, jbase, misc, cap, shift, toff, orec, okj, xper, pf, thist, pos_out, phist, km, HotL1{});
}

// The compact order-free form with hot buckets (HotL1 above); the same kernel name on purpose: it is the level-1
// scatter of the merges that take it.
template <int kItems = kL1Items>
__global__ __launch_bounds__(kPThreads) void k_part_scatter1(
    const uint32_t* __restrict__ keyw, const int64_t* __restrict__ lt, const uint32_t* __restrict__ rank,
    const uint32_t* __restrict__ val, TileMap tm, uint32_t jbase, Misc* __restrict__ misc, uint64_t cap,
    uint32_t shift, const uint32_t* __restrict__ toff, void* __restrict__ orec, void* __restrict__ okj,
    uint32_t xper, PackFrame pf, const uint32_t* __restrict__ thist, HotL1 hl)
{
    part_scatter1_body<true, false, true, kItems, true, true, false, true, false, true>(
        keyw, lt, rank, val, tm, jbase, misc, cap, shift, toff, orec, okj, xper, pf, thist, nullptr, nullptr,
        KeyMap{0u, 8u}, hl);
}

// ---------------------------------------------------------------------- resolve
// Work items: a bucket of n records is cut into parts of kRPart records (parts = 1 for
// all but hot buckets, so a Zipf head does not serialise on one CU).  Per item the
// state of every key of the bucket is {lt, rank, val, j}: j < kWindow is the window
// changeset of the record that set it, kJLocal = the local row, kJAbsent = no row.
//   k_bucket_items : item prefix over buckets (one workgroup)
//   k_resolve<true>: hot buckets only, each part folded alone (state starts absent,
//                    no counts) -> part state [item][key]
//   k_part_carry   : hot buckets, carry-in of part p = table row folded with parts < p
//   k_resolve<false>: every item from its carry-in (the table row for unsplit buckets):
//                    global order, n_present / n_won per record; the last part of a
//                    bucket writes the bucket's changed rows (mod = R_j).
constexpr uint32_t kRPart = 32 * kRChunk;         // 65,536 records per part
constexpr uint32_t kJLocal = 0xFFFFFFFFu;
constexpr uint32_t kJAbsent = 0xFFFFFFFEu;

struct KeyState {           // part states and carries, SoA per item (4096 keys each)
    int64_t* lt;
    uint32_t* rank;
    uint32_t* val;
    uint32_t* j;
};

__device__ inline uint32_t bucket_parts(const uint32_t* bstart, uint32_t b) {
    const uint32_t n = bstart[b + 1] - bstart[b];
    return (n + kRPart - 1) / kRPart;
}

// ibase[b] = first item of bucket b, ibase[nb] = items; hbase[b] = first part-state slot of
// bucket b (split buckets only), hbase[nb] = slots.  One workgroup per 1024 buckets, each
// thread one bucket; the items of all earlier buckets are re-counted by every workgroup from
// bstart (<= 256 KB of L2-resident reads), so no workgroup waits on another.  (One workgroup
// scanning all 2^16 buckets in LDS chunks took 106 us; a per-thread walk 140 us.)
// Also: misc->key_end = max(.., end of the last non-empty bucket) — every row the resolve writes
// lies below it (the table's high-water mark after the merge, crdt_ctx::hw).
// ebase (the map-side combine's emit, nullable): ebase[b] = sum over b' < b of min(kSKeys, records of b'),
// the first emit slot of bucket b (a bucket emits at most one entry per key, and no more than its records).
__global__ __launch_bounds__(1024) void k_bucket_items(const uint32_t* __restrict__ bstart, uint32_t nb,
                                                       uint32_t* __restrict__ ibase, uint32_t* __restrict__ hbase,
                                                       uint32_t* __restrict__ hot, Misc* __restrict__ misc,
                                                       uint32_t* __restrict__ ebase = nullptr)
{
    __shared__ uint32_t s_p[16], s_hp[16], s_cp[16], s_w[16], s_h[16], s_c[16], s_e[16], s_ep[16], s_ew[16];
    const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const uint32_t b0 = blockIdx.x * 1024u;
    auto parts = [&](uint32_t k) { return (bstart[k + 1] - bstart[k] + kRPart - 1) / kRPart; };
    auto eslots = [&](uint32_t k) { return std::min<uint32_t>(kSKeys, bstart[k + 1] - bstart[k]); };
    uint32_t pre = 0, hpre = 0, cpre = 0, epre = 0;
#pragma unroll 8
    for (uint32_t k = tid; k < b0; k += 1024) {        // b0 is a multiple of 1024: no tail
        const uint32_t np = parts(k);
        pre += np;
        hpre += np > 1 ? np : 0u;
        cpre += np > 1 ? 1u : 0u;
        if (ebase) epre += eslots(k);
    }
    const uint32_t k = b0 + tid;
    const uint32_t np = k < nb ? parts(k) : 0u, hp = np > 1 ? np : 0u, cp = np > 1 ? 1u : 0u;
    const uint32_t ep = ebase && k < nb ? eslots(k) : 0u;
    uint32_t inc = np, hinc = hp, cinc = cp, einc = ep;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t u = __shfl_up(inc, off, 64), hu = __shfl_up(hinc, off, 64), cu = __shfl_up(cinc, off, 64);
        const uint32_t eu = __shfl_up(einc, off, 64);
        if (lane >= (uint32_t)off) { inc += u; hinc += hu; cinc += cu; einc += eu; }
        pre += __shfl_xor(pre, off, 64);
        hpre += __shfl_xor(hpre, off, 64);
        cpre += __shfl_xor(cpre, off, 64);
        epre += __shfl_xor(epre, off, 64);
    }
    uint32_t kend = k < nb && bstart[k + 1] > bstart[k] ? (k + 1) << kSBits : 0u;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) kend = std::max(kend, (uint32_t)__shfl_xor(kend, off, 64));
    if (lane == 63) {
        s_w[w] = inc; s_h[w] = hinc; s_c[w] = cinc; s_p[w] = pre; s_hp[w] = hpre; s_cp[w] = cpre;
        s_ew[w] = einc; s_ep[w] = epre;
    }
    if (lane == 0) s_e[w] = kend;
    __syncthreads();
    if (tid == 0) {
        for (uint32_t q = 1; q < 16; ++q) kend = std::max(kend, s_e[q]);
        if (kend) atomicMax(&misc->key_end, (unsigned long long)kend);
    }
    uint32_t run = inc - np, hrun = hinc - hp, crun = cinc - cp, erun = einc - ep;
    for (uint32_t q = 0; q < 16; ++q) {
        run += s_p[q] + (q < w ? s_w[q] : 0u);
        hrun += s_hp[q] + (q < w ? s_h[q] : 0u);
        crun += s_cp[q] + (q < w ? s_c[q] : 0u);
        erun += s_ep[q] + (q < w ? s_ew[q] : 0u);
    }
    if (k < nb) {
        if (ebase) ebase[k] = erun;
        ibase[k] = run;
        hbase[k] = hrun;
        if (cp) hot[1 + crun] = k;                     // split buckets, in bucket order
        if (k == nb - 1) { ibase[nb] = run + np; hbase[nb] = hrun + hp; hot[0] = crun + cp; }
    }
}

// Per-kernel item lists of the order-free packed resolve (round 6).  Its three kernels — the split buckets' part
// fold, the dense unsplit buckets, the sparse ones (k_resolve_sparse) — each ran one workgroup per item slot of the
// whole item range (nb + parts, ~67K on two levels), the other kinds' items and the empty slots exiting after a load
// or three; with 512-thread workgroups two or three per CU, cfg3's ~25K real items in 3 x 67K slots paid ~100-200 us
// of such exits per merge.  Here every unsplit bucket is classed once (its records, kRPart, sparse_t, hw — the
// kernels' own conditions) and the item ids of each kind are written in bucket order; the host reads the four
// counts and launches each kernel on exactly its list.  lists: [0] fold items, [1] dense items, [2] sparse items,
// [3] split buckets (hot[0]), [4] items (ibase[nb]); from [8] the fold list, the dense list and the sparse list, cap
// entries each.
constexpr uint32_t kListHead = 8;
__global__ __launch_bounds__(1024) void k_item_lists(const uint32_t* __restrict__ bstart, uint32_t nb,
                                                     const uint32_t* __restrict__ ibase,
                                                     const uint32_t* __restrict__ hbase,
                                                     const uint32_t* __restrict__ hot, uint64_t hw, uint32_t sparse_t,
                                                     uint32_t* __restrict__ lists, uint32_t cap)
{
    __shared__ uint32_t s_d[16], s_s[16], s_dw[16], s_sw[16];
    const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const uint32_t b0 = blockIdx.x * 1024u;
    auto kind = [&](uint32_t k) -> uint32_t {          // 0 none / split, 1 dense, 2 sparse
        const uint32_t n = bstart[k + 1] - bstart[k];
        if (n == 0 || n > kRPart) return 0u;
        return n < sparse_t && ((uint64_t)k << kSBits) < hw ? 2u : 1u;
    };
    uint32_t dpre = 0, spre = 0;
#pragma unroll 8
    for (uint32_t k = tid; k < b0; k += 1024) {        // earlier workgroups' buckets, re-counted (as k_bucket_items)
        const uint32_t c = kind(k);
        dpre += c == 1u;
        spre += c == 2u;
    }
    const uint32_t k = b0 + tid;
    const uint32_t c = k < nb ? kind(k) : 0u;
    const uint32_t dd = c == 1u, ss = c == 2u;
    uint32_t dinc = dd, sinc = ss;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t du = __shfl_up(dinc, off, 64), su = __shfl_up(sinc, off, 64);
        if (lane >= (uint32_t)off) { dinc += du; sinc += su; }
        dpre += __shfl_xor(dpre, off, 64);
        spre += __shfl_xor(spre, off, 64);
    }
    if (lane == 63) { s_dw[w] = dinc; s_sw[w] = sinc; s_d[w] = dpre; s_s[w] = spre; }
    __syncthreads();
    uint32_t drun = dinc - dd, srun = sinc - ss;
    for (uint32_t q = 0; q < 16; ++q) {
        drun += s_d[q] + (q < w ? s_dw[q] : 0u);
        srun += s_s[q] + (q < w ? s_sw[q] : 0u);
    }
    if (k >= nb) return;
    uint32_t* fl = lists + kListHead;
    const uint32_t n = bstart[k + 1] - bstart[k];
    if (n > kRPart) {                                   // a split bucket's parts, at its part-state slots
        const uint32_t np = (n + kRPart - 1) / kRPart, i0 = ibase[k], h0 = hbase[k];
        for (uint32_t p = 0; p < np; ++p) fl[h0 + p] = i0 + p;
    } else if (dd) {
        fl[cap + drun] = ibase[k];
    } else if (ss) {
        fl[2 * (size_t)cap + srun] = ibase[k];
    }
    if (k == nb - 1) {
        lists[0] = hbase[nb];
        lists[1] = drun + dd;
        lists[2] = srun + ss;
        lists[3] = hot[0];
        lists[4] = ibase[nb];
    }
}

#ifdef CRDT_PROF_RESOLVE
// phase clocks of k_resolve<false> (wall_clock64, 100 MHz), summed over workgroups:
// [0] init, [1] chunk phase A (link + prefetch issue), [2] phase B (walk), [3] final rows,
// [4] items, [5] chunks
__device__ unsigned long long g_rprof[8];
__device__ unsigned long long g_item_dur[1 << 18];     // per item: duration (10 ns) << 24 | chunks << 8 | part flag
#define RPROF(i, v) do { if (!kFold && threadIdx.x == 0) atomicAdd(&g_rprof[i], (unsigned long long)(v)); } while (0)
#define RPROFMAX(i, v) do { if (!kFold && threadIdx.x == 0) atomicMax(&g_rprof[i], (unsigned long long)(v)); } while (0)
#else
#define RPROF(i, v) do { } while (0)
#define RPROFMAX(i, v) do { } while (0)
#endif

// Order-free fold (kFree, the sorted path without per-record counts): records of a bucket may
// come in any order, so ties on (lt, rank) are decided by the changeset — the earlier one wins,
// the local row before every changeset (crdt.dart:83-84 applied in changeset order).
__device__ inline uint32_t jkey(uint32_t j) { return j == 0xFFFFu || j == kJLocal ? 0u : j + 1u; }
__device__ inline bool beats_j(int64_t l, uint32_t r, uint32_t j, int64_t ol, uint32_t orr, uint32_t oj) {
    return l > ol || (l == ol && (r > orr || (r == orr && jkey(j) < jkey(oj))));
}

template <bool kFold, bool kFree = false>
__global__ __launch_bounds__(kRThreads) void k_resolve(
    const uint32_t* __restrict__ bstart, const uint32_t* __restrict__ ibase, const uint32_t* __restrict__ hbase,
    const uint32_t* __restrict__ item_bucket, uint32_t nb, const u32x4* __restrict__ irec, const uint32_t* __restrict__ ikj, Table table,
    uint64_t cap, const int64_t* __restrict__ Rj, uint32_t jbase, KeyState ps, KeyState carry,
    Misc* __restrict__ misc)
{
    __shared__ int64_t st_lt[kSKeys];          // 32 KB
    __shared__ uint32_t st_rank[kSKeys];       // 16 KB
    __shared__ uint32_t st_val[kSKeys];        // 16 KB
    __shared__ uint16_t st_j[kSKeys];          //  8 KB: window changeset, 0xFFFF local, 0xFFFE absent
    __shared__ uint32_t head[kSKeys];          // 16 KB: (chunk tag << 11) | chunk index
    __shared__ int64_t c_lt[kRChunk];          // 16 KB
    __shared__ uint32_t c_rank[kRChunk];       //  8 KB
    __shared__ uint32_t c_next[kRChunk];       //  8 KB
    __shared__ uint16_t c_j[kFree ? kRChunk : 2];   // 4 KB: window changeset of each chunk record
    const uint32_t item = blockIdx.x;
    if (item >= ibase[nb]) return;
    if (misc->err & 1u) return;                      // a key id out of range: store nothing
    const uint32_t b = item_bucket[item];
    const uint32_t nparts = ibase[b + 1] - ibase[b];
    const uint32_t part = item - ibase[b];
    if (kFold && nparts <= 1) return;
    if (kFree && !kFold && nparts > 1) return;       // k_part_carry<true> writes split buckets' rows
    const uint32_t s = bstart[b] + part * kRPart;
    const uint32_t e = std::min<uint32_t>(bstart[b + 1], s + kRPart);
    const int tid = threadIdx.x;
#ifdef CRDT_PROF_RESOLVE
    uint64_t pt = wall_clock64();
    const uint64_t t_item = pt;
#endif
    const uint64_t row0 = (uint64_t)b << kSBits;
    const uint32_t nk = (uint32_t)std::min<uint64_t>(kSKeys, cap - row0);
    // records: three register buffers in rotation — chunk c is linked and walked while c + 1
    // lands and c + 2 is issued (one chunk in flight per CU left the loads' latency exposed);
    // the loop below is unrolled by three so no buffer is ever copied while a load targets it
    u32x4 ra[kRItems], rb[kRItems], rc[kRItems];
    uint32_t va[kRItems], vb[kRItems], vc[kRItems];
    auto issue = [&](uint32_t p, u32x4 (&r)[kRItems], uint32_t (&v)[kRItems]) {
        // unconditional (past the end it reloads record s): the number of loads in flight is
        // then the same on every path, so the compiler's waits count instead of draining
#pragma unroll
        for (int q = 0; q < kRItems; ++q) {
            const uint32_t i = p + q * kRThreads + tid;
            const uint32_t ii = i < e ? i : s;
            r[q] = __builtin_nontemporal_load(irec + ii);
            v[q] = __builtin_nontemporal_load(ikj + ii);
        }
    };
    auto prefetch = [&] {                       // the first two chunks, issued after the state
        issue(s, ra, va);                       // loads so that waiting for those keeps these in flight
        issue(s + kRChunk, rb, vb);
    };
    const uint64_t cbase = (uint64_t)(hbase[b] + part) * kSKeys;      // split buckets only
    // state init: every thread's 4 rows (or carries) are loaded before any is stored, so the
    // item starts with one memory round trip, not four (a store right after each load drained
    // the whole queue, prefetched chunks included)
    constexpr int kKPer = kSKeys / kRThreads;
    static_assert(kSKeys % kRThreads == 0, "keys per thread");
    if (kFold) {
        prefetch();
#pragma unroll
        for (int kk = 0; kk < kKPer; ++kk) {
            const uint32_t k = kk * kRThreads + tid;
            head[k] = 0;
            st_j[k] = 0xFFFE;
        }
    } else if (nparts == 1) {                   // a split bucket's last part rewrites these rows
        // (loads of a row index clamped below nk and used unconditionally, so the compiler
        // cannot sink each one into a branch of its own; keys >= nk stay absent)
        uint4 h[kKPer];
#pragma unroll
        for (int kk = 0; kk < kKPer; ++kk) {
            const uint32_t k = kk * kRThreads + tid;
            h[kk] = load_hot(table, row0 + (k < nk ? k : nk - 1));
        }
        prefetch();
#pragma unroll
        for (int kk = 0; kk < kKPer; ++kk) {
            const uint32_t k = kk * kRThreads + tid;
            head[k] = 0;
            st_lt[k] = (int64_t)(((uint64_t)h[kk].y << 32) | h[kk].x);
            st_rank[k] = h[kk].z;
            st_j[k] = (k < nk && (int32_t)h[kk].w >= 0) ? 0xFFFF : 0xFFFE;
        }
    } else {
        int64_t cl[kKPer];
        uint32_t cr[kKPer], cv[kKPer], cjj[kKPer];
#pragma unroll
        for (int kk = 0; kk < kKPer; ++kk) {
            const uint32_t k = kk * kRThreads + tid;
            const uint64_t ck = cbase + (k < nk ? k : nk - 1);
            cjj[kk] = carry.j[ck];
            cl[kk] = carry.lt[ck];
            cr[kk] = carry.rank[ck];
            cv[kk] = carry.val[ck];
        }
        prefetch();
#pragma unroll
        for (int kk = 0; kk < kKPer; ++kk) {
            const uint32_t k = kk * kRThreads + tid;
            head[k] = 0;
            st_lt[k] = cl[kk];
            st_rank[k] = cr[kk];
            st_val[k] = cv[kk];
            st_j[k] = k >= nk || cjj[kk] == kJAbsent ? 0xFFFE : cjj[kk] == kJLocal ? 0xFFFF : (uint16_t)cjj[kk];
        }
    }
    __syncthreads();
#ifdef CRDT_PROF_RESOLVE
    { const uint64_t now = wall_clock64(); RPROF(0, now - pt); RPROF(4, 1); pt = now; }
#endif
    uint32_t npres = 0, nwon = 0;
    uint32_t tag = 0;
    auto chunk = [&](uint32_t p0, const u32x4 (&r)[kRItems], const uint32_t (&v)[kRItems]) {
        ++tag;
        uint32_t key[kRItems], rr[kRItems], vv[kRItems], jw[kRItems], oldh[kRItems];
        int64_t ll[kRItems];
        bool act[kRItems];
#pragma unroll
        for (int q = 0; q < kRItems; ++q) {
            const uint32_t li = q * kRThreads + tid;
            act[q] = p0 + li < e;
            ll[q] = (int64_t)(((uint64_t)r[q].y << 32) | r[q].x);
            key[q] = v[q] & (kSKeys - 1);
            jw[q] = v[q] >> kJShift;
            rr[q] = r[q].z;
            vv[q] = r[q].w;
            oldh[q] = 0;
            if (act[q]) {
                c_lt[li] = ll[q];
                c_rank[li] = rr[q];
                if (kFree) c_j[kFree ? li : 0] = (uint16_t)jw[q];
                oldh[q] = atomicExch(&head[key[q]], (tag << 11) | li);
                c_next[li] = oldh[q];
            }
        }
        __syncthreads();
#ifdef CRDT_PROF_RESOLVE
        { const uint64_t now = wall_clock64(); RPROF(1, now - pt); RPROF(5, 1); pt = now; }
#endif
        bool upd[kRItems];
#pragma unroll
        for (int q = 0; q < kRItems; ++q) {
            upd[q] = false;
            if (!act[q]) continue;
            const uint32_t li = q * kRThreads + tid;
            bool have = st_j[key[q]] != 0xFFFE;         // (bl, br) = max of state and earlier records
            int64_t bl = st_lt[key[q]];
            uint32_t br = st_rank[key[q]];
            bool later_gt = false;
            uint32_t h = head[key[q]];
            // the common case, the only record of its key in the chunk: no list to walk
            if (h == ((tag << 11) | li) && (oldh[q] >> 11) != tag) h = 0;
            while ((h >> 11) == tag) {
                const uint32_t m = h & (kRChunk - 1);
                if (kFree && m != li) {                  // any order: is q the chunk's best?
                    if (beats_j(c_lt[m], c_rank[m], c_j[kFree ? m : 0], ll[q], rr[q], jw[q])) later_gt = true;
                } else if (m != li) {
                    const int64_t ml = c_lt[m];
                    const uint32_t mr = c_rank[m];
                    if (m < li) {
                        if (!have || ml > bl || (ml == bl && mr > br)) { bl = ml; br = mr; }
                        have = true;
                    } else if (ml > ll[q] || (ml == ll[q] && mr > rr[q])) {
                        later_gt = true;
                    }
                }
                h = c_next[m];
            }
            const bool win = kFree ? (!have || beats_j(ll[q], rr[q], jw[q], bl, br, st_j[key[q]]))
                                   : (!have || ll[q] > bl || (ll[q] == bl && rr[q] > br));
            if (!kFold && !kFree) {
                npres += have ? 1u : 0u;
                nwon += win ? 1u : 0u;
            }
            upd[q] = win && !later_gt;
        }
        __syncthreads();
#ifdef CRDT_PROF_RESOLVE
        { const uint64_t now = wall_clock64(); RPROF(2, now - pt); RPROFMAX(6, now - pt); pt = now; }
#endif
        // state updates share the next chunk's first barrier interval: that phase writes
        // only c_* and head, which no thread reads until after its barrier
#pragma unroll
        for (int q = 0; q < kRItems; ++q) {
            if (upd[q]) {
                st_lt[key[q]] = ll[q];
                st_rank[key[q]] = rr[q];
                st_val[key[q]] = vv[q];
                st_j[key[q]] = (uint16_t)jw[q];
            }
        }
    };
    // main loop without exits inside the unrolled body: every iteration enters with the same
    // two chunks in flight, so the compiler's memory-count waits stay at "two chunks pending"
    // (with a break after each chunk it drained them at the loop head)
    const uint32_t nch = (e - s + kRChunk - 1) / kRChunk;
    uint32_t p0 = s, c = 0;
    for (; c + 3 <= nch; c += 3) {
        issue(p0 + 2 * kRChunk, rc, vc);
        chunk(p0, ra, va);
        p0 += kRChunk;
        issue(p0 + 2 * kRChunk, ra, va);
        chunk(p0, rb, vb);
        p0 += kRChunk;
        issue(p0 + 2 * kRChunk, rb, vb);
        chunk(p0, rc, vc);
        p0 += kRChunk;
    }
    if (c < nch) chunk(p0, ra, va);
    if (c + 1 < nch) chunk(p0 + kRChunk, rb, vb);
    __syncthreads();
    if (kFold) {
        for (uint32_t k = tid; k < kSKeys; k += kRThreads) {
            const uint16_t jj = st_j[k];
            ps.lt[cbase + k] = st_lt[k];
            ps.rank[cbase + k] = st_rank[k];
            ps.val[cbase + k] = st_val[k];
            ps.j[cbase + k] = jj == 0xFFFE ? kJAbsent : jj;
        }
        return;
    }
#ifdef CRDT_PROF_RESOLVE
    pt = wall_clock64();
#endif
    if (part + 1 == nparts) {
        for (uint32_t k = tid; k < nk; k += kRThreads) {
            const uint32_t jj = st_j[k];
            if (jj < kWindow) store_row(table, row0 + k, st_lt[k], st_rank[k], st_val[k], Rj[jbase + jj]);
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        npres += __shfl_xor(npres, off, 64);
        nwon += __shfl_xor(nwon, off, 64);
    }
    if ((tid & 63) == 0) {
        const int slot = (item * (kRThreads / 64) + (tid >> 6)) & (kCounterSlots - 1);
        if (npres) atomicAdd(&misc->present[slot], (unsigned long long)npres);
        if (nwon) atomicAdd(&misc->won[slot], (unsigned long long)nwon);
    }
#ifdef CRDT_PROF_RESOLVE
    RPROF(3, wall_clock64() - pt);
    RPROFMAX(7, wall_clock64() - t_item);
#ifdef CRDT_PROF_RESOLVE
    if (!kFold && tid == 0 && item < (1u << 18))
        g_item_dur[item] = ((wall_clock64() - t_item) << 24) | ((uint64_t)((e - s + kRChunk - 1) / kRChunk) << 8) |
                           (nparts > 1 ? 1u : 0u) | (part + 1 == nparts ? 2u : 0u);
#endif
#endif
}

// Carry-in of every part p of a hot bucket: the table row folded with the part
// states of parts 0..p-1 (a later part's best replaces the carry only if strictly
// greater: equal keeps the earlier record, crdt.dart:83-84).
// One workgroup row (blockIdx.y) per split bucket of the hot list k_bucket_items wrote.
// kFree (order-free sorted path): parts hold any changesets, so ties go to the earlier changeset
// (beats_j), and the last part's carry folded with that part is the final row, stored here.
template <bool kFree = false>
__global__ __launch_bounds__(256) void k_part_carry(const uint32_t* __restrict__ hot,
                                                    const uint32_t* __restrict__ ibase,
                                                    const uint32_t* __restrict__ hbase,
                                                    Table table, uint64_t cap, KeyState ps,
                                                    KeyState carry, const int64_t* __restrict__ Rj, uint32_t jbase,
                                                    const Misc* __restrict__ misc)
{
    if (blockIdx.y >= hot[0]) return;
    if (misc->err & 1u) return;
    const uint32_t b = hot[1 + blockIdx.y];
    const uint32_t np = ibase[b + 1] - ibase[b], i0 = hbase[b];
    const uint32_t k = blockIdx.x * 256 + threadIdx.x;
    const uint64_t row0 = (uint64_t)b << kSBits;
    if (row0 + k >= cap) return;
    const uint4 h = load_hot(table, row0 + k);
    int64_t l = (int64_t)(((uint64_t)h.y << 32) | h.x);
    uint32_t r = h.z, v = 0, j = (int32_t)h.w >= 0 ? kJLocal : kJAbsent;
    // parts are folded in batches of 8 whose state loads are all issued before the batch's
    // carries are stored (the loads do not depend on the fold; one round trip per batch)
    constexpr uint32_t kB = 8;
    for (uint32_t p0 = 0; p0 < np; p0 += kB) {
        int64_t bl[kB];
        uint32_t br[kB], bv[kB], bj[kB];
#pragma unroll
        for (uint32_t q = 0; q < kB; ++q) {
            const uint32_t p = p0 + q;
            bj[q] = kJAbsent;
            bl[q] = 0;                                 // (defined even where unused: the fold below
            br[q] = bv[q] = 0;                         // is compiled into selects that read them)
            if (p > 0 && p < np) {
                const uint64_t src = (uint64_t)(i0 + p - 1) * kSKeys + k;
                bj[q] = ps.j[src];
                bl[q] = ps.lt[src];
                br[q] = ps.rank[src];
                bv[q] = ps.val[src];
            }
        }
#pragma unroll
        for (uint32_t q = 0; q < kB; ++q) {
            const uint32_t p = p0 + q;
            if (p >= np) break;
            bool take = bj[q] != kJAbsent;
            if (take && j != kJAbsent) {
                if (kFree) {
                    const uint32_t kq = jkey(bj[q]), kc = jkey(j);
                    take = bl[q] > l || (bl[q] == l && (br[q] > r || (br[q] == r && kq < kc)));
                } else {
                    take = bl[q] > l || (bl[q] == l && br[q] > r);
                }
            }
            if (take) { l = bl[q]; r = br[q]; v = bv[q]; j = bj[q]; }
            const uint64_t dst = (uint64_t)(i0 + p) * kSKeys + k;
            carry.lt[dst] = l;
            carry.rank[dst] = r;
            carry.val[dst] = v;
            carry.j[dst] = j;
        }
    }
    if (!kFree) return;                                // k_resolve<false> resolves from the carries
    const uint64_t src = (uint64_t)(i0 + np - 1) * kSKeys + k;
    const uint32_t pj = ps.j[src];
    if (pj != kJAbsent) {
        const int64_t pl = ps.lt[src];
        const uint32_t pr = ps.rank[src];
        bool take = j == kJAbsent;
        if (!take) {
            const uint32_t kq = jkey(pj), kc = jkey(j);
            take = pl > l || (pl == l && (pr > r || (pr == r && kq < kc)));
        }
        if (take) { l = pl; r = pr; v = ps.val[src]; j = pj; }
    }
    if (j < kWindow) store_row(table, row0 + k, l, r, v, Rj[jbase + j]);
}

constexpr uint32_t kFill = 0x80808080u;          // every word of a never-written row (crdt_reserve)
constexpr int kQThreads = 512;                      // packed resolve: 48 KB of LDS, several per CU
constexpr int kQItems = 4;
constexpr int kQChunk = kQThreads * kQItems;        // 2048 records per chunk

// The map-side combine of a sharded merge (comm_path.inc): a rank folds its home records into one
// packed maximum per distinct key and emits (key, packed key, value handle) instead of rows.  Each
// emitting workgroup ("emit item") owns kSKeys slots of the output and counts what it wrote, also per
// owner rank (key % G) — no global atomics (one shared counter serialised ~2M waves: 94 ms measured).
constexpr uint32_t kEmitMaxOwners = 1024;      // = kRouteMaxRanks
struct EmitOut {
    uint32_t* key;
    uint64_t* pk;
    uint32_t* val;                             // emit slots: bucket b's from bbase[b], min(kSKeys, its records)
    const uint32_t* bbase;                     // [buckets] first slot of each bucket (k_bucket_items' ebase)
    uint32_t* ibase;                           // [emit items] first slot of each item (read by k_comb_scatter)
    uint32_t* icount;                          // [emit items] entries written (zeroed by the caller)
    uint32_t* ocount;                          // [emit items][G] entries per owner (zeroed by the caller)
    uint32_t G;
    uint32_t osh;                              // owner of an emitted key: key % G (0), or key >> osh (route_l1's
                                               // head fold: bucket rows numbered owner-major)
    uint32_t item0;                            // k_part_carry_packed's first emit item (after the resolve's)
    uint32_t n_items;                          // (host) emit items of the launch pair
};

// Append the lanes with e set to this workgroup's slots from `base` (one LDS atomic per wave) and count
// per owner.  A resolve item emits its bucket's keys (<= min(kSKeys, records)); a carry block of a split
// bucket its 256 keys at base + 256 x block.
__device__ inline void emit_local(const EmitOut& eo, uint64_t base0, bool e, uint32_t key, uint64_t pk, uint32_t val,
                                  uint32_t* s_ec, uint32_t* s_oc) {
    const unsigned long long m = __ballot(e);
    if (!m) return;
    const int lane = threadIdx.x & 63, L = __ffsll((long long)m) - 1;
    uint32_t base = 0;
    if (lane == L) base = atomicAdd(s_ec, (uint32_t)__popcll(m));
    base = __shfl(base, L, 64);
    if (e) {
        const uint64_t slot = base0 + base + (uint32_t)__popcll(m & ((1ull << lane) - 1));
        eo.key[slot] = key;
        eo.pk[slot] = pk;
        eo.val[slot] = val;
        atomicAdd(&s_oc[eo.osh ? key >> eo.osh : key % eo.G], 1u);
    }
}

// After the workgroup's last emit_local (and a barrier): its counts.
__device__ inline void emit_counts(const EmitOut& eo, uint32_t item, uint64_t base0, const uint32_t* s_ec,
                                   const uint32_t* s_oc) {
    if (threadIdx.x == 0) {
        eo.icount[item] = *s_ec;
        eo.ibase[item] = (uint32_t)base0;
    }
    for (uint32_t o = threadIdx.x; o < eo.G; o += blockDim.x) eo.ocount[(uint64_t)item * eo.G + o] = s_oc[o];
}

// kFold: split buckets only, each part folded alone from "absent" into the part state
// (packed key + value handle per key); otherwise unsplit buckets from their table rows, the
// changed rows written back.  Exits when the frame does not fit (the list form runs).
// kK8: records from k_part_scatter2<false, true, true> (key bits [4, 12) in a 1-B column, [0, 4) in
// the packed key's top bits); otherwise the key is the low 12 bits of the 4-B kj column.
// kEmit (unsplit buckets, hw = 0: every row absent): the bucket's maxima are emitted (EmitOut), no row
// is read or written.
// sparse_t (unsplit buckets, whole-line form): a bucket of fewer records than sparse_t does not load its
// 4096 rows up front — its records are folded from "absent", and only the keys that got a record read their
// row (the decision half) afterwards and store it when a record beats it.  A sparse bucket's rows are mostly
// untouched, so this reads ~one 64-B granule per touched key instead of the bucket's 96 KB and rewrites only
// the winners (partial lines) instead of every line (the Zipf tail of cfg3; DESIGN.md §5.2).
// kC (the compact form): the key's low 12 bits are the record word's bits [44, 56), the packed key bits [0, 44);
// no key column is read.
template <bool kFold, bool kWL = true, bool kK8 = false, bool kEmit = false, bool kC = false>
__global__ __launch_bounds__(kQThreads) void k_resolve_packed(
    const uint32_t* __restrict__ bstart, const uint32_t* __restrict__ ibase, const uint32_t* __restrict__ hbase,
    const uint32_t* __restrict__ item_bucket, uint32_t nb, const Rec12* __restrict__ irec,
    const void* __restrict__ ikj, Table table, uint64_t cap, uint64_t hw, const int64_t* __restrict__ Rj,
    uint32_t jbase, uint64_t* __restrict__ ps_key, uint32_t* __restrict__ ps_val, PackFrame f,
    const Misc* __restrict__ misc, EmitOut eo = EmitOut{}, uint32_t sparse_t = 0, bool sparse_skip = false,
    const uint32_t* __restrict__ ilist = nullptr)
{
    static_assert(!kEmit || (!kFold && !kWL), "emit: the unsplit-bucket pass, no row writes");
    __shared__ unsigned long long st[kSKeys];      // 32 KB
    __shared__ uint32_t st_val[kSKeys];            // 16 KB
    __shared__ uint32_t s_ec[1];                   // kEmit: this item's emitted entries, per owner
    __shared__ uint32_t s_oc[kEmit ? kEmitMaxOwners : 1];
    const uint32_t item = ilist ? ilist[blockIdx.x] : blockIdx.x;   // (k_item_lists: this kernel's items only)
    if (item >= ibase[nb]) return;
    if (misc->err & 3u) return;                   // a rank over the declared bound: store nothing
    // records of changesets >= stop take no part (the level-1 scatter has left them out; the map-side
    // combine's emit runs on the same records): changeset field 4096 - jw
    const uint32_t stop = misc->stop;
    const uint32_t jf_min = f.jwin - (stop > jbase ? std::min<uint32_t>(stop - jbase, f.jwin) : 0u);
    const uint64_t jmask = pack_jmask(f);
    const uint32_t b = item_bucket[item];
    const uint32_t nparts = ibase[b + 1] - ibase[b];
    const uint32_t part = item - ibase[b];
    if (kFold != (nparts > 1)) return;
    const uint32_t s = bstart[b] + part * kRPart;
    const uint32_t e = std::min<uint32_t>(bstart[b + 1], s + kRPart);
    const int tid = threadIdx.x;
    const uint64_t row0 = (uint64_t)b << kSBits;
    const uint32_t nk = (uint32_t)std::min<uint64_t>(kSKeys, cap - row0);
    constexpr int kKPer = kSKeys / kQThreads;
    Rec12 ra[kQItems], rb[kQItems];
    uint32_t va[kQItems], vb[kQItems];
    constexpr bool kKeep = !kFold && kWL;
    uint4 h[kFold ? 1 : kKPer];                   // the bucket's rows as loaded: the epilogue writes
    uint2 hx[kKeep ? kKPer : 1];                  // whole lines, unchanged rows from these
    const bool sparse = kKeep && !kEmit && e - s < sparse_t && row0 < hw;   // (uniform per workgroup)
    if (sparse && sparse_skip) return;                                        // k_resolve_sparse's bucket
    auto issue = [&](uint32_t p, Rec12 (&r)[kQItems], uint32_t (&v)[kQItems]) {
#pragma unroll
        for (int q = 0; q < kQItems; ++q) {
            const uint32_t i = p + q * kQThreads + tid;
            const uint32_t ii = i < e ? i : s;          // unconditional: same loads in flight on every path
            r[q] = irec[ii];
            v[q] = kC ? 0u
                 : kK8 ? (uint32_t)__builtin_nontemporal_load(static_cast<const uint8_t*>(ikj) + ii)
                       : __builtin_nontemporal_load(static_cast<const uint32_t*>(ikj) + ii);
        }
    };
    if (kFold || sparse) {
        issue(s, ra, va);
#pragma unroll
        for (int kk = 0; kk < kKPer; ++kk) st[kk * kQThreads + tid] = 0ull;
    } else {
#pragma unroll
        for (int kk = 0; kk < kKPer; ++kk) {              // rows >= hw are the fill: not read
            const uint32_t k = kk * kQThreads + tid;
            const uint64_t row = row0 + (k < nk ? k : nk - 1);
            const bool rd = row < hw;
            h[kk] = (!kEmit && rd) ? load_hot(table, row) : make_uint4(kFill, kFill, kFill, kFill);   // kEmit: no table
            if (kKeep) hx[kKeep ? kk : 0] = rd ? load_cold(table, row) : make_uint2(kFill, kFill);
        }
        issue(s, ra, va);
#pragma unroll
        for (int kk = 0; kk < kKPer; ++kk) {
            const uint32_t k = kk * kQThreads + tid;
            const int64_t l = (int64_t)(((uint64_t)h[kk].y << 32) | h[kk].x);
            st[k] = pack_local(f, k < nk && (int32_t)h[kk].w >= 0, l, h[kk].z);
        }
        if constexpr (kEmit) {
            if (tid == 0) s_ec[0] = 0;
            for (uint32_t o = tid; o < eo.G; o += kQThreads) s_oc[kEmit ? o : 0] = 0;
        }
    }
    __syncthreads();
    auto chunk = [&](uint32_t p0, const Rec12 (&r)[kQItems], const uint32_t (&v)[kQItems]) {
        uint64_t pk[kQItems];
        uint32_t key[kQItems];
        bool act[kQItems];
#pragma unroll
        for (int q = 0; q < kQItems; ++q) {
            if (kC) {
                key[q] = (r[q].b >> (kCKeyShift - 32)) & (kSKeys - 1);
                pk[q] = ((uint64_t)(r[q].b & ((1u << (kCKeyShift - 32)) - 1)) << 32) | r[q].a;
            } else if (kK8) {
                key[q] = (v[q] << 4) | (r[q].b >> 28);
                pk[q] = ((uint64_t)(r[q].b & 0x0FFFFFFFu) << 32) | r[q].a;
            } else {
                key[q] = v[q] & (kSKeys - 1);
                pk[q] = ((uint64_t)r[q].b << 32) | r[q].a;
            }
            act[q] = p0 + q * kQThreads + tid < e && (uint32_t)(pk[q] & jmask) > jf_min;
            if (act[q]) atomicMax(&st[key[q]], (unsigned long long)pk[q]);
        }
        __syncthreads();
        // the record equal to the chunk's new max stores its handle; a later chunk's atomics may
        // already have raised the max (then that chunk's winner stores after its own barrier,
        // which every thread reaches only after this store)
#pragma unroll
        for (int q = 0; q < kQItems; ++q)
            if (act[q] && st[key[q]] == pk[q]) st_val[key[q]] = r[q].c;
    };
    const uint32_t nch = (e - s + kQChunk - 1) / kQChunk;
    uint32_t p0 = s, c = 0;
    for (; c + 2 <= nch; c += 2) {                      // unrolled by two: no buffer copies
        issue(p0 + kQChunk, rb, vb);
        chunk(p0, ra, va);
        p0 += kQChunk;
        issue(p0 + kQChunk, ra, va);
        chunk(p0, rb, vb);
        p0 += kQChunk;
    }
    if (c < nch) chunk(p0, ra, va);
    __syncthreads();
    if (kFold) {
        const uint64_t cbase = (uint64_t)(hbase[b] + part) * kSKeys;
        for (uint32_t k = tid; k < kSKeys; k += kQThreads) {
            ps_key[cbase + k] = st[k];
            ps_val[cbase + k] = st_val[k];
        }
        return;
    }
    if constexpr (kEmit) {
        for (uint32_t k0 = 0; k0 < kSKeys; k0 += kQThreads) {
            const uint32_t k = k0 + tid;
            const uint64_t x = k < nk ? st[k] : 0ull;
            emit_local(eo, eo.bbase[b], k < nk && pack_is_record(f, x), (uint32_t)(row0 + k), x,
                       k < nk ? st_val[k] : 0u, s_ec, s_oc);
        }
        __syncthreads();
        emit_counts(eo, item, eo.bbase[b], s_ec, s_oc);
        return;
    }
    if (kKeep && sparse) {                        // the keys that got a record: their rows now
        // every touched row's load issued before the first compare (into the dense path's row registers,
        // unused here): one memory latency per thread instead of one per touched key
        uint64_t xs[kKeep ? kKPer : 1];
#pragma unroll
        for (int kk = 0; kk < kKPer; ++kk) {
            const uint32_t k = kk * kQThreads + tid;
            xs[kKeep ? kk : 0] = k < nk ? st[k] : 0ull;
            const uint64_t row = row0 + k;
            h[kk] = xs[kKeep ? kk : 0] != 0 && row < hw ? load_hot(table, row) : make_uint4(kFill, kFill, kFill, kFill);
        }
#pragma unroll
        for (int kk = 0; kk < kKPer; ++kk) {
            const uint32_t k = kk * kQThreads + tid;
            const uint64_t x = xs[kKeep ? kk : 0];
            if (x == 0) continue;
            const uint4 r = h[kk];
            const uint64_t loc = pack_local(f, (int32_t)r.w >= 0, (int64_t)(((uint64_t)r.y << 32) | r.x), r.z);
            if (!pack_is_record(f, x) || x <= loc) continue;
            store_row(table, row0 + k, pack_lt(f, x), pack_rank(f, x), st_val[k],
                      Rj[jbase + pack_jw(f, x)]);
        }
        return;
    }
    if (kKeep) {
        // whole lines: a wave covers 64 consecutive rows = 1536 B = 12 whole 128-B lines, all
        // written when any of the 64 changes — the unchanged rows from the prologue's registers —
        // so no line is written partially (a partial line costs HBM a read-modify-write; on a
        // fan-in nearly every such group holds a winner)
#pragma unroll
        for (int kk = 0; kk < kKPer; ++kk) {
            const uint32_t k = kk * kQThreads + tid;
            const uint64_t x = st[k];
            const bool win = k < nk && pack_is_record(f, x);
            if (!__ballot(win) || k >= nk) continue;
            uint4 o = h[kKeep ? kk : 0];
            uint2 ox = hx[kKeep ? kk : 0];
            if (win) {
                const uint32_t jw = pack_jw(f, x);
                const int64_t l = pack_lt(f, x);
                const int64_t m = Rj[jbase + jw];
                o = make_uint4((uint32_t)l, (uint32_t)((uint64_t)l >> 32), pack_rank(f, x),
                               (uint32_t)((uint64_t)m >> 32));
                ox = make_uint2((uint32_t)m, st_val[k]);
            }
            store_hc(table, row0 + k, o, ox);
        }
        return;
    }
    for (uint32_t k = tid; k < nk; k += kQThreads) {
        const uint64_t x = st[k];
        if (!pack_is_record(f, x)) continue;
        store_row(table, row0 + k, pack_lt(f, x), pack_rank(f, x), st_val[k],
                  Rj[jbase + pack_jw(f, x)]);
    }
}

// The sparse buckets of the packed order-free form (round 6), apart from the dense ones: an unsplit bucket of
// fewer records than sparse_t below the high-water mark.  k_resolve_packed's sparse branch runs them inside its
// 512-thread, 48-KB, 102-VGPR workgroups (the dense buckets' row registers): two per CU, and a sparse bucket's
// workgroup is short and latency-bound (its records, then its touched rows), so ~22K of them on cfg3's Zipf
// tail ran as ~40 rounds of mostly-waiting workgroups.  Here a 256-thread workgroup with only the 32-KB max table:
// its records fold into st[key] (one LDS 64-bit max each), and then the record holding its key's maximum — the
// packed key is unique per key within a bucket: one record per (key, changeset) — reads that key's row itself and
// stores the row when it wins; no value table, no sweep over the 4096 slots.  Records of changesets >= stop take
// no part.  Same decisions as k_resolve_packed's sparse branch (the row loaded and compared only for touched keys).
constexpr int kSpThreads = 256;
constexpr int kSpItems = 8;                          // 2048 records per round (= the default sparse_t)
template <bool kK8, bool kC>
__global__ __launch_bounds__(kSpThreads) void k_resolve_sparse(
    const uint32_t* __restrict__ bstart, const uint32_t* __restrict__ ibase, const uint32_t* __restrict__ item_bucket,
    uint32_t nb, const Rec12* __restrict__ irec, const void* __restrict__ ikj, Table table, uint64_t hw,
    const int64_t* __restrict__ Rj, uint32_t jbase, PackFrame f, const Misc* __restrict__ misc, uint32_t sparse_t,
    const uint32_t* __restrict__ ilist = nullptr)
{
    __shared__ unsigned long long st[kSKeys];      // 32 KB
    const uint32_t item = ilist ? ilist[blockIdx.x] : blockIdx.x;
    if (item >= ibase[nb]) return;
    if (misc->err & 3u) return;                   // a rank over the declared bound: store nothing
    const uint32_t b = item_bucket[item];
    if (ibase[b + 1] - ibase[b] != 1) return;     // split buckets: the part fold and carry
    const uint32_t s = bstart[b], e = bstart[b + 1];
    const uint64_t row0 = (uint64_t)b << kSBits;
    if (!(e - s < sparse_t && row0 < hw)) return; // dense: k_resolve_packed
    const uint32_t stop = misc->stop;
    const uint32_t jf_min = f.jwin - (stop > jbase ? std::min<uint32_t>(stop - jbase, f.jwin) : 0u);
    const uint64_t jmask = pack_jmask(f);
    const int tid = threadIdx.x;
#pragma unroll
    for (int kk = 0; kk < (int)(kSKeys / kSpThreads); ++kk) st[kk * kSpThreads + tid] = 0ull;
    constexpr uint32_t kRound = kSpThreads * kSpItems;
    const bool one = e - s <= kRound;             // one round: phase 2 reuses phase 1's registers
    Rec12 r[kSpItems];
    uint32_t v[kSpItems];
    auto load = [&](uint32_t p0) {
#pragma unroll
        for (int q = 0; q < kSpItems; ++q) {
            const uint32_t i = p0 + q * kSpThreads + tid;
            const uint32_t ii = i < e ? i : s;
            r[q] = irec[ii];
            v[q] = kC ? 0u
                 : kK8 ? (uint32_t)static_cast<const uint8_t*>(ikj)[ii]
                       : static_cast<const uint32_t*>(ikj)[ii];
        }
    };
    auto decode = [&](int q, uint32_t p0, uint32_t& key, uint64_t& pk) -> bool {
        if (kC) {
            key = (r[q].b >> (kCKeyShift - 32)) & (kSKeys - 1);
            pk = ((uint64_t)(r[q].b & ((1u << (kCKeyShift - 32)) - 1)) << 32) | r[q].a;
        } else if (kK8) {
            key = (v[q] << 4) | (r[q].b >> 28);
            pk = ((uint64_t)(r[q].b & 0x0FFFFFFFu) << 32) | r[q].a;
        } else {
            key = v[q] & (kSKeys - 1);
            pk = ((uint64_t)r[q].b << 32) | r[q].a;
        }
        return p0 + q * kSpThreads + tid < e && (uint32_t)(pk & jmask) > jf_min;
    };
    __syncthreads();                              // st zeroed
    for (uint32_t p0 = s; p0 < e; p0 += kRound) {
        load(p0);
#pragma unroll
        for (int q = 0; q < kSpItems; ++q) {
            uint32_t key;
            uint64_t pk;
            if (decode(q, p0, key, pk)) atomicMax(&st[key], (unsigned long long)pk);
        }
    }
    __syncthreads();
    for (uint32_t p0 = s; p0 < e; p0 += kRound) {
        if (!one) load(p0);
        uint4 h[kSpItems];
        bool win[kSpItems];
#pragma unroll
        for (int q = 0; q < kSpItems; ++q) {      // every winner's row load in flight before the first compare
            uint32_t key;
            uint64_t pk;
            win[q] = decode(q, p0, key, pk) && st[key] == pk;
            const uint64_t row = row0 + key;
            h[q] = win[q] && row < hw ? load_hot(table, row) : make_uint4(kFill, kFill, kFill, kFill);
        }
#pragma unroll
        for (int q = 0; q < kSpItems; ++q) {
            if (!win[q]) continue;
            uint32_t key;
            uint64_t pk;
            decode(q, p0, key, pk);
            const uint64_t loc = pack_local(f, (int32_t)h[q].w >= 0, (int64_t)(((uint64_t)h[q].y << 32) | h[q].x),
                                            h[q].z);
            if (!pack_is_record(f, pk) || pk <= loc) continue;
            store_row(table, row0 + key, pack_lt(f, pk), pack_rank(f, pk), r[q].c, Rj[jbase + pack_jw(f, pk)]);
        }
    }
}

// Split buckets of the packed form: per key, the table row folded with every part's state
// (the max packed key; its value handle), the row written when a record wins.
// kEmit: the map-side combine's split buckets (hw = 0): the folded maximum is emitted, not stored.
template <bool kEmit = false>
__global__ __launch_bounds__(256) void k_part_carry_packed(const uint32_t* __restrict__ hot,
                                                           const uint32_t* __restrict__ ibase,
                                                           const uint32_t* __restrict__ hbase,
                                                           Table table, uint64_t cap, uint64_t hw,
                                                           const uint64_t* __restrict__ ps_key,
                                                           const uint32_t* __restrict__ ps_val,
                                                           const int64_t* __restrict__ Rj, uint32_t jbase,
                                                           PackFrame f, const Misc* __restrict__ misc,
                                                           EmitOut eo = EmitOut{})
{
    if (blockIdx.y >= hot[0]) return;
    if (misc->err & 3u) return;
    const uint32_t b = hot[1 + blockIdx.y];
    const uint32_t np = ibase[b + 1] - ibase[b], i0 = hbase[b];
    const uint32_t k = blockIdx.x * 256 + threadIdx.x;
    const uint64_t row0 = (uint64_t)b << kSBits;
    if constexpr (kEmit) {                               // every lane reaches the wave's ballot
        __shared__ uint32_t s_ec[1];
        __shared__ uint32_t s_oc[kEmitMaxOwners];
        const uint32_t item = eo.item0 + blockIdx.y * gridDim.x + blockIdx.x;
        if (threadIdx.x == 0) s_ec[0] = 0;
        for (uint32_t o = threadIdx.x; o < eo.G; o += 256) s_oc[o] = 0;
        __syncthreads();
        const bool in = row0 + k < cap;
        uint64_t best = 0;
        uint32_t bv = 0;
        for (uint32_t p = 0; in && p < np; ++p) {
            const uint64_t v = ps_key[(uint64_t)(i0 + p) * kSKeys + k];
            if (v > best) { best = v; bv = ps_val[(uint64_t)(i0 + p) * kSKeys + k]; }
        }
        const uint64_t base0 = (uint64_t)eo.bbase[b] + blockIdx.x * 256u;
        emit_local(eo, base0, in && pack_is_record(f, best), (uint32_t)(row0 + k), best, bv, s_ec, s_oc);
        __syncthreads();
        emit_counts(eo, item, base0, s_ec, s_oc);
        return;
    }
    if (row0 + k >= cap) return;
    const uint4 h = row0 + k < hw ? load_hot(table, row0 + k) : make_uint4(kFill, kFill, kFill, kFill);
    uint64_t best = pack_local(f, (int32_t)h.w >= 0, (int64_t)(((uint64_t)h.y << 32) | h.x), h.z);
    uint32_t bp = UINT32_MAX;
    constexpr uint32_t kB = 8;                          // state loads of 8 parts in flight at once
    for (uint32_t p0 = 0; p0 < np; p0 += kB) {
        uint64_t v[kB];
#pragma unroll
        for (uint32_t q = 0; q < kB; ++q)
            v[q] = p0 + q < np ? ps_key[(uint64_t)(i0 + p0 + q) * kSKeys + k] : 0ull;
#pragma unroll
        for (uint32_t q = 0; q < kB; ++q)
            if (v[q] > best) { best = v[q]; bp = p0 + q; }
    }
    if (bp == UINT32_MAX || !pack_is_record(f, best)) return;
    store_row(table, row0 + k, pack_lt(f, best), pack_rank(f, best),
              ps_val[(uint64_t)(i0 + bp) * kSKeys + k], Rj[jbase + pack_jw(f, best)]);
}

// ---------------------------------------------------------------------- win flags (flagged form)
// Crdt.merge leaves the remote map holding exactly the records that won, and watch() emits one
// event per winner (crdt.dart:80-90, map_crdt.dart:33-39).  A record wins iff it beats its key's
// row AS LEFT BY every earlier changeset — the left-to-right maxima of the key's records in
// changeset order, not only the final winner — and the flag belongs at the record's input index.
// The flagged form keeps the packed 12-B records and adds three things:
//   * level 2 orders each digit's records by changeset (k_part_scatter2_seg: sub-tiles of records
//     within 16 changesets, ranked by (digit, changeset)), so every final bucket holds its records
//     in changeset order (level-1 tiles are single changesets placed in tile order);
//   * the resolve walks each bucket in that order (k_resolve_pflags): per 2048-record chunk the
//     same-key records are linked in LDS, and a record wins iff its packed key exceeds the key's
//     state before the chunk and every earlier same-key record of the chunk (the packed key orders
//     (lt, rank) and puts the earlier changeset first on a tie, crdt.dart:83-84); one flag byte per
//     record is written in level-2 order — coalesced.  Buckets over kRPart records are cut into
//     parts (changeset ranges, by the stable order): k_resolve_packed<true> folds each part to its
//     per-key maximum, k_part_cin_packed turns those into every part's carry-in (the row folded with
//     the parts before it), and each part then walks from its carry-in;
//   * the flags travel back through the partitions along the positions the scatters wrote
//     (k_flags_back, one pass per level: level 2 -> level 1 order, level 1 -> input order): each
//     tile stages its runs of flags in LDS and writes four flags per 4-B store, never a random
//     single-byte store.

// Atomic exchange of a 16-bit LDS word (a CAS on the 32-bit word holding it); returns the old value.
__device__ inline uint32_t lds_exch16(uint16_t* p, uint16_t v) {
    uint32_t* w = reinterpret_cast<uint32_t*>(reinterpret_cast<uintptr_t>(p) & ~(uintptr_t)3);
    const uint32_t sh = (reinterpret_cast<uintptr_t>(p) & 2u) * 8u;
    uint32_t old = *w, assumed;
    do {
        assumed = old;
        old = atomicCAS(w, assumed, (assumed & ~(0xFFFFu << sh)) | ((uint32_t)v << sh));
    } while (old != assumed);
    return (old >> sh) & 0xFFFFu;
}

// Carry-in of every part of a split bucket: (packed state, value handle, key present) before it.
__global__ __launch_bounds__(256) void k_part_cin_packed(const uint32_t* __restrict__ hot,
                                                         const uint32_t* __restrict__ ibase,
                                                         const uint32_t* __restrict__ hbase,
                                                         Table table, uint64_t cap, uint64_t hw,
                                                         const uint64_t* __restrict__ ps_key,
                                                         const uint32_t* __restrict__ ps_val, PackFrame f,
                                                         const Misc* __restrict__ misc,
                                                         uint64_t* __restrict__ cin_key, uint32_t* __restrict__ cin_val,
                                                         uint8_t* __restrict__ cin_pres)
{
    if (blockIdx.y >= hot[0]) return;
    if (misc->err & 3u) return;
    const uint32_t b = hot[1 + blockIdx.y];
    const uint32_t np = ibase[b + 1] - ibase[b], i0 = hbase[b];
    const uint32_t k = blockIdx.x * 256 + threadIdx.x;
    const uint64_t row0 = (uint64_t)b << kSBits;
    const bool in = row0 + k < cap;
    const uint4 h = in && row0 + k < hw ? load_hot(table, row0 + k) : make_uint4(kFill, kFill, kFill, kFill);
    const bool vis = in && (int32_t)h.w >= 0;
    uint64_t best = pack_local(f, vis, (int64_t)(((uint64_t)h.y << 32) | h.x), h.z);
    uint32_t bv = 0xFFFFFFFFu;
    uint8_t pr = vis ? 1 : 0;
    for (uint32_t p = 0; p < np; ++p) {
        const uint64_t ix = (uint64_t)(i0 + p) * kSKeys + k;
        cin_key[ix] = best;
        cin_val[ix] = bv;
        cin_pres[ix] = pr;
        const uint64_t v = ps_key[ix];                  // 0: the part holds no record of this key
        if (v > best) { best = v; bv = ps_val[ix]; }
        pr |= v != 0 ? 1 : 0;
    }
}

// The ordered packed resolve with per-record flags (level-2 order) and exact n_present / n_won.
// kK8: records from k_part_scatter2<true, true, true, ..> (1-B key column); else 4-B kj.
// kT threads per workgroup, kT * kTI = 2048 records per chunk; 16-bit list heads (a CAS loop, 76.5 KB of
// LDS: two workgroups per CU).  Measured and not kept (DESIGN.md §5.4): 512-thread workgroups, 32-bit heads
// (one workgroup per CU) and the flags as a bit array (the resolve's bit buffers cost it 15 VGPRs).
template <bool kK8, bool kC = false>    // kC: the compact form's 12-B records (k_resolve_packed)
__global__ __launch_bounds__(kRThreads, 8) void k_resolve_pflags(   // two workgroups per CU: <= 64 VGPRs

    const uint32_t* __restrict__ bstart, const uint32_t* __restrict__ ibase, const uint32_t* __restrict__ hbase,
    const uint32_t* __restrict__ item_bucket, uint32_t nb, const Rec12* __restrict__ irec,
    const void* __restrict__ ikj, Table table, uint64_t cap, uint64_t hw, const int64_t* __restrict__ Rj,
    uint32_t jbase, const uint64_t* __restrict__ cin_key, const uint32_t* __restrict__ cin_val,
    const uint8_t* __restrict__ cin_pres, PackFrame f, Misc* __restrict__ misc, uint8_t* __restrict__ flag,
    uint32_t which = 0)      // 0: every item; 1: unsplit buckets only; 2: split buckets' parts only (round 6:
                             // the unsplit ones run beside the split buckets' fold and carry-ins)
{
    constexpr int kT = kRThreads;
    // 76.5 KB: two workgroups per CU (one waits at a barrier while the other works)
    __shared__ unsigned long long st[kSKeys];      // 32 KB: the key's state (row / carry, then records)
    __shared__ uint32_t st_val[kSKeys];            // 16 KB
    __shared__ uint16_t head16[kSKeys];            //  8 KB: (chunk tag << 11) | chunk index, tags 1..31
    __shared__ uint32_t pres[kSKeys / 32];         // 512 B: bit k = key k present before the part (read-only)
    __shared__ unsigned long long c_pk[kRChunk];   // 16 KB
    __shared__ uint16_t c_next[kRChunk];           //  4 KB
    const uint32_t item = blockIdx.x;
    if (item >= ibase[nb]) return;
    if (misc->err & 3u) return;
    const uint32_t stop = misc->stop;
    const uint32_t jf_min = f.jwin - (stop > jbase ? std::min<uint32_t>(stop - jbase, f.jwin) : 0u);
    const uint64_t jmask = pack_jmask(f);
    const uint32_t b = item_bucket[item];
    const uint32_t nparts = ibase[b + 1] - ibase[b];
    const uint32_t part = item - ibase[b];
    if ((which == 1 && nparts > 1) || (which == 2 && nparts == 1)) return;
    const uint32_t s = bstart[b] + part * kRPart;
    const uint32_t e = std::min<uint32_t>(bstart[b + 1], s + kRPart);
    const int tid = threadIdx.x;
    constexpr int kTI = kRChunk / kT;                  // records per thread per chunk
    auto head_set = [&](uint32_t k, uint32_t v) { head16[k] = (uint16_t)v; };
    const uint64_t row0 = (uint64_t)b << kSBits;
    const uint32_t nk = (uint32_t)std::min<uint64_t>(kSKeys, cap - row0);
    constexpr int kKPer = kSKeys / kT;
    static_assert(kSKeys % kT == 0, "keys per thread");
    // records: three register buffers in rotation — chunk c is resolved while c + 1 lands and c + 2 is issued
    // (with one chunk ahead the loads' latency was exposed: two workgroups per CU keep too little in flight)
    Rec12 ra[kTI], rb[kTI], rc[kTI];
    uint32_t va[kTI], vb[kTI], vc[kTI];
    auto issue = [&](uint32_t p, Rec12 (&r)[kTI], uint32_t (&v)[kTI]) {
#pragma unroll
        for (int q = 0; q < kTI; ++q) {
            const uint32_t i = p + q * kT + tid;
            const uint32_t ii = i < e ? i : s;
            r[q] = irec[ii];
            v[q] = kC ? 0u : kK8 ? (uint32_t)__builtin_nontemporal_load(static_cast<const uint8_t*>(ikj) + ii)
                       : __builtin_nontemporal_load(static_cast<const uint32_t*>(ikj) + ii);
        }
    };
    if (nparts == 1) {
        uint4 h[kKPer];
#pragma unroll
        for (int kk = 0; kk < kKPer; ++kk) {             // rows >= hw are the fill: not read
            const uint32_t k = kk * kT + tid;
            const uint64_t row = row0 + (k < nk ? k : nk - 1);
            h[kk] = row < hw ? load_hot(table, row) : make_uint4(kFill, kFill, kFill, kFill);
        }
        issue(s, ra, va);
        issue(s + kRChunk, rb, vb);
#pragma unroll
        for (int kk = 0; kk < kKPer; ++kk) {
            const uint32_t k = kk * kT + tid;
            const bool vis = k < nk && (int32_t)h[kk].w >= 0;
            st[k] = pack_local(f, vis, (int64_t)(((uint64_t)h[kk].y << 32) | h[kk].x), h[kk].z);
            st_val[k] = 0xFFFFFFFFu;
            const unsigned long long pb = __ballot(vis);          // 64 consecutive keys per wave
            if ((tid & 63) == 0) {
                pres[k / 32] = (uint32_t)pb;
                pres[k / 32 + 1] = (uint32_t)(pb >> 32);
            }
            head_set(k, 0);
        }
    } else {
        const uint64_t cb = (uint64_t)(hbase[b] + part) * kSKeys;
        uint64_t ck[kKPer];
        uint32_t cv[kKPer];
        uint8_t cp[kKPer];
#pragma unroll
        for (int kk = 0; kk < kKPer; ++kk) {
            const uint32_t k = kk * kT + tid;
            ck[kk] = cin_key[cb + k];
            cv[kk] = cin_val[cb + k];
            cp[kk] = cin_pres[cb + k];
        }
        issue(s, ra, va);
        issue(s + kRChunk, rb, vb);
#pragma unroll
        for (int kk = 0; kk < kKPer; ++kk) {
            const uint32_t k = kk * kT + tid;
            st[k] = ck[kk];
            st_val[k] = cv[kk];
            const unsigned long long pb = __ballot(cp[kk] != 0);
            if ((tid & 63) == 0) {
                pres[k / 32] = (uint32_t)pb;
                pres[k / 32 + 1] = (uint32_t)(pb >> 32);
            }
            head_set(k, 0);
        }
    }
    __syncthreads();
    uint32_t npres = 0, nwon = 0, tag = 0;
    // Per chunk, two phases and two barriers.  A: every record reads its key's state S before the chunk
    // (st; the previous chunk's updates are behind the last barrier); a record with pk <= S loses and
    // leaves the state as it is (S only grows), so only the CANDIDATES (pk > S) are linked into their
    // key's list.  B: a candidate walks its list — the prefix maximum over the earlier same-key records
    // needs only the earlier candidates (a non-candidate is <= S) — and the chunk's maximum of a key
    // stores itself (nothing in phase B reads st).  present (n_present) = the state is a record or a
    // row above the frame (> 0), or the key's read-only bit (a visible row below the frame packs to 0).
    auto chunk = [&](uint32_t p0, const Rec12 (&r)[kTI], const uint32_t (&v)[kTI]) {
        if (++tag == 32) {                     // 5-bit tags: clear the heads every 31 chunks
            tag = 1;
#pragma unroll
            for (int kk = 0; kk < kKPer; ++kk) head_set(kk * kT + tid, 0);
            __syncthreads();
        }
        uint64_t pk[kTI], sv[kTI];
        uint32_t key[kTI], oldh[kTI];
        bool cand[kTI];
#pragma unroll
        for (int q = 0; q < kTI; ++q) {
            const uint32_t li = q * kT + tid;
            if (kC) {
                key[q] = (r[q].b >> (kCKeyShift - 32)) & (kSKeys - 1);
                pk[q] = ((uint64_t)(r[q].b & ((1u << (kCKeyShift - 32)) - 1)) << 32) | r[q].a;
            } else if (kK8) {
                key[q] = (v[q] << 4) | (r[q].b >> 28);
                pk[q] = ((uint64_t)(r[q].b & 0x0FFFFFFFu) << 32) | r[q].a;
            } else {
                key[q] = v[q] & (kSKeys - 1);
                pk[q] = ((uint64_t)r[q].b << 32) | r[q].a;
            }
            const bool act = p0 + li < e && (uint32_t)(pk[q] & jmask) > jf_min;
            sv[q] = act ? st[key[q]] : ~0ull;
            cand[q] = act && pk[q] > sv[q];
            oldh[q] = 0;
            if (cand[q]) {
                c_pk[li] = pk[q];
                oldh[q] = lds_exch16(&head16[key[q]], (uint16_t)((tag << 11) | li));
                c_next[li] = (uint16_t)oldh[q];
            } else if (act) {
                npres += 1u;                               // S >= pk > 0: present, loses
            }
            if (flag && p0 + li < e && !cand[q]) flag[p0 + li] = 0;
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < kTI; ++q) {
            if (!cand[q]) continue;
            const uint32_t li = q * kT + tid;
            uint64_t best = sv[q];                        // the state before this chunk ...
            bool later_gt = false;                        // a later same-key candidate beats this one
            uint32_t h = head16[key[q]];
            if (h == ((tag << 11) | li) && (oldh[q] >> 11) != tag) h = 0;   // alone in the chunk
            while ((h >> 11) == tag) {                    // ... and every earlier same-key candidate
                const uint32_t m = h & (kRChunk - 1);
                const uint64_t x = c_pk[m];
                if (m < li) best = x > best ? x : best;
                else if (m > li && x > pk[q]) later_gt = true;
                h = c_next[m];
            }
            const bool win = pk[q] > best;
            const bool pr = best != 0 || ((pres[key[q] >> 5] >> (key[q] & 31)) & 1u);
            npres += pr ? 1u : 0u;
            nwon += win ? 1u : 0u;
            if (flag) flag[p0 + li] = win ? 1 : 0;
            // the chunk's last winner of its key is its maximum: the one record that updates the state
            if (win && !later_gt) {
                st[key[q]] = pk[q];
                st_val[key[q]] = r[q].c;
            }
        }
        __syncthreads();                                  // the next chunk reads st, rewrites the lists
    };
    const uint32_t nch = (e - s + kRChunk - 1) / kRChunk;
    uint32_t p0 = s, c = 0;
    for (; c + 3 <= nch; c += 3) {                      // unrolled by three: no buffer copies
        issue(p0 + 2 * kRChunk, rc, vc);
        chunk(p0, ra, va);
        p0 += kRChunk;
        issue(p0 + 2 * kRChunk, ra, va);
        chunk(p0, rb, vb);
        p0 += kRChunk;
        issue(p0 + 2 * kRChunk, rb, vb);
        chunk(p0, rc, vc);
        p0 += kRChunk;
    }
    if (c < nch) chunk(p0, ra, va);
    if (c + 1 < nch) chunk(p0 + kRChunk, rb, vb);
    __syncthreads();
    if (part + 1 == nparts) {                           // the bucket's last part stores its rows
        for (uint32_t k = tid; k < nk; k += kT) {
            const uint64_t x = st[k];
            if (!pack_is_record(f, x)) continue;
            store_row(table, row0 + k, pack_lt(f, x), pack_rank(f, x), st_val[k],
                      Rj[jbase + pack_jw(f, x)]);
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        npres += __shfl_xor(npres, off, 64);
        nwon += __shfl_xor(nwon, off, 64);
    }
    if ((tid & 63) == 0) {
        const int slot = (item * (kT / 64) + (tid >> 6)) & (kCounterSlots - 1);
        if (npres) atomicAdd(&misc->present[slot], (unsigned long long)npres);
        if (nwon) atomicAdd(&misc->won[slot], (unsigned long long)nwon);
    }
}

// The flags carried back through one partition level, one workgroup per tile of that level: the
// tile's records went to one run per digit, [toff[t][d], + hist[t][d]).  The workgroup stages those
// runs of fsrc (flags in the level's output order) in LDS in digit order — neighbouring threads read
// neighbouring bytes of a run — then writes fdst[p] = s_f[pos[p]] for its records p in the level's input
// order: pos (written by the level's scatter) is the record's index in that staging order, so no digit
// or key is read.  Four records per thread on 4-aligned indices: one 8-B position load, one 4-B flag
// store.  kStop (level 1): tiles of changesets >= stop keep the zeros written before the call.
// kChkSh > 0: a staged index's run is searched between two checkpoints (the run of every 2^kChkSh-th
// staged index, found once per tile) instead of over all 256 digits.
// kT: the tile size the launch's tiles have at most — level 2's 8192-record tiles stage 8 KB (and search 128
// checkpoints), not level 1's 28 KB / 448, so more workgroups share a CU and each does a third of the fixed work
// kWide (round 6): the staging reads the runs four staged bytes per thread — one run search per four bytes and
// dword loads (two aligned dwords funnel-shifted when the run's bytes are not 4-aligned in fsrc; a group that
// straddles runs takes its bytes one by one) — instead of one byte load and one search per staged byte.
// xper > 0: the XCD-contiguous tile order of the scatters (xcd_tile): a line of fsrc holds the runs of
// neighbouring tiles for one digit, so those tiles read it through one L2 instead of up to four.
// fsrc must be readable 8 bytes past its last flag (the callers allocate nw + 8).
template <bool kStop, int kChkSh = 6, int kT = kPTile, bool kWide = true>
__global__ __launch_bounds__(512) void k_flags_back(TileMap tm, const uint32_t* __restrict__ hist,
                                                    const uint32_t* __restrict__ toff,
                                                    const uint16_t* __restrict__ pos,
                                                    const uint8_t* __restrict__ fsrc, uint8_t* __restrict__ fdst,
                                                    const Misc* __restrict__ misc, uint32_t xper = 0)
{
    __shared__ __attribute__((aligned(16))) uint8_t s_f[kT];
    __shared__ uint32_t s_dst[kDigits + 1];
    __shared__ uint32_t s_off[kDigits];
    __shared__ uint32_t s_w[4];
    constexpr bool kChk = kChkSh > 0;
    constexpr uint32_t kNChk = kChk ? (uint32_t)kT >> kChkSh : 1u;
    __shared__ uint8_t s_chk[kNChk];
    static_assert(!kChk || kNChk <= 4 * 512, "checkpoints: a few per thread");
    if (misc->err & 3u) return;
    const uint32_t t = xcd_tile(blockIdx.x, xper, xper != 0);
    if (t >= tm.tbase[tm.nseg]) return;
    uint32_t seg, len;
    uint64_t beg;
    tile_info(tm, t, &seg, &beg, &len);
    if (kStop && tm.seg_j[seg] >= misc->stop) return;
    const int tid = threadIdx.x;
    const uint32_t hv = tid < (int)kDigits ? hist[(uint64_t)t * kDigits + tid] : 0u;
    uint32_t all;
    const uint32_t ex = scan256_excl(hv, s_w, &all);
    if (tid < (int)kDigits) {
        s_dst[tid] = ex;
        s_off[tid] = toff[(uint64_t)t * kDigits + tid];
        if (tid == kDigits - 1) s_dst[kDigits] = ex + hv;
    }
    __syncthreads();
    if (kChk) {   // checkpoint m: the run of staged index m << kChkSh
        for (uint32_t m = tid; m < kNChk; m += 512u) {
            const uint32_t x = m << kChkSh;
            uint32_t lo = 0, hi = kDigits;
            while (hi - lo > 1) {
                const uint32_t mid = (lo + hi) >> 1;
                if (s_dst[mid] <= x) lo = mid; else hi = mid;
            }
            s_chk[m] = (uint8_t)lo;
        }
        __syncthreads();
    }
    // staged index x -> its run (largest d with s_dst[d] <= x)
    const uint32_t staged = std::min<uint32_t>(s_dst[kDigits], kT);
    auto run_of = [&](uint32_t x) -> uint32_t {
        const uint32_t m = std::min<uint32_t>(x >> (kChk ? kChkSh : 0), kNChk - 1);
        uint32_t lo = kChk ? s_chk[m] : 0u;
        uint32_t hi = kChk && m + 1 < kNChk ? s_chk[m + 1] + 1u : kDigits;
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if (s_dst[mid] <= x) lo = mid; else hi = mid;
        }
        return lo;
    };
    if (kWide) {            // four staged bytes per thread, 4 groups in flight
        const uint32_t ng = (staged + 3u) >> 2;
        for (uint32_t g0 = tid; g0 < ng; g0 += 512u * 4u) {
            uint32_t w[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const uint32_t g = g0 + u * 512u;
                const uint32_t x = g << 2;
                uint32_t out = 0;
                if (g < ng) {
                    uint32_t lo = run_of(x);
                    if (x + 4u <= s_dst[lo + 1] && x + 4u <= staged) {        // one run: a 4-byte window
                        const uint64_t a = (uint64_t)s_off[lo] + (x - s_dst[lo]);
                        const uint32_t* p = reinterpret_cast<const uint32_t*>(fsrc + (a & ~3ull));
                        const uint32_t sh = (uint32_t)(a & 3u);
                        out = sh ? __builtin_amdgcn_alignbyte(p[1], p[0], sh) : p[0];
                    } else {                                                 // straddles runs / the end:
                        uint64_t src[4];                                     // the four sources first (LDS
#pragma unroll                                                               // only), then four independent
                        for (uint32_t b = 0; b < 4u; ++b) {                  // byte loads
                            const uint32_t xb = std::min<uint32_t>(x + b, staged - 1u);
                            while (s_dst[lo + 1] <= xb) ++lo;                // (runs may be empty)
                            src[b] = (uint64_t)s_off[lo] + (xb - s_dst[lo]);
                        }
                        uint32_t by[4];
#pragma unroll
                        for (uint32_t b = 0; b < 4u; ++b) by[b] = fsrc[src[b]];
#pragma unroll
                        for (uint32_t b = 0; b < 4u; ++b)
                            if (x + b < staged) out |= by[b] << (8u * b);
                    }
                }
                w[u] = out;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (g0 + u * 512u < ng) reinterpret_cast<uint32_t*>(s_f)[g0 + u * 512u] = w[u];
        }
    } else                  // one staged byte per thread, 8 loads in flight
    for (uint32_t x0 = tid; x0 < staged; x0 += 512u * 8u) {
        uint8_t v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const uint32_t x = x0 + u * 512u;
            const uint32_t m = std::min<uint32_t>(x >> (kChk ? kChkSh : 0), kNChk - 1);
            uint32_t lo = kChk ? s_chk[m] : 0u;
            uint32_t hi = kChk && m + 1 < kNChk ? s_chk[m + 1] + 1u : kDigits;
            while (hi - lo > 1) {
                const uint32_t mid = (lo + hi) >> 1;
                if (s_dst[mid] <= x) lo = mid; else hi = mid;
            }
            v[u] = x < staged ? fsrc[s_off[lo] + (x - s_dst[lo])] : (uint8_t)0;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (x0 + u * 512u < staged) s_f[x0 + u * 512u] = v[u];
    }
    __syncthreads();
    const uint32_t a0 = std::min<uint32_t>((uint32_t)((4u - (beg & 3u)) & 3u), len);   // to a 4-aligned index
    if (tid < (int)a0) fdst[beg + tid] = s_f[pos[beg + tid]];
    if (kWide) {            // eight records per thread: one 16-B position load, one 8-B flag store
        for (uint32_t i = a0 + tid * 8u; i < len; i += 512u * 8u) {
            const uint64_t g = beg + i;
            if (i + 8u <= len) {
                const u32x4u pv = *reinterpret_cast<const u32x4u*>(pos + g);
                u32x2u o;
                o.x = (uint32_t)s_f[pv.x & 0xFFFFu] | ((uint32_t)s_f[pv.x >> 16] << 8) |
                      ((uint32_t)s_f[pv.y & 0xFFFFu] << 16) | ((uint32_t)s_f[pv.y >> 16] << 24);
                o.y = (uint32_t)s_f[pv.z & 0xFFFFu] | ((uint32_t)s_f[pv.z >> 16] << 8) |
                      ((uint32_t)s_f[pv.w & 0xFFFFu] << 16) | ((uint32_t)s_f[pv.w >> 16] << 24);
                *reinterpret_cast<u32x2u*>(fdst + g) = o;
            } else {
                for (uint32_t x = i; x < len; ++x) fdst[beg + x] = s_f[pos[beg + x]];
            }
        }
        return;
    }
    for (uint32_t i = a0 + tid * 4u; i < len; i += 512u * 4u) {
        const uint64_t g = beg + i;
        if (i + 4u <= len) {
            const u32x2u pv = *reinterpret_cast<const u32x2u*>(pos + g);
            *reinterpret_cast<uint32_t*>(fdst + g) = (uint32_t)s_f[pv.x & 0xFFFFu] | ((uint32_t)s_f[pv.x >> 16] << 8) |
                                                     ((uint32_t)s_f[pv.y & 0xFFFFu] << 16) |
                                                     ((uint32_t)s_f[pv.y >> 16] << 24);
        } else {
            for (uint32_t x = i; x < len; ++x) fdst[beg + x] = s_f[pos[beg + x]];
        }
    }
}

// The flag pass with its memory round trips overlapped (round 6; VERDICT r5 item 3).  k_flags_back's waves spend
// ~76 % of their cycles parked on memory counters (SQ_WAIT_ANY, profiles/r06_pmc_flags_sq*.txt) with few issue
// stalls: each workgroup walks its tile as a chain of dependent round trips — the histogram, then the staged bytes
// eight per thread at a time, then each 2048-record slice of positions and its stores (level 2: ~6, level 1: ~21).
// Here the tile's positions (2 B per record; 8 per 16-B load) are loaded into registers first, beside the
// histogram and offsets, before anything waits; the staged bytes go kB per thread per batch (level 2's 16 in one);
// the gather then reads them from registers and LDS only and stores 8 flags per 8-B store.  kPV: 16-B position
// loads per thread (covers kPV * 8 * kTh records: the tile size).  kTh: threads (level 2: 256 — twice the bytes in
// flight per wave at the same waves per CU).
template <bool kStop, int kChkSh, int kT, int kB, int kTh = 512, bool kPT = false>
__global__ __launch_bounds__(kTh) void k_flags_back_pre(TileMap tm, const uint32_t* __restrict__ hist,
                                                        const uint32_t* __restrict__ toff,
                                                        const uint16_t* __restrict__ pos,
                                                        const uint8_t* __restrict__ fsrc, uint8_t* __restrict__ fdst,
                                                        const Misc* __restrict__ misc)
{
    constexpr int kPV = (kT + 8 * kTh - 1) / (8 * kTh);
    static_assert(kChkSh > 0 && kT % kTh == 0 && (kT / kTh) % kB == 0 && kTh >= (int)kDigits,
                  "whole batches of staged bytes; a thread per digit");
    __shared__ __attribute__((aligned(16))) uint8_t s_f[kT];
    __shared__ uint32_t s_dst[kDigits + 1];
    __shared__ uint32_t s_off[kDigits];
    __shared__ uint32_t s_w[4];
    constexpr uint32_t kNChk = (uint32_t)kT >> kChkSh;
    __shared__ uint8_t s_chk[kNChk];
    if (misc->err & 3u) return;
    const uint32_t t = blockIdx.x;
    if (t >= tm.tbase[tm.nseg]) return;
    uint32_t seg, len;
    uint64_t beg;
    tile_info(tm, t, &seg, &beg, &len);
    if (kStop && tm.seg_j[seg] >= misc->stop) return;
    const int tid = threadIdx.x;
    // the aligned body: 8-record groups from a0 (beg + a0 a multiple of 8: 16-B position loads, 8-B flag stores)
    // kPT (k_part_scatter1<.., kPT>): tile t's positions start at pos[t * kT], aligned; the flags still go to beg + i
    const uint32_t a0 = std::min<uint32_t>((uint32_t)((8u - (beg & 7u)) & 7u), len);
    const uint32_t ng = (len - a0) >> 3;
    const uint16_t* __restrict__ pt = kPT ? pos + (uint64_t)t * kT : pos + beg;     // position of record i: pt[i]
    // (the histogram and offsets first — vmcnt waits in issue order, so the scan below waits only for them — and
    // every load unconditional, clamped in range: a load under a branch makes the compiler wait for all of them)
    const uint32_t hv0 = hist[(uint64_t)t * kDigits + (tid & (kDigits - 1))];
    const uint32_t ov0 = toff[(uint64_t)t * kDigits + (tid & (kDigits - 1))];
    u32x4u pv[kPV];
    uint32_t pe[kPT ? kPV : 1];
    const uint32_t glast = ng ? ng - 1u : 0u;           // (pos is allocated 8 entries past its last record)
    // kPT: pt is 16-B aligned and a0 follows beg's alignment, so pt + a0 is dword-aligned only for an even a0; for
    // an odd one the group's 8 positions are the aligned block from one entry earlier, shifted by 16 bits, plus the
    // entry after it (pe)
    const bool odd = kPT && (a0 & 1u);
#pragma unroll
    for (int i = 0; i < kPV; ++i) {
        const uint32_t g = std::min<uint32_t>((uint32_t)tid + (uint32_t)kTh * i, glast);
        if (kPT) {
            const uint32_t x = a0 + 8u * g - (odd ? 1u : 0u);
            pv[i] = *reinterpret_cast<const u32x4u*>(pt + x);
            pe[kPT ? i : 0] = pt[x + 8u];
        } else {
            pv[i] = *reinterpret_cast<const u32x4u*>(pos + beg + a0 + 8u * g);
        }
    }
    const uint32_t hv = tid < (int)kDigits ? hv0 : 0u;
    const uint32_t ov = ov0;
    uint32_t all;
    const uint32_t ex = scan256_excl(hv, s_w, &all);
    if (tid < (int)kDigits) {
        s_dst[tid] = ex;
        s_off[tid] = ov;
        if (tid == kDigits - 1) s_dst[kDigits] = ex + hv;
    }
    __syncthreads();
    for (uint32_t m = tid; m < kNChk; m += (uint32_t)kTh) {      // checkpoint m: the run of staged index m << kChkSh
        const uint32_t x = m << kChkSh;
        uint32_t lo = 0, hi = kDigits;
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if (s_dst[mid] <= x) lo = mid; else hi = mid;
        }
        s_chk[m] = (uint8_t)lo;
    }
    __syncthreads();
    const uint32_t staged = std::min<uint32_t>(s_dst[kDigits], kT);
#pragma unroll 1
    for (int b0 = 0; b0 < kT / kTh; b0 += kB) {
        uint8_t v[kB];
#pragma unroll
        for (int u = 0; u < kB; ++u) {                   // every byte of the batch in flight before the first use
            const uint32_t x = (uint32_t)tid + (uint32_t)kTh * (uint32_t)(b0 + u);
            const uint32_t m = std::min<uint32_t>(x >> kChkSh, kNChk - 1);
            uint32_t lo = s_chk[m];
            uint32_t hi = m + 1 < kNChk ? s_chk[m + 1] + 1u : kDigits;
            while (hi - lo > 1) {
                const uint32_t mid = (lo + hi) >> 1;
                if (s_dst[mid] <= x) lo = mid; else hi = mid;
            }
            v[u] = x < staged ? fsrc[s_off[lo] + (x - s_dst[lo])] : (uint8_t)0;
        }
#pragma unroll
        for (int u = 0; u < kB; ++u) {
            const uint32_t x = (uint32_t)tid + (uint32_t)kTh * (uint32_t)(b0 + u);
            if (x < staged) s_f[x] = v[u];
        }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kPV; ++i) {
        const uint32_t g = (uint32_t)tid + (uint32_t)kTh * i;
        if (g < ng) {
            u32x4u p = pv[i];
            if (odd) {
                const u32x4u q = p;
                p.x = (q.x >> 16) | (q.y << 16);
                p.y = (q.y >> 16) | (q.z << 16);
                p.z = (q.z >> 16) | (q.w << 16);
                p.w = (q.w >> 16) | (pe[kPT ? i : 0] << 16);
            }
            u32x2u o;
            o.x = (uint32_t)s_f[p.x & 0xFFFFu] | ((uint32_t)s_f[p.x >> 16] << 8) |
                  ((uint32_t)s_f[p.y & 0xFFFFu] << 16) | ((uint32_t)s_f[p.y >> 16] << 24);
            o.y = (uint32_t)s_f[p.z & 0xFFFFu] | ((uint32_t)s_f[p.z >> 16] << 8) |
                  ((uint32_t)s_f[p.w & 0xFFFFu] << 16) | ((uint32_t)s_f[p.w >> 16] << 24);
            *reinterpret_cast<u32x2u*>(fdst + beg + a0 + 8u * g) = o;
        }
    }
    // the head (< 8 records before the aligned body) and the tail (< 8 after it)
    const uint32_t tl = a0 + 8u * ng;
    if (tid < (int)a0) fdst[beg + tid] = s_f[pt[tid]];
    if (tl + (uint32_t)tid < len) fdst[beg + tl + tid] = s_f[pt[tl + tid]];
}
