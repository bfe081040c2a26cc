/* crdt_merge.h — C-ABI of the MI355X-native MapCrdt merge hot path.
 *
 * The reference (Dart package `crdt` v4.0.2, /root/reference) has no FFI: its
 * boundary is the abstract class Crdt<K,V> (lib/src/crdt.dart:7) and its
 * storage SPI (lib/src/crdt.dart:140-169), implemented by MapCrdt
 * (lib/src/map_crdt.dart:9-53).  This header is the C surface a dart:ffi shim
 * subclassing Crdt would bind (INTEGRATION.md shows that binding); every entry
 * point names the reference member it replaces.
 *
 * Data model.  The host (Dart, or the Python mirror in crdt_amd/) owns keys,
 * values and node-id strings and interns them:
 *   key_id  : dense uint32 id, assigned in first-committed order, so id order is
 *             the LinkedHashMap insertion order (map_crdt.dart:10);
 *   lt      : int64 Hlc.logicalTime = (millis << 16) + counter (hlc.dart:16);
 *   rank    : uint32 order-preserving rank of the nodeId under Dart
 *             String.compareTo (hlc.dart:160), so nodeId equality == rank equality;
 *   val     : uint32 value handle; CRDT_NULL_VALUE marks a tombstone
 *             (record.dart:17, isDeleted <=> value == null).
 * The device keeps one row per key id: {i64 lt; u32 rank; i32 mod_hi; u32 mod_lo; u32 val},
 * 24 B apart by default (32 B with crdt_set_row_bytes: 8 zero bytes of padding), where
 * mod is Record.modified.logicalTime.  A row whose mod < 0 is invisible to
 * merge and to recordMap() (map_crdt.dart:42-45); never-written rows hold a
 * negative mod.
 *
 * Domain: |millis| < 2^47 for every clock and wall value (Dart int wraps past it).
 * Threading: a ctx is one replica shard (one GPU); calls on one ctx are synchronous and
 * must not run concurrently, exactly like the single-isolate reference.  A ctx joined
 * to a communicator (crdt_comm_init_*) is one of n_ranks key shards of ONE replica: its
 * crdt_merge calls are collective (every rank calls with the same n_changesets and
 * wall_millis) and the library runs the exchanges itself (SURVEY §8(b) "Threading").
 */
#ifndef CRDT_MERGE_H
#define CRDT_MERGE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CRDT_ABI_VERSION 5          /* 3: crdt_timing gained part1_records (round 3); 4: crdt_route_tune_info
                                       reports five ways, crdt_timing gained sent_bytes (round 5); 5: the
                                       collective deadline, crdt_set_comm_timeout / crdt_comm_state (round 6) */
#define CRDT_NULL_VALUE 0xFFFFFFFFu

/* Status codes.  1..3 mirror the reference exceptions (hlc.dart:164-189); the
 * host rethrows them with the exact messages of hlc.dart:170,179,188. */
enum crdt_status {
    CRDT_OK = 0,
    CRDT_CLOCK_DRIFT = 1,      /* ClockDriftException(drift_ms)         hlc.dart:164-171 */
    CRDT_DUPLICATE_NODE = 2,   /* DuplicateNodeException(local nodeId)  hlc.dart:182-189 */
    CRDT_OVERFLOW = 3,         /* OverflowException(counter)            hlc.dart:173-180 */
    CRDT_E_INVALID = -1,       /* bad argument (offsets, sizes, null pointers) */
    CRDT_E_HIP = -2,           /* HIP runtime error */
    CRDT_E_NOMEM = -3,         /* device allocation failed */
    CRDT_E_KEY_RANGE = -4,     /* a key_id >= capacity.  crdt_merge on one context: nothing stored and
                                  the canonical unchanged for device batches and on the sorted path;
                                  a host batch on the gather path (its keys stream in under the
                                  apply) may have stored the changesets before the bad id's launch;
                                  on a sharded context the other ranks' rows are stored */
    CRDT_E_NO_DEVICE = -5,     /* no usable gfx950 device */
    CRDT_E_COMM = -6           /* the communicator failed (RCCL error, missing librccl, a callback's error) */
};

/* Where the column pointers of a call live. */
enum crdt_mem { CRDT_MEM_HOST = 0, CRDT_MEM_DEVICE = 1 };

typedef struct crdt_ctx crdt_ctx;

/* R remote changesets, concatenated column-wise.  Changeset j is rows
 * [offsets[j], offsets[j+1]); it is one Map<K, Record<V>> handed to merge()
 * (crdt.dart:77), in its iteration order, so its key ids must be distinct. */
typedef struct crdt_batch {
    const uint32_t* key_id;    /* [n] */
    const int64_t* lt;         /* [n] */
    const uint32_t* rank;      /* [n] */
    const uint32_t* val;       /* [n] */
    const int64_t* millis;     /* optional [n]: Hlc.millis where it differs from lt >> 16 (a parsed
                                  counter > 0xFFFF, hlc.dart:43); NULL means millis = lt >> 16 */
    const uint64_t* offsets;   /* HOST memory, [n_changesets + 1], offsets[0] == 0 */
    uint32_t n_changesets;
    int32_t mem;               /* enum crdt_mem of the five column pointers (and win_flags) */
} crdt_batch;

/* Outcome of a merge / put call. */
typedef struct crdt_result {
    int32_t status;            /* enum crdt_status */
    uint32_t n_stored;         /* changesets whose winners were stored (putRecords ran) */
    uint32_t exc_changeset;    /* changeset that raised, when status in 1..3 */
    uint32_t reserved;
    uint64_t exc_index;        /* record (in that changeset) whose recv() raised; UINT64_MAX when
                                  send() raised after storing (crdt.dart:93) */
    int64_t canonical_lt;      /* Crdt._canonicalTime.logicalTime after the call (crdt.dart:9) */
    int64_t drift_ms;          /* ClockDriftException.drift (hlc.dart:167) */
    int64_t counter;           /* OverflowException.counter (hlc.dart:176) */
    uint64_t n_present;        /* records whose key was present in the local snapshot */
    uint64_t n_won;            /* records stored (winners) */
} crdt_result;

/* Device-side kernel timing of the last call, measured with HIP events on the
 * ctx stream (bench / roofline support; zeros unless enabled). */
typedef struct crdt_timing {
    double scan_ms;            /* K3a: per-changeset max + candidate tiles */
    double clock_ms;           /* K3b/K3c: canonical prefix-max scan, exception resolution (+ the
                                  clock collectives on a sharded ctx) */
    double apply_ms;           /* K2: summed durations of SAMPLED windows of back-to-back apply launches
                                  (8 launches every 32; the sorted path: its whole apply region) */
    uint32_t apply_launches;   /* apply launches inside the sampled windows */
    uint32_t apply_total;      /* apply launches in the call */
    double total_ms;           /* first to last event of the call */
    double route_ms;           /* sharded ctx: route count, count exchange, scatter, record exchange */
    /* sorted path (first window of changesets): the level-1 partition scatter, the level-2 partition
       (its histogram and scatter), the resolve (fold, carry and resolve launches); 0 otherwise */
    double part1_ms;
    double part2_ms;
    double resolve_ms;
    uint64_t part1_records;    /* records the level-1 partition scatter read in that window */
    uint64_t sent_bytes;       /* sharded ctx: bytes this rank handed its peers in the call's all-to-all
                                  exchanges (records, counts; its own part excluded); 0 on one GPU.
                                  Filled whether or not timing is on. */
} crdt_timing;

/* ---- lifecycle ------------------------------------------------------------ */
int crdt_abi_version(void);
const char* crdt_status_string(int status);
int crdt_device_count(int* out);

/* MapCrdt(nodeId) (map_crdt.dart:16) + Crdt() -> refreshCanonicalTime() on the
 * empty map (crdt.dart:31-33): canonical lt = 0.  local_rank is the rank of the
 * local nodeId.  capacity rows are allocated and marked absent. */
int crdt_create(int device, uint32_t local_rank, uint64_t capacity, crdt_ctx** out);
void crdt_destroy(crdt_ctx* ctx);
int crdt_reserve(crdt_ctx* ctx, uint64_t capacity);          /* grow; new rows absent */
/* Pre-size the sorted path's partition scratch for merges of up to n_records applied records
 * (two partitioned copies in the packed form, 27 B per record; a wider form grows them in its first
 * merge), so the first large merge allocates nothing and the buffers are placed while device memory is
 * still unfragmented.  On a single-GPU ctx it also asks for the placement tuner's trials
 * (crdt_place_info): the next sorted merge takes the candidate level-1 buffers, sized for its form
 * (14 B per record at the fan-in) and together at most 1/8 of the device's HBM; they are freed once
 * timed, or after two merges that do not take the sorted path.  Optional. */
int crdt_reserve_scratch(crdt_ctx* ctx, uint64_t n_records);
/* Row size of the device table: 24 (default) or 32 bytes; the rows are copied over.  24-B rows move
 * 25 % fewer bytes in the sorted path's coalesced passes (many-changeset fan-ins); 32-B rows make
 * the gather path's random winner writes one aligned 32-B store (streaming calls where most
 * records win).  Results are identical. */
int crdt_set_row_bytes(crdt_ctx* ctx, uint32_t row_bytes);
int crdt_capacity(const crdt_ctx* ctx, uint64_t* out);
int crdt_set_local_rank(crdt_ctx* ctx, uint32_t rank);        /* after a rank remap */

/* Crdt._canonicalTime (crdt.dart:9-11). */
int crdt_get_canonical(const crdt_ctx* ctx, int64_t* lt);
int crdt_set_canonical(crdt_ctx* ctx, int64_t lt);

/* ---- storage SPI (crdt.dart:140-169) --------------------------------------- */
/* putRecord / putRecords (map_crdt.dart:27-39) and the seed addAll
 * (map_crdt.dart:17): store rows verbatim, no clock update. */
int crdt_put_rows(crdt_ctx* ctx, const uint32_t* key_id, const int64_t* lt, const uint32_t* rank,
                  const uint32_t* val, const int64_t* mod, uint64_t n, int32_t mem);
/* getRecord (map_crdt.dart:24): gather rows; any output pointer may be NULL. */
int crdt_read_rows(crdt_ctx* ctx, const uint32_t* key_id, uint64_t n, int64_t* lt, uint32_t* rank,
                   uint32_t* val, int64_t* mod, int32_t mem);
/* recordMap(modifiedSince) filter (map_crdt.dart:42-45): ids in [0, n_rows) with
 * mod >= since_lt, ascending (= insertion order).  out_ids (HOST) holds n_rows. */
int crdt_modified_since(crdt_ctx* ctx, uint64_t n_rows, int64_t since_lt, uint32_t* out_ids,
                        uint64_t* n_out);
/* ---- changeset export: recordMap(modifiedSince) left on the device (crdt.dart:157-160) ----
 * The rows of [0, n_rows) whose mod is not < since_lt (crdt_modified_since's predicate, on the raw
 * signed 64-bit value), ascending by id, as the five columns of a changeset.  The export reads the
 * table twice (a count pass, a scan of the tile counts, a write pass that skips tiles holding no
 * selected row) and moves nothing to the host.
 *
 * Ownership: the columns belong to the ctx that exported them, in buffers of their own sized from the
 * count pass (not the staging crdt_merge / crdt_put_rows reuse).  They stay valid until the next
 * crdt_export_since, crdt_export_flagged, crdt_export_release or crdt_destroy on THAT ctx; calls on other ctxs, and merges
 * or puts on the same ctx, leave them alone.  crdt_export_since is synchronous: the ctx's stream is
 * drained before it returns, so another ctx's stream may read the columns at once.  n_rows == 0 and an
 * empty selection give n = 0 (the pointers may then be NULL).
 *
 * Replica-to-replica sync.  For two ctxs on the SAME device whose host shares one key, node and value
 * interning,
 *     crdt_export v;  crdt_export_since(src, n_rows, since, &v);
 *     uint64_t offs[2] = {0, v.n};
 *     crdt_batch b = {v.key_id, v.lt, v.rank, v.val, NULL, offs, 1, CRDT_MEM_DEVICE};
 *     crdt_merge(dst, &b, wall_millis, flags_or_NULL, &res);
 * is dst.merge(src.recordMap(modifiedSince: since)) without a byte crossing to the host (an empty
 * view is still one merge() call: the closing Hlc.send advances dst's canonical, crdt.dart:93).
 * On a sharded ctx the export is rank-local and key_id holds slots, as crdt_modified_since's ids do. */
typedef struct crdt_export {        /* a changeset: one Map<K, Record<V>> in insertion (id) order */
    const uint32_t* key_id;
    const int64_t* lt;
    const uint32_t* rank;
    const uint32_t* val;
    const int64_t* mod;
    uint64_t n;                /* records */
    uint64_t n_live;           /* of them not tombstones (val != CRDT_NULL_VALUE) */
    int32_t mem;               /* CRDT_MEM_DEVICE */
    int32_t device;            /* the exporting ctx's device */
} crdt_export;
int crdt_export_since(crdt_ctx* ctx, uint64_t n_rows, int64_t since_lt, crdt_export* out);
/* Records [first, first + count) of the ctx's current view copied to HOST arrays; any pointer may be
 * NULL.  CRDT_E_INVALID without a view (none exported yet, or released) or past its end. */
int crdt_export_read(crdt_ctx* ctx, uint64_t first, uint64_t count, uint32_t* key_id, int64_t* lt,
                     uint32_t* rank, uint32_t* val, int64_t* mod);
/* Ends the view and frees its buffers. */
int crdt_export_release(crdt_ctx* ctx);
/* The export's n and n_live alone: the count pass only, no column and nothing sized by the table is
 * allocated (Crdt.length = n_live at since_lt = 0, crdt.dart:20). */
int crdt_count_since(crdt_ctx* ctx, uint64_t n_rows, int64_t since_lt, uint64_t* n, uint64_t* n_live);
/* ---- flag-predicated export: "which records did that merge store?" as a changeset ----
 * The rows of ctx in [0, n_rows) whose flags[i] & bits is non-zero, ascending by id, as the five columns
 * of a crdt_export with n and n_live filled.  Ownership, lifetime and synchrony are crdt_export_since's:
 * the columns live in the ctx's export buffers, the call ends the ctx's earlier view and becomes the
 * current one (crdt_export_read / crdt_export_release work on it, the next crdt_export_since or
 * crdt_export_flagged ends it), the stream is drained before return, and buffers over four times too
 * large are given back first.  Rows are read as they are: a flagged row at or above the high-water mark
 * is exported with its fill contents (the flags are the caller's; nothing is clipped).  The table's
 * rows, canonical and high-water mark are untouched.  The passes: the flag bytes alone (n_rows bytes), a
 * scan of the tile counts, and a write pass that loads only the flagged rows of the tiles that hold one.
 *
 * flags ([n_rows] bytes, CRDT_MEM_DEVICE, on the ctx's device) is read-only and may be NULL when n_rows
 * is 0.  CRDT_E_INVALID, with nothing touched and the earlier view kept, for a NULL ctx, out or flags, n_rows
 * above the capacity, a ctx joined to a communicator, and flags_mem == CRDT_MEM_HOST.  bits == 0 and
 * n_rows == 0 give an empty valid view.
 *
 * Call it on the table the merged records CAME FROM, with the merge's flags: the stored record is the
 * source's {lt, rank, val} (its mod in the destination is the destination's stamp, which the caller
 * knows from the result), and the source is not written by the merge, while the destination's row may
 * be overwritten again before anyone looks.
 *   crdt_merge_table(dst, src, .., flags):  crdt_export_flagged(src, n_rows, flags, DEVICE, 1, &v) is
 *       exactly the records dst stored: the reference's map after removeWhere (crdt.dart:80-85).
 *   crdt_fanin_tables(dst, srcs, .., mask): bit j read against srcs[j] gives merge j's stored records,
 *       even where a later merge of the call overwrote the row in dst.
 *   crdt_fanout_tables(src, dsts, .., mask): bit j read against src gives destination j's.
 *   crdt_sync_tables(a, b, .., flags_a, flags_b): flags_a reads against b and flags_b against a.  A row
 *       that a took from b ties in the second merge (equal keeps local), so b's copy is unchanged where
 *       flags_a is set; a is not written after the first merge, so it holds what b stored.
 *   crdt_diff_tables(a, b, .., diff_flags): CRDT_DIFF_A_AHEAD read against a is the changeset b lacks (what
 *       b.merge(a.recordMap()) would store), CRDT_DIFF_B_AHEAD read against b the one a lacks, and
 *       CRDT_DIFF_CONFLICT read against either gives that side's records of the rows no merge can heal.
 *   crdt_tombstone_live(ctx, .., row_flags): read against ctx itself, key_id holds the ids of the watch()
 *       events of that clear(), in id order (every such record is the tombstone {C, local node, null, C}).
 *   crdt_purge_tombstones(ctxs, .., row_flags): read against any member, key_id is the list of purged ids, in
 *       id order (the other columns are the fill the purge left).
 *   crdt_diff_group(ctxs, .., behind_mask, hold_mask, conflict_flags): behind_mask with bits = 1 << j, read against
 *       any member: key_id lists the keys on which member j is behind, in id order (the other columns belong to
 *       the member the export was read from and mean nothing here, as after the purge).  hold_mask with
 *       bits = 1 << h, read against member h: the records on which h holds the group's winner (what a member
 *       whose behind bit is set there lacks).  conflict_flags, read against a member: that member's records on
 *       the rows in conflict, the same ids in the same order on every member. */
int crdt_export_flagged(crdt_ctx* ctx, uint64_t n_rows, const uint8_t* flags, int32_t flags_mem,
                        uint8_t bits, crdt_export* out);
/* purge() (map_crdt.dart:51-52) and rollback of interned-but-uncommitted ids. */
int crdt_clear_rows(crdt_ctx* ctx, uint64_t first, uint64_t count);
/* Re-rank stored node ids after the host inserts a new nodeId between existing
 * ranks: rank := old_to_new[rank] for rows [0, n_rows). */
int crdt_remap_ranks(crdt_ctx* ctx, uint64_t n_rows, const uint32_t* old_to_new, uint32_t n_ranks);

/* ---- Crdt API ------------------------------------------------------------ */
/* put / putAll / delete (crdt.dart:39-58): ONE Hlc.send (hlc.dart:51-74) for the
 * whole call, then rows {C, local_rank, val, C}; n == 0 is a no-op (crdt.dart:48). */
int crdt_put_stamped(crdt_ctx* ctx, const uint32_t* key_id, const uint32_t* val, uint64_t n,
                     int64_t wall_millis, int32_t mem, crdt_result* out);

/* clear() (crdt.dart:67-73: putAll of null over the live view) on the table itself.  A row i of [0, n_rows) is
 * visible iff !(mod < 0) on the raw signed 64-bit value (crdt_export_since's predicate at since_lt = 0) and
 * live iff it is visible and val != CRDT_NULL_VALUE.  For every input the call leaves exactly what
 *     crdt_export_since(ctx, n_rows, 0, &v);
 *     ids = { v.key_id[x] : v.val[x] != CRDT_NULL_VALUE }                 (v.n_live of them, ascending)
 *     crdt_put_stamped(ctx, ids, {CRDT_NULL_VALUE, ..}, v.n_live, wall_millis, CRDT_MEM_DEVICE, out);
 * leaves: the table's rows byte for byte (the zero padding of 32-B rows included), the canonical, every field
 * of *out and the return status.  No live row: a no-op (crdt.dart:48), CRDT_OK and the canonical where it was
 * even when Hlc.send at wall_millis would raise.  Hlc.send raises and there is a live row: status 1 or 3,
 * nothing stored, the canonical unchanged.  Otherwise every live row becomes {lt = C, rank = the local rank,
 * mod = C, val = CRDT_NULL_VALUE} with C = Hlc.send(canonical, wall_millis), the canonical becomes C and n_won
 * is the number of live rows.  Unlike the composition it leaves the ctx's export view alone and allocates
 * nothing that grows with the table or the selection: one streaming pass reads 12 B of every row below the
 * high-water mark (every line of the table once) and stores the live ones whole; its scratch is one word
 * (and, for flags in host memory, the ctx's flag staging).  When Hlc.send raises the pass is
 * crdt_count_since's, which writes nothing.
 * Untouched: every row that is not live (tombstones, invisible rows whatever their val, rows at or above
 * n_rows, the never-written fill), the high-water mark (only rows below it can be live), crdt_last_plan,
 * crdt_last_path and crdt_timing.
 * row_flags (optional, memory of kind flags_mem, any alignment): [n_rows] bytes indexed by ROW id, every entry
 * written: 1 where the row was tombstoned, else 0; all zero after a raise or a no-op.  They feed
 * crdt_export_flagged on the same ctx (its list above).
 * CRDT_E_INVALID, nothing touched: a null ctx or out, n_rows above the capacity, a bad flags_mem with a flags
 * pointer, a ctx joined to a communicator.  Synchronous on the ctx's stream. */
int crdt_tombstone_live(crdt_ctx* ctx, uint64_t n_rows, int64_t wall_millis, uint8_t* row_flags,
                        int32_t flags_mem, crdt_result* out);
/* The map getter's rows (crdt.dart:23): the records of crdt_export_since(ctx, n_rows, 0, ..) whose val !=
 * CRDT_NULL_VALUE, in the same order, so n == n_live.  The same three passes with the second predicate;
 * ownership, lifetime, synchrony and error cases are crdt_export_since's, and it becomes the ctx's current
 * view (crdt_export_read / crdt_export_release work on it). */
int crdt_export_live(crdt_ctx* ctx, uint64_t n_rows, crdt_export* out);

/* refreshCanonicalTime (crdt.dart:114-121) over rows [0, n_rows). */
int crdt_refresh_canonical(crdt_ctx* ctx, uint64_t n_rows, int64_t* out_lt);

/* R sequential Crdt.merge(changeset_j) calls (crdt.dart:77-94), wall clock
 * fixed at wall_millis for every clock read (hlc.dart:53,82).  Stops at the
 * first exception exactly as the reference: a recv() failure in changeset j
 * stores nothing of j and leaves canonical = the running max before the failing
 * record; a send() failure after j leaves j stored and canonical = R_j.
 * win_flags (optional, [n], same memory kind as the batch): 1 where the record
 * was stored — the Map the reference's removeWhere leaves behind (crdt.dart:80-85)
 * and the watch() events (map_crdt.dart:36-38). */
int crdt_merge(crdt_ctx* ctx, const crdt_batch* batch, int64_t wall_millis, uint8_t* win_flags,
               crdt_result* out);

/* dst.merge(src.recordMap(modifiedSince)) for two ctxs on the SAME device sharing one key / node / value
 * interning, without an export: ONE merge() call (crdt.dart:77-94) whose changeset is the rows of
 * src [0, n_rows) with !(mod < since_lt), ascending by id.  For every input it leaves exactly what
 *     crdt_export_since(src, n_rows, since_lt, &v);
 *     crdt_merge(dst, {v.key_id, v.lt, v.rank, v.val, NULL, {0, v.n}, 1, CRDT_MEM_DEVICE}, wall_millis, flags, out)
 * leaves — dst's rows and canonical, every field of crdt_result, the return status (an empty selection
 * is still one merge() call; exc_index counts among the selected rows; CRDT_E_KEY_RANGE, with nothing
 * stored, when a selected id is >= dst's capacity) — and src's rows, canonical and export view untouched.
 * Key k is row k of both tables, so the merge is two streaming passes and allocates nothing that grows
 * with the selection (its scratch: a count per tile and one bit per row): a clock pass over src (each
 * tile's selected rows, a selection bit per row, the selection's max lt and id, whether any selected row
 * may raise in recv()), a read-back of four words, and an apply pass that skips the tiles holding no
 * selected row, reads the selected rows of both tables and stores the winners with mod = the canonical
 * after the recv loop.
 * Whenever a selected row may raise (lt above dst's canonical with dst's node id, or over 60000 ms ahead
 * of wall_millis), a selected id lies outside dst, src == dst, dst is pinned to CRDT_PATH_SORTED, or the
 * environment says CRDT_TABLE_MERGE=0 (read at crdt_create of dst), the call runs the composition above
 * itself: nothing has been written by then.
 * row_flags (optional, memory of kind flags_mem): [n_rows] bytes indexed by ROW id, every entry written:
 * 1 where dst's row was stored, else 0 (the composition's win flags at their key ids: the watch() events).
 * CRDT_E_INVALID, nothing touched: a null ctx or out, n_rows > src's capacity, different devices, a ctx
 * joined to a communicator.  Neither ctx may be in another call; the work runs on dst's stream after
 * src's is drained, and the call is synchronous.  Afterwards crdt_last_path(dst) is CRDT_PATH_GATHER and
 * crdt_last_plan(dst) CRDT_PLAN_TABLE alone (after a fallback: what the composition's crdt_merge reports);
 * crdt_timing gets scan_ms (the clock pass), apply_ms (the apply pass) and total_ms. */
int crdt_merge_table(crdt_ctx* dst, crdt_ctx* src, uint64_t n_rows, int64_t since_lt, int64_t wall_millis,
                     uint8_t* row_flags, int32_t flags_mem, crdt_result* out);

/* The two-replica exchange a.merge(b.recordMap(modifiedSince: since_b)); b.merge(a.recordMap(modifiedSince:
 * since_a)) for two ctxs on the SAME device sharing one key / node / value interning.  For every input it
 * leaves exactly what
 *     s1 = crdt_merge_table(a, b, n_rows, since_b, wall_millis, flags_a, flags_mem, out_a);
 *     if (s1 == 0) s2 = crdt_merge_table(b, a, n_rows, since_a, wall_millis, flags_b, flags_mem, out_b);
 * leaves: both tables' rows and canonicals, every field of both crdt_results, both row-flag arrays
 * ([n_rows] bytes each, indexed by ROW id, every entry written) and both ctxs' export views untouched.  The
 * second merge selects from a AS THE FIRST LEFT IT: a row of b that won into a carries mod = a's canonical
 * after its recv loop and goes back to b's merge (where it loses the tie unless b's row is invisible).
 * s1 != 0 (an exception in a.merge ends the exchange, as in Dart, or an error): b is untouched, *out_b is
 * zero except exc_index = UINT64_MAX and canonical_lt = b's canonical, flags_b (if given) is all zero, and
 * the call returns s1.  Otherwise it returns s2; a negative s2 (an error in the second merge) leaves a
 * MERGED: step 1 is not undone.
 * The win decision (crdt.dart:83-84) reads no canonical clock, so both directions are decided on one read
 * of the two rows: a clock pass over {lt, rank, mod} of both tables (each tile's rows selected either way,
 * two selection bits per row, and per direction the selection's max lt, largest id, count and whether a row
 * may raise in recv()), one read-back of eight words, and an apply pass that skips the tiles holding no
 * selected row, loads both rows of the selected ones and stores the winners on each side (a with mod =
 * a's canonical after its recv loop, b with b's).  Scratch, on a: the words, a count per tile and two bits
 * per row; nothing grows with the selection.
 * The call runs the composition above itself, nothing written by then, whenever a selected row may raise in
 * either direction, step 1's closing Hlc.send raises, a's canonical after its recv loop is below since_a
 * (step 1's winners would not be selected by step 2), a == b, either ctx is pinned to CRDT_PATH_SORTED, or
 * either ctx was created under CRDT_TABLE_MERGE=0.  Step 2's Hlc.send raising after its store is reported
 * in place (status 1 or 3 in *out_b and as the return value, both tables stored).
 * CRDT_E_INVALID, nothing touched: a null ctx or out, n_rows above either capacity, different devices, a ctx
 * joined to a communicator, a bad flags_mem with a flags pointer.  Neither ctx may be in another call; the
 * work runs on a's stream after b's is drained, and the call is synchronous.  After the fused form
 * crdt_last_plan of BOTH ctxs is CRDT_PLAN_TABLE | CRDT_PLAN_SYNC and crdt_last_path CRDT_PATH_GATHER (after
 * a fallback: what the composition's calls report); crdt_timing is recorded on a: scan_ms (the clock
 * pass), apply_ms (the apply pass) and total_ms. */
int crdt_sync_tables(crdt_ctx* a, crdt_ctx* b, uint64_t n_rows, int64_t since_a, int64_t since_b,
                     int64_t wall_millis, uint8_t* flags_a, uint8_t* flags_b, int32_t flags_mem,
                     crdt_result* out_a, crdt_result* out_b);

/* The hub: for j in 0 .. n_src-1: dst.merge(srcs[j].recordMap(modifiedSince: since_lt[j])), 1 <= n_src <=
 * CRDT_FANIN_MAX ctxs on the SAME device sharing one key / node / value interning.  For every input it leaves
 * exactly what
 *     for (j = 0; j < n_src; ++j) {
 *         s_j = crdt_merge_table(dst, srcs[j], n_rows, since_lt[j], wall_millis, flags_j, mask_mem, &out[j]);
 *         if (s_j != 0) break;
 *     }
 * leaves: dst's rows and canonical, every field of every out[j], the return value (the first non-zero s_j,
 * else 0) and the mask.  win_mask (optional, memory of kind mask_mem): [n_rows] bytes indexed by ROW id, every
 * entry written: win_mask[i] = OR_j (flags_j[i] << j), bit j set where merge j stored row i (the watch()
 * events of the n_src merges; a row can be stored more than once in one call).  After a stop at step j the
 * steps before j stay merged (a negative s_j does not undo them), every out[k], k > j, is zero except
 * exc_index = UINT64_MAX and canonical_lt = dst's canonical at the stop, and no bit k > j is set.  An empty
 * selection is still one merge() call: its closing Hlc.send advances dst's canonical.  The sources are
 * read-only (rows, canonical, plan and export view untouched, and dst's export view too); a source may appear
 * more than once.  n_src == 1 runs crdt_merge_table and reports its plan.
 * The win decision (crdt.dart:83-84) reads no canonical clock and no source is written, so the whole call is
 * decided on ONE read of dst's row: crdt_merge_table's clock pass once per source (its tile counts, one
 * selection bit per row, four words; the candidate bit against dst's canonical at entry, C_0: canonicals
 * never decrease, so no candidate against C_0 means that no recv() of the sequence raises), one read-back of
 * 4 * n_src words, the host's chain R_j = max(C_{j-1}, max lt of selection j), C_j = Hlc.send(R_j), and one
 * apply pass that skips the tiles no source selected, loads dst's row once, folds the sources' selected rows
 * over it in registers in call order (the plain rule; a row stored by an earlier step is visible iff its
 * stamp R_i is non-negative) and stores the last winner with mod = its step's R.  Scratch, on dst: 4 * n_src
 * words, n_src counts per tile and n_src bits per row (134 MB for 8 sources of 2^27 rows); nothing grows
 * with the selection.
 * The call runs the composition above itself, nothing written by then, whenever a selected row is a candidate
 * against C_0 (lt above C_0 with dst's node id, or over 60000 ms ahead of wall_millis), a selected id is >=
 * dst's capacity, any Hlc.send of the chain raises, a srcs[j] is dst, dst is pinned to CRDT_PATH_SORTED, or
 * dst was created under CRDT_TABLE_MERGE=0.
 * CRDT_E_INVALID, nothing touched: a null dst, srcs, since_lt, out or srcs[j] (checked before any ctx is
 * read), n_src == 0 or > CRDT_FANIN_MAX, n_rows above any source's capacity, a ctx on another device, a ctx
 * joined to a communicator, a bad mask_mem with a mask pointer.  No ctx involved may be in another call; the
 * work runs on dst's stream after every source's is drained, and the call is synchronous.  After the fused
 * form crdt_last_plan(dst) is CRDT_PLAN_TABLE | CRDT_PLAN_FANIN and crdt_last_path(dst) CRDT_PATH_GATHER
 * (after a fallback: what the composition's last call reports); crdt_timing on dst gets scan_ms (the clock
 * passes), apply_ms (the apply pass) and total_ms. */
#define CRDT_FANIN_MAX 8
int crdt_fanin_tables(crdt_ctx* dst, crdt_ctx* const* srcs, const int64_t* since_lt, uint32_t n_src,
                      uint64_t n_rows, int64_t wall_millis, uint8_t* win_mask, int32_t mask_mem,
                      crdt_result* out /* [n_src] */);

/* The hub's outbound half: for j in 0 .. n_dst-1: dsts[j].merge(src.recordMap(modifiedSince: since_lt[j])),
 * 1 <= n_dst <= CRDT_FANOUT_MAX ctxs on the SAME device sharing one key / node / value interning.  For every
 * input it leaves exactly what
 *     for (j = 0; j < n_dst; ++j) {
 *         s_j = crdt_merge_table(dsts[j], src, n_rows, since_lt[j], wall_millis, flags_j, mask_mem, &out[j]);
 *         if (s_j != 0) break;
 *     }
 * leaves: every destination's rows and canonical, every field of every out[j], the return value (the first
 * non-zero s_j, else 0) and the mask.  win_mask (optional, memory of kind mask_mem): [n_rows] bytes indexed by
 * ROW id, every entry written: win_mask[i] = OR_j (flags_j[i] << j), bit j set where destination j stored row
 * i.  After a stop at step j the destinations before j stay merged, dsts[k], k > j, is untouched, out[k] is
 * zero except exc_index = UINT64_MAX and canonical_lt = dsts[k]'s own canonical, and no bit k > j is set.  An
 * empty selection is still one merge() call on that destination: its closing Hlc.send advances its canonical.
 * src is read-only (rows, canonical, plan, export view and high-water mark untouched, and every destination's
 * export view too).  n_dst == 1 runs crdt_merge_table and reports its plan.
 * The win decision (crdt.dart:83-84) reads no canonical clock, src is never written and the destinations are
 * independent, so the whole call is decided on ONE read of src: one clock pass over {lt, rank, mod} of src's
 * rows, every line once whatever n_dst is (per destination its tile counts, one selection bit per row and four
 * words, the candidate bit against THAT destination's canonical and node id), one read-back of 4 * n_dst
 * words, per destination R_j = max(C_j, max lt of selection j) and C_j' = Hlc.send(R_j), and one apply pass
 * that skips the tiles no destination selected, loads src's selected rows once and, destination by
 * destination, the decision half of its selected rows, and stores the winners with mod = R_j.  Scratch, on
 * dsts[0]: 4 * n_dst words, n_dst counts per tile and n_dst bits per row, and the per-destination count
 * words; nothing grows with the selection.
 * The call runs the composition above itself, nothing written by then, whenever a row selected for
 * destination j is a candidate for it (lt above dsts[j]'s canonical with its node id, or over 60000 ms ahead
 * of wall_millis) or has an id >= dsts[j]'s capacity, any destination's Hlc.send raises, src is among the
 * destinations, a destination appears twice, or any destination is pinned to CRDT_PATH_SORTED or was created
 * under CRDT_TABLE_MERGE=0.
 * CRDT_E_INVALID, nothing touched: a null src, dsts, since_lt, out or dsts[j] (checked before any ctx is
 * read), n_dst == 0 or > CRDT_FANOUT_MAX, n_rows above src's capacity, a ctx on another device, a ctx joined
 * to a communicator, a bad mask_mem with a mask pointer.  No ctx involved may be in another call; the work
 * runs on dsts[0]'s stream after src's and every other destination's is drained, and the call is synchronous.
 * After the fused form crdt_last_plan of EVERY destination is CRDT_PLAN_TABLE | CRDT_PLAN_FANOUT and
 * crdt_last_path CRDT_PATH_GATHER (after a fallback: what each one's own crdt_merge_table reported);
 * crdt_timing on dsts[0] gets scan_ms (the clock pass), apply_ms (the apply pass) and total_ms. */
#define CRDT_FANOUT_MAX 8
int crdt_fanout_tables(crdt_ctx* src, crdt_ctx* const* dsts, const int64_t* since_lt, uint32_t n_dst,
                       uint64_t n_rows, int64_t wall_millis, uint8_t* win_mask, int32_t mask_mem,
                       crdt_result* out /* [n_dst] */);

/* ---- read-only comparison of two replicas: "are they converged, and if not, who is ahead on which rows?" ----
 * For two ctxs on the SAME device sharing one key / node / value interning.  Per row i of [0, n_rows), with
 * va = (mod_a >= 0) and vb likewise (the visibility of recordMap() and of the table forms at since = 0) and
 * hlc = (lt, rank) compared as the merges compare it (signed lt, then unsigned rank):
 *   CRDT_DIFF_A_AHEAD  iff va && (!vb || hlc_a > hlc_b): exactly the win rule of b.merge(a.recordMap())
 *                      (crdt.dart:83-84).  For every input diff_flags[i] & 1 is the row_flags[i] that
 *                      crdt_merge_table(b, a, n_rows, 0, ..) would write and n_a_ahead its n_won, whenever
 *                      that merge does not raise.
 *   CRDT_DIFF_B_AHEAD  the same with a and b swapped.
 *   CRDT_DIFF_CONFLICT iff va && vb && hlc_a == hlc_b && val_a != val_b: the divergence no merge heals (equal
 *                      keeps local on both sides).  Values are compared by handle.
 *   else 0: both rows invisible (never written, cleared, above the high-water mark: their contents are not
 *           compared), or both visible with equal hlc and val, what Record == sees (record.dart:34-35).  mod is
 *           never compared: replicas stamp their own.
 * diff_flags (optional, memory of kind flags_mem, any alignment): [n_rows] bytes indexed by ROW id, every entry
 * written.  They feed crdt_export_flagged (its list above).  *out: the rows carrying each bit, the visible
 * rows of each side, and the smallest row id with a non-zero byte.
 * Untouched: both tables' rows, canonicals, high-water marks and export views, crdt_last_plan, crdt_last_path
 * and crdt_timing.  a == b is allowed (all zero); n_rows == 0 gives a zero struct with first_diff = UINT64_MAX.
 * One streaming pass over both tables (table_diff.inc); its scratch is six words (and, for flags in host
 * memory, the ctx's flag staging).  CRDT_E_INVALID, nothing touched: a null ctx or out (checked before any
 * ctx is read), n_rows above either capacity, different devices, a ctx joined to a communicator, a bad
 * flags_mem with a flags pointer.  Neither ctx may be in another call; the work runs on a's stream after b's
 * is drained, and the call is synchronous. */
enum crdt_diff_bits { CRDT_DIFF_A_AHEAD = 1, CRDT_DIFF_B_AHEAD = 2, CRDT_DIFF_CONFLICT = 4 };
typedef struct crdt_diff {
    uint64_t n_a_ahead, n_b_ahead, n_conflict;   /* rows carrying each bit */
    uint64_t n_visible_a, n_visible_b;           /* rows of [0, n_rows) with mod >= 0 */
    uint64_t first_diff;                         /* smallest row id with a non-zero byte; UINT64_MAX: none */
} crdt_diff;
int crdt_diff_tables(crdt_ctx* a, crdt_ctx* b, uint64_t n_rows, uint8_t* diff_flags, int32_t flags_mem,
                     crdt_diff* out);

/* One 64-bit word per block of rows: word k is the wrapping sum of mix(i, row_i) over the rows i of
 * [k * block_rows, min((k + 1) * block_rows, n_rows)), ceil(n_rows / block_rows) words in all, with
 *     h = lt * P0 ^ mod * P1 ^ ((rank << 32 | val) * P2) ^ (i * P3);  h ^= h >> 29;  h *= P4;  h ^= h >> 32
 *     P0..P4 = 0x9E3779B97F4A7C15, 0xC2B2AE3D27D4EB4F, 0x165667B19E3779F9, 0xD6E8FEB86659FD93, 0xFF51AFD7ED558CCD
 * CRDT_DIGEST_ROWS takes every row as stored, the never-written fill included: a table compares with rows held
 * elsewhere without being read.  CRDT_DIGEST_STATE is the digest of what Record == sees: an invisible row
 * (mod < 0) contributes 0 and a visible one leaves the mod term out, so two tables of one id space have equal
 * STATE words whenever crdt_diff_tables reports all zeros, whatever their capacities, row sizes, stamps and
 * never-written rows.  out_words (memory of kind mem; 8-byte aligned device memory) may be NULL when n_rows is 0.
 * Read-only as crdt_diff_tables is.  CRDT_E_INVALID: a null ctx, a null out_words with n_rows > 0, n_rows above
 * the capacity, block_rows not a power of two or below 2048 (a kernel tile never straddles two blocks), a bad
 * kind or mem, a ctx joined to a communicator.  Synchronous. */
enum crdt_digest_kind { CRDT_DIGEST_ROWS = 0, CRDT_DIGEST_STATE = 1 };
int crdt_digest_rows(crdt_ctx* ctx, uint64_t n_rows, uint64_t block_rows, int32_t kind,
                     uint64_t* out_words, int32_t mem /* of out_words */);

/* ---- tombstone collection: drop the deletions a group of replicas agrees on ----
 * A deletion is a record that is kept "since the deletion needs to be propagated" (crdt.dart:56-58, 64-66); once
 * every replica holds it, it propagates to nobody.  For 1 <= n_ctx <= CRDT_PURGE_MAX DISTINCT ctxs on the SAME
 * device sharing one key / node / value interning.  For row i of [0, n_rows) and member j:
 *     vis_j  = !(mod_j < 0)                        (crdt_tombstone_live's predicates)
 *     tomb_j = vis_j && val_j == CRDT_NULL_VALUE
 * Row i is a CANDIDATE iff tomb_0 && lt_0 < before_lt (signed, strict), and PURGED iff it is a candidate and for
 * every j: tomb_j && lt_j == lt_0 && rank_j == rank_0.  mod is never compared: replicas stamp their own.
 * A purged row is overwritten in EVERY member with the never-written fill: the bytes crdt_clear_rows(ctx, i, 1)
 * writes, over the row's whole stride.  Every other row of every member, and every row at or above n_rows, is
 * untouched.  A member that holds the row invisibly (never written, cleared, above its high-water mark) blocks
 * the purge: a replica that has not seen the deletion could still be handed the older live record.
 * For every input the call leaves what this composition leaves:
 *     crdt_export_since(ctxs[j], n_rows, 0, ..) of every member; the intersection above on the host;
 *     crdt_clear_rows(ctxs[j], id, 1) for each purged id on every member
 * except the high-water marks, which the call leaves alone ("rows at or above it hold the fill" stays true).
 * out->n_candidates counts the candidate rows, out->n_purged the purged ones (the same number on every member).
 * row_flags (optional, memory of kind flags_mem, any alignment): [n_rows] bytes indexed by ROW id, every entry
 * written: 1 where the row was purged, else 0.  They feed crdt_export_flagged (its list above).
 * Untouched: every canonical, every export view, crdt_last_plan, crdt_last_path and crdt_timing.  The call takes
 * no clock and cannot raise.  n_rows == 0 gives zeros; before_lt == INT64_MIN purges nothing; n_ctx == 1 is one
 * table collecting its own tombstones.
 * One streaming pass (table_purge.inc): member 0's table is read once, a later member only at the rows that are
 * still agreed, and only the purged rows are stored.  Its scratch is two words on ctxs[0] (and, for flags in host
 * memory, its flag staging): nothing grows with the table.
 * CRDT_E_INVALID, nothing touched: a null ctxs, out or ctxs[j] (checked before any ctx is read), n_ctx == 0 or
 * > CRDT_PURGE_MAX, a ctx listed twice, n_rows above any member's capacity, a ctx on another device, a ctx
 * joined to a communicator, a bad flags_mem with a flags pointer.  No member may be in another call; the work
 * runs on ctxs[0]'s stream after every other member's stream is drained, and the call is synchronous. */
#define CRDT_PURGE_MAX 8
typedef struct crdt_purge { uint64_t n_candidates, n_purged; } crdt_purge;
int crdt_purge_tombstones(crdt_ctx* const* ctxs, uint32_t n_ctx, uint64_t n_rows, int64_t before_lt,
                          uint8_t* row_flags, int32_t flags_mem, crdt_purge* out);

/* ---- read-only comparison of a group of replicas: "are they all converged, who lacks the winning record, who
 * holds news nobody else has?" ----
 * For 1 <= n_ctx <= CRDT_GROUP_MAX DISTINCT ctxs on the SAME device sharing one key / node / value interning.  The
 * predicates are crdt_diff_tables': vis_j = (mod_j >= 0); hlc = (lt, rank), signed lt first, then unsigned rank;
 * mod is never compared (replicas stamp their own); values are compared by handle.  For row i of [0, n_rows):
 *     W        = { j : vis_j }.  W empty: all three bytes are 0 and the row's contents are not compared.
 *     top      = the greatest hlc over W
 *     hold     bit j set iff j is in W and hlc_j == top
 *     behind   bit j set iff j < n_ctx and bit j of hold is clear: "not visible" and "visible but lower" alike
 *     conflict = 1 iff two members whose bits are set in hold have different val (members below the top take no
 *                part: a conflict between two members that a third overrules with a higher hlc is none)
 * so hold & behind == 0, and hold | behind == (1 << n_ctx) - 1 wherever W is not empty.
 * behind_mask, hold_mask, conflict_flags (each optional, all of the memory kind flags_mem, any alignment): [n_rows]
 * bytes indexed by ROW id, every entry of an array that is passed written.  They feed crdt_export_flagged (its list
 * above).  *out: n_held counts the rows with W not empty, n_disputed those with a non-zero behind byte, n_conflict
 * those with conflict == 1, first_diff is the smallest row id that is disputed or in conflict (UINT64_MAX: none);
 * per member j < n_ctx, n_visible[j] counts its rows with mod >= 0, n_behind[j] the rows carrying its behind bit,
 * n_sole[j] the rows whose hold byte is exactly 1 << j (news nobody else has).  Entries at or above n_ctx are 0.
 * Identities:
 *   n_ctx == 2, ctxs = {a, b}: behind bit 1 is crdt_diff_tables(a, b)'s CRDT_DIFF_A_AHEAD, behind bit 0 its
 *       CRDT_DIFF_B_AHEAD, conflict its CRDT_DIFF_CONFLICT; first_diff, n_visible[0] and n_visible[1] are its
 *       first_diff, n_visible_a and n_visible_b.
 *   n_ctx == 1: behind and conflict are 0 and hold is vis.
 *   n_disputed == 0 && n_conflict == 0: every member has the same CRDT_DIGEST_STATE words (crdt_digest_rows).
 *   wherever bit h of hold is set, crdt_diff_tables(ctxs[h], ctxs[j]) has CRDT_DIFF_A_AHEAD set iff bit j of
 *       behind is set.
 * Untouched: every table's rows, canonical, high-water mark and export view, crdt_last_plan, crdt_last_path and
 * crdt_timing.  The call takes no clock and cannot raise.  n_rows == 0 gives zeros with first_diff = UINT64_MAX.
 * One streaming pass (table_group.inc): every row of every member is read exactly once, no table is written.  Its
 * scratch is the 28 result words on ctxs[0] (and, for arrays in host memory, its flag staging, one [n_rows] part
 * per array that is passed): nothing else grows with the table.
 * CRDT_E_INVALID, nothing touched: a null ctxs, out or ctxs[j] (checked before any ctx is read), n_ctx == 0 or
 * > CRDT_GROUP_MAX, a ctx listed twice, n_rows above any member's capacity, a ctx on another device, a ctx
 * joined to a communicator, a bad flags_mem with any array pointer.  No member may be in another call; the work
 * runs on ctxs[0]'s stream after every other member's stream is drained, and the call is synchronous. */
#define CRDT_GROUP_MAX 8
typedef struct crdt_group_diff {
    uint64_t n_held;        /* rows some member holds visibly */
    uint64_t n_disputed;    /* rows with a non-zero behind byte */
    uint64_t n_conflict;    /* rows with conflict == 1 */
    uint64_t first_diff;    /* smallest row id that is disputed or in conflict; UINT64_MAX: none */
    uint64_t n_visible[CRDT_GROUP_MAX];  /* per member: rows with mod >= 0 */
    uint64_t n_behind[CRDT_GROUP_MAX];   /* per member: rows carrying its behind bit */
    uint64_t n_sole[CRDT_GROUP_MAX];     /* per member: rows whose hold byte is exactly its bit */
} crdt_group_diff;
int crdt_diff_group(crdt_ctx* const* ctxs, uint32_t n_ctx, uint64_t n_rows,
                    uint8_t* behind_mask, uint8_t* hold_mask, uint8_t* conflict_flags,
                    int32_t flags_mem, crdt_group_diff* out);

/* ---- key-sharded multi-GPU (north star config 4) -------------
 * n_ranks ctxs — one per GPU, normally one process per GPU — form ONE replica whose
 * keys are sharded: rank d owns key k iff k % n_ranks == d and stores it at slot
 * k / n_ranks (so each ctx's capacity counts slots).  crdt_merge on such a ctx is
 * collective: every rank passes the same n_changesets and wall_millis and its own
 * PART of each changeset; changeset j is the concatenation, in rank order, of the
 * ranks' parts (a Map's iteration order is whatever its sender produced, so this is a
 * legal order; a replica that arrives whole on one rank is the case where the other
 * parts are empty).  Inside the call the library:
 *   1. scans its parts (per-part max, tiles that may raise);
 *   2. all-gathers the R part maxima and counts -> M_j, and each part's preceding
 *      max / record offset inside changeset j;
 *   3. runs the canonical recurrence and exception scan, MIN all-reduce of the first
 *      event, MAX all-reduce of its details -> the same stop point everywhere;
 *   4. counts its records per (owner, changeset), exchanges the counts, scatters the
 *      records into owner-major send columns {slot, lt, rank, val} and moves them with
 *      ONE grouped all-to-all (every column of every peer in one group);
 *   5. applies the records it received (gather or sorted path) with mod = R_j;
 *   6. SUM all-reduce of the per-record counts and of the key-range error.
 * Every rank returns the same status, stop point, canonical and counts; win_flags
 * (optional, [n] of the local batch) come back to the rank that passed the record.
 * A failure local to one rank (CRDT_E_NOMEM, CRDT_E_INVALID of its own batch, CRDT_E_HIP
 * of a launch or copy) is carried through the call's collectives and returned by EVERY
 * rank — no rank is left waiting in a collective its peers will not post.  Before the
 * record exchange nothing is stored and the canonical clock does not move; a failure in the
 * owners' apply (after the exchange) leaves the other ranks' rows of the stopped call stored
 * and the canonical unchanged (re-merging the same batch is exact).  Rank-local still: a
 * failing transport, a rank that cannot allocate the call's O(R) gather words, and a HIP
 * failure of a read-back of agreed words (without them the rank cannot post what its peers
 * post next).  Those — and a peer that died, hung or faulted — end at the call's DEADLINE:
 * every host wait of a sharded call polls against it (crdt_set_comm_timeout); past it the
 * communicator is aborted (ncclCommAbort for RCCL) and the call returns CRDT_E_COMM.  After
 * CRDT_E_COMM the ctx refuses sharded merges (CRDT_E_COMM) until it joins a communicator
 * again (crdt_comm_free + crdt_comm_init_*), and the rows of its shard the failed call may
 * have touched are undefined (re-sync the shard).
 * Keys in the batch are GLOBAL key ids, unless crdt_set_presharded(ctx, 1): then every
 * record is already on its owner and key_id holds its slot (no record exchange).
 *
 * Backends: RCCL over xGMI (crdt_comm_unique_id on one rank, the host broadcasts the
 * 128 bytes, crdt_comm_init_rccl on every rank; librccl is opened on first use), or a
 * caller's crdt_comm_ops table (a host transport: MPI, TCP, gloo).  No reference
 * counterpart: the reference is single-process (example/crdt_example.dart:21-25). */
enum crdt_reduce_op { CRDT_REDUCE_SUM = 0, CRDT_REDUCE_MAX = 1, CRDT_REDUCE_MIN = 2 };

typedef struct crdt_comm_ops {
    void* user;                /* passed back to every callback */
    int32_t mem;               /* CRDT_MEM_DEVICE: pointers are device memory and an operation is
                                  ordered on `stream` (a hipStream_t) like RCCL's;
                                  CRDT_MEM_HOST: the library synchronises, stages the words through
                                  host memory and the call completes before it returns */
    int32_t reserved;
    /* in-place all-reduce of n signed 64-bit words */
    int (*all_reduce_i64)(void* user, int64_t* words, uint64_t n, int32_t op, void* stream);
    /* recv[r * n + i] = send[i] of rank r */
    int (*all_gather_i64)(void* user, const int64_t* send, int64_t* recv, uint64_t n, void* stream);
    /* one grouped exchange of n_cols columns (column c has elem_bytes[c]-byte elements): to each
       peer d this rank sends elements [send_displs[d], + send_counts[d]) of every column and
       receives [recv_displs[d], + recv_counts[d]) from it; the entries for this rank are 0 (the
       library moves its own chunk itself) */
    int (*all_to_all_v)(void* user, uint32_t n_cols, const void* const* send_cols, void* const* recv_cols,
                        const uint32_t* elem_bytes, const uint64_t* send_counts, const uint64_t* send_displs,
                        const uint64_t* recv_counts, const uint64_t* recv_displs, void* stream);
} crdt_comm_ops;

#define CRDT_COMM_ID_BYTES 128
int crdt_comm_unique_id(uint8_t* id /* [CRDT_COMM_ID_BYTES] */);
int crdt_comm_init_rccl(crdt_ctx* ctx, uint32_t n_ranks, uint32_t rank, const uint8_t* id);
int crdt_comm_init_ops(crdt_ctx* ctx, uint32_t n_ranks, uint32_t rank, const crdt_comm_ops* ops);
int crdt_comm_info(const crdt_ctx* ctx, uint32_t* n_ranks, uint32_t* rank);
int crdt_comm_free(crdt_ctx* ctx);
/* The deadline of one collective crdt_merge, in ms from the call's entry (default 300000, or the
 * CRDT_COMM_TIMEOUT_MS environment variable at crdt_create; 0 = wait forever).  With RCCL every
 * host wait of the call polls the device against it and against ncclCommGetAsyncError; past it
 * the communicator is aborted and the call returns CRDT_E_COMM.  A CRDT_MEM_HOST transport blocks
 * inside its callbacks and must bound each operation itself (e.g. its own timeout); a callback
 * that fails, or returns after the deadline, fails the call the same way. */
int crdt_set_comm_timeout(crdt_ctx* ctx, uint32_t ms);
/* *state: 0 = the communicator is usable, 1 = aborted at a deadline, 2 = aborted on a transport
 * error; *phase: where the current or last collective merge is or was (static text, e.g.
 * "route_l1: record exchange").  Safe to call from another thread while crdt_merge runs (a
 * watchdog's report); the pointer stays valid for the process's life. */
int crdt_comm_state(const crdt_ctx* ctx, int32_t* state, const char** phase);
/* presharded = 1: batches hold only records this rank owns, key_id = slot (no exchange) */
int crdt_set_presharded(crdt_ctx* ctx, int presharded);

/* ---- merge strategy --------------------------------------------------------
 * crdt_merge resolves a batch either by the gather path (one launch per changeset,
 * every record reads its row: K2) or by the sorted path (the applied records are
 * partitioned by key into 4096-key buckets, each bucket's rows are read and written
 * once and its records resolved in LDS; sorted_path.inc).  Both give identical
 * rows, canonical, status and counts.  The sorted path needs: canonical >= 0,
 * capacity <= 2^28; with win_flags, also a batch frame that fits its 64-bit packed key (its
 * flagged form; on a sharded ctx the receivers take it on the all-gathered global frame, with
 * the records crossing the exchange unpacked), else the gather path runs.  path: CRDT_PATH_AUTO (default, also set by the
 * CRDT_MERGE_PATH environment variable = gather | sorted), CRDT_PATH_GATHER,
 * CRDT_PATH_SORTED (whenever allowed).  crdt_last_path reports the path the last
 * crdt_merge took (CRDT_PATH_GATHER or CRDT_PATH_SORTED). */
enum crdt_path { CRDT_PATH_AUTO = 0, CRDT_PATH_GATHER = 1, CRDT_PATH_SORTED = 2 };
int crdt_set_merge_path(crdt_ctx* ctx, int path);

/* Per-record counts (crdt_result.n_present / n_won): library extras, not part of the
 * reference's merge (crdt.dart:77-94 exposes none).  exact = 1 (default): both paths count
 * them.  exact = 0: when the sorted path runs it folds each bucket's records in any order
 * (ties on (lt, rank) decided by changeset, the local row first — the same rows, canonical and
 * status) and reports both counts as UINT64_MAX; the gather path still counts. */
int crdt_set_counts(crdt_ctx* ctx, int exact);
/* A promise that every node-id rank in later batches is < bound (the host interns node ids
 * densely; 0 = no promise, the default).  The sorted path then takes the rank part of its packed
 * key's frame from the bound instead of reading every rank in the scan.  A batch that breaks the
 * promise is never merged wrongly: where the bound is used (a single ctx's packed sorted form) the
 * call returns CRDT_E_INVALID having stored nothing and left the canonical clock as it was (the
 * check runs before any row is written); elsewhere the bound is ignored and the merge is exact. */
int crdt_set_rank_bound(crdt_ctx* ctx, uint32_t bound);
int crdt_last_path(const crdt_ctx* ctx, int* path);
/* How the last crdt_merge ran (diagnostics for tests and profiles): bit flags. */
enum crdt_plan_flags {
    CRDT_PLAN_SORTED = 1,        /* the sorted path ran */
    CRDT_PLAN_PACKED = 2,        /* ... in its packed order-free form (64-bit keys, sorted_path.inc) */
    CRDT_PLAN_TWO_LEVEL = 4,     /* ... with two partition levels (capacity > 2^20) */
    CRDT_PLAN_HIST_IN_SCAN = 8,  /* ... with its level-1 histogram counted by the scan */
    CRDT_PLAN_KEY8 = 16,         /* ... with 13-B final records (1-B key column, 4 key bits in the packed key) */
    CRDT_PLAN_KEY16 = 32,        /* ... and 14-B level-1 records (2-B key column) */
    CRDT_PLAN_HIGH_WATER = 64,   /* ... and its resolve did not read the rows at or above the table's
                                    high-water mark of written rows (never-written fill) */
    CRDT_PLAN_ANCHORED = 128,    /* retired in round 5 (the anchored sorted form, measured 0.25 ms slower
                                    per fan-in step, was removed): never set */
    CRDT_PLAN_WIRE_PACKED = 256, /* sharded ctx: records crossed the all-to-all as 16-B packed
                                    {slot, (lt, rank, changeset) key, val} instead of 20 B */
    CRDT_PLAN_OWN_IN_PLACE = 512, /* sharded ctx: the records this rank owns of its own batch were
                                    scattered straight into the receive columns (no device copy) */
    CRDT_PLAN_FLAGGED = 1024,    /* the sorted path's flagged form: per-record win flags (changeset-ordered
                                    level 2, ordered resolve, flags carried back to input order; sorted_path.inc) */
    CRDT_PLAN_ORDERED = 2048,    /* ... its ordered packed resolve (flags and / or exact n_present / n_won) */
    CRDT_PLAN_COMBINED = 4096,   /* sharded ctx: home records folded to one packed maximum per key before
                                    the all-to-all (the order-free form's map-side combine) */
    CRDT_PLAN_ROUTE_L1 = 8192,   /* sharded ctx: home records partitioned once, straight into their owners'
                                    level-1 buckets; 14-B level-1 records crossed the exchange and the
                                    owners started at level 2 (comm_path.inc, route_l1) */
    CRDT_PLAN_ROUTE_TUNED = 16384, /* sharded ctx: the way (route_l1 or the combine) came from the routing
                                    tuner, a trial or its measured choice (crdt_route_tune_info) */
    CRDT_PLAN_RL1_PIECES_SHIFT = 15, /* bits 15-17: route_l1's pipelined pieces (1-4; 0: not route_l1) */
    CRDT_PLAN_RL1_HEAD = 262144, /* route_l1 folded each owner's first level-1 digit (its 2^20 lowest slots,
                                    the Zipf head) at the sender: one packed maximum per key crossed the
                                    exchange for those keys (comm_path.inc) */
    CRDT_PLAN_COMPACT = 524288,  /* the sorted path's compact form: the records' lt field packed as
                                    (lt >> 16 - min, lt & 0xFFFF) in as many bits as the batch needs, so a record's
                                    whole 20-bit level-1 slot rides in its 64-bit key: 12-B partition records
                                    (sorted_path.inc, PackFrame::cb) */
    CRDT_PLAN_HOT_DIRECT = 1048576, /* the compact order-free form of a two-level table: level 1 wrote the records of
                                    the first CRDT_HOT_BUCKETS final buckets (keys < H * 4096) straight into their
                                    final bucket; they skipped level 2 (sorted_path.inc, HotL1) */
    CRDT_PLAN_TABLE = 2097152,    /* the last merge on this ctx was a crdt_merge_table that ran the fused table
                                    form (table_merge.inc); set alone */
    CRDT_PLAN_SYNC = 4194304,     /* ... or, with CRDT_PLAN_TABLE, one side of a crdt_sync_tables that ran its
                                    fused two-way form (set on both ctxs) */
    CRDT_PLAN_FANIN = 8388608,    /* ... or, with CRDT_PLAN_TABLE, the destination of a crdt_fanin_tables that ran
                                    its fused form */
    CRDT_PLAN_FANOUT = 16777216   /* ... or, with CRDT_PLAN_TABLE, a destination of a crdt_fanout_tables that ran
                                    its fused form (set on every destination) */
};
int crdt_last_plan(const crdt_ctx* ctx, uint32_t* flags);

/* Sharded ctx: the measured routing of order-free many-changeset fan-ins (comm_path.inc, RouteTune;
 * CRDT_ROUTE_TUNE=0 turns it off).  While every way is open (the auto settings), the first calls take each
 * way twice, the second call of each timed on the host and MAX-reduced over the ranks; later calls with the
 * same (changesets, ranks, capacity) take the fastest.  *best: -1 while the trials run (or before any such
 * call), 0 = route_l1 in 2 pipelined pieces, 1 = the map-side combine, 2 = route_l1 in 4 pieces,
 * 3 = route_l1 in one, 4 = route_l1 in 2 pieces with the head fold (CRDT_PLAN_RL1_HEAD); us[0 .. 4]: their
 * timed calls in microseconds (-1: not yet).  Every way leaves the same rows. */
int crdt_route_tune_info(const crdt_ctx* ctx, int32_t* best, int64_t* us /* [5] */);

/* The level-1 scatter's placement tuner (crdt_merge.hip, PlaceTune; CRDT_PLACE_TRIES, default 3, 1 = off):
 * crdt_reserve_scratch on a single-GPU ctx asks for that many candidate level-1 partition buffers (the
 * warm-up merge takes those that fit in 1/8 of HBM); the next sorted-path merges time the level-1 scatter
 * on each in turn, two
 * rounds, and keep the fastest (the scatter's time follows where its destination lies in physical memory;
 * DESIGN.md §6).  *n: candidates (0 / 1: no trials); *kept: the kept one (-1 while the trials run); *done:
 * merges the tuner has used (the warm-up, then two per candidate); ms[0 .. 3]: each candidate's level-1
 * scatter (the faster of its two trials). */
int crdt_place_info(const crdt_ctx* ctx, int32_t* n, int32_t* kept, int32_t* done, float* ms /* [4] */);

/* ---- measurement ---------------------------------------------------------- */
int crdt_set_timing(crdt_ctx* ctx, int enable);
int crdt_get_timing(const crdt_ctx* ctx, crdt_timing* out);

#ifdef __cplusplus
}
#endif
#endif /* CRDT_MERGE_H */
