"""Row sets and the numpy model for the replica diff and the block digests (crdt_diff_tables,
crdt_digest_rows), pure numpy (test helper; nothing here imports the library).

``gen_diff_pair`` starts both replicas from one ``tests/_table_cases.gen_rows`` table and perturbs disjoint
random subsets of its rows, one subset per way two replicas can come to differ (or to look different and be
equal), and from 64 rows on plants nine rows that hold the comparisons a kernel can get wrong.  At least 40 % of
the rows stay equal and every class occurs in every shape of at least 64 rows: the generator asserts both."""
from __future__ import annotations

import numpy as np

from tests import _table_cases as tc
from tests._cases import ABSENT_MOD, NULL

T = 2048                                  # rows per tile of both kernels (table_diff.inc: kTmTile)
GRID = 2048                               # their capped grid (kDfGrid)
LARGE = (GRID + 1) * T + 5                # more tiles than workgroups, a partial last tile
A_AHEAD, B_AHEAD, CONFLICT = 1, 2, 4
NONE = (1 << 64) - 1                      # first_diff when nothing differs
PLANT_FROM = 64
FIELDS = ("n_a_ahead", "n_b_ahead", "n_conflict", "n_visible_a", "n_visible_b", "first_diff")
P = [np.uint64(x) for x in (0x9E3779B97F4A7C15, 0xC2B2AE3D27D4EB4F, 0x165667B19E3779F9, 0xD6E8FEB86659FD93,
                            0xFF51AFD7ED558CCD)]                      # bench.row_digests' constants

# the random classes: name -> the byte every row of the class must get
CLASSES = {"a_newer_lt": A_AHEAD, "b_newer_lt": B_AHEAD, "a_higher_rank": A_AHEAD, "b_higher_rank": B_AHEAD,
           "conflict_live": CONFLICT, "conflict_tombstone": CONFLICT, "mod_only": 0,
           "a_negative_mod": B_AHEAD, "b_negative_mod": A_AHEAD, "a_cleared": B_AHEAD, "b_cleared": A_AHEAD,
           "both_invisible": 0, "a_only": A_AHEAD, "b_only": B_AHEAD}
SHARE = 0.02                              # of the rows, per random class (the two cleared ranges: 1/16 each)

_X = int(tc.STAMPS[0]) & ~(1 << 31)       # an lt with bit 31 clear; with it set, 32768 ms later (inside the drift)
_S5 = int(tc.STAMPS[5])
# id -> ((lt, rank, val, mod) of a, of b, the byte); "last" is row n_rows - 1
PLANTED = {
    0: ((_X, 2, 10, _S5), (_X | (1 << 31), 2, 10, _S5), B_AHEAD),           # lts that differ only in bit 31
    1: ((_X | (1 << 31), 2, 11, _S5), (_X, 2, 11, _S5), A_AHEAD),
    2: ((_X, 2, 12, _S5), (_X | -(1 << 63), 2, 12, _S5), A_AHEAD),          # ... only in bit 63: lt is signed
    3: ((-(5 << 16), 3, 13, _S5), (5 << 16, 3, 13, _S5), B_AHEAD),          # a negative lt against a positive one
    4: ((_S5, 0x7FFFFFFF, 14, _S5), (_S5, 0x80000000, 14, _S5), B_AHEAD),   # rank is unsigned
    5: ((_S5, 0x80000000, 15, _S5), (_S5, 0x7FFFFFFF, 15, _S5), A_AHEAD),
    6: ((_S5, 4, 16, _S5), (_S5, 4, NULL, _S5), CONFLICT),                  # one hlc, a tombstone against a live value
    7: ((_S5, 4, 17, _S5), (_S5, 4, 17, int(tc.STAMPS[9])), 0),             # only mod differs
    "last": ((_X | (1 << 31), 1, 18, _S5), (_X, 1, 18, _S5), A_AHEAD),
}


def _rows_of(d: dict, written: np.ndarray, clear) -> dict:
    ids = np.flatnonzero(written).astype(np.uint32)
    return {"n_rows": len(written), "ids": ids, "lt": d["lt"][ids], "rank": d["rank"][ids], "val": d["val"][ids],
            "mod": d["mod"][ids], "clear": clear}


def gen_diff_pair(n_rows: int, seed: int) -> tuple[dict, dict]:
    """(rows of a, rows of b) in tests/_table_cases' form ({ids, lt, rank, val, mod, clear}); ``a["classes"]``
    maps every class (and "planted") to its row ids."""
    base = tc.gen_rows(n_rows, seed)
    rng = np.random.default_rng(seed + 104729)
    written = np.zeros(n_rows, bool)
    written[base["ids"]] = True
    d = {k: np.zeros(n_rows, base[k].dtype) for k in ("lt", "rank", "val", "mod")}
    for k in d:
        d[k][base["ids"]] = base[k]
    a, b = {k: v.copy() for k, v in d.items()}, {k: v.copy() for k, v in d.items()}
    wa, wb = written.copy(), written.copy()
    span = n_rows // 16
    clear_a, clear_b = (n_rows // 3, span), (2 * n_rows // 3, span)
    taken = np.zeros(n_rows, bool)
    for first, count in (clear_a, clear_b):
        taken[first:first + count] = True
    planted = {}
    if n_rows >= PLANT_FROM:
        planted = {(n_rows - 1 if k == "last" else k): v for k, v in PLANTED.items()}
        taken[list(planted)] = True
    classes = {}
    free = rng.permutation(np.flatnonzero(written & (d["mod"] >= 0) & ~taken))   # visible on both sides so far
    take = max(1, int(n_rows * SHARE))
    for name in CLASSES:
        if name in ("a_cleared", "b_cleared"):
            continue
        classes[name], free = np.sort(free[:take]), free[take:]
    c = classes
    a["lt"][c["a_newer_lt"]] += 3 << 16
    b["lt"][c["b_newer_lt"]] += (1 << 16) + 1
    a["rank"][c["a_higher_rank"]] += 1
    b["rank"][c["b_higher_rank"]] += 2
    live = c["conflict_live"]
    a["val"][live] = rng.integers(0, 1 << 19, len(live))
    b["val"][live] = a["val"][live] + (1 << 19)
    tomb = c["conflict_tombstone"]
    a["val"][tomb[::2]], b["val"][tomb[::2]] = NULL, 7          # a tombstone on either side against a live value
    a["val"][tomb[1::2]], b["val"][tomb[1::2]] = 8, NULL
    b["mod"][c["mod_only"]] = tc.STAMPS[rng.integers(0, tc.N_STAMPS, len(c["mod_only"]))] + 1
    a["mod"][c["a_negative_mod"]] = -(1 << 20) - 3
    b["mod"][c["b_negative_mod"]] = -1
    both = c["both_invisible"]                                  # different garbage under two negative mods
    a["mod"][both], b["mod"][both] = -(1 << 30), -2
    b["lt"][both] += 99 << 16
    b["val"][both] = 0x12345
    wb[c["a_only"]] = False                                     # never written on the other side
    wa[c["b_only"]] = False
    for k, (ra, rb, _) in planted.items():
        wa[k] = wb[k] = True
        for j, name in enumerate(("lt", "rank", "val", "mod")):
            a[name][k], b[name][k] = ra[j], rb[j]
    ra, rb = _rows_of(a, wa, clear_a), _rows_of(b, wb, clear_b)
    da, db = tc.dense(ra, n_rows), tc.dense(rb, n_rows)
    classes["a_cleared"] = np.flatnonzero((np.arange(n_rows) >= clear_a[0]) & (np.arange(n_rows) < sum(clear_a)) &
                                          (db["mod"] >= 0))
    classes["b_cleared"] = np.flatnonzero((np.arange(n_rows) >= clear_b[0]) & (np.arange(n_rows) < sum(clear_b)) &
                                          (da["mod"] >= 0))
    classes["planted"] = np.array(sorted(planted), np.int64)
    if n_rows >= PLANT_FROM:                                    # what the issue asks of every such shape
        flags = model_diff(da, db, n_rows)[0]
        assert np.mean(flags == 0) >= 0.40, (n_rows, seed, np.mean(flags == 0))
        for name, byte in CLASSES.items():
            assert len(classes[name]) > 0 and np.all(flags[classes[name]] == byte), (n_rows, seed, name)
        for k, (_, _, byte) in planted.items():
            assert flags[k] == byte, (n_rows, seed, k)
    ra["classes"] = classes
    return ra, rb


def max_lt(*rows) -> int:
    """The largest lt any of the row sets holds: a canonical at or above it keeps every recv() quiet."""
    return max([int(r["lt"].max()) for r in rows if len(r["lt"])] + [0])


def model_diff(a: dict, b: dict, n_rows: int):
    """(flag bytes, dict of the six crdt_diff fields) of two dense tables ({lt, rank, val, mod} arrays)."""
    al, ar, av, am = (np.asarray(a[k][:n_rows]) for k in ("lt", "rank", "val", "mod"))
    bl, br, bv, bm = (np.asarray(b[k][:n_rows]) for k in ("lt", "rank", "val", "mod"))
    va, vb = am >= 0, bm >= 0
    agt = (al > bl) | ((al == bl) & (ar > br))
    bgt = (bl > al) | ((bl == al) & (br > ar))
    a_ahead, b_ahead = va & (~vb | agt), vb & (~va | bgt)
    conflict = va & vb & ~agt & ~bgt & (av != bv)
    flags = (a_ahead * A_AHEAD + b_ahead * B_AHEAD + conflict * CONFLICT).astype(np.uint8)
    nz = np.flatnonzero(flags)
    return flags, {"n_a_ahead": int(a_ahead.sum()), "n_b_ahead": int(b_ahead.sum()), "n_conflict": int(conflict.sum()),
                   "n_visible_a": int(va.sum()), "n_visible_b": int(vb.sum()),
                   "first_diff": int(nz[0]) if len(nz) else NONE}


def model_digest(dense: dict, n_rows: int, block_rows: int, state: bool) -> np.ndarray:
    """crdt_digest_rows' words of a dense table: the wrapping sums of bench.row_digests' mix per block."""
    if n_rows == 0:
        return np.zeros(0, np.uint64)
    lt = np.ascontiguousarray(dense["lt"][:n_rows], np.int64).view(np.uint64)
    mod = np.ascontiguousarray(dense["mod"][:n_rows], np.int64)
    rv = (np.asarray(dense["rank"][:n_rows]).astype(np.uint64) << np.uint64(32)) | \
        np.asarray(dense["val"][:n_rows]).astype(np.uint64)
    with np.errstate(over="ignore"):
        h = lt * P[0] ^ rv * P[2] ^ np.arange(n_rows, dtype=np.uint64) * P[3]
        if not state:
            h ^= mod.view(np.uint64) * P[1]
        h ^= h >> np.uint64(29)
        h *= P[4]
        h ^= h >> np.uint64(32)
        if state:
            h[mod < 0] = 0
        return np.add.reduceat(h, np.arange(0, n_rows, block_rows))


def fill_dense(capacity: int) -> dict:
    """A never-written table."""
    return tc.dense({"ids": np.zeros(0, np.uint32), "lt": np.zeros(0, np.int64), "rank": np.zeros(0, np.uint32),
                     "val": np.zeros(0, np.uint32), "mod": np.zeros(0, np.int64), "clear": (0, 0)}, capacity)


assert ABSENT_MOD < 0
