"""A catalogue of merge steps and a runner that plays them on ONE long-lived DeviceTable (test helper).

A crdt_ctx keeps its scratch buffers between calls (DBuf::ensure keeps a buffer that is large enough), so
a merge after a larger merge, or after a merge of another form, runs on the earlier call's bytes.  Every
step resets the table's rows and canonical to its case's start, so only the context's scratch carries over
and every step is checked against a fresh oracle_run of its case; the sequences of
tests/test_gpu_scratch_reuse.py play the whole catalogue in seeded orders, forwards and backwards, with
the scratch fresh from hipMalloc or filled with 0x5A (CRDT_POISON_ALLOC=1).

The cases come from the builders the suite already has (the smallest shapes at which each form is known to
run); the plan bits a step asserts are those its source test asserts.  One or two partition levels follow
the table's capacity: a sequence starts at PHASE1_CAP rows (phase 1, one level), reserves PHASE2_CAP once
and goes on in two levels (phase 2); the phases of a step are fixed here."""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

from tests._cases import ABSENT_MOD, make_case, oracle_run
from tests.test_gpu_hot_buckets import _boundary_case, _split_case
from tests.test_gpu_parity import (RESULT_FIELDS, _cold_bucket_case, _frame_edge_case, _fused_cases, _kind_case,
                                   _late_drift_case)

PHASE1_CAP = 600_000                 # <= 2^20 rows: one partition level
PHASE2_CAP = (1 << 21) + 37          # two levels
PEER_CAP = 1_100_000                 # the second long-lived table: every case's ids fit
PEER_RANK = 250                      # a node id no case uses
U64_MAX = (1 << 64) - 1
ROW_FIELDS = ("lt", "rank", "val", "mod")

# Every switch a step may set, at its default: read_env_knobs keeps a value whose variable is unset, so each
# step sets them all.  CRDT_HOT_PROBE=0: a merge that counted the hot bins without taking them does not turn
# them off for the next merges of the table (the plan of a step would follow the steps before it).
ENV_DEFAULTS = {"CRDT_NO_FUSE": "0", "CRDT_PACKED": "1", "CRDT_SPARSE_T": "2048", "CRDT_HOT_BUCKETS": "256",
                "CRDT_HOT_PROBE": "0", "CRDT_SORTED_FORM": "0", "CRDT_FBACK_CHK": "6"}


def _wide_frame_case():              # test_sorted_wide_frame_takes_list_form
    case = make_case(seed=93, R=30, per_cs=1500, n_local=2500, n_new=1500, millis_span=6, counter_span=3,
                     n_ranks=11, tomb_frac=0.1)
    rng = np.random.default_rng(93)
    old = rng.random(len(case["lt"])) < 0.05
    case["lt"] = np.where(old, rng.integers(1, 1 << 20, len(case["lt"])), case["lt"]).astype(np.int64)
    return case


def _narrow_window_case(R=1500):     # test_sorted_wide_frame_narrow_window
    case = make_case(seed=77 + R, R=R, per_cs=50, n_local=3000, n_new=1000, millis_span=4,
                     counter_span=3, n_ranks=9, tomb_frac=0.1)
    rng = np.random.default_rng(R)
    lt = case["lt"].copy()
    hi = int(lt.max())
    pick = np.nonzero(rng.random(len(lt)) < 0.02)[0]
    lt[pick] = hi - rng.integers(0, 1 << 48, len(pick))
    lt[pick[0]] = hi - ((1 << 49) + 3)
    case["lt"] = lt
    return case


_CASES = {
    "fused0": lambda: list(_fused_cases())[0],
    "fused2": lambda: list(_fused_cases())[2],
    "fused3": lambda: list(_fused_cases())[3],
    "rows32": lambda: make_case(seed=61, R=80, per_cs=1200, n_local=3000, n_new=1500, millis_span=4,
                                counter_span=2, n_ranks=7, tomb_frac=0.1),
    **{f"kind_{k}": (lambda k=k: _kind_case(k)[0])
       for k in ("edges", "late_drift", "dup", "send_overflow", "hot", "cold", "one_level")},
    "sparse": lambda: make_case(seed=4242, n_local=10000, n_new=6384, R=8, per_cs=16384, millis_span=3,
                                counter_span=3, n_ranks=5, neg_mod_frac=0.05, local_rank=1),
    "wide_frame": _wide_frame_case,
    "narrow_window": _narrow_window_case,
    "windows": lambda: make_case(seed=84, R=5000, per_cs=20, n_local=3000, n_new=2000, millis_span=20,
                                 force=[(4500, 7, "drift")]),
    "edges99": lambda: _frame_edge_case(99),
    "edges91": lambda: _frame_edge_case(91),
    "boundary": _boundary_case,
    "host_windows": lambda: make_case(seed=3200, R=7, per_cs=3000, n_local=12_000, n_new=6000, millis_span=30,
                                      counter_span=3, n_ranks=9, local_rank=2),
    "ties": lambda: make_case(seed=79, R=300, per_cs=2000, n_local=40_000, n_new=20_000, millis_span=8,
                              counter_span=4, n_ranks=301),
    "split": _split_case,
    "late_drift97": lambda: _late_drift_case(97),
    "cold95": lambda: _cold_bucket_case(95),
    "rank_promise": lambda: make_case(seed=94, R=20, per_cs=1000, n_local=2000, n_new=500, millis_span=4,
                                      counter_span=2, n_ranks=9, tomb_frac=0.1),
    "key_range": lambda: make_case(seed=77, R=70, per_cs=1500, n_local=3000, n_new=1000, millis_span=4,
                                   counter_span=2, n_ranks=5, tomb_frac=0.1),
}


@functools.lru_cache(maxsize=None)
def case(name: str) -> dict:
    """The case of that name, built once and shared: nobody writes into it."""
    return _CASES[name]()


@functools.lru_cache(maxsize=None)
def reference(name: str):
    """oracle_run(case) once per case: (rows, result dict, win flags), shared and left unchanged."""
    rows, res, flags = oracle_run(case(name))
    rows.flags.writeable = False
    flags.flags.writeable = False
    return rows, res, flags


@dataclass(frozen=True)
class Step:
    """(name, case, settings, expectation)."""
    name: str
    case: str
    path: str = "sorted"             # set_merge_path, and the last_path() the step must report
    flags: bool = False              # per-record win flags
    counts: bool = True              # set_counts
    bound: str = "none"              # set_rank_bound: none (0) | fit (max rank + 1) | broken (max rank)
    device: bool = False             # device-resident columns
    row_bytes: int = 24
    env: dict = field(default_factory=dict)
    plan: dict = field(default_factory=dict)       # last_plan() bits the source test asserts
    plan2: dict = field(default_factory=dict)      # ... in two levels only
    phases: tuple = (1, 2)
    expect: str = "ok"               # ok | invalid (CRDT_E_INVALID) | key_range (CRDT_E_KEY_RANGE): refused calls
    bad_key: bool = False            # one key id at capacity + 5


def _gather(name, case_, **kw):
    return Step(name, case_, path="gather", flags=True, **kw)


def _free(name, case_, **kw):        # the sorted path's order-free form as test_sorted_packed_kinds runs it
    kw.setdefault("bound", "fit")
    kw.setdefault("device", True)
    return Step(name, case_, counts=False, **kw)


def _flagged(name, case_, **kw):
    plan = dict(flagged=True, **kw.pop("plan", {}))
    return Step(name, case_, flags=True, plan=plan, **kw)


PACKED = {"packed": True}
CATALOGUE = (
    # gather path, win flags, host columns
    _gather("gather_fused", "fused0"),
    _gather("gather_unfused", "fused0", env={"CRDT_NO_FUSE": "1"}),
    _gather("gather_late_dup", "fused2"),
    _gather("gather_300k_one_changeset", "fused3"),
    _gather("gather_rows32", "rows32", row_bytes=32),
    # sorted path, order-free: counts off, no flags, a rank bound, device columns
    _free("free_edges", "kind_edges", plan=PACKED),
    _free("free_late_drift", "kind_late_drift", plan=PACKED),
    _free("free_dup", "kind_dup", plan=PACKED),
    _free("free_send_overflow", "kind_send_overflow", plan=PACKED),
    _free("free_hot_split_bucket", "kind_hot", plan=PACKED),
    _free("free_cold", "kind_cold", plan=PACKED, phases=(2,)),
    _free("free_one_level", "kind_one_level", plan=PACKED, phases=(1,)),
    _free("free_sparse_kernel", "sparse", env={"CRDT_SPARSE_T": "1000000000"}, plan=PACKED),
    _free("free_list_form", "wide_frame", plan={"packed": False}),
    _free("free_narrow_window", "narrow_window", plan=PACKED),
    _free("free_windows_late_drift", "windows"),
    _free("free_no_compact", "edges99", env={"CRDT_SORTED_FORM": "1048576"}, plan={"packed": True, "compact": False},
          plan2={"two_level": True}),
    _free("free_16B_records", "edges99", env={"CRDT_SORTED_FORM": "448"}, plan={"packed": True, "key8": False},
          plan2={"two_level": True}),
    _free("free_unpacked", "edges91", env={"CRDT_PACKED": "0"}, plan={"packed": False}),
    _free("free_hot_buckets3", "boundary", env={"CRDT_HOT_BUCKETS": "3"},
          plan={"compact": True, "hist_in_scan": True, "hot_direct": True, "two_level": True}, phases=(2,)),
    _free("free_no_bound_host", "host_windows", bound="none", device=False, plan={"hist_in_scan": False}),
    # sorted path, exact counts, no flags
    Step("counted_ties", "ties"),
    Step("counted_split_bucket", "split"),
    # the flagged form
    _flagged("flagged_ties", "ties"),
    _flagged("flagged_split_bucket", "split"),
    _flagged("flagged_late_drift", "late_drift97"),
    _flagged("flagged_cold", "cold95", plan={"key16": True}, phases=(2,)),
    _flagged("flagged_split_chk0", "split", env={"CRDT_FBACK_CHK": "0", "CRDT_SORTED_FORM": "134217728"}),
    # refused calls: nothing stored, and the next step untouched by what they left behind
    Step("refused_rank_bound", "rank_promise", counts=False, bound="broken", expect="invalid"),
    Step("refused_key_gather", "key_range", path="gather", device=True, bad_key=True, expect="key_range"),
    Step("refused_key_sorted", "key_range", counts=False, device=True, bad_key=True, expect="key_range"),
)
assert len({s.name for s in CATALOGUE}) == len(CATALOGUE)


def steps_of(phase: int):
    return [s for s in CATALOGUE if phase in s.phases]


def _to_device(a):
    import torch
    return torch.from_numpy(a).cuda()


def reset(t, c: dict):
    """The table back at the case's start: every row cleared, the local rows, the canonical."""
    t.local_rank = c["local_rank"]
    t.clear_rows(0, t.capacity)
    loc = c["local"]
    keep = loc["mod"] != ABSENT_MOD
    ids = np.arange(c["n_local"], dtype=np.uint32)[keep]
    if len(ids):
        t.put_rows(ids, loc["lt"][keep], loc["rank"][keep], loc["val"][keep], loc["mod"][keep])
    t.canonical = c["c0"]


def rows_equal(t, want, n: int, tag):
    for f, a in zip(ROW_FIELDS, t.read_rows(np.arange(n, dtype=np.uint32))):
        bad = np.flatnonzero(a != want[f][:n])
        assert not len(bad), (tag, f, len(bad), bad[:5].tolist())


def run_step(t, step: Step, phase: int, setenv) -> bool:
    """One step on the caller's table: reset, settings, merge, compare, plan.  `setenv(name, value)` sets an
    environment variable (the table was created under CRDT_ENV_DYNAMIC=1, so the merge reads it).  Returns
    whether the merge was made (False: a refused call)."""
    from crdt_amd import CrdtNativeError, _capi
    c = case(step.case)
    n = c["n_ids"]
    tag = (step.name, phase)
    assert n <= t.capacity, tag
    t.set_row_bytes(step.row_bytes)
    reset(t, c)
    t.set_merge_path(step.path)
    t.set_counts(step.counts)
    top = int(c["rank"].max())
    t.set_rank_bound({"none": 0, "fit": top + 1, "broken": top}[step.bound])
    for k, v in {**ENV_DEFAULTS, **step.env}.items():
        setenv(k, v)
    key = c["key"]
    if step.bad_key:
        key = key.copy()
        key[len(key) // 2] = t.capacity + 5
    cols = [key, c["lt"], c["rank"], c["val"]]
    millis = c["millis"]
    if step.device:
        cols = [_to_device(a) for a in cols]
        millis = None if millis is None else _to_device(millis)
    if step.expect != "ok":
        try:
            t.merge(*cols, c["offsets"], c["wall"], millis=millis, win_flags=step.flags)
            status = 0
        except CrdtNativeError as e:
            status = e.status
        want = {"invalid": _capi.CRDT_E_INVALID, "key_range": _capi.CRDT_E_KEY_RANGE}[step.expect]
        assert status == want, (tag, status)
        assert t.last_path() == step.path, (tag, t.last_path())
        loc = c["local"]
        rows_equal(t, loc, c["n_local"], tag)                       # rows and canonical unchanged
        rest = t.read_rows(np.arange(c["n_local"], n, dtype=np.uint32))[3]
        assert (rest == ABSENT_MOD).all(), tag
        assert t.canonical == c["c0"], tag
        return False
    res, fl = t.merge(*cols, c["offsets"], c["wall"], millis=millis, win_flags=step.flags)
    orows, ores, oflags = reference(step.case)
    path, plan = t.last_path(), t.last_plan()
    assert path == step.path, (tag, path, plan)
    want_plan = {**step.plan, **(step.plan2 if phase == 2 else {})}
    got_plan = {k: plan[k] for k in want_plan}
    assert got_plan == want_plan, (tag, got_plan, plan)
    rows_equal(t, orows, n, tag)
    if step.flags:
        fl = fl.cpu().numpy() if step.device else fl
        bad = np.flatnonzero(fl != oflags)
        assert not len(bad), (tag, "flags", len(bad), bad[:5].tolist())
    else:
        assert fl is None, tag
    for k in RESULT_FIELDS:
        if not step.counts and path == "sorted" and k in ("n_present", "n_won"):
            assert res[k] == U64_MAX, (tag, k, res[k])
            continue
        assert res[k] == ores[k], (tag, k, res[k], ores[k])
    assert t.canonical == res["canonical_lt"], tag
    return True


def oracle_table(step: Step, capacity: int | None = None):
    """An OracleTable in the state the step's merge leaves ([0, n_ids) of `capacity` rows, default n_ids)."""
    from oracle.oracle_c import OracleTable
    c = case(step.case)
    orows, ores, _ = reference(step.case)
    if capacity is None:
        o = OracleTable(16, c["local_rank"], ores["canonical_lt"])
        o.rows = orows                                              # (shared, read only)
    else:
        o = OracleTable(capacity, c["local_rank"], ores["canonical_lt"])
        o.rows[:c["n_ids"]] = orows
    return o


def check_views(t, step: Step):
    """The other users of the context's scratch on the rows the merge left: modified_since, count_since and
    export_since (tests/test_gpu_export.check_export) at two of the step's own clocks and one above them, then
    refresh_canonical (the canonical restored after it)."""
    import tests.test_gpu_export as gx
    c = case(step.case)
    o = oracle_table(step)
    after = o.canonical
    for since in (c["c0"], after, max(after, int(o.rows["mod"].max())) + 1):
        gx.check_export(t, o, c["n_ids"], since)
    assert t.refresh_canonical(c["n_ids"]) == o.refresh(c["n_ids"]), step.name
    t.canonical = after


def check_merge_table(peer, opeer, t, step: Step):
    """peer.merge_table(t, ...) with row flags into the second long-lived table, against the composition on
    the oracle (tests/test_gpu_table_merge.oracle_merge_table)."""
    from tests.test_gpu_table_merge import oracle_merge_table
    c = case(step.case)
    n = c["n_ids"]
    ores, oflags, _ = oracle_merge_table(opeer, oracle_table(step), n, c["c0"], c["wall"])
    res, flags = peer.merge_table(t, n, c["c0"], c["wall"], row_flags=True)
    for f in RESULT_FIELDS:
        assert res[f] == ores[f], (step.name, "merge_table", f, res[f], ores[f])
    assert np.array_equal(flags.cpu().numpy(), oflags), (step.name, "merge_table flags")
    rows_equal(peer, opeer.rows, peer.capacity, (step.name, "merge_table"))
    assert peer.canonical == opeer.canonical, step.name
    rows_equal(t, reference(step.case)[0], n, (step.name, "merge_table src untouched"))


def check_merge_from(peer, opeer, t, step: Step):
    """merge_from once from each side: the peer takes the table's rows, then the table the peer's."""
    import tests.test_gpu_export as gx
    c = case(step.case)
    n = c["n_ids"]
    ores, oflags, m = gx._oracle_merge_from(opeer, oracle_table(step), n, c["c0"], c["wall"])
    res, flags = peer.merge_from(t, n, c["c0"], c["wall"])
    for f in RESULT_FIELDS:
        assert res[f] == ores[f], (step.name, "peer.merge_from", f, res[f], ores[f])
    assert len(flags) == m and np.array_equal(flags.cpu().numpy(), oflags), (step.name, "peer.merge_from flags")
    rows_equal(peer, opeer.rows, peer.capacity, (step.name, "peer.merge_from"))
    assert peer.canonical == opeer.canonical
    # the other way: every peer row the table can hold, merged with exact counts and win flags
    n = min(t.capacity, peer.capacity)
    ot = oracle_table(step, t.capacity)
    t.set_merge_path("auto")
    t.set_counts(True)
    t.set_rank_bound(0)
    ores, oflags, m = gx._oracle_merge_from(ot, opeer, n, c["c0"], c["wall"] + 1)
    res, flags = t.merge_from(peer, n, c["c0"], c["wall"] + 1)
    for f in RESULT_FIELDS:
        assert res[f] == ores[f], (step.name, "t.merge_from", f, res[f], ores[f])
    assert len(flags) == m and np.array_equal(flags.cpu().numpy(), oflags), (step.name, "t.merge_from flags")
    rows_equal(t, ot.rows, t.capacity, (step.name, "t.merge_from"))
    assert t.canonical == ot.canonical


def run_phase(t, peer, opeer, phase: int, seed: int, setenv, ran: dict, counter: list):
    """A seeded permutation of the phase's steps forwards, then the same permutation backwards; the views after
    every successful step, merge_table after every fourth, merge_from once (in phase 2's forward pass)."""
    steps = steps_of(phase)
    order = np.random.default_rng(1000 * phase + seed).permutation(len(steps)).tolist()
    due = -1
    for pos, i in enumerate(order + order[::-1]):
        step = steps[i]
        ok = run_step(t, step, phase, setenv)
        ran[(step.name, phase)] = ran.get((step.name, phase), 0) + 1
        if phase == 2 and pos == len(order) // 2:
            due = 0
        if not ok:
            continue
        check_views(t, step)
        counter[0] += 1
        if counter[0] % 4 == 0:
            check_merge_table(peer, opeer, t, step)
        if due == 0:
            check_merge_from(peer, opeer, t, step)
            due = 1
            ran["merge_from"] = ran.get("merge_from", 0) + 1


def run_sequence(seed: int, setenv, phases=(1, 2)):
    """One context through the phases' catalogue (see the module text); fails unless every step ran twice
    in each of its phases."""
    from crdt_amd import DeviceTable
    from oracle.oracle_c import OracleTable
    t = DeviceTable(0, local_rank=0, capacity=PHASE1_CAP)
    peer = DeviceTable(0, local_rank=PEER_RANK, capacity=PEER_CAP)
    opeer = OracleTable(PEER_CAP, PEER_RANK, 0)
    ran, counter = {}, [0]
    try:
        for phase in phases:
            if phase == 2:
                t.reserve(PHASE2_CAP)
                assert t.capacity == PHASE2_CAP
            else:
                assert t.capacity == PHASE1_CAP
            run_phase(t, peer, opeer, phase, seed, setenv, ran, counter)
    finally:
        t.close()
        peer.close()
    want = {(s.name, p): 2 for p in phases for s in steps_of(p)}
    if 2 in phases:
        want["merge_from"] = 1
    assert ran == want, sorted(set(want.items()) ^ set(ran.items()))
    return ran
