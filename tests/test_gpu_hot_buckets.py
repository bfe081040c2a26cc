"""The hot-bucket level 1 of the sorted path (CRDT_HOT_BUCKETS=H, CRDT_PLAN_HOT_DIRECT): on a two-level table
the compact order-free form writes the records of the first H final buckets (keys < H * 4096) straight into
their final bucket in its level-1 scatter; they skip level 2.  Every case compares all rows, the canonical and
the result fields with the C oracle and checks that the plan reports whether the path ran."""
import numpy as np
import pytest

from tests._cases import ABSENT_MOD, make_case
from tests.test_gpu_parity import _fanin_reference, compare_with_oracle

pytestmark = pytest.mark.gpu

_TWO = (1 << 20) + 3            # two partition levels


def _run(case, capacity=_TWO, **kw):
    """The order-free sorted form whose level-1 histogram the scan counts (device columns, a rank bound)."""
    args = dict(path="sorted", flags=False, counts=False, device_cols=True, capacity=capacity,
                rank_bound=int(case["rank"].max()) + 1)
    args.update(kw)
    res = compare_with_oracle(case, **args)
    assert res["path"] == "sorted"
    return res


def _boundary_case():
    """Keys over five final buckets (tombstones, invisible rows): a small H puts the hot boundary inside them."""
    return make_case(seed=311, R=48, per_cs=2500, n_local=16000, n_new=4480, millis_span=6, counter_span=3,
                     n_ranks=9, tomb_frac=0.2, neg_mod_frac=0.05)


def _shift_keys(case, by):
    """The same case with every key (and local row) `by` slots higher: the rows below are absent."""
    out = dict(case)
    out["key"] = (case["key"] + np.uint32(by)).astype(np.uint32)
    loc = case["local"]
    pad = {"lt": np.zeros(by, np.int64), "rank": np.zeros(by, np.uint32), "val": np.zeros(by, np.uint32),
           "mod": np.full(by, ABSENT_MOD, np.int64)}
    out["local"] = {f: np.concatenate([pad[f], loc[f]]) for f in ("lt", "rank", "val", "mod")}
    out["n_local"] = case["n_local"] + by
    out["n_ids"] = case["n_ids"] + by
    return out


@pytest.mark.parametrize("H", [0, 1, 3])
def test_hot_boundary_inside_keys(gpu_device, monkeypatch, H):
    monkeypatch.setenv("CRDT_HOT_BUCKETS", str(H))
    res = _run(_boundary_case())
    assert res["plan"]["compact"] and res["plan"]["hist_in_scan"], res["plan"]
    assert res["plan"]["hot_direct"] == (H > 0), res["plan"]


def _split_case():
    return make_case(seed=85, R=120, per_cs=2000, n_local=3000, n_new=1000, millis_span=4, counter_span=3,
                     n_ranks=9, tomb_frac=0.2, neg_mod_frac=0.05)


def test_everything_hot_one_split_bucket(gpu_device, monkeypatch):
    """Every record in final bucket 0 (240K records: four parts, folded and carried): level 2 has nothing to
    partition."""
    monkeypatch.setenv("CRDT_HOT_BUCKETS", "64")
    res = _run(_split_case())
    assert res["plan"]["hot_direct"], res["plan"]


@pytest.mark.parametrize("share", ["0", None])
def test_nothing_hot(gpu_device, monkeypatch, share):
    """The same records shifted past the hot buckets.  CRDT_HOT_SHARE=0: the path runs with empty hot digits;
    the default share: the scan's count of hot records (none) keeps the merge off the path."""
    monkeypatch.setenv("CRDT_HOT_BUCKETS", "64")
    if share is not None:
        monkeypatch.setenv("CRDT_HOT_SHARE", share)
    res = _run(_shift_keys(_split_case(), 64 * 4096))
    assert res["plan"]["hot_direct"] == (share == "0"), res["plan"]


def test_hot_rest_of_digit0_and_digit1(gpu_device, monkeypatch):
    monkeypatch.setenv("CRDT_HOT_BUCKETS", "64")
    n_ids = (1 << 20) + 9000
    case = make_case(seed=312, R=16, per_cs=20000, n_local=n_ids - 5000, n_new=5000, millis_span=6, counter_span=3,
                     n_ranks=9, tomb_frac=0.1, absent_frac=0.3)
    res = _run(case, capacity=n_ids)
    assert res["plan"]["hot_direct"] and res["plan"]["two_level"], res["plan"]


def test_several_tiles_per_changeset(gpu_device, monkeypatch):
    """Two level-1 tiles and a ragged tail per changeset: the odd tile fills hot and ordinary digits downwards."""
    monkeypatch.setenv("CRDT_HOT_BUCKETS", "8")
    case = make_case(seed=313, R=6, per_cs=60000, n_local=50000, n_new=20000, millis_span=6, counter_span=3,
                     n_ranks=9, tomb_frac=0.1)
    res = _run(case)
    assert res["plan"]["hot_direct"], res["plan"]


def test_stop_point_in_the_middle(gpu_device, monkeypatch):
    """A raising record in changeset 20 of 40: the exception fields are the oracle's and nothing of the
    changesets from the stop point on is stored."""
    monkeypatch.setenv("CRDT_HOT_BUCKETS", "2")
    case = make_case(seed=314, R=40, per_cs=1500, n_local=12000, n_new=4384, millis_span=6, counter_span=3,
                     n_ranks=9, tomb_frac=0.1, force=[(20, 700, "dup")])
    res = _run(case)
    assert res["exc_changeset"] == 20, res
    assert res["plan"]["hot_direct"], res["plan"]


def test_sparse_hot_buckets(gpu_device, monkeypatch):
    """Four final buckets of about 1600 records each, below CRDT_SPARSE_T = 2048; two of them hot."""
    monkeypatch.setenv("CRDT_HOT_BUCKETS", "2")
    case = make_case(seed=315, R=64, per_cs=100, n_local=12000, n_new=4384, millis_span=6, counter_span=3,
                     n_ranks=9, tomb_frac=0.1)
    assert np.bincount(case["key"] >> 12).max() < 2048
    res = _run(case)
    assert res["plan"]["hot_direct"], res["plan"]


@pytest.mark.parametrize("form", ["flagged", "counts", "no_compact", "no_rank_bound", "one_level", "low_share"])
def test_forms_that_do_not_take_it(gpu_device, monkeypatch, form):
    """The scan counted the hot bins apart (or not at all); these forms get today's partition and the
    oracle's rows."""
    monkeypatch.setenv("CRDT_HOT_BUCKETS", "3")
    kw = {"flagged": dict(flags=True, counts=True), "counts": dict(counts=True),
          "no_compact": {}, "no_rank_bound": dict(rank_bound=0), "one_level": dict(capacity=100_000),
          "low_share": {}}[form]
    if form == "no_compact":
        monkeypatch.setenv("CRDT_SORTED_FORM", "1048576")
    if form == "low_share":         # three of the five buckets are hot: 60 % of the records, below the share asked
        monkeypatch.setenv("CRDT_HOT_SHARE", "90")
    res = _run(_boundary_case(), **kw)
    assert not res["plan"]["hot_direct"], res["plan"]
    assert res["plan"]["hist_in_scan"] == (form != "no_rank_bound"), res["plan"]


def test_key_out_of_range(gpu_device, monkeypatch):
    import torch
    from crdt_amd import CrdtNativeError, DeviceTable
    monkeypatch.setenv("CRDT_HOT_BUCKETS", "64")
    case = make_case(seed=77, R=70, per_cs=1500, n_local=3000, n_new=1000, millis_span=4, counter_span=2,
                     n_ranks=5, tomb_frac=0.1)
    key = case["key"].copy()
    key[len(key) // 2] = _TWO + 5
    t = DeviceTable(0, local_rank=case["local_rank"], capacity=_TWO)
    t.set_merge_path("sorted")
    t.set_counts(False)
    t.set_rank_bound(int(case["rank"].max()) + 1)
    loc = case["local"]
    keep = loc["mod"] != ABSENT_MOD
    ids = np.arange(case["n_local"], dtype=np.uint32)[keep]
    t.put_rows(ids, loc["lt"][keep], loc["rank"][keep], loc["val"][keep], loc["mod"][keep])
    t.canonical = case["c0"]
    every = np.arange(case["n_ids"], dtype=np.uint32)
    before = t.read_rows(every)
    cols = [torch.from_numpy(c).cuda() for c in (key, case["lt"], case["rank"], case["val"])]
    with pytest.raises(CrdtNativeError, match="key id out of range"):
        t.merge(*cols, case["offsets"], case["wall"], win_flags=False)
    assert t.last_path() == "sorted"
    assert t.last_plan()["hot_direct"], t.last_plan()
    for a, b in zip(before, t.read_rows(every)):
        assert np.array_equal(a, b)
    assert t.canonical == case["c0"]
    t.close()


def test_reuse_grow_and_switch_off(gpu_device, monkeypatch):
    """One table: a merge with H = 64, one three times larger (the buffers grow), one with the switch off
    (re-read per merge); each against the oracle continued from the same state."""
    import torch
    from crdt_amd import DeviceTable
    from oracle.oracle_c import OracleTable
    monkeypatch.setenv("CRDT_ENV_DYNAMIC", "1")
    monkeypatch.setenv("CRDT_HOT_BUCKETS", "64")
    kw = dict(n_local=6000, n_new=3000, per_cs=3000, millis_span=6, counter_span=3, n_ranks=9, tomb_frac=0.15)
    cases = [make_case(seed=321, R=16, **kw), make_case(seed=322, R=48, **kw), make_case(seed=323, R=16, **kw)]
    first = cases[0]
    n_ids = first["n_ids"]
    t = DeviceTable(0, local_rank=first["local_rank"], capacity=_TWO)
    t.set_merge_path("sorted")
    t.set_counts(False)
    t.set_rank_bound(9)
    o = OracleTable(n_ids, first["local_rank"], first["c0"])
    loc = first["local"]
    ids = np.arange(first["n_local"], dtype=np.uint32)
    t.put_rows(ids, loc["lt"], loc["rank"], loc["val"], loc["mod"])
    o.put_rows(ids, loc["lt"], loc["rank"], loc["val"], loc["mod"])
    t.canonical = first["c0"]
    every = np.arange(n_ids, dtype=np.uint32)
    for step, case in enumerate(cases):
        if step == 2:
            monkeypatch.setenv("CRDT_HOT_BUCKETS", "0")
        cols = [torch.from_numpy(case[f]).cuda() for f in ("key", "lt", "rank", "val")]
        res, _ = t.merge(*cols, case["offsets"], case["wall"], win_flags=False)
        ores, _ = o.merge(case["key"], case["lt"], case["rank"], case["val"], case["offsets"], case["wall"],
                          want_flags=False)
        ores = ores.as_dict()
        plan = t.last_plan()
        assert t.last_path() == "sorted" and plan["compact"], (step, plan)
        assert plan["hot_direct"] == (step < 2), (step, plan)
        for f in ("status", "n_stored", "exc_changeset", "exc_index", "canonical_lt", "drift_ms", "counter"):
            assert res[f] == ores[f], (step, f, res[f], ores[f])
        for f, a in zip(("lt", "rank", "val", "mod"), t.read_rows(every)):
            assert np.array_equal(a, np.array(o.rows[f])), (step, f)
    t.close()


def test_fanin_shape(gpu_device, monkeypatch):
    """The bench's shape (gen_fanin, Zipf 0.8) at 3M records over 2^22 keys, with and without the hot buckets."""
    from crdt_amd import DeviceTable
    from crdt_amd.workload import gen_fanin
    K, total, R = 1 << 22, 3_000_000, 64
    ref, rows = _fanin_reference(K, total, R)
    wl = gen_fanin(total=total, R=R, K=K, n_local=K // 2, s=0.8, device="cuda")
    loc, own = wl["local"], wl["owned"]
    for H in (0, 64):
        monkeypatch.setenv("CRDT_HOT_BUCKETS", str(H))
        t = DeviceTable(0, local_rank=0, capacity=wl["capacity"])
        t.set_counts(False)
        t.set_merge_path("sorted")
        t.set_rank_bound(R + 1)
        t.put_rows(loc["slot"], loc["lt"], loc["rank"], loc["val"], loc["mod"])
        t.canonical = wl["c0"]
        res, _ = t.merge(own["key"], own["lt"], own["rank"], own["val"], wl["owned_offsets"], wl["wall"],
                         win_flags=False)
        plan = t.last_plan()
        assert plan["compact"] and plan["hot_direct"] == (H > 0), plan
        for f in ("status", "n_stored", "canonical_lt"):
            assert res[f] == ref[f], (H, f)
        for a, b in zip(t.read_rows(np.arange(wl["capacity"], dtype=np.uint32)), rows):
            assert np.array_equal(a, b), H
        t.close()


def test_skip_after_unused_hot_bins_then_probe_again(gpu_device, monkeypatch):
    """A merge whose hot bins went unused (no hot record) turns them off in the next 15 scans of the table — those
    merges take the plain partition even with every key hot — and the 16th counts them again.  Rows, canonical
    and result fields follow the oracle through the whole sequence."""
    import torch
    from crdt_amd import DeviceTable
    from oracle.oracle_c import OracleTable
    monkeypatch.setenv("CRDT_HOT_BUCKETS", "64")
    kw = dict(n_local=3000, n_new=1000, R=4, per_cs=500, millis_span=6, counter_span=3, n_ranks=9, tomb_frac=0.15)
    cold = _shift_keys(make_case(seed=331, **kw), 64 * 4096)
    n_ids = cold["n_ids"]
    t = DeviceTable(0, local_rank=cold["local_rank"], capacity=_TWO)
    t.set_merge_path("sorted")
    t.set_counts(False)
    t.set_rank_bound(9)
    o = OracleTable(n_ids, cold["local_rank"], cold["c0"])
    t.canonical = cold["c0"]
    every = np.arange(n_ids, dtype=np.uint32)
    for step in range(17):
        case = cold if step == 0 else make_case(seed=331 + step, **kw)
        cols = [torch.from_numpy(case[f]).cuda() for f in ("key", "lt", "rank", "val")]
        res, _ = t.merge(*cols, case["offsets"], case["wall"], win_flags=False)
        ores, _ = o.merge(case["key"], case["lt"], case["rank"], case["val"], case["offsets"], case["wall"],
                          want_flags=False)
        ores = ores.as_dict()
        plan = t.last_plan()
        assert t.last_path() == "sorted" and plan["compact"], (step, plan)
        assert plan["hot_direct"] == (step == 16), (step, plan)
        for f in ("status", "n_stored", "canonical_lt"):
            assert res[f] == ores[f], (step, f, res[f], ores[f])
    for f, a in zip(("lt", "rank", "val", "mod"), t.read_rows(every)):
        assert np.array_equal(a, np.array(o.rows[f])), f
    t.close()
