"""The replica-network schedule of tests/_replica_net.py, checked on the C restatement alone: conditions on
the INPUTS of tests/test_gpu_replica_net.py, over the seeds it runs, so that it cannot pass for the wrong
reason (a walk that never leaves the fused forms, never raises, or whose replicas would not converge in the
reference either)."""
import functools

import numpy as np

from crdt_amd import _capi
from tests import _replica_net as rn


@functools.lru_cache(maxsize=None)
def walks():
    """seed -> (the model after the whole schedule, the stats at the end of the walk proper, its op count)."""
    out = {}
    for seed in rn.SEEDS:
        ops, n_walk = rn.schedule(seed)
        net = rn.Net().run(ops[:n_walk])
        at_walk = {k: (dict(v) if isinstance(v, dict) else v) for k, v in net.stats.items()}
        raises = net.stats["raises"]
        net.run(ops[n_walk:], first=n_walk)
        out[seed] = (net, at_walk, n_walk, net.stats["raises"] - raises)
    return out


def total(key, form=None):
    vals = [w[1][key] if form is None else w[1][key][form] for w in walks().values()]
    return sum(vals)


def test_network_shape():
    assert rn.T == _capi.TABLE_TILE and rn.K == 5 * _capi.TABLE_TILE + 9 == 10249
    assert rn.CAPS == (rn.K, rn.K + 777, 2 * rn.K, rn.K + 1) and rn.ROW_BYTES[1] == 32
    for net, _, n_walk, _ in walks().values():
        assert rn.N_OPS <= n_walk < rn.N_OPS + 10


def test_schedule_is_replayable():
    ops, n_walk = rn.schedule(3)
    again, _ = rn.schedule(3)
    assert [rn.brief(o) for o in ops] == [rn.brief(o) for o in again]
    a, b = rn.replay(3, 60), rn.replay(3, 60)
    for x, y in zip(a.model, b.model):
        assert np.array_equal(x.rows, y.rows) and x.canonical == y.canonical
    assert a.marks == b.marks


def test_external_values_are_a_function_of_the_clock():
    key = np.array([5, 5, 6], np.uint32)
    lt = np.array([77 << 16, 77 << 16, 77 << 16], np.int64)
    rank = np.array([4, 4, 4], np.uint32)
    v = rn.ext_val(key, lt, rank)
    assert v[0] == v[1] != v[2]
    big = rn.ext_val(np.arange(20000, dtype=np.uint32), np.full(20000, 1 << 50, np.int64), np.full(20000, 5, np.uint32))
    assert 0.10 < np.mean(big == rn.NULL) < 0.20 and len(np.unique(big)) > 15000


def test_convergence():
    for seed, (net, _, _, quiescence_raises) in walks().items():
        assert quiescence_raises == 0, (seed, "a quiescence call raised")
        assert rn.converged(net.model) == [], seed
        vis = net.model[0].rows["mod"][:rn.K] >= 0
        assert vis.sum() > rn.K // 2, seed                    # (they converged on something)


def test_fused_share():
    for form in rn.TABLE_FORMS:
        fused, composed = total("fused", form), total("composed", form)
        assert fused >= 0.8 * (fused + composed), (form, fused, composed)


def test_composed_and_stops():
    for form in rn.TABLE_FORMS:
        assert total("composed", form) >= 4, (form, total("composed", form))
    assert total("fanin_stops") >= 2


def test_coverage_floors():
    kinds = {}
    for _, at_walk, _, _ in walks().values():
        for k, n in at_walk["kinds"].items():
            kinds[k] = kinds.get(k, 0) + n
    assert set(kinds) == set(rn.WEIGHTS), sorted(set(rn.WEIGHTS) - set(kinds))
    assert all(n >= 8 for n in kinds.values()), kinds
    assert total("select_nothing") >= 20
    assert total("sync_both") >= 40
    assert total("ext_raises") >= 8


def test_sorted_pin_flips_the_prediction():
    """A destination pinned to the sorted path is predicted composed whatever its rows say."""
    ops, _ = rn.schedule(0)
    net = rn.Net()
    i = next(i for i, o in enumerate(ops) if o["op"] == "merge_table" and o["via"] == "table")
    net.run(ops[:i])
    free = net.predict(ops[i])
    net.pinned[ops[i]["dst"]] = True
    assert net.predict(ops[i]) is False and free is not None


def report() -> str:
    """The measured numbers of the conditions above, one line per seed and the totals."""
    lines = []
    for seed, (net, s, n_walk, _) in walks().items():
        lines.append(f"seed {seed}: {n_walk} ops {dict(sorted(s['kinds'].items()))} fused {s['fused']} "
                     f"composed {s['composed']} fanin_stops {s['fanin_stops']} select_nothing {s['select_nothing']} "
                     f"sync_both {s['sync_both']} ext_raises {s['ext_raises']}")
    lines.append("total: " + ", ".join(
        f"{f} {total('fused', f)}/{total('fused', f) + total('composed', f)} fused" for f in rn.TABLE_FORMS)
        + f", fanin_stops {total('fanin_stops')}, select_nothing {total('select_nothing')}, "
          f"sync_both {total('sync_both')}, ext_raises {total('ext_raises')}")
    return "\n".join(lines)


if __name__ == "__main__":
    print(report())
