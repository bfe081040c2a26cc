"""Every form of the sorted apply on one small batch: each CRDT_SORTED_FORM and CRDT_FBACK_CHK value the suite
uses, CRDT_HOT_BUCKETS=0 and CRDT_PACKED=0, on a two-level and a one-level table, in the order-free, the
exact-count and the flagged mode.  Rows, result fields and flags equal the C oracle's, and the path and
last_plan() equal tests/golden/sorted_plan_bits.json, which a build of the commit before the sorted apply was
split into phases recorded (run_mode() is what recorded it): the form a call takes is part of the contract."""
import json
import os

import numpy as np
import pytest

from tests._cases import make_case, oracle_run
from tests.test_gpu_parity import RESULT_FIELDS, device_run

pytestmark = pytest.mark.gpu

FORMS = ("0", "64", "128", "256", "448", "512", "1024", "2048", "8192", "32768", "65536", "131072", "1048576",
         "2097152", "4194304", "8388608", "14680064", "16777216", "33554432", "67108864", "134217728", "268435456",
         "536870912", "2147483648")
ENVS = ([{"CRDT_SORTED_FORM": f} for f in FORMS] +
        [{"CRDT_FBACK_CHK": k} for k in ("0", "4", "6")] +
        [{"CRDT_FBACK_CHK": k, "CRDT_SORTED_FORM": "134217728"} for k in ("0", "4")] +
        [{"CRDT_HOT_BUCKETS": "0"}, {"CRDT_PACKED": "0"}])
CAPS = {"two_level": (1 << 20) + 3, "one_level": 1 << 20}
MODES = {"order_free": dict(flags=False, counts=False), "counts": dict(flags=False, counts=True),
         "flagged": dict(flags=True, counts=True)}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sorted_plan_bits.json")

_shared = {}


def env_id(env):
    return "-".join(f"{k[5:].lower()}{v}" for k, v in sorted(env.items()))


def shared_case():
    """The batch of test_flagged_back_pass_search_forms (R = 120, 2000 records per changeset) and the oracle's
    answer, computed once."""
    if "case" not in _shared:
        case = make_case(seed=85, R=120, per_cs=2000, n_local=3000, n_new=1000, millis_span=4, counter_span=3,
                         n_ranks=9, tomb_frac=0.2, neg_mod_frac=0.05)
        _shared["case"] = case
        _shared["oracle"] = oracle_run(case)
    return _shared["case"], _shared["oracle"]


def golden_plans():
    if "golden" not in _shared:
        with open(GOLDEN) as fh:
            _shared["golden"] = json.load(fh)
    return _shared["golden"]


def run_mode(level, mode):
    """One merge under the environment as it stands: (rows, result with path and plan, flags)."""
    case, _ = shared_case()
    return device_run(case, device_cols=True, capacity=CAPS[level], path="sorted",
                      rank_bound=int(case["rank"].max()) + 1, **MODES[mode])


def plan_record(res):
    """What the golden table keeps of a call: the path, the plan bits that are set, route_l1's pieces."""
    plan = res["plan"]
    return {"path": res["path"], "on": sorted(k for k, v in plan.items() if v is True),
            "rl1_pieces": plan["rl1_pieces"]}


@pytest.mark.parametrize("level", list(CAPS))
@pytest.mark.parametrize("env", ENVS, ids=env_id)
def test_sorted_form(gpu_device, monkeypatch, env, level):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    golden = golden_plans()
    _, (orows, ores, oflags) = shared_case()
    for mode, kw in MODES.items():
        rows, res, flags = run_mode(level, mode)
        tag = (env, level, mode)
        for col, got in zip(("lt", "rank", "val", "mod"), rows):
            assert np.array_equal(got, orows[col]), (tag, col)
        if kw["flags"]:
            assert np.array_equal(flags, oflags), tag
        for k in RESULT_FIELDS:
            if not kw["counts"] and res["path"] == "sorted" and k in ("n_present", "n_won"):
                assert res[k] == (1 << 64) - 1, (tag, k, res[k])
            else:
                assert res[k] == ores[k], (tag, k, res[k], ores[k])
        want = golden[f"{env_id(env)}/{level}/{mode}"]
        assert plan_record(res) == want, (tag, plan_record(res), want)
