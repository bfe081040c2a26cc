"""Hlc.send(R) at the wall (hlc.dart:51-74: drift first, then counter overflow, else the new canonical) gives
one answer wherever the library evaluates it: put_stamped, merge (the device-side resolve), merge_table, and
each step of sync_tables.  The receiving replica's canonical is set to values around the two limits and
every incoming lt lies below it, so R is that canonical and no recv() can raise: what the call reports is
send's own status, drift, counter and canonical, as the C restatement's or_send gives them
(oracle.oracle_c.send_scalar), and the rows and canonicals are the oracle's.  64-row tables: one partial
tile.  Everything is integer data: every comparison is exact."""
import numpy as np
import pytest

import tests.test_gpu_sync_tables as gs
import tests.test_gpu_table_merge as gt
from crdt_amd import DeviceTable, _capi
from oracle.oracle_c import OracleTable, send_scalar
from tests import _ctx_sequence as seq
from tests import _sync_cases as sc
from tests import _table_cases as tc

pytestmark = pytest.mark.gpu

N = 64
W = tc.MERGE_WALL                                            # above every generated stamp's millis
OK, DRIFT, OVERFLOW = _capi.CRDT_OK, _capi.CRDT_CLOCK_DRIFT, _capi.CRDT_OVERFLOW
QUIET = W << 16                                              # the other replica of a sync: above every lt, sends fine

# (millis, counter) of the canonical -> (status, drift_ms, counter, canonical left) of send at the wall W
CASES = {
    "drift_limit": ((W + 60000, 5), (OK, 0, 0, ((W + 60000) << 16) | 6)),
    "drift_limit_plus_1": ((W + 60001, 5), (DRIFT, 60001, 0, ((W + 60001) << 16) | 5)),
    "counter_limit": ((W, 0xFFFE), (OK, 0, 0, (W << 16) | 0xFFFF)),
    "counter_overflow": ((W, 0xFFFF), (OVERFLOW, 0, 0x10000, (W << 16) | 0xFFFF)),
    "drift_before_overflow": ((W + 60001, 0xFFFF), (DRIFT, 60001, 0, ((W + 60001) << 16) | 0xFFFF)),
    "wall_ahead": ((W - 1, 0xFFFF), (OK, 0, 0, W << 16)),
}


def canonical_of(case) -> int:
    (millis, counter), _ = CASES[case]
    c = (millis << 16) | counter
    assert tc.TOP < c                                        # every incoming lt is below it: R = c
    return c


def want_of(case):
    """(status, drift_ms, counter, canonical_lt) by the oracle's send, which the table of the cases restates."""
    c = canonical_of(case)
    st, out, drift, counter = send_scalar(c, W)
    want = (st, drift, counter, out if st == OK else c)
    assert want == CASES[case][1], (case, want)
    return want


def assert_send(res: dict, case, tag):
    got = (res["status"], res["drift_ms"], res["counter"], res["canonical_lt"])
    assert got == want_of(case), (tag, case, got)
    assert res["exc_index"] == gt.U64_MAX, (tag, case)


def single(case, local_rank=3):
    t = DeviceTable(0, local_rank=local_rank, capacity=N)
    o = OracleTable(N, local_rank, canonical_of(case))
    t.canonical = o.canonical
    return t, o


@pytest.mark.parametrize("case", list(CASES))
def test_put_stamped(gpu_device, case):
    t, o = single(case)
    key, val = np.array([5, 63, 0], np.uint32), np.array([1, 2, 3], np.uint32)
    want = o.put_stamped(key, val, W).as_dict()
    res = t.put_stamped(key, val, W)
    for f in gt.RESULT_FIELDS:
        assert res[f] == want[f], (case, f, res[f], want[f])
    assert_send(res, case, "put_stamped")
    seq.rows_equal(t, o.rows, N, case)
    assert t.canonical == o.canonical == want_of(case)[3]
    t.close()


@pytest.mark.parametrize("case", list(CASES))
def test_merge_of_one_record(gpu_device, case):
    t, o = single(case)
    cols = (np.array([9], np.uint32), np.array([tc.STAMPS[3]], np.int64), np.array([1], np.uint32),
            np.array([77], np.uint32), np.array([0, 1], np.uint64))
    want, _ = o.merge(*cols, W)
    res, _ = t.merge(*cols, W)
    for f in gt.RESULT_FIELDS:
        assert res[f] == want.as_dict()[f], (case, f, res[f])
    assert_send(res, case, "merge")
    assert res["n_stored"] == 1 and res["n_won"] == 1        # send follows the store, raising or not
    seq.rows_equal(t, o.rows, N, case)
    assert t.canonical == o.canonical == want_of(case)[3]
    t.close()


@pytest.mark.parametrize("case", list(CASES))
def test_merge_table(gpu_device, case):
    srows, drows = tc.gen_pair(N, seed=6100)
    src, osrc = gt.load(srows, N, local_rank=1, canonical=123)
    dst, odst = gt.load(drows, N, local_rank=tc.DST_RANK, canonical=canonical_of(case))
    res, oflags, _ = gt.check(dst, odst, src, osrc, N, 0, W, case, table=True)
    assert_send(res, case, "merge_table")
    assert res["n_stored"] == 1 and res["n_won"] == int(oflags.sum()) > 0
    assert dst.canonical == want_of(case)[3]
    src.close()
    dst.close()


@pytest.mark.parametrize("side", ["a", "b"])
@pytest.mark.parametrize("case", list(CASES))
def test_sync_tables(gpu_device, case, side):
    a_rows, b_rows = sc.pair(N, seed=6200)
    c = canonical_of(case)
    a, oa, b, ob = gs.load_pair(a_rows, b_rows, N, c_a=c if side == "a" else QUIET, c_b=c if side == "b" else QUIET)
    m, (res_a, ofl_a, res_b, ofl_b) = gs.check_sync(a, oa, b, ob, N, 0, 0, W, (case, side))
    status = want_of(case)[0]
    if side == "a":                                          # step 1's send: where it raises, the exchange ends
        assert_send(res_a, case, "sync_tables, step 1")
        assert m["fused"] == (status == OK)
        assert res_a["n_stored"] == 1 and res_a["n_won"] == int(ofl_a.sum()) > 0
        assert a.canonical == want_of(case)[3]
        assert res_b["n_stored"] == (1 if status == OK else 0)
    else:                                                    # step 2's send: raising after its store, still fused
        assert_send(res_b, case, "sync_tables, step 2")
        assert m["fused"] and res_a["status"] == OK
        assert res_b["n_stored"] == 1 and res_b["n_won"] == int(ofl_b.sum()) > 0
        assert b.canonical == want_of(case)[3]
    gs.close(a, b)
