"""The model of crdt_tombstone_live / crdt_export_live (tests/_live_cases.py) against the object-level oracle's
MapCrdt.clear(wall), the restatement of crdt.dart:67-73, on small maps; and the generator's self-checks at
every shape the GPU tests use.  No GPU, no library."""
import numpy as np
import pytest

from oracle import crdt_oracle as O
from oracle.oracle_c import OracleTable, send_scalar
from tests import _live_cases as lc
from tests._cases import NULL, WALL

NODES = ["a", "b", "c"]                   # ranks are their positions (already in compareTo order)
LOCAL = "b"


def mirror(m: O.MapCrdt):
    """An OracleTable holding m's records, key ids in insertion order; (table, key names, value list)."""
    names = list(m._map)
    values: list = []
    o = OracleTable(len(names) + 3, NODES.index(m.node_id), m.canonical_time.logical_time)
    for i, k in enumerate(names):
        r = m._map[k]
        val = NULL
        if r.value is not None:
            values.append(r.value)
            val = len(values) - 1
        o.put_rows([i], [r.hlc.logical_time], [NODES.index(r.hlc.node_id)], [val], [r.modified.logical_time])
    return o, names, values


def run_both(m: O.MapCrdt, wall: int):
    """clear(wall) on the oracle map and the model on its mirror; compares everything; returns the status."""
    o, names, values = mirror(m)
    n = len(names)
    before = m.canonical_time.logical_time
    want_live = lc.model_live(o.rows, n)
    assert [names[i] for i in want_live["key"]] == list(m.map.keys())
    assert [values[v] for v in want_live["val"]] == list(m.map.values())
    m.events.clear()
    exc = None
    try:
        m.clear(wall)
    except (O.ClockDriftException, O.OverflowException) as e:
        exc = e
    res, flags = lc.model_tombstone(o, n, wall)
    if isinstance(exc, O.ClockDriftException):
        assert (res["status"], res["drift_ms"]) == (1, exc.drift) and res["drift_ms"] == send_scalar(before, wall)[2]
    elif isinstance(exc, O.OverflowException):
        assert (res["status"], res["counter"]) == (3, exc.counter) and res["counter"] == send_scalar(before, wall)[3]
    else:
        assert res["status"] == 0
    if exc is not None:
        assert not flags.any() and res["n_won"] == 0 and o.canonical == before
    assert o.canonical == m.canonical_time.logical_time == res["canonical_lt"]
    assert [(names[i], None) for i in np.flatnonzero(flags)] == m.events       # the watch() events, in id order
    assert res["n_won"] == int(flags.sum())
    for i, k in enumerate(names):
        r, row = m._map[k], o.rows[i]
        assert (int(row["lt"]), NODES[row["rank"]], int(row["mod"])) == \
            (r.hlc.logical_time, r.hlc.node_id, r.modified.logical_time), k
        assert (None if row["val"] == NULL else values[row["val"]]) == r.value, k
    assert np.all(o.rows["mod"][n:] < 0)                                       # nothing past the map was written
    return res["status"]


def mixed_map(wall=WALL) -> O.MapCrdt:
    m = O.MapCrdt(LOCAL)
    m.put_all({"k0": 0, "k1": 1, "k2": 2}, wall)
    m.put("k3", 3, wall + 5)
    m.delete("k1", wall + 6)
    m.merge({"k4": O.Record(O.Hlc(wall + 7, 2, "c"), "remote", O.Hlc(0, 0, "x")),
             "k5": O.Record(O.Hlc(wall + 7, 3, "a"), None, O.Hlc(0, 0, "x"))}, wall + 8)
    m.put_record("k6", O.Record(O.Hlc(wall, 0, "a"), "hidden", O.Hlc.from_logical_time(-7, LOCAL)))  # invisible
    m.put_record("k7", O.Record(O.Hlc(wall, 1, "c"), "zero", O.Hlc.from_logical_time(0, LOCAL)))     # mod == 0
    return m


def test_mixed_map():
    m = mixed_map()
    assert run_both(m, WALL + 20) == 0
    assert m.length == 0 and m.get_record("k6").value == "hidden" and len(m.events) == 5
    assert run_both(m, WALL + 30) == 0 and not m.events       # a second clear finds nothing live


def test_empty_map_and_only_tombstones_leave_the_canonical():
    m = O.MapCrdt(LOCAL)
    assert run_both(m, WALL) == 0 and m.canonical_time.logical_time == 0
    m.put_all({"x": 1, "y": 2}, WALL)
    m.put_all({"x": None, "y": None}, WALL + 1)
    c = m.canonical_time.logical_time
    assert run_both(m, WALL + 2) == 0 and m.canonical_time.logical_time == c
    assert run_both(m, WALL - 70000) == 0 and m.canonical_time.logical_time == c   # no send: no drift either


def test_drift_raise_changes_nothing():
    m = mixed_map()
    assert run_both(m, WALL - 60001) == 1


def test_overflow_raise_changes_nothing():
    m = mixed_map()
    m._canonical_time = O.Hlc(WALL + 100, 0xFFFF, LOCAL)
    assert run_both(m, WALL + 100) == 3
    assert run_both(m, WALL + 50) == 3
    assert run_both(m, WALL + 101) == 0


@pytest.mark.parametrize("n_rows", lc.SHAPES + (lc.T + 9, 2 * lc.T + 5, 2 * lc.T + 9, 3 * lc.T + 17, lc.LARGE))
def test_generator_self_checks(n_rows):
    rows = lc.gen_live(n_rows, 500 + n_rows)
    dead = lc.gen_dead(n_rows, 600 + n_rows)
    from tests import _table_cases as tc
    assert not lc.live_mask(tc.dense(dead, n_rows + 1), n_rows).any()
    if n_rows >= lc.PLANT_FROM:
        d = tc.dense(rows, n_rows + 1)
        live = lc.live_mask(d, n_rows + 1)
        assert live[0] and live[n_rows - 1] and live[n_rows]
        assert send_scalar(lc.C0, lc.DRIFT_WALL)[0] == 1 and send_scalar(lc.C0, lc.WALL)[0] == 0
