"""The step catalogue of tests/_ctx_sequence.py without a GPU: every case builds, its oracle run completes,
and the catalogue's fixed rules hold (phases by capacity, refused calls, unique names)."""
import numpy as np

from tests import _ctx_sequence as seq


def test_catalogue_builds_and_oracle_runs():
    for step in seq.CATALOGUE:
        c = seq.case(step.case)
        rows, res, flags = seq.reference(step.case)
        assert len(rows) == c["n_ids"] and len(flags) == len(c["key"]), step.name
        assert c["n_ids"] <= seq.PEER_CAP, step.name
        for phase in step.phases:
            assert c["n_ids"] <= (seq.PHASE1_CAP if phase == 1 else seq.PHASE2_CAP), (step.name, phase)
        if step.expect == "invalid":
            assert step.bound == "broken", step.name
        if step.expect == "key_range":
            assert step.bad_key and step.device, step.name
    assert seq.PHASE1_CAP <= (1 << 20) < seq.PHASE2_CAP


def test_catalogue_covers_every_form_and_phase():
    names = {s.name for s in seq.CATALOGUE}
    assert len(names) == len(seq.CATALOGUE) >= 30
    one, two = {s.name for s in seq.steps_of(1)}, {s.name for s in seq.steps_of(2)}
    assert one | two == names
    assert "free_one_level" in one - two
    assert {"free_cold", "free_hot_buckets3", "flagged_cold"} <= two - one
    assert {s.expect for s in seq.CATALOGUE} == {"ok", "invalid", "key_range"}
    for s in seq.CATALOGUE:                                   # every switch a step sets has a default to go back to
        assert set(s.env) <= set(seq.ENV_DEFAULTS), s.name


def test_shared_references_are_read_only():
    rows, _, flags = seq.reference("fused0")
    assert not rows.flags.writeable and not flags.flags.writeable
    assert seq.reference("fused0")[0] is rows and seq.case("fused0") is seq.case("fused0")
    assert np.array_equal(seq.oracle_table(seq.CATALOGUE[0]).rows, rows)
