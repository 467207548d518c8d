"""The parity recorder of tests/test_gpu_configs.py from a module that merely imports it: _close records
a mismatch into a module list, and an autouse fixture reports the list only for tests of the module that
defines the fixture. The reporting scope (_reporting, entered by _run_and_compare itself) must raise on
its own, whoever calls it, and must hand nothing on to a fixture that would report it a second time."""

import pytest

import test_gpu_configs as G


def test_scope_raises_for_a_recorded_mismatch():
    before = list(G._FAILS)
    with pytest.raises(AssertionError, match=r"\bx\b") as ei:
        with G._reporting():
            G._close(1.0, 2.0, 1e-12, 0.0, "x")
    assert "1.000e+00" in str(ei.value)  # max|diff| of the recorded line
    assert G._FAILS == before            # taken off the list: no second report at a fixture's teardown


def test_clean_scope_exits_silently():
    with G._reporting():
        G._close(1.0, 1.0 + 1e-13, 1e-12, 0.0, "y")
        G._close([0.0, 3.0], [1e-13, 3.0], 0.0, 1e-12, "z")
    assert not G._FAILS


def test_scope_reports_mismatches_when_its_body_raises():
    """The hard asserts inside a scan (Σ_b N_b, isfinite) or a device error end the body early: what was
    recorded up to there is listed with the error, not dropped."""
    with pytest.raises(AssertionError, match=r"(?s)boom.*\bw\b") as ei:
        with G._reporting():
            G._close(1.0, 2.0, 1e-12, 0.0, "w")
            raise RuntimeError("boom")
    assert isinstance(ei.value.__cause__, RuntimeError)
    assert not G._FAILS
    with pytest.raises(RuntimeError, match="boom"):   # nothing recorded: the body's own error, unchanged
        with G._reporting():
            raise RuntimeError("boom")


def test_scope_leaves_earlier_entries_to_their_owner():
    """Entries recorded outside the scope (test_gpu_shards.py appends its own) stay for the fixture."""
    G._FAILS.append("outer")
    try:
        with pytest.raises(AssertionError) as ei:
            with G._reporting():
                G._close(1.0, 2.0, 0.0, 0.0, "inner")
        assert "inner" in str(ei.value) and "outer" not in str(ei.value)
        assert G._FAILS == ["outer"]
    finally:
        G._FAILS.clear()


def test_cond_bound_follows_from_the_eigenvalue_bars():
    """cond_rel_bound covers the worst case the eig_max (1e-10 relative) and eig_min (1e-12 eig_max
    absolute) bars allow, wherever it is applied (below 0.5)."""
    for cond in (1.0, 50.0, 1e5, 1e8, 1e10, 2e11):
        rel = G.cond_rel_bound(cond)
        assert rel < 0.5
        lmax, lmin = 1.0, 1.0 / cond
        worst = max((lmax * (1 + 1e-10)) / (lmin - 1e-12 * lmax) / cond - 1,
                    1 - (lmax * (1 - 1e-10)) / (lmin + 1e-12 * lmax) / cond)
        assert worst <= rel, (cond, worst, rel)
    assert G.cond_rel_bound(1e12) > 0.5
