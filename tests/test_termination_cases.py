"""The termination table (termination_cases.py) against two independent CPU statements of
the rule, before any device sees it: the oracle's (mc_oracle.pre_step_outcome, and
sixdof_oracle.pre_step_outcome for the 14-state rows) and the package's own host loop
(experiments/monte_carlo.py: MonteCarloSimulator.run_single with LandingConstraints under
the run_experiments tolerances).  The table's codes are literals; neither side computes them."""
import numpy as np
import pytest

import termination_cases as tc


def test_table_shape_and_coverage():
    """About 60 rows, every outcome of the ladder at step 0 present, live rows among
    them, boundary values really one ulp off their thresholds."""
    assert 55 <= len(tc.CASES) <= 80, len(tc.CASES)
    assert len({c.name for c in tc.CASES}) == len(tc.CASES)
    assert set(tc.codes().tolist()) == {0, 1, 2, 3, 4, 6}
    assert sum(c.code == 0 for c in tc.CASES) >= 6
    assert tc.FUEL_EDGE == 1.0 + 0.01 and tc.UP(tc.FUEL_EDGE) > tc.FUEL_EDGE
    assert tc.BELOW_ZERO < 0.0 and tc.BELOW_ZERO / 2 == 0.0
    assert tc.UP(1e6) > 1e6 and tc.DOWN(5.0) < 5.0 and tc.DOWN(1.0) < 1.0
    assert np.signbit(tc.CASES[0].x7[1]) and tc.CASES[0].x7[1] == 0.0   # -0.0 survives the table
    assert all(c.code7 == c.code for c in tc.SEVEN_STATE)
    assert tc.states14().shape == (len(tc.CASES), 14) and tc.states7(tc.SEVEN_STATE).shape[1] == 7


@pytest.mark.parametrize("case", tc.CASES, ids=[c.name for c in tc.CASES])
def test_oracle_agrees_with_the_table(case):
    from oracle import mc_oracle, sixdof_oracle
    x14 = tc.states14([case])[0]
    with np.errstate(invalid="ignore"):
        assert mc_oracle.pre_step_outcome(x14[:7], x14[0]) == case.code7
        assert sixdof_oracle.pre_step_outcome(x14, x14[0]) == case.code


def test_oracle_rollout_step_records_the_table_outcome():
    """rollout_step itself (not only its ladder) on every terminated row: outcome, fuel,
    the final state in the record, nothing else touched; TIMEOUT before everything."""
    from oracle import sixdof_oracle as so
    for case in tc.CASES:
        x = tc.states14([case])[0]
        S = so.new_rollout(x, 5)
        with np.errstate(invalid="ignore"):   # inf - inf and NaN rows
            if case.code:
                T, info = so.rollout_step(None, None, S)
                assert info is None and T["rec"][0] == case.code, case.name
                np.testing.assert_array_equal(T["rec"][4:11], x[:7])
                np.testing.assert_array_equal(T["rec"][2], x[0] - x[0])
                assert T["rec"][1] == 0 and T["rec"][3] == 0 and T["rec"][11] == 0
            T, info = so.rollout_step(None, None, S, max_steps=0)
            assert info is None and T["rec"][0] == 5, case.name


class _StepRan(Exception):
    pass


class _Plant:
    n_x, n_u = 7, 3

    def step(self, x, u, dt):
        raise _StepRan


class _Controller:
    def step(self, x):
        import types
        return types.SimpleNamespace(u0=np.zeros(3))


@pytest.mark.parametrize("case", tc.CASES, ids=[c.name for c in tc.CASES])
def test_package_host_loop_agrees_with_the_table(case):
    """run_single from the row as x0: a row that continues reaches dynamics.step; every
    other row ends with the table's outcome before the controller runs.  The host loop
    flies seven states, so a 14-state row goes in as its first seven (code7)."""
    from gp_mpc_rocket_landing_amd.experiments.monte_carlo import (LandingOutcome, MonteCarloSimulator,
                                                                   SimulationConfig)
    cfg = SimulationConfig.run_experiments()
    sim = MonteCarloSimulator(_Plant(), _Controller(), cfg)
    x0 = np.array(case.x7)
    with np.errstate(invalid="ignore"):
        try:
            res = sim.run_single(0, x0=x0)
        except _StepRan:
            assert case.code7 == 0
            return
    assert res.outcome == LandingOutcome(case.code7) and len(res.controls) == 0
    if case.code7 in (1, 4):   # the verdict is LandingConstraints.check_landing's
        with np.errstate(invalid="ignore"):
            ok, _ = cfg.landing_constraints.check_landing(x0, x0[0])
        assert ok == (case.code7 == 1)
