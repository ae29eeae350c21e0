"""gpmpc_tube_plan (no device): the shapes the GPU tests of the tube kernels use lie on both
sides of the linear kernel's pass boundary and at and below the Monte-Carlo kernel's cap."""
import pytest

import tube_cases as tc
from gp_mpc_rocket_landing_amd import _lib


def test_the_plan_reports_the_kernels_constants():
    assert _lib.tube_plan() == (tc.K_TILE, tc.MC_CAP)
    assert _lib.tube_plan(15, 100) == (tc.K_TILE, tc.MC_CAP)
    with pytest.raises(_lib.HIPError) as e:
        _lib.tube_plan(-1, 0)
    assert e.value.rc == -2
    with pytest.raises(_lib.HIPError):
        _lib.tube_plan(0, -1)


def test_the_horizons_cross_a_pass_boundary():
    k_tile, _ = _lib.tube_plan(max(tc.HORIZONS), 0)
    passes = {N: -(-N // k_tile) for N in tc.HORIZONS}
    assert set(passes.values()) == {1, 2}
    assert passes[k_tile - 1] == passes[k_tile] == 1 and passes[k_tile + 1] == 2
    assert k_tile - 1 in tc.HORIZONS and k_tile in tc.HORIZONS and k_tile + 1 in tc.HORIZONS
    assert 1 in tc.HORIZONS and 2 in tc.HORIZONS      # A is never read; the first horizon that reads it
    # 18 plant steps per horizon step: a pass fills the 256 lanes of a workgroup but for four
    assert 18 * k_tile <= 256 < 18 * (k_tile + 1)


def test_the_particle_counts_lie_at_and_below_the_cap():
    _, cap = _lib.tube_plan(0, 0)
    counts = [n for n, _ in tc.MC_CASES] + list(tc.MC_LARGE)
    assert max(counts) == cap and all(1 <= n <= cap for n in counts)
    # one lane per particle in workgroups of 128, 256 and 1024 lanes: a count in each, and the edges of a wave
    assert any(n <= 128 for n in counts) and any(128 < n <= 256 for n in counts) and any(256 < n for n in counts)
    assert {1, 2, 63, 64, 65} <= set(counts)
