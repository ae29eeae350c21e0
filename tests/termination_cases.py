"""The termination ladder at step 0, as a hand-written table shared by the host test
(test_termination_cases.py) and the device tests (test_gpu_rollouts6_termination.py,
test_gpu_fleet_parity.py).

The rules are the checks at the top of every step of MonteCarloSimulator.run_single
(monte_carlo.py:458-488) with the run_experiments tolerances (pos_tol_xy 5, pos_tol_z 1,
vel_tol_xy 1, vel_tol_z 3, min_fuel_margin 0.05), in this order:

    alt < 0                      -> CRASH (2)
    m <= 1.0 + 0.01              -> FUEL_EXHAUSTED (3)
    any |x| > 1e6 or NaN         -> DIVERGENCE (6)       (first seven states)
    alt < 1 and |vx| < 5         -> SUCCESS (1) if check_landing else CONSTRAINT_VIOLATION (4)
    (6-DoF only) any of the 14 states > 1e6 or NaN -> DIVERGENCE (6)
    otherwise the step runs      -> 0

Every row is a first-seven-state vector [m, alt, y, z, vx, vy, vz] at step 0, where the
initial mass m0 is the row's own m, and the outcome code written as a literal: nothing here
is computed from a rule.  A row changes one or two slots of a benign state (mass 2, all else
0, altitude 0.5 where the row is about the landing check and 10 otherwise); boundary values
are one ulp off the threshold (np.nextafter), so each comparison is met from both sides.
The 14-state rows carry q and omega too; every other row flies with the unit quaternion
and zero rates.  ``code7`` is what the seven-state ladder alone gives the row (it differs
from ``code`` only where q / omega diverge away from the ground).
"""
from collections import namedtuple

import numpy as np

Case = namedtuple("Case", "name x7 code qw code7")

NAN, INF = float("nan"), float("inf")


def UP(v):
    """The next double above v > 0."""
    return float(np.nextafter(v, INF))


def DOWN(v):
    """The next double below v > 0."""
    return float(np.nextafter(v, 0.0))


BELOW_ZERO = float(np.nextafter(0.0, -1.0))         # the smallest negative subnormal
FUEL_EDGE = 1.0 + 0.01                              # as the rule writes it (not the literal 1.01)
SLOTS = ("m", "alt", "y", "z", "vx", "vy", "vz")
UNIT_QW = (1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0)

CASES = []


def _add(name, code, alt, qw=None, code7=None, **slots):
    x = dict(m=2.0, alt=alt, y=0.0, z=0.0, vx=0.0, vy=0.0, vz=0.0)
    x.update(slots)
    CASES.append(Case(name, tuple(float(x[s]) for s in SLOTS), code, qw, code if code7 is None else code7))


# ---- the threshold edges of the ladder
_add("alt -0.0 is not below zero: landing check", 1, -0.0)
_add("alt one ulp below zero", 2, BELOW_ZERO)
_add("m at the fuel edge 1.0 + 0.01", 3, 10.0, m=FUEL_EDGE)
_add("m one ulp above the fuel edge", 0, 10.0, m=UP(FUEL_EDGE))
_add("alt 1.0: no landing check", 0, 1.0)
_add("alt one ulp below 1.0", 1, DOWN(1.0))
_add("vx -5.0 at alt 0.5: no landing check", 0, 0.5, vx=-5.0)
_add("vx +5.0 at alt 0.5: no landing check", 0, 0.5, vx=5.0)
_add("vx one ulp inside -5.0 at alt 0.5: vertical velocity above 3", 4, 0.5, vx=-DOWN(5.0))
_add("vx one ulp inside +5.0 at alt 0.5: vertical velocity above 3", 4, 0.5, vx=DOWN(5.0))

# ---- |value| = 1e6 is not a divergence.  Near the ground the landing verdict shows it
# (a divergence would come first); alt and vx cannot reach that check, so their rows continue
_add("m 1e6 at alt 0.5", 1, 0.5, m=1e6)
_add("y -1e6 at alt 0.5", 4, 0.5, y=-1e6)
_add("z 1e6 at alt 0.5", 4, 0.5, z=1e6)
_add("vy 1e6 at alt 0.5", 4, 0.5, vy=1e6)
_add("vz -1e6 at alt 0.5", 4, 0.5, vz=-1e6)
_add("alt 1e6", 0, 1e6)
_add("vx -1e6 at alt 10", 0, 10.0, vx=-1e6)

# ---- one ulp above 1e6, inf and NaN in each slot: DIVERGENCE (NaN in alt is no CRASH,
# NaN in m no FUEL_EXHAUSTED: every comparison with a NaN is false)
_add("m one ulp above 1e6", 6, 10.0, m=UP(1e6))
_add("m inf", 6, 10.0, m=INF)
_add("m NaN", 6, 10.0, m=NAN)
_add("alt one ulp above 1e6", 6, UP(1e6))
_add("alt inf", 6, INF)
_add("alt NaN", 6, NAN)
_add("y one ulp below -1e6", 6, 10.0, y=-UP(1e6))
_add("y inf", 6, 10.0, y=INF)
_add("y NaN", 6, 10.0, y=NAN)
_add("z one ulp above 1e6", 6, 10.0, z=UP(1e6))
_add("z -inf", 6, 10.0, z=-INF)
_add("z NaN", 6, 10.0, z=NAN)
_add("vx one ulp below -1e6", 6, 10.0, vx=-UP(1e6))
_add("vx inf", 6, 10.0, vx=INF)
_add("vx NaN", 6, 10.0, vx=NAN)
_add("vy one ulp above 1e6", 6, 10.0, vy=UP(1e6))
_add("vy -inf", 6, 10.0, vy=-INF)
_add("vy NaN", 6, 10.0, vy=NAN)
_add("vz one ulp below -1e6", 6, 10.0, vz=-UP(1e6))
_add("vz inf", 6, 10.0, vz=INF)
_add("vz NaN", 6, 10.0, vz=NAN)

# ---- the landing tolerances at alt 0.5: at the tolerance, and one ulp beyond, both signs
_add("y +5", 1, 0.5, y=5.0)
_add("y -5", 1, 0.5, y=-5.0)
_add("y one ulp above +5", 4, 0.5, y=UP(5.0))
_add("y one ulp below -5", 4, 0.5, y=-UP(5.0))
_add("z +5", 1, 0.5, z=5.0)
_add("z -5", 1, 0.5, z=-5.0)
_add("z one ulp above +5", 4, 0.5, z=UP(5.0))
_add("z one ulp below -5", 4, 0.5, z=-UP(5.0))
_add("vx +3", 1, 0.5, vx=3.0)
_add("vx -3", 1, 0.5, vx=-3.0)
_add("vx one ulp above +3", 4, 0.5, vx=UP(3.0))
_add("vx one ulp below -3", 4, 0.5, vx=-UP(3.0))
_add("vy +1", 1, 0.5, vy=1.0)
_add("vy -1", 1, 0.5, vy=-1.0)
_add("vy one ulp above +1", 4, 0.5, vy=UP(1.0))
_add("vy one ulp below -1", 4, 0.5, vy=-UP(1.0))
_add("vz +1", 1, 0.5, vz=1.0)
_add("vz -1", 1, 0.5, vz=-1.0)
_add("vz one ulp above +1", 4, 0.5, vz=UP(1.0))
_add("vz one ulp below -1", 4, 0.5, vz=-UP(1.0))

# ---- the order of the ladder
_add("crash and low mass: CRASH first", 2, -1.0, m=1.0)
_add("crash and y 1e7: CRASH first", 2, -1.0, y=1e7)
_add("low mass and y 1e7: FUEL_EXHAUSTED first", 3, 10.0, m=1.0, y=1e7)
_add("y 1e7 at alt 0.5: DIVERGENCE, no landing verdict", 6, 0.5, y=1e7)

# ---- the 14-state extension: q / omega diverge after the landing check
_add("q1 NaN at alt 10", 6, 10.0, qw=(1.0, NAN, 0.0, 0.0, 0.0, 0.0, 0.0), code7=0)
_add("q3 1e7 at alt 10", 6, 10.0, qw=(1.0, 0.0, 0.0, 1e7, 0.0, 0.0, 0.0), code7=0)
_add("w0 NaN at alt 10", 6, 10.0, qw=(1.0, 0.0, 0.0, 0.0, NAN, 0.0, 0.0), code7=0)
_add("w2 -1e7 at alt 10", 6, 10.0, qw=(1.0, 0.0, 0.0, 0.0, 0.0, 0.0, -1e7), code7=0)
_add("w1 one ulp above 1e6 at alt 10", 6, 10.0, qw=(1.0, 0.0, 0.0, 0.0, 0.0, UP(1e6), 0.0), code7=0)
_add("q0 NaN at alt 0.5: the landing verdict wins", 1, 0.5, qw=(NAN, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0))
_add("q2 1e7 at alt 0.5, vy 2: the landing verdict wins", 4, 0.5, vy=2.0, qw=(1.0, 0.0, 1e7, 0.0, 0.0, 0.0, 0.0))
_add("w1 NaN at alt 0.5, vx -4: the landing verdict wins", 4, 0.5, vx=-4.0,
     qw=(1.0, 0.0, 0.0, 0.0, 0.0, NAN, 0.0))
_add("w2 1e7 at alt 0.5: the landing verdict wins", 1, 0.5, qw=(1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1e7))

# ---- ordinary flight states: the step runs
_add("descending at 31 m", 0, 31.2, m=2.05, y=1.9, z=-4.5, vx=-3.2, vy=0.1, vz=-0.3)
_add("descending at 12 m", 0, 12.0, m=1.9, y=-2.0, z=1.0, vx=-2.0, vy=0.3, vz=0.2)
_add("descending at 4 m", 0, 4.0, m=1.6, y=0.5, z=-0.5, vx=-1.5, vy=0.0, vz=0.1)


def states7(cases=None):
    """(n, 7) array of the rows' first seven states."""
    return np.array([c.x7 for c in (CASES if cases is None else cases)], float)


def states14(cases=None):
    """(n, 14) array: the first seven states, then the row's q / omega or the unit
    quaternion and zero rates."""
    return np.array([c.x7 + (c.qw or UNIT_QW) for c in (CASES if cases is None else cases)], float)


def codes(cases=None):
    return np.array([c.code for c in (CASES if cases is None else cases)], int)


SEVEN_STATE = [c for c in CASES if c.qw is None]   # the 3-DoF fleet's rows
