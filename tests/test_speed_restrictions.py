"""
Speed restrictions per scenario, host side (no device): the rule of include/mseetc_hip.h as casadiSolver.restrictedLimits states it in numpy, against
the host's own track code -- a track whose speed limits were lowered section by section packs, on the same grid, exactly the row of limits the rule gives --
the validation of the records and the clipping of the end speeds.  The device side: tests/test_speed_restrictions_gpu.py.
"""

import numpy as np
import pytest

import cases

from mseetc.ocp import casadiSolver

IO = dict(numSteps=1, numApproxSteps=1)
SECTIONS = (0.0, 25000.0, 35000.0)      # where the three speed limits of 00_var_speed_limit_100 begin [m]
LENGTH = 48531.0

# the sets of the GPU tests
S0 = []
S1 = [(25000, 35000, 80/3.6)]
S2 = [(10000, 12000, 60/3.6)]
S3 = [(10000, 20000, 90/3.6), (15000, 18000, 50/3.6)]
S4 = [(20000, 20300, 5.0)]
S5 = [(0, 3000, 40/3.6), (46000, 48531, 40/3.6)]
SETS = [S0, S1, S2, S3, S4, S5]


def _solver(N, track=None):
    return casadiSolver(cases.train_default(), track if track is not None else cases.track_00(), dict(numIntervals=N, maxIterations=500, integrationOptions=IO))


def _bmax(solver):
    return np.asarray(solver._desc._keep[3], dtype=float)


def _rule(solver, restrictions):
    "the rule of the header, written out node by node"
    pos, bmax, N = solver.points.index.values, _bmax(solver), solver.numIntervals
    row = bmax.copy()
    hit = lambda i, b, e: pos[i] < e and pos[i + 1] > b
    for b, e, v in restrictions:
        for i in range(1, N):
            if hit(i - 1, b, e) or hit(i, b, e):
                row[i] = min(row[i], v*v)
    return row


@pytest.mark.parametrize('N', [63, 64, 100, 130])
def test_restricted_limits_are_the_limits_of_the_edited_track(N):
    solver = _solver(N)
    ends = SECTIONS[1:] + (LENGTH,)
    for k in range(3):
        for factor in (0.8, 0.5):
            track = cases.track_00()
            col = track.speedLimits.columns[0]
            assert list(track.speedLimits.index) == list(SECTIONS)
            v = factor*float(track.speedLimits[col].values[k])
            track.speedLimits.iloc[k, 0] = v
            edited = _solver(N, track)
            assert np.array_equal(edited.points.index.values, solver.points.index.values)      # same grid: the sections' breakpoints are nodes already
            row = solver.restrictedLimits([(SECTIONS[k], ends[k], v)], 1)
            assert row.shape == (1, N + 1)
            assert np.array_equal(row[0], _bmax(edited))
            assert not np.array_equal(row[0], _bmax(solver))
    # a "restriction" above the section's limit changes nothing
    assert np.array_equal(solver.restrictedLimits([(0, 25000, 200/3.6)], 1)[0], _bmax(solver))


@pytest.mark.parametrize('N', [63, 100])
def test_restricted_limits_follow_the_rule(N):
    solver = _solver(N)
    pos = solver.points.index.values
    rows = solver.restrictedLimits(SETS, len(SETS))
    assert rows.shape == (len(SETS), N + 1)
    for k, one in enumerate(SETS):
        assert np.array_equal(rows[k], _rule(solver, one)), k
        assert rows[k, 0] == _bmax(solver)[0] and rows[k, N] == _bmax(solver)[N]
    assert np.array_equal(rows[0], _bmax(solver))
    # S3: the overlap takes the minimum
    inner = (pos[1:-1] > 15000) & (pos[1:-1] < 18000)
    assert inner.any() and np.all(rows[3, 1:-1][inner] == (50/3.6)*(50/3.6))
    outer = (pos[1:-1] > 10000) & (pos[1:-1] < 14000)
    assert outer.any() and np.all(rows[3, 1:-1][outer] == (90/3.6)*(90/3.6))
    # end points exactly on nodes: intervals 10 and 11 are restricted, so nodes 10 ... 12 and no others
    on_nodes = [(pos[10], pos[12], 10.0)]
    row = solver.restrictedLimits(on_nodes, 1)[0]
    changed = np.flatnonzero(row != _bmax(solver))
    assert changed.tolist() == [10, 11, 12] and np.all(row[changed] == 100.0)
    # a single sequence is repeated for the batch
    assert np.array_equal(solver.restrictedLimits(S3, 4), np.repeat(rows[3:4], 4, axis=0))


def test_validation():
    solver = _solver(63)
    bad = dict(not_finite=[(10000, np.inf, 20.0)], nan_velocity=[(10000, 12000, np.nan)], end_before_begin=[(12000, 10000, 20.0)], empty=[(10000, 10000, 20.0)],
               no_interval_behind=[(LENGTH, LENGTH + 100, 20.0)], no_interval_in_front=[(-50.0, 0.0, 20.0)], minimum_velocity=[(10000, 12000, 1.0)],
               below_minimum=[(10000, 12000, 0.5)], negative_velocity=[(10000, 12000, -20.0)], too_many=[(100.0*k, 100.0*k + 50, 20.0) for k in range(17)],
               not_a_triple=[[(10000, 12000)]])
    for name, one in bad.items():
        with pytest.raises(ValueError):
            solver.restrictedLimits(one, 1)
        with pytest.raises(ValueError):
            solver.solveBatch(2300, speedRestrictions=one)      # (raised in front of any device call)
    # sixteen are allowed
    solver.restrictedLimits([(100.0*k, 100.0*k + 50, 20.0) for k in range(16)], 1)
    # a wrong batch length
    with pytest.raises(ValueError):
        solver.restrictedLimits(SETS, 4)
    with pytest.raises(ValueError):
        solver.solveBatch([2300.0]*4, speedRestrictions=SETS)


def test_entry_points_refuse_a_null_handle():
    "the library exports both entry points; without a handle they are invalid calls with a message (no device is touched)"
    import ctypes
    import __graft_entry__ as g
    L = ctypes.CDLL(str(g.build()))
    L.msd_last_error.restype = ctypes.c_char_p
    assert L.msd_problem_speed_restrictions(None, 0, 1, None, None) == -1 and b'handle' in L.msd_last_error()
    assert L.msd_problem_limit_rows(None, None) == -1


def test_end_speeds_are_clipped_to_the_restricted_limits():
    solver = _solver(63)
    scen = solver._scenarios(2300, 0, 20, 20, solver._restrictions(S5))
    assert scen.shape == (1, 4) and scen[0, 2] == (40/3.6)**2 and scen[0, 3] == (40/3.6)**2
    scen = solver._scenarios(2300, 0, 20, 20)
    assert scen[0, 2] == 20.0**2 and scen[0, 3] == 20.0**2
    # per scenario: only the restricted ones are clipped, and only at the restricted end
    scen = solver._scenarios(2300, 0, 20, 20, solver._restrictions([S0, S2, S5, [(46000, 48531, 30/3.6)]]))
    assert scen[:, 2].tolist() == [400.0, 400.0, (40/3.6)**2, 400.0]
    assert scen[:, 3].tolist() == [400.0, 400.0, (40/3.6)**2, (30/3.6)**2]
    # the minimum velocity still bounds from below
    assert solver._scenarios(2300, 0, 0.1, 0.1, solver._restrictions(S5))[0, 2:].tolist() == [1.0, 1.0]
