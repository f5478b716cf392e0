"""
Depth of the stage-parallel KKT scans on the device (ParallelRiccati::solve; tests/test_scan_depth_emulation.py has the same horizons in the host emulation):
eight scenarios each at horizons on both sides of a change of the scan depth -- N = 5 and 34 on the 64 x 1 kernels (4 and 33 chunks: two and six levels),
66 and 100 on the 64 x 2 kernels (33 and 50 chunks) -- against the oracle through the public ABI, and one shifted primal-dual warm re-solve at N = 30,
the kind of launch the shrinking-horizon loop makes.  Bounds: those of tests/test_gpu_parity.py (_compare; the shifted re-solve:
test_shifted_primal_dual_warm_start_vs_oracle).
"""

import copy

import numpy as np
import pytest

import cases
from test_gpu_parity import OBJ_RTOL, Z_RTOL, _compare, _solver

pytestmark = pytest.mark.gpu


def _journey(N):
    "about 400 m per interval like tests/test_scan_depth_emulation.py; the whole track at N = 100"
    if N >= 100:
        return cases.track_00(), 1541.0
    crop = 400.0*N
    return cases.track_00(crop), crop/14.0 + 60.0


@pytest.mark.parametrize('N', [5, 34, 66, 100])
def test_scan_depths_vs_oracle(N):
    train = cases.train_default()
    track, T0 = _journey(N)
    T = T0*np.linspace(1.0, 1.14, 8)
    solver = _solver(train, track, N, start='profile')
    _compare(solver, cases.oracle_problem(train, track, N), T)


def test_shifted_warm_resolve_at_a_short_horizon_vs_oracle():
    from oracle import oracle
    from mseetc.track import computeDiscretizationPoints
    N, stp = 32, 5
    train = cases.train_default()
    track, T0 = _journey(N)
    T = T0*np.array([1.0, 1.05, 1.1])
    s1 = _solver(train, track, N, start='profile')
    s1.problem.keep_duals(True)
    r1 = s1.solveBatch(T, classifyFailures=False)
    assert np.all(r1['status'] == 0), r1['status']
    pos = computeDiscretizationPoints(track, N).index.values
    track2 = copy.deepcopy(track); track2.updateLimits(positionStart=float(pos[2]))
    s2 = _solver(train, track2, N - 2, start='profile').adoptDevice(s1)      # 30 intervals: 29 chunks, five levels
    t_now = r1['z'][:, stp*2 + 3]*1.003
    v_now = np.sqrt(np.abs(r1['z'][:, stp*2 + 4]))*0.997
    r2 = s2.solveBatch(T, initialTime=t_now, initialVelocity=v_now, shift=2, warmMu=1e-4, warmPush=1e-3, classifyFailures=False)
    assert np.all(r2['status'] == 0), r2['status']
    prob1, prob2 = cases.oracle_problem(train, track, N), cases.oracle_problem(train, track2, N - 2)
    for k in range(len(T)):
        first = oracle.solve_dual(prob1, prob1.scenario(float(T[k])), start='profile')
        sc = prob2.scenario(float(T[k]), float(t_now[k]), 1.0, float(v_now[k]))
        warm = oracle.solve_dual(prob2, sc, guess=first['z'][stp*2:], duals=first['duals'][2:], mu0=1e-4, push=1e-3)
        assert warm['stats']['STATUS'] == 0
        assert abs(r2['cost'][k] - warm['stats']['OBJ']) <= OBJ_RTOL*abs(warm['stats']['OBJ'])
        assert np.max(np.abs(r2['z'][k] - warm['z'])/np.maximum(1.0, np.abs(warm['z']))) <= 10*Z_RTOL
        assert abs(int(r2['iterations'][k]) - int(warm['stats']['ITERS'])) <= 2
    s2.close()
