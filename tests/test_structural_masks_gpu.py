"""
The FAST first-pass kernels on the device after round 8: the lane predicates of the fused passes come from the compiled-in structure (msd_kernel.hpp:
Solver::on), a scenario whose data fix a variable the structure has free is handed over with reason 0, and the early results live in twin kernels that
only a begun batch or an iteration budget launches.  Needs an MI355X: run with -m gpu.

Tolerances: those of tests/test_gpu_parity.py (_compare) -- objective 1e-8 relative, every variable 1e-6 relative to max(1, |z|), iterations within 2.
"""
import numpy as np
import pytest

import cases

pytestmark = pytest.mark.gpu

OBJ_RTOL = 1e-8
Z_RTOL = 1e-6
B = 64
RK11 = dict(numSteps=1, numApproxSteps=1)


def _solver(train, track, N):
    from mseetc.ocp import casadiSolver
    return casadiSolver(train, track, dict(numIntervals=N, maxIterations=500, integrationOptions=RK11), startingPoint='profile')


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _records(stats):
    "stats records without their time stamps"
    from mseetc._device import ST
    out = stats.copy()
    out[:, ST['CYC_TOTAL']] = out[:, ST['CYC_KKT']] = 0
    return out


# (train, crop of track 00, N, shortest and longest running time of the 64 scenarios, geometry).  The ranges were screened with the oracle: every scenario
# converges without a second-order correction -- a first pass without SOCK hands such a scenario over, which is not what these tests are about (the test
# asserts the screening).  N = 100 is the flagship shape and takes the first 64 scenarios of the benchmark's own batch (bench.py, workloads.c1_times); on an
# evenly spaced batch from 1541 s to 1926 s one scenario ends two iterations from the oracle at 1.293e-06 on the variables -- the flat directions that
# tests/test_gpu_parity.py gives 1e-5 on its 256-scenario samples; the kernels compute there what the parent commit computes
SHAPES = [('both', 3000, 5, (190.0, 235.0), (64, 2)), ('both', 13000, 33, (760.0, 900.0), (64, 2)), ('both', None, 100, 'c1', (64, 2)),
          ('both', 8000, 17, (440.0, 500.0), (64, 1)), ('both', None, 200, (1541.0, 1926.0), (128, 2)), ('fig10', 12000, 30, (520.0, 650.0), (64, 1))]


@pytest.mark.parametrize('variant,crop,N,T,geometry', SHAPES)
def test_parity_with_the_oracle(variant, crop, N, T, geometry):
    from mseetc._device import ST, lib
    from oracle import oracle
    train = cases.train_default() if variant == 'both' else cases.train_fig10()
    track = cases.track_00(crop)
    # (64 x 2 below 64 nodes: the ladder alone gives those horizons 64 x 1)
    forced = geometry == (64, 2) and N + 1 <= 64
    if forced:
        assert lib().msd_tuning(b'geometry', 16*64 + 2) == 0
    try:
        s = _solver(train, track, N)
        s.problem      # (the handle, and with it the plan, is made on first use)
    finally:
        if forced:
            assert lib().msd_tuning(b'geometry', 0) == 0
    assert s.problem.geometry() == geometry
    scen = s._scenarios(cases.c1_times(B, seed=20260612) if T == 'c1' else np.linspace(T[0], T[1], B), 0, 1, 1)
    total0, why0 = s.problem.follow_counts()
    res = s.problem.solve_batch(scen)
    total1, why1 = s.problem.follow_counts()
    name = s.problem.last_first_pass()
    s.close()
    assert total1 == total0 and why1 == why0      # nothing handed over
    assert 'solve_kernel' in name
    prob = cases.oracle_problem(train, track, N)
    zr, sr, nfail = oracle.solve_batch(prob, scen, start='profile')
    st = res['stats']
    dz = np.max(np.abs(res['z'] - zr)/np.maximum(1.0, np.abs(zr)), axis=1)
    dobj = np.abs(st[:, ST['OBJ']] - sr[:, ST['OBJ']])/np.abs(sr[:, ST['OBJ']])
    dit = np.abs(st[:, ST['ITERS']] - sr[:, ST['ITERS']])
    print('N %d %s: objective %.3e, variables %.3e, iterations differ by at most %d' % (N, variant, dobj.max(), dz.max(), dit.max()))
    assert nfail == 0 and np.all(sr[:, ST['STATUS']] == 0) and not np.any(sr[:, ST['N_SOC']])
    assert np.all(st[:, ST['STATUS']] == 0), st[:, ST['STATUS']]
    assert np.all(dobj <= OBJ_RTOL) and np.all(dz <= Z_RTOL) and np.all(dit <= 2)


def test_a_scenario_without_running_time_is_handed_over_with_reason_0():
    from mseetc._device import ST
    N = 33
    s = _solver(cases.train_default(), cases.track_00(13000), N)
    scen = s._scenarios(np.linspace(760.0, 900.0, B), 0, 1, 1)      # (the N = 33 batch of SHAPES)
    plain = s.problem.solve_batch(scen)
    plain = dict(z=plain['z'].copy(), stats=_records(plain['stats']))
    assert np.all(plain['stats'][:, ST['STATUS']] == 0)
    guard = scen.copy()
    guard[7, 0] = guard[7, 1]      # t0 == tEnd: every t is fixed by the data, the structure has them free
    total0, why0 = s.problem.follow_counts()
    res = s.problem.solve_batch(guard)
    total1, why1 = s.problem.follow_counts()
    s.close()
    print('handed over', total1 - total0, 'by reason', [a - b for a, b in zip(why1, why0)], 'status of the scenario', res['stats'][7, ST['STATUS']], 'iterations', res['stats'][7, ST['ITERS']])
    assert total1 - total0 == 1
    assert [a - b for a, b in zip(why1, why0)] == [1, 0, 0, 0, 0, 0, 0, 0]
    others = np.arange(B) != 7
    assert _same_bits(res['z'][others], plain['z'][others]) and _same_bits(_records(res['stats'])[others], plain['stats'][others])


def test_early_results_run_in_the_twin_kernels():
    from mseetc._device import ST
    N = 100
    train, track = cases.train_default(), cases.track_00()
    scen = None
    runs = {}
    for how in ('default', 'begun', 'budget'):
        s = _solver(train, track, N)
        if scen is None:
            scen = s._scenarios(1541.0*np.linspace(1.0, 1.25, B), 0, 1, 1)
        assert s.problem.last_first_pass() == '-'
        if how == 'begun':
            res = s.problem.solve_batch_begin(scen, want_multipliers=True).result()
        else:
            if how == 'budget':
                s.problem.iteration_budget(400)      # (more than any of the scenarios needs: nobody is handed over)
            res = s.problem.solve_batch(scen, want_multipliers=True)
        runs[how] = (s.problem.last_first_pass(), res['z'].copy(), _records(res['stats']), s.problem.follow_counts()[0])
        s.close()
    print({how: r[0] for how, r in runs.items()})
    default, begun, budget = runs['default'][0], runs['begun'][0], runs['budget'][0]
    # the twin is solve_kernel_early with the template arguments of the default solve_kernel (mangled: the length in front of the name)
    assert '12solve_kernelI' in default and begun == budget
    assert default.replace('12solve_kernelI', '18solve_kernel_earlyI') == begun
    assert np.all(runs['default'][2][:, ST['STATUS']] == 0)
    for how in ('begun', 'budget'):
        assert runs[how][3] == 0
        assert _same_bits(runs[how][1], runs['default'][1]) and _same_bits(runs[how][2], runs['default'][2])
