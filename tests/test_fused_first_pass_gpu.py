"""
Round 11 on the device: the default first passes of the fused family hold one integrator (numSteps = 1, numApprox = 1); a problem with another integrator runs
in the twin (solve_kernel_early), which keeps the run-time choice.
Needs an MI355X: run with -m gpu.

Tolerances: those of tests/test_gpu_parity.py (_compare) -- objective 1e-8 relative, every variable 1e-6 relative to max(1, |z|), iterations within 2.
"""
import numpy as np
import pytest

import cases

pytestmark = pytest.mark.gpu

OBJ_RTOL = 1e-8
Z_RTOL = 1e-6
B = 16

# (train, crop of track 00, N, shortest and longest running time of the 16 scenarios, geometry).  Screened with the oracle: from the profile start every
# scenario converges without a second-order correction for each of the three integrators below -- a first pass without SOCK hands such a scenario over, which
# is not what these tests are about (the tests assert the screening)
SHAPES = [('both', 1500, 2, (160.0, 200.0), (64, 1)), ('both', 4000, 7, (260.0, 320.0), (64, 1)), ('both', 12000, 30, (760.0, 900.0), (64, 1)),
          ('both', None, 100, (1541.0, 1926.0), (64, 2)),
          ('fig10', 1500, 2, (200.0, 240.0), (64, 1)), ('fig10', 4000, 7, (300.0, 360.0), (64, 1)), ('fig10', 12000, 30, (520.0, 650.0), (64, 1)),
          ('fig10', None, 100, (1700.0, 2000.0), (64, 2))]
# from the reference's starting point (PART = 3) the one-brake train needs other running times on the two shortest horizons: no correction in the oracle there
REFERENCE_T = {('fig10', 2): (240.0, 300.0), ('fig10', 7): (260.0, 300.0)}


def _train(variant):
    return cases.train_default() if variant == 'both' else cases.train_fig10()


def _solver(train, track, N, steps=(1, 1), start='profile'):
    from mseetc.ocp import casadiSolver
    return casadiSolver(train, track, dict(numIntervals=N, maxIterations=500, integrationOptions=dict(numSteps=steps[0], numApproxSteps=steps[1])), startingPoint=start)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _records(stats):
    "stats records (status, iterations, cost, ...) without their time stamps"
    from mseetc._device import ST
    out = stats.copy()
    out[:, ST['CYC_TOTAL']] = out[:, ST['CYC_KKT']] = 0
    return out


_oracle_cache = {}


def _oracle(variant, crop, N, T, steps, start):
    "the oracle's batch, computed once per case and shared"
    from oracle import oracle
    key = (variant, crop, N, T, steps, start)
    if key not in _oracle_cache:
        train, track = _train(variant), cases.track_00(crop)
        prob = cases.oracle_problem(train, track, N, numSteps=steps[0], numApproxSteps=steps[1])
        s = _solver(train, track, N, steps, start)
        scen = s._scenarios(np.linspace(T[0], T[1], B), 0, 1, 1)
        zr, sr, nfail = oracle.solve_batch(prob, scen, start=start)
        zr.setflags(write=False); sr.setflags(write=False)
        _oracle_cache[key] = (scen, zr, sr, nfail)
    return _oracle_cache[key]


def _parity(res, zr, sr, label):
    from mseetc._device import ST
    st = res['stats']
    dz = np.max(np.abs(res['z'] - zr)/np.maximum(1.0, np.abs(zr)), axis=1)
    dobj = np.abs(st[:, ST['OBJ']] - sr[:, ST['OBJ']])/np.abs(sr[:, ST['OBJ']])
    dit = np.abs(st[:, ST['ITERS']] - sr[:, ST['ITERS']])
    print('%s: objective %.3e, variables %.3e, iterations differ by at most %d' % (label, dobj.max(), dz.max(), dit.max()))
    assert np.all(st[:, ST['STATUS']] == 0), st[:, ST['STATUS']]
    assert np.all(dobj <= OBJ_RTOL) and np.all(dz <= Z_RTOL) and np.all(dit <= 2)


@pytest.mark.parametrize('variant,crop,N,T,geometry', SHAPES)
def test_compiled_in_integrator_against_the_run_time_choice(variant, crop, N, T, geometry):
    "numSteps = 1, numApprox = 1: a plain launch runs the default kernel, a begun batch its twin -- the fixed integrator against the run-time one, bit for bit"
    from mseetc._device import ST
    train, track = _train(variant), cases.track_00(crop)
    scen, zr, sr, nfail = _oracle(variant, crop, N, T, (1, 1), 'profile')
    assert nfail == 0 and np.all(sr[:, ST['STATUS']] == 0) and not np.any(sr[:, ST['N_SOC']])
    s = _solver(train, track, N)
    assert s.problem.geometry() == geometry
    plain = s.problem.solve_batch(scen)
    plain = dict(name=s.problem.last_first_pass(), z=plain['z'].copy(), stats=plain['stats'].copy())
    begun = s.problem.solve_batch_begin(scen).result()
    twin = s.problem.last_first_pass()
    total, why = s.problem.follow_counts()
    s.close()
    print(plain['name'], twin)
    assert '12solve_kernelI' in plain['name'] and plain['name'].replace('12solve_kernelI', '18solve_kernel_earlyI') == twin
    assert total == 0
    # z, cost, status and iterations (and the rest of the records)
    assert _same_bits(begun['z'], plain['z']) and _same_bits(_records(begun['stats']), _records(plain['stats']))
    _parity(plain, zr, sr, 'N %d %s, profile start' % (N, variant))


@pytest.mark.parametrize('steps', [(2, 1), (1, 2)])
@pytest.mark.parametrize('variant,crop,N,T,geometry', SHAPES)
def test_another_integrator_runs_in_the_twin(variant, crop, N, T, geometry, steps):
    from mseetc._device import ST
    train, track = _train(variant), cases.track_00(crop)
    scen, zr, sr, nfail = _oracle(variant, crop, N, T, steps, 'profile')
    assert nfail == 0 and np.all(sr[:, ST['STATUS']] == 0) and not np.any(sr[:, ST['N_SOC']])
    s = _solver(train, track, N, steps)
    assert s.problem.geometry() == geometry
    total0, why0 = s.problem.follow_counts()
    res = s.problem.solve_batch(scen)
    total1, why1 = s.problem.follow_counts()
    name = s.problem.last_first_pass()
    s.close()
    assert '18solve_kernel_earlyI' in name      # the twin, by name
    assert total1 == total0 and why1 == why0      # nothing handed over
    _parity(res, zr, sr, 'N %d %s, numSteps %d, numApprox %d' % ((N, variant) + steps))


@pytest.mark.parametrize('variant,crop,N,T,geometry', SHAPES)
def test_the_first_pass_behind_the_multiplier_estimate(variant, crop, N, T, geometry):
    "the reference's starting point: PART = 3 holds the compiled-in integrator too"
    from mseetc._device import ST
    T = REFERENCE_T.get((variant, N), T)
    train, track = _train(variant), cases.track_00(crop)
    scen, zr, sr, nfail = _oracle(variant, crop, N, T, (1, 1), 'reference')
    assert nfail == 0 and np.all(sr[:, ST['STATUS']] == 0)
    s = _solver(train, track, N, start='reference')
    res = s.problem.solve_batch(scen)
    name = s.problem.last_first_pass()
    s.close()
    assert '12solve_kernelI' in name and 'Li3E' in name      # the default kernel with PART = 3
    _parity(res, zr, sr, 'N %d %s, reference start' % (N, variant))
