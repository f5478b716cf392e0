"""
Speed restrictions per scenario on the device (include/mseetc_hip.h: msd_problem_speed_restrictions; casadiSolver.solveBatch(speedRestrictions=...)).
Every restricted scenario is checked against the CPU oracle solving the restricted problem as a problem of its own: the oracle's Problem.bmax is
replaced by the scenario's row of limits (casadiSolver.restrictedLimits, pinned against the host's track code in tests/test_speed_restrictions.py).

Track 00_var_speed_limit_100, v0 = vN = 1, RK4 with one step; the sets S0 ... S5 of tests/test_speed_restrictions.py.  Tolerances: those of
tests/test_gpu_parity.py (_compare: objective 1e-8 relative, variables 1e-6 relative to max(1, |z|), iterations within 2, b_N exact, t_N <= T (1 + 1.01e-8)),
in every case, the streamed kernel and the collocation integrator included.
"""

import numpy as np
import pytest

import cases
from test_gpu_parity import OBJ_RTOL, Z_RTOL
from test_speed_restrictions import S0, S2, S3, S5, SETS, IO

pytestmark = pytest.mark.gpu

T_RUN = 2300.0
KWH_MARGIN = 1.0      # the oracle's costs under S2 ... S5 exceed the cost under S0 by 2.2 ... 30.8 kWh: rows that are ignored fail this


def _solver(train, N, start='profile', **opts):
    from mseetc.ocp import casadiSolver
    return casadiSolver(train, cases.track_00(), dict(dict(numIntervals=N, maxIterations=500, integrationOptions=IO), **opts), startingPoint=start)


def _under(prob, row):
    "the oracle's problem with the scenario's row of limits in place of its own"
    from oracle import oracle
    return oracle.Problem(prob.ip, prob.dp, prob.ds, prob.grad, prob.curv, row, prob.vlim0, prob.vlimN, prob.totalMass, prob.positions)


def _against_oracle(res, k, prob, row, start):
    from oracle import oracle
    from oracle.oracle import DP
    sc = res['scenarios'][k]
    dp = prob.dp.copy()
    dp[DP['T0']], dp[DP['TEND']], dp[DP['V0SQ']], dp[DP['VNSQ']] = sc
    ref = oracle.solve(_under(prob, row), dp, start=start)
    assert ref['stats']['STATUS'] == 0 and res['status'][k] == 0
    dobj = abs(res['stats'][k, 2] - ref['stats']['OBJ'])/abs(ref['stats']['OBJ'])
    dz = np.max(np.abs(res['z'][k] - ref['z'])/np.maximum(1.0, np.abs(ref['z'])))
    dit = abs(int(res['iterations'][k]) - int(ref['stats']['ITERS']))
    print('scenario %d: objective %.3e  variables %.3e  iterations %d / %d' % (k, dobj, dz, int(res['iterations'][k]), int(ref['stats']['ITERS'])))
    assert dobj <= OBJ_RTOL
    assert dz <= Z_RTOL
    assert dit <= 2
    assert res['z'][k][-1] == sc[3]
    assert res['z'][k][-2] <= sc[1]*(1 + 1.01e-8)
    return ref


def _batch_against_oracle(solver, prob, sets, restricted=None, **kw):
    "one batch, a set per scenario, at T_RUN; `restricted`: the scenarios whose cost must exceed the cost of scenario 0 (set S0)"
    res = solver.solveBatch(T_RUN, multipliers=True, speedRestrictions=sets, **kw)
    assert np.all(res['status'] == 0), res['status']
    rows = solver.restrictedLimits(sets, len(sets))
    for k in range(len(sets)):
        _against_oracle(res, k, prob, rows[k], solver.startingPoint)
    for k in (restricted if restricted is not None else range(2, len(sets))):
        assert res['cost'][k] > res['cost'][0] + KWH_MARGIN, (k, res['cost'])
    return res


@pytest.mark.parametrize('N', [63, 64, 100, 700])
def test_rows_on_the_device(N):
    "limit_rows_kernel against the numpy statement of the rule, bit for bit"
    s = _solver(cases.train_default(), N)
    pos = s.points.index.values
    sets = SETS + [[(pos[10], pos[12], 10.0)]]      # (end points exactly on nodes)
    want = s.restrictedLimits(sets, len(sets))
    rs = s._restrictions(sets)
    got = s.problem.speed_restrictions(rs['count'], rs['records']).limit_rows(len(sets))
    assert got.shape == want.shape and np.array_equal(got, want)
    assert not np.array_equal(got[2], got[0])
    # one restriction per scenario at most: the narrowest records
    rs = s._restrictions([S2, S0])
    assert rs['records'].shape[1] == 1
    assert np.array_equal(s.problem.speed_restrictions(rs['count'], rs['records']).limit_rows(2), want[[2, 0]])
    s.problem.speed_restrictions(None)
    with pytest.raises(ValueError):
        s.problem.limit_rows(2)
    s.close()


@pytest.mark.parametrize('start', ['reference', 'profile'])
@pytest.mark.parametrize('N', [63, 64, 100, 130])      # 64 x 1 first pass, 64 x 2, node constants in LDS, two waves
@pytest.mark.parametrize('variant', ['both', 'rg'])
def test_restricted_batches_vs_oracle(variant, N, start):
    train = cases.train_default() if variant == 'both' else cases.train_fig10()
    s = _solver(train, N, start)
    _batch_against_oracle(s, cases.oracle_problem(train, cases.track_00(), N), SETS)
    s.close()


@pytest.mark.parametrize('start', ['reference', 'profile'])
def test_restricted_batch_streamed_vs_oracle(start):
    train = cases.train_fig10()
    s = _solver(train, 700, start, maxIterations=1000)
    _batch_against_oracle(s, cases.oracle_problem(train, cases.track_00(), 700, maxIterations=1000), [S0, S3, S5], restricted=(1, 2))
    s.close()


@pytest.mark.parametrize('start', ['reference', 'profile'])
def test_restricted_batch_collocation_vs_oracle(start):
    "a family outside the fused iteration; its follow-up kernel is the streamed one"
    train = cases.train_default()
    s = _solver(train, 63, start, integrationMethod='IRK', integrationOptions=dict(order=2, numSteps=1, numApproxSteps=1))
    prob = cases.oracle_problem(train, cases.track_00(), 63, integration=dict(integrationMethod='IRK', order=2, collMethod='radau', maxIter=10))
    _batch_against_oracle(s, prob, [S0, S2, S5], restricted=(1, 2))
    s.close()


def test_row_k_stays_with_scenario_k_through_the_scenario_counter():
    "more scenarios than resident workgroups: the workgroups draw scenario indices from the launch's counter"
    train, N, B = cases.train_default(), 63, 4200
    s = _solver(train, N)
    sets = [SETS[k % 6] for k in range(B)]
    res = s.solveBatch(T_RUN, multipliers=True, speedRestrictions=sets)
    assert np.all(res['status'] == 0)
    for k in range(6):
        same = np.arange(k, B, 6)
        assert np.all(res['z'][same] == res['z'][k]), k
        assert np.all(res['lam_g'][same] == res['lam_g'][k]), k
        assert np.all(res['stats'][same][:, [0, 1, 2, 3, 4]] == res['stats'][k, [0, 1, 2, 3, 4]]), k
    prob, rows = cases.oracle_problem(train, cases.track_00(), N), s.restrictedLimits(SETS, 6)
    for k in range(6):
        _against_oracle(res, B - 6 + k, prob, rows[k], s.startingPoint)
    assert np.all(res['cost'][2:6] > res['cost'][0] + KWH_MARGIN)
    s.close()


def test_row_k_stays_with_scenario_k_through_the_follow_up_list():
    "an iteration budget of 3 hands every scenario to the follow-up kernel, which takes scenario indices off the list"
    train, N = cases.train_default(), 64
    s = _solver(train, N)
    before = s.problem.follow_counts()
    s.problem.iteration_budget(3)
    _batch_against_oracle(s, cases.oracle_problem(train, cases.track_00(), N), SETS)
    after = s.problem.follow_counts()
    assert after[1][7] - before[1][7] == 6      # (reason 7: the budget ran out)
    s.problem.iteration_budget(0)
    s.close()


def test_state_of_the_rows():
    from mseetc import _device
    train, N = cases.train_default(), 100
    s = _solver(train, N)
    T = np.full(6, T_RUN)
    with_rows = s.solveBatch(T, multipliers=True, speedRestrictions=SETS)
    assert np.all(with_rows['status'] == 0) and np.all(with_rows['cost'][2:] > with_rows['cost'][0] + KWH_MARGIN)
    # cleared after the solve: the next one is the plain problem's, bit for bit a fresh solver's
    plain = s.solveBatch(T, multipliers=True)
    fresh = _solver(train, N)
    want = fresh.solveBatch(T, multipliers=True)
    assert np.array_equal(plain['z'], want['z']) and np.array_equal(plain['lam_g'], want['lam_g']) and np.array_equal(plain['cost'], want['cost'])
    assert np.array_equal(with_rows['z'][0], want['z'][0])      # (set S0 inside a restricted batch: the problem's own limits)
    fresh.close()

    # C level: rows of 6 scenarios, a launch of 4 -> MSD_E_INVALID (ValueError); rows of 6 again -> solved under them; reconfigure clears them
    rs = s._restrictions(SETS)
    scen = s._scenarios(T, 0, 1, 1)
    s.problem.speed_restrictions(rs['count'], rs['records'])
    with pytest.raises(ValueError):
        s.problem.solve_batch(scen[:4])
    d = [s.problem.alloc(8*n) for n in (4*4, 4*s.problem.nz, 4*_device.ST['COUNT'])]
    s.problem.to_device(d[0], scen[:4])
    with pytest.raises(ValueError):
        s.problem.solve_batch_device(4, d[0], d[1], None, d[2])
    for p in d:
        s.problem.free(p)
    again = s.problem.solve_batch(scen, want_multipliers=True)
    assert np.array_equal(again['z'], with_rows['z'])
    s.problem.reconfigure(s._desc)
    with pytest.raises(ValueError):
        s.problem.limit_rows(6)
    assert np.array_equal(s.problem.solve_batch(scen[:4])['z'], want['z'][:4])

    # two handles on one device: slices of the rows per handle, the bits of one handle
    two = s.solveBatch(T, multipliers=True, speedRestrictions=SETS, devices=[0, 0])
    assert np.array_equal(two['z'], with_rows['z']) and np.array_equal(two['lam_g'], with_rows['lam_g'])
    assert np.array_equal(s.solveBatch(T, devices=[0, 0])['z'], want['z'])      # (cleared on both)

    # early results under restrictions: the rows of the partial result are final where the mask is set
    calls = []
    early = s.solveBatch(T, multipliers=True, speedRestrictions=SETS, onFirstPass=lambda mask, part: calls.append((mask.copy(), {k: np.copy(v) for k, v in part.items()})))
    assert len(calls) == 1
    mask, part = calls[0]
    assert mask.any()
    assert np.array_equal(part['z'][mask], early['z'][mask]) and np.array_equal(part['cost'][mask], early['cost'][mask])
    assert np.array_equal(early['z'], with_rows['z'])

    # a warm start from the batch's own solution, under the same rows
    warm = s.solveBatch(T, speedRestrictions=SETS, guess=with_rows['z'])
    assert np.all(warm['status'] == 0)
    assert np.allclose(warm['cost'], with_rows['cost'], rtol=1e-7, atol=0)

    # the end speeds are clipped to the restricted limits
    res = s.solveBatch(T_RUN, initialVelocity=20, terminalVelocity=20, speedRestrictions=[S0, S5])
    assert res['scenarios'][:, 2].tolist() == [20.0**2, (40/3.6)**2] and res['scenarios'][:, 3].tolist() == [20.0**2, (40/3.6)**2]
    assert np.all(res['status'] == 0)
    s.close()


def test_running_time_infeasible_only_under_the_restriction():
    """
    T = 1700 s at N = 100: feasible on the open line and under S2, below the minimum running time under S3 and S5 (minimum running times of the
    oracle's time-optimal problem under the rows: 1479.9 / 1615.5 / 1781.7 / 1926.7 s).  The certificate is the time-optimal twin under the scenario's rows.
    """
    from oracle import oracle
    from mseetc import _device
    train, N, T = cases.train_default(), 100, 1700.0
    sets = [S0, S2, S3, S5]
    s = _solver(train, N)
    res = s.solveBatch(T, multipliers=True, speedRestrictions=sets)
    assert res['status'].tolist() == [0, 0, _device.STATUS_INFEASIBLE, _device.STATUS_INFEASIBLE]
    rows = s.restrictedLimits(sets, 4)
    prob = cases.oracle_problem(train, cases.track_00(), N)
    for k in (0, 1):
        _against_oracle(res, k, prob, rows[k], s.startingPoint)
    tmin, ok = s.minimumTime(res['scenarios'], speedRestrictions=sets)
    assert np.all(ok)
    twin = cases.oracle_problem(train, cases.track_00(), N, energyOptimal=False, losses='none')
    loose = max(3*cases.track_00().length/train.velocityMax, 3*T)
    for k, printed in enumerate((1479.9, 1615.5, 1781.7, 1926.7)):
        p = _under(twin, rows[k])
        ref = oracle.solve(p, p.scenario(loose), start='profile')
        assert ref['stats']['STATUS'] == 0
        assert abs(ref['z'][-2] - printed) <= 0.05
        print('minimum running time %d: %.4f s, oracle %.4f s' % (k, tmin[k], ref['z'][-2]))
        assert abs(tmin[k] - ref['z'][-2]) <= 1e-6*ref['z'][-2]
    s.close()
