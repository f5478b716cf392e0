"""
Parity of the HIP path (through the C ABI) with the CPU oracle on the same seeded inputs, plus size-independent
properties at the benchmark sizes.  Needs an MI355X: run with -m gpu.

Tolerances: BASELINE.json's north_star asks for 1e-4 relative on energy and terminal constraints; the HIP kernel
and the oracle implement the same algorithm, so much tighter bounds are asserted.  The default (`_compare`): objective 1e-8 relative,
every variable 1e-6 relative to max(1,|z|), iteration counts within 2.  Where a test asserts something wider, it says why next to the
number; the wider bounds in this file are
  * objective 1e-7 where the two solvers end at different barrier parameters (the last barrier test looks at a dual infeasibility that is
    rounding noise by then: one of them may stop one reduction further down the central path -- see test_randomized_problems_vs_oracle);
  * variables 1e-5 on the 256-scenario samples and 1e-4 on the config-3 sample and the long horizons (flat directions of the optimum:
    loss slacks and coasting speeds that the objective barely sees);
  * objective 1e-6 / variables 1e-3 between the two starting points of one problem (two interior-point paths to one optimum);
  * iteration counts within 5 on the dynamic-loss solves (spline rows: one backtracking decision taken differently costs several);
  * the closed loops of config 4: measured times 1e-6, speeds 1e-5, costs 1e-5 early and 5e-3 late in the journey (the energy of the last
    kilometres is steep in the running-time reserve).
All of them are inside north_star's 1e-4 on energy and terminal constraints.
"""

import numpy as np
import pytest

import cases
from nlp_numpy import kkt_certificate

pytestmark = pytest.mark.gpu

OBJ_RTOL = 1e-8
Z_RTOL = 1e-6


def _solver(train, track, N, energyOptimal=True, numSteps=1, numApproxSteps=1, start='reference', maxIterations=500, restoration=True, watchdogTrigger=0):
    # the oracle comparisons pin the whole iteration, so both sides start from the same point; 'reference' unless a test says otherwise
    from mseetc.ocp import casadiSolver
    opts = dict(numIntervals=N, maxIterations=maxIterations, energyOptimal=energyOptimal,
                integrationOptions=dict(numSteps=numSteps, numApproxSteps=numApproxSteps))
    return casadiSolver(train, track, opts, startingPoint=start, restoration=restoration, watchdogTrigger=watchdogTrigger)


def _compare(solver, prob, T, **kw):
    from oracle import oracle
    res = solver.solveBatch(T, multipliers=True, **kw)
    assert np.all(res['status'] == 0), res['status']
    for k in range(len(res['status'])):
        sc = res['scenarios'][k]
        dp = prob.dp.copy()
        from oracle.oracle import DP
        dp[DP['T0']], dp[DP['TEND']], dp[DP['V0SQ']], dp[DP['VNSQ']] = sc
        ref = oracle.solve(prob, dp, start=solver.startingPoint)
        assert ref['stats']['STATUS'] == 0
        obj = res['stats'][k, 2]
        assert abs(obj - ref['stats']['OBJ']) <= OBJ_RTOL*abs(ref['stats']['OBJ'])
        assert np.max(np.abs(res['z'][k] - ref['z'])/np.maximum(1.0, np.abs(ref['z']))) <= Z_RTOL
        assert abs(int(res['iterations'][k]) - int(ref['stats']['ITERS'])) <= 2
        # terminal constraints: b_N = vN^2 exactly (parameter), t_N <= T (relaxed by 1e-8 like IPOPT)
        assert res['z'][k][-1] == sc[3]
        assert res['z'][k][-2] <= sc[1]*(1 + 1.01e-8)
    return res


def test_stage_eval_matches_oracle():
    from oracle import oracle
    solver = _solver(cases.train_default(), cases.track_00(), 100, numSteps=2, numApproxSteps=2)
    prob = cases.oracle_problem(cases.train_default(), cases.track_00(), 100, numSteps=2, numApproxSteps=2)
    rng = np.random.default_rng(11)
    n = 257
    b, w, ds = rng.uniform(300, 1500, n), rng.uniform(-0.4, 0.5, n), rng.uniform(5, 300, n)
    grad, curv = rng.uniform(-0.015, 0.015, n), rng.uniform(-1/320, 1/320, n)
    out = solver.problem.stage_eval(b, w, ds, grad, curv)
    for k in range(n):
        ref = oracle.stage_eval(prob, b[k], w[k], ds[k], grad[k], curv[k])
        assert np.allclose(out[k], ref, rtol=1e-12, atol=1e-15)


def test_stage_eval_independent_of_the_oracle_source():
    """
    The device's interval map checked WITHOUT the oracle (whose stage functions share their derivation with the kernel's):
    values against the numpy restatement of tests/nlp_numpy.py, first derivatives against complex-step differentiation of
    that restatement, second derivatives against central differences of the device's own first derivatives, and the
    integrated ODE against scipy's DOP853 on the figure-4 braking cases (simulations/figure4.py:22-23: 100 m of braking
    with f = -0.5 N/kg end at 1 and 10 km/h) with the reference's high-resolution setting numSteps = 50.
    """
    from scipy.integrate import solve_ivp
    from oracle.oracle import DP
    for numSteps, numApprox in ((1, 1), (2, 2), (2, 0)):
        solver = _solver(cases.train_default(), cases.track_00(), 100, numSteps=numSteps, numApproxSteps=numApprox)
        nlp = cases.numpy_nlp(cases.oracle_problem(cases.train_default(), cases.track_00(), 100, numSteps=numSteps, numApproxSteps=numApprox))
        rng = np.random.default_rng(17)
        n = 64
        b, w, ds = rng.uniform(300, 1500, n), rng.uniform(-0.4, 0.5, n), rng.uniform(5, 300, n)
        grad, curv = rng.uniform(-0.015, 0.015, n), rng.uniform(-1/320, 1/320, n)
        out = solver.problem.stage_eval(b, w, ds, grad, curv)
        c = np.abs(curv)
        crv = np.where(c <= 1/300, nlp.g*0.5*c/(1 - 30*c), nlp.g*0.65*c/(1 - 55*c))           # train.py:252-253
        nlp.ds, nlp.G = ds, nlp.g*grad/nlp.rho + crv/nlp.rho
        tau, bp = nlp.interval(b, w)
        assert np.allclose(out[:, 0], tau, rtol=1e-12, atol=0) and np.allclose(out[:, 1], bp, rtol=1e-12, atol=0)
        h = 1e-30
        tb, bb = nlp.interval(b + 1j*h, w + 0j)
        tw, bw = nlp.interval(b + 0j, w + 1j*h)
        for col, ref in ((2, tb.imag/h), (3, tw.imag/h), (4, bb.imag/h), (5, bw.imag/h)):
            assert np.all(np.abs(out[:, col] - ref) <= 1e-10*np.maximum(1e-6, np.abs(ref)))
        e = 1e-5
        up, dn = solver.problem.stage_eval(b*(1 + e), w, ds, grad, curv), solver.problem.stage_eval(b*(1 - e), w, ds, grad, curv)
        uw, dw = solver.problem.stage_eval(b, w + e, ds, grad, curv), solver.problem.stage_eval(b, w - e, ds, grad, curv)
        db, dww = (up[:, 2:6] - dn[:, 2:6])/(2*e*b[:, None]), (uw[:, 2:6] - dw[:, 2:6])/(2*e)
        # columns: 6 tau_bb 7 tau_bw 8 tau_ww 9 b+_bb 10 b+_bw 11 b+_ww
        for col, ref in ((6, db[:, 0]), (7, dww[:, 0]), (7, db[:, 1]), (8, dww[:, 1]), (9, db[:, 2]), (10, dww[:, 2]), (10, db[:, 3]), (11, dww[:, 3])):
            # (differences of first derivatives that carry the 1-2 ulp of the device's division: absolute floor 5e-9)
            assert np.all(np.abs(out[:, col] - ref) <= 2e-4*np.abs(ref) + 5e-9)
    # figure 4: 100 pieces of 1 m with the joint RK4 (numSteps = 50, numApproxSteps = 0) against the ODE itself
    solver = _solver(cases.train_default(), cases.track_00(), 100, numSteps=50, numApproxSteps=0)
    prob = cases.oracle_problem(cases.train_default(), cases.track_00(), 100)
    dp = prob.dp
    for v0kmh, expect in ((36.61894, 1.0), (37.95880, 10.0)):
        bcur, tcur = (v0kmh/3.6)**2, 0.0
        for _ in range(100):
            o = solver.problem.stage_eval([bcur], [-0.5], [1.0], [0.0], [0.0])[0]
            tcur, bcur = tcur + o[0], o[1]
        assert abs(np.sqrt(bcur)*3.6 - expect) < 2e-3
        rhs = lambda s_, y: [1/np.sqrt(y[1]), 2*(-0.5 - (dp[DP['SR0']] + dp[DP['SR1']]*np.sqrt(y[1]) + dp[DP['SR2']]*y[1]))]
        sol = solve_ivp(rhs, [0, 100.0], [0.0, (v0kmh/3.6)**2], rtol=1e-13, atol=1e-13, method='DOP853')
        assert abs(bcur - sol.y[1, -1]) < 1e-8*max(1, sol.y[1, -1]) and abs(tcur - sol.y[0, -1]) < 1e-6*sol.y[0, -1]


@pytest.mark.parametrize('name,B', [('c1', 1024), ('c2', 8192)])
def test_full_batches_both_starts_same_optimum(name, B):
    """
    The library's default starting point (device-built profile) against the reference's cold start (ocp.py:325-339) on the FULL
    batches of BASELINE configs 1 and 2: every scenario converges from both, to the same optimum (objective within 1e-8
    relative for 99 % of the scenarios and within 1e-6 for all: both solves stop at a scaled KKT error of 1e-8, which pins the
    objective of a flat problem to about 1e-7), terminal constraints hold; and a random sample of 256 scenarios of each batch
    agrees with the oracle solving the same NLPs.
    """
    from mseetc import workloads as wl
    from oracle import oracle
    train, track, N = wl.config(name)
    T = wl.c1_times(B) if name == 'c1' else wl.c2_times(B)
    res = {}
    for start in ('profile', 'reference'):
        s = _solver(train, track, N, start=start)
        res[start] = s.solveBatch(T)
        assert np.all(res[start]['status'] == 0), (start, np.flatnonzero(res[start]['status'] != 0)[:10])
        z = res[start]['z']
        assert np.all(z[:, -1] == 1.0) and np.all(z[:, -2] <= T*(1 + 1.01e-8))
        s.close()
    cp, cr = res['profile']['cost'], res['reference']['cost']
    rel = np.abs(cp - cr)/np.abs(cr)
    assert rel.max() <= 1e-6 and np.quantile(rel, 0.99) <= 1e-8, (rel.max(), int(np.argmax(rel)), np.quantile(rel, 0.99))
    # the trajectory (t, b) is what the energy determines; how a braking force is split between the two brakes is only weakly determined
    assert np.max(np.abs(res['profile']['z'] - res['reference']['z'])/np.maximum(1.0, np.abs(res['reference']['z']))) <= 1e-3
    assert res['profile']['iterations'].mean() < 0.6*res['reference']['iterations'].mean()
    prob = cases.oracle_problem(train, track, N)
    pick = np.random.default_rng(99).choice(B, 256, replace=False)
    scen = np.stack([np.zeros(256), T[pick], np.ones(256), np.ones(256)], axis=1)
    zo, sto, nfail = oracle.solve_batch(prob, scen, nthreads=0, start='profile')
    assert nfail == 0
    from oracle.oracle import ST as OST
    assert np.max(np.abs(cp[pick] - sto[:, OST['OBJ']])/np.abs(sto[:, OST['OBJ']])) <= OBJ_RTOL
    assert np.max(np.abs(res['profile']['z'][pick] - zo)/np.maximum(1.0, np.abs(zo))) <= 10*Z_RTOL      # 128 000 variables: the tail of the 1e-6 the small batches meet


def test_config1_small_batch_vs_oracle():
    # BASELINE config 1 shape (N=100, VIRM6 defaults, both brakes), first 16 of the seeded running times
    train, track = cases.train_default(), cases.track_00()
    _compare(_solver(train, track, 100), cases.oracle_problem(train, track, 100), cases.c1_times(16))


def test_config2_CH_track_vs_oracle():
    train, track = cases.train_default(), cases.track_CH()
    _compare(_solver(train, track, 200), cases.oracle_problem(train, track, 200), cases.c2_times(8))


def test_figure10_configuration_and_gpops_limit():
    import pandas as pd
    from pathlib import Path
    train = cases.train_fig10()
    e = {}
    for N in (100, 300):
        res = _compare(_solver(train, cases.track_00(), N), cases.oracle_problem(train, cases.track_00(), N), [1541.0])
        e[N] = res['cost'][0]
    g2 = pd.read_csv(Path(__file__).resolve().parent / 'golden' / '00_var_speed_limit_100_GPOPSII.csv')['Energy [kWh]'].iloc[0]
    assert abs((9*e[300] - e[100])/8 - g2) < 0.005      # (measured: 0.0016 kWh of 440.14)


def test_figure10_solution_against_the_gpops_trajectory():
    """
    The only reference-held TRAJECTORIES of this OCP: the HIP solution of figure10.py's configuration at N = 1000 and N = 5000 (streamed
    kernels) follows GPOPS-II's v(s) and t(s), closer with every refinement -- max |dv| 0.21 -> 0.08 m/s, rms 0.054 -> 0.018 m/s, max |dt| 2.3 -> 0.6 s of
    1541 s (first order in 1/N: piecewise-constant forces against GPOPS's hp-collocation; N = 100 / 300: 2.1 / 0.64 m/s).  The energies: 440.377 / 440.181 kWh
    against 440.1406.
    """
    train, track = cases.train_fig10(), cases.track_00()
    dev = {}
    for N in (1000, 5000):
        s = _solver(train, track, N, start='profile', maxIterations=1000)
        res = s.solveBatch([1541.0])
        assert res['status'][0] == 0
        dev[N] = cases.gpops_profile_deviation(res['z'][0], np.diff(s.points.index.values)) + (float(res['cost'][0]),)
        s.close()
    assert dev[1000][0] < 0.25 and dev[1000][1] < 0.065 and dev[1000][2] < 2.6, dev
    assert dev[5000][0] < 0.10 and dev[5000][1] < 0.025 and dev[5000][2] < 0.8, dev
    assert dev[5000][0] < 0.5*dev[1000][0] and dev[5000][2] < 0.4*dev[1000][2]
    assert abs(dev[1000][3] - 440.3766) < 2e-3 and abs(dev[5000][3] - 440.1810) < 2e-3 and dev[5000][3] > 440.1406


def test_minimum_time_constant_of_figure5():
    # simulations/figure5.py:96 -- an output of the reference's own solver
    train = cases.train_fig5()
    train.powerLosses = lambda f, v: 0
    solver = _solver(train, cases.track_00(8500), 300, energyOptimal=False)
    prob = cases.oracle_problem(train, cases.track_00(8500), 300, energyOptimal=False, losses='none')
    res = _compare(solver, prob, [400.0], terminalVelocity=100/3.6, initialVelocity=1)
    assert abs(res['z'][0][-2] - 272.4726) < 1.5e-4
    assert abs(res['cost'][0] - res['z'][0][-2]) < 1e-2     # cost [s] = t_N + tiny regularisation


def test_initial_time_and_velocities_and_joint_rk4():
    # MPC-like re-solve: initialTime > 0, initialVelocity in the middle of the range; joint (t,b) RK4 with 2 steps
    train, track = cases.train_default(), cases.track_00(crop=20000)
    _compare(_solver(train, track, 40), cases.oracle_problem(train, track, 40), [900.0, 950.0], initialTime=100.0, initialVelocity=20.0, terminalVelocity=5.0)
    _compare(_solver(train, track, 64, numSteps=2, numApproxSteps=0), cases.oracle_problem(train, track, 64, numSteps=2, numApproxSteps=0), [800.0])


@pytest.mark.parametrize('start', ['reference', 'profile'])
@pytest.mark.parametrize('N,variant', [(63, 'both'), (100, 'rg'), (127, 'both'), (150, 'rg'), (255, 'both'), (300, 'rg'), (383, 'both'), (450, 'rg'), (560, 'both')])
def test_every_launch_geometry_vs_oracle(N, variant, start):
    """
    One solve per launch geometry (64x1, 64x2, 128x2, 192x2, 256x2, 320x2: one to five waves per scenario) against the oracle,
    from both starting points and for both control sets (both brakes / regenerative brake only, figure10.py:16-22): the
    stage-parallel KKT solve exchanges data between lanes and waves differently in every one of them.
    """
    train = cases.train_default() if variant == 'both' else cases.train_fig10()
    track = cases.track_00()
    _compare(_solver(train, track, N, start=start), cases.oracle_problem(train, track, N), [1541.0])


@pytest.mark.parametrize('N', [700, 1000, 5000])
def test_long_horizons_streamed_kernel_vs_oracle(N):
    """
    simulations/table3.py:34 sweeps numIntervals up to 5000; beyond 560 intervals the stage blocks leave LDS and the streamed
    kernel (1024 threads x 5 nodes, blocks in device memory) takes over.  Same NLP, same optimum as the oracle.
    """
    from oracle import oracle
    train, track = cases.train_fig10(), cases.track_00()       # table3.py uses the figure-10 train
    s = _solver(train, track, N, start='profile', maxIterations=1000)
    assert s.problem.geometry() == {700: (512, 2), 1000: (512, 2), 5000: (512, 10)}[N]
    res = s.solveBatch([1541.0, 1620.0])
    assert np.all(res['status'] == 0), res['status']
    prob = cases.oracle_problem(train, track, N, maxIterations=1000)
    for k, T in enumerate((1541.0, 1620.0)):
        ref = oracle.solve(prob, prob.scenario(T), start='profile')
        assert ref['stats']['STATUS'] == 0
        assert abs(res['cost'][k] - ref['stats']['OBJ']) <= OBJ_RTOL*abs(ref['stats']['OBJ'])
        assert np.max(np.abs(res['z'][k] - ref['z'])/np.maximum(1.0, np.abs(ref['z']))) <= 1e-5
        assert res['z'][k][-1] == 1.0 and res['z'][k][-2] <= T*(1 + 1.01e-8)
    s.close()


def _random_problem(seed, tmp_path):
    "A random TTOBench-style track (speed limits, gradients, sometimes curves) and a randomly perturbed VIRM6, as the loaders would read them."
    import json
    from mseetc.track import Track, computeDiscretizationPoints
    rng = np.random.default_rng(1000 + seed)
    L = float(rng.uniform(6e3, 40e3))
    cut = lambda k: np.sort(rng.uniform(0.05*L, 0.95*L, k)).round(0)
    lim = [[0.0, float(rng.choice([100, 120, 140]))]] + [[float(p), float(rng.choice([80, 100, 120, 140, 160]))] for p in cut(rng.integers(1, 4))]
    grd = [[0.0, float(rng.uniform(-6, 6))]] + [[float(p), float(rng.uniform(-12, 12))] for p in cut(rng.integers(2, 7))]
    data = {"metadata": {"id": "rnd%d" % seed, "library version": "TTOBench v1.1"}, "altitude": {"unit": "m", "value": 0},
            "stops": {"unit": "m", "values": [0.0, L]},
            "speed limits": {"units": {"position": "m", "velocity": "km/h"}, "values": lim},
            "gradients": {"units": {"position": "m", "slope": "permil"}, "values": grd}}
    (tmp_path / ("rnd%d.json" % seed)).write_text(json.dumps(data))
    track = Track(config={'id': 'rnd%d' % seed}, pathJSON=tmp_path)
    if rng.random() < 0.4:
        r = float(rng.uniform(400, 1500))
        track.importCurvatureTuples([[0.0, np.inf, np.inf], [float(round(0.3*L)), r, r], [float(round(0.3*L) + 600), np.inf, np.inf]])
    train = cases.train_default()
    train.mass *= float(rng.uniform(0.85, 1.2))
    train.etaTraction, train.etaRgBrake = float(rng.uniform(0.75, 0.95)), float(rng.uniform(0.6, 0.9))
    kind = rng.integers(0, 3)
    if kind == 1:
        train.forceMinPn = 0                       # regenerative brake only
    elif kind == 2:
        train.forceMin = 0                         # pneumatic brake only
    rows = len(track.mergeDataFrames())
    N = int(rng.integers(max(rows + 6, 24), 260))
    for _ in range(20):                            # a breakpoint on a fill-in node is an error of the grid (track.py:103-105): next N
        try:
            computeDiscretizationPoints(track, N)
            break
        except ValueError:
            N += 1
    return train, track, N, rng


@pytest.mark.parametrize('seed', range(24))
def test_randomized_problems_vs_oracle(seed, tmp_path):
    """
    Problems nobody tuned anything on: random tracks (length, speed-limit sections, gradients up to 12 permil, sometimes a curve), a
    perturbed train with a random brake configuration, a random horizon (24 ... 260 intervals: one to three waves per scenario) and
    running times 8 ... 45 % above the minimum, which the time-optimal twin of the problem provides.  Energy-optimal and time-optimal
    solves against the oracle.
    """
    train, track, N, rng = _random_problem(seed, tmp_path)
    v0, vN = float(rng.uniform(1, 15)), float(rng.uniform(1, 15))
    fast = _solver(train, track, N, energyOptimal=False, start='profile')
    Tloose = 3*track.length/train.velocityMax       # a bound the train can meet (a far looser one only costs the time-optimal solve iterations)
    rt = fast.solveBatch([Tloose], initialVelocity=v0, terminalVelocity=vN)
    assert rt['status'][0] == 0
    tmin = float(rt['z'][0][-2])
    po = cases.oracle_problem(train, track, N, energyOptimal=False, losses='none')
    ot = oracle_solve = __import__('oracle.oracle', fromlist=['x'])
    reft = ot.solve(po, po.scenario(Tloose, 0.0, vN, v0), start='profile')
    assert reft['stats']['STATUS'] == 0 and abs(tmin - reft['z'][-2]) <= 1e-7*tmin
    T = tmin*np.array([1.08, 1.2, 1.45])
    s = _solver(train, track, N, start='profile')
    res = s.solveBatch(T, initialVelocity=v0, terminalVelocity=vN)
    assert np.all(res['status'] == 0), (seed, N, res['status'])
    assert int(res['stats'][:, 13].sum()) == 0        # no fallbacks from the stage-parallel KKT solve
    pe = cases.oracle_problem(train, track, N)
    for k in range(3):
        ref = ot.solve(pe, pe.scenario(float(T[k]), 0.0, vN, v0), start='profile')
        assert ref['stats']['STATUS'] == 0
        # Same final barrier parameter: same point to OBJ_RTOL.  Where the two solvers' last barrier test (E_mu <= 10 mu, on a dual
        # infeasibility that is rounding noise by then: 1e-8 against 9e-8 on seed 22) falls differently, one of them ends a barrier
        # reduction further down the central path and its objective is lower by about mu times the number of active bounds: 1e-7
        same_mu = abs(res['stats'][k, 4] - ref['stats']['MU']) <= 1e-3*ref['stats']['MU']
        assert abs(res['cost'][k] - ref['stats']['OBJ']) <= (OBJ_RTOL if same_mu else 1e-7)*abs(ref['stats']['OBJ']), (seed, N, k)
        assert np.max(np.abs(res['z'][k] - ref['z'])/np.maximum(1.0, np.abs(ref['z']))) <= 1e-4, (seed, N, k)
    assert np.all(np.diff(res['cost']) < 0)
    s.close(); fast.close()


def test_fast_reciprocal_and_square_root():
    """
    The fused iteration's reciprocal and square root (csrc/msd_fastmath.hpp: v_rcp_f64 / v_rsq_f64 + refinement, without the compiler's range
    scaling and special-case fix-up) against the correctly rounded results in extended precision: at most one ulp on operands of the iteration's
    range (slacks from 1e-13, multipliers to 1e13, squared speeds), the square root at most half an ulp off the rounded one.  The reciprocal
    square root scales the Jacobian of every interval: at 2^-45 -- one refinement step less -- a short-horizon re-solve of config 4 stalled at a
    dual residual of 1e-6 (test_config4_full_size_warm_and_cold).
    """
    from mseetc._device import fastmath_probe
    rng = np.random.default_rng(5)
    x = np.concatenate([10.0**rng.uniform(-13, 13, 200000), rng.uniform(0.5, 2.0, 100000), rng.uniform(1.0, 7000.0, 100000),
                        [1.0, 2.0, 4.0, 0.25, 3.0, 1e-300, 1e300, np.nextafter(1.0, 2.0), np.nextafter(1.0, 0.0)]])
    rc, sq, rs = fastmath_probe(x)
    xl = x.astype(np.longdouble)
    def ulps(got, exact):
        return np.abs((got.astype(np.longdouble) - exact)/np.spacing(np.asarray(exact, dtype=np.float64)).astype(np.longdouble)).astype(np.float64)
    e_rc, e_sq, e_rs = ulps(rc, 1/xl), ulps(sq, np.sqrt(xl)), ulps(rs, 1/np.sqrt(xl))
    assert e_rc.max() <= 1.0 and e_sq.max() <= 1.0 and e_rs.max() <= 1.5, (e_rc.max(), e_sq.max(), e_rs.max())
    assert (rc == 1.0/x).mean() > 0.9 and (sq == np.sqrt(x)).mean() > 0.99      # (mostly the rounded result itself)
    # what the callers' finiteness / positivity tests rely on
    rc0, sq0, rs0 = fastmath_probe(np.array([0.0, -1.0, np.inf, np.nan]))
    assert not np.isfinite(rc0[0]) and rc0[1] == -1.0 and not np.isfinite(rc0[3])
    assert not (sq0[1] >= 0) and not np.isfinite(sq0[3])


@pytest.mark.parametrize('seed,factor', [(176, 2.0), (22, 3.0), (35, 3.0)])
def test_degenerate_zero_cost_journeys_vs_oracle(seed, factor, tmp_path):
    """
    Random problems of the round-4 sweeps on which device and oracle parted (profiles/r04/random_sweep_150_450.txt, random_sweep_loose_2.5_3.txt): loose
    schedules on downhill tracks -- a zero-cost optimum, a singular reduced Hessian, Newton steps of norm 200 along the flat directions.  Seed 176
    (N = 154, pneumatic brake only, twice the minimum running time) ended with Restoration_Failed on the device from both starting points; seeds 22 and
    35 (three times the minimum) ended 1.7e-6 from the oracle's objective.  Cause (round 5): the last interval always eliminated Fel through its
    b row; with Fel on a bound its barrier curvature of 1e11 went through every reduced entry, the value function of stage N-1 lost all its digits and
    the inertia of stage N-2 was decided by rounding (last_interval in msd_kernel.hpp; compute_direction in the oracle).  Both now eliminate the force
    with the smaller curvature.  From both starting points: a solution (the reference surfaces anything else as df = None, ocp.py:359-370), the oracle's
    objective and -- from the same starting point -- the oracle's iterates.
    """
    from oracle import oracle
    train, track, N, rng = _random_problem(seed, tmp_path)
    v0, vN = float(rng.uniform(1, 15)), float(rng.uniform(1, 15))
    po = cases.oracle_problem(train, track, N, energyOptimal=False, losses='none')
    reft = oracle.solve(po, po.scenario(3*track.length/train.velocityMax, 0.0, vN, v0), start='profile')
    assert reft['stats']['STATUS'] == 0
    T = factor*float(reft['z'][-2])
    pe = cases.oracle_problem(train, track, N)
    ref = oracle.solve(pe, pe.scenario(T, 0.0, vN, v0), start='profile')
    assert ref['stats']['STATUS'] == 0
    scale = max(1.0, abs(ref['stats']['OBJ']))      # (kWh; the journeys cost nothing)
    for start in ('profile', 'reference'):
        s = _solver(train, track, N, start=start)
        res = s.solveBatch([T], initialVelocity=v0, terminalVelocity=vN)
        s.close()
        assert res['status'][0] == 0, (seed, start, res['status'], res['iterations'])
        assert abs(res['cost'][0] - ref['stats']['OBJ']) <= 1e-7*scale, (seed, start, res['cost'][0], ref['stats']['OBJ'])
        if start == 'profile':
            assert abs(int(res['iterations'][0]) - int(ref['stats']['ITERS'])) <= 2, (seed, res['iterations'][0], ref['stats']['ITERS'])
            assert np.max(np.abs(res['z'][0] - ref['z'])/np.maximum(1.0, np.abs(ref['z']))) <= 1e-5


def test_velocity_clipping_like_the_reference():
    # initial/terminal speeds are clipped to [vmin, local speed limit] (ocp.py:343-344)
    train, track = cases.train_default(), cases.track_00(crop=20000)
    s = _solver(train, track, 40)
    res = s.solveBatch([800.0], initialVelocity=0.1, terminalVelocity=1000.0)
    assert res['scenarios'][0][2] == 1.0 and abs(res['scenarios'][0][3] - (140/3.6)**2) < 1e-9


@pytest.mark.parametrize('case', ['c1', 'c1_tight', 'c1_loose', 'c2', 'fig10', 'mintime', 'mpc_resolve'])
def test_kkt_certificate_of_gpu_solution(case):
    """
    First-order optimality of the GPU's (z, lam_g) checked by an implementation that shares nothing with the kernel or the
    oracle: the numpy restatement of the reference's NLP (tests/nlp_numpy.py, ocp.py:166-284) with complex-step Jacobians.
    Covers the benchmark problems themselves (configs 1 and 2: both brakes, JSON efficiencies and power limits), for which the
    reference holds no stored solution, next to the figure-10 and minimum-time configurations that it does pin.
    """
    kw, eo = {}, True
    if case.startswith('c1'):
        train, track, N, T = cases.train_default(), cases.track_00(), 100, {'c1': 1600.0, 'c1_tight': 1500.0, 'c1_loose': 1772.0}[case]
    elif case == 'c2':
        train, track, N, T = cases.train_default(), cases.track_CH(), 200, 1300.0
    elif case == 'fig10':
        train, track, N, T = cases.train_fig10(), cases.track_00(), 100, 1541.0
    elif case == 'mintime':
        train, track, N, T, eo = cases.train_fig5(), cases.track_00(8500), 100, 400.0, False
        kw = dict(terminalVelocity=100/3.6, initialVelocity=1)
    else:
        train, track, N, T = cases.train_default(), cases.track_00(crop=20000), 40, 900.0
        kw = dict(initialTime=100.0, initialVelocity=20.0, terminalVelocity=5.0)
    solver = _solver(train, track, N, energyOptimal=eo, start='profile')
    res = solver.solveBatch([T], multipliers=True, **kw)
    assert res['status'][0] == 0
    prob = cases.oracle_problem(train, track, N, energyOptimal=eo, losses='static' if eo else 'none')      # (only packs the problem data for the numpy NLP)
    nlp = cases.numpy_nlp(prob)
    sc = res['scenarios'][0]
    cert = kkt_certificate(nlp, res['z'][0], res['lam_g'][0], sc[0], sc[1], sc[2], sc[3])
    # feasibility: IPOPT's bound relaxation (1e-8 relative).  stat / sign_g are complementarity products of the multipliers the
    # certificate reconstructs: the solver stops when the scaled optimality error is below 1e-8 and IPOPT's unscaled side
    # condition compl_inf_tol = 1e-4 holds, so 1e-4 is the bound the stopping rule guarantees (typical values are 1e-6 .. 1e-5)
    assert cert['feas_g'] < 1.5e-8 and cert['feas_z'] < 1.5e-8 and cert['stat'] < 1e-4 and cert['sign_g'] < 1e-4, cert
    # the objective the kernel reports is the NLP's objective at z
    assert abs(float(nlp.obj(res['z'][0])) - res['stats'][0, 2]) <= 1e-10*abs(res['stats'][0, 2])


def test_full_config1_batch_properties():
    # B = 1024 at the benchmark size: every scenario converges; energy decreases monotonically with the allowed running time
    # (a longer T relaxes the only scenario-dependent constraint); batch result == single-scenario result (no cross-talk).
    train, track = cases.train_default(), cases.track_00()
    solver = _solver(train, track, 100)
    T = cases.c1_times(1024)
    res = solver.solveBatch(T)
    assert np.all(res['status'] == 0)
    order = np.argsort(T)
    assert np.all(np.diff(res['cost'][order]) <= 1e-6)
    for k in (0, 511, 1023):
        one = solver.solveBatch([T[k]])
        assert np.array_equal(one['z'][0], res['z'][k])
    # determinism (the reference's scripts assert identical iteration counts over repeated solves, figure6.py:191-193)
    again = solver.solveBatch(T)
    assert np.array_equal(again['z'], res['z']) and np.array_equal(again['iterations'], res['iterations'])


def test_dataframe_surface():
    train, track = cases.train_default(), cases.track_00()
    solver = _solver(train, track, 100)
    df, stats = solver.solve(1541)
    assert df is not None and set(stats) == {'Solver status', 'IP iterations', 'CPU time [s]', 'Cost'}
    for col in ['Position [m]', 'Velocity [m/s]', 'Force (el) [N]', 'Force (pnb) [N]', 'Slacks', 'Energy [kWh]', 'Losses [kWh]', 'Acceleration [m/s^2]']:
        assert col in df.columns
    assert df.index.name == 'Time [s]' and len(df) == 101
    # energy accounting equals the cost minus the 1e-3 smoothing term
    assert abs(df['Energy [kWh]'].sum() - stats['Cost']) < 1e-3*stats['Cost']
    # infeasible running time -> failure is reported, not raised (ocp.py:364-370)
    df2, st2 = solver.solve(900)
    assert df2 is None and st2['Solver status'] != 'Solve_Succeeded'


def test_config3_rolling_stock_perturbations_vs_oracle():
    # BASELINE config 3: +-5 % (clipped at 2 sigma) perturbation of mass, r0, r1, r2 per scenario.  Reference mechanism:
    # a new Train(config={...}) per scenario (train.py:44-62); here one launch with per-scenario overrides.
    from oracle import oracle
    from mseetc.train import Train
    rng = np.random.default_rng(20260614)
    B = 6
    T = 1541*(1 + 0.15*rng.random(B))
    pert = 1 + 0.05*np.clip(rng.standard_normal((B, 4)), -2, 2)
    base = cases.train_default()
    solver = _solver(base, cases.track_00(), 100)
    res = solver.solveBatch(T, mass=base.mass*pert[:, 0], r0=base.r0*pert[:, 1], r1=base.r1*pert[:, 2], r2=base.r2*pert[:, 3])
    assert np.all(res['status'] == 0)
    for k in range(B):
        tr = Train(config={'id': 'NL_Intercity_VIRM6',
                           'mass': {'unit': 'kg', 'value': base.mass*pert[k, 0]},
                           'rolling resistance r0': {'unit': 'N', 'value': base.r0*pert[k, 1]},
                           'rolling resistance r1': {'unit': 'N/(m/s)', 'value': base.r1*pert[k, 2]},
                           'rolling resistance r2': {'unit': 'N/(m/s)^2', 'value': base.r2*pert[k, 3]}})
        prob = cases.oracle_problem(tr, cases.track_00(), 100)
        ref = oracle.solve(prob, prob.scenario(float(T[k])))
        assert ref['stats']['STATUS'] == 0
        assert abs(res['cost'][k] - ref['stats']['OBJ']) <= OBJ_RTOL*abs(ref['stats']['OBJ'])
        # the two sides compute r/M with different roundings; the energy agrees to 1e-8 but weakly determined variables
        # (how the last braking metres are split between the two brakes) move by ~1e-5 -> the north_star tolerance is used here
        assert np.max(np.abs(res['z'][k] - ref['z'])/np.maximum(1.0, np.abs(ref['z']))) <= 1e-4


def test_config4_shrinking_horizon_vs_oracle():
    # BASELINE config 4 in miniature: 4 re-solves, stride 2, 1 % measurement noise, 6 scenarios; the same driver is run
    # with the device solver and with the oracle standing in for it -- same noise stream, so the logs must agree.
    from mseetc.mpc import shrinkingHorizon
    from oracle import oracle

    class OracleSolver():
        "casadiSolver look-alike backed by the oracle (checker only)"
        def __init__(self, train, track, opts):
            from mseetc.ocp import casadiSolver
            self._front = casadiSolver(train, track, opts)     # host-side packing only; never touches the device
            self.points, self.withPnBrake = self._front.points, self._front.withPnBrake
            io = opts.get('integrationOptions', {})
            self._prob = cases.oracle_problem(train, track, opts['numIntervals'], numSteps=io.get('numSteps', 1), numApproxSteps=io.get('numApproxSteps', 0))
        def solveBatch(self, T, initialTime=0, terminalVelocity=1, initialVelocity=1, classifyFailures=False):
            scen = self._front._scenarios(T, initialTime, terminalVelocity, initialVelocity)
            z, st, nfail = oracle.solve_batch(self._prob, scen, nthreads=4)
            return dict(z=z, status=st[:, 0].astype(int), iterations=st[:, 1].astype(int), cost=st[:, 2])

    train, track = cases.train_default(), cases.track_00(crop=20000)
    opts = dict(numIntervals=40, maxIterations=300, integrationOptions=dict(numSteps=1, numApproxSteps=1))
    T = np.linspace(800.0, 950.0, 6)
    from mseetc.ocp import casadiSolver
    gpu = shrinkingHorizon(train, track, opts, T, numResolves=4, noise=0.01, seed=3,
                           solverFactory=lambda a, b, c: casadiSolver(a, b, c, startingPoint='reference'))
    ref = shrinkingHorizon(train, track, opts, T, numResolves=4, noise=0.01, seed=3, solverFactory=lambda a, b, c: OracleSolver(a, b, c))
    assert len(gpu) == len(ref) == 4
    for g, r in zip(gpu, ref):
        assert g['numIntervals'] == r['numIntervals'] and g['position'] == r['position']
        assert np.array_equal(g['status'], r['status']) and np.all(g['status'] == 0)
        assert np.allclose(g['t0'], r['t0'], rtol=1e-7) and np.allclose(g['v0'], r['v0'], rtol=1e-7)
        assert np.allclose(g['cost'], r['cost'], rtol=1e-7)


@pytest.mark.parametrize('case', ['config1', 'config2', 'fig10', 'fig5', 'mintime'])
def test_profile_start_same_optimum_fewer_iterations(case):
    # the default starting point (MSD_START_PROFILE): iterate-for-iterate equal to the oracle's profile start, the optimum of
    # the reference's cold start, and markedly fewer iterations
    if case == 'config1':
        train, track, N, kw, T = cases.train_default(), cases.track_00(), 100, {}, cases.c1_times(12)
    elif case == 'config2':
        train, track, N, kw, T = cases.train_default(), cases.track_CH(), 200, {}, cases.c2_times(6)
    elif case == 'fig10':
        train, track, N, kw, T = cases.train_fig10(), cases.track_00(), 300, {}, np.array([1541.0])
    elif case == 'fig5':
        train = cases.train_fig5(); train.etaTraction = train.etaRgBrake = 0.73
        track, N, kw, T = cases.track_00(8500), 100, dict(terminalVelocity=100/3.6, initialVelocity=1), 272.4726*np.array([1.05, 1.2, 1.3])
    else:
        train = cases.train_fig5()
        track, N, kw, T = cases.track_00(8500), 300, dict(terminalVelocity=100/3.6, initialVelocity=1), np.array([400.0])
    eo = case != 'mintime'
    prob = cases.oracle_problem(train, track, N, energyOptimal=eo, losses='static' if eo else 'none')
    fast = _solver(train, track, N, energyOptimal=eo, start='profile')
    res = _compare(fast, prob, T, **kw)
    cold = _solver(train, track, N, energyOptimal=eo, start='reference').solveBatch(T, **kw)
    assert np.all(cold['status'] == 0)
    assert np.allclose(res['cost'], cold['cost'], rtol=1e-8)
    assert np.max(np.abs(res['z'] - cold['z'])/np.maximum(1.0, np.abs(cold['z']))) <= 1e-5
    assert res['iterations'].mean() < 0.7*cold['iterations'].mean()


def test_profile_start_falls_back_to_the_reference_point():
    # a scenario that breaks down from the profile start (here: infeasible running times, the line search gives up) is repeated
    # from the reference's point inside the launch; the iterations of both attempts are reported, exactly like the oracle does.
    # (restoration=False: with the restoration phase a hopeless scenario spends hundreds of iterations there before either attempt gives
    # up -- tests/test_restoration.py -- and where exactly that happens is not reproducible to a few iterations; no watchdog procedure for the
    # same reason: these hopeless solves crawl with shortened steps, the procedure starts, and the trial points it takes without the filter's
    # consent send the two implementations different ways -- tests/test_watchdog.py is where the procedure is compared)
    from oracle import oracle
    train, track = cases.train_default(), cases.track_00()
    fast = _solver(train, track, 100, start='profile', restoration=False, watchdogTrigger=-1)
    cold = _solver(train, track, 100, start='reference', restoration=False, watchdogTrigger=-1)
    T = [1541.0, 900.0, 1000.0]
    res, ref = fast.solveBatch(T, classifyFailures=False), cold.solveBatch(T, classifyFailures=False)
    assert list(res['status'] >= 0) == [True, False, False] == list(ref['status'] >= 0)
    prob = cases.oracle_problem(train, track, 100, watchdogTrigger=-1)
    oracle.lib().oracle_set_restoration(0)
    try:
        for k in (1, 2):
            for got, start in ((res, 'profile'), (ref, 'reference')):      # both directions: the second attempt starts from the other point
                chk = oracle.solve(prob, prob.scenario(T[k]), start=start)
                assert got['status'][k] == int(chk['stats']['STATUS'])
                # both attempts are counted; where exactly a hopeless line search gives up depends on alpha_min, whose powers the device
                # evaluates in single precision: a few iterations either way
                assert abs(int(got['iterations'][k]) - int(chk['stats']['ITERS'])) <= 6
            assert abs(int(res['iterations'][k]) - int(ref['iterations'][k])) <= 6        # the same two attempts in the other order
    finally:
        oracle.lib().oracle_set_restoration(1)
    # the iteration limit is not a breakdown: no second attempt, and a cap between the two starting points' needs separates them
    few = _solver(train, track, 100, start='profile', maxIterations=12).solveBatch([1541.0])
    assert few['status'][0] == -1 and few['iterations'][0] == 12
    mid = _solver(train, track, 100, start='profile', maxIterations=30).solveBatch([1541.0])
    late = _solver(train, track, 100, start='reference', maxIterations=30).solveBatch([1541.0])
    assert mid['status'][0] == 0 and late['status'][0] == -1


def test_profile_start_very_loose_schedules():
    # running times many times the minimum (the train crawls at 2-4 m/s): the profile start keeps the start from standstill moving
    # (it starts Fpb where the interior push would put it and lets Fel make up for it) and converges where the reference's
    # starting point runs into a line-search failure
    from oracle import oracle
    train, track = cases.train_default(), cases.track_00()
    prob = cases.oracle_problem(train, track, 100)
    T = [8000.0, 12000.0, 20000.0]
    fast = _solver(train, track, 100, start='profile').solveBatch(T)
    assert np.all(fast['status'] == 0)
    for k, t in enumerate(T):
        ref = oracle.solve(prob, prob.scenario(t), start='profile')
        assert ref['stats']['STATUS'] == 0 and abs(fast['cost'][k] - ref['stats']['OBJ']) <= OBJ_RTOL*abs(ref['stats']['OBJ'])
        assert abs(int(fast['iterations'][k]) - int(ref['stats']['ITERS'])) <= 2
    assert np.all(np.diff(fast['cost']) < 0)      # more time, less energy
    cold = _solver(train, track, 100, start='reference').solveBatch(T)
    assert cold['status'][0] == 0 and abs(cold['cost'][0] - fast['cost'][0]) <= 1e-7*fast['cost'][0]


def test_warm_start_vs_oracle():
    # msd_solve_batch_warm: same iterates as the oracle's warm start (iteration counts equal up to the last convergence test), same optimum as a cold solve
    from oracle import oracle
    train, track = cases.train_default(), cases.track_00()
    N = 100
    solver = _solver(train, track, N)
    prob = cases.oracle_problem(train, track, N)
    T = np.array([1500.0, 1560.0, 1620.0, 1700.0])
    first = solver.solveBatch(T)
    assert np.all(first['status'] == 0)
    T2 = T*1.005
    cold = solver.solveBatch(T2)
    warm = solver.solveBatch(T2, guess=first['z'], warmMu=1e-2, warmPush=1e-3)
    assert np.all(warm['status'] == 0) and np.all(cold['status'] == 0)
    assert np.all(warm['iterations'] < cold['iterations'])
    assert np.allclose(warm['cost'], cold['cost'], rtol=1e-7)
    for k in range(len(T)):
        ref = oracle.solve(prob, prob.scenario(T2[k]), guess=first['z'][k], mu0=1e-2, push=1e-3)
        # the last iterate's error sits at the rounding level (1e-10 ... 3e-9 between oracle and kernel builds, tol = 1e-8): the
        # convergence test of the last iteration can fall either way, so the counts may differ by one
        assert ref['stats']['STATUS'] == 0 and abs(int(ref['stats']['ITERS']) - int(warm['iterations'][k])) <= 1
        assert np.max(np.abs(warm['z'][k] - ref['z'])/np.maximum(1.0, np.abs(ref['z']))) <= 1e-7
    # one guess broadcast over the batch; bad guesses are rejected before the launch
    one = solver.solveBatch(T2, guess=first['z'][1])
    assert np.all(one['status'] == 0) and np.allclose(one['cost'], cold['cost'], rtol=1e-7)
    with pytest.raises(ValueError):
        solver.solveBatch(T2, guess=first['z'][:, :-1])
    bad = first['z'].copy(); bad[0, 3] = np.nan
    with pytest.raises(ValueError):
        solver.solveBatch(T2, guess=bad)


def test_config4_warm_started_mpc_matches_cold():
    # warm-started shrinking horizon: same closed loop as the cold one, fewer iterations
    from mseetc.mpc import shrinkingHorizon
    train, track = cases.train_default(), cases.track_00()
    opts = dict(numIntervals=100, maxIterations=300, integrationOptions=dict(numSteps=1, numApproxSteps=1))
    T = 1541*(1 + 0.15*np.random.default_rng(5).random(16))
    cold = shrinkingHorizon(train, track, opts, T, numResolves=6, noise=0.01, seed=11)
    warm = shrinkingHorizon(train, track, opts, T, numResolves=6, noise=0.01, seed=11, warmStart=True)
    assert len(cold) == len(warm) == 6
    itc = itw = 0
    for k, (c, w) in enumerate(zip(cold, warm)):
        assert np.all(c['status'] == 0) and np.all(w['status'] == 0)
        assert np.allclose(c['t0'], w['t0'], rtol=1e-6) and np.allclose(c['v0'], w['v0'], rtol=1e-6)
        assert np.allclose(c['cost'], w['cost'], rtol=1e-6)
        if k > 0:
            itc += c['iterations'].sum(); itw += w['iterations'].sum()
    assert itw < 0.85*itc      # the cold re-solves already use the profile start (about 21 iterations); warm ones need about 15


def test_config3_full_size_vs_oracle():
    """
    BASELINE config 3 at its per-GPU size (8192 scenarios, running times and rolling stock perturbed per scenario): every scenario
    converges, no fallbacks, and 256 random scenarios agree with the oracle solving the same perturbed NLPs (each with its own
    `Train`: the reference's mechanism, train.py:44-62).
    """
    from oracle import oracle
    from mseetc import workloads as wl
    from mseetc.track import computeDiscretizationPoints
    train, track, N = wl.config('c3')
    solver = _solver(train, track, N, start='profile')
    B = 8192
    T, pert = wl.c3_scenarios(B, train)
    res = solver.solveBatch(T, **pert)
    assert np.all(res['status'] == 0), np.unique(res['status'], return_counts=True)
    assert int(res['stats'][:, 13].sum()) == 0 and int(res['stats'][:, 8].sum()) == 0      # scan fallbacks, inertia corrections
    assert res['iterations'].max() <= 40
    pts = computeDiscretizationPoints(track, N)
    opts = dict(numIntervals=N, maxIterations=500, energyOptimal=True, minimumVelocity=1, numSteps=1, numApproxSteps=1)
    sample = np.random.default_rng(7).choice(B, 256, replace=False)
    probs, dps = [], []
    for k in sample:
        tr = wl.train_default()
        tr.mass, tr.r0, tr.r1, tr.r2 = pert['mass'][k], pert['r0'][k], pert['r1'][k], pert['r2'][k]
        prob = oracle.pack_problem(tr, pts, opts, 1, (1 - tr.etaTraction)/tr.etaTraction, 1 - tr.etaRgBrake, track.length)
        ref = oracle.solve(prob, prob.scenario(float(T[k])), start='profile')
        assert ref['stats']['STATUS'] == 0
        same_mu = abs(res['stats'][k, 4] - ref['stats']['MU']) <= 1e-3*ref['stats']['MU']      # (see test_randomized_problems_vs_oracle)
        assert abs(res['cost'][k] - ref['stats']['OBJ']) <= (OBJ_RTOL if same_mu else 1e-7)*abs(ref['stats']['OBJ']), k
        assert abs(int(res['iterations'][k]) - int(ref['stats']['ITERS'])) <= 2, k
        assert np.max(np.abs(res['z'][k] - ref['z'])/np.maximum(1.0, np.abs(ref['z']))) <= 1e-4, k
    solver.close()


def test_config4_full_size_warm_and_cold():
    """
    BASELINE config 4 at its per-GPU size: 512 scenarios x 50 shrinking-horizon re-solves (stride 2, 1 % measurement noise), once from
    cold starts like the reference and once warm-started from the previous solutions and multipliers on the device.  Same closed loop
    (measured states and arrival times to 1e-6 wherever neither loop had to move an arrival time), every re-solve succeeds -- where the
    measured state no longer allows the arrival time, the loop moves it to the certified minimum running time -- and the moved arrival
    times are exactly the scenarios the time-optimal twin declares late.
    """
    from mseetc import workloads as wl
    from mseetc.mpc import shrinkingHorizon
    train, track, N = wl.config('c4')
    T = wl.c1_times(512, seed=20260615)
    logs = {}
    for warm in (False, True):
        logs[warm] = shrinkingHorizon(train, track, wl.options(N), T, numResolves=50, noise=0.01, seed=1, warmStart=warm)
        assert len(logs[warm]) == 50
    cold, warm = logs[False], logs[True]
    moved_c = np.zeros(512, dtype=bool); moved_w = np.zeros(512, dtype=bool)
    itc = itw = 0
    for k, (c, w) in enumerate(zip(cold, warm)):
        assert c['numIntervals'] == w['numIntervals'] == N - 2*k
        # every re-solve ends with a solution: where the arrival time had to move the repeated solve succeeds (the last two horizons,
        # four and two intervals long with a few seconds left, may keep a handful of scenarios that even the margins do not rescue)
        assert (c['status'] < 0).sum() <= (0 if k < 48 else 4) and (w['status'] < 0).sum() <= (0 if k < 48 else 4), (k, c['status'].min(), w['status'].min())
        moved_c |= c['relaxed']; moved_w |= w['relaxed']
        same = ~(moved_c | moved_w)
        # the same closed loop: measured times to 1e-6, measured speeds to 1e-5 (two optima converged to 1e-8 differ by 1e-7 ... 5e-6 in the
        # speed two intervals ahead).  The energies follow to 1e-5 while the running-time reserve is comfortable; towards the end of the
        # journey the energy of the remaining kilometres is steep in the reserve (it diverges at the minimum running time), so a 1e-7
        # difference in the measured time shows as up to 2e-3 there
        assert np.allclose(c['t0'][same], w['t0'][same], rtol=1e-6, atol=1e-6), k
        assert np.allclose(c['v0'][same], w['v0'][same], rtol=1e-5), k
        assert np.allclose(c['cost'][same], w['cost'][same], rtol=1e-5 if k < 30 else 5e-3, atol=1e-5), k
        # a moved arrival time is later than the one asked for, by what 1 % noise on the absolute time can explain
        for log in (c, w):
            m = log['relaxed']
            if m.any():
                assert np.all(log['T'][m] > T[m]) and np.all(log['T'][m] - T[m] < 0.08*T[m])
        if k > 0:
            itc += c['iterations'].sum(); itw += w['iterations'].sum()
    assert itw < 0.8*itc      # primal-dual warm starts: about 10 against 19 iterations per re-solve while the arrival times hold
    # 1 % noise on the absolute time (15 s late in the journey) cannot be made up on the last kilometres: arrival times move from the 28th
    # re-solve on, in both loops for the same scenarios
    assert not moved_c[:].any() or min(k for k, c in enumerate(cold) if c['relaxed'].any()) >= 20
    assert (moved_c ^ moved_w).sum() <= 0.02*512


def test_shifted_primal_dual_warm_start_vs_oracle():
    """
    msd_solve_batch_shifted with msd_problem_keep_duals: the re-solve of a horizon shortened by two intervals starts from the
    previous solutions and multipliers, which never leave the device.  Against the oracle's primal-dual warm start, scenario by
    scenario; a scenario whose first solve failed starts cold inside the same launch.
    """
    import copy
    from oracle import oracle
    from mseetc.track import computeDiscretizationPoints
    train, track, N = cases.train_default(), cases.track_00(), 100
    T = np.array([1541.0, 1600.0, 900.0, 1720.0])           # the third is infeasible: no guess for its re-solve
    s1 = _solver(train, track, N, start='profile')
    s1.problem.keep_duals(True)
    r1 = s1.solveBatch(T, classifyFailures=False)
    assert list(r1['status'] >= 0) == [True, True, False, True]
    pos = computeDiscretizationPoints(track, N).index.values
    track2 = copy.deepcopy(track); track2.updateLimits(positionStart=float(pos[2]))
    s2 = _solver(train, track2, N - 2, start='profile').adoptDevice(s1)
    stp = 5
    t_now = np.where(r1['status'] >= 0, r1['z'][:, stp*2 + 3]*1.003, 60.0)
    v_now = np.where(r1['status'] >= 0, np.sqrt(np.abs(r1['z'][:, stp*2 + 4]))*0.997, 15.0)
    T2 = T.copy(); T2[2] = 1650.0                             # feasible now, but without a guess
    r2 = s2.solveBatch(T2, initialTime=t_now, initialVelocity=v_now, shift=2, warmMu=1e-4, warmPush=1e-3, classifyFailures=False)
    assert np.all(r2['status'] == 0), r2['status']
    prob1, prob2 = cases.oracle_problem(train, track, N), cases.oracle_problem(train, track2, N - 2)
    for k in (0, 1, 3):
        first = oracle.solve_dual(prob1, prob1.scenario(float(T[k])), start='profile')
        sc = prob2.scenario(float(T2[k]), float(t_now[k]), 1.0, float(v_now[k]))
        warm = oracle.solve_dual(prob2, sc, guess=first['z'][stp*2:], duals=first['duals'][2:], mu0=1e-4, push=1e-3)
        cold = oracle.solve(prob2, sc, start='profile')
        assert warm['stats']['STATUS'] == 0
        assert abs(r2['cost'][k] - warm['stats']['OBJ']) <= OBJ_RTOL*abs(warm['stats']['OBJ'])
        assert np.max(np.abs(r2['z'][k] - warm['z'])/np.maximum(1.0, np.abs(warm['z']))) <= 10*Z_RTOL
        assert abs(int(r2['iterations'][k]) - int(warm['stats']['ITERS'])) <= 2
        assert int(r2['iterations'][k]) <= 0.6*int(cold['stats']['ITERS'])
    sc = prob2.scenario(float(T2[2]), float(t_now[2]), 1.0, float(v_now[2]))
    cold = oracle.solve(prob2, sc, start='profile')
    assert abs(int(r2['iterations'][2]) - int(cold['stats']['ITERS'])) <= 2 and abs(r2['cost'][2] - cold['stats']['OBJ']) <= OBJ_RTOL*abs(cold['stats']['OBJ'])
    s2.close()


def test_direct_results_are_the_copied_results():
    """
    msd_problem_direct_results (the Python wrapper's default): the kernels store z* and the multipliers in the page-locked result arrays themselves.
    Same bits as the copies behind the launch, for a batch that goes through the follow-up kernel too; arrays in pageable memory are served by
    copies; a shifted warm start cannot begin from such a solve and says so.
    """
    import ctypes
    from mseetc._device import lib, DeviceError, ST, _d
    train, track, N = cases.train_default(), cases.track_00(), 100
    T = np.concatenate([cases.c1_times(96), [900.0, 11000.0, 15000.0]])      # an infeasible running time and two loose schedules among them
    s = _solver(train, track, N, start='profile')
    prob = s.problem
    scen = s._scenarios(T, 0, 1, 1)
    prob.solve_batch(scen)      # (the handle settles on its first-pass kernel: a launch that hands a second-order correction over switches to the instantiation that has it)
    direct = prob.solve_batch(scen, want_multipliers=True)
    zd, ld, sd = direct['z'].copy(), direct['lam_g'].copy(), direct['stats'].copy()
    assert (sd[:, ST['STATUS']] >= 0).sum() >= 98
    prob.direct_results(False)
    copied = prob.solve_batch(scen, want_multipliers=True)
    ok = copied['stats'][:, ST['STATUS']] >= 0
    assert np.array_equal(zd[ok], copied['z'][ok]) and np.array_equal(ld[ok], copied['lam_g'][ok])
    assert np.array_equal(sd[:, ST['STATUS']], copied['stats'][:, ST['STATUS']]) and np.array_equal(sd[:, ST['ITERS']], copied['stats'][:, ST['ITERS']])
    # pageable arrays with the switch on: copies, same bits
    prob.direct_results(True)
    z = np.zeros_like(zd); st = np.zeros_like(sd); ms = ctypes.c_float(0)
    assert lib().msd_solve_batch(prob._h, len(T), _d(np.ascontiguousarray(scen)), _d(z), None, _d(st), ctypes.byref(ms)) == 0
    assert np.array_equal(z[ok], zd[ok])
    # no device copy behind a direct solve: the shifted warm start refuses
    prob.solve_batch(scen)
    with pytest.raises(ValueError, match='host memory directly'):
        prob.solve_batch(scen, shift=0)
    s.close()


@pytest.mark.parametrize('family', ['loss_table_one_brake', 'loss_table_both_brakes', 'streamed', 'time_optimal'])
def test_structure_compiled_in_matches_the_general_kernels(family):
    """
    Round 6 compiled the structure of the reference's rolling stock (rows on, row bounds, brakes, objective) into the first-pass kernels of three more families: the
    loss table (msd_kernels_dynamic2/3.hip), the streamed static family (msd_kernels_stream5/6.hip) and the time-optimal problem (msd_kernels_time*.hip).  Same
    iterates as the kernels that read that structure from the problem record (msd_tuning("no_full", 1)): status, iteration counts, objective, variables.
    """
    from mseetc._device import lib
    from mseetc.ocp import casadiSolver
    if family.startswith('loss_table'):
        from mseetc.train import Train
        from mseetc.efficiency import totalLossesFunction
        train = Train(config={'id': 'NL_Intercity_VIRM6'})
        if family.endswith('one_brake'):
            train.forceMinPn = 0
        train.powerLosses = totalLossesFunction(train, auxiliaries=27000, etaGear=0.96)
        track, T, kw = cases.track_00(8500), 272.4726*np.array([1.08, 1.15, 1.25, 1.3]), dict(terminalVelocity=100/3.6)      # (not next to the kink bands of DESIGN.md section 8)
        horizons, eo = (50, 100, 180), True
    elif family == 'streamed':
        train, track, T, kw, horizons, eo = cases.train_fig10(), cases.track_00(), np.array([1500.0, 1541.0, 1600.0]), {}, (700,), True
    else:
        train, track, T, kw, horizons, eo = cases.train_default(), cases.track_00(), np.array([1541.0, 1600.0]), {}, (50, 100, 200), True      # (through minimumTime: the twin is built there)
    for N in horizons:
        out = {}
        for general in (0, 1):
            assert lib().msd_tuning(b'no_full', general) == 0
            try:
                s = casadiSolver(train, track, dict(numIntervals=N, maxIterations=500, energyOptimal=eo, integrationOptions=dict(numSteps=1, numApproxSteps=1)), startingPoint='profile')
                if family == 'time_optimal':
                    tmin, ok = s.minimumTime(s._scenarios(T, 0, 1, 1))
                    assert np.all(ok)
                    out[general] = dict(status=np.zeros(len(T)), iterations=np.zeros(len(T)), cost=tmin, z=tmin[:, None])
                else:
                    out[general] = s.solveBatch(T, classifyFailures=False, **kw)
                s.close()
            finally:
                lib().msd_tuning(b'no_full', 0)
        a, b = out[0], out[1]
        assert np.all(a['status'] == 0) and np.all(b['status'] == 0), (family, N, a['status'], b['status'])
        assert np.max(np.abs(a['iterations'] - b['iterations'])) <= 1, (family, N, a['iterations'], b['iterations'])
        assert np.max(np.abs(a['cost'] - b['cost'])/np.maximum(1.0, np.abs(b['cost']))) <= 1e-8, (family, N)      # (two builds of the same arithmetic: FMA contraction differs)
        assert np.max(np.abs(a['z'] - b['z'])/np.maximum(1.0, np.abs(b['z']))) <= 1e-5, (family, N)


def test_handle_reuse_across_problems():
    # msd_problem_reconfigure: one device handle carried through problems of different horizon, track and layout gives the
    # results of fresh handles (the receding-horizon loop reuses its stream and buffers this way)
    train = cases.train_default()
    nopn = cases.train_default(); nopn.forceMinPn = 0
    problems = [(train, cases.track_00(), 100, cases.c1_times(8)), (train, cases.track_00(crop=20000), 40, np.linspace(800.0, 950.0, 5)),
                (train, cases.track_CH(), 200, cases.c2_times(12)), (nopn, cases.track_00(), 100, cases.c1_times(3))]
    carried = None
    for tr, tk, N, T in problems:
        fresh = _solver(tr, tk, N, start='profile')
        want = fresh.solveBatch(T, multipliers=True)
        fresh.close()
        solver = _solver(tr, tk, N, start='profile').adoptDevice(carried)
        got = solver.solveBatch(T, multipliers=True)
        assert np.array_equal(got['status'], want['status']) and np.all(got['status'] == 0)
        assert np.array_equal(got['z'], want['z']) and np.array_equal(got['lam_g'], want['lam_g']) and np.array_equal(got['iterations'], want['iterations'])
        assert carried is None or carried._problem is None
        carried = solver
    carried.close()


def test_dynamic_loss_model_vs_oracle():
    # simulations/figure5.py configuration with the dynamic losses of efficiency.py (fun2): 8.5 km, v0 = 1, vN = 100 km/h
    from oracle import oracle
    from mseetc.train import Train
    from mseetc.efficiency import totalLossesFunction
    from mseetc.track import computeDiscretizationPoints
    train = Train(config={'id': 'NL_Intercity_VIRM6'})
    train.forceMinPn = 0
    train.powerLosses = totalLossesFunction(train, auxiliaries=27000, etaGear=0.96)
    track = cases.track_00(8500)
    oracle.set_loss_table(train.powerLosses.parameters(train.mass*train.rho))
    for N, reserves in ((100, (1.1, 1.2, 1.3)), (300, (1.0, 1.1))):
        solver = _solver(train, track, N)
        pts = computeDiscretizationPoints(track, N)
        prob = oracle.pack_problem(train, pts, dict(numIntervals=N, maxIterations=500, energyOptimal=True, minimumVelocity=1, numSteps=1, numApproxSteps=1),
                                   2, 0.0, 0.0, track.length)
        T = [272.4726*r for r in reserves]
        res = solver.solveBatch(T, terminalVelocity=100/3.6, initialVelocity=1)
        assert np.all(res['status'] == 0)
        for k, t in enumerate(T):
            ref = oracle.solve(prob, prob.scenario(t, terminalVelocity=100/3.6, initialVelocity=1))
            assert ref['stats']['STATUS'] == 0
            assert abs(res['cost'][k] - ref['stats']['OBJ']) <= OBJ_RTOL*abs(ref['stats']['OBJ'])
            assert np.max(np.abs(res['z'][k] - ref['z'])/np.maximum(1.0, np.abs(ref['z']))) <= 1e-5
            # same path up to rounding (order of the wave reductions; until the end of round 3 also 1-2 ulp divisions): with the spline rows one
            # of these five solves took 4 iterations more than the oracle's 41 on the fast-math build (the host emulation of the same code: 41)
            assert abs(int(res['iterations'][k]) - int(ref['stats']['ITERS'])) <= 5


def test_arbitrary_loss_function_vs_oracle():
    """
    train.py:190-219 + utils.py:197-220: `train.powerLosses` may be any function of (F, v).  The device gets it as a table over the train's
    operating range (efficiency.TabulatedLosses, exact for the piecewise cubic used here); kernels against the oracle on the same table for
    the LDS-resident, the collocation and the streamed kernel, and post-processing with the function itself.
    """
    from oracle import oracle
    from mseetc.train import Train
    from mseetc.track import computeDiscretizationPoints
    from mseetc.ocp import casadiSolver
    from test_efficiency import _copper_iron
    train = Train(config={'id': 'NL_Intercity_VIRM6'})
    train.forceMinPn = 0
    train.powerLosses = _copper_iron
    track = cases.track_00(8500)
    fun = train.lossesCallable()
    assert fun.maxDeviation < 1e-12
    oracle.set_loss_table(fun.parameters(train.mass*train.rho))
    for N, T, kw in ((100, (300.0, 330.0, 380.0), {}), (60, (320.0,), dict(integrationMethod='IRK', integrationOptions=dict(order=2, numSteps=1, numApproxSteps=0))),
                     (600, (330.0,), {})):
        opts = dict(numIntervals=N, maxIterations=500, energyOptimal=True, integrationOptions=dict(numSteps=1, numApproxSteps=1))
        opts.update(kw)
        solver = casadiSolver(train, track, opts, startingPoint='reference')
        pts = computeDiscretizationPoints(track, N)
        oopts = dict(numIntervals=N, maxIterations=500, energyOptimal=True, minimumVelocity=1, numSteps=1, numApproxSteps=1 if not kw else 0)
        if kw:
            from mseetc.train import collocationTables
            oopts.update(integrationMethod='IRK', order=2, collMethod='radau', maxIter=10)
            oracle.set_collocation(*collocationTables(2, 'radau'))
        prob = oracle.pack_problem(train, pts, oopts, 2, 0.0, 0.0, track.length)
        res = solver.solveBatch(list(T), terminalVelocity=80/3.6, initialVelocity=1)
        assert np.all(res['status'] == 0), res['status']
        for k, t in enumerate(T):
            ref = oracle.solve(prob, prob.scenario(t, terminalVelocity=80/3.6, initialVelocity=1))
            assert ref['stats']['STATUS'] == 0
            assert abs(res['cost'][k] - ref['stats']['OBJ']) <= OBJ_RTOL*abs(ref['stats']['OBJ'])
            assert np.max(np.abs(res['z'][k] - ref['z'])/np.maximum(1.0, np.abs(ref['z']))) <= 1e-5
            assert abs(int(res['iterations'][k]) - int(ref['stats']['ITERS'])) <= 5
        if N == 100:
            # the solver's surface: a solution frame whose losses are those of the function at the solution (utils.py:261-289)
            df, stats = solver.solve(300.0, terminalVelocity=80/3.6, initialVelocity=1)
            v = df['Velocity [m/s]'].values
            vm = 0.5*(v[:-1] + v[1:])
            fel = df['Force (el) [N]'].values[:-1]
            expect = 1e-6/3.6*np.diff(df['Position [m]'].values)*np.array([_copper_iron(f, w) for f, w in zip(fel, vm)])/vm
            assert np.allclose(df['Losses [kWh]'].values[:-1], expect, rtol=1e-9, atol=1e-12)
            # the slacks sit on the loss rows wherever energy is priced: the frame's energy is the objective up to its smoothing term
            assert abs(np.nansum(df['Energy [kWh]'].values) - stats['Cost']) <= 2e-3*stats['Cost']
            # integrateLosses=True in post-processing (utils.py:261-289) integrates the table on the device: against a quadrature of the function
            # itself along the re-integrated speed of each interval
            from scipy.integrate import solve_ivp
            from mseetc.utils import postProcessDataFrame
            raw = solver.unpack(solver.solveBatch(300.0, terminalVelocity=80/3.6, initialVelocity=1)['z'][0])
            dfb = postProcessDataFrame(raw, solver.points, train, CVODES=False, integrateLosses=True)
            M, model, t = train.mass*train.rho, train.exportModel(), raw.index.values
            ref = []
            for i in range(N):
                G = model.resistance(df['Gradient [permil]'].values[i]/1e3, df['Curvature [1/m]'].values[i])
                ftot = (raw['Force (el) [N]'].values[i] + raw['Force (pnb) [N]'].values[i])/M
                rhs = lambda tt, y: [ftot - (model.sr0 + model.sr1*y[0] + model.sr2*y[0]**2) - G, _copper_iron(raw['Force (el) [N]'].values[i], y[0])]
                sol = solve_ivp(rhs, [0, t[i + 1] - t[i]], [raw['Velocity [m/s]'].values[i], 0.0], method='DOP853', rtol=1e-12, atol=1e-12)
                ref.append(sol.y[1, -1]*(1e-6/3.6))
            assert np.allclose(dfb['Losses [kWh]'].values[:-1], np.array(ref), rtol=1e-5, atol=1e-9)
        solver.close()


def test_constant_efficiencies_through_the_table_are_the_static_kernel():
    "The same NLP through two kernels: closed-form loss rows (static kernel, structure compiled in) and the tabulated function (table kernel)."
    from mseetc.efficiency import TabulatedLosses
    train = cases.train_default()
    track = cases.track_00()
    T = cases.c1_times(8)
    a = _solver(train, track, 100, start='profile')
    ra = a.solveBatch(T)
    a.close()
    et, er = train.etaTraction, train.etaRgBrake
    t2 = cases.train_default()
    t2.powerLosses = TabulatedLosses(lambda f, v: f*v*(f > 0)*(1 - et)/et - (1 - er)*f*v*(f < 0), t2.forceMin, t2.forceMax, t2.velocityMax)
    b = _solver(t2, track, 100, start='profile')
    rb = b.solveBatch(T)
    b.close()
    assert np.all(ra['status'] == 0) and np.all(rb['status'] == 0)
    assert np.max(np.abs(rb['cost'] - ra['cost'])/np.abs(ra['cost'])) <= 1e-7
    assert np.max(np.abs(rb['z'] - ra['z'])/np.maximum(1.0, np.abs(ra['z']))) <= 1e-4


def test_dynamic_losses_with_per_scenario_rolling_stock():
    # config 3's perturbations composed with the loss model of efficiency.py, which the reference composes freely
    # (train.py:44-62 + efficiency.py:101-141): one launch with overrides against one oracle problem per scenario
    from oracle import oracle
    from mseetc.train import Train
    from mseetc.efficiency import totalLossesFunction
    from mseetc.track import computeDiscretizationPoints
    def make(mass=None, r0=None):
        cfg = {'id': 'NL_Intercity_VIRM6'}
        if mass is not None:
            cfg['mass'] = {'unit': 'kg', 'value': mass}
        if r0 is not None:
            cfg['rolling resistance r0'] = {'unit': 'N', 'value': r0}
        tr = Train(config=cfg)
        tr.forceMinPn = 0
        tr.powerLosses = totalLossesFunction(tr, auxiliaries=27000, etaGear=0.96)
        return tr
    base = make()
    track, N = cases.track_00(8500), 100
    solver = _solver(base, track, N)
    pts = computeDiscretizationPoints(track, N)
    fm, fr = np.array([1.0, 1.08, 0.93]), np.array([1.0, 0.9, 1.1])
    T = 272.4726*np.array([1.15, 1.2, 1.25])
    res = solver.solveBatch(T, terminalVelocity=100/3.6, initialVelocity=1, mass=base.mass*fm, r0=base.r0*fr)
    assert np.all(res['status'] == 0)
    for k in range(3):
        tr = make(base.mass*fm[k], base.r0*fr[k])
        oracle.set_loss_table(tr.powerLosses.parameters(tr.mass*tr.rho))
        prob = oracle.pack_problem(tr, pts, dict(numIntervals=N, maxIterations=500, energyOptimal=True, minimumVelocity=1, numSteps=1, numApproxSteps=1),
                                   2, 0.0, 0.0, track.length)
        ref = oracle.solve(prob, prob.scenario(float(T[k]), terminalVelocity=100/3.6, initialVelocity=1))
        assert ref['stats']['STATUS'] == 0
        assert abs(res['cost'][k] - ref['stats']['OBJ']) <= OBJ_RTOL*abs(ref['stats']['OBJ'])
        assert np.max(np.abs(res['z'][k] - ref['z'])/np.maximum(1.0, np.abs(ref['z']))) <= 1e-4
    assert abs(res['cost'][1] - res['cost'][0]) > 1e-3*res['cost'][0]      # the perturbation is visible in the energy


def test_arbitrary_loss_function_with_per_scenario_rolling_stock():
    "The same composition for a tabulated loss function (absolute force on the table axis: a scenario's own mass converts its specific force)."
    from oracle import oracle
    from mseetc.train import Train
    from mseetc.track import computeDiscretizationPoints
    from test_efficiency import _copper_iron
    def make(mass=None, r0=None):
        cfg = {'id': 'NL_Intercity_VIRM6'}
        if mass is not None:
            cfg['mass'] = {'unit': 'kg', 'value': mass}
        if r0 is not None:
            cfg['rolling resistance r0'] = {'unit': 'N', 'value': r0}
        tr = Train(config=cfg)
        tr.forceMinPn = 0
        tr.powerLosses = _copper_iron
        return tr
    base = make()
    track, N = cases.track_00(8500), 100
    solver = _solver(base, track, N)
    pts = computeDiscretizationPoints(track, N)
    fm, fr = np.array([1.0, 1.08, 0.93]), np.array([1.0, 0.9, 1.1])
    T = np.array([300.0, 320.0, 350.0])
    res = solver.solveBatch(T, terminalVelocity=80/3.6, initialVelocity=1, mass=base.mass*fm, r0=base.r0*fr)
    assert np.all(res['status'] == 0)
    for k in range(3):
        tr = make(base.mass*fm[k], base.r0*fr[k])
        oracle.set_loss_table(tr.lossesCallable().parameters(tr.mass*tr.rho))
        prob = oracle.pack_problem(tr, pts, dict(numIntervals=N, maxIterations=500, energyOptimal=True, minimumVelocity=1, numSteps=1, numApproxSteps=1),
                                   2, 0.0, 0.0, track.length)
        ref = oracle.solve(prob, prob.scenario(float(T[k]), terminalVelocity=80/3.6, initialVelocity=1))
        assert ref['stats']['STATUS'] == 0
        assert abs(res['cost'][k] - ref['stats']['OBJ']) <= OBJ_RTOL*abs(ref['stats']['OBJ'])
        assert np.max(np.abs(res['z'][k] - ref['z'])/np.maximum(1.0, np.abs(ref['z']))) <= 1e-4
    solver.close()


def test_multi_handle_launches_overlap():
    """
    msd_solve_batch_multi launches on every handle before it copies any result back (a copy into pageable host memory holds the
    calling thread until the kernel in front of it has finished).  Two handles on the one visible device, 256 scenarios each -- both
    launches fit the device side by side --: the pair must take clearly less than two single launches.
    """
    import time
    train, track = cases.train_default(), cases.track_00()
    s = _solver(train, track, 100, start='profile')
    T1, T2 = cases.c1_times(256), cases.c1_times(512)
    s.solveBatch(T1); s.solveBatch(T2, devices=[0, 0])      # handles, buffers, first launches
    def best(f, n=7):
        ts = []
        for _ in range(n):
            t0 = time.perf_counter(); f(); ts.append(time.perf_counter() - t0)
        return min(ts)
    t_one = best(lambda: s.solveBatch(T1, classifyFailures=False))
    t_two = best(lambda: s.solveBatch(T2, devices=[0, 0], classifyFailures=False))
    assert t_two < 1.7*t_one, (t_one, t_two)
    s.close()


def test_single_process_multi_device_dispatch():
    """
    SURVEY 8(b)/(e): `devices[]` -- one handle and one stream per device from a single process, contiguous slices of the batch,
    no collective.  One GPU is visible to the tests, so the list repeats it (two and three handles on device 0): the sharded
    result must equal the single-handle result bit for bit, for even and ragged splits, with multipliers and overrides.
    """
    from mseetc import _device
    train, track = cases.train_default(), cases.track_00()
    s = _solver(train, track, 100, start='profile')
    T = cases.c1_times(37)
    one = s.solveBatch(T, multipliers=True)
    for devs in ([0, 0], [0, 0, 0], [0]*4, [0]*8):      # (shard equivalence, SURVEY section 4: 1 / 2 / 3 / 4 / 8 contiguous slices, the same bits)
        many = s.solveBatch(T, multipliers=True, devices=devs)
        for key in ('z', 'lam_g', 'status', 'iterations', 'cost'):
            assert np.array_equal(one[key], many[key]), key
    m = train.mass*(1 + 0.03*np.linspace(-1, 1, 37))
    assert np.array_equal(s.solveBatch(T, mass=m)['z'], s.solveBatch(T, mass=m, devices=[0, 0])['z'])
    assert np.array_equal(s.solveBatch(T[:1])['z'], s.solveBatch(T[:1], devices=[0, 0, 0])['z'])      # fewer scenarios than handles
    with pytest.raises((ValueError, _device.DeviceError)):
        s.solveBatch(T, devices=[0, 99])
    s.close()


def test_infeasible_running_time_is_reported_like_ipopt(capsys):
    """
    ocp.py:362-370: a failed solve prints IPOPT's status and returns (None, stats).  A running time below the minimum is
    'Infeasible_Problem_Detected' in IPOPT (end of its restoration phase); here the restoration phase of the device ends such a solve
    with a failure status of its own and the minimum-time certificate (casadiSolver._classify_failures) names the reason.  Feasible neighbours in the same batch are untouched; a scenario that is
    feasible but fails for another reason would keep its own status.
    """
    from mseetc import _device
    train, track = cases.train_default(), cases.track_00()
    for start in ('profile', 'reference'):
        s = _solver(train, track, 100, start=start)
        df, stats = s.solve(900)
        assert df is None and stats['Solver status'] == 'Infeasible_Problem_Detected'
        assert "Solver failed with status 'Infeasible_Problem_Detected'" in capsys.readouterr().out
        res = s.solveBatch([1541.0, 900.0, 1600.0, 1000.0, 1455.0])
        assert list(res['status']) == [0, _device.STATUS_INFEASIBLE, 0, _device.STATUS_INFEASIBLE, _device.STATUS_INFEASIBLE]
        # the certificate is the minimum running time itself: just above it the problem is solved, just below it is infeasible
        twin = _solver(train, track, 100, energyOptimal=False, start='profile')
        tmin = float(twin.solveBatch([5000.0])['z'][0][-2])
        edge = s.solveBatch([tmin*1.002, tmin*0.998])
        assert edge['status'][0] == 0 and edge['status'][1] == _device.STATUS_INFEASIBLE
        # the device's own verdict: a failure -- 'Restoration_Failed' where the restoration phase breaks down itself, 'Infeasible_Problem_
        # Detected' where it converges, or the iteration limit (tests/test_restoration.py); the certificate above settles it
        raw = s.solveBatch([900.0], classifyFailures=False)
        assert raw['status'][0] in (_device.STATUS_MAXITER, _device.STATUS_LINESEARCH, _device.STATUS_INFEASIBLE)
        s.close(); twin.close()


def test_loose_schedules_converge_from_both_starts():
    # 8 to 13 times the minimum running time: from the reference's point the filter line search breaks down (IPOPT would
    # restore); the solver restarts such a scenario from the other starting point inside the launch
    train, track = cases.train_default(), cases.track_00()
    T = np.array([8000.0, 12000.0, 20000.0])
    ref = None
    for start in ('profile', 'reference'):
        s = _solver(train, track, 100, start=start)
        res = s.solveBatch(T)
        assert np.all(res['status'] == 0), (start, res['status'])
        if ref is None:
            ref = res['cost']
        assert np.max(np.abs(res['cost'] - ref)/np.abs(ref)) < 1e-6
        s.close()


def test_postprocessing_integrations_vs_scipy():
    # simulateCVODES (utils.py:164-194) and integrateLosses=True (utils.py:261-289) on the device,
    # checked against scipy's DOP853 at tight tolerance on the same controls.
    from scipy.integrate import solve_ivp
    from mseetc.utils import postProcessDataFrame
    train, track = cases.train_default(), cases.track_00()
    solver = _solver(train, track, 100)
    df, stats = solver.solve(1600)
    assert df is not None
    for col in ('Position - cvodes [m]', 'Velocity - cvodes [m/s]', 'Error position [m]', 'Error velocity [m/s]'):
        assert col in df.columns
    M = train.mass*train.rho
    model = train.exportModel()
    t = df.index.values
    f = df['Force [N]'].values/M
    s, v = df['Position [m]'].values[0], df['Velocity [m/s]'].values[0]
    ps, vs = [s], [v]
    for i in range(100):
        G = model.resistance(df['Gradient [permil]'].values[i]/1e3, df['Curvature [1/m]'].values[i])
        rhs = lambda tt, y: [y[1], f[i] - (model.sr0 + model.sr1*y[1] + model.sr2*y[1]**2) - G]
        sol = solve_ivp(rhs, [0, t[i + 1] - t[i]], [s, v], method='DOP853', rtol=1e-13, atol=1e-13)
        s, v = sol.y[0, -1], sol.y[1, -1]
        ps.append(s); vs.append(v)
    assert np.max(np.abs(df['Position - cvodes [m]'].values - np.array(ps))) < 1e-6
    assert np.max(np.abs(df['Velocity - cvodes [m/s]'].values - np.array(vs))) < 1e-8
    # the RK4/trapezoid transcription error the reference plots (figure5): small but not zero
    assert 0 < df['Error position [m]'].max() < 50 and 0 < df['Error velocity [m/s]'].max() < 1.0

    # integrated losses vs quadrature of the static loss model along the re-integrated speed of each interval
    raw = solver.unpack(solver.solveBatch(1600.0)['z'][0])
    dfb = postProcessDataFrame(raw, solver.points, train, CVODES=False, integrateLosses=True)
    fun = train.lossesCallable()
    fel = raw['Force (el) [N]'].values
    ref = []
    for i in range(100):
        G = model.resistance(df['Gradient [permil]'].values[i]/1e3, df['Curvature [1/m]'].values[i])
        ftot = df['Force [N]'].values[i]/M
        rhs = lambda tt, y: [ftot - (model.sr0 + model.sr1*y[0] + model.sr2*y[0]**2) - G, fun(fel[i], y[0])]
        sol = solve_ivp(rhs, [0, t[i + 1] - t[i]], [raw['Velocity [m/s]'].values[i], 0.0], method='DOP853', rtol=1e-12, atol=1e-12)
        ref.append(sol.y[1, -1]*(1e-6/3.6))
    got = dfb['Losses [kWh]'].values[:-1]
    assert np.allclose(got, np.array(ref), rtol=1e-5, atol=1e-9)
    # mid-point rule (default) and integration agree to the discretisation error
    assert abs(np.nansum(dfb['Losses [kWh]'].values) - np.nansum(df['Losses [kWh]'].values)) < 0.02*np.nansum(df['Losses [kWh]'].values)


def test_edge_cases_sizes_and_errors():
    from mseetc.ocp import casadiSolver
    from mseetc import _device
    from oracle import oracle
    train = cases.train_default()
    # smallest horizons the grid allows on a single-section track: N = 1, 2, 3 (one wave, mostly idle lanes)
    track = cases.track_00(crop=3000)
    for N, T in ((1, 400.0), (2, 330.0), (3, 300.0)):
        s = _solver(train, track, N)
        prob = cases.oracle_problem(train, track, N)
        res = s.solveBatch([T], classifyFailures=False)
        ref = oracle.solve(prob, prob.scenario(T))
        assert res['status'][0] == int(ref['stats']['STATUS'])
        if res['status'][0] == 0:
            assert abs(res['cost'][0] - ref['stats']['OBJ']) <= 1e-7*abs(ref['stats']['OBJ'])
    # geometry boundaries: 63/64 intervals (one node per lane <-> two), 127/128 (one wave <-> two)
    track = cases.track_00(crop=29000)     # (a crop where no fill-in node coincides with the 25 km speed-limit breakpoint)
    for N in (63, 64, 127, 128):
        s = _solver(train, track, N)
        prob = cases.oracle_problem(train, track, N)
        res = s.solveBatch([1100.0, 1250.0])
        assert np.all(res['status'] == 0)
        for k, T in enumerate((1100.0, 1250.0)):
            ref = oracle.solve(prob, prob.scenario(T))
            assert abs(res['cost'][k] - ref['stats']['OBJ']) <= OBJ_RTOL*abs(ref['stats']['OBJ'])
    # largest LDS-resident horizon family (320 threads x 2 nodes): N = 560
    track = cases.track_00()
    s = _solver(train, track, 560)
    res = s.solveBatch([1541.0])
    prob = cases.oracle_problem(train, track, 560)
    ref = oracle.solve(prob, prob.scenario(1541.0))
    assert res['status'][0] == 0 and abs(res['cost'][0] - ref['stats']['OBJ']) <= OBJ_RTOL*abs(ref['stats']['OBJ'])
    # beyond the LDS-resident family the streamed kernel takes over (test_long_horizons_streamed_kernel_vs_oracle); its own limit is loud
    with pytest.raises(_device.DeviceError):
        _solver(train, track, 5200).solveBatch([1541.0])
    # infeasible scenarios fail individually without poisoning their neighbours (failure isolation)
    s = _solver(train, track, 100)
    res = s.solveBatch([1541.0, 900.0, 1600.0, 1000.0])
    assert list(res['status'] >= 0) == [True, False, True, False]
    alone = s.solveBatch([1541.0, 1600.0])
    assert np.array_equal(res['z'][[0, 2]], alone['z'])
    # bad arguments are ValueErrors like the reference's (ocp.py:314-320)
    with pytest.raises(ValueError):
        s.solveBatch([-5.0])
    with pytest.raises(ValueError):
        s.solveBatch([100.0], initialTime=-1.0)
    with pytest.raises(ValueError):
        s.solveBatch([1541.0], mass=[-1.0])
    # maxIterations is honoured and reported like IPOPT's Maximum_Iterations_Exceeded
    few = casadiSolver(train, track, dict(numIntervals=100, maxIterations=5, integrationOptions=dict(numApproxSteps=1)))
    r = few.solveBatch([1541.0])
    assert r['status'][0] == -1 and r['iterations'][0] == 5


def test_second_order_corrections_go_through_the_follow_up_kernel():
    """
    Round 4: the first-pass kernels hold the fused iteration alone; a rejected first trial point that qualifies for a second-order
    correction (W&B section 2.4) hands the scenario to the follow-up kernel, whose general iteration has the correction.  N = 40 on 16 km
    from the profile start: a quarter of these running times take one correction (oracle: N_SOC = 1).  Same iterates as the oracle --
    iteration counts, number of corrections, optimum -- and the telemetry counts exactly those scenarios (reason 3).
    """
    from oracle import oracle
    from mseetc._device import ST
    train, track = cases.train_default(), cases.track_00(16000)
    s = _solver(train, track, 40, start='profile')
    prob = cases.oracle_problem(train, track, 40)
    T = 640.0*(1.0 + 0.5*np.random.default_rng(5).random(256))
    T[0], T[1] = 804.9041795334854, 762.6780418513658
    t0, why0 = s.problem.follow_counts()
    res = s.solveBatch(T)
    t1, why1 = s.problem.follow_counts()
    assert np.all(res['status'] == 0)
    scen = np.stack([np.zeros_like(T), T, np.ones_like(T), np.ones_like(T)], axis=1)
    z, st, nfail = oracle.solve_batch(prob, scen, nthreads=0, start='profile')
    assert nfail == 0
    nsoc = res['stats'][:, ST['N_SOC']]
    assert nsoc[0] == 1 and nsoc[1] == 1 and nsoc.sum() >= 20
    assert np.array_equal(nsoc, st[:, ST['N_SOC']])
    assert t1 - t0 == why1[3] - why0[3] == int((nsoc > 0).sum())
    assert np.max(np.abs(res['iterations'] - st[:, ST['ITERS']])) <= 2
    assert np.max(np.abs(res['cost'] - st[:, ST['OBJ']])/np.abs(st[:, ST['OBJ']])) <= 1e-7
    assert np.max(np.abs(res['z'] - z)/np.maximum(1.0, np.abs(z))) <= 1e-5
    # Round 6: a handle whose launch has handed a correction over takes the first-pass kernel with the correction INSIDE the fused iteration from then on
    # (msd_kernel.hpp: SOCK; msd_api.hip: launch) -- the same batch again: nothing is handed over for that reason, the corrections are counted by the fused
    # iteration itself and agree with the oracle's, scenario for scenario
    res2 = s.solveBatch(T)
    t2, why2 = s.problem.follow_counts()
    assert np.all(res2['status'] == 0)
    assert why2[3] == why1[3], (why1, why2)
    assert np.array_equal(res2['stats'][:, ST['N_SOC']], st[:, ST['N_SOC']])
    assert np.max(np.abs(res2['iterations'] - st[:, ST['ITERS']])) <= 2
    assert np.max(np.abs(res2['cost'] - st[:, ST['OBJ']])/np.abs(st[:, ST['OBJ']])) <= 1e-7
    assert np.max(np.abs(res2['z'] - z)/np.maximum(1.0, np.abs(z))) <= 1e-5
    s.close()
    # ... on two nodes per lane as well (N = 100, config 1's geometry with the node constants in LDS): loose-ish schedules on the cropped track
    track = cases.track_00(30000)
    s = _solver(train, track, 70, start='profile')
    prob = cases.oracle_problem(train, track, 70)
    T = 1050.0*(1.0 + 0.4*np.random.default_rng(6).random(256))
    T[0] = 1140.8291957305269*(70/60)
    first = s.solveBatch(T)
    w1 = s.problem.follow_counts()[1]
    again = s.solveBatch(T)
    w2 = s.problem.follow_counts()[1]
    scen = np.stack([np.zeros_like(T), T, np.ones_like(T), np.ones_like(T)], axis=1)
    z, st, nfail = oracle.solve_batch(prob, scen, nthreads=0, start='profile')
    assert nfail == 0 and np.all(first['status'] == 0) and np.all(again['status'] == 0)
    if st[:, ST['N_SOC']].sum() > 0:
        assert w1[3] > 0 and w2[3] == w1[3]
    for r in (first, again):
        assert np.array_equal(r['stats'][:, ST['N_SOC']], st[:, ST['N_SOC']])
        assert np.max(np.abs(r['iterations'] - st[:, ST['ITERS']])) <= 2
        assert np.max(np.abs(r['cost'] - st[:, ST['OBJ']])/np.abs(st[:, ST['OBJ']])) <= 1e-7
    s.close()


def test_split_launches_hand_rare_scenarios_to_the_follow_up_kernel():
    """
    The two launches of a split solve (first pass + follow-up kernel, msd_api.hip: launch): a batch mixing ordinary running times with
    very loose ones -- whose line search breaks down on the way, so that they need the restoration phase, which only the follow-up
    kernel holds -- comes back complete: the ordinary scenarios are bit-identical to a batch without the loose ones, the loose ones
    converge through the restoration phase, and the telemetry counts exactly the scenarios that were handed over.
    """
    from mseetc._device import ST
    train, track = cases.train_default(), cases.track_00()
    s = _solver(train, track, 100, start='reference')
    T = cases.c1_times(48)
    loose = np.linspace(12000.0, 19000.0, 16)
    alone = s.solveBatch(T)
    t0, why0 = s.problem.follow_counts()
    mixed = s.solveBatch(np.concatenate([T[:24], loose, T[24:]]))
    t1, why1 = s.problem.follow_counts()
    assert np.all(mixed['status'] >= 0)
    keep = np.r_[0:24, 40:64]
    assert np.array_equal(mixed['z'][keep], alone['z']) and np.array_equal(mixed['iterations'][keep], alone['iterations'])
    nresto = mixed['stats'][24:40, ST['N_RESTO']]
    assert nresto.sum() >= 8                                      # most of the loose schedules go through at least one restoration phase
    assert t1 - t0 >= int((nresto > 0).sum())                     # ... and every one of those went through the list
    assert sum(why1[:5]) - sum(why0[:5]) == t1 - t0               # (every hand-over has its reason: tiny step, rejected trial point, line search ...)
    s.close()


def test_one_brake_kernels_vs_oracle():
    """
    The configuration of the reference's scripts (forceMinPn = 0: figure5.py:88, figure6.py:108, figure10.py:17, table3.py:18) runs on
    kernels with that structure compiled in (FULL_RG: split launches with the fused iteration, like the rolling stock of the JSON files).
    Against the oracle from both starting points on three launch geometries; the N = 300 optimum is the one that extrapolates to GPOPS-II.
    """
    train = cases.train_fig10()
    for N, crop, T in ((40, 16000, [700.0, 760.0]), (100, None, [1541.0, 1600.0, 1700.0]), (300, None, [1541.0])):
        track = cases.track_00(crop) if crop else cases.track_00()
        prob = cases.oracle_problem(train, track, N)
        for start in ('profile', 'reference'):
            s = _solver(train, track, N, start=start)
            assert not s.withPnBrake
            res = _compare(s, prob, T)
            if N == 300:
                assert abs(res['cost'][0] - 441.0838) < 2e-3
            s.close()


def test_device_resident_shrinking_horizon_loop_vs_host_loop():
    """
    BASELINE config 4 with the loop's bookkeeping on the device (csrc/msd_mpc.hip: measured states, scenario records, warm starts, moved
    arrival times and the log as kernels between the solver's launches) against the host loop of mseetc/mpc.py, 128 scenarios x 50
    re-solves with 1 % noise.  Cold starts: the two loops launch the same kernels on the same records up to the last place of the measured
    speeds (the device's square root differs from numpy's there now and then) until the first arrival time has to move (the device
    repeats such a scenario with the follow-up kernel's iteration, the host with another first-pass launch: same optimum, other rounding).  Warm starts: the same closed loop to the tolerances of
    test_config4_full_size_warm_and_cold.  Every re-solve ends with a solution in both.
    """
    from mseetc import workloads as wl
    from mseetc.mpc import shrinkingHorizon, DeviceLoop
    train, track, N = wl.config('c4')
    T = wl.c1_times(128, seed=20260615)
    for warm in (False, True):
        host = shrinkingHorizon(train, track, wl.options(N), T, numResolves=50, noise=0.01, seed=1, warmStart=warm)
        loop = DeviceLoop(train, track, wl.options(N), 50, noise=0.01, warmStart=warm)
        dev = loop.run(T, seed=1)
        again = loop.run(T, seed=1, keepZ=False)      # the loop object is reusable; same inputs, same log
        loop.close()
        assert len(host) == len(dev) == 50
        moved = np.zeros(128, dtype=bool)
        first_move = None
        for k, (h, d, a) in enumerate(zip(host, dev, again)):
            assert h['numIntervals'] == d['numIntervals'] == N - 2*k and abs(h['position'] - d['position']) < 1e-9
            assert (h['status'] < 0).sum() <= (0 if k < 48 else 4) and (d['status'] < 0).sum() <= (0 if k < 48 else 4), (k, h['status'].min(), d['status'].min())
            assert np.array_equal(d['status'], a['status']) and np.array_equal(d['t0'], a['t0']) and np.array_equal(d['cost'], a['cost']) and a['z'] is None
            if first_move is None and (h['relaxed'].any() or d['relaxed'].any()):
                first_move = k
            if not warm and first_move is None:
                # same kernels on (nearly) the same records: the last-place differences of the measured speeds grow to what two optima
                # converged to 1e-8 differ by, no further
                # (round 6: the device loop's re-solves run the first-pass kernel with the second-order correction inside the fused iteration, the host loop's
                #  launches hand such a scenario to the follow-up kernel, which solves it again from its starting point: a few scenarios per re-solve take
                #  another number of iterations to the same optimum)
                di = np.abs(h['iterations'] - d['iterations'])
                assert np.array_equal(h['status'], d['status']) and int((di > 2).sum()) <= 4 and di.max() <= 12, (k, di.max())
                assert np.array_equal(h['T'], d['T'])
                for key, tol in (('t0', 1e-7), ('v0', 1e-6), ('cost', 1e-6), ('z', 1e-4)):
                    assert np.allclose(h[key], d[key], rtol=tol, atol=tol), (k, key)
            moved |= h['relaxed'] | d['relaxed']
            same = ~moved
            assert np.allclose(h['t0'][same], d['t0'][same], rtol=1e-6, atol=1e-6), k
            assert np.allclose(h['v0'][same], d['v0'][same], rtol=1e-5), k
            assert np.allclose(h['cost'][same], d['cost'][same], rtol=1e-5 if k < 30 else 5e-3, atol=1e-5), k
            for log in (h, d):
                m = log['relaxed']
                if m.any():
                    assert np.all(log['T'][m] > T[m]) and np.all(log['T'][m] - T[m] < 0.08*T[m])
        # arrival times move late in the journey, in both loops, for (nearly) the same scenarios
        assert first_move is None or first_move >= 20
        hm = np.any([h['relaxed'] for h in host], axis=0); dm = np.any([d['relaxed'] for d in dev], axis=0)
        assert (hm != dm).sum() <= 2


def test_fused_iteration_corrects_the_inertia_itself():
    """
    Round 5: where a pivot of the stage recursion is not positive the fused iteration puts delta_w on the diagonal and runs its pass over the point
    again (W&B Algorithm IC, the schedule of the general iteration and of the oracle) instead of handing the scenario to the follow-up kernel.
    Warm-started re-solves of config 4 meet it in a few per cent of the solves: the loop's handles report inertia corrections, none of its
    scenarios goes to the follow-up kernel for that reason, and the closed loop is the cold-started one (test_config4_full_size_warm_and_cold
    holds the full comparison).
    """
    from mseetc import workloads as wl
    from mseetc.mpc import shrinkingHorizon
    from mseetc.ocp import casadiSolver
    train, track, N = wl.config('c4')
    T = wl.c1_times(128, seed=20260615)
    counts = []

    def factory(tr, tk, op):
        s = casadiSolver(tr, tk, op, restoration=False, watchdogTrigger=-1)
        close = s.close

        def closing():
            counts.append(s.problem.follow_counts())
            close()
        s.close = closing
        return s
    log = shrinkingHorizon(train, track, wl.options(N), T, numResolves=50, noise=0.01, seed=1, warmStart=True, solverFactory=factory)
    reg = sum(int(l['regularisations'].sum()) for l in log)
    by_reason = np.sum([c[1] for c in counts], axis=0)      # (no fused start, inertia / scan, tiny step, second-order correction, line search, ...)
    assert reg > 0 and by_reason[1] == 0, (reg, by_reason)
    assert all((l['status'] < 0).sum() <= (0 if k < 48 else 4) for k, l in enumerate(log))


@pytest.mark.parametrize('variant', ['rg', 'both'])
def test_short_horizons_through_the_follow_up_kernel(variant):
    """
    Horizons of up to 63 intervals (one node per lane in the first pass) whose scenarios need the follow-up kernel: loose schedules from the
    reference's starting point (inertia corrections, restoration phases) and from the profile start, N = 40 and N = 63, both rolling-stock
    structures -- against the oracle.  (Round 4: the 64 x 1 instantiation of the one-brake follow-up kernel faulted on the device; the follow-up
    kernel of these horizons is the two-nodes-per-lane one since, msd_api.hip: make_plan.  Found by tests/tools/random_sweep.py, seed 15.)
    """
    from oracle import oracle
    from mseetc._device import ST
    train = cases.train_fig10() if variant == 'rg' else cases.train_default()
    for N, crop in ((40, 16000), (63, 30000)):
        track = cases.track_00(crop)
        prob = cases.oracle_problem(train, track, N, maxIterations=800)
        T = np.array([700.0, 2500.0, 6000.0, 9000.0])*(crop/16000.0)
        for start in ('profile', 'reference'):
            s = _solver(train, track, N, start=start, maxIterations=800)
            before = s.problem.follow_counts()[0]
            res = s.solveBatch(T)
            assert np.all(res['status'] == 0), (N, start, res['status'])
            assert s.problem.follow_counts()[0] - before >= 2      # the loose ones went through the follow-up kernel
            for k, t in enumerate(T):
                ref = oracle.solve(prob, prob.scenario(float(t)), start=start)
                assert ref['stats']['STATUS'] == 0
                through_resto = res['stats'][k, ST['N_RESTO']] > 0 or ref['stats']['N_RESTO'] > 0
                if not through_resto:      # (a hundred iterations through restoration phases do not repeat to the iteration: there the optimum is compared)
                    assert abs(int(res['iterations'][k]) - int(ref['stats']['ITERS'])) <= 2, (N, start, k, res['iterations'][k], ref['stats']['ITERS'])
                assert abs(res['cost'][k] - ref['stats']['OBJ']) <= (1e-6 if through_resto else 1e-7)*max(1e-3, abs(ref['stats']['OBJ'])), (N, start, k)
            s.close()


@pytest.mark.parametrize('case', ['seed105', 'seed125', 'short_rg', 'short_both', 'n100_rg'])
def test_follow_up_kernels_are_deterministic_launch_to_launch(case, tmp_path):
    """
    The follow-up kernels (general iteration, restoration phase, second attempt) return the same bits from launch to launch -- what the reference's scripts
    assert of repeated solves (figure6.py:191-193: identical iteration counts).  Round 5 shipped a register read before its first write (Solver::evs) that no
    test could see: one-brake problems from the reference's starting point took 45 / 46 / 47 iterations in the follow-up kernel from one launch to the next
    where the oracle takes 71 (random-sweep seeds 105 and 125).  Six launches of the same running times: identical status, iteration counts, z and
    statistics; the scenarios went through the follow-up kernel; iteration counts equal the oracle's where no restoration phase is on the way.
    """
    from oracle import oracle
    from mseetc._device import ST
    if case.startswith('seed'):
        train, track, N, rng = _random_problem(int(case[4:]), tmp_path)
        v0, vN = float(rng.uniform(1, 15)), float(rng.uniform(1, 15))
        po = cases.oracle_problem(train, track, N, energyOptimal=False, losses='none')
        tmin = float(oracle.solve(po, po.scenario(3*track.length/train.velocityMax, 0.0, vN, v0), start='profile')['z'][-2])
        T = tmin*np.array([1.05, 1.1, 1.2, 1.45, 2.0])
    else:
        train = cases.train_default() if case == 'short_both' else cases.train_fig10()
        N, crop = (100, None) if case == 'n100_rg' else (50, 20000)
        track = cases.track_00(crop) if crop else cases.track_00()
        v0 = vN = 1.0
        T = np.array([1541.0, 1700.0, 4000.0, 9000.0, 14000.0])*((crop or 48531)/48531.0)
    s = _solver(train, track, N, start='reference', maxIterations=800)
    before = s.problem.follow_counts()[0]
    runs = [s.solveBatch(T, initialVelocity=v0, terminalVelocity=vN) for _ in range(6)]
    handed = s.problem.follow_counts()[0] - before
    s.close()
    first = runs[0]
    for r in runs[1:]:
        assert np.array_equal(r['status'], first['status']) and np.array_equal(r['iterations'], first['iterations']), (case, [list(x['iterations']) for x in runs])
        assert np.array_equal(r['z'], first['z'])
        keep = [k for k in range(ST['COUNT']) if k not in (ST['CYC_TOTAL'], ST['CYC_KKT'])]      # (time stamps)
        assert np.array_equal(r['stats'][:, keep], first['stats'][:, keep])
    assert np.all(first['status'] >= 0), first['status']
    if case != 'n100_rg':
        assert handed >= 6      # (at least one scenario per launch took the follow-up kernel's path)
    prob = cases.oracle_problem(train, track, N, maxIterations=800)
    for k, t in enumerate(T):
        ref = oracle.solve(prob, prob.scenario(float(t), 0.0, vN, v0), start='reference')
        assert ref['stats']['STATUS'] >= 0
        # (iteration for iteration where the solve is an ordinary one; a loose schedule that crawls for a hundred iterations with steps of 1e-4 or goes through
        #  restoration phases does not repeat to the iteration between two implementations: there the optimum is compared)
        if first['stats'][k, ST['N_RESTO']] == 0 and ref['stats']['N_RESTO'] == 0 and ref['stats']['ITERS'] <= 100:
            assert abs(int(first['iterations'][k]) - int(ref['stats']['ITERS'])) <= 2, (case, k, first['iterations'][k], ref['stats']['ITERS'])
        assert abs(first['cost'][k] - ref['stats']['OBJ']) <= 1e-6*max(1e-3, abs(ref['stats']['OBJ'])), (case, k)


def _described(solver):
    "the fields of msd_plan_describe's line for the solver's description"
    import ctypes
    from mseetc import _device
    buf = ctypes.create_string_buffer(4096)
    _device._check(_device.lib().msd_plan_describe(ctypes.byref(solver._desc), buf, len(buf)))
    return dict(f.split('=', 1) for f in buf.value.decode().split())


def test_handle_runs_the_described_plan():
    """
    A handle runs the plan msd_plan_describe reports for its description (tests/test_abi.py pins those lines against tests/golden/plan_table.json on
    the CPU): geometry() against NT SPT of the line, and one solve, at the smallest shapes on each side of a code path of the plan's selection --
    both brakes at N = 63 (64 x 1 first pass, the 64 x 2 follow-up kernel: from the reference's starting point, through the least-squares first
    pass) and N = 64, the dynamic loss model at N = 100 (resident first pass, streamed follow-up), collocation at N = 40, the streamed kernel at
    N = 700.  Then a reconfiguration the selection rejects: MSD_E_UNSUPPORTED, the handle holds no problem until a valid one, which solves.
    """
    from mseetc import _device
    from mseetc.ocp import casadiSolver
    from mseetc.train import Train
    from mseetc.efficiency import totalLossesFunction
    both = cases.train_fig10(); both.forceMinPn = cases.train_default().forceMinPn
    dyn = Train(config={'id': 'NL_Intercity_VIRM6'}); dyn.forceMinPn = 0
    dyn.powerLosses = totalLossesFunction(dyn, auxiliaries=27000, etaGear=0.96)      # (test_dynamic_loss_model_vs_oracle)
    rk = dict(numSteps=1, numApproxSteps=1)
    shapes = [('both_63', both, cases.track_00(30000), dict(numIntervals=63, maxIterations=800, integrationOptions=rk), 'reference', [1300.0, 16875.0], {}, (64, 1, 64, 2)),
              ('both_64', both, cases.track_00(30000), dict(numIntervals=64, integrationOptions=rk), 'profile', [1300.0], {}, (64, 2, 64, 2)),
              ('dynamic_100', dyn, cases.track_00(8500), dict(numIntervals=100, integrationOptions=rk), 'reference', [272.4726*1.2], dict(terminalVelocity=100/3.6, initialVelocity=1), None),
              ('collocation_40', cases.train_default(), cases.track_00(20000), dict(numIntervals=40, integrationMethod='IRK', integrationOptions=dict(order=2, **rk)), 'profile', [760.0], {}, None),
              ('streamed_700', cases.train_default(), cases.track_00(), dict(numIntervals=700, integrationOptions=rk), 'profile', [1541.0], {}, (512, 2, 512, 2))]
    for name, train, track, opts, start, T, kw, want in shapes:
        s = casadiSolver(train, track, dict(dict(maxIterations=500), **opts), startingPoint=start)
        line = _described(s)
        print(name, line)
        assert '?' not in line.values()
        assert s.problem.geometry() == (int(line['NT']), int(line['SPT'])), name
        assert want is None or tuple(int(line[k]) for k in ('NT', 'SPT', 'NT2', 'SPT2')) == want, name
        assert (line['stream'] == '1') == (name == 'streamed_700') and (not name.startswith('both') or line['kernel_lsq'] != '-')
        before = s.problem.follow_counts()[0]
        res = s.solveBatch(T, **kw)
        print(name, res['status'], res['iterations'], s.problem.follow_counts())
        assert np.all(res['status'] == 0), (name, res['status'])
        if name == 'both_63':
            assert s.problem.follow_counts()[0] - before >= 1      # the loose schedule went through the 64 x 2 follow-up kernel
        if name == 'dynamic_100':
            # a description the selection rejects (the dynamic loss model ends at 1023 intervals): the handle holds no problem until the next valid one
            long = casadiSolver(train, track, dict(numIntervals=1100, maxIterations=500, integrationOptions=rk), startingPoint=start)
            with pytest.raises(_device.DeviceError, match='msd error -3: numIntervals = 1100 exceeds the 1023 intervals'):
                s.problem.reconfigure(long._desc)
            with pytest.raises(ValueError, match=r'the handle holds no problem: its last \(re\)configuration failed'):
                s.solveBatch(T, **kw)
            # ... and the same after a description the argument checks reject
            s.problem.reconfigure(s._desc)
            s._desc.max_iterations = 0
            with pytest.raises(ValueError, match='Maximum number of iterations'):
                s.problem.reconfigure(s._desc)
            s._desc.max_iterations = 500
            with pytest.raises(ValueError, match=r'the handle holds no problem: its last \(re\)configuration failed'):
                s.solveBatch(T, **kw)
            s.problem.reconfigure(s._desc)
            again = s.solveBatch(T, **kw)
            assert np.array_equal(again['status'], res['status']) and np.array_equal(again['z'], res['z'])
        s.close()
