"""
The energy account of the shrinking-horizon loop, host side (no device): include/mseetc_mpc.h: msd_mpc_energy as mseetc/mpc.py states it -- plantEnergy (the numpy
statement the device's mpc_energy is held to) against the reference's accounting (utils.py:243-257, :291: postProcessDataFrame), against the objective the solver
minimises, against scipy for the loss integral of a loss table, against plantAdvance for the trajectory; a plant that stalls; the host loop with the account; what
is refused; the two entry points of the C ABI.  The device side: tests/test_mpc_energy_gpu.py (which takes its inputs from here).

Shapes and the six scenarios: tests/test_mpc_rolling_stock.py (shape6, stock, OracleStock).  The table shape: the figure-5 train (cases.train_fig5() with
totalLossesFunction(train, auxiliaries=27000, etaGear=0.96)) on track 00 cropped to 8.5 km, N = 30, K = 3, stride 2, terminal velocity 100 km/h, six arrival times
TABLE_TIMES = 272.4726 s x (1.10, 1.13, 1.16, 1.19, 1.25, 1.33): clear of the kink bands 1.21 ... 1.22 and 1.28 ... 1.29 of DESIGN.md section 8.  Every re-solve of
every scenario of every input of the device tests converges on the oracle at these times (test_the_inputs_converge_on_the_oracle); no time had to be moved.

Measured on the oracle (printed by the tests):
  objective: cost - smoothing term against traction + regenerated + losses of plantEnergy, relative to the cost, maximum over the six scenarios of crop20_N40 and
  full_N66_rg: 2.54e-7 (SLACK_MEASURED; 2.07e-7 ... 2.54e-7 on crop20_N40, 2.06e-7 ... 2.26e-7 on full_N66_rg).  The objective prices LESS than the account on every
  one of them: the slack variables end below the loss rows, not above them, by about 1e-8 N/kg per row -- what an interior-point method that relaxes the rows' bounds
  by 1e-8 leaves: over 40 intervals of 500 m and 414 t that is 2.3e-5 kWh of 111 kWh (not traced further than that).  Asserted: 10 x the maximum.
  loss integral against DOP853, two intervals of the table shape from node 1, relative: 7.88e-8 with 8 steps, 4.10e-9 with 16 (19.2 x) with the plant; 8.31e-8 and
  3.64e-9 (22.8 x) without one.
  final leg with a plant on the static shapes: the plans brake to the minimum velocity at the platform, and a plant that is not the plan's own one-step integrator
  falls below it in the last interval: the stall rule ends the leg in front of that interval (33 of 34 intervals on crop20_N40 for five of the six scenarios),
  `complete` is False there and the arrival is the state in front of the last interval.
"""

import re

import numpy as np
import pytest

import cases

from test_mpc_speed_restrictions import _opts, host_loop
from test_mpc_rolling_stock import B, PLANT_STEPS, stock, shape6, OracleStock, own_train, plant_rows, make

STRIDE = 2
SLACK_MEASURED = 2.54e-7      # (the module's docstring)
TABLE_TIMES = 272.4726*np.array([1.10, 1.13, 1.16, 1.19, 1.25, 1.33])
TABLE_N, TABLE_K, TABLE_VN = 30, 3, 100/3.6
TABLE_PLANT = dict(plantMass=1.05, plantR2=1.10)      # of the train's: the plant of the table shape


def table_shape():
    "(train, track, N, K, T, keywords of the loop) of the table shape"
    from mseetc.efficiency import totalLossesFunction
    train = cases.train_fig5()
    train.powerLosses = totalLossesFunction(train, auxiliaries=27000, etaGear=0.96)
    return train, cases.track_00(crop=8500), TABLE_N, TABLE_K, TABLE_TIMES.copy(), dict(terminalVelocity=TABLE_VN)


def table_plant(train):
    return dict(plantMass=train.mass*TABLE_PLANT['plantMass'], plantR2=train.r2*TABLE_PLANT['plantR2'], plantSteps=PLANT_STEPS)


class OracleTable(OracleStock):
    "OracleStock for a train with a loss table: the oracle's problem with loss kind 2 on the train's own table"

    def problem(self, mass, r0, r1, r2):
        from oracle import oracle
        from mseetc.track import computeDiscretizationPoints
        key = (float(mass), float(r0), float(r1), float(r2))
        tr = own_train(self.train, *key)
        oracle.set_loss_table(self.train.lossesCallable().parameters(tr.mass*tr.rho))      # (module state of the oracle: the last problem packed owns it)
        if key not in self._own:
            opts = dict(numIntervals=self._N, maxIterations=self._maxit, energyOptimal=True, minimumVelocity=1, numSteps=self._io['numSteps'],
                        numApproxSteps=self._io['numApproxSteps'], watchdogTrigger=-1)
            self._own[key] = oracle.pack_problem(tr, computeDiscretizationPoints(self.track, self._N), opts, 2, 0.0, 0.0, self.track.length)
        return self._own[key]


def make_table(a, b, c):
    return OracleTable(a, b, c)


def inputs(name):
    "(train, track, N, K, T, loop keywords, solver factory, [keywords of the run without a plant, with a plant]) of a shape of the device tests"
    if name == 'table_N30':
        train, track, N, K, T, kw = table_shape()
        return train, track, N, K, T, kw, make_table, [dict(), table_plant(train)]
    train, track, N, K, T = shape6(name)
    model, plant = stock(train)
    return train, track, N, K, T, dict(), make, [dict(), dict(model, **plant)]


SHAPES = ['crop20_N40', 'full_N66_rg', 'table_N30']
NOISE, SEED = 0.01, 3


def rows_of(train, kw):
    "(plant rows or None, total mass of the models (B,), model rows (B, 3)) of the keywords of a run"
    from mseetc.mpc import _rollingStock
    model, plant = _rollingStock(train, B, kw.get('mass'), kw.get('r0'), kw.get('r1'), kw.get('r2'), kw.get('plantMass'), None, None, kw.get('plantR2'), kw.get('plantSteps', PLANT_STEPS))
    m = model if model is not None else dict(mass=np.full(B, train.mass), r0=np.full(B, train.r0), r1=np.full(B, train.r1), r2=np.full(B, train.r2))
    M = m['mass']*train.rho
    return plant, M, np.stack([m['r0']/M, m['r1']/M, m['r2']/M], axis=1)


def statement(loop, log, k, train, kw, eta=None, steps=PLANT_STEPS, scen=None):
    "plantEnergy on the logged solutions of re-solve k from its logged initial state (`scen`: its scenario records, where restrictions clip them): the leg behind it (the whole plan behind the last re-solve)"
    from mseetc.mpc import plantEnergy
    r = log[k]
    K = len(log)
    plant, M, mrows = rows_of(train, kw)
    if scen is None:
        scen = loop.solvers[k]._scenarios(r['T'], r['t0'], loop.terminalVelocity, r['v0'])
    n = STRIDE if k < K - 1 else r['numIntervals']
    return plantEnergy(loop.solvers[k], r['z'], scen[:, 0], scen[:, 2], plant, steps, n, M, eta=eta, modelRows=mrows)


@pytest.fixture(scope='module')
def oracle_plans():
    "one oracle solve per scenario on the first grid of the two static shapes (the train of the problem) and of the table shape"
    out = {}
    for name in SHAPES:
        train, track, N, K, T, kw, factory, _ = inputs(name)
        solver = factory(train, track, _opts(N))
        res = solver.solveBatch(T, **kw)
        assert np.all(res['status'] == 0), (name, res['status'])
        out[name] = (train, solver, res)
    return out


@pytest.mark.parametrize('name', ['crop20_N40', 'full_N66_rg'])
def test_account_is_the_references_accounting(oracle_plans, name):
    """
    Static efficiencies, no plant, n = N: traction + regenerated + losses of plantEnergy is the sum of postProcessDataFrame's 'Energy [kWh]' (utils.py:243-257, :291,
    the formula this package restates) of the same solution, and the pneumatic brake's energy is its 'Energy (pnb) [kWh]' with the other sign.  1e-12 relative: both
    are sums of at most 130 products and the speed cancels.
    """
    from mseetc.mpc import plantEnergy
    from mseetc.utils import postProcessDataFrame
    train, solver, res = oracle_plans[name]
    N = solver._N
    M = train.mass*train.rho
    acc = plantEnergy(solver, res['z'], res['scenarios'][:, 0], res['scenarios'][:, 2], None, PLANT_STEPS, N, M)
    assert np.all(acc['intervals'] == N) and not acc['stalled'].any()
    stp = 4 + int(solver.withPnBrake)
    assert np.array_equal(acc['t'], res['z'][:, stp*N]) and np.array_equal(acc['v'], np.sqrt(res['z'][:, stp*N + 1]))
    for s in range(B):
        df = postProcessDataFrame(solver._front.unpack(res['z'][s]), solver.points, train, CVODES=False)
        want = df['Energy [kWh]'].sum()
        got = acc['traction'][s] + acc['regenerated'][s] + acc['losses'][s]
        print('%s scenario %d: Energy [kWh] %.12f, account %.12f (relative %.3e)' % (name, s, want, got, abs(got - want)/abs(want)))
        assert abs(got - want) <= 1e-12*abs(want)
        assert abs(acc['losses'][s] - df['Losses [kWh]'].sum()) <= 1e-12*abs(df['Losses [kWh]'].sum())
        assert abs(acc['pnBrake'][s] + df['Energy (pnb) [kWh]'].sum()) <= 1e-12*max(abs(acc['pnBrake'][s]), 1e-300)
        assert acc['traction'][s] > 0 and acc['regenerated'][s] <= 0 and acc['losses'][s] > 0


def test_account_against_the_objective(oracle_plans):
    """
    On the same solutions: the oracle's cost without its smoothing term 1e-3 sum (dFel)^2 (ocp.py:223; in kWh through the objective's scaling) against `total`.  The
    two differ by what the interior-point method leaves between the slack variables and the loss rows; measured on the oracle: the module's docstring; asserted:
    10 x the measured maximum.
    """
    from mseetc.mpc import plantEnergy
    from oracle.oracle import DP
    worst = 0.0
    for name in ('crop20_N40', 'full_N66_rg'):
        train, solver, res = oracle_plans[name]
        N = solver._N
        M = train.mass*train.rho
        acc = plantEnergy(solver, res['z'], res['scenarios'][:, 0], res['scenarios'][:, 2], None, PLANT_STEPS, N, M)
        stp = 4 + int(solver.withPnBrake)
        fel = res['z'][:, 0:stp*N:stp]
        smooth = 1e-3*np.sum(np.diff(fel, axis=1)**2, axis=1)/solver._prob.dp[DP['OBJ_DEN']]
        priced = res['cost'] - smooth
        total = acc['traction'] + acc['regenerated'] + acc['losses']
        d = np.abs(priced - total)/np.abs(res['cost'])
        print('%s: cost %s  smoothing term %s  total %s  relative slack %s' % (name, res['cost'].tolist(), smooth.tolist(), total.tolist(), d.tolist()))
        worst = max(worst, d.max())
    print('maximum relative distance between the priced and the accounted energy: %.3e' % worst)
    assert worst <= 10*SLACK_MEASURED


def _exact_losses(solver, rows, scale, z, t0, b0, n, M, first, restart):
    "the augmented space-domain ODE d t/d s = 1/sqrt(b), d b/d s = 2 (w - r(b) - G), d E/d s = L(F, sqrt(b))/sqrt(b) through scipy's DOP853, interval by interval"
    from scipy.integrate import solve_ivp
    prob = solver._prob
    g, rho = solver.train.g, solver.train.rho
    fun = solver.train.lossesCallable()
    stp = 4 + int(solver.withPnBrake)
    E = np.zeros(B)
    for s in range(B):
        y = np.array([t0[s], b0[s], 0.0])
        for i in range(n):
            c = abs(prob.curv[first + i])
            cr = g*0.5*c/(1 - 30*c) if c <= 1/300 else g*0.65*c/(1 - 55*c)
            G = g*prob.grad[first + i]/rho + cr/rho
            fel = z[s, stp*i]
            w = (fel + (z[s, stp*i + 1] if stp == 5 else 0.0))*scale[s]
            F = fel*M
            if restart:
                y[1] = z[s, stp*i + stp - 1]
            f = lambda x, y: [1/np.sqrt(y[1]), 2*(w - (rows[s, 0] + rows[s, 1]*np.sqrt(y[1]) + rows[s, 2]*y[1]) - G), fun(F, np.sqrt(y[1]))/np.sqrt(y[1])]
            y = solve_ivp(f, (0.0, prob.ds[first + i]), y, method='DOP853', rtol=1e-12, atol=1e-14).y[:, -1]
        E[s] = y[2]*(1e-6/3.6)
    return E


@pytest.mark.parametrize('withPlant', [True, False])
def test_table_quadrature_vs_scipy_is_of_fourth_order(oracle_plans, withPlant):
    """
    The loss integral of plantEnergy with 8 and with 16 steps per interval against DOP853 (rtol 1e-12) of the same augmented space-domain equations, two intervals of
    the table shape from node 1 of the plans (a running train: tests/test_mpc_rolling_stock.py: test_plant_advance_vs_scipy_is_of_fourth_order on why not from the
    platform), with the plant of the table shape (the walk of plantAdvance) and without one (every interval from the plan's own b_i under the model).  Fourth order
    divides the error by 16; asserted: by 8 at least.  Measured, maximum over the six scenarios, relative: printed.
    """
    from mseetc.mpc import plantEnergy
    train, solver, res = oracle_plans['table_N30']
    M = train.mass*train.rho
    plant, _, mrows = rows_of(train, table_plant(train) if withPlant else {})
    stp = 4 + int(solver.withPnBrake)
    first, n = 1, 2
    z = res['z'][:, stp*first:]
    t0, b0 = res['z'][:, stp*first + stp - 2], res['z'][:, stp*first + stp - 1]

    class Shifted():
        points, withPnBrake, train, velocityMin = solver.points.iloc[first:], solver.withPnBrake, solver.train, solver.velocityMin
    rows, scale = (plant, plant[:, 3]) if withPlant else (mrows, np.ones(B))
    exact = _exact_losses(solver, rows, scale, z, t0, b0, n, M, first, restart=not withPlant)
    err = {}
    for steps in (8, 16):
        acc = plantEnergy(Shifted, z, t0, b0, plant, steps, n, M, modelRows=mrows)
        assert np.all(acc['intervals'] == n) and np.all(acc['losses'] > 0)
        err[steps] = np.max(np.abs(acc['losses'] - exact)/exact)
    print('loss integral of two intervals (%s), relative error: %.3e with 8 steps, %.3e with 16 (%.1f x)' % ('plant' if withPlant else 'plan', err[8], err[16], err[8]/err[16]))
    assert err[16] <= err[8]/8


@pytest.mark.parametrize('name', SHAPES)
def test_the_trajectory_is_plant_advances(oracle_plans, name):
    "with plant rows, (t, v, stalled) of plantEnergy at n = stride are plantAdvance's, bit for bit; so are they at n = 5, and the account of a longer leg extends that of a shorter one"
    from mseetc.mpc import plantEnergy, plantAdvance
    train, solver, res = oracle_plans[name]
    plant, M, mrows = rows_of(train, inputs(name)[7][1])
    t0, v0sq = res['scenarios'][:, 0], res['scenarios'][:, 2]
    for n in (STRIDE, 5):
        acc = plantEnergy(solver, res['z'], t0, v0sq, plant, PLANT_STEPS, n, M, modelRows=mrows)
        t, v, stalled = plantAdvance(solver, res['z'], t0, v0sq, plant, PLANT_STEPS, n)
        assert np.array_equal(acc['t'], t) and np.array_equal(acc['v'], v) and np.array_equal(acc['stalled'], stalled) and not stalled.any()
        assert np.all(acc['intervals'] == n)
    short = plantEnergy(solver, res['z'], t0, v0sq, plant, PLANT_STEPS, STRIDE, M, modelRows=mrows)
    assert np.all(acc['traction'] >= short['traction']) and np.all(acc['losses'] > short['losses'])


def test_a_stall_ends_the_leg():
    """
    The stalling plant of tests/test_mpc_rolling_stock.py: test_a_plant_that_stalls (scenario 2, an r0 the planned force cannot move) stalls in its first interval from
    wherever it starts: that input is in test_a_plant_that_stalls_ends_its_account.  Here its r0 is 0.3 times the maximum tractive effort and it starts as a running
    train (node 4 of the plans of crop20_N40, 23.6 m/s) over ten intervals: it decelerates for four intervals and falls below the minimum velocity in the fifth.  The
    account counts the intervals in front of the one that stalled it and none behind it: it is, bit for bit, the account of the leg of that many intervals, which
    does not stall.
    """
    from mseetc.mpc import plantEnergy, plantAdvance, _rollingStock
    train, track, N, K, T = shape6('crop20_N40')
    solver = OracleStock(train, track, _opts(N))
    res = solver.solveBatch(T)
    assert np.all(res['status'] == 0)
    rows = _rollingStock(train, B, None, None, None, None, train.mass, np.where(np.arange(B) == 2, 0.3*train.forceMax, train.r0), None, None, PLANT_STEPS)[1]
    M = train.mass*train.rho
    stp, first, n = 5, 4, 10
    z = res['z'][:, stp*first:]
    t0, b0 = res['z'][:, stp*first + stp - 2], res['z'][:, stp*first + stp - 1]

    class Shifted():
        points, withPnBrake, train, velocityMin = solver.points.iloc[first:], solver.withPnBrake, solver.train, solver.velocityMin
    acc = plantEnergy(Shifted, z, t0, b0, rows, PLANT_STEPS, n, M)
    t, v, stalled = plantAdvance(Shifted, z, t0, b0, rows, PLANT_STEPS, n)
    assert acc['stalled'].tolist() == [False, False, True, False, False, False] == stalled.tolist()
    assert np.array_equal(acc['t'], t) and np.array_equal(acc['v'], v)
    m = int(acc['intervals'][2])
    print('the plant of scenario 2 stalls in interval %d of the leg, at %.3f m/s' % (m, v[2]))
    assert m == 4 and np.all(np.delete(acc['intervals'], 2) == n)
    short = plantEnergy(Shifted, z, t0, b0, rows, PLANT_STEPS, m, M)
    assert not short['stalled'].any() and short['intervals'][2] == m
    for key in ('traction', 'regenerated', 'pnBrake', 'losses', 't', 'v'):
        assert short[key][2] == acc[key][2], key
    assert acc['traction'][2] > 0


@pytest.fixture(scope='module')
def host_runs():
    "the host loop on the oracle stand-in, crop20_N40, 1 % noise: model rows and plants -- without the account, with it, with plant efficiencies of their own; and the stalling plant"
    from mseetc.mpc import shrinkingHorizon
    train, track, N, K, T = shape6('crop20_N40')
    model, plant = stock(train)
    eta = dict(plantEtaTraction=np.linspace(0.80, 0.90, B), plantEtaRgBrake=0.7)
    run = lambda **kw: shrinkingHorizon(train, track, _opts(N), T, numResolves=K, noise=NOISE, seed=SEED, solverFactory=make, **kw)
    stall = dict(plantMass=train.mass, plantR0=np.where(np.arange(B) == 2, 1.2*train.forceMax, train.r0))
    return dict(off=run(**model, **plant), on=run(**model, **plant, energyAccount=True), eta=run(**model, **plant, **eta), plain=run(energyAccount=True),
                stall=run(initialTime=5.0, energyAccount=True, **stall), stall_off=run(initialTime=5.0, **stall)), train, track, N, K, T, dict(model, **plant), eta


def test_host_loop_keeps_the_account(host_runs):
    """
    shrinkingHorizon(energyAccount=True) on the oracle stand-in: the account changes nothing else in the log; every leg's record is plantEnergy on the logged solutions
    from the logged initial state (the same function: bit for bit), `stride` intervals per leg and the whole plan behind the last re-solve; closedLoopEnergy sums the
    legs.  With plantEta* the losses follow the plants' efficiencies and nothing else moves: the plans are bit-equal to the run without them.
    """
    from mseetc.mpc import closedLoopEnergy
    runs, train, track, N, K, T, kw, eta = host_runs
    loop = host_loop(train, track, N, K)
    etas = np.stack([eta['plantEtaTraction'], np.full(B, eta['plantEtaRgBrake'])], axis=1)
    for name, e in (('on', None), ('eta', etas), ('plain', None)):
        log = runs[name]
        assert len(log) == K
        total = {key: np.zeros(B) for key in ('traction', 'regenerated', 'pnBrake', 'losses')}
        for k, r in enumerate(log):
            assert np.all(r['status'] == 0)
            want = statement(loop, log, k, train, kw if name != 'plain' else {}, eta=e)
            for key, logged in (('traction', 'energyTraction'), ('regenerated', 'energyRegenerated'), ('pnBrake', 'energyPnBrake'), ('losses', 'energyLosses')):
                assert np.array_equal(r[logged], want[key]), (name, k, key)
                total[key] += r[logged]
            full = STRIDE if k < K - 1 else N - STRIDE*k
            if name == 'plain' or k < K - 1:
                assert np.array_equal(r['legIntervals'], np.full(B, full))
            else:
                # the plans brake to the minimum velocity at the platform (terminal velocity 1 m/s = minimumVelocity): a plant that is not the plan's own one-step
                # integrator falls below it in the last interval, and the stall rule ends its leg in front of that interval
                assert np.all((r['legIntervals'] == full) | (r['legIntervals'] == full - 1)) and np.array_equal(r['legIntervals'], want['intervals'])
            assert ('tArrival' in r) == (k == K - 1)
            if name != 'plain':
                for key in ('t0', 'v0', 'T', 'status', 'iterations', 'cost', 'z'):
                    assert np.array_equal(r[key], runs['off'][k][key]), (name, k, key)
                if k < K - 1:
                    assert np.array_equal(r['tPlant'], runs['off'][k]['tPlant']) and np.array_equal(r['vPlant'], runs['off'][k]['vPlant'])
        assert np.array_equal(log[-1]['tArrival'], want['t']) and np.array_equal(log[-1]['vArrival'], want['v'])
        out = closedLoopEnergy(log)
        for key in total:
            assert np.array_equal(out[key], total[key])
        assert np.array_equal(out['total'], total['traction'] + total['regenerated'] + total['losses'])
        assert np.array_equal(out['complete'], log[-1]['legIntervals'] == N - STRIDE*(K - 1)) and (name != 'plain' or out['complete'].all())
        assert np.array_equal(out['arrivalTime'], log[-1]['tArrival']) and np.array_equal(out['arrivalVelocity'], log[-1]['vArrival'])
        print('%s: closed-loop energy %s kWh, arrival %s s at %s m/s (asked for %s)' % (name, out['total'].tolist(), out['arrivalTime'].tolist(), out['arrivalVelocity'].tolist(), T.tolist()))
    assert 'energyTraction' not in runs['off'][0]
    with pytest.raises(ValueError):
        closedLoopEnergy(runs['off'])
    # the plants' own efficiencies: the losses are ct, cr of `etas` on the same forces; nothing else moves
    a, b = closedLoopEnergy(runs['on']), closedLoopEnergy(runs['eta'])
    assert np.array_equal(a['traction'], b['traction']) and np.array_equal(a['regenerated'], b['regenerated']) and np.array_equal(a['arrivalTime'], b['arrivalTime'])
    ct, cr = (1 - etas[:, 0])/etas[:, 0], 1 - etas[:, 1]
    assert np.allclose(b['losses'], ct*b['traction'] - cr*b['regenerated'], rtol=1e-12, atol=0)
    assert np.all(b['losses'] != a['losses'])
    # without a plant the arrival is the last plan's terminal node, read
    last = runs['plain'][-1]
    assert np.array_equal(last['tArrival'], last['z'][:, -2]) and np.array_equal(last['vArrival'], np.sqrt(last['z'][:, -1]))


def test_a_plant_that_stalls_ends_its_account(host_runs):
    "the stalling plant of tests/test_mpc_rolling_stock.py in the loop: it stalls in the first interval of the first leg -- every leg of it is zero with legIntervals 0, `complete` is False; the others are complete"
    from mseetc.mpc import closedLoopEnergy
    runs, train, track, N, K, T, _, _ = host_runs
    log = runs['stall']
    for k, r in enumerate(log):
        assert r['legIntervals'][2] == 0
        assert all(r[key][2] == 0 for key in ('energyTraction', 'energyRegenerated', 'energyPnBrake', 'energyLosses'))
        others = np.delete(r['legIntervals'], 2)
        assert np.all(others == STRIDE) if k < K - 1 else np.all(others >= N - STRIDE*k - 1)      # (the last interval of the final leg: test_host_loop_keeps_the_account)
        for key in ('t0', 'v0', 'T', 'status', 'cost', 'z'):
            assert np.array_equal(r[key], runs['stall_off'][k][key]), (k, key)
    assert log[0]['stalled'][2]
    out = closedLoopEnergy(log)
    assert not out['complete'][2]
    assert out['total'][2] == 0 and out['arrivalTime'][2] == 0 and np.all(np.delete(out['total'], 2) > 0)


def test_what_is_refused():
    from mseetc.mpc import DeviceLoop, shrinkingHorizon, plantEnergy
    train, track, N, K, T = shape6('crop20_N40')
    loop = DeviceLoop(train, track, _opts(N), K, deferDevice=True)
    bad = dict(zero=dict(plantEtaTraction=0.0), above_one=dict(plantEtaRgBrake=1.0 + 1e-12), negative=dict(plantEtaTraction=-0.5), nan=dict(plantEtaRgBrake=np.nan),
               inf=dict(plantEtaTraction=np.inf), one_bad=dict(plantEtaTraction=[0.8, 0.8, 0.0, 0.8, 0.8, 0.8]), wrong_length=dict(plantEtaTraction=[0.8]*4),
               two_dimensional=dict(plantEtaRgBrake=np.full((B, 1), 0.8)), no_steps=dict(energyAccount=True, plantSteps=0), too_many_steps=dict(energyAccount=True, plantSteps=65),
               half_a_step=dict(plantEtaTraction=0.8, plantSteps=2.5))

    def never(*a):
        class Front(OracleStock):
            def solveBatch(self, *a, **kw):
                raise AssertionError("solved")
        return Front(*a)
    for name, kw in bad.items():
        with pytest.raises(ValueError):
            loop.run(T, **kw)      # (raised in front of any device call: the loop has no device side)
        with pytest.raises(ValueError):
            shrinkingHorizon(train, track, _opts(N), T, numResolves=K, solverFactory=never, **kw)
    assert loop._loop is None
    solver = OracleStock(train, track, _opts(N))
    z = np.zeros((B, 5*N + 2))
    M = train.mass*train.rho
    for kw in (dict(steps=0), dict(steps=65), dict(n=N + 1), dict(n=-1), dict(totalMass=0.0), dict(totalMass=np.nan), dict(eta=np.full((B, 2), 1.5)), dict(eta=np.full((B, 3), 0.8)),
               dict(z=np.zeros((B, 5*N))), dict(eta=np.full((B, 2), 0.0))):
        args = dict(dict(z=z, steps=PLANT_STEPS, n=STRIDE, totalMass=M, eta=None), **kw)
        with pytest.raises(ValueError):
            plantEnergy(solver, args['z'], 0.0, 1.0, None, args['steps'], args['n'], args['totalMass'], eta=args['eta'])
    # an efficiency of exactly 1 is allowed: no losses on that side
    from mseetc.mpc import _energyAccount
    assert _energyAccount(train, B, False, None, None) == (False, None) and _energyAccount(train, B, True, None, None) == (True, None)
    on, eta = _energyAccount(train, B, False, 1.0, None)
    assert on and np.all(eta[:, 0] == 1.0) and np.all(eta[:, 1] == train.etaRgBrake)


def test_entry_points_are_declared_and_refuse_a_null_handle():
    import ctypes
    import __graft_entry__ as g
    from mseetc import _device
    header = (g.ROOT / 'include' / 'mseetc_mpc.h').read_text()
    assert re.search(r'\bint\s+msd_mpc_energy\s*\(\s*msd_mpc_handle\s+\w+,\s*int\s+nscen,\s*double\s+total_mass,\s*const\s+double\s*\*\s*eta\s*(/\*.*?\*/)?\s*,\s*int\s+steps\s*\)', header)
    assert re.search(r'\bint\s+msd_mpc_energy_records\s*\(\s*msd_mpc_handle\s+\w+,\s*double\s*\*\s*records\s*(/\*.*?\*/)?\s*\)', header)
    assert re.search(r'MSD_MPC_EN_TRACTION\s*=\s*0,\s*MSD_MPC_EN_REGENERATED,\s*MSD_MPC_EN_PNBRAKE,\s*MSD_MPC_EN_LOSSES,', header)
    assert re.search(r'MSD_MPC_EN_T,\s*MSD_MPC_EN_V,.*\n\s*MSD_MPC_EN_INTERVALS,.*\n\s*MSD_MPC_EN_COUNT', header)
    assert _device.MPC_EN == dict(TRACTION=0, REGENERATED=1, PNBRAKE=2, LOSSES=3, T=4, V=5, INTERVALS=6, COUNT=7)
    L = ctypes.CDLL(str(g.build()))
    L.msd_last_error.restype = ctypes.c_char_p
    L.msd_mpc_energy.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_void_p, ctypes.c_int]
    assert L.msd_mpc_energy(None, 0, 1.0, None, 8) == -1 and b'handle' in L.msd_last_error()
    assert L.msd_mpc_energy(None, 6, 1.0, None, 8) == -1
    assert L.msd_mpc_energy_records(None, None) == -1


@pytest.mark.parametrize('name', SHAPES)
def test_the_inputs_converge_on_the_oracle(name):
    """
    Every re-solve of every scenario of every input of tests/test_mpc_energy_gpu.py ends with status 0 on the oracle, is not relaxed and does not stall: the three
    shapes with 1 % noise (seed 3), without a plant and with one, and crop20_N40 under the restrictions of its shape as well.  No scenario is left out.
    """
    from mseetc.mpc import shrinkingHorizon, closedLoopEnergy
    from test_mpc_speed_restrictions import shape
    train, track, N, K, T, loopkw, factory, runs = inputs(name)
    assert len(T) == B
    if name == 'crop20_N40':
        runs = runs + [dict(runs[1], speedRestrictions=shape(name)[5][:B])]
    for kw in runs:
        log = shrinkingHorizon(train, track, _opts(N), T, numResolves=K, noise=NOISE, seed=SEED, solverFactory=factory, energyAccount=True, **loopkw, **kw)
        assert len(log) == K
        for k, r in enumerate(log):
            assert np.all(r['status'] == 0) and not r['relaxed'].any(), (name, sorted(kw), k, r['status'])
            assert 'stalled' not in r or not r['stalled'].any()
        out = closedLoopEnergy(log)
        # (with a plant the plans of the static shapes, which brake to the minimum velocity, may lose the last interval of the final leg to the stall rule)
        assert np.all(log[-1]['legIntervals'] >= N - STRIDE*(K - 1) - 1) and all(np.all(r['legIntervals'] == STRIDE) for r in log[:-1])
        assert out['complete'].all() or ('plantMass' in kw and name != 'table_N30')
        print('%s %s: closed-loop energy %s kWh, complete %s' % (name, sorted(kw), out['total'].tolist(), out['complete'].tolist()))
