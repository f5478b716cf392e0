"""
Rolling stock of their own and a plant per scenario inside the device-resident shrinking-horizon loop (include/mseetc_mpc.h: msd_mpc_rolling_stock, msd_mpc_plant_states;
mseetc.mpc.DeviceLoop.run(mass=..., plantMass=...)).  Every re-solve of every scenario is checked against the CPU oracle solving that scenario's problem with its own
train from the logged measured state; the plant's states against the numpy statement mseetc.mpc.plantAdvance on the logged solutions; the device loop against the host
loop.  Shapes, arrival times: tests/test_mpc_speed_restrictions.py: shape; the six scenarios and the oracle stand-in: tests/test_mpc_rolling_stock.py (which states the
condition these inputs meet on the oracle).  Tolerances: those of tests/test_gpu_parity.py.
"""

import numpy as np
import pytest

import cases
from test_gpu_parity import OBJ_RTOL, Z_RTOL
from test_mpc_speed_restrictions import shape, _opts, oracle_solve
from test_mpc_rolling_stock import B, PLANT_STEPS, stock, own_train, shape6, plant_rows

pytestmark = pytest.mark.gpu

SHAPES = ['crop20_N40', 'full_N66', 'full_N66_rg', 'full_N130']
KEYS = ('t0', 'v0', 'T', 'status', 'iterations', 'cost', 'z')
STRIDE = 2


def _loop(name, **kw):
    from mseetc.mpc import DeviceLoop
    train, track, N, K, T = shape6(name)
    return DeviceLoop(train, track, _opts(N), K, **kw), train, N, K, T


def _vs_oracle(loop, train, N, k, r, s, model, row=None):
    "re-solve k of scenario s against the oracle solving the scenario's own problem (its own train; `row`: its row of limits) from the logged state"
    tr = own_train(train, model['mass'][s], model['r0'][s], model['r1'][s], model['r2'][s])
    prob = cases.oracle_problem(tr, loop.solvers[k].track, N - STRIDE*k, watchdogTrigger=-1)
    scen = loop.solvers[k]._scenarios(r['T'][s], r['t0'][s], loop.terminalVelocity, r['v0'][s])[0]
    ref = oracle_solve(prob, prob.bmax if row is None else row, scen, 'profile')
    assert ref['stats']['STATUS'] == 0
    dobj = abs(r['cost'][s] - ref['stats']['OBJ'])/abs(ref['stats']['OBJ'])
    dz = np.max(np.abs(r['z'][s] - ref['z'])/np.maximum(1.0, np.abs(ref['z'])))
    print('re-solve %d scenario %d: objective %.3e  variables %.3e  iterations %d / %d' % (k, s, dobj, dz, int(r['iterations'][s]), int(ref['stats']['ITERS'])))
    assert dobj <= OBJ_RTOL
    assert dz <= Z_RTOL
    assert abs(int(r['iterations'][s]) - int(ref['stats']['ITERS'])) <= 2


@pytest.mark.parametrize('name', SHAPES)
def test_model_rows_in_the_loop_vs_oracle(name):
    loop, train, N, K, T = _loop(name)
    model, _ = stock(train)
    log = loop.run(T, seed=3, **model)
    plain = loop.run(T, seed=3)
    assert len(log) == K
    for k, r in enumerate(log):
        assert np.all(r['status'] == 0), (k, r['status'])
        assert not r['relaxed'].any() and np.array_equal(r['T'], T) and 'tPlant' not in r
        for s in range(B):
            _vs_oracle(loop, train, N, k, r, s, model)
        for key in KEYS:
            assert np.array_equal(np.asarray(r[key])[0], np.asarray(plain[k][key])[0]), (k, key)      # the train of the problem: the plain loop's bits
        assert r['cost'][1] != plain[k]['cost'][1] and r['cost'][2] != plain[k]['cost'][2]
    loop.close()


@pytest.mark.parametrize('name', SHAPES)
def test_plant_states_on_the_device(name):
    """
    1 % noise.  The plant's state behind every advance against plantAdvance on the logged solution of that re-solve, from its logged initial state: rtol
    stride x 2e-12 (tests/test_mpc_rolling_stock.py: the chain of interval maps).  The state the next re-solve starts from is the noise rule applied to the plant's
    state, bit for bit (the rule is rounded products and one rounded sum on both sides).
    """
    from mseetc.mpc import plantAdvance
    noise, seed = 0.01, 3
    loop, train, N, K, T = _loop(name, noise=noise)
    model, plant = stock(train)
    rows = plant_rows(train, model, plant)
    log = loop.run(T, seed=seed, **model, **plant)
    rng = np.random.default_rng(seed)
    for k in range(K):
        r = log[k]
        assert np.all(r['status'] == 0), (k, r['status'])
        if k == K - 1:
            assert 'tPlant' not in r
            break
        scen = loop.solvers[k]._scenarios(r['T'], r['t0'], loop.terminalVelocity, r['v0'])
        t, v, stalled = plantAdvance(loop.solvers[k], r['z'], scen[:, 0], scen[:, 2], rows, PLANT_STEPS, STRIDE)
        dt, dv = np.max(np.abs(r['tPlant'] - t)/np.abs(t)), np.max(np.abs(r['vPlant'] - v)/v)
        print('advance %d: plant state against the host statement, relative: time %.3e  speed %.3e' % (k, dt, dv))
        assert not stalled.any() and not r['stalled'].any()
        assert dt <= STRIDE*2e-12 and dv <= STRIDE*2e-12
        n1, n2 = rng.standard_normal(B), rng.standard_normal(B)
        assert np.array_equal(log[k + 1]['t0'], np.maximum(r['tPlant']*(1 + noise*n1), 0.0))
        assert np.array_equal(log[k + 1]['v0'], r['vPlant']*(1 + noise*n2))
        # the plants that are not their models leave the plan (whose defects the solver closes to 1e-8)
        stp = 4 + int(loop.withPnBrake)
        planned = np.sqrt(r['z'][:, stp*STRIDE + stp - 1])
        assert np.all(np.abs(r['vPlant'][3:] - planned[3:]) > 1e-6*planned[3:])
    loop.close()


def test_twin_under_model_rows():
    """
    Track 00 cropped to 20 km, N = 40: the oracle's time-optimal problem needs 626.07 s with the train of the problem and 645.86 s with 1.3 times its mass (found on
    the CPU; the energy problem of the lighter train converges on the oracle at 638 s).  An arrival at 638 s is feasible for the first (12 s of room) and late for
    the second (8 s short): the heavy scenario ends `relaxed` with a solution, its arrival time moved to its own minimum running time at least and to that
    minimum x (1 + 21 lateMargin) at most (the third margin is 16 lateMargin; the bound leaves the twin's own error room); the light one is untouched.
    The twin's column MSD_OV_OBJ_DEN: the twin runs under the heavy scenario's row with the twin's own objective scaling (514.29 s here) in place of the energy
    problem's (3.6 / (1e-6 M) = 6.68).  The scaling does not move the minimiser, it changes the path and where inside the tolerance of 1e-8 the solve ends: on the
    oracle the two scalings give 645.86132 s and 645.86125 s, 1.1e-7 relative apart.  The window above does not see that.  What does: the moved arrival time against
    the host path, t0 + tmin (1 + lateMargin) with tmin from casadiSolver.minimumTime(scen, overrides=rows) -- which writes the twin's scaling into the rows and
    runs the twin on the device -- held to 1e-8 relative, a tenth of the distance between the two scalings on the oracle.  The same host path with the energy
    problem's scaling left in the column is printed beside it (not asserted: how far it lands is a property of the convergence path).
    """
    from oracle import oracle
    loop, train, N, K, _ = _loop('crop20_N40')
    mass = train.mass*np.array([1.0, 1.3])
    T = np.full(2, 638.0)
    log = loop.run(T, mass=mass)
    plain = loop.run(T)
    for k, r in enumerate(log):
        assert np.all(r['status'] >= 0), (k, r['status'])
        assert not r['relaxed'][0] and r['T'][0] == 638.0
        for key in KEYS:
            assert np.array_equal(np.asarray(r[key])[0], np.asarray(plain[k][key])[0]), (k, key)
    assert log[0]['relaxed'].tolist() == [False, True]
    tmin = []
    for m in mass:
        twin = cases.oracle_problem(own_train(train, m, train.r0, train.r1, train.r2), loop.solvers[0].track, N, energyOptimal=False, losses='none')
        ref = oracle.solve(twin, twin.scenario(9*20000.0/train.velocityMax), start='profile')
        assert ref['stats']['STATUS'] == 0
        tmin.append(ref['z'][-2])
    print('moved arrival times %s, oracle minima %s' % (log[0]['T'], tmin))
    assert abs(tmin[0] - 626.07) <= 0.05 and abs(tmin[1] - 645.86) <= 0.05
    assert tmin[0] < 638.0 < tmin[1]
    assert tmin[1] <= log[0]['T'][1] <= tmin[1]*(1 + 21*5e-3)
    # the host path of the same verdict: minimumTime under the row with the twin's scaling
    from mseetc import _device
    first = loop.solvers[0]
    scen = first._scenarios(T, 0.0, loop.terminalVelocity, 1.0)
    rows = first._overrides(2, mass, None, None, None)
    tm, ok = first.minimumTime(scen, overrides=rows)
    assert ok.all() and tm[0] < 638.0 < tm[1]
    want = 0.0 + tm[1]*(1 + 5e-3)
    loose = scen.copy()
    loose[:, 1] = np.maximum(3*first.track.length/first._vmaxTrain, 3*scen[:, 1])
    wrong = first._twin.problem.solve_batch(loose, overrides=rows)['z'][:, -2]      # (the energy problem's scaling left in the column)
    print('moved arrival time %.9f, host path %.9f (relative %.3e); minimum under the energy problem\'s scaling %.9f against %.9f (relative %.3e); oracle %.9f'
          % (log[0]['T'][1], want, abs(log[0]['T'][1] - want)/want, wrong[1], tm[1], abs(wrong[1] - tm[1])/tm[1], tmin[1]))
    assert rows[1, _device.OV['OBJ_DEN']] != first._twin._desc.obj_den
    assert abs(log[0]['T'][1] - want) <= 1e-8*want
    loop.close()


def test_a_plant_that_stalls_on_the_device():
    """
    The stall of tests/test_mpc_rolling_stock.py: test_a_plant_that_stalls on the device, crop20_N40 with 1 % noise from t = 5 s: scenario 2 runs a plant whose r0 is
    1.2 times the maximum tractive effort.  It falls below the minimum velocity in the first interval of the first advance: flagged in every record, the record
    holds the state in front of that interval (which is the measurement it keeps), every re-solve of it starts from the initial state, and the other scenarios are
    those of the same loop without that plant, bit for bit.  The host statement says the same of the first advance.
    """
    from mseetc.mpc import plantAdvance, _rollingStock
    loop, train, N, K, T = _loop('crop20_N40', noise=0.01)
    r0 = np.where(np.arange(B) == 2, 1.2*train.forceMax, train.r0)
    base = loop.run(T, seed=4, initialTime=5.0, plantMass=train.mass)
    log = loop.run(T, seed=4, initialTime=5.0, plantMass=train.mass, plantR0=r0)
    others = [0, 1, 3, 4, 5]
    for k in range(K):
        r = log[k]
        assert r['t0'][2] == 5.0 and r['v0'][2] == 1.0
        if k < K - 1:
            assert r['stalled'].tolist() == [False, False, True, False, False, False] and not base[k]['stalled'].any()
            assert r['tPlant'][2] == 5.0 and r['vPlant'][2] == 1.0
            assert np.array_equal(r['tPlant'][others], base[k]['tPlant'][others]) and np.array_equal(r['vPlant'][others], base[k]['vPlant'][others])
        else:
            assert 'stalled' not in r
        for key in KEYS:
            assert np.array_equal(np.asarray(r[key])[others], np.asarray(base[k][key])[others]), (k, key)
    rows = _rollingStock(train, B, None, None, None, None, train.mass, r0, None, None, PLANT_STEPS)[1]
    scen = loop.solvers[0]._scenarios(log[0]['T'], log[0]['t0'], loop.terminalVelocity, log[0]['v0'])
    t, v, stalled = plantAdvance(loop.solvers[0], log[0]['z'], scen[:, 0], scen[:, 2], rows, PLANT_STEPS, STRIDE)
    assert stalled.tolist() == log[0]['stalled'].tolist() and t[2] == 5.0 and v[2] == 1.0
    loop.close()


@pytest.mark.parametrize('warm', [False, True])
def test_device_loop_vs_host_loop_with_plant(warm):
    """
    The device loop against the host loop of mseetc/mpc.py (device solver, plantAdvance on the host) with model rows and plants, 1 % noise: the comparison of
    tests/test_mpc_speed_restrictions_gpu.py::test_device_loop_vs_host_loop_under_restrictions.
    """
    from mseetc.mpc import shrinkingHorizon
    loop, train, N, K, T = _loop('full_N66', noise=0.01, warmStart=warm)
    _, track, _, _, _ = shape6('full_N66')
    model, plant = stock(train)
    host = shrinkingHorizon(train, track, _opts(N), T, numResolves=K, noise=0.01, seed=1, warmStart=warm, **model, **plant)
    dev = loop.run(T, seed=1, **model, **plant)
    loop.close()
    assert len(host) == len(dev) == K
    moved = np.zeros(len(T), dtype=bool)
    for k, (h, d) in enumerate(zip(host, dev)):
        assert h['numIntervals'] == d['numIntervals'] == N - 2*k and abs(h['position'] - d['position']) < 1e-9
        assert np.all(h['status'] == 0) and np.all(d['status'] == 0)
        moved |= h['relaxed'] | d['relaxed']
        same = ~moved
        assert same.any()
        if not warm:
            di = np.abs(h['iterations'] - d['iterations'])[same]
            assert int((di > 2).sum()) <= 4 and di.max() <= 12, (k, di.max())
            assert np.array_equal(h['T'][same], d['T'][same])
            for key, tol in (('t0', 1e-7), ('v0', 1e-6), ('cost', 1e-6), ('z', 1e-4)):
                assert np.allclose(h[key][same], d[key][same], rtol=tol, atol=tol), (k, key)
        assert np.allclose(h['t0'][same], d['t0'][same], rtol=1e-6, atol=1e-6), k
        assert np.allclose(h['v0'][same], d['v0'][same], rtol=1e-5), k
        assert np.allclose(h['cost'][same], d['cost'][same], rtol=1e-5, atol=1e-5), k
        if k < K - 1:
            assert not h['stalled'].any() and not d['stalled'].any()
            assert np.allclose(h['tPlant'][same], d['tPlant'][same], rtol=1e-6, atol=1e-6) and np.allclose(h['vPlant'][same], d['vPlant'][same], rtol=1e-5), k


def test_state_of_the_records():
    from mseetc import _device
    loop, train, N, K, T = _loop('crop20_N40', noise=0.01)
    _, _, _, _, _, sets = shape('crop20_N40')
    sets = sets[:B]
    model, plant = stock(train)
    fresh = loop.run(T, seed=2)
    first = loop.run(T, seed=2, **model, **plant)
    # cleared after the run: the plain loop's bits again; and the object is reusable under the same records
    plain = loop.run(T, seed=2)
    again = loop.run(T, seed=2, **model, **plant)
    for k in range(K):
        for key in KEYS:
            assert np.array_equal(plain[k][key], fresh[k][key]), (k, key)
            assert np.array_equal(again[k][key], first[k][key]), (k, key)
        assert not np.array_equal(first[k]['z'][1], fresh[k]['z'][1])
    with pytest.raises(ValueError):
        loop.device.plant_states()      # (cleared: the loop holds no plant)
    # C level: records of B scenarios, a run of 4 -> MSD_E_INVALID (ValueError), nothing enqueued; a run of B is under them
    rows = loop.solvers[0]._overrides(B, **model)
    prow = plant_rows(train, model, plant)
    z4 = np.zeros((K - 1, 4))
    loop.device.rolling_stock(rows, prow, PLANT_STEPS)
    with pytest.raises(ValueError):
        loop.device.plant_states()      # (no run under the plant yet)
    with pytest.raises(ValueError):
        loop.device.run(T[:4], 0.0, 1.0, z4, z4)
    rng = np.random.default_rng(2)
    n = [(rng.standard_normal(B), rng.standard_normal(B)) for _ in range(K - 1)]
    n1, n2 = np.array([a for a, _ in n]), np.array([b for _, b in n])
    log, zs, _ = loop.device.run(T, 0.0, 1.0, n1, n2)
    assert all(np.array_equal(zs[k], first[k]['z']) for k in range(K))
    states = loop.device.plant_states()
    assert states.shape == (K - 1, B, 3) and all(np.array_equal(states[k, :, 0], first[k]['tPlant']) for k in range(K - 1))
    # records the library refuses leave the previous ones in place
    OV, PL = _device.OV, _device.MPC_PL
    for what, col, value in (('model', OV['OBJ_DEN'], 0.0), ('model', OV['SR1'], -1.0), ('model', OV['F_MAX'], -100.0), ('model', OV['TOTAL_MASS'], np.nan),
                             ('plant', PL['SR2'], -1e-9), ('plant', PL['SR0'], np.inf), ('plant', PL['FORCE_SCALE'], 0.0), ('plant', PL['FORCE_SCALE'], np.nan)):
        r, p = rows.copy(), prow.copy()
        (r if what == 'model' else p)[1, col] = value
        with pytest.raises(ValueError):
            loop.device.rolling_stock(r, p, PLANT_STEPS)
    for steps in (0, 65, -1):
        with pytest.raises(ValueError):
            loop.device.rolling_stock(rows, prow, steps)
    log, zs, _ = loop.device.run(T, 0.0, 1.0, n1, n2)
    assert all(np.array_equal(zs[k], first[k]['z']) for k in range(K))
    # composes with the speed restrictions; the counts must agree, whichever comes second
    with pytest.raises(ValueError):
        loop.device.speed_restrictions(*loop.restrictionRecords(sets[:4], 4))
    loop.device.rolling_stock(None)
    loop.device.speed_restrictions(*loop.restrictionRecords(sets[:4], 4))
    with pytest.raises(ValueError):
        loop.device.rolling_stock(rows, prow, PLANT_STEPS)
    loop.device.speed_restrictions(None)
    log, zs, _ = loop.device.run(T, 0.0, 1.0, n1, n2)
    assert all(np.array_equal(zs[k], fresh[k]['z']) for k in range(K))
    # one run with both: every re-solve ends with status 0, and the restricted scenarios with a train of their own are the oracle's under their row with their train
    both = loop.run(T, seed=2, speedRestrictions=sets, **model, **plant)
    for k, r in enumerate(both):
        assert np.all(r['status'] == 0), (k, r['status'])
        limits = loop.restrictedLimits(k, sets, B)
        for s in (1, 4):
            scen = loop.restrictedScenarios(k, r['T'], r['t0'], r['v0'], sets, B)[s]
            tr = own_train(train, model['mass'][s], model['r0'][s], model['r1'][s], model['r2'][s])
            prob = cases.oracle_problem(tr, loop.solvers[k].track, N - STRIDE*k, watchdogTrigger=-1)
            ref = oracle_solve(prob, limits[s], scen, 'profile')
            assert ref['stats']['STATUS'] == 0
            assert abs(r['cost'][s] - ref['stats']['OBJ']) <= OBJ_RTOL*abs(ref['stats']['OBJ'])
            assert np.max(np.abs(r['z'][s] - ref['z'])/np.maximum(1.0, np.abs(ref['z']))) <= Z_RTOL
            assert abs(int(r['iterations'][s]) - int(ref['stats']['ITERS'])) <= 2
    assert not np.array_equal(both[0]['z'][1], first[0]['z'][1])
    assert np.array_equal(loop.run(T, seed=2)[K - 1]['z'], fresh[K - 1]['z'])
    loop.close()
