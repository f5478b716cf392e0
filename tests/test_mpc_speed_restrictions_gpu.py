"""
Speed restrictions inside the device-resident shrinking-horizon loop (include/mseetc_mpc.h: msd_mpc_speed_restrictions; mseetc.mpc.DeviceLoop.run(speedRestrictions=...)).
The rows the loop's kernel builds are held to the host statement bit for bit, and every re-solve of every scenario is checked against the CPU oracle solving the
restricted problem of that re-solve as a problem of its own, from the logged measured state (shapes, sets and the oracle stand-in: tests/test_mpc_speed_restrictions.py).

Shapes: track 00 cropped to 20 km, N = 40, K = 4 (the 64 x 1 kernel with the corrections inside); the full track, N = 66, K = 3, both brakes (grids 66 / 64 / 62: from the
64 x 2 kernel to 64 x 1); the same with the figure-10 train (the one-brake family, whose follow-up kernel takes the corrections); N = 130, K = 2 (a two-wave first pass).
On the oracle every re-solve of every scenario below ends with status 0 at these arrival times, with and without 1 % noise (checked on the CPU), and the record near
the start restricts no interval from re-solve 1 on (tests/test_mpc_speed_restrictions.py asserts it).
Tolerances: those of tests/test_gpu_parity.py (_compare).
"""

import numpy as np
import pytest

import cases
from test_gpu_parity import OBJ_RTOL, Z_RTOL
from test_mpc_speed_restrictions import shape, _opts, oracle_solve, under, V60
from test_speed_restrictions import _bmax

pytestmark = pytest.mark.gpu

SHAPES = ['crop20_N40', 'full_N66', 'full_N66_rg', 'full_N130']
# Restricted from the start (sets 1, 3, 4, 5) in re-solve 0, announced at re-solve 1 (set 2) in re-solve 1, a scenario costs more than the same scenario of the
# unrestricted loop, which starts that re-solve from the same measured state (no noise): on the oracle by 1.885 kWh at least (N = 130, set 1; the others 2.2 ... 11.3 kWh).
# Asserted: half of the smallest difference.
KWH_MARGIN = 0.94


def _loop(name, **kw):
    from mseetc.mpc import DeviceLoop
    train, track, N, K, T, sets = shape(name)
    return DeviceLoop(train, track, _opts(N), K, **kw), train, N, K, T, sets


@pytest.mark.parametrize('name', SHAPES)
def test_rows_on_the_device(name):
    "the loop's kernel against the numpy statement, bit for bit, for every re-solve"
    loop, train, N, K, T, sets = _loop(name)
    B = len(sets)
    with pytest.raises(ValueError):
        loop.device.limit_rows(0, B)      # (no records yet)
    loop.device.speed_restrictions(*loop.restrictionRecords(sets, B))
    for k in range(K):
        got, want, bmax = loop.device.limit_rows(k, B), loop.restrictedLimits(k, sets, B), _bmax(loop.solvers[k])
        assert got.shape == want.shape == (B, N - 2*k + 1) and np.array_equal(got, want), k
        assert np.array_equal(got[0], bmax) and not np.array_equal(got[1], bmax)
        assert np.array_equal(got[2], bmax) == (k < 1)      # announced at re-solve 1
        assert np.array_equal(got[4], bmax) == (k > 0)      # behind the train from re-solve 1 on
    with pytest.raises(ValueError):
        loop.device.limit_rows(K, B)
    with pytest.raises(ValueError):
        loop.device.limit_rows(0, B - 1)
    # one record per scenario at most: the narrowest records
    two = [sets[2], sets[0]]
    loop.device.speed_restrictions(*loop.restrictionRecords(two, 2))
    assert np.array_equal(loop.device.limit_rows(1, 2), loop.restrictedLimits(1, sets, B)[[2, 0]])
    loop.device.speed_restrictions(None)
    with pytest.raises(ValueError):
        loop.device.limit_rows(0, 2)
    loop.close()


@pytest.mark.parametrize('name', SHAPES)
def test_cold_loop_vs_oracle(name):
    loop, train, N, K, T, sets = _loop(name)
    B = len(sets)
    log = loop.run(T, seed=3, speedRestrictions=sets)
    plain = loop.run(T, seed=3)
    assert len(log) == K
    for k, r in enumerate(log):
        assert np.all(r['status'] == 0), (k, r['status'])
        assert not r['relaxed'].any() and np.array_equal(r['T'], T)
        rows = loop.restrictedLimits(k, sets, B)
        scen = loop.restrictedScenarios(k, r['T'], r['t0'], r['v0'], sets, B)
        prob = cases.oracle_problem(train, loop.solvers[k].track, N - 2*k, watchdogTrigger=-1)
        for s in range(B):
            ref = oracle_solve(prob, rows[s], scen[s], 'profile')
            assert ref['stats']['STATUS'] == 0
            dobj = abs(r['cost'][s] - ref['stats']['OBJ'])/abs(ref['stats']['OBJ'])
            dz = np.max(np.abs(r['z'][s] - ref['z'])/np.maximum(1.0, np.abs(ref['z'])))
            print('re-solve %d scenario %d: objective %.3e  variables %.3e  iterations %d / %d' % (k, s, dobj, dz, int(r['iterations'][s]), int(ref['stats']['ITERS'])))
            assert dobj <= OBJ_RTOL
            assert dz <= Z_RTOL
            assert abs(int(r['iterations'][s]) - int(ref['stats']['ITERS'])) <= 2
            assert r['z'][s][-1] == scen[s, 3]
            assert r['z'][s][-2] <= scen[s, 1]*(1 + 1.01e-8)
    # the restrictions cost energy where both loops start from the same state
    for s in (1, 3, 4, 5):
        assert log[0]['cost'][s] > plain[0]['cost'][s] + KWH_MARGIN, (s, log[0]['cost'], plain[0]['cost'])
    assert np.array_equal(log[1]['t0'][2], plain[1]['t0'][2]) and log[1]['cost'][2] > plain[1]['cost'][2] + KWH_MARGIN
    loop.close()


@pytest.mark.parametrize('name', ['crop20_N40', 'full_N66_rg'])
def test_announcement(name):
    "the same loop object with and without restrictions, same seed, 1 % noise: a scenario changes with the re-solve that learns of its restriction, not before"
    loop, train, N, K, T, sets = _loop(name, noise=0.01)
    with_rs = loop.run(T, seed=5, speedRestrictions=sets)
    without = loop.run(T, seed=5)
    keys = ('t0', 'v0', 'T', 'status', 'iterations', 'cost', 'z')
    for k in range(K):
        for key in keys:
            assert np.array_equal(with_rs[k][key][0], without[k][key][0]), (k, key)      # the unrestricted scenario: identical throughout
            if k == 0 or (k == 1 and key in ('t0', 'v0')) or key in ('T', 'status'):      # (re-solve 1 still starts from the state re-solve 0 led to)
                assert np.array_equal(with_rs[k][key][2], without[k][key][2]), (k, key)
            elif key != 'iterations':
                assert not np.array_equal(with_rs[k][key][2], without[k][key][2]), (k, key)
        assert np.all(with_rs[k]['status'] == 0) and np.all(without[k]['status'] == 0)
    loop.close()


@pytest.mark.parametrize('warm', [False, True])
def test_device_loop_vs_host_loop_under_restrictions(warm):
    """
    The device loop against the host loop of mseetc/mpc.py under the same restrictions, 1 % noise: the comparison of
    tests/test_gpu_parity.py::test_device_resident_shrinking_horizon_loop_vs_host_loop, on the scenarios whose arrival time neither loop moved.
    """
    from mseetc.mpc import shrinkingHorizon
    loop, train, N, K, T, sets = _loop('full_N66', noise=0.01, warmStart=warm)
    _, track, _, _, _, _ = shape('full_N66')
    host = shrinkingHorizon(train, track, _opts(N), T, numResolves=K, noise=0.01, seed=1, warmStart=warm, speedRestrictions=sets)
    dev = loop.run(T, seed=1, speedRestrictions=sets)
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


def test_state_of_the_records():
    loop, train, N, K, T, sets = _loop('crop20_N40', noise=0.01)
    B = len(sets)
    fresh = loop.run(T, seed=2)
    first = loop.run(T, seed=2, speedRestrictions=sets)
    # cleared after the run: the unrestricted bits again; and the object is reusable under the same records
    plain = loop.run(T, seed=2)
    again = loop.run(T, seed=2, speedRestrictions=sets)
    for k in range(K):
        for key in ('t0', 'v0', 'T', 'status', 'iterations', 'cost', 'z'):
            assert np.array_equal(plain[k][key], fresh[k][key]), (k, key)
            assert np.array_equal(again[k][key], first[k][key]), (k, key)
        assert not np.array_equal(first[k]['z'][1], fresh[k]['z'][1])
    # C level: records of B scenarios, a run of 4 -> MSD_E_INVALID (ValueError), nothing enqueued; a run of B is under them; cleared: the plain loop
    z = np.zeros((K - 1, 4))
    loop.device.speed_restrictions(*loop.restrictionRecords(sets, B))
    with pytest.raises(ValueError):
        loop.device.run(T[:4], 0.0, 1.0, z, z)
    rng = np.random.default_rng(2)
    n = [(rng.standard_normal(B), rng.standard_normal(B)) for _ in range(K - 1)]
    n1, n2 = np.array([a for a, _ in n]), np.array([b for _, b in n])
    log, zs, _ = loop.device.run(T, 0.0, 1.0, n1, n2)
    assert all(np.array_equal(zs[k], first[k]['z']) for k in range(K))
    # records the library refuses leave the previous ones in place
    origin, count, records = loop.restrictionRecords(sets, B)
    for change in ('begin', 'velocity', 'resolve', 'grid0', 'origin'):
        o, r = origin.copy(), records.copy()
        if change == 'begin':
            r[1, 0, 0] = r[1, 0, 1]
        elif change == 'velocity':
            r[1, 0, 2] = 1.0
        elif change == 'resolve':
            r[1, 0, 3] = K
        elif change == 'grid0':
            r[1, 0, :2] = 20000.0, 20500.0
        else:
            o[2] = o[1] - 1.0
        with pytest.raises(ValueError):
            loop.device.speed_restrictions(o, count, r)
    with pytest.raises(ValueError):
        loop.device.speed_restrictions(origin, count + 2, records)
    assert np.array_equal(loop.device.limit_rows(1, B), loop.restrictedLimits(1, sets, B))
    loop.device.speed_restrictions(None)
    log, zs, _ = loop.device.run(T, 0.0, 1.0, n1, n2)
    assert all(np.array_equal(zs[k], fresh[k]['z']) for k in range(K))
    loop.close()


def test_arrival_time_infeasible_only_under_the_restriction():
    """
    Track 00 cropped to 20 km, N = 40: the oracle's time-optimal twin needs 626.07 s on the open line and 745.42 s under 60 km/h between 10000 m and 12000 m
    (from re-solve 1's state: 600.36 s and 719.71 s after the first kilometre).  An arrival at 690 s is feasible without the record (64 s of room) and late with
    it (55 s short): the restricted scenario ends `relaxed` with a solution, its arrival time moved to the minimum running time under the row at least; the
    scenario that learns of the restriction at re-solve 1 is moved there.
    """
    from oracle import oracle
    loop, train, N, K, _, _ = _loop('crop20_N40')
    rec = (10000, 12000, V60)
    sets = [[], [rec], [rec + (1,)]]
    T = np.full(3, 690.0)
    log = loop.run(T, speedRestrictions=sets)
    for k, r in enumerate(log):
        assert np.all(r['status'] >= 0), (k, r['status'])
        assert not r['relaxed'][0] and r['T'][0] == 690.0
        assert k == 0 or np.all(r['T'] >= log[k - 1]['T'])
    assert log[0]['relaxed'].tolist() == [False, True, False] and log[1]['relaxed'][2]
    twin = cases.oracle_problem(train, loop.solvers[0].track, N, energyOptimal=False, losses='none')
    p = under(twin, loop.restrictedLimits(0, sets, 3)[1])
    ref = oracle.solve(p, p.scenario(9*20000.0/train.velocityMax), start='profile')
    assert ref['stats']['STATUS'] == 0 and abs(ref['z'][-2] - 745.42) <= 0.05
    print('moved arrival times %s, oracle minimum %.4f s' % (log[0]['T'], ref['z'][-2]))
    assert ref['z'][-2] <= log[0]['T'][1] <= ref['z'][-2]*(1 + 21*5e-3)
    assert log[0]['T'][2] == 690.0 and log[1]['T'][2] > 690.0
    loop.close()
