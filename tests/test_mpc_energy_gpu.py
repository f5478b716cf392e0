"""
The energy account inside the device-resident shrinking-horizon loop (include/mseetc_mpc.h: msd_mpc_energy, msd_mpc_energy_records; mseetc.mpc.DeviceLoop.run(
energyAccount=True, plantEta*=...)).  Every leg's record is checked against the numpy statement mseetc.mpc.plantEnergy on the logged solutions from the logged initial
state; the account must change nothing else in the loop, bit for bit; the device loop against the host loop.  Shapes, scenarios and the inputs' condition on the oracle:
tests/test_mpc_energy.py (crop20_N40 with K = 4 and both brakes, full_N66_rg with K = 3 and one brake, the N = 30 table shape with K = 3; six scenarios, 1 % noise).

Tolerances.  Components in closed form (traction, regenerated, pneumatic brake, losses with constant efficiencies): 1e-12 relative to the component's own magnitude
(sums of at most 130 products; the device contracts a b + c).  State at the end of a leg with a plant: n x 2e-12 relative, n the intervals of the leg (the plant
tolerance of tests/test_mpc_rolling_stock_gpu.py); without a plant it is read from the plan: bit for bit.  Losses of the loss table: TABLE_MEASURED below is the maximum
relative deviation measured on the table shape over all legs, with and without the plant; asserted: 10 x that.

Measured on an MI355X (printed by the tests), maximum relative deviation from the statement over all legs and scenarios:
  closed-form components  2.1e-16 / 5.4e-16 (crop20_N40 without / with the plants), 3.7e-16 / 3.5e-16 (full_N66_rg), 3.2e-16 / 2.6e-16 (table shape)
  state per interval      8.2e-17 (crop20_N40), 1.6e-16 (full_N66_rg), 9.7e-17 (table shape); without a plant bit-equal
  table losses            2.14e-16 without the plant, 3.41e-16 with it (TABLE_MEASURED): rounding of a sum of Runge-Kutta stages, far below 1e-9 -- device and numpy
                          evaluate the same bicubic patches in the same order, and what differs is the contraction of a b + c
  device loop against host loop (crop20_N40, model rows and plants), relative to the component's own magnitude: traction, losses and total 1.25e-12, pneumatic
                          brake 4.1e-15, regenerated 3.89e-10 (a residue: test_device_loop_vs_host_loop), arrival time 1.6e-13, arrival speed 5.3e-12
"""

import numpy as np
import pytest

from test_mpc_speed_restrictions import shape, _opts
from test_mpc_rolling_stock import B, PLANT_STEPS
from test_mpc_energy import SHAPES, NOISE, SEED, STRIDE, inputs, rows_of, statement

pytestmark = pytest.mark.gpu

KEYS = ('t0', 'v0', 'T', 'status', 'iterations', 'cost', 'z', 'relaxed')
ENERGY = (('traction', 'energyTraction'), ('regenerated', 'energyRegenerated'), ('pnBrake', 'energyPnBrake'), ('losses', 'energyLosses'))
TABLE_MEASURED = 3.41e-16      # (the module's docstring)
ETA = dict(plantEtaTraction=np.linspace(0.80, 0.90, B), plantEtaRgBrake=0.7)


@pytest.fixture(scope='module')
def loops():
    "one DeviceLoop per (shape, warm start), its runs cached by their keywords"
    from mseetc.mpc import DeviceLoop
    cache = {}

    def get(name, warm=False):
        if (name, warm) not in cache:
            train, track, N, K, T, loopkw, _, runs = inputs(name)
            cache[(name, warm)] = dict(loop=DeviceLoop(train, track, _opts(N), K, noise=NOISE, warmStart=warm, **loopkw), train=train, track=track, N=N, K=K, T=T, kw=runs, logs={})
        return cache[(name, warm)]
    yield get
    for c in cache.values():
        c['loop'].close()


def run(c, plant, account, tag='', **extra):
    key = (bool(plant), bool(account), tag)
    if key not in c['logs']:
        c['logs'][key] = c['loop'].run(c['T'], seed=SEED, energyAccount=account, **c['kw'][int(plant)], **extra)
    return c['logs'][key]


def against_statement(c, log, kw, eta=None, scen=None):
    "every leg's record against plantEnergy on the logged solutions; returns the maximum relative deviations (closed-form components, table losses, state)"
    loop, train, K = c['loop'], c['train'], c['K']
    plant = rows_of(train, kw)[0] is not None
    table = eta is None and loop.solvers[0]._desc.loss_kind == 2
    worst = dict(static=0.0, table=0.0, state=0.0)
    for k, r in enumerate(log):
        assert np.all(r['status'] == 0), (k, r['status'])
        want = statement(loop, log, k, train, kw, eta=eta, scen=None if scen is None else scen(k, r))
        n = STRIDE if k < K - 1 else r['numIntervals']
        assert np.array_equal(r['legIntervals'], want['intervals']), (k, r['legIntervals'], want['intervals'])
        for key, logged in ENERGY:
            d = np.abs(r[logged] - want[key])
            scale = np.abs(want[key])
            rel = float(np.max(np.where(scale > 0, d/np.where(scale > 0, scale, 1.0), d)))
            if key == 'losses' and table:
                worst['table'] = max(worst['table'], rel)      # (asserted by the caller, behind its print)
            else:
                worst['static'] = max(worst['static'], rel)
                assert rel <= 1e-12, (k, key, rel, r[logged], want[key])
        if k == K - 1:
            t, v = r['tArrival'], r['vArrival']
        elif plant:
            t, v = r['tPlant'], r['vPlant']
        else:
            continue
        if plant:
            dt, dv = float(np.max(np.abs(t - want['t'])/np.abs(want['t']))), float(np.max(np.abs(v - want['v'])/want['v']))
            worst['state'] = max(worst['state'], dt/n, dv/n)
            assert dt <= n*2e-12 and dv <= n*2e-12, (k, dt, dv)
        else:
            assert np.array_equal(t, want['t']) and np.array_equal(v, want['v'])
    return worst


def integrated_losses_for_information(c, log):
    """
    Printed, not asserted (profiles/r14/README.md records the figures): the account's table losses without a plant against postProcessDataFrame(integrateLosses=True)
    of the same plans -- msd_integrate_losses, in the time domain from `vstart` over the plan's dt_i at CVODES' tolerances, where the account integrates in the space
    domain with PLANT_STEPS Runge-Kutta steps from the plan's own b_i -- and against the mid-point rule (integrateLosses=False).  The distance is a property of the
    discretisation, not a pass mark.
    """
    from mseetc.utils import postProcessDataFrame
    loop, train, K = c['loop'], c['train'], c['K']
    for k, r in enumerate(log):
        n = STRIDE if k < K - 1 else r['numIntervals']
        d = np.zeros((B, 2))
        for s in range(B):
            frame = loop.solvers[k].unpack(r['z'][s])
            for j, integrate in enumerate((True, False)):
                want = postProcessDataFrame(frame, loop.solvers[k].points, train, CVODES=False, integrateLosses=integrate)['Losses [kWh]'].values[:n].sum()
                d[s, j] = abs(r['energyLosses'][s] - want)/want
        print('leg %d (%d intervals): table losses of the account against the integrated losses %.3e ... %.3e, against the mid-point rule %.3e ... %.3e (relative)'
              % (k, n, d[:, 0].min(), d[:, 0].max(), d[:, 1].min(), d[:, 1].max()))


@pytest.mark.parametrize('plant', [False, True])
@pytest.mark.parametrize('name', SHAPES)
def test_records_against_the_statement(loops, name, plant):
    """
    With and without plant rows, every leg's record -- the final leg included: the arrival -- against plantEnergy on the logged solutions and the logged initial state.
    """
    c = loops(name)
    log = run(c, plant, True)
    worst = against_statement(c, log, c['kw'][int(plant)])
    print('%s, %s: maximum relative deviation from the statement: closed-form components %.3e, table losses %.3e, state per interval %.3e'
          % (name, 'plant' if plant else 'plan', worst['static'], worst['table'], worst['state']))
    assert worst['table'] <= 10*TABLE_MEASURED
    if name == 'table_N30' and not plant:
        integrated_losses_for_information(c, log)
    from mseetc.mpc import closedLoopEnergy
    out = closedLoopEnergy(log)
    assert np.all(out['total'] > 0) and np.all(out['losses'] > 0)
    print('closed-loop energy %s kWh (losses %s), arrival %s s at %s m/s, complete %s' % (out['total'].tolist(), out['losses'].tolist(), out['arrivalTime'].tolist(),
                                                                                          out['arrivalVelocity'].tolist(), out['complete'].tolist()))


@pytest.mark.parametrize('name', SHAPES)
def test_final_leg_without_a_plant_is_the_last_plan(loops, name):
    "without a plant the arrival is the last plan's terminal node, bit for bit, every leg is complete, and the legs in front of it end at node `stride` of their plans"
    c = loops(name)
    log = run(c, False, True)
    last = log[-1]
    assert np.array_equal(last['tArrival'], last['z'][:, -2]) and np.array_equal(last['vArrival'], np.sqrt(last['z'][:, -1]))
    assert np.array_equal(last['legIntervals'], np.full(B, c['N'] - STRIDE*(c['K'] - 1)))
    assert all(np.array_equal(r['legIntervals'], np.full(B, STRIDE)) for r in log[:-1])
    assert all('tArrival' not in r for r in log[:-1])


@pytest.mark.parametrize('name,warm,plant', [('crop20_N40', False, True), ('crop20_N40', True, True), ('crop20_N40', False, False), ('crop20_N40', True, False),
                                             ('full_N66_rg', False, True), ('table_N30', False, True), ('table_N30', False, False)])
def test_the_account_changes_nothing_else(loops, name, warm, plant):
    """
    The log and the solutions of the run with the account are those of the same run without it, bit for bit, from warm and from cold starts; with a plant -- where
    mpc_energy stands in mpc_plant's place -- so are the plant's states, the stall flags and the measured state the next re-solve starts from.
    """
    c = loops(name, warm)
    on, off = run(c, plant, True), run(c, plant, False)
    assert len(on) == len(off) == c['K']
    for k, (a, b) in enumerate(zip(on, off)):
        for key in KEYS:
            assert np.array_equal(a[key], b[key]), (k, key)
        assert 'energyTraction' in a and 'energyTraction' not in b and 'legIntervals' not in b
        if plant and k < c['K'] - 1:
            for key in ('tPlant', 'vPlant', 'stalled'):
                assert np.array_equal(a[key], b[key]), (k, key)
        else:
            assert 'tPlant' not in a


def test_plant_efficiencies_of_their_own(loops):
    "plantEta*: the losses are the statement's under `eta`, every other component and every plan is that of the run without them, bit for bit"
    c = loops('crop20_N40')
    kw = c['kw'][1]
    log = run(c, True, True, tag='eta', **ETA)
    base = run(c, True, True)
    eta = np.stack([ETA['plantEtaTraction'], np.full(B, ETA['plantEtaRgBrake'])], axis=1)
    against_statement(c, log, kw, eta=eta)
    for k, (a, b) in enumerate(zip(log, base)):
        for key in KEYS + ('energyTraction', 'energyRegenerated', 'energyPnBrake', 'legIntervals'):
            assert np.array_equal(a[key], b[key]), (k, key)
        assert np.all(a['energyLosses'] != b['energyLosses'])
    implied = run(c, True, False, tag='eta', **ETA)      # (the efficiencies imply the account)
    assert all(np.array_equal(a['energyLosses'], b['energyLosses']) for a, b in zip(implied, log))


# device loop against host loop, measured on an MI355X (printed by the test): relative to the component's own magnitude, maximum over the six scenarios
HOST_MEASURED = dict(total=1.25e-12, traction=1.25e-12, regenerated=3.89e-10, pnBrake=4.1e-15, losses=1.25e-12)


def test_device_loop_vs_host_loop(loops):
    """
    closedLoopEnergy of the device loop against that of the host loop of mseetc/mpc.py (device solver, plantAdvance and plantEnergy on the host) on crop20_N40 with
    model rows and plants, 1 % noise, at the tolerances of this module: every component to 1e-12 relative to its own magnitude, arrival time and speed to n x 2e-12
    (n = 34, the intervals of the final leg), leg counts and `complete` equal.  Where a component's measured distance exceeds 1e-12 the bound is 10 x the measured
    maximum (HOST_MEASURED), because the two accounts are then not sums over the same plans.  The plans differ from re-solve 0 on, which both loops start from the
    same state, bit for bit: the device loop launches its solves with one attempt per scenario on the first-pass kernel that has the second-order correction inside,
    the host loop through solveBatch, and the two end, at the tolerance of 1e-8, on points 3.9e-12 apart (relative to max(1, |z|); 3.2e-11, 3.6e-11, 6.7e-11 in the
    later re-solves, whose measured states are then 2e-16 ... 3e-12 apart) -- printed below.  Measured: traction, losses and total 1.25e-12 (scenario 4; at most
    5.3e-13 on the others), pneumatic brake 4.1e-15, arrival time 1.6e-13, arrival speed 5.3e-12.  `regenerated` 3.89e-10: on five of the six scenarios it is not
    braking energy but the interior-point residue of forces at their bound 0 (2e-9 ... 4e-8 kWh of 100 kWh), and its relative distance is that of the residue
    between two plans; on the scenario that does brake regeneratively (17.2 kWh) it is 5.5e-13.
    """
    from mseetc.mpc import shrinkingHorizon, closedLoopEnergy
    c = loops('crop20_N40')
    kw = c['kw'][1]
    dev = run(c, True, True)
    host = shrinkingHorizon(c['train'], c['track'], _opts(c['N']), c['T'], numResolves=c['K'], noise=NOISE, seed=SEED, energyAccount=True, **kw)
    a, b = closedLoopEnergy(dev), closedLoopEnergy(host)
    for k in range(c['K']):
        assert np.array_equal(dev[k]['legIntervals'], host[k]['legIntervals']), k
        for key in ('t0', 'v0', 'z'):
            print('re-solve %d: %s of the two loops apart by %.3e' % (k, key, np.max(np.abs(dev[k][key] - host[k][key])/np.maximum(1.0, np.abs(host[k][key])))))
    assert np.array_equal(a['complete'], b['complete'])
    n = c['N'] - STRIDE*(c['K'] - 1)
    dt = np.max(np.abs(a['arrivalTime'] - b['arrivalTime'])/b['arrivalTime'])
    dv = np.max(np.abs(a['arrivalVelocity'] - b['arrivalVelocity'])/b['arrivalVelocity'])
    print('arrival: time apart by %.3e, speed by %.3e (relative)' % (dt, dv))
    worst = {}
    for key in ('total', 'traction', 'regenerated', 'pnBrake', 'losses'):
        worst[key] = float(np.max(np.abs(a[key] - b[key])/np.abs(b[key])))
        print('%s: device %s host %s (relative to its own magnitude %.3e)' % (key, a[key].tolist(), b[key].tolist(), worst[key]))
    assert dt <= n*2e-12 and dv <= n*2e-12
    for key, d in worst.items():
        assert d <= max(1e-12, 10*HOST_MEASURED[key]), (key, d)


def test_state_of_the_records(loops):
    from mseetc import _device
    c = loops('crop20_N40')
    loop, train, K, T = c['loop'], c['train'], c['K'], c['T']
    M = train.mass*train.rho
    model = {key: c['kw'][1][key] for key in ('mass', 'r0', 'r1', 'r2')}
    first = run(c, True, True)
    plain = run(c, False, True)
    # cleared after a run
    with pytest.raises(ValueError):
        loop.device.energy_records()
    # C level: no records before a run under the account; a run of another count is refused and enqueues nothing; a run of B keeps the account
    rng = np.random.default_rng(SEED)
    n = [(rng.standard_normal(B), rng.standard_normal(B)) for _ in range(K - 1)]
    n1, n2 = np.array([a for a, _ in n]), np.array([b for _, b in n])
    z4 = np.zeros((K - 1, 4))
    loop.device.energy(B, M, None, PLANT_STEPS)
    with pytest.raises(ValueError):
        loop.device.energy_records()
    with pytest.raises(ValueError):
        loop.device.run(T[:4], 0.0, 1.0, z4, z4)
    with pytest.raises(ValueError):
        loop.device.energy_records()
    log, zs, _ = loop.device.run(T, 0.0, 1.0, n1, n2)
    rec = loop.device.energy_records()
    EN = _device.MPC_EN
    assert rec.shape == (K, B, EN['COUNT'])
    assert all(np.array_equal(zs[k], plain[k]['z']) and np.array_equal(rec[k, :, EN['LOSSES']], plain[k]['energyLosses']) for k in range(K))
    assert np.array_equal(rec[K - 1, :, EN['T']], plain[K - 1]['tArrival'])
    # what the library refuses leaves the account in place
    bad_eta = np.full((B, 2), 0.8)
    for args in ((B, 0.0, None, PLANT_STEPS), (B, -M, None, PLANT_STEPS), (B, np.nan, None, PLANT_STEPS), (B, np.inf, None, PLANT_STEPS), (B, M, None, 0), (B, M, None, 65)):
        with pytest.raises(ValueError):
            loop.device.energy(*args)
    for value in (0.0, 1.0 + 1e-9, -0.1, np.nan):
        e = bad_eta.copy(); e[3, 1] = value
        with pytest.raises(ValueError):
            loop.device.energy(B, M, e, PLANT_STEPS)
    with pytest.raises(ValueError):
        _device._check(_device.lib().msd_mpc_energy(loop.device._m, -1, M, None, PLANT_STEPS))
    assert np.array_equal(loop.device.energy_records(), rec)
    log, zs, _ = loop.device.run(T, 0.0, 1.0, n1, n2)
    assert np.array_equal(loop.device.energy_records(), rec)
    # cleared by nscen = 0: the plain loop, and no records
    loop.device.energy(None)
    with pytest.raises(ValueError):
        loop.device.energy_records()
    log, zs, _ = loop.device.run(T[:4], 0.0, 1.0, z4, z4)
    # the counts of account, rolling stock and restrictions must agree, whichever comes later; the steps are the plant's
    rows = loop.solvers[0]._overrides(B, **model)
    prow = rows_of(train, c['kw'][1])[0]
    loop.device.rolling_stock(rows, prow, PLANT_STEPS)
    for args in ((4, M, None, PLANT_STEPS), (B, M, None, PLANT_STEPS + 1)):
        with pytest.raises(ValueError):
            loop.device.energy(*args)
    loop.device.energy(B, M, None, PLANT_STEPS)
    sets = shape('crop20_N40')[5][:B]
    with pytest.raises(ValueError):
        loop.device.speed_restrictions(*loop.restrictionRecords(sets[:4], 4))
    with pytest.raises(ValueError):
        loop.device.rolling_stock(rows[:4], prow[:4], PLANT_STEPS)
    log, zs, _ = loop.device.run(T, 0.0, 1.0, n1, n2)
    rec = loop.device.energy_records()
    assert all(np.array_equal(zs[k], first[k]['z']) and np.array_equal(rec[k, :, EN['TRACTION']], first[k]['energyTraction']) for k in range(K))
    loop.device.rolling_stock(rows, prow, PLANT_STEPS + 1)      # (a plant with other steps behind the account: the run is refused)
    with pytest.raises(ValueError):
        loop.device.run(T, 0.0, 1.0, n1, n2)
    loop.device.energy(None); loop.device.rolling_stock(None)
    # one run with restrictions, rolling stock and the account: every re-solve ends with status 0 and the records are the statement's under the restricted scenario records
    both = loop.run(T, seed=SEED, speedRestrictions=sets, energyAccount=True, **c['kw'][1])
    against_statement(c, both, c['kw'][1], scen=lambda k, r: loop.restrictedScenarios(k, r['T'], r['t0'], r['v0'], sets, B))
    assert not np.array_equal(both[0]['z'][1], first[0]['z'][1])
    again = loop.run(T, seed=SEED, energyAccount=True, **c['kw'][1])
    assert all(np.array_equal(again[k]['z'], first[k]['z']) and np.array_equal(again[k]['energyLosses'], first[k]['energyLosses']) for k in range(K))
