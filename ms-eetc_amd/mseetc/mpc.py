"""
Receding (shrinking) horizon re-solves on top of the batched solver -- BASELINE config 4.

The reference has no MPC loop; its mechanism for a re-solve from the current position is
`Track.updateLimits(positionStart=...)` (track.py:420-450) + a new `casadiSolver` on the cropped track +
`solve(T, initialTime=t_now, initialVelocity=v_now)` (ocp.py:310), always from a cold start (ocp.py:325-339).
This driver does exactly that for a whole batch of scenarios at once: the position sequence only depends on the
grids, so every re-solve is one problem shared by the batch and one kernel launch.
"""

import copy
from concurrent.futures import ThreadPoolExecutor

import numpy as np
from ._device import ST as _ST

from .ocp import casadiSolver


def transferSolution(z, positionsOld, positionsNew, withPnBrake):
    """
    Move solutions z (B, nz_old), laid out as ocp.py:166-272 on the grid `positionsOld`, onto the grid `positionsNew`
    (same length unit and origin, covered by the old grid): states t and b = v^2 are interpolated linearly in position,
    the piecewise-constant controls and slacks are taken from the old interval that contains the midpoint of the new
    one.  Used to warm-start a re-solve on a shorter horizon.  Returns (B, nz_new).
    """

    z = np.atleast_2d(np.asarray(z, dtype=float))
    pOld = np.asarray(positionsOld, dtype=float)
    pNew = np.asarray(positionsNew, dtype=float)
    No, Nn = len(pOld) - 1, len(pNew) - 1
    pn = int(bool(withPnBrake))
    stp = 4 + pn

    if z.shape[1] != stp*No + 2:
        raise ValueError("Solution does not match the old grid!")

    # the common case of the shrinking horizon: the new grid is a tail of the old one -> a slice
    off = No - Nn
    if 0 <= off and np.allclose(pNew, pOld[off:], rtol=0, atol=1e-6):
        return np.ascontiguousarray(z[:, stp*off:])

    body = z[:, :stp*No].reshape(-1, No, stp)
    tOld = np.concatenate([body[:, :, 2 + pn], z[:, stp*No:stp*No + 1]], axis=1)
    bOld = np.concatenate([body[:, :, 3 + pn], z[:, stp*No + 1:stp*No + 2]], axis=1)

    k = np.clip(np.searchsorted(pOld, pNew, side='right') - 1, 0, No - 1)
    w = np.clip((pNew - pOld[k])/(pOld[k + 1] - pOld[k]), 0.0, 1.0)
    tNew = tOld[:, k]*(1 - w) + tOld[:, k + 1]*w
    bNew = bOld[:, k]*(1 - w) + bOld[:, k + 1]*w

    mid = 0.5*(pNew[:-1] + pNew[1:])
    km = np.clip(np.searchsorted(pOld, mid, side='right') - 1, 0, No - 1)

    out = np.empty((z.shape[0], stp*Nn + 2))
    nb = out[:, :stp*Nn].reshape(-1, Nn, stp)
    nb[:, :, :2 + pn] = body[:, km, :2 + pn]
    nb[:, :, 2 + pn] = tNew[:, :Nn]
    nb[:, :, 3 + pn] = bNew[:, :Nn]
    out[:, stp*Nn] = tNew[:, Nn]
    out[:, stp*Nn + 1] = bNew[:, Nn]

    return out


def _restrictionSets(speedRestrictions, B, K, velocityMin, positionsFirst):
    """
    Speed restrictions of a loop (include/mseetc_mpc.h), validated like casadiSolver._restrictions: a sequence of B sequences of
    (begin [m], end [m], velocity [m/s][, firstResolve]) in route coordinates (0: the first node of the first grid), or one such sequence for every
    scenario; firstResolve (default 0) is the re-solve from which the restriction is known.  Returns a list of B lists of 4-tuples of floats.
    `K` re-solves, `positionsFirst` the nodes of the first grid.
    """

    from . import _device

    sets = list(speedRestrictions)
    def record(e):
        try:
            return len(e) in (_device.RS_COUNT, _device.MPC_RS_COUNT) and all(np.ndim(x) == 0 for x in e)
        except TypeError:
            return False

    def records(one):
        try:
            return all(record(e) for e in one)
        except TypeError:
            return False

    if all(record(e) for e in sets):      # (one sequence of restrictions -- an empty one too -- for the whole batch)
        sets = [sets]*B
    if not all(records(one) for one in sets):
        raise ValueError("Speed restrictions are given as (begin [m], end [m], velocity [m/s][, firstResolve])!")
    if len(sets) != B:
        raise ValueError("{} sets of speed restrictions for a batch of {} scenarios!".format(len(sets), B))
    if max([len(one) for one in sets], default=0) > _device.RS_MAX:
        raise ValueError("At most {} speed restrictions per scenario!".format(_device.RS_MAX))

    pos = np.asarray(positionsFirst, dtype=float)
    out = []
    for s, one in enumerate(sets):
        recs = []
        for j, rec in enumerate(one):
            begin, end, velocity = [float(x) for x in rec[:3]]
            first = float(rec[3]) if len(rec) == _device.MPC_RS_COUNT else 0.0
            if not np.all(np.isfinite([begin, end, velocity, first])):
                raise ValueError("Speed restriction {} of scenario {} is not finite!".format(j, s))
            if end <= begin:
                raise ValueError("Speed restriction {} of scenario {} ends at or before its beginning!".format(j, s))
            if velocity <= 0 or velocity*velocity <= float(velocityMin)**2:
                raise ValueError("Speed restriction {} of scenario {} is not above the minimum velocity!".format(j, s))
            if first != np.floor(first) or not 0 <= first <= K - 1:
                raise ValueError("Speed restriction {} of scenario {} is not known from a re-solve 0 ... {}!".format(j, s, K - 1))
            if not ((pos[:-1] < end) & (pos[1:] > begin)).any():
                raise ValueError("Speed restriction {} of scenario {} restricts no interval of the first grid!".format(j, s))
            recs.append((begin, end, velocity, first))
        out.append(recs)

    return out


def _restrictionsOfResolve(sets, k, origin, positions):
    """
    The restrictions (begin, end, velocity) of re-solve k in the coordinates of its grid, per scenario: the records of _restrictionSets that are known by
    re-solve k, moved by the route coordinate `origin` of the grid's first node (one rounded subtraction each), without those that restrict no interval
    of the grid any more (`positions`: its nodes, first one 0) -- a restriction wholly behind the train.  What casadiSolver.solveBatch / restrictedLimits take.
    """

    pos = np.asarray(positions, dtype=float)
    origin = float(origin)
    out = []
    for one in sets:
        keep = []
        for begin, end, velocity, first in one:
            if first > k:
                continue
            b, e = begin - origin, end - origin
            if ((pos[:-1] < e) & (pos[1:] > b)).any():
                keep.append((b, e, velocity))
        out.append(keep)

    return out


def _rollingStock(train, B, mass, r0, r1, r2, plantMass, plantR0, plantR1, plantR2, plantSteps):
    """
    Rolling stock of a loop (include/mseetc_mpc.h: msd_mpc_rolling_stock), validated: the model's `mass`, `r0`, `r1`, `r2` as casadiSolver.solveBatch takes them
    (SI units, scalars or one value per scenario; None: the train's) and the plant's -- the train that actually runs; a plant value that is not given is the
    scenario's model value.  Returns (model, plant): `model` a dict of (B,) arrays mass, r0, r1, r2, or None when none of them is given; `plant` the
    (B, MPC_PL['COUNT']) rows (specific Davis coefficients of the plant, force_scale = M_model/M_plant), or None when no plant value is given.
    """

    from ._device import MPC_PL, MPC_PLANT_STEPS_MAX

    def full(a, default, what):
        a = np.asarray(default if a is None else a, dtype=float)
        if a.ndim > 1 or (a.ndim == 1 and a.shape[0] not in (1, B)):
            raise ValueError("{} of {} scenarios for a batch of {}!".format(what, a.shape[0] if a.ndim == 1 else a.shape, B))
        return np.broadcast_to(a, (B,)).copy()

    given = [a is not None for a in (mass, r0, r1, r2)]
    m = dict(mass=full(mass, train.mass, 'mass'), r0=full(r0, train.r0, 'r0'), r1=full(r1, train.r1, 'r1'), r2=full(r2, train.r2, 'r2'))
    if not all(np.all(np.isfinite(a)) for a in m.values()) or np.any(m['mass'] <= 0) or any(np.any(m[k] < 0) for k in ('r0', 'r1', 'r2')):
        raise ValueError("Train mass must be positive and rolling resistance coefficients non-negative!")

    plant = None
    if any(a is not None for a in (plantMass, plantR0, plantR1, plantR2)):
        if int(plantSteps) != plantSteps or not 1 <= int(plantSteps) <= MPC_PLANT_STEPS_MAX:
            raise ValueError("plantSteps must be 1 ... {}!".format(MPC_PLANT_STEPS_MAX))
        pm, p0, p1, p2 = (full(plantMass, m['mass'], 'plantMass'), full(plantR0, m['r0'], 'plantR0'), full(plantR1, m['r1'], 'plantR1'),
                          full(plantR2, m['r2'], 'plantR2'))
        if not all(np.all(np.isfinite(a)) for a in (pm, p0, p1, p2)) or np.any(pm <= 0) or np.any(p0 < 0) or np.any(p1 < 0) or np.any(p2 < 0):
            raise ValueError("Plant mass must be positive and its rolling resistance coefficients non-negative!")
        M = pm*train.rho
        plant = np.zeros((B, MPC_PL['COUNT']))
        plant[:, MPC_PL['SR0']], plant[:, MPC_PL['SR1']], plant[:, MPC_PL['SR2']] = p0/M, p1/M, p2/M
        plant[:, MPC_PL['FORCE_SCALE']] = (m['mass']*train.rho)/M

    return (m if any(given) else None), plant


def _plantAdvance(points, withPnBrake, g, rho, vminSq, z, t0, v0sq, plantRows, plantSteps, stride):
    "plantAdvance behind the solver: `points` the grid frame (computeDiscretizationPoints), g and rho the train's, vminSq the square of the minimum velocity."

    from ._device import MPC_PL

    z = np.atleast_2d(np.asarray(z, dtype=float))
    rows = np.atleast_2d(np.asarray(plantRows, dtype=float))
    B = z.shape[0]
    pn = int(bool(withPnBrake))
    stp = 4 + pn
    pos = points.index.values.astype(float)
    ds = np.diff(pos)
    grad = points['Gradient [permil]'].values.astype(float)/1e3
    curv = np.abs(points['Curvature [1/m]'].values.astype(float))
    sr0, sr1, sr2, scale = rows[:, MPC_PL['SR0']], rows[:, MPC_PL['SR1']], rows[:, MPC_PL['SR2']], rows[:, MPC_PL['FORCE_SCALE']]
    t = np.broadcast_to(np.asarray(t0, dtype=float), (B,)).copy()
    b = np.broadcast_to(np.asarray(v0sq, dtype=float), (B,)).copy()
    stalled = np.zeros(B, dtype=bool)
    n = int(plantSteps)
    h = 1.0/n

    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        for i in range(int(stride)):
            c = curv[i]
            cr = g*0.5*c/(1 - 30*c) if c <= 1.0/300.0 else g*0.65*c/(1 - 55*c)      # train.py:252-253
            G = g*grad[i]*(1/rho) + cr*(1/rho)
            w = (z[:, stp*i] + (z[:, stp*i + 1] if pn else 0.0))*scale
            fb = lambda x: ((w - (sr0 + (np.sqrt(x)*sr1 + x*sr2))) - G)*(2*ds[i])      # d(b)/d(sigma) on the unit interval (train.py:251-259)
            ft = lambda x: ds[i]/np.sqrt(x)                                             # d(t)/d(sigma)
            bi, tau = b.copy(), np.zeros(B)
            for _ in range(n):
                k1b, k1t = fb(bi), ft(bi)
                b2 = bi + k1b*(0.5*h)
                k2b, k2t = fb(b2), ft(b2)
                b3 = bi + k2b*(0.5*h)
                k3b, k3t = fb(b3), ft(b3)
                b4 = bi + k3b*h
                k4b, k4t = fb(b4), ft(b4)
                bi = bi + ((k1b + k2b*2.0) + (k3b*2.0 + k4b))*(h/6)
                tau = tau + ((k1t + k2t*2.0) + (k3t*2.0 + k4t))*(h/6)
            stalled |= ~stalled & (~(bi >= vminSq) | ~np.isfinite(tau))      # (a NaN fails the comparison)
            t = np.where(stalled, t, t + tau)
            b = np.where(stalled, b, bi)

    return t, np.sqrt(b), stalled


def plantAdvance(solver, z, t0, v0sq, plantRows, plantSteps, stride):
    """
    The plant of a loop advances `stride` intervals of the solver's grid: the numpy statement of csrc/msd_mpc.hip: mpc_plant, the definition the device is held to.
    From the re-solve's own initial state (`t0` (B,), `v0sq` (B,): t0 and the clipped v0^2 of its scenario records) under the planned forces of its solutions
    `z` (B, nz): interval i < stride runs under w_i = (Fel_i + Fpb_i) force_scale through explicit Runge-Kutta of 4th order in the space domain, `plantSteps` steps,
    time and b = v^2 integrated jointly (the interval map of the solver with numSteps = plantSteps, numApproxSteps = 0), with the plant's specific Davis
    coefficients of `plantRows` (B, MPC_PL['COUNT']) and the train's g and rho.  After an interval, b+ < vmin^2 (or a NaN, or a running time that is not finite) marks
    the scenario stalled: it stays at the state in front of that interval.  Returns (t (B,), v (B,), stalled (B,) bool), before any noise.
    """

    return _plantAdvance(solver.points, solver.withPnBrake, solver.train.g, solver.train.rho, float(solver.velocityMin)**2, z, t0, v0sq, plantRows, plantSteps, stride)


KWH = 1e-6/3.6      # Nm -> kWh (utils.py:243)
ENERGY_KEYS = ('traction', 'regenerated', 'pnBrake', 'losses')


def _plantEnergy(points, withPnBrake, g, rho, vminSq, z, t0, v0sq, plantRows, steps, n, totalMass, modelRows, lossKind, ct, cr, lossFun):
    """
    plantEnergy behind the solver: `points` the grid frame, g and rho the train's, vminSq the square of the minimum velocity, modelRows (B, >= 3) the specific
    Davis coefficients of the scenarios' models, lossKind 0 / 1 / 2 (utils.LOSS_*) with the slopes ct, cr (B,) of kind 1 and the callable L(F [N], v) [W] of kind 2.
    """

    from ._device import MPC_PL
    from .utils import LOSS_STATIC, LOSS_DYNAMIC

    z = np.atleast_2d(np.asarray(z, dtype=float))
    B = z.shape[0]
    pn = int(bool(withPnBrake))
    stp = 4 + pn
    pos = points.index.values.astype(float)
    ds = np.diff(pos)
    N = len(ds)
    n = int(n)
    if not 0 <= n <= N or z.shape[1] != stp*N + 2:
        raise ValueError("A leg of {} intervals on a plan of {} ({} variables)!".format(n, N, z.shape[1]))
    grad = points['Gradient [permil]'].values.astype(float)/1e3
    curv = np.abs(points['Curvature [1/m]'].values.astype(float))
    M = np.broadcast_to(np.asarray(totalMass, dtype=float), (B,))
    withPlant = plantRows is not None
    rows = np.atleast_2d(np.asarray(plantRows if withPlant else modelRows, dtype=float))
    sr0, sr1, sr2 = rows[:, MPC_PL['SR0']], rows[:, MPC_PL['SR1']], rows[:, MPC_PL['SR2']]
    scale = rows[:, MPC_PL['FORCE_SCALE']] if withPlant else 1.0
    table = lossKind == LOSS_DYNAMIC
    t = np.broadcast_to(np.asarray(t0, dtype=float), (B,)).copy()
    b = np.broadcast_to(np.asarray(v0sq, dtype=float), (B,)).copy()
    stalled = np.zeros(B, dtype=bool)
    done = np.zeros(B, dtype=int)
    acc = {key: np.zeros(B) for key in ENERGY_KEYS}      # [Nm]
    m = int(steps)
    h = 1.0/m

    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        for i in range(n):
            fel = z[:, stp*i]
            fpb = z[:, stp*i + 1] if pn else np.zeros(B)
            F, Fpn = fel*M, fpb*M
            lossE = np.zeros(B)
            if withPlant or table:
                c = curv[i]
                cres = g*0.5*c/(1 - 30*c) if c <= 1.0/300.0 else g*0.65*c/(1 - 55*c)      # train.py:252-253
                G = g*grad[i]*(1/rho) + cres*(1/rho)
                w = (fel + fpb)*scale
                fb = lambda x: ((w - (sr0 + (np.sqrt(x)*sr1 + x*sr2))) - G)*(2*ds[i])      # (_plantAdvance's)
                ft = lambda x: ds[i]/np.sqrt(x)

                def fe(x):
                    "d(E)/d(sigma) [Nm] on the unit interval: ds L(F, v)/v"
                    v = np.sqrt(x)
                    return np.array([ds[i]*lossFun(F[s], v[s])/v[s] for s in range(B)]) if table else np.zeros(B)

                bi = b.copy() if withPlant else z[:, stp*i + stp - 1].copy()      # (without a plant every interval restarts from the plan's own b_i)
                tau = np.zeros(B)
                for _ in range(m):
                    k1b, k1t, k1e = fb(bi), ft(bi), fe(bi)
                    b2 = bi + k1b*(0.5*h)
                    k2b, k2t, k2e = fb(b2), ft(b2), fe(b2)
                    b3 = bi + k2b*(0.5*h)
                    k3b, k3t, k3e = fb(b3), ft(b3), fe(b3)
                    b4 = bi + k3b*h
                    k4b, k4t, k4e = fb(b4), ft(b4), fe(b4)
                    bi = bi + ((k1b + k2b*2.0) + (k3b*2.0 + k4b))*(h/6)
                    tau = tau + ((k1t + k2t*2.0) + (k3t*2.0 + k4t))*(h/6)
                    lossE = lossE + ((k1e + k2e*2.0) + (k3e*2.0 + k4e))*(h/6)
                if withPlant:
                    stalled |= ~stalled & (~(bi >= vminSq) | ~np.isfinite(tau))      # (_plantAdvance's rule)
                    t = np.where(stalled, t, t + tau)
                    b = np.where(stalled, b, bi)
            if lossKind == LOSS_STATIC:
                lossE = ds[i]*(ct*np.maximum(F, 0.0) + cr*np.maximum(-F, 0.0))      # (the speed cancels: train.py:199-212)
            go = ~stalled
            done += go
            acc['traction'] += np.where(go, ds[i]*np.maximum(F, 0.0), 0.0)
            acc['regenerated'] += np.where(go, ds[i]*np.minimum(F, 0.0), 0.0)
            acc['pnBrake'] += np.where(go, ds[i]*Fpn, 0.0)
            acc['losses'] += np.where(go, lossE, 0.0)

    if not withPlant:      # the plan's node n, read
        node = stp*n + (stp - 2 if n < N else 0)
        t, b = z[:, node].copy(), z[:, node + 1].copy()
    out = {key: a*KWH for key, a in acc.items()}
    out.update(t=t, v=np.sqrt(b), intervals=done, stalled=stalled)

    return out


def _etaSlopes(eta, B):
    "(ct, cr) (B,) of (B, 2) efficiencies etaTraction, etaRgBrake (train.py:199-212), validated"

    eta = np.asarray(eta, dtype=float)
    if eta.shape != (B, 2) or not np.all(np.isfinite(eta)) or np.any(eta <= 0) or np.any(eta > 1):
        raise ValueError("Plant efficiencies are given as ({}, 2) values in (0, 1]!".format(B))
    return (1 - eta[:, 0])/eta[:, 0], 1 - eta[:, 1]


def plantEnergy(solver, z, t0, v0sq, plantRows, steps, n, totalMass, eta=None, modelRows=None):
    """
    The energy account of one leg of a loop: the numpy statement of csrc/msd_mpc.hip: mpc_energy, the definition the device is held to (include/mseetc_mpc.h:
    msd_mpc_energy).  The first `n` intervals of the plans `z` (B, nz) on the solver's grid, per scenario; forces in newtons are the plan's specific forces times
    `totalMass` (scalar or (B,): mass rho of the scenario's MODEL -- the plant's traction equipment receives the commanded newtons whatever the plant weighs).
    With `plantRows` (B, MPC_PL['COUNT']) the speed trajectory is plantAdvance's, from (`t0`, `v0sq`) with the same arithmetic, stall rule and bits: a stall ends the
    leg in front of the interval that stalled it, and what was spent up to there counts.  With plantRows None the plan is the plant: every interval restarts from
    the plan's own b_i, integrated with the model's specific Davis coefficients (`modelRows` (B, >= 3); None: the solver's train) and force_scale 1 -- what the
    reference's post-processing does per interval (utils.py:261-289) -- and the state at the end is the plan's node n, read.
    Per interval, summed over the intervals completed (reference: utils.py:243-257, :291): traction ds max(F_el, 0), regenerated ds min(F_el, 0), pnBrake ds F_pn, and
    losses: with constant efficiencies (the train's, or `eta` (B, 2): etaTraction, etaRgBrake of the PLANT) ds (ct max(F, 0) + cr max(-F, 0)) with ct = (1 - eta_t)/eta_t,
    cr = 1 - eta_r, in closed form (the speed cancels); with a loss table (efficiency.DynamicLosses / TabulatedLosses, no eta) the integral of L(F_el, v)/v over the
    interval as a third component of the same Runge-Kutta steps, k_E(x) = ds L(F, sqrt(x))/sqrt(x) at the four stage values of b, combined like the running time;
    without a loss model and without eta 0.
    Returns a dict: traction, regenerated, pnBrake, losses [kWh] (B,), t, v (B,) the state at the end of the leg (before any noise), intervals (B,) completed, stalled (B,).
    """

    from .utils import classifyLosses, LOSS_STATIC, LOSS_DYNAMIC

    z = np.atleast_2d(np.asarray(z, dtype=float))
    B = z.shape[0]
    train = solver.train
    if int(steps) != steps or not 1 <= int(steps) <= 64:
        raise ValueError("steps must be 1 ... 64!")
    if eta is not None:
        kind, fun = LOSS_STATIC, None
        ct, cr = _etaSlopes(eta, B)
    else:
        fun = train.lossesCallable()
        kind, ct, cr = classifyLosses(fun)
    if modelRows is None:
        Mt = train.mass*train.rho
        modelRows = np.repeat(np.array([[train.r0/Mt, train.r1/Mt, train.r2/Mt]]), B, axis=0)
    M = np.broadcast_to(np.asarray(totalMass, dtype=float), (B,))
    if not np.all(np.isfinite(M)) or np.any(M <= 0):
        raise ValueError("totalMass must be positive!")

    return _plantEnergy(solver.points, solver.withPnBrake, train.g, train.rho, float(solver.velocityMin)**2, z, t0, v0sq, plantRows, steps, n, M, modelRows,
                        kind, ct, cr, fun if kind == LOSS_DYNAMIC else None)


def _energyAccount(train, B, energyAccount, plantEtaTraction, plantEtaRgBrake):
    """
    (account, eta): whether a loop keeps the energy account, and the (B, 2) efficiencies of the plants or None.  `plantEtaTraction`, `plantEtaRgBrake` (scalars or
    one value per scenario, in (0, 1]) imply the account; one that is not given is the train's.  Validated like plantMass.
    """

    if plantEtaTraction is None and plantEtaRgBrake is None:
        return bool(energyAccount), None
    eta = np.zeros((B, 2))
    for j, (a, name) in enumerate(((plantEtaTraction, 'etaTraction'), (plantEtaRgBrake, 'etaRgBrake'))):
        if a is None:
            if getattr(train, name, None) is None:
                raise ValueError("The train has no {}: give both efficiencies of the plant!".format(name))
            a = getattr(train, name)
        a = np.asarray(a, dtype=float)
        if a.ndim > 1 or (a.ndim == 1 and a.shape[0] not in (1, B)):
            raise ValueError("plant {} of {} scenarios for a batch of {}!".format(name, a.shape[0] if a.ndim == 1 else a.shape, B))
        eta[:, j] = np.broadcast_to(a, (B,))
    _etaSlopes(eta, B)

    return True, eta


def _legRecord(leg, active):
    "the log's keys of one leg: a scenario that is not advanced (its re-solve failed, or it stalled earlier) has a zero record with 0 intervals"

    out = {'energy' + key[0].upper() + key[1:]: np.where(active, leg[key], 0.0) for key in ENERGY_KEYS}
    out['legIntervals'] = np.where(active, leg['intervals'], 0)
    return out


def closedLoopEnergy(log):
    """
    The energy the closed loop drew, from the log of a loop run with `energyAccount` (shrinkingHorizon, DeviceLoop.run): per scenario `total` (traction +
    regenerated + losses: what the objective prices) and the four components [kWh], summed over the legs -- `stride` intervals behind every re-solve but the last,
    the whole plan behind the last --, `arrivalTime` [s] and `arrivalVelocity` [m/s] (the state at the end of the last leg), and `complete`: every leg ran its full
    interval count (False for a scenario whose re-solve failed or whose plant stalled: its account ends there).
    Read `complete` with the totals.  With a plant and plans that brake to the minimum velocity at the platform (the default terminal velocity of 1 m/s is the
    minimum velocity) the plant usually falls below the minimum in the last interval, and the stall rule ends the final leg in front of it: `complete` is False, and
    `total`, `arrivalTime` and `arrivalVelocity` are those of the state in front of that interval -- one interval short of the platform -- not of the arrival.
    """

    if not log or 'energyTraction' not in log[0]:
        raise ValueError("The log holds no energy account (energyAccount=True)!")
    out = {key: sum(r['energy' + key[0].upper() + key[1:]] for r in log) for key in ENERGY_KEYS}
    out['total'] = out['traction'] + out['regenerated'] + out['losses']
    out['arrivalTime'], out['arrivalVelocity'] = log[-1]['tArrival'].copy(), log[-1]['vArrival'].copy()
    K = len(log)
    full = [r['numIntervals'] - log[k + 1]['numIntervals'] if k < K - 1 else r['numIntervals'] for k, r in enumerate(log)]      # (stride; the whole last plan)
    out['complete'] = np.all([r['legIntervals'] == full[k] for k, r in enumerate(log)], axis=0)

    return out


class DeviceLoop():
    """
    The shrinking-horizon loop with its bookkeeping on the device (csrc/msd_mpc.hip, include/mseetc_mpc.h): the grid sequence does not depend
    on the solutions, so the problem records of all re-solves are built and uploaded once (here), and `run` executes a whole loop -- measured
    states, scenario records, warm starts, the handling of arrival times that can no longer be met, the log -- as launches on one stream
    without the host in between.  Same loop as shrinkingHorizon(); reusable for any number of batches of arrival times.
    """

    def __init__(self, train, track, optsDict, numResolves, stride=2, noise=0.0, terminalVelocity=1.0, device=0, warmStart=False, warmPush=1e-3,
                 dualMu=1e-4, relaxInfeasible=True, lateMargin=5e-3, deferDevice=False):

        from . import _device

        N = int(optsDict.get('numIntervals', 100))
        current = copy.deepcopy(track)
        position = 0.0
        self.solvers, self.twins, self.positions = [], [], []
        tail, previous = [], None
        for k in range(numResolves):
            Nk = N - stride*k
            if Nk < 1:
                break
            opts = dict(optsDict); opts['numIntervals'] = Nk
            # (no restoration phase, like shrinkingHorizon: a re-solve that fails is certified and relaxed by the loop itself; no watchdog procedure for the same
            #  reason -- a re-solve that crawls through ten shortened iterations would leave the fused iteration for the follow-up kernel, and a launch lasts as
            #  long as its slowest scenario.  On config 4 it makes no measurable difference either way)
            solver = casadiSolver(train, current, opts, device=device, restoration=False, watchdogTrigger=-1)
            self.solvers.append(solver)
            if relaxInfeasible:
                topts = dict(opts); topts['energyOptimal'] = False; topts.pop('integrateLosses', None)
                self.twins.append(casadiSolver(train, current, topts, device=device, startingPoint='profile', restoration=False, watchdogTrigger=-1))
            pos = position + solver.points.index.values
            tail.append(int(previous is not None and len(previous) - len(pos) == stride and np.allclose(pos, previous[stride:], rtol=0, atol=1e-6)))
            self.positions.append(pos)
            previous = pos
            if Nk - stride < 1:
                break
            nxt = copy.deepcopy(current)
            nxt.updateLimits(positionStart=float(solver.points.index.values[stride]))
            position += float(solver.points.index.values[stride])
            current = nxt
        first = self.solvers[0]
        vlim = first.points['Speed limit [m/s]'].values
        self.stride, self.noise, self.K = stride, noise, len(self.solvers)
        self.energyOptimal = first.energyOptimal
        self.scale = 1.0 if first.energyOptimal else first.scalingFactorObjective
        self.withPnBrake = first.withPnBrake
        self.terminalVelocity = terminalVelocity
        # everything above is host work, and so are restrictedLimits and restrictedScenarios: with `deferDevice` the device side is created by the first run
        self._loop = None
        self._make = lambda: _device.DeviceLoop(first.problem, self.twins[0].problem if relaxInfeasible else None, [s._desc for s in self.solvers],
                                                [t._desc for t in self.twins] if relaxInfeasible else None, stride,
                                                [s.points['Speed limit [m/s]'].values[0] for s in self.solvers], [s.track.length for s in self.solvers], tail,
                                                first.velocityMin, first._vmaxTrain, min(max(terminalVelocity, first.velocityMin), vlim[-1]), warmStart, dualMu,
                                                warmPush, noise, relaxInfeasible, lateMargin)
        if not deferDevice:
            self._loop = self._make()

    @property
    def device(self):
        "The owner of the loop's device handle (_device.DeviceLoop), created on first use."

        if self._loop is None:
            self._loop = self._make()
        return self._loop

    # ---- speed restrictions inside the loop (include/mseetc_mpc.h) ------------------------------

    def _restrictionSets(self, speedRestrictions, B):
        return _restrictionSets(speedRestrictions, B, self.K, self.solvers[0].velocityMin, self.positions[0])

    def _restrictionsOfResolve(self, k, speedRestrictions, B):
        "The restrictions that count in re-solve k, per scenario, in the coordinates of grid k."

        if not 0 <= int(k) < self.K:
            raise ValueError("Re-solve {} is outside 0 ... {}!".format(k, self.K - 1))
        return _restrictionsOfResolve(self._restrictionSets(speedRestrictions, int(B)), int(k), self.positions[k][0], self.solvers[k].points.index.values)

    def restrictionRecords(self, speedRestrictions, B):
        "(origin (K,), count (B,), records (B, M, 4)): the restrictions as msd_mpc_speed_restrictions takes them (_device.DeviceLoop.speed_restrictions)."

        from ._device import MPC_RS_COUNT

        sets = self._restrictionSets(speedRestrictions, int(B))
        count = np.array([len(one) for one in sets], dtype=np.int32)
        records = np.zeros((int(B), max(1, int(count.max(initial=0))), MPC_RS_COUNT))
        for s, one in enumerate(sets):
            for j, rec in enumerate(one):
                records[s, j] = rec

        return np.array([float(p[0]) for p in self.positions]), count, records

    def restrictedLimits(self, k, speedRestrictions, B):
        """
        (B, N_k+1) upper bounds of b = v^2 of re-solve k under the loop's speed restrictions (`speedRestrictions` as in run): the numpy statement of the
        rows the device builds.  The records known by re-solve k, in the coordinates of grid k, without those behind the train; then the rule of
        casadiSolver.restrictedLimits on that grid.
        """

        now = self._restrictionsOfResolve(k, speedRestrictions, B)

        return self.solvers[k].restrictedLimits(now, int(B))

    def restrictedScenarios(self, k, terminalTime, initialTime, initialVelocity, speedRestrictions, B):
        "(B, 4) scenario records (t0, T, v0^2, vN^2) of re-solve k from the measured state: the end speeds clipped to the restricted limits per scenario (casadiSolver._scenarios)."

        now = self._restrictionsOfResolve(k, speedRestrictions, B)
        solver = self.solvers[k]
        rs = solver._restrictionsOf(solver._restrictions(now), int(B))
        scen = solver._scenarios(terminalTime, initialTime, self.terminalVelocity, initialVelocity, rs)
        return np.broadcast_to(scen, (int(B), scen.shape[1])).copy()

    def run(self, terminalTime, seed=0, initialTime=0.0, initialVelocity=1.0, keepZ=True, speedRestrictions=None, mass=None, r0=None, r1=None, r2=None,
            plantMass=None, plantR0=None, plantR1=None, plantR2=None, plantSteps=8, energyAccount=False, plantEtaTraction=None, plantEtaRgBrake=None):
        """
        One loop; returns the log of shrinkingHorizon() (list of dicts per re-solve; 'z' None without keepZ) -- `loop_ms` in every entry is the device time of the whole loop.
        `energyAccount`: the energy the closed loop really spends, kept on the device (msd_mpc_energy; plantEnergy is its statement): every log entry gains
        'energyTraction', 'energyRegenerated', 'energyPnBrake', 'energyLosses' [kWh] and 'legIntervals' of the leg driven behind its re-solve (`stride` intervals;
        behind the last re-solve the whole remaining plan), the last entry also 'tArrival', 'vArrival': with a plant the plant's arrival, without one the plan's.
        closedLoopEnergy(log) sums them.  `plantEtaTraction`, `plantEtaRgBrake` (in (0, 1], scalars or one value per scenario): a plant whose efficiencies are not
        the model's; they imply the account and change no plan.  Without a plant the loss integral of a loss table takes `plantSteps` Runge-Kutta steps per interval.
        `speedRestrictions`: a sequence of B sequences of (begin [m], end [m], velocity [m/s][, firstResolve]), or one such sequence for every scenario --
        restrictions in route coordinates (0: the first node of the first grid) that are known from re-solve `firstResolve` on (default 0): from then on the
        scenario's re-solves run under restrictedLimits(k, ...), their end speeds clipped to the restricted limits; a restriction the train has passed is
        ignored.  ValueError: a record that is not finite, ends at or before its beginning, restricts no interval of the first grid, is not above the minimum
        velocity or names no re-solve of the loop; more than 16 per scenario; a wrong batch length.  The records are the loop's for this run only.
        `mass`, `r0`, `r1`, `r2` (SI units, scalars or one value per scenario): the scenarios' own rolling stock, as in casadiSolver.solveBatch -- what the controller
        believes its train to be, in every re-solve, the minimum running times included.  `plantMass`, `plantR0`, `plantR1`, `plantR2`: the train that actually runs
        (a value that is not given is the scenario's model value).  With any of them the state a re-solve starts from is no longer read from the previous plan: the
        plant is integrated under the planned forces (plantAdvance, `plantSteps` Runge-Kutta steps per interval), and the log entries in front of the last one gain
        'tPlant', 'vPlant' (the plant's state behind the advance, before the noise) and 'stalled' (the plant fell below the minimum velocity in this or an earlier
        advance: the scenario keeps its last measurement).  ValueError: values the library refuses, plantSteps outside 1 ... 64, a wrong batch length.
        """

        from ._device import MPC, MPC_PS, MPC_EN, MPC_PLANT_STEPS_MAX

        T = np.array(np.atleast_1d(np.asarray(terminalTime, dtype=float)), copy=True)
        B = T.shape[0]
        account, eta = _energyAccount(self.solvers[0].train, B, energyAccount, plantEtaTraction, plantEtaRgBrake)
        if account and (int(plantSteps) != plantSteps or not 1 <= int(plantSteps) <= MPC_PLANT_STEPS_MAX):
            raise ValueError("plantSteps must be 1 ... {}!".format(MPC_PLANT_STEPS_MAX))
        sets = self._restrictionSets(speedRestrictions, B) if speedRestrictions is not None else None
        rng = np.random.default_rng(seed)
        n1, n2 = np.zeros((max(self.K - 1, 0), B)), np.zeros((max(self.K - 1, 0), B))
        for k in range(self.K - 1):      # (the order of shrinkingHorizon's draws)
            n1[k], n2[k] = rng.standard_normal(B), rng.standard_normal(B)
        model, plant = _rollingStock(self.solvers[0].train, B, mass, r0, r1, r2, plantMass, plantR0, plantR1, plantR2, plantSteps)
        rows = self.solvers[0]._overrides(B, model['mass'], model['r0'], model['r1'], model['r2']) if model is not None else None      # (the rule of solveBatch)
        restricted = sets is not None and any(sets)
        states, legs = None, None
        if restricted or rows is not None or plant is not None or account:
            try:
                if restricted:
                    self.device.speed_restrictions(*self.restrictionRecords(sets, B))
                if rows is not None or plant is not None:
                    self.device.rolling_stock(rows, plant, plantSteps)
                if account:
                    train = self.solvers[0].train
                    self.device.energy(B, train.mass*train.rho, eta, plantSteps)
                log, zs, ms = self.device.run(T, initialTime, initialVelocity, n1, n2, keepZ=keepZ)
                if plant is not None and self.K > 1:
                    states = self.device.plant_states()
                if account:
                    legs = self.device.energy_records()
            finally:
                self.device.energy(None)
                self.device.rolling_stock(None)
                self.device.speed_restrictions(None)
        else:      # (no scenario is restricted or has a train of its own: the plain loop)
            log, zs, ms = self.device.run(T, initialTime, initialVelocity, n1, n2, keepZ=keepZ)
        out = []
        for k in range(self.K):
            r = log[k]
            out.append(dict(position=float(self.positions[k][0]), numIntervals=self.solvers[k].numIntervals, t0=r[:, MPC['T0']].copy(), v0=r[:, MPC['V0']].copy(),
                            T=r[:, MPC['T']].copy(), status=r[:, MPC['STATUS']].astype(int), iterations=r[:, MPC['ITERS']].astype(int),
                            cost=r[:, MPC['OBJ']]*self.scale, z=zs[k] if zs is not None else None, relaxed=r[:, MPC['RELAXED']] > 0,
                            kernel_ms=ms/self.K, loop_ms=ms))
            if states is not None and k < self.K - 1:
                out[-1].update(tPlant=states[k, :, MPC_PS['T']].copy(), vPlant=states[k, :, MPC_PS['V']].copy(), stalled=states[k, :, MPC_PS['STALLED']] > 0)
            if legs is not None:
                e = legs[k]
                out[-1].update(energyTraction=e[:, MPC_EN['TRACTION']].copy(), energyRegenerated=e[:, MPC_EN['REGENERATED']].copy(),
                               energyPnBrake=e[:, MPC_EN['PNBRAKE']].copy(), energyLosses=e[:, MPC_EN['LOSSES']].copy(), legIntervals=e[:, MPC_EN['INTERVALS']].astype(int))
                if k == self.K - 1:
                    out[-1].update(tArrival=e[:, MPC_EN['T']].copy(), vArrival=e[:, MPC_EN['V']].copy())
        return out

    def close(self):

        if getattr(self, '_loop', None) is not None:
            self._loop.close()
            self._loop = None
        for s in self.solvers + self.twins:
            s.close()
        self.solvers, self.twins = [], []


def shrinkingHorizon(train, track, optsDict, terminalTime, numResolves, stride=2, noise=0.0, seed=0,
                     initialTime=0.0, initialVelocity=1.0, terminalVelocity=1.0, device=0, solverFactory=None,
                     warmStart=False, warmMu=1e-2, warmPush=1e-3, dualMu=1e-4, relaxInfeasible=True, lateMargin=5e-3, onDevice=False,
                     speedRestrictions=None, mass=None, r0=None, r1=None, r2=None, plantMass=None, plantR0=None, plantR1=None, plantR2=None, plantSteps=8,
                     energyAccount=False, plantEtaTraction=None, plantEtaRgBrake=None):
    """
    Re-solve `numResolves` times; after each solve the train advances `stride` intervals of the current grid, the
    measured time and speed at that node are perturbed by `noise` (relative, standard normal) and the remaining
    horizon (stride intervals shorter) is solved again -- from a cold start like the reference, or with
    `warmStart=True` from the previous solution moved onto the new grid -- on the device when the new grid is the tail of the old
    one (msd_solve_batch_shifted: primal point and multipliers, barrier parameter `dualMu`), through transferSolution otherwise (primal
    point only, `warmMu`); a warm start that breaks down is repeated cold inside the launch.

    A re-solve that fails because the measured state no longer allows the arrival time (near the end of the horizon a
    late measurement leaves less than the minimum running time) is repeated with the arrival time moved to the scenario's certified
    minimum running time from there (casadiSolver.minimumTime, plus `lateMargin` relative): the train arrives late and keeps
    being controlled (`relaxInfeasible`; off: such a scenario keeps its last measurement).  The moved arrival time stays for the
    rest of the horizon; 'relaxed' in the log marks the scenarios it was applied to.

    terminalTime: array (B,) of arrival times (absolute).
    Returns a list of dicts per re-solve: position [m], numIntervals, t0 (B,), v0 (B,), T (B,), status, iterations, cost, z, relaxed (B,) bool.
    `solverFactory(train, track, opts)` lets tests substitute the solver (default: the device solver).

    `speedRestrictions`: restrictions per scenario that become known while the train is under way -- a sequence of B sequences of
    (begin [m], end [m], velocity [m/s][, firstResolve]) in route coordinates (0: the start of `track`), or one such sequence for every scenario; as in
    DeviceLoop.run.  From re-solve `firstResolve` on the scenario is solved under the restriction (casadiSolver.solveBatch(speedRestrictions=...) on the grid
    of the re-solve), its minimum running time is the one under the restriction, and a restriction the train has passed is ignored.  A substituted solver
    must accept the keyword `speedRestrictions` in solveBatch.

    `mass`, `r0`, `r1`, `r2`: the scenarios' own rolling stock (casadiSolver.solveBatch) in every re-solve and in the minimum running times; `plantMass`,
    `plantR0`, `plantR1`, `plantR2`, `plantSteps`: the train that actually runs, as in DeviceLoop.run -- with any of them the measured state comes from plantAdvance
    under the planned forces instead of the plan, and the log entries in front of the last one gain 'tPlant', 'vPlant' and 'stalled'.  A substituted solver must
    accept the keywords `mass`, `r0`, `r1`, `r2` in solveBatch when any of them is given, and with a plant return its (B, 4) scenario records as 'scenarios'.

    `energyAccount`, `plantEtaTraction`, `plantEtaRgBrake`: the energy the closed loop really spends, as in DeviceLoop.run -- computed here with plantEnergy on the
    solutions of every re-solve, so that the two loops stay comparable: the log entries gain 'energyTraction', 'energyRegenerated', 'energyPnBrake', 'energyLosses',
    'legIntervals', the last one 'tArrival', 'vArrival' (closedLoopEnergy sums them).
    """

    if onDevice:
        # the same loop with its bookkeeping on the device (DeviceLoop): one call, no host work between the launches
        if solverFactory is not None:
            raise ValueError("onDevice runs the device solver!")
        loop = DeviceLoop(train, track, optsDict, numResolves, stride=stride, noise=noise, terminalVelocity=terminalVelocity, device=device, warmStart=warmStart,
                          warmPush=warmPush, dualMu=dualMu, relaxInfeasible=relaxInfeasible, lateMargin=lateMargin)
        try:
            return loop.run(terminalTime, seed=seed, initialTime=initialTime, initialVelocity=initialVelocity, speedRestrictions=speedRestrictions,
                            mass=mass, r0=r0, r1=r1, r2=r2, plantMass=plantMass, plantR0=plantR0, plantR1=plantR1, plantR2=plantR2, plantSteps=plantSteps,
                            energyAccount=energyAccount, plantEtaTraction=plantEtaTraction, plantEtaRgBrake=plantEtaRgBrake)
        finally:
            loop.close()

    # (no restoration phase: a re-solve that fails is certified and relaxed below, and a launch lasts as long as its slowest scenario)
    make = solverFactory or (lambda tr, tk, op: casadiSolver(tr, tk, op, device=device, restoration=False, watchdogTrigger=-1))

    T = np.array(np.atleast_1d(np.asarray(terminalTime, dtype=float)), copy=True)
    B = T.shape[0]
    rng = np.random.default_rng(seed)
    model, plant = _rollingStock(train, B, mass, r0, r1, r2, plantMass, plantR0, plantR1, plantR2, plantSteps)
    own = (lambda idx=slice(None): {key: a[idx] for key, a in model.items()}) if model is not None else (lambda idx=None: {})
    stalled = np.zeros(B, dtype=bool)
    account, eta = _energyAccount(train, B, energyAccount, plantEtaTraction, plantEtaRgBrake)
    if plant is not None or account:
        from .ocp import OptionsCasadiSolver
        vminPlant = float(OptionsCasadiSolver(optsDict).minimumVelocity)
    if account:
        # the account of every leg: plantEnergy on the re-solve's solutions (include/mseetc_mpc.h: msd_mpc_energy)
        from ._device import MPC_PLANT_STEPS_MAX
        from .utils import classifyLosses, LOSS_STATIC, LOSS_DYNAMIC
        if int(plantSteps) != plantSteps or not 1 <= int(plantSteps) <= MPC_PLANT_STEPS_MAX:      # (without a plant: the steps of the table's loss integral)
            raise ValueError("plantSteps must be 1 ... {}!".format(MPC_PLANT_STEPS_MAX))
        if eta is not None:
            lossModel = (LOSS_STATIC,) + _etaSlopes(eta, B) + (None,)
        else:
            lossModel = classifyLosses(train.lossesCallable())
            lossModel = lossModel + (train.lossesCallable() if lossModel[0] == LOSS_DYNAMIC else None,)
        own0 = model if model is not None else dict(mass=np.full(B, float(train.mass)), r0=np.full(B, float(train.r0)), r1=np.full(B, float(train.r1)), r2=np.full(B, float(train.r2)))
        massModel = own0['mass']*train.rho
        rowsModel = np.stack([own0['r0']/massModel, own0['r1']/massModel, own0['r2']/massModel], axis=1)

    N = int(optsDict.get('numIntervals', 100))
    t_now = np.full(B, float(initialTime))
    v_now = np.full(B, float(initialVelocity))
    position = 0.0
    current = copy.deepcopy(track)
    previous = None
    batchOnDevice = False      # the handle's last launch solved the whole batch (its solutions are what a shifted warm start reads)
    last = None
    log = []

    # The sequence of positions, grids and problem descriptions does not depend on the solutions: while the device solves re-solve k a
    # worker thread prepares problem k + 1 (crop of the track, grid, description -- pandas work that releases the interpreter while the
    # main thread waits inside the launch).  Only with the device solver; a substituted factory is called in line.
    pool = ThreadPoolExecutor(max_workers=1) if solverFactory is None else None

    def prepare(trackNow, Nk):
        "(solver for Nk intervals on trackNow, track after the train has advanced `stride` intervals or None)"
        opts = dict(optsDict)
        opts['numIntervals'] = Nk
        solver = make(train, trackNow, opts)
        nxt = None
        if Nk - stride >= 1:
            nxt = copy.deepcopy(trackNow)
            nxt.updateLimits(positionStart=float(solver.points.index.values[stride]))
        return solver, nxt

    pending = None

    try:
        for k in range(numResolves):

            Nk = N - stride*k

            if Nk < 1:
                break

            solver, following = pending.result() if pending is not None else prepare(current, Nk)
            pending = None
            if pool is not None and following is not None and k + 1 < numResolves:
                pending = pool.submit(prepare, following, Nk - stride)

            if hasattr(solver, 'adoptDevice'):
                solver.adoptDevice(last)      # same device handle for every re-solve
                twin = last.__dict__.pop('_twin', None) if last is not None else None
                if twin is not None:
                    if solver.__dict__.get('_twin') is None and hasattr(twin, 'adoptDevice'):
                        # the time-optimal twin of the previous problem hands its device handle to the twin of this one
                        opts = dict(solver._optsDict); opts['energyOptimal'] = False; opts.pop('integrateLosses', None)
                        solver._twin = type(solver)(solver.train, solver.track, opts, device=solver._device, startingPoint='profile', restoration=solver.restoration).adoptDevice(twin)
                    twin.close()
                if warmStart and solverFactory is None:
                    solver.problem.keep_duals(True)      # the multipliers of every solve stay on the device for the next re-solve
                    solver.problem.direct_results(False)      # ... and so do the solutions: the shifted warm start reads them there

            common = dict(initialTime=t_now, terminalVelocity=terminalVelocity, initialVelocity=v_now, **own())

            setsNow = None
            if speedRestrictions is not None:
                # the restrictions known by now, in the coordinates of this grid, without those behind the train (include/mseetc_mpc.h)
                if k == 0:
                    from .ocp import OptionsCasadiSolver
                    numSolves = sum(1 for j in range(numResolves) if N - stride*j >= 1)
                    sets = _restrictionSets(speedRestrictions, B, numSolves, OptionsCasadiSolver(optsDict).minimumVelocity, solver.points.index.values)
                setsNow = _restrictionsOfResolve(sets, k, position + solver.points.index.values[0], solver.points.index.values)
                common['speedRestrictions'] = setsNow

            posNew = position + solver.points.index.values
            tail = (warmStart and previous is not None and batchOnDevice and hasattr(solver, 'adoptDevice') and solverFactory is None and
                    len(previous[1]) - len(posNew) == stride and np.allclose(posNew, previous[1][stride:], rtol=0, atol=1e-6))

            if tail:
                # the new grid is the tail of the old one and the previous solutions are still on the device (same handle): the re-solve
                # warm-starts from them there -- no upload, and scenarios without a usable guess start cold inside the same launch
                res = solver.solveBatch(T, shift=stride, warmMu=dualMu, warmPush=warmPush, classifyFailures=False, **common)
                batchOnDevice = True
            elif warmStart and previous is not None:
                zPrev, posPrev, okPrev = previous
                guess = transferSolution(zPrev, posPrev, position + solver.points.index.values, solver.withPnBrake)
                usable = okPrev & np.isfinite(guess).all(axis=1)
                if usable.any():
                    # scenarios without a usable guess get another scenario's solution as a placeholder: a warm start that breaks down is
                    # repeated from the problem's own starting point inside the launch (solve_kernel), so no second launch is needed
                    if not usable.all():
                        guess[~usable] = guess[np.flatnonzero(usable)[0]]
                    res = solver.solveBatch(T, guess=guess, warmMu=warmMu, warmPush=warmPush, classifyFailures=False, **common)
                else:
                    res = solver.solveBatch(T, classifyFailures=False, **common)
                batchOnDevice = True
            else:
                res = solver.solveBatch(T, classifyFailures=False, **common)
                batchOnDevice = True

            relaxed = np.zeros(B, dtype=bool)
            kernel_extra = 0.0
            bad = np.flatnonzero(res['status'] < 0)
            if relaxInfeasible and bad.size and hasattr(solver, 'minimumTime'):
                # what stops these scenarios is their arrival time: the minimum running time from the measured state (time-optimal twin of
                # this re-solve's problem) tells, and becomes the new arrival time where it is later than the one asked for
                ovBad = dict(overrides=solver._overrides(bad.size, **own(bad))) if model is not None else {}      # (minimumTime gives the rows the twin's own objective scaling)
                if setsNow is None:
                    scenBad = solver._scenarios(T[bad], t_now[bad], terminalVelocity, v_now[bad])
                    tmin, okMin = solver.minimumTime(scenBad, **ovBad)
                else:
                    setsBad = [setsNow[i] for i in bad]
                    scenBad = solver._scenarios(T[bad], t_now[bad], terminalVelocity, v_now[bad], solver._restrictions(setsBad))
                    tmin, okMin = solver.minimumTime(scenBad, speedRestrictions=setsBad, **ovBad)
                late = okMin & (tmin > (T[bad] - t_now[bad]))
                if late.any():
                    idx, tm = bad[late], tmin[late]
                    relaxed[idx] = True
                    margin = lateMargin
                    for attempt in range(3):
                        # (an interior-point solve needs some room above the minimum running time: a scenario that still breaks down gets four times the margin)
                        T[idx] = t_now[idx] + tm*(1 + margin)
                        under = {} if setsNow is None else dict(speedRestrictions=[setsNow[i] for i in idx])
                        again = solver.solveBatch(T[idx], initialTime=t_now[idx], terminalVelocity=terminalVelocity, initialVelocity=v_now[idx], classifyFailures=False, **under,
                                                  **own(idx))
                        for key in ('z', 'status', 'iterations', 'cost'):
                            res[key][idx] = again[key]
                        kernel_extra += float(again.get('kernel_ms', 0.0))
                        still = again['status'] < 0
                        if not still.any():
                            break
                        idx, tm, margin = idx[still], tm[still], 4*margin
                    batchOnDevice = False      # the handle's last launch held these scenarios only: the next re-solve takes its guess from the host copy

            previous = (res['z'], position + solver.points.index.values, res['status'] >= 0)

            log.append(dict(position=position, numIntervals=Nk, t0=t_now.copy(), v0=v_now.copy(), T=T.copy(), status=res['status'].copy(),
                            iterations=res['iterations'].copy(), cost=res['cost'].copy(), z=res['z'], relaxed=relaxed,
                            kernel_ms=float(res.get('kernel_ms', 0.0)) + kernel_extra,
                            # (inertia corrections of the main launch's solves, where the solver reports its statistics: the device solver)
                            regularisations=(res['stats'][:, _ST['N_REG']].astype(int) if 'stats' in res else None)))

            last = solver

            def scenariosNow():
                "the scenario records of this re-solve (its clipped v0^2, under the restrictions of this re-solve): what a plant starts from"
                if 'scenarios' in res:
                    return np.asarray(res['scenarios'])
                if hasattr(solver, '_scenarios'):
                    return solver._scenarios(T, t_now, terminalVelocity, v_now, solver._restrictions(setsNow) if setsNow is not None else None)
                raise ValueError("With a plant a substituted solver returns its scenario records as 'scenarios' from solveBatch!")

            if account:
                # the leg driven behind this re-solve: `stride` intervals, behind the last re-solve the whole plan (no noise, nothing measured any more)
                final = k + 1 >= numResolves or Nk - stride < 1
                active = (res['status'] >= 0) & ~stalled      # (a scenario whose re-solve failed or that stalled earlier is not advanced: a zero record)
                if active.any():
                    zLeg = np.where(active[:, None], res['z'], res['z'][np.flatnonzero(active)[0]])      # (the rows that are not advanced are not read)
                    leg = _plantEnergy(solver.points, solver.withPnBrake, train.g, train.rho, vminPlant**2, zLeg, t_now, scenariosNow()[:, 2] if plant is not None else v_now*v_now,
                                       plant, plantSteps, Nk if final else stride, massModel, rowsModel, *lossModel)
                else:
                    leg = dict({key: np.zeros(B) for key in ENERGY_KEYS}, t=np.zeros(B), v=np.zeros(B), intervals=np.zeros(B, dtype=int))
                log[-1].update(_legRecord(leg, active))
                if final:
                    log[-1].update(tArrival=np.where(active, leg['t'], 0.0), vArrival=np.where(active, leg['v'], 0.0))

            if Nk - stride < 1:
                break

            # state at node `stride` of this grid (layout ocp.py:376-405): t and b of stage `stride`
            stp = 4 + int(solver.withPnBrake)
            t_meas = res['z'][:, stp*stride + 2 + int(solver.withPnBrake)]
            v_meas = np.sqrt(res['z'][:, stp*stride + 3 + int(solver.withPnBrake)])

            # failed scenarios keep coasting on their last measurement
            ok = res['status'] >= 0
            n1, n2 = rng.standard_normal(B), rng.standard_normal(B)
            if plant is not None and k + 1 < numResolves:      # (behind the last re-solve nothing is measured any more)
                # the train that runs is the plant, not the plan: from the re-solve's own initial state under the planned forces (include/mseetc_mpc.h: msd_mpc_rolling_stock)
                # (its clipped v0^2: the scenario records of the solve, under the restrictions of this re-solve)
                scenNow = scenariosNow()
                tP, vP, now = _plantAdvance(solver.points, solver.withPnBrake, train.g, train.rho, vminPlant**2, res['z'], t_now, scenNow[:, 2], plant, plantSteps, stride)
                moved = ok & ~stalled      # (a scenario whose re-solve failed or that has stalled keeps its last measurement: its record holds that)
                stalled = stalled | (moved & now)
                log[-1].update(tPlant=np.where(moved, tP, t_now), vPlant=np.where(moved, vP, v_now), stalled=stalled.copy())
                t_meas, v_meas, ok = tP, vP, moved & ~now
            t_now = np.where(ok, np.maximum(t_meas*(1 + noise*n1), 0.0), t_now)
            v_now = np.where(ok, v_meas*(1 + noise*n2), v_now)

            position += float(solver.points.index.values[stride])
            current = following

    finally:
        # also on an exception in a solve or a reconfigure: no worker thread (building the next problem on the shared train) is left behind
        if pool is not None:
            pool.shutdown(wait=True, cancel_futures=True)

    if last is not None and hasattr(last, 'close'):
        last.close()

    return log
