"""
Round 11, the first passes of the fused family on the host emulation: the default kernels hold one integrator (numSteps = 1, numApprox = 1: msd_kernel.hpp,
Solver::FIXED_INTEG).  The emulation is built twice from the same sources: as shipped, and with -DMSD_RUNTIME_INTEGRATOR=1, which restores the kernels of round 10.
Both must compute the same bits.  (The second part of the round, the sums of the first iteration in a pass in front of the loop with its switch
-DMSD_MERIT_IN_LOOP, was measured and taken out: profiles/r11/README.md.  It passed these tests with both switches set in the second build.)

Which first pass a launch takes is the rule of msd_select.hpp (first_pass_twin), which the library's launch code and the driver of these tests share
(tests/hip_emu/emu_k_first_pass.cpp, with the twins of tests/hip_emu/emu_k_full_early.cpp: a library of the fused family alone, built through UNITS of
tests/hip_emu/build.sh; the emulation's default build and its driver are untouched).
"""
import ctypes
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

import cases

EMU = Path(__file__).resolve().parent / 'hip_emu'
ROOT = EMU.parent.parent
MAX_ITER = 300
SWITCHES = '-DMSD_RUNTIME_INTEGRATOR=1'


UNITS = 'emu_driver emu_k_full emu_k_full_early emu_k_first_pass'
DEFAULT_FIRST, NO_FOLLOW = 1, 2      # flags of emu_first_pass_solve


def _load(so, objdir, extra):
    "Build (when out of date) and load one emulation library; both go through tests/hip_emu/build.sh, same compiler, same flags but `extra`."
    src = sorted(EMU.glob('*.cpp')) + sorted(EMU.glob('*.h')) + [EMU / 'build.sh', EMU / 'hip' / 'hip_runtime.h'] \
        + sorted((ROOT / 'ms-eetc_amd' / 'csrc').glob('*.hpp')) + [ROOT / 'include' / 'mseetc_hip.h']
    if not so.exists() or so.stat().st_mtime < max(f.stat().st_mtime for f in src):
        env = dict(os.environ, OUT=str(so), OBJDIR=str(objdir), EXTRA=extra, UNITS=UNITS)
        env.pop('SAN', None)
        subprocess.run([str(EMU / 'build.sh')], check=True, env=env)
    from mseetc._device import ProblemDesc
    lib = ctypes.CDLL(str(so))
    dp = ctypes.POINTER(ctypes.c_double)
    lib.emu_first_pass_solve.argtypes = [ctypes.POINTER(ProblemDesc), ctypes.c_int, dp, dp, dp, dp, ctypes.c_double, ctypes.c_double, dp, dp, dp, ctypes.c_int,
                                         ctypes.POINTER(ctypes.c_int)]
    return lib


@pytest.fixture(scope='module')
def builds():
    "(shipped, run-time integrator) emulation libraries of the fused family in one process"
    return (_load(EMU / 'libmsd_emu_r11.so', EMU / 'obj_r11', ''),
            _load(EMU / 'libmsd_emu_r11_rtinteg.so', EMU / 'obj_r11_rtinteg', SWITCHES))


def _d(a):
    return None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def _solve(lib, solver, scen, guess=None, duals=None, mu0=0.0, push=0.0, flags=0):
    """
    one scenario: (z, multipliers, stats record without its time stamps, multipliers for a warm start,
    dict(twin, part, geometry, full, follow: PART of the follow-up kernel that ran or 0, why: scenarios handed over by reason))
    """
    from mseetc._device import ST
    from oracle import oracle
    N = solver.numIntervals
    nz = (4 + int(solver.withPnBrake))*N + 2
    z, lam, st = np.zeros((1, nz)), np.zeros((1, 7*N)), np.full((1, ST['COUNT']), np.nan)
    out = np.zeros((N + 1, oracle.DUAL_STRIDE))
    scen = np.ascontiguousarray(scen, dtype=np.float64)
    info = (ctypes.c_int*16)()
    assert lib.emu_first_pass_solve(ctypes.byref(solver._desc), 1, _d(scen), _d(guess), _d(duals), _d(out), mu0, push, _d(z), _d(lam), _d(st), flags, info) == 0
    st[0, ST['CYC_TOTAL']] = st[0, ST['CYC_KKT']] = 0      # (time stamps)
    return z[0], lam[0], st[0], out, dict(twin=bool(info[0]), part=info[1], geometry=(info[2], info[3]), full=info[4], follow=info[5], why=list(info[8:16]))


def _solver(train, track, N, start='profile', steps=(1, 1), maxIterations=MAX_ITER):
    from mseetc.ocp import casadiSolver
    return casadiSolver(train, track, dict(numIntervals=N, maxIterations=maxIterations, integrationOptions=dict(numSteps=steps[0], numApproxSteps=steps[1])), startingPoint=start)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


# ---- the rule ----

PAIRS = [(1, 1), (2, 1), (1, 2), (1, 0)]


@pytest.fixture(scope='module')
def rule(tmp_path_factory):
    "msd_host::first_pass_twin through a small program of its own (tests/hip_emu/unit/first_pass_twin.cpp): no emulation library needed"
    exe = tmp_path_factory.mktemp('unit') / 'first_pass_twin'
    subprocess.run(['g++', '-std=c++17', '-O1', '-pthread', '-I', str(EMU), '-o', str(exe), str(EMU / 'unit' / 'first_pass_twin.cpp')], check=True)

    def twin(fused_family, early, steps, approx):
        return int(subprocess.run([str(exe)] + [str(int(v)) for v in (fused_family, early, steps, approx)], check=True, capture_output=True, text=True).stdout)
    return twin


@pytest.mark.parametrize('steps,approx', PAIRS)
def test_which_first_pass_a_launch_takes(rule, steps, approx):
    compiled = (steps, approx) == (1, 1)
    assert bool(rule(1, 0, steps, approx)) == (not compiled)      # fused family: the default kernel for the compiled-in integrator only
    assert rule(1, 1, steps, approx) == 1                         # early results (begun batch, iteration budget): always the twin
    assert rule(0, 0, steps, approx) == 0                         # another family: its kernels choose at run time, each is its own twin
    assert rule(0, 1, steps, approx) == 1


# ---- same bits as the kernels of round 10 ----
# (train, crop of track 00, N, T, geometry of the first pass).  N = 2, 30 and 100 with both brakes are cases of tests/test_structural_masks_emulation.py; the others
# were screened the same way: the oracle converges on each.  Every case runs from the profile start and then, from its own solution and multipliers, as a
# primal-dual warm start (barrier parameter 1e-4, push 1e-3: the re-solves of the shrinking-horizon loop).
CASES = [('both', 1500, 2, 160.0, (64, 1)), ('both', 4000, 7, 260.0, (64, 1)), ('both', 12000, 30, 520.0, (64, 1)), ('both', None, 100, 1541.0, (64, 2)),
         ('fig10', 1500, 2, 200.0, (64, 1)), ('fig10', 4000, 7, 300.0, (64, 1)), ('fig10', 12000, 30, 650.0, (64, 1)), ('fig10', None, 100, 1700.0, (64, 2))]


@pytest.mark.parametrize('variant,crop,N,T,geometry', CASES)
def test_the_shipped_first_pass_computes_the_bits_of_round_10(builds, variant, crop, N, T, geometry):
    from mseetc._device import ST
    shipped, r10 = builds
    train = cases.train_default() if variant == 'both' else cases.train_fig10()
    solver = _solver(train, cases.track_00(crop), N)
    scen = solver._scenarios(T, 0, 1, 1)
    za, la, sa, da, ka = _solve(shipped, solver, scen)
    zb, lb, sb, db, kb = _solve(r10, solver, scen)
    print('N %d %s, profile start: status %g after %g iterations, %g inertia corrections' % (N, variant, sa[ST['STATUS']], sa[ST['ITERS']], sa[ST['N_REG']]))
    assert ka == kb and ka['geometry'] == geometry and ka['part'] == 1 and ka['full'] == (1 if variant == 'both' else 2)
    assert not ka['twin'] and not any(ka['why'])      # the default kernel: numSteps = 1, numApprox = 1
    assert sa[ST['STATUS']] == 0
    assert _same(za, zb) and _same(la, lb) and _same(sa, sb) and _same(da, db)
    # primal-dual warm start from that solution
    zc, lc, sc, dc, kc = _solve(shipped, solver, scen, guess=za, duals=da, mu0=1e-4, push=1e-3)
    zd, ld, sd, dd, kd = _solve(r10, solver, scen, guess=za, duals=da, mu0=1e-4, push=1e-3)
    print('N %d %s, primal-dual warm start: status %g after %g iterations, %g inertia corrections' % (N, variant, sc[ST['STATUS']], sc[ST['ITERS']], sc[ST['N_REG']]))
    assert kc == kd and kc['part'] == 1 and not kc['twin']
    assert sc[ST['STATUS']] == 0
    assert _same(zc, zd) and _same(lc, ld) and _same(sc, sd) and _same(dc, dd)


def test_the_first_pass_behind_the_multiplier_estimate_too(builds):
    "PART = 3 (the reference's starting point) is a kernel with the compiled-in integrator as well"
    from mseetc._device import ST
    shipped, r10 = builds
    solver = _solver(cases.train_default(), cases.track_00(12000), 30, start='reference')
    scen = solver._scenarios(520.0, 0, 1, 1)
    za, la, sa, da, ka = _solve(shipped, solver, scen)
    zb, lb, sb, db, kb = _solve(r10, solver, scen)
    assert ka == kb and ka['part'] == 3 and not ka['twin'] and sa[ST['STATUS']] == 0
    assert _same(za, zb) and _same(la, lb) and _same(sa, sb) and _same(da, db)


def test_an_inertia_correction_on_the_way(builds):
    """
    A wrong inertia repeats the pass over the same point with delta_w on the diagonal (`iter--; continue`).  The one-brake train on the two-interval crop, from
    the reference's starting point, meets it five times (N_REG), at later iterations.  A correction *at iteration 0* was looked for and not found among the small
    cases: with an iteration limit of 1 a solve ends behind iteration 0, so N_REG then counts the corrections made there -- it was 0 in 168 solves: every case of
    this file from both starting points, their primal-dual warm starts at barrier parameters 1e-4, 1e-2 and 1e-1, and the N = 2 and N = 7 crops of both trains
    over 16 running times each from both starting points.
    """
    from mseetc._device import ST
    shipped, r10 = builds
    solver = _solver(cases.train_fig10(), cases.track_00(1500), 2, start='reference')
    scen = solver._scenarios(240.0, 0, 1, 1)
    za, la, sa, da, ka = _solve(shipped, solver, scen)
    zb, lb, sb, db, kb = _solve(r10, solver, scen)
    print('status %g after %g iterations, %g inertia corrections' % (sa[ST['STATUS']], sa[ST['ITERS']], sa[ST['N_REG']]))
    assert ka == kb and ka['part'] == 3 and ka['full'] == 2 and not ka['twin']
    assert sa[ST['STATUS']] == 0 and sa[ST['N_REG']] >= 1 and not any(ka['why'])      # corrected inside the fused loop, not handed over
    assert _same(za, zb) and _same(la, lb) and _same(sa, sb) and _same(da, db)


# ---- another integrator ----

@pytest.mark.parametrize('steps', [(2, 1), (1, 2)])
def test_another_integrator_takes_the_twin_and_the_default_kernel_hands_it_over(builds, steps):
    """
    A problem with another integrator runs in the twin, in both builds the same bits (the twin keeps the run-time choice).  The default kernel forced onto it
    hands the scenario over with reason 0 and the follow-up kernel ends where the run-time build ends: status 0, objective 1e-8 relative, variables 1e-6 (the
    device-vs-oracle bounds of DESIGN section 3 -- the follow-up kernel runs the general iteration, not the same arithmetic).
    """
    from mseetc._device import ST
    shipped, r10 = builds
    solver = _solver(cases.train_default(), cases.track_00(12000), 30, steps=steps)
    scen = solver._scenarios(520.0, 0, 1, 1)
    za, la, sa, da, ka = _solve(shipped, solver, scen)
    zb, lb, sb, db, kb = _solve(r10, solver, scen)
    assert ka == kb and ka['full'] == 1 and ka['part'] == 1 and ka['twin']
    assert sa[ST['STATUS']] == 0 and not any(ka['why'])
    assert _same(za, zb) and _same(la, lb) and _same(sa, sb)
    zc, lc, sc, dc, kc = _solve(shipped, solver, scen, flags=DEFAULT_FIRST)
    print('default kernel forced: handed over by reason', kc['why'], 'status', sc[ST['STATUS']], 'iterations', sc[ST['ITERS']], 'against', sb[ST['ITERS']])
    assert not kc['twin'] and kc['part'] == 1 and kc['follow'] == 2
    assert kc['why'] == [1, 0, 0, 0, 0, 0, 0, 0]
    assert sc[ST['STATUS']] == 0
    assert abs(sc[ST['OBJ']] - sb[ST['OBJ']]) <= 1e-8*abs(sb[ST['OBJ']])
    assert np.max(np.abs(zc - zb)/np.maximum(1, np.abs(zb))) <= 1e-6
    # the run-time build's default kernel solves it itself: no guard there
    zd, ld, sd, dd, kd = _solve(r10, solver, scen, flags=DEFAULT_FIRST)
    assert not kd['twin'] and not any(kd['why']) and _same(zd, zb) and _same(sd, sb)
    # without the follow-up kernel the shipped build leaves the record as the caller left it
    ze, le, se, de, ke = _solve(shipped, solver, scen, flags=DEFAULT_FIRST | NO_FOLLOW)
    assert ke['follow'] == 0 and ke['why'][0] == 1 and np.all(np.isnan(se[[ST['STATUS'], ST['ITERS'], ST['OBJ']]])) and not np.any(ze)
