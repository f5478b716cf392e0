"""
The lane predicates "variable k of node j is free" of the fused passes (msd_kernel.hpp: Solver::on) come from the compiled-in structure, not from the
flag word.  Host emulation of the kernels, built twice from the same sources: as shipped, and with -DMSD_FLAG_WORD_MASKS=1, which restores the flag-word
predicates in the FAST kernels.  On regular problems the two builds compute the same bits; on problems whose data fix a variable the structure has free
the shipped build hands the scenario to the follow-up kernel (reason 0) and ends where the flag-word build ends.
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


def _load(so, objdir, extra):
    "Build (when out of date) and load one emulation library; both go through tests/hip_emu/build.sh, same compiler, same flags but `extra`."
    src = sorted(EMU.glob('*.cpp')) + sorted(EMU.glob('*.h')) + [EMU / 'build.sh', EMU / 'hip' / 'hip_runtime.h'] \
        + sorted((ROOT / 'ms-eetc_amd' / 'csrc').glob('*.hpp')) + [ROOT / 'include' / 'mseetc_hip.h']
    if not so.exists() or so.stat().st_mtime < max(f.stat().st_mtime for f in src):
        env = dict(os.environ, OUT=str(so), OBJDIR=str(objdir), EXTRA=extra)
        env.pop('SAN', None)
        subprocess.run([str(EMU / 'build.sh')], check=True, env=env)
    from mseetc._device import ProblemDesc
    lib = ctypes.CDLL(str(so))
    dp = ctypes.POINTER(ctypes.c_double)
    lib.emu_solve_batch_ex.argtypes = [ctypes.POINTER(ProblemDesc), ctypes.c_int, dp, dp, dp, dp, dp, dp, ctypes.c_int]
    lib.emu_last_kernels.restype = ctypes.c_char_p
    return lib


@pytest.fixture(scope='module')
def builds():
    "(shipped, flag-word) emulation libraries in one process"
    return (_load(EMU / 'libmsd_emu.so', EMU / 'obj', ''),
            _load(EMU / 'libmsd_emu_flagword.so', EMU / 'obj_flagword', '-DMSD_FLAG_WORD_MASKS=1'))


def _d(a):
    return None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def _kernels(lib):
    "the template arguments of the kernels the last call ran: dict(first=[NT, SPT, WPS, DYN, STREAM, GEN, FULL, PART, SLDS, SOCK], follow=[...])"
    return {name: [int(v) for v in ids.split(',')] for name, ids in (f.split('=') for f in lib.emu_last_kernels().decode().split())}


def _solve(lib, solver, scen, ovr=None):
    from mseetc._device import ST
    N = solver.numIntervals
    nz = (4 + int(solver.withPnBrake))*N + 2
    z, lam, st, hist = np.zeros((1, nz)), np.zeros((1, 7*N)), np.full((1, ST['COUNT']), np.nan), np.zeros((8, 8))
    scen = np.ascontiguousarray(scen, dtype=np.float64)
    assert lib.emu_solve_batch_ex(ctypes.byref(solver._desc), 1, _d(scen), _d(ovr), _d(z), _d(lam), _d(st), _d(hist), 8) == 0
    st[0, ST['CYC_TOTAL']] = st[0, ST['CYC_KKT']] = 0      # (time stamps)
    return z[0], lam[0], st[0], _kernels(lib)


def _solver(train, track, N, start='profile'):
    from mseetc.ocp import casadiSolver
    return casadiSolver(train, track, dict(numIntervals=N, maxIterations=MAX_ITER, integrationOptions=dict(numSteps=1, numApproxSteps=1)), startingPoint=start)


# (train, crop of track 00, N, T, start, geometry NT x SPT of the first pass, its PART, its FULL).  The running times were chosen with the oracle: it converges
# on each (the shortest crops need a loose schedule to be feasible at all).  One-brake train: at T = 520, the running time of the neighbouring cases, both
# builds take 19 iterations where the oracle takes 17 -- the known extra barrier reduction that tests/test_kernel_emulation.py allows its one-brake cases
# (two iterations), not a matter of the lane masks; T = 650 has none
REGULAR = [('both', 2000, 3, 170.0, 'profile', (64, 2), 1, 1), ('both', 3000, 5, 190.0, 'profile', (64, 2), 1, 1),
           ('both', 13000, 33, 600.0, 'profile', (64, 2), 1, 1), ('both', None, 100, 1541.0, 'profile', (64, 2), 1, 1),
           ('both', 1500, 2, 160.0, 'profile', (64, 1), 1, 1), ('both', 8000, 17, 400.0, 'profile', (64, 1), 1, 1),
           ('both', None, 200, 1541.0, 'profile', (128, 2), 1, 1), ('fig10', 12000, 30, 650.0, 'profile', (64, 1), 1, 2),
           ('both', 12000, 30, 520.0, 'reference', (64, 1), 3, 1),
           # a second-order correction on the way (tests/test_kernel_emulation.py::test_emulated_kernel_matches_oracle)
           ('both', 16000, 40, 804.9041795334854, 'profile', (64, 1), 1, 1)]


def _geometry_env(monkeypatch, N, geometry):
    "the 64 x 2 cases of up to 63 intervals: the ladder alone would give them 64 x 1"
    if geometry == (64, 2) and N + 1 <= 64:
        monkeypatch.setenv('EMU_GEOMETRY', '64x2')


@pytest.mark.parametrize('variant,crop,N,T,start,geometry,part,full', REGULAR)
def test_structural_masks_compute_the_flag_word_bits(builds, monkeypatch, variant, crop, N, T, start, geometry, part, full):
    from mseetc._device import ST
    from oracle import oracle
    shipped, flagword = builds
    _geometry_env(monkeypatch, N, geometry)
    train = cases.train_default() if variant == 'both' else cases.train_fig10()
    track = cases.track_00(crop)
    solver = _solver(train, track, N, start)
    scen = solver._scenarios(T, 0, 1, 1)
    za, la, sa, ka = _solve(shipped, solver, scen)
    zb, lb, sb, kb = _solve(flagword, solver, scen)
    assert ka == kb and tuple(ka['first'][:2]) == geometry and ka['first'][7] == part and ka['first'][6] == full
    assert np.array_equal(za, zb) and np.array_equal(la, lb) and np.array_equal(sa, sb)
    prob = cases.oracle_problem(train, track, N, maxIterations=MAX_ITER)
    ref = oracle.solve(prob, prob.scenario(T), start=start)
    print('N %d %s: iterations %d (oracle %d), z %.3e, multipliers %.3e' % (
        N, variant, sa[ST['ITERS']], ref['stats']['ITERS'], np.max(np.abs(za - ref['z'])/np.maximum(1, np.abs(ref['z']))),
        np.max(np.abs(la[:len(ref['lam_g'])] - ref['lam_g'])/np.maximum(1, np.abs(ref['lam_g'])))))
    assert sa[ST['STATUS']] == 0 and ref['stats']['STATUS'] == 0
    assert int(sa[ST['ITERS']]) == int(ref['stats']['ITERS'])
    assert np.max(np.abs(za - ref['z'])/np.maximum(1, np.abs(ref['z']))) < 1e-8
    assert np.max(np.abs(la[:len(ref['lam_g'])] - ref['lam_g'])/np.maximum(1, np.abs(ref['lam_g']))) < 1e-7


# ---- problems whose data fix a variable that the structure has free ----
# What the oracle and the flag-word build do with them was looked at on the CPU before the tests were written: no running time (t0 == tEnd) and a pneumatic
# brake without force both end with a negative status in the oracle and in the flag-word build (line-search failure, -2, after 36 ... 108 iterations).  The
# tests still carry both branches the issue states: where the flag-word build converges, the shipped build must reach the same optimum (status 0, objective
# 1e-8 relative, variables 1e-6: the device-vs-oracle bounds of DESIGN section 3); where it ends negative, so must the shipped build, within the iteration
# limit.  ITERS counts both attempts of a solve that was repeated from the other starting point (mseetc/_device.py), so the limit of 300 shows there as 600.

GUARD = [(5, 3000, 190.0), (30, 12000, 520.0)]


def _guarded(builds, monkeypatch, solver, scen, ovr=None):
    "a scenario the first pass must hand over: both builds, and the shipped one without its follow-up kernel"
    from mseetc._device import ST
    shipped, flagword = builds
    za, la, sa, ka = _solve(shipped, solver, scen, ovr)
    zb, lb, sb, kb = _solve(flagword, solver, scen, ovr)
    print('shipped: status %g after %g iterations; flag words: status %g after %g iterations' % (sa[ST['STATUS']], sa[ST['ITERS']], sb[ST['STATUS']], sb[ST['ITERS']]))
    assert ka == kb and ka['first'][6] == 1 and ka['first'][7] == 1 and ka['follow'][7] == 2      # the fused first pass and its follow-up kernel
    if sb[ST['STATUS']] >= 0:
        assert sa[ST['STATUS']] == 0
        assert abs(sa[ST['OBJ']] - sb[ST['OBJ']]) <= 1e-8*abs(sb[ST['OBJ']])
        assert np.max(np.abs(za - zb)/np.maximum(1, np.abs(zb))) <= 1e-6
    else:
        assert sa[ST['STATUS']] < 0 and sa[ST['ITERS']] <= 2*MAX_ITER
    # the handover: without the follow-up kernel the scenario's record stays as the caller left it
    monkeypatch.setenv('EMU_NO_FOLLOW', '1')
    z0, l0, s0, k0 = _solve(shipped, solver, scen, ovr)
    assert k0['follow'][0] == 0 and np.all(np.isnan(s0[[ST['STATUS'], ST['ITERS'], ST['OBJ']]])) and not np.any(z0)


@pytest.mark.parametrize('N,crop,T', GUARD)
def test_a_scenario_without_running_time_is_handed_over(builds, monkeypatch, N, crop, T):
    solver = _solver(cases.train_default(), cases.track_00(crop), N)
    scen = solver._scenarios(T, 0, 1, 1)
    scen[0, 0] = scen[0, 1]      # t0 == tEnd
    _guarded(builds, monkeypatch, solver, scen)


@pytest.mark.parametrize('N,crop,T', GUARD)
def test_an_override_without_pneumatic_brake_force_is_handed_over(builds, monkeypatch, N, crop, T):
    from mseetc._device import OV
    train = cases.train_default()
    solver = _solver(train, cases.track_00(crop), N)
    assert solver.withPnBrake
    ovr = solver._overrides(1, train.mass, None, None, None)
    ovr[0, OV['F_MIN_PN']] = 0.0      # (config 3 style: the rolling stock of the scenario)
    _guarded(builds, monkeypatch, solver, solver._scenarios(T, 0, 1, 1), ovr)


@pytest.mark.parametrize('N,crop,T', GUARD)
def test_a_speed_limit_at_the_minimum_speed_is_handed_over(builds, monkeypatch, N, crop, T):
    "cases.py crops tracks but builds no speed-limit sections: one interior bmax of the description is set to vmin_sq (a loose schedule: the train has to crawl there)"
    solver = _solver(cases.train_default(), cases.track_00(crop), N)
    bmax = np.ctypeslib.as_array(solver._desc.bmax, shape=(N + 1,))
    bmax[N//2] = solver._desc.vmin_sq
    _guarded(builds, monkeypatch, solver, solver._scenarios(1.5*T, 0, 1, 1))
