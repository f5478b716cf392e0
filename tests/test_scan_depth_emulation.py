"""
Depth of the stage-parallel KKT scans (ParallelRiccati::solve, ms-eetc_amd/csrc/msd_kernel.hpp) in the host emulation: the three scans
run ceil(log2(chunks)) levels instead of six -- the levels left out had no lane with a partner, so every result is bit for bit what it was.  Full solves
against the oracle at the smallest horizons on each side of every change of the depth -- 64 x 2: chunks 1|2, 2|3 (N = 3, 4, 5), 16|17 (33, 34), 32|33 (65, 66),
50 (100: the benchmark), 63 (127); 64 x 1: chunks 1, 16, 32, 62 -- and one horizon on two waves (N = 200, 128 x 2), where the depth is that of the fullest
wave.  Same status, same iteration count, same point as the oracle, with the bounds of tests/test_kernel_emulation.py::test_emulated_kernel_matches_oracle.
"""

import ctypes
import functools

import numpy as np
import pytest

import cases
from test_kernel_emulation import load_emulation

# (geometry, N) -> (track crop [m] or None for the whole track, running time [s]): about 400 m per interval like the cases of tests/test_kernel_emulation.py
HORIZONS_64x2 = [3, 4, 5, 33, 34, 65, 66, 100, 127]
HORIZONS_64x1 = [2, 17, 33, 63]
CASES = [('64x2', N) for N in HORIZONS_64x2] + [('64x1', N) for N in HORIZONS_64x1] + [('128x2', 200)]


def _journey(N):
    if N >= 100:
        return None, 1541.0
    crop = 400.0*N
    return crop, crop/14.0 + 60.0


@functools.lru_cache(maxsize=None)
def _solve(geometry, N):
    "one emulated solve with that geometry forced, and the oracle's"
    import os
    from mseetc.ocp import casadiSolver
    from mseetc._device import ST
    from oracle import oracle
    emu = load_emulation()
    crop, T = _journey(N)
    train, track = cases.train_default(), (cases.track_00(crop) if crop else cases.track_00())
    solver = casadiSolver(train, track, dict(numIntervals=N, maxIterations=300, integrationOptions=dict(numSteps=1, numApproxSteps=1)), startingPoint='profile')
    scen = solver._scenarios(T, 0, 1, 1)
    nz = (4 + int(solver.withPnBrake))*N + 2
    z, lam, st, hist = np.zeros((1, nz)), np.zeros((1, 7*N)), np.zeros((1, ST['COUNT'])), np.zeros((8, 8))
    d = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    old = os.environ.get('EMU_GEOMETRY')
    os.environ['EMU_GEOMETRY'] = geometry
    try:
        rc = emu.emu_solve_batch(ctypes.byref(solver._desc), 1, d(scen), d(z), d(lam), d(st), d(hist), 8)
        emu.emu_last_kernels.restype = ctypes.c_char_p
        kernels = emu.emu_last_kernels().decode()
    finally:
        if old is None:
            del os.environ['EMU_GEOMETRY']
        else:
            os.environ['EMU_GEOMETRY'] = old
    assert rc == 0
    prob = cases.oracle_problem(train, track, N)
    ref = oracle.solve(prob, prob.scenario(T), start='profile')
    return dict(st=st[0].copy(), z=z[0].copy(), lam=lam[0].copy(), ref=ref, kernels=kernels, ST=ST)


@pytest.mark.parametrize('geometry,N', CASES)
def test_emulated_scan_depths_match_oracle(geometry, N):
    r = _solve(geometry, N)
    st, ref, ST = r['st'], r['ref'], r['ST']
    NT, SPT = (int(v) for v in geometry.split('x'))
    assert r['kernels'].startswith('first=%d,%d,' % (NT, SPT)), r['kernels']
    assert st[ST['STATUS']] == 0 and ref['stats']['STATUS'] == 0
    assert int(st[ST['ITERS']]) == int(ref['stats']['ITERS'])
    assert int(st[ST['N_FALLBACK']]) == 0      # no scan broke down: every Newton system went through the stage-parallel solve
    assert np.max(np.abs(r['z'] - ref['z'])/np.maximum(1, np.abs(ref['z']))) < 1e-8
    assert np.max(np.abs(r['lam'] - ref['lam_g'])/np.maximum(1, np.abs(ref['lam_g']))) < 1e-7
