"""
What speed restrictions per scenario cost (profiles/r10/README.md): the config-1 batch (N = 100, 1024 running times) with one seeded set of restrictions per
scenario against the same batch without, through the device-resident entry point (msd_solve_batch_device: HIP events over the launches) and through the
host-buffer one (msd_solve_batch: wall clock per call, setting and clearing the rows included, as casadiSolver.solveBatch does); and the time to upload the
records and build the rows on the device for 1024 and 8192 scenarios (the events around the call include the host's checks of the records; limit_rows_kernel
alone: a kernel trace of --rows-only).

    python tools/restriction_timing.py [--steps 200] [--rows-only]      (--rows-only: the part to run under a kernel trace)
"""
import argparse
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in ('ms-eetc_amd', ''):
    sys.path.insert(0, str(ROOT / p))

import numpy as np


def random_sets(B, length, seed=20261019):
    "one or two restrictions per scenario: 300 ... 800 m long, 110 ... 130 km/h, anywhere on the line (mild: the tightest of config 1's running times leaves 60 s of reserve)"
    rng = np.random.default_rng(seed)
    sets = []
    for _ in range(B):
        one = []
        for _ in range(int(rng.integers(1, 3))):
            begin = float(rng.uniform(0, length - 1100))
            one.append((begin, begin + float(rng.uniform(300, 800)), float(rng.uniform(110, 130))/3.6))
        sets.append(one)
    return sets


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--rows-only', action='store_true')
    args = ap.parse_args()

    from mseetc import workloads as wl
    from mseetc.ocp import casadiSolver
    from mseetc._device import ST

    train, track, N = wl.config('c1')
    solver = casadiSolver(train, track, wl.options(N), startingPoint='profile')
    prob = solver.problem

    for B in (1024, 8192):
        rs = solver._restrictionsOf(solver._restrictions(random_sets(B, track.length)), B)
        prob.speed_restrictions(rs['count'], rs['records'])      # (buffers, code object)
        prob.synchronize()
        dev, wall = [], []
        for _ in range(20):
            t0 = time.perf_counter()
            prob.timer_begin()
            prob.speed_restrictions(rs['count'], rs['records'])
            dev.append(prob.timer_end())
            wall.append(1e3*(time.perf_counter() - t0))
        assert np.array_equal(prob.limit_rows(B), solver.restrictedLimits(rs, B))
        print('rows of %d scenarios (%d records, max %d per scenario): checks + upload + limit_rows_kernel %.4f ms between HIP events around the call (median of 20; min %.4f), the call %.4f ms (wall, median)'
              % (B, int(rs['count'].sum()), rs['records'].shape[1], np.median(dev), np.min(dev), np.median(wall)))
        prob.speed_restrictions(None)
    if args.rows_only:
        return

    B = 1024
    T = wl.c1_times(B)
    scen = solver._scenarios(T, 0, 1, 1)
    rs = solver._restrictionsOf(solver._restrictions(random_sets(B, track.length)), B)
    scen_rs = solver._scenarios(T, 0, 1, 1, rs)
    d_scen, d_z, d_st = prob.alloc(scen.nbytes), prob.alloc(8*prob.nz*B), prob.alloc(8*ST['COUNT']*B)

    def device_leg(restricted):
        prob.to_device(d_scen, scen_rs if restricted else scen)
        prob.speed_restrictions(rs['count'], rs['records']) if restricted else prob.speed_restrictions(None)
        for _ in range(10):
            prob.solve_batch_device(B, d_scen, d_z, None, d_st)
        prob.synchronize()
        prob.timer_begin()
        for _ in range(args.steps):
            prob.solve_batch_device(B, d_scen, d_z, None, d_st)
        ms = prob.timer_end()/args.steps
        st = np.zeros((B, ST['COUNT']))
        prob.to_host(st, d_st)
        prob.speed_restrictions(None)
        return ms, st

    def host_leg(restricted):
        def call():
            if restricted:
                prob.speed_restrictions(rs['count'], rs['records'])
            out = prob.solve_batch(scen_rs if restricted else scen)
            if restricted:
                prob.speed_restrictions(None)
            return out
        for _ in range(5):
            call()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            call()
        return 1e3*(time.perf_counter() - t0)/args.steps

    print('config-1 batch, %d scenarios, N = %d, %d launches per leg, legs alternating' % (B, N, args.steps))
    for rep in range(3):
        for restricted in (False, True):
            ms, st = device_leg(restricted)
            ok = st[:, ST['STATUS']] >= 0
            print('  msd_solve_batch_device  %-12s %.4f ms per launch  converged %d / %d  iterations mean %.2f max %d  cost mean %.3f kWh'
                  % ('restricted' if restricted else 'plain', ms, int(ok.sum()), B, st[ok, ST['ITERS']].mean(), int(st[:, ST['ITERS']].max()), st[ok, ST['OBJ']].mean()))
    for rep in range(3):
        for restricted in (False, True):
            print('  msd_solve_batch         %-12s %.4f ms per call (wall; rows set and cleared per call)' % ('restricted' if restricted else 'plain', host_leg(restricted)))
    for d in (d_scen, d_z, d_st):
        prob.free(d)
    solver.close()


if __name__ == '__main__':
    main()
