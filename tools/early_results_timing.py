"""
Diagnostic (GPU): what early results bring and what they cost (profiles/r07/early_results.txt).

    python tools/early_results_timing.py benefit [--blocking-only]
    python tools/early_results_timing.py cost [--blocking-only] [--runs 5]

benefit: the 1024 running times of bench.py's alt.dynamic_losses_N300 (figure-5 configuration, dynamic loss model, N = 300), the ones that do
    not converge included: wall time of the blocking launch with and without them, then a begun batch -- time to MSD_WAIT_FIRST_PASS, words set by
    then, time to MSD_WAIT_ALL -- without a budget and with a first-pass budget of three times the median iteration count.
cost: config 1 (1024 scenarios, N = 100): wall and kernel time of the blocking launch, and of begin + result with early results on; medians.

--blocking-only: only the calls that every library version has (the tool copied into a checkout of the parent commit times the parent with it).
Does not go through bench.py.
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ('ms-eetc_amd', '', 'tests'):
    sys.path.insert(0, os.path.join(ROOT, p))

import numpy as np

from mseetc import workloads as wl
from mseetc._device import ST
from mseetc.ocp import casadiSolver

part = sys.argv[1] if len(sys.argv) > 1 else 'benefit'
blocking_only = '--blocking-only' in sys.argv
runs = int(sys.argv[sys.argv.index('--runs') + 1]) if '--runs' in sys.argv else 5
med = lambda a: float(np.median(a))


def blocking(prob, scen, n):
    "n blocking launches behind one warm-up: (wall ms, kernel ms) of each"
    prob.solve_batch(scen)
    wall, kern = [], []
    for _ in range(n):
        t0 = time.perf_counter()
        out = prob.solve_batch(scen)
        wall.append(1e3*(time.perf_counter() - t0)); kern.append(out['kernel_ms'])
    return wall, kern, out


def begun(prob, scen, n):
    "n begun batches: ms to the end of the first pass, words set by then, ms to the end of everything, final words"
    first, seen, total = [], [], []
    for _ in range(n):
        t0 = time.perf_counter()
        pend = prob.solve_batch_begin(scen)
        mask = pend.wait_first_pass()
        first.append(1e3*(time.perf_counter() - t0)); seen.append(int(mask.sum()))
        pend.result()
        total.append(1e3*(time.perf_counter() - t0))
    return first, seen, total, pend.done.copy()


if part == 'benefit':
    from mseetc.train import Train
    from mseetc.efficiency import totalLossesFunction
    tr = Train(config={'id': 'NL_Intercity_VIRM6'})
    tr.forceMinPn = 0
    tr.powerLosses = totalLossesFunction(tr, auxiliaries=27000, etaGear=0.96)
    sv = casadiSolver(tr, wl.track_00(8500), wl.options(300))
    Td = 272.4726*(1.05 + 0.25*np.random.default_rng(20260616).random(1024))      # (bench.py: alt_workloads)
    sc = sv._scenarios(Td, 0, 100/3.6, 1)
    prob = sv.problem
    wall, kern, out = blocking(prob, sc, 3)
    st = out['stats']
    good = st[:, ST['STATUS']] >= 0
    it = st[:, ST['ITERS']]
    print('dynamic_losses_N300: %d running times, %d without a KKT point (iterations %s); median iterations of the others %d, max %d'
          % (len(Td), int((~good).sum()), it[~good].astype(int).tolist(), int(np.median(it[good])), int(it[good].max())))
    print('blocking launch, all %d: wall ms median %.2f (%s), kernel ms median %.2f' % (len(Td), med(wall), ' '.join('%.2f' % w for w in wall), med(kern)))
    scg = np.ascontiguousarray(sc[good])
    wallg, kerng, _ = blocking(prob, scg, 5)
    print('blocking launch without them (%d): wall ms median %.2f, kernel ms median %.2f' % (len(scg), med(wallg), med(kerng)))
    if not blocking_only:
        for budget in (0, 3*int(np.median(it[good]))):
            prob.iteration_budget(budget)
            total0, why0 = prob.follow_counts()
            first, seen, total, words = begun(prob, sc, 3)
            total1, why1 = prob.follow_counts()
            print('begun batch, budget %d: first pass ended after ms median %.2f (%s), words set by then %s of %d; everything after ms median %.2f; final words: %d x 1, %d x 2; '
                  'handed over per launch %.1f (reason 7: %.1f)' % (budget, med(first), ' '.join('%.2f' % w for w in first), seen, len(Td), med(total), int((words == 1).sum()),
                                                                   int((words == 2).sum()), (total1 - total0)/3, (why1[7] - why0[7])/3))
            print('    first pass / launch without the stragglers: %.2f (goal of the verdict: at most 3)' % (med(first)/med(wallg)))
            wallb, kernb, outb = blocking(prob, sc, 2)
            print('    blocking launch with this budget: wall ms median %.2f; statuses equal to the run without a budget: %s' % (med(wallb), bool(np.array_equal(outb['stats'][:, ST['STATUS']], st[:, ST['STATUS']]))))
        prob.iteration_budget(0)
    sv.close()

elif part == 'cost':
    sv = casadiSolver(wl.train_default(), wl.track_00(), wl.options(100))
    sc = sv._scenarios(wl.c1_times(1024), 0, 1, 1)
    prob = sv.problem
    wall, kern, out = blocking(prob, sc, 20)
    print('config 1, blocking, %s: wall ms median %.4f min %.4f, kernel ms median %.4f min %.4f, converged %d' % (os.environ.get('MSD_LIB', 'product'), med(wall), min(wall), med(kern), min(kern),
                                                                                                 int((out['stats'][:, ST['STATUS']] == 0).sum())))
    if not blocking_only:
        first, seen, total, words = begun(prob, sc, 21)
        print('config 1, begin + result (early results on): wall ms median %.4f min %.4f; first pass after ms median %.4f; words %d x 1, %d x 2'
              % (med(total[1:]), min(total[1:]), med(first[1:]), int((words == 1).sum()), int((words == 2).sum())))
    sv.close()
