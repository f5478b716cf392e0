"""
One process: the config-4 shape (512 scenarios x 50 re-solves, 1 % noise), warm and cold, through DeviceLoop.run.
  mpc_restriction_timing.py <tag> <package dir> <library> <out dir> [tight | mild]
tight: 80 km/h over 2 km from the start and 70 km/h over 1 km announced at re-solve 10 -- most of the benchmark's arrival times (1541 s +- 15 % on a line whose
minimum running time is 1480 s) can no longer be met.  mild: the same two stretches at 1 km/h under the line's limits there (99 and 139 km/h) -- the mechanism with hardly a change of the journeys.
Writes <out>/<tag>.json: loop_ms of the timed runs, mean iterations per re-solve, and sha256 of log columns and z of the last run.
"""
import hashlib, json, os, sys
tag, pkg, libpath, out = sys.argv[1:5]
restricted = sys.argv[5] if len(sys.argv) > 5 else None
v1, v2 = (80/3.6, 70/3.6) if restricted == 'tight' else (99/3.6, 139/3.6)
os.environ['MSD_LIB'] = libpath
sys.path[:0] = [pkg]
import numpy as np
from mseetc import workloads as wl
from mseetc.mpc import DeviceLoop
import mseetc
assert os.path.realpath(os.path.dirname(mseetc.__file__)).startswith(os.path.realpath(pkg)), mseetc.__file__
train, track, N = wl.config('c4')
T = wl.c1_times(512, seed=20260615)
res = dict(tag=tag, lib=libpath, pkg=pkg)
for warm in (True, False):
    loop = DeviceLoop(train, track, wl.options(N), 50, noise=0.01, warmStart=warm)
    kw = {}
    if restricted:
        # two records per scenario: one known from the start, one announced at re-solve 10 (the train is near 9.7 km then)
        kw['speedRestrictions'] = [[(30000.0 + 20.0*(s % 50), 32000.0, v1), (40000.0, 41000.0 + 10.0*(s % 30), v2, 10)] for s in range(512)]
    loop.run(T, seed=1, keepZ=False, **kw)      # warm-up: code objects, buffers
    ms = []
    for rep in range(5):
        log = loop.run(T, seed=1, keepZ=(rep == 4), **kw)
        ms.append(log[0]['loop_ms'])
    h = hashlib.sha256()
    for l in log:
        for key in ('t0', 'v0', 'T', 'status', 'iterations', 'cost', 'z'):
            h.update(np.ascontiguousarray(l[key]).tobytes())
    name = 'warm' if warm else 'cold'
    res[name] = dict(loop_ms=ms, median_ms=float(np.median(ms)), sha256=h.hexdigest(), iterations_per_resolve=float(np.mean([l['iterations'].mean() for l in log])),
                     failed=int(sum((l['status'] < 0).sum() for l in log)), relaxed=int(sum(l['relaxed'].sum() for l in log)))
    loop.close()
os.makedirs(out, exist_ok=True)
json.dump(res, open(os.path.join(out, tag + '.json'), 'w'), indent=1)
print(json.dumps(res))
