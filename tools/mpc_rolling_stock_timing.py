"""
One process: the config-4 shape (512 scenarios x 50 re-solves, 1 % noise), warm and cold, through DeviceLoop.run.
  mpc_rolling_stock_timing.py <tag> <package dir> <library> <out dir> [model | plant]
model: a train of its own per scenario -- config 3's draw (mass, r0, r1, r2 x (1 + 0.05 n), n standard normal clipped to +-2).  plant: the same models, and per
scenario a plant of its own (mass x (1 + 0.05 n), r2 x (1 + 0.1 |n|): a head wind; 8 Runge-Kutta steps per interval).
Writes <out>/<tag>.json: loop_ms of the timed runs, mean iterations per re-solve, re-solves with a moved arrival time, failures, stalled plants, and sha256 of log
columns and z of the last run (the scheme of tools/mpc_restriction_timing.py).
"""
import hashlib, json, os, sys
tag, pkg, libpath, out = sys.argv[1:5]
mode = sys.argv[5] if len(sys.argv) > 5 else None
os.environ['MSD_LIB'] = libpath
sys.path[:0] = [pkg]
import numpy as np
from mseetc import workloads as wl
from mseetc.mpc import DeviceLoop
import mseetc
assert os.path.realpath(os.path.dirname(mseetc.__file__)).startswith(os.path.realpath(pkg)), mseetc.__file__
train, track, N = wl.config('c4')
T = wl.c1_times(512, seed=20260615)
kw = {}
if mode:
    _, kw = wl.c3_scenarios(512, train)
if mode == 'plant':
    n = np.clip(np.random.default_rng(20260616).standard_normal((2, 512)), -2, 2)
    kw.update(plantMass=kw['mass']*(1 + 0.05*n[0]), plantR2=kw['r2']*(1 + 0.1*np.abs(n[1])), plantSteps=8)
res = dict(tag=tag, lib=libpath, pkg=pkg, mode=mode)
for warm in (True, False):
    loop = DeviceLoop(train, track, wl.options(N), 50, noise=0.01, warmStart=warm)
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
                     failed=int(sum((l['status'] < 0).sum() for l in log)), relaxed=int(sum(l['relaxed'].sum() for l in log)),
                     stalled=int(log[-2]['stalled'].sum()) if 'stalled' in log[-2] else None)
    loop.close()
os.makedirs(out, exist_ok=True)
json.dump(res, open(os.path.join(out, tag + '.json'), 'w'), indent=1)
print(json.dumps(res))
