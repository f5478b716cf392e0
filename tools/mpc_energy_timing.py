"""
One process: the config-4 shape (512 scenarios x 50 re-solves, 1 % noise), warm and cold, through DeviceLoop.run, with and without the energy account.
  mpc_energy_timing.py <tag> <package dir> <library> <out dir> [account]
Without `account`: five timed runs of the plain loop (the keyword energyAccount is never passed: the script runs against a package that does not know it).
With `account`: five alternating pairs of runs in the same build, account off then account on.
Writes <out>/<tag>.json: loop_ms of the timed runs (per mode), their medians, the cost of the account in per cent of the plain loop's median, sha256 of the log columns
and z of the last plain run and of the last run with the account (the scheme of tools/mpc_rolling_stock_timing.py), and the closed-loop energy of the batch.
"""
import hashlib, json, os, sys
tag, pkg, libpath, out = sys.argv[1:5]
account = len(sys.argv) > 5 and sys.argv[5] == 'account'
os.environ['MSD_LIB'] = libpath
sys.path[:0] = [pkg]
import numpy as np
from mseetc import workloads as wl
from mseetc.mpc import DeviceLoop
import mseetc
assert os.path.realpath(os.path.dirname(mseetc.__file__)).startswith(os.path.realpath(pkg)), mseetc.__file__
train, track, N = wl.config('c4')
T = wl.c1_times(512, seed=20260615)


def digest(log):
    h = hashlib.sha256()
    for l in log:
        for key in ('t0', 'v0', 'T', 'status', 'iterations', 'cost', 'z'):
            h.update(np.ascontiguousarray(l[key]).tobytes())
    return h.hexdigest()


res = dict(tag=tag, lib=libpath, pkg=pkg, account=account)
for warm in (True, False):
    loop = DeviceLoop(train, track, wl.options(N), 50, noise=0.01, warmStart=warm)
    loop.run(T, seed=1, keepZ=False)      # warm-up: code objects, buffers
    if account:
        loop.run(T, seed=1, keepZ=False, energyAccount=True)
    off, on = [], []
    for rep in range(5):
        log = loop.run(T, seed=1, keepZ=(rep == 4))
        off.append(log[0]['loop_ms'])
        if account:
            acc = loop.run(T, seed=1, keepZ=(rep == 4), energyAccount=True)
            on.append(acc[0]['loop_ms'])
    r = dict(loop_ms=off, median_ms=float(np.median(off)), sha256=digest(log), iterations_per_resolve=float(np.mean([l['iterations'].mean() for l in log])),
             failed=int(sum((l['status'] < 0).sum() for l in log)), relaxed=int(sum(l['relaxed'].sum() for l in log)))
    if account:
        from mseetc.mpc import closedLoopEnergy
        e = closedLoopEnergy(acc)
        r.update(account_loop_ms=on, account_median_ms=float(np.median(on)), account_cost_percent=100*(float(np.median(on)) - r['median_ms'])/r['median_ms'],
                 account_sha256=digest(acc), energy_kwh_mean=float(e['total'].mean()), energy_kwh_min=float(e['total'].min()), energy_kwh_max=float(e['total'].max()),
                 losses_kwh_mean=float(e['losses'].mean()), complete=int(e['complete'].sum()), arrival_delay_s_max=float(np.max(e['arrivalTime'] - acc[-1]['T'])))
    res['warm' if warm else 'cold'] = r
    loop.close()
os.makedirs(out, exist_ok=True)
json.dump(res, open(os.path.join(out, tag + '.json'), 'w'), indent=1)
print(json.dumps(res))
