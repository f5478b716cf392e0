"""
The launch plan the library selects (msd_plan_describe, include/mseetc_aux.h) for every kind of problem description over the horizons at which the
selection changes, in the form tests/golden/plan_table.json keeps it.  tests/test_abi.py::test_plan_selection_matches_the_recorded_table runs
`enumerate_plans` against the built library and compares with the file; run as a script, this module writes the file:

    python tests/golden/make_plan_table.py

The file is a record of what the library decided at one commit.  It is written again only when a change of the selection is intended, and the
difference of the file is then the statement of that change.

Layout:  lines   the distinct lines of text without the fields that grow with N (lds_bytes, lds_bytes2, work_doubles, nz, nl; in the text of a
                 rejection the horizon reads N), so that a person can read which kernels a description gets
         table   "<description> | <tuning>" -> runs:   [N_first, N_last, index into lines] for every stretch of horizons with one selection
                                                sha256: digest over the complete lines of all those horizons, which pins the fields left out above
No GPU is needed: the probe makes no device call.
"""

import ctypes
import hashlib
import itertools
import json
import re
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
TABLE = Path(__file__).resolve().parent / 'plan_table.json'

N_SHORT = list(range(1, 701))      # the LDS-fit fallbacks between the resident geometries live here
# ... the ends of the streamed geometries (N + 1 around 1024, 2048, 3072, 5120) and every multiple of 256 in between
N_LONG = sorted(set(n1 - 1 for top in (1024, 2048, 3072, 5120) for n1 in range(top - 1, top + 3)) | set(range(768, 5121, 256)))
TUNINGS = (('default', None, N_SHORT + N_LONG), ('no_full', b'no_full', N_SHORT), ('two_nodes_per_lane', b'two_nodes_per_lane', N_SHORT))
INTEGRATORS = (('explicit', None), ('adaptive', ('CVODES', 1e-8, 1e-6)), ('collocation2', ('IRK', 2, 10, np.zeros(12), np.zeros(0))))
GROWS_WITH_N = re.compile(r' (lds_bytes|lds_bytes2|work_doubles|nz|nl)=\d+')


def descriptions():
    "(name, ProblemDesc with room for the longest horizon) of the 288 kinds of description"

    from mseetc import _device
    nmax = max(N_LONG)
    table = np.zeros(13 + 2 + 2 + 16)      # a loss table of one cell
    table[11] = table[12] = 1
    for pn, power, eo, acc, loss, (iname, integ), intloss in itertools.product((0, 1), (0, 1), (0, 1), ('finite', 'infinite'), (0, 1, 2), INTEGRATORS, (0, 1)):
        a = 1.0 if acc == 'finite' else np.inf
        d = _device.make_desc(nmax, pn, power, eo, 1, 1, loss, 100, (0.0, 0.0, 0.0), 9.81, 1.0, 1.0, -1.0, -1.0, 1.0, 1.0, -a, a, 0.1, 0.1, 1.0, 1.0, 1e-8,
                              np.ones(nmax), np.zeros(nmax), np.zeros(nmax), np.ones(nmax + 1), lossTable=table if loss == 2 else None, integrator=integ,
                              integrateLosses=bool(intloss))
        yield 'pn_brake={} power_rows={} energy_optimal={} acc={} loss_kind={} integrator={} integrate_losses={}'.format(pn, power, eo, acc, loss, iname, intloss), d


def enumerate_plans(L):
    "L: the loaded library (mseetc._device.lib()).  Returns dict(lines, table) as described above."

    buf = ctypes.create_string_buffer(4096)
    lines, index, table = [], {}, {}
    try:
        for name, d in descriptions():
            for tname, switch, horizons in TUNINGS:
                if switch:
                    assert L.msd_tuning(switch, 1) == 0
                digest, runs = hashlib.sha256(), []
                for N in horizons:
                    d.num_intervals = N
                    rc = L.msd_plan_describe(ctypes.byref(d), buf, len(buf))
                    if rc == 0:
                        full = buf.value.decode()
                        short = GROWS_WITH_N.sub('', full)
                    else:
                        full = 'error {}: {}'.format(rc, L.msd_last_error().decode())
                        short = full.replace('numIntervals = {} '.format(N), 'numIntervals = N ')
                    digest.update('{} {}\n'.format(N, full).encode())
                    k = index.get(short)
                    if k is None:
                        k = index[short] = len(lines)
                        lines.append(short)
                    if runs and runs[-1][2] == k:      # (a run may bridge the horizons left out above 700)
                        runs[-1][1] = N
                    else:
                        runs.append([N, N, k])
                if switch:
                    assert L.msd_tuning(switch, 0) == 0
                table['{} | {}'.format(name, tname)] = dict(runs=runs, sha256=digest.hexdigest())
    finally:
        for _, switch, _ in TUNINGS:
            if switch:
                L.msd_tuning(switch, 0)
    return dict(lines=lines, table=table)


def dumps(t):
    "one table entry per line: the file stays readable and its differences small"

    rows = ',\n'.join('  {}: {}'.format(json.dumps(k), json.dumps(v, separators=(',', ':'))) for k, v in t['table'].items())
    return '{\n"lines": [\n' + ',\n'.join('  ' + json.dumps(l) for l in t['lines']) + '\n],\n"table": {\n' + rows + '\n}\n}\n'


if __name__ == '__main__':
    sys.path.insert(0, str(ROOT))
    import __graft_entry__ as g
    g.build()
    from mseetc import _device
    TABLE.write_text(dumps(enumerate_plans(_device.lib())))
    print('{}: {} bytes'.format(TABLE, TABLE.stat().st_size))
