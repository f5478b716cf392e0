"""
Early results on the device (include/mseetc_hip.h: msd_solve_batch_begin / _wait / _done, msd_problem_iteration_budget): a batch that holds one
scenario without a solution next to easy ones.  The easy ones are readable -- final, bit for bit -- when the first pass has ended, while the
follow-up kernel still works on the straggler.

Reference for bit equality: the blocking solve_batch on a second handle of the same description, early results off.  Stats records are compared
without their two shader-clock columns (CYC_TOTAL, CYC_KKT: telemetry of the run, not of the solve) against another run, and in full against
the same run's final records.  Converged scenarios are also held against the oracle within the bounds of tests/test_gpu_parity.py (_compare).

Running times (the oracle on all of them): the 1.1 ... 1.4 multiples of the minimum running time converge in 12-19 iterations without a correction
or a restoration phase; the 0.9 multiples end with status -2 after 216-423 iterations and 13-16 restoration phases, so they need the follow-up kernel.
No test asserts that a word is still 0: the follow-up kernel may have ended by the time the host looks.
"""

import ctypes

import numpy as np
import pytest

import cases
from test_gpu_parity import OBJ_RTOL, Z_RTOL

pytestmark = pytest.mark.gpu

RK11 = dict(numSteps=1, numApproxSteps=1)
FIG5_TMIN = 272.4726      # simulations/figure5.py:96 (tests/test_gpu_parity.py pins it against the device and the oracle)
FIG5_KW = dict(terminalVelocity=100/3.6, initialVelocity=1.0)


def _st():
    from mseetc._device import ST
    return ST


def _solve_columns():
    "the columns of a stats record that the solve determines (everything but the shader-clock telemetry)"
    ST = _st()
    return [k for k in range(ST['COUNT']) if k not in (ST['CYC_TOTAL'], ST['CYC_KKT'])]


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _blocking(solver, scen):
    "the reference run: blocking, early results off; copies (the result arrays are pooled)"
    out = solver.problem.solve_batch(scen, want_multipliers=True)
    return dict(z=out['z'].copy(), stats=out['stats'].copy(), lam_g=out['lam_g'].copy())


def _assert_rows_equal(got, ref, rows, what):
    cols = _solve_columns()
    for k in rows:
        assert _same_bits(got['z'][k], ref['z'][k]), (what, 'z', k)
        assert _same_bits(got['lam_g'][k], ref['lam_g'][k]), (what, 'lam_g', k)
        assert _same_bits(got['stats'][k][cols], ref['stats'][k][cols]), (what, 'stats', k, got['stats'][k], ref['stats'][k])


def _against_oracle(res, scen, prob, rows, start='profile'):
    "the checks of test_gpu_parity._compare on rows of a result"
    from oracle import oracle
    from oracle.oracle import DP
    ST = _st()
    for k in rows:
        assert res['stats'][k, ST['STATUS']] == 0, (k, res['stats'][k])
        dp = prob.dp.copy()
        dp[DP['T0']], dp[DP['TEND']], dp[DP['V0SQ']], dp[DP['VNSQ']] = scen[k]
        ref = oracle.solve(prob, dp, start=start)
        assert ref['stats']['STATUS'] == 0
        assert abs(res['stats'][k, ST['OBJ']] - ref['stats']['OBJ']) <= OBJ_RTOL*abs(ref['stats']['OBJ'])
        assert np.max(np.abs(res['z'][k] - ref['z'])/np.maximum(1.0, np.abs(ref['z']))) <= Z_RTOL
        assert abs(int(res['stats'][k, ST['ITERS']]) - int(ref['stats']['ITERS'])) <= 2
        assert res['z'][k][-1] == scen[k][3]
        assert res['z'][k][-2] <= scen[k][1]*(1 + 1.01e-8)


def _early_run(solver, scen, ref, straggler):
    """
    One begun batch on `solver`'s handle against the blocking reference `ref`: snapshot at the end of the first pass, then everything.  Returns
    the final words.
    """
    ST = _st()
    prob = solver.problem
    listed0 = prob.follow_counts()[0]
    pend = prob.solve_batch_begin(scen, want_multipliers=True)
    mask = pend.wait_first_pass()
    words_then = pend.done.copy()            # (read in front of the rows)
    snap = pend.snapshot()
    first = np.flatnonzero(words_then == 1)
    print('words after the first pass', words_then.tolist())
    assert mask.dtype == bool and mask.shape == (len(scen),) and np.all(mask[first])
    res = pend.result()
    words = pend.done.copy()
    print('words at the end', words.tolist(), 'status', res['stats'][:, ST['STATUS']].tolist(), 'iterations', res['stats'][:, ST['ITERS']].tolist())
    # what was readable at the end of the first pass was final: against the same run (the whole record) and against the blocking run
    for k in first:
        assert _same_bits(snap['z'][k], res['z'][k]) and _same_bits(snap['lam_g'][k], res['lam_g'][k]) and _same_bits(snap['stats'][k], res['stats'][k]), k
    _assert_rows_equal(snap, ref, first, 'snapshot')
    _assert_rows_equal(res, ref, range(len(scen)), 'final')
    # the mirror ends as the copy of the records
    assert _same_bits(pend.snapshot()['stats'], res['stats'])
    assert set(words.tolist()) <= {1, 2}
    assert int(np.sum(words == 2)) == prob.follow_counts()[0] - listed0
    assert np.all(words[first] == 1)
    if straggler is not None:
        assert words[straggler] == 2 and res['stats'][straggler, ST['STATUS']] < 0
        assert np.any(words == 1)
    return words, res


# ---- case 1, 5, 6: the fused family, a single wave, LDS-resident follow-up kernel ----

def _fused_solver():
    from mseetc.ocp import casadiSolver
    return casadiSolver(cases.train_default(), cases.track_00(12000), dict(numIntervals=40, maxIterations=500, integrationOptions=RK11), startingPoint='profile')


@pytest.fixture(scope='module')
def fused():
    "the batch of cases 1, 5 and 6 and its blocking reference (computed once, never written to)"
    from oracle import oracle
    train, track = cases.train_default(), cases.track_00(12000)
    po = cases.oracle_problem(train, track, 40, energyOptimal=False, losses='none')
    reft = oracle.solve(po, po.scenario(3*track.length/train.velocityMax, 0.0, 1.0, 1.0), start='profile')
    assert reft['stats']['STATUS'] == 0
    tmin = float(reft['z'][-2])
    assert abs(tmin - 412.946) < 1e-2, tmin      # (the figure the running times below were chosen by)
    T = tmin*np.array([1.1, 1.15, 1.2, 1.25, 1.3, 1.35, 1.4, 0.9])
    blocking = _fused_solver()
    scen = blocking._scenarios(T, 0, 1, 1)
    ref = _blocking(blocking, scen)
    blocking.close()
    for a in ref.values():
        a.setflags(write=False)
    scen.setflags(write=False)
    return dict(scen=scen, ref=ref, prob=cases.oracle_problem(train, track, 40))


def test_fused_single_wave(fused):
    s = _fused_solver()
    assert s.problem.geometry()[0] == 64
    words, res = _early_run(s, fused['scen'], fused['ref'], straggler=7)
    _against_oracle(res, fused['scen'], fused['prob'], range(7))
    s.close()


# ---- cases 2, 3: the loss-table family ----

def _table_case(N, factors, geometry):
    from mseetc.ocp import casadiSolver
    from test_integrated_loss_table import _dynamic_train, _problem
    train, track = _dynamic_train(), cases.track_00(8500)
    make = lambda: casadiSolver(train, track, dict(numIntervals=N, maxIterations=500, integrationOptions=RK11), startingPoint='profile')
    blocking, s = make(), make()
    assert s._desc.loss_kind == 2 and s._desc.integrate_losses == 0
    assert s.problem.geometry() == geometry
    scen = s._scenarios(FIG5_TMIN*np.array(factors), 0, FIG5_KW['terminalVelocity'], FIG5_KW['initialVelocity'])
    ref = _blocking(blocking, scen)
    blocking.close()
    words, res = _early_run(s, scen, ref, straggler=len(factors) - 1)
    _against_oracle(res, scen, _problem(train, track, N, integrateLosses=False), range(len(factors) - 1))
    s.close()


def test_loss_table_streamed_follow_up():
    _table_case(40, (1.1, 1.2, 1.213, 1.285, 0.9), (64, 1))


def test_two_wave_first_pass():
    "the smallest shape where the completion word could overtake another wave's stores"
    _table_case(100, (1.2, 1.285, 0.9), (128, 1))


# ---- case 4: a streamed first pass ----

def test_streamed_first_pass():
    from test_gpu_parity import _solver
    train, track = cases.train_fig10(), cases.track_00()
    make = lambda: _solver(train, track, 700, start='profile', maxIterations=1000)
    blocking, s = make(), make()
    assert s.problem.geometry() == (512, 2)
    scen = s._scenarios([1541.0, 1620.0], 0, 1, 1)
    ref = _blocking(blocking, scen)
    blocking.close()
    pend = s.problem.solve_batch_begin(scen, want_multipliers=True)
    pend.wait_first_pass()
    res = pend.result()
    _assert_rows_equal(res, ref, range(2), 'final')
    assert np.all(pend.done != 0) and set(pend.done.tolist()) <= {1, 2}
    assert np.all(res['stats'][:, _st()['STATUS']] == 0)
    s.close()


# ---- case 5: the iteration budget of the first pass ----

def test_iteration_budget(fused):
    ST = _st()
    scen = fused['scen'][:7]
    ref = {k: v[:7] for k, v in fused['ref'].items()}
    s = _fused_solver()
    prob = s.problem

    def run(budget):
        prob.iteration_budget(budget)
        total0, why0 = prob.follow_counts()
        pend = prob.solve_batch_begin(scen, want_multipliers=True)
        res = pend.result()
        total1, why1 = prob.follow_counts()
        print('budget', budget, 'words', pend.done.tolist(), 'iterations', res['stats'][:, ST['ITERS']].tolist(), 'handed over', total1 - total0, 'reason 7', why1[7] - why0[7])
        return pend.done.copy(), dict(z=res['z'].copy(), stats=res['stats'].copy(), lam_g=res['lam_g'].copy()), total1 - total0, why1[7] - why0[7]

    # 5 iterations are fewer than any of the seven needs (12-19): every one is handed over, and the follow-up kernel solves it from its starting point
    words, res, handed, why7 = run(5)
    assert words.tolist() == [2]*7 and handed == 7 and why7 == 7
    _against_oracle(res, scen, fused['prob'], range(7))
    # more than any of them needs, and none: nobody is handed over and nothing changes
    for budget in (200, 0):
        words, res, handed, why7 = run(budget)
        assert words.tolist() == [1]*7 and handed == 0 and why7 == 0
        _assert_rows_equal(res, ref, range(7), 'budget {}'.format(budget))
    with pytest.raises(ValueError):
        prob.iteration_budget(-1)
    s.close()


# ---- case 6: the protocol ----

def test_protocol(fused):
    from mseetc import _device
    L = _device.lib()
    s = _fused_solver()
    prob = s.problem
    scen, B = np.ascontiguousarray(fused['scen']), len(fused['scen'])
    z, st = prob._results.empty('z', (B, prob.nz)), prob._results.empty('st', (B, _device.ST['COUNT']))
    n = ctypes.c_int(-1)
    # early results are off until asked for: begin is an invalid call, and so is a wait without a begun batch
    assert L.msd_solve_batch_begin(prob._h, B, _device._d(scen), None, _device._d(z), None, _device._d(st)) == -1
    assert b'early results' in L.msd_last_error()
    assert L.msd_solve_batch_wait(prob._h, _device.WAIT_ALL, ctypes.byref(n)) == -1
    # result arrays the device cannot address
    prob.early_results(True)
    pageable = np.zeros((B, prob.nz))
    assert L.msd_solve_batch_begin(prob._h, B, _device._d(scen), None, _device._d(pageable), None, _device._d(st)) == -1
    assert b'page-locked' in L.msd_last_error()
    # a second begin, or any other solve of the handle, before MSD_WAIT_ALL
    pend = prob.solve_batch_begin(scen, want_multipliers=True)
    with pytest.raises(ValueError):
        prob.solve_batch_begin(scen)
    with pytest.raises(ValueError):
        prob.solve_batch(scen)
    assert L.msd_solve_batch_wait(prob._h, _device.WAIT_FIRST_PASS, ctypes.byref(n)) == 0 and 0 <= n.value < B      # (the first pass has ended some)
    assert L.msd_solve_batch_wait(prob._h, 3, ctypes.byref(n)) == -1
    res = pend.result()
    _assert_rows_equal(res, fused['ref'], range(B), 'begun')
    assert L.msd_solve_batch_wait(prob._h, _device.WAIT_ALL, ctypes.byref(n)) == -1      # (waited for in full: nothing is begun)
    # the handle is an ordinary one again
    again = _blocking(s, scen)
    _assert_rows_equal(again, fused['ref'], range(B), 'blocking afterwards')
    prob.keep_duals(True)
    with pytest.raises(ValueError):
        prob.solve_batch_begin(scen)
    s.close()


def test_solve_batch_on_first_pass_callback(fused):
    "casadiSolver.solveBatch(onFirstPass=...): called once with the mask and the partial result; the return value is the blocking one"
    s = _fused_solver()
    T = fused['scen'][:, 1]
    calls = []
    res = s.solveBatch(T, multipliers=True, classifyFailures=False, onFirstPass=lambda mask, part: calls.append((mask.copy(), {k: np.copy(v) for k, v in part.items()})))
    assert len(calls) == 1
    mask, part = calls[0]
    assert mask.dtype == bool and mask.shape == (8,) and mask.any()
    rows = np.flatnonzero(mask)
    _assert_rows_equal(part, fused['ref'], rows, 'partial')
    assert np.array_equal(part['status'][rows], res['status'][rows]) and np.array_equal(part['iterations'][rows], res['iterations'][rows])
    _assert_rows_equal(res, fused['ref'], range(8), 'returned')
    assert res['status'][7] < 0 and np.all(res['status'][:7] == 0)
    with pytest.raises(ValueError):
        s.solveBatch(T, onFirstPass=lambda mask, part: None, shift=1)
    s.close()
