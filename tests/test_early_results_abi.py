"""
CPU-only checks of the early-results boundary (include/mseetc_hip.h: msd_problem_early_results ... msd_solve_batch_done): the header declares the
entry points and the MSD_WAIT_* constants, the built library exports them, the ctypes layer binds them with the header's argument counts, and
without a device the asynchronous front end fails as loudly as the blocking one.  No compute call is made here; what needs a handle -- early
results switched off and msd_solve_batch_begin, the protocol -- is in tests/test_early_results_gpu.py.
"""

import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

import cases

ROOT = Path(__file__).resolve().parent.parent

NAMES = ('msd_problem_early_results', 'msd_problem_iteration_budget', 'msd_solve_batch_begin', 'msd_solve_batch_wait', 'msd_solve_batch_done')


@pytest.fixture(scope='module')
def built():
    import __graft_entry__ as g
    return g.build()


def _header():
    return (ROOT / 'include' / 'mseetc_hip.h').read_text()


def _declared_args(name):
    "number of parameters of `name` as the header declares it"
    m = re.search(r'\bint\s+' + name + r'\s*\(([^)]*)\)\s*;', _header())
    assert m, name
    return len([a for a in m.group(1).split(',') if a.strip()])


def test_header_declares_the_entry_points_and_wait_constants():
    from mseetc import _device
    header = _header()
    for n in NAMES:
        assert _declared_args(n) >= 2, n
    assert re.search(r'^#define MSD_WAIT_FIRST_PASS {}$'.format(_device.WAIT_FIRST_PASS), header, re.M)
    assert re.search(r'^#define MSD_WAIT_ALL {}$'.format(_device.WAIT_ALL), header, re.M)
    assert _device.WAIT_FIRST_PASS != _device.WAIT_ALL
    assert '#define MSD_ABI_VERSION 6' in header      # opt-in entry points: the description record and its version stay


def test_library_exports_them(built):
    lib = ctypes.CDLL(str(built))
    for n in NAMES:
        assert hasattr(lib, n), n


def test_device_layer_binds_them(built):
    from mseetc import _device
    L = _device.lib()
    for n in NAMES:
        fn = getattr(L, n)
        assert fn.argtypes is not None and len(fn.argtypes) == _declared_args(n), n
    for method in ('iteration_budget', 'early_results', 'solve_batch_begin'):
        assert callable(getattr(_device.DeviceProblem, method))
    for method in ('wait_first_pass', 'snapshot', 'result'):
        assert callable(getattr(_device.PendingBatch, method))
    # reason 7 (the budget of the first pass ran out) fits the telemetry the binding asks for
    assert '9 entries' in _header()


def test_null_handle_is_an_invalid_argument(built):
    "every new entry point refuses a null handle with MSD_E_INVALID and a message, without touching a device"
    from mseetc import _device
    L = _device.lib()
    n = ctypes.c_int(7)
    buf = np.zeros(16)
    p = buf.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    words, stats = ctypes.POINTER(ctypes.c_int)(), ctypes.POINTER(ctypes.c_double)()
    assert L.msd_problem_early_results(None, 1) == -1 and L.msd_last_error()
    assert L.msd_problem_iteration_budget(None, 3) == -1
    assert L.msd_solve_batch_begin(None, 1, p, None, p, None, p) == -1
    assert L.msd_solve_batch_wait(None, _device.WAIT_ALL, ctypes.byref(n)) == -1 and n.value == 7
    assert L.msd_solve_batch_done(None, ctypes.byref(words), ctypes.byref(stats)) == -1 and not words


def test_no_device_begin_fails_loudly(built):
    from mseetc import _device
    if _device.lib().msd_device_count() > 0:
        pytest.skip("a GPU is present")
    from mseetc.ocp import casadiSolver
    from mseetc._device import DeviceError
    solver = casadiSolver(cases.train_default(), cases.track_00(), {'numIntervals': 100, 'integrationOptions': {'numApproxSteps': 1}})
    with pytest.raises(DeviceError):
        solver.problem.solve_batch_begin(solver._scenarios([1541.0], 0, 1, 1))
    seen = []
    with pytest.raises(DeviceError):
        solver.solveBatch([1541.0], onFirstPass=lambda mask, part: seen.append(mask))
    assert not seen
