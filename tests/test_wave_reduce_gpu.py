"""
The workgroup reductions of the kernels (msd_kernel.hpp: block_reduce<K> -- one value through DPP moves without an identity register, K values at once
through a transposing butterfly) on the device, against the numpy replay of tests/test_wave_reduce_model.py: sums bit for bit the balanced tree over
aligned blocks of lanes, maxima and minima exact, in every lane.  Then solves against the oracle at the shapes where a lane pattern can go wrong.
Needs an MI355X: run with -m gpu.

What runs where: block_reduce takes the new steps (wave_reduce_from) in a workgroup of one wave only, so the probe on 64 threads is the test of the new code;
on 128 and 256 threads it holds the unchanged reductions of the multi-wave kernels (wave_reduce per value, the waves' totals folded through the LDS) to the
same tree.  The probe's kernels have the thread count as a template argument, like the solver kernels.  Of the solves, N = 5, 100, 127 and 30 run the new
code and N = 200 (128 x 2) the unchanged cross-wave path.

Tolerances of the solves: those of tests/test_gpu_parity.py (_compare) -- objective 1e-8 relative, every variable 1e-6 relative to max(1, |z|),
iterations within 2.
"""
import numpy as np
import pytest

import cases
from test_wave_reduce_model import CASES, bits, block_reference, probe_inputs

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('nthreads,K,op', CASES)
def test_block_reduce_is_the_balanced_tree_in_every_lane(nthreads, K, op):
    from mseetc._device import reduce_probe
    x = probe_inputs(nthreads, K, op)
    ref = block_reference(x, op)
    out = reduce_probe(x, op)
    assert out.shape == (K, nthreads)
    for k in range(K):
        print('K %d op %d threads %d value %d: reference %r, lane 0 holds %r, lanes that differ from the reference: %d'
              % (K, op, nthreads, k, ref[k], out[k, 0], np.count_nonzero(bits(out[k]) != bits(ref[k]))))
    assert np.array_equal(bits(out), np.broadcast_to(bits(ref)[:, None], out.shape))


def test_probe_rejects_what_it_does_not_instantiate():
    from mseetc._device import reduce_probe
    for shape in [(3, 64), (7, 128), (2, 96), (2, 512)]:
        with pytest.raises(ValueError):
            reduce_probe(np.zeros(shape), 0)
    with pytest.raises(ValueError):
        reduce_probe(np.zeros((2, 64)), 3)


# (train, crop of track 00, N, running times, geometry): N = 5 on 64 x 2 has nodes in three lanes; N = 100 leaves 13 lanes idle and N = 127 none; N = 30 is the
# one-node-per-lane kernel; N = 200 with 8 scenarios takes the totals of two waves through the LDS
SHAPES = [(3000, 5, (190.0, 235.0), (64, 2)), (None, 100, (1541.0, 1926.0), (64, 2)), (None, 127, (1541.0, 1926.0), (64, 2)),
          (12000, 30, (520.0, 650.0), (64, 1)), (None, 200, (1541.0, 1926.0), (128, 2))]


@pytest.mark.parametrize('start', ['profile', 'reference'])
@pytest.mark.parametrize('crop,N,T,geometry', SHAPES)
def test_solves_at_the_shapes_where_a_lane_pattern_can_go_wrong(crop, N, T, geometry, start):
    from mseetc._device import lib
    from test_gpu_parity import _compare, _solver
    train, track = cases.train_default(), cases.track_00(crop)
    # (64 x 2 below 64 nodes: the ladder alone gives those horizons 64 x 1)
    forced = geometry == (64, 2) and N + 1 <= 64
    if forced:
        assert lib().msd_tuning(b'geometry', 16*64 + 2) == 0
    try:
        s = _solver(train, track, N, start=start)
        s.problem      # (the handle, and with it the plan, is made on first use)
    finally:
        if forced:
            assert lib().msd_tuning(b'geometry', 0) == 0
    assert s.problem.geometry() == geometry
    _compare(s, cases.oracle_problem(train, track, N), list(np.linspace(T[0], T[1], 8 if N == 200 else 4)))
    s.close()
