"""
The reductions over a workgroup (msd_kernel.hpp: wave_reduce, block_reduce) as a numpy replay -- the reference of tests/test_wave_reduce_gpu.py, and the
checks that make that comparison mean something.  Runs without a GPU.

A sum over the 64 lanes of a wave is the balanced tree over aligned blocks: neighbouring lanes, neighbouring pairs, quads, halves of a row, rows 0+1 and
2+3, the two halves of the wave.  The operands of one addition may stand either way round (IEEE addition commutes); the grouping is fixed, and with it every
bit of the result.  The totals of the waves of a workgroup are then folded in the order of the waves (block_reduce's pass through the LDS).  Maxima and minima
do not depend on the order.  `tree` below is that reference in float64; `replay` walks the lane moves of the device code (DPP quad permutations and row
shifts, row broadcasts, the lane swaps of gfx950, the transposing butterfly for K values at once) on arrays of 64 lanes and has to land on the same bits.

The inputs (`probe_inputs`) span 1e-300 ... 1e300 and hold +-0, +-inf and lanes at the operation's identity; a test below shows that another grouping of
the same additions -- the top-down xor order of the host emulation -- gives other bits on them.
"""
import numpy as np
import pytest

SUM, MAX, MIN = 0, 1, 2
OPS = {SUM: np.add, MAX: np.fmax, MIN: np.fmin}
IDENTITY = {SUM: 0.0, MAX: -np.inf, MIN: np.inf}
KS = (1, 2, 4, 5, 6, 8)
THREADS = (64, 128, 256)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def tree(x, op):
    "x: (..., 64) -> (...): the balanced tree over aligned blocks of lanes"
    f = OPS[op]
    x = np.asarray(x, dtype=np.float64)
    while x.shape[-1] > 1:
        x = f(x[..., 1::2], x[..., 0::2])
    return x[..., 0]


def topdown_xor(x, op):
    "the same 63 combinations grouped the other way: distances 32, 16, ..., 1 (wave_reduce of the host emulation)"
    f = OPS[op]
    x = np.array(x, dtype=np.float64)
    lanes = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        x = f(x, x[..., lanes ^ off])
    return x[..., 0]


def block_reference(x, op):
    "x: (K, nthreads) -> (K,): block_reduce -- the tree in every wave, then the waves' totals folded in their order"
    f = OPS[op]
    K, nt = x.shape
    w = tree(x.reshape(K, nt//64, 64), op)
    r = w[:, 0]
    for k in range(1, nt//64):
        r = f(r, w[:, k])
    return r


def probe_inputs(nthreads, K, op, seed=0):
    """
    (K, nthreads) operands.  Row k has a scale of its own between 1e-300 and 1e300 (K rows spread over the whole range; the mantissas are random, so every
    addition rounds), a tenth of the lanes twenty decades below it, +-0 in some lanes and the identity of the operation in others.  One row of a sum holds
    +inf or -inf (never both: the sum would be a NaN, whose bits are nobody's contract), a maximum's rows hold +inf, -inf or neither in turn.
    """
    with np.errstate(over='ignore'):
        rng = np.random.default_rng([seed, nthreads, K, op])
        x = np.empty((K, nthreads))
        for k in range(K):
            decade = -300.0 + 600.0*((k*5 + nthreads//64) % 8)/7.0 if K > 1 else (-300.0, 0.0, 300.0)[(nthreads//64) % 3]
            scale = 10.0**min(decade, 299.0)
            v = scale*rng.uniform(0.5, 1.0, nthreads)*rng.choice([-1.0, 1.0], nthreads)
            v[rng.random(nthreads) < 0.1] *= 1e-20 if decade > -280 else 1.0
            v[rng.random(nthreads) < 0.08] = 0.0
            v[rng.random(nthreads) < 0.08] = -0.0
            v[rng.random(nthreads) < 0.15] = IDENTITY[op]
            # a positive and a negative operand in every row: the extremum is no zero, whose sign a maximum need not define
            v[rng.integers(nthreads)] = scale
            v[(np.flatnonzero(v == scale)[0] + 1) % nthreads] = -scale
            x[k] = v
        if op == SUM:
            if K >= 4:
                x[K - 1, rng.integers(nthreads)] = np.inf if nthreads == 128 else -np.inf
        else:
            for k in range(K):
                if k % 3 == 1:
                    x[k, rng.integers(nthreads)] = np.inf
                elif k % 3 == 2:
                    x[k, rng.integers(nthreads)] = -np.inf
    return x


# ---- the lane moves of the device code ------------------------------------------------------------------------------------------------------------------
LANES = np.arange(64)


def quad_perm(x, p):
    return x[(LANES & ~3) | np.asarray(p)[LANES & 3]]


def row_shr(x, n):
    "lane l reads lane l - n of its row of 16; 0 where there is none (bound_ctrl)"
    return np.where((LANES & 15) >= n, x[np.maximum(LANES - n, 0)], 0.0)


def row_bcast15(x):
    return np.where(LANES >= 16, x[np.maximum((LANES & ~15) - 1, 0)], 0.0)


def row_bcast31(x):
    return np.where(LANES >= 32, x[31], 0.0)


def swap16(a, b):
    "rows 1 and 3 of a change places with rows 0 and 2 of b"
    a, b = a.copy(), b.copy()
    for r in (0, 32):
        t = a[r + 16:r + 32].copy()
        a[r + 16:r + 32] = b[r:r + 16]
        b[r:r + 16] = t
    return a, b


def swap32(a, b):
    "the upper half of a changes places with the lower half of b"
    a, b = a.copy(), b.copy()
    t = a[32:].copy()
    a[32:] = b[:32]
    b[:32] = t
    return a, b


def replay_one(x, f):
    x = f(x, quad_perm(x, (1, 0, 3, 2)))
    x = f(x, quad_perm(x, (2, 3, 0, 1)))
    x = f(x, row_shr(x, 4))
    x = f(x, row_shr(x, 8))
    x = f(x, row_bcast15(x))
    x = f(x, row_bcast31(x))
    return x[63]


def replay(v, op):
    "v: (K, 64) -> (K,): wave_reduce_from<K, 0> of msd_kernel.hpp, move for move"
    f = OPS[op]
    K = v.shape[0]
    out = np.empty(K)
    o = 0
    with np.errstate(invalid='ignore'):      # (lanes that nobody reads may add inf and -inf)
        while K - o >= 2:
            four = K - o >= 4
            if op != SUM:
                a, b = swap32(v[o], v[o + 1])
                x = f(a, b)
                if four:
                    a, b = swap32(v[o + 2], v[o + 3])
                    a, b = swap16(x, f(a, b))
                    x = f(a, b)
                x = f(x, quad_perm(x, (1, 0, 3, 2)))
                x = f(x, quad_perm(x, (2, 3, 0, 1)))
                x = f(x, row_shr(x, 4))
                x = f(x, row_shr(x, 8))
                if four:
                    out[o:o + 4] = x[15], x[47], x[31], x[63]
                else:
                    x = f(x, row_bcast15(x))
                    out[o:o + 2] = x[31], x[63]
            else:
                def transpose(a, b, upper, p):
                    return f(np.where(upper, b, a), quad_perm(np.where(upper, a, b), p))
                x = transpose(v[o], v[o + 1], (LANES & 1) != 0, (1, 0, 3, 2))
                if four:
                    y = transpose(v[o + 2], v[o + 3], (LANES & 1) != 0, (1, 0, 3, 2))
                    x = transpose(x, y, (LANES & 2) != 0, (2, 3, 0, 1))
                else:
                    x = f(x, quad_perm(x, (2, 3, 0, 1)))
                x = f(x, row_shr(x, 4))
                x = f(x, row_shr(x, 8))
                a, b = swap16(x, x)
                x = f(a, b)
                a, b = swap32(x, x)
                x = f(a, b)
                if four:
                    out[o:o + 4] = x[60:64]
                else:
                    out[o:o + 2] = x[62:64]
            o += 4 if four else 2
        if K - o == 1:
            out[o] = replay_one(v[o], f)
    return out


CASES = [(nt, K, op) for nt in THREADS for K in KS for op in (SUM, MAX, MIN)]


@pytest.mark.parametrize('nthreads,K,op', CASES)
def test_inputs_cover_what_the_issue_lists(nthreads, K, op):
    x = probe_inputs(nthreads, K, op)
    assert x.shape == (K, nthreads) and not np.any(np.isnan(x))
    assert np.any(bits(x) == bits(0.0)) and np.any(bits(x) == bits(-0.0)) and np.any(x == IDENTITY[op])
    ref = block_reference(x, op)
    assert not np.any(np.isnan(ref)) and not np.any(ref == 0.0)


def test_inputs_span_the_exponent_range_and_hold_infinities():
    mags, infs = [], set()
    for nt, K, op in CASES:
        x = probe_inputs(nt, K, op)
        fin = np.abs(x[np.isfinite(x) & (x != 0)])
        mags += [fin.min(), fin.max()]
        infs |= {(op, s) for s in (np.inf, -np.inf) if np.any(x == s) and s != IDENTITY[op]}
    assert min(mags) <= 1e-299 and max(mags) >= 1e299
    assert infs == {(SUM, np.inf), (SUM, -np.inf), (MAX, np.inf), (MIN, -np.inf)}


@pytest.mark.parametrize('K', KS)
def test_another_grouping_of_the_sums_gives_other_bits(K):
    moved = total = 0
    for nthreads in THREADS:
        x = probe_inputs(nthreads, K, SUM).reshape(K, nthreads//64, 64)
        a, b = tree(x, SUM), topdown_xor(x, SUM)
        fin = np.isfinite(a)
        size = np.sum(np.abs(np.where(np.isfinite(x), x, 0.0)), axis=-1)
        assert np.all(np.abs(a[fin] - b[fin]) <= 1e-13*size[fin])    # (the same sum ...)
        moved += np.count_nonzero(bits(a) != bits(b))                # (... in other bits)
        total += a.size
    print('%d of %d wave sums differ between the two groupings' % (moved, total))
    assert 4*moved >= total


@pytest.mark.parametrize('op', [MAX, MIN])
def test_extrema_do_not_depend_on_the_grouping(op):
    for nt, K, o in CASES:
        if o == op:
            x = probe_inputs(nt, K, op)
            direct = x.max(axis=1) if op == MAX else x.min(axis=1)
            assert np.array_equal(bits(block_reference(x, op)), bits(direct))


@pytest.mark.parametrize('nthreads,K,op', CASES)
def test_lane_moves_of_the_device_code_land_on_the_tree(nthreads, K, op):
    x = probe_inputs(nthreads, K, op).reshape(K, nthreads//64, 64)
    for w in range(nthreads//64):
        assert np.array_equal(bits(replay(x[:, w], op)), bits(tree(x[:, w], op)))
