"""Host side of the training decoder's dropout ("The dropout mask rule"); no GPU.

1. Statistics of the restated masks (tests/dropout_ref.py).  They say something about the kernels only because
   tests/test_train_dropout_gpu.py pins the restatement to the kernels element for element.
2. TrainStep's seed: one mask stream per (optimizer step, data-parallel rank, accumulation micro-step).
3. Both C entries refuse a dropout_p outside [0, 1), NaN included, before any launch."""
import ctypes
import functools

import numpy as np
import pytest

import dropout_ref as R
from img2latex_amd import _lib
from img2latex_amd.training.train_step import step_seed
from test_train_batched_host import FAKE, _weights

N = 1 << 20
SEEDS = [0, 1234, 2 ** 62 - 1, 2 ** 64 - 1]
STREAMS = [R.DS_X, R.DS_OUT, R.DS_LAYER0, R.DS_LAYER0 + 1, R.DS_LAYER0 + 2]
SEED_STEPS = [1, 4099, 7919, 4099 * 1000003]           # what step_seed adds for the next rank / step / micro-step / seed
LAGS = [1, 64, 256, 512]                               # neighbours in a row, and rows of H = 64 / 256 / 512 apart
SIGMAS = 5.0


@functools.lru_cache(maxsize=None)
def _mask(seed, stream, p):
    return R.keep_mask(seed % 2 ** 64, stream, N, p)


def _corr_sigmas(a, b):
    """Pearson correlation of two keep indicators in units of its standard deviation under independence, 1/sqrt(n)."""
    a, b = a.astype(np.float64), b.astype(np.float64)
    r = ((a * b).mean() - a.mean() * b.mean()) / (a.std() * b.std())
    return abs(r) * np.sqrt(a.size)


# ------------------------------------------------------------------------------------------------ 1. the restated masks
def test_restatement_fixed_points():
    """The hash itself, worked by hand with Python integers for a few (seed, stream, index), so that a slip in the
    numpy restatement (a shift, a constant, uint64 wrap-around) does not hide behind statistics."""
    M = (1 << 64) - 1

    def u(seed, stream, idx):
        z = (seed + idx * 0x9E3779B97F4A7C15 + stream * 0xD1B54A32D192ED03) & M
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
        z ^= z >> 31
        return (z >> 40) / 2.0 ** 24

    for seed in SEEDS:
        for stream in STREAMS:
            got = R.uniforms(seed, stream, 1000)
            want = np.array([u(seed, stream, i) for i in range(1000)])
            assert got.dtype == np.float32 and np.array_equal(got.astype(np.float64), want), (seed, stream)
            far = R.uniforms(seed, stream, 3, start=2 ** 33)                  # an index past 32 bits
            assert np.array_equal(far.astype(np.float64), [u(seed, stream, 2 ** 33 + i) for i in range(3)])
    assert R.keep_mask(7, 1, 100, 0.0).all()
    assert R.scale(0.0) == 1.0 and R.scale(0.5) == 2.0
    assert R.scale(0.1) == float(np.float32(1) / (np.float32(1) - np.float32(0.1)))


@pytest.mark.parametrize("p", [0.1, 0.3, 0.5])
def test_restated_mask_statistics(p):
    """n = 2^20 elements per mask: the keep fraction of every stream, the correlation of every pair of streams at equal
    indices, and stream X against itself at the neighbouring seeds and at lags.  Each within 5 standard deviations
    (276 statistics over the three p: one beyond 5 sigma has probability 2e-4 for an ideal generator; the worst measured
    on this restatement is 2.34)."""
    keep = 1.0 - float(np.float32(p))
    worst = 0.0
    for seed in SEEDS:
        for s in STREAMS:
            z = abs(_mask(seed, s, p).mean() - keep) / np.sqrt(keep * (1.0 - keep) / N)
            worst = max(worst, z)
            assert z <= SIGMAS, ("keep fraction", p, seed, s, z)
        for i, s in enumerate(STREAMS):
            for s2 in STREAMS[i + 1:]:
                z = _corr_sigmas(_mask(seed, s, p), _mask(seed, s2, p))
                worst = max(worst, z)
                assert z <= SIGMAS, ("streams", p, seed, s, s2, z)
        x = _mask(seed, R.DS_X, p)
        for d in SEED_STEPS:
            z = _corr_sigmas(x, _mask((seed + d) % 2 ** 64, R.DS_X, p))
            worst = max(worst, z)
            assert z <= SIGMAS, ("seed step", p, seed, d, z)
        for lag in LAGS:
            z = _corr_sigmas(x[:-lag], x[lag:])
            worst = max(worst, z)
            assert z <= SIGMAS, ("lag", p, seed, lag, z)
    print(f"dropout mask statistics p={p}: worst {worst:.2f} sigma")


# ------------------------------------------------------------------------------------------------ 2. TrainStep's seed
@pytest.mark.parametrize("seed", [0, 11, 2 ** 62 - 1])
def test_step_seeds_are_distinct(seed):
    seeds = {step_seed(seed, step, rank, micro) for step in range(3000) for rank in range(8) for micro in range(16)}
    assert len(seeds) == 3000 * 8 * 16
    assert all(0 <= s < 2 ** 62 for s in (min(seeds), max(seeds)))


def test_step_seed_is_the_formula_train_step_used():
    for seed, step, rank, micro in [(0, 0, 0, 0), (11, 5, 3, 2), (2 ** 62 - 1, 2999, 7, 15), (123456789, 17, 1, 0)]:
        want = ((seed * 1000003 + step) * 4099 + rank + 7919 * micro) & 0x3FFFFFFFFFFFFFFF
        assert step_seed(seed, step, rank, micro) == want


# ------------------------------------------------------------------------------------------------ 3. refusals
def _fwd(w, p):
    return _lib.lib().i2l_decoder_train_fwd(ctypes.byref(w), FAKE, FAKE, 3, 4, p, 1, 0, FAKE, 0, FAKE, 0, None)


def _bwd(w, p):
    """Every gradient pointer is set (and fake), so that a call which passed the argument checks reaches the workspace
    check, as the forward does."""
    g = _lib.DecoderGrads()
    arrs = [(ctypes.c_void_p * 2)(FAKE, FAKE) for _ in range(4)]
    g.embedding, g.w_out, g.b_out = FAKE, FAKE, FAKE
    g.w_ih, g.w_hh, g.b_ih, g.b_hh = arrs
    return _lib.lib().i2l_decoder_train_bwd(ctypes.byref(w), FAKE, 3, 4, p, 1, 0, FAKE, 0, FAKE, ctypes.byref(g), FAKE,
                                            0, None, None)


@pytest.mark.parametrize("call", [_fwd, _bwd], ids=["fwd", "bwd"])
def test_dropout_p_outside_the_unit_interval_is_refused_before_any_launch(call):
    """Pointers are fake and the workspace is 0 bytes: an accepted p answers I2L_ERR_WORKSPACE, a refused one
    I2L_ERR_ARG, and neither touches anything.  NaN fails both `p < 0` and `p >= 1`; p = 1 scales by 1 / 0."""
    w, keep = _weights(10, 4, 64, 2)
    for p in (-0.1, 1.0, 1.5, float("nan"), float("inf"), -float("inf")):
        assert call(w, p) == _lib.ERR_ARG, p
    for p in (0.0, 0.999):
        assert call(w, p) == _lib.ERR_WORKSPACE, p
    del keep
