"""Conditioning of the tilt series without a GPU: the plain statements of tests/ref64_condition.py against brute force, the host rules
of tomo_tv_amd/align.py, the ABI of the three calls, and what despeckling does to a noisy series with injected spikes."""
import os
import re

import numpy as np
import pytest

import ref64
import ref64_condition as R
import sequences as S
import sequences_condition  # noqa: F401  (registers this feature's rows of the call-sequence closure table)
from conftest import ROOT
from tomo_tv_amd import align

F32 = np.float32
CALLS = ("tomo_sino_window_stats", "tomo_sino_median", "tomo_sino_intensity")


def series(P, N, ns, seed):
    """strictly positive random samples on a per-projection pedestal"""
    rng = np.random.default_rng(seed)
    return (rng.uniform(0.5, 1.5, (P, N, ns)) + 3.0 * np.arange(1, P + 1)[:, None, None]).astype(F32)


def brute_median(X, radius):
    P, N, ns = X.shape
    out = np.zeros_like(X)
    for a in range(P):
        for r in range(N):
            for s in range(ns):
                win = [X[a, min(max(r + i, 0), N - 1), min(max(s + j, 0), ns - 1)] for i in range(-radius, radius + 1)
                       for j in range(-radius, radius + 1)]
                out[a, r, s] = sorted(win)[len(win) // 2]
    return out


@pytest.mark.parametrize("radius", [1, 2])
@pytest.mark.parametrize("shape", [(4, 3), (9, 5), (16, 7), (3, 4)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_median_statement_against_a_sorted_window_per_sample(shape, radius):
    """(3, 4) with radius 2: the window is larger than the image along r, every row index is clamped at both ends"""
    X = series(2, shape[0], shape[1], 10 * shape[0] + radius)
    m = R.median(X, radius)
    assert m.dtype == F32 and np.array_equal(m, brute_median(X, radius))
    assert np.all(np.isin(m, X))                                                   # a selection: every output is an input


def test_replace_and_stats_statements():
    X = series(3, 9, 5, 4)
    X[1, 4, 2] += F32(50)
    m, d = R.diff(X, 1)
    assert d.dtype == F32 and np.array_equal(d, X - m)
    st, bound = R.median_stats(X, 1)
    assert np.allclose(st[:, 0], d.astype(np.float64).sum((1, 2)), rtol=1e-12, atol=1e-12) and np.all(st[:, 3] == 45) and not st[:, 4].any()
    assert np.allclose(st[:, 2], (d.astype(np.float64) ** 2).sum((1, 2)), rtol=1e-12) and np.all(bound > 0)
    out, rep = R.replace(X, 1, np.full(3, np.inf, F32))
    assert not rep.any() and np.array_equal(out.view(np.uint32), X.view(np.uint32))
    out, rep = R.replace(X, 1, np.zeros(3, F32))
    assert np.array_equal(out, m) and np.array_equal(rep, X != m)
    out, rep = R.replace(X, 1, np.full(3, 10, F32))
    assert rep.sum() == 1 and rep[1, 4, 2] and out[1, 4, 2] == m[1, 4, 2]
    assert R.median_stats(X, 1, np.full(3, 10, F32))[0][:, 4].tolist() == [0, 1, 0]
    ws, _ = R.window_stats(X, (4, 5, 2, 3))
    assert np.array_equal(ws[1], [X[1, 4, 2], float(X[1, 4, 2]) ** 2, X[1, 4, 2], X[1, 4, 2]])


def test_fma_statement_rounds_once():
    # 3 * (1 + 2^-23) + 2^-24 = 3 + 7 * 2^-24 exactly; the binary32 numbers around it are 3 + 4 * 2^-24 and 3 + 8 * 2^-24
    x = np.array([[[1 + 2.0 ** -23]]], F32)
    assert R.fma32([3.0], x, [2.0 ** -24])[0, 0, 0] == F32(3 + 2.0 ** -21)
    # (1 + 2^-12)^2 - 1 = 2^-11 + 2^-24 exactly (fused); rounding the product to binary32 first loses the 2^-24
    y = np.array([[[1 + 2.0 ** -12]]], F32)
    got = R.fma32([1 + 2.0 ** -12], y, [-1.0])[0, 0, 0]
    assert got == F32(2.0 ** -11 + 2.0 ** -24) and got != F32(F32(y[0, 0, 0] * y[0, 0, 0]) - F32(1))
    z = np.array([[[2.0, -3.0]]], F32)
    assert R.fma32([-1.0], z, [0.5], clamp=True).tolist() == [[[0.0, 3.5]]]
    assert np.array_equal(R.fma32([1.0], z, [0.0]), z)


@pytest.mark.parametrize("n", range(1, 10))
def test_background_window_is_the_references(n):
    """cpu/utils/logger.py:258-259: XRANGE = [0, Nx // 4], YRANGE = [0, Ny // 4] -- kept at least one sample wide"""
    for m in (1, 4, 9):
        want = (0, max(int(n // 4), 1), 0, max(int(m // 4), 1))
        assert align.background_window(n, m) == want == R.background_window(n, m)


def test_despeckle_thresholds_and_mass_gains():
    st = np.array([[0.0, 8.0, 9.0, 16.0, 0.0], [0.0, 0.0, 0.0, 16.0, 0.0], [1.0, 4.0, 2.0, 4.0, 0.0]])
    th = align.despeckle_thresholds(st, 6.0)
    assert th.dtype == F32 and th.shape == (3,)
    assert th[0] == F32(6.0 * np.sqrt(np.pi / 2) * 0.5) and np.isposinf(th[1]) and th[2] == F32(6.0 * np.sqrt(np.pi / 2))
    assert np.array_equal(th, R.despeckle_thresholds(st, 6.0))
    with pytest.raises(ValueError):
        align.despeckle_thresholds(st, 0.0)
    mom = np.array([[2.0, 1.0, 1.0], [4.0, 0.0, 0.0], [6.0, 5.0, 5.0]])
    g = align.mass_gains(mom)
    assert np.array_equal(g, [2.0, 1.0, 4.0 / 6.0]) and np.allclose(g, R.mass_gains(mom[:, 0]))
    assert np.allclose(g * mom[:, 0], 4.0)
    for bad in (0.0, -1.0):
        mom[1, 0] = bad
        with pytest.raises(ValueError):
            align.mass_gains(mom)


def test_header_declares_and_library_exports_the_three_calls():
    """test_abi_cpu's check narrowed to this feature's names (it fails on a library without them)."""
    from tomo_tv_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tomo_hip.h")).read(), flags=re.S)
    L = _lib.load()
    for name in CALLS:
        assert re.search(r"\bint\s+%s\s*\(\s*tomo_engine\s*\*" % name, src), name
        assert hasattr(L, name) and name in _lib.SIGNATURES, name
    assert L.tomo_sino_window_stats(None, 0, 0, 1, 0, 1, None) == 1 and L.tomo_sino_median(None, 0, -1, 1, None, None) == 1
    assert L.tomo_sino_intensity(None, 0, 0, None, 0) == 1 and L.tomo_last_error()              # a null engine: TOMO_ERR_ARG, no crash
    import sequences_affine3d, sequences_register3d, sequences_sino_normal, sequences_tilt  # noqa: F401, E401  (the other features' rows)
    names = S.header_prototypes(open(os.path.join(ROOT, "include", "tomo_hip.h")).read())
    assert set(sequences_condition.ROWS) == set(CALLS) <= set(names) and S.closure_errors(names) == []


# ---- what despeckling does: the property ----------------------------------------------------------------------------------------------
NOISE, SPIKE, N_SIGMA = 0.05, 40.0, 12.0
SPIKES = [(0, 0, 0), (0, 0, 15), (0, 31, 0), (0, 31, 15),          # (projection, ray, slice): the four corners,
          (1, 0, 7), (2, 13, 0),                                   # an edge along each axis,
          (3, 10, 5), (3, 10, 6),                                  # two in adjacent slices,
          (4, 20, 9), (4, 21, 9),                                  # two in adjacent rays,
          (5, 16, 8), (6, 5, 3), (7, 27, 12), (8, 15, 15)]         # and singles, so that every projection carries one


def spiked_series():
    from tomo_tv_amd.phantom import ellipsoids
    ang = np.linspace(-60, 60, 9)
    clean = R.images(ref64.Matrix(32, ang).fp(ellipsoids(16, 32, seed=5)), 32)
    noisy = (clean + np.random.default_rng(6).normal(0.0, NOISE, clean.shape)).astype(F32)
    X = noisy.copy()
    for a, r, s in SPIKES:
        X[a, r, s] += F32(SPIKE)
    return noisy, X


def test_despeckle_removes_the_spikes_and_little_else():
    """Noise-free projections of ``phantom.ellipsoids(16, 32, seed=5)`` at 9 angles in [-60, 60] (Nray = 32, Nslice = 16; values up
    to about 15), Gaussian noise of sigma = 0.05 (seed 6), 14 spikes of +40 at SPIKES, ``despeckle(n_sigma=12, radius=1)`` as replayed.
    At 32 x 16 samples the object itself is rough against a 3 x 3 median: without spikes |x - median| has the median 0.04 (the
    noise), 1.0 at the 90th percentile and 5.55 at most, and the mean absolute deviation, 0.25 .. 0.33 per projection, measures that
    structure; hence n_sigma = 12 and a spike well above the object.  Observed here: thresholds 5.24 .. 8.41, all 14 spikes replaced
    (the lowest stands 34.9 above its median, four times the largest threshold), 2 of the other 4594 samples replaced (cap: 0.5 % =
    22), and the largest mass change against the spike-free series 11.1 where its bound is 24.7."""
    noisy, X = spiked_series()
    out, counts, masks = R.despeckle(X, N_SIGMA, 1)
    inj = np.zeros(X.shape, bool)
    for a, r, s in SPIKES:
        inj[a, r, s] = True
    th = R.despeckle_thresholds(R.median_stats(X, 1)[0], N_SIGMA)
    others = int((masks[0] & ~inj).sum())
    print(f"thresholds {th.min():.3f} .. {th.max():.3f}; injected replaced {int((masks[0] & inj).sum())} of {inj.sum()}; others replaced "
          f"{others} of {(~inj).sum()}; largest spike-free |d| {np.abs(R.diff(noisy, 1)[1]).max():.3f}")
    assert np.all(masks[0][inj])                                                              # every injected sample
    assert others <= 0.005 * (~inj).sum()                                                     # and hardly anything else
    assert np.array_equal(counts, masks[0].sum((1, 2)))
    # the mass: a replaced sample receives a value of its window that is no spike (at most 4 of the 9 window entries are spikes, the
    # corner counted four times), i.e. a value of the spike-free series; so does the spike-free sample it stands for: per projection
    # |mass(out) - mass(spike-free)| <= (number replaced) * (max - min of the spike-free projection)
    change = np.abs(out.astype(np.float64).sum((1, 2)) - noisy.astype(np.float64).sum((1, 2)))
    bound = counts * (noisy.max((1, 2)).astype(np.float64) - noisy.min((1, 2)))
    print(f"largest mass change {change.max():.3f}, its bound {bound[np.argmax(change)]:.3f}")
    assert np.all(change <= bound)
    assert np.array_equal(out[~masks[0]], X[~masks[0]])                                       # nothing else was touched
