"""DART on the CPU: the numpy statements of tests/ref64_dart.py against brute-force loops, the hash against hand-computed values, the
smoother's bound against a binary32 replay of the kernel's order of operations, the driver loop in binary64 (scipy), and the argument
refusals of the C ABI that need no GPU.

The smoother's bound is derived in the docstring of ref64_dart; the replay below performs exactly the kernel's roundings (sequential
binary32 sum in ascending (dy, dz, ds) order, 1 / count rounded once, one multiply, one subtraction, one fma -- the fma through
binary64, where beta * d is exact and only the sum rounds before the final rounding to binary32: a second rounding of at most
2^-53 relative, far inside a bound whose terms are multiples of 2^-24)."""
import ctypes
import os

import numpy as np
import pytest

import ref64_dart as R
from conftest import GOLDEN

SHAPE = (5, 6, 7)


def _vol(seed, shape=SHAPE):
    """a smooth ramp plus noise: the classes form regions, so that boundary and interior voxels both occur"""
    rng = np.random.default_rng(seed)
    s, y, z = np.meshgrid(*[np.arange(n) for n in shape], indexing="ij")
    return ((s + y + z) / (sum(shape) - 3.0) * 1.6 - 0.3 + rng.uniform(-0.05, 0.05, shape)).astype(np.float32)


def _cube(shape):
    return [(s, y, z) for s in range(shape[0]) for y in range(shape[1]) for z in range(shape[2])]


def _neighbours(v, shape, connectivity):
    for dy in (-1, 0, 1):
        for dz in (-1, 0, 1):
            for ds in (-1, 0, 1):
                if (ds, dy, dz) == (0, 0, 0) or (connectivity == 6 and abs(ds) + abs(dy) + abs(dz) != 1):
                    continue
                w = (v[0] + ds, v[1] + dy, v[2] + dz)
                if all(0 <= w[i] < shape[i] for i in range(3)):
                    yield w


def _mix_int(a):
    a ^= a >> 16
    a = (a * 0x7feb352d) & 0xffffffff
    a ^= a >> 15
    a = (a * 0x846ca68b) & 0xffffffff
    a ^= a >> 16
    return a


def test_hash_against_hand_computed_values():
    # mix(0) = 0 (every step maps 0 to 0); mix(1): 1 -> 1 -> 0x7feb352d -> ^ (>> 15 = 0xffd6) = 0x7febcafb -> * 0x846ca68b -> ...
    assert int(R.mix(np.uint32(0))) == 0
    a = 1
    a ^= a >> 16
    assert a == 1
    a = (a * 0x7feb352d) & 0xffffffff
    assert a == 0x7feb352d
    a ^= a >> 15
    assert a == 0x7feb352d ^ 0xffd6 == 0x7febcafb
    a = (a * 0x846ca68b) & 0xffffffff
    a ^= a >> 16
    assert int(R.mix(np.uint32(1))) == a == _mix_int(1)
    vals = np.array([0, 1, 2, 0xdeadbeef, 0xffffffff, 123456789], np.uint32)
    assert [int(v) for v in R.mix(vals)] == [_mix_int(int(v)) for v in vals]
    # the voxel index and the seed
    shape, seed = (3, 4, 4), 0x1234abcd
    h = R.draws(shape, seed)
    for (s, y, z) in _cube(shape):
        assert int(h[s, y, z]) == _mix_int(_mix_int((s * 4 + y) * 4 + z) ^ seed)


@pytest.mark.parametrize("free_fraction", [0.0, 0.15, 0.5, 1.0])
def test_free_draws_hit_the_fraction(free_fraction):
    n = 2 ** 16
    h = R.draws((16, 64, 64), 99).ravel()
    assert h.size == n
    got = int((h < np.uint32(R.free_threshold(free_fraction))).sum())
    sigma = np.sqrt(n * free_fraction * (1 - free_fraction))
    assert abs(got - n * free_fraction) <= 4 * sigma + (1 if free_fraction == 1.0 else 0)     # threshold 2^32 - 1 leaves out h = 2^32 - 1


@pytest.mark.parametrize("seed", [0, 1])
def test_labels_boundary_free_restore_against_loops(seed):
    x = _vol(seed)
    thr = np.array([0.1, 0.5, 0.9], np.float32)
    x[1, 2, 3], x[0, 0, 0], x[4, 5, 6], x[2, 2, 2] = np.nan, np.inf, thr[1], -np.inf
    lab = R.labels(x, thr)
    for v in _cube(SHAPE):
        assert lab[v] == sum(1 for t in thr if x[v] >= t)
    assert lab[1, 2, 3] == 0 and lab[0, 0, 0] == 3 and lab[4, 5, 6] == 2 and lab[2, 2, 2] == 0
    grey = np.array([0.0, 0.3, 0.7, 1.0], np.float32)
    for C in (6, 26):
        bnd = R.boundary(lab, C)
        for v in _cube(SHAPE):
            assert bnd[v] == any(lab[w] != lab[v] for w in _neighbours(v, SHAPE, C)), (C, v)
        assert bnd.any() and not bnd.all()
        tf = R.free_threshold(0.3)
        fr = R.free_set(bnd, 5, tf)
        st = R.state(x, thr, C, 5, tf)
        for (s, y, z) in _cube(SHAPE):
            h = _mix_int(_mix_int((s * SHAPE[1] + y) * SHAPE[1] + z) ^ 5)      # N = the y extent (volumes are square in y, z on the GPU)
            assert R.draws(SHAPE, 5)[s, y, z] == h
            assert fr[s, y, z] == (bool(bnd[s, y, z]) or h < tf)
            assert st[s, y, z] == int(lab[s, y, z]) | (64 if bnd[s, y, z] else 0) | (128 if fr[s, y, z] else 0)
        out = R.restore(x, st, grey)
        for v in _cube(SHAPE):
            want = x[v] if fr[v] else grey[lab[v]]
            assert out[v].tobytes() == np.float32(want).tobytes()
        assert np.array_equal(R.restore(x, st, grey, everywhere=True), grey[lab])


def _smooth32(x, st, beta):
    """the kernel's order of operations, one voxel at a time, in binary32"""
    out = x.copy()
    beta = np.float32(beta)
    for v in _cube(x.shape):
        if not st[v] & R.FREE:
            continue
        acc, k = np.float32(0), 0
        for w in _neighbours(v, x.shape, 26):
            acc = np.float32(acc + x[w])
            k += 1
        if k == 0:
            continue
        m = np.float32(acc * np.float32(np.float32(1) / np.float32(k)))
        d = np.float32(m - x[v])
        out[v] = np.float32(np.float64(beta) * np.float64(d) + np.float64(x[v]))
    return out


@pytest.mark.parametrize("seed,beta", [(0, 0.1), (1, 0.5), (2, 1.0), (3, 0.0)])
def test_smooth_statement_and_bound(seed, beta):
    x = _vol(10 + seed)
    st = R.state(x, np.array([0.5], np.float32), 26, seed, R.free_threshold(0.4))
    want, bound, fr = R.smooth(x, st, beta)
    # the statement against loops
    for v in _cube(SHAPE):
        nb = [float(x[w]) for w in _neighbours(v, SHAPE, 26)]
        ref = float(x[v]) + float(np.float32(beta)) * (sum(nb) / len(nb) - float(x[v])) if st[v] & R.FREE else float(x[v])
        assert abs(want[v] - ref) <= 1e-14
    got = _smooth32(x, st, beta)
    assert fr.any() and (~fr).any()
    assert np.all(np.abs(got.astype(np.float64) - want) <= bound)
    assert np.array_equal(got[~fr].view(np.uint32), x[~fr].view(np.uint32))
    if beta == 0.0:
        assert np.array_equal(got.view(np.uint32), x.view(np.uint32))
    # the bound is tight to within an order of magnitude or two: it is not a tolerance that would hide a wrong neighbour
    assert bound[fr].max() < 40 * 2.0 ** -24 * 1.5


def test_smooth_keeps_a_constant():
    """c = 0.75, beta = 0.25: the partial sums j c are binary32 numbers, |m - c| <= c 2^-23 (1/k and the product round once each), and
    beta |m - c| < half an ulp of c, so the fma returns c."""
    x = np.full(SHAPE, 0.75, np.float32)
    st = np.full(SHAPE, R.FREE, np.uint8)
    assert np.array_equal(_smooth32(x, st, 0.25).view(np.uint32), x.view(np.uint32))


def test_class_stats_against_loops():
    x = _vol(3)
    thr = np.array([0.2, 0.8], np.float32)
    x[0, 1, 2], x[3, 3, 3], x[1, 1, 1] = np.nan, np.inf, thr[0]
    got = R.class_stats(x, thr)
    want = np.zeros((3, 2))
    for v in _cube(SHAPE):
        c = sum(1 for t in thr if x[v] >= t)
        want[c, 1] += 1
        if np.isfinite(x[v]):
            want[c, 0] += float(x[v])
    assert np.array_equal(got[:, 1], want[:, 1]) and np.allclose(got[:, 0], want[:, 0], rtol=0, atol=1e-12)
    assert got[:, 1].sum() == x.size


@pytest.fixture(scope="module")
def replay():
    g = np.load(os.path.join(GOLDEN, "A_N32_P9.npz"))
    N, P, D = int(g["N"]), len(g["angles_deg"]), R.DRIVER
    assert N == D["N"]
    ph = R.driver_phantom(D["Nslice"], N)
    S = R.Sirt64(g["A"], N * P, N * N)
    b = S.project(ph.astype(np.float64))
    x, lab, rec = R.dart_loop(S, b, D["grey"], D["Niter"], D["arm_iters"], D["init_iters"], D["fix_probability"], D["smoothing"],
                              D["connectivity"], D["seed"], ph.shape)
    xs = np.zeros(ph.shape)
    for _ in range(D["init_iters"] + D["Niter"] * D["arm_iters"]):
        xs = S.step(xs, b)
    xl = xs.copy()
    for _ in range(R.LLOYD_SIRT_ITERS - D["init_iters"] - D["Niter"] * D["arm_iters"]):
        xl = S.step(xl, b)
    return dict(ph=ph, x=x, lab=lab, rec=rec, sirt=xs, long=xl)


def test_driver_replay_beats_thresholded_sirt_by_a_factor_of_two(replay):
    """Phantom, angles and parameters are ref64_dart.DRIVER / driver_phantom (nine angles, -70 .. 70 degrees, 4 x 32 x 32): DART and
    SIRT + threshold at the same 60 iterations.  Measured in binary64: 2 against 16 misclassified voxels of 4096."""
    truth = (replay["ph"] > 0.5).astype(np.uint8)
    mis_dart = int((replay["lab"] != truth).sum())
    mis_sirt = int((R.labels(replay["sirt"].astype(np.float32), R.thresholds(R.DRIVER["grey"])) != truth).sum())
    print("misclassified: DART", mis_dart, "thresholded SIRT", mis_sirt)
    assert mis_sirt > 0 and 2 * mis_dart <= mis_sirt
    assert set(np.unique(replay["x"])) <= set(R.DRIVER["grey"])
    assert max(replay["rec"]["n_free"]) < truth.size and min(replay["rec"]["n_boundary"]) > 0


def test_lloyd_levels_of_the_replay_are_within_five_percent(replay):
    """5 % of the contrast (the phantom's values are 0 and 1; a relative bound means nothing at 0)."""
    lev = R.lloyd(replay["long"].astype(np.float32), 2)
    print("Lloyd levels", lev)
    assert np.all(np.abs(lev - np.array([0.0, 1.0])) <= 0.05)


def test_null_engine_is_refused_with_a_message():
    from tomo_tv_amd import _lib
    L = _lib.load()
    thr = (ctypes.c_float * 1)(0.5)
    grey = (ctypes.c_float * 2)(0.0, 1.0)
    out = (ctypes.c_double * 4)()
    st = (ctypes.c_uint8 * 4)()
    for fn, args in (("tomo_dart_classify", (None, 0, thr, 1, 26, 0, 0)), ("tomo_dart_restore", (None, 0, grey, 2)),
                     ("tomo_dart_segment", (None, 0, grey, 2)), ("tomo_dart_arm", (None, 0, 0, 1, grey, 2)),
                     ("tomo_dart_smooth", (None, 0, 5, 0.1)), ("tomo_dart_class_stats", (None, 0, thr, 1, out)),
                     ("tomo_dart_get_state", (None, st))):
        assert getattr(L, fn)(*args) != 0, fn
        assert L.tomo_last_error(), fn
