"""The tilt-angle refinement without a GPU: the binary32 replay of ``k_vol_rot_derivative`` inside its a-priori bound, the derivative
volume against the finite difference of the oracle's own matrix, the gauge, the recovery experiment in binary64 on a dense matrix
(tests/ref64_tilt.py) and the edge cases of ``align.tilt_increment``; plus the two new symbols in the library."""
import ctypes

import numpy as np
import pytest

import ref64_tilt as T
import sequences_tilt  # noqa: F401  (registers this feature's rows of the call-sequence closure table)


def test_the_library_exports_the_two_calls_and_refuses_a_null_engine():
    from tomo_tv_amd import _lib
    L = _lib.load()
    assert _lib.SIGNATURES["tomo_volume_rot_derivative"] and _lib.SIGNATURES["tomo_sino_tilt_normal"]
    out = np.zeros(4)
    assert L.tomo_volume_rot_derivative(None, 0, 1) == 1 and L.tomo_last_error()
    assert L.tomo_sino_tilt_normal(None, 0, 1, 2, 1, out.ctypes.data_as(ctypes.c_void_p)) == 1


@pytest.mark.parametrize("shape", [(5, 9), (3, 16), (2, 33)])
def test_binary32_replay_stays_within_the_bound(shape):
    ns, N = shape
    rng = np.random.default_rng(N)
    for f in (rng.standard_normal((ns, N, N)), 1e3 + rng.random((ns, N, N)), rng.random((ns, N, N)) * 1e-30):
        f = f.astype(np.float32)
        err = np.abs(T.rot_derivative_f32(f).astype(np.float64) - T.rot_derivative(f))
        ratio = float(np.max(err / T.rot_derivative_bound(f)))
        print(f"{shape}: worst error / bound {ratio:.3f}")
        assert ratio <= 1.0
    const = np.full((ns, N, N), 3.25, np.float32)
    assert not T.rot_derivative_f32(const).any() and not T.rot_derivative(const).any()


def test_border_rule_and_radial_symmetry():
    N = 9
    f = np.zeros((1, N, N))
    f[0, 0, 4] = 1.0                                      # on the top row: only its row neighbours (d_X) and the row below (d_Y) see it
    D = T.rot_derivative(f)
    Y0 = 0.5 * (N - 1)
    assert D[0, 0, 3] == -0.5 * Y0 and D[0, 0, 5] == 0.5 * Y0 and D[0, 0, 4] == 0.0      # -Y d_X f on the row itself
    assert D[0, 1, 4] == 0.0                              # X = 0 in the centre column: X d_Y f vanishes
    assert np.count_nonzero(D) == 2
    f[0, 0, 4], f[0, 0, 2] = 0.0, 1.0
    D = T.rot_derivative(f)
    assert D[0, 1, 2] == 0.5 * (2 - Y0) * (1.0 - 0.0)    # (X / 2)(f[i-1] - f[i+1]) = (X / 2) * 1 with X = 2 - 4 = -2
    # a function of the radius alone does not change under a rotation: away from the border rows and columns the two terms of D f,
    # each as large as X d_Y f, cancel up to the truncation error of a central difference (relative to the derivative about
    # 1 / (2 sigma^2) = 2 % for a Gaussian of sigma = 5 pixels)
    X, Y = T._coords(33)
    rad = np.exp(-(X ** 2 + Y ** 2) / (2 * 5.0 ** 2))
    D = T.rot_derivative(rad)[0, 1:-1, 1:-1]
    assert np.max(np.abs(D)) < 0.05 * np.max(np.abs(X[0] * np.gradient(rad[0], axis=0)))


def test_projection_of_the_derivative_volume_is_the_angle_derivative_of_the_projection():
    """A (D f) against (A(theta + h) - A(theta - h)) f / 2h of the oracle's matrix, per projection, N = 32, nine angles away from the
    axes, h = 0.5 degree.  Measured in binary64: correlations 0.9144 ... 0.9969 (the matrix of a 32-pixel grid is itself rough in the
    angle: at h = 0.25 the smallest is 0.884), ratios <fd, d> / <d, d> 0.96 ... 1.19 and 2.29 for the projection next to the axis (3.7 degrees).  Threshold: the smallest measured correlation
    minus a margin of 0.014 -> 0.90; a wrong sign gives -0.9, exchanged axes about 0."""
    N, P, h = 32, 9, 0.5
    ang = np.linspace(-70, 70, P) + 3.7
    f = T.blobs(N)
    fd = ((T.dense_matrix(N, ang + h) - T.dense_matrix(N, ang - h)) @ f.ravel() / (2 * np.deg2rad(h))).reshape(P, N)
    d = (T.dense_matrix(N, ang) @ T.rot_derivative(f[None]).ravel()).reshape(P, N)
    corr = np.sum(fd * d, 1) / np.sqrt(np.sum(fd * fd, 1) * np.sum(d * d, 1))
    ratio = np.sum(fd * d, 1) / np.sum(d * d, 1)
    print("correlation per projection", np.round(corr, 4), "ratio", np.round(ratio, 3))
    assert corr.min() >= 0.90
    assert ratio.min() >= 0.8 and 0.9 <= np.median(ratio) <= 1.2              # per radian: the scale and the sign


def test_gauge_a_common_offset_yields_increments_without_a_mean():
    from tomo_tv_amd.align import tilt_increment
    N, P = 32, 11
    nominal, truth = T.angle_case(P, 2.0, seed=3)
    f = T.blobs(N)
    b = T.dense_matrix(N, truth + 1.5) @ f.ravel()                  # all true angles moved by the same 1.5 degrees
    A = T.dense_matrix(N, nominal)
    g, d = (A @ f.ravel()).reshape(P, N), (A @ T.rot_derivative(f[None]).ravel()).reshape(P, N)
    r = b.reshape(P, N) - g
    rd, dd = np.sum(r * d, 1), np.sum(d * d, 1)
    raw = np.rad2deg(rd / dd)
    assert abs(raw.mean()) > 0.5                                    # the ungauged steps do carry the offset ...
    inc = tilt_increment(rd, dd)
    assert abs(inc.mean()) < 1e-12 and np.allclose(inc, raw - raw.mean(), rtol=0, atol=1e-12)     # ... the increments do not
    assert np.allclose(inc, T.step_deg(A, f.ravel(), b, N, P)[0], rtol=0, atol=1e-12)


@pytest.fixture(scope="module")
def recovered():
    return T.recover(32, 31, 3)


def test_recovery_in_binary64(recovered):
    """N = 32, P = 31, +-4 degrees, 100 SIRT iterations per pass.  This run: rms 2.230 -> 0.763 -> 0.513 -> 0.463 degrees (0.34 x after
    pass 1), sum rr 92.4 -> 8.60 -> 5.08."""
    rms, rr = recovered["rms"], recovered["rr"]
    print("rms", np.round(rms, 4), "rr", np.round(rr, 3))
    assert rms[1] <= 0.5 * rms[0]
    assert rr[0] > rr[1] > rr[2]


def test_tilt_increment_edge_cases():
    from tomo_tv_amd.align import tilt_increment
    rd, dd = np.array([0.02, -0.01, 0.5, 0.0]), np.array([1.0, 2.0, 0.0, 4.0])
    raw = np.rad2deg([0.02, -0.005, 0.0, 0.0])                      # dd == 0: a zero step, whatever rd is
    assert np.allclose(tilt_increment(rd, dd), raw - raw.mean(), rtol=0, atol=1e-15)
    assert np.allclose(tilt_increment(rd, dd, damping=0.5), 0.5 * (raw - raw.mean()), rtol=0, atol=1e-15)
    clipped = np.clip(raw, -0.5, 0.5)                                # the clip comes BEFORE the mean is removed
    assert raw.max() > 0.5
    assert np.allclose(tilt_increment(rd, dd, max_step_deg=0.5), clipped - clipped.mean(), rtol=0, atol=1e-15)
    assert not tilt_increment(np.zeros(3), np.zeros(3)).any()
    for bad in (dict(damping=0.0), dict(damping=1.5), dict(max_step_deg=0.0)):
        with pytest.raises(ValueError):
            tilt_increment(rd, dd, **bad)
    with pytest.raises(ValueError):
        tilt_increment([np.nan], [1.0])
    with pytest.raises(ValueError):
        tilt_increment([1.0], [-1.0])


def test_sums_statement_counts_and_margin():
    rng = np.random.default_rng(2)
    B, G, D = (rng.standard_normal((2, 9, 5)) for _ in range(3))
    for m, n in ((0, 45), (1, 21), (2, 5)):
        out = T.tilt_normal(B, G, D, m)
        assert np.all(out[:, 3] == n)
    r = (B - G)[:, 1:-1, 1:-1]
    assert np.allclose(T.tilt_normal(B, G, D, 1)[:, 0], np.sum(r * D[:, 1:-1, 1:-1], (1, 2)), rtol=1e-13)
