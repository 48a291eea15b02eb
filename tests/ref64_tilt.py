"""Binary64 statements of the two kernels of the tilt-angle refinement (``tomo_volume_rot_derivative``, ``tomo_sino_tilt_normal``), a
binary32 replay of the first in the kernel's order of operations, a-priori error bounds for both, and the small dense-matrix
experiment the CPU and GPU tests share.  numpy only; written from the definitions in include/tomo_hip.h.

Convention (the system matrix's, cpu/utils/pytvlib.py:8-121): the pixel i * N + j of a slice sits at X = j - (N - 1) / 2,
Y = (N - 1) / 2 - i; ray t of angle theta runs through (t cos, t sin) along (-sin, cos).  D f = X d_Y f - Y d_X f with central
differences, the difference ACROSS the border taken as 0:
    dy[i][j] = f[i - 1][j] - f[i + 1][j]  (0 for i = 0 and i = N - 1; i grows against Y),   dx[i][j] = f[i][j + 1] - f[i][j - 1]  (0 for j = 0, N - 1)
    D f = (X / 2) dy - (Y / 2) dx.
Volumes are ``f[s][i][j]``; sinogram images ``X[a][r][s]`` (``ref64_align.images`` / ``packed`` convert to the engine's host layout).

Bound of ``rot_derivative_bound`` (u = 2^-24).  The kernel rounds four times per voxel: the two differences, the product
q = (Y / 2) dx, and the fused multiply-add fma(X / 2, dy, -q); the halved coordinates are exact.  With |e_k| <= u,
    got = ((X/2) dy (1 + e1) - (Y/2) dx (1 + e2)(1 + e3)) (1 + e4),
so  |got - D f| <= |X/2||dy| (2 u + u^2) + |Y/2||dx| (3 u + 3 u^2 + u^3)  <=  3.01 u (|X||d_Y f| + |Y||d_X f|)
with d_Y f = dy / 2, d_X f = dx / 2 the exact differences of the binary32 input.  Where a result or q falls into the subnormal range a
rounding is absolute, at most 2^-150 each: TINY = 2^-148 is added.  Derived from the operation count, not fitted.

Bound of ``tilt_normal_bound`` (v = 2^-53).  Every term is formed and added in binary64: res = b - g rounds once, the product inside
the fused multiply-add does not round, and a sum of n terms in ANY order (a thread's chain, the wave tree, the waves, the workgroups)
has error at most gamma_{n - 1} sum |term|.  Per sum: (n + 3) v sum |term| / (1 - (n + 3) v) covers the two roundings of res in
res^2, the one in res d, and the additions.  The count is exact (integers far below 2^53)."""
import numpy as np

U = 2.0 ** -24
V = 2.0 ** -53
TINY = 2.0 ** -148


def _coords(N):
    c = 0.5 * (N - 1)
    X = (np.arange(N, dtype=np.float64) - c)[None, None, :]
    Y = (c - np.arange(N, dtype=np.float64))[None, :, None]
    return X, Y


def _differences(f):
    """(dy, dx) of f[s][i][j] in f's own dtype, one rounding each where that is binary32"""
    dy, dx = np.zeros_like(f), np.zeros_like(f)
    dy[:, 1:-1, :] = f[:, :-2, :] - f[:, 2:, :]
    dx[:, :, 1:-1] = f[:, :, 2:] - f[:, :, :-2]
    return dy, dx


def rot_derivative(f):
    """D f of the volume f[s][i][j] in binary64 (the input is taken as it is: pass the binary32 data the engine holds)"""
    f = np.asarray(f, np.float64)
    X, Y = _coords(f.shape[-1])
    dy, dx = _differences(f)
    return (0.5 * X) * dy - (0.5 * Y) * dx


def rot_derivative_bound(f):
    """per-element bound of |kernel - rot_derivative(f)| (module docstring)"""
    f = np.asarray(f, np.float64)
    X, Y = _coords(f.shape[-1])
    dy, dx = _differences(f)
    return 3.01 * U * (np.abs(X) * np.abs(0.5 * dy) + np.abs(Y) * np.abs(0.5 * dx)) + TINY


def rot_derivative_f32(f):
    """The kernel's arithmetic replayed in binary32: two subtractions, q = (0.5 Y) dx, fma(0.5 X, dy, -q).  The fused multiply-add is
    formed in binary64 (the product of two binary32 numbers is exact there) and rounded to binary32."""
    f = np.ascontiguousarray(f, np.float32)
    N = f.shape[-1]
    c = np.float32(0.5) * np.float32(N - 1)
    hx = (np.float32(0.5) * (np.arange(N, dtype=np.float32) - c))[None, None, :]
    hy = (np.float32(0.5) * (c - np.arange(N, dtype=np.float32)))[None, :, None]
    assert np.all(hx.astype(np.float64) == 0.5 * _coords(N)[0]) and np.all(hy.astype(np.float64) == 0.5 * _coords(N)[1])   # exact
    dy, dx = _differences(f)
    q = (hy * dx).astype(np.float32)
    return (hx.astype(np.float64) * dy.astype(np.float64) - q.astype(np.float64)).astype(np.float32)


# ---- the per-projection sums -------------------------------------------------------------------------------------------------------
def _mask(N, ns, margin):
    r, s = np.arange(N)[:, None], np.arange(ns)[None, :]
    return (r >= margin) & (r <= N - 1 - margin) & (s >= margin) & (s <= ns - 1 - margin)


def tilt_normal(B, G, D, margin=1):
    """(P, 4) float64: per projection sum (b - g) d, sum d^2, sum (b - g)^2 and the count over the samples ``margin`` inside the image;
    B, G, D are X[a][r][s]"""
    return tilt_normal_bound(B, G, D, margin)[0]


def tilt_normal_bound(B, G, D, margin=1):
    """-> (the (P, 4) sums, the bound of |kernel - statement| for each; 0 for the count)"""
    B, G, D = (np.asarray(x, np.float64) for x in (B, G, D))
    P, N, ns = B.shape
    ok = _mask(N, ns, margin)
    n = int(ok.sum())
    out, bnd = np.zeros((P, 4)), np.zeros((P, 4))
    k = (n + 3) * V / (1.0 - (n + 3) * V)
    for a in range(P):
        res, d = (B[a] - G[a])[ok], D[a][ok]
        terms = (res * d, d * d, res * res)
        out[a] = [np.sum(t) for t in terms] + [n]       # numpy's pairwise sum: its own error is inside k sum |term| as well
        bnd[a, :3] = [2.0 * k * np.sum(np.abs(t)) for t in terms]   # kernel against exact + this statement against exact
    return out, bnd


# ---- the dense-matrix experiment ---------------------------------------------------------------------------------------------------
def dense_matrix(N, angles_deg):
    """the oracle's parallel_ray as a dense binary64 (P * N, N * N) matrix, row = angle * N + ray"""
    import oracle
    A3 = oracle.parallel_ray(N, np.asarray(angles_deg, np.float64))
    A = np.zeros((len(angles_deg) * N, N * N))
    np.add.at(A, (A3[0].astype(np.int64), A3[1].astype(np.int64)), A3[2].astype(np.float64))
    return A


def blobs(N):
    """a sum of four super-Gaussian blobs, f[i][j] in binary64: smooth, zero towards the border, no symmetry; placed a third of the
    image away from the tilt axis, where an angle error moves detail most"""
    X, Y = _coords(N)
    X, Y = np.broadcast_arrays(X[0], Y[0])
    f = np.zeros((N, N))
    for cx, cy, rx, ry, amp in ((-0.3125, 0.09375, 0.078125, 0.125, 1.0), (0.21875, 0.3125, 0.125, 0.0625, 0.8),
                                (0.3125, -0.1875, 0.0625, 0.125, 0.9), (-0.15625, -0.3125, 0.125, 0.0625, 0.7)):
        f += amp * np.exp(-(((X / N - cx) / rx) ** 2 + ((Y / N - cy) / ry) ** 2) ** 2)
    return f


def angle_case(P, spread_deg=4.0, seed=1):
    """(nominal, true) angles in degrees: linspace(-70, 70, P) and that plus uniform(-spread, spread) with the mean removed"""
    nominal = np.linspace(-70.0, 70.0, P)
    err = np.random.default_rng(seed).uniform(-spread_deg, spread_deg, P)
    return nominal, nominal + (err - err.mean())


def rms_centered(angles, truth):
    e = np.asarray(angles, np.float64) - np.asarray(truth, np.float64)
    return float(np.sqrt(np.mean((e - e.mean()) ** 2)))


def sirt(A, b, niter):
    """niter normalised SIRT iterations from zero with a positivity clamp per pass: x <- max(0, x + C A^T R (b - A x))"""
    rs, cs = A.sum(1), A.sum(0)
    R, C = np.where(rs > 0, 1.0 / np.where(rs > 0, rs, 1.0), 0.0), np.where(cs > 0, 1.0 / np.where(cs > 0, cs, 1.0), 0.0)
    x = np.zeros(A.shape[1])
    for _ in range(int(niter)):
        x = np.maximum(0.0, x + C * (A.T @ (R * (b - A @ x))))
    return x


def step_deg(A, x, b, N, P):
    """(the Gauss-Newton increments in degrees with the mean removed, rr per projection) at the volume x (one slice, flat)"""
    g = (A @ x).reshape(P, N)
    d = (A @ rot_derivative(x.reshape(1, N, N)).ravel()).reshape(P, N)
    r = b.reshape(P, N) - g
    rd, dd = np.sum(r * d, axis=1), np.sum(d * d, axis=1)
    inc = np.rad2deg(np.where(dd > 0, rd / np.where(dd > 0, dd, 1.0), 0.0))
    return inc - inc.mean(), np.sum(r * r, axis=1)


def recover(N, P, passes, sirt_iters=100, spread_deg=4.0, seed=1):
    """The recovery experiment in binary64: data at the true angles, ``passes`` passes of (SIRT at the current angles, one step) from
    the nominal ones.  -> dict(rms = [before, after pass 1, ...], rr = [sum of rr at pass 1, ...])"""
    nominal, truth = angle_case(P, spread_deg, seed)
    b = dense_matrix(N, truth) @ blobs(N).ravel()
    ang = nominal.copy()
    out = dict(rms=[rms_centered(ang, truth)], rr=[])
    for _ in range(int(passes)):
        A = dense_matrix(N, ang)
        inc, rr = step_deg(A, sirt(A, b, sirt_iters), b, N, P)
        ang = ang + inc
        out["rms"].append(rms_centered(ang, truth))
        out["rr"].append(float(rr.sum()))
    return out
