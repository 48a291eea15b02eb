"""Binary64 statements of ``tomo_sino_affine`` and ``tomo_sino_axis_profile``, of the common-line score and of the tilt-axis
estimator built on them, with a per-element error bound and a binary32 replay of the kernel's arithmetic.  numpy only; written from
the definitions in include/tomo_hip.h and in the docstrings of ``TomoGPU``, not from the kernels.

Images: ``X[a][r][s]`` as in tests/ref64_align.py (``images`` / ``packed`` there convert from and to the engine's host layout).  A
matrix row ``(m00, m01, m02, m10, m11, m12)`` maps a destination sample (r, s) to its source position
``r' = m00 r + m01 s + m02``, ``s' = m10 r + m11 s + m12``; ``dst[r][s]`` is the bilinear interpolation of ``src`` there, taps outside
the image being zero and a tap of weight zero being left out (not multiplied by zero).

The bound of ``bound`` (u = 2^-24), two terms per output element:

* Arithmetic: the weights 1 - t (one rounding), their product (one), the four products with the samples (one each) and three
  additions -- at most 7 roundings on the longest path, 7 u < 4 ulp = 8 u of ``sum |w_i x_i|``, the figure ``ref64_align.shift``
  already justifies for the same four-tap expression.
* Position: the kernel interpolates at a position that differs from the exact (r', s') by ``delta_r``, ``delta_s``, and a bilinear
  interpolant changes by at most ``|delta| * (max tap - min tap)`` of its cell per axis (its slope along an axis is a difference of
  two interpolated values, each between the smallest and the largest tap).  ``delta`` = 2^-24, the rounding of a fraction in
  [0, 1) to binary32 (2^-25 would do: the spare factor 2 also pays for the weights of the first term being those of the moved
  position), plus the binary64 error of the coordinate on both sides: the kernel's two fused multiply-adds and this file's four
  plain operations, 6 roundings, each below 2^-53 of ``|m00| r + |m01| s + |m02|`` -- taken as 8 * 2^-53 of it.
  Bilinear interpolation is continuous across cells, so a floor that differs by one changes nothing in this argument -- except
  whose taps the slope is made of: where the exact coordinate lies within ``delta`` of an integer, the kernel may stand in the cell
  on the other side, and ``max tap - min tap`` is taken over the taps of both cells that meet there.
"""
import numpy as np

import ref64_align as RA

U = 2.0 ** -24
DCOORD = 8.0 * 2.0 ** -53


def matrices(shifts, rotation_deg, magnification, N, ns, corner=False, flip_sign=False, transpose=False):
    """(P, 6): the content is rotated by +rotation_deg about the centre ((N-1)/2, (ns-1)/2) -- counter-clockwise from the r axis
    towards the s axis --, scaled by the magnification, moved by +shift; the row is the inverse map
    ``src = R(-phi) / mag . (dst - c - d) + c``.  ``corner`` / ``flip_sign`` / ``transpose`` are the deliberately wrong forms the CPU tests
    must see outside the bound: rotation about the corner (c = 0), the sign of phi flipped, the 2 x 2 part transposed."""
    d = np.asarray(shifts, np.float64).reshape(-1, 2)
    P = d.shape[0]
    rot = np.broadcast_to(np.asarray(rotation_deg, np.float64), (P,))
    mag = np.broadcast_to(np.asarray(magnification, np.float64), (P,))
    c = np.zeros(2) if corner else np.array([0.5 * (N - 1), 0.5 * (ns - 1)])
    M = np.zeros((P, 6))
    for a in range(P):
        phi = np.deg2rad(-rot[a] if flip_sign else rot[a])
        A = np.array([[np.cos(phi), np.sin(phi)], [-np.sin(phi), np.cos(phi)]]) / mag[a]
        if transpose:
            A = A.T
        t = c - A @ (c + d[a])
        M[a] = (A[0, 0], A[0, 1], t[0], A[1, 0], A[1, 1], t[1])
    return M


def _coords(m, N, ns):
    r, s = np.meshgrid(np.arange(N, dtype=np.float64), np.arange(ns, dtype=np.float64), indexing="ij")
    return m[0] * r + m[1] * s + m[2], m[3] * r + m[4] * s + m[5], r, s


def _tap(Xa, i, j):
    """Xa[i][j] with zero outside the image; i, j integer arrays"""
    N, ns = Xa.shape
    inside = (i >= 0) & (i < N) & (j >= 0) & (j < ns)
    return np.where(inside, Xa[np.clip(i, 0, N - 1), np.clip(j, 0, ns - 1)], 0.0)


def _floor_int(x, size):
    """floor as int64, pinned just outside [-2, size + 1] (every tap is outside there anyway); nan -> outside"""
    f = np.floor(np.where(np.isfinite(x), x, -4.0))
    return np.clip(f, -4.0, size + 3.0).astype(np.int64), x - f


def affine(X, M):
    """dst[a][r][s] = bilinear(src_a)(r', s') in binary64, and sum |w_i x_i| of every output element"""
    X = np.asarray(X, np.float64)
    P, N, ns = X.shape
    out, mag = np.zeros_like(X), np.zeros_like(X)
    for a in range(P):
        rp, sp, _, _ = _coords(np.asarray(M[a], np.float64), N, ns)
        i, tr = _floor_int(rp, N)
        j, ts = _floor_int(sp, ns)
        far = (i <= -4) | (i >= N + 3) | (j <= -4) | (j >= ns + 3)
        tr, ts = np.where(far, 0.0, tr), np.where(far, 0.0, ts)
        for di, wr in ((0, 1.0 - tr), (1, tr)):
            for dj, ws in ((0, 1.0 - ts), (1, ts)):
                w = wr * ws
                with np.errstate(invalid="ignore"):
                    term = np.where(w == 0.0, 0.0, w * _tap(X[a], i + di, j + dj))
                out[a] += term
                mag[a] += np.abs(term)
    return out, mag


def bound(X, M):
    """per-element bound of |kernel - affine| (module docstring)"""
    X = np.asarray(X, np.float64)
    P, N, ns = X.shape
    _, mag = affine(X, M)
    pos = np.zeros_like(X)
    for a in range(P):
        m = np.asarray(M[a], np.float64)
        rp, sp, r, s = _coords(m, N, ns)
        dr = U + DCOORD * (abs(m[0]) * r + abs(m[1]) * s + abs(m[2]))
        ds = U + DCOORD * (abs(m[3]) * r + abs(m[4]) * s + abs(m[5]))
        i, tr = _floor_int(rp, N)
        j, ts = _floor_int(sp, ns)
        lo_i, hi_i = np.where(tr <= dr, -1, 0), np.where(1.0 - tr <= dr, 2, 1)
        lo_j, hi_j = np.where(ts <= ds, -1, 0), np.where(1.0 - ts <= ds, 2, 1)
        tmax, tmin = np.full((N, ns), -np.inf), np.full((N, ns), np.inf)
        for di in (-1, 0, 1, 2):
            for dj in (-1, 0, 1, 2):
                use = (di >= lo_i) & (di <= hi_i) & (dj >= lo_j) & (dj <= hi_j)
                t = _tap(X[a], i + di, j + dj)
                tmax, tmin = np.where(use, np.maximum(tmax, t), tmax), np.where(use, np.minimum(tmin, t), tmin)
        pos[a] = (dr + ds) * (tmax - tmin)
    return 4 * 2.0 ** -23 * mag + pos


def affine_replay_f32(X, M):
    """The kernel's arithmetic restated in numpy: coordinates and their split into floor and fraction in binary64, the fraction rounded
    to binary32 (a fraction that rounds to 1 is the next whole pixel), then the binary32 weights and sums of ``k_sino_shift`` in its
    order, one rounding per operation; a zero fraction drops its tap."""
    X = np.asarray(X, np.float32)
    P, N, ns = X.shape
    out = np.zeros_like(X)
    one = np.float32(1.0)
    for a in range(P):
        m = np.asarray(M[a], np.float64)
        r, s = np.meshgrid(np.arange(N, dtype=np.float64), np.arange(ns, dtype=np.float64), indexing="ij")
        rp, sp = m[0] * r + (m[1] * s + m[2]), m[3] * r + (m[4] * s + m[5])
        with np.errstate(invalid="ignore"):
            inside = (rp > -1.0) & (rp < N) & (sp > -1.0) & (sp < ns)
        rp, sp = np.where(inside, rp, 0.0), np.where(inside, sp, 0.0)
        fr, fs = np.floor(rp), np.floor(sp)
        tr, ts = (rp - fr).astype(np.float32), (sp - fs).astype(np.float32)
        i, j = fr.astype(np.int64), fs.astype(np.int64)
        i, tr = np.where(tr >= one, i + 1, i), np.where(tr >= one, np.float32(0.0), tr)
        j, ts = np.where(ts >= one, j + 1, j), np.where(ts >= one, np.float32(0.0), ts)
        f = [[_tap(X[a], i + di, j + dj).astype(np.float32) for dj in (0, 1)] for di in (0, 1)]
        wr, ws = one - tr, one - ts
        with np.errstate(invalid="ignore", over="ignore"):
            four = (wr * ws) * f[0][0] + (wr * ts) * f[0][1] + (tr * ws) * f[1][0] + (tr * ts) * f[1][1]
            only_s = (one - ts) * f[0][0] + ts * f[0][1]
            only_r = (one - tr) * f[0][0] + tr * f[1][0]
        o = np.where((tr == 0) & (ts == 0), f[0][0], np.where(tr == 0, only_s, np.where(ts == 0, only_r, four)))
        out[a] = np.where(inside, o, np.float32(0.0))
    return out


# ---- the per-slice mass profile, the common-line score, the estimator -----------------------------------------------------------
def profile(X):
    """c[a][s] = sum_r X[a][r][s] in binary64"""
    return np.asarray(X, np.float64).sum(axis=1)


def score_border(N, search_deg):
    """H = ceil(N/2 sin(search_deg)): the slices H <= s < ns - H never see zero fill under a rotation of up to search_deg"""
    return int(np.ceil(0.5 * N * np.sin(np.deg2rad(search_deg)) - 1e-12))


def score(c, H):
    """sum_s Var_a(c_a[s]) / sum_s mean_a(c_a[s])^2 over H <= s < ns - H (population variance over the projections)"""
    c = np.asarray(c, np.float64)
    ns = c.shape[1]
    if ns - 2 * H <= 0:
        raise ValueError("empty range of slices")
    c = c[:, H:ns - H]
    mean = c.mean(axis=0)
    return float(np.sum(((c - mean) ** 2).mean(axis=0)) / np.sum(mean ** 2))


def grid(search_deg, step_deg):
    K = int(np.floor(search_deg / step_deg + 1e-9))
    return step_deg * np.arange(-K, K + 1, dtype=np.float64)


def minimum(g, sc):
    """first grid minimum, 3-point parabola clamped to +-1/2 step; on the border: the grid value, flagged.
    -> (rotation, grid index, at_border)"""
    sc = np.asarray(sc, np.float64)
    k = int(np.argmin(sc))
    if k == 0 or k == len(sc) - 1:
        return float(g[k]), k, True
    den = sc[k - 1] - 2.0 * sc[k] + sc[k + 1]
    off = float(np.clip(0.5 * (sc[k - 1] - sc[k + 1]) / den, -0.5, 0.5)) if den > 0.0 else 0.0
    return float(g[k] + off * (g[1] - g[0])), k, False


def estimate(X, shifts, search_deg=10.0, step_deg=0.5, magnification=1.0):
    """``TomoGPU.estimate_tilt_axis_rotation`` on the CPU with the binary64 statement.  -> (rotation, grid index, at_border, grid, scores)"""
    X = np.asarray(X, np.float64)
    P, N, ns = X.shape
    H = score_border(N, search_deg)
    g = grid(search_deg, step_deg)
    sc = np.array([score(profile(affine(X, matrices(shifts, phi, magnification, N, ns))[0]), H) for phi in g])
    rot, k, border = minimum(g, sc)
    return rot, k, border, g, sc


# The estimator's case: Gaussian blobs (slice, y, x, sigma, amplitude) cut to zero beyond 3 sigma, all well inside the volume, so that
# every projection has a zero border and slices of different mass; projected by the oracle's matrix, then every projection rotated by
# PHI0 with the binary64 statement and rounded to binary32.  Chosen on the CPU so that the binary64 replay meets the acceptance (half a
# grid step).  The replay's result on this case (AXIS_REPLAY): grid minimum at -3.0 degrees (index 14 of 41, score 4.8e-5 against
# 7.8e-5 and 8.7e-5 beside it and 6.7e-7 for the series before it was rotated), -3.0323 degrees after the parabola.
AXIS_CASE = dict(nslice=32, n=32, nproj=9, phi0=3.0, search_deg=10.0, step_deg=0.5,
                 blobs=[(9.0, 13.0, 18.0, 1.6, 1.0), (13.5, 19.0, 12.5, 2.0, 0.8), (17.0, 14.0, 15.0, 1.4, 1.2),
                        (21.0, 17.5, 19.5, 1.8, 0.9), (24.0, 12.5, 13.0, 1.5, 1.1), (11.0, 18.0, 20.0, 1.3, 0.7)])
AXIS_REPLAY = dict(rotation=-3.0323, index=14)


def axis_volume(c=None):
    c = c or AXIS_CASE
    ns, n = c["nslice"], c["n"]
    z, y, x = np.meshgrid(np.arange(ns), np.arange(n), np.arange(n), indexing="ij")
    vol = np.zeros((ns, n, n))
    for (cz, cy, cx, sig, amp) in c["blobs"]:
        d2 = (z - cz) ** 2 + (y - cy) ** 2 + (x - cx) ** 2
        vol += np.where(d2 <= (3.0 * sig) ** 2, amp * np.exp(-d2 / (2.0 * sig ** 2)), 0.0)
    return vol.astype(np.float32)


def axis_case(c=None):
    """(angles in degrees, the clean series, the series rotated by phi0) as X[a][r][s] float32"""
    import oracle
    from tomo_tv_amd.phantom import tilt_angles
    c = c or AXIS_CASE
    ang = tilt_angles(c["nproj"])
    o = oracle.ctvlib(c["nslice"], c["n"], c["nproj"])
    o.load_A(oracle.parallel_ray(c["n"], ang))
    o.original_volume = axis_volume(c)
    o.create_projections()
    clean = RA.images(o.b, c["n"]).astype(np.float32)
    M = matrices(np.zeros((c["nproj"], 2)), c["phi0"], 1.0, c["n"], c["nslice"])
    return ang, clean, affine(clean, M)[0].astype(np.float32)
