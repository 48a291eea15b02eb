"""Binary64 statement of ``tomo_volume_affine`` / ``tomo_volume_affine_axpy``, a per-element error bound, a binary32 replay of the
kernel's arithmetic, the matrix builder's inverse-map statement and the binary64 replay of the registered dual-axis loop.  numpy
only; written from the text of include/tomo_hip.h and the docstrings of ``align.affine_matrix_3d`` / ``DualAxisTomo``, not from the
kernel.

Volumes are ``X[s][y][z]``.  ``M`` holds the 12 entries of a row-major 3 x 4 matrix that maps a destination voxel (s, y, z) to its
source position ``s' = m00 s + m01 y + m02 z + m03`` (y', z' likewise); ``dst[s][y][z]`` is the trilinear interpolation of ``src``
there, the eight taps at floor and floor + 1 per axis with weights (1 - t, t), taps outside the source being zero and a tap of
weight zero being left out (not multiplied by zero, so an Inf beside a copied sample stays out).

The bound of ``bound`` (u = 2^-24), per output element:

* Arithmetic, in units of ``sum |w x|`` over the kept taps: a weight (wy wz) ws carries at most three roundings on its longest
  path (one subtraction 1 - t, two products), the first product w x one more, and each of the at most seven fused multiply-adds
  one on the running sum, whose magnitude stays below ``sum |w x|`` up to these same terms.  The usual recursive-sum argument gives
  at most (3 + 8) u = 11 u to first order; taken as 12 u = 6 * 2^-23.
* Position, per axis: the kernel interpolates at a position that differs from the exact one by ``delta`` along that axis, and a
  trilinear interpolant changes by at most ``delta * (max tap - min tap)`` of its cell along one axis (its slope there is the
  difference of two bilinear face values, each between the smallest and the largest tap).  ``delta`` = 2^-24, the rounding of a
  fraction in [0, 1) to binary32 (2^-25 would do; the spare factor pays for the weights of the first term being those of the moved
  position), plus the binary64 error of the coordinate on both sides: the kernel's three fused multiply-adds and this file's six
  plain operations, nine roundings each below 2^-53 of ``|m0| s + |m1| y + |m2| z + |m3|`` -- taken as 12 * 2^-53 of it.
  Trilinear interpolation is continuous across cells, so a floor that differs by one changes nothing in this argument except whose
  taps the slope is made of: where the exact coordinate lies within ``delta`` of an integer along an axis, ``max tap - min tap`` is
  taken over the taps of both cells that meet there.
"""
import numpy as np

import ref64_dual as D

U = 2.0 ** -24
DCOORD = 12.0 * 2.0 ** -53
ARITH = 12.0 * U


# ---- the matrix builder's statement ------------------------------------------------------------------------------------------------
def rotation(rotation_deg, flip_sign=False):
    """R = Rz Ry Rs in (s, y, z) coordinates; each right-handed in the cyclic order s -> y -> z -> s: about s a point on +y moves
    towards +z, about y a point on +z towards +s, about z a point on +s towards +y (so a point on +y towards -s)."""
    a, b, g = np.deg2rad(np.asarray(rotation_deg, np.float64) * (-1.0 if flip_sign else 1.0))
    Rs = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    Rz = np.array([[np.cos(g), -np.sin(g), 0], [np.sin(g), np.cos(g), 0], [0, 0, 1]])
    return Rz @ Ry @ Rs


def matrix(rotation_deg, shift, magnification, src_shape, dst_shape=None, corner=False, flip_sign=False, transpose=False):
    """The inverse-map statement: the content is moved by ``dst = c_dst + mag R (src - c_src) + shift`` with c = (size - 1) / 2 per
    axis, and the 12 entries are ``src = R^T / mag (dst - c_dst - shift) + c_src``.  ``corner`` / ``flip_sign`` / ``transpose`` are
    the deliberately wrong forms the CPU tests must see outside the bound."""
    src = np.asarray(src_shape, np.float64)
    dst = src if dst_shape is None else np.asarray(dst_shape, np.float64)
    cs, cd = (np.zeros(3), np.zeros(3)) if corner else (0.5 * (src - 1), 0.5 * (dst - 1))
    A = rotation(rotation_deg, flip_sign).T / float(magnification)
    if transpose:
        A = A.T
    M = np.empty((3, 4))
    M[:, :3], M[:, 3] = A, cs - A @ (cd + np.asarray(shift, np.float64))
    return M.ravel()


def forward_point(p, rotation_deg, shift, magnification, src_shape, dst_shape=None):
    """where the content at source position p lands"""
    src = np.asarray(src_shape, np.float64)
    dst = src if dst_shape is None else np.asarray(dst_shape, np.float64)
    return 0.5 * (dst - 1) + magnification * rotation(rotation_deg) @ (np.asarray(p, np.float64) - 0.5 * (src - 1)) + np.asarray(shift, np.float64)


def apply(M, p):
    M = np.asarray(M, np.float64).reshape(3, 4)
    return M[:, :3] @ np.asarray(p, np.float64) + M[:, 3]


# ---- the statement -----------------------------------------------------------------------------------------------------------------
def _grid(dst_shape):
    return np.meshgrid(*(np.arange(n, dtype=np.float64) for n in dst_shape), indexing="ij")


def _coords(M, dst_shape):
    m = np.asarray(M, np.float64).reshape(3, 4)
    s, y, z = _grid(dst_shape)
    c = [m[a, 0] * s + m[a, 1] * y + m[a, 2] * z + m[a, 3] for a in range(3)]
    mag = [abs(m[a, 0]) * s + abs(m[a, 1]) * y + abs(m[a, 2]) * z + abs(m[a, 3]) for a in range(3)]
    return c, mag


def _tap(X, i, j, k):
    """X[i][j][k] with zero outside the volume; integer arrays"""
    a, b, c = X.shape
    inside = (i >= 0) & (i < a) & (j >= 0) & (j < b) & (k >= 0) & (k < c)
    return np.where(inside, X[np.clip(i, 0, a - 1), np.clip(j, 0, b - 1), np.clip(k, 0, c - 1)], 0.0)


def _floor_int(x, size):
    """floor as int64 pinned just outside [-2, size + 1] (every tap is outside there anyway) and the fraction (0 when pinned)"""
    f = np.floor(np.where(np.isfinite(x), x, -4.0))
    far = (f <= -4.0) | (f >= size + 3.0) | ~np.isfinite(x)
    return np.clip(f, -4.0, size + 3.0).astype(np.int64), np.where(far, 0.0, x - f)


def affine(X, M, dst_shape=None):
    """-> (dst, sum |w x| of every output element), binary64"""
    X = np.asarray(X, np.float64)
    dst_shape = X.shape if dst_shape is None else tuple(dst_shape)
    c, _ = _coords(M, dst_shape)
    (i, ts), (j, ty), (k, tz) = (_floor_int(c[a], X.shape[a]) for a in range(3))
    out, mag = np.zeros(dst_shape), np.zeros(dst_shape)
    for di, ws in ((0, 1.0 - ts), (1, ts)):
        for dj, wy in ((0, 1.0 - ty), (1, ty)):
            for dk, wz in ((0, 1.0 - tz), (1, tz)):
                w = ws * wy * wz
                with np.errstate(invalid="ignore"):
                    term = np.where(w == 0.0, 0.0, w * _tap(X, i + di, j + dj, k + dk))
                out += term
                mag += np.abs(term)
    return out, mag


def affine_loops(X, M, dst_shape=None):
    """the same with three plain loops and eight explicit taps"""
    X = np.asarray(X, np.float64)
    dst_shape = X.shape if dst_shape is None else tuple(dst_shape)
    m = np.asarray(M, np.float64).reshape(3, 4)
    out = np.zeros(dst_shape)
    for s in range(dst_shape[0]):
        for y in range(dst_shape[1]):
            for z in range(dst_shape[2]):
                p = [m[a, 0] * s + m[a, 1] * y + m[a, 2] * z + m[a, 3] for a in range(3)]
                f = [int(np.floor(v)) for v in p]
                t = [v - fl for v, fl in zip(p, f)]
                acc = 0.0
                for di in (0, 1):
                    for dj in (0, 1):
                        for dk in (0, 1):
                            w = (t[0] if di else 1 - t[0]) * (t[1] if dj else 1 - t[1]) * (t[2] if dk else 1 - t[2])
                            q = (f[0] + di, f[1] + dj, f[2] + dk)
                            if w != 0.0 and all(0 <= q[a] < X.shape[a] for a in range(3)):
                                acc += w * X[q]
                out[s, y, z] = acc
    return out


def bound(X, M, dst_shape=None):
    """per-element bound of |kernel - affine| (module docstring)"""
    X = np.asarray(X, np.float64)
    dst_shape = X.shape if dst_shape is None else tuple(dst_shape)
    _, mag = affine(X, M, dst_shape)
    c, cm = _coords(M, dst_shape)
    delta = [U + DCOORD * cm[a] for a in range(3)]
    idx, lo, hi = [], [], []
    for a in range(3):
        i, t = _floor_int(c[a], X.shape[a])
        idx.append(i)
        lo.append(np.where(t <= delta[a], -1, 0))
        hi.append(np.where(1.0 - t <= delta[a], 2, 1))
    tmax, tmin = np.full(dst_shape, -np.inf), np.full(dst_shape, np.inf)
    for di in (0, 1):
        for dj in (0, 1):
            for dk in (0, 1):
                t = _tap(X, idx[0] + di, idx[1] + dj, idx[2] + dk)
                tmax, tmin = np.maximum(tmax, t), np.minimum(tmin, t)
    # the few voxels within delta of a cell face: the taps of both cells
    near = np.nonzero((lo[0] < 0) | (lo[1] < 0) | (lo[2] < 0) | (hi[0] > 1) | (hi[1] > 1) | (hi[2] > 1))
    if near[0].size:
        sub = [v[near] for v in idx]
        slo, shi = [v[near] for v in lo], [v[near] for v in hi]
        smax, smin = tmax[near], tmin[near]
        for di in (-1, 0, 1, 2):
            for dj in (-1, 0, 1, 2):
                for dk in (-1, 0, 1, 2):
                    use = ((di >= slo[0]) & (di <= shi[0]) & (dj >= slo[1]) & (dj <= shi[1]) & (dk >= slo[2]) & (dk <= shi[2]))
                    t = _tap(X, sub[0] + di, sub[1] + dj, sub[2] + dk)
                    smax, smin = np.where(use, np.maximum(smax, t), smax), np.where(use, np.minimum(smin, t), smin)
        tmax[near], tmin[near] = smax, smin
    return ARITH * mag + (delta[0] + delta[1] + delta[2]) * (tmax - tmin)


def ratio(got, ref, bnd):
    """worst |got - ref| / bound over the elements with a positive bound; an element with bound 0 must be exact (inf otherwise)"""
    err = np.abs(np.asarray(got, np.float64) - ref)
    if np.any((bnd == 0) & (err != 0)) or not np.all(np.isfinite(err)):
        return np.inf
    pos = bnd > 0
    return float(np.max(err[pos] / bnd[pos])) if pos.any() else 0.0


def axpy(value, Dst, a, clamp=False):
    """``Dst + a value`` in binary64 (a rounded to binary32 first, as the C call receives it), then the clamp in the sense of fmaxf"""
    with np.errstate(invalid="ignore"):
        v = float(np.float32(a)) * np.asarray(value, np.float64) + np.asarray(Dst, np.float64)
        if clamp:
            v = np.where(np.isnan(v), 0.0, np.maximum(v, 0.0))
    return v


# ---- the kernel's arithmetic restated ------------------------------------------------------------------------------------------------
def affine_replay_f32(X, M, dst_shape=None, nearest=False, swap_fractions=False):
    """Coordinates and their split in binary64 (the chain inner link first), the fraction rounded to binary32 (a fraction that rounds
    to 1 is the next whole voxel), weights (1 - t, t) in binary32 with weight exactly 1 and a single tap where t = 0, the kept taps in
    ascending (dy, dz, ds) order: the first as ((wy wz) ws) x, the others by a fused multiply-add (here: the product exact in
    binary64, added there and rounded to binary32).  A voxel with three zero fractions copies its tap.
    ``nearest`` / ``swap_fractions``: deliberately wrong forms for the CPU tests (the nearest sample; the fractions of y and z swapped)."""
    X = np.asarray(X, np.float32)
    dst_shape = X.shape if dst_shape is None else tuple(dst_shape)
    m = np.asarray(M, np.float64).reshape(3, 4)
    s, y, z = _grid(dst_shape)
    one, zero = np.float32(1.0), np.float32(0.0)
    idx, frac, inside = [], [], np.ones(dst_shape, bool)
    for a in range(3):
        c = m[a, 0] * s + (m[a, 1] * y + (m[a, 2] * z + m[a, 3]))
        with np.errstate(invalid="ignore"):
            ok = (c > -1.0) & (c < X.shape[a])
        inside &= ok
        c = np.where(ok, c, 0.0)
        f = np.floor(c)
        t = (c - f).astype(np.float32)
        i = f.astype(np.int64)
        idx.append(np.where(t >= one, i + 1, i))
        frac.append(np.where(t >= one, zero, t))
    if nearest:
        out = _tap(X, *(i + (t >= np.float32(0.5)) for i, t in zip(idx, frac))).astype(np.float32)
        return np.where(inside, out, zero)
    if swap_fractions:
        frac[1], frac[2] = frac[2], frac[1]
    (i, ts), (j, ty), (k, tz) = zip(idx, frac)
    w = {0: [np.where(t == 0, one, one - t) for t in (ts, ty, tz)], 1: [ts, ty, tz]}
    out = np.zeros(dst_shape, np.float64)
    first = True
    with np.errstate(invalid="ignore", over="ignore"):
        for dy in (0, 1):
            for dz in (0, 1):
                for ds in (0, 1):
                    kept = ((ts != 0) | (ds == 0)) & ((ty != 0) | (dy == 0)) & ((tz != 0) | (dz == 0))
                    wt = (w[dy][1] * w[dz][2]) * w[ds][0]                          # binary32, one rounding per product
                    x = _tap(X, i + ds, j + dy, k + dz).astype(np.float32)
                    if first:
                        out = (wt * x).astype(np.float64)
                        first = False
                    else:
                        new = (wt.astype(np.float64) * x.astype(np.float64) + out).astype(np.float32).astype(np.float64)
                        out = np.where(kept, new, out)
    copy = (ts == 0) & (ty == 0) & (tz == 0)
    out = np.where(copy, _tap(X, i, j, k), out)
    return np.where(inside, out, 0.0).astype(np.float32)


# ---- the registered dual-axis loop (DualAxisTomo.sirt after set_registration) --------------------------------------------------------
def moved_series_b(MB, X, to_b):
    """what series B measures of a volume of record X under a registration: A_B cross(T^-1 X)"""
    return D.fp_b(MB, affine(X, to_b)[0])


def dual_axis_registered(MA, MB, bA, bB, tA, tB, niter, to_a, to_b, x0=None):
    """Per iteration: a Landweber step on A; B's copy xb = cross(T^-1 x) (one interpolation of a scratch copy); B's step; only the
    increment comes back, x <- max(0, x + T cross(xb_new - xb)).  -> (x, B's data distance of the final x)"""
    N = MA.N
    x = np.zeros((N, N, N)) if x0 is None else np.array(x0, np.float64)
    for _ in range(int(niter)):
        x = D.landweber(MA, x, bA, tA)
        xb = D.cross(affine(x, to_b)[0])
        xb_new = D.landweber(MB, xb, bB, tB)
        x = np.maximum(x + affine(D.cross(xb_new - xb), to_a)[0], 0.0)
    dd_b = float(np.sqrt(np.sum((moved_series_b(MB, x, to_b) - np.asarray(bB, np.float64).reshape(N, MB.nrow)) ** 2)))
    return x, dd_b
