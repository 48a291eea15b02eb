"""Binary64 statements of ``tomo_sino_bin`` / ``tomo_volume_bin`` / ``tomo_volume_prolong``, binary32 replays of the kernels' arithmetic
in the order include/tomo_hip.h gives, per-element error bounds, and projection matching over a pyramid of binned series replayed on
the CPU.  numpy only; written from the definitions in the header, not from the kernels.

Sinograms are images ``X[a][r][s]`` (tests/ref64_align.py); volumes are ``V[s][y][z]``, the public (Nslice, Nray, Nray) layout.
f is the factor (2 or 4), k = min(f, Nslice - f s') the number of fine slices in coarse slice s', c = 1 / (f^2 k).

Bounds (u = 2^-24, gamma_m = m u / (1 - m u), ``ref64_align.gamma``):

* bins.  A bin adds m samples in binary32 from the first one on (m = f k for a sinogram, f^2 k for a volume): m - 1 roundings, then one
  multiply by c: m roundings, ``gamma(m) * c * sum |x|``.  c is a power of two except for k = 3 (1/48 at f = 4), where its own rounding
  is one more: gamma(m + 1).
* prolongation.  A lerp fma(t, b - a, a) rounds b - a and the fma: |error| <= u t |b - a| + u |a + t (b - a)| <= 2 u (|a| + |b|), and
  passes errors of a and b on with weights 1 - t and t, i.e. not enlarged.  Every intermediate value is a convex combination of the
  eight taps, so |a| + |b| <= 2 T with T = max |tap| at each of the three levels: 12 u T, six ulp of the largest tap; ``PROLONG_SLACK``
  covers the second-order terms.
"""
import numpy as np

from ref64_align import U, gamma, peaks, shift_int, xcorr

PROLONG_SLACK = 1.0 + 1e-5


def counts(ns, f):
    """k of every coarse slice"""
    return np.minimum(f, ns - f * np.arange(-(-ns // f)))


def _blocks(X, f, axes_full, axis_s):
    """sum and sum of magnitudes over the bins: the full axes in blocks of f, the slice axis zero-padded to whole bins"""
    X = np.asarray(X, np.float64)
    ns = X.shape[axis_s]
    pad = [(0, 0)] * X.ndim
    pad[axis_s] = (0, -(-ns // f) * f - ns)
    out = []
    for Y in (X, np.abs(X)):
        Y = np.pad(Y, pad)
        shape = []
        for ax, n in enumerate(Y.shape):
            shape += [n // f, f] if ax in axes_full or ax == axis_s else [n]
        Y = Y.reshape(shape)
        red, k = [], 0
        for ax in range(X.ndim):
            if ax in axes_full or ax == axis_s:
                red.append(k + 1)
                k += 2
            else:
                k += 1
        with np.errstate(invalid="ignore"):
            out.append(Y.sum(axis=tuple(red)))
    return out


def bin_sino(X, f):
    """-> (dst[a][r'][s'] = c sum_{i<f, j<k} X[a][f r' + i][f s' + j], its bound)"""
    X = np.asarray(X, np.float64)
    assert X.shape[1] % f == 0
    k = counts(X.shape[2], f)
    c = 1.0 / (f * f * k)
    s, mag = _blocks(X, f, (1,), 2)
    m = f * k + (np.log2(f * f * k) % 1 != 0)
    return s * c, gamma(m) * c * mag


def bin_volume(V, f):
    """V[s][y][z] -> (the mean over the f x f x k blocks [s'][y'][z'], its bound)"""
    V = np.asarray(V, np.float64)
    assert V.shape[1] % f == 0 and V.shape[2] % f == 0
    k = counts(V.shape[0], f)
    c = (1.0 / (f * f * k))[:, None, None]
    s, mag = _blocks(V, f, (1, 2), 0)
    m = (f * f * k + (np.log2(f * f * k) % 1 != 0))[:, None, None]
    return s * c, gamma(m) * c * mag


def bin_sino_loops(X, f):
    """the definition as plain loops"""
    X = np.asarray(X, np.float64)
    P, N, ns = X.shape
    out = np.zeros((P, N // f, -(-ns // f)))
    for a in range(P):
        for r in range(N // f):
            for s in range(out.shape[2]):
                k = min(f, ns - f * s)
                out[a, r, s] = sum(X[a, f * r + i, f * s + j] for i in range(f) for j in range(k)) / (f * f * k)
    return out


def bin_volume_loops(V, f):
    V = np.asarray(V, np.float64)
    ns, N, _ = V.shape
    out = np.zeros((-(-ns // f), N // f, N // f))
    for s in range(out.shape[0]):
        k = min(f, ns - f * s)
        for y in range(N // f):
            for z in range(N // f):
                out[s, y, z] = np.mean(V[f * s:f * s + k, f * y:f * y + f, f * z:f * z + f])
    return out


def bin_replay_f32(X, f, volume=False, partial_as_full=False):
    """The kernels' arithmetic: binary32 additions in ascending (i, j) order for a sinogram X[a][r][s], ascending (y, z, s) for a
    volume V[s][y][z], from the first sample on, then one multiply by c rounded to binary32.  ``partial_as_full``: the deliberately
    wrong form that scales the trailing partial bin by 1 / f^3 as well."""
    X = np.asarray(X, np.float32)
    ns = X.shape[0] if volume else X.shape[2]
    nc = -(-ns // f)
    k = counts(ns, f)
    c = (np.float32(1.0) / (f * f * (np.full(nc, f) if partial_as_full else k)).astype(np.float32)).astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        if volume:
            acc = np.zeros((nc, X.shape[1] // f, X.shape[2] // f), np.float32)
            for y in range(f):
                for z in range(f):
                    for l in range(f):
                        sel = np.nonzero(l < k)[0]
                        acc[sel] = acc[sel] + X[f * sel + l, y::f, z::f]
            return acc * c[:, None, None]
        acc = np.zeros((X.shape[0], X.shape[1] // f, nc), np.float32)
        for i in range(f):
            for j in range(f):
                sel = np.nonzero(j < k)[0]
                acc[:, :, sel] = acc[:, :, sel] + X[:, i::f, f * sel + j]
        return acc * c


def axis_taps(nf, nc, f, half_cell=True, clamp=True):
    """taps (a, b) and the weight t of every fine index of one axis: u = (i + 0.5) / f - 0.5, floor(u) and floor(u) + 1 clamped to the
    coarse range.  The wrong forms: ``half_cell=False`` takes u = i / f, ``clamp=False`` wraps around instead of clamping."""
    i = np.arange(nf, dtype=np.float64)
    u = (i + 0.5) / f - 0.5 if half_cell else i / f
    fl = np.floor(u)
    a, b = fl.astype(np.int64), fl.astype(np.int64) + 1
    if clamp:
        a, b = np.clip(a, 0, nc - 1), np.clip(b, 0, nc - 1)
    else:
        a, b = a % nc, b % nc
    return a, b, u - fl


def _lerp(t, a, b, same, dtype):
    """fma(t, b - a, a) in ``dtype`` (binary32: the difference rounded, the product-and-add in binary64 rounded once); a copy where
    both taps are the same sample"""
    with np.errstate(invalid="ignore", over="ignore"):
        if dtype == np.float64:
            r = a + t * (b - a)
        else:
            d = (b - a).astype(np.float32)
            r = (t.astype(np.float64) * d.astype(np.float64) + a.astype(np.float64)).astype(np.float32)
    return np.where(same, a, r)


def _prolong(C, f, ns, dtype, **wrong):
    C = np.asarray(C, dtype)
    nsc, nc, _ = C.shape
    sa, sb, ts = axis_taps(ns, nsc, f, **wrong)
    ya, yb, ty = axis_taps(f * nc, nc, f, **wrong)
    ts, ty = ts.astype(dtype), ty.astype(dtype)
    v = _lerp(ts[:, None, None], C[sa], C[sb], (sa == sb)[:, None, None], dtype)              # along s
    v = _lerp(ty[None, None, :], v[:, :, ya], v[:, :, yb], (ya == yb)[None, None, :], dtype)   # along z
    return _lerp(ty[None, :, None], v[:, ya], v[:, yb], (ya == yb)[None, :, None], dtype)      # along y


def prolong(C, f, ns):
    """C[s'][y'][z'] -> (fine [s][y][z] with ``ns`` slices and f times the rows, its bound 12 u max |tap|)"""
    A = np.abs(np.asarray(C, np.float64))
    nsc, nc, _ = A.shape
    sa, sb, _ = axis_taps(ns, nsc, f)
    ya, yb, _ = axis_taps(f * nc, nc, f)
    T = np.maximum(A[sa], A[sb])
    T = np.maximum(T[:, :, ya], T[:, :, yb])
    T = np.maximum(T[:, ya], T[:, yb])
    return _prolong(C, f, ns, np.float64), 12.0 * U * PROLONG_SLACK * T


def prolong_replay_f32(C, f, ns, **wrong):
    return _prolong(C, f, ns, np.float32, **wrong)


def prolong_loops(C, f, ns):
    """the definition as plain loops: weights (1 - t, t) per axis on the clamped taps"""
    C = np.asarray(C, np.float64)
    nsc, nc, _ = C.shape
    out = np.zeros((ns, f * nc, f * nc))

    def taps(i, n):
        u = (i + 0.5) / f - 0.5
        fl = int(np.floor(u))
        return ((min(max(fl, 0), n - 1), 1.0 - (u - fl)), (min(max(fl + 1, 0), n - 1), u - fl))
    for s in range(ns):
        for y in range(f * nc):
            for z in range(f * nc):
                out[s, y, z] = sum(ws * wy * wz * C[js, jy, jz] for js, ws in taps(s, nsc) for jy, wy in taps(y, nc) for jz, wz in taps(z, nc))
    return out


# ---- projection matching over a pyramid, replayed on the CPU ------------------------------------------------------------------------
# 64 rays x 32 slices, 31 projections (the count at which the plain form works: tests/test_align_cpu.py), whole-pixel shifts of up to
# +-10 rays and +-10 slices, max_shift = 4: one level cannot see them (every window peaks on its border), the pyramid reaches 16.
# Phantom, seed and shifts chosen on the CPU so that the replay alone meets the test (tests/test_bin_cpu.py): of 80 combinations of
# phantom seed, shift seed, 3 or 4 passes and 10 or 20 iterations tried, this one ends within a pixel (0.99 rays, 0.55 slices outside
# the gauge); the others keep 1 to 2.5 pixels, the plain form's known remainder (ref64_align.PLAIN_CASE).
PYRAMID_CASE = dict(nslice=32, n=64, nproj=31, seed=11, shift_seed=2, span=10, max_shift=4, nouter=3, niter=20, pyramid=(4, 2, 1))


def pyramid_case(c=None):
    """(angles in degrees, the clean series, the misaligned one X[a][r][s] float32, the injected shifts)"""
    import oracle
    from ref64_align import images
    from tomo_tv_amd.phantom import ellipsoids, tilt_angles
    c = c or PYRAMID_CASE
    ang = tilt_angles(c["nproj"])
    o = oracle.ctvlib(c["nslice"], c["n"], c["nproj"])
    o.load_A(oracle.parallel_ray(c["n"], ang))
    o.original_volume = ellipsoids(c["nslice"], c["n"], seed=c["seed"])
    o.create_projections()
    clean = images(o.b, c["n"])
    inj = np.random.default_rng(c["shift_seed"]).integers(-c["span"], c["span"] + 1, (c["nproj"], 2))
    return ang, clean, shift_int(clean, inj, wrap=False), inj


def pyramid_replay(angles_deg, X, pyramid, nouter, max_shift, niter=20):
    """``TomoGPU.refine_alignment(subpixel=False, pyramid=...)`` on the CPU: per level the series, moved by the totals, is binned with
    the kernel's binary32 arithmetic, reconstructed by the oracle's SIRT from zero, projected and correlated in binary64; the
    whole-pixel peaks times the factor move the totals.  -> (totals after every pass, peaks of every pass in full-resolution pixels,
    border flags of every pass)"""
    import oracle
    from ref64_align import _model
    X = np.asarray(X, np.float32)
    P, N, ns = X.shape
    total = np.zeros((P, 2))
    cur, hist, pks, borders = X, [], [], []
    for f in pyramid:
        o = oracle.ctvlib(-(-ns // f), N // f, P)
        o.load_A(oracle.parallel_ray(N // f, angles_deg))
        for _ in range(nouter):
            lvl = cur if f == 1 else bin_replay_f32(cur, f)
            pk, border, _ = peaks(xcorr(_model(o, lvl, N // f, niter, False), lvl, max_shift), subpixel=False)
            pk = pk * f
            total = total - pk
            total[:, 1] -= np.round(total[:, 1].mean())
            cur = shift_int(X, total, wrap=False)
            hist.append(total.copy())
            pks.append(pk)
            borders.append(border)
    return hist, pks, borders
