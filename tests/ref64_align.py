"""Binary64 statements of the alignment operations (``tomo_sino_moments`` / ``tomo_sino_xcorr`` / ``tomo_sino_shift``), of the peak
rule and of the reference's centre-of-mass rule, with per-element error bounds.  numpy only; written from the definitions in
include/tomo_hip.h, not from the kernels.

Images: ``X[a][r][s]``, projection a, ray r in [0, N), slice s in [0, Nslice).  The engine's host sinogram is ``[s][a * N + r]``
(``images`` / ``packed`` convert).  A shift (dr, ds) moves content by +d: ``dst[r][s] = src(r - dr, s - ds)``, the sense of np.roll.

Bounds (u = 2^-24, gamma_m = m u / (1 - m u)):

* ``xcorr``.  The kernel (kernels_align.hip.h: k_sino_xcorr) adds the products of one window entry in this order: a lane (= slice
  modulo 64) runs a binary32 FMA chain over the 16 rows of its wave and the up to ``KC`` = 4 chunks of 64 slices of its workgroup --
  at most ``16 * min(KC, ceil(Nslice / 64))`` links, one rounding each --, the 64 lanes are added in a tree of depth 6, and everything
  after that (waves, workgroups) is binary64.  So with m = that chain length + 6 the summation costs at most
  ``gamma_m sum |a'_i b'_i|`` over the staged values a', b' (any tree of depth m obeys this), and the binary64 part fewer than 1e4
  additions, ``DSUM`` = 1e4 * 2^-53 relative to the same sum: nothing visible.
  The staged values carry the rounding of the mean subtraction: the kernel subtracts the binary32 rounding of the mean (whose
  binary64 value is exact to ~1e-13 relative: the moments are summed in binary64) and rounds the difference, so
  ``|a'_kernel - a'| <= da := 1.01 u (|mean_A| + |a'|)`` per sample, likewise db; without mean subtraction da = db = 0 (x - 0 is exact).
  Together: ``|C - C64| <= (1 + gamma_m + DSUM) sum (|a'| + da)(|b'| + db) - sum |a'||b'|`` per window entry, the sums over the
  overlap of that entry -- two more correlations of non-negative images.
* ``moments``.  Binary64 from the first sample on (x, r x and s x are exact there): fewer than N * Nslice additions per sum,
  relative error below N * Nslice * 2^-53 for the non-negative images the tests use -- ten orders below the 1e-6 they ask for.
* ``shift``.  Whole-pixel shifts copy: exact.  Fractions: the weights 1 - t (one rounding), their product (one), the four
  products with the samples (one each) and three additions: at most 7 roundings on the longest path, 7 u < 4 ulp = 8 u of
  ``sum |w_i x_i|``; the tests use the 4 ulp.
"""
import numpy as np

U = 2.0 ** -24
ROWS_PER_WAVE, KC, LANE_DEPTH = 16, 4, 6
DSUM = 1e4 * 2.0 ** -53


def gamma(m):
    return m * U / (1.0 - m * U)


def images(b, N):
    """host sinogram [s][a * N + r] -> X[a][r][s]"""
    b = np.asarray(b)
    ns = b.shape[0]
    return np.ascontiguousarray(b.reshape(ns, -1, N).transpose(1, 2, 0))


def packed(X):
    """X[a][r][s] -> host sinogram [s][a * N + r]"""
    X = np.asarray(X)
    P, N, ns = X.shape
    return np.ascontiguousarray(X.transpose(2, 0, 1).reshape(ns, P * N))


def moments(X):
    """[a] -> (sum X, sum r X, sum s X) in binary64"""
    X = np.asarray(X, np.float64)
    r = np.arange(X.shape[1], dtype=np.float64)[None, :, None]
    s = np.arange(X.shape[2], dtype=np.float64)[None, None, :]
    return np.stack([X.sum((1, 2)), (r * X).sum((1, 2)), (s * X).sum((1, 2))], axis=1)


def _corr(A, B, S):
    """sum_{r,s} A[a][r][s] B[a][r+u][s+v] over the overlap, [a][u+S][v+S], binary64"""
    P, N, ns = A.shape
    C = np.zeros((P, 2 * S + 1, 2 * S + 1))
    for u in range(-S, S + 1):
        ra, rb = slice(max(0, -u), min(N, N - u)), slice(max(0, u), min(N, N + u))
        for v in range(-S, S + 1):
            sa, sb = slice(max(0, -v), min(ns, ns - v)), slice(max(0, v), min(ns, ns + v))
            C[:, u + S, v + S] = (A[:, ra, sa] * B[:, rb, sb]).sum((1, 2))
    return C


def _centred(X, subtract_mean):
    X = np.asarray(X, np.float64)
    m = X.mean((1, 2), keepdims=True) if subtract_mean else np.zeros((X.shape[0], 1, 1))
    return X - m, m


def xcorr(A, B, S, subtract_mean=True):
    """C[a][u+S][v+S] = sum (A[r][s] - mA)(B[r+u][s+v] - mB) over the samples inside both images; binary64"""
    return _corr(_centred(A, subtract_mean)[0], _centred(B, subtract_mean)[0], S)


def xcorr_chain(nslice):
    """roundings on the longest path of the kernel's binary32 summation (module docstring)"""
    return ROWS_PER_WAVE * min(KC, -(-int(nslice) // 64)) + LANE_DEPTH


def xcorr_bound(A, B, S, subtract_mean=True):
    """per-element bound of |kernel - xcorr| (module docstring)"""
    a, ma = _centred(A, subtract_mean)
    b, mb = _centred(B, subtract_mean)
    a, b = np.abs(a), np.abs(b)
    da = 1.01 * U * (np.abs(ma) + a) if subtract_mean else 0.0
    db = 1.01 * U * (np.abs(mb) + b) if subtract_mean else 0.0
    g = gamma(xcorr_chain(np.shape(A)[2]))
    return (1.0 + g + DSUM) * _corr(a + da, b + db, S) - _corr(a, b, S)


def xcorr_replay_f32(A, B, S, subtract_mean=True, flip_v=False, skip_mean=False):
    """The kernel's arithmetic restated in numpy: staged values rounded to binary32, per-lane chains over 16 rows x up to KC chunks
    (an FMA as a binary64 product-and-add rounded to binary32), the lane tree, binary64 above.  ``flip_v`` / ``skip_mean`` are the
    deliberately wrong forms the CPU tests must see outside the bound: B read at s - v, the means not subtracted."""
    A32, B32 = np.asarray(A, np.float32), np.asarray(B, np.float32)
    P, N, ns = A32.shape
    if subtract_mean and not skip_mean:
        mA = np.asarray(A32, np.float64).mean((1, 2)).astype(np.float32)[:, None, None]
        mB = np.asarray(B32, np.float64).mean((1, 2)).astype(np.float32)[:, None, None]
        A32, B32 = A32 - mA, B32 - mB                  # binary32 subtraction, as staged
    nch = -(-ns // 64)
    pad = nch * 64 - ns
    a = np.pad(A32, ((0, 0), (0, 0), (0, pad))).astype(np.float64)
    bp = np.pad(B32, ((0, 0), (S, S + 64), (S, S + pad))).astype(np.float64)      # zeros wherever B is outside the image
    C = np.zeros((P, 2 * S + 1, 2 * S + 1))
    for u in range(-S, S + 1):
        for v in range(-S, S + 1):
            vv = -v if flip_v else v
            prod = np.zeros((P, N + 64 + S, nch * 64))                             # indexed by the B row rho = r + u
            for r in range(N):
                if 0 <= r + u:
                    prod[:, r + u] = a[:, r] * bp[:, r + u + S, S + vv:S + vv + nch * 64]
            tot = np.zeros(P)
            for rho0 in range(0, N, 16):                                            # one wave's rows
                for cg in range(0, nch, KC):
                    acc = np.zeros((P, 64), np.float32)
                    for ch in range(cg, min(nch, cg + KC)):
                        for i in range(rho0, rho0 + 16):
                            acc = (acc.astype(np.float64) + prod[:, i, ch * 64:(ch + 1) * 64]).astype(np.float32)
                    while acc.shape[1] > 1:
                        acc = acc[:, 0::2] + acc[:, 1::2]
                    tot += acc[:, 0].astype(np.float64)
            C[:, u + S, v + S] = tot
    return C


def _split(d):
    nd = -np.float64(np.float32(d))
    k = np.floor(nd)
    return int(k), float(nd - k)


def shift(X, shifts, wrap=False):
    """dst[a][r][s] = bilinear(src_a)(r - dr_a, s - ds_a) in binary64, and sum |w_i x_i| of every output element"""
    X = np.asarray(X, np.float64)
    P, N, ns = X.shape
    out, mag = np.zeros_like(X), np.zeros_like(X)
    r, s = np.arange(N), np.arange(ns)
    for a in range(P):
        kr, tr = _split(shifts[a][0])
        ks, ts = _split(shifts[a][1])
        for di, wr in ((0, 1.0 - tr), (1, tr)):
            for dj, ws in ((0, 1.0 - ts), (1, ts)):
                if wr == 0.0 or ws == 0.0:
                    continue
                i, j = r + kr + di, s + ks + dj
                if wrap:
                    tap = X[a][np.ix_(i % N, j % ns)]
                else:
                    oi, oj = (i >= 0) & (i < N), (j >= 0) & (j < ns)
                    tap = np.where(np.outer(oi, oj), X[a][np.ix_(np.clip(i, 0, N - 1), np.clip(j, 0, ns - 1))], 0.0)
                out[a] += wr * ws * tap
                mag[a] += np.abs(wr * ws * tap)
    return out, mag


def shift_int(X, shifts, wrap=False):
    """whole-pixel shifts with the array's own dtype: np.roll (wrap) or its zero-filled form"""
    X = np.asarray(X)
    out = np.zeros_like(X)
    P, N, ns = X.shape
    for a in range(P):
        dr, ds = int(shifts[a][0]), int(shifts[a][1])
        if wrap:
            out[a] = np.roll(np.roll(X[a], dr, axis=0), ds, axis=1)
        elif abs(dr) < N and abs(ds) < ns:
            out[a, max(0, dr):min(N, N + dr), max(0, ds):min(ns, ns + ds)] = X[a, max(0, -dr):min(N, N - dr), max(0, -ds):min(ns, ns - ds)]
    return out


def center_of_mass(X):
    """cpu/utils/logger.py:237-252 per projection: the integer shifts (dr, ds) and the rolled images"""
    X = np.asarray(X)
    P, N, ns = X.shape
    R, Sg = np.meshgrid(np.linspace(0, N - 1, N), np.linspace(0, ns - 1, ns), indexing="ij")
    sh = np.zeros((P, 2), np.int64)
    for a in range(P):
        img = X[a].astype(np.float64)
        sh[a] = (-(int(np.sum(img * R) / np.sum(img)) - N // 2), -(int(np.sum(img * Sg) / np.sum(img)) - ns // 2))
    return sh, shift_int(X, sh, wrap=True)


def peaks(C, subpixel=True):
    """argmax of every window (first in row-major order); with ``subpixel`` a 3-point parabola per axis, clamped to +-0.5; a
    maximum on the border keeps its integer position.  -> (peaks [a][2], at_border [a], margin [a]) with margin = (peak - runner-up)
    / peak of the window"""
    C = np.asarray(C, np.float64)
    P, w, _ = C.shape
    S = w // 2
    pk, border, margin = np.zeros((P, 2)), np.zeros(P, bool), np.zeros(P)
    for a in range(P):
        flat = C[a].ravel()
        k = int(np.argmax(flat))
        iu, iv = divmod(k, w)
        top = flat[k]
        margin[a] = (top - np.max(np.delete(flat, k))) / top
        border[a] = iu == 0 or iv == 0 or iu == w - 1 or iv == w - 1
        off = [0.0, 0.0]
        if subpixel and not border[a]:
            for ax, (cm, cp) in enumerate(((C[a, iu - 1, iv], C[a, iu + 1, iv]), (C[a, iu, iv - 1], C[a, iu, iv + 1]))):
                den = cm - 2.0 * top + cp
                if den < 0.0:
                    off[ax] = float(np.clip(0.5 * (cm - cp) / den, -0.5, 0.5))
        pk[a] = (iu - S + off[0], iv - S + off[1])
    return pk, border, margin


def gauge_residual(total, injected, angles_deg):
    """What is left of total + injected outside the gauge of projection matching: for dr the span of cos(theta), sin(theta) (a
    translation of the volume across the tilt axis), for ds a constant (one along it).  -> (residual of dr, residual of ds)"""
    e = np.asarray(total, np.float64) + np.asarray(injected, np.float64)
    th = np.deg2rad(np.asarray(angles_deg, np.float64))
    G = np.stack([np.cos(th), np.sin(th)], axis=1)
    coef = np.linalg.lstsq(G, e[:, 0], rcond=None)[0]
    return e[:, 0] - G @ coef, e[:, 1] - e[:, 1].mean()


# ---- projection matching replayed on the CPU: the oracle's SIRT and projector, the binary64 correlation, whole-pixel shifts ----
# Seed and shifts chosen on the CPU so that the leave-one-out replay recovers the shifts exactly and every peak is clear (the tests
# assert both).  The plain form (the model of every projection comes from a reconstruction that saw that projection) cannot: at 9
# projections of 32 x 32 slices the reconstruction reproduces each measured projection where it lies, every peak is (0, 0) and
# nothing moves -- tried with seeds 3, 7, 11, bead phantoms, 1 to 20 iterations, up to 8 passes.
REFINE_CASE = dict(nslice=32, n=32, nproj=9, seed=3, max_shift=8, nouter=4, niter=5,
                   injected=[[2, -1], [-3, 2], [1, 3], [0, -2], [-1, 0], [3, 1], [-2, -3], [1, 2], [-1, -2]])


# The plain form (the default) where it does work: 31 projections.  It removes most of the misplacement -- the RMS outside the gauge
# falls from 2.1 / 1.9 pixels (dr / ds) to 0.76 / 0 in three passes on the replay -- but about a pixel of dr stays.
PLAIN_CASE = dict(nslice=32, n=32, nproj=31, seed=3, max_shift=8, nouter=3, niter=20, injected=None)   # shifts: default_rng(seed) in [-3, 3]


def refine_case(c=None):
    """(angles in degrees, the clean series and the misaligned one as X[a][r][s] float32, injected shifts) of case ``c`` (default
    ``REFINE_CASE``): a seeded phantom of ellipsoids whose slices differ, projected by the oracle, every projection moved by its
    injected whole-pixel shift"""
    import oracle
    from tomo_tv_amd.phantom import ellipsoids, tilt_angles
    c = c or REFINE_CASE
    ang = tilt_angles(c["nproj"])
    o = oracle.ctvlib(c["nslice"], c["n"], c["nproj"])
    o.load_A(oracle.parallel_ray(c["n"], ang))
    o.original_volume = ellipsoids(c["nslice"], c["n"], seed=c["seed"])
    o.create_projections()
    clean = images(o.b, c["n"])
    if c["injected"] is None:
        inj = np.random.default_rng(c["seed"]).integers(-3, 4, (c["nproj"], 2))
    else:
        inj = np.array(c["injected"], np.int64)
    return ang, clean, shift_int(clean, inj, wrap=False), inj


def gauge_rms(total, injected, angles_deg):
    """RMS over the projections of what ``gauge_residual`` leaves, (dr, ds)"""
    return tuple(float(np.sqrt(np.mean(x ** 2))) for x in gauge_residual(total, injected, angles_deg))


def _model(o, cur, N, niter, leave_one_out):
    """the model projections G[a][r][s] of the series ``cur``: from one SIRT reconstruction of all of it, or with ``leave_one_out``
    projection a from a reconstruction that never saw projection a (its data are replaced by the model's own before every step,
    so its residual is zero)"""
    b = packed(cur)
    if not leave_one_out:
        o.set_tilt_series(b)
        o.restart_recon()
        o.SIRT_norm(niter)
        o.forward_projection()
        return images(o.g, N)
    G = np.zeros_like(cur)
    for a in range(cur.shape[0]):
        o.set_tilt_series(b)
        o.restart_recon()
        for _ in range(niter):
            o.forward_projection()
            o.b[:, a * N:(a + 1) * N] = o.g[:, a * N:(a + 1) * N]
            o.SIRT_norm(1)
        o.forward_projection()
        G[a] = images(o.g, N)[a]
    return G


def refine_replay(angles_deg, X, nouter, max_shift, niter=20, leave_one_out=False):
    """``TomoGPU.refine_alignment(subpixel=False)`` on the CPU.  -> (shifts after every pass, peaks of every pass, smallest margin)"""
    import oracle
    X = np.asarray(X, np.float32)
    P, N, ns = X.shape
    o = oracle.ctvlib(ns, N, P)
    o.load_A(oracle.parallel_ray(N, angles_deg))
    total = np.zeros((P, 2))
    cur, hist, pks, worst = X, [], [], np.inf
    for _ in range(nouter):
        pk, _, margin = peaks(xcorr(_model(o, cur, N, niter, leave_one_out), cur, max_shift), subpixel=False)
        worst = min(worst, float(margin.min()))
        total = total - pk
        total[:, 1] -= np.round(total[:, 1].mean())
        cur = shift_int(X, total, wrap=False)
        hist.append(total.copy())
        pks.append(pk)
    return hist, pks, worst
