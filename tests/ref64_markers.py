"""Plain numpy statements of the marker-detection calls (``tomo_sino_template_ncc`` / ``tomo_sino_peaks``) and of sub-pixel positions,
written from the definitions in include/tomo_hip.h, plus a replay of the correlation kernel's binary32 order of operations.

Images: ``X[a][r][s]`` (binary32), projection a, ray r in [0, N), slice s in [0, Nslice); ``ref64_align.images`` / ``packed`` convert
from and to the engine's host sinogram.

What is exact and what is bounded:

* the prepared template (``prepare_template``: binary64 mean and norm, rounded to binary32) is data of both statements;
* the peaks are a selection: the device records must equal ``peaks`` bit for bit;
* the correlation is W = (2R+1)^2 binary32 operations deep.  ``ncc`` states it in binary64; ``ncc_bound`` is the a-priori
  per-element bound of the binary32 evaluation that removes the mean before it sums (derivation below); ``ncc_replay32`` repeats
  the kernel's operations in ``np.float32`` and ``ncc_wrong32`` is the form that must NOT be used (sumsq - sum^2 / W).

The bound.  u = 2^-24, g(k) = k u / (1 - k u), n = W.  For one window with exact mean m, d_i = x_i - m, c = sum t_i d_i,
v = sum d_i^2:

* the computed mean is m + e with |e| <= em = g(n) sum|x_i| / n  (n - 1 additions and one division);
* the computed d_i is (d_i - e)(1 + delta_i), |delta_i| <= u, so |computed d_i| <= D_i = (|d_i| + em)(1 + u).  The error e is the
  SAME in every term: in c it meets sum t_i (0 but for the rounding of t, and known exactly), in v it meets sum d_i = 0:
  sum t_i (d_i - e) = c - e sum t_i  and  sum (d_i - e)^2 = v + n e^2;
* one multiplication and at most n additions per accumulated term: g(n + 1) relative to the sum of magnitudes.  Hence
  |computed c - c| <= ec = em |sum t_i| + (u + g(n + 1)) sum |t_i| D_i,
  |computed v - v| <= ev = n em^2 + (3 u + g(n + 1)) sum D_i^2;
* c / sqrt(v) with both operations correctly rounded (relative 3 u together) and the mean-value theorem on v^(-1/2) over
  [v - ev, v + ev]:  bound = ec / sqrt(v - ev) + |c| ev / (2 (v - ev)^1.5) + 3 u (|c| + ec) / sqrt(v - ev), plus 2^-40 for the
  binary64 statement itself.  Where v - ev <= 0 the bound is infinite (no claim).

The flat-window branch: where |v - var_floor W| <= ev (``in_band``) either branch is right; the tests choose inputs that leave
the band empty and assert that."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

from ref64_align import images, packed  # noqa: F401  (the layout converters, for the test modules)

F32 = np.float32
U = 2.0 ** -24


def gamma(k):
    return k * U / (1.0 - k * U)


def prepare_template(T):
    """t = T - mean(T), scaled to sum t^2 = 1, in binary64; rounded to binary32"""
    T = np.asarray(T, F32).astype(np.float64)
    t = T - T.sum() / T.size
    return (t * (1.0 / np.sqrt((t * t).sum()))).astype(F32)


def _windows(X, R, dtype):
    """[a][r - R][s - R][k][j] over the samples whose window lies inside the image; None when there is none"""
    X = np.asarray(X, F32)
    W = 2 * R + 1
    if X.shape[1] < W or X.shape[2] < W:
        return None
    return sliding_window_view(X.astype(dtype), (W, W), axis=(1, 2))


def _embed(inner, shape, R, dtype):
    out = np.zeros(shape, dtype)
    if inner is not None:
        out[:, R:shape[1] - R, R:shape[2] - R] = inner
    return out


def ncc_parts(X, T, R):
    """binary64: (c, v, ec, ev) on the inner samples (None when the image is smaller than the template)"""
    win = _windows(X, R, np.float64)
    if win is None:
        return None
    t = prepare_template(T).astype(np.float64)
    n = float(t.size)
    m = win.sum((3, 4)) / n
    d = win - m[..., None, None]
    c, v = (t * d).sum((3, 4)), (d * d).sum((3, 4))
    em = gamma(n) * np.abs(win).sum((3, 4)) / n
    D = (np.abs(d) + em[..., None, None]) * (1.0 + U)
    ec = em * abs(t.sum()) + (U + gamma(n + 1)) * (np.abs(t) * D).sum((3, 4))
    ev = n * em * em + (3.0 * U + gamma(n + 1)) * (D * D).sum((3, 4))
    return c, v, ec, ev


def ncc(X, T, var_floor=0.0):
    """-> (out, bound, in_band), each [a][r][s]: the binary64 correlation (0 where the window leaves the image or
    v <= var_floor W), the a-priori bound on a binary32 evaluation in the kernel's form, and where the flat-window test is within
    the bound of its threshold (either branch is right there)."""
    X = np.asarray(X, F32)
    T = np.asarray(T, F32)
    R = (T.shape[0] - 1) // 2
    parts = ncc_parts(X, T, R)
    if parts is None:
        z = np.zeros(X.shape)
        return z, z.copy(), np.zeros(X.shape, bool)
    c, v, ec, ev = parts
    thr = float(F32(var_floor) * F32(T.size))
    keep = v > thr
    lo = v - ev
    with np.errstate(divide="ignore", invalid="ignore"):
        val = np.where(keep, c / np.sqrt(np.where(keep, v, 1.0)), 0.0)
        slo = np.sqrt(np.where(lo > 0, lo, 1.0))
        b = ec / slo + np.abs(c) * ev / (2.0 * slo ** 3) + 3.0 * U * (np.abs(c) + ec) / slo + 2.0 ** -40
        bound = np.where(keep, np.where(lo > 0, b, np.inf), 0.0)
    band = np.abs(v - thr) <= ev
    return _embed(val, X.shape, R, np.float64), _embed(bound, X.shape, R, np.float64), _embed(band, X.shape, R, bool)


def ncc_replay32(X, T, var_floor=0.0):
    """the kernel's operations in np.float32, in its order: row-major over the window from 0, every operation rounded on its own"""
    X = np.asarray(X, F32)
    T = np.asarray(T, F32)
    R = (T.shape[0] - 1) // 2
    win = _windows(X, R, F32)
    if win is None:
        return np.zeros(X.shape, F32)
    t, W = prepare_template(T), T.shape[0]
    total = np.zeros(win.shape[:3], F32)
    for k in range(W):
        for j in range(W):
            total = total + win[..., k, j]
    m = total / F32(W * W)
    c, v = np.zeros_like(m), np.zeros_like(m)
    for k in range(W):
        for j in range(W):
            d = win[..., k, j] - m
            c = c + t[k, j] * d
            v = v + d * d
    assert c.dtype == F32 and v.dtype == F32 and m.dtype == F32
    keep = v > F32(var_floor) * F32(W * W)
    with np.errstate(divide="ignore", invalid="ignore"):
        val = np.where(keep, c / np.sqrt(np.where(keep, v, F32(1))), F32(0)).astype(F32)
    return _embed(val, X.shape, R, F32)


def ncc_wrong32(X, T, var_floor=0.0):
    """binary32 with v = sum x^2 - (sum x)^2 / W and c = sum t x (the mean NOT removed first): what the kernel must not do"""
    X = np.asarray(X, F32)
    T = np.asarray(T, F32)
    R = (T.shape[0] - 1) // 2
    win = _windows(X, R, F32)
    t, W = prepare_template(T), T.shape[0]
    s1, s2, c = (np.zeros(win.shape[:3], F32) for _ in range(3))
    for k in range(W):
        for j in range(W):
            x = win[..., k, j]
            s1, s2, c = s1 + x, s2 + x * x, c + t[k, j] * x
    v = s2 - s1 * s1 / F32(W * W)
    keep = v > F32(var_floor) * F32(W * W)
    with np.errstate(divide="ignore", invalid="ignore"):
        val = np.where(keep, c / np.sqrt(np.where(keep, v, F32(1))), F32(0)).astype(F32)
    return _embed(val, X.shape, R, F32)


# ---- local maxima ------------------------------------------------------------------------------------------------------------------
def peak_mask(X, radius, threshold):
    """[a][r][s] bool: x >= threshold, x > x' for the samples of the clipped window that precede (r, s) in row-major order, x >= x'
    for those that follow (a comparison with a NaN fails)"""
    X = np.asarray(X, F32)
    _, N, ns = X.shape
    with np.errstate(invalid="ignore"):
        ok = X >= F32(threshold)
        for dr in range(-radius, radius + 1):
            for ds in range(-radius, radius + 1):
                if dr == 0 and ds == 0:
                    continue
                r0, r1, s0, s1 = max(0, -dr), min(N, N - dr), max(0, -ds), min(ns, ns - ds)      # the samples that have this neighbour
                if r0 >= r1 or s0 >= s1:
                    continue
                x, y = X[:, r0:r1, s0:s1], X[:, r0 + dr:r1 + dr, s0 + ds:s1 + ds]
                ok[:, r0:r1, s0:s1] &= (x > y) if (dr < 0 or (dr == 0 and ds < 0)) else (x >= y)
    return ok


def peaks(X, radius, threshold):
    """-> (count[a], [records (count[a], 8) int32]): r, s, the bits of x, x(r-1, s), x(r+1, s), x(r, s-1), x(r, s+1) (outside the
    image: x), 0; sorted by r * Nslice + s"""
    X = np.asarray(X, F32)
    _, N, ns = X.shape
    mask = peak_mask(X, radius, threshold)
    out = []
    for a in range(len(X)):
        rs = np.argwhere(mask[a])                                                  # row-major order
        rec = np.zeros((len(rs), 8), np.int32)
        val = np.zeros((len(rs), 5), F32)
        for k, (r, s) in enumerate(rs):
            x = X[a, r, s]
            val[k] = (x, X[a, r - 1, s] if r > 0 else x, X[a, r + 1, s] if r + 1 < N else x,
                      X[a, r, s - 1] if s > 0 else x, X[a, r, s + 1] if s + 1 < ns else x)
        rec[:, :2] = rs
        rec[:, 2:7] = val.view(np.int32)
        out.append(rec)
    return np.array([len(r) for r in out], np.int32), out


# ---- sub-pixel positions -----------------------------------------------------------------------------------------------------------
def positions(records):
    """(k, 2): (r, s) plus the vertex of the parabola through the centre value and its two neighbours along each axis,
    0.5 (cm - cp) / (cm - 2 c0 + cp), where that denominator is negative (else 0), clamped to +-0.5"""
    rec = np.asarray(records, np.int32).reshape(-1, 8)
    val = rec[:, 2:7].copy().view(F32).astype(np.float64)
    out = rec[:, :2].astype(np.float64)
    for axis, (lo, hi) in enumerate(((1, 2), (3, 4))):
        den = val[:, lo] - 2.0 * val[:, 0] + val[:, hi]
        with np.errstate(divide="ignore", invalid="ignore"):
            off = np.where(den < 0, 0.5 * (val[:, lo] - val[:, hi]) / np.where(den < 0, den, 1.0), 0.0)
        out[:, axis] += np.clip(off, -0.5, 0.5)
    return out


# ---- the end-to-end case: six beads, known distortion ----------------------------------------------------------------------------------
E2E = dict(N=64, ns=70, angles=np.linspace(-70.0, 70.0, 15), rot0=2.0, bead_radius=2.0, marker_radius=2.0, R=4, threshold=0.5,
           search_radius=6.0, min_views=15,
           # (slice, y index, z index): non-collinear, inside the central cylinder, at least 9 apart along the slices
           beads=((8, 20, 30), (19, 44, 25), (30, 27, 46), (41, 38, 14), (52, 15, 38), (62, 46, 42)))
# What the binary64 pipeline (``pipeline`` on the binary64 correlation of the distorted series) leaves against the gauge-removed
# truth, measured by tests/test_markers_cpu.py::test_end_to_end_yardstick, which asserts that these records hold: the largest
# shift error in pixels and the rotation error in degrees.  The GPU test allows twice these.
E2E_SHIFT_ERR, E2E_PHI_ERR = 0.231, 0.138


def bead_phantom(c=E2E):
    """(ns, N, N) float32: balls of radius ``bead_radius`` voxels and value 1 at ``beads``"""
    x = np.zeros((c["ns"], c["N"], c["N"]), F32)
    s, y, z = np.meshgrid(np.arange(c["ns"]), np.arange(c["N"]), np.arange(c["N"]), indexing="ij")
    for bs, by, bz in c["beads"]:
        x[(s - bs) ** 2 + (y - by) ** 2 + (z - bz) ** 2 <= c["bead_radius"] ** 2] = 1.0
    return x


def e2e_distortion(c=E2E):
    """-> (d0, the (P, 6) maps of ``sino_affine`` that distort, true shifts, true rotation in degrees).  The series is distorted by
    rotating its content by ``rot0`` and moving it by d0 (|d0| <= 4 per axis, seeded); the alignment that undoes it is
    phi = -rot0 with d = -R(-rot0) d0."""
    import ref64_affine
    P = len(c["angles"])
    d0 = np.random.default_rng(5).uniform(-4.0, 4.0, (P, 2))
    M = ref64_affine.matrices(d0, c["rot0"], 1.0, c["N"], c["ns"])
    t = np.deg2rad(-c["rot0"])
    Rm = np.array([[np.cos(t), -np.sin(t)], [np.sin(t), np.cos(t)]])
    return d0, M, -(d0 @ Rm.T), -c["rot0"]


def remove_gauge(shifts, angles_deg):
    """dr without its least-squares components along cos theta and sin theta, ds without its mean"""
    d = np.array(shifts, np.float64)
    t = np.deg2rad(np.asarray(angles_deg, np.float64))
    B = np.stack([np.cos(t), np.sin(t)], axis=1)
    d[:, 0] -= B @ np.linalg.lstsq(B, d[:, 0], rcond=None)[0]
    d[:, 1] -= d[:, 1].mean()
    return d


def detect(C, radius, threshold):
    """per projection the (k, 2) sub-pixel positions of the peaks of C[a][r][s] (any float dtype, used as it is), row-major order:
    the peak rule, then the parabola through the values of C along each axis (a peak on the border keeps its integer position)"""
    C = np.asarray(C)
    _, N, ns = C.shape
    mask = peak_mask(C, radius, threshold) if C.dtype == F32 else _peak_mask64(C, radius, threshold)
    out = []
    for a in range(len(C)):
        rs = np.argwhere(mask[a])
        pos = rs.astype(np.float64)
        for k, (r, s) in enumerate(rs):
            x = float(C[a, r, s])
            if 0 < r < N - 1:
                pos[k, 0] += _vertex(float(C[a, r - 1, s]), x, float(C[a, r + 1, s]))
            if 0 < s < ns - 1:
                pos[k, 1] += _vertex(float(C[a, r, s - 1]), x, float(C[a, r, s + 1]))
        out.append(pos)
    return out


def _vertex(cm, c0, cp):
    den = cm - 2.0 * c0 + cp
    return min(0.5, max(-0.5, 0.5 * (cm - cp) / den)) if den < 0.0 else 0.0


def _peak_mask64(C, radius, threshold):
    _, N, ns = C.shape
    ok = C >= threshold
    for dr in range(-radius, radius + 1):
        for ds in range(-radius, radius + 1):
            if dr == 0 and ds == 0:
                continue
            r0, r1, s0, s1 = max(0, -dr), min(N, N - dr), max(0, -ds), min(ns, ns - ds)
            x, y = C[:, r0:r1, s0:s1], C[:, r0 + dr:r1 + dr, s0 + ds:s1 + ds]
            ok[:, r0:r1, s0:s1] &= (x > y) if (dr < 0 or (dr == 0 and ds < 0)) else (x >= y)
    return ok


def pipeline(C, c=E2E):
    """detections of the correlation C -> tracks -> the least-squares model (tomo_tv_amd.align), as ``TomoGPU.align_markers`` runs them"""
    from tomo_tv_amd import align
    pos = detect(C, c["R"], c["threshold"])
    tracks = align.link_markers(pos, c["angles"], c["N"], c["search_radius"], c["min_views"])
    out = align.solve_markers(tracks, c["angles"], c["N"], c["ns"])
    out["tracks"], out["n_detected"] = tracks, np.array([len(p) for p in pos])
    return out
