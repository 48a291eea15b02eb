"""Host side of the tilt-series alignment: the peak rule of projection matching, the centre-of-mass rule of the reference, the
matrices of the affine resampling and the score and minimum rule of the tilt-axis estimate.

The windows are ``Nangles * (2S+1)^2`` doubles, the matrices ``Nangles * 6`` and the profiles ``Nangles * Nslice``, so this is
bookkeeping, not hot path: the correlation itself, the moments, the profiles and the resampling are HIP kernels
(``tomoengine.sino_xcorr`` / ``sino_moments`` / ``sino_axis_profile`` / ``sino_shift`` / ``sino_affine``).  Likewise the Gauss-Newton
loops of the 3-D registration and of the per-projection similarity matching: the normal equations are reduced on the device
(``volume_affine_normal`` / ``sino_affine_normal``), the 6 x 6 and 4 x 4 solves and the composition of the maps happen here.  The
tilt angles are refined the same way: ``volume_rot_derivative`` and ``sino_tilt_normal`` reduce four numbers per projection on the
device, the division, the clip and the gauge are here (``tilt_increment``, ``match_tilt_angles``)."""
import numpy as np

from ._lib import SINO_G, SINO_USER0, VOL_RECON, VOL_TEMP


def _parabola(cm, c0, cp):
    """Offset of the vertex of the parabola through (-1, cm), (0, c0), (1, cp), clamped to +-0.5; 0 where the parabola opens upwards
    or is flat.  At an argmax (cm <= c0 >= cp) the vertex is 0.5 (a - b) / (a + b) with a = c0 - cm, b = c0 - cp >= 0, inside +-0.5
    by itself (+-0.5 exactly at a tie with a neighbour); the clamp only guards callers that pass another point."""
    den = cm - 2.0 * c0 + cp
    if not den < 0.0:
        return 0.0
    return float(min(0.5, max(-0.5, 0.5 * (cm - cp) / den)))


def find_peaks(C, subpixel=True):
    """Peak (u, v) of every window ``C[a]`` ((2S+1, 2S+1), index [u+S][v+S]): the first maximum in row-major order, refined with
    ``subpixel`` by a 3-point parabola along each axis (clamped to +-0.5).  A maximum on the window's border keeps its integer
    position.  Returns ``(peaks (Nangles, 2) float64, at_border (Nangles,) bool)``."""
    C = np.asarray(C, np.float64)
    na, w, _ = C.shape
    S = (w - 1) // 2
    peaks, border = np.zeros((na, 2)), np.zeros(na, bool)
    for a in range(na):
        iu, iv = np.unravel_index(int(np.argmax(C[a])), (w, w))
        border[a] = iu in (0, w - 1) or iv in (0, w - 1)
        du = dv = 0.0
        if subpixel and not border[a]:
            du = _parabola(C[a, iu - 1, iv], C[a, iu, iv], C[a, iu + 1, iv])
            dv = _parabola(C[a, iu, iv - 1], C[a, iu, iv], C[a, iu, iv + 1])
        peaks[a] = (iu - S + du, iv - S + dv)
    return peaks, border


def _cos_sin_deg(deg):
    """cos and sin of an angle in degrees; at multiples of 90 the exact 0 and +-1, never the output of cos or sin"""
    q = float(deg) % 360.0
    if q % 90.0 == 0.0:
        return ((1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0))[int(q // 90.0)]
    t = np.deg2rad(float(deg))
    return float(np.cos(t)), float(np.sin(t))


def affine_matrices(shifts, rotation_deg, magnification, N, Nslice):
    """(Nproj, 6) float64 for ``tomoengine.sino_affine``: per projection the content is rotated by ``+rotation_deg`` about the image
    centre c = ((N-1)/2, (Nslice-1)/2), counter-clockwise from the r axis towards the s axis (a sample on the +r side of the centre
    moves towards +s), then scaled by ``magnification`` about c, then moved by ``+shift`` = (dr, ds) in ``np.roll``'s sense.  The row
    (m00, m01, m02, m10, m11, m12) is the inverse map, from a destination sample to its source position:
    ``src = R(-phi) / mag . (dst - c - d) + c``.  ``rotation_deg`` and ``magnification`` may be scalars (the same for every projection)
    or one value per projection.  Rotation 0 with magnification 1 gives the exact translation (1, 0, -dr, 0, 1, -ds), and a rotation by
    a multiple of 90 degrees takes cos and sin as exact 0 and +-1 (a quarter turn of a square image then maps samples onto samples)."""
    d = np.asarray(shifts, np.float64).reshape(-1, 2)
    P = d.shape[0]
    rot = np.broadcast_to(np.asarray(rotation_deg, np.float64), (P,))
    mag = np.broadcast_to(np.asarray(magnification, np.float64), (P,))
    if not np.all(np.isfinite(mag)) or np.any(mag <= 0.0):
        raise ValueError("magnification must be positive and finite")
    cr, cs = 0.5 * (N - 1), 0.5 * (Nslice - 1)
    M = np.zeros((P, 6))
    for a in range(P):
        if rot[a] % 360.0 == 0.0 and mag[a] == 1.0:
            M[a] = (1.0, 0.0, -d[a, 0], 0.0, 1.0, -d[a, 1])
            continue
        c, s = _cos_sin_deg(rot[a])
        m00, m01, m10, m11 = c / mag[a], s / mag[a], -s / mag[a], c / mag[a]
        pr, ps = cr + d[a, 0], cs + d[a, 1]
        M[a] = (m00, m01, cr - (m00 * pr + m01 * ps), m10, m11, cs - (m10 * pr + m11 * ps))
    return M


def rotation_3d(rotation_deg):
    """The 3 x 3 content rotation of ``affine_matrix_3d`` in (s, y, z) coordinates, ``Rz @ Ry @ Rs`` for ``rotation_deg`` = (about s,
    about y, about z); multiples of 90 degrees give exact 0 and +-1."""
    a, b, g = (float(v) for v in rotation_deg)
    (ca, sa), (cb, sb), (cg, sg) = _cos_sin_deg(a), _cos_sin_deg(b), _cos_sin_deg(g)
    Rs = np.array([[1.0, 0.0, 0.0], [0.0, ca, -sa], [0.0, sa, ca]])
    Ry = np.array([[cb, 0.0, sb], [0.0, 1.0, 0.0], [-sb, 0.0, cb]])
    Rz = np.array([[cg, -sg, 0.0], [sg, cg, 0.0], [0.0, 0.0, 1.0]])
    return Rz @ Ry @ Rs


def affine_matrix_3d(rotation_deg=(0, 0, 0), shift=(0, 0, 0), magnification=1.0, src_shape=None, dst_shape=None, matrix=None):
    """The 12 float64 entries (row-major 3 x 4) for ``tomoengine.volume_affine_to``: the map from a destination voxel (s, y, z) to its
    source position.  The content of a volume of ``src_shape`` = (Nslice, N, N) is rotated about the volume centre (each axis at
    (size - 1) / 2), scaled by ``magnification`` about it, then moved by ``+shift`` = (ds, dy, dz) voxels (``np.roll``'s sense) into a
    volume of ``dst_shape`` (default: ``src_shape``), centre onto centre:  ``dst = c_dst + mag R (src - c_src) + shift``, and the
    result is the inverse map  ``src = R^T / mag . (dst - c_dst - shift) + c_src``.

    ``rotation_deg`` = (about s, about y, about z), applied in that order (R = Rz Ry Rs), each right-handed in the cyclic order
    s -> y -> z -> s.  By what a point on the +y axis (as seen from the centre) does under a small positive angle: about s it moves
    towards +z; about y it stays where it is (a point on the +z axis moves towards +s); about z it moves towards -s (a point on the
    +s axis moves towards +y).  ``matrix=`` takes the 3 x 3 content rotation R directly, in (s, y, z) coordinates, instead of the angles.

    Rotations by multiples of 90 degrees take cos and sin as exact 0 and +-1, so quarter turns between equal cubes are integer
    matrices (samples onto samples); no rotation with magnification 1 gives the exact translation."""
    if src_shape is None:
        raise ValueError("src_shape = (Nslice, N, N) is required")
    src = np.asarray(src_shape, np.float64).ravel()
    dst = src if dst_shape is None else np.asarray(dst_shape, np.float64).ravel()
    d = np.asarray(shift, np.float64).ravel()
    mag = float(magnification)
    if src.shape != (3,) or dst.shape != (3,) or d.shape != (3,) or np.any(src < 1) or np.any(dst < 1):
        raise ValueError("src_shape, dst_shape and shift must have three entries, the shapes positive")
    if not np.isfinite(mag) or mag <= 0.0:
        raise ValueError("magnification must be positive and finite")
    if matrix is None:
        rot = np.asarray(rotation_deg, np.float64).ravel()
        if rot.shape != (3,) or not np.all(np.isfinite(rot)):
            raise ValueError("rotation_deg must be three finite angles (about s, about y, about z)")
        R = rotation_3d(rot)
    else:
        R = np.asarray(matrix, np.float64)
        if R.shape != (3, 3) or not np.all(np.isfinite(R)):
            raise ValueError("matrix must be a finite 3 x 3 rotation")
    if not np.all(np.isfinite(d)):
        raise ValueError("shift must be finite")
    A = R.T / mag if mag != 1.0 else R.T.copy()
    cs, cd = 0.5 * (src - 1.0), 0.5 * (dst - 1.0)
    M = np.empty((3, 4))
    M[:, :3] = A
    M[:, 3] = cs - A @ (cd + d)
    return M.ravel()


# ---- 3-D rigid registration of two volumes: the host side of ``tomoengine.volume_affine_normal`` (32 numbers per iteration) -----------
def rigid_increment(H, b, damping=0.0):
    """The Gauss-Newton step ``delta`` = (shift s, y, z; rotation vector s, y, z in radians) of ``(H + damping diag(H)) delta = -b``
    in binary64.  ``ValueError`` when ``H`` or ``b`` is not finite, ``damping`` is negative, or ``H`` is singular (numerically: a
    reciprocal condition number below 1e-14) with ``damping`` = 0."""
    H, b, lam = np.asarray(H, np.float64), np.asarray(b, np.float64), float(damping)
    if H.shape != (6, 6) or b.shape != (6,):
        raise ValueError("H must be 6 x 6 and b have 6 entries")
    if not np.all(np.isfinite(H)) or not np.all(np.isfinite(b)):
        raise ValueError("the normal equations are not finite")
    if not lam >= 0.0:
        raise ValueError("damping must not be negative")
    A = H + lam * np.diag(np.diag(H))
    sv = np.linalg.svd(A, compute_uv=False)
    if not sv[0] > 0.0 or sv[-1] < 1e-14 * sv[0]:
        if lam == 0.0:
            raise ValueError("the normal equations are singular: the volumes do not determine all six parameters (try damping > 0)")
        raise ValueError("the normal equations are singular even with damping: a parameter has no gradient at all")
    return np.linalg.solve(A, -b)


def _rodrigues(omega):
    """exp of the rotation vector: 1 + sin(t) K + (1 - cos(t)) K^2 with K the cross-product matrix of the unit axis"""
    w = np.asarray(omega, np.float64)
    t = float(np.linalg.norm(w))
    if t == 0.0:
        return np.eye(3)
    k = w / t
    K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return np.eye(3) + np.sin(t) * K + (1.0 - np.cos(t)) * (K @ K)


def compose_rigid_increment(M, delta, src_shape):
    """The map after a step: ``x -> c + Rot(delta[3:]) (M x - c) + delta[:3]`` with c = (src_shape - 1) / 2, the centre of the moving
    volume, and ``Rot`` by Rodrigues' formula, so the linear part of a rigid map stays a rotation.  ``delta`` = 0 returns ``M``'s
    entries unchanged, bit for bit."""
    m = np.array(M, np.float64).reshape(3, 4)
    d = np.asarray(delta, np.float64).ravel()
    c = 0.5 * (np.asarray(src_shape, np.float64).ravel() - 1.0)
    if d.shape != (6,) or c.shape != (3,) or not np.all(np.isfinite(d)):
        raise ValueError("delta must be six finite numbers and src_shape three sizes")
    if not d.any():
        return m.ravel()
    Rm = _rodrigues(d[3:])
    out = np.empty((3, 4))
    out[:, :3] = Rm @ m[:, :3]
    out[:, 3] = c + Rm @ (m[:, 3] - c) + d[:3]
    return out.ravel()


def decode_rigid(M, src_shape, dst_shape=None):
    """``(R, shift)`` with ``affine_matrix_3d(matrix=R, shift=shift, src_shape=..., dst_shape=...) == M``: the content rotation and the
    shift in voxels of a rigid destination-to-source map."""
    m = np.asarray(M, np.float64).reshape(3, 4)
    src = np.asarray(src_shape, np.float64).ravel()
    dst = src if dst_shape is None else np.asarray(dst_shape, np.float64).ravel()
    if src.shape != (3,) or dst.shape != (3,) or not np.all(np.isfinite(m)):
        raise ValueError("M must be 12 finite entries and the shapes three sizes")
    A = m[:, :3]
    return A.T.copy(), np.linalg.solve(A, 0.5 * (src - 1.0) - m[:, 3]) - 0.5 * (dst - 1.0)


def rotation_angle_deg(Rm):
    """the angle of a rotation matrix in degrees (from the antisymmetric part and the trace: accurate near 0)"""
    Rm = np.asarray(Rm, np.float64)
    s = 0.5 * np.sqrt((Rm[2, 1] - Rm[1, 2]) ** 2 + (Rm[0, 2] - Rm[2, 0]) ** 2 + (Rm[1, 0] - Rm[0, 1]) ** 2)
    return float(np.rad2deg(np.arctan2(s, 0.5 * (np.trace(Rm) - 1.0))))


def register_volumes(fixed, moving, M0=None, max_iter=30, tol_shift=1e-3, tol_deg=1e-3, margin=1, damping=0.0, fixed_vol=0, moving_vol=0):
    """Intensity-based rigid registration by Gauss-Newton: the map M (12 entries, from a voxel of volume ``fixed_vol`` of engine
    ``fixed`` to its position in volume ``moving_vol`` of engine ``moving``; ``volume_affine_to``'s convention) that minimises
    sum (moving(M x) - fixed(x))^2 over the six rigid parameters, from ``M0`` (default: centre onto centre, no rotation).  Every
    iteration is one ``fixed.volume_affine_normal`` on the device and a 6 x 6 solve here.  Stops when a step is below ``tol_shift``
    voxels in every component and below ``tol_deg`` degrees, or after ``max_iter`` steps.  -> dict: ``M``; ``R``, ``shift`` (the
    content rotation and shift of ``affine_matrix_3d`` / ``DualAxisTomo.set_registration``); per evaluation ``ssd``, ``count`` and
    ``ncc``; per step ``step`` = (largest shift component in voxels, rotation in degrees); ``converged``.  ``RuntimeError`` when
    fewer than one eighth of the fixed volume's voxels count: the volumes no longer overlap."""
    fshape, mshape = (fixed.Nslice_, fixed.Ny, fixed.Nz), (moving.Nslice_, moving.Ny, moving.Nz)
    M = affine_matrix_3d(src_shape=mshape, dst_shape=fshape) if M0 is None else np.array(M0, np.float64).ravel()
    if M.shape != (12,) or not np.all(np.isfinite(M)):
        raise ValueError("M0 must be 12 finite entries")
    if int(max_iter) < 0 or not tol_shift >= 0 or not tol_deg >= 0:
        raise ValueError("max_iter, tol_shift and tol_deg must not be negative")
    nvox = fshape[0] * fshape[1] * fshape[2]
    out = dict(ssd=[], count=[], ncc=[], step=[], converged=False)
    for _ in range(int(max_iter)):
        H, b, ssd, count, ncc = fixed.volume_affine_normal(moving, M, margin=margin, fixed_vol=fixed_vol, moving_vol=moving_vol)
        out["ssd"].append(ssd), out["count"].append(count), out["ncc"].append(ncc)
        if 8 * count < nvox:
            raise RuntimeError(f"only {count} of the fixed volume's {nvox} voxels count: the volumes no longer overlap")
        delta = rigid_increment(H, b, damping)
        M = compose_rigid_increment(M, delta, mshape)
        step = (float(np.max(np.abs(delta[:3]))), float(np.rad2deg(np.linalg.norm(delta[3:]))))
        out["step"].append(step)
        if step[0] <= tol_shift and step[1] <= tol_deg:
            out["converged"] = True
            break
    out["M"] = M
    out["R"], out["shift"] = decode_rigid(M, mshape, fshape)
    return out


# ---- per-projection similarity matching: the host side of ``tomoengine.sino_affine_normal`` (21 numbers per projection and iteration) ----
_TRIU4 = np.triu_indices(4)


def unpack_similarity_normal(out):
    """``(H, b, ssd, count, ncc)`` from the (Nproj, 21) sums of ``tomo_sino_affine_normal``: H (Nproj, 4, 4) symmetric, b (Nproj, 4),
    ssd (Nproj,), count (Nproj,) int64 and the mean-subtracted normalised correlation
    (sum F w - sum F sum w / n) / sqrt((sum F^2 - (sum F)^2 / n)(sum w^2 - (sum w)^2 / n)), 0 where a variance is not positive."""
    out = np.asarray(out, np.float64).reshape(-1, 21)
    P = out.shape[0]
    H = np.zeros((P, 4, 4))
    H[:, _TRIU4[0], _TRIU4[1]] = out[:, :10]
    H = H + np.triu(H, 1).transpose(0, 2, 1)
    n = out[:, 15]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        vf, vw = out[:, 16] - out[:, 19] ** 2 / n, out[:, 17] - out[:, 20] ** 2 / n
        den = vf * vw
        good = (n > 0) & (vf > 0.0) & (vw > 0.0) & np.isfinite(den)
        ncc = np.where(good, (out[:, 18] - out[:, 19] * out[:, 20] / n) / np.sqrt(np.where(good, den, 1.0)), 0.0)
    return H, out[:, 10:14].copy(), out[:, 14].copy(), n.astype(np.int64), ncc


def similarity_increment(H, b, damping=0.0, rotation=True, magnification=True, active=None):
    """The Gauss-Newton step per projection, ``delta`` (Nproj, 4) = (shift r, shift s, rotation omega in radians, log-magnification
    lambda), of ``(H + damping diag(H)) delta = -b`` in binary64.  A parameter switched off by ``rotation`` / ``magnification`` is
    removed from the system (not damped) and its entry of ``delta`` is exactly 0.  ``ValueError``, naming the projection, when ``H``
    or ``b`` is not finite or the (reduced) ``H`` is singular (numerically: a reciprocal condition number below 1e-14); also when
    ``damping`` is negative.  ``active`` (Nproj,) bool: a projection outside it is not looked at and gets a zero step (the loop's
    converged projections: their systems can no longer stop it)."""
    H, b, lam = np.asarray(H, np.float64), np.asarray(b, np.float64), float(damping)
    if H.ndim != 3 or H.shape[1:] != (4, 4) or b.shape != (H.shape[0], 4):
        raise ValueError("H must be (Nproj, 4, 4) and b (Nproj, 4)")
    if not lam >= 0.0:
        raise ValueError("damping must not be negative")
    act = np.ones(H.shape[0], bool) if active is None else np.asarray(active, bool)
    if act.shape != (H.shape[0],):
        raise ValueError("active must hold one flag per projection")
    keep = np.array([0, 1] + ([2] if rotation else []) + ([3] if magnification else []))
    delta = np.zeros((H.shape[0], 4))
    for a in np.flatnonzero(act):
        if not np.all(np.isfinite(H[a])) or not np.all(np.isfinite(b[a])):
            raise ValueError(f"projection {a}: the normal equations are not finite")
        A = H[a][np.ix_(keep, keep)]
        A = A + lam * np.diag(np.diag(A))
        sv = np.linalg.svd(A, compute_uv=False)
        if not sv[0] > 0.0 or sv[-1] < 1e-14 * sv[0]:
            if lam == 0.0:
                raise ValueError(f"projection {a}: the normal equations are singular: the images do not determine all parameters (try damping > 0)")
            raise ValueError(f"projection {a}: the normal equations are singular even with damping: a parameter has no gradient at all")
        delta[a, keep] = np.linalg.solve(A, -b[a, keep])
    return delta


def compose_similarity_increment(M, delta, N, Nslice):
    """The maps after a step: per projection ``x -> c + e^lambda Rot(omega) (M x - c) + t`` with ``delta`` = (t_r, t_s, omega, lambda),
    c = ((N-1)/2, (Nslice-1)/2) the centre of the moving image and Rot(omega) = [[cos, -sin], [sin, cos]] in (r, s), so the linear part
    of a similarity stays a scaled rotation.  A projection whose ``delta`` is all zero keeps its entries of ``M``, bit for bit."""
    m = np.array(M, np.float64).reshape(-1, 6)
    d = np.asarray(delta, np.float64).reshape(-1, 4)
    if d.shape[0] != m.shape[0] or not np.all(np.isfinite(d)):
        raise ValueError("delta must be four finite numbers per projection")
    c = np.array([0.5 * (N - 1), 0.5 * (Nslice - 1)])
    out = m.copy()
    for a in range(m.shape[0]):
        if not d[a].any():
            continue
        k = np.exp(d[a, 3])
        S = k * np.array([[np.cos(d[a, 2]), -np.sin(d[a, 2])], [np.sin(d[a, 2]), np.cos(d[a, 2])]])
        A, t = m[a].reshape(2, 3)[:, :2], m[a].reshape(2, 3)[:, 2]
        out[a].reshape(2, 3)[:, :2] = S @ A
        out[a].reshape(2, 3)[:, 2] = c + S @ (t - c) + d[a, :2]
    return out


def decode_similarity(M, N, Nslice):
    """``(shift (Nproj, 2), rotation_deg (Nproj,), magnification (Nproj,))`` with ``affine_matrices(shift, rotation_deg, magnification,
    N, Nslice) == M`` for maps whose linear part is a scaled rotation: the inverse of ``affine_matrices``."""
    m = np.asarray(M, np.float64).reshape(-1, 6)
    if not np.all(np.isfinite(m)):
        raise ValueError("M must be finite")
    c = np.array([0.5 * (N - 1), 0.5 * (Nslice - 1)])
    P = m.shape[0]
    shift, rot, mag = np.zeros((P, 2)), np.zeros(P), np.ones(P)
    for a in range(P):
        A, t = m[a].reshape(2, 3)[:, :2], m[a].reshape(2, 3)[:, 2]
        det = A[0, 0] * A[1, 1] - A[0, 1] * A[1, 0]
        if not det > 0.0:
            raise ValueError(f"projection {a}: the linear part is not a scaled rotation")
        mag[a] = 1.0 / np.sqrt(det)
        rot[a] = np.rad2deg(np.arctan2(A[0, 1] - A[1, 0], A[0, 0] + A[1, 1]))
        shift[a] = np.linalg.solve(A, c - t) - c
    return shift, rot, mag


def match_projections(eng, fixed, moving, M0=None, max_iter=20, tol_shift=1e-3, tol_deg=1e-3, tol_mag=1e-5, margin=2, damping=0.0,
                      rotation=True, magnification=True):
    """Intensity-based matching of every projection by Gauss-Newton: per projection the map M (6 entries, from a sample of slot
    ``fixed`` to its position in slot ``moving``; ``sino_affine``'s convention) that minimises sum (moving(M x) - fixed(x))^2 over
    shift, in-plane rotation and magnification, from ``M0`` (default: the identity).  All projections advance together: every
    iteration is one ``eng.sino_affine_normal`` on the device and a 4 x 4 solve per projection here.  A projection stops when a step
    is below ``tol_shift`` pixels in both components, ``tol_deg`` degrees and ``tol_mag`` in log-magnification, and keeps its map from
    then on; the loop ends when all have, or after ``max_iter`` steps.  -> dict: ``M`` (Nproj, 6); ``shift``, ``rotation_deg``,
    ``magnification`` (``decode_similarity``: what ``affine_matrices`` / ``set_alignment`` take); per evaluation ``ssd``, ``count``,
    ``ncc`` (each (Nproj,)); per step ``step`` (Nproj, 3) = (largest shift component, rotation in degrees, |log-magnification|);
    ``converged`` (Nproj,) bool.  ``RuntimeError``, naming the projections, when fewer than one eighth of a projection's samples count."""
    P, N, ns = eng.Nproj, eng.Ny, eng.Nslice_
    M = np.tile(np.array([1.0, 0, 0, 0, 1.0, 0]), (P, 1)) if M0 is None else np.array(M0, np.float64).reshape(-1, 6)
    if M.shape != (P, 6) or not np.all(np.isfinite(M)):
        raise ValueError(f"M0 must be {(P, 6)} finite entries")
    if int(max_iter) < 0 or not tol_shift >= 0 or not tol_deg >= 0 or not tol_mag >= 0:
        raise ValueError("max_iter and the tolerances must not be negative")
    out = dict(ssd=[], count=[], ncc=[], step=[])
    done = np.zeros(P, bool)
    for _ in range(int(max_iter)):
        H, b, ssd, count, ncc = eng.sino_affine_normal(fixed, moving, M, margin=margin)
        out["ssd"].append(ssd), out["count"].append(count), out["ncc"].append(ncc)
        few = np.flatnonzero(8 * count < N * ns)
        if few.size:
            raise RuntimeError(f"projections {few.tolist()}: fewer than one eighth of the {N * ns} samples count: the images no longer overlap")
        delta = similarity_increment(H, b, damping, rotation, magnification, active=~done)
        M = compose_similarity_increment(M, delta, N, ns)
        step = np.stack([np.max(np.abs(delta[:, :2]), axis=1), np.rad2deg(np.abs(delta[:, 2])), np.abs(delta[:, 3])], axis=1)
        out["step"].append(step)
        done = done | ((step[:, 0] <= tol_shift) & (step[:, 1] <= tol_deg) & (step[:, 2] <= tol_mag))
        if done.all():
            break
    out["converged"] = done
    out["M"] = M
    out["shift"], out["rotation_deg"], out["magnification"] = decode_similarity(M, N, ns)
    return out


# ---- per-projection tilt angles: the host side of ``tomoengine.sino_tilt_normal`` (4 numbers per projection and evaluation) ---------
TILT_SCRATCH_SLOT = SINO_USER0 + 37    # sinogram slot the derivative's projections go to, unless the caller names another


def tilt_increment(rd, dd, damping=1.0, max_step_deg=None):
    """The Gauss-Newton step of every tilt angle in DEGREES from the sums of ``sino_tilt_normal``: ``damping * rd / dd`` radians,
    exactly 0 where ``dd == 0`` (a projection whose derivative vanishes says nothing about its angle), clipped to
    +-``max_step_deg`` where that is given, and THEN with the mean removed: a common offset of all angles is a rotation of the
    volume about the tilt axis, which the data cannot see, so the increments of a pass carry none.  (After the clip a step can
    therefore exceed ``max_step_deg`` by the removed mean.)  ``damping`` is the fraction of the full step that is taken, 1.0 = all of
    it.  ``ValueError`` for sums that are not finite, a negative ``dd``, a ``damping`` outside (0, 1] or a ``max_step_deg`` that is
    not positive."""
    rd, dd = np.asarray(rd, np.float64).ravel(), np.asarray(dd, np.float64).ravel()
    if rd.shape != dd.shape or rd.size == 0:
        raise ValueError("rd and dd must hold one value per projection")
    if not (np.all(np.isfinite(rd)) and np.all(np.isfinite(dd))) or np.any(dd < 0.0):
        raise ValueError("the sums must be finite and dd must not be negative")
    if not 0.0 < float(damping) <= 1.0:
        raise ValueError("damping must lie in (0, 1]")
    if max_step_deg is not None and not float(max_step_deg) > 0.0:
        raise ValueError("max_step_deg must be positive")
    step = np.zeros_like(rd)
    ok = dd > 0.0
    step[ok] = np.rad2deg(float(damping) * rd[ok] / dd[ok])
    if max_step_deg is not None:
        step = np.clip(step, -float(max_step_deg), float(max_step_deg))
    return step - step.mean()


def match_tilt_angles(eng, b_sino, vol=VOL_RECON, margin=1, deriv_vol=VOL_TEMP, deriv_sino=TILT_SCRATCH_SLOT):
    """One evaluation of the tilt-angle matching on engine ``eng``: how well the projections of volume ``vol`` at the engine's
    angles explain the data in sinogram slot ``b_sino``, and in which direction every angle should move.  Four device steps: the
    rotational derivative of ``vol`` (``volume_rot_derivative``), the projection of ``vol`` (the model) and of the derivative, and
    the per-projection sums (``sino_tilt_normal``) over the samples ``margin`` inside the image.  -> ``(rd, dd, rr, count)``
    (``tilt_increment(rd, dd)`` turns them into steps; ``rr`` is the squared data distance per projection over the same samples).

    OVERWRITES: volume slot ``deriv_vol`` (default ``VOL_TEMP``, the slot of ``copy_recon``) with the derivative volume; sinogram slot
    ``SINO_G`` with the model ``A vol`` (as ``forward_projection`` does); sinogram slot ``deriv_sino`` (default
    ``TILT_SCRATCH_SLOT`` = ``SINO_USER0 + 37``) with ``A (D vol)``.  ``vol`` and ``b_sino`` are only read."""
    if int(deriv_vol) == int(vol):
        raise ValueError("deriv_vol must be another slot than vol")
    if int(deriv_sino) in (int(b_sino), SINO_G):
        raise ValueError("deriv_sino must be neither the data slot nor SINO_G")
    eng.volume_rot_derivative(vol, deriv_vol)
    eng.be.c("forward_projection", int(vol), SINO_G)
    eng.be.c("forward_projection", int(deriv_vol), int(deriv_sino))
    return eng.sino_tilt_normal(b_sino, SINO_G, deriv_sino, margin=margin)


def axis_score_border(N, search_deg):
    """H = ceil(N/2 sin(search_deg)): a rotation by up to ``search_deg`` about the centre moves a sample of a row of N rays by at most
    that many slices, so the slices H <= s < Nslice - H of the resampled series never hold zero fill"""
    return int(np.ceil(0.5 * N * np.sin(np.deg2rad(abs(float(search_deg)))) - 1e-12))


def axis_score(profile, H):
    """Common-line score of a profile c[a][s] (``sino_axis_profile``): sum_s Var_a(c_a[s]) / sum_s mean_a(c_a[s])^2 over the slices
    H <= s < Nslice - H (population variance over the projections).  Zero for a parallel-beam series whose axis runs along s."""
    c = np.asarray(profile, np.float64)
    if c.shape[1] - 2 * H <= 0:
        raise ValueError(f"no slice is left between the borders of {H} slices: lower search_deg")
    c = c[:, H:c.shape[1] - H]
    return float(np.sum(np.var(c, axis=0)) / np.sum(np.mean(c, axis=0) ** 2))


def axis_grid(search_deg, step_deg):
    """the candidate rotations k * step_deg, |k| <= search_deg / step_deg, symmetric about 0"""
    if not (search_deg > 0 and step_deg > 0):
        raise ValueError("search_deg and step_deg must be positive")
    K = int(np.floor(float(search_deg) / float(step_deg) + 1e-9))
    return float(step_deg) * np.arange(-K, K + 1, dtype=np.float64)


def axis_minimum(grid, scores):
    """The first minimum of ``scores`` over ``grid``, refined by a 3-point parabola clamped to +-1/2 step.  A minimum on the grid's
    border keeps its grid value and is flagged.  -> (rotation, index of the grid point, at_border)"""
    sc = np.asarray(scores, np.float64)
    k = int(np.argmin(sc))
    border = k in (0, len(sc) - 1)
    off = 0.0 if border else _parabola(-sc[k - 1], -sc[k], -sc[k + 1])
    step = float(grid[1] - grid[0]) if len(grid) > 1 else 0.0
    return float(grid[k] + off * step), k, bool(border)


def center_of_mass_shifts(moments, nray, nslice):
    """cpu/utils/logger.py:237-247 per projection from its moments (sum X, sum r X, sum s X): the centre of mass truncated to an
    integer, moved to ``size // 2`` on both axes.  (Nangles, 2) int64 of (dr, ds)."""
    m = np.asarray(moments, np.float64)
    out = np.zeros((m.shape[0], 2), np.int64)
    for a in range(m.shape[0]):
        out[a, 0] = -(int(m[a, 1] / m[a, 0]) - nray // 2)
        out[a, 1] = -(int(m[a, 2] / m[a, 0]) - nslice // 2)
    return out


# ---- conditioning of the tilt series: the host side of ``tomoengine.sino_window_stats`` / ``sino_median`` / ``sino_intensity`` --------
def background_window(Nray, Nslice):
    """The reference's background window (cpu/utils/logger.py:258-259: the first quarter of both axes) as ``(r0, r1, s0, s1)``:
    rays [0, Nray // 4), slices [0, Nslice // 4), each at least 1 wide (the reference's window is empty below 4 samples)."""
    return 0, max(1, int(Nray) // 4), 0, max(1, int(Nslice) // 4)


def despeckle_thresholds(stats, n_sigma):
    """(Nproj,) float32 thresholds from the (Nproj, 5) sums of a measuring ``sino_median``: ``n_sigma * sqrt(pi / 2) * (sum |d| / n)``,
    the Gaussian sigma estimated from the mean absolute deviation from the local median -- which the outliers themselves inflate far
    less than they inflate the RMS.  A projection whose mean absolute deviation is 0 gets ``+Inf``: nothing is replaced there."""
    st = np.asarray(stats, np.float64)
    if not float(n_sigma) > 0:
        raise ValueError("n_sigma must be positive")
    mad = st[:, 1] / st[:, 3]
    with np.errstate(over="ignore"):
        return np.where(mad > 0, float(n_sigma) * np.sqrt(np.pi / 2) * mad, np.inf).astype(np.float32)


def mass_gains(moments):
    """(Nproj,) float64 gains ``mean_a(mass) / mass_a`` from the (Nproj, >= 1) sums of ``sino_moments`` or ``sino_window_stats``
    (column 0: the total mass): for a parallel-beam series the mass is the same in every projection.  ``ValueError`` if a mass is
    not positive (subtract the background first, and mind what it leaves of an empty projection)."""
    mass = np.asarray(moments, np.float64).reshape(len(moments), -1)[:, 0]
    if not np.all(mass > 0) or not np.all(np.isfinite(mass)):
        raise ValueError("every projection needs a positive, finite total mass")
    return mass.mean() / mass


# ---- marker (fiducial / feature) alignment: the host side of ``tomoengine.sino_template_ncc`` / ``sino_peaks`` ------------------------
# Coordinates: an observation is (a, r, s) -- projection index, position along the rays, position along the tilt axis, in samples.  A
# marker is (y, z, sigma): its position in a slice of the volume relative to the slice centre ((N-1)/2, (N-1)/2), in voxels along
# the first and second axis of the (Nslice, N, N) volume, and its slice relative to the detector centre c_s = (Nslice-1)/2.
MARKER_NCC_SLOT = SINO_USER0 + 36      # sinogram slot TomoGPU.align_markers writes the correlation into
MARKER_MAX_MISSES = 2                  # a track ends after this many consecutive projections without a detection


def marker_template(radius_px, R, bright=True):
    """(2R+1, 2R+1) float64: an anti-aliased disc of radius ``radius_px`` about the window centre, the share of every sample's
    unit square that the disc covers (8 x 8 sub-samples), 1 inside and 0 outside for a ``bright`` marker (a gold bead in a
    dark-field or inverted series), the negative for a dark one.  ``ValueError`` when the result would be constant: a disc that
    leaves no background inside the window, or none at all."""
    R, rad = int(R), float(radius_px)
    if R < 1 or not rad > 0.0 or not np.isfinite(rad):
        raise ValueError("R must be at least 1 and radius_px positive and finite")
    sub = (np.arange(8) + 0.5) / 8.0 - 0.5
    g = (np.arange(-R, R + 1)[:, None] + sub[None, :]).ravel()
    inside = (g[:, None] ** 2 + g[None, :] ** 2 <= rad * rad).astype(np.float64)
    T = inside.reshape(2 * R + 1, 8, 2 * R + 1, 8).mean((1, 3))
    if T.max() - T.min() <= 0.0:
        raise ValueError("the disc fills the whole window (or none of it): the template would be constant")
    return T if bright else -T


def marker_positions(records, shape=None):
    """(k, 2) float64 sub-pixel positions (r, s) from the (k, 8) int32 records of ``tomoengine.sino_peaks``: the integer position
    plus, along each axis, the vertex of the parabola through the centre value and its two neighbours (``_parabola``: inside
    +-0.5).  With ``shape`` = (N, Nslice) a peak on the image border keeps its integer position along that axis (its record
    repeats the centre value there)."""
    rec = np.ascontiguousarray(records, np.int32).reshape(-1, 8)
    val = rec[:, 2:7].view(np.float32).astype(np.float64)
    out = rec[:, :2].astype(np.float64)
    for k in range(len(rec)):
        r, s = int(rec[k, 0]), int(rec[k, 1])
        if shape is None or 0 < r < int(shape[0]) - 1:
            out[k, 0] += _parabola(val[k, 1], val[k, 0], val[k, 2])
        if shape is None or 0 < s < int(shape[1]) - 1:
            out[k, 1] += _parabola(val[k, 3], val[k, 0], val[k, 4])
    return out


def marker_detector_coordinate(angles_deg, N):
    """(Nangles, 2) float64 rows ``u_a`` = (-sin theta_a, cos theta_a): a point at (y, z) voxels from the centre of a slice
    (voxel index minus (N-1)/2 along the first and second axis of the slice) is seen in projection a at ray coordinate
    ``(N-1)/2 + u_a . (y, z)``.  From the ray convention of sysmat.cpp: ray j passes through offset_j (cos, sin) with direction
    (-sin, cos), offset_j = j - (N-1)/2, and voxel (iy, iz) is the unit square centred at x = iz - (N-1)/2, y_math = (N-1)/2 - iy
    (column floor(N/2 - y_math) * N + floor(x + N/2)); a point lies on the ray whose offset is x cos + y_math sin."""
    t = np.deg2rad(np.asarray(angles_deg, np.float64).ravel())
    return np.stack([-np.sin(t), np.cos(t)], axis=1)


def _nearest(P, Q):
    """for every row of P the index of and the distance to the nearest row of Q (first on ties)"""
    d = np.sqrt(((P[:, None, :] - Q[None, :, :]) ** 2).sum(2))
    k = np.argmin(d, axis=1)
    return k, d[np.arange(len(P)), k]


def link_markers(positions, angles_deg, N, search_radius, min_views, max_misses=MARKER_MAX_MISSES, max_offset=None):
    """Follow markers through the series.  ``positions[a]`` = (n_a, 2) detections (r, s) of projection a.  -> a list of tracks, each
    a (k, 3) float64 array of rows (a, r, s) sorted by a, k >= ``min_views``.

    The projection nearest zero tilt starts one track per detection; the others are visited outwards from it, first towards higher
    indices, then towards lower ones.  In a visited projection every live track predicts its position: its last position, or, once
    it has three points, the sinusoid ``(N-1)/2 + u_a . (y, z)`` fitted to them (``marker_detector_coordinate``) with the mean of its
    s.  A shift of a whole projection moves all its detections together, so the predictions are first moved by one common offset:
    among the differences (detection - prediction) no longer than ``max_offset`` (default 2 ``search_radius``: the shift of a
    projection against the starting one), the one with the least sum over the tracks of
    min(distance to the nearest detection, ``search_radius``)^2; no offset is a candidate too, and wins ties.
    Tracks remember positions with that offset removed, so it does not enter later predictions.  Then a track takes the
    detection nearest its moved prediction if that is within ``search_radius`` AND the track is that detection's nearest live
    track: a choice that is not mutual is a miss.  A track ends after more than ``max_misses`` consecutive misses in one
    direction (it can still grow in the other); a detection nobody took starts no new track."""
    ang = np.asarray(angles_deg, np.float64).ravel()
    P = len(ang)
    if len(positions) != P:
        raise ValueError("positions must hold one array per projection")
    det = [np.asarray(p, np.float64).reshape(-1, 2) for p in positions]
    rad = float(search_radius)
    if not rad > 0.0 or int(min_views) < 1 or int(max_misses) < 0:
        raise ValueError("search_radius must be positive, min_views at least 1 and max_misses not negative")
    far = 2.0 * rad if max_offset is None else float(max_offset)
    U, c = marker_detector_coordinate(ang, N), 0.5 * (N - 1)
    a0 = int(np.argmin(np.abs(ang)))
    # a track: {a: (observed r, observed s, r and s with the common offset removed)}
    tracks = [{a0: (p[0], p[1], p[0], p[1])} for p in det[a0]]

    def predict(tr, a):
        pts = np.array([(k, v[2], v[3]) for k, v in sorted(tr.items())])
        if len(pts) < 3:
            last = pts[np.argmin(np.abs(pts[:, 0] - a))]
            return last[1:]
        yz = np.linalg.lstsq(U[pts[:, 0].astype(int)], pts[:, 1] - c, rcond=None)[0]
        return np.array([c + U[a] @ yz, pts[:, 2].mean()])

    for order in (range(a0 + 1, P), range(a0 - 1, -1, -1)):
        misses = [0] * len(tracks)
        for a in order:
            live = [t for t in range(len(tracks)) if misses[t] <= int(max_misses)]
            if not live or not len(det[a]):
                for t in live:
                    misses[t] += 1
                continue
            pred = np.array([predict(tracks[t], a) for t in live])
            diff = (det[a][None, :, :] - pred[:, None, :]).reshape(-1, 2)
            diff = diff[np.sqrt((diff ** 2).sum(1)) <= far]
            diff = np.vstack([np.zeros((1, 2)), diff])                   # no offset is always a candidate, and the first
            cost = [np.sum(np.minimum(_nearest(pred + o, det[a])[1], rad) ** 2) for o in diff]
            off = diff[int(np.argmin(cost))]
            moved = pred + off
            kd, dd = _nearest(moved, det[a])
            kt, _ = _nearest(det[a], moved)
            for i, t in enumerate(live):
                if dd[i] <= rad and kt[kd[i]] == i:
                    q = det[a][kd[i]]
                    tracks[t][a] = (q[0], q[1], q[0] - off[0], q[1] - off[1])
                    misses[t] = 0
                else:
                    misses[t] += 1
    out = [np.array([(a, v[0], v[1]) for a, v in sorted(tr.items())], np.float64) for tr in tracks]
    return [t for t in out if len(t) >= int(min_views)]


def marker_gauge(shifts, angles_deg):
    """``(shifts', (alpha, beta, gamma))``: the shifts without the three modes that marker positions can absorb -- dr loses its
    least-squares components alpha cos theta_a + beta sin theta_a, ds its mean gamma.  Moving every marker by (y, z, sigma) +=
    (beta, -alpha, -gamma) explains the same observations."""
    d = np.array(shifts, np.float64).reshape(-1, 2)
    t = np.deg2rad(np.asarray(angles_deg, np.float64).ravel())
    B = np.stack([np.cos(t), np.sin(t)], axis=1)
    ab = np.linalg.lstsq(B, d[:, 0], rcond=None)[0]
    g = float(d[:, 1].mean())
    d[:, 0] -= B @ ab
    d[:, 1] -= g
    return d, (float(ab[0]), float(ab[1]), g)


def solve_markers(tracks, angles_deg, N, Nslice, rotation=True):
    """The least-squares marker model.  With R(phi) = [[cos, -sin], [sin, cos]] in (r, s), c = ((N-1)/2, (Nslice-1)/2) and
    ``q = R(phi) (obs - c) + d_a`` -- where ``set_alignment(d, rotation_deg=phi)`` (``affine_matrices``) moves an observed position
    to, relative to c -- the model is ``q = (u_a . (y_j, z_j), sigma_j)`` for marker j in projection a (``marker_detector_coordinate``).
    Unknowns: (y, z, sigma) per marker, d_a per projection, and one in-plane rotation phi.

    For a fixed phi the problem is linear and its matrix A does not depend on phi, while the right-hand side is
    cos(phi) b0 + sin(phi) b1.  Variable projection therefore has a closed form: with g0, g1 the parts of b0, b1 outside the range
    of A, phi minimises |cos(phi) g0 + sin(phi) g1| -- the right singular vector of [g0 g1] with the smallest singular value, taken
    in (-90, 90] degrees.  ``rotation=False`` keeps phi = 0.  Then positions and shifts come from one linear solve.

    Gauge: the returned shifts have no component along cos theta_a and sin theta_a in dr and no mean in ds (``marker_gauge``); the
    marker positions carry those modes.  -> dict: ``shifts`` (Nangles, 2), ``rotation_deg``, ``markers`` (J, 3) of (y, z, sigma),
    ``residuals`` (one (k, 2) array per track, q - model in pixels) and ``residual_rms`` (root mean square length over all
    observations).  ``ValueError``: fewer than three markers, or observations that do not determine every unknown beyond the
    gauge (a projection no track visits, a marker seen at too few angles)."""
    ang = np.asarray(angles_deg, np.float64).ravel()
    P, J = len(ang), len(tracks)
    if J < 3:
        raise ValueError(f"marker alignment needs at least three markers, got {J}")
    U = marker_detector_coordinate(ang, N)
    c = np.array([0.5 * (N - 1), 0.5 * (Nslice - 1)])
    trk = [np.asarray(t, np.float64).reshape(-1, 3) for t in tracks]
    nobs = sum(len(t) for t in trk)
    A = np.zeros((2 * nobs, 3 * J + 2 * P))
    b0, b1 = np.zeros(2 * nobs), np.zeros(2 * nobs)
    row = 0
    for j, t in enumerate(trk):
        for a, r, s in t:
            a = int(a)
            if not 0 <= a < P:
                raise ValueError(f"track {j} names projection {a} of {P}")
            A[row, 3 * j:3 * j + 2] = U[a]
            A[row + 1, 3 * j + 2] = 1.0
            A[row, 3 * J + 2 * a] = A[row + 1, 3 * J + 2 * a + 1] = -1.0
            o = np.array([r, s]) - c
            b0[row:row + 2] = o
            b1[row:row + 2] = (-o[1], o[0])
            row += 2
    Uu, sv, Vt = np.linalg.svd(A, full_matrices=False)
    rank = int(np.sum(sv > 1e-10 * sv[0]))
    if rank < A.shape[1] - 3:
        raise ValueError(f"the tracks do not determine the model: rank {rank} where {A.shape[1] - 3} is needed beyond the gauge "
                         "(every projection needs a tracked marker, every marker views at two or more tilts)")
    Q = Uu[:, :rank]
    phi = 0.0
    if rotation:
        G = np.stack([b0 - Q @ (Q.T @ b0), b1 - Q @ (Q.T @ b1)], axis=1)
        v = np.linalg.svd(G, full_matrices=False)[2][-1]
        if v[0] < 0.0 or (v[0] == 0.0 and v[1] < 0.0):
            v = -v
        phi = float(np.arctan2(v[1], v[0]))
    b = np.cos(phi) * b0 + np.sin(phi) * b1
    x = Vt[:rank].T @ ((Q.T @ b) / sv[:rank])
    res = (b - A @ x).reshape(-1, 2)
    shifts, (alpha, beta, gamma) = marker_gauge(x[3 * J:].reshape(P, 2), ang)
    markers = x[:3 * J].reshape(J, 3) + np.array([beta, -alpha, -gamma])
    cut = np.cumsum([len(t) for t in trk])[:-1]
    return dict(shifts=shifts, rotation_deg=float(np.rad2deg(phi)), markers=markers, residuals=np.split(res, cut),
                residual_rms=float(np.sqrt(np.mean((res ** 2).sum(1)))))
