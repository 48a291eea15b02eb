"""Binary64 statement of ``tomo_volume_affine_normal`` (the 32 sums of one Gauss-Newton iteration of the rigid registration of two
volumes), a bound for each sum, a binary32 replay of the kernel's value and gradient arithmetic with four deliberately wrong forms, and
the Gauss-Newton loop in numpy.  numpy only; written from the text of include/tomo_hip.h and the docstrings of ``align``, on the
coordinate helpers of tests/ref64_affine3d.py.

Volumes are ``X[s][y][z]``; ``F`` is the fixed volume, ``G`` the moving one, ``M`` the 12 entries of the map from a voxel x of F to its
position p = M x in G.  A voxel counts when the cell of p lies inside G (0 <= floor and floor + 1 <= size - 1 per axis) and x lies
``margin`` voxels inside F.  Per counting voxel: w = the trilinear value, g = the gradient of the trilinear interpolant of the cell,
r = w - F(x), q = p - (size_G - 1) / 2, J = (g, q x g); the sums are the upper triangle of J^T J [0..20], J^T r [21..26], sum r^2 [27],
the count [28], sum F^2, sum w^2, sum F w [29..31].

The bound of ``bound`` (u = 2^-24), per sum: the per-voxel errors of w and g, carried through the products by the magnitudes that
multiply them, summed over the counting voxels, plus the binary64 summation term.

* w: the per-element bound of ``ref64_affine3d.bound`` (12 u of sum |w x| plus the position term).
* g, per component a with b, c the two other axes: g_a = sum over the four (db, dc) of (w_b w_c) e, e the tap difference along a.
  Arithmetic: the difference rounds once (u |e|), a weight product carries at most two roundings (1 - t and the product), the first
  term's product or a term's fused multiply-add one more, and the running sum three: at most 7 u of sum |w_b w_c| |e| to first order,
  taken as 8 u.  Position: g_a is linear in t_b and in t_c and does not depend on t_a inside a cell; moving t_b by delta_b changes it by
  at most delta_b (max e - min e) over the four differences, likewise c, with delta = 2^-24 (the fraction rounded to binary32) plus
  12 * 2^-53 of |m0| s + |m1| y + |m2| z + |m3| (the coordinate chains of both sides), as in ref64_affine3d.  An axis whose matrix row
  is all whole numbers has exact coordinates on both sides and delta = 0.
* q: 12 * 2^-53 of the same magnitude; the cross product's own binary64 roundings 4 * 2^-53 of |q_b g_c| + |q_c g_b|.
* A voxel within delta of a cell face along an axis with delta > 0 ("near") may sit in the neighbouring cell on the other side: g_a
  jumps there and the voxel may start or stop counting.  Such a voxel enters every bound with the full magnitude of its term, built
  from |g_a| <= 2 (max G - min G), and the count's bound with 1.  No map of the tests has one; the code is there so that the bound
  stays a bound.
* Summation: n terms added in binary64 in any order are off by at most (n - 1) 2^-53 sum |term|; the fused multiply-add that forms
  a term rounds with the addition.  Taken as (n + 64) 2^-53 sum |term| to pay for numpy's own pairwise sum as well.
"""
import numpy as np

import ref64_affine3d as A3
import ref64_bin as B

U, U64 = 2.0 ** -24, 2.0 ** -53
PAIRS = [(a, b) for a in range(6) for b in range(a, 6)]
OTHER = {0: (1, 2), 1: (2, 0), 2: (0, 1)}            # the two other axes of (s, y, z), in the cyclic order of the cross product


def _margin_mask(fshape, margin):
    g = A3._grid(fshape)
    ok = np.ones(fshape, bool)
    for a in range(3):
        ok &= (g[a] >= margin) & (g[a] <= fshape[a] - 1 - margin)
    return ok


def _taps(G, idx):
    """T[ds][dy][dz], zero outside G"""
    return [[[A3._tap(G, idx[0] + ds, idx[1] + dy, idx[2] + dz) for dz in (0, 1)] for dy in (0, 1)] for ds in (0, 1)]


def _diffs(T, a):
    """the four tap differences along axis a, indexed [db][dc] by the offsets along the two other axes b, c = OTHER[a]"""
    def tap(o):
        return T[o[0]][o[1]][o[2]]
    out = [[None, None], [None, None]]
    b, c = OTHER[a]
    for db in (0, 1):
        for dc in (0, 1):
            hi, lo = [0, 0, 0], [0, 0, 0]
            hi[a], lo[a] = 1, 0
            hi[b] = lo[b] = db
            hi[c] = lo[c] = dc
            with np.errstate(invalid="ignore"):
                out[db][dc] = tap(hi) - tap(lo)
    return out


def _cross(q, g):
    return [q[1] * g[2] - q[2] * g[1], q[2] * g[0] - q[0] * g[2], q[0] * g[1] - q[1] * g[0]]


def _assemble(ok, J, r, Fv, w):
    """the 32 sums over the voxels of ``ok`` (a voxel outside contributes nothing, whatever it holds)"""
    def s(term):
        with np.errstate(invalid="ignore", over="ignore"):
            return float(np.sum(np.where(ok, term, 0.0)))
    with np.errstate(invalid="ignore", over="ignore"):
        out = [s(J[a] * J[b]) for a, b in PAIRS] + [s(J[a] * r) for a in range(6)]
        out += [s(r * r), float(np.count_nonzero(ok)), s(Fv * Fv), s(w * w), s(Fv * w)]
    return np.array(out)


def pieces(F, G, M, margin=1):
    """the per-voxel quantities of the statement, binary64: dict(ok, w, g[3], r, q[3], J[6], and the geometry c, cm, idx, frac, T)"""
    F, G = np.asarray(F, np.float64), np.asarray(G, np.float64)
    c, cm = A3._coords(M, F.shape)
    idx, frac = zip(*(A3._floor_int(c[a], G.shape[a]) for a in range(3)))
    ok = _margin_mask(F.shape, margin)
    for a in range(3):
        ok &= (idx[a] >= 0) & (idx[a] + 1 <= G.shape[a] - 1)
    T = _taps(G, idx)
    wt = [[1.0 - frac[a], frac[a]] for a in range(3)]
    w = np.zeros(F.shape)
    with np.errstate(invalid="ignore"):
        for ds in (0, 1):
            for dy in (0, 1):
                for dz in (0, 1):
                    k = wt[0][ds] * wt[1][dy] * wt[2][dz]
                    w += np.where(k == 0.0, 0.0, k * T[ds][dy][dz])
        g = []
        for a in range(3):
            b, cc = OTHER[a]
            e = _diffs(T, a)
            g.append(sum(wt[b][db] * wt[cc][dc] * e[db][dc] for db in (0, 1) for dc in (0, 1)))
        q = [c[a] - 0.5 * (G.shape[a] - 1) for a in range(3)]
        J = g + _cross(q, g)
        r = w - F
    return dict(ok=ok, w=w, g=g, r=r, q=q, J=J, c=c, cm=cm, idx=idx, frac=frac, T=T, F=F)


def normal(F, G, M, margin=1):
    """the 32 sums, binary64"""
    p = pieces(F, G, M, margin)
    return _assemble(p["ok"], p["J"], p["r"], p["F"], p["w"])


def normal_loops(F, G, M, margin=1):
    """the same with three plain loops and eight explicit taps"""
    F, G = np.asarray(F, np.float64), np.asarray(G, np.float64)
    m = np.asarray(M, np.float64).reshape(3, 4)
    out = np.zeros(32)
    for s in range(F.shape[0]):
        for y in range(F.shape[1]):
            for z in range(F.shape[2]):
                x = (s, y, z)
                if any(x[a] < margin or x[a] > F.shape[a] - 1 - margin for a in range(3)):
                    continue
                p = [m[a, 0] * s + m[a, 1] * y + m[a, 2] * z + m[a, 3] for a in range(3)]
                i = [int(np.floor(v)) for v in p]
                if any(i[a] < 0 or i[a] + 1 > G.shape[a] - 1 for a in range(3)):
                    continue
                t = [v - fl for v, fl in zip(p, i)]
                X = G[i[0]:i[0] + 2, i[1]:i[1] + 2, i[2]:i[2] + 2]
                ws, wy, wz = [(1 - v, v) for v in t]
                w = sum(ws[a] * wy[b] * wz[c] * X[a, b, c] for a in (0, 1) for b in (0, 1) for c in (0, 1))
                g = [sum(wy[b] * wz[c] * (X[1, b, c] - X[0, b, c]) for b in (0, 1) for c in (0, 1)),
                     sum(ws[a] * wz[c] * (X[a, 1, c] - X[a, 0, c]) for a in (0, 1) for c in (0, 1)),
                     sum(ws[a] * wy[b] * (X[a, b, 1] - X[a, b, 0]) for a in (0, 1) for b in (0, 1))]
                q = [p[a] - 0.5 * (G.shape[a] - 1) for a in range(3)]
                J = g + [q[1] * g[2] - q[2] * g[1], q[2] * g[0] - q[0] * g[2], q[0] * g[1] - q[1] * g[0]]
                r = w - F[x]
                out[:21] += [J[a] * J[b] for a, b in PAIRS]
                out[21:27] += [J[a] * r for a in range(6)]
                out[27:] += [r * r, 1.0, F[x] * F[x], w * w, F[x] * w]
    return out


def unpack(out):
    """-> (H 6 x 6 symmetric, b, ssd, count, ncc)"""
    H = np.zeros((6, 6))
    H[np.triu_indices(6)] = out[:21]
    H = H + np.triu(H, 1).T
    den = out[29] * out[30]
    return H, np.array(out[21:27]), float(out[27]), int(out[28]), (float(out[31] / np.sqrt(den)) if den > 0 else 0.0)


# ---- the bound -----------------------------------------------------------------------------------------------------------------------
def _box(v, m):
    """the voxels at least m from every face: the margin rule is a slice"""
    return v[m:v.shape[0] - m, m:v.shape[1] - m, m:v.shape[2] - m]


def count(fshape, gshape, M, margin=1):
    """the number of counting voxels alone: coordinates, floors and two masks"""
    c, _ = A3._coords(M, fshape)
    ok = np.ones(fshape, bool)
    for a in range(3):
        i, _ = A3._floor_int(c[a], gshape[a])
        ok &= (i >= 0) & (i + 1 <= gshape[a] - 1)
    return int(np.count_nonzero(_box(ok, margin))) if 2 * margin < min(fshape) else 0


def evaluate(F, G, M, margins=(1,)):
    """-> {margin: (the 32 sums of the statement, the bound of |kernel - statement| for each, its summation term alone)} (module
    docstring).  The per-voxel quantities do not depend on the margin, which only cuts a box out of them: they are formed once, one
    sum at a time, and every margin takes its slice."""
    p = pieces(F, G, M, 0)
    F, G = p["F"], np.asarray(G, np.float64)
    m = np.asarray(M, np.float64).reshape(3, 4)
    ok, c, cm, frac, T = p["ok"], p["c"], p["cm"], p["frac"], p["T"]
    exact = [bool(np.all(m[a] == np.round(m[a]))) for a in range(3)]
    delta = [np.zeros(F.shape) if exact[a] else U + A3.DCOORD * cm[a] for a in range(3)]
    near = np.zeros(F.shape, bool)
    for a in range(3):
        if not exact[a]:
            near |= ((frac[a] <= delta[a]) | (1.0 - frac[a] <= delta[a])) & (c[a] > -2.0) & (c[a] < G.shape[a] + 1.0)
    any_near = bool(near.any())
    finite = G[np.isfinite(G)]
    rng = float(finite.max() - finite.min()) if finite.size else 0.0
    with np.errstate(invalid="ignore", over="ignore"):
        # a whole-voxel map has exact coordinates and zero fractions on both sides: w is a copy of a sample, without error
        eW = np.zeros(F.shape) if all(exact) else np.where(near, rng, A3.bound(G, M, F.shape))
        wt = [[1.0 - frac[a], frac[a]] for a in range(3)]
        eG = []
        for a in range(3):
            b, cc = OTHER[a]
            e = _diffs(T, a)
            flat = [e[db][dc] for db in (0, 1) for dc in (0, 1)]
            mag = sum(np.abs(wt[b][db] * wt[cc][dc] * e[db][dc]) for db in (0, 1) for dc in (0, 1))
            spread = np.maximum.reduce(flat) - np.minimum.reduce(flat)
            eG.append(np.where(near, 2.0 * rng, 8.0 * U * mag + (delta[b] + delta[cc]) * spread))
        aG = [np.where(near, 0.0, np.abs(v)) for v in p["g"]]            # a near voxel: |g| <= eG alone
        aQ, eQ = [np.abs(v) for v in p["q"]], [A3.DCOORD * cm[a] for a in range(3)]
        J, aJ, eJ = p["J"], list(aG), list(eG)
        for a in range(3):
            b, cc = OTHER[a]                                             # (q x g)_a = q_b g_c - q_c g_b
            aJ.append(np.where(near, 0.0, np.abs(J[3 + a])))
            eJ.append(aQ[b] * eG[cc] + aQ[cc] * eG[b] + eQ[b] * (aG[cc] + eG[cc]) + eQ[cc] * (aG[b] + eG[b])
                      + 4.0 * U64 * (aQ[b] * (aG[cc] + eG[cc]) + aQ[cc] * (aG[b] + eG[b])))
        r, w = p["r"], p["w"]
        aR = np.where(near, np.abs(F), np.abs(r))
        aW, aF, zero, one = np.where(near, 0.0, np.abs(w)), np.abs(F), np.zeros(F.shape), np.ones(F.shape)

        def terms():
            """per sum: (the term, its error, the full magnitude a near voxel enters with), one at a time"""
            for a, b in PAIRS:
                yield J[a] * J[b], aJ[a] * eJ[b] + aJ[b] * eJ[a] + eJ[a] * eJ[b], (aJ[a] + eJ[a]) * (aJ[b] + eJ[b])
            for a in range(6):
                yield J[a] * r, aJ[a] * eW + aR * eJ[a] + eJ[a] * eW, (aJ[a] + eJ[a]) * (aR + eW)
            yield r * r, 2.0 * aR * eW + eW * eW, (aR + eW) ** 2
            yield one, zero, one
            yield F * F, zero, F * F
            yield w * w, 2.0 * aW * eW + eW * eW, (aW + eW) ** 2
            yield F * w, aF * eW, aF * (aW + eW)
        margins = [int(v) for v in margins]
        use = ok & ~near
        ref, mag, tot = ({v: [] for v in margins} for _ in range(3))
        for val, err, full in terms():
            v_ok = np.where(ok, val, 0.0)
            a_ok, e_use = np.abs(v_ok), np.where(use, err, 0.0)
            f_near = np.where(near, full, 0.0) if any_near else None
            for v in margins:
                ref[v].append(float(np.sum(_box(v_ok, v))))
                mag[v].append(float(np.sum(_box(a_ok, v))))
                tot[v].append(float(np.sum(_box(e_use, v))) + (float(np.sum(_box(f_near, v))) if any_near else 0.0))
    out = {}
    for v in margins:
        n = int(np.count_nonzero(_box(ok, v)))
        summ = (n + 64) * U64 * np.array(mag[v])
        summ[28] = 0.0                                                   # whole numbers below 2^53: every partial sum is exact
        sums = np.array(ref[v])
        sums[28] = float(n)
        out[v] = (sums, np.array(tot[v]) + summ, summ)
    return out


def bound(F, G, M, margin=1):
    """-> (the bound for each of the 32 sums, its summation term alone) at one margin"""
    _, bnd, summ = evaluate(F, G, M, (margin,))[int(margin)]
    return bnd, summ


def ratios(got, ref, bnd):
    """|got - ref| / bound per sum; a sum with bound 0 must be exact (inf otherwise)"""
    err = np.abs(np.asarray(got, np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bnd > 0, err / bnd, np.where(err == 0, 0.0, np.inf))
    return np.where(np.isfinite(err), r, np.inf)


# ---- the kernel's arithmetic restated ------------------------------------------------------------------------------------------------
def _fma32(a, b, c):
    """fmaf: the product of two binary32 values is exact in binary64; added there and rounded to binary32"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def normal_replay_f32(F, G, M, margin=1, nearest_gradient=False, corner=False, cross_sign=False, zero_padded=False):
    """Coordinates and their split in binary64 (the chain's inner link first), the fraction rounded to binary32 (one that rounds to 1
    is the next whole voxel); w with the arithmetic of ``ref64_affine3d.affine_replay_f32``; per gradient component the four tap
    differences along its axis (binary32), the first weighted by the product of the two other axes' weights, the others added by
    fused multiply-adds in ascending order of the two other offsets -- g_s over (dy, dz), g_y over (dz, ds), g_z over (dy, ds), the
    first-named offset slowest; r, q, J and the sums in binary64.
    The deliberately wrong forms: ``nearest_gradient`` takes the one difference of the nearest tap pair with weight 1;  ``corner``
    takes q about the corner (c_G = 0);  ``cross_sign`` takes g x q;  ``zero_padded`` counts every voxel whose coordinates lie in
    (-1, size) with taps outside G as zero (the inclusion rule of ``tomo_volume_affine``)."""
    F32, G32 = np.asarray(F, np.float32), np.asarray(G, np.float32)
    fshape = F32.shape
    m = np.asarray(M, np.float64).reshape(3, 4)
    s, y, z = A3._grid(fshape)
    one, zero = np.float32(1.0), np.float32(0.0)
    idx, frac, coord = [], [], []
    ok = _margin_mask(fshape, margin)
    for a in range(3):
        c = m[a, 0] * s + (m[a, 1] * y + (m[a, 2] * z + m[a, 3]))
        coord.append(c)
        with np.errstate(invalid="ignore"):
            inside = (c > -1.0) & (c < G32.shape[a]) if zero_padded else (c >= 0.0) & (c < G32.shape[a])
        cz = np.where(inside, c, 0.0)
        f = np.floor(cz)
        t = (cz - f).astype(np.float32)
        i = f.astype(np.int64)
        i, t = np.where(t >= one, i + 1, i), np.where(t >= one, zero, t)
        idx.append(i), frac.append(t)
        ok &= inside if zero_padded else inside & (i + 1 <= G32.shape[a] - 1)
    w = A3.affine_replay_f32(G32, M, fshape)
    wt = [[np.where(t == 0, one, one - t), t] for t in frac]
    T = [[[A3._tap(G32, idx[0] + ds, idx[1] + dy, idx[2] + dz).astype(np.float32) for dz in (0, 1)] for dy in (0, 1)] for ds in (0, 1)]
    order = {0: (1, 2), 1: (2, 0), 2: (1, 0)}                            # (slow, fast) offsets of each component's four terms
    g = []
    with np.errstate(invalid="ignore", over="ignore"):
        for a in range(3):
            b, c2 = order[a]

            def diff(db, dc):
                hi, lo = [0, 0, 0], [0, 0, 0]
                hi[a] = 1
                hi[b] = lo[b] = db
                hi[c2] = lo[c2] = dc
                return T[hi[0]][hi[1]][hi[2]] - T[lo[0]][lo[1]][lo[2]]
            if nearest_gradient:
                nb, nc = frac[b] >= np.float32(0.5), frac[c2] >= np.float32(0.5)
                ga = np.where(nb, np.where(nc, diff(1, 1), diff(1, 0)), np.where(nc, diff(0, 1), diff(0, 0)))
            else:
                ga = (wt[b][0] * wt[c2][0]) * diff(0, 0)
                for db, dc in ((0, 1), (1, 0), (1, 1)):
                    ga = _fma32(wt[b][db] * wt[c2][dc], diff(db, dc), ga)
            g.append(ga.astype(np.float64))
        q = [coord[a] - (0.0 if corner else 0.5 * (G32.shape[a] - 1)) for a in range(3)]
        x = _cross(g, q) if cross_sign else _cross(q, g)
        wd, Fd = w.astype(np.float64), F32.astype(np.float64)
        return _assemble(ok, g + x, wd - Fd, Fd, wd)


# ---- the host side of the loop ---------------------------------------------------------------------------------------------------------
def rodrigues(omega):
    w = np.asarray(omega, np.float64)
    t = float(np.linalg.norm(w))
    if t == 0.0:
        return np.eye(3)
    k = w / t
    K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return np.eye(3) + np.sin(t) * K + (1.0 - np.cos(t)) * (K @ K)


def compose(M, delta, src_shape):
    """x -> c + Rot(delta[3:]) (M x - c) + delta[:3], c the centre of the moving volume"""
    m = np.asarray(M, np.float64).reshape(3, 4)
    c = 0.5 * (np.asarray(src_shape, np.float64) - 1.0)
    Rm = rodrigues(delta[3:])
    return np.hstack([Rm @ m[:, :3], (c + Rm @ (m[:, 3] - c) + np.asarray(delta[:3]))[:, None]]).ravel()


def decode(M, src_shape, dst_shape):
    """(R, shift) of the rigid map M = [R^T | c_src - R^T (c_dst + shift)]"""
    m = np.asarray(M, np.float64).reshape(3, 4)
    cs, cd = 0.5 * (np.asarray(src_shape, np.float64) - 1.0), 0.5 * (np.asarray(dst_shape, np.float64) - 1.0)
    return m[:, :3].T.copy(), np.linalg.solve(m[:, :3], cs - m[:, 3]) - cd


def angle_deg(Rm):
    s = 0.5 * np.sqrt((Rm[2, 1] - Rm[1, 2]) ** 2 + (Rm[0, 2] - Rm[2, 0]) ** 2 + (Rm[1, 0] - Rm[0, 1]) ** 2)
    return float(np.rad2deg(np.arctan2(s, 0.5 * (np.trace(Rm) - 1.0))))


def pose_error(M, M_true, src_shape, dst_shape):
    """(rotation error in degrees, worst shift error in voxels) between two rigid maps"""
    Ra, da = decode(M, src_shape, dst_shape)
    Rb, db = decode(M_true, src_shape, dst_shape)
    return angle_deg(Ra @ Rb.T), float(np.max(np.abs(da - db)))


def gauss_newton(F, G, M0=None, max_iter=30, tol_shift=1e-3, tol_deg=1e-3, margin=1, sums=normal):
    """``align.register_volumes`` on the CPU: per iteration the 32 sums at M (``sums`` = ``normal`` or ``normal_replay_f32``), the
    step of H delta = -b, the composition; stops when a step is below both tolerances or after ``max_iter`` steps.
    -> (M, dict(ssd, count, step))"""
    F, G = np.asarray(F), np.asarray(G)
    M = np.eye(3, 4).ravel() if M0 is None else np.array(M0, np.float64).ravel()
    if M0 is None:
        M[3::4] = 0.5 * (np.asarray(G.shape, np.float64) - 1.0) - 0.5 * (np.asarray(F.shape, np.float64) - 1.0)
    hist = dict(ssd=[], count=[], step=[])
    for _ in range(int(max_iter)):
        H, b, ssd, count, _ = unpack(sums(F, G, M, margin))
        hist["ssd"].append(ssd), hist["count"].append(count)
        if 8 * count < F.size:
            raise RuntimeError("the volumes no longer overlap")
        delta = np.linalg.solve(H, -b)
        M = compose(M, delta, G.shape)
        step = (float(np.max(np.abs(delta[:3]))), float(np.rad2deg(np.linalg.norm(delta[3:]))))
        hist["step"].append(step)
        if step[0] <= tol_shift and step[1] <= tol_deg:
            break
    return M, hist


def pyramid(F, G, factors=(4, 2, 1), **kw):
    """``DualAxisTomo.estimate_registration(pyramid=...)`` on the CPU for two cubes of one size: per level both volumes binned in
    binary64 (``ref64_bin.bin_volume``), the loop from the level before's rotation and its shift scaled by the ratio of the factors.
    -> (M at full resolution, the per-level (factor, M, hist))"""
    F, G = np.asarray(F, np.float64), np.asarray(G, np.float64)
    Rm, d, levels = np.eye(3), np.zeros(3), []
    for f in factors:
        Ff, Gf = (F, G) if f == 1 else (B.bin_volume(F, f)[0], B.bin_volume(G, f)[0])
        c = 0.5 * (np.asarray(Ff.shape, np.float64) - 1.0)
        M0 = np.hstack([Rm.T, (c - Rm.T @ (c + d / f))[:, None]]).ravel()
        M, hist = gauss_newton(Ff, Gf, M0, **kw)
        Rm, d = decode(M, Gf.shape, Ff.shape)
        d = d * f
        levels.append((f, M, hist))
    return levels[-1][1], levels
