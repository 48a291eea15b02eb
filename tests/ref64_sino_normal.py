"""Binary64 statement of ``tomo_sino_affine_normal`` (per projection the 21 sums of one Gauss-Newton iteration of the matching by shift,
in-plane rotation and magnification), a bound for each sum, a binary32 replay of the kernel's value and gradient arithmetic with three
deliberately wrong forms, and the Gauss-Newton loop of ``align.match_projections`` in numpy.  numpy only; written from the text of
include/tomo_hip.h and the docstrings of ``align``, on the coordinate helpers of tests/ref64_affine.py.

Images are ``X[a][r][s]``; ``F`` is the fixed series (the model), ``G`` the moving one, ``M[a]`` the 6 entries of the map from a sample
x = (r, s) of F_a to its position p = M x in G_a.  A sample counts when the cell of p lies inside G (0 <= floor and floor + 1 <= size - 1
on both axes) and x lies ``margin`` pixels inside F.  Per counting sample: w = the bilinear value, g = the gradient of the bilinear
interpolant of the cell, res = w - F(x), q = p - ((N-1)/2, (ns-1)/2), J = (g_r, g_s, q_r g_s - q_s g_r, q_r g_r + q_s g_s); the sums are
the upper triangle of J^T J [0..9], J^T res [10..13], sum res^2 [14], the count [15], sum F^2, sum w^2, sum F w [16..18], sum F, sum w
[19..20].

The bound of ``bound`` (u = 2^-24), per sum: the per-sample errors of w and g, carried through the products by the magnitudes that
multiply them, summed over the counting samples, plus the binary64 summation term.

* w: the per-element bound of ``ref64_affine.bound`` (8 u of sum |w x| plus the position term).
* g, per component a with b the other axis: g_a = u_b[0] e_0 + u_b[1] e_1, e the two tap differences along a.  Arithmetic (the order
  of kernels_align_normal.hip.h): a difference rounds once (u |e|), the weight 1 - t once, the first term's product once, the fused
  multiply-add of the second once: at most 4 u of sum |u_b e| to first order, taken as 5 u.  Position: g_a is linear in t_b and does not
  depend on t_a inside a cell; moving t_b by delta_b changes it by at most delta_b |e_1 - e_0|, with delta = 2^-24 (the fraction
  rounded to binary32) plus 8 * 2^-53 of |m0| r + |m1| s + |m2| (the coordinate chains of both sides), as in ref64_affine.  An axis
  whose matrix row is all whole numbers has exact coordinates on both sides and delta = 0.
* q: 8 * 2^-53 of the same magnitude; the two products of J[2] and J[3] in binary64, 4 * 2^-53 of |q_r g| + |q_s g|.
* A sample within delta of a cell face along an axis with delta > 0 ("near") may sit in the neighbouring cell on the other side: g
  jumps there and the sample may start or stop counting.  Such a sample enters every bound with the full magnitude of its term, built
  from |g| <= 2 (max G - min G), and the count's bound with 1.  No map of the tests has one; the code is there so that the bound stays
  a bound.
* Summation: n terms added in binary64 in any order are off by at most (n - 1) 2^-53 sum |term|; the fused multiply-add that forms a
  term rounds with the addition.  Taken as (n + 64) 2^-53 sum |term| to pay for numpy's own pairwise sum as well.
"""
import numpy as np

import ref64_affine as RF

U, U64 = 2.0 ** -24, 2.0 ** -53
NS = 21
PAIRS = [(a, b) for a in range(4) for b in range(a, 4)]


def _margin_mask(N, ns, margin):
    r, s = np.meshgrid(np.arange(N), np.arange(ns), indexing="ij")
    return (r >= margin) & (r <= N - 1 - margin) & (s >= margin) & (s <= ns - 1 - margin)


def _assemble(ok, J, res, Fv, w):
    """the 21 sums over the samples of ``ok`` (a sample outside contributes nothing, whatever it holds)"""
    def s(term):
        with np.errstate(invalid="ignore", over="ignore"):
            return float(np.sum(np.where(ok, term, 0.0)))
    with np.errstate(invalid="ignore", over="ignore"):
        out = [s(J[a] * J[b]) for a, b in PAIRS] + [s(J[a] * res) for a in range(4)]
        out += [s(res * res), float(np.count_nonzero(ok)), s(Fv * Fv), s(w * w), s(Fv * w), s(Fv), s(w)]
    return np.array(out)


def pieces(Fa, Ga, m, margin):
    """the per-sample quantities of the statement for one projection, binary64"""
    Fa, Ga, m = np.asarray(Fa, np.float64), np.asarray(Ga, np.float64), np.asarray(m, np.float64)
    N, ns = Fa.shape
    rp, sp, r, s = RF._coords(m, N, ns)
    i, tr = RF._floor_int(rp, N)
    j, ts = RF._floor_int(sp, ns)
    ok = _margin_mask(N, ns, margin) & (i >= 0) & (i + 1 <= N - 1) & (j >= 0) & (j + 1 <= ns - 1)
    T = [[RF._tap(Ga, i + di, j + dj) for dj in (0, 1)] for di in (0, 1)]
    ur, us = [1.0 - tr, tr], [1.0 - ts, ts]
    with np.errstate(invalid="ignore", over="ignore"):
        w = np.zeros((N, ns))
        for di in (0, 1):
            for dj in (0, 1):
                k = ur[di] * us[dj]
                w += np.where(k == 0.0, 0.0, k * T[di][dj])
        er, es = [T[1][0] - T[0][0], T[1][1] - T[0][1]], [T[0][1] - T[0][0], T[1][1] - T[1][0]]
        g = [us[0] * er[0] + us[1] * er[1], ur[0] * es[0] + ur[1] * es[1]]
        q = [rp - 0.5 * (N - 1), sp - 0.5 * (ns - 1)]
        J = g + [q[0] * g[1] - q[1] * g[0], q[0] * g[0] + q[1] * g[1]]
        res = w - Fa
    cm = [abs(m[0]) * r + abs(m[1]) * s + abs(m[2]), abs(m[3]) * r + abs(m[4]) * s + abs(m[5])]
    return dict(ok=ok, w=w, g=g, res=res, q=q, J=J, c=[rp, sp], cm=cm, frac=[tr, ts], e=[er, es], wt=[ur, us], F=Fa)


def normal(F, G, M, margin=1):
    """the (P, 21) sums, binary64"""
    out = []
    for a in range(len(F)):
        p = pieces(F[a], G[a], M[a], margin)
        out.append(_assemble(p["ok"], p["J"], p["res"], p["F"], p["w"]))
    return np.array(out)


def normal_loops(F, G, M, margin=1):
    """the same with plain loops and four explicit taps"""
    F, G, M = np.asarray(F, np.float64), np.asarray(G, np.float64), np.asarray(M, np.float64)
    P, N, ns = F.shape
    out = np.zeros((P, NS))
    for a in range(P):
        m = M[a]
        for r in range(N):
            for s in range(ns):
                if r < margin or r > N - 1 - margin or s < margin or s > ns - 1 - margin:
                    continue
                p = (m[0] * r + m[1] * s + m[2], m[3] * r + m[4] * s + m[5])
                i, j = int(np.floor(p[0])), int(np.floor(p[1]))
                if i < 0 or i + 1 > N - 1 or j < 0 or j + 1 > ns - 1:
                    continue
                tr, ts = p[0] - i, p[1] - j
                X = G[a, i:i + 2, j:j + 2]
                w = (1 - tr) * (1 - ts) * X[0, 0] + (1 - tr) * ts * X[0, 1] + tr * (1 - ts) * X[1, 0] + tr * ts * X[1, 1]
                gr = (1 - ts) * (X[1, 0] - X[0, 0]) + ts * (X[1, 1] - X[0, 1])
                gs = (1 - tr) * (X[0, 1] - X[0, 0]) + tr * (X[1, 1] - X[1, 0])
                qr, qs = p[0] - 0.5 * (N - 1), p[1] - 0.5 * (ns - 1)
                J = [gr, gs, qr * gs - qs * gr, qr * gr + qs * gs]
                f = F[a, r, s]
                res = w - f
                out[a, :10] += [J[x] * J[y] for x, y in PAIRS]
                out[a, 10:14] += [J[x] * res for x in range(4)]
                out[a, 14:] += [res * res, 1.0, f * f, w * w, f * w, f, w]
    return out


def unpack(out):
    """-> (H (P, 4, 4) symmetric, b (P, 4), ssd, count, ncc): the mean-subtracted normalised correlation, 0 where undefined"""
    out = np.asarray(out, np.float64).reshape(-1, NS)
    P = out.shape[0]
    H = np.zeros((P, 4, 4))
    for k, (a, b) in enumerate(PAIRS):
        H[:, a, b] = H[:, b, a] = out[:, k]
    ncc = np.zeros(P)
    for a in range(P):
        n = out[a, 15]
        if n > 0:
            vf, vw = out[a, 16] - out[a, 19] ** 2 / n, out[a, 17] - out[a, 20] ** 2 / n
            if vf > 0 and vw > 0:
                ncc[a] = (out[a, 18] - out[a, 19] * out[a, 20] / n) / np.sqrt(vf * vw)
    return H, out[:, 10:14].copy(), out[:, 14].copy(), out[:, 15].astype(np.int64), ncc


# ---- the bound -----------------------------------------------------------------------------------------------------------------------
def bound(F, G, M, margin=1):
    """-> (the (P, 21) sums of the statement, the bound of |kernel - statement| for each, its summation term alone) (module docstring)"""
    F, G, M = np.asarray(F, np.float64), np.asarray(G, np.float64), np.asarray(M, np.float64)
    P, N, ns = F.shape
    eW_all = RF.bound(G, M)
    refs, bnds, summs = [], [], []
    for a in range(P):
        p = pieces(F[a], G[a], M[a], margin)
        m, ok, c, cm, frac, Fa = M[a], p["ok"], p["c"], p["cm"], p["frac"], p["F"]
        size = (N, ns)
        exact = [bool(np.all(m[3 * k:3 * k + 3] == np.round(m[3 * k:3 * k + 3]))) for k in range(2)]
        delta = [np.zeros((N, ns)) if exact[k] else U + RF.DCOORD * cm[k] for k in range(2)]
        near = np.zeros((N, ns), bool)
        for k in range(2):
            if not exact[k]:
                near |= ((frac[k] <= delta[k]) | (1.0 - frac[k] <= delta[k])) & (c[k] > -2.0) & (c[k] < size[k] + 1.0)
        finite = G[a][np.isfinite(G[a])]
        rng = float(finite.max() - finite.min()) if finite.size else 0.0
        with np.errstate(invalid="ignore", over="ignore"):
            eW = np.zeros((N, ns)) if all(exact) else np.where(near, rng, eW_all[a])
            eG, aG = [], []
            for k in range(2):
                b = 1 - k
                e, wt = p["e"][k], p["wt"][b]
                mag = np.abs(wt[0] * e[0]) + np.abs(wt[1] * e[1])
                eG.append(np.where(near, 2.0 * rng, 5.0 * U * mag + delta[b] * np.abs(e[1] - e[0])))
                aG.append(np.where(near, 0.0, np.abs(p["g"][k])))
            aQ, eQ = [np.abs(v) for v in p["q"]], [RF.DCOORD * cm[k] for k in range(2)]
            J, aJ, eJ = p["J"], list(aG), list(eG)
            for x, y in ((1, 0), (0, 1)):                                # J[2] = q_r g_s - q_s g_r;  J[3] = q_r g_r + q_s g_s
                aJ.append(np.where(near, 0.0, np.abs(J[len(aJ)])))
                eJ.append(aQ[0] * eG[x] + aQ[1] * eG[y] + eQ[0] * (aG[x] + eG[x]) + eQ[1] * (aG[y] + eG[y])
                          + 4.0 * U64 * (aQ[0] * (aG[x] + eG[x]) + aQ[1] * (aG[y] + eG[y])))
            res, w = p["res"], p["w"]
            aR = np.where(near, np.abs(Fa), np.abs(res))
            aW, aF, zero, one = np.where(near, 0.0, np.abs(w)), np.abs(Fa), np.zeros((N, ns)), np.ones((N, ns))
            terms = [(J[x] * J[y], aJ[x] * eJ[y] + aJ[y] * eJ[x] + eJ[x] * eJ[y], (aJ[x] + eJ[x]) * (aJ[y] + eJ[y])) for x, y in PAIRS]
            terms += [(J[x] * res, aJ[x] * eW + aR * eJ[x] + eJ[x] * eW, (aJ[x] + eJ[x]) * (aR + eW)) for x in range(4)]
            terms += [(res * res, 2.0 * aR * eW + eW * eW, (aR + eW) ** 2), (one, zero, one), (Fa * Fa, zero, Fa * Fa),
                      (w * w, 2.0 * aW * eW + eW * eW, (aW + eW) ** 2), (Fa * w, aF * eW, aF * (aW + eW)), (Fa, zero, aF), (w, eW, aW + eW)]
            in_box = _margin_mask(N, ns, margin)
            use, nr = ok & ~near, near & in_box
            ref, mag, tot = [], [], []
            for val, err, full in terms:
                v_ok = np.where(ok, val, 0.0)
                ref.append(float(np.sum(v_ok)))
                mag.append(float(np.sum(np.abs(v_ok))))
                tot.append(float(np.sum(np.where(use, err, 0.0))) + float(np.sum(np.where(nr, full, 0.0))))
        n = int(np.count_nonzero(ok))
        summ = (n + 64) * U64 * np.array(mag)
        summ[15] = 0.0                                                   # whole numbers below 2^53: every partial sum is exact
        sums = np.array(ref)
        sums[15] = float(n)
        refs.append(sums), bnds.append(np.array(tot) + summ), summs.append(summ)
    return np.array(refs), np.array(bnds), np.array(summs)


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


def normal_replay_f32(F, G, M, margin=1, swapped_gradient=False, corner=False, zero_padded=False):
    """Coordinates and their split in binary64 (the chain's inner link first), the fraction rounded to binary32 (one that rounds to 1 is
    the next whole pixel); w with the arithmetic of ``ref64_affine.affine_replay_f32``; per gradient component the two tap differences
    along its axis (binary32), the first weighted by the other axis's first weight (a product), the second added by a fused
    multiply-add; res, q, J and the sums in binary64.
    The deliberately wrong forms: ``swapped_gradient`` exchanges g_r and g_s;  ``corner`` takes q about the corner (c_G = 0);
    ``zero_padded`` counts every sample whose coordinates lie in (-1, size) with taps outside G as zero (the inclusion rule of
    ``tomo_sino_affine``)."""
    F32, G32, M = np.asarray(F, np.float32), np.asarray(G, np.float32), np.asarray(M, np.float64)
    P, N, ns = F32.shape
    one, zero = np.float32(1.0), np.float32(0.0)
    W = RF.affine_replay_f32(G32, M)
    r, s = np.meshgrid(np.arange(N, dtype=np.float64), np.arange(ns, dtype=np.float64), indexing="ij")
    out = []
    for a in range(P):
        m = M[a]
        coord = [m[0] * r + (m[1] * s + m[2]), m[3] * r + (m[4] * s + m[5])]
        ok = _margin_mask(N, ns, margin)
        idx, frac = [], []
        for k, size in enumerate((N, ns)):
            c = coord[k]
            with np.errstate(invalid="ignore"):
                inside = (c > -1.0) & (c < size)
            cz = np.where(inside, c, 0.0)
            f = np.floor(cz)
            t = (cz - f).astype(np.float32)
            i = f.astype(np.int64)
            i, t = np.where(t >= one, i + 1, i), np.where(t >= one, zero, t)
            idx.append(i), frac.append(t)
            ok &= inside if zero_padded else inside & (i >= 0) & (i + 1 <= size - 1)     # the rule acts on the first tap AFTER the split
        T = [[RF._tap(G32[a], idx[0] + di, idx[1] + dj).astype(np.float32) for dj in (0, 1)] for di in (0, 1)]
        u = [[np.where(t == 0, one, one - t), t] for t in frac]
        with np.errstate(invalid="ignore", over="ignore"):
            gr = _fma32(u[1][1], T[1][1] - T[0][1], u[1][0] * (T[1][0] - T[0][0]))
            gs = _fma32(u[0][1], T[1][1] - T[1][0], u[0][0] * (T[0][1] - T[0][0]))
            if swapped_gradient:
                gr, gs = gs, gr
            g = [gr.astype(np.float64), gs.astype(np.float64)]
            q = [coord[0] - (0.0 if corner else 0.5 * (N - 1)), coord[1] - (0.0 if corner else 0.5 * (ns - 1))]
            J = g + [q[0] * g[1] - q[1] * g[0], q[0] * g[0] + q[1] * g[1]]
            wd, Fd = W[a].astype(np.float64), F32[a].astype(np.float64)
            out.append(_assemble(ok, J, wd - Fd, Fd, wd))
    return np.array(out)


# ---- the host side of the loop ---------------------------------------------------------------------------------------------------------
def identity(P):
    return np.tile(np.array([1.0, 0.0, 0.0, 0.0, 1.0, 0.0]), (P, 1))


def compose(M, delta, N, ns):
    """per projection x -> c + e^lambda Rot(omega)(M x - c) + t, delta = (t_r, t_s, omega, lambda), c the centre of the moving image"""
    M, delta = np.asarray(M, np.float64).reshape(-1, 6), np.asarray(delta, np.float64).reshape(-1, 4)
    c = np.array([0.5 * (N - 1), 0.5 * (ns - 1)])
    out = np.empty_like(M)
    for a in range(len(M)):
        A, t = M[a].reshape(2, 3)[:, :2], M[a].reshape(2, 3)[:, 2]
        co, si, k = np.cos(delta[a, 2]), np.sin(delta[a, 2]), np.exp(delta[a, 3])
        S = k * np.array([[co, -si], [si, co]])
        out[a] = np.hstack([S @ A, (c + S @ (t - c) + delta[a, :2])[:, None]]).ravel()
    return out


def decode(M, N, ns):
    """(shift, rotation_deg, magnification) of the maps M[a] = [A | c - A (c + d)], A = Rot(-phi) / mag (``ref64_affine.matrices``)"""
    M = np.asarray(M, np.float64).reshape(-1, 6)
    c = np.array([0.5 * (N - 1), 0.5 * (ns - 1)])
    d, rot, mag = np.zeros((len(M), 2)), np.zeros(len(M)), np.zeros(len(M))
    for a in range(len(M)):
        A, t = M[a].reshape(2, 3)[:, :2], M[a].reshape(2, 3)[:, 2]
        mag[a] = 1.0 / np.sqrt(np.linalg.det(A))
        rot[a] = np.rad2deg(np.arctan2(A[0, 1] - A[1, 0], A[0, 0] + A[1, 1]))
        d[a] = np.linalg.solve(A, c - t) - c
    return d, rot, mag


def gauss_newton(F, G, M0=None, max_iter=20, tol_shift=1e-3, tol_deg=1e-3, tol_mag=1e-5, margin=2, rotation=True, magnification=True,
                 sums=normal):
    """``align.match_projections`` on the CPU: per iteration the 21 sums of every projection at M (``sums`` = ``normal`` or
    ``normal_replay_f32``), the step of the kept parameters' H delta = -b, the composition; a projection whose step is below all three
    tolerances keeps its map from then on.  -> (M, dict(ssd, count, ncc, step, converged))"""
    F, G = np.asarray(F), np.asarray(G)
    P, N, ns = F.shape
    M = identity(P) if M0 is None else np.array(M0, np.float64).reshape(P, 6)
    keep = [0, 1] + ([2] if rotation else []) + ([3] if magnification else [])
    hist = dict(ssd=[], count=[], ncc=[], step=[])
    done = np.zeros(P, bool)
    for _ in range(int(max_iter)):
        H, b, ssd, count, ncc = unpack(sums(F, G, M, margin))
        hist["ssd"].append(ssd), hist["count"].append(count), hist["ncc"].append(ncc)
        if np.any(8 * count < N * ns):
            raise RuntimeError("the images no longer overlap")
        delta = np.zeros((P, 4))
        for a in range(P):
            if not done[a]:
                delta[a, keep] = np.linalg.solve(H[a][np.ix_(keep, keep)], -b[a, keep])
        M = np.where(done[:, None], M, compose(M, delta, N, ns))
        step = np.stack([np.max(np.abs(delta[:, :2]), axis=1), np.rad2deg(np.abs(delta[:, 2])), np.abs(delta[:, 3])], axis=1)
        hist["step"].append(step)
        done = done | ((step[:, 0] <= tol_shift) & (step[:, 1] <= tol_deg) & (step[:, 2] <= tol_mag))
        if done.all():
            break
    hist["converged"] = done
    return M, hist


# ---- the recovery fixture ------------------------------------------------------------------------------------------------------------
# (Nslice, Nray, P): per projection a model of 9 Gaussian blobs (sigma 1.5 - 3.5 pixels) with centres inside the central half of the
# image, and the moving image = that model warped by a known similarity (shift within +-1.5 pixels, rotation within +-2 degrees,
# magnification within +-2 %, one draw per projection), both sampled from the analytic blobs and rounded to binary32.
RECOVERY_SHAPES = [(70, 33, 5), (40, 48, 4)]


def recovery_case(shape, seed=7):
    """-> (F, G as X[a][r][s] float32, the true maps (P, 6), the true (shift, rotation_deg, magnification))"""
    ns, N, P = shape
    rng = np.random.default_rng(seed + ns)
    d = rng.uniform(-1.5, 1.5, (P, 2))
    rot, mag = rng.uniform(-2.0, 2.0, P), 1.0 + rng.uniform(-0.02, 0.02, P)
    M = RF.matrices(d, rot, mag, N, ns)
    r, s = np.meshgrid(np.arange(N, dtype=np.float64), np.arange(ns, dtype=np.float64), indexing="ij")
    F, G = np.zeros((P, N, ns)), np.zeros((P, N, ns))
    for a in range(P):
        cen = np.stack([rng.uniform(0.25 * (N - 1), 0.75 * (N - 1), 9), rng.uniform(0.25 * (ns - 1), 0.75 * (ns - 1), 9)], axis=1)
        sig, amp = rng.uniform(1.5, 3.5, 9), rng.uniform(0.5, 1.5, 9)

        def blobs(x, y):
            return sum(amp[k] * np.exp(-((x - cen[k, 0]) ** 2 + (y - cen[k, 1]) ** 2) / (2.0 * sig[k] ** 2)) for k in range(9))
        A, t = M[a].reshape(2, 3)[:, :2], M[a].reshape(2, 3)[:, 2]
        inv = np.linalg.inv(A)                                           # G(y) = F(M^-1 y): then F(x) = G(M x) for the continuous images
        F[a] = blobs(r, s)
        G[a] = blobs(inv[0, 0] * (r - t[0]) + inv[0, 1] * (s - t[1]), inv[1, 0] * (r - t[0]) + inv[1, 1] * (s - t[1]))
    return F.astype(np.float32), G.astype(np.float32), M, (d, rot, mag)


# ---- the driver: TomoGPU.refine_alignment_affine(leave_one_out=True) on the CPU ------------------------------------------------------
# The geometry of tests/golden/A_N32_P9.npz (32 rays, 9 projections over +-70 degrees, 32 slices) and the phantom of the alignment
# tests (ref64_align.refine_case); every projection distorted by its own shift (within +-1.2 pixels), rotation (within +-1.5 degrees)
# and magnification (within +-1.5 %): at most about 1.6 + 0.4 + 0.25 pixels at the image border, inside the capture range.
DRIVER_CASE = dict(nslice=32, n=32, nproj=9, seed=3, injected=None, nouter=3, loo_iters=20, dseed=5)


def driver_case(c=None):
    """(angles in degrees, the clean series, the distorted one as X[a][r][s] float32, the distortion's maps (P, 6))"""
    import ref64_align as RA
    c = c or DRIVER_CASE
    ang, clean, _, _ = RA.refine_case(dict(c, injected=[[0, 0]] * c["nproj"]))
    rng = np.random.default_rng(c["dseed"])
    P = c["nproj"]
    Md = RF.matrices(rng.uniform(-1.2, 1.2, (P, 2)), rng.uniform(-1.5, 1.5, P), 1.0 + rng.uniform(-0.015, 0.015, P), c["n"], c["nslice"])
    return ang, clean, RF.affine(clean, Md)[0].astype(np.float32), Md


def chain(Ma, Mb):
    """per projection the map x -> Ma (Mb x)"""
    out = np.empty_like(np.asarray(Mb, np.float64))
    for a in range(len(out)):
        A, ta = Ma[a].reshape(2, 3)[:, :2], Ma[a].reshape(2, 3)[:, 2]
        B, tb = Mb[a].reshape(2, 3)[:, :2], Mb[a].reshape(2, 3)[:, 2]
        out[a] = np.hstack([A @ B, (A @ tb + ta)[:, None]]).ravel()
    return out


def driver_distance(shift, rot, mag, Md, angles_deg, N, ns):
    """How far the alignment (shift, rotation_deg, magnification) is from undoing the distortion Md, in pixels at the image border.
    The aligned series is X(Md M x) with M the alignment's maps: E = Md M would be the identity.  Its shift, rotation and magnification
    are taken modulo what no projection matching can see or this driver removes: for dr the span of cos(theta), sin(theta), for ds,
    the rotation and the log-magnification a constant.  -> RMS shift residual + N/2 (RMS rotation residual in radians + RMS
    log-magnification residual)"""
    import ref64_align as RA
    e, er, em = decode(chain(Md, RF.matrices(shift, rot, mag, N, ns)), N, ns)
    rr, rs = RA.gauge_residual(e, np.zeros_like(e), angles_deg)
    er, el = np.deg2rad(er - er.mean()), np.log(em) - np.log(em).mean()
    return float(np.sqrt(np.mean(rr ** 2 + rs ** 2)) + 0.5 * N * (np.sqrt(np.mean(er ** 2)) + np.sqrt(np.mean(el ** 2))))


def driver_replay(angles_deg, X, nouter, loo_iters, max_iter=20, margin=2):
    """the passes of ``refine_alignment_affine(leave_one_out=True)``: the oracle's leave-one-out model of the current series, the
    binary64 loop from the current totals against the series as given, the three gauges, the series as given resampled once by the
    binary64 statement of ``tomo_sino_affine`` (shifts rounded to binary32 as ``_align_resample`` does).  -> [(shift, rot, mag)] per pass"""
    import oracle
    import ref64_align as RA
    X = np.asarray(X, np.float32)
    P, N, ns = X.shape
    o = oracle.ctvlib(ns, N, P)
    o.load_A(oracle.parallel_ray(N, angles_deg))
    shift, rot, mag = np.zeros((P, 2)), np.zeros(P), np.ones(P)
    cur, hist = X, []
    for _ in range(nouter):
        model = RA._model(o, cur, N, loo_iters, True)
        M, _ = gauss_newton(model, X, RF.matrices(shift, rot, mag, N, ns), max_iter=max_iter, margin=margin)
        d, r2, m2 = decode(M, N, ns)
        d[:, 1] -= d[:, 1].mean()
        drot, dlog = r2 - rot, np.log(m2) - np.log(mag)
        shift, rot, mag = d, rot + (drot - drot.mean()), mag * np.exp(dlog - dlog.mean())
        cur = RF.affine(X, RF.matrices(shift.astype(np.float32).astype(np.float64), rot, mag, N, ns))[0].astype(np.float32)
        hist.append((shift.copy(), rot.copy(), mag.copy()))
    return hist


def recovery_error(M, truth, N, ns):
    """(worst shift error in pixels, worst rotation error in degrees, worst magnification error) over the projections"""
    d, rot, mag = decode(M, N, ns)
    return float(np.max(np.abs(d - truth[0]))), float(np.max(np.abs(rot - truth[1]))), float(np.max(np.abs(mag - truth[2])))
