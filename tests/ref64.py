"""Binary64 reference of the projectors, SIRT / SART steps and the TV / FGP steps, with per-element error bounds.

numpy only (GPU tests import it).  The matrix is the engine's own (``tomo_tv_amd.engine.system_matrix``, float32 weights); every
product of a float32 weight and a float32 value is exact in binary64, so the references below are the exact results up to one
binary64 rounding per addition -- far below anything a float32 kernel can reach.

Bounds (u = 2^-24, gamma_m = m u / (1 - m u)):

* FP / BP, worst case.  ``|y - y64| <= gamma_m (|A||x|)_i`` per element, m = the entry count of that row (column) plus
  ``EXTRA_SUMS``, a safe upper limit for what a form adds on top of the entry sums (partial sums over strips / tiles, the
  epilogue).  This holds for ANY summation order and any FMA use, so it cannot flake: a kernel outside it dropped, doubled,
  moved or mis-weighted an entry.
* FP / BP, typical case.  The RMS of ``|y - y64| / (u (|A||x|)_i)`` over the elements with ``(|A||x|)_i > 0`` must be at most
  twice the float32 oracle's on the same input (``TYPICAL_FLOOR`` keeps the comparison meaningful where the oracle is
  nearly exact): a systematically worse accumulation fails it.
* SIRT-type step (``tomo_sirt``, Landweber, Cimmino): ``x + cw A^T (rw (b - A x))``, clamped at 0.  The FP bound is carried
  through the residual, the row weights rw, the BP and the column weights cw to first order (each float32 multiplication,
  division and weight sum costs its own gamma), times ``SAFETY`` for the second-order terms.  The clamp is 1-Lipschitz, so the
  clamped values obey the same bound as the values before it.
* SART sweep, ``tv_gd``, FGP.  Sequential: no cheap a-priori bound.  The float32 oracle's own error is the yardstick:
  ``|hip - f64| <= 4 max_slice |oracle - f64| + 8 u |f64|`` per element (``seq_bound``).
"""
import numpy as np

U = 2.0 ** -24
EXTRA_SUMS = 16          # partial sums and epilogue operations a form may add to a row's / column's entry sums
TYPICAL_FLOOR = 0.25     # in units of u (|A||x|)_i: the RMS a kernel may always have
SAFETY = 1.5             # first-order propagation of the SIRT-type bound: room for the second-order terms


def gamma(m):
    m = np.asarray(m, np.float64)
    return m * U / (1.0 - m * U)


class Matrix:
    """The engine's system matrix for ``N`` rays and the tilt angles (degrees) in the order given, in binary64.

    ``rows`` / ``cols`` index the sinogram row ``angle * N + ray`` and the pixel ``y * N + z``."""

    def __init__(self, N, angles_deg, A=None):
        if A is None:
            from tomo_tv_amd.engine import system_matrix
            A = system_matrix(N, np.asarray(angles_deg, np.float64))
        self.N, self.P = int(N), int(np.size(angles_deg))
        self.nrow, self.ncol = self.N * self.P, self.N * self.N
        self.rows = A[0].astype(np.int64)
        self.cols = A[1].astype(np.int64)
        self.w32 = np.ascontiguousarray(A[2], np.float32)
        self.vals = self.w32.astype(np.float64)
        key = self.rows * self.ncol + self.cols
        # row-major (CSR) and column-major (CSC) orders of the entries (the builder emits them row-major already: no sort then)
        order = np.arange(key.size) if np.all(key[1:] >= key[:-1]) else np.argsort(key, kind="stable")
        k = key[order]
        self.duplicates = int(np.count_nonzero(k[1:] == k[:-1]))
        self._r = self._layout(order, self.rows[order], self.nrow)
        ordc = order[np.argsort(self.cols[order], kind="stable")]
        self._c = self._layout(ordc, self.cols[ordc], self.ncol)
        self._csr = None
        self.row_nnz = self._r[2]
        self.col_nnz = self._c[2]
        self.rowsum = np.bincount(self.rows, self.vals, self.nrow)
        self.colsum = np.bincount(self.cols, self.vals, self.ncol)
        self.rowinner = np.bincount(self.rows, self.vals * self.vals, self.nrow)

    @staticmethod
    def _layout(order, keys_sorted, n):
        cnt = np.bincount(keys_sorted, minlength=n)
        ptr = np.zeros(n + 1, np.int64)
        np.cumsum(cnt, out=ptr[1:])
        return order, ptr, cnt

    def csr(self):
        """(ptr, idx, val): the matrix in the oracle's CSR layout (``oracle.CSR``), built once."""
        if self._csr is None:
            o, p, _ = self._r
            self._csr = (p.astype(np.int64), np.ascontiguousarray(self.cols[o], np.int32), np.ascontiguousarray(self.w32[o]))
        return self._csr

    # ---- the entries of one row / column --------------------------------------------------------------------------------------
    def row(self, i):
        """(pixels, float32 weights) of sinogram row i."""
        o, p, _ = self._r
        e = o[p[i]:p[i + 1]]
        return self.cols[e], self.w32[e]

    def column(self, j):
        """(sinogram rows, float32 weights) of pixel j."""
        o, p, _ = self._c
        e = o[p[j]:p[j + 1]]
        return self.rows[e], self.w32[e]

    def dense_column_f32(self, j):
        """Column j as a float32 sinogram row: the value of a one-hot forward projection.  Duplicate (row, col) entries are
        summed in float32 in entry order (the engine never holds any for its own matrices: ``duplicates`` says so)."""
        out = np.zeros(self.nrow, np.float32)
        r, w = self.column(j)
        if not self.duplicates:
            out[r] = w
            return out
        for rr, ww in zip(r, w):
            out[rr] = np.float32(out[rr] + ww)
        return out

    def dense_row_f32(self, i):
        out = np.zeros(self.ncol, np.float32)
        c, w = self.row(i)
        if not self.duplicates:
            out[c] = w
            return out
        for cc, ww in zip(c, w):
            out[cc] = np.float32(out[cc] + ww)
        return out

    # ---- A x and A^T r in binary64, slice by slice (memory bounded at N = 512) -------------------------------------------------
    def _apply(self, v, src, dst, nout, absolute):
        v = np.asarray(v, np.float64).reshape(len(v), -1)
        w = np.abs(self.vals) if absolute else self.vals
        out = np.empty((len(v), nout))
        for s in range(len(v)):
            vs = np.abs(v[s]) if absolute else v[s]
            out[s] = np.bincount(dst, w * vs[src], nout)
        return out

    def fp(self, x, absolute=False):
        """A x per slice: (nslice, N, N) -> (nslice, P N); ``absolute``: |A||x|."""
        return self._apply(x, self.cols, self.rows, self.nrow, absolute)

    def bp(self, r, absolute=False):
        """A^T r per slice: (nslice, P N) -> (nslice, N, N); ``absolute``: |A|^T|r|."""
        return self._apply(r, self.rows, self.cols, self.ncol, absolute).reshape(len(r), self.N, self.N)

    # ---- bounds ----------------------------------------------------------------------------------------------------------------
    def fp_bound(self, x):
        """(A x in binary64, the worst-case bound per element, |A||x|)."""
        ax = self.fp(x, absolute=True)
        return self.fp(x), gamma(self.row_nnz + EXTRA_SUMS)[None, :] * ax, ax

    def bp_bound(self, r):
        ar = self.bp(r, absolute=True)
        g = gamma(self.col_nnz + EXTRA_SUMS).reshape(self.N, self.N)
        return self.bp(r), g[None] * ar, ar

    # ---- SIRT-type steps ---------------------------------------------------------------------------------------------------------
    def sirt_step(self, x, b, rw, cw, wrel_r=0.0, wrel_c=0.0):
        """One step ``max(0, x + cw A^T (rw (b - A x)))`` in binary64 with its first-order worst-case bound.

        rw (per row) and cw (per pixel, or a scalar) in binary64; ``wrel_r`` / ``wrel_c``: the relative error of the float32
        weights the kernel holds in their place (a sum of m entries: gamma_m; each rounding: u)."""
        x = np.asarray(x, np.float64)
        nx = len(x)
        b = np.asarray(b, np.float64).reshape(nx, self.nrow)
        cw = np.broadcast_to(np.asarray(cw, np.float64), (self.ncol,)).reshape(self.N, self.N)
        y, ey, _ = self.fp_bound(x)
        res = b - y
        t = rw[None] * res
        et = np.abs(rw)[None] * (ey + U * np.abs(res)) + np.abs(t) * (wrel_r + 2 * U)
        s = self.bp(t)
        es = self.bp(et, absolute=True) + gamma(self.col_nnz + EXTRA_SUMS).reshape(self.N, self.N)[None] * self.bp(t, absolute=True)
        upd = cw[None] * s
        eu = np.abs(cw)[None] * es + np.abs(upd) * (wrel_c + 2 * U)
        new = x + upd
        bound = SAFETY * (eu + U * np.abs(new))
        return np.maximum(new, 0.0), bound

    def tomo_sirt_step(self, x, b):
        """``tomo_sirt``: R = 1/(A 1), C = 1/(A^T 1), 1/0 := 0."""
        rw = np.where(self.rowsum > 0, 1.0 / np.where(self.rowsum > 0, self.rowsum, 1), 0.0)
        cw = np.where(self.colsum > 0, 1.0 / np.where(self.colsum > 0, self.colsum, 1), 0.0)
        return self.sirt_step(x, b, rw, cw, gamma(self.row_nnz + 2), gamma(self.col_nnz + 2)[None].reshape(self.N, self.N))

    def landweber_step(self, x, b, beta):
        return self.sirt_step(x, b, np.ones(self.nrow), float(np.float32(beta)), 0.0, U)

    def cimmino_step(self, x, b, beta):
        """ctvlib SIRT after ``cimminos_method``: x += A^T M (b - A x) beta / Nrow, M = diag(|A_i|^2) (as the reference writes it)."""
        cw = float(np.float32(np.float32(beta) / np.float32(self.nrow)))
        return self.sirt_step(x, b, self.rowinner, cw, gamma(self.row_nnz + 2), 2 * U)

    # ---- SART sweep ---------------------------------------------------------------------------------------------------------------
    def sart(self, x, b, beta, order=None, nsweep=1):
        """SART sweeps in binary64 with the formula of ``orc_sart``: per angle i (in ``order``), r_j = (b_j - A_j x) / (A_j 1) over its
        rays (0 where A_j 1 = 0), x_p = max(0, x_p + beta (sum_j A_jp r_j) / (sum_j A_jp)) (unchanged where the denominator is 0)."""
        x = np.array(x, np.float64).reshape(len(x), self.ncol)
        b = np.asarray(b, np.float64).reshape(len(x), self.nrow)
        order = np.arange(self.P) if order is None else np.asarray(order)
        beta = float(np.float32(beta))
        for _ in range(nsweep):
            for i in order:
                o, p, _ = self._r                     # the angle's entries: rows i N .. (i + 1) N - 1
                sel = o[p[i * self.N]:p[(i + 1) * self.N]]
                r, c, w = self.rows[sel] - i * self.N, self.cols[sel], self.vals[sel]
                rs = np.bincount(r, w, self.N)
                den = np.bincount(c, w, self.ncol)
                for s in range(len(x)):
                    dot = np.bincount(r, w * x[s, c], self.N)
                    res = np.where(rs > 0, (b[s, i * self.N:(i + 1) * self.N] - dot) / np.where(rs > 0, rs, 1), 0.0)
                    num = np.bincount(c, w * res[r], self.ncol)
                    upd = np.where(den > 0, num / np.where(den > 0, den, 1), 0.0)
                    x[s] = np.maximum(x[s] + beta * upd, 0.0)
        return x.reshape(len(x), self.N, self.N)


    def art(self, x, b, beta):
        """One Kaczmarz sweep over the rows in natural order in binary64 (the formula of ``orc_art``): x += beta a_j (b_j - a_j x) /
        |a_j|^2 for rows with |a_j|^2 > 0, then the clamp at 0."""
        x = np.array(x, np.float64).reshape(len(x), self.ncol)
        b = np.asarray(b, np.float64).reshape(len(x), self.nrow)
        beta = float(np.float32(beta))
        o, p, _ = self._r
        for j in range(self.nrow):
            if not self.rowinner[j] > 0:
                continue
            e = o[p[j]:p[j + 1]]
            c, w = self.cols[e], self.vals[e]
            a = (b[:, j] - x[:, c] @ w) / self.rowinner[j]
            x[:, c] += beta * a[:, None] * w[None, :]
        return np.maximum(x, 0.0).reshape(len(x), self.N, self.N)


# ---- TV steps (volume (nx, ny, nz), axis 0 = the slice axis) ------------------------------------------------------------------------
def _face(ax, i):
    idx = [slice(None)] * 3
    idx[ax] = i
    return tuple(idx)


def _shift(a, axis, d, wrong_face=None):
    """a at index i + d (d = +-1) along ``axis``, periodic.  ``wrong_face = (axis, "lo" | "hi")``: on that ONE face the edge value is
    repeated instead of wrapped (tests: a stencil with a wrong boundary rule on one face)."""
    s = np.roll(a, -d, axis)
    if wrong_face == (axis, "hi") and d > 0:
        s[_face(axis, -1)] = a[_face(axis, -1)]
    if wrong_face == (axis, "lo") and d < 0:
        s[_face(axis, 0)] = a[_face(axis, 0)]
    return s


def tv_gd(x, ng, dPOCS, eps, wrong_face=None):
    """``ng`` steps x -= dPOCS g / ||g|| of the TV gradient of ctvlib.cpp:431-447 (periodic in all three axes), then the clamp at
    0 -- in binary64 (the formula of ``orc_tv_gd_f64``).  ``wrong_face``: see ``_shift``."""
    v = np.array(x, np.float64)

    def S(a, ax, d):
        return _shift(a, ax, d, wrong_face)

    def D(c, a1, a2, a3):
        return np.sqrt(eps + (c - a1) ** 2 + (c - a2) ** 2 + (c - a3) ** 2)
    for _ in range(int(ng)):
        c = v
        xp, yp, zp = S(v, 0, 1), S(v, 1, 1), S(v, 2, 1)
        xm, ym, zm = S(v, 0, -1), S(v, 1, -1), S(v, 2, -1)
        g = (3 * c - xp - yp - zp) / D(c, xp, yp, zp)
        g += (c - xm) / D(xm, c, S(xm, 1, 1), S(xm, 2, 1))
        g += (c - ym) / D(ym, S(ym, 0, 1), c, S(ym, 2, 1))
        g += (c - zm) / D(zm, S(zm, 0, 1), S(zm, 1, 1), c)
        v = v - (float(dPOCS) / np.sqrt(np.sum(g * g))) * g
    return np.maximum(v, 0.0)


def tv_fgp(x, iters, lam, wrong_face=None):
    """FGP-TV prox (isotropic, nonnegative) in binary64: a port of ``orc_tv_fgp`` (tv_fgp.cu:192-281): zero outside the volume.
    ``wrong_face = (axis, "lo" | "hi")``: a different rule on that ONE face (tests): "lo" repeats P's edge value where the kernel
    reads 0 (a wrap would read P's last plane, which is always 0), "hi" wraps the difference of D around."""
    f = np.asarray(x, np.float64)
    lam = float(np.float32(lam))
    mult = 1.0 / (26.0 * lam)
    P = [np.zeros_like(f) for _ in range(3)]
    D = np.zeros_like(f)

    def back(a, ax):                              # a[i - 1], 0 at i = 0
        s = np.roll(a, 1, ax)
        s[_face(ax, 0)] = a[_face(ax, 0)] if wrong_face == (ax, "lo") else 0
        return s

    def fwd_diff(a, ax):                          # a[i] - a[i + 1], 0 at the last i
        d = a - np.roll(a, -1, ax)
        if wrong_face != (ax, "hi"):
            d[_face(ax, -1)] = 0
        return d
    for _ in range(int(iters)):
        D = np.maximum(f - lam * (P[0] + P[1] + P[2] - back(P[0], 0) - back(P[1], 1) - back(P[2], 2)), 0.0)
        Q = [P[a] + mult * fwd_diff(D, a) for a in range(3)]
        den = Q[0] ** 2 + Q[1] ** 2 + Q[2] ** 2
        sc = np.where(den > 1.0, 1.0 / np.sqrt(np.where(den > 1.0, den, 1.0)), 1.0)
        P = [q * sc for q in Q]
    return D if iters > 0 else np.zeros_like(f)


# ---- checks -------------------------------------------------------------------------------------------------------------------------
def _where(mask, shape, k=5):
    idx = np.argwhere(mask.reshape(shape))
    return [tuple(int(t) for t in i) for i in idx[:k]]


def assert_within(name, got, ref, bound):
    """Every element: |got - ref| <= bound (an AssertionError names the first offenders)."""
    got = np.asarray(got, np.float64)
    ref = np.asarray(ref, np.float64).reshape(got.shape)
    bound = np.broadcast_to(bound, got.shape)
    err = np.abs(got - ref)
    bad = ~(err <= bound)
    if bad.any():
        k = np.argmax(np.where(bad, err - bound, -np.inf))
        raise AssertionError(f"{name}: {int(bad.sum())} of {got.size} elements outside the bound, first at {_where(bad, got.shape)}; "
                             f"worst {np.unravel_index(k, got.shape)}: got {got.flat[k]!r}, f64 {ref.flat[k]!r}, bound {bound.flat[k]!r}")


def typical_ratio(got, ref, scale):
    """RMS of |got - ref| / (u scale) over the elements with scale > 0."""
    got = np.asarray(got, np.float64).ravel()
    ref = np.asarray(ref, np.float64).ravel()
    scale = np.asarray(scale, np.float64).ravel()
    m = scale > 0
    if not m.any():
        return 0.0
    return float(np.sqrt(np.mean(((got[m] - ref[m]) / (U * scale[m])) ** 2)))


def assert_typical(name, got, oracle_out, ref, scale):
    """RMS error of ``got`` (in units of u (|A||x|)_i) at most twice the oracle's on the same input (or ``TYPICAL_FLOOR``)."""
    g, o = typical_ratio(got, ref, scale), typical_ratio(oracle_out, ref, scale)
    if not g <= max(2.0 * o, TYPICAL_FLOOR):
        raise AssertionError(f"{name}: RMS error {g:.3f} u |A||x| against the oracle's {o:.3f}")


def seq_bound(oracle_out, ref):
    """The yardstick of the sequential operations: 4 max_slice |oracle - f64| + 8 u |f64| (slices along axis 0)."""
    o = np.asarray(oracle_out, np.float64)
    ref = np.asarray(ref, np.float64).reshape(o.shape)
    per = np.abs(o - ref).reshape(len(o), -1).max(axis=1)
    return 4.0 * per.reshape((-1,) + (1,) * (o.ndim - 1)) + 8 * U * np.abs(ref)


def assert_seq(name, got, oracle_out, ref):
    assert_within(name, got, ref, seq_bound(oracle_out, ref))


def dense_volume(nx, n, seed=0):
    """Values in [0.5, 1.5] with a different offset per slice: every face, border voxel and slice non-zero."""
    rng = np.random.default_rng(seed)
    off = (np.arange(nx) % 7) * 0.05 - 0.15
    return (rng.uniform(0.65, 1.35, (nx, n, n)) + off[:, None, None]).astype(np.float32)


def signed_sino(nx, nrow, seed=0):
    """Signed sinogram rows with a different offset per slice."""
    rng = np.random.default_rng(seed)
    off = (np.arange(nx) % 5) * 0.1 - 0.2
    return (rng.uniform(-1.0, 1.0, (nx, nrow)) + off[:, None]).astype(np.float32)
