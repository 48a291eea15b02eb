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
* FP epilogues (``Matrix.residual``, ``data_distance``, ``poisson``), the scalar reductions (``sqdiff``, ``l1``, ``tv_value``,
  ``tv_gnorm``), the fusion steps (``mm_model``, ``mm_update``) and the host's Lipschitz constants: first-order worst-case bounds,
  stated with each function.  Those built on device transcendentals use ``LOGF_ULP``, ``C_EXP`` and ``C_LOG``, which are
  assumptions about the device's logf / exp2f / log2f, not measurements.  ``proj_max`` / ``proj_scale`` are exact.
* CGLS (``tomo_cgls``: per-slice alpha and beta).  One step from a zero volume has an a-priori first-order bound
  (``Matrix.cgls_first_step``: there r = b exactly and the chain is BP, two slice sums, a ratio and one axpy); several steps are
  sequential (``Matrix.cgls`` against ``cgls_f32`` under ``seq_bound``).  ``cgls_sino`` builds a sinogram whose per-slice alpha
  differ between neighbouring slices by far more than their bound (``alpha_separation``): a coefficient read from the wrong
  slice cannot hide.
* The WBP row filter (``filter_rows``): ``gamma(N + 1) sum_k |h| |in|`` per element, any order, any FMA use.
* The FISTA passes.  ``soft_threshold`` is the exact float32 result; ``momentum`` / ``sino_extrapolate`` (y = r + beta (r - old))
  carry one rounding each for the difference, the product and the sum (the last two one rounding under FMA contraction).
"""
import numpy as np

U = 2.0 ** -24
EXTRA_SUMS = 16          # partial sums and epilogue operations a form may add to a row's / column's entry sums
TYPICAL_FLOOR = 0.25     # in units of u (|A||x|)_i: the RMS a kernel may always have
SAFETY = 1.5             # first-order propagation of the SIRT-type bound: room for the second-order terms
EPS_POISSON = float(np.float32(0.1))   # the float32 eps of the Poisson epilogue ((a - b)/(a + eps), log(a + eps))
# Accuracy ASSUMED of the device's float32 transcendentals, in units of u of the result (not measured here: the GPU tests confirm
# that the kernels stay inside the bounds built on them, and print the worst ratio of error to bound they saw).
LOGF_ULP = 2.0           # logf
C_EXP = 2.0              # exp2f
C_LOG = 2.0              # log2f
TINY = 2.0 ** -149       # absolute floor of a result that may be subnormal (or flushed to 0)


def DSUM(n):
    """Relative error of a sum of n non-negative binary64 terms in any order (the double accumulations of the reductions)."""
    return n * 2.0 ** -53 * 1.01


def POW_REL(t):
    """Relative error of exp2f(t') for t' = g * log2f(x) = t (1 + (1 + C_LOG) u): (C_EXP + ln2 (1 + C_LOG) |t|) u."""
    return (C_EXP + np.log(2.0) * (1.0 + C_LOG) * np.abs(t)) * U


def gamma(m):
    m = np.asarray(m, np.float64)
    return m * U / (1.0 - m * U)


class Matrix:
    """The engine's system matrix for ``N`` rays and the tilt angles (degrees) in the order given, in binary64.

    ``rows`` / ``cols`` index the sinogram row ``angle * N + ray`` and the pixel ``y * N + z``.

    ``A=``: float32 (3, nnz) triplets in place of the engine's own matrix.  They must be CANONICAL -- no (row, col) twice (every
    sum below would count both assignments, where the engine and the oracle keep the last one); explicit zero weights and rows in
    any order are fine.  ``tests/user_matrices.py: canonical()`` makes any triplet list so; ``duplicates`` counts what is left."""

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

    # ---- FP epilogues (k_fp_rows, k_fp_rows_g, k_fp_tile_reduce, k_sino_resid) -------------------------------------------------------
    def residual(self, x, b, mode):
        """The residual epilogues, with their bounds (e = the FP bound of A x, d = b - A x):

        * "resid"  ``b - A x``: ``e (1 + u) + u |d|`` (one rounding of the difference).
        * "norm"   ``(b - A x) / rowsum``, 0 where rowsum = 0 (exactly): ``(e + u |d|) / rowsum + |r| (gamma(row_nnz + 2) + 2u)``
          (the float32 row sum the kernel divides by, and the division).
        * "mul"    ``(b - A x) * rowinner`` (Cimmino): ``(e + u |d|) rowinner + |r| (gamma(row_nnz + 2) + 2u)``."""
        x = np.asarray(x, np.float64)
        b = np.asarray(b, np.float64).reshape(len(x), self.nrow)
        y, ey, _ = self.fp_bound(x)
        d = b - y
        ed = ey * (1 + U) + U * np.abs(d)
        if mode == "resid":
            return d, ed
        wrel = gamma(self.row_nnz + 2)[None] + 2 * U
        if mode == "norm":
            ok = self.rowsum > 0
            rw = np.where(ok, 1.0 / np.where(ok, self.rowsum, 1), 0.0)[None]
        elif mode == "mul":
            rw = self.rowinner[None]
        else:
            raise ValueError(mode)
        r = d * rw
        return r, ed * rw + np.abs(r) * wrel

    def data_distance(self, x, b, yb=None):
        """FP_DD: (G = A x, its FP bound, S_DD = sum (A x - b)^2, its bound).  Per term d = fl(acc - b) (error e = e_fp + u |d|), a
        float32 square, a double sum: ``sum(2 |d| e + e^2 + 3u d^2)`` plus the double summation.  ``yb``: as for ``poisson``."""
        y, ey = yb if yb is not None else self.fp_bound(x)[:2]
        b = np.asarray(b, np.float64).reshape(y.shape)
        d = y - b
        e = ey * (1 + U) + U * np.abs(d)
        s = float(np.sum(d * d))
        return y, ey, s, float(np.sum(2 * np.abs(d) * e + e * e + 3 * U * d * d)) + DSUM(d.size) * s

    def poisson(self, x, b, yb=None):
        """FP_POISSON (multimodal.cpp:284-292; eps = ``EPS_POISSON``, b >= 0, A x > -eps):

        * residual ``(a - b)/(a + eps)``: the FP error e_a times ``|d/da| = |eps + b|/(a + eps)^2``, plus three roundings
          (difference, sum, quotient), times ``SAFETY``;
        * cost ``sum(a - b log(a + eps))``: per term ``|1 - b/(a + eps)| e_a + |b log(a + eps)| LOGF_ULP u + u |b|`` (the rounded
          a + eps) ``+ u (|a| + |b log|)`` (product and difference), times ``SAFETY``, plus the double summation.

        Returns (residual, its bound, cost, its bound).  ``yb = (A x, its FP bound)`` in place of x: a projection already in hand."""
        a, ea = yb if yb is not None else self.fp_bound(x)[:2]
        b = np.asarray(b, np.float64).reshape(a.shape)
        den = a + EPS_POISSON
        r = (a - b) / den
        er = SAFETY * (ea * np.abs(EPS_POISSON + b) / den ** 2 + 3 * U * np.abs(r))
        lg = b * np.log(den)
        cost = float(np.sum(a - lg))
        ec = SAFETY * (np.abs(1 - b / den) * ea + np.abs(lg) * LOGF_ULP * U + U * np.abs(b) + U * (np.abs(a) + np.abs(lg)))
        return r, er, cost, float(np.sum(ec)) + DSUM(a.size) * float(np.sum(np.abs(a) + np.abs(lg)))

    # ---- the host's Lipschitz constants (sysmat.cpp) --------------------------------------------------------------------------------
    def lipschitz(self, cimmino=False):
        """``max_p (A^T A 1)_p`` (or ``max_p (A^T M A 1)_p``, M = diag(|A_i|^2)) in binary64 and a bound of the float32 host value:
        every term is positive, each a product of float32 row sums (gamma(row_nnz)) and weights summed over a column, so
        ``gamma(max row_nnz + col_nnz + 4)`` relative (``+ max row_nnz`` more for M)."""
        t = self.rowsum * (self.rowinner if cimmino else 1.0)
        v = np.bincount(self.cols, self.vals * t[self.rows], self.ncol)
        p = int(np.argmax(v))
        m = int(self.row_nnz.max()) * (2 if cimmino else 1) + int(self.col_nnz.max()) + 4
        return float(v[p]), float(gamma(m) * v[p])

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


    def art(self, x, b, beta, order=None):
        """One Kaczmarz sweep over the rows in natural order (or in ``order``, a sequence of row numbers) in binary64 (the formula of
        ``orc_art``): x += beta a_j (b_j - a_j x) / |a_j|^2 for rows with |a_j|^2 > 0, then the clamp at 0."""
        x = np.array(x, np.float64).reshape(len(x), self.ncol)
        b = np.asarray(b, np.float64).reshape(len(x), self.nrow)
        beta = float(np.float32(beta))
        o, p, _ = self._r
        for j in (range(self.nrow) if order is None else np.asarray(order, np.int64)):
            if not self.rowinner[j] > 0:
                continue
            e = o[p[j]:p[j + 1]]
            c, w = self.cols[e], self.vals[e]
            a = (b[:, j] - x[:, c] @ w) / self.rowinner[j]
            x[:, c] += beta * a[:, None] * w[None, :]
        return np.maximum(x, 0.0).reshape(len(x), self.N, self.N)

    # ---- CGLS (tomo_cgls: k_slice_sumsq, k_slice_sumsq_finish, k_slice_ratio, k_slice_axpy, k_slice_xpay) ----------------------------
    def cgls(self, x0, b, niter, slices=None):
        """``niter`` textbook CGLS steps per slice in binary64, in the form ``tomo_cgls`` runs: r = b - A x, z = A^T r, p = z,
        gam = |z|^2; per step w = A p, alpha = gam / |w|^2, x += alpha p, r -= alpha w, z = A^T r, beta = |z|^2 / gam, p = z + beta p
        (0/0 := 0); the clamp at 0 at the end.  alpha and beta are rounded to float32, as ``k_slice_ratio`` stores them.  The slices
        are independent: ``slices`` selects the ones to compute (of ``x0`` and ``b`` alike; ``x0 = None``: a zero start).
        Returns (x, alpha, beta), the coefficients as (niter, nslice) arrays."""
        b = np.asarray(b)
        sl = np.arange(len(b)) if slices is None else np.asarray(slices)
        b = b[sl].astype(np.float64).reshape(len(sl), self.nrow)
        x = np.zeros((len(sl), self.N, self.N)) if x0 is None else np.array(np.asarray(x0)[sl], np.float64)

        def quot(num, den):
            return np.where(den > 0, num / np.where(den > 0, den, 1.0), 0.0).astype(np.float32).astype(np.float64)
        r = b - self.fp(x)
        z = self.bp(r)
        p = z.copy()
        gam = np.sum(z * z, axis=(1, 2))
        alphas, betas = np.zeros((niter, len(sl))), np.zeros((niter, len(sl)))
        for it in range(int(niter)):
            w = self.fp(p)
            alpha = quot(gam, np.sum(w * w, axis=1))
            x += alpha[:, None, None] * p
            r -= alpha[:, None] * w
            z = self.bp(r)
            gnew = np.sum(z * z, axis=(1, 2))
            beta = quot(gnew, gam)
            gam = gnew
            p = z + beta[:, None, None] * p
            alphas[it], betas[it] = alpha, beta
        return np.maximum(x, 0.0), alphas, betas

    def cgls_first_step(self, b):
        """One CGLS step from x0 = 0 in binary64 with an a-priori first-order bound per element.  From zero r = b exactly (the
        projection of a zero volume is 0), so the chain is short:

        * z = A^T b under ``bp_bound``: e_z;
        * gam = sum z^2 (float32 squares, a double sum): d_gam = ``sum(2 |z| e_z + e_z^2 + u z^2) + DSUM gam`` (the form of ``tv_gnorm``);
        * w = A z: e_w = ``fp_bound(z)`` (the projector's own sums) + ``|A| e_z`` (it projects the device's z); den = sum w^2 likewise;
        * alpha = gam / den, a double quotient rounded to float32: rel_alpha = d_gam / gam + d_den / den + u;
        * x1 = alpha z (``k_slice_axpy`` onto a zero volume: a product, and a sum with 0): |alpha| e_z + |z| |alpha| rel_alpha +
          2u |alpha z|, times ``SAFETY`` for the second-order terms; the clamp is 1-Lipschitz.

        A slice with gam = 0 or den = 0 has alpha = 0 and x1 = 0 exactly (bound 0).
        Returns (x1, bound, alpha, rel_alpha): the unrounded binary64 alpha per slice and the bound of its relative error."""
        b = np.asarray(b, np.float64).reshape(len(b), self.nrow)
        z, ez, _ = self.bp_bound(b)
        az = np.abs(z)
        gam = np.sum(z * z, axis=(1, 2))
        dgam = np.sum(2 * az * ez + ez * ez + U * z * z, axis=(1, 2)) + DSUM(self.ncol) * gam
        w, ew, _ = self.fp_bound(z)
        ew = ew + self.fp(ez, absolute=True)
        den = np.sum(w * w, axis=1)
        dden = np.sum(2 * np.abs(w) * ew + ew * ew + U * w * w, axis=1) + DSUM(self.nrow) * den
        ok = (gam > 0) & (den > 0)
        alpha = np.where(ok, gam / np.where(ok, den, 1.0), 0.0)
        rel = np.where(ok, dgam / np.where(ok, gam, 1.0) + dden / np.where(ok, den, 1.0) + U, 0.0)
        a3 = alpha[:, None, None]
        x1 = a3 * z
        bound = SAFETY * (a3 * ez + az * a3 * rel[:, None, None] + 2 * U * np.abs(x1))
        return np.maximum(x1, 0.0), bound, alpha, rel


# ---- CGLS in float32, inputs with well separated per-slice coefficients ---------------------------------------------------------------
def cgls_f32(fp, bp, x0, b, niter):
    """The iteration of ``Matrix.cgls`` in float32 with double slice sums: ``fp(volume)`` / ``bp(sinogram)`` are the float32
    oracle's projectors.  The yardstick of ``niter >= 2`` under ``seq_bound``."""
    F = np.float32
    b = np.asarray(b, F)
    x = np.array(x0, F)

    def quot(num, den):
        return np.where(den > 0, num / np.where(den > 0, den, 1.0), 0.0).astype(F)
    r = (b - fp(x)).astype(F)
    z = bp(r)
    p = z.copy()
    gam = np.sum(z.astype(np.float64) ** 2, axis=(1, 2))
    for _ in range(int(niter)):
        w = fp(p)
        alpha = quot(gam, np.sum(w.astype(np.float64) ** 2, axis=1))
        x = (x + alpha[:, None, None] * p).astype(F)
        r = (r - alpha[:, None] * w).astype(F)
        z = bp(r)
        gnew = np.sum(z.astype(np.float64) ** 2, axis=(1, 2))
        beta = quot(gnew, gam)
        gam = gnew
        p = (z + beta[:, None, None] * p).astype(F)
    return np.maximum(x, F(0))


def cgls_zero_slice(nx):
    """The slice ``cgls_sino`` leaves entirely zero: lane 1 of the float4 group in the middle of the slab."""
    return 4 * ((nx // 2) // 4) + 1 if nx > 1 else None


def _cgls_pattern(M, s):
    """A smooth per-ray pattern of slice s (its frequency, phase and drift across the projections differ from slice to slice)."""
    ray = (np.arange(M.nrow) % M.N + 0.5) / M.N
    proj = np.arange(M.nrow) // M.N
    return np.cos(np.pi * (1 + s % 3) * ray + 0.7 * proj + 0.37 * s)


def cgls_sino(M, nx, seed=0, min_sep=0.02):
    """A ``signed_sino`` plus a smooth per-ray pattern that differs per slice, slice ``cgls_zero_slice(nx)`` entirely zero.  The first
    CGLS coefficient from a zero start, alpha_s = |A^T b_s|^2 / |A A^T b_s|^2, is scale-free, so it is the SHAPE of b_s that is
    varied: the pattern's amplitude steps through 13 levels, and where the alpha of a slice still lies within ``min_sep``
    (relative) of an earlier slice of its own or the previous float4 group, more of the pattern is added until it does not
    (chosen on the CPU: ``alpha_separation`` is what the tests then assert)."""
    b = signed_sino(nx, M.nrow, seed).astype(np.float64)
    amp = ((np.arange(nx) * 5) % 13 + 1) * 0.35
    for s in range(nx):
        b[s] += amp[s] * _cgls_pattern(M, s)
    b = b.astype(np.float32)
    zs = cgls_zero_slice(nx)
    if zs is not None:
        b[zs] = 0

    def alpha_of(row):
        z = M.bp(row[None].astype(np.float64))
        w = M.fp(z)
        den = float(np.sum(w * w))
        return float(np.sum(z * z)) / den if den > 0 else 0.0
    alpha = np.zeros(nx)
    for s in range(nx):
        if s == zs:
            continue
        for k in range(1, 60):
            alpha[s] = alpha_of(b[s])
            near = [t for t in range(max(0, 4 * (s // 4 - 1)), s) if t != zs]
            if all(abs(alpha[s] - alpha[t]) > min_sep * max(alpha[s], alpha[t]) for t in near):
                break
            b[s] = (b[s] + np.float32(0.23 * k) * _cgls_pattern(M, s + k)).astype(np.float32)
        else:
            raise AssertionError(f"cgls_sino: slice {s} not separated")
    return b


def alpha_separation(alpha, rel):
    """The smallest ``|alpha_s - alpha_t| / max(alpha_s, alpha_t)`` over ``100 max(rel_s, rel_t)``, over every pair of slices of one
    float4 group or of neighbouring groups (slices with alpha = 0, the zero slice, left out: any other coefficient there shows as a
    non-zero voxel).  Above 1, a coefficient taken from a neighbour moves the step by more than 100 bounds of alpha."""
    alpha, rel = np.asarray(alpha, np.float64), np.asarray(rel, np.float64)
    worst = np.inf
    for s in range(len(alpha)):
        for t in range(max(0, 4 * (s // 4 - 1)), s):
            if alpha[s] > 0 and alpha[t] > 0:
                worst = min(worst, abs(alpha[s] - alpha[t]) / max(alpha[s], alpha[t]) / (100 * max(rel[s], rel[t])))
    return worst


def slice_sample(nx):
    """The slices a large case is compared on: the first and the last real slice, both sides of every 64-slice boundary, and one
    slice in each lane of a float4 group (slices 4k + lane of four different groups), ``cgls_zero_slice`` among them."""
    s = {0, nx - 1} | {c for k in range(64, nx, 64) for c in (k - 1, k)}
    s |= {4 * g + lane for lane, g in enumerate((1, nx // 8 + 1, nx // 5, (nx - 1) // 4 - 1))}
    s.add(cgls_zero_slice(nx))
    return np.array(sorted(t for t in s if t is not None and 0 <= t < nx))


# ---- the WBP row filter (k_filter_rows) -------------------------------------------------------------------------------------------------
def filter_rows(sino, taps, P, N):
    """``out[p, j] = sum_k h[|j - k|] in[p, k]`` per slice and projection in binary64 (h: the float32 taps the device holds), and the
    bound ``gamma(N + 1) sum_k |h[|j - k|]| |in[p, k]|``: N products and N sums in any order, with or without FMA contraction."""
    h = np.asarray(taps, np.float32).astype(np.float64)
    idx = np.abs(np.arange(N)[:, None] - np.arange(N)[None, :])
    H = h[idx]
    s = np.asarray(sino, np.float64).reshape(len(sino), P, N)
    out = np.einsum("jk,spk->spj", H, s)
    mag = np.einsum("jk,spk->spj", np.abs(H), np.abs(s))
    return out.reshape(len(sino), P * N), (float(gamma(N + 1)) * mag).reshape(len(sino), P * N)


# ---- the FISTA passes (k_soft_threshold, k_momentum, k_sino_extrapolate) ----------------------------------------------------------------
def soft_threshold(v, l):
    """``|v| > l ? copysign(|v| - l, v) : +0`` in float32: one exactly rounded subtraction, so the kernel's result bit for bit
    (subnormals kept, -0 and |v| == l give +0)."""
    v = np.asarray(v, np.float32)
    l = np.float32(l)
    a = np.abs(v)
    return np.where(a > l, np.copysign((a - l).astype(np.float32), v), np.float32(0)).astype(np.float32)


def momentum(r, old, beta):
    """``y = r + beta (r - old)`` (k_momentum; beta the float32 value) in binary64 and its bound.  The kernel rounds the difference
    (u |r - old|, carried through beta), then either the product and the sum (u |beta (r - old)| + u |y|) or, contracted to an FMA,
    the sum alone: ``u (2 |beta (r - old)| + |y|)``, times 1.01 for the second-order terms, plus ``2 TINY`` for a difference or
    product that underflows."""
    beta = float(np.float32(beta))
    r, old = np.asarray(r, np.float64), np.asarray(old, np.float64)
    t = beta * (r - old)
    y = r + t
    return y, 1.01 * U * (2 * np.abs(t) + np.abs(y)) + 2 * TINY


def sino_extrapolate(g, p_old, beta):
    """``q = g + beta (g - p_old)`` (k_sino_extrapolate: A yk from A r and A r_old): the expression of ``momentum``, and its bound.
    The kernel's second output, the saved A r, is a copy of g: bit for bit."""
    return momentum(g, p_old, beta)


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


def tv_grad(v, eps, wrong_face=None):
    """The TV gradient of ctvlib.cpp:431-447 (periodic in all three axes) in binary64, and a first-order bound of a float32 kernel's
    error in it per element: every difference, square, sum, sqrtf and division of one of the four quotients n / d rounds once,
    so ``|dn| <= gamma(3) (sum of |differences|)``, ``|dd| <= gamma(5) d`` (eps + three squares, the root) and one division:
    ``|d(n/d)| <= (|dn| + gamma(6) |n|) / d``.  ``wrong_face``: see ``_shift``."""
    v = np.asarray(v, np.float64)

    def S(a, ax, d):
        return _shift(a, ax, d, wrong_face)

    def D(c, a1, a2, a3):
        return np.sqrt(eps + (c - a1) ** 2 + (c - a2) ** 2 + (c - a3) ** 2)
    c = v
    xp, yp, zp = S(v, 0, 1), S(v, 1, 1), S(v, 2, 1)
    xm, ym, zm = S(v, 0, -1), S(v, 1, -1), S(v, 2, -1)
    terms = [((c - xp) + (c - yp) + (c - zp), np.abs(c - xp) + np.abs(c - yp) + np.abs(c - zp), D(c, xp, yp, zp)),
             (c - xm, np.abs(c - xm), D(xm, c, S(xm, 1, 1), S(xm, 2, 1))),
             (c - ym, np.abs(c - ym), D(ym, S(ym, 0, 1), c, S(ym, 2, 1))),
             (c - zm, np.abs(c - zm), D(zm, S(zm, 0, 1), S(zm, 1, 1), c))]
    g = sum(n / d for n, _, d in terms)
    eg = sum((gamma(3) * a + gamma(6) * np.abs(n)) / d for n, a, d in terms) + gamma(4) * sum(np.abs(n) / d for n, _, d in terms)
    return g, eg


def tv_gnorm(x, eps, wrong_face=None):
    """S_GNORM: sum g^2 of the TV gradient of ``x`` (float32 g squared in float32, summed in double), with its bound
    ``sum(2 |g| e_g + e_g^2 + u g^2)`` plus the double summation."""
    g, eg = tv_grad(np.asarray(x, np.float64), float(np.float32(eps)), wrong_face)
    ref = float(np.sum(g * g))
    return ref, float(np.sum(2 * np.abs(g) * eg + eg * eg + U * g * g)) + DSUM(g.size) * ref


def tv_gd(x, ng, dPOCS, eps, wrong_face=None):
    """``ng`` steps x -= dPOCS g / ||g|| of the TV gradient of ctvlib.cpp:431-447 (periodic in all three axes), then the clamp at
    0 -- in binary64 (the formula of ``orc_tv_gd_f64``).  ``wrong_face``: see ``_shift``."""
    v = np.array(x, np.float64)
    for _ in range(int(ng)):
        g, _ = tv_grad(v, eps, wrong_face)
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


# ---- scalar reductions (k_sqdiff, k_l1, k_tv_value and the TV value of the gradient kernels; grid-stride, summed in double) ------
def sqdiff(a, b):
    """S_DIFF / S_RMSE: sum (a - b)^2; per term a float32 difference and a float32 square (3u), then the double summation."""
    d = np.asarray(a, np.float64) - np.asarray(b, np.float64)
    s = float(np.sum(d * d))
    return s, 3 * U * s * 1.01 + DSUM(d.size) * s


def l1(a):
    """S_L1: sum |a|; the terms are exact, only the double summation rounds."""
    s = float(np.sum(np.abs(np.asarray(a, np.float64))))
    return s, DSUM(np.size(a)) * s


def tv_value(x, eps, wrong_face=None):
    """S_TV: sum sqrtf(eps + (c - x_ip)^2 + (c - x_jp)^2 + (c - x_kp)^2), periodic in all three axes (``orc_tv``); eps is the
    float32 value.  Per term: three rounded differences and squares, three additions and the root: ``gamma(6)`` relative; then the
    double summation.  ``wrong_face``: see ``_shift``."""
    v = np.asarray(x, np.float64)
    eps = float(np.float32(eps))
    c = v
    t = np.sqrt(eps + sum((c - _shift(v, ax, 1, wrong_face)) ** 2 for ax in range(3)))
    s = float(np.sum(t))
    return s, float(gamma(6)) * s + DSUM(t.size) * s


# ---- the fusion kernels (k_mm_model / k_mm_update: multimodal.cpp:425-438, 277-304) ------------------------------------------------
def _pow(x, g):
    """x^g in binary64 with the kernel's rules at 0 (0^0 = 1, 0^g = 0 for g > 0, inf for g < 0) and its per-element bound: exact
    at x == 0 and where g == 1; else ``POW_REL(g log2 |x|) |x^g| + TINY``.  x < 0 takes powf (numpy's value: NaN unless g is an
    integer), under the same allowance."""
    x = np.asarray(x, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        p = np.power(x, g)
        p = np.where(x == 0, 1.0 if g == 0 else (0.0 if g > 0 else np.inf), p)
        t = g * np.log2(np.where(x != 0, np.abs(x), 1.0))
    e = np.where(x == 0, 0.0, POW_REL(t) * np.abs(np.where(np.isfinite(p), p, 0)) + TINY)
    return p, e


def mm_model(xs, w, g):
    """``sum_e w_e x_e^g``.  g == 1: the plain float32 sum, ``gamma(nel + 1) sum |w_e x_e|``.  Otherwise each power carries its
    ``_pow`` allowance times |w_e|, plus ``gamma(nel + 1) sum |w_e x_e^g|``.  Returns (model, bound)."""
    g = float(np.float32(g))
    w = np.asarray(w, np.float32).astype(np.float64)
    acc, mag, err = 0.0, 0.0, 0.0
    for e in range(len(xs)):
        p, ep = (np.asarray(xs[e], np.float64), 0.0) if g == 1.0 else _pow(xs[e], g)
        acc = acc + w[e] * p
        mag = mag + np.abs(w[e] * p)
        err = err + np.abs(w[e]) * ep
    with np.errstate(invalid="ignore"):
        return acc, err + gamma(len(xs) + 1) * mag + 2 * len(xs) * TINY     # (products and sums that underflow)


def mm_update(xs, us, w, g, lamC_over_L, lamH, upd=None, model=None):
    """``x_e <- max(0, x_e - (c u_e - lamH g x_e^(g-1) w_e (upd - model)))``, c = lamC_over_L (float32 values), per element e.
    lamH == 0 is poisson_ML (multimodal.cpp:277-304): ``max(0, x_e - c u_e)``, bound ``u |c u_e| + u |x_e - c u_e|``.  Otherwise the
    HAADF term H carries ``(POW_REL + 5u) |H|`` (difference, two products, g *, the power; TINY for a subnormal power) and the rest
    one rounding per operation, times ``SAFETY`` (and 8 ``TINY`` for products that underflow).  At x_e == 0 with g < 1 the power is inf: the engine's value there is +inf where
    w_e (upd - model) > 0 and 0 elsewhere (inf * 0 = NaN, and fmaxf(NaN, 0) = 0); those elements are exact (bound 0).
    Returns a list of (new x_e, bound)."""
    g = float(np.float32(g))
    c, lamH = float(np.float32(lamC_over_L)), float(np.float32(lamH))
    w = np.asarray(w, np.float32).astype(np.float64)
    out = []
    D = None if lamH == 0 else np.asarray(upd, np.float64) - np.asarray(model, np.float64)
    for e in range(len(xs)):
        x, u = np.asarray(xs[e], np.float64), np.asarray(us[e], np.float64)
        A = c * u
        if lamH == 0:
            v = x - A
            bound = U * np.abs(A) + U * np.abs(v) * 1.01 + 2 * TINY
            out.append((np.maximum(v, 0.0), bound))
            continue
        wd = w[e] * D
        if g == 1.0:
            H, eH = lamH * wd, 3 * U * np.abs(lamH * wd)
            special = np.zeros(x.shape, bool)
        else:
            p, ep = _pow(x, g - 1.0)
            special = ~np.isfinite(p)
            with np.errstate(invalid="ignore"):
                H = np.where(special, 0.0, lamH * g * p * wd)
                eH = np.where(special, 0.0, np.abs(H) * 5 * U + lamH * abs(g) * ep * np.abs(wd))
        v = x - (A - H)
        bound = SAFETY * (eH + U * np.abs(A) + U * np.abs(A - H) + U * np.abs(v)) + 8 * TINY
        new = np.maximum(v, 0.0)
        new = np.where(special, np.where(wd > 0, np.inf, 0.0), new)
        out.append((new, np.where(special, 0.0, bound)))
    return out


# ---- per-projection max / scale (k_proj_max, k_proj_scale: multimodal.cpp:312-328) -------------------------------------------------
def proj_max(sino, P, N):
    """Max over the rays and slices of each projection of a (nslice, P N) sinogram: exact (a float32 max)."""
    s = np.asarray(sino, np.float32).reshape(len(sino), P, N)
    return s.max(axis=(0, 2))


def proj_scale(sino, P, N, div, mul):
    """``(b / div_p) * mul_p`` per projection, each operation correctly rounded in float32: exact."""
    s = np.asarray(sino, np.float32).reshape(len(sino), P, N)
    d = np.asarray(div, np.float32)[None, :, None]
    m = np.asarray(mul, np.float32)[None, :, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        return ((s / d).astype(np.float32) * m).astype(np.float32).reshape(len(sino), P * N)


def assert_scalar(name, got, ref, bound):
    """|got - ref| <= bound for one scalar."""
    if not abs(float(got) - float(ref)) <= bound:
        raise AssertionError(f"{name}: got {float(got)!r}, f64 {float(ref)!r}: error {abs(float(got) - float(ref)):.3e} > bound {bound:.3e}")


def ratio(got, ref, bound):
    """The largest |got - ref| / bound over the elements with a bound > 0 (how close a kernel came to its bound)."""
    got = np.asarray(got, np.float64)
    ref = np.asarray(ref, np.float64).reshape(got.shape)
    bound = np.broadcast_to(np.asarray(bound, np.float64), got.shape)
    m = (bound > 0) & np.isfinite(ref)
    return float(np.max(np.abs(got[m] - ref[m]) / bound[m])) if m.any() else 0.0


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


def sentinel_positions(nx, n):
    """(slice, y, z) of the reduction sentinels: the first element, the last real element of the last slice, the first element of the
    second 64-slice chunk (when there is one) and an element in lane 3 of a float4 group (slice 3 of a middle pixel)."""
    pos = [(0, 0, 0), (nx - 1, n - 1, n - 1)]
    if nx > 64:
        pos.append((64, 0, 0))
    if nx > 3:
        pos.append((3, n // 2, n // 3))
    return sorted(set(pos))


def with_sentinels(x, factor=64.0):
    """A copy of volume x with its ``sentinel_positions`` values multiplied by ``factor``: dropping or double-counting any one of them
    moves a reduction far outside its bound."""
    x = np.array(x, np.float32)
    for p in sentinel_positions(*x.shape[:2]):
        x[p] *= np.float32(factor)
    return x
