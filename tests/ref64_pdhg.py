"""Binary64 reference of the Chambolle-Pock iteration (``tomo_pdhg*``) with per-element error bounds; numpy only.

The problem is  min_{x >= 0} 1/2 |Ax - b|^2 + lam |grad x|_{2,1}  on volumes ``x[s][y][z]`` (nx, n, n), the three axes alike:

* ``grad``: ``(grad x)_a[i] = x[i + 1_a] - x[i]`` where ``i_a < n_a - 1``, else 0.
* ``div``: ``(div p)[i] = sum_a p_a[i] - p_a[i - 1_a]`` with ``p_a[-1] = 0``; with ``p_a = 0`` at the last index of axis a,
  ``<grad x, p> = <x, -div p>`` exactly.
* one iteration: ``g = A xbar``; ``q <- (q + S (g - b)) / (1 + S)`` (``sino_dual``); ``u = A^T q``; then ``tv_step``:
  ``a = p + s_grad grad xbar`` (0 where the difference row does not exist), ``p <- a / max(1, |a|_2 / lam)``,
  ``x_new = max(0, x - T (u - div p))``, ``xbar <- x_new + theta (x_new - x)``.
* step sizes.  Scalar: ``S = s_grad = sigma``, ``T = tau``, ``tau = ratio / sqrt(L + 12)``, ``sigma = 1 / (ratio sqrt(L + 12))`` evaluated in
  double and rounded to float32 once (``scalar_steps``), L the engine's float32 Lipschitz constant.  Diagonal (``precond``):
  ``S_i = 1 / rowsum_i`` (0 for an empty ray), ``s_grad = 1/2``, ``T_j = 1 / (colsum_j + d_j)``, ``d_j`` the difference rows that touch
  voxel j.  The row and column sums are DATA of the iteration: the float32 tables the engine uploads (``tables_f32`` rebuilds them:
  float32 sums in ascending column / row order), the same numbers in the binary64 and the float32 replay.

Every function takes ``dtype``: ``np.float64`` is the reference, ``np.float32`` replays the same operations with every one of them
rounded to float32 (FP and BP by the dense float32 matrix); the float32 replay is the yardstick of the sequential loop
(``ref64.seq_bound``), as the oracle is for the sequential tests of ``ref64``.

Bounds of ONE ``sino_dual`` / ``tv_step`` given float32 inputs: first order, worst case.  Each float32 addition, multiplication,
division, square root and reciprocal costs u = 2^-24 of its result (the kernels use the correctly rounded forms: no rsqrt, no
reciprocal approximation, so no assumed ulp constant is needed); a fused multiply-add may replace a multiplication and an addition
(the bound charges both); ``max(1, .)`` and the clamp at 0 are 1-Lipschitz, and so is the Euclidean norm of a; times ``ref64.SAFETY``.
At a branch point (``|a|_2 = lam``, ``x = T (u - div p)``) both branches agree to first order, so the bound covers either side.
"""
import numpy as np

import ref64
from ref64 import SAFETY, U


# ---- operators -----------------------------------------------------------------------------------------------------------------
def grad(x, dtype=np.float64):
    x = np.asarray(x, dtype)
    g = np.zeros((3,) + x.shape, dtype)
    g[0][:-1] = x[1:] - x[:-1]
    g[1][:, :-1] = x[:, 1:] - x[:, :-1]
    g[2][:, :, :-1] = x[:, :, 1:] - x[:, :, :-1]
    return g


def _back(a, ax):
    """a[i - 1_ax], 0 at i_ax = 0."""
    out = np.zeros_like(a)
    dst = [slice(None)] * 3
    src = [slice(None)] * 3
    dst[ax], src[ax] = slice(1, None), slice(None, -1)
    out[tuple(dst)] = a[tuple(src)]
    return out


def div(p, dtype=np.float64):
    p = np.asarray(p, dtype)
    d = [p[a] - _back(p[a], a) for a in range(3)]
    return (d[0] + d[1]) + d[2]


def _mask_last(shape, a):
    """1 where the difference row of axis a exists (i_a < n_a - 1)."""
    m = np.ones(shape, bool)
    sl = [slice(None)] * 3
    sl[a] = slice(-1, None)
    m[tuple(sl)] = False
    return m


def touch_count(nx, n):
    """d_j: the difference rows that touch voxel j (0..6)."""
    d = np.zeros((nx, n, n))
    for a, m in enumerate((nx, n, n)):
        i = np.arange(m).reshape([-1 if k == a else 1 for k in range(3)])
        d = d + (i > 0) + (i < m - 1)
    return d


def tables_f32(M):
    """(rowsum, colsum) as the engine builds them: float32 sums of the float32 weights, rows in ascending column order, columns in
    ascending row order (sequential, one rounding per addition)."""
    if getattr(M, "_pdhg_tables", None) is None:
        out = []
        for order, ptr, cnt in (M._r, M._c):
            s = np.zeros(len(cnt), np.float32)
            for k in range(int(cnt.max()) if len(cnt) else 0):
                live = np.nonzero(cnt > k)[0]
                s[live] = s[live] + M.w32[order[ptr[live] + k]]
            out.append(s)
        M._pdhg_tables = tuple(out)
    return M._pdhg_tables


def scalar_steps(L, ratio=1.0):
    """(sigma, tau) of the scalar mode as float32: tau sigma (L + 12) = 1 up to rounding."""
    s, r = np.sqrt(float(np.float32(L)) + 12.0), float(np.float32(ratio))
    return np.float32(1.0 / (r * s)), np.float32(r / s)


def primal_T(colsum, nx, n, dtype=np.float64):
    """T_j = 1 / (colsum_pixel(j) + d_j) of the diagonal mode (0 where the denominator is 0)."""
    den = np.asarray(colsum, dtype).reshape(1, n, n) + touch_count(nx, n).astype(dtype)
    with np.errstate(divide="ignore"):
        return np.where(den > 0, dtype(1) / den, dtype(0)).astype(dtype)


def dual_S(rowsum, dtype=np.float64):
    rs = np.asarray(rowsum, dtype)
    with np.errstate(divide="ignore"):
        return np.where(rs > 0, dtype(1) / rs, dtype(0)).astype(dtype)


# ---- the two steps -------------------------------------------------------------------------------------------------------------
def sino_dual(q, g, b, S, dtype=np.float64):
    """q <- (q + S (g - b)) / (1 + S); S a scalar or one value per sinogram row."""
    q, g, b = (np.asarray(v, dtype) for v in (q, g, b))
    S = np.asarray(S, dtype)
    if S.ndim:
        S = S.reshape(1, -1)
    return ((q + S * (g - b)) / (dtype(1) + S)).astype(dtype)


def dual_field(xbar, p, s_grad, lam, dtype=np.float64):
    """(p_new, a): p_new = a / max(1, |a|_2 / lam)."""
    g = grad(xbar, dtype)
    p = np.asarray(p, dtype)
    a = np.zeros_like(g)
    for k in range(3):
        a[k] = np.where(_mask_last(g[k].shape, k), dtype(s_grad) * g[k] + p[k], dtype(0))
    nn = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]
    inv = dtype(1) / np.maximum(dtype(1), np.sqrt(nn) / dtype(lam))
    return (a * inv[None]).astype(dtype), a


def tv_step(x, xbar, u, p, s_grad, T, lam, theta=1.0, dtype=np.float64):
    """(x_new, xbar_new, p_new); T a scalar or an (nx, n, n) array."""
    x, u = np.asarray(x, dtype), np.asarray(u, dtype)
    pn, _ = dual_field(xbar, p, s_grad, lam, dtype)
    xn = np.maximum(x - np.asarray(T, dtype) * (u - div(pn, dtype)), dtype(0)).astype(dtype)
    xb = (xn + dtype(theta) * (xn - x)).astype(dtype)
    return xn, xb, pn


def sino_dual_bound(q, g, b, S=None, rowsum=None):
    """(binary64 result, bound) of one float32 ``sino_dual`` on float32 inputs; ``rowsum`` given: S = 1 / rowsum is formed in float32."""
    q, g, b = (np.asarray(v, np.float64) for v in (q, g, b))
    if rowsum is not None:
        S = dual_S(rowsum).reshape(1, -1)
        eS = U * S                                                  # the reciprocal
    else:
        S = np.float64(S)
        eS = 0.0
    d = g - b
    t = q + S * d
    den = 1.0 + S
    r = t / den
    e_den = eS + U * den
    e_t = eS * np.abs(d) + 2 * U * np.abs(S * d) + U * np.abs(t)   # rounded difference, product, sum
    return r, SAFETY * (e_t / den + np.abs(t) * e_den / den ** 2 + U * np.abs(r))


def tv_step_bound(x, xbar, u, p, s_grad, lam, theta=1.0, tau=None, colsum=None):
    """(binary64 (x_new, xbar_new, p_new), bounds of the three) of one float32 ``tv_step`` on float32 inputs.  ``tau``: scalar mode;
    ``colsum``: diagonal mode, T = 1 / (colsum + d) formed in float32 (an addition and a reciprocal)."""
    x, xbar, u, p = (np.asarray(v, np.float64) for v in (x, xbar, u, p))
    nx, n = x.shape[0], x.shape[1]
    if colsum is not None:
        T = primal_T(colsum, nx, n)
        eT = 2 * U * T
    else:
        T, eT = np.float64(tau), 0.0
    xn, xb, pn = tv_step(x, xbar, u, p, s_grad, T, lam, theta)
    g = grad(xbar)
    _, a = dual_field(xbar, p, s_grad, lam)
    m = np.stack([_mask_last(x.shape, k) for k in range(3)])
    # a_a = s_grad (xbar+ - xbar) + p_a: the difference, the product, the sum
    e_a = np.where(m, 2 * U * np.abs(s_grad * g) + U * np.abs(a), 0.0)
    nrm = np.sqrt(np.sum(a * a, axis=0))
    e_nrm = np.sqrt(np.sum(e_a * e_a, axis=0)) + 2.5 * U * nrm     # the norm is 1-Lipschitz; three squares, two sums, the root
    r = nrm / lam
    e_r = e_nrm / lam + U * r
    mx = np.maximum(1.0, r)
    inv = 1.0 / mx
    e_inv = e_r / mx ** 2 + U * inv                                 # max(1, .) is 1-Lipschitz
    e_p = e_a * inv[None] + np.abs(a) * e_inv[None] + U * np.abs(pn)
    dd = np.stack([pn[k] - _back(pn[k], k) for k in range(3)])
    e_div = sum(e_p[k] + _back(e_p[k], k) for k in range(3)) + 3 * U * np.sum(np.abs(dd), axis=0)
    dv = div(pn)
    t = u - dv
    e_t = e_div + U * np.abs(t)
    v = x - T * t
    e_x = eT * np.abs(t) + T * e_t + U * np.abs(T * t) + U * np.abs(v)          # the clamp is 1-Lipschitz
    dx = xn - x
    e_dx = e_x + U * np.abs(dx)
    e_xb = e_x + abs(theta) * e_dx + U * np.abs(theta * dx) + U * np.abs(xb)
    return (xn, xb, pn), (SAFETY * e_x, SAFETY * e_xb, SAFETY * e_p)


# ---- the loop ------------------------------------------------------------------------------------------------------------------
def dense(M, dtype=np.float64):
    key = "_pdhg_dense_%s" % np.dtype(dtype).name
    if getattr(M, key, None) is None:
        D = np.zeros((M.nrow, M.ncol), dtype)
        np.add.at(D, (M.rows, M.cols), M.w32.astype(dtype))
        setattr(M, key, D)
    return getattr(M, key)


def objective(M, x, b, lam):
    """1/2 |Ax - b|^2 + lam |grad x|_{2,1} in binary64."""
    x = np.asarray(x, np.float64)
    r = x.reshape(len(x), -1) @ dense(M).T - np.asarray(b, np.float64)
    g = grad(x)
    return 0.5 * float(np.sum(r * r)) + lam * float(np.sum(np.sqrt(np.sum(g * g, axis=0))))


def pdhg(M, b, niter, lam, theta=1.0, precond=True, ratio=1.0, L=None, dtype=np.float64, state=None):
    """``niter`` iterations from x = 0 (or from ``state``, a dict this function returned); returns the state: x, xbar, p, q, u and
    ``sqdiff`` = sum (x_new - x)^2 of the last iteration.  ``L``: the Lipschitz constant of the scalar mode (default: M.lipschitz())."""
    b = np.asarray(b, dtype)
    nx, n = len(b), M.N
    D = dense(M, dtype)
    if precond:
        rs, cs = tables_f32(M)
        S, sg, T = dual_S(rs, dtype), dtype(0.5), primal_T(cs, nx, n, dtype)
    else:
        if L is None:
            L = M.lipschitz()[0]
        sigma, tau = scalar_steps(L, ratio)
        S, sg, T = dtype(sigma), dtype(sigma), dtype(tau)
    if state is None:
        z = np.zeros((nx, n, n), dtype)
        state = dict(x=z, xbar=z.copy(), p=np.zeros((3, nx, n, n), dtype), q=np.zeros((nx, M.nrow), dtype), u=z.copy(), sqdiff=0.0)
    x, xbar, p, q, u = (np.asarray(state[k], dtype) for k in ("x", "xbar", "p", "q", "u"))
    sq = state.get("sqdiff", 0.0)
    for _ in range(niter):
        g = (xbar.reshape(nx, -1) @ D.T).astype(dtype)
        q = sino_dual(q, g, b, S, dtype)
        u = (q @ D).astype(dtype).reshape(nx, n, n)
        xn, xbar, p = tv_step(x, xbar, u, p, sg, T, lam, theta, dtype)
        sq = float(np.sum((xn.astype(np.float64) - x.astype(np.float64)) ** 2))
        x = xn
    return dict(x=x, xbar=xbar, p=p, q=q, u=u, sqdiff=sq)


def block_phantom(nx, n):
    """Piecewise-constant test object: two boxes of different height on a zero background, a different extent per slice."""
    x = np.zeros((nx, n, n), np.float32)
    for s in range(nx):
        a = n // 4 + (s % 3)
        x[s, a:a + n // 3, n // 5:n // 5 + n // 2] = 1.0
        x[s, n // 2:n // 2 + n // 4, n // 2 + (s % 2):n // 2 + n // 3] = 2.0
    return x


__all__ = ["grad", "div", "sino_dual", "tv_step", "pdhg", "sino_dual_bound", "tv_step_bound", "objective", "scalar_steps", "tables_f32",
           "primal_T", "dual_S", "dense", "block_phantom", "touch_count", "dual_field", "ref64"]
