"""Binary64 statements of the dual-axis calls (``tomo_volume_cross``, ``tomo_volume_cross_axpy``), of the second engine's stacked
operator and of the alternating Landweber loop of ``DualAxisTomo.sirt``.  numpy only (GPU tests import it); the matrices are
``ref64.Matrix`` objects.

Convention: the public volume is ``X[s][y][z]``; engine A has slice index s, engine B slice index z, row index y and column index s,
``X_B[z][y][s] = X_A[s][y][z]``.  A sinogram is packed like the engine's host calls: ``[slice][angle * N + ray]``."""
import numpy as np


def cross(X):
    """The volume in the other engine's layout: an involution."""
    return np.ascontiguousarray(np.asarray(X).transpose(2, 1, 0))


def cross_loops(X):
    X = np.asarray(X)
    N = X.shape[0]
    out = np.empty_like(X)
    for z in range(N):
        for y in range(N):
            for s in range(N):
                out[z, y, s] = X[s, y, z]
    return out


def cross_axpy(S, D, a, clamp=False):
    """``D + a cross(S)`` in binary64 for binary32 inputs (the product is exact there, the sum rounds once at 2^-53), then the clamp
    ``max(0, .)`` in the sense of fmaxf: a NaN becomes 0.  ``a`` is rounded to binary32 first, as the C call receives it."""
    with np.errstate(invalid="ignore"):
        v = float(np.float32(a)) * cross(S).astype(np.float64) + np.asarray(D, np.float64)
        if clamp:
            v = np.where(np.isnan(v), 0.0, np.maximum(v, 0.0))
    return v


def cross_axpy_loops(S, D, a, clamp=False):
    S, D = np.asarray(S, np.float64), np.asarray(D, np.float64)
    N = S.shape[0]
    out = np.empty((N, N, N))
    for z in range(N):
        for y in range(N):
            for s in range(N):
                v = float(np.float32(a)) * S[s, y, z] + D[z, y, s]
                out[z, y, s] = (0.0 if v != v or v < 0 else v) if clamp else v
    return out


def fp_a(MA, X):
    """b_A[s] = A_A vec(X[s]): (N, Pa N)."""
    return MA.fp(X)


def fp_b(MB, X):
    """b_B[z] = A_B vec(X[:, :, z]^T), the image with rows y and columns s: (N, Pb N)."""
    return MB.fp(cross(X))


def bp_b(MB, R):
    """The adjoint of ``fp_b``: a volume X[s][y][z]."""
    return cross(MB.bp(R))


def dense(M):
    A = np.zeros((M.nrow, M.ncol))
    np.add.at(A, (M.rows, M.cols), M.vals)
    return A


def fp_b_dense(MB, X):
    """The same as one matrix product: ``A_B @ cross(X).reshape(N, N * N).T``, returned as (N, Pb N)."""
    N = MB.N
    return (dense(MB) @ cross(X).reshape(N, N * N).T).T


def landweber(M, x, b, t):
    """max(0, x + t A^T (b - A x)) on an engine's own layout."""
    return np.maximum(x + t * M.bp(np.asarray(b, np.float64).reshape(len(x), M.nrow) - M.fp(x)), 0.0)


def single_axis(M, b, t, niter, x0=None):
    x = np.zeros((M.N, M.N, M.N)) if x0 is None else np.array(x0, np.float64)
    for _ in range(int(niter)):
        x = landweber(M, x, b, t)
    return x


def dual_axis(MA, MB, bA, bB, tA, tB, niter, x0=None):
    """``DualAxisTomo.sirt``: per iteration a Landweber step on A, the volume crossed, a Landweber step on B, the volume crossed
    back.  Returns the volume of record X[s][y][z]."""
    x = np.zeros((MA.N, MA.N, MA.N)) if x0 is None else np.array(x0, np.float64)
    for _ in range(int(niter)):
        x = landweber(MA, x, bA, tA)
        x = cross(landweber(MB, cross(x), bB, tB))
    return x


def phantom(N):
    """The recovery case: an off-centre box with a slot cut through it and a small denser block, asymmetric in all three axes."""
    X, a = np.zeros((N, N, N)), N // 4
    X[a:N - a - 2, a + 1:N - a, a + 2:N - a - 1] = 1.0
    X[a + 2:a + 4, a + 3:N - a - 3, :] = 0.0
    X[N // 2:N // 2 + 3, N // 2 - 1:N // 2 + 4, N // 2 + 1:N // 2 + 3] = 2.0
    return X


def rmse(x, X):
    return float(np.sqrt(np.mean((np.asarray(x, np.float64) - X) ** 2)))


def ulp32(v):
    """The spacing of binary32 at |v| (binary64 in, binary64 out; the subnormal spacing below 2^-126)."""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.spacing(np.abs(np.asarray(v, np.float64)).astype(np.float32)).astype(np.float64)
