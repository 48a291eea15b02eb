"""Vectorised numpy statements of the DART kernels (tomo_tv_amd/csrc/kernels_dart.hip.h, include/tomo_hip.h) and of the driver loop.

Volumes are (Nslice, N, N) arrays indexed [s][y][z].  Neighbours are not periodic: a neighbour outside the array does not exist.

The smoother's bound.  The kernel forms, in binary32 (u = 2^-24, gamma_n = n u / (1 - n u)):
    S = the sequential sum of the k <= 26 existing neighbours v_i       |S - sum v_i| <= gamma_{k-1} sum |v_i|
    r = fl(1 / k),  m = fl(S r)                                         two more roundings: m = (sum v_i / k)(1 + theta), |theta| <= gamma_{k+1}
    d = fl(m - x)                                                       d = (m - x)(1 + d3), |d3| <= u
    out = fl(beta d + x)  (one fma)                                     out = (beta d + x)(1 + d4), |d4| <= u
With the exact m* = sum v_i / k, A = sum |v_i| / k and out* = x + beta (m* - x):
    e_m = |m - m*|  <= gamma_{k+1} A
    e_d = |d - (m* - x)| <= e_m + u (|m* - x| + e_m)
    |out - out*| <= beta e_d + u (|out*| + beta e_d)                    =: bound
(no underflow: the tests use values of order one).  ``smooth`` returns out* in binary64 and this bound per element."""
import numpy as np

LABEL_MASK, BOUNDARY, FREE = 15, 64, 128
U32 = np.float64(2.0 ** -24)


def labels(x, thr):
    """label = the number of thresholds t with x >= t, compared in binary32 (NaN: 0, +Inf: len(thr))."""
    x = np.asarray(x, np.float32)
    lab = np.zeros(x.shape, np.uint8)
    with np.errstate(invalid="ignore"):
        for t in np.asarray(thr, np.float32).ravel():
            lab += (x >= t).astype(np.uint8)
    return lab


def offsets(connectivity):
    offs = [(ds, dy, dz) for dy in (-1, 0, 1) for dz in (-1, 0, 1) for ds in (-1, 0, 1) if (ds, dy, dz) != (0, 0, 0)]
    if connectivity == 6:
        offs = [o for o in offs if abs(o[0]) + abs(o[1]) + abs(o[2]) == 1]
    elif connectivity != 26:
        raise ValueError("connectivity must be 6 or 26")
    return offs                                           # ascending (dy, dz, ds): the smoother's order of summation


def _shifted(a, off, fill):
    """b[v] = a[v + off] where v + off lies inside the array, else fill; and the mask of where it does."""
    out = np.full(a.shape, fill, a.dtype)
    ok = np.zeros(a.shape, bool)
    src, dst = [], []
    for d, n in zip(off, a.shape):
        dst.append(slice(max(0, -d), n - max(0, d)))
        src.append(slice(max(0, d), n - max(0, -d)))
    out[tuple(dst)] = a[tuple(src)]
    ok[tuple(dst)] = True
    return out, ok


def boundary(lab, connectivity):
    b = np.zeros(lab.shape, bool)
    for off in offsets(connectivity):
        nb, ok = _shifted(lab, off, 0)
        b |= ok & (nb != lab)
    return b


def mix(a):
    a = np.asarray(a, np.uint32).copy()
    a ^= a >> np.uint32(16)
    a *= np.uint32(0x7feb352d)
    a ^= a >> np.uint32(15)
    a *= np.uint32(0x846ca68b)
    a ^= a >> np.uint32(16)
    return a


def draws(shape, seed):
    """h(v) = mix(mix(idx) ^ seed), idx = (s N + y) N + z in uint32 arithmetic."""
    ns, n, nz = shape                                     # (the GPU's volumes have nz == n; N of the index is the y extent)
    s, y, z = np.meshgrid(np.arange(ns, dtype=np.uint32), np.arange(n, dtype=np.uint32), np.arange(nz, dtype=np.uint32), indexing="ij")
    idx = (s * np.uint32(n) + y) * np.uint32(n) + z
    return mix(mix(idx) ^ np.uint32(seed))


def free_threshold(free_fraction):
    return min(int(free_fraction * 2 ** 32), 2 ** 32 - 1)


def free_set(bnd, seed, thr_free):
    return bnd | (draws(bnd.shape, seed) < np.uint32(thr_free))


def state(x, thr, connectivity, seed, thr_free):
    lab = labels(x, thr)
    bnd = boundary(lab, connectivity)
    fr = free_set(bnd, seed, thr_free)
    return (lab | (bnd * np.uint8(BOUNDARY)) | (fr * np.uint8(FREE))).astype(np.uint8)


def restore(x, st, grey, everywhere=False):
    x = np.asarray(x, np.float32)
    g = np.asarray(grey, np.float32)[st & LABEL_MASK]
    return g if everywhere else np.where((st & FREE) != 0, x, g)


def smooth(x, st, beta):
    """-> (out* in binary64, the per-element bound of the module docstring, free mask).  Fixed voxels: out* = x, bound 0."""
    x32 = np.asarray(x, np.float32)
    x64 = x32.astype(np.float64)
    beta = np.float64(np.float32(beta))
    tot, tot_abs, cnt = np.zeros(x64.shape), np.zeros(x64.shape), np.zeros(x64.shape)
    for off in offsets(26):
        nb, ok = _shifted(x64, off, 0.0)
        tot += nb
        tot_abs += np.abs(nb)
        cnt += ok
    fr = ((np.asarray(st) & FREE) != 0) & (cnt > 0)
    k = np.maximum(cnt, 1.0)
    m = tot / k
    A = tot_abs / k
    out = np.where(fr, x64 + beta * (m - x64), x64)
    gam = (k + 1) * U32 / (1 - (k + 1) * U32)
    e_m = gam * A
    e_d = e_m + U32 * (np.abs(m - x64) + e_m)
    bound = np.where(fr, beta * e_d + U32 * (np.abs(out) + beta * e_d), 0.0)
    return out, bound, fr


def class_stats(x, thr):
    """(K, 2) float64: the sum of the finite voxels of every class and the number of its voxels (finite or not)."""
    x = np.asarray(x, np.float32)
    lab = labels(x, thr)
    K = np.asarray(thr).size + 1
    out = np.zeros((K, 2))
    fin = np.isfinite(x)
    for c in range(K):
        sel = lab == c
        out[c, 0] = x[sel & fin].astype(np.float64).sum()
        out[c, 1] = sel.sum()
    return out


def thresholds(levels):
    g = np.asarray(levels, np.float64).ravel()
    return (0.5 * (g[:-1] + g[1:])).astype(np.float32)


def lloyd(x, K, iters=20):
    """TomoGPU.estimate_grey_levels on a host array."""
    x = np.asarray(x, np.float32)
    levels = np.linspace(float(x.min()), float(x.max()), K)
    for _ in range(iters):
        if K == 1 or not np.all(np.diff(levels.astype(np.float32)) > 0):
            break
        st = class_stats(x, thresholds(levels))
        new = np.where(st[:, 1] > 0, st[:, 0] / np.maximum(st[:, 1], 1.0), levels)
        if np.array_equal(new, levels):
            break
        levels = new
    return levels


# ---- the driver loop in binary64 (scipy) ---------------------------------------------------------------------------------------
class Sirt64:
    """Normalised SIRT as in oracle: x = max(0, x + C A^T R (b - A x)), R = 1 / row sums, C = 1 / column sums (0 where a sum is 0)."""

    def __init__(self, A3, nrow, ncol):
        import scipy.sparse as sp
        A3 = np.asarray(A3)
        self.A = sp.csr_matrix((A3[2].astype(np.float64), (A3[0].astype(np.int64), A3[1].astype(np.int64))), shape=(nrow, ncol))
        rs, cs = np.asarray(self.A.sum(1)).ravel(), np.asarray(self.A.sum(0)).ravel()
        self.R = np.where(rs > 0, 1.0 / np.where(rs > 0, rs, 1.0), 0.0)
        self.C = np.where(cs > 0, 1.0 / np.where(cs > 0, cs, 1.0), 0.0)

    def project(self, x):                                  # x (Nslice, N, N) -> (Nslice, nrow)
        return (self.A @ x.reshape(x.shape[0], -1).T).T

    def step(self, x, b):
        r = (b - self.project(x)) * self.R
        u = (self.A.T @ r.T).T * self.C
        return np.maximum(0.0, x + u.reshape(x.shape))


def _smooth64(x, st, beta):
    tot, cnt = np.zeros(x.shape), np.zeros(x.shape)
    for off in offsets(26):
        nb, ok = _shifted(x, off, 0.0)
        tot += nb
        cnt += ok
    fr = ((st & FREE) != 0) & (cnt > 0)
    return np.where(fr, x + beta * (tot / np.maximum(cnt, 1.0) - x), x)


def dart_loop(sirt, b, grey, Niter, arm_iters, init_iters, fix_probability, smoothing, connectivity, seed, shape, segment=True):
    """TomoGPU.dart from a zero volume, in binary64 (the labels compare in binary32, like the kernel).  -> (volume, labels, records)."""
    grey = np.asarray(grey, np.float64)
    thr = thresholds(grey)
    x = np.zeros(shape)
    for _ in range(init_iters):
        x = sirt.step(x, b)
    rec = {"n_free": [], "n_boundary": [], "data_distance": []}
    tf = free_threshold(1.0 - fix_probability)
    for k in range(Niter):
        st = state(x.astype(np.float32), thr, connectivity, (seed * 0x9E3779B1 + k) & 0xffffffff, tf)
        fixed = (st & FREE) == 0
        g = grey[st & LABEL_MASK]
        x = np.where(fixed, g, x)
        for _ in range(arm_iters):
            x = np.where(fixed, g, sirt.step(x, b))
        if smoothing != 0:
            x = _smooth64(x, st, smoothing)
        rec["n_free"].append(int((~fixed).sum()))
        rec["n_boundary"].append(int(((st & BOUNDARY) != 0).sum()))
        rec["data_distance"].append(float(np.linalg.norm(sirt.project(x) - b)))
    lab = labels(x.astype(np.float32), thr)
    if segment:
        x = grey[lab]
    return x, lab, rec


# ---- the phantom and parameters of the driver tests (CPU replay and GPU) -------------------------------------------------------
DRIVER = dict(Nslice=4, N=32, grey=(0.0, 1.0), Niter=8, arm_iters=5, init_iters=20, fix_probability=0.85, smoothing=0.1,
              connectivity=26, seed=7)


LLOYD_SIRT_ITERS = 400        # estimate_grey_levels(2) is asked of a SIRT reconstruction of this many iterations


def driver_phantom(Nslice=4, N=32):
    """Two phases: background 0 and a block of grey level 1 with a slot-shaped hole, shifted by one pixel per slice (so that slice
    neighbours matter).  With the nine angles of tests/golden/A_N32_P9.npz (-70 .. 70 degrees) the binary64 replay misclassifies
    2 voxels by DART against 16 by SIRT + threshold at the same 60 iterations, and the two Lloyd levels of a 400-iteration SIRT
    reconstruction are 0.035 and 0.954."""
    v = np.zeros((Nslice, N, N), np.float32)
    for s in range(Nslice):
        v[s, 5 + s:27 + s, 6:26] = 1.0
        v[s, 14 + s:17 + s, 12:20] = 0.0
    return v
