"""Connected components in plain numpy: the statement of include/tomo_hip.h (tomo_components_*), independent of scipy.

foreground:   lo <= x <= hi in binary32; a NaN is never foreground
neighbours:   6 (faces) or 26 (faces, edges, corners), not periodic
numbering:    components 1..K in ascending order of their smallest linear index p = (s Ny + y) Nz + z; background 0
measurements: integers per component -- voxels, sum_s / _y / _z, inclusive bounding box, first (smallest p), surface (voxels with one of
              the SIX face neighbours background or outside the volume)

The labelling is a vectorised minimum propagation: every foreground voxel takes the smallest label in its neighbourhood, hooks the
voxel its label names onto that minimum too, and the labels are then flattened by pointer jumping; repeated until nothing changes.
A fixed point has one label per component, and that label is the component's smallest index.
"""
import numpy as np

from tomo_tv_amd._lib import COMPONENT_FIELDS

DTYPE = np.dtype(COMPONENT_FIELDS)


def foreground(x, lo, hi):
    x = np.asarray(x, np.float32)
    with np.errstate(invalid="ignore"):
        return (x >= np.float32(lo)) & (x <= np.float32(hi))


def offsets(connectivity):
    if connectivity not in (6, 26):
        raise ValueError("connectivity must be 6 or 26")
    rng = (-1, 0, 1)
    every = [(a, b, c) for a in rng for b in rng for c in rng if (a, b, c) != (0, 0, 0)]
    return [o for o in every if connectivity == 26 or sum(map(abs, o)) == 1]


def _shifted(a, off, fill):
    """out[v] = a[v + off] where v + off lies inside the array, else fill"""
    out = np.full_like(a, fill)
    src, dst = [], []
    for d, n in zip(off, a.shape):
        src.append(slice(max(d, 0), n + min(d, 0)))
        dst.append(slice(max(-d, 0), n - max(d, 0)))
    out[tuple(dst)] = a[tuple(src)]
    return out


def label(fg, connectivity):
    """-> (labels int32 of fg's shape, K)"""
    fg = np.asarray(fg, bool)
    big = fg.size
    L = np.where(fg, np.arange(fg.size, dtype=np.int64).reshape(fg.shape), big)
    at = np.flatnonzero(fg)
    offs = offsets(connectivity)
    while at.size:
        m = L.copy()
        for off in offs:
            m = np.minimum(m, _shifted(L, off, big))
        m = np.where(fg, m, big)
        if np.array_equal(m, L):
            break
        flat, mf = L.reshape(-1).copy(), m.reshape(-1)
        np.minimum.at(flat, flat[at], mf[at])            # the voxel a label names hooks onto the smaller label as well
        flat[at] = np.minimum(flat[at], mf[at])
        while True:                                      # pointer jumping
            nxt = flat[flat[at]]
            if np.array_equal(nxt, flat[at]):
                break
            flat[at] = nxt
        L = flat.reshape(fg.shape)
    roots = np.unique(L[fg])                             # ascending: the numbering rule
    out = np.zeros(fg.shape, np.int32)
    out[fg] = np.searchsorted(roots, L[fg]) + 1
    return out, int(roots.size)


def surface_mask(labels):
    """foreground voxels with a face neighbour that is background or outside the volume"""
    fgd = labels > 0
    inner = fgd.copy()
    for off in offsets(6):
        inner &= _shifted(fgd, off, False)
    return fgd & ~inner


def stats(labels):
    """-> structured array (K,) of DTYPE, record k - 1 for component k"""
    labels = np.asarray(labels)
    K = int(labels.max()) if labels.size else 0
    out = np.zeros(K, DTYPE)
    if not K:
        return out
    s, y, z = np.nonzero(labels)
    k = labels[s, y, z].astype(np.int64) - 1
    p = (s.astype(np.int64) * labels.shape[1] + y) * labels.shape[2] + z
    out["voxels"] = np.bincount(k, minlength=K)
    for name, c in (("s", s), ("y", y), ("z", z)):
        out["sum_" + name] = np.bincount(k, weights=c.astype(np.float64), minlength=K).astype(np.int64)   # exact: far below 2^53
        mn, mx = np.full(K, np.iinfo(np.int32).max, np.int64), np.full(K, -1, np.int64)
        np.minimum.at(mn, k, c)
        np.maximum.at(mx, k, c)
        out["min_" + name], out["max_" + name] = mn, mx
    first = np.full(K, labels.size, np.int64)
    np.minimum.at(first, k, p)
    out["first"] = first
    out["surface"] = np.bincount(k, weights=surface_mask(labels)[s, y, z].astype(np.float64), minlength=K).astype(np.int64)
    return out


def components(x, lo, hi, connectivity):
    """-> (labels, K, records) of volume x"""
    lab, K = label(foreground(x, lo, hi), connectivity)
    return lab, K, stats(lab)


def keep(x, labels, table, fill):
    """the volume after tomo_components_keep"""
    out = np.array(x, np.float32, copy=True)
    out[(labels > 0) & ~np.asarray(table, bool)[labels]] = np.float32(fill)
    return out
