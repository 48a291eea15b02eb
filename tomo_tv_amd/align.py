"""Host side of the tilt-series alignment: the peak rule of projection matching and the centre-of-mass rule of the reference.

The windows are ``Nangles * (2S+1)^2`` doubles, so this is bookkeeping, not hot path: the correlation itself, the moments and the
resampling are HIP kernels (``tomoengine.sino_xcorr`` / ``sino_moments`` / ``sino_shift``)."""
import numpy as np


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


def center_of_mass_shifts(moments, nray, nslice):
    """cpu/utils/logger.py:237-247 per projection from its moments (sum X, sum r X, sum s X): the centre of mass truncated to an
    integer, moved to ``size // 2`` on both axes.  (Nangles, 2) int64 of (dr, ds)."""
    m = np.asarray(moments, np.float64)
    out = np.zeros((m.shape[0], 2), np.int64)
    for a in range(m.shape[0]):
        out[a, 0] = -(int(m[a, 1] / m[a, 0]) - nray // 2)
        out[a, 1] = -(int(m[a, 2] / m[a, 0]) - nslice // 2)
    return out
