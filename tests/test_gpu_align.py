"""Alignment on the GPU, every output element against tests/ref64_align.py.  The shapes are the smallest at which each hazard
appears (pitch padding, several 64-slice chunks, Nslice < 2S+1, S = N/2, the S cap with more than one ray block)."""
import ctypes

import numpy as np
import pytest

import ref64_align as R
from test_align_cpu import blobs

pytestmark = pytest.mark.gpu

SHAPES = [((70, 33, 5), 4), ((256, 40, 4), 3), ((5, 24, 2), 4), ((64, 16, 3), 8), ((64, 200, 2), 16)]
IDS = ["pad58", "chunks4", "thin", "halfN", "cap16"]
A_SLOT, B_SLOT, D_SLOT, E_SLOT = 3, 4, 5, 6          # TOMO_SINO_USER0 ...


class Case:
    def __init__(self, shape, S):
        from tomo_tv_amd.engine import tomoengine
        self.ns, self.N, self.P = shape
        self.S = S
        self.eng = tomoengine(self.ns, self.N, np.deg2rad(np.linspace(-60, 60, self.P)), device=0)
        self.A, self.B = blobs(self.P, self.N, self.ns, 100 + self.N), blobs(self.P, self.N, self.ns, 200 + self.N)
        self.put(A_SLOT, self.A)
        self.put(B_SLOT, self.B)

    def put(self, slot, X):
        b = R.packed(np.asarray(X, np.float32))
        self.eng.be.c("set_sinogram", slot, b.ctypes.data_as(ctypes.c_void_p))

    def get(self, slot):
        return R.images(self.eng._sino(slot), self.N)

    def int_shifts(self, seed):
        rng = np.random.default_rng(seed)
        return rng.integers(-self.S, self.S + 1, (self.P, 2))


@pytest.fixture(scope="module", params=list(zip(SHAPES, IDS)), ids=IDS)
def case(request, gpu):
    (shape, S), _ = request.param
    return Case(shape, S)


def worst(err, bound):
    return float(np.max(err / np.maximum(bound, 1e-300)))


@pytest.mark.parametrize("sub", [True, False])
def test_xcorr_every_element_within_its_bound(case, sub):
    C = case.eng.sino_xcorr(A_SLOT, B_SLOT, case.S, sub)
    err, bound = np.abs(C - R.xcorr(case.A, case.B, case.S, sub)), R.xcorr_bound(case.A, case.B, case.S, sub)
    print(f"worst error / bound: {worst(err, bound):.3f}")
    assert np.all(err <= bound)
    assert np.array_equal(C, case.eng.sino_xcorr(A_SLOT, B_SLOT, case.S, sub))          # bit-identical from run to run


# How far a copy of A moved by d (with wrap-around) still peaks at d, per shape, found with the binary64 correlation on the CPU:
# the sums are not divided by the overlap, so the entry at d loses the factor (1 - |dr| / N)(1 - |ds| / Nslice) against its
# neighbours towards zero.  Roomy shapes hold over the whole window; at N = 16 with S = 8 half the rows are lost beyond |dr| = 3, at
# Nslice = 5 one slice of shift already costs a fifth of the sum, and at Nslice = 64 the last entry (|ds| = 16 of 16) falls to 15.
PEAK_LIMITS = {"pad58": (4, 4), "chunks4": (3, 3), "thin": (4, 0), "halfN": (3, 8), "cap16": (16, 15)}


def test_xcorr_peaks(case, request):
    S = case.S
    pk, _, _ = R.peaks(case.eng.sino_xcorr(A_SLOT, A_SLOT, S), subpixel=False)
    assert not pk.any()                                                                   # A with itself: (0, 0)
    # B = A moved by d: the peak is at d, for d on the axes' ends, in the four corners and at random inside PEAK_LIMITS
    lim_r, lim_s = PEAK_LIMITS[request.node.callspec.id]
    rng = np.random.default_rng(7)
    rows = [np.stack([rng.integers(-lim_r, lim_r + 1, case.P), rng.integers(-lim_s, lim_s + 1, case.P)], axis=1)]
    rows += [np.tile([a * lim_r, b * lim_s], (case.P, 1)) for a in (-1, 0, 1) for b in (-1, 0, 1) if a or b]
    for d in rows:
        case.eng.sino_shift(A_SLOT, D_SLOT, d, wrap=True)
        pk, _, _ = R.peaks(case.eng.sino_xcorr(A_SLOT, D_SLOT, S), subpixel=False)
        assert np.array_equal(pk, d), d[0]


def test_moments(case):
    m, ref = case.eng.sino_moments(A_SLOT), R.moments(case.A)
    print(f"worst relative error: {np.max(np.abs(m - ref) / ref):.3e}")
    assert m.shape == (case.P, 3) and np.all(np.abs(m - ref) <= 1e-6 * np.abs(ref))
    assert np.array_equal(m, case.eng.sino_moments(A_SLOT))


@pytest.mark.parametrize("wrap", [False, True])
def test_shift_whole_pixels_is_bit_exact(case, wrap):
    d = case.int_shifts(11)
    d[0] = (0, 0)
    case.eng.sino_shift(A_SLOT, D_SLOT, d, wrap=wrap)
    assert np.array_equal(case.get(D_SLOT), R.shift_int(case.A, d, wrap=wrap))


@pytest.mark.parametrize("wrap", [False, True])
def test_shift_fractions_and_padding(case, wrap):
    rng = np.random.default_rng(13)
    d = rng.uniform(-case.S, case.S, (case.P, 2)).astype(np.float32)
    d[0, 1] = np.float32(round(float(d[0, 1])))                  # one axis whole, the other not: the two-tap paths
    if case.P > 1:
        d[1, 0] = np.float32(round(float(d[1, 0])))
    case.eng.sino_shift(A_SLOT, D_SLOT, d, wrap=wrap)
    ref, mag = R.shift(case.A, d, wrap=wrap)
    got = case.get(D_SLOT)
    err, bound = np.abs(got - ref), 4 * 2.0 ** -23 * mag
    print(f"worst error / bound: {worst(err, bound + 1e-300):.3f}")
    assert np.all(err <= bound)
    # the padding slices of dst are still zero: its auto-correlation at v = +-S meets its bound (the issue's check) ...
    C = case.eng.sino_xcorr(D_SLOT, D_SLOT, case.S, False)
    assert np.all(np.abs(C - R.xcorr(got, got, case.S, False)) <= R.xcorr_bound(got, got, case.S, False))
    # ... and, since that kernel never reads the padding, a reduction that does sweep the whole pitch: the real samples of dst
    # uploaded into another slot (an upload writes zero padding) differ from dst by exactly nothing, padding included
    case.put(E_SLOT, got)
    case.eng.be.c("sino_diff_norm_sq", D_SLOT, E_SLOT, 1)
    assert case.eng.be.scalars()[1] == 0.0


def test_shift_by_a_fraction_that_rounds_to_a_whole_pixel_copies(case):
    """d = 2^-30: the binary32 fraction of -d is 1, i.e. the whole-pixel shift 0 -- taken by the copy path, bit for bit"""
    d = np.full((case.P, 2), 2.0 ** -30, np.float32)
    d[-1] = (-(2.0 ** -30), 3 + 2.0 ** -30)               # 3 + 2^-30 is 3 in binary32; a tiny negative d has a tiny exact fraction
    for wrap in (False, True):
        case.eng.sino_shift(A_SLOT, D_SLOT, d, wrap=wrap)
        got = case.get(D_SLOT)
        assert np.array_equal(got[:-1], case.A[:-1])
        ref, mag = R.shift(case.A, d, wrap=wrap)
        assert np.all(np.abs(got - ref) <= 4 * 2.0 ** -23 * mag)


def test_shift_beyond_the_image_gives_zeros(case):
    d = np.zeros((case.P, 2), np.float32)
    d[:, 0] = case.N
    d[-1] = (0.5, -(case.ns + 0.25))
    d[0] = (-3e9, 1e30)
    case.eng.sino_shift(A_SLOT, D_SLOT, d, wrap=False)
    assert not case.get(D_SLOT).any()


def test_argument_errors_leave_the_engine_usable(case):
    from tomo_tv_amd import _lib
    L, h, P = case.eng.be.L, case.eng.be.h, case.P
    out = np.zeros((P, 33, 33))
    po = out.ctypes.data_as(ctypes.c_void_p)
    sh = np.zeros((P, 2), np.float32)
    ps = sh.ctypes.data_as(ctypes.c_void_p)
    bad = sh.copy()
    bad[-1, 1] = np.nan
    inf = sh.copy()
    inf[0, 0] = np.inf
    calls = [L.tomo_sino_moments(h, -1, po), L.tomo_sino_moments(h, 43, po), L.tomo_sino_moments(h, A_SLOT, None),
             L.tomo_sino_xcorr(h, 99, B_SLOT, 1, 1, po), L.tomo_sino_xcorr(h, A_SLOT, -2, 1, 1, po),
             L.tomo_sino_xcorr(h, A_SLOT, B_SLOT, 0, 1, po), L.tomo_sino_xcorr(h, A_SLOT, B_SLOT, 17, 1, po),
             L.tomo_sino_xcorr(h, A_SLOT, B_SLOT, min(case.N, case.ns), 1, po), L.tomo_sino_xcorr(h, A_SLOT, B_SLOT, 1, 1, None),
             L.tomo_sino_shift(h, A_SLOT, A_SLOT, ps, 0), L.tomo_sino_shift(h, A_SLOT, 77, ps, 0), L.tomo_sino_shift(h, A_SLOT, D_SLOT, None, 0),
             L.tomo_sino_shift(h, A_SLOT, D_SLOT, bad.ctypes.data_as(ctypes.c_void_p), 0),
             L.tomo_sino_shift(h, A_SLOT, D_SLOT, inf.ctypes.data_as(ctypes.c_void_p), 1)]
    assert calls == [1] * len(calls) and L.tomo_last_error()
    with pytest.raises(_lib.TomoError):
        case.eng.sino_xcorr(A_SLOT, B_SLOT, 17)
    assert np.array_equal(case.get(A_SLOT), case.A)                                       # nothing was touched
    C = case.eng.sino_xcorr(A_SLOT, B_SLOT, case.S)
    assert np.all(np.abs(C - R.xcorr(case.A, case.B, case.S)) <= R.xcorr_bound(case.A, case.B, case.S))


# ---- TomoGPU ------------------------------------------------------------------------------------------------------------------
def public(X):
    """X[a][r][s] -> the (Nslice, Nray, Nangles) array TomoGPU is given"""
    return np.ascontiguousarray(np.asarray(X).transpose(2, 1, 0))


def test_align_center_of_mass_is_the_references_rule(gpu):
    from tomo_tv_amd.reconstructor import TomoGPU
    X = blobs(5, 33, 70, 31)
    rec = TomoGPU(np.linspace(-60, 60, 5), public(X), gpu_id=0)
    sh = rec.align_center_of_mass()
    want, rolled = R.center_of_mass(X)
    assert sh.shape == (5, 2) and np.issubdtype(sh.dtype, np.integer) and np.array_equal(sh, want) and want.any()
    assert np.array_equal(rec.get_projections(), public(rolled))
    assert np.array_equal(rec.get_alignment(), want)
    assert np.array_equal(R.images(rec.tomo._sino(rec.ALIGN_SLOT), 33), X)               # the series as given is kept
    rec.set_alignment(np.zeros((5, 2)))
    assert np.array_equal(rec.get_projections(), public(X))                               # totals, not increments: back to the start


@pytest.fixture(scope="module", params=[False, True], ids=["plain31", "leave_one_out9"])
def refine_gpu(request, gpu):
    """plain projection matching at 31 projections (ref64_align.PLAIN_CASE) and leave-one-out at 9 (REFINE_CASE), each beside its
    CPU replay"""
    from tomo_tv_amd.reconstructor import TomoGPU
    loo = request.param
    c = R.REFINE_CASE if loo else R.PLAIN_CASE
    ang, clean, X, inj = R.refine_case(c)
    rec = TomoGPU(ang, public(X), gpu_id=0)
    kw = dict(leave_one_out=True, loo_iters=c["niter"]) if loo else dict(recon=lambda r: r.sirt(c["niter"], show_convergence=False))
    total = rec.refine_alignment(Nouter=c["nouter"], max_shift=c["max_shift"], subpixel=False, **kw)
    return ang, X, inj, rec, total, R.refine_replay(ang, X, c["nouter"], c["max_shift"], c["niter"], leave_one_out=loo), loo


def test_refine_alignment_follows_the_cpu_replay_pass_by_pass(refine_gpu):
    ang, X, inj, rec, total, (hist, pks, _), loo = refine_gpu
    assert len(rec.align_history) == len(hist)
    for k in range(len(hist)):
        assert np.array_equal(rec.align_peaks[k], pks[k]) and np.array_equal(rec.align_history[k], hist[k]), k
        assert np.array_equal(rec.align_int_peaks[k], pks[k])
    assert np.array_equal(total, hist[-1]) and not np.any(rec.align_at_border)
    assert np.array_equal(rec.get_projections(), public(R.shift_int(X, total)))


def test_refine_alignment_recovers_the_injected_shifts(refine_gpu):
    """subpixel=False on the CPU replays' inputs.  Leave-one-out at 9 projections: the recovered shifts equal the injected ones up to
    the gauge.  The plain form at 31 projections: less than half of the injected misplacement is left on both axes (it stalls at 9
    projections and keeps about a pixel of dr at 31: tests/test_align_cpu.py)."""
    ang, X, inj, rec, total, _, loo = refine_gpu
    before, after = R.gauge_rms(np.zeros_like(total), inj, ang), R.gauge_rms(total, inj, ang)
    print("leave_one_out" if loo else "plain", f"RMS outside the gauge (dr, ds): {before} -> {after}")
    if loo:
        rr, rs = R.gauge_residual(total, inj, ang)
        assert np.abs(rr).max() < 1e-9 and np.abs(rs).max() < 1e-9
    else:
        assert after[0] < 0.5 * before[0] and after[1] < 0.5 * before[1]


def test_refine_alignment_subpixel_lowers_the_data_distance(gpu):
    from tomo_tv_amd.reconstructor import TomoGPU
    ang, clean, X, inj = R.refine_case()
    rec = TomoGPU(ang, public(X), gpu_id=0)
    few = lambda r: r.sirt(R.REFINE_CASE["niter"], show_convergence=False)  # noqa: E731
    few(rec)
    before = rec.tomo.data_distance()
    rec.refine_alignment(Nouter=3, max_shift=8, subpixel=True, leave_one_out=True, loo_iters=R.REFINE_CASE["niter"])
    few(rec)
    after = rec.tomo.data_distance()
    print(f"data distance {before:.4f} -> {after:.4f}")
    assert after < before
    # every refined peak within half a pixel of the whole-pixel maximum of the same window, and the refinement did something
    assert len(rec.align_peaks) == len(rec.align_int_peaks) == 3
    for pk, whole in zip(rec.align_peaks, rec.align_int_peaks):
        assert np.array_equal(whole, np.round(whole)) and np.all(np.abs(pk - whole) <= 0.5)
    assert any(np.any(pk != whole) for pk, whole in zip(rec.align_peaks, rec.align_int_peaks))


def test_device_tensor_series_equals_the_host_path(gpu):
    import torch
    from tomo_tv_amd.reconstructor import TomoGPU
    X = blobs(4, 24, 37, 41)
    sh = np.array([[1.5, -2.25], [0, 3], [-4, 0.5], [2, 2]])
    host = TomoGPU(np.linspace(-60, 60, 4), public(X), gpu_id=0)
    host.set_alignment(sh)
    dev = TomoGPU(np.linspace(-60, 60, 4), torch.from_numpy(public(X)).to("cuda:0"), gpu_id=0)
    dev.set_alignment(sh)
    t = dev.get_projections(as_tensor=True)
    assert t.is_cuda and np.array_equal(t.cpu().numpy(), host.get_projections())
    assert np.array_equal(dev.get_alignment(), sh)
