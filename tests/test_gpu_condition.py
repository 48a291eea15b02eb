"""Conditioning on the GPU through the C ABI, against tests/ref64_condition.py: the median and the gain / offset pass bit for bit, the
sums within their a-priori bounds, the refusals, the TomoGPU drivers and the call sequences.  Shapes (Nslice, Nray, Nproj): below
one wave, exactly one pitch, one slice into the second 64-slice chunk, an odd ray count with three chunks."""
import ctypes

import numpy as np
import pytest

import ref64_condition as R
import sequences as S
import sequences_condition as SC
from test_gpu_align import public
from tomo_tv_amd import _lib, align
from tomo_tv_amd._lib import SINO_B, SINO_G

pytestmark = pytest.mark.gpu
F32 = np.float32
SHAPES = [(5, 16, 3), (64, 16, 3), (65, 16, 3), (130, 9, 2)]
IDS = ["thin5", "pitch64", "chunk65", "odd130x9"]
A_SLOT, D_SLOT, E_SLOT = 3, 4, 5          # TOMO_SINO_USER0 ...
_P = ctypes.c_void_p


def ptr(a):
    return a.ctypes.data_as(_P)


def make_series(P, N, ns, seed):
    """strictly positive samples (no zeros: no tied signed zeros), a different pedestal per projection, a few spikes"""
    rng = np.random.default_rng(seed)
    X = (rng.uniform(0.5, 1.5, (P, N, ns)) + 3.0 * np.arange(1, P + 1)[:, None, None]).astype(F32)
    for a in range(P):
        for r, s in ((0, 0), (N - 1, ns - 1), (N // 2, ns // 2), (N // 2, min(ns // 2 + 1, ns - 1)), (0, ns - 1)):
            X[a, r, s] += F32(25 + a)
    return X


class Case:
    def __init__(self, shape):
        from tomo_tv_amd.engine import tomoengine
        self.ns, self.N, self.P = shape
        self.eng = tomoengine(self.ns, self.N, np.deg2rad(np.linspace(-60, 60, self.P)), device=0)
        self.X = make_series(self.P, self.N, self.ns, 7 * self.ns + self.N)
        self.put(A_SLOT, self.X)

    def put(self, slot, X):
        self.eng.be.c("set_sinogram", slot, ptr(R.packed(np.asarray(X, F32))))

    def get(self, slot):
        return R.images(self.eng._sino(slot), self.N)

    def padding_is_zero(self, slot, spare=E_SLOT):
        """the slot against an upload of its own real samples (an upload writes zero padding), summed over the whole pitch"""
        self.put(spare, self.get(slot))
        self.eng.be.c("sino_diff_norm_sq", slot, spare, 1)
        return self.eng.be.scalars()[1] == 0.0


@pytest.fixture(scope="module", params=SHAPES, ids=IDS)
def case(request, gpu):
    return Case(request.param)


def bits(x):
    return np.ascontiguousarray(x, F32).view(np.uint32)


def check_stats(got, ref, bound, nsums):
    err = np.abs(got[:, :nsums] - ref[:, :nsums])
    print(f"worst error / bound of the sums: {float(np.max(err / np.maximum(bound, 1e-300))):.3f}")
    assert np.all(err <= bound)
    assert np.array_equal(got[:, nsums:], ref[:, nsums:])                                   # counts, or min and max: exact


@pytest.mark.parametrize("radius", [1, 2])
def test_median_measures_and_replaces(case, radius):
    e, X = case.eng, case.X
    sentinel = make_series(case.P, case.N, case.ns, 99)
    case.put(D_SLOT, sentinel)
    st = e.sino_median(A_SLOT, radius=radius)
    check_stats(st, *R.median_stats(X, radius), 3)
    assert np.array_equal(st, e.sino_median(A_SLOT, radius=radius))                         # the same bits from call to call
    assert np.array_equal(bits(case.get(A_SLOT)), bits(X)) and np.array_equal(bits(case.get(D_SLOT)), bits(sentinel))   # a measuring call writes nothing
    th = align.despeckle_thresholds(st, 3.0)
    assert np.array_equal(th, R.despeckle_thresholds(st, 3.0)) and np.all(np.isfinite(th))
    for thresh in (th, np.full(case.P, np.inf, F32), np.zeros(case.P, F32)):
        st = e.sino_median(A_SLOT, D_SLOT, radius=radius, thresh=thresh)
        want, rep = R.replace(X, radius, thresh)
        got = case.get(D_SLOT)
        assert np.array_equal(bits(got), bits(want))
        check_stats(st, *R.median_stats(X, radius, thresh), 3)
        assert np.array_equal(st, e.sino_median(A_SLOT, D_SLOT, radius=radius, thresh=thresh))
        assert case.padding_is_zero(D_SLOT)
        assert np.array_equal(bits(case.get(A_SLOT)), bits(X))
    assert np.array_equal(bits(got), bits(R.median(X, radius)))                             # threshold 0: the median image
    assert rep.sum() == st[:, 4].sum() > 0


def test_window_stats(case):
    N, ns = case.N, case.ns
    for window in ((0, N, 0, ns), (N // 2, N // 2 + 1, ns // 2, ns // 2 + 1), align.background_window(N, ns), (N - 3, N, max(ns - 70, 0), ns)):
        got = case.eng.sino_window_stats(A_SLOT, window)
        check_stats(got, *R.window_stats(case.X, window), 2)
        assert np.array_equal(got, case.eng.sino_window_stats(A_SLOT, window))
    assert np.array_equal(case.eng.sino_window_stats(A_SLOT), case.eng.sino_window_stats(A_SLOT, (0, N, 0, ns)))


@pytest.mark.parametrize("clamp", [False, True])
def test_intensity_is_the_correctly_rounded_fma(case, clamp):
    e, X, P = case.eng, case.X, case.P
    gain = np.array([1.0 + 2.0 ** -12, -0.37, 1.0 / 3.0][:P], F32)
    off = np.array([-1.0, 1.25, -1.7][:P], F32)
    e.sino_intensity(A_SLOT, D_SLOT, gain, off, clamp=clamp)                                # between slots
    want = R.fma32(gain, X, off, clamp)
    assert (want < 0).any() != clamp and (want == 0).any() == clamp                         # the negative gain bites
    assert np.array_equal(bits(case.get(D_SLOT)), bits(want)) and case.padding_is_zero(D_SLOT)
    e.sino_intensity(D_SLOT, D_SLOT, off, gain, clamp=clamp)                                # in place
    assert np.array_equal(bits(case.get(D_SLOT)), bits(R.fma32(off, want, gain, clamp))) and case.padding_is_zero(D_SLOT)
    e.sino_intensity(A_SLOT, D_SLOT, 1.0, 0.0, clamp=clamp)                                 # gain 1, offset 0: a copy
    assert np.array_equal(bits(case.get(D_SLOT)), bits(X)) and np.array_equal(bits(case.get(A_SLOT)), bits(X))


def test_refusals_leave_everything_as_it_was(case):
    from tomo_tv_amd.engine import tomoengine
    L, h, P, N, ns = case.eng.be.L, case.eng.be.h, case.P, case.N, case.ns
    sentinel = make_series(P, N, ns, 98)
    case.put(D_SLOT, sentinel)
    out = np.zeros((P, 5))
    th, go = np.ones(P, F32), np.ones((P, 2), F32)
    neg, nan, inf = th.copy(), th.copy(), go.copy()
    neg[-1], nan[0], inf[-1, 1] = -1.0, np.nan, np.inf
    arg = [L.tomo_sino_window_stats(h, -1, 0, N, 0, ns, ptr(out)), L.tomo_sino_window_stats(h, 43, 0, N, 0, ns, ptr(out)),
           L.tomo_sino_window_stats(h, A_SLOT, 0, N, 0, ns, None), L.tomo_sino_window_stats(h, A_SLOT, 2, 2, 0, ns, ptr(out)),
           L.tomo_sino_window_stats(h, A_SLOT, 0, N, 3, 2, ptr(out)), L.tomo_sino_window_stats(h, A_SLOT, 0, N + 1, 0, ns, ptr(out)),
           L.tomo_sino_window_stats(h, A_SLOT, 0, N, -1, ns, ptr(out)), L.tomo_sino_window_stats(h, A_SLOT, 0, N, 0, ns + 1, ptr(out)),
           L.tomo_sino_median(h, -1, -1, 1, None, ptr(out)), L.tomo_sino_median(h, A_SLOT, 43, 1, ptr(th), ptr(out)),
           L.tomo_sino_median(h, A_SLOT, -1, 1, None, None), L.tomo_sino_median(h, A_SLOT, D_SLOT, 0, ptr(th), ptr(out)),
           L.tomo_sino_median(h, A_SLOT, D_SLOT, 3, ptr(th), ptr(out)), L.tomo_sino_median(h, A_SLOT, D_SLOT, 1, None, ptr(out)),
           L.tomo_sino_median(h, A_SLOT, -1, 1, ptr(th), ptr(out)), L.tomo_sino_median(h, D_SLOT, D_SLOT, 1, ptr(th), ptr(out)),
           L.tomo_sino_median(h, A_SLOT, D_SLOT, 1, ptr(neg), ptr(out)), L.tomo_sino_median(h, A_SLOT, D_SLOT, 2, ptr(nan), ptr(out)),
           L.tomo_sino_intensity(h, A_SLOT, D_SLOT, None, 0), L.tomo_sino_intensity(h, 43, D_SLOT, ptr(go), 0),
           L.tomo_sino_intensity(h, A_SLOT, -1, ptr(go), 0), L.tomo_sino_intensity(h, A_SLOT, D_SLOT, ptr(inf), 1)]
    assert arg == [1] * len(arg) and L.tomo_last_error()
    with pytest.raises(_lib.TomoError, match="error 1"):
        case.eng.sino_median(A_SLOT, D_SLOT, radius=4, thresh=1.0)
    assert np.array_equal(bits(case.get(D_SLOT)), bits(sentinel)) and np.array_equal(bits(case.get(A_SLOT)), bits(case.X))
    # TOMO_ERR_STATE: a slab of a larger volume, then (on an engine of its own) released geometry
    case.eng.be.c("set_slab_edges", 1, 0)
    state = [L.tomo_sino_window_stats(h, A_SLOT, 0, N, 0, ns, ptr(out)), L.tomo_sino_median(h, A_SLOT, D_SLOT, 1, ptr(th), ptr(out)),
             L.tomo_sino_median(h, A_SLOT, -1, 1, None, ptr(out)), L.tomo_sino_intensity(h, A_SLOT, D_SLOT, ptr(go), 0)]
    case.eng.be.c("set_slab_edges", 1, 1)
    assert state == [3] * 4
    assert np.array_equal(bits(case.get(D_SLOT)), bits(sentinel))
    gone = tomoengine(ns, N, np.deg2rad(np.linspace(-60, 60, P)), device=0)
    assert L.tomo_release_geometry(gone.be.h) == 0
    g = gone.be.h
    assert [L.tomo_sino_window_stats(g, A_SLOT, 0, N, 0, ns, ptr(out)), L.tomo_sino_median(g, A_SLOT, -1, 1, None, ptr(out)),
            L.tomo_sino_intensity(g, A_SLOT, D_SLOT, ptr(go), 0)] == [3, 3, 3]
    check = R.median_stats(case.X, 1)                                                       # the engine is usable as before
    check_stats(case.eng.sino_median(A_SLOT, radius=1), *check, 3)


# ---- TomoGPU ------------------------------------------------------------------------------------------------------------------
def driver_spikes():
    """the spikes of the CPU property test that lie outside the background window (a spike inside it enters the background of
    its projection, 40 / 32 per sample here, and leaves that projection with a negative mass)"""
    from test_condition_cpu import SPIKES
    _, r1, _, s1 = align.background_window(32, 16)
    return [(a, r, s) for a, r, s in SPIKES if not (r < r1 and s < s1)]


@pytest.fixture(scope="module")
def spiked():
    from test_condition_cpu import SPIKE, spiked_series
    X = spiked_series()[0].copy()                                                           # X[a][r][s]: 9 x 32 x 16, noisy, no spikes yet
    for a, r, s in driver_spikes():
        X[a, r, s] += F32(SPIKE)
    return X


def tomo(X, tensor=False):
    from tomo_tv_amd.reconstructor import TomoGPU
    pub = public(X)
    if tensor:
        import torch
        pub = torch.from_numpy(pub).to("cuda:0")
    return TomoGPU(np.linspace(-60, 60, len(X)), pub, gpu_id=0)


def test_condition_and_alignment_commute(gpu, spiked):
    a = tomo(spiked)
    sh = a.align_center_of_mass()
    out_a = a.condition(n_sigma=12.0)
    b = tomo(spiked)
    out_b = b.condition(n_sigma=12.0)
    b.set_alignment(sh, wrap=True)
    assert sh.any() and out_a["replaced"].sum() >= len(driver_spikes()) == 12
    assert np.array_equal(bits(a.get_projections()), bits(b.get_projections()))
    for k in out_a:
        assert np.array_equal(out_a[k], out_b[k]), k
    c = tomo(spiked, tensor=True)                                                            # a device tensor goes through the same calls
    c.align_center_of_mass()
    c.condition(n_sigma=12.0)
    t = c.get_projections(as_tensor=True)
    assert t.is_cuda and np.array_equal(bits(t.cpu().numpy()), bits(a.get_projections()))
    assert np.all(out_a["replaced"] >= np.bincount([a for a, _, _ in driver_spikes()], minlength=9))     # every injected spike, at least


def test_drivers_rules_and_record(gpu, spiked):
    rec = tomo(spiked)
    t = rec.tomo
    bg = rec.subtract_background()
    ref_bg = R.subtract_background(spiked)[1]
    assert np.allclose(bg, ref_bg, rtol=2.0 ** -23, atol=0) and rec.recon is None
    # a second pass finds what rounding left: each sample moved by at most half an ulp of itself, the offset by half an ulp of the mean
    again = rec.subtract_background()
    print(f"second background: largest {np.abs(again).max():.3e}")
    assert np.all(np.abs(again) <= 2.0 ** -23 * np.abs(spiked).max())
    counts = rec.despeckle(n_sigma=12.0)
    gains = rec.normalize_intensity()
    with pytest.raises(ValueError):
        rec.normalize_intensity(mode="median")
    kept = R.images(t._sino(rec.ALIGN_SLOT), 32).astype(np.float64)
    mass, mag = kept.sum((1, 2)), np.abs(kept).sum((1, 2))
    # the gain is rounded to binary32 (2^-24 of the mass) and so is every product (2^-24 of sum |x|): 2^-23 sum |x| against the
    # common target, twice that between a mass and the mean of all
    spread = np.abs(mass - mass.mean())
    print(f"masses after normalising: spread / bound {np.max(spread) / (2.0 ** -22 * mag.max()):.3f}")
    assert np.all(spread <= 2.0 ** -22 * mag.max())
    c = rec.conditioning
    assert np.array_equal(c["replaced"], counts) and np.array_equal(c["gain"], gains)
    off = -(bg.astype(F32).astype(np.float64) + again.astype(F32).astype(np.float64))
    assert np.allclose(c["offset"], gains * off, rtol=1e-15, atol=0)
    more = rec.despeckle(n_sigma=12.0, passes=2)
    assert np.array_equal(rec.conditioning["replaced"], counts + more)
    assert np.array_equal(bits(rec.get_projections()), bits(public(R.images(t._sino(rec.ALIGN_SLOT), 32))))   # no alignment: B is the kept copy
    rec.set_tilt_series(public(spiked))
    assert not rec.conditioning["replaced"].any() and np.all(rec.conditioning["gain"] == 1)


# ---- call sequences -----------------------------------------------------------------------------------------------------------
def _engine(gid):
    import test_gpu_sequences as G
    return G.engine(gid)


@pytest.mark.parametrize("gid", ["A", "C"])
def test_used_engine_gives_a_fresh_engines_bits(gpu, gid):
    want = SC.condition_calls(_engine(gid))
    e = _engine(gid)
    e.restart_recon()
    e.SIRT(2)
    S.align_calls(e)
    got = SC.condition_calls(e)
    assert got.keys() == want.keys()
    for k in want:
        assert np.array_equal(got[k], want[k]), k
    again = SC.condition_calls(e)
    for k in want:
        assert np.array_equal(again[k], want[k]), k
    X = R.images(e._sino(SINO_B), e.Ny)                                                      # ... and the right answer, not only a repeatable one
    assert np.array_equal(bits(R.images(want["median2"], e.Ny)), bits(R.replace(X, 2, (F32(0.02) * (1 + np.arange(e.Nproj))).astype(F32))[0]))


def test_the_new_calls_leave_a_later_sirt_run_alone(gpu):
    """After a cost evaluation G is the projection of RECON and the next SIRT step starts from it.  Calls that only read G keep that;
    a call that writes G must drop it, or the step would start from the overwritten G."""
    out = []
    for used in (True, False):
        e = _engine("C")
        e.restart_recon()
        e.SIRT(2)
        e.data_distance()
        if used:
            SC.condition_calls(e)
            e.sino_median(SINO_G, radius=1)
            e.sino_window_stats(SINO_G)
            e.sino_intensity(SINO_G, SC.SINO_USER0 + 9, 2.0, 1.0)
            mid = e.get_volume()
            e.SIRT(1)
            first = e.get_volume()
            e.data_distance()
            e.sino_intensity(SINO_B, SINO_G, 2.0, 1.0)                                      # G is the destination: the claim goes
            e.sino_median(SINO_B, SINO_G, radius=1, thresh=0.0)
        else:
            mid = e.get_volume()
            e.SIRT(1)
            first = e.get_volume()
            e.data_distance()
        e.SIRT(1)
        out.append((mid, first, e.get_volume(), e.data_distance()))
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1]) and np.array_equal(out[0][2], out[1][2])
    assert out[0][3] == out[1][3] and np.abs(out[0][2]).max() > 0
