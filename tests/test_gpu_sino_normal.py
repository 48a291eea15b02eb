"""``tomo_sino_affine_normal`` on the GPU: the 21 sums of every projection against the binary64 statement inside their bounds
(tests/ref64_sino_normal.py), the exact count, the copy property of whole-pixel maps, the same bits from call to call and under pending
work, nothing written and no claim dropped, the empty overlap, Inf and NaN outside the counting set, every refusal, the Gauss-Newton
loop against its CPU replay and ``TomoGPU.refine_alignment_affine`` end to end.
Shapes (Nslice, Nray, P): (70, 33, 5) two 64-slice chunks with 58 padding slices, three row blocks, the last with one row; (256, 40, 4)
four chunks, three row blocks; (5, 24, 2) thinner than a wave; (64, 16, 3) one full chunk, one row block."""
import ctypes

import numpy as np
import pytest

import ref64_affine as RF
import ref64_align as RA
import ref64_sino_normal as SN
import sequences_affine3d  # noqa: F401
import sequences_register3d  # noqa: F401
import sequences_sino_normal  # noqa: F401  (registers this feature's row of the call-sequence closure table)
from test_sino_normal_cpu import recovery, smooth

pytestmark = pytest.mark.gpu

SHAPES = [(70, 33, 5), (256, 40, 4), (5, 24, 2), (64, 16, 3)]
IDS = ["pad58", "chunks4", "thin5", "chunk1"]
F_SLOT, G_SLOT, X_SLOT, Y_SLOT = 3, 4, 5, 6          # TOMO_SINO_USER0 ...
SINO_B, SINO_G = 0, 1
ARG, STATE = 1, 3
IDENT = np.array([1.0, 0, 0, 0, 1.0, 0])


def engine(ns, N, P):
    from tomo_tv_amd.engine import tomoengine
    return tomoengine(ns, N, np.deg2rad(np.linspace(-60, 60, P)), device=0)


def public(X):
    """X[a][r][s] -> the (Nslice, Nray, Nangles) array TomoGPU is given"""
    return np.ascontiguousarray(np.asarray(X).transpose(2, 1, 0))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def put(eng, slot, X):
    b = RA.packed(np.asarray(X, np.float32))
    eng.be.c("set_sinogram", slot, b.ctypes.data_as(ctypes.c_void_p))


def get(eng, slot):
    return RA.images(eng._sino(slot), eng.Ny)


def raw(eng, fixed, moving, M, margin):
    """the (P, 21) sums as the C call writes them"""
    from tomo_tv_amd import _lib
    m, out = np.ascontiguousarray(M, np.float64), np.full((eng.Nproj, 21), np.nan)
    _lib.check(_lib.load().tomo_sino_affine_normal(eng.be.h, fixed, moving, m.ctypes.data_as(ctypes.c_void_p), int(margin),
                                                   out.ctypes.data_as(ctypes.c_void_p)))
    return out


class Case:
    def __init__(self, shape):
        self.ns, self.N, self.P = shape
        self.eng = engine(*shape)
        self.F, self.G = smooth(self.P, self.N, self.ns, 17 + self.N), smooth(self.P, self.N, self.ns, 18 + self.N)
        put(self.eng, F_SLOT, self.F), put(self.eng, G_SLOT, self.G)

    def maps(self, which=0):
        """One map per projection, all different, out of: the identity, a whole-pixel shift, a general map (1.3 degrees, 1.02, a
        fractional shift), a map that pushes part of the taps outside G, a second general map.  Set 0 puts the general and the outside
        map first, set 1 the identity and the whole-pixel shift: between them every shape, the two-projection one included, sees all
        four kinds.  -> (the maps, the index of the outside map or None)"""
        N, ns = self.N, self.ns
        M = [IDENT.copy(), np.array([1.0, 0, -1, 0, 1.0, 1]), RF.matrices([[0.3, -0.6]], 1.3, 1.02, N, ns)[0],
             RF.matrices([[0.35 * N, -0.2 * ns]], -2.0, 0.9, N, ns)[0], RF.matrices([[-0.7, 0.45]], -0.8, 0.99, N, ns)[0]]
        order = ([2, 3, 1, 0, 4] if which == 0 else [0, 1, 4, 3, 2])[:self.P]
        return np.array([M[k] for k in order]), (order.index(3) if 3 in order else None)


@pytest.fixture(scope="module", params=list(zip(SHAPES, IDS)), ids=IDS)
def case(request, gpu):
    return Case(request.param[0])


def usable(eng):
    """the engine still reconstructs: one Landweber step gives a finite, non-zero volume"""
    eng._set_sino_local(np.abs(RA.packed(smooth(eng.Nproj, eng.Ny, eng.Nslice_, 3))))
    eng.restart_recon()
    eng.be.c("sirt_landweber", 0, 1.0 / eng.get_lipschitz(), 1)
    x = eng.get_volume(0)
    assert np.isfinite(x).all() and x.any()


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("margin", [0, 1, 2])
def test_sums_against_binary64(case, margin, which):
    M, outside = case.maps(which)
    ref, bnd, summ = SN.bound(case.F, case.G, M, margin)
    got = raw(case.eng, F_SLOT, G_SLOT, M, margin)
    r = SN.ratios(got, ref, bnd)
    print(f"{(case.ns, case.N, case.P)}, map set {which}, margin {margin}: worst error / bound per projection {np.round(r.max(axis=1), 4)}, "
          f"samples that count {ref[:, 15].astype(int)} of {case.N * case.ns}")
    assert np.array_equal(got[:, 15], ref[:, 15]) and np.all(ref[:, 15] > 0)               # the count is exact
    assert r.max() <= 1.0, (margin, np.unravel_index(int(r.argmax()), r.shape), r.max())
    if outside is not None:                                                               # the map that leaves G does cut samples
        assert ref[outside, 15] < SN.bound(case.F, case.G, np.tile(IDENT, (case.P, 1)), margin)[0][outside, 15]
    assert which == 0 or np.all(M[:2] == np.round(M[:2]))                                 # set 1: the copy paths at every shape
    for a in range(case.P):                                                               # w copies samples: the summation term alone
        if np.all(M[a] == np.round(M[a])):
            assert np.all(np.abs(got[a, 16:] - ref[a, 16:]) <= summ[a, 16:]), a
    if margin == 1:                                                                       # the Python call unpacks the same numbers
        H, b, ssd, count, ncc = case.eng.sino_affine_normal(F_SLOT, G_SLOT, M, margin=1)
        H2, b2, ssd2, count2, ncc2 = SN.unpack(got)
        assert np.array_equal(H, H2) and np.array_equal(H, H.transpose(0, 2, 1)) and np.array_equal(b, b2) and np.array_equal(ssd, ssd2)
        assert np.array_equal(count, count2) and np.allclose(ncc, ncc2, rtol=1e-13, atol=0)


def test_a_fraction_that_rounds_to_one_is_the_next_whole_pixel(case):
    """The identity moved by -2^-30 on both axes: the coordinates of row 0 and slice 0 lie just below 0, their fractions round to 1 in
    binary32, so they are pixel 0 with t = 0 and count; every sample is a copy.  The sums that do not hold q are the identity's bits."""
    tiny = np.tile([1.0, 0, -2.0 ** -30, 0, 1.0, -2.0 ** -30], (case.P, 1))
    got, ident = raw(case.eng, F_SLOT, G_SLOT, tiny, 0), raw(case.eng, F_SLOT, G_SLOT, np.tile(IDENT, (case.P, 1)), 0)
    assert np.all(got[:, 15] == (case.N - 1) * (case.ns - 1))
    assert np.array_equal(got[:, 14:].view(np.uint64), ident[:, 14:].view(np.uint64))
    assert np.array_equal(got[:, [0, 1, 4, 10, 11]].view(np.uint64), ident[:, [0, 1, 4, 10, 11]].view(np.uint64))      # g only


def test_one_projection_without_a_counting_sample(case):
    """that projection is all +0.0, the others are unchanged bit for bit"""
    M, _ = case.maps()
    base = raw(case.eng, F_SLOT, G_SLOT, M, 1)
    for a in (0, case.P - 1):
        Mo = M.copy()
        Mo[a] = RF.matrices([[3.0 * max(case.N, case.ns), 0.0]], 1.3, 1.02, case.N, case.ns)[0]
        out = raw(case.eng, F_SLOT, G_SLOT, Mo, 1)
        assert not out[a].view(np.uint64).any()                                            # every sum +0.0: no NaN, no -0.0
        keep = np.arange(case.P) != a
        assert np.array_equal(out[keep].view(np.uint64), base[keep].view(np.uint64))
    none = raw(case.eng, F_SLOT, G_SLOT, np.tile([1.0, 0, 0, 0, 1.0, -2.0 * case.ns], (case.P, 1)), 0)
    assert not none.view(np.uint64).any()


def test_repeats_bit_for_bit_and_changes_nothing(case):
    M, _ = case.maps()
    first = raw(case.eng, F_SLOT, G_SLOT, M, 1)
    again = raw(case.eng, F_SLOT, G_SLOT, M, 1)
    assert np.array_equal(first.view(np.uint64), again.view(np.uint64))
    # next to other calls of the alignment family, which share the partial-sum buffers
    case.eng.sino_xcorr(F_SLOT, G_SLOT, 2)
    case.eng.sino_moments(G_SLOT)
    third = raw(case.eng, F_SLOT, G_SLOT, M, 1)
    case.eng.sino_axis_profile(F_SLOT)
    assert np.array_equal(first.view(np.uint64), third.view(np.uint64))
    assert np.array_equal(bits(get(case.eng, F_SLOT)), bits(case.F)) and np.array_equal(bits(get(case.eng, G_SLOT)), bits(case.G))
    # fixed == moving with the identity: no residual at all
    same = raw(case.eng, G_SLOT, G_SLOT, np.tile(IDENT, (case.P, 1)), 0)
    assert np.all(same[:, 15] == (case.N - 1) * (case.ns - 1)) and not same[:, 14].any() and not same[:, 10:14].any()
    assert np.array_equal(same[:, 16], same[:, 17]) and np.array_equal(same[:, 16], same[:, 18]) and np.array_equal(same[:, 19], same[:, 20])


def test_claim_survives(gpu):
    """G = A * RECON in hand (a data distance), then the sums with the model sinogram as F and the series as G: the next data distance
    is that of an engine that was left alone, bit for bit (it does not project again), and so is the step after it."""
    ns, N, P = 40, 24, 5
    e, f = engine(ns, N, P), engine(ns, N, P)
    b = np.abs(RA.packed(smooth(P, N, ns, 61)))
    X = np.abs(np.random.default_rng(62).random((ns, N, N), dtype=np.float32))
    for eng in (e, f):
        eng._set_sino_local(b)
        eng.set_volume(X, 0)
        eng.data_distance()
    recon = bits(e.get_volume(0))
    out = raw(e, SINO_G, SINO_B, np.tile(IDENT, (P, 1)), 1)
    assert np.all(out[:, 15] == (N - 2) * (ns - 2)) and np.isfinite(out).all() and out[:, 14].all()
    assert e.data_distance() == f.data_distance()
    assert np.array_equal(bits(e.get_volume(0)), recon) and np.array_equal(bits(e._sino(SINO_B)), bits(f._sino(SINO_B)))
    assert np.array_equal(bits(e._sino(SINO_G)), bits(f._sino(SINO_G)))
    t = 1.0 / e.get_lipschitz()
    e.be.c("sirt_landweber", 0, t, 1), f.be.c("sirt_landweber", 0, t, 1)
    assert np.array_equal(bits(e.get_volume(0)), bits(f.get_volume(0)))


@pytest.mark.parametrize("kind", ["snapshot", "dd_begin"])
def test_while_work_is_pending(gpu, kind):
    """as tomo_sino_xcorr (tests/test_gpu_sequences.py, section (d)): neither side refuses, both deliver what the un-interleaved order
    delivers, and the engine goes on as its twin"""
    ns, N, P = 40, 24, 5
    b = np.abs(RA.packed(smooth(P, N, ns, 61)))
    M = RF.matrices(np.tile([0.3, -0.6], (P, 1)), 1.3, 1.02, N, ns)

    def begin(e):
        e._set_sino_local(b)
        e.restart_recon()
        e.SIRT(2)
        if kind == "snapshot":
            e.data_distance()
            e.be.scalars_snapshot()
            return lambda: e.be.scalars_snapshot_read()
        e.data_distance_begin()
        return lambda: (e.data_distance_end(),)
    x, y = engine(ns, N, P), engine(ns, N, P)
    finish = begin(x)
    red_x = raw(x, SINO_G, SINO_B, M, 1)                               # while the item is pending
    pend_x = finish()
    finish = begin(y)
    pend_y = finish()                                                  # the un-interleaved order
    red_y = raw(y, SINO_G, SINO_B, M, 1)
    assert np.allclose(np.asarray(pend_x, np.float64), np.asarray(pend_y, np.float64), rtol=1e-10, atol=0), (pend_x, pend_y)
    assert np.array_equal(red_x.view(np.uint64), red_y.view(np.uint64)) and red_x[:, 15].all()
    x.SIRT(1), y.SIRT(1)
    assert np.array_equal(bits(x.get_volume(0)), bits(y.get_volume(0)))


def test_inf_and_nan_outside_the_counting_set_stay_out(case):
    """p = x + (2, 1): the rows r' < 2 and the slices s' < 1 of G (one more each with margin 1) hold no tap of a counting sample, and
    the border of F lies in the margin."""
    M = np.tile([1.0, 0, 2, 0, 1.0, 1], (case.P, 1))
    clean = raw(case.eng, F_SLOT, G_SLOT, M, 1)
    Fv, Gv = case.F.copy(), case.G.copy()
    Gv[:, 0], Gv[:, 1, ::2], Gv[:, 2, 1::2], Gv[:, :, 0], Gv[:, 3::2, 1] = np.inf, np.nan, -np.inf, np.nan, np.inf
    Fv[:, 0], Fv[:, -1], Fv[:, :, 0], Fv[:, 1::2, -1] = np.nan, np.inf, -np.inf, np.nan
    Fv[:, case.N - 3:], Fv[:, :, case.ns - 2:] = np.nan, np.inf           # x with r + 3 > N - 1 or s + 2 > ns - 1 does not count either
    put(case.eng, X_SLOT, Fv), put(case.eng, Y_SLOT, Gv)
    got = raw(case.eng, X_SLOT, Y_SLOT, M, 1)
    assert np.isfinite(got).all() and np.all(got[:, 15] > 0) and np.array_equal(got.view(np.uint64), clean.view(np.uint64))


def test_refusals_leave_the_engine_usable(gpu):
    from tomo_tv_amd import _lib
    from tomo_tv_amd.engine import tomoengine
    L = _lib.load()
    c = Case((9, 12, 3))
    h = c.eng.be.h
    I = np.tile(IDENT, (3, 1))
    ok = I.ctypes.data_as(ctypes.c_void_p)
    out = np.full((3, 21), -1.0)
    o = out.ctypes.data_as(ctypes.c_void_p)
    bad = [I.copy() for _ in range(3)]
    bad[0][0, 2], bad[1][1, 0], bad[2][2, 5] = np.nan, np.inf, -np.inf

    def call(e=h, fx=F_SLOT, mv=G_SLOT, m=ok, margin=1, dst=o):
        return L.tomo_sino_affine_normal(e, fx, mv, m, margin, dst)
    calls = [call(e=None), call(fx=-1), call(fx=43), call(mv=-1), call(mv=43), call(m=None), call(dst=None), call(margin=-1),
             call(margin=5), call(margin=6)]                                      # 2 * 5 >= 9 slices; 2 * 6 >= 12 rays
    calls += [call(m=m.ctypes.data_as(ctypes.c_void_p)) for m in bad]
    assert calls == [ARG] * len(calls) and L.tomo_last_error()
    with pytest.raises(ValueError):
        c.eng.sino_affine_normal(F_SLOT, G_SLOT, I, margin=5)
    c.eng.be.c("set_slab_edges", 1, 0)                                           # a slab of a larger volume
    assert call() == STATE and b"slab" in L.tomo_last_error()
    c.eng.be.c("set_slab_edges", 1, 1)
    with pytest.raises(NotImplementedError):                                     # the sharded classes refuse in Python already
        tomoengine(8, 12, np.deg2rad(np.linspace(-60, 60, 3)), device=0, sub_slabs=2).sino_affine_normal(F_SLOT, G_SLOT, I)
    gone = engine(9, 12, 3)
    assert L.tomo_release_geometry(gone.be.h) == 0
    assert call(e=gone.be.h) == STATE and b"released" in L.tomo_last_error()
    assert np.all(out == -1.0)                                                   # no refused call wrote anything
    assert call(margin=4) == 0 and np.all(out[:, 15] == 1 * 4)                   # 2 * 4 < 9: the largest margin is taken: slice 4, rows 4 .. 7
    assert np.array_equal(bits(get(c.eng, F_SLOT)), bits(c.F)) and np.array_equal(bits(get(c.eng, G_SLOT)), bits(c.G))
    usable(c.eng)


def test_refuses_an_engine_with_a_communicator(gpu):
    """A one-rank RCCL communicator bound through the C ABI, in a fresh child process like the other one-rank tests."""
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(here, "sino_normal_comm_script.py")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "SINO_NORMAL_COMM_REFUSED_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ---- the loop --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SN.RECOVERY_SHAPES)
def test_loop_agrees_with_the_cpu_replay(gpu, shape):
    """The recovery fixture of tests/test_sino_normal_cpu.py, 8 iterations with all tolerances 0 (every run takes all 8, past
    convergence: the replay converges in 4).  The yardstick is measured here, on the CPU alone: the loop in binary64 against the loop
    with the binary32 replay in place of the statement -- the distance a faithful binary32 evaluation of the 21 sums puts between two
    runs of the same loop; the fixed point is stable (the loop contracts), so rounding differences of single evaluations do not
    accumulate, and the device's final maps may lie twice that far from the binary64 loop's.  Recorded: the figures printed
    below."""
    from tomo_tv_amd.align import match_projections
    c = recovery(shape)
    ns, N, P = shape
    kw = dict(max_iter=8, tol_shift=0.0, tol_deg=0.0, tol_mag=0.0, margin=2)
    M64, _ = SN.gauss_newton(c["F"], c["G"], **kw)
    M32, _ = SN.gauss_newton(c["F"], c["G"], sums=SN.normal_replay_f32, **kw)
    allow = 2.0 * float(np.max(np.abs(M64 - M32)))
    eng = engine(ns, N, P)
    put(eng, F_SLOT, c["F"]), put(eng, G_SLOT, c["G"])
    res = match_projections(eng, F_SLOT, G_SLOT, **kw)
    dist = float(np.max(np.abs(res["M"] - M64)))
    err = SN.recovery_error(res["M"], c["truth"], N, ns)
    print(f"{shape}: final maps, worst entry: binary64 loop against the binary32 replay {0.5 * allow:.3e}; device against the binary64 loop "
          f"{dist:.3e}; device against the truth: {err[0]:.3e} px, {err[1]:.3e} degrees, {err[2]:.3e} in magnification")
    assert allow > 0 and dist <= allow
    assert len(res["step"]) == 8 and len(res["ssd"]) == 8 and not res["converged"].any() and np.all(res["count"][-1] > N * ns // 8)
    # the default tolerances stop early and end where the replay with the default tolerances ends, to the shift tolerance
    quick = match_projections(eng, F_SLOT, G_SLOT, margin=2)
    assert quick["converged"].all() and len(quick["step"]) <= len(c["hist"]["step"]) + 1
    assert np.max(np.abs(quick["M"] - c["M"])) <= 1e-3
    assert np.allclose(RF.matrices(quick["shift"], quick["rotation_deg"], quick["magnification"], N, ns), quick["M"], rtol=0, atol=1e-10)
    far = SN.identity(P)
    far[P - 1, 2] = 0.95 * N
    with pytest.raises(RuntimeError, match=rf"projections \[{P - 1}\]"):
        match_projections(eng, F_SLOT, G_SLOT, M0=far, margin=2)


# ---- the driver ------------------------------------------------------------------------------------------------------------------------
def test_refine_alignment_affine_end_to_end(gpu):
    """``ref64_sino_normal.DRIVER_CASE``: the geometry of tests/golden/A_N32_P9.npz, the phantom of the alignment tests, every projection
    distorted by its own shift, rotation and magnification; three leave-one-out passes.  The distance to the truth modulo the gauges
    (``driver_distance``, pixels at the image border) falls from pass to pass and ends below 1.25 times what the twin run of the
    binary64 replay reaches: the two runs differ by the binary32 rounding of the device's SIRT, projector and resampling against the
    oracle's (relative 1e-6 of the model), which moves a minimum that is located to a few hundredths of a pixel by far less than a
    quarter of the replay's own remaining distance.  Recorded: the figures printed below."""
    from tomo_tv_amd.reconstructor import TomoGPU
    c = SN.DRIVER_CASE
    ang, clean, X, Md = SN.driver_case()
    P, N, ns = X.shape
    rec = TomoGPU(ang, public(X), gpu_id=0)
    sh, rot, mag = rec.refine_alignment_affine(Nouter=c["nouter"], leave_one_out=True, loo_iters=c["loo_iters"])
    twin = SN.driver_replay(ang, X, c["nouter"], c["loo_iters"])
    start = SN.driver_distance(np.zeros((P, 2)), np.zeros(P), np.ones(P), Md, ang, N, ns)
    dev = [SN.driver_distance(*h, Md, ang, N, ns) for h in rec.align_affine_history]
    cpu = [SN.driver_distance(*h, Md, ang, N, ns) for h in twin]
    print(f"distance to the truth in border pixels: start {start:.4f}; device per pass {np.round(dev, 4)}; binary64 replay {np.round(cpu, 4)}")
    assert len(dev) == c["nouter"] and all(b < a for a, b in zip([start] + dev, dev))
    assert dev[-1] <= 1.25 * cpu[-1]
    # what was estimated is what is stored and applied: the series as given, resampled once
    r2, m2 = rec.get_alignment_rotation()
    assert np.array_equal(rot, r2) and np.array_equal(mag, m2) and np.array_equal(sh, rec.get_alignment()) and rot.any() and np.any(mag != 1.0)
    assert abs(rot.mean()) < 1e-12 and abs(np.log(mag).mean()) < 1e-12 and abs(sh[:, 1].mean()) < 1e-12           # the gauges
    assert np.array_equal(bits(RA.images(rec.tomo._sino(rec.ALIGN_SLOT), N)), bits(X))
    from tomo_tv_amd.align import affine_matrices
    M = affine_matrices(sh.astype(np.float32).astype(np.float64), rot, mag, N, ns)
    got = RA.images(rec.tomo._sino(SINO_B), N)
    assert np.all(np.abs(got - RF.affine(X, M)[0]) <= RF.bound(X, M))
    assert len(rec.align_affine_cost) == c["nouter"] and all(len(k["ssd"]) == len(k["ncc"]) for k in rec.align_affine_cost)
    # shifts only: the stored rotation and magnification stay bit-identical
    rec.refine_alignment_affine(Nouter=1, rotation=False, magnification=False, leave_one_out=True, loo_iters=5)
    r3, m3 = rec.get_alignment_rotation()
    assert r3.tobytes() == rot.tobytes() and m3.tobytes() == mag.tobytes() and np.any(rec.get_alignment() != sh)
    # a new series drops the estimate
    rec.set_tilt_series(public(X))
    r4, m4 = rec.get_alignment_rotation()
    assert not r4.any() and np.all(m4 == 1.0) and not rec.get_alignment().any()
    fresh = TomoGPU(ang, public(X), gpu_id=0)
    fresh.refine_alignment_affine(Nouter=1, rotation=False, magnification=False, leave_one_out=True, loo_iters=5)
    assert fresh._align_rot is None                                                   # nothing stored where nothing was estimated
