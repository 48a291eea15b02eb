"""``tomo_volume_affine_normal`` on the GPU: the 32 sums against the binary64 statement inside their bounds
(tests/ref64_register3d.py), the exact count, the copy property of whole-voxel maps, the same bits from call to call and next to other
calls, nothing written and no claim dropped, the empty overlap, Inf and NaN outside the counting set, every refusal, the
Gauss-Newton loop against its CPU replay and ``DualAxisTomo.estimate_registration`` on the realistic case.
Shapes (those of test_gpu_affine3d.py): cubes of N = 8 (one partial lane group), 40, 70 (two lane groups, one partial), 130 (three
lane groups, more blocks of rows than workgroups: the capped grid), and the unequal pair 5 x 12^2 (moving) against 9 x 10^2 (fixed)."""
import ctypes

import numpy as np
import pytest

import ref64_dual as D
import ref64_register3d as G3
import sequences_affine3d  # noqa: F401
import sequences_register3d  # noqa: F401  (registers this feature's row of the call-sequence closure table)
from test_bin_cpu import mixed
from test_register3d_cpu import exact_case, realistic, smooth

pytestmark = pytest.mark.gpu

SHAPES = [((8, 8, 8), (8, 8, 8)), ((40, 40, 40), (40, 40, 40)), ((70, 70, 70), (70, 70, 70)), ((130, 130, 130), (130, 130, 130)),
          ((5, 12, 12), (9, 10, 10))]
FLAT = (8, 48, 48)                            # 8 slices x 48 x 48: 288 blocks of AF_ROWS rows, so 288 workgroups' rows for the 256 threads of the second stage
V0, V1, V2 = 5, 6, 7                          # TOMO_VOL_USER0 ..
ANG_A, ANG_B = np.linspace(-60, 60, 2), np.linspace(-50, 40, 3)
ARG, STATE = 1, 3
IDENT = np.eye(3, 4).ravel()


def engine(ns, N, ang):
    from tomo_tv_amd.engine import tomoengine
    return tomoengine(ns, N, np.deg2rad(ang), device=0)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def raw(fixed, fv, moving, mv, M, margin):
    """the 32 sums as the C call writes them"""
    from tomo_tv_amd import _lib
    m, out = np.ascontiguousarray(M, np.float64), np.full(32, np.nan)
    _lib.check(_lib.load().tomo_volume_affine_normal(fixed.be.h, fv, moving.be.h, mv, m.ctypes.data_as(ctypes.c_void_p), int(margin),
                                                     out.ctypes.data_as(ctypes.c_void_p)))
    return out


class Pair:
    """a: the moving engine (G, slot V0); b: the fixed engine (F, slot V1); twin: an engine of a's size (b itself for the cubes)"""
    def __init__(self, src, dst):
        self.src, self.dst, self.same = src, dst, src == dst
        self.a, self.b = engine(src[0], src[1], ANG_A), engine(dst[0], dst[1], ANG_B)
        self.Fv, self.Gv = smooth(dst, 17), smooth(src, 18)
        self.b.set_volume(self.Fv, V1), self.a.set_volume(self.Gv, V0)

    def maps(self):
        from tomo_tv_amd.align import affine_matrix_3d
        kw = dict(src_shape=self.src, dst_shape=self.dst)
        return {"identity": IDENT.copy(), "whole-voxel shift": np.array([1, 0, 0, -1, 0, 1, 0, 1, 0, 0, 1, 0], np.float64),
                "general": affine_matrix_3d((7.3, -11.0, 4.0), shift=(0.3, -0.6, 0.9), **kw)}


@pytest.fixture(scope="module", params=SHAPES, ids=[f"{s[0]}x{s[1]}_onto_{d[0]}x{d[1]}" for s, d in SHAPES])
def pair(request, gpu):
    return Pair(*request.param)


def usable(p):
    """both engines still reconstruct: one Landweber step each gives a finite, non-zero volume"""
    for eng, ang, shp in ((p.a, ANG_A, p.src), (p.b, ANG_B, p.dst)):
        eng._set_sino_local(np.abs(mixed((shp[0], shp[1] * len(ang)), 3)))
        eng.restart_recon()
        eng.be.c("sirt_landweber", 0, 1.0 / eng.get_lipschitz(), 1)
        x = eng.get_volume(0)
        assert np.isfinite(x).all() and x.any()


@pytest.mark.parametrize("name", ["identity", "whole-voxel shift", "general"])
def test_sums_against_binary64(pair, name):
    """Every shape, every map, the margins 0, 1 and 3.  The per-voxel quantities of the statement and of its bound do not depend on the
    margin, so the host forms them once per map (``ref64_register3d.evaluate``) and every margin takes its slice."""
    M = pair.maps()[name]
    worst = 0.0
    for margin, (ref, bnd, summ) in G3.evaluate(pair.Fv, pair.Gv, M, (0, 1, 3)).items():
        got = raw(pair.b, V1, pair.a, V0, M, margin)
        r = G3.ratios(got, ref, bnd)
        worst = max(worst, float(r.max()))
        assert got[28] == ref[28] and ref[28] > 0, (name, margin)                         # the count is exact
        assert r.max() <= 1.0, (name, margin, int(r.argmax()), r.max())
        if name != "general":                                                           # w copies samples: the summation term alone
            assert np.all(np.abs(got[29:] - ref[29:]) <= summ[29:]), (name, margin)
        if name == "identity" and margin == 1:                                           # the Python call unpacks the same numbers
            H, b, ssd, count, ncc = pair.b.volume_affine_normal(pair.a, M, margin=1, fixed_vol=V1, moving_vol=V0)
            H2, b2, ssd2, count2, ncc2 = G3.unpack(got)
            assert np.array_equal(H, H2) and np.array_equal(H, H.T) and np.array_equal(b, b2) and (ssd, count, ncc) == (ssd2, count2, ncc2)
    print(f"{pair.src} onto {pair.dst}, {name}: worst error / bound over the margins and the 32 sums {worst:.4f}")


def test_sums_with_more_rows_than_threads_in_the_second_stage(gpu):
    """``FLAT`` against itself: the smallest pair at which a thread of the second stage adds more than one of the workgroups' rows with
    few voxels per workgroup.  The statement and the bounds of test_sums_against_binary64, margins 0 and 1."""
    p = Pair(FLAT, FLAT)
    for name, M in p.maps().items():
        for margin, (ref, bnd, summ) in G3.evaluate(p.Fv, p.Gv, M, (0, 1)).items():
            got = raw(p.b, V1, p.a, V0, M, margin)
            r = G3.ratios(got, ref, bnd)
            assert got[28] == ref[28] and ref[28] > 0 and r.max() <= 1.0, (name, margin, int(r.argmax()), r.max())
            if name != "general":
                assert np.all(np.abs(got[29:] - ref[29:]) <= summ[29:]), (name, margin)
        assert np.array_equal(got.view(np.uint64), raw(p.b, V1, p.a, V0, M, margin).view(np.uint64))


def test_one_engine_with_two_slots_equals_two_engines(pair):
    """F and a moving volume of F's size in two slots of the fixed engine, against the same moving volume on an engine of its own"""
    from tomo_tv_amd.align import affine_matrix_3d
    G2 = smooth(pair.dst, 19)
    other = engine(pair.dst[0], pair.dst[1], ANG_A)
    pair.b.set_volume(G2, V2), other.set_volume(G2, V0)
    for M in (IDENT, np.array([1, 0, 0, -1, 0, 1, 0, 1, 0, 0, 1, 0], np.float64),
              affine_matrix_3d((2.0, -3.0, 1.5), shift=(0.3, -0.6, 0.9), src_shape=pair.dst)):
        one, two = raw(pair.b, V1, pair.b, V2, M, 1), raw(pair.b, V1, other, V0, M, 1)
        assert np.array_equal(one.view(np.uint64), two.view(np.uint64)) and one[28] > 0
        assert one[28] == G3.count(pair.dst, pair.dst, M, 1)


def test_repeats_bit_for_bit_and_changes_nothing(pair):
    M = pair.maps()["general"]
    first = raw(pair.b, V1, pair.a, V0, M, 1)
    again = raw(pair.b, V1, pair.a, V0, M, 1)
    assert np.array_equal(first.view(np.uint64), again.view(np.uint64))
    # next to other calls of both engines, nothing synchronised in between
    pair.a.set_volume(pair.Gv, V2)
    pair.a.be.c("scale_volume", V2, 0.5)
    pair.b.be.c("l1_norm", V1)
    pair.b.set_volume(pair.Fv, V2)
    third = raw(pair.b, V1, pair.a, V0, M, 1)
    pair.a.be.c("scale_volume", V2, 2.0)
    pair.b.be.c("diff_norm_sq", V2, V1, 1)
    assert np.array_equal(first.view(np.uint64), third.view(np.uint64))
    assert pair.b.be.scalars()[1] == 0.0
    assert np.array_equal(bits(pair.a.get_volume(V0)), bits(pair.Gv)) and np.array_equal(bits(pair.b.get_volume(V1)), bits(pair.Fv))
    assert np.array_equal(bits(pair.a.get_volume(V2)), bits(pair.Gv))


def test_claim_survives(gpu):
    """G = A * RECON in hand (a data distance), then the sums with RECON as F and as G: the next data distance is that of an engine
    that was left alone, bit for bit, and F == G at the identity has no residual."""
    N = 40
    e, f = engine(N, N, ANG_B), engine(N, N, ANG_B)
    b = np.abs(mixed((N, N * len(ANG_B)), 61))
    X = np.abs(smooth((N, N, N), 62))
    for eng in (e, f):
        eng._set_sino_local(b)
        eng.set_volume(X, 0)
        eng.data_distance()
    out = raw(e, 0, e, 0, IDENT, 0)
    assert out[28] == (N - 1) ** 3 and out[27] == 0.0 and not out[21:27].any() and out[29] == out[30] == out[31]
    t = 1.0 / e.get_lipschitz()
    assert e.data_distance() == f.data_distance()
    e.be.c("sirt_landweber", 0, t, 1), f.be.c("sirt_landweber", 0, t, 1)
    assert np.array_equal(bits(e.get_volume(0)), bits(f.get_volume(0)))


def test_no_overlap_gives_zeros(pair):
    from tomo_tv_amd.align import affine_matrix_3d
    M = affine_matrix_3d((7.3, -11.0, 4.0), shift=(3.0 * max(pair.src + pair.dst), 0, 0), src_shape=pair.src, dst_shape=pair.dst)
    out = raw(pair.b, V1, pair.a, V0, M, 0)
    assert not out.view(np.uint64).any()                                           # every sum +0.0: no NaN, no -0.0


def test_inf_and_nan_outside_the_counting_set_stay_out(pair):
    """p = x + (2, 0, 0): the planes s' < 2 of G (s' < 3 with margin 1) hold no tap of a counting voxel, and the faces of F lie in the margin."""
    M = np.array([1, 0, 0, 2, 0, 1, 0, 0, 0, 0, 1, 0], np.float64)
    clean = raw(pair.b, V1, pair.a, V0, M, 1)
    Fv, Gv = pair.Fv.copy(), pair.Gv.copy()
    Gv[0], Gv[1, ::2], Gv[2, 1::2] = np.inf, np.nan, -np.inf
    Fv[0, 0, 0], Fv[-1], Fv[:, 0, 1], Fv[1, 1, -1] = np.nan, np.inf, -np.inf, np.nan
    Fv[pair.src[0] - 3:] = np.nan                                                  # x with s + 3 > size_G - 1 does not count either
    pair.b.set_volume(Fv, V2), pair.a.set_volume(Gv, V2)
    try:
        got = raw(pair.b, V2, pair.a, V2, M, 1)
        assert np.isfinite(got).all() and got[28] > 0 and np.array_equal(got.view(np.uint64), clean.view(np.uint64))
    finally:
        pair.b.set_volume(pair.Fv, V2), pair.a.set_volume(pair.Gv, V2)


def test_refusals_leave_both_engines_usable(gpu):
    from tomo_tv_amd import _lib
    from tomo_tv_amd.engine import tomoengine
    L = _lib.load()
    p = Pair((5, 12, 12), (9, 10, 10))
    ha, hb = p.a.be.h, p.b.be.h
    ok = IDENT.ctypes.data_as(ctypes.c_void_p)
    out = np.full(32, -1.0)
    o = out.ctypes.data_as(ctypes.c_void_p)
    bad = [IDENT.copy() for _ in range(3)]
    bad[0][3], bad[1][0], bad[2][11] = np.nan, np.inf, -np.inf

    def call(fx, fv, mv_e, mv, m=ok, margin=1, dst=o):
        return L.tomo_volume_affine_normal(fx, fv, mv_e, mv, m, margin, dst)
    calls = [call(None, V1, ha, V0), call(hb, V1, None, V0), call(hb, -1, ha, V0), call(hb, 45, ha, V0), call(hb, V1, ha, -1),
             call(hb, V1, ha, 45), call(hb, V1, ha, V0, None), call(hb, V1, ha, V0, ok, 1, None), call(hb, V1, ha, V0, ok, -1),
             call(hb, V1, ha, V0, ok, 5), call(ha, V0, hb, V1, ok, 3)]           # 2 * 5 >= 9 slices of F; 2 * 3 >= 5 with the roles exchanged
    calls += [call(hb, V1, ha, V0, m.ctypes.data_as(ctypes.c_void_p)) for m in bad]
    assert calls == [ARG] * len(calls) and L.tomo_last_error()
    assert call(hb, V1, ha, V0, ok, 4) == 0                                       # 2 * 4 < 9: the largest margin is taken
    out[:] = -1.0
    if gpu > 1:                                                                  # different devices
        far = tomoengine(5, 12, np.deg2rad(ANG_B), device=1)
        assert call(hb, V1, far.be.h, V0) == ARG and call(far.be.h, V0, hb, V1) == ARG
    p.b.be.c("set_slab_edges", 1, 0)                                             # a slab of a larger volume, as F, as G and as both
    assert [call(hb, V1, ha, V0), call(ha, V0, hb, V1), call(hb, V1, hb, V1)] == [STATE] * 3 and b"slab" in L.tomo_last_error()
    p.b.be.c("set_slab_edges", 1, 1)
    with pytest.raises(NotImplementedError):                                     # the sharded classes refuse in Python already
        tomoengine(8, 12, np.deg2rad(ANG_A), device=0, sub_slabs=2).volume_affine_normal(p.b, IDENT)
    gone = engine(5, 12, ANG_B)
    assert L.tomo_release_geometry(gone.be.h) == 0
    assert [call(hb, V1, gone.be.h, V0), call(gone.be.h, V0, hb, V1)] == [STATE] * 2 and b"released" in L.tomo_last_error()
    assert np.all(out == -1.0)                                                   # no refused call wrote anything
    assert np.array_equal(bits(p.a.get_volume(V0)), bits(p.Gv)) and np.array_equal(bits(p.b.get_volume(V1)), bits(p.Fv))
    usable(p)


def test_refuses_an_engine_with_a_communicator(gpu):
    """A one-rank RCCL communicator bound through the C ABI, in a fresh child process like the other one-rank tests."""
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(here, "register3d_comm_script.py")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "REGISTER3D_COMM_REFUSED_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ---- the loop --------------------------------------------------------------------------------------------------------------------------
def test_loop_agrees_with_the_cpu_replay(gpu):
    """The exact case at N = 32 with F rounded to binary32, 20 iterations with both tolerances 0 (every run takes all 20, past
    convergence).  The yardstick is measured here: the CPU loop in binary64 against the CPU loop with the binary32 replay in place of
    the statement; the device's final map may lie twice that far from the binary64 loop's.  Recorded: the two figures
    printed below."""
    from tomo_tv_amd.align import register_volumes
    Fv, Gv, M_true = exact_case()
    Fv = Fv.astype(np.float32)
    kw = dict(max_iter=20, tol_shift=0.0, tol_deg=0.0, margin=1)
    M64, _ = G3.gauss_newton(Fv, Gv, **kw)
    M32, _ = G3.gauss_newton(Fv, Gv, sums=G3.normal_replay_f32, **kw)
    allow = 2.0 * float(np.max(np.abs(M64 - M32)))
    fx, mv = engine(32, 32, ANG_B), engine(32, 32, ANG_A)
    fx.set_volume(Fv, V1), mv.set_volume(Gv.astype(np.float32), V0)
    res = register_volumes(fx, mv, fixed_vol=V1, moving_vol=V0, **kw)
    dist = float(np.max(np.abs(res["M"] - M64)))
    print(f"final map, worst entry: binary64 loop against the binary32 replay {0.5 * allow:.3e}; device against the binary64 loop {dist:.3e}; "
          f"against the true map {np.max(np.abs(res['M'] - M_true)):.3e}")
    assert allow > 0 and dist <= allow
    assert len(res["step"]) == 20 and len(res["ssd"]) == 20 and not res["converged"] and res["count"][-1] > 32 ** 3 // 8
    assert np.allclose(res["R"] @ res["R"].T, np.eye(3), atol=1e-12)
    # the default tolerances stop early, and a start without overlap is refused
    quick = register_volumes(fx, mv, fixed_vol=V1, moving_vol=V0)
    assert quick["converged"] and len(quick["step"]) < 30 and np.max(np.abs(quick["M"] - M_true)) < 1e-2
    from tomo_tv_amd.align import affine_matrix_3d
    with pytest.raises(RuntimeError):
        register_volumes(fx, mv, M0=affine_matrix_3d(shift=(29.0, 0, 0), src_shape=(32, 32, 32)), fixed_vol=V1, moving_vol=V0)


def public(b, N, P):
    return np.ascontiguousarray(b.reshape(N, P, N).transpose(0, 2, 1))


def test_estimate_registration_with_a_pyramid(gpu):
    """The realistic case of tests/test_register3d_cpu.py on the device with pyramid (2, 1): rotation error <= 0.5 degrees, shift error
    <= 0.25 voxel, and the RMSE of 30 registered iterations with the estimate below the midpoint of the true-pose and the ignored
    figures.  ``apply=False`` leaves the object as it was; ``apply=True`` sets the estimate."""
    from tomo_tv_amd.dual_axis import DualAxisTomo
    c = realistic(0)
    N, X, reg = c["M"].N, c["X"], c["reg"]
    ang = np.linspace(-70, 70, 9)                                              # the geometry of tests/golden/A_N32_P9.npz
    bA, bB = public(c["bA"].astype(np.float32), N, 9), public(c["bB"].astype(np.float32), N, 9)
    dual, plain = DualAxisTomo(ang, bA, ang, bB, gpu_id=0), DualAxisTomo(ang, bA, ang, bB, gpu_id=0)

    def reconstruct(obj):
        for t in (obj.a.tomo, obj.b.tomo):
            t.restart_recon()
            t.be.c("sirt_landweber", 0, 1.0 / t.get_lipschitz(), 30)
    reconstruct(dual), reconstruct(plain)
    planted = smooth((N, N, N), 5)
    dual.a.tomo.set_volume(planted, V0), dual.b.tomo.set_volume(planted, dual.VOL_SAVED)
    before = [bits(dual.a.tomo.get_volume(0)), bits(dual.b.tomo.get_volume(0))]
    est = dual.estimate_registration(pyramid=(2, 1), apply=False)
    assert dual._reg is None and np.array_equal(dual.get_registration()[0], np.eye(3))
    assert [f for f, _ in est["levels"]] == [2, 1] and est["levels"][-1][1]["M"] is est["M"]
    # neither reconstruction moved, nor a user slot of A other than the documented scratch, nor B's saved slot
    assert np.array_equal(bits(dual.a.tomo.get_volume(0)), before[0]) and np.array_equal(bits(dual.b.tomo.get_volume(0)), before[1])
    assert np.array_equal(bits(dual.a.tomo.get_volume(V0)), bits(planted))
    assert np.array_equal(bits(dual.b.tomo.get_volume(dual.VOL_SAVED)), bits(planted))
    assert np.array_equal(before[0], bits(plain.a.tomo.get_volume(0))) and before[0].any()
    # ... and the object goes on as a twin that was reconstructed the same way and never estimated: from the volumes as they stand
    ca, cb = dual.sirt(3, restart=False), plain.sirt(3, restart=False)
    assert np.array_equal(ca, cb) and np.array_equal(bits(dual.a.tomo.get_volume(0)), bits(plain.a.tomo.get_volume(0)))
    assert np.array_equal(bits(dual.b.tomo.get_volume(0)), bits(plain.b.tomo.get_volume(0)))
    reconstruct(dual)
    again = dual.estimate_registration(pyramid=(2, 1), apply=True)
    Rm, d = dual.get_registration()
    assert np.array_equal(Rm, again["R"]) and np.array_equal(d, again["shift"]) and np.array_equal(again["M"], est["M"])
    rot_err = G3.angle_deg(Rm @ reg["R"].T)
    shift_err = float(np.max(np.abs(d - reg["shift"])))
    print(f"pyramid (2, 1) on the device: rotation error {rot_err:.3f} degrees, worst shift error {shift_err:.3f} voxel, "
          f"iterations {[len(r['step']) for _, r in est['levels']]}, ncc {est['ncc'][-1]:.4f}")
    assert rot_err <= 0.5 and shift_err <= 0.25
    rmse = {}
    dual.sirt(30, show_convergence=False)
    rmse["estimate"] = D.rmse(dual.get_recon(), X)
    dual.set_registration(matrix=reg["R"], shift=reg["shift"])
    dual.sirt(30, show_convergence=False)
    rmse["true"] = D.rmse(dual.get_recon(), X)
    dual.set_registration()
    dual.sirt(30, show_convergence=False)
    rmse["ignored"] = D.rmse(dual.get_recon(), X)
    print(f"RMSE after 30 registered iterations on the device: {rmse}")
    assert rmse["estimate"] < 0.5 * (rmse["true"] + rmse["ignored"])
