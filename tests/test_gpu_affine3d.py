"""``tomo_volume_affine`` / ``tomo_volume_affine_axpy`` on the GPU: the bit properties the header states (identity, the permutation of
``tomo_volume_cross``, whole-voxel shifts, quarter turns, Inf beside a copied sample), general maps inside the ref64 bound
(tests/ref64_affine3d.py), the fused multiply-add form to one ulp, one engine with two slots, the zero padding, stream ordering,
the claim on the model sinogram, every refusal, and the Python users: ``TomoGPU.reorient`` and ``DualAxisTomo`` with a registration.
Shapes: cubes of N = 8 (one partial lane group), 40, 70 (pitch 128: two lane groups, one partial), 130 (three lane groups), and the
non-cube pair Nslice = 5, N = 12 into Nslice = 9, N = 10."""
import numpy as np
import pytest

import ref64 as R
import ref64_affine3d as F
import ref64_dual as D
import sequences_affine3d  # noqa: F401  (registers this feature's rows of the call-sequence closure table)
from test_bin_cpu import mixed

pytestmark = pytest.mark.gpu

SHAPES = [((8, 8, 8), (8, 8, 8)), ((40, 40, 40), (40, 40, 40)), ((70, 70, 70), (70, 70, 70)), ((130, 130, 130), (130, 130, 130)),
          ((5, 12, 12), (9, 10, 10))]
V0, V1, V2 = 5, 6, 7                          # TOMO_VOL_USER0 ..
ANG_A, ANG_B = np.linspace(-60, 60, 2), np.linspace(-50, 40, 3)
ARG, STATE = 1, 3
IDENT = np.eye(3, 4).ravel()
PERM = np.array([0, 0, 1, 0, 0, 1, 0, 0, 1, 0, 0, 0], np.float64)
SPECIAL = np.array([0x7fc00001, 0xffc12345, 0x7f800000, 0xff800000, 0x80000000, 0x00000001, 0x807fffff], np.uint32)
# two quiet NaNs with different payloads and signs, +Inf, -Inf, -0.0, the smallest and the largest (negative) denormal


def engine(ns, N, ang):
    from tomo_tv_amd.engine import tomoengine
    return tomoengine(ns, N, np.deg2rad(ang), device=0)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def edges(n):
    """corners, their neighbours, the middle, and both sides of a lane-group edge (16 lanes x 4 slices = 64) where the axis has one"""
    return sorted({0, 1, n // 2, n - 2, n - 1, min(63, n - 1), min(64, n - 1), min(127, n - 1), min(128, n - 1)})


def planted(shape, seed):
    V = mixed(shape, seed)
    u, k = V.view(np.uint32), 0
    for s in edges(shape[0]):
        for y in (0, shape[1] // 3, shape[1] - 1):
            for z in edges(shape[2]):
                u[s, y, z] = SPECIAL[k % len(SPECIAL)]
                k += 1
    return V


def index_map(X, M, dst_shape):
    """numpy indexing for a whole-voxel map: dst[p] = X[M p] where that index exists, else 0 (bits)"""
    m = np.asarray(M, np.float64).reshape(3, 4)
    assert np.array_equal(m, np.round(m))
    g = np.meshgrid(*(np.arange(n) for n in dst_shape), indexing="ij")
    q = [(m[a, 0] * g[0] + m[a, 1] * g[1] + m[a, 2] * g[2] + m[a, 3]).astype(np.int64) for a in range(3)]
    ok = np.ones(dst_shape, bool)
    for a in range(3):
        ok &= (q[a] >= 0) & (q[a] < X.shape[a])
    out = np.zeros(dst_shape, np.float32)
    out[ok] = X[q[0][ok], q[1][ok], q[2][ok]]
    return out


class Pair:
    """a: the source engine; b: the destination engine; twin: an engine of a's size (b itself for the cubes)"""
    def __init__(self, src, dst):
        self.src, self.dst, self.cube = src, dst, src == dst and src[0] == src[1]
        self.a, self.b = engine(src[0], src[1], ANG_A), engine(dst[0], dst[1], ANG_B)
        self.twin = self.b if src == dst else engine(src[0], src[1], ANG_B)


@pytest.fixture(scope="module", params=SHAPES, ids=[f"{s[0]}x{s[1]}_to_{d[0]}x{d[1]}" for s, d in SHAPES])
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


def run(p, X, M, dst_fill=np.nan):
    p.a.set_volume(X, V0)
    p.b.set_volume(np.full(p.dst, dst_fill, np.float32), V1)                       # the destination is not read
    p.a.volume_affine_to(p.b, M, src=V0, dst=V1)
    return p.b.get_volume(V1)


def test_identity_and_permutation_move_bits(pair):
    X = planted(pair.src, 11)
    assert np.isnan(X).sum() > 8 and np.isinf(X).sum() > 8
    got = run(pair, X, IDENT)
    ref = np.zeros(pair.dst, np.float32)
    c = tuple(slice(0, min(a, b)) for a, b in zip(pair.src, pair.dst))
    ref[c] = X[c]                                                                 # equal sizes: the source itself
    assert np.array_equal(bits(got), bits(ref))
    assert np.array_equal(bits(pair.a.get_volume(V0)), bits(X))                    # the source was only read
    assert np.array_equal(bits(run(pair, X, IDENT)), bits(got))                    # the same bits from run to run
    if pair.cube:
        via_affine = run(pair, X, PERM)
        pair.a.cross_volume_to(pair.b, src=V0, dst=V2)
        assert np.array_equal(bits(via_affine), bits(pair.b.get_volume(V2))) and np.array_equal(bits(via_affine), bits(D.cross(X)))


def test_whole_voxel_shift_and_quarter_turns_copy_samples(pair):
    from tomo_tv_amd.align import affine_matrix_3d
    X = mixed(pair.src, 12)
    for s in edges(pair.src[0]):
        X[s, pair.src[1] // 3, pair.src[2] // 2] = np.inf if s % 2 else -np.inf
    maps = [np.array([1, 0, 0, 2, 0, 1, 0, -3, 0, 0, 1, 1], np.float64), np.array([1, 0, 0, -1, 0, 1, 0, 0, 0, 0, 1, 0], np.float64),
            affine_matrix_3d((90, 0, 0), src_shape=pair.src, dst_shape=pair.dst), affine_matrix_3d((-90, 0, 0), shift=(1, 0, -2), src_shape=pair.src, dst_shape=pair.dst)]
    if pair.cube:
        maps += [affine_matrix_3d((0, 90, 0), src_shape=pair.src), affine_matrix_3d((0, 0, 90), src_shape=pair.src),
                 affine_matrix_3d((180, 0, 270), src_shape=pair.src), np.array([-1, 0, 0, pair.src[0] - 1, 0, 1, 0, 0, 0, 0, 1, 0], np.float64)]
    for M in maps:
        got = run(pair, X, M)
        ref = index_map(X, M, pair.dst)
        assert np.array_equal(bits(got), bits(ref)), M
        assert not np.isnan(got).any() and np.isinf(got).sum() == np.isinf(ref).sum()
    # a fraction along one axis only: the Inf spreads along that axis and nowhere else, and never becomes NaN
    got = run(pair, X, np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0.25], np.float64))
    assert not np.isnan(got).any()


def general_maps(src, dst, few):
    """``few`` (N = 130): only the rotations and the partly-outside map, which already walk all three lane groups -- the binary64
    statement and its bound take about two seconds per map at 130^3 on the host, and a case is to stay within a few seconds."""
    from tomo_tv_amd.align import affine_matrix_3d
    kw = dict(src_shape=src, dst_shape=dst)
    half = tuple(0.5 * n for n in dst)
    maps = {"rotations": affine_matrix_3d((7.3, -11.0, 4.0), **kw),
            "partly outside": affine_matrix_3d((3.0, 5.0, -2.0), shift=(half[0] + 0.3, -half[1] + 0.6, 1.2), **kw)}
    if not few:
        maps.update({"shift with fractions": affine_matrix_3d(shift=(1.25, -2.5, 0.375), **kw),
                     "magnification 1.1": affine_matrix_3d((1.0, 0.0, -2.0), magnification=1.1, **kw)})
    maps["all outside"] = affine_matrix_3d((7.3, -11.0, 4.0), shift=(3.0 * max(src + dst), 0, 0), **kw)
    return maps


def test_general_maps_inside_the_bound(pair):
    X = mixed(pair.src, 13)
    for name, M in general_maps(pair.src, pair.dst, few=pair.src[0] >= 130).items():
        got = run(pair, X, M)
        if name == "all outside":
            assert not bits(got).any()                                            # all zeros, +0.0
            continue
        ref, _ = F.affine(X, M, pair.dst)
        r = F.ratio(got, ref, F.bound(X, M, pair.dst))
        print(f"{pair.src} -> {pair.dst}, {name}: worst error / bound {r:.3f}, {np.mean(ref != 0):.2f} of the elements non-zero")
        assert r <= 1.0 and ref.any()
        assert name != "partly outside" or 0.05 < np.mean(ref == 0)


@pytest.mark.parametrize("a", [0.0, 1.0, -0.75, 0.3])
def test_axpy_to_one_ulp_of_the_final_fma(pair, a):
    """The interpolated value is the kernel's own (the plain call, bit-reproducible); what is checked here is the fused multiply-add
    on top of it, the clamp, and the NaN / Inf rules of ``tomo_volume_cross_axpy``."""
    from tomo_tv_amd.align import affine_matrix_3d
    S, Dst = mixed(pair.src, 21), mixed(pair.dst, 22)
    c, cd = tuple(n // 2 for n in pair.src), tuple(n // 2 for n in pair.dst)      # near the centre: every map of this test reaches them
    S[c], S[c[0] - 2, c[1], c[2]], S[c[0], c[1] - 2, c[2] + 2] = np.inf, -np.inf, np.nan
    Dst[cd], Dst[0, 2, 0], Dst[0, 1, 0] = np.inf, np.float32(-0.0), np.float32(2.0 ** -140)
    for M in (IDENT, affine_matrix_3d((2.0, -3.0, 1.0), shift=(0.25, 0.5, -0.75), src_shape=pair.src, dst_shape=pair.dst)):
        value = run(pair, S, M)
        for clamp in (False, True):
            pair.b.set_volume(Dst, V1)
            pair.a.volume_affine_axpy_to(pair.b, M, a, clamp=clamp, src=V0, dst=V1)
            got = pair.b.get_volume(V1)
            ref = F.axpy(value, Dst, a, clamp)
            nan = np.isnan(ref)
            assert np.array_equal(np.isnan(got), nan) and (not clamp or not nan.any()) and (clamp or nan.any())
            inf = np.isinf(ref)
            assert np.array_equal(got[inf], ref[inf])
            fin = np.isfinite(ref)
            assert np.all(np.abs(got[fin].astype(np.float64) - ref[fin]) <= D.ulp32(ref[fin]))
            if clamp:
                assert got.min() >= 0.0
            if a == 0.0 and not clamp:                                            # a = 0 keeps the destination's bits where the value is finite
                keep = np.isfinite(value) & (Dst != 0)
                assert np.array_equal(bits(got)[keep], bits(Dst)[keep])


def test_one_engine_with_two_slots_equals_two_engines(pair):
    from tomo_tv_amd.align import affine_matrix_3d
    X, D0 = planted(pair.src, 31), mixed(pair.src, 32)
    M = affine_matrix_3d((4.0, -6.0, 2.5), shift=(0.7, -1.2, 0.4), magnification=0.95, src_shape=pair.src)
    a, t = pair.a, pair.twin
    a.set_volume(X, V0)
    for axpy in (False, True):
        a.set_volume(D0, V1), t.set_volume(D0, V1)
        if axpy:
            a.volume_affine_axpy_to(a, M, -0.5, src=V0, dst=V1), a.volume_affine_axpy_to(t, M, -0.5, src=V0, dst=V1)
        else:
            a.volume_affine_to(a, M, src=V0, dst=V1), a.volume_affine_to(t, M, src=V0, dst=V1)
        one, two = a.get_volume(V1), t.get_volume(V1)
        assert np.array_equal(bits(one), bits(two)) and np.isfinite(one).any()
    assert np.array_equal(bits(a.get_volume(V0)), bits(X))


def test_padding_of_the_destination_is_zero(pair):
    """Both routes of tests/test_gpu_dual.py: the real voxels uploaded into another slot (an upload writes zero padding) differ from the
    kernel's output by exactly nothing over the whole pitch, and the sum of |x| over the whole pitch is the binary64 sum over the real
    voxels.  The destination holds non-zero real voxels at the pitch edge before the call; its padding is zero before every public
    call, so that the stores cover the slices Nslice .. pitch - 1 is read from the kernel."""
    from tomo_tv_amd._lib import S_L1
    from tomo_tv_amd.align import affine_matrix_3d
    X, D0 = mixed(pair.src, 5), mixed(pair.dst, 6)
    M = affine_matrix_3d((2.0, 1.0, -3.0), shift=(0.5, 0.25, -0.5), src_shape=pair.src, dst_shape=pair.dst)
    pair.a.set_volume(X, V0)
    for axpy in (False, True):
        pair.b.set_volume(D0, V1)
        if axpy:
            pair.a.volume_affine_axpy_to(pair.b, M, -1.5, src=V0, dst=V1)
        else:
            pair.a.volume_affine_to(pair.b, M, src=V0, dst=V1)
        got = pair.b.get_volume(V1)
        pair.b.set_volume(got, V2)
        pair.b.be.c("diff_norm_sq", V2, V1, 1)
        assert pair.b.be.scalars()[1] == 0.0
        pair.b.be.c("l1_norm", V1)
        ref, bound = R.l1(got)
        R.assert_scalar("l1 over the pitch", pair.b.be.scalars()[S_L1], ref, bound)


def test_no_synchronise_is_needed(gpu):
    from tomo_tv_amd.align import affine_matrix_3d
    p = Pair((40, 40, 40), (40, 40, 40))
    X = np.abs(mixed(p.src, 41))
    fwd = affine_matrix_3d((1.0, -2.0, 0.5), shift=(0.25, 0, -0.5), src_shape=p.src)
    back = affine_matrix_3d((-0.5, 2.0, -1.0), shift=(-0.25, 0.1, 0.5), src_shape=p.src)
    out = []
    for sync in (False, True):
        def wait():
            if sync:
                p.a.synchronize(), p.b.synchronize()
        p.a.set_volume(X, 0), p.b.restart_recon()
        wait()
        for _ in range(5):                                                        # ten calls: two engines and one engine in turn
            p.a.volume_affine_to(p.b, fwd, src=0, dst=0)
            wait()
            p.b.volume_affine_axpy_to(p.b, back, 0.5, src=0, dst=V1)
            wait()
            p.b.volume_affine_to(p.a, back, src=V1, dst=0)
            wait()
        out.append((p.a.get_volume(0), p.b.get_volume(V1)))
        p.b.set_volume(np.zeros(p.dst, np.float32), V1)
    assert np.array_equal(bits(out[0][0]), bits(out[1][0])) and np.array_equal(bits(out[0][1]), bits(out[1][1])) and out[0][0].any()


def test_claim_is_dropped_by_a_resampled_volume(gpu):
    """The model sinogram G = A * RECON in hand (a data distance), then RECON overwritten by the resampling: the next step must project
    again.  Against a fresh engine that is given the same volume by an upload."""
    N = 40
    e, f = engine(N, N, ANG_B), engine(N, N, ANG_B)
    b = np.abs(mixed((N, N * len(ANG_B)), 61))
    X, Y = np.abs(mixed((N, N, N), 62)), np.abs(mixed((N, N, N), 63))
    M = np.array([1, 0, 0, 0.5, 0, 1, 0, -1, 0, 0, 1, 0.25], np.float64)
    t = 1.0 / e.get_lipschitz()
    for axpy in (False, True):
        e._set_sino_local(b), f._set_sino_local(b)
        e.set_volume(X, 0), e.set_volume(Y, V0)
        e.be.c("data_distance_sq", 0)
        if axpy:
            e.volume_affine_axpy_to(e, M, 0.5, src=V0, dst=0)
        else:
            e.volume_affine_to(e, M, src=V0, dst=0)
        moved = e.get_volume(0)
        e.be.c("sirt_landweber", 0, t, 1)
        f.set_volume(moved, 0)
        f.be.c("sirt_landweber", 0, t, 1)
        assert np.array_equal(bits(e.get_volume(0)), bits(f.get_volume(0))) and not np.array_equal(moved, X)


def test_refusals_leave_both_engines_usable(gpu):
    import ctypes
    from tomo_tv_amd import _lib
    from tomo_tv_amd.engine import tomoengine
    L = _lib.load()
    p = Pair((5, 12, 12), (9, 10, 10))
    V, W = mixed(p.src, 51), mixed(p.dst, 52)
    p.a.set_volume(V, V0), p.b.set_volume(W, V1)
    ha, hb = p.a.be.h, p.b.be.h
    ok = IDENT.ctypes.data_as(ctypes.c_void_p)
    bad = [IDENT.copy() for _ in range(3)]
    bad[0][3], bad[1][0], bad[2][11] = np.nan, np.inf, -np.inf

    def both(src, sv, dst, dv, m=ok):
        return [L.tomo_volume_affine(src, sv, dst, dv, m), L.tomo_volume_affine_axpy(src, sv, dst, dv, m, 0.5, 0)]
    calls = (both(None, V0, hb, V1) + both(ha, V0, None, V1) + both(ha, V0, ha, V0) + both(ha, -1, hb, V1) + both(ha, 45, hb, V1) +
             both(ha, V0, hb, -1) + both(ha, V0, hb, 45) + both(ha, V0, hb, V1, None))
    for m in bad:
        calls += both(ha, V0, hb, V1, m.ctypes.data_as(ctypes.c_void_p))
    assert calls == [ARG] * len(calls) and L.tomo_last_error()
    if gpu > 1:                                                                  # different devices
        far = tomoengine(5, 12, np.deg2rad(ANG_B), device=1)
        assert both(ha, V0, far.be.h, V1) == [ARG, ARG] and both(far.be.h, V0, ha, V1) == [ARG, ARG]
    # a slab of a larger volume (what a sharded engine is), as source and as destination
    p.b.be.c("set_slab_edges", 1, 0)
    assert both(ha, V0, hb, V1) == [STATE, STATE] and both(hb, V1, ha, V0) == [STATE, STATE] and b"slab" in L.tomo_last_error()
    assert both(hb, V1, hb, V2) == [STATE, STATE]
    p.b.be.c("set_slab_edges", 1, 1)
    with pytest.raises(NotImplementedError):                                     # the sharded classes refuse in Python already
        tomoengine(8, 12, np.deg2rad(ANG_A), device=0, sub_slabs=2).volume_affine_to(p.b, IDENT)
    # nothing was enqueued or written
    assert np.array_equal(bits(p.a.get_volume(V0)), bits(V)) and np.array_equal(bits(p.b.get_volume(V1)), bits(W))
    usable(p)
    # released geometry: TOMO_ERR_STATE on either side; the other engine goes on
    gone = engine(5, 12, ANG_B)
    assert L.tomo_release_geometry(gone.be.h) == 0
    assert both(ha, V0, gone.be.h, V1) == [STATE, STATE] and both(gone.be.h, V0, ha, V1) == [STATE, STATE]
    assert b"released" in L.tomo_last_error()
    usable(p)


def test_refuses_an_engine_with_a_communicator(gpu):
    """A one-rank RCCL communicator bound through the C ABI, in a fresh child process like the other one-rank tests."""
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(here, "affine3d_comm_script.py")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "AFFINE3D_COMM_REFUSED_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ---- TomoGPU.reorient -----------------------------------------------------------------------------------------------------------------
def test_reorient_and_back_stays_inside_the_two_bounds(gpu):
    from tomo_tv_amd.align import affine_matrix_3d, rotation_3d
    from tomo_tv_amd.reconstructor import TomoGPU
    ns, N, ang = 24, 32, np.linspace(-60, 60, 3)
    rec = TomoGPU(ang, np.zeros((ns, N, 3), np.float32), gpu_id=0)
    s, y, z = np.meshgrid(np.arange(ns), np.arange(N), np.arange(N), indexing="ij")
    X = (np.exp(-((s - 11.0) ** 2 + (y - 17.0) ** 2 + (z - 14.5) ** 2) / 40.0) + 0.5 * np.exp(-((s - 14.0) ** 2 + (y - 12.0) ** 2 + (z - 19.0) ** 2) / 18.0)).astype(np.float32)
    rot, d = (3.0, -5.0, 2.0), np.array([0.6, -0.4, 1.1])
    rec.tomo.set_volume(X, 0)
    M1 = rec.reorient(rot, d)
    assert np.array_equal(M1, affine_matrix_3d(rot, d, src_shape=X.shape))
    Y = rec.tomo.get_volume(0)
    Rm = rotation_3d(rot)
    # the inverse motion has the rotation R^T, which is no (about s, about y, about z) triple in general: the matrix route
    M2 = affine_matrix_3d(shift=-(Rm.T @ d), src_shape=X.shape, matrix=Rm.T)
    rec.tomo.volume_affine_to(rec.tomo, M2, src=0, dst=V0)
    Z = rec.tomo.get_volume(V0)
    ref1, _ = F.affine(X, M1)
    b1 = F.bound(X, M1)
    assert F.ratio(Y, ref1, b1) <= 1.0
    ref2, _ = F.affine(ref1, M2)
    b2 = F.bound(Y, M2) + F.affine(b1, M2)[0]                                     # the second call's own bound + the first's, carried through
    r = F.ratio(Z, ref2, b2)
    print(f"reorient and back: worst error / (sum of the two bounds) {r:.3f}; distance from the phantom {np.max(np.abs(Z - X)):.3e}")
    assert r <= 1.0
    # in place through the documented scratch slot, twice gives the same bits
    rec.tomo.set_volume(X, 0)
    rec.reorient(rot, d)
    assert np.array_equal(bits(rec.tomo.get_volume(0)), bits(Y))


# ---- DualAxisTomo with a registration ---------------------------------------------------------------------------------------------------
def public(b, N, P):
    return np.ascontiguousarray(b.reshape(N, P, N).transpose(0, 2, 1))


ROT, SHIFT = (0.0, 8.0, 0.0), np.array([1.5, 0.0, -2.25])


@pytest.fixture(scope="module")
def driver(gpu):
    from tomo_tv_amd.align import rotation_3d
    from tomo_tv_amd.dual_axis import DualAxisTomo, registration_maps
    N, ang = 32, np.linspace(-70, 70, 9)                                       # the geometry of tests/golden/A_N32_P9.npz
    M = R.Matrix(N, ang)
    X = D.phantom(N)
    Rm = rotation_3d(ROT)
    reg = registration_maps(N, shift=-(Rm.T @ SHIFT), matrix=Rm.T)             # B is made from the phantom moved by (ROT, SHIFT)
    bA, bB = D.fp_a(M, X).astype(np.float32), F.moved_series_b(M, X, reg["to_b"]).astype(np.float32)
    dual = DualAxisTomo(ang, public(bA, N, 9), ang, public(bB, N, 9), gpu_id=0)
    return dict(N=N, M=M, X=X, bA=bA, bB=bB, dual=dual, reg=reg, ang=ang)


def test_identity_registration_is_the_unregistered_driver(driver):
    from tomo_tv_amd.dual_axis import DualAxisTomo
    N, ang, dual = driver["N"], driver["ang"], driver["dual"]
    plain = DualAxisTomo(ang, public(driver["bA"], N, 9), ang, public(driver["bB"], N, 9), gpu_id=0)
    dual.set_registration()
    dual.set_registration((0, 360, 0), (0, 0, 0))
    ca, cb = dual.sirt(3), plain.sirt(3)
    assert np.array_equal(ca, cb) and np.array_equal(dual.get_recon(), plain.get_recon())
    dual.sart(2, beta=0.5, show_convergence=False), plain.sart(2, beta=0.5, show_convergence=False)
    assert np.array_equal(dual.get_recon(), plain.get_recon())
    dual.combine(0.25), plain.combine(0.25)
    assert np.array_equal(dual.get_recon(), plain.get_recon()) and dual.get_recon().any()


def test_combine_with_a_registration(driver):
    dual, reg = driver["dual"], driver["reg"]
    dual.set_registration(matrix=reg["R"], shift=reg["shift"])
    try:
        dual.a.sirt(5, show_convergence=False)
        dual.b.sirt(5, show_convergence=False)
        ra, rb = dual.a.tomo.get_volume(0), dual.b.tomo.get_volume(0)
        w = 0.25
        dual.combine(w)
        got = dual.a.tomo.get_volume(0).astype(np.float64)
        moved, _ = F.affine(D.cross(rb), reg["to_a"])
        ref = (1.0 - w) * ra.astype(np.float64) + w * moved
        # the scaling rounds once, the fused multiply-add once; the interpolated value is inside its own bound
        bnd = w * F.bound(D.cross(rb), reg["to_a"]) + D.ulp32((1.0 - w) * ra.astype(np.float64)) + D.ulp32(ref)
        r = F.ratio(got, ref, bnd)
        print(f"combine with a registration: worst error / bound {r:.3f}")
        assert r <= 1.0 and moved.any() and not np.allclose(moved, D.cross(rb), atol=1e-3)
    finally:
        dual.set_registration()


def test_sirt_with_a_registration_against_the_binary64_replay(driver):
    """The rule of tests/test_gpu_dual.py: the yardstick is the worst element deviation of the single-axis ``sirt_landweber`` (20
    iterations, the same data) from its own binary64 replay, measured here; the registered dual-axis loop (10 iterations) may deviate
    at most twice as much from its replay (tests/ref64_affine3d.py: dual_axis_registered).  Recorded: the two values
    printed below."""
    M, bA, bB, dual, reg = driver["M"], driver["bA"], driver["bB"], driver["dual"], driver["reg"]
    ta, tb = dual.a.tomo, dual.b.tomo
    tA, tB = float(np.float32(1.0 / ta.get_lipschitz())), float(np.float32(1.0 / tb.get_lipschitz()))
    ta.restart_recon()
    ta.be.c("sirt_landweber", 0, tA, 20)
    dev_single = float(np.max(np.abs(ta.get_volume(0).astype(np.float64) - D.single_axis(M, bA, tA, 20))))
    dual.set_registration(matrix=reg["R"], shift=reg["shift"])
    try:
        cost = dual.sirt(10)
        got = dual.get_recon()
        ref, dd_b = F.dual_axis_registered(M, M, bA, bB, tA, tB, 10, reg["to_a"], reg["to_b"])
        dev_dual = float(np.max(np.abs(got - ref)))
        print(f"worst element deviation from the binary64 replay: single-axis (20 iterations) {dev_single:.3e}, registered dual-axis (10) {dev_dual:.3e}")
        assert dev_single > 0 and dev_dual <= 2 * dev_single
        assert cost.shape == (10, 2) and cost[-1].sum() < cost[0].sum()
        assert abs(cost[-1, 1] - dd_b) <= 1e-4 * dd_b
        first = ta.get_volume(0)
        dual.sirt(10, show_convergence=False)                                    # the same bits from run to run, with or without the read-backs
        assert np.array_equal(bits(ta.get_volume(0)), bits(first))
        dual.sart(2, beta=0.5)
        assert np.isfinite(dual.get_recon()).all() and dual.get_recon().any()
        # ignoring the registration fits series B worse (the CPU recovery case, on the device)
        dual.set_registration()
        worse = dual.sirt(10)
        assert worse[-1, 1] > cost[-1, 1]
    finally:
        dual.set_registration()
