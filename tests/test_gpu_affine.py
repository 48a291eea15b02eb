"""``sino_affine`` / ``sino_axis_profile`` on the GPU, every output element against tests/ref64_affine.py, the copy guarantees bit for
bit, and ``TomoGPU``'s rotation bookkeeping.  Shapes (Nslice, N, Nproj): (8, 8, 5) square and smaller than a wave; (70, 33, 5) two
64-slice chunks, 58 padding slices, an odd row length; (130, 16, 3) three chunks, the last with two slices."""
import ctypes

import numpy as np
import pytest

import ref64_affine as F
import ref64_align as RA
from test_affine_cpu import params

pytestmark = pytest.mark.gpu

SHAPES = [(8, 8, 5), (70, 33, 5), (130, 16, 3)]
IDS = ["square8", "pad58", "chunks3"]
A_SLOT, D_SLOT, E_SLOT = 3, 5, 6          # TOMO_SINO_USER0 ...


class Case:
    def __init__(self, shape):
        from tomo_tv_amd.engine import tomoengine
        self.ns, self.N, self.P = shape
        self.eng = tomoengine(self.ns, self.N, np.deg2rad(np.linspace(-60, 60, self.P)), device=0)
        self.A = np.random.default_rng(self.ns + self.N).random((self.P, self.N, self.ns), dtype=np.float32)
        self.put(A_SLOT, self.A)

    def put(self, slot, X):
        b = RA.packed(np.asarray(X, np.float32))
        self.eng.be.c("set_sinogram", slot, b.ctypes.data_as(ctypes.c_void_p))

    def get(self, slot):
        return RA.images(self.eng._sino(slot), self.N)

    def padding_is_zero(self, slot):
        """Padding slices cannot be read through the ABI, and tomo_l1_norm sums volumes only; tomo_sino_diff_norm_sq sweeps the whole
        pitch of two sinogram slots and its terms are exact for equal samples: the real samples of ``slot`` uploaded into another
        slot (an upload writes zero padding) differ from ``slot`` by exactly nothing, padding included"""
        self.put(E_SLOT, self.get(slot))
        self.eng.be.c("sino_diff_norm_sq", slot, E_SLOT, 1)
        assert self.eng.be.scalars()[1] == 0.0


@pytest.fixture(scope="module", params=list(zip(SHAPES, IDS)), ids=IDS)
def case(request, gpu):
    return Case(request.param[0])


def test_affine_every_element_within_its_bound(case):
    from tomo_tv_amd.align import affine_matrices
    sh, rot, mag = params(case.P, 23 + case.N)
    M = affine_matrices(sh, rot, mag, case.N, case.ns)
    case.eng.sino_affine(A_SLOT, D_SLOT, M)
    got = case.get(D_SLOT)
    ref, _ = F.affine(case.A, M)
    err, bound = np.abs(got - ref), F.bound(case.A, M)
    print(f"worst error / bound: {np.max(err / np.maximum(bound, 1e-300)):.3f}; equal to the binary32 replay: "
          f"{np.mean(got == F.affine_replay_f32(case.A, M)):.3f} of the elements")
    assert got.any() and np.all(err <= bound)
    case.padding_is_zero(D_SLOT)
    case.eng.sino_affine(A_SLOT, E_SLOT, M)
    assert np.array_equal(case.get(E_SLOT), got)                                       # bit-identical from run to run


def test_identity_and_translations_copy_the_bits(case):
    from tomo_tv_amd.align import affine_matrices
    ident = np.tile([1.0, 0, 0, 0, 1.0, 0], (case.P, 1))
    case.eng.sino_affine(A_SLOT, D_SLOT, ident)
    assert np.array_equal(case.get(D_SLOT), case.A)
    case.padding_is_zero(D_SLOT)
    rng = np.random.default_rng(11)
    whole = rng.integers(-3, 4, (case.P, 2)).astype(np.float64)
    frac = rng.uniform(-3, 3, (case.P, 2)).astype(np.float32).astype(np.float64)
    frac[0, 1] = np.round(frac[0, 1])                     # one axis whole, the other not: the two-tap paths
    frac[1, 0] = np.round(frac[1, 0])
    tiny = np.full((case.P, 2), 2.0 ** -30)               # the fraction of -d rounds to 1 in binary32: the whole-pixel shift 0
    tiny[-1] = (-(2.0 ** -30), 3.0)
    for d in (whole, frac, tiny):
        case.eng.sino_shift(A_SLOT, E_SLOT, d, wrap=False)
        case.eng.sino_affine(A_SLOT, D_SLOT, affine_matrices(d, 0.0, 1.0, case.N, case.ns))
        assert np.array_equal(case.get(D_SLOT).view(np.uint32), case.get(E_SLOT).view(np.uint32)), d[0]
    case.eng.sino_affine(A_SLOT, D_SLOT, affine_matrices(whole, 0.0, 1.0, case.N, case.ns))
    assert np.array_equal(case.get(D_SLOT), RA.shift_int(case.A, whole, wrap=False))


def test_quarter_turn_of_a_square_image_is_rot90(case):
    from tomo_tv_amd.align import affine_matrices
    if case.N != case.ns:
        # not square: +90 degrees about the centre is still a whole- or half-pixel map; against the statement, within the bound
        M = affine_matrices(np.zeros((case.P, 2)), 90.0, 1.0, case.N, case.ns)
        case.eng.sino_affine(A_SLOT, D_SLOT, M)
        assert np.all(np.abs(case.get(D_SLOT) - F.affine(case.A, M)[0]) <= F.bound(case.A, M))
        return
    case.eng.sino_affine(A_SLOT, D_SLOT, affine_matrices(np.zeros((case.P, 2)), 90.0, 1.0, case.N, case.ns))
    got = case.get(D_SLOT)
    assert all(np.array_equal(got[a], np.rot90(case.A[a])) for a in range(case.P))


def test_inf_beside_a_copied_sample_and_maps_that_leave_the_image(case):
    from tomo_tv_amd.align import affine_matrices
    X = case.A.copy()
    X[0, case.N // 2, case.ns // 2] = np.inf
    case.put(E_SLOT, X)
    d = np.tile([1.0, -2.0], (case.P, 1))
    case.eng.sino_affine(E_SLOT, D_SLOT, affine_matrices(d, 0.0, 1.0, case.N, case.ns))
    got = case.get(D_SLOT)
    assert not np.isnan(got).any() and np.isinf(got).sum() == 1 and np.array_equal(got, RA.shift_int(X, d))
    # everything outside: far translations, a magnified far corner, entries whose products overflow
    M = np.tile([1.0, 0, 0, 0, 1.0, 0], (case.P, 1))
    M[:, 2] = case.N
    M[0] = (1.0, 0.0, -3e9, 0.0, 1.0, 1e30)
    M[1] = (1e300, 1e300, 1e300, -1e300, -1e300, -1e300)
    M[-1] = (1.0, 0.0, 0.5, 0.0, 1.0, -(case.ns + 0.25))
    case.eng.sino_affine(A_SLOT, D_SLOT, M)
    assert not case.get(D_SLOT).any()
    case.padding_is_zero(D_SLOT)


def test_axis_profile(case):
    c, ref = case.eng.sino_axis_profile(A_SLOT), F.profile(case.A)
    print(f"worst relative error: {np.max(np.abs(c - ref) / ref):.3e}")
    assert c.shape == (case.P, case.ns) and np.all(np.abs(c - ref) <= 1e-12 * np.abs(ref))
    assert np.array_equal(c, case.eng.sino_axis_profile(A_SLOT))


def test_sums_over_several_workgroups_per_projection(gpu):
    """Nray = 72 with 5 slices and 2 angles: two workgroups per projection for the profile (64 rays each), three for the moments (32)
    and five for the normal equations (16), the last one partial every time, so the second stage adds more than one row per output.
    The statements and bounds are those of the tests of each call: test_axis_profile, test_gpu_align.py (moments) and
    test_gpu_sino_normal.py (ref64_sino_normal.bound, the exact count)."""
    import ref64_sino_normal as SN
    c = Case((5, 72, 2))
    prof, ref = c.eng.sino_axis_profile(A_SLOT), F.profile(c.A)
    assert prof.shape == (c.P, c.ns) and np.all(np.abs(prof - ref) <= 1e-12 * np.abs(ref))
    assert np.array_equal(prof, c.eng.sino_axis_profile(A_SLOT))
    m, ref = c.eng.sino_moments(A_SLOT), RA.moments(c.A)
    assert m.shape == (c.P, 3) and np.all(np.abs(m - ref) <= 1e-6 * np.abs(ref))
    assert np.array_equal(m, c.eng.sino_moments(A_SLOT))
    Fx = np.random.default_rng(72).random((c.P, c.N, c.ns), dtype=np.float32)
    c.put(D_SLOT, Fx)
    M = np.array([[1.0, 0, 0, 0, 1.0, 0], F.matrices([[0.3, -0.6]], 1.3, 1.02, c.N, c.ns)[0]])
    for margin in (0, 1):
        ref, bnd, _ = SN.bound(Fx, c.A, M, margin)
        got = np.full((c.P, 21), np.nan)
        c.eng.be.c("sino_affine_normal", D_SLOT, A_SLOT, M.ctypes.data_as(ctypes.c_void_p), margin, got.ctypes.data_as(ctypes.c_void_p))
        r = SN.ratios(got, ref, bnd)
        print(f"margin {margin}: worst error / bound per projection {np.round(r.max(axis=1), 4)}, samples that count {ref[:, 15].astype(int)}")
        assert np.array_equal(got[:, 15], ref[:, 15]) and np.all(ref[:, 15] > 0) and r.max() <= 1.0


def test_refusals_leave_the_engine_usable(case):
    from tomo_tv_amd import _lib
    L, h, P = case.eng.be.L, case.eng.be.h, case.P
    ident = np.tile([1.0, 0, 0, 0, 1.0, 0], (P, 1))
    pm = ident.ctypes.data_as(ctypes.c_void_p)
    out = np.zeros((P, case.ns))
    po = out.ctypes.data_as(ctypes.c_void_p)
    bad = []
    for pos, v in (((P - 1, 5), np.nan), ((0, 0), np.inf), ((0, 2), -np.inf)):
        m = ident.copy()
        m[pos] = v
        bad.append(m)
    calls = [L.tomo_sino_affine(h, A_SLOT, A_SLOT, pm), L.tomo_sino_affine(h, A_SLOT, 77, pm), L.tomo_sino_affine(h, -1, D_SLOT, pm),
             L.tomo_sino_affine(h, A_SLOT, D_SLOT, None), L.tomo_sino_axis_profile(h, A_SLOT, None), L.tomo_sino_axis_profile(h, 43, po),
             L.tomo_sino_axis_profile(h, -1, po)] + [L.tomo_sino_affine(h, A_SLOT, D_SLOT, m.ctypes.data_as(ctypes.c_void_p)) for m in bad]
    assert calls == [1] * len(calls) and L.tomo_last_error()
    with pytest.raises(_lib.TomoError):
        case.eng.sino_affine(A_SLOT, D_SLOT, bad[0])
    with pytest.raises(ValueError):
        case.eng.sino_affine(A_SLOT, D_SLOT, ident[:-1])
    assert np.array_equal(case.get(A_SLOT), case.A)                                       # nothing was touched
    case.eng.sino_affine(A_SLOT, D_SLOT, ident)
    assert np.array_equal(case.get(D_SLOT), case.A)


def test_engines_with_a_communicator_or_sub_slabs_refuse(gpu):
    from local_ring import ThreadRing
    from tomo_tv_amd.engine import tomoengine
    ang = np.deg2rad(np.linspace(-60, 60, 3))

    def body(comm):
        t = tomoengine(8, 8, ang, device=0, comm=comm)
        for call in (lambda: t.sino_affine(A_SLOT, D_SLOT, np.tile([1.0, 0, 0, 0, 1.0, 0], (3, 1))), lambda: t.sino_axis_profile(A_SLOT)):
            with pytest.raises(NotImplementedError):
                call()
        return True
    assert ThreadRing(2).run(body) == [True, True]
    t = tomoengine(8, 8, ang, device=0, sub_slabs=2)
    with pytest.raises(NotImplementedError):
        t.sino_axis_profile(A_SLOT)
    with pytest.raises(NotImplementedError):
        t.sino_affine(A_SLOT, D_SLOT, np.tile([1.0, 0, 0, 0, 1.0, 0], (3, 1)))


# ---- TomoGPU ------------------------------------------------------------------------------------------------------------------
def public(X):
    """X[a][r][s] -> the (Nslice, Nray, Nangles) array TomoGPU is given"""
    return np.ascontiguousarray(np.asarray(X).transpose(2, 1, 0))


def test_set_alignment_without_and_with_a_rotation(gpu):
    from tomo_tv_amd._lib import SINO_B
    from tomo_tv_amd.align import affine_matrices
    from tomo_tv_amd.reconstructor import TomoGPU
    P, N, ns = 5, 33, 70
    X = np.random.default_rng(41).random((P, N, ns), dtype=np.float32)
    sh, _, _ = params(P, 43)
    rec = TomoGPU(np.linspace(-60, 60, P), public(X), gpu_id=0)
    t, scratch = rec.tomo, rec.ALIGN_SLOT + 5
    # no rotation: the bits of the shift pass on the kept copy, which is what the call did before rotations existed
    rec.set_alignment(sh)
    t.sino_shift(rec.ALIGN_SLOT, scratch, sh, wrap=False)
    assert np.array_equal(t._sino(SINO_B), t._sino(scratch)) and np.array_equal(RA.images(t._sino(rec.ALIGN_SLOT), N), X)
    assert np.array_equal(rec.get_alignment_rotation()[0], np.zeros(P)) and np.array_equal(rec.get_alignment_rotation()[1], np.ones(P))
    with pytest.raises(ValueError):
        rec.set_alignment(sh, wrap=True, rotation_deg=2.0)
    # a stored rotation of zero takes the affine pass and still gives those bits
    rec.set_alignment(sh, rotation_deg=0.0)
    assert np.array_equal(t._sino(SINO_B), t._sino(scratch))
    # two successive calls: the second resamples the kept copy by its shifts and the remembered rotation, in one interpolation
    rot = np.linspace(-4.0, 4.0, P)
    rec.set_alignment(sh, rotation_deg=rot, magnification=1.03)
    sh2 = sh + np.float32(0.75)
    assert np.array_equal(rec.set_alignment(sh2), sh2)
    M = affine_matrices(sh2, rot, 1.03, N, ns)
    t.sino_affine(rec.ALIGN_SLOT, scratch, M)
    got = t._sino(SINO_B)
    assert np.array_equal(got, t._sino(scratch))
    assert np.all(np.abs(RA.images(got, N) - F.affine(X, M)[0]) <= F.bound(X, M))
    assert np.array_equal(rec.get_alignment_rotation()[0], rot) and np.array_equal(rec.get_alignment_rotation()[1], np.full(P, 1.03))
    with pytest.raises(ValueError):
        rec.set_alignment(sh2, wrap=True)
    rec.set_tilt_series(public(X))
    assert np.array_equal(rec.get_alignment_rotation()[0], np.zeros(P)) and not rec.get_alignment().any()


def test_refine_alignment_keeps_a_stored_rotation(gpu):
    from tomo_tv_amd._lib import SINO_B
    from tomo_tv_amd.align import affine_matrices
    from tomo_tv_amd.reconstructor import TomoGPU
    ang, clean, X = F.axis_case()
    P, N, ns = X.shape
    rec = TomoGPU(ang, public(X), gpu_id=0)
    rec.set_alignment(np.zeros((P, 2)), rotation_deg=-3.0)
    total = rec.refine_alignment(Nouter=1, max_shift=4, recon=lambda r: r.sirt(5, show_convergence=False))
    assert np.array_equal(rec.get_alignment_rotation()[0], np.full(P, -3.0)) and np.array_equal(total, rec.get_alignment())
    scratch = rec.ALIGN_SLOT + 5
    rec.tomo.sino_affine(rec.ALIGN_SLOT, scratch, affine_matrices(total.astype(np.float32), -3.0, 1.0, N, ns))
    assert np.array_equal(rec.tomo._sino(SINO_B), rec.tomo._sino(scratch))
    assert np.array_equal(RA.images(rec.tomo._sino(rec.ALIGN_SLOT), N), X)


def test_estimate_tilt_axis_rotation_follows_the_replay(gpu):
    from tomo_tv_amd.align import affine_matrices
    from tomo_tv_amd.reconstructor import TomoGPU
    c = F.AXIS_CASE
    ang, clean, X = F.axis_case()
    P, N, ns = X.shape
    want, k, border, g, sc = F.estimate(X, np.zeros((P, 2)), c["search_deg"], c["step_deg"])
    rec = TomoGPU(ang, public(X), gpu_id=0)
    got = rec.estimate_tilt_axis_rotation(c["search_deg"], c["step_deg"])
    grid, scores = rec.align_axis_scores
    print(f"GPU {got:.6f}, replay {want:.6f} degrees; largest relative score difference {np.max(np.abs(scores - sc) / sc):.2e}")
    assert np.array_equal(grid, g) and int(np.argmin(scores)) == k == F.AXIS_REPLAY["index"] and not rec.align_axis_at_border
    assert abs(got - want) <= 1e-3 and abs(got + c["phi0"]) <= 0.5 * c["step_deg"]
    # applied: the series is the kept copy under that rotation, and it is remembered
    assert np.array_equal(rec.get_alignment_rotation()[0], np.full(P, got)) and not rec.get_alignment().any()
    M = affine_matrices(np.zeros((P, 2)), got, 1.0, N, ns)
    assert np.all(np.abs(RA.images(rec.tomo._sino(0), N) - F.affine(X, M)[0]) <= F.bound(X, M))
    with pytest.raises(ValueError):
        rec.estimate_tilt_axis_rotation(search_deg=80.0)
