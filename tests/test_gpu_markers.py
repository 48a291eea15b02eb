"""Marker detection on the GPU through the C ABI, against tests/ref64_markers.py: the correlation element by element under its
a-priori bound, the peaks bit for bit, the refusals, the call sequences and TomoGPU.align_markers end to end.  Shapes (Nslice, Nray,
Nproj): 70 slices = one 64-slice chunk seam and six padding lanes, 33 rays = one row past a 32-row tile; 3 slices < any template."""
import ctypes

import numpy as np
import pytest

import ref64_markers as R
import sequences as S
import sequences_markers as SM
from test_gpu_align import public
from tomo_tv_amd import _lib, align
from tomo_tv_amd._lib import SINO_B, SINO_G, SINO_USER0, VOL_ORIGINAL

pytestmark = pytest.mark.gpu
F32 = np.float32
SHAPES = [(70, 33, 3), (3, 33, 3)]
IDS = ["seam70x33", "thin3"]
A_SLOT, D_SLOT, E_SLOT = 3, 4, 5          # TOMO_SINO_USER0 ...
VAR_FLOOR = 1e-4
_P = ctypes.c_void_p


def ptr(a):
    return a.ctypes.data_as(_P)


def make_series(P, N, ns, seed):
    """noise on a pedestal per projection, two bright blobs, and a flat region (rays 20.., slices 40..: exactly constant)"""
    rng = np.random.default_rng(seed)
    X = (rng.uniform(0.5, 1.5, (P, N, ns)) + 3.0 * np.arange(1, P + 1)[:, None, None]).astype(F32)
    r, s = np.meshgrid(np.arange(N), np.arange(ns), indexing="ij")
    for a in range(P):
        for r0, s0 in ((9 + a, ns // 3), (N - 7, min(ns - 1, 62 + a))):
            X[a] += (4.0 * np.exp(-((r - r0) ** 2 + (s - s0) ** 2) / 6.0)).astype(F32)
    X[:, 20:, 40:] = F32(3.75)
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
        self.put(spare, self.get(slot))
        self.eng.be.c("sino_diff_norm_sq", slot, spare, 1)
        return self.eng.be.scalars()[1] == 0.0


@pytest.fixture(scope="module", params=SHAPES, ids=IDS)
def case(request, gpu):
    return Case(request.param)


def bits(x):
    return np.ascontiguousarray(x, F32).view(np.uint32)


@pytest.mark.parametrize("Rt", [1, 2, 5, 8])
def test_ncc_every_element_within_its_bound(case, Rt):
    T = SM.template(Rt)                                                                     # entries of both signs
    assert (T < 0).any() and (T > 0).any()
    case.put(D_SLOT, make_series(case.P, case.N, case.ns, 99))
    case.eng.sino_template_ncc(A_SLOT, D_SLOT, T, var_floor=VAR_FLOOR)
    got = case.get(D_SLOT)
    want, bound, band = R.ncc(case.X, T, VAR_FLOOR)
    assert not band.any() and np.all(np.isfinite(bound))                                    # no element near the flat-window threshold
    err = np.abs(got.astype(np.float64) - want)
    print(f"R={Rt}: worst error / bound {float(np.max(err / np.maximum(bound, 1e-300))):.3f}, largest bound {bound.max():.3e}")
    assert np.all(err <= bound)
    if case.ns >= 2 * Rt + 1:
        if case.ns > 60:
            assert np.abs(want).max() > 0.25 and not got[:, 20 + Rt:case.N - Rt, 40 + Rt:case.ns - Rt].any()   # the flat region is zeroed
        assert not got[:, :Rt].any() and not got[:, :, :Rt].any() and not got[:, case.N - Rt:].any() and not got[:, :, case.ns - Rt:].any()
    else:
        assert not got.any()                                                                # the image is smaller than the template
    assert case.padding_is_zero(D_SLOT)
    assert np.array_equal(bits(got), bits(R.ncc_replay32(case.X, T, VAR_FLOOR)))            # the replay states the kernel's order
    assert np.array_equal(bits(case.get(A_SLOT)), bits(case.X))
    case.eng.sino_template_ncc(A_SLOT, D_SLOT, T, var_floor=VAR_FLOOR)
    assert np.array_equal(bits(case.get(D_SLOT)), bits(got))                                # the same bits from call to call


def plateau_series(P, N, ns):
    """integers with plateaus: one spanning the chunk seam (slices 62..66), one on the corner, ties across the window edge, a NaN"""
    rng = np.random.default_rng(3)
    X = rng.integers(0, 6, (P, N, ns)).astype(F32)
    if ns > 66:
        X[0, 10, 62:67] = 9.0
        X[1, 10:13, 63:66] = 9.0
        X[2, 5, 60], X[2, 5, 60 + 3] = 8.0, 8.0                                             # a tie just outside / inside the window
    X[0, 0, 0] = X[0, 0, 1] = X[0, 1, 0] = 7.0
    X[1, N - 1, ns - 1] = 7.0
    X[2, 20, 1] = np.nan
    X[2, 25, min(2, ns - 1)] = 6.5                                                          # a threshold equal to a sample value
    return X


@pytest.mark.parametrize("radius", [1, 2, 5, 8])
def test_peaks_bit_for_bit(case, radius):
    e = case.eng
    X = plateau_series(case.P, case.N, case.ns)
    case.put(D_SLOT, X)
    for thr in (6.5, 2.0):
        want_n, want = R.peaks(X, radius, thr)
        n, rec = e.sino_peaks(D_SLOT, radius, thr)
        assert np.array_equal(n, want_n) and n.sum() > 0
        for a in range(case.P):
            assert np.array_equal(rec[a], want[a]), (a, thr)
        assert np.array_equal(align.marker_positions(np.concatenate(rec)), R.positions(np.concatenate(want)))
    # a capacity below the count: the counts are true, and the wrapper's second call is complete
    want_n, want = R.peaks(X, 1, 2.0)
    assert want_n.max() > 2
    cnt, raw = np.zeros(case.P, np.int32), np.full((case.P, 2, 8), -1, np.int32)
    e.be.c("sino_peaks", D_SLOT, 1, 2.0, 2, ptr(cnt), ptr(raw))
    assert np.array_equal(cnt, want_n)
    n, rec = e.sino_peaks(D_SLOT, 1, 2.0, capacity=2)
    assert np.array_equal(n, want_n) and all(np.array_equal(rec[a], want[a]) for a in range(case.P))
    assert np.array_equal(bits(case.get(D_SLOT)[~np.isnan(X)]), bits(X[~np.isnan(X)]))      # the slot is only read


def test_refusals_leave_everything_as_it_was(case):
    from tomo_tv_amd.engine import tomoengine
    L, h, P, N, ns = case.eng.be.L, case.eng.be.h, case.P, case.N, case.ns
    sentinel = make_series(P, N, ns, 98)
    case.put(D_SLOT, sentinel)
    T, flat, bad = SM.template(2), np.full((5, 5), 2.5, F32), SM.template(2)
    bad[1, 1] = np.inf
    cnt, rec = np.full(P, -7, np.int32), np.full((P, 4, 8), -7, np.int32)
    f = ctypes.c_float
    arg = [L.tomo_sino_template_ncc(h, -1, D_SLOT, ptr(T), 2, f(0)), L.tomo_sino_template_ncc(h, A_SLOT, 43, ptr(T), 2, f(0)),
           L.tomo_sino_template_ncc(h, D_SLOT, D_SLOT, ptr(T), 2, f(0)), L.tomo_sino_template_ncc(h, A_SLOT, D_SLOT, None, 2, f(0)),
           L.tomo_sino_template_ncc(h, A_SLOT, D_SLOT, ptr(T), 0, f(0)), L.tomo_sino_template_ncc(h, A_SLOT, D_SLOT, ptr(T), 9, f(0)),
           L.tomo_sino_template_ncc(h, A_SLOT, D_SLOT, ptr(flat), 2, f(0)), L.tomo_sino_template_ncc(h, A_SLOT, D_SLOT, ptr(bad), 2, f(0)),
           L.tomo_sino_template_ncc(h, A_SLOT, D_SLOT, ptr(T), 2, f(-1.0)), L.tomo_sino_template_ncc(h, A_SLOT, D_SLOT, ptr(T), 2, f(np.nan)),
           L.tomo_sino_peaks(h, -1, 1, f(0), 4, ptr(cnt), ptr(rec)), L.tomo_sino_peaks(h, 43, 1, f(0), 4, ptr(cnt), ptr(rec)),
           L.tomo_sino_peaks(h, A_SLOT, 0, f(0), 4, ptr(cnt), ptr(rec)), L.tomo_sino_peaks(h, A_SLOT, 9, f(0), 4, ptr(cnt), ptr(rec)),
           L.tomo_sino_peaks(h, A_SLOT, 1, f(np.nan), 4, ptr(cnt), ptr(rec)), L.tomo_sino_peaks(h, A_SLOT, 1, f(0), 0, ptr(cnt), ptr(rec)),
           L.tomo_sino_peaks(h, A_SLOT, 1, f(0), 4, None, ptr(rec)), L.tomo_sino_peaks(h, A_SLOT, 1, f(0), 4, ptr(cnt), None)]
    assert arg == [1] * len(arg) and L.tomo_last_error()
    with pytest.raises(_lib.TomoError, match="error 1"):
        case.eng.sino_template_ncc(A_SLOT, D_SLOT, np.ones((3, 3), F32))
    with pytest.raises(ValueError):
        case.eng.sino_template_ncc(A_SLOT, D_SLOT, np.ones((3, 4), F32))
    # TOMO_ERR_STATE: a slab of a larger volume, then (on an engine of its own) released geometry
    case.eng.be.c("set_slab_edges", 1, 0)
    state = [L.tomo_sino_template_ncc(h, A_SLOT, D_SLOT, ptr(T), 2, f(0)), L.tomo_sino_peaks(h, A_SLOT, 1, f(0), 4, ptr(cnt), ptr(rec))]
    case.eng.be.c("set_slab_edges", 1, 1)
    gone = tomoengine(ns, N, np.deg2rad(np.linspace(-60, 60, P)), device=0)
    assert L.tomo_release_geometry(gone.be.h) == 0
    g = gone.be.h
    state += [L.tomo_sino_template_ncc(g, A_SLOT, D_SLOT, ptr(T), 2, f(0)), L.tomo_sino_peaks(g, A_SLOT, 1, f(0), 4, ptr(cnt), ptr(rec))]
    assert state == [3] * 4
    assert np.all(cnt == -7) and np.all(rec == -7)                                          # nothing was written
    assert np.array_equal(bits(case.get(D_SLOT)), bits(sentinel)) and np.array_equal(bits(case.get(A_SLOT)), bits(case.X))
    n, _ = case.eng.sino_peaks(A_SLOT, 2, 0.0)                                              # the engine is usable as before
    assert np.array_equal(n, R.peaks(case.X, 2, 0.0)[0])


def test_a_sharded_engine_refuses(gpu):
    from tomo_tv_amd.engine import tomoengine
    e = tomoengine(12, 16, np.deg2rad(np.linspace(-60, 60, 3)), device=0, sub_slabs=2)
    with pytest.raises(NotImplementedError):
        e.sino_template_ncc(SINO_B, SINO_USER0 + 1, SM.template(1))
    with pytest.raises(NotImplementedError):
        e.sino_peaks(SINO_B, 1, 0.0)


# ---- call sequences -----------------------------------------------------------------------------------------------------------
def _engine(gid):
    import test_gpu_sequences as G
    return G.engine(gid)


@pytest.mark.parametrize("gid", ["A", "C"])
def test_used_engine_gives_a_fresh_engines_bits(gpu, gid):
    want = SM.marker_calls(_engine(gid))
    e = _engine(gid)
    e.restart_recon()
    e.SIRT(2)
    S.align_calls(e)
    got = SM.marker_calls(e)
    assert got.keys() == want.keys()
    for k in want:
        assert np.array_equal(got[k], want[k]), k
    again = SM.marker_calls(e)
    for k in want:
        assert np.array_equal(again[k], want[k]), k
    X = R.images(e._sino(SINO_B), e.Ny)                                                      # ... and the right answer, not only a repeatable one
    assert np.array_equal(bits(R.images(want["ncc3"], e.Ny)), bits(R.ncc_replay32(X, SM.template(3), 1e-6)))
    assert np.array_equal(want["records_b"], np.concatenate(R.peaks(X, 2, 0.5)[1])) and want["count_b"].sum() > 0


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
            SM.marker_calls(e)
            e.sino_template_ncc(SINO_G, SINO_USER0 + 9, SM.template(2))
            e.sino_peaks(SINO_G, 2, 0.0)
            mid = e.get_volume()
            e.SIRT(1)
            first = e.get_volume()
            e.data_distance()
            e.sino_template_ncc(SINO_B, SINO_G, SM.template(2))                             # G is the destination: the claim goes
        else:
            mid = e.get_volume()
            e.SIRT(1)
            first = e.get_volume()
            e.data_distance()
        e.SIRT(1)
        out.append((mid, first, e.get_volume(), e.data_distance()))
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1]) and np.array_equal(out[0][2], out[1][2])
    assert out[0][3] == out[1][3] and np.abs(out[0][2]).max() > 0


# ---- end to end ---------------------------------------------------------------------------------------------------------------
def test_align_markers_end_to_end(gpu):
    """Six beads of radius 2 (N = 64, Nslice = 70, 15 angles in [-70, 70]), projected by ``create_projections``, distorted by
    ``sino_affine`` with seeded shifts |d| <= 4 and a 2 degree rotation.  The yardstick is the binary64 pipeline of
    tests/test_markers_cpu.py::test_end_to_end_yardstick (ref64_markers.E2E_SHIFT_ERR = 0.231 px, E2E_PHI_ERR = 0.138 degrees against
    the gauge-removed truth); the GPU result may be twice as far from the truth."""
    from tomo_tv_amd.engine import tomoengine
    from tomo_tv_amd.reconstructor import TomoGPU
    c = R.E2E
    N, ns, ang = c["N"], c["ns"], c["angles"]
    e = tomoengine(ns, N, np.deg2rad(ang), device=0)
    e.set_volume(R.bead_phantom(), VOL_ORIGINAL)
    e.create_projections()
    _, M, d_true, phi_true = R.e2e_distortion()
    e.sino_affine(SINO_B, A_SLOT, M)
    X = R.images(e._sino(A_SLOT), N)                                                         # the distorted series, downloaded
    rec = TomoGPU(ang, public(X), gpu_id=0)
    rec.tomo.restart_recon()
    rec.tomo.SIRT(30)
    dd_before = rec.tomo.data_distance()
    out = rec.align_markers(marker_radius=c["marker_radius"], R=c["R"], threshold=c["threshold"], search_radius=c["search_radius"],
                            min_views=c["min_views"])
    assert out is rec.marker_alignment and np.all(out["n_detected"] == 6) and len(out["tracks"]) == 6
    assert all(len(t) == len(ang) for t in out["tracks"])                                    # every bead in every projection
    replay = R.pipeline(R.ncc_replay32(X, align.marker_template(c["marker_radius"], c["R"]), 0.0))
    d_err, p_err = np.abs(out["shifts"] - replay["shifts"]).max(), abs(out["rotation_deg"] - replay["rotation_deg"])
    print(f"against the CPU replay: shifts {d_err:.3e} px, rotation {p_err:.3e} degrees")
    assert d_err <= 1e-6 and p_err <= 1e-6
    s_err = np.abs(out["shifts"] - R.remove_gauge(d_true, ang)).max()
    r_err = abs(out["rotation_deg"] - phi_true)
    print(f"against the truth: shifts {s_err:.4f} px (yardstick {R.E2E_SHIFT_ERR}), rotation {r_err:.4f} degrees (yardstick "
          f"{R.E2E_PHI_ERR}); residual rms {out['residual_rms']:.4f} px")
    assert s_err <= 2 * R.E2E_SHIFT_ERR and r_err <= 2 * R.E2E_PHI_ERR
    assert np.array_equal(rec.get_alignment(), out["shifts"]) and rec.recon is None
    assert np.allclose(rec.get_alignment_rotation()[0], out["rotation_deg"])
    rec.tomo.restart_recon()
    rec.tomo.SIRT(30)
    dd_after = rec.tomo.data_distance()
    print(f"SIRT(30) data distance: distorted {dd_before:.4e}, aligned {dd_after:.4e}")
    assert dd_after < dd_before
