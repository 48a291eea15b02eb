"""Binning and prolongation on the GPU: every output element against tests/ref64_bin.py within its derived bound, the bit identities,
stream ordering, engine state, argument errors, and the drivers ``TomoGPU.binned`` / ``coarse_to_fine`` / ``refine_alignment(pyramid=)``.
Shapes: a partial bin, a coarse width that crosses a 64-lane chunk on both sides, an odd coarse N with a trailing bin of 2, full bins."""
import ctypes

import numpy as np
import pytest

import ref64_align as RA
import ref64_bin as B
from conftest import rel_l2
from test_bin_cpu import CONST, mixed
from test_gpu_parity import TOL            # the tolerance SIRT at these iteration counts is held to against the oracle

pytestmark = pytest.mark.gpu

SHAPES = [(2, 8, 5, 3), (2, 16, 130, 2), (4, 12, 70, 3), (4, 16, 64, 2)]          # (f, N, Nslice, P)
IDS = ["f2_partial", "f2_chunks", "f4_odd_tail2", "f4_full"]
U0, U1 = 3, 4                               # TOMO_SINO_USER0 ..
V0, V1 = 5, 6                               # TOMO_VOL_USER0 ..


def engine(ns, N, P):
    from tomo_tv_amd.engine import tomoengine
    return tomoengine(ns, N, np.deg2rad(np.linspace(-60, 60, P)), device=0)


def put_sino(eng, slot, X):
    b = RA.packed(np.asarray(X, np.float32))
    eng.be.c("set_sinogram", slot, b.ctypes.data_as(ctypes.c_void_p))


def get_sino(eng, slot):
    return RA.images(eng._sino(slot), eng.Ny)


class Case:
    def __init__(self, f, N, ns, P):
        self.f, self.N, self.ns, self.P, self.nc = f, N, ns, P, -(-ns // f)
        self.fine, self.coarse = engine(ns, N, P), engine(self.nc, N // f, P)
        self.X, self.V, self.C = mixed((P, N, ns), 7 * N), mixed((ns, N, N), 7 * N + 1), mixed((self.nc, N // f, N // f), 7 * N + 2)


@pytest.fixture(scope="module", params=SHAPES, ids=IDS)
def case(request, gpu):
    return Case(*request.param)


def inside(got, ref, bound, what):
    fin = np.isfinite(ref)
    assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(got[~fin & ~np.isnan(ref)], ref[~fin & ~np.isnan(ref)]), what
    err = np.abs(got.astype(np.float64)[fin] - ref[fin])
    print(f"{what}: worst error / bound {np.max(err / np.maximum(bound[fin], 1e-300)):.3f}")
    assert np.all(err <= bound[fin]), what


def test_every_element_within_its_bound(case):
    f = case.f
    X, V, C = case.X.copy(), case.V.copy(), case.C.copy()
    X[-1, 3, case.ns - 1] = V[case.ns - 1, 2, 3] = C[0, 0, 0] = np.inf          # one Inf each: in the trailing bin, at a clamped corner
    put_sino(case.fine, U0, X)
    case.fine.bin_sinogram_to(case.coarse, f, src=U0, dst=U1)
    got = get_sino(case.coarse, U1)
    inside(got, *B.bin_sino(X, f), "sino_bin")
    assert np.isinf(got[-1, 3 // f, -1]) and not np.isnan(got).any()
    case.fine.set_volume(V, V0)
    case.fine.bin_volume_to(case.coarse, f, src=V0, dst=V1)
    got = case.coarse.get_volume(V1)
    inside(got, *B.bin_volume(V, f), "volume_bin")
    assert np.isinf(got[-1, 2 // f, 3 // f]) and not np.isnan(got).any()
    case.coarse.set_volume(C, V0)
    case.coarse.prolong_volume_to(case.fine, f, src=V0, dst=V1)
    got = case.fine.get_volume(V1)
    inside(got, *B.prolong(C, f, case.ns), "volume_prolong")
    assert np.all(got[:f // 2, :f // 2, :f // 2] == np.inf)                        # the clamped copies of the Inf corner stay Inf
    if case.ns % f == 0:                                                           # (a partial last bin: the last fine slice has two taps)
        assert got[-1, -1, -1] == C[-1, -1, -1]
    # the same bits from run to run
    case.coarse.prolong_volume_to(case.fine, f, src=V0, dst=V0)
    assert np.array_equal(case.fine.get_volume(V0), got, equal_nan=True)


def test_bit_identities_and_zero_padding(case):
    f = case.f
    case.coarse.set_volume(np.full((case.nc, case.N // f, case.N // f), np.float32(0.3)), V0)
    case.coarse.prolong_volume_to(case.fine, f, src=V0, dst=V1)
    fine = case.fine.get_volume(V1)
    assert np.all(fine == np.float32(0.3))
    put_sino(case.fine, U0, np.full((case.P, case.N, case.ns), CONST))
    case.fine.bin_sinogram_to(case.coarse, f, src=U0, dst=U1)
    got = get_sino(case.coarse, U1)
    k = B.counts(case.ns, f)
    assert np.all(got[:, :, (k & (k - 1)) == 0] == CONST / np.float32(f))
    # padding of the destinations: the real samples uploaded into another slot (an upload writes zero padding) differ from the
    # kernel's output by exactly nothing over the whole pitch
    put_sino(case.coarse, U0, got)
    case.coarse.be.c("sino_diff_norm_sq", U0, U1, 1)
    assert case.coarse.be.scalars()[1] == 0.0
    case.fine.set_volume(fine, V0)
    case.fine.be.c("diff_norm_sq", V0, V1, 1)
    assert case.fine.be.scalars()[1] == 0.0
    case.fine.set_volume(case.V, V0)
    case.fine.bin_volume_to(case.coarse, f, src=V0, dst=V1)
    case.coarse.set_volume(case.coarse.get_volume(V1), V0)
    case.coarse.be.c("diff_norm_sq", V0, V1, 1)
    assert case.coarse.be.scalars()[1] == 0.0


def test_no_synchronise_is_needed_between_the_engines(case):
    from tomo_tv_amd._lib import SINO_B, SINO_G, VOL_RECON
    f = case.f
    B0 = np.abs(case.X)
    put_sino(case.fine, SINO_B, B0)
    out = []
    for sync in (False, True):
        case.coarse.restart_recon()
        case.fine.bin_sinogram_to(case.coarse, f)
        if sync:
            case.fine.synchronize(), case.coarse.synchronize()
        case.coarse.SIRT(1)
        case.coarse.forward_projection()
        g = get_sino(case.coarse, SINO_G)
        case.coarse.prolong_volume_to(case.fine, f)
        if sync:
            case.fine.synchronize(), case.coarse.synchronize()
        case.fine.SIRT(1)
        out.append((g, case.fine.get_volume(VOL_RECON)))
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1]) and out[0][1].any()


def test_prolongation_drops_the_projection_in_hand(case):
    put_sino(case.fine, 0, np.abs(case.X))
    case.fine.restart_recon()
    case.fine.SIRT(1)
    before = case.fine.data_distance()                  # G = A * recon is in hand now
    case.coarse.set_volume(np.abs(case.C), 0)
    case.coarse.prolong_volume_to(case.fine, case.f)
    after = case.fine.data_distance()
    case.fine.set_option("fp_reuse", 0)
    try:
        case.fine.forward_projection()
        fresh = case.fine.data_distance()
    finally:
        case.fine.set_option("fp_reuse", 1)
    assert after == fresh and after != before


def test_argument_errors_leave_both_engines_usable(case):
    from tomo_tv_amd import _lib
    f, L, hf, hc = case.f, case.fine.be.L, case.fine.be.h, case.coarse.be.h
    put_sino(case.fine, U0, case.X)
    case.fine.bin_sinogram_to(case.coarse, f, src=U0, dst=U1)
    good = get_sino(case.coarse, U1)
    other = engine(case.nc + 1, case.N // f, case.P)            # mismatched Nslice
    rays = engine(case.nc, case.N // f + 1, case.P)             # Nray that f times does not give
    angles = engine(case.nc, case.N // f, case.P + 1)           # mismatched Nangles
    calls = [L.tomo_sino_bin(hf, U0, hc, U1, 3), L.tomo_sino_bin(hf, U0, hc, U1, 6 - f), L.tomo_sino_bin(hf, U0, other.be.h, U1, f),
             L.tomo_sino_bin(hf, U0, rays.be.h, U1, f), L.tomo_sino_bin(hf, U0, hf, U1, f), L.tomo_sino_bin(hf, U0, angles.be.h, U1, f),
             L.tomo_sino_bin(hf, 43, hc, U1, f), L.tomo_sino_bin(hf, U0, hc, -1, f), L.tomo_sino_bin(None, U0, hc, U1, f),
             L.tomo_volume_bin(hf, V0, hc, 45, f), L.tomo_volume_bin(hf, V0, hc, V1, 0), L.tomo_volume_bin(hf, V0, other.be.h, V1, f),
             L.tomo_volume_bin(hc, V0, hc, V1, f), L.tomo_volume_prolong(hc, V0, hf, -1, f), L.tomo_volume_prolong(hf, V0, hc, V1, f),
             L.tomo_volume_prolong(hc, V0, hc, V1, f), L.tomo_volume_prolong(rays.be.h, V0, hf, V1, f)]
    assert calls == [1] * len(calls) and L.tomo_last_error()
    with pytest.raises(_lib.TomoError):
        case.fine.bin_sinogram_to(case.coarse, 3)
    assert np.array_equal(get_sino(case.coarse, U1), good) and np.array_equal(get_sino(case.fine, U0), case.X)      # nothing was touched
    case.fine.bin_sinogram_to(case.coarse, f, src=U0, dst=U1)
    assert np.array_equal(get_sino(case.coarse, U1), good)
    inside(good, *B.bin_sino(case.X, f), "sino_bin after the refused calls")


# ---- TomoGPU -------------------------------------------------------------------------------------------------------------------------
def public(X):
    return np.ascontiguousarray(np.asarray(X).transpose(2, 1, 0))


@pytest.fixture(scope="module")
def series(gpu):
    """32 x 32 x 9 (Nslice 30: a partial bin at factor 4): a phantom's projections by the oracle"""
    c = dict(RA.REFINE_CASE, nslice=30)
    ang, clean, _, _ = RA.refine_case(c)
    return ang, clean


def oracle_of(ang, X):
    import oracle
    P, N, ns = X.shape
    o = oracle.ctvlib(ns, N, P)
    o.load_A(oracle.parallel_ray(N, ang))
    o.set_tilt_series(RA.packed(X))
    return o


def test_binned_sirt_equals_the_oracle_on_the_numpy_binned_series(series):
    from tomo_tv_amd.reconstructor import TomoGPU
    ang, X = series
    rec = TomoGPU(ang, public(X), gpu_id=0)
    with pytest.raises(ValueError):
        rec.binned(3)
    c = rec.binned(2)
    assert (c.Nslice, c.Nray, c.Nangles) == (15, 16, 9) and c.tomo.gpuID == rec.tomo.gpuID
    Xc = B.bin_replay_f32(X, 2)
    assert np.array_equal(c.get_projections(), public(Xc))
    c.sirt(5)
    o = oracle_of(ang, Xc)
    o.SIRT_norm(5)
    assert rel_l2(c.get_recon(), o.recon) < TOL
    odd = TomoGPU(ang, public(X[:, :30]), gpu_id=0)
    with pytest.raises(ValueError):
        odd.binned(4)


def test_coarse_to_fine_equals_the_calls_by_hand_and_the_cpu_restatement(series):
    from tomo_tv_amd.reconstructor import TomoGPU
    ang, X = series
    rec = TomoGPU(ang, public(X), gpu_id=0)
    costs = rec.coarse_to_fine((2,), Niter=(10, 5))
    got = rec.get_recon()
    fine = TomoGPU(ang, public(X), gpu_id=0).tomo
    coarse = fine.binned_engine(2)
    fine.bin_sinogram_to(coarse, 2)
    coarse.restart_recon()
    dd = []
    for t, n in ((coarse, 10), (fine, 5)):
        if t is fine:
            coarse.prolong_volume_to(fine, 2)
        for _ in range(n):
            t.SIRT(1)
            dd.append(t.data_distance())
    assert np.array_equal(fine.get_volume().astype(np.float64), got) and np.array_equal(np.concatenate(costs), dd)
    oc, of = oracle_of(ang, B.bin_replay_f32(X, 2)), oracle_of(ang, X)
    oc.SIRT_norm(10)
    of.recon[:] = B.prolong(oc.recon, 2, 30)[0]
    of.SIRT_norm(5)
    assert rel_l2(got, of.recon) < TOL
    assert abs(costs[1][-1] - of.data_distance(normalize=False)) <= 2e-5 * costs[1][-1]
    assert costs[1][0] < oracle_first_cost(ang, X)                      # the warm start is ahead of a start from zero


def oracle_first_cost(ang, X):
    o = oracle_of(ang, X)
    o.SIRT_norm(1)
    return o.data_distance(normalize=False)


def test_refine_alignment_pyramid_follows_the_cpu_replay_and_recovers(gpu):
    from tomo_tv_amd.reconstructor import TomoGPU
    c = B.PYRAMID_CASE
    ang, clean, X, inj = B.pyramid_case()
    rec = TomoGPU(ang, public(X), gpu_id=0)
    total = rec.refine_alignment(Nouter=c["nouter"], max_shift=c["max_shift"], subpixel=False, pyramid=c["pyramid"],
                                 recon=lambda r: r.sirt(c["niter"], show_convergence=False))
    hist, pks, borders = B.pyramid_replay(ang, X, c["pyramid"], c["nouter"], c["max_shift"], c["niter"])
    assert len(rec.align_history) == len(hist) == 3 * c["nouter"]
    for k in range(len(hist)):
        assert np.array_equal(rec.align_int_peaks[k], pks[k]) and np.array_equal(rec.align_peaks[k], pks[k]), k
        assert np.array_equal(rec.align_history[k], hist[k]) and np.array_equal(rec.align_at_border[k], borders[k]), k
    assert np.array_equal(total, hist[-1]) and np.array_equal(rec.get_projections(), public(RA.shift_int(X, total)))
    rr, rs = RA.gauge_residual(total, inj, ang)
    print(f"left outside the gauge: {np.abs(rr).max():.3f} rays, {np.abs(rs).max():.3f} slices")
    assert np.abs(rr).max() <= 1.0 and np.abs(rs).max() <= 1.0


def test_device_tensor_series_gives_the_host_paths_binned_bits(series):
    import torch
    from tomo_tv_amd.reconstructor import TomoGPU
    ang, X = series
    host = TomoGPU(ang, public(X), gpu_id=0).binned(4)
    dev = TomoGPU(ang, torch.from_numpy(public(X)).to("cuda:0"), gpu_id=0).binned(4)
    assert host.Nslice == 8 and np.array_equal(dev.get_projections(), host.get_projections())
    assert np.array_equal(host.get_projections(), public(B.bin_replay_f32(X, 4)))
