"""Dual-axis tomography on the GPU: ``tomo_volume_cross`` bit for bit, ``tomo_volume_cross_axpy`` against binary64 to one ulp, the zero
padding, the projection through the crossed volume, stream ordering, every refusal, and ``DualAxisTomo`` against the binary64 replay
(tests/ref64_dual.py).  Cubes: N = 8 (less than a wave, pitch 64), 40 (a multiple of 8, not of the 64 x 64 tile), 64 (exactly one tile
per plane: the path without guards), 70 (pitch 128, a partial second tile, N % 8 != 0 and N % 4 != 0), 130 (three tiles per axis)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import ref64 as R
import ref64_dual as D
from conftest import rel_l2
from test_bin_cpu import mixed

pytestmark = pytest.mark.gpu

SIZES = [8, 40, 64, 70, 130]
V0, V1 = 5, 6                               # TOMO_VOL_USER0 ..
ANG_A, ANG_B = np.linspace(-60, 60, 2), np.linspace(-50, 40, 3)      # degrees; Nproj may differ between the engines
ARG, STATE = 1, 3
SPECIAL = np.array([0x7fc00001, 0xffc12345, 0x7f800000, 0xff800000, 0x80000000, 0x00000001, 0x807fffff], np.uint32)
# two quiet NaNs with different payloads and signs, +Inf, -Inf, -0.0, the smallest and the largest (negative) denormal


def engine(ns, N, ang):
    from tomo_tv_amd.engine import tomoengine
    return tomoengine(ns, N, np.deg2rad(ang), device=0)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def edges(N):
    """corners, the neighbours of the corners, the middle, and both sides of a tile edge where the cube has one"""
    return sorted({0, 1, N // 2, N - 2, N - 1, min(63, N - 1), min(64, N - 1), min(127, N - 1), min(128, N - 1)})


def planted(N, seed):
    V = mixed((N, N, N), seed)
    u, k = V.view(np.uint32), 0
    for s in edges(N):
        for y in (0, N // 3, N - 1):
            for z in edges(N):
                u[s, y, z] = SPECIAL[k % len(SPECIAL)]
                k += 1
    return V


class Pair:
    def __init__(self, N):
        self.N, self.a, self.b = N, engine(N, N, ANG_A), engine(N, N, ANG_B)


@pytest.fixture(scope="module", params=SIZES, ids=[f"N{n}" for n in SIZES])
def pair(request, gpu):
    return Pair(request.param)


def usable(p):
    """both engines still reconstruct: one Landweber step each from a crossed volume gives a finite, non-zero volume"""
    N = p.N
    for eng, ang in ((p.a, ANG_A), (p.b, ANG_B)):
        eng._set_sino_local(np.abs(mixed((N, N * len(ang)), 3)))
        eng.restart_recon()
        eng.be.c("sirt_landweber", 0, 1.0 / eng.get_lipschitz(), 1)
        x = eng.get_volume(0)
        assert np.isfinite(x).all() and x.any()


def test_cross_moves_bits(pair):
    N, V = pair.N, planted(pair.N, 11)
    assert np.isnan(V).sum() > 8 and np.isinf(V).sum() > 8
    pair.a.set_volume(V, V0)
    assert np.array_equal(bits(pair.a.get_volume(V0)), bits(V))                      # (the upload and the download keep the bits)
    pair.b.set_volume(np.full((N, N, N), np.nan, np.float32), V1)                  # the destination is not read
    pair.a.cross_volume_to(pair.b, src=V0, dst=V1)
    got = pair.b.get_volume(V1)
    assert np.array_equal(bits(got), bits(D.cross(V)))
    assert np.isnan(got).sum() == np.isnan(V).sum()                                # no NaN but the transposed ones
    pair.b.cross_volume_to(pair.a, src=V1, dst=V1)                                 # twice: the source bits
    assert np.array_equal(bits(pair.a.get_volume(V1)), bits(V))
    pair.a.cross_volume_to(pair.b, src=V0, dst=V0)                                 # the same bits from run to run
    assert np.array_equal(bits(pair.b.get_volume(V0)), bits(got))
    assert np.array_equal(bits(pair.a.get_volume(V0)), bits(V))                      # the source was only read


def test_padding_of_the_destination_is_zero(pair):
    """The route of tests/test_gpu_bin.py: the real voxels uploaded into another slot (an upload writes zero padding) differ from the
    kernel's output by exactly nothing over the whole pitch; and the sum of |x| the engine forms over the whole pitch is the binary64
    sum over the N^3 voxels.  (No public call leaves non-zero padding behind, so a kernel that merely kept the padding cannot be told
    from one that writes it: that the stores cover the columns N .. pitch - 1 is read from the kernel)"""
    from tomo_tv_amd._lib import S_L1
    N, V = pair.N, mixed((pair.N,) * 3, 5)
    pair.a.set_volume(V, V0)
    D0 = mixed((N, N, N), 6)
    for axpy in (False, True):
        pair.b.set_volume(D0, V1)
        if axpy:
            pair.a.cross_axpy_volume_to(pair.b, -1.5, src=V0, dst=V1)
        else:
            pair.a.cross_volume_to(pair.b, src=V0, dst=V1)
        got = pair.b.get_volume(V1)
        pair.b.set_volume(got, V0)
        pair.b.be.c("diff_norm_sq", V0, V1, 1)
        assert pair.b.be.scalars()[1] == 0.0
        pair.b.be.c("l1_norm", V1)
        ref, bound = R.l1(got)
        R.assert_scalar("l1 over the pitch", pair.b.be.scalars()[S_L1], ref, bound)


def axpy_inputs(N):
    """half of the planes on a grid of 1/256 (every a * s + d below is then a binary32 number: bit equality), half random; Inf of
    both signs in the source and in the destination, a denormal and -0.0 in the destination"""
    S, Dst = mixed((N, N, N), 21), mixed((N, N, N), 22)
    S[::2] = np.round(S[::2] * 256) / 256
    Dst[:, ::2] = np.round(Dst[:, ::2] * 256) / 256
    e = edges(N)
    S[e[0], 0, e[-1]], S[e[-1], N - 1, e[0]], S[e[1], 0, e[1]] = np.inf, -np.inf, np.inf
    Dst[e[1], 0, e[1]] = np.inf                                                   # Inf + a * Inf
    Dst[e[2], N - 1, e[-1]], Dst[e[-1], 0, e[2]] = -np.inf, np.inf               # Inf in the destination alone
    Dst[0, 1, 0], Dst[0, 2, 0] = np.float32(2.0 ** -140), np.float32(-0.0)
    return S, Dst


@pytest.mark.parametrize("a", [0.0, 1.0, -0.75, 0.3])
def test_cross_axpy_to_one_ulp_and_bit_equal_where_exact(pair, a):
    N = pair.N
    S, Dst = axpy_inputs(N)
    pair.a.set_volume(S, V0)
    for clamp in (False, True):
        pair.b.set_volume(Dst, V1)
        pair.a.cross_axpy_volume_to(pair.b, a, clamp=clamp, src=V0, dst=V1)
        got = pair.b.get_volume(V1)
        ref = D.cross_axpy(S, Dst, a, clamp)
        nan = np.isnan(ref)
        # the rule as stated: IEEE fmaf, so a = 0 against an Inf is NaN (and Inf - Inf is); fmaxf takes a NaN to 0
        assert np.array_equal(np.isnan(got), nan) and (not clamp or not nan.any())
        assert clamp or a != 0.0 or nan.sum() >= 3                               # 0 * Inf, stated in the header
        inf = np.isinf(ref)
        assert np.array_equal(got[inf], ref[inf]) and inf.sum() >= 1                # Inf stays Inf
        fin = np.isfinite(ref)
        g, r = got[fin].astype(np.float64), ref[fin]
        assert np.all(np.abs(g - r) <= D.ulp32(r))
        exact = r.astype(np.float32).astype(np.float64) == r
        assert (a == 0.3 or exact.mean() > 0.2) and np.array_equal(g[exact], r[exact])
        print(f"N = {N}, a = {a}, clamp = {clamp}: {exact.mean():.2f} of the elements exact, worst error {np.max(np.abs(g - r) / D.ulp32(r)):.3f} ulp")
        if clamp:
            assert got.min() >= 0.0
        if a == 0.0 and not clamp:                                               # a = 0 keeps the destination's bits where the source is finite
            keep = np.isfinite(D.cross(S)) & (Dst != 0)
            assert np.array_equal(bits(got)[keep], bits(Dst)[keep]) and got[0, 1, 0] == np.float32(2.0 ** -140)
    # a NaN in the source: NaN without the clamp, 0 with it
    S2 = S.copy()
    S2[1, 1, 1] = np.nan
    pair.a.set_volume(S2, V0)
    for clamp in (False, True):
        pair.b.set_volume(Dst, V1)
        pair.a.cross_axpy_volume_to(pair.b, a, clamp=clamp, src=V0, dst=V1)
        v = pair.b.get_volume(V1)[1, 1, 1]
        assert v == 0.0 if clamp else np.isnan(v)


@pytest.mark.parametrize("N", [40, 70])
def test_projection_through_the_crossed_volume(gpu, N):
    from tomo_tv_amd._lib import SINO_G
    p = Pair(N)
    X = np.abs(mixed((N, N, N), 31))
    p.a.set_volume(X, 0)
    p.a.cross_volume_to(p.b)
    p.b.forward_projection()
    got = p.b._sino(SINO_G)
    M = R.Matrix(N, ANG_B)
    ref, bound, _ = M.fp_bound(D.cross(X))
    print(f"N = {N}: worst error / bound {R.ratio(got, ref, bound):.3f}")
    R.assert_within("FP_B(cross(X))", got, ref, bound)
    assert np.allclose(ref, D.fp_b(M, X))


def test_no_synchronise_is_needed_between_the_engines(gpu):
    N = 40
    p = Pair(N)
    p.a._set_sino_local(np.abs(mixed((N, N * len(ANG_A)), 41)))
    p.b._set_sino_local(np.abs(mixed((N, N * len(ANG_B)), 42)))
    ta, tb = 1.0 / p.a.get_lipschitz(), 1.0 / p.b.get_lipschitz()
    out = []
    for sync in (False, True):
        def wait():
            if sync:
                p.a.synchronize(), p.b.synchronize()
        p.a.restart_recon(), p.b.restart_recon()
        wait()
        for _ in range(20):
            p.a.be.c("sirt_landweber", 0, ta, 1)
            wait()
            p.a.cross_volume_to(p.b)
            wait()
            p.b.be.c("sirt_landweber", 0, tb, 1)
            wait()
            p.b.cross_volume_to(p.a)
            wait()
        out.append(p.a.get_volume(0))
    assert np.array_equal(bits(out[0]), bits(out[1])) and out[0].any()


def test_refusals_leave_both_engines_usable(gpu):
    from tomo_tv_amd import _lib
    from tomo_tv_amd.engine import tomoengine
    L = _lib.load()
    N = 8
    p = Pair(N)
    V = mixed((N, N, N), 51)
    p.a.set_volume(V, V0)
    p.b.set_volume(V, V1)
    ha, hb = p.a.be.h, p.b.be.h
    flat, other = engine(N + 1, N, ANG_B), engine(N + 8, N + 8, ANG_B)       # not a cube; a cube of another N

    def both(src, sv, dst, dv):
        return [L.tomo_volume_cross(src, sv, dst, dv), L.tomo_volume_cross_axpy(src, sv, dst, dv, 0.5, 0)]
    calls = (both(None, V0, hb, V1) + both(ha, V0, None, V1) + both(ha, V0, ha, V1) + both(ha, -1, hb, V1) + both(ha, 45, hb, V1) +
             both(ha, V0, hb, -1) + both(ha, V0, hb, 45) + both(flat.be.h, V0, hb, V1) + both(ha, V0, flat.be.h, V1) +
             both(ha, V0, other.be.h, V1) + both(other.be.h, V0, hb, V1))
    assert calls == [ARG] * len(calls) and L.tomo_last_error()
    if gpu > 1:                                                                  # different devices
        far = tomoengine(N, N, np.deg2rad(ANG_B), device=1)
        assert both(ha, V0, far.be.h, V1) == [ARG, ARG] and both(far.be.h, V0, ha, V1) == [ARG, ARG]
    # a slab of a larger volume (what a sharded engine is), as source and as destination
    p.b.be.c("set_slab_edges", 1, 0)
    assert both(ha, V0, hb, V1) == [STATE, STATE] and both(hb, V1, ha, V0) == [STATE, STATE] and b"slab" in L.tomo_last_error()
    p.b.be.c("set_slab_edges", 1, 1)
    with pytest.raises(NotImplementedError):                                     # the sharded classes refuse in Python already
        tomoengine(N, N, np.deg2rad(ANG_A), device=0, sub_slabs=2).cross_volume_to(p.b)
    # nothing was enqueued or written
    assert np.array_equal(bits(p.a.get_volume(V0)), bits(V)) and np.array_equal(bits(p.b.get_volume(V1)), bits(V))
    p.a.cross_volume_to(p.b, src=V0, dst=V1)
    assert np.array_equal(bits(p.b.get_volume(V1)), bits(D.cross(V)))
    usable(p)
    # released geometry: TOMO_ERR_STATE on either side; the other engine goes on
    gone = engine(N, N, ANG_B)
    assert L.tomo_release_geometry(gone.be.h) == 0
    assert both(ha, V0, gone.be.h, V1) == [STATE, STATE] and both(gone.be.h, V0, ha, V1) == [STATE, STATE]
    assert b"released" in L.tomo_last_error()
    usable(p)


def test_refuses_an_engine_with_a_communicator(gpu):
    """A one-rank RCCL communicator bound through the C ABI, in a fresh child process like the other one-rank tests."""
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(here, "dual_comm_script.py")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "DUAL_COMM_REFUSED_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ---- DualAxisTomo ----------------------------------------------------------------------------------------------------------------------
def public(b, N, P):
    """packed [slice][angle * N + ray] -> (Nslice, Nray, Nangles), what TomoGPU is given"""
    return np.ascontiguousarray(b.reshape(N, P, N).transpose(0, 2, 1))


@pytest.fixture(scope="module")
def driver(gpu):
    from tomo_tv_amd.dual_axis import DualAxisTomo
    N, ang = 32, np.linspace(-70, 70, 9)                                       # the geometry of tests/golden/A_N32_P9.npz
    M = R.Matrix(N, ang)
    X = D.phantom(N)
    bA, bB = D.fp_a(M, X).astype(np.float32), D.fp_b(M, X).astype(np.float32)
    dual = DualAxisTomo(ang, public(bA, N, 9), ang, public(bB, N, 9), gpu_id=0)
    return dict(N=N, M=M, X=X, bA=bA, bB=bB, dual=dual)


def test_driver_sirt_against_the_binary64_replay(driver):
    """The yardstick is the existing code: the worst element deviation of the single-axis ``sirt_landweber`` (20 iterations, the same
    data) from its own binary64 replay; the dual-axis loop (10 iterations: as many projector applications) may deviate at most twice as
    much from its replay -- the margin covers the second matrix and the differing order; ``cross`` itself adds no rounding.
    Recorded: see the two values printed below."""
    M, bA, bB, dual = driver["M"], driver["bA"], driver["bB"], driver["dual"]
    ta, tb = dual.a.tomo, dual.b.tomo
    tA, tB = float(np.float32(1.0 / ta.get_lipschitz())), float(np.float32(1.0 / tb.get_lipschitz()))
    ta.restart_recon()
    ta.be.c("sirt_landweber", 0, tA, 20)
    dev_single = float(np.max(np.abs(ta.get_volume(0).astype(np.float64) - D.single_axis(M, bA, tA, 20))))
    cost = dual.sirt(10)
    got = dual.get_recon()
    ref = D.dual_axis(M, M, bA, bB, tA, tB, 10)
    dev_dual = float(np.max(np.abs(got - ref)))
    print(f"worst element deviation from the binary64 replay: single-axis (20 iterations) {dev_single:.3e}, dual-axis (10) {dev_dual:.3e}")
    assert dev_single > 0 and dev_dual <= 2 * dev_single
    assert got.shape == (32, 32, 32) and got.dtype == np.float64
    # the costs: the two data distances of the volume of record after every iteration
    dd = (float(np.sqrt(np.sum((D.fp_a(M, ref) - bA) ** 2))), float(np.sqrt(np.sum((D.fp_b(M, ref) - bB) ** 2))))
    assert cost.shape == (10, 2) and cost[-1].sum() < cost[0].sum()
    assert abs(cost[-1, 0] - dd[0]) <= 2e-5 * dd[0] and abs(cost[-1, 1] - dd[1]) <= 2e-5 * dd[1]
    again = dual.data_distance()
    assert np.allclose(again, cost[-1], rtol=1e-6, atol=0)
    # B's volume is the crossed volume of record; a second run gives the same bits; the tensor form is A's volume
    assert np.array_equal(bits(tb.get_volume(0)), bits(D.cross(ta.get_volume(0))))
    first = ta.get_volume(0)
    dual.sirt(10, show_convergence=False)
    assert np.array_equal(bits(ta.get_volume(0)), bits(first))
    assert np.array_equal(dual.get_recon(as_tensor=True).cpu().numpy(), first)
    dual.sirt(1, restart=False)                                                # goes on from the volume of record
    eleven = ta.get_volume(0)
    dual.sirt(11, show_convergence=False)
    assert np.array_equal(bits(ta.get_volume(0)), bits(eleven)) and not np.array_equal(eleven, first)


def test_driver_sart_and_pass_throughs(driver):
    M, X, bA, bB, dual = driver["M"], driver["X"], driver["bA"], driver["bB"], driver["dual"]
    cost = dual.sart(3, beta=0.5)
    got = dual.get_recon()
    x = np.zeros_like(X)
    for _ in range(3):
        x = M.sart(x, bA, 0.5)
        x = D.cross(M.sart(D.cross(x), bB, 0.5))
    assert rel_l2(got, x) < 1e-5
    assert cost.shape == (3, 2) and cost[-1].sum() < cost[0].sum()
    tv0 = dual.tv_fgp(3, 0.05)
    assert tv0 > 0 and dual.tv_gd(2, 0.01) > 0 and np.isfinite(dual.get_recon()).all()


def test_combine_of_two_single_axis_runs(driver):
    dual = driver["dual"]
    dual.a.sirt(5, show_convergence=False)
    dual.b.sirt(5, show_convergence=False)
    ra, rb = dual.a.tomo.get_volume(0), dual.b.tomo.get_volume(0)
    assert ra.any() and rb.any() and not np.array_equal(ra, D.cross(rb))
    dual.combine(0.5)
    got = dual.a.tomo.get_volume(0).astype(np.float64)
    ref = 0.5 * ra.astype(np.float64) + 0.5 * D.cross(rb).astype(np.float64)
    assert np.all(np.abs(got - ref) <= D.ulp32(ref))
    dual.a.tomo.set_volume(ra, 0)
    # 0.75 ra rounds once, the fma once: half an ulp of 0.75 ra and half an ulp of the result, which is the larger (both volumes >= 0)
    dual.combine(0.25)
    got = dual.a.tomo.get_volume(0).astype(np.float64)
    ref = 0.75 * ra.astype(np.float64) + 0.25 * D.cross(rb).astype(np.float64)
    assert np.all(np.abs(got - ref) <= D.ulp32(ref))


def test_driver_takes_device_tensors(driver):
    import torch
    from tomo_tv_amd.dual_axis import DualAxisTomo
    N, bA, bB = driver["N"], driver["bA"], driver["bB"]
    ang = np.linspace(-70, 70, 9)
    host = driver["dual"]
    host.sirt(2, show_convergence=False)
    dev = DualAxisTomo(ang, torch.from_numpy(public(bA, N, 9)).to("cuda:0"), ang, torch.from_numpy(public(bB, N, 9)).to("cuda:0"))
    assert dev.a.tomo.gpuID == 0 and dev.b.tomo.gpuID == 0
    dev.sirt(2, show_convergence=False)
    assert np.array_equal(dev.get_recon(), host.get_recon())
    with pytest.raises(ValueError):
        DualAxisTomo(ang, public(bA, N, 9)[:, :30], ang, public(bB, N, 9), gpu_id=0)
