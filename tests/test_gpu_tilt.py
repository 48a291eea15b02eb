"""The tilt-angle refinement on the GPU: ``tomo_volume_rot_derivative`` element by element inside its a-priori bound,
``tomo_sino_tilt_normal`` per projection inside the binary64 accumulation bound (tests/ref64_tilt.py), exact counts, every refusal
with its status and untouched bits, a used engine against a fresh one, the claim on the model sinogram, and
``TomoGPU.refine_tilt_angles`` end to end at full resolution and at ``factor=2``.
Shapes (Nslice, N): (5, 9) odd N, thinner than a wave; (64, 16) one full chunk; (70, 32) a chunk plus a remainder; (1, 8) one slice."""
import ctypes

import numpy as np
import pytest

import ref64_align as RA
import ref64_tilt as T
import sequences_tilt  # noqa: F401  (registers this feature's rows of the call-sequence closure table)

pytestmark = pytest.mark.gpu

VOL_RECON, VOL_TEMP, VOL_ORIGINAL, VOL_YK, VOL_RECON_OLD, VOL_USER0 = 0, 1, 2, 3, 4, 5
SINO_B, SINO_G = 0, 1
B_SLOT, G_SLOT, D_SLOT = 3, 4, 5                    # TOMO_SINO_USER0 ...
ARG, STATE = 1, 3
VSHAPES = [(5, 9), (64, 16), (70, 32), (1, 8)]
SSHAPES = [(5, 9, 5), (64, 16, 5), (70, 32, 9)]


def engine(ns, N, P=3):
    from tomo_tv_amd.engine import tomoengine
    return tomoengine(ns, N, np.deg2rad(np.linspace(-60, 60, P)), device=0)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def lib():
    from tomo_tv_amd import _lib
    return _lib.load()


def volumes(ns, N):
    """name -> float32 volume [s][i][j]: random, constant, radially symmetric, one nonzero voxel on the border"""
    rng = np.random.default_rng(100 * N + ns)
    X, Y = T._coords(N)
    one = np.zeros((ns, N, N), np.float32)
    one[ns // 2, 0, N // 2 - 1] = 2.5
    one[0, N - 2, N - 1] = -1.5
    return {"random": rng.standard_normal((ns, N, N)).astype(np.float32),
            "constant": np.full((ns, N, N), 3.25, np.float32),
            "radial": np.broadcast_to(np.exp(-(X ** 2 + Y ** 2) / (0.08 * N * N)), (ns, N, N)).astype(np.float32),
            "border": one}


@pytest.fixture(scope="module", params=VSHAPES, ids=[f"{s}x{n}" for s, n in VSHAPES])
def vcase(request, gpu):
    ns, N = request.param
    return engine(ns, N), volumes(ns, N)


def test_rot_derivative_element_by_element(vcase):
    eng, vols = vcase
    for name, f in vols.items():
        eng.set_volume(f, VOL_RECON)
        eng.volume_rot_derivative()
        got = eng.get_volume(VOL_TEMP).astype(np.float64)
        ref, bnd = T.rot_derivative(f), T.rot_derivative_bound(f)
        ratio = float(np.max(np.abs(got - ref) / bnd))
        print(f"{f.shape} {name}: worst error / bound {ratio:.3f}")
        assert ratio <= 1.0, name
        assert np.array_equal(bits(eng.get_volume(VOL_RECON)), bits(f))                       # the source is only read
        if name == "constant":
            assert not got.any()                                                               # exact zeros
        if name == "border":                                                                   # the border rule, exactly
            assert np.array_equal(got, ref) and np.count_nonzero(got) == np.count_nonzero(ref) > 0
        if name == "random":                                                                   # the kernel's own order of operations
            assert np.array_equal(bits(got.astype(np.float32)), bits(T.rot_derivative_f32(f)))


def test_every_slot_pair_gives_the_default_pairs_bits(vcase):
    eng, vols = vcase
    f = vols["random"]
    eng.set_volume(f, VOL_RECON)
    eng.volume_rot_derivative()
    base = bits(eng.get_volume(VOL_TEMP))
    slots = [VOL_RECON, VOL_TEMP, VOL_ORIGINAL, VOL_YK, VOL_RECON_OLD, VOL_USER0, VOL_USER0 + 39]
    for src in slots:
        for dst in slots:
            if src == dst:
                continue
            eng.set_volume(f, src)
            eng.set_volume(np.full_like(f, 7.0), dst)
            eng.volume_rot_derivative(src, dst)
            assert np.array_equal(bits(eng.get_volume(dst)), base), (src, dst)
            assert np.array_equal(bits(eng.get_volume(src)), bits(f)), (src, dst)


def smooth(P, N, ns, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((P, N, ns)) + 2.0).astype(np.float32)


def put(eng, slot, X):
    b = RA.packed(np.asarray(X, np.float32))
    eng.be.c("set_sinogram", slot, b.ctypes.data_as(ctypes.c_void_p))


def get(eng, slot):
    return RA.images(eng._sino(slot), eng.Ny)


def raw(eng, b, g, d, margin, fill=np.nan):
    out = np.full((eng.Nproj, 4), fill)
    rc = lib().tomo_sino_tilt_normal(eng.be.h, b, g, d, int(margin), out.ctypes.data_as(ctypes.c_void_p))
    return rc, out


@pytest.fixture(scope="module", params=SSHAPES, ids=[f"{s}x{n}x{p}" for s, n, p in SSHAPES])
def scase(request, gpu):
    ns, N, P = request.param
    eng = engine(ns, N, P)
    X = [smooth(P, N, ns, 11 * N + k) for k in range(3)]
    for slot, x in zip((B_SLOT, G_SLOT, D_SLOT), X):
        put(eng, slot, x)
    return eng, X


@pytest.mark.parametrize("margin", [0, 1, 3])
def test_tilt_normal_against_binary64(scase, margin):
    eng, (B, G, D) = scase
    ns, N = eng.Nslice_, eng.Ny
    if 2 * margin >= min(ns, N):
        rc, out = raw(eng, B_SLOT, G_SLOT, D_SLOT, margin)
        assert rc == ARG and np.isnan(out).all()                                             # nothing is left: refused, nothing written
        return
    ref, bnd = T.tilt_normal_bound(B, G, D, margin)
    rc, got = raw(eng, B_SLOT, G_SLOT, D_SLOT, margin)
    assert rc == 0
    assert np.array_equal(got[:, 3], ref[:, 3]) and np.all(got[:, 3] == (N - 2 * margin) * (ns - 2 * margin))     # the count is exact
    ratio = np.abs(got[:, :3] - ref[:, :3]) / bnd[:, :3]
    rel = np.abs(got[:, :3] - ref[:, :3]) / np.abs(ref[:, :3])
    print(f"{(ns, N, eng.Nproj)} margin {margin}: worst error / bound {ratio.max():.3f}, worst relative error {rel.max():.2e}")
    assert ratio.max() <= 1.0
    rd, dd, rr, count = eng.sino_tilt_normal(B_SLOT, G_SLOT, D_SLOT, margin=margin)           # the Python call: the same numbers
    assert np.array_equal(rd, got[:, 0]) and np.array_equal(dd, got[:, 1]) and np.array_equal(rr, got[:, 2])
    assert count.dtype == np.int64 and np.array_equal(count, got[:, 3].astype(np.int64))
    rc, again = raw(eng, B_SLOT, G_SLOT, D_SLOT, margin)                                      # the same bits from call to call
    assert np.array_equal(again.view(np.uint64), got.view(np.uint64))
    for slot, x in zip((B_SLOT, G_SLOT, D_SLOT), (B, G, D)):                                  # nothing written
        assert np.array_equal(bits(get(eng, slot)), bits(x))


def test_samples_outside_the_margin_are_not_looked_at(scase):
    eng, (B, G, D) = scase
    base = raw(eng, B_SLOT, G_SLOT, D_SLOT, 1)[1]
    Bp, Dp = B.copy(), D.copy()
    Bp[:, 0, :], Bp[:, :, -1], Dp[:, -1, :], Dp[:, :, 0] = np.inf, np.nan, np.nan, np.inf
    put(eng, B_SLOT, Bp), put(eng, D_SLOT, Dp)
    out = raw(eng, B_SLOT, G_SLOT, D_SLOT, 1)[1]
    put(eng, B_SLOT, B), put(eng, D_SLOT, D)
    assert np.array_equal(out.view(np.uint64), base.view(np.uint64))


def test_refusals_leave_the_destination_untouched(gpu):
    eng = engine(6, 12, 4)
    L = lib()
    f = volumes(6, 12)["random"]
    eng.set_volume(f, VOL_RECON), eng.set_volume(f + 1, VOL_TEMP)
    for src, dst in ((VOL_RECON, VOL_RECON), (VOL_TEMP, VOL_TEMP), (-1, VOL_TEMP), (VOL_RECON, 45), (45, VOL_TEMP), (VOL_RECON, -1)):
        assert L.tomo_volume_rot_derivative(eng.be.h, src, dst) == ARG and L.tomo_last_error(), (src, dst)
    assert L.tomo_volume_rot_derivative(None, 0, 1) == ARG
    assert np.array_equal(bits(eng.get_volume(VOL_RECON)), bits(f)) and np.array_equal(bits(eng.get_volume(VOL_TEMP)), bits(f + 1))
    with pytest.raises(Exception):
        eng.volume_rot_derivative(VOL_TEMP, VOL_TEMP)
    X = smooth(4, 12, 6, 5)
    for slot in (B_SLOT, G_SLOT, D_SLOT):
        put(eng, slot, X)
    for args in ((-1, G_SLOT, D_SLOT, 1), (B_SLOT, 43, D_SLOT, 1), (B_SLOT, G_SLOT, 1000, 1), (B_SLOT, G_SLOT, D_SLOT, -1),
                 (B_SLOT, G_SLOT, D_SLOT, 3), (B_SLOT, G_SLOT, D_SLOT, 100)):
        rc, out = raw(eng, *args)
        assert rc == ARG and np.isnan(out).all(), args
    assert L.tomo_sino_tilt_normal(eng.be.h, B_SLOT, G_SLOT, D_SLOT, 1, None) == ARG
    with pytest.raises(ValueError):
        eng.sino_tilt_normal(B_SLOT, G_SLOT, D_SLOT, margin=3)
    # a slab of a larger volume: TOMO_ERR_STATE from both, nothing written
    eng.be.c("set_slab_edges", 1, 0)
    assert L.tomo_volume_rot_derivative(eng.be.h, VOL_RECON, VOL_TEMP) == STATE
    rc, out = raw(eng, B_SLOT, G_SLOT, D_SLOT, 1)
    assert rc == STATE and np.isnan(out).all()
    eng.be.c("set_slab_edges", 1, 1)
    assert np.array_equal(bits(eng.get_volume(VOL_TEMP)), bits(f + 1))
    rc, out = raw(eng, B_SLOT, G_SLOT, D_SLOT, 1)
    assert rc == 0 and np.all(out[:, 3] == 10 * 4)


def test_sharded_engines_refuse(gpu):
    from tomo_tv_amd.engine import tomoengine
    grp = tomoengine(8, 16, np.deg2rad(np.linspace(-60, 60, 5)), device=0, sub_slabs=2)
    with pytest.raises(NotImplementedError):
        grp.volume_rot_derivative()
    with pytest.raises(NotImplementedError):
        grp.sino_tilt_normal(B_SLOT, G_SLOT, D_SLOT)
    from tomo_tv_amd.reconstructor import TomoGPU
    rec = TomoGPU(np.linspace(-60, 60, 5), np.zeros((8, 16, 5), np.float32), gpu_id=0, sub_slabs=2)
    with pytest.raises(NotImplementedError):
        rec.refine_tilt_angles(Nouter=1)


def test_used_engine_gives_a_fresh_engines_bits(gpu):
    """Both calls after a history of other work -- reconstruction, TV, the alignment family's reductions (which share the partial-sum
    buffers), a pending asynchronous data distance -- against the same calls on a fresh engine."""
    ns, N, P = 70, 32, 9
    f = volumes(ns, N)["random"]
    X = [smooth(P, N, ns, 40 + k) for k in range(3)]

    def calls(eng):
        eng.set_volume(f, VOL_USER0)
        for slot, x in zip((B_SLOT, G_SLOT, D_SLOT), X):
            put(eng, slot, x)
        eng.volume_rot_derivative(VOL_USER0, VOL_USER0 + 1)
        return bits(eng.get_volume(VOL_USER0 + 1)), raw(eng, B_SLOT, G_SLOT, D_SLOT, 1)[1].view(np.uint64)

    fresh = calls(engine(ns, N, P))
    used = engine(ns, N, P)
    used._set_sino_local(np.abs(RA.packed(X[0])))
    used.restart_recon()
    used.SIRT(3)
    used.tv_gd(2, 0.1)
    used.sino_moments(SINO_B), used.sino_xcorr(SINO_B, SINO_B, 8), used.sino_axis_profile(SINO_B)
    used.sino_affine_normal(SINO_B, SINO_B, np.tile([1.0, 0, 0, 0, 1.0, 0], (P, 1)))
    used.copy_recon()
    used.data_distance_begin()                                                                 # left pending across the calls
    got = calls(used)
    dd = used.data_distance_end()
    assert np.array_equal(got[0], fresh[0]) and np.array_equal(got[1], fresh[1])
    assert np.isfinite(dd)
    again = calls(used)
    assert np.array_equal(again[0], fresh[0]) and np.array_equal(again[1], fresh[1])


def test_claim_is_dropped_by_a_derivative_into_the_projected_volume(gpu):
    """G = A * RECON is remembered (fp_reuse); a derivative written INTO RECON must drop that, a derivative FROM it must not."""
    ns, N, P = 6, 16, 5
    eng = engine(ns, N, P)
    f = np.abs(volumes(ns, N)["random"])
    eng.set_volume(f, VOL_ORIGINAL)
    eng.create_projections()
    eng.set_volume(f, VOL_RECON)
    d0 = eng.data_distance()                                                                   # projects RECON into G: the claim
    eng.volume_rot_derivative(VOL_RECON, VOL_TEMP)
    assert eng.data_distance() == d0
    eng.volume_rot_derivative(VOL_ORIGINAL, VOL_RECON)                                         # RECON is now D f
    ref = engine(ns, N, P)
    ref.set_volume(f, VOL_ORIGINAL)
    ref.create_projections()
    ref.set_volume(eng.get_volume(VOL_RECON), VOL_RECON)
    assert eng.data_distance() == ref.data_distance() != d0


# ---- end to end -------------------------------------------------------------------------------------------------------------------
def tilt_series(ns, N, P):
    """(nominal, true, series (Nslice, Nray, Nangles)): the blob phantom, a little different in every slice, projected by an engine at
    the TRUE angles"""
    nominal, truth = T.angle_case(P)
    vol = np.stack([(1.0 + 0.1 * s) * T.blobs(N) for s in range(ns)]).astype(np.float32)
    from tomo_tv_amd.engine import tomoengine
    src = tomoengine(ns, N, np.deg2rad(truth), device=0)
    src.set_volume(vol, VOL_ORIGINAL)
    src.create_projections()
    b = src.get_projections()
    return nominal, truth, np.ascontiguousarray(b.reshape(ns, P, N).transpose(0, 2, 1))


def test_refine_tilt_angles_end_to_end(gpu):
    """Nslice = 4, N = 32, P = 31, +-4 degrees: the rms angle error (mean removed) after pass 1 is at most half the one before, and the
    summed rr falls over the three passes; shifts, rotation and magnification keep their bits."""
    from tomo_tv_amd.reconstructor import TomoGPU
    ns, N, P = 4, 32, 31
    nominal, truth, series = tilt_series(ns, N, P)
    rec = TomoGPU(nominal, series, gpu_id=0)
    rec.set_alignment(np.zeros((P, 2)), rotation_deg=0.0, magnification=1.0)     # alignment state: ALIGN_SLOT is kept, B resampled from it
    b0, kept0 = bits(rec.tomo.get_projections()), bits(rec.tomo._sino(rec.ALIGN_SLOT))
    assert np.array_equal(b0, kept0) and b0.any()
    assert np.allclose(rec.get_tilt_angles(), nominal, rtol=0, atol=1e-12)
    state = (rec.get_alignment(), *rec.get_alignment_rotation())
    out = rec.refine_tilt_angles(Nouter=3)
    rms = [T.rms_centered(nominal, truth)] + [T.rms_centered(a, truth) for a in rec.tilt_history]
    rr = [float(np.sum(c["rr"])) for c in rec.tilt_cost]
    print("rms", np.round(rms, 4), "rr", np.round(rr, 3), "data distance", [round(c["data_distance"], 3) for c in rec.tilt_cost])
    assert len(rec.tilt_history) == 3 and np.array_equal(out, rec.tilt_history[-1])
    assert np.allclose(rec.get_tilt_angles(), out, rtol=0, atol=1e-12)
    assert rms[1] <= 0.5 * rms[0]
    assert rr[0] > rr[1] > rr[2]
    for x, y in zip(state, (rec.get_alignment(), *rec.get_alignment_rotation())):
        assert np.array_equal(np.asarray(x).view(np.uint64), np.asarray(y).view(np.uint64))
    # the sinogram slots the alignment state lives in survived the rebuilds, bit for bit
    assert np.array_equal(bits(rec.tomo.get_projections()), b0) and np.array_equal(bits(rec.tomo._sino(rec.ALIGN_SLOT)), kept0)
    # apply=False: the engine is left with the angles it had
    now = rec.get_tilt_angles()
    rec.refine_tilt_angles(Nouter=2, apply=False)
    assert np.allclose(rec.get_tilt_angles(), now, rtol=0, atol=1e-12) and len(rec.tilt_history) == 2
    assert np.array_equal(bits(rec.tomo.get_projections()), b0)


def test_refine_tilt_angles_on_the_binned_object(gpu):
    """factor = 2 at N = 64: the passes run at 32 x 32, the full-resolution engine is rebuilt once; the first condition holds, and no
    binned object with the old angles is kept."""
    from tomo_tv_amd.reconstructor import TomoGPU
    ns, N, P = 4, 64, 31
    nominal, truth, series = tilt_series(ns, N, P)
    rec = TomoGPU(nominal, series, gpu_id=0)
    b0 = bits(rec.tomo.get_projections())
    rebuilds = []
    real = rec.tomo.update_projection_angles
    rec.tomo.update_projection_angles = lambda a: (rebuilds.append(1), real(a))[1]
    out = rec.refine_tilt_angles(Nouter=3, factor=2)
    rms = [T.rms_centered(nominal, truth)] + [T.rms_centered(a, truth) for a in rec.tilt_history]
    print("factor 2: rms", np.round(rms, 4), "rr", [round(float(np.sum(c["rr"])), 3) for c in rec.tilt_cost])
    assert rms[1] <= 0.5 * rms[0]
    assert len(rebuilds) == 1
    assert np.allclose(rec.get_tilt_angles(), out, rtol=0, atol=1e-12) and rec._pyramid == {}
    assert np.array_equal(bits(rec.tomo.get_projections()), b0)
    coarse = rec.binned(2)                                                                     # a new binned object has the new angles
    assert np.allclose(coarse.get_tilt_angles(), out, rtol=0, atol=1e-12)
