"""DART on the GPU: the state bytes and counts against tests/ref64_dart.py exactly, no periodic neighbours, restore / arm / smooth /
class statistics with their bit identities and bounds, every refusal, and the driver ``TomoGPU.dart`` on the phantom of the CPU replay.
Shapes (Nslice, N, P): no slice neighbours; a small odd one; one 64-lane chunk edge; two chunk edges."""
import ctypes

import numpy as np
import pytest

import ref64_dart as R

pytestmark = pytest.mark.gpu

SHAPES = [(1, 8, 3), (5, 12, 3), (70, 8, 3), (130, 16, 2)]
IDS = ["one_slice", "small", "one_chunk_edge", "two_chunk_edges"]
V0, V1 = 5, 6                              # TOMO_VOL_USER0 ..
THR = {0: [], 1: [0.5], 3: [0.2, 0.5, 0.8], 15: list(np.linspace(-0.2, 1.2, 15))}


def engine(ns, N, P):
    from tomo_tv_amd.engine import tomoengine
    return tomoengine(ns, N, np.deg2rad(np.linspace(-60, 60, P)), device=0)


def volume(shape, seed, thr):
    """smooth blobs in [-0.3, 1.3] plus a little noise, with a NaN, a +Inf and values exactly equal to thresholds"""
    rng = np.random.default_rng(seed)
    s, y, z = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")
    v = 0.5 + 0.8 * np.sin(0.9 * y + 0.2 * s) * np.cos(0.7 * z - 0.13 * s) + rng.uniform(-0.03, 0.03, shape)
    v = v.astype(np.float32)
    flat = v.reshape(-1)
    pick = rng.choice(flat.size, size=min(flat.size, 6 + len(thr)), replace=False)
    flat[pick[0]], flat[pick[1]] = np.nan, np.inf
    for i, t in enumerate(thr):
        flat[pick[2 + i]] = np.float32(t)
    return v


class Case:
    def __init__(self, ns, N, P):
        self.shape, self.P = (ns, N, N), P
        self.eng = engine(ns, N, P)
        self.x = volume(self.shape, 11 * N + ns, THR[3])


@pytest.fixture(scope="module", params=SHAPES, ids=IDS)
def case(request, gpu):
    return Case(*request.param)


@pytest.fixture(scope="module")
def small(gpu):
    return Case(5, 12, 3)


@pytest.mark.parametrize("nthr", [0, 1, 3, 15])
@pytest.mark.parametrize("connectivity", [6, 26])
def test_state_is_exact(case, connectivity, nthr):
    e = case.eng
    thr = np.asarray(THR[nthr], np.float32)
    x = volume(case.shape, 5 + nthr, thr)
    e.set_volume(x, V0)
    for frac in (0.0, 0.15, 1.0):
        for seed in (0, 0xC0FFEE11):
            nf, nb = e.dart_classify(thr, V0, connectivity, seed, frac)
            want = R.state(x, thr, connectivity, seed, R.free_threshold(frac))
            got = e.dart_state()
            assert np.array_equal(got, want), (frac, seed, np.argwhere(got != want)[:5])
            assert nf == int(((want & R.FREE) != 0).sum()) and nb == int(((want & R.BOUNDARY) != 0).sum())
    assert np.array_equal(e.get_volume(V0).view(np.uint32), x.view(np.uint32))          # classify only reads


@pytest.mark.parametrize("connectivity", [6, 26])
def test_no_wrap(case, connectivity):
    """An object that fills the planes s = 0, y = 0 and z = N - 1, background on the opposite faces: with periodic neighbours (the TV
    kernels') every voxel of those six faces would be a boundary voxel; without them only the object's own surface is."""
    e = case.eng
    ns, N, _ = case.shape
    x = np.zeros(case.shape, np.float32)
    x[: max(1, ns // 2), : N // 2, N // 2:] = 1.0
    e.set_volume(x, V0)
    nf, nb = e.dart_classify([0.5], V0, connectivity, 0, 0.0)
    got, want = e.dart_state(), R.state(x, [0.5], connectivity, 0, 0)
    assert np.array_equal(got, want)
    bnd = (got & R.BOUNDARY) != 0
    assert not bnd[0, 0, N - 1] and not bnd[ns - 1, N - 1, 0]                          # the corners that face each other through a wrap
    assert not bnd[:, N - 1, :].any() and not bnd[:, :, 0].any() and (ns < 3 or not bnd[ns - 1].any())
    assert nf == nb == int(bnd.sum())


def test_restore_and_arm(case):
    e = case.eng
    thr, grey = np.asarray(THR[3], np.float32), np.array([0.0, 0.3, 0.6, 1.0], np.float32)
    rng = np.random.default_rng(3)
    x = np.full(case.shape, 0.1, np.float32)                                            # two regions with interiors, also at 1 x 8 x 8
    x[:, : case.shape[1] // 2, :] = 0.9
    x += rng.uniform(-0.05, 0.05, case.shape).astype(np.float32)
    b = rng.uniform(0.5, 2.0, (case.shape[0], case.P * case.shape[1])).astype(np.float32)
    e.set_tilt_series(b)
    e.set_volume(x, V0)
    e.dart_classify(thr, V0, 26, 4, 0.3)
    st = e.dart_state()
    fixed = (st & R.FREE) == 0
    assert fixed.any() and (~fixed).any()
    e.dart_restore(grey, V0)
    r = e.get_volume(V0)
    assert np.array_equal(r.view(np.uint32), R.restore(x, st, grey).view(np.uint32))
    # padding stays zero: restoring the restored volume gives the same bits, and so does its projection
    e.be.c("forward_projection", V0, 3)
    p0 = e._sino(3).copy()
    e.dart_restore(grey, V0)
    e.be.c("forward_projection", V0, 3)
    assert np.array_equal(e.get_volume(V0).view(np.uint32), r.view(np.uint32))
    assert np.array_equal(e._sino(3).view(np.uint32), p0.view(np.uint32))
    # three masked SIRT iterations: the fixed voxels still hold their grey value, the free ones moved
    e.dart_arm(3, grey, V0)
    a = e.get_volume(V0)
    assert np.array_equal(a[fixed].view(np.uint32), grey[st & R.LABEL_MASK][fixed].view(np.uint32))
    assert not np.array_equal(a[~fixed], r[~fixed])
    # every voxel free: the bits of tomo_sirt_data
    n = x.size
    nf, _ = e.dart_classify(thr, V0, 26, 4, 1.0)
    assert nf == n
    e.set_volume(x, V0)
    e.set_volume(x, V1)
    e.dart_arm(3, grey, V0)
    e.be.c("sirt_data", V1, 0, 3)
    assert np.array_equal(e.get_volume(V0).view(np.uint32), e.get_volume(V1).view(np.uint32))
    # no voxel free (one class: no boundary): the restored volume stays as it is
    nf, nb = e.dart_classify([], V0, 26, 4, 0.0)
    assert nf == 0 and nb == 0
    e.dart_restore([0.25], V0)
    e.dart_arm(2, [0.25], V0)
    assert np.array_equal(e.get_volume(V0), np.full(case.shape, 0.25, np.float32))
    # the final segmentation sets every voxel
    e.set_volume(x, V0)
    e.dart_classify(thr, V0, 6, 0, 0.0)
    st = e.dart_state()
    e.dart_restore(grey, V0, everywhere=True)
    assert np.array_equal(e.get_volume(V0), grey[st & R.LABEL_MASK])


def test_smooth(case):
    e = case.eng
    x = case.x.copy()
    x[~np.isfinite(x)] = 0.4
    e.set_volume(x, V0)
    e.dart_classify([0.5], V0, 26, 9, 0.3)
    st = e.dart_state()
    for beta in (0.1, 1.0):
        e.set_volume(np.full(case.shape, 7.0, np.float32), V1)                           # dst is overwritten, not blended
        e.dart_smooth(V0, V1, beta)
        got = e.get_volume(V1)
        want, bound, fr = R.smooth(x, st, beta)
        err = np.abs(got.astype(np.float64) - want)
        print(f"smooth beta={beta}: max err / bound {np.max(err[fr] / bound[fr]) if fr.any() else 0:.3f}")
        assert np.all(err <= bound), np.argwhere(err > bound)[:5]
        assert np.array_equal(got[~fr].view(np.uint32), x[~fr].view(np.uint32))
    e.dart_smooth(V0, V1, 0.0)
    assert np.array_equal(e.get_volume(V1).view(np.uint32), x.view(np.uint32))
    # a constant stays constant, bit for bit (c = 0.75, beta = 0.25: tests/test_dart_cpu.py says why), every voxel free
    c = np.full(case.shape, 0.75, np.float32)
    e.set_volume(c, V0)
    nf, _ = e.dart_classify([0.5], V0, 26, 1, 1.0)
    assert nf == c.size
    e.dart_smooth(V0, V1, 0.25)
    assert np.array_equal(e.get_volume(V1).view(np.uint32), c.view(np.uint32))
    # an Inf beside a fixed voxel does not make it NaN
    y = np.zeros(case.shape, np.float32)
    y[0, 3, 3] = np.inf
    e.set_volume(y, V0)
    e.dart_classify([], V0, 26, 0, 0.0)                                                  # one class: every voxel fixed
    e.dart_smooth(V0, V1, 0.5)
    assert np.array_equal(e.get_volume(V1).view(np.uint32), y.view(np.uint32))


def check_class_stats(e, shape, nthr):
    thr = np.asarray(THR[nthr], np.float32)
    x = volume(shape, 17 + nthr, thr)
    e.set_volume(x, V0)
    got, again, want = e.dart_class_stats(thr, V0), e.dart_class_stats(thr, V0), R.class_stats(x, thr)
    assert np.array_equal(got[:, 1], want[:, 1])
    fin = np.isfinite(x)
    lab = R.labels(x, thr)
    for c in range(nthr + 1):
        tol = want[c, 1] * 2.0 ** -53 * np.abs(x[fin & (lab == c)].astype(np.float64)).sum()
        assert abs(got[c, 0] - want[c, 0]) <= tol, (c, got[c, 0], want[c, 0], tol)
    assert np.array_equal(got.view(np.uint64), again.view(np.uint64))


@pytest.mark.parametrize("nthr", [0, 1, 3, 15])
def test_class_stats(case, nthr):
    check_class_stats(case.eng, case.shape, nthr)


@pytest.mark.parametrize("nthr", [1, 15])
def test_class_stats_with_more_than_256_workgroups(gpu, nthr):
    """One slice of 65 x 65 is 4225 rows of pitch 64, 265 workgroups of 1024 floats: the smallest volume at which a thread of the
    second stage (256 threads per output) adds more than one of the workgroups' rows.  The statement and the bound of test_class_stats."""
    check_class_stats(engine(1, 65, 2), (1, 65, 65), nthr)


def test_refusals(small):
    from tomo_tv_amd import _lib
    from tomo_tv_amd.engine import tomoengine
    L = _lib.load()
    fresh = engine(5, 12, 3)
    h = fresh.be.h
    thr = (ctypes.c_float * 3)(0.2, 0.5, 0.8)
    grey = (ctypes.c_float * 4)(0.0, 0.3, 0.6, 1.0)
    st = (ctypes.c_uint8 * (5 * 12 * 12))()
    out = (ctypes.c_double * 32)()
    ARG, STATE = 1, 3
    # before any classify
    assert L.tomo_dart_restore(h, V0, grey, 4) == STATE and L.tomo_dart_segment(h, V0, grey, 4) == STATE
    assert L.tomo_dart_arm(h, V0, 0, 1, grey, 4) == STATE and L.tomo_dart_smooth(h, V0, V1, 0.1) == STATE
    assert L.tomo_dart_get_state(h, st) == STATE and L.tomo_last_error()
    x = small.x
    fresh.set_volume(x, V0)
    bad_thr = [((ctypes.c_float * 2)(0.5, 0.5), 2), ((ctypes.c_float * 2)(0.6, 0.5), 2), ((ctypes.c_float * 2)(0.5, float("inf")), 2),
               ((ctypes.c_float * 1)(float("nan")), 1), (thr, -1), (thr, 16), (None, 2)]
    for t, n in bad_thr:
        assert L.tomo_dart_classify(h, V0, t, n, 26, 0, 0) == ARG, n
        assert L.tomo_dart_class_stats(h, V0, t, n, out) == ARG, n
    assert L.tomo_dart_classify(h, V0, thr, 3, 18, 0, 0) == ARG and L.tomo_dart_classify(h, -1, thr, 3, 26, 0, 0) == ARG
    assert L.tomo_dart_classify(h, 45, thr, 3, 26, 0, 0) == ARG and L.tomo_dart_class_stats(h, V0, thr, 3, None) == ARG
    assert L.tomo_dart_get_state(h, st) == STATE                                        # the refused calls made no state
    assert L.tomo_dart_classify(h, V0, thr, 3, 26, 0, 0) == 0
    assert L.tomo_dart_restore(h, V0, grey, 3) == ARG and L.tomo_dart_restore(h, V0, None, 4) == ARG and L.tomo_dart_restore(h, 99, grey, 4) == ARG
    assert L.tomo_dart_segment(h, V0, grey, 5) == ARG
    assert L.tomo_dart_arm(h, V0, 0, 1, grey, 2) == ARG and L.tomo_dart_arm(h, V0, 99, 1, grey, 4) == ARG and L.tomo_dart_arm(h, V0, 0, -1, grey, 4) == ARG
    assert L.tomo_dart_arm(h, V0, 0, 1, None, 4) == ARG
    assert L.tomo_dart_smooth(h, V0, V0, 0.1) == ARG and L.tomo_dart_smooth(h, V0, 99, 0.1) == ARG
    for beta in (-0.1, 1.5, float("nan"), float("inf")):
        assert L.tomo_dart_smooth(h, V0, V1, beta) == ARG, beta
    assert L.tomo_dart_get_state(h, None) == ARG
    # after all of that the engine still computes the right state
    assert np.array_equal(fresh.dart_state(), R.state(x, np.array(thr[:], np.float32), 26, 0, 0))
    with pytest.raises(NotImplementedError):                                            # sharded engines refuse in Python already
        tomoengine(8, 12, np.deg2rad([0.0, 30.0]), device=0, sub_slabs=2).dart_classify([0.5])
    # an engine whose geometry was released: every call is TOMO_ERR_STATE, also with a state in hand
    assert L.tomo_release_geometry(h) == 0
    for rc in _every_call(L, h, thr, grey, out, st):
        assert rc == STATE
    assert b"released" in L.tomo_last_error()


def _every_call(L, h, thr, grey, out, st):
    """the seven tomo_dart_* calls with arguments that are valid for a 3-threshold state"""
    yield L.tomo_dart_classify(h, V0, thr, 3, 26, 0, 0)
    yield L.tomo_dart_restore(h, V0, grey, 4)
    yield L.tomo_dart_segment(h, V0, grey, 4)
    yield L.tomo_dart_arm(h, V0, 0, 1, grey, 4)
    yield L.tomo_dart_smooth(h, V0, V1, 0.1)
    yield L.tomo_dart_class_stats(h, V0, thr, 3, out)
    yield L.tomo_dart_get_state(h, st)


def test_refuses_two_to_the_32_voxels(gpu):
    """Nslice * N * N = 16384 * 512 * 512 = 2^32: the voxel index of the free draw no longer fits 32 bits, every call is TOMO_ERR_ARG.
    The engine itself costs what tomo_create allocates for any engine, here the reconstruction (16 GiB, cleared once) and the measured
    sinogram of two angles (64 MiB); the refused calls must come back before they allocate a volume, a state buffer (4 GiB) or a
    staging buffer, so none of them may take longer than a host call."""
    import time
    from tomo_tv_amd import _lib
    from tomo_tv_amd.engine import tomoengine
    L = _lib.load()
    big = tomoengine(16384, 512, np.deg2rad([0.0, 30.0]), device=0)
    try:
        thr = (ctypes.c_float * 3)(0.2, 0.5, 0.8)
        grey = (ctypes.c_float * 4)(0.0, 0.3, 0.6, 1.0)
        out, st = (ctypes.c_double * 32)(), (ctypes.c_uint8 * 16)()
        big.synchronize()
        t0 = time.perf_counter()
        for rc in _every_call(L, big.be.h, thr, grey, out, st):
            assert rc == 1 and b"2^32" in L.tomo_last_error()
        assert time.perf_counter() - t0 < 0.5
        opt = ctypes.c_int(-1)
        assert L.tomo_get_option(big.be.h, b"form_sart", ctypes.byref(opt)) == 0          # the engine is still usable
    finally:
        big.be.close()


def test_refuses_an_engine_with_a_communicator(gpu):
    """A one-rank RCCL communicator bound through the C ABI, in a fresh child process like the other one-rank tests: every
    tomo_dart_* call is TOMO_ERR_STATE."""
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    p = subprocess.run([sys.executable, os.path.join(here, "dart_comm_script.py")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "DART_COMM_REFUSED_OK" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]


@pytest.fixture(scope="module")
def driver(gpu):
    from tomo_tv_amd.reconstructor import TomoGPU
    D = R.DRIVER
    ph = R.driver_phantom(D["Nslice"], D["N"])
    ang = np.linspace(-70, 70, 9)                                                       # the angles of tests/golden/A_N32_P9.npz
    eng = engine_deg(D["Nslice"], D["N"], ang)
    eng.set_volume(ph, 2)
    eng.create_projections()
    b = eng.get_projections().reshape(D["Nslice"], 9, D["N"]).transpose(0, 2, 1).copy()
    kw = {k: D[k] for k in ("Niter", "arm_iters", "init_iters", "fix_probability", "smoothing", "connectivity", "seed")}

    def run(**over):
        rec = TomoGPU(ang, b, gpu_id=0)
        rec.tomo.restart_recon()
        out = rec.dart(D["grey"], **{**kw, **over})
        return rec, out
    return dict(ph=ph, ang=ang, b=b, run=run, first=run())


def engine_deg(ns, N, ang):
    from tomo_tv_amd.engine import tomoengine
    return tomoengine(ns, N, np.deg2rad(ang), device=0)


def test_driver(driver):
    from tomo_tv_amd.reconstructor import TomoGPU
    D, ph = R.DRIVER, driver["ph"]
    rec, out = driver["first"]
    vol = rec.get_recon()
    assert set(np.unique(vol)) <= {float(np.float32(g)) for g in D["grey"]}
    assert np.all(out["n_free"] < ph.size) and np.all(out["n_boundary"] > 0) and np.all(out["n_free"] >= out["n_boundary"])
    truth = (ph > 0.5).astype(np.uint8)
    lab = rec.get_dart_labels()
    assert np.array_equal(np.asarray(D["grey"], np.float64)[lab], vol)
    sirt = TomoGPU(driver["ang"], driver["b"], gpu_id=0)
    sirt.sirt(D["init_iters"] + D["Niter"] * D["arm_iters"], show_convergence=False)
    mis_dart, mis_sirt = int((lab != truth).sum()), int((R.labels(sirt.get_recon().astype(np.float32), [0.5]) != truth).sum())
    print("misclassified: DART", mis_dart, "thresholded SIRT", mis_sirt, "data distance", out["data_distance"])
    assert mis_dart < mis_sirt
    # the grey levels estimated from a long SIRT run: within 5 % of the contrast of the phantom's two values (0 and 1)
    sirt.tomo.SIRT(R.LLOYD_SIRT_ITERS - D["init_iters"] - D["Niter"] * D["arm_iters"])
    lev = sirt.estimate_grey_levels(2)
    print("estimated grey levels", lev)
    assert np.all(np.abs(lev - np.array([0.0, 1.0])) <= 0.05)


def test_driver_run_to_run(driver):
    rec, out = driver["first"]
    rec2, out2 = driver["run"]()
    assert np.array_equal(rec.get_recon(), rec2.get_recon())
    assert np.array_equal(out["n_free"], out2["n_free"]) and np.array_equal(out["data_distance"], out2["data_distance"])
    # another seed: another free set (already in the first iteration, where the volumes are still the same)
    rec3, out3 = driver["run"](seed=R.DRIVER["seed"] + 1, Niter=1, segment=False)
    rec4, out4 = driver["run"](Niter=1, segment=False)
    f3, f4 = rec3.tomo.dart_state() & R.FREE, rec4.tomo.dart_state() & R.FREE
    assert out4["n_free"][0] == out["n_free"][0] and not np.array_equal(f3, f4)
