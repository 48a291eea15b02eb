"""Connected components on the GPU: labels, K and every record field exactly equal to tests/ref64_components.py; keep, repeatability,
used engines, a later SIRT run, every refusal, and ``TomoGPU.label_particles`` end to end.
Shapes (Nslice, N): no slice neighbours; a small odd one; one 64-lane chunk edge; two chunk edges (the pitch edges of the DART tests);
and N = 24, where the 64-pixel tiles of the init pass end inside image rows."""
import ctypes

import numpy as np
import pytest

import ref64_components as R
import sequences as S
import sequences_components as SC
from tomo_tv_amd._lib import VOL_RECON

pytestmark = pytest.mark.gpu

SHAPES = [(1, 16), (5, 16), (70, 16), (130, 16), (5, 24)]
IDS = ["one_slice", "small", "one_chunk_edge", "two_chunk_edges", "tile_edges_inside"]
V0 = 5                                     # TOMO_VOL_USER0
ARG, STATE = 1, 3
INF = float("inf")

# name -> (volume(shape), lo, hi)
CASES = {
    "empty": (lambda sh: np.zeros(sh, np.float32), SC.LO, SC.HI),
    "full": (lambda sh: np.ones(sh, np.float32), SC.LO, SC.HI),
    "checkerboard": (SC.checkerboard, SC.LO, SC.HI),
    "edge_touch": (lambda sh: SC.touching_blocks(sh, False), SC.LO, SC.HI),
    "corner_touch": (lambda sh: SC.touching_blocks(sh, True), SC.LO, SC.HI),
    "serpentine": (SC.serpentine, SC.LO, SC.HI),
    "serpentine_path": (SC.serpentine_path, SC.LO, SC.HI),
    "random031_a": (lambda sh: SC.random_volume(sh, 0.31, 1), SC.LO, SC.HI),
    "random031_b": (lambda sh: SC.random_volume(sh, 0.31, 2), SC.LO, SC.HI),
    "random010_a": (lambda sh: SC.random_volume(sh, 0.10, 3), SC.LO, SC.HI),
    "random010_b": (lambda sh: SC.random_volume(sh, 0.10, 4), SC.LO, SC.HI),
    "no_wrap": (SC.no_wrap, SC.LO, SC.HI),
    "bounds_nan_inf": (lambda sh: SC.special_values(sh, 6), 0.25, 0.75),
    "all_but_nan": (lambda sh: SC.special_values(sh, 6), -INF, INF),
    # background voxels (0) are the foreground: the padding slices of the volume hold 0 as well and must stay out of it
    "zero_is_foreground": (lambda sh: SC.random_volume(sh, 0.6, 8), -0.5, 0.5),
}


def engine(ns, N, P=2):
    from tomo_tv_amd.engine import tomoengine
    return tomoengine(ns, N, np.deg2rad(np.linspace(-60, 60, P)), device=0)


@pytest.fixture(scope="module", params=SHAPES, ids=IDS)
def shaped(request, gpu):
    ns, N = request.param
    return (ns, N, N), engine(ns, N)


def check(e, x, lo, hi, connectivity, want=None):
    e.set_volume(x, V0)
    lab, K, st = R.components(x, lo, hi, connectivity) if want is None else want
    got_k = e.label_components(V0, lo, hi, connectivity)
    got = e.component_labels()
    assert got_k == K, (got_k, K)
    assert got.dtype == np.int32 and np.array_equal(got, lab), np.argwhere(got != lab)[:5]
    rec = e.component_stats()
    assert rec.dtype == R.DTYPE and rec.shape == st.shape
    for f in R.DTYPE.names:
        assert np.array_equal(rec[f], st[f]), (f, np.flatnonzero(rec[f] != st[f])[:5])
    assert np.array_equal(e.get_volume(V0).view(np.uint32), x.view(np.uint32))          # labelling only reads
    return lab, K, st


@pytest.mark.parametrize("connectivity", [6, 26])
@pytest.mark.parametrize("name", list(CASES))
def test_labels_and_records_are_exact(shaped, name, connectivity):
    shape, e = shaped
    make, lo, hi = CASES[name]
    x = make(shape)
    lab, K, st = check(e, x, lo, hi, connectivity)
    n = shape[0] * shape[1] * shape[2]
    if name == "empty":
        assert K == 0
    if name == "full":
        assert K == 1 and st["voxels"][0] == n
    if name == "checkerboard":
        assert K == ((n + 1) // 2 if connectivity == 6 else 1)
    if name == "edge_touch" or (name == "corner_touch" and shape[0] > 1):
        assert K == (2 if connectivity == 6 else 1)
    if name in ("serpentine", "serpentine_path"):
        assert K == 1
    if name == "no_wrap":
        assert K == (8 if shape[0] >= 3 else 7)


@pytest.mark.parametrize("connectivity, density", [(6, 0.31), (26, 0.10)])
def test_medium_volume_against_scipy(gpu, connectivity, density):
    ndi = pytest.importorskip("scipy.ndimage")
    x = SC.random_volume((128, 128, 128), density, 9)
    lab, K = ndi.label(x > 0, structure=ndi.generate_binary_structure(3, 1 if connectivity == 6 else 3))
    lab = lab.astype(np.int32)
    check(engine(128, 128), x, SC.LO, SC.HI, connectivity, want=(lab, K, R.stats(lab)))


@pytest.mark.parametrize("connectivity", [6, 26])
def test_keep(shaped, connectivity):
    shape, e = shaped
    x = SC.random_volume(shape, 0.2 if connectivity == 6 else 0.06, 12) * np.float32(0.75) + np.float32(0.125) * SC.random_volume(shape, 0.5, 13)
    x.reshape(-1)[:2] = np.nan, -0.0                                                    # bits that only a bit-exact copy keeps
    lab, K, st = check(e, x, 0.5, 1.0, connectivity)
    assert K > 2
    table = np.concatenate([[False], st["voxels"] >= 2])                                # entry 0 is not read: the background stays
    table[K] = False
    e.keep_components(V0, table, -3.0)
    got, want = e.get_volume(V0), R.keep(x, lab, table, -3.0)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) and (got == -3.0).sum() > 0
    assert np.array_equal(e.component_labels(), lab)                                    # the label state is not changed
    check(e, got, 0.5, 1.0, connectivity)                                               # ... and a second labelling is the kept set's
    assert e.label_components(V0, 0.5, 1.0, connectivity) == int(table[1:].sum())


def test_stats_with_a_small_capacity_writes_only_that_many(shaped):
    from tomo_tv_amd import _lib
    shape, e = shaped
    x = SC.random_volume(shape, 0.2, 21)
    lab, K, st = check(e, x, SC.LO, SC.HI, 6)
    assert K > 4
    buf = np.full(K * 72, 0xAB, np.uint8)
    _lib.check(_lib.load().tomo_components_stats(e.be.h, K - 3, buf.ctypes.data))
    assert np.array_equal(buf[:(K - 3) * 72].view(R.DTYPE), st[:K - 3]) and np.all(buf[(K - 3) * 72:] == 0xAB)
    _lib.check(_lib.load().tomo_components_stats(e.be.h, 0, None))


def _with_series(ns=6, N=32):
    e = engine(ns, N, 9)
    e.set_volume(S.phantom(ns, N), 2)
    e.create_projections()
    return e


def test_used_engine_gives_a_fresh_engines_labels(gpu):
    x = SC.random_volume((6, 32, 32), 0.25, 31)
    want = SC.component_calls(_with_series(), x, V0)
    e = _with_series()
    e.restart_recon()
    e.SIRT(2)
    S.d_dart(e, "A", None)
    e.tv_fgp(3, 0.02)
    got = SC.component_calls(e, x, V0)
    again = SC.component_calls(e, x, V0)                                                # the same call twice: the same bits
    assert got.keys() == want.keys()
    for k in want:
        assert np.array_equal(got[k], want[k]) and np.array_equal(again[k], want[k]), k
    for c in (6, 26):                                                                   # ... and the right answer, not only a repeatable one
        lab, K, st = R.components(x, SC.LO, SC.HI, c)
        assert want[f"K{c}"][0] == K and np.array_equal(want[f"labels{c}"], lab) and np.array_equal(want[f"stats{c}"].view(R.DTYPE), st)


def test_the_new_calls_leave_a_later_sirt_run_alone(gpu):
    """After a cost evaluation G is the projection of RECON and the next SIRT step starts from it.  Labelling and the queries only read
    RECON and keep that; tomo_components_keep writes RECON and must drop it, or the step would start from the projection of the
    volume of before: the unused engine is given the same volume by tomo_set_volume."""
    out = []
    for used in (True, False):
        e = _with_series()
        e.restart_recon()
        e.SIRT(2)
        e.data_distance()
        if used:
            assert e.label_components(VOL_RECON, 0.4, INF, 26) > 0
            e.component_labels(), e.component_stats()
        mid = e.get_volume()
        e.SIRT(1)
        first = e.get_volume().astype(np.float32)
        e.data_distance()
        lab, K, _ = R.components(first, 0.4, INF, 6)
        table = np.ones(K + 1, bool)
        table[1] = False
        assert K >= 1
        if used:
            assert e.label_components(VOL_RECON, 0.4, INF, 6) == K
            e.keep_components(VOL_RECON, table, 0.0)
        else:
            e.set_volume(R.keep(first, lab, table, 0.0))
        kept = e.get_volume()
        e.SIRT(1)
        out.append((mid, first, kept, e.get_volume(), e.data_distance()))
    for a, b in zip(out[0][:4], out[1][:4]):
        assert np.array_equal(a, b)
    assert out[0][4] == out[1][4] and not np.array_equal(out[0][1], out[0][2])


def test_refusals(gpu):
    from tomo_tv_amd import _lib
    from tomo_tv_amd.engine import tomoengine
    L = _lib.load()
    e = engine(5, 12, 3)
    h = e.be.h
    x = SC.random_volume((5, 12, 12), 0.3, 2)
    e.set_volume(x, V0)
    k = ctypes.c_int64(-7)
    lab = np.full(x.shape, -7, np.int32)
    rec = np.zeros(64, R.DTYPE)
    tab = np.ones(64, np.uint8)
    nan = float("nan")

    def queries(n):
        return [L.tomo_components_get_labels(h, lab.ctypes.data), L.tomo_components_stats(h, 4, rec.ctypes.data),
                L.tomo_components_keep(h, V0, tab.ctypes.data, n, 0.0)]
    assert queries(1) == [STATE] * 3 and b"labelling" in L.tomo_last_error()           # before any labelling
    bad = [(V0, 0.5, 1.5, 18), (V0, 0.5, 1.5, 0), (-1, 0.5, 1.5, 26), (45, 0.5, 1.5, 26), (V0, nan, 1.5, 26), (V0, 0.5, nan, 26), (V0, 1.5, 0.5, 26)]
    for vol, lo, hi, c in bad:
        assert L.tomo_components_label(h, vol, lo, hi, c, ctypes.byref(k)) == ARG, (vol, lo, hi, c)
    assert L.tomo_components_label(h, V0, 0.5, 1.5, 26, None) == ARG
    assert queries(1) == [STATE] * 3 and k.value == -7                                  # the refused calls made no labelling
    assert L.tomo_components_label(h, V0, 0.5, 0.5, 26, ctypes.byref(k)) == 0 and k.value == 0          # lo == hi is a valid band
    want, K, st = R.components(x, 0.5, 1.5, 6)
    assert e.label_components(V0, 0.5, 1.5, 6) == K and 2 < K < 63                      # (the Python object remembers K for component_stats)
    for n in (K, K + 2, 0, -1):
        assert L.tomo_components_keep(h, V0, tab.ctypes.data, n, 0.0) == ARG, n
    assert L.tomo_components_keep(h, V0, None, K + 1, 0.0) == ARG and L.tomo_components_keep(h, 99, tab.ctypes.data, K + 1, 0.0) == ARG
    assert L.tomo_components_get_labels(h, None) == ARG and L.tomo_components_stats(h, 4, None) == ARG
    assert L.tomo_components_stats(h, -1, rec.ctypes.data) == ARG
    # after all of that the engine still holds the right labelling and an untouched volume
    assert np.array_equal(e.component_labels(), want) and np.array_equal(e.component_stats(), st)
    assert np.array_equal(e.get_volume(V0).view(np.uint32), x.view(np.uint32))
    with pytest.raises(NotImplementedError):                                            # sharded engines refuse in Python already
        tomoengine(8, 12, np.deg2rad([0.0, 30.0]), device=0, sub_slabs=2).label_components(V0, 0.5, 1.5)
    # release: the state is gone, a second release is a no-op, and labelling builds it again
    e.release_components()
    e.release_components()
    assert queries(K + 1) == [STATE] * 3
    assert e.label_components(V0, 0.5, 1.5, 6) == K and np.array_equal(e.component_labels(), want)
    # an engine whose geometry was released: TOMO_ERR_STATE, also with a labelling in hand
    assert L.tomo_release_geometry(h) == 0
    assert L.tomo_components_label(h, V0, 0.5, 1.5, 6, ctypes.byref(k)) == STATE and queries(K + 1) == [STATE] * 3
    assert b"released" in L.tomo_last_error()
    assert L.tomo_components_release(h) == 0


def test_refuses_two_to_the_31_voxels(gpu):
    """Nslice * N * N = 8192 * 512 * 512 = 2^31: label + 1 no longer fits int32, every call is TOMO_ERR_ARG.  The engine costs what
    tomo_create allocates for any engine (the reconstruction, 8 GiB, cleared once, and a sinogram of two angles); the refused calls
    must come back before they allocate a volume or the label state (8 GiB), so none of them may take longer than a host call."""
    import time
    from tomo_tv_amd import _lib
    from tomo_tv_amd.engine import tomoengine
    L = _lib.load()
    big = tomoengine(8192, 512, np.deg2rad([0.0, 30.0]), device=0)
    try:
        k, buf = ctypes.c_int64(0), (ctypes.c_uint8 * 144)()
        big.synchronize()
        t0 = time.perf_counter()
        for rc in (L.tomo_components_label(big.be.h, V0, 0.5, 1.5, 26, ctypes.byref(k)), L.tomo_components_get_labels(big.be.h, buf),
                   L.tomo_components_stats(big.be.h, 2, buf), L.tomo_components_keep(big.be.h, V0, buf, 1, 0.0)):
            assert rc == ARG and b"2^31" in L.tomo_last_error()
        assert time.perf_counter() - t0 < 0.5
        opt = ctypes.c_int(-1)
        assert L.tomo_get_option(big.be.h, b"form_sart", ctypes.byref(opt)) == 0          # the engine is still usable
    finally:
        big.be.close()


def test_refuses_an_engine_with_a_communicator(gpu):
    """A one-rank RCCL communicator bound through the C ABI, in a fresh child process like the other one-rank tests."""
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    p = subprocess.run([sys.executable, os.path.join(here, "components_comm_script.py")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "COMPONENTS_COMM_REFUSED_OK" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]


def test_label_particles_end_to_end(gpu):
    """Four separated spheres of radius 4 and grey level 1 at N = Nslice = 32, projected over 31 angles in [-75, 75], reconstructed by
    SIRT + DART: as many particles as spheres, every centroid within one voxel of its sphere's centre."""
    from tomo_tv_amd.reconstructor import TomoGPU
    N, ang = 32, np.linspace(-75, 75, 31)
    centres = np.array([[8.0, 9.0, 10.0], [9.0, 22.0, 21.0], [22.0, 10.0, 22.0], [23.0, 21.0, 9.0]])
    g = np.indices((N, N, N)).transpose(1, 2, 3, 0)
    ph = np.zeros((N, N, N), np.float32)
    for c in centres:
        ph[((g - c) ** 2).sum(-1) <= 16.0] = 1.0
    from tomo_tv_amd.engine import tomoengine
    eng = tomoengine(N, N, np.deg2rad(ang), device=0)
    eng.set_volume(ph, 2)
    eng.create_projections()
    b = eng.get_projections().reshape(N, ang.size, N).transpose(0, 2, 1).copy()
    rec = TomoGPU(ang, b, gpu_id=0)
    rec.tomo.restart_recon()
    rec.dart([0.0, 1.0], Niter=10, arm_iters=5, init_iters=30)
    out = rec.label_particles()
    print("particles:", out["count"], "voxels", out["voxels"], "centroids", out["centroid"])
    assert out["count"] == len(centres)
    for c in centres:
        d = np.sqrt(((out["centroid"] - c) ** 2).sum(1))
        print("sphere", c, "nearest centroid at", d.min())
        assert d.min() <= 1.0
    lab = rec.get_particle_labels()
    assert lab.shape == ph.shape and lab.max() == out["count"] and np.array_equal(np.bincount(lab.ravel())[1:], out["voxels"])
