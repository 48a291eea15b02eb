"""3-D affine resampling of volumes without a GPU: the binary64 statement (tests/ref64_affine3d.py) against plain loops, the binary32
replay of the kernel's arithmetic inside the bound and five deliberately wrong replays outside it, ``align.affine_matrix_3d``, the ABI,
the Python refusals, and the binary64 recovery case of the registered dual-axis loop."""
import os
import re

import numpy as np
import pytest

import ref64 as R
import ref64_affine3d as F
import ref64_dual as D
import sequences_affine3d  # noqa: F401  (registers this feature's rows of the call-sequence closure table)
from conftest import GOLDEN, ROOT
from test_bin_cpu import mixed

# the maps of the replay tests: (rotation about s, y, z in degrees, shift, magnification)
MAPS = [((7.3, -11.0, 4.0), (0.0, 0.0, 0.0), 1.0), ((0.0, 0.0, 0.0), (1.25, -2.5, 0.375), 1.0), ((30.0, 0.0, 0.0), (0.5, 0.0, 0.0), 0.8),
        ((0.0, -30.0, 12.0), (0.0, 1.0, -0.7), 1.25), ((5.0, 8.0, -30.0), (-1.5, 0.25, 2.0), 1.1)]


@pytest.mark.parametrize("N", [5, 6])
def test_statement_equals_the_loops(N):
    X = mixed((N, N, N), N).astype(np.float64)
    for rot, d, mag in MAPS:
        M = F.matrix(rot, d, mag, X.shape)
        got, mg = F.affine(X, M)
        assert np.allclose(got, F.affine_loops(X, M), rtol=1e-13, atol=1e-13) and np.all(mg >= np.abs(got) - 1e-12)
    # a non-cube pair, zero outside, identity
    Y = mixed((4, N, N), 3).astype(np.float64)
    M = F.matrix((10.0, 0.0, 0.0), (0.5, 0.0, 0.0), 1.0, Y.shape, (N, N + 1, N + 1))
    assert np.allclose(F.affine(Y, M, (N, N + 1, N + 1))[0], F.affine_loops(Y, M, (N, N + 1, N + 1)), rtol=1e-13, atol=1e-13)
    assert np.array_equal(F.affine(X, [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0])[0], X)
    assert not F.affine(X, [1, 0, 0, 3 * N, 0, 1, 0, 0, 0, 0, 1, 0])[0].any()
    assert np.array_equal(F.affine(X, [0, 0, 1, 0, 0, 1, 0, 0, 1, 0, 0, 0])[0], D.cross(X))


@pytest.mark.parametrize("k", range(len(MAPS)))
def test_replay_is_inside_the_bound_and_wrong_replays_are_outside(k):
    rot, d, mag = MAPS[k]
    N = 12
    X = mixed((N, N, N), 40 + k)
    M = F.matrix(rot, d, mag, X.shape)
    ref, _ = F.affine(X, M)
    bnd = F.bound(X, M)
    r = F.ratio(F.affine_replay_f32(X, M), ref, bnd)
    print(f"map {k}: replay worst error / bound {r:.3f}")
    assert r <= 1.0
    wrong = {"nearest-neighbour": F.affine_replay_f32(X, M, nearest=True), "fractions of y and z swapped": F.affine_replay_f32(X, M, swap_fractions=True)}
    if any(rot):
        wrong["matrix transposed"] = F.affine_replay_f32(X, F.matrix(rot, d, mag, X.shape, transpose=True))
        wrong["rotation about the corner"] = F.affine_replay_f32(X, F.matrix(rot, d, mag, X.shape, corner=True))
        wrong["angle sign flipped"] = F.affine_replay_f32(X, F.matrix(rot, d, mag, X.shape, flip_sign=True))
    for name, w in wrong.items():
        assert F.ratio(w, ref, bnd) > 1.0, name
    assert k != 0 or len(wrong) == 5


def test_replay_copies_bits_on_whole_voxel_maps():
    N = 7
    X = mixed((N, N, N), 9)
    X[2, 3, 4], X[2, 3, 5], X[0, 0, 0] = np.inf, -0.0, np.float32(2.0 ** -140)
    u = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)   # noqa: E731
    assert np.array_equal(u(F.affine_replay_f32(X, [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0])), u(X))
    assert np.array_equal(u(F.affine_replay_f32(X, [0, 0, 1, 0, 0, 1, 0, 0, 1, 0, 0, 0])), u(D.cross(X)))
    got = F.affine_replay_f32(X, [1, 0, 0, 1, 0, 1, 0, 0, 0, 0, 1, -2])                # dst[s][y][z] = src[s + 1][y][z - 2]
    ref = np.zeros_like(X)
    ref[:N - 1, :, 2:] = X[1:, :, :N - 2]
    assert np.array_equal(u(got), u(ref)) and not np.isnan(got).any()
    # a fraction along s only: the Inf's neighbours along y and z are not touched by it
    got = F.affine_replay_f32(X, [1, 0, 0, 0.5, 0, 1, 0, 0, 0, 0, 1, 0])
    assert not np.isnan(got).any() and np.isinf(got).sum() == 2


def test_affine_matrix_3d_against_its_statement():
    from tomo_tv_amd.align import affine_matrix_3d, rotation_3d
    shp, dshp = (9, 12, 12), (11, 10, 10)
    for rot, d, mag in MAPS:
        M = affine_matrix_3d(rot, d, mag, src_shape=shp, dst_shape=dshp)
        assert M.shape == (12,) and M.dtype == np.float64
        assert np.allclose(M, F.matrix(rot, d, mag, shp, dshp), rtol=1e-13, atol=1e-13)
        # the inverse-map statement: a source point, moved forward, maps back onto itself
        for p in ((0.0, 0.0, 0.0), (3.5, 2.0, 7.25), (8.0, 11.0, 0.0)):
            assert np.allclose(F.apply(M, F.forward_point(p, rot, d, mag, shp, dshp)), p, rtol=0, atol=1e-12)
        # composition with its inverse is the identity to 1e-12
        Rm = rotation_3d(rot)
        Minv = affine_matrix_3d(shift=-(Rm.T @ np.asarray(d)) / mag, magnification=1.0 / mag, src_shape=dshp, dst_shape=shp, matrix=Rm.T)
        A, B = np.vstack([M.reshape(3, 4), [0, 0, 0, 1]]), np.vstack([Minv.reshape(3, 4), [0, 0, 0, 1]])
        assert np.allclose(A @ B, np.eye(4), rtol=0, atol=1e-12) and np.allclose(B @ A, np.eye(4), rtol=0, atol=1e-12)
        assert np.allclose(affine_matrix_3d(shift=d, magnification=mag, src_shape=shp, dst_shape=dshp, matrix=Rm), M, rtol=0, atol=1e-15)
    # quarter turns between equal cubes are exact integer matrices, the identity and the translation exact
    cube = (8, 8, 8)
    for rot in ((90, 0, 0), (0, 90, 0), (0, 0, 90), (180, 0, 270), (-90, 90, 180), (360, 0, 0)):
        M = affine_matrix_3d(rot, src_shape=cube)
        assert np.array_equal(M, np.round(M)) and set(np.abs(M.reshape(3, 4)[:, :3]).ravel()) == {0.0, 1.0}, rot
        assert abs(np.linalg.det(M.reshape(3, 4)[:, :3]) - 1.0) == 0.0
    assert np.array_equal(affine_matrix_3d(src_shape=cube), [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0])
    assert np.array_equal(affine_matrix_3d(shift=(1.5, 0, -2.25), src_shape=cube), [1, 0, 0, -1.5, 0, 1, 0, 0, 0, 0, 1, 2.25])
    for bad in (dict(src_shape=None), dict(src_shape=(8, 8)), dict(src_shape=cube, shift=(0, np.nan, 0)), dict(src_shape=cube, rotation_deg=(np.inf, 0, 0)),
                dict(src_shape=cube, magnification=0.0), dict(src_shape=cube, magnification=np.nan), dict(src_shape=cube, matrix=np.eye(2)),
                dict(src_shape=cube, rotation_deg=(1, 2))):
        with pytest.raises(ValueError):
            affine_matrix_3d(**bad)


def test_the_sense_of_each_angle_by_tracking_a_point():
    """A bright voxel, resampled with the builder's matrix through the binary64 statement: where does its mass go?"""
    from tomo_tv_amd.align import affine_matrix_3d
    N, c, r = 21, 10, 8
    def centroid(point, rot):   # noqa: E306
        X = np.zeros((N, N, N))
        X[point] = 1.0
        Y = F.affine(X, affine_matrix_3d(rot, src_shape=X.shape))[0]
        g = np.meshgrid(*(np.arange(N),) * 3, indexing="ij")
        return np.array([np.sum(a * Y) for a in g]) / Y.sum() - c
    plus_y, plus_z, plus_s = (c, c + r, c), (c, c, c + r), (c + r, c, c)
    p = centroid(plus_y, (10.0, 0, 0))                                  # about s: +y moves towards +z
    assert p[2] > 1.0 and abs(p[0]) < 1e-9 and 0 < p[1] < r
    p = centroid(plus_y, (0, 10.0, 0))                                  # about y: a point on +y stays
    assert np.allclose(p, (0, r, 0), atol=1e-9)
    p = centroid(plus_z, (0, 10.0, 0))                                  # ... and +z moves towards +s
    assert p[0] > 1.0 and abs(p[1]) < 1e-9 and 0 < p[2] < r
    p = centroid(plus_y, (0, 0, 10.0))                                  # about z: +y moves towards -s
    assert p[0] < -1.0 and abs(p[2]) < 1e-9 and 0 < p[1] < r
    p = centroid(plus_s, (0, 0, 10.0))                                  # ... and +s towards +y
    assert p[1] > 1.0 and abs(p[2]) < 1e-9 and 0 < p[0] < r
    p = centroid(plus_y, (90, 0, 0))                                    # a quarter turn lands on the +z voxel exactly
    assert np.array_equal(p, (0, 0, r))
    X = np.zeros((N, N, N))
    X[3, 4, 5] = 1.0
    Y = F.affine(X, affine_matrix_3d(shift=(2, -1, 3), src_shape=X.shape))[0]     # +shift in np.roll's sense
    assert Y[5, 3, 8] == 1.0 and Y.sum() == 1.0


def test_symbols_in_header_library_and_table():
    from tomo_tv_amd import _lib
    src = open(os.path.join(ROOT, "include", "tomo_hip.h")).read()
    L = _lib.load()
    sig = {"tomo_volume_affine": [_lib._p, _lib._i, _lib._p, _lib._i, _lib._p],
           "tomo_volume_affine_axpy": [_lib._p, _lib._i, _lib._p, _lib._i, _lib._p, _lib._f, _lib._i]}
    for name, args in sig.items():
        assert re.search(r"\bint %s\s*\(" % name, src), name
        assert hasattr(L, name) and _lib.SIGNATURES[name] == args
    ident = np.eye(3, 4).ravel()
    m = ident.ctypes.data
    assert L.tomo_volume_affine(None, 0, None, 0, m) == 1 and L.tomo_last_error()               # null engines: TOMO_ERR_ARG, no crash
    assert L.tomo_volume_affine_axpy(None, 0, None, 0, m, 1.0, 0) == 1 and L.tomo_last_error()
    for phrase in ("maps a DESTINATION voxel (s, y, z) to its SOURCE position", "fma(m00, s, fma(m01, y, fma(m02, z, m03)))",
                   "gives the bits of tomo_volume_cross"):
        assert phrase in src, phrase


def test_entry_points_have_their_rows_in_the_closure_table():
    import sequences as S
    names = S.header_prototypes(open(os.path.join(ROOT, "include", "tomo_hip.h")).read())
    assert set(sequences_affine3d.ROWS) <= set(names) and S.closure_errors(names) == []


def test_python_refusals_come_before_the_library(monkeypatch):
    from tomo_tv_amd import _lib, dual_axis, engine, inprocess, reconstructor

    def boom(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "load", boom)

    class Untouchable:
        def __getattr__(self, name):
            boom()
    dual = object.__new__(dual_axis.DualAxisTomo)
    dual.N, dual.a, dual.b, dual._reg = 16, Untouchable(), Untouchable(), None
    bad = [dict(rotation_deg=(0, 0)), dict(shift=(1, 2, 3, 4)), dict(rotation_deg=(0, np.nan, 0)), dict(shift=(np.inf, 0, 0)),
           dict(matrix=np.eye(4)), dict(matrix=np.full((3, 3), np.nan)), dict(matrix=2 * np.eye(3)), dict(matrix=np.diag([1.0, 1.0, -1.0]))]
    for kw in bad:
        with pytest.raises(ValueError):
            dual.set_registration(**kw)
    assert dual._reg is None
    dual.set_registration((0, 8, 0), (1.5, 0, -2.25))
    Rm, d = dual.get_registration()
    assert np.allclose(Rm, F.rotation((0, 8, 0))) and np.array_equal(d, (1.5, 0, -2.25))
    A, B = (np.vstack([dual._reg[k].reshape(3, 4), [0, 0, 0, 1]]) for k in ("to_a", "to_b"))
    assert np.allclose(A @ B, np.eye(4), rtol=0, atol=1e-12)
    assert np.allclose(dual._reg["to_a"], F.matrix((0, 8, 0), (1.5, 0, -2.25), 1.0, (16,) * 3), rtol=0, atol=1e-13)
    dual.set_registration()                                                      # the identity switches it off
    assert dual._reg is None and np.array_equal(dual.get_registration()[0], np.eye(3))
    dual.set_registration((360, 0, 0), (0, 0, 0))
    assert dual._reg is None

    rec = object.__new__(reconstructor.TomoGPU)
    rec.Nslice, rec.Nray, rec.Nangles, rec.tomo = 8, 16, 3, Untouchable()
    for kw in (dict(rotation_deg=(0, 0)), dict(shift=(np.nan, 0, 0)), dict(rotation_deg=(np.inf, 0, 0)), dict(magnification=0.0),
               dict(magnification=np.nan), dict(shift=(1, 2))):
        with pytest.raises(ValueError):
            rec.reorient(**kw)
    # sharded and sub-slab objects refuse in Python; so do the group backend and the in-process multi-GPU class
    sharded = object.__new__(engine.tomoengine)
    sharded.comm, sharded.sub_slabs, sharded.be = object(), 1, None
    subslab = object.__new__(engine.tomoengine)
    subslab.comm, subslab.sub_slabs, subslab.be = None, 2, object.__new__(engine._GroupBackend)
    whole = object.__new__(engine.tomoengine)
    whole.comm, whole.sub_slabs, whole.be = None, 1, object.__new__(engine._SlabBackend)
    I = np.eye(3, 4).ravel()
    for eng in (sharded, subslab):
        rec.tomo = eng
        with pytest.raises(NotImplementedError):
            rec.reorient((1, 2, 3))
        with pytest.raises(NotImplementedError):
            eng.volume_affine_to(whole, I)
        with pytest.raises(NotImplementedError):
            eng.volume_affine_axpy_to(whole, I, 0.5)
        with pytest.raises(NotImplementedError):
            whole.volume_affine_to(eng, I)
    with pytest.raises(TypeError):
        whole.volume_affine_to(object(), I)
    for M in (np.eye(3), np.zeros(11), np.full(12, np.nan)):
        with pytest.raises(ValueError):
            whole.volume_affine_to(whole, M, dst=1)
    group = object.__new__(engine._GroupBackend)
    for name, args in (("volume_affine", (0, None, 0, None)), ("volume_affine_axpy", (0, None, 0, None, 1.0, 0))):
        with pytest.raises(NotImplementedError):
            group.c(name, *args)
    for name in ("volume_affine_to", "volume_affine_axpy_to"):
        with pytest.raises(NotImplementedError):
            getattr(inprocess.InProcessMultiGPU, name)(None, whole, I)
    whole.be = subslab.be = None                                                 # (nothing to destroy)
    rec.tomo = None


def test_recovery_with_the_true_registration_beats_ignoring_it():
    """tests/golden/A_N32_P9.npz, both series with the fixture's angles, t = 1 / L, K = 30 alternating iterations.  Series B is made
    from the phantom moved by an 8 degree rotation about y plus a shift of (1.5, 0, -2.25) voxels (B measures cross(move(X))), so the
    true registration -- B's content into A's frame -- is the inverse motion.  Run once with it and once with it ignored (the plain
    ``dual_axis`` loop): B's final data distance and the RMSE against the phantom must both be lower with the registration set.
    Recorded: see the figures printed below."""
    from tomo_tv_amd.align import rotation_3d
    from tomo_tv_amd.dual_axis import registration_maps
    g = np.load(os.path.join(GOLDEN, "A_N32_P9.npz"), allow_pickle=False)
    M = R.Matrix(int(g["N"]), g["angles_deg"], A=g["A"])
    N, K = M.N, 30
    X = D.phantom(N)
    Rm, dm = rotation_3d((0, 8, 0)), np.array([1.5, 0.0, -2.25])
    reg = registration_maps(N, shift=-(Rm.T @ dm), matrix=Rm.T)
    assert np.allclose(reg["to_b"], F.matrix((0, 8, 0), dm, 1.0, X.shape), rtol=0, atol=1e-12)     # T^-1 is the motion itself
    bA, bB = D.fp_a(M, X), F.moved_series_b(M, X, reg["to_b"])
    t = 1.0 / M.lipschitz()[0]
    x_reg, dd_reg = F.dual_axis_registered(M, M, bA, bB, t, t, K, reg["to_a"], reg["to_b"])
    x_ign = D.dual_axis(M, M, bA, bB, t, t, K)
    dd_ign = float(np.sqrt(np.sum((D.fp_b(M, x_ign) - bB) ** 2)))
    e_reg, e_ign = D.rmse(x_reg, X), D.rmse(x_ign, X)
    print(f"K = {K}: B's data distance {dd_reg:.4f} with the registration, {dd_ign:.4f} ignoring it; RMSE {e_reg:.4f} and {e_ign:.4f}")
    assert dd_reg < dd_ign
    assert e_reg < e_ign
