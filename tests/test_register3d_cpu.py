"""The 3-D registration of two volumes without a GPU: the binary64 statement of the 32 sums (tests/ref64_register3d.py) against plain
loops, the binary32 replay of the kernel's arithmetic inside the bound and four deliberately wrong replays outside it, the host
helpers of ``align``, the ABI, the Python refusals, and the Gauss-Newton loop on the exact and on the realistic case."""
import functools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import ref64 as R
import ref64_affine3d as F
import ref64_dual as D
import ref64_register3d as G3
import sequences_affine3d  # noqa: F401  (the rows of the resampling calls: the closure check below needs the whole table)
import sequences_register3d  # noqa: F401  (registers this feature's row of the call-sequence closure table)
from conftest import GOLDEN, ROOT
from test_bin_cpu import mixed

# the maps of the replay tests: (rotation about s, y, z in degrees, shift): rotations up to 30 degrees, with shifts
MAPS = [((0.0, 8.0, 0.0), (1.5, 0.0, -2.25)), ((7.3, -11.0, 4.0), (0.3, -0.6, 0.9)), ((30.0, 0.0, 0.0), (0.5, 0.0, 0.0)),
        ((0.0, -30.0, 12.0), (0.0, 1.0, -0.7)), ((5.0, 8.0, -30.0), (-1.5, 0.25, 2.0))]
POSE, POSE2 = ((0.0, 8.0, 0.0), np.array([1.5, 0.0, -2.25])), ((3.0, -5.0, 4.0), np.array([-2.0, 1.25, 0.75]))


def smooth(shape, seed):
    """a few Gaussian blobs on a slope: every gradient component and the residual are non-trivial"""
    rng = np.random.default_rng(seed)
    g = np.meshgrid(*(np.arange(n, dtype=np.float64) for n in shape), indexing="ij")
    X = 0.02 * g[0] - 0.01 * g[1] + 0.015 * g[2]
    for _ in range(4):
        c, w = [rng.uniform(0.25 * n, 0.75 * n) for n in shape], rng.uniform(0.15, 0.3) * min(shape)
        X += rng.uniform(0.5, 1.5) * np.exp(-sum((a - b) ** 2 for a, b in zip(g, c)) / (2 * w * w))
    return X.astype(np.float32)


@pytest.mark.parametrize("N", [5, 6])
def test_statement_equals_the_loops(N):
    Fv, Gv = mixed((N, N, N), N).astype(np.float64), mixed((N, N + 1, N + 1), N + 1).astype(np.float64)
    for margin in (0, 1):
        for rot, d in MAPS[:3] + [((0.0, 0.0, 0.0), (0.0, 0.0, 0.0)), ((0.0, 0.0, 0.0), (1.0, 0.0, -1.0))]:
            M = F.matrix(rot, d, 1.0, Gv.shape, Fv.shape)
            a, b = G3.normal(Fv, Gv, M, margin), G3.normal_loops(Fv, Gv, M, margin)
            assert np.allclose(a, b, rtol=1e-12, atol=1e-12) and a[28] == b[28], (rot, d, margin)
    ident = G3.normal(Fv, Fv, np.eye(3, 4).ravel(), 0)
    assert ident[28] == (N - 1) ** 3 and ident[27] == 0.0 and not ident[21:27].any()     # the last plane of G never counts
    assert G3.normal(Fv, Gv, F.matrix((0, 0, 0), (3.0 * N, 0, 0), 1.0, Gv.shape, Fv.shape), 0)[28] == 0


@pytest.mark.parametrize("k", range(len(MAPS)))
def test_replay_is_inside_the_bound_and_wrong_replays_are_outside(k):
    rot, d = MAPS[k]
    N = 14
    Fv, Gv = smooth((N, N, N), 70 + k), smooth((N, N, N), 80 + k)
    M = F.matrix(rot, d, 1.0, Gv.shape)
    ref = G3.normal(Fv, Gv, M, 1)
    bnd, _ = G3.bound(Fv, Gv, M, 1)
    r = G3.ratios(G3.normal_replay_f32(Fv, Gv, M, 1), ref, bnd)
    print(f"map {k}: replay worst error / bound {r.max():.3f} (sum {int(r.argmax())}), {int(ref[28])} voxels count")
    assert r.max() <= 1.0 and ref[28] > N ** 3 // 8
    for wrong in ("nearest_gradient", "corner", "cross_sign", "zero_padded"):
        rw = G3.ratios(G3.normal_replay_f32(Fv, Gv, M, 1, **{wrong: True}), ref, bnd)
        assert rw.max() > 1.0, wrong


def test_replay_copies_samples_on_whole_voxel_maps():
    """identity and a whole-voxel shift: w is a copy, so the count and the three correlation sums carry the summation term alone"""
    N = 9
    Fv, Gv = smooth((N, N, N), 3), smooth((N, N, N), 4)
    for M in (np.eye(3, 4).ravel(), np.array([1, 0, 0, 1, 0, 1, 0, -2, 0, 0, 1, 0], np.float64)):
        ref, got = G3.normal(Fv, Gv, M, 0), G3.normal_replay_f32(Fv, Gv, M, 0)
        _, summ = G3.bound(Fv, Gv, M, 0)
        assert got[28] == ref[28] and np.all(np.abs(got[29:] - ref[29:]) <= summ[29:])


def test_host_helpers():
    from tomo_tv_amd.align import affine_matrix_3d, compose_rigid_increment, decode_rigid, rigid_increment, rotation_3d
    shp, dshp = (9, 12, 12), (11, 10, 10)
    for rot, d in MAPS:
        M = affine_matrix_3d(rot, d, src_shape=shp, dst_shape=dshp)
        assert compose_rigid_increment(M, np.zeros(6), shp).tobytes() == M.tobytes()          # bit for bit
        Rm, sh = decode_rigid(M, shp, dshp)
        assert np.allclose(Rm, rotation_3d(rot), rtol=0, atol=1e-12) and np.allclose(sh, d, rtol=0, atol=1e-12)
        assert np.allclose(affine_matrix_3d(matrix=Rm, shift=sh, src_shape=shp, dst_shape=dshp), M, rtol=0, atol=1e-12)
        # against this file's own statement of the composition
        delta = np.array([0.3, -0.2, 0.1, 0.01, -0.02, 0.03])
        assert np.allclose(compose_rigid_increment(M, delta, shp), G3.compose(M, delta, shp), rtol=0, atol=1e-13)
    # a pure shift increment moves the source position by it; a pure rotation turns it about the centre of the moving volume
    M = affine_matrix_3d((0, 0, 0), (0, 0, 0), src_shape=shp)
    assert np.allclose(compose_rigid_increment(M, [1, 2, 3, 0, 0, 0], shp)[3::4], (1, 2, 3))
    c = 0.5 * (np.asarray(shp) - 1.0)
    assert np.allclose(F.apply(compose_rigid_increment(M, [0, 0, 0, 0.1, 0.2, -0.3], shp), c), c, atol=1e-13)
    quarter = compose_rigid_increment(M, [0, 0, 0, np.pi / 2, 0, 0], shp).reshape(3, 4)[:, :3]     # about s: +y towards +z
    assert np.allclose(quarter @ [0, 1, 0], [0, 0, 1], atol=1e-15)
    # the linear part stays a rotation through 50 compositions
    M = affine_matrix_3d((3, -5, 4), (1, 2, 3), src_shape=shp)
    rng = np.random.default_rng(0)
    for _ in range(50):
        M = compose_rigid_increment(M, rng.uniform(-0.2, 0.2, 6), shp)
    A = M.reshape(3, 4)[:, :3]
    assert np.allclose(A @ A.T, np.eye(3), rtol=0, atol=1e-12) and abs(np.linalg.det(A) - 1.0) < 1e-12
    # the step: H delta = -b, with damping (H + damping diag H) delta = -b; refusals
    Q = rng.normal(size=(8, 6))
    H, b = Q.T @ Q, rng.normal(size=6)
    assert np.allclose(H @ rigid_increment(H, b), -b, atol=1e-12)
    assert np.allclose((H + 0.5 * np.diag(np.diag(H))) @ rigid_increment(H, b, 0.5), -b, atol=1e-12)
    sing = H.copy()
    sing[:, 5], sing[5, :] = sing[:, 4], sing[4, :]
    sing[5, 5] = sing[4, 4]
    for bad in ((np.full((6, 6), np.nan), b, 0.0), (H, np.full(6, np.inf), 0.0), (sing, b, 0.0), (np.zeros((6, 6)), b, 1.0), (H, b, -1.0),
                (np.eye(5), b, 0.0)):
        with pytest.raises(ValueError):
            rigid_increment(*bad)
    assert np.all(np.isfinite(rigid_increment(sing, b, 0.1)))


def test_python_refusals_come_before_the_library(monkeypatch):
    from tomo_tv_amd import _lib, dual_axis, engine, inprocess

    def boom(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "load", boom)

    class Untouchable:
        def __getattr__(self, name):
            boom()
    sharded = object.__new__(engine.tomoengine)
    sharded.comm, sharded.sub_slabs, sharded.be = object(), 1, None
    subslab = object.__new__(engine.tomoengine)
    subslab.comm, subslab.sub_slabs, subslab.be = None, 2, object.__new__(engine._GroupBackend)
    whole = object.__new__(engine.tomoengine)
    whole.comm, whole.sub_slabs, whole.be = None, 1, object.__new__(engine._SlabBackend)
    I = np.eye(3, 4).ravel()
    for eng in (sharded, subslab):
        with pytest.raises(NotImplementedError):
            eng.volume_affine_normal(whole, I)
        with pytest.raises(NotImplementedError):
            whole.volume_affine_normal(eng, I)
    with pytest.raises(TypeError):
        whole.volume_affine_normal(object(), I)
    for M in (np.eye(3), np.zeros(11), np.full(12, np.nan)):
        with pytest.raises(ValueError):
            whole.volume_affine_normal(whole, M)
    with pytest.raises(ValueError):
        whole.volume_affine_normal(whole, I, margin=-1)
    with pytest.raises(NotImplementedError):
        object.__new__(engine._GroupBackend).c("volume_affine_normal", 0, None, 0, None, 1, None)
    with pytest.raises(NotImplementedError):
        inprocess.InProcessMultiGPU.volume_affine_normal(None, whole, I)
    dual = object.__new__(dual_axis.DualAxisTomo)
    dual.N, dual.a, dual.b, dual._reg = 16, Untouchable(), Untouchable(), None
    for pyr in ((), (2,), (1, 2), (3, 1), (2, 2, 1), (8, 1)):
        with pytest.raises(ValueError):
            dual.estimate_registration(pyramid=pyr)
    dual.N = 18
    with pytest.raises(ValueError):
        dual.estimate_registration(pyramid=(4, 1))
    assert dual._reg is None
    whole.be = subslab.be = None                                                 # (nothing to destroy)


def test_symbols_in_header_library_and_table():
    from tomo_tv_amd import _lib
    import sequences as S
    import test_abi_cpu
    src = open(os.path.join(ROOT, "include", "tomo_hip.h")).read()
    L = _lib.load()
    name = "tomo_volume_affine_normal"
    assert re.search(r"\bint %s\s*\(" % name, src) and hasattr(L, name)
    assert _lib.SIGNATURES[name] == [_lib._p, _lib._i, _lib._p, _lib._i, _lib._p, _lib._i, _lib._p]
    ident, out = np.eye(3, 4).ravel(), np.zeros(32)
    assert L.tomo_volume_affine_normal(None, 0, None, 0, ident.ctypes.data, 1, out.ctypes.data) == 1 and L.tomo_last_error()
    # the header declares exactly what the library exports
    nm = shutil.which("nm")
    assert nm, "binutils' nm is needed to list the library's exports"
    sym = subprocess.run([nm, "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = sorted(set(re.findall(r" T (tomo_\w+)$", sym, re.M)))
    declared = test_abi_cpu.declared_symbols()
    assert len(exported) == len(declared) and exported == declared
    names = S.header_prototypes(src)
    assert set(sequences_register3d.ROWS) <= set(names) and S.closure_errors(names) == []
    for phrase in ("all eight tap positions lie inside G", "[0..20] the upper triangle of J^T J, row-major", "q_y g_z - q_z g_y"):
        assert phrase in src, phrase


# ---- the loop ----------------------------------------------------------------------------------------------------------------------------
def exact_case(N=32):
    """F = the phantom resampled by the true map in binary64, G = the phantom: at the true map every counting voxel has r = 0"""
    X = D.phantom(N)
    M_true = F.matrix(POSE[0], POSE[1], 1.0, X.shape)
    return F.affine(X, M_true)[0], X, M_true


def test_exact_case_single_level_and_pyramid():
    Fv, Gv, M_true = exact_case()
    M, hist = G3.gauss_newton(Fv, Gv, max_iter=30, tol_shift=1e-12, tol_deg=1e-12)
    print(f"single level: {len(hist['step'])} iterations, worst entry error {np.max(np.abs(M - M_true)):.2e}, last step {hist['step'][-1]}")
    assert len(hist["step"]) < 30 and np.max(np.abs(M - M_true)) <= 1e-9
    Mp, levels = G3.pyramid(Fv, Gv, (4, 2, 1), max_iter=30, tol_shift=1e-12, tol_deg=1e-12)
    print(f"pyramid (4, 2, 1): iterations {[len(h['step']) for _, _, h in levels]}, worst entry error {np.max(np.abs(Mp - M_true)):.2e}")
    assert np.max(np.abs(Mp - M_true)) <= 1e-9
    with pytest.raises(RuntimeError):
        G3.gauss_newton(Fv, Gv, F.matrix((0, 0, 0), (29.0, 0, 0), 1.0, Gv.shape))      # 2 of 32 planes overlap: fewer than an eighth


@functools.lru_cache(maxsize=None)
def realistic(which):
    """tests/golden/A_N32_P9.npz, the phantom of DESIGN 8i, series B from the phantom moved by the pose (as
    test_affine3d_cpu.test_recovery_with_the_true_registration_beats_ignoring_it builds it), 30 Landweber iterations for each series
    on its own; F = x_A, G = cross(x_B), the loop from the identity with margin 1.
    -> dict(reg: the true registration's maps, est: the estimated (R, shift), err: (degrees, voxels), and what the drivers need)"""
    from tomo_tv_amd.align import rotation_3d
    from tomo_tv_amd.dual_axis import registration_maps
    rot, dm = POSE if which == 0 else POSE2
    g = np.load(os.path.join(GOLDEN, "A_N32_P9.npz"), allow_pickle=False)
    M = R.Matrix(int(g["N"]), g["angles_deg"], A=g["A"])
    N = M.N
    X = D.phantom(N)
    Rm = rotation_3d(rot)
    reg = registration_maps(N, shift=-(Rm.T @ dm), matrix=Rm.T)
    bA, bB = D.fp_a(M, X), F.moved_series_b(M, X, reg["to_b"])
    t = 1.0 / M.lipschitz()[0]
    xA, xB = D.single_axis(M, bA, t, 30), D.single_axis(M, bB, t, 30)
    Mest, hist = G3.gauss_newton(xA, D.cross(xB), max_iter=30, margin=1)
    Re, de = G3.decode(Mest, X.shape, X.shape)
    err = G3.pose_error(Mest, reg["to_a"], X.shape, X.shape)
    return dict(M=M, X=X, reg=reg, bA=bA, bB=bB, t=t, est=(Re, de), err=err, hist=hist, xA=xA, xB=xB)


def rmse_three_ways(c, R_est, d_est, K=30):
    """RMSE against the phantom after K registered alternating iterations with the true pose, with the estimate, and ignoring it"""
    from tomo_tv_amd.dual_axis import registration_maps
    M, X, t = c["M"], c["X"], c["t"]
    est = registration_maps(M.N, shift=d_est, matrix=R_est)
    x_true = F.dual_axis_registered(M, M, c["bA"], c["bB"], t, t, K, c["reg"]["to_a"], c["reg"]["to_b"])[0]
    x_est = F.dual_axis_registered(M, M, c["bA"], c["bB"], t, t, K, est["to_a"], est["to_b"])[0]
    x_ign = D.dual_axis(M, M, c["bA"], c["bB"], t, t, K)
    return D.rmse(x_true, X), D.rmse(x_est, X), D.rmse(x_ign, X)


def test_realistic_case_recovers_the_pose():
    """Recorded: the figures printed below."""
    c = realistic(0)
    print(f"8 degrees about y + (1.5, 0, -2.25): rotation error {c['err'][0]:.3f} degrees, worst shift error {c['err'][1]:.3f} voxel, "
          f"{len(c['hist']['step'])} iterations, last step {c['hist']['step'][-1]}")
    assert c["err"][0] <= 0.5 and c["err"][1] <= 0.25
    e_true, e_est, e_ign = rmse_three_ways(c, *c["est"])
    print(f"RMSE after 30 registered iterations: {e_est:.4f} with the estimate, {e_true:.4f} with the true pose, {e_ign:.4f} ignoring it")
    assert e_est < 0.5 * (e_true + e_ign)


def test_realistic_case_second_pose():
    """(3, -5, 4) degrees with shift (-2, 1.25, 0.75): the pose error is recorded, the condition is the RMSE midpoint."""
    c = realistic(1)
    print(f"second pose: rotation error {c['err'][0]:.3f} degrees, worst shift error {c['err'][1]:.3f} voxel, {len(c['hist']['step'])} iterations")
    e_true, e_est, e_ign = rmse_three_ways(c, *c["est"])
    print(f"RMSE after 30 registered iterations: {e_est:.4f} with the estimate, {e_true:.4f} with the true pose, {e_ign:.4f} ignoring it")
    assert e_est < 0.5 * (e_true + e_ign)
