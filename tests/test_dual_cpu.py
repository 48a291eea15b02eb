"""Dual-axis tomography without a GPU: the binary64 statements (tests/ref64_dual.py) against plain loops, the adjointness of the second
engine's stacked operator, the zero-tilt transpose property that fixes the geometry convention, the recovery case (the alternating
loop beats a single axis at the same number of projector applications), the ABI, and ``DualAxisTomo``'s refusals."""
import os
import re

import numpy as np
import pytest

import ref64 as R
import ref64_dual as D
from conftest import GOLDEN, ROOT


def matrix(name):
    g = np.load(os.path.join(GOLDEN, name), allow_pickle=False)
    return R.Matrix(int(g["N"]), g["angles_deg"], A=g["A"]), g["angles_deg"]


@pytest.fixture(scope="module")
def m16():
    return matrix("A_N16_P5.npz")[0]


@pytest.fixture(scope="module")
def m32():
    return matrix("A_N32_P9.npz")


@pytest.mark.parametrize("N", [3, 4])
def test_statements_equal_the_loops(N):
    rng = np.random.default_rng(N)
    S, Dst = rng.standard_normal((N, N, N)).astype(np.float32), rng.standard_normal((N, N, N)).astype(np.float32)
    assert np.array_equal(D.cross(S), D.cross_loops(S)) and np.array_equal(D.cross(D.cross(S)), S)
    assert D.cross(S)[2, 1, 0] == S[0, 1, 2]
    for a in (0.0, 1.0, -0.75, 2.5):
        for clamp in (False, True):
            assert np.array_equal(D.cross_axpy(S, Dst, a, clamp), D.cross_axpy_loops(S, Dst, a, clamp))
    S[0, 1, 2] = np.nan
    got = D.cross_axpy(S, Dst, 1.0, True)
    assert got[2, 1, 0] == 0.0 and np.isnan(D.cross_axpy(S, Dst, 1.0, False)[2, 1, 0])             # the clamp takes a NaN to 0
    S[0, 1, 2] = np.inf
    assert np.isnan(D.cross_axpy(S, Dst, 0.0)[2, 1, 0]) and D.cross_axpy(S, Dst, 0.5)[2, 1, 0] == np.inf


def test_stacked_operator_of_the_second_engine_and_its_adjoint(m16):
    N = m16.N
    rng = np.random.default_rng(0)
    x, r = rng.standard_normal((N, N, N)), rng.standard_normal((N, m16.nrow))
    fp = D.fp_b(m16, x)
    assert np.allclose(fp, D.fp_b_dense(m16, x), rtol=1e-13, atol=1e-13)
    # slice z of B's data is the projection of the image X[:, :, z]^T (rows y, columns s)
    z = 5
    assert np.allclose(fp[z], D.dense(m16) @ x[:, :, z].T.ravel(), rtol=1e-13, atol=1e-13)
    lhs, rhs = float(np.vdot(fp, r)), float(np.vdot(x, D.bp_b(m16, r)))
    print(f"<A_B x, r> = {lhs!r}, <x, A_B^T r> = {rhs!r}, relative gap {abs(lhs - rhs) / abs(lhs):.1e}")
    assert abs(lhs - rhs) <= 1e-13 * abs(lhs)


def test_zero_tilt_projections_of_the_two_series_are_transposes(m32):
    M, ang = m32
    N, k = M.N, 4
    assert ang[k] == 0.0
    # the rule behind it: at 0 degrees the rays run along the image's row index and ray j meets column j
    img = np.zeros((1, N, N))
    img[0, :, 7] = 1.0                                                     # one column set: a single ray
    p = M.fp(img).reshape(M.P, N)[k]
    assert np.count_nonzero(p) == 1 and p[7] > 0
    img[:] = 0.0
    img[0, 7, :] = 1.0                                                     # one row set: every ray
    assert np.count_nonzero(M.fp(img).reshape(M.P, N)[k]) == N
    X = np.random.default_rng(1).random((N, N, N))
    PA = D.fp_a(M, X).reshape(N, M.P, N)[:, k, :]                          # [s][ray = z]
    PB = D.fp_b(M, X).reshape(N, M.P, N)[:, k, :]                          # [z][ray = s]
    assert np.allclose(PB, PA.T, rtol=1e-13, atol=1e-13)
    assert not np.allclose(D.fp_b(M, X).reshape(N, M.P, N)[:, 2, :], D.fp_a(M, X).reshape(N, M.P, N)[:, 2, :].T, rtol=1e-3)


@pytest.mark.parametrize("name,K", [("A_N32_P9.npz", 100), ("A_N16_P5.npz", 100)])
def test_recovery_dual_axis_beats_a_single_axis_at_equal_projector_work(name, K):
    """Both series with the fixture's angles, beta = 1 / L, clamp at 0.  The alternating loop after K iterations against the
    single-axis loop after 2K (the same number of projector applications).  Recorded:
    N = 32, P = 9: single K 0.0607, single 2K 0.0522, dual K 0.0456;  N = 16, P = 5: 0.0472, 0.0393, 0.0259."""
    M, _ = matrix(name)
    X = D.phantom(M.N)
    bA, bB = D.fp_a(M, X), D.fp_b(M, X)
    t = 1.0 / M.lipschitz()[0]
    single = D.single_axis(M, bA, t, K)
    e1, e2 = D.rmse(single, X), D.rmse(D.single_axis(M, bA, t, K, x0=single), X)
    ed = D.rmse(D.dual_axis(M, M, bA, bB, t, t, K), X)
    print(f"{name}: RMSE single {K}: {e1:.4f}, single {2 * K}: {e2:.4f}, dual-axis {K}: {ed:.4f}")
    assert ed < e2 < e1


def test_symbols_in_header_library_and_table():
    from tomo_tv_amd import _lib
    src = open(os.path.join(ROOT, "include", "tomo_hip.h")).read()
    L = _lib.load()
    sig = {"tomo_volume_cross": [_lib._p, _lib._i, _lib._p, _lib._i],
           "tomo_volume_cross_axpy": [_lib._p, _lib._i, _lib._p, _lib._i, _lib._f, _lib._i]}
    for name, args in sig.items():
        assert re.search(r"\bint %s\s*\(" % name, src), name
        assert hasattr(L, name) and _lib.SIGNATURES[name] == args
    assert L.tomo_volume_cross(None, 0, None, 0) == 1 and L.tomo_last_error()                 # null engines: TOMO_ERR_ARG, no crash
    assert L.tomo_volume_cross_axpy(None, 0, None, 0, 1.0, 0) == 1 and L.tomo_last_error()
    assert "X_B[z][y][s] = X_A[s][y][z]" in src and "P_B[z][ray = s] = P_A[s][ray = z]" in src


def test_dual_axis_tomo_refuses_non_cubes_before_touching_the_library(monkeypatch):
    from tomo_tv_amd import _lib, dual_axis

    def boom(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "load", boom)
    monkeypatch.setattr(dual_axis, "TomoGPU", boom)
    ang = np.linspace(-60, 60, 3)
    z = lambda *s: np.zeros(s, np.float32)   # noqa: E731
    for sa, sb in (((8, 6, 3), (8, 8, 3)), ((8, 8, 3), (6, 8, 3)), ((8, 8, 3), (16, 16, 3)), ((8, 8), (8, 8, 3)), ((6, 8, 3), (6, 8, 3))):
        with pytest.raises(ValueError):
            dual_axis.DualAxisTomo(ang, z(*sa), ang, z(*sb))


def test_sharded_group_and_inprocess_classes_refuse():
    from tomo_tv_amd import engine, inprocess
    sharded = object.__new__(engine.tomoengine)
    sharded.comm, sharded.sub_slabs, sharded.be = object(), 1, None
    subslab = object.__new__(engine.tomoengine)
    subslab.comm, subslab.sub_slabs, subslab.be = None, 2, object.__new__(engine._GroupBackend)
    whole = object.__new__(engine.tomoengine)
    whole.comm, whole.sub_slabs, whole.be = None, 1, object.__new__(engine._SlabBackend)
    for eng in (sharded, subslab):
        with pytest.raises(NotImplementedError):
            eng.cross_volume_to(whole)
        with pytest.raises(NotImplementedError):
            eng.cross_axpy_volume_to(whole, 0.5)
        with pytest.raises(NotImplementedError):
            whole.cross_volume_to(eng)                                                 # ... as the partner too
    with pytest.raises(TypeError):
        whole.cross_volume_to(object())
    group = object.__new__(engine._GroupBackend)
    with pytest.raises(NotImplementedError):
        group.c("volume_cross", 0, None, 0)
    with pytest.raises(NotImplementedError):
        group.c("volume_cross_axpy", 0, None, 0, 1.0, 0)
    for name in ("cross_volume_to", "cross_axpy_volume_to"):
        with pytest.raises(NotImplementedError):
            getattr(inprocess.InProcessMultiGPU, name)(None, whole)
    whole.be = None                                                                    # (nothing to destroy)
    subslab.be = None
