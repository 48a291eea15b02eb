"""Chambolle-Pock (``pdhg_tv``) without a GPU: the binary64 reference of tests/ref64_pdhg.py against its own mathematics (adjointness,
descent, both step modes reach the same minimum), the bound helpers against the float32 replay (dense data and both branch points),
and the presence of the new entry points in the header, the ctypes table, the built library and the Python surface."""
import inspect
import os
import re

import numpy as np
import pytest

import ref64
import ref64_pdhg as R
from conftest import ROOT

F32 = np.float32
SYMBOLS = ("tomo_pdhg_sino_dual", "tomo_pdhg_tv_step", "tomo_pdhg_begin", "tomo_pdhg")


@pytest.mark.parametrize("nx,n", [(1, 8), (3, 5), (65, 4)])
def test_divergence_is_the_negative_adjoint_of_the_gradient(nx, n):
    rng = np.random.default_rng(nx * 100 + n)
    x = rng.standard_normal((nx, n, n))
    p = rng.standard_normal((3, nx, n, n))
    p[0][-1] = 0
    p[1][:, -1] = 0
    p[2][:, :, -1] = 0
    lhs, rhs = float(np.sum(R.grad(x) * p)), -float(np.sum(x * R.div(p)))
    scale = float(np.sum(np.abs(R.grad(x) * p)))
    assert abs(lhs - rhs) <= 1e-12 * scale, (lhs, rhs)


@pytest.fixture(scope="module")
def small():
    """lin70-like geometry: N = 16, 9 angles, 3 slices, b = A x_true of a block phantom."""
    M = ref64.Matrix(16, np.linspace(-70, 70, 9))
    xt = R.block_phantom(3, 16)
    b = xt.reshape(3, -1).astype(np.float64) @ R.dense(M).T
    return M, b


def test_objective_descends_in_both_modes(small):
    M, b = small
    lam = 0.1
    for precond in (False, True):
        s50 = R.pdhg(M, b, 50, lam, precond=precond)
        s400 = R.pdhg(M, b, 350, lam, precond=precond, state=s50)
        o50, o400 = R.objective(M, s50["x"], b, lam), R.objective(M, s400["x"], b, lam)
        print(f"precond={precond}: objective {o50:.6g} after 50, {o400:.6g} after 400")
        assert o400 < o50


def test_both_modes_reach_the_same_minimum(small):
    """The gap between the modes' objectives at 4000 iterations is no larger than ten times what either still changes up to 8000
    (floor: the binary64 rounding of the objective itself, 1e-12 relative)."""
    M, b = small
    lam = 0.1
    obj = {}
    for precond in (False, True):
        s4 = R.pdhg(M, b, 4000, lam, precond=precond)
        s8 = R.pdhg(M, b, 4000, lam, precond=precond, state=s4)
        obj[precond] = (R.objective(M, s4["x"], b, lam), R.objective(M, s8["x"], b, lam))
    gap = abs(obj[False][0] - obj[True][0])
    change = max(abs(o[0] - o[1]) for o in obj.values())
    print(f"objective at 4000: scalar {obj[False][0]:.12g}, diagonal {obj[True][0]:.12g}; gap {gap:.3e}, 4000->8000 change {change:.3e}")
    assert gap <= 10 * change + 1e-12 * abs(obj[True][0])


def test_float32_replay_within_its_own_yardstick(small):
    M, b = small
    for precond in (False, True):
        b32 = b.astype(F32)
        f64 = R.pdhg(M, b32, 20, 0.125, precond=precond)
        f32 = R.pdhg(M, b32, 20, 0.125, precond=precond, dtype=F32)
        ref64.assert_seq(f"pdhg replay precond={precond}", f32["x"], f32["x"], f64["x"])
        assert f32["x"].dtype == F32 and f32["p"].dtype == F32 and f32["q"].dtype == F32
        assert np.max(np.abs(f32["x"] - f64["x"])) < 1e-3 * np.max(np.abs(f64["x"]))


def _dense_inputs(nx, n, lam, seed):
    rng = np.random.default_rng(seed)
    x = ref64.dense_volume(nx, n, seed)
    xbar = ref64.dense_volume(nx, n, seed + 1)
    p = (rng.standard_normal((3, nx, n, n)) * lam * 0.55).astype(F32)         # |p|_2 > lam on about a third of the voxels
    u = (rng.standard_normal((nx, n, n)) * 3.0).astype(F32)                   # signed: some voxels clamp
    return x, xbar, u, p


def _check_step(name, x, xbar, u, p, sg, lam, theta, tau=None, colsum=None):
    (xn, xb, pn), (ex, exb, ep) = R.tv_step_bound(x, xbar, u, p, sg, lam, theta, tau=tau, colsum=colsum)
    T = F32(tau) if colsum is None else R.primal_T(colsum, x.shape[0], x.shape[1], F32)
    g = R.tv_step(x, xbar, u, p, F32(sg), T, F32(lam), F32(theta), F32)
    for what, got, ref, bound in (("x", g[0], xn, ex), ("xbar", g[1], xb, exb), ("p", g[2], pn, ep)):
        print(f"ratio {name} {what}: {ref64.ratio(got, ref, bound):.3f}")
        ref64.assert_within(f"{name} {what}", got, ref, bound)
    return xn, pn


def test_one_step_bounds_hold_for_the_float32_replay_dense():
    nx, n, lam = 5, 9, 0.5
    x, xbar, u, p = _dense_inputs(nx, n, lam, 3)
    xn, pn = _check_step("scalar", x, xbar, u, p, 0.3, lam, 1.0, tau=0.2)
    over = np.sqrt(np.sum(np.asarray(p, np.float64) ** 2, axis=0)) > lam
    assert 0.15 < over.mean() < 0.6 and (xn == 0).any() and (xn > 0).any()
    colsum = np.random.default_rng(4).uniform(3.0, 9.0, n * n).astype(F32)
    _check_step("diagonal", x, xbar, u, p, 0.5, lam, 1.0, colsum=colsum)


def test_one_step_bounds_cover_both_sides_of_the_branch_points():
    nx, n, lam = 4, 6, 0.5
    x, xbar, u, p = _dense_inputs(nx, n, lam, 7)
    # |a|_2 = lam exactly: constant xbar, p = (0.3, 0.4, 0) lam-scaled where the rows exist
    xbar_c = np.full_like(xbar, 1.0)
    pb = np.zeros_like(p)
    pb[0], pb[1] = F32(0.3), F32(0.4)
    _, a = R.dual_field(xbar_c, pb, 0.5, lam)
    nrm = np.sqrt(np.sum(a * a, axis=0))
    assert np.count_nonzero(np.abs(nrm - 0.5) < 1e-7) > nx * n * n // 2
    _check_step("|a|=lam", x, xbar_c, u, pb, 0.5, 0.5, 1.0, tau=0.2)
    # x = T (u - div p) exactly: p = 0 and constant xbar give div p = 0; T = 1/4, u = 4 x
    z = np.zeros_like(p)
    _check_step("x=T(u-div)", x, xbar_c, (x * F32(4)).astype(F32), z, 0.5, lam, 1.0, tau=0.25)


def test_sino_dual_bound_holds_for_the_float32_replay():
    q, g, b = (ref64.signed_sino(5, 40, s) for s in (1, 2, 3))
    rs = np.random.default_rng(5).uniform(2.0, 20.0, 40).astype(F32)
    rs[::9] = 0
    r, e = R.sino_dual_bound(q, g, b, S=F32(0.07))
    ref64.assert_within("sino scalar", R.sino_dual(q, g, b, F32(0.07), F32), r, e)
    r, e = R.sino_dual_bound(q, g, b, rowsum=rs)
    ref64.assert_within("sino diagonal", R.sino_dual(q, g, b, R.dual_S(rs, F32), F32), r, e)
    assert np.array_equal(r[:, ::9], q[:, ::9].astype(np.float64))            # an empty ray leaves q alone


def test_symbols_in_header_ctypes_table_and_library():
    from tomo_tv_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tomo_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(tomo_[a-z0-9_]+)\s*\(", src))
    L = _lib.load()
    for name in SYMBOLS:
        assert name in declared, name
        assert name in _lib.SIGNATURES, name
        assert hasattr(L, name), name
    assert "tv_chambolle.cu" in open(os.path.join(ROOT, "include", "tomo_hip.h")).read()
    # null engines: an error code and a message, nothing initialised
    assert L.tomo_pdhg_begin(None) != 0 and L.tomo_last_error()
    assert L.tomo_pdhg(None, 1, 0.1, 1.0, 1, 1.0, -1) != 0
    assert L.tomo_pdhg_sino_dual(None, 3, 1, 0, 0.1, 0) != 0
    assert L.tomo_pdhg_tv_step(None, 0, 3, 1, 5, 0.1, 0.1, 0.1, 1.0, 0, -1) != 0


def test_python_surface():
    from tomo_tv_amd import pytvlib
    from tomo_tv_amd.engine import tomoengine
    from tomo_tv_amd.reconstructor import TomoGPU
    E = inspect.Parameter.empty
    sig = lambda f: [(p.name, p.default) for p in inspect.signature(f).parameters.values()]  # noqa: E731
    assert sig(TomoGPU.pdhg_tv) == [("self", E), ("Niter", 100), ("lambda_param", 0.1), ("theta", 1.0), ("precond", True), ("ratio", 1.0),
                                    ("show_convergence", True)]
    assert sig(tomoengine.pdhg)[:6] == [("self", E), ("niter", E), ("lam", E), ("theta", 1.0), ("precond", True), ("ratio", 1.0)]
    assert sig(tomoengine.pdhg_begin) == [("self", E)]
    assert callable(tomoengine.pdhg_sino_dual) and callable(tomoengine.pdhg_tv_step)

    class Spy:
        def __getattr__(self, name):
            return lambda *a, **k: calls.append((name, a, k))
    calls = []
    pytvlib.initialize_algorithm(Spy(), "pdhg")
    pytvlib.run(Spy(), "pdhg", 0.2, 7, theta=1.0, precond=False, ratio=2.0)
    assert ("pdhg", (7, 0.2), dict(theta=1.0, precond=False, ratio=2.0)) in calls
