"""Chambolle-Pock (``tomo_pdhg*``, k_pdhg_tv / k_pdhg_sino) on the GPU against the binary64 reference of tests/ref64_pdhg.py.

Shapes of the TV / FGP element-wise tests: N in {8, 31, 33} x Nx in {1, 63, 64, 65, 129} (a partial chunk, a chunk edge, two chunks plus
one slice, n % 8 != 0).  Exact structure bit for bit (one-hot xbar -> p, one-hot p -> div p, the extrapolation on a 2^-8 grid), one dense
step and the dual sinogram inside their per-element bounds in both step modes, the loop against the float32 replay's yardstick, the
driver, the refusals and non-interference with ``fista`` / ``asd_pocs``.  Padding slices cannot be read through the ABI; tomo_l1_norm
sums a whole slot, padding included, and its terms are exact, so "padding is 0" is checked as S_L1 == sum |real slices| to the
double summation's rounding.
"""
import numpy as np
import pytest

import ref64
import ref64_pdhg as R
from tomo_tv_amd import _lib
from tomo_tv_amd._lib import S_DIFF, S_L1, SINO_USER0, VOL_RECON, VOL_USER0, VOL_YK
from tomo_tv_amd.engine import _ptr, ctvlib, system_matrix, tomoengine
from tomo_tv_amd.reconstructor import TomoGPU

pytestmark = pytest.mark.gpu
F32 = np.float32
X, XBAR, UVOL, P0 = VOL_USER0, VOL_USER0 + 1, VOL_USER0 + 2, VOL_USER0 + 3
ANGLES = np.linspace(-70, 70, 5)
CASES = [(n, nx) for n in (8, 31, 33) for nx in (1, 63, 64, 65, 129)]
IDS = [f"N{n}-nx{nx}" for n, nx in CASES]
_M = {}


def matrix(n, angles=ANGLES):
    key = (n, tuple(angles))
    if key not in _M:
        _M[key] = ref64.Matrix(n, angles)
    return _M[key]


def new_engine(n, nx, angles=ANGLES):
    return tomoengine(nx, n, np.asarray(angles) * np.pi / 180)


def positions(nx, n):
    """Every corner, every face centre, the chunk-edge slices 63 and 64 and an interior voxel."""
    pos = {(s, y, z) for s in (0, nx - 1) for y in (0, n - 1) for z in (0, n - 1)}
    c = (nx // 2, n // 2, n // 2)
    for a, m in enumerate((nx, n, n)):
        for e in (0, m - 1):
            q = list(c)
            q[a] = e
            pos.add(tuple(q))
    pos.update((s, n // 2, n // 3) for s in (63, 64) if s < nx)
    pos.add((nx // 3, n // 3, n // 2 + 1))
    return sorted(pos)


def put(t, **fields):
    slot = dict(x=X, xbar=XBAR, u=UVOL)
    for k, v in fields.items():
        if k == "p":
            for a in range(3):
                t.set_volume(v[a], P0 + a)
        else:
            t.set_volume(v, slot[k])


def get_p(t):
    return np.stack([t.get_volume(P0 + a) for a in range(3)])


def padding_is_zero(t, slots_and_values):
    for slot, v in slots_and_values:
        t.be.c("l1_norm", slot)
        ref, bound = ref64.l1(v)
        ref64.assert_scalar(f"padding of slot {slot}", t._scalar(S_L1), ref, bound + ref64.TINY)


@pytest.mark.parametrize("n,nx", CASES, ids=IDS)
def test_exact_structure(gpu, n, nx):
    t = new_engine(n, nx)
    shape = (nx, n, n)
    four, zero = np.full(shape, 4.0, F32), np.zeros(shape, F32)
    # (1) p = 0, lambda = 2^20, sigma = 1/2: p_new = 1/2 grad xbar exactly, 0 at the last index of each axis and in the padding
    for pos in positions(nx, n):
        xbar = four.copy()
        xbar[pos] = 5.0
        put(t, x=four, xbar=xbar, u=zero, p=np.zeros((3,) + shape, F32))
        t.pdhg_tv_step(X, XBAR, UVOL, P0, sigma=0.5, tau=1.0, lam=2.0 ** 20, theta=1.0, precond=False)
        p = get_p(t)
        want = 0.5 * R.grad(xbar)
        assert np.array_equal(p.astype(np.float64), want), pos
        for a in range(3):
            assert not np.take(p[a], -1, axis=a).any(), (pos, a)
        padding_is_zero(t, [(P0 + a, p[a]) for a in range(3)])
    # (2) constant xbar (p unchanged), u = 0, tau = 1, lambda = 2, one-hot p_a = 1: x_new - 4 = div p exactly; a one-hot at the
    #     last index of its axis contributes nothing and is read back as 0
    for pos in positions(nx, n):
        for a in range(3):
            p = np.zeros((3,) + shape, F32)
            p[a][pos] = 1.0
            put(t, x=four, xbar=four, u=zero, p=p)
            t.pdhg_tv_step(X, XBAR, UVOL, P0, sigma=0.5, tau=1.0, lam=2.0, theta=1.0, precond=False)
            pn = get_p(t)
            want = p.copy()
            if pos[a] == shape[a] - 1:
                want[a][pos] = 0.0
            assert np.array_equal(pn, want), (pos, a)
            assert np.array_equal(t.get_volume(X).astype(np.float64) - 4.0, R.div(want)), (pos, a)
    # (3) the extrapolation with theta = 1 on a 2^-8 grid: xbar_new = x_new + (x_new - x) exactly
    rng = np.random.default_rng(n * 1000 + nx)
    x = (rng.integers(0, 1024, shape) / 256.0).astype(F32)
    u = (rng.integers(-512, 1024, shape) / 256.0).astype(F32)
    put(t, x=x, xbar=four, u=u, p=np.zeros((3,) + shape, F32))
    t.pdhg_tv_step(X, XBAR, UVOL, P0, sigma=0.5, tau=1.0, lam=2.0, theta=1.0, precond=False)
    xn = t.get_volume(X)
    assert np.array_equal(xn, np.maximum(x - u, 0))
    assert np.array_equal(t.get_volume(XBAR).astype(np.float64), 2.0 * xn.astype(np.float64) - x)
    padding_is_zero(t, [(X, xn), (XBAR, t.get_volume(XBAR))])


def dense_inputs(nx, n, lam, seed):
    rng = np.random.default_rng(seed)
    x = ref64.dense_volume(nx, n, seed)
    xbar = ref64.dense_volume(nx, n, seed + 1)
    p = (rng.standard_normal((3, nx, n, n)) * lam * 0.55).astype(F32)         # |p|_2 > lambda on about a third of the voxels
    u = (rng.standard_normal((nx, n, n)) * 3.0).astype(F32)                   # signed: some voxels clamp
    return x, xbar, u, p


@pytest.mark.parametrize("n,nx", CASES, ids=IDS)
def test_one_dense_step_within_bounds(gpu, n, nx):
    M = matrix(n)
    t = new_engine(n, nx)
    lam, theta = 0.5, 1.0
    x, xbar, u, p = dense_inputs(nx, n, lam, n * 100 + nx)
    over = np.sqrt(np.sum(p.astype(np.float64) ** 2, axis=0)) > lam
    assert 0.15 < over.mean() < 0.6
    for precond in (False, True):
        put(t, x=x, xbar=xbar, u=u, p=p)
        if precond:
            ref, bound = R.tv_step_bound(x, xbar, u, p, 0.5, lam, theta, colsum=R.tables_f32(M)[1])
        else:
            ref, bound = R.tv_step_bound(x, xbar, u, p, F32(0.3), lam, theta, tau=F32(0.2))
        t.pdhg_tv_step(X, XBAR, UVOL, P0, sigma=0.3, tau=0.2, lam=lam, theta=theta, precond=precond, slot=S_DIFF)
        got = (t.get_volume(X), t.get_volume(XBAR), get_p(t))
        assert (ref[0] == 0).any() and (ref[0] > 0).any()
        for name, g, r, b in zip(("x", "xbar", "p"), got, ref, bound):
            print(f"ratio pdhg_tv_step precond={int(precond)} {name}: {ref64.ratio(g, r, b):.3f}")
        for name, g, r, b in zip(("x", "xbar", "p"), got, ref, bound):
            ref64.assert_within(f"precond={int(precond)} {name}", g, r, b)
        sq, sqb = ref64.sqdiff(got[0], x)
        ref64.assert_scalar("sum (x_new - x)^2", t._scalar(S_DIFF), sq, sqb)
        padding_is_zero(t, [(X, got[0]), (XBAR, got[1])] + [(P0 + a, got[2][a]) for a in range(3)])
        assert np.array_equal(t.get_volume(UVOL), u)


@pytest.mark.parametrize("n,nx", [(8, 65), (33, 129), (31, 64)], ids=["N8-nx65", "N33-nx129", "N31-nx64"])
def test_sino_dual_within_bounds(gpu, n, nx):
    A = system_matrix(n, ANGLES)
    empty = n + n // 2                                                        # a ray of the second angle, emptied
    A = np.ascontiguousarray(A[:, A[0] != empty])
    M = ref64.Matrix(n, ANGLES, A=A)
    assert M.row_nnz[empty] == 0
    t = ctvlib(nx, n, len(ANGLES))
    t.load_A(A)
    q, g, b = (ref64.signed_sino(nx, M.nrow, s + nx) for s in (1, 2, 3))
    q[:, empty] = 0
    QS, GS, BS = SINO_USER0, SINO_USER0 + 1, SINO_USER0 + 2
    for precond in (False, True):
        for slot, v in ((QS, q), (GS, g), (BS, b)):
            t.be.c("set_sinogram", slot, _ptr(v))
        if precond:
            ref, bound = R.sino_dual_bound(q, g, b, rowsum=R.tables_f32(M)[0])
        else:
            ref, bound = R.sino_dual_bound(q, g, b, S=F32(0.07))
        t.pdhg_sino_dual(QS, GS, BS, sigma=0.07, precond=precond)
        got = t._sino(QS)
        print(f"ratio pdhg_sino_dual precond={int(precond)}: {ref64.ratio(got, ref, bound):.3f}")
        ref64.assert_within(f"sino_dual precond={int(precond)}", got, ref, bound)
        if precond:
            assert not got[:, empty].any()
        assert np.array_equal(t._sino(GS), g) and np.array_equal(t._sino(BS), b)


LOOP = {"lin70": (np.linspace(-70, 70, 9), 32, 128), "repeat": (np.array([-40.0, -10.0, 15.0, 15.0, 50.0]), 8, 65)}


@pytest.mark.parametrize("gid", list(LOOP))
@pytest.mark.parametrize("precond", [False, True], ids=["scalar", "diagonal"])
def test_loop_against_the_replays(gpu, gid, precond):
    ang, n, nx = LOOP[gid]
    M = matrix(n, ang)
    b = M.fp(R.block_phantom(nx, n)).astype(F32)
    lam = 0.125                                                               # exact in float32: the same number in the engine and the replays
    t = new_engine(n, nx, ang)
    t.set_tilt_series(b)
    t.restart_recon()
    t.pdhg_begin()
    t.pdhg(20, lam, precond=precond)
    x20, xb20 = t.get_volume(VOL_RECON), t.get_volume(VOL_YK)
    L = t.get_lipschitz()
    f64 = R.pdhg(M, b, 20, lam, precond=precond, L=L)
    f32 = R.pdhg(M, b, 20, lam, precond=precond, L=L, dtype=F32)
    bound = ref64.seq_bound(f32["x"], f64["x"])
    print(f"ratio pdhg loop {gid} precond={int(precond)}: {ref64.ratio(x20, f64['x'], bound):.3f}")
    ref64.assert_within(f"pdhg x {gid}", x20, f64["x"], bound)
    assert np.max(np.abs(f64["x"])) > 0.05
    # 4 calls of 5 (the last split 4 + 1, with the step norm of the last iteration) give the same bits
    t.restart_recon()
    t.pdhg_begin()
    for _ in range(3):
        t.pdhg(5, lam, precond=precond)
    t.pdhg(4, lam, precond=precond)
    x19 = t.get_volume(VOL_RECON)
    t.pdhg(1, lam, precond=precond, slot=S_DIFF)
    assert np.array_equal(t.get_volume(VOL_RECON), x20) and np.array_equal(t.get_volume(VOL_YK), xb20)
    sq, sqb = ref64.sqdiff(x20, x19)
    ref64.assert_scalar("sum (x_new - x)^2", t._scalar(S_DIFF), sq, sqb)
    t.restart_recon()
    t.pdhg_begin()
    for _ in range(4):
        t.pdhg(5, lam, precond=precond)
    assert np.array_equal(t.get_volume(VOL_RECON), x20)


def _tilt_series(M, nx):
    b = M.fp(R.block_phantom(nx, M.N)).astype(F32)
    return b, np.ascontiguousarray(b.reshape(nx, M.P, M.N).transpose(0, 2, 1))


def test_driver_and_refusals(gpu):
    ang, n, nx = np.linspace(-70, 70, 9), 32, 6
    M = matrix(n, ang)
    b, ts = _tilt_series(M, nx)
    g = TomoGPU(ang, ts, gpu_id=0)
    cost = g.pdhg_tv(Niter=10)
    assert cost.shape == (10,) and np.all(np.isfinite(cost)) and np.all(cost > 0)
    t = new_engine(n, nx, ang)
    t.set_tilt_series(b)
    t.restart_recon()
    t.pdhg_begin()
    t.pdhg(10, 0.1)
    assert np.array_equal(g.get_recon(), t.get_volume(VOL_RECON).astype(np.float64))
    quiet = TomoGPU(ang, ts, gpu_id=0)
    quiet.pdhg_tv(Niter=10, show_convergence=False)
    assert np.array_equal(quiet.get_recon(), g.recon)
    with pytest.raises(NotImplementedError, match="one whole-volume engine"):
        TomoGPU(ang, ts, gpu_id=0, sub_slabs=2).pdhg_tv(Niter=1)
    L = _lib.load()
    assert L.tomo_set_slab_edges(t.be.h, 0, 1) == 0
    for rc in (L.tomo_pdhg_begin(t.be.h), L.tomo_pdhg(t.be.h, 1, 0.1, 1.0, 1, 1.0, -1), L.tomo_pdhg_sino_dual(t.be.h, 3, 1, 0, 0.1, 0),
               L.tomo_pdhg_tv_step(t.be.h, X, XBAR, UVOL, P0, 0.1, 0.1, 0.1, 1.0, 0, -1)):
        assert rc == 3 and b"whole-volume" in L.tomo_last_error()
    assert L.tomo_set_slab_edges(t.be.h, 1, 1) == 0
    # bad arguments: overlapping or out-of-range slots, lambda <= 0, sigma or tau <= 0 in scalar mode
    for args in ((X, X, UVOL, P0, 0.1, 0.1, 0.1, 1.0, 0, -1), (X, XBAR, UVOL, P0 - 1, 0.1, 0.1, 0.1, 1.0, 0, -1),
                 (X, XBAR, UVOL, 43, 0.1, 0.1, 0.1, 1.0, 0, -1), (X, XBAR, UVOL, P0, 0.1, 0.1, 0.0, 1.0, 1, -1),
                 (X, XBAR, UVOL, P0, 0.0, 0.1, 0.1, 1.0, 0, -1), (X, XBAR, UVOL, P0, 0.1, -1.0, 0.1, 1.0, 0, -1)):
        assert L.tomo_pdhg_tv_step(t.be.h, *args) == 1, args
    assert L.tomo_pdhg_sino_dual(t.be.h, 3, 3, 0, 0.1, 0) == 1 and L.tomo_pdhg_sino_dual(t.be.h, 3, 1, 0, 0.0, 0) == 1
    assert L.tomo_pdhg(t.be.h, 1, -0.1, 1.0, 1, 1.0, -1) == 1


def test_other_drivers_are_left_alone(gpu):
    """fista and asd_pocs after a pdhg_tv run on the same engine give the bits of a fresh engine: the scratch volumes, YK, TEMP and
    the projection claims are left coherent."""
    ang, n, nx = np.linspace(-70, 70, 9), 32, 6
    _, ts = _tilt_series(matrix(n, ang), nx)
    used, fresh = TomoGPU(ang, ts, gpu_id=0), TomoGPU(ang, ts, gpu_id=0)
    used.pdhg_tv(Niter=3)
    for g in (used, fresh):
        g.tomo.restart_recon()
    # (the cost vectors come from double sums that the workgroups add atomically: equal to the rounding of that order, 1e-12)
    assert np.allclose(used.fista(Niter=2), fresh.fista(Niter=2), rtol=1e-12, atol=0)
    assert np.array_equal(used.get_recon(), fresh.get_recon())
    used.pdhg_tv(Niter=2, precond=False)
    for a, b in zip(used.asd_pocs(Niter=2), fresh.asd_pocs(Niter=2)):
        assert np.allclose(a, b, rtol=1e-12, atol=0)
    assert np.array_equal(used.get_recon(), fresh.get_recon())
