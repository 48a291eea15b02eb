"""Chambolle-Pock on a volume split into slabs (``tomo_pdhg_slab_*``, k_pdhg_tv<.., SLAB>): 2 and 3 slab engines on ONE GPU through
``tests/local_ring.ThreadRing`` (the product's in-process world with every rank on the same device), against the whole-volume engine
bit for bit where the arithmetic is the same by construction, and against the binary64 yardsticks of tests/ref64.py / ref64_pdhg.py.

Slab sizes 1, 43, 44, 63, 64, 65 and 129 reach every branch of the slab pass: a slab with both neighbours in planes, an upper halo
plane that enters at lane 63 (64 slices) and at a lane in the middle of a partial chunk (63, 43, 1 slices), a lower halo plane under
chunk 0 with more chunks above it (65, 129).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import ref64
import ref64_pdhg as R
from conftest import rel_l2
from local_ring import ThreadRing
from test_gpu_pdhg import ANGLES, LOOP, P0, UVOL, X, XBAR, _tilt_series, dense_inputs, get_p, matrix, new_engine, put
from tomo_tv_amd import _lib, pytvlib
from tomo_tv_amd._lib import S_DIFF, S_L1, SINO_USER0, VOL_RECON, VOL_YK
from tomo_tv_amd.distributed import slab_partition
from tomo_tv_amd.engine import _ptr, tomoengine
from tomo_tv_amd.reconstructor import TomoGPU

pytestmark = pytest.mark.gpu
F32 = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
SLABS = {(2, 2): [1, 1], (3, 3): [1, 1, 1], (2, 127): [64, 63], (2, 129): [65, 64], (3, 130): [44, 43, 43], (2, 258): [129, 129]}
FIELDS = (X, XBAR, P0, P0 + 1, P0 + 2)


def sizes(world, nx):
    return [slab_partition(nx, world, r)[1] for r in range(world)]


def run_ring(world, nx, n, ang_deg, script, b=None):
    """Every rank builds its slab engine with the GLOBAL sizes and runs ``script(engine)``; rank 0's result."""
    ring = ThreadRing(world)

    def body(comm):
        t = tomoengine(nx, n, np.asarray(ang_deg) * np.pi / 180, device=0, comm=comm)
        assert (t.first, t.nloc) == slab_partition(nx, world, comm.rank)
        if b is not None:
            t.set_tilt_series(b)
        return script(t)
    return ring.run(body)[0]


def read_fields(t):
    return [t.get_volume(s) for s in FIELDS]


def l1_sums(t):
    out = []
    for s in FIELDS:
        t.be.c("l1_norm", s)
        out.append(t._scalar(S_L1))
    return out


def two_steps(t, inputs, lam, sharded):
    """Both step modes, two steps each: [(fields, S_DIFF, l1 sums)] * 2 per mode.  Sharded: one pack, an exchange before every step."""
    x, xbar, u, p = inputs
    out = {}
    for precond in (False, True):
        put(t, x=x, xbar=xbar, u=u, p=p)
        if sharded:
            t.pdhg_slab_pack(XBAR, P0)
        steps = []
        for _ in range(2):
            if sharded:
                t.pdhg_exchange()
            t.pdhg_tv_step(X, XBAR, UVOL, P0, sigma=0.3, tau=0.2, lam=lam, theta=1.0, precond=precond, slot=S_DIFF)
            steps.append((read_fields(t), t._scalar(S_DIFF), l1_sums(t)))
        out[precond] = steps
    return out


@pytest.mark.parametrize("n", [8, 33])
@pytest.mark.parametrize("world,nx", list(SLABS), ids=[f"w{w}-nx{nx}" for w, nx in SLABS])
def test_dense_steps_equal_the_whole_volume_bit_for_bit(gpu, world, nx, n):
    assert sizes(world, nx) == SLABS[(world, nx)]
    lam = 0.5
    inputs = dense_inputs(nx, n, lam, n * 100 + nx)
    over = np.sqrt(np.sum(inputs[3].astype(np.float64) ** 2, axis=0)) > lam
    assert 0.15 < over.mean() < 0.6
    want = two_steps(new_engine(n, nx), inputs, lam, False)
    got = run_ring(world, nx, n, ANGLES, lambda t: two_steps(t, inputs, lam, True))
    for precond in (False, True):
        for k, ((gf, gs, gl), (wf, ws, _)) in enumerate(zip(got[precond], want[precond])):
            for name, g, w in zip(("x", "xbar", "p0", "p1", "p2"), gf, wf):
                bad = np.argwhere(g != w)
                assert np.array_equal(g, w), (precond, k, name, len(bad), bad[:4].tolist())
            print(f"S_DIFF precond={int(precond)} step {k}: sharded {gs!r} whole {ws!r}")
            assert abs(gs - ws) <= 1e-12 * abs(ws)
            for name, g, v in zip(("x", "xbar", "p0", "p1", "p2"), gf, gl):     # padding slices were written as 0
                ref, bound = ref64.l1(g)
                ref64.assert_scalar(f"padding of {name}", v, ref, bound + ref64.TINY)
        assert (want[precond][0][0][0] == 0).any() and (want[precond][0][0][0] > 0).any()


@pytest.mark.parametrize("n", [8, 33])
@pytest.mark.parametrize("world,nx", [(2, 2), (2, 127), (3, 130)], ids=["w2-nx2", "w2-nx127", "w3-nx130"])
def test_exact_structure_across_an_interior_face(gpu, world, nx, n):
    c0 = SLABS[(world, nx)][0]                                               # rank 0 holds slices 0 .. c0 - 1
    shape = (nx, n, n)
    four, zero = np.full(shape, 4.0, F32), np.zeros(shape, F32)
    y, z = n // 2, n // 3

    def script(t):
        out = {}

        def step(lam, **fields):
            put(t, **fields)
            t.pdhg_slab_pack(XBAR, P0)
            t.pdhg_exchange()
            t.pdhg_tv_step(X, XBAR, UVOL, P0, sigma=0.5, tau=1.0, lam=lam, theta=1.0, precond=False)
            return t.get_volume(X), get_p(t)
        for s in (c0 - 1, c0):
            xbar = four.copy()
            xbar[s, y, z] = 5.0
            out["hot", s] = (xbar, step(2.0 ** 20, x=four, xbar=xbar, u=zero, p=np.zeros((3,) + shape, F32))[1])
        for s in (c0 - 1, nx - 1):
            p = np.zeros((3,) + shape, F32)
            p[0][s, y, z] = 1.0
            out["p", s] = (p,) + step(2.0, x=four, xbar=four, u=zero, p=p)
        return out
    got = run_ring(world, nx, n, ANGLES, script)
    for s in (c0 - 1, c0):
        xbar, p = got["hot", s]
        assert np.array_equal(p.astype(np.float64), 0.5 * R.grad(xbar)), s
    p, xn, pn = got["p", c0 - 1]                                             # an interior face is not the volume's end: kept
    assert np.array_equal(pn, p)
    assert np.array_equal(xn.astype(np.float64) - 4.0, R.div(p))
    assert xn[c0 - 1, y, z] == 5.0 and xn[c0, y, z] == 3.0
    p, xn, pn = got["p", nx - 1]                                             # the volume's last slice: read back as 0
    assert not pn.any() and np.array_equal(xn, four)


_REF = {}


def loop_reference(gid, precond, L):
    """The replays and the whole-volume engine's result, computed once per geometry and mode and left unchanged."""
    key = (gid, precond)
    if key not in _REF:
        ang, n, nx = LOOP[gid]
        M = matrix(n, ang)
        b = M.fp(R.block_phantom(nx, n)).astype(F32)
        f64 = R.pdhg(M, b, 20, 0.125, precond=precond, L=L)
        f32 = R.pdhg(M, b, 20, 0.125, precond=precond, L=L, dtype=F32)
        t = new_engine(n, nx, ang)
        t.set_tilt_series(b)
        t.restart_recon()
        t.pdhg_begin()
        t.pdhg(20, 0.125, precond=precond)
        _REF[key] = (b, f64["x"], ref64.seq_bound(f32["x"], f64["x"]), t.get_volume(VOL_RECON))
    return _REF[key]


def loop_script(precond, lam=0.125):
    def script(t):
        out = {"L": t.get_lipschitz()}
        t.restart_recon()
        t.pdhg_begin()
        t.pdhg(20, lam, precond=precond)
        out["x20"], out["xb20"] = t.get_volume(VOL_RECON), t.get_volume(VOL_YK)
        t.restart_recon()
        t.pdhg_begin()
        for _ in range(3):
            t.pdhg(5, lam, precond=precond)
        t.pdhg(4, lam, precond=precond)
        out["x19"] = t.get_volume(VOL_RECON)
        t.pdhg(1, lam, precond=precond, slot=S_DIFF)
        out["split"], out["split_xb"], out["sq"] = t.get_volume(VOL_RECON), t.get_volume(VOL_YK), t._scalar(S_DIFF)
        t.restart_recon()
        t.pdhg_begin()
        for _ in range(4):
            t.pdhg(5, lam, precond=precond)
        out["4x5"] = t.get_volume(VOL_RECON)
        # the driver's way in
        t.restart_recon()
        t.pdhg_begin()
        pytvlib.run(t, "pdhg", lam, 20, theta=1.0, precond=precond, ratio=1.0)
        out["driver"] = t.get_volume(VOL_RECON)
        return out
    return script


def _lipschitz(gid):
    ang, n, _ = LOOP[gid]
    return new_engine(n, 1, ang).get_lipschitz()


@pytest.mark.parametrize("gid,world", [("lin70", 2), ("lin70", 3), ("repeat", 3)], ids=["lin70-w2", "lin70-w3", "repeat-w3"])
@pytest.mark.parametrize("precond", [False, True], ids=["scalar", "diagonal"])
def test_loop_against_the_replays(gpu, gid, world, precond):
    ang, n, nx = LOOP[gid]
    b, f64x, bound, whole = loop_reference(gid, precond, _lipschitz(gid))
    got = run_ring(world, nx, n, ang, loop_script(precond), b=b)
    assert got["L"] == _lipschitz(gid)                                       # the 2-D matrix only: every rank derives the same steps
    print(f"ratio sharded pdhg loop {gid} world={world} precond={int(precond)}: {ref64.ratio(got['x20'], f64x, bound):.3f}"
          f"   rel-L2 to the whole-volume engine: {rel_l2(got['x20'], whole):.3e}")
    ref64.assert_within(f"sharded pdhg x {gid} world={world}", got["x20"], f64x, bound)
    assert np.max(np.abs(f64x)) > 0.05
    assert np.array_equal(got["split"], got["x20"]) and np.array_equal(got["split_xb"], got["xb20"])
    assert np.array_equal(got["4x5"], got["x20"])
    sq, sqb = ref64.sqdiff(got["x20"], got["x19"])
    ref64.assert_scalar("sum (x_new - x)^2", got["sq"], sq, sqb)
    assert np.array_equal(got["driver"], got["x20"])                          # pytvlib.run(t, "pdhg", ...) is the engine call


def test_sino_dual_on_a_slab_equals_the_whole_volume_call(gpu):
    n, nx, world = 8, 65, 3
    M = matrix(n)
    q, g, b = (ref64.signed_sino(nx, M.nrow, s + nx) for s in (1, 2, 3))
    QS, GS, BS = SINO_USER0, SINO_USER0 + 1, SINO_USER0 + 2

    def script(t):
        out = {}
        for precond in (False, True):
            for slot, v in ((QS, q), (GS, g), (BS, b)):
                t.be.c("set_sinogram", slot, _ptr(np.ascontiguousarray(v[t.first:t.first + t.nloc])))
            t.pdhg_sino_dual(QS, GS, BS, sigma=0.07, precond=precond)
            out[precond] = t._sino(QS)
        return out
    want = script(new_engine(n, nx))
    got = run_ring(world, nx, n, ANGLES, script)
    for precond in (False, True):
        assert np.array_equal(got[precond], want[precond]) and want[precond].any()


def test_refusals_and_the_whole_volume_slab(gpu):
    n, nx = 8, 5
    L = _lib.load()
    t = new_engine(n, nx)
    h = t.be.h
    ok = (X, XBAR, UVOL, P0, 0.1, 0.1, 0.1, 1.0, 0, -1)
    assert L.tomo_pdhg_slab_iter(h, 0.1, 1.0, 1, 1.0, -1) == 3               # before tomo_pdhg_slab_begin
    assert L.tomo_comm_pdhg(h, 1, 0.1, 1.0, 1, 1.0, -1) == 3 and b"communicator" in L.tomo_last_error()
    assert L.tomo_comm_pdhg_exchange(h) == 3 and b"communicator" in L.tomo_last_error()
    assert L.tomo_set_slab_edges(h, 0, 1) == 0
    assert L.tomo_pdhg_slab_tv_step(h, *ok) == 3 and b"tomo_bind_pdhg_halo" in L.tomo_last_error()
    assert L.tomo_set_slab_edges(h, 1, 1) == 0
    for args in ((X, X, UVOL, P0, 0.1, 0.1, 0.1, 1.0, 0, -1), (X, XBAR, UVOL, P0 - 1, 0.1, 0.1, 0.1, 1.0, 0, -1),
                 (X, XBAR, UVOL, 43, 0.1, 0.1, 0.1, 1.0, 0, -1), (X, XBAR, UVOL, P0, 0.1, 0.1, 0.0, 1.0, 1, -1),
                 (X, XBAR, UVOL, P0, 0.0, 0.1, 0.1, 1.0, 0, -1), (X, XBAR, UVOL, P0, 0.1, -1.0, 0.1, 1.0, 0, -1)):
        assert L.tomo_pdhg_slab_tv_step(h, *args) == 1, args
    # a slab that is both first and last needs no planes and gives the bits of tomo_pdhg_tv_step
    inputs = dense_inputs(nx, n, 0.5, 7)
    res = []
    for fn in (L.tomo_pdhg_tv_step, L.tomo_pdhg_slab_tv_step):
        put(t, x=inputs[0], xbar=inputs[1], u=inputs[2], p=inputs[3])
        assert fn(h, X, XBAR, UVOL, P0, 0.3, 0.2, 0.5, 1.0, 1, S_DIFF) == 0
        res.append(read_fields(t) + [t._scalar(S_DIFF)])
    assert all(np.array_equal(a, b) for a, b in zip(*res))


def test_native_whole_call_on_one_rank(gpu):
    """tomo_comm_pdhg on a one-rank RCCL communicator (self-sends) in a fresh child process: the bits of tomo_pdhg."""
    p = subprocess.run([sys.executable, os.path.join(HERE, "nccl_world1_pdhg_script.py")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "NCCL_WORLD1_PDHG_OK" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]


@pytest.mark.parametrize("precond", [False, True], ids=["scalar", "diagonal"])
def test_two_devices_through_the_facade(gpu, precond):
    """TomoGPU.pdhg_tv on the in-process multi-GPU facade: activates by itself on a box with >= 2 GPUs."""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    gid = "lin70"
    ang, n, nx = LOOP[gid]
    _, f64x, bound, whole = loop_reference(gid, precond, _lipschitz(gid))
    _, ts = _tilt_series(matrix(n, ang), nx)
    g = TomoGPU(ang, ts)
    assert g.tomo.is_multi_gpu_enabled()
    g.pdhg_tv(Niter=20, lambda_param=0.125, precond=precond, show_convergence=False)
    x = g.tomo.get_volume(VOL_RECON)
    print(f"ratio facade pdhg_tv precond={int(precond)}: {ref64.ratio(x, f64x, bound):.3f}   rel-L2 to one engine: {rel_l2(x, whole):.3e}")
    ref64.assert_within("facade pdhg_tv", x, f64x, bound)
