"""Call sequences on one engine: a used engine must give a fresh engine's bits (tables: tests/sequences.py).

(a) used equals fresh: every disturber x every probe; the fresh side is computed once per probe and geometry and anchored against the
    binary64 replays with the bounds of the element-wise / parity tests of that operation.
(b) old_is_recon (the state after tomo_fista_momentum: RECON_OLD's buffer is stale) under the newer readers and writers.
(c) the projection claim under every newer writer: data_distance -> writer -> SIRT step, fp_reuse = 1 against 0 and against a fresh
    engine that is given the written volume; the FISTA analogue with the projection formed by linearity.
(d) the newer reduction users while a deferred TV read, a scalar snapshot or an asynchronous data distance is pending
    (contract: include/tomo_hip.h, after tomo_scalars_snapshot_read).
(e) the staging buffer across types and sizes, al_part / al_out across a change of the angle count, the registry's byte count.
"""
import ctypes

import numpy as np
import pytest

import oracle
import ref64
import ref64_bin
import ref64_dart
import ref64_dual
import ref64_pdhg
import sequences as S
from conftest import rel_l2
from tomo_tv_amd import _lib
from tomo_tv_amd._lib import (S_DD, S_DIFF, SINO_B, SINO_G, SINO_PUBLIC, SINO_USER0, VOL_RECON, VOL_RECON_OLD, VOL_TEMP, VOL_USER0,
                              VOL_YK, check)
from tomo_tv_amd.engine import _ptr, fbp_filter_taps, tomoengine

pytestmark = pytest.mark.gpu
F32 = np.float32
RTOL = 1e-12                       # double sums that the workgroups add atomically (test_gpu_pdhg: test_other_drivers_are_left_alone)
TOL = 1e-5                         # the parity tests' relative L2 against a replay (test_gpu_parity.TOL)
_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def matrix(gid, ang=None):
    g = S.GEOM[gid]
    ang = g["ang"] if ang is None else ang
    return cached(("M", g["n"], tuple(ang)), lambda: ref64.Matrix(g["n"], ang))


def series(gid, ang=None):
    g = S.GEOM[gid]
    return cached(("b", gid, None if ang is None else tuple(ang)), lambda: matrix(gid, ang).fp(S.phantom(g["nx"], g["n"])).astype(F32))


def engine(gid):
    e = S.new_engine(gid)
    e.set_tilt_series(series(gid))
    return e


def fresh(gid, probe):
    def run():
        e = engine(gid)
        e.restart_recon()
        return S.PROBES[probe](e, gid)
    return cached(("fresh", gid, probe), run)


def same(name, got, want):
    assert got.keys() == want.keys()
    for k in want:
        if k.startswith("s_"):
            assert np.allclose(got[k], want[k], rtol=RTOL, atol=0), (name, k, got[k], want[k])
        else:
            assert np.array_equal(got[k], want[k]), (name, k, rel_l2(got[k], want[k]))


# ---- (a) ---------------------------------------------------------------------------------------------------------------------------------
PAIRS = S.pairs()


@pytest.mark.parametrize("gid,disturber,probe", PAIRS, ids=[f"{g}-{d}-{p}" for g, d, p in PAIRS])
def test_used_equals_fresh(gpu, gid, disturber, probe):
    want = fresh(gid, probe)
    e = engine(gid)
    wrote_b = S.DISTURBERS[disturber](e, gid, series(gid))
    S.restore_inputs(e, series(gid), wrote_b)
    same(f"{disturber} -> {probe}", S.PROBES[probe](e, gid), want)


def _slices(gid):
    nx = S.GEOM[gid]["nx"]
    return np.arange(nx) if nx <= 32 else np.array([0, 63, 64, nx - 1])


def _oracle(M, b, x=None):
    orc = oracle.ctvlib(len(b), M.N, M.P)
    orc.A = oracle.CSR(M.nrow, M.ncol, *M.csr())
    orc.set_tilt_series(b)
    if x is not None:
        orc.recon[:] = x
    return orc


def _kaczmarz(M, b, beta, order):
    """tomo_art_order in binary64: the sweep of ref64.Matrix.art over the rows in ``order``."""
    x = np.zeros((len(b), M.ncol))
    o, p, _ = M._r
    for j in order:
        if M.rowinner[j] > 0:
            en = o[p[j]:p[j + 1]]
            c, w = M.cols[en], M.vals[en]
            x[:, c] += float(F32(beta)) * ((b[:, j] - x[:, c] @ w) / M.rowinner[j])[:, None] * w[None, :]
    return np.maximum(x, 0.0).reshape(len(b), M.N, M.N)


def _anchor_sirt(o, M, b, sl):
    """The volumes on the slices ``sl`` (slices are independent).  S_DD and G need every slice of the replay, so they are anchored
    where ``sl`` is the whole slab (geometries A and C); at B the list projector's FP_DD sum and G are anchored by the
    data_distance probe, which replays all 128 slices."""
    z = np.zeros_like(o["x1"][sl])
    ref64.assert_within("SIRT 1", o["x1"][sl], *M.tomo_sirt_step(z, b[sl]))
    ref64.assert_within("SIRT 2", o["x2"][sl], *M.tomo_sirt_step(o["x1"][sl], b[sl]))
    if len(sl) == len(b):
        for x, dd in ((o["x1"], o["s_dd1"]), (o["x2"], o["s_dd2"])):
            y, ey, s, sb = M.data_distance(x, b)
            ref64.assert_scalar("S_DD", dd[0] ** 2, s, sb + 1e-15 * s)
        ref64.assert_within("G", o["g"], y, ey)


def _anchor_cgls(o, M, b, sl):
    x1, bound, _, _ = M.cgls_first_step(b[sl])
    ref64.assert_within("CGLS from zero", o["x1"][sl], x1, bound)
    orc = _oracle(M, b[sl])

    def fp(v):
        orc.recon[:] = v
        orc.forward_projection()
        return orc.g.copy()
    x32 = ref64.cgls_f32(fp, orc.back_projection, o["x1"][sl], b[sl], 1)
    ref64.assert_seq("CGLS restart", o["x2"][sl], x32, M.cgls(o["x1"][sl], b[sl], 1)[0])


def _anchor_sart(o, M, b, sl):
    x0 = np.zeros_like(o["x1"][sl])
    for x_in, got in ((x0, o["x1"][sl]), (o["x1"][sl], o["x2"][sl])):
        orc = _oracle(M, b[sl], x_in)
        orc.SART(0.7, 1)
        ref64.assert_seq("SART", got, orc.recon, M.sart(x_in, b[sl], 0.7))


def _anchor_art(o, M, b, sl):
    orc = _oracle(M, b[sl], np.zeros_like(o["x1"][sl]))
    orc.row_inner_product()
    orc.ART(0.6)
    ref64.assert_seq("ART", o["x1"][sl], orc.recon, M.art(np.zeros_like(o["x1"][sl]), b[sl], 0.6))


def _anchor_art_random(o, M, b, sl):
    assert rel_l2(o["x1"][sl], _kaczmarz(M, b[sl].astype(np.float64), 0.6, S.art_order(M.nrow))) < TOL


def _anchor_fista(o, M, b, sl):
    z = np.zeros(o["recon0"].shape)
    recon, old, yk, t0 = z, z, z, 1.0
    assert [bool(o[f"done{k}"][0]) for k in range(3)] == [True, True, True]     # beta = 0 first, then by linearity twice
    for k in range(3):
        step = M.tomo_sirt_step(yk, b)[0]
        r = ref64.tv_fgp(step, S.FISTA_TV, S.FISTA_LAM)
        tk = 0.5 * (1 + np.sqrt(1 + 4 * t0 ** 2))
        yk, old, recon, t0 = ref64.momentum(r, recon, (t0 - 1) / tk)[0], r, r, tk
        assert rel_l2(o[f"step{k}"], step) < 2e-5 and rel_l2(o[f"recon{k}"], recon) < 2e-5 and rel_l2(o[f"yk{k}"], yk) < 2e-5, k
        assert np.array_equal(o[f"old{k}"], o[f"recon{k}"])                     # recon_old == recon after every Nesterov step
        cost = 0.5 * M.data_distance(recon, b)[2] + S.FISTA_LAM * ref64.tv_value(recon, 1e-6)[0]
        assert abs(o["s_cost"][k] - cost) <= 1e-4 * cost, (k, o["s_cost"][k], cost)


def _anchor_asd(o, M, b, sl):
    x, beta, norm = np.zeros(o["x"].shape), 0.25, float(b.size)
    for i in range(2):
        temp = x
        x = M.sart(x, b, beta)
        dp = np.sqrt(np.sum((x - temp) ** 2))
        dPOCS = dp * 0.2 if i == 0 else dPOCS
        beta *= 0.9985
        dd = np.sqrt(M.data_distance(x, b)[2]) / norm
        tv0 = ref64.tv_value(x, 1e-6)[0]
        sart = x
        x = ref64.tv_gd(x, 3, dPOCS, 1e-6)
        dg = np.sqrt(np.sum((x - sart) ** 2))
        assert abs(o["s_dd"][i] - dd) <= 1e-5 * dd and abs(o["s_tv"][i] - tv0) <= 1e-5 * tv0, (i, o["s_dd"][i], dd, o["s_tv"][i], tv0)
        if dg > dp * 0.95 and dd > 0.025:
            dPOCS *= 0.95
    assert rel_l2(o["x"], x) < TOL and np.array_equal(o["temp"], o["x"])


def _anchor_fgp(o, M, b, sl):
    for x_in, got, tv in ((o["x0"], o["x1"], o["s_tv1"]), (o["x1"], o["x2"], o["s_tv2"])):
        orc = oracle.ctvlib(len(x_in), M.N, 1)
        orc.recon[:] = x_in
        orc.tv_fgp(3, 0.02)
        ref64.assert_seq("FGP", got, orc.recon, ref64.tv_fgp(x_in, 3, 0.02))
        ref64.assert_scalar("S_TV", tv[0], *ref64.tv_value(x_in, 1e-6))


def _anchor_pdhg(o, M, b, sl):
    f64, f32 = ref64_pdhg.pdhg(M, b, 2, 0.125), ref64_pdhg.pdhg(M, b, 2, 0.125, dtype=F32)
    ref64.assert_within("pdhg x", o["x"], f64["x"], ref64.seq_bound(f32["x"], f64["x"]))
    ref64.assert_within("pdhg xbar", o["xbar"], f64["xbar"], ref64.seq_bound(f32["xbar"], f64["xbar"]))
    assert abs(o["s_diff"][0] - f64["sqdiff"]) <= 1e-4 * f64["sqdiff"]


def _anchor_wbp(o, M, b, sl):
    f, _ = ref64.filter_rows(b[sl], fbp_filter_taps(M.N, "ram-lak"), M.P, M.N)
    want = np.maximum(float(F32(np.pi / M.P)) * M.bp(f), 0.0)
    assert rel_l2(o["x"][sl], want) < 2e-5                     # the bound of the parity tests of the WBP


def _anchor_poisson(o, M, b, sl):
    x0 = o["x0"][sl]
    r, _, cost, cb = M.poisson(x0, b[sl])
    want = np.maximum(x0 - (0.1 / M.lipschitz()[0]) * M.bp(r), 0.0)
    assert rel_l2(o["x1"][sl], want) < TOL
    if len(sl) == len(b):
        ref64.assert_scalar("S_COST", o["s_cost"][0], cost, cb)


def _anchor_dd(o, M, b, sl):
    y, ey, s, sb = M.data_distance(o["x0"], b)
    ref64.assert_within("G", o["g"], y, ey)
    ref64.assert_scalar("S_DD", o["s_dd"][0] ** 2, s, sb + 1e-15 * s)


ANCHORS = {"sirt": _anchor_sirt, "cgls": _anchor_cgls, "sart_resident": _anchor_sart, "sart_tile": _anchor_sart, "sart_angle": _anchor_sart,
           "art": _anchor_art, "art_random": _anchor_art_random, "fista": _anchor_fista, "asd_pocs": _anchor_asd, "tv_fgp": _anchor_fgp,
           "pdhg": _anchor_pdhg, "wbp": _anchor_wbp, "poisson_ml": _anchor_poisson, "data_distance": _anchor_dd}
FRESH = sorted({(g, p) for g, _, p in PAIRS})


@pytest.mark.parametrize("gid,probe", FRESH, ids=[f"{g}-{p}" for g, p in FRESH])
def test_fresh_side_against_binary64(gpu, gid, probe):
    """The fresh side of (a) is the right answer, not only a repeatable one -- and repeatable it is: a second fresh engine, same bits."""
    o = fresh(gid, probe)
    e = engine(gid)
    e.restart_recon()
    same(f"fresh twice {probe}", S.PROBES[probe](e, gid), o)
    ANCHORS[probe](o, matrix(gid), series(gid), _slices(gid))


@pytest.mark.parametrize("gid", ["A", "C"])
def test_small_grid_sums_have_the_same_bits_on_every_engine(gpu, gid):
    """The data distance at these sizes: every wave of the producing launch adds into a partial-sum slot of its own (at most 256
    waves), so no order of atomic additions enters the value -- the drivers' cost vectors of two engines compare bit for bit
    (test_gpu_bin compares coarse_to_fine's that way)."""
    out = []
    for _ in range(4):
        e = engine(gid)
        e.restart_recon()
        dd = []
        for _ in range(3):
            e.SIRT(1)
            dd.append(e.data_distance())
        out.append(dd)
    assert out[0] == out[1] == out[2] == out[3], out
    _, _, s, sb = matrix(gid).data_distance(e.get_volume(), series(gid))
    ref64.assert_scalar("S_DD", out[0][-1] ** 2, s, sb + 1e-15 * s)


# ---- (b) ---------------------------------------------------------------------------------------------------------------------------------
SENTINEL = F32(7777.0)


def grid_volume(n, seed):
    """Values on a 2^-8 grid in [0, 2.5): sums, means and a * x with a = 1/2 are exact in binary32."""
    return (np.random.default_rng(seed).integers(0, 640, (n, n, n)) / 256.0).astype(F32)


def stale_old(gid="C"):
    """-> (engine, y): RECON and (logically) RECON_OLD hold y, RECON_OLD's own buffer holds the sentinel."""
    n = S.GEOM[gid]["n"]
    e, y = engine(gid), grid_volume(n, 1)
    e.set_volume(grid_volume(n, 2))
    e.initialize_fista()
    e.set_volume(y, VOL_YK)
    e.set_volume(np.full((n, n, n), SENTINEL), VOL_RECON_OLD)          # a real write: the buffer now holds the pattern
    e.fista_momentum(0.5)
    e.remove_momentum()
    return e, y


def both(e, recon, old):
    for vol, want in ((VOL_RECON, recon), (VOL_RECON_OLD, old)):
        got = e.get_volume(vol)
        assert not (got == SENTINEL).any(), vol
        if want is not None:
            assert np.array_equal(got, want), vol


def test_stale_recon_old_readers(gpu):
    e, y = stale_old()
    import torch
    assert np.array_equal(e.get_volume_tensor(VOL_RECON_OLD, dtype=torch.float64).cpu().numpy(), y.astype(np.float64))
    n_free, n_bnd = e.dart_classify(S.THR, vol=VOL_RECON_OLD, connectivity=26, seed=3, free_fraction=0.25)
    st = ref64_dart.state(y, S.THR, 26, 3, ref64_dart.free_threshold(0.25))
    assert np.array_equal(e.dart_state(), st) and n_bnd == int(((st & _lib.DART_BOUNDARY) != 0).sum()) and n_free == int(((st & _lib.DART_FREE) != 0).sum())
    assert np.array_equal(e.dart_class_stats(S.THR, vol=VOL_RECON_OLD), ref64_dart.class_stats(y, S.THR))
    coarse = e.binned_engine(2)
    e.bin_volume_to(coarse, 2, src=VOL_RECON_OLD)
    assert np.array_equal(coarse.get_volume(), ref64_bin.bin_replay_f32(y, 2, volume=True))
    other = S.new_engine("C")
    e.cross_volume_to(other, src=VOL_RECON_OLD)
    assert np.array_equal(other.get_volume(), ref64_dual.cross(y))
    d = other.get_volume()
    e.cross_axpy_volume_to(other, 0.5, src=VOL_RECON_OLD)
    assert np.array_equal(other.get_volume().astype(np.float64), ref64_dual.cross_axpy(y, d, 0.5))
    check(e.be.L.tomo_copy_volume_from(other.be.h, VOL_USER0, e.be.h, VOL_RECON_OLD))
    assert np.array_equal(other.get_volume(VOL_USER0), y)
    both(e, y, y)


WRITES = ["smooth_into_recon", "smooth_into_old", "prolong_into_recon", "prolong_into_old", "cross_into_recon", "cross_into_old",
          "axpy_into_recon", "axpy_into_old", "copy_from_into_recon", "copy_from_into_old"]


@pytest.mark.parametrize("case", WRITES)
def test_stale_recon_old_writers(gpu, case):
    """After a write to RECON, RECON_OLD holds what RECON held before; after a write to RECON_OLD, RECON is untouched."""
    e, y = stale_old()
    n = y.shape[0]
    dst = VOL_RECON if case.endswith("recon") else VOL_RECON_OLD
    src = VOL_RECON_OLD if dst == VOL_RECON else VOL_RECON
    z = grid_volume(n, 5)
    if case.startswith("smooth"):
        e.dart_classify(S.THR, vol=VOL_RECON_OLD, connectivity=26, seed=3, free_fraction=0.25)
        st = ref64_dart.state(y, S.THR, 26, 3, ref64_dart.free_threshold(0.25))
        e.dart_smooth(src, dst, 0.5)
        ref, bound, fr = ref64_dart.smooth(y, st, 0.5)
        got = e.get_volume(dst)
        ref64.assert_within("smooth", got, ref, bound)
        assert fr.any() and np.array_equal(got[~fr], y[~fr])
        new = got
    elif case.startswith("prolong"):
        coarse = e.binned_engine(2)
        c = grid_volume(n, 6)[:n // 2, :n // 2, :n // 2]
        coarse.set_volume(c)
        coarse.prolong_volume_to(e, 2, dst=dst)
        new = ref64_bin.prolong_replay_f32(c, 2, n)
    elif case.startswith("copy_from"):
        other = S.new_engine("C")
        other.set_volume(z, VOL_USER0 + 1)
        check(e.be.L.tomo_copy_volume_from(e.be.h, dst, other.be.h, VOL_USER0 + 1))
        new = z
    else:
        other = S.new_engine("C")
        other.set_volume(z)
        if case.startswith("cross"):
            other.cross_volume_to(e, dst=dst)
            new = ref64_dual.cross(z)
        else:
            other.cross_axpy_volume_to(e, 0.5, dst=dst)
            new = ref64_dual.cross_axpy(z, y, 0.5).astype(F32)
            assert np.array_equal(new.astype(np.float64), ref64_dual.cross_axpy(z, y, 0.5))     # exact on the grid
    both(e, new if dst == VOL_RECON else y, y if dst == VOL_RECON else new)


# ---- (c) ---------------------------------------------------------------------------------------------------------------------------------
def _partner(e, kind):
    g = S.GEOM["C"]
    if kind == "fine":
        t = tomoengine(2 * g["nx"], 2 * g["n"], g["ang"] * np.pi / 180)
        t.set_volume(S.user_volume(2 * g["nx"], 2 * g["n"], 50))
        t.be.c("forward_projection", VOL_RECON, SINO_B)
    else:
        t = S.new_engine("C")
        t.set_volume(S.user_volume(g["nx"], g["n"], 51))
    return t


def w_dart_restore(e):
    e.dart_classify(S.THR, connectivity=26, seed=1, free_fraction=0.3)
    e.data_distance()
    e.dart_restore(S.GREYS)


def w_dart_segment(e):
    e.dart_classify(S.THR, connectivity=6)
    e.data_distance()
    e.dart_restore(S.GREYS, everywhere=True)


def w_dart_arm(e):
    e.dart_classify(S.THR, connectivity=26, seed=1, free_fraction=0.3)
    e.data_distance()
    e.dart_arm(1, S.GREYS)


def w_dart_smooth(e):
    e.copy_recon()
    e.dart_classify(S.THR, connectivity=26, seed=1, free_fraction=0.3)
    e.data_distance()
    e.dart_smooth(VOL_TEMP, VOL_RECON, 0.4)


def w_bin(e):
    _partner(e, "fine").bin_volume_to(e, 2)


def w_cross(e):
    _partner(e, "cube").cross_volume_to(e)


def w_axpy(e):
    _partner(e, "cube").cross_axpy_volume_to(e, 0.25, clamp=True)


def w_mm_update(e):
    he = _partner(e, "cube")
    e.be.share_stream_with(he.be)
    he.set_volume(S.user_volume(e.Nslice_, e.Ny, 52), VOL_USER0)
    e.set_volume(S.user_volume(e.Nslice_, e.Ny, 53), VOL_USER0 + 2)
    e.data_distance()
    xv, uv, w = np.array([VOL_RECON], np.int32), np.array([VOL_USER0 + 2], np.int32), np.array([0.9], F32)
    e.be.mm_update(xv, uv, w, 1.5, 0.01, 0.1, he.be, VOL_RECON, VOL_USER0)
    e.synchronize()
    he.be.close()


def w_pdhg(e):
    e.pdhg_begin()
    e.data_distance()
    e.pdhg(1, 0.125)


def w_set_slice(e):
    e.set_recon(S.user_volume(1, e.Ny, 54)[0], 3)


def w_sino(kind):
    def write(e):
        if kind == "shift":
            e.sino_shift(SINO_B, SINO_G, S.shifts_for(e.Nproj))
        elif kind == "affine":
            e.sino_affine(SINO_B, SINO_G, S.affine_for(e.Nproj, e.Ny, e.Nslice_))
        elif kind == "bin":
            _partner(e, "fine").bin_sinogram_to(e, 2, dst=SINO_G)
        else:
            import torch
            t = torch.full((e.Nslice_, e.Ny, e.Nproj), 3.0, dtype=torch.float64, device=torch.device("cuda", e.gpuID))
            e.be.set_tilt_series_tensor(t, SINO_PUBLIC, which=SINO_G)
            torch.cuda.synchronize()
    return write


WRITERS = {"tomo_dart_restore": w_dart_restore, "tomo_dart_segment": w_dart_segment, "tomo_dart_arm": w_dart_arm,
           "tomo_dart_smooth": w_dart_smooth, "tomo_volume_bin": w_bin, "tomo_volume_cross": w_cross, "tomo_volume_cross_axpy": w_axpy,
           "tomo_mm_update": w_mm_update, "tomo_pdhg": w_pdhg, "tomo_set_slice": w_set_slice, "tomo_sino_shift": w_sino("shift"),
           "tomo_sino_affine": w_sino("affine"), "tomo_sino_bin": w_sino("bin"), "tomo_set_sinogram_device": w_sino("device")}


def _claim_run(writer, reuse):
    e = engine("C")
    e.set_option("fp_reuse", reuse)
    e.restart_recon()
    e.SIRT(2)
    e.data_distance()                                           # the claim: G = A * RECON
    writer(e)
    v = e.get_volume()
    e.SIRT(1)
    return v, e.get_volume()


@pytest.mark.parametrize("name", list(WRITERS))
def test_claim_is_dropped_by_every_writer(gpu, name):
    v1, x1 = _claim_run(WRITERS[name], 1)
    v0, x0 = _claim_run(WRITERS[name], 0)
    assert np.array_equal(v1, v0) and np.array_equal(x1, x0)
    f = engine("C")
    f.set_volume(v1)
    f.SIRT(1)
    assert np.array_equal(x1, f.get_volume())
    ref64.assert_within("the step of the written volume", x1, *matrix("C").tomo_sirt_step(v1, series("C")))


def test_claim_is_dropped_by_a_new_geometry(gpu):
    ang13 = np.linspace(-65, 65, 13)
    b13 = series("C", ang13)
    out = []
    for reuse in (1, 0):
        e = engine("C")
        e.set_option("fp_reuse", reuse)
        e.restart_recon()
        e.SIRT(2)
        e.data_distance()
        v = e.get_volume()
        e.update_projection_angles(ang13 * np.pi / 180)         # tomo_adopt_volumes
        e.set_tilt_series(b13)
        e.SIRT(1)
        out.append((v, e.get_volume()))
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    f = S.new_engine("C", ang=ang13)
    f.set_tilt_series(b13)
    f.set_volume(out[0][0])
    f.SIRT(1)
    assert np.array_equal(out[0][1], f.get_volume())


def test_a_refused_fgp_end_leaves_the_engine_as_it_was(gpu):
    """tomo_fgp_end / tomo_fgp_fused_end without a begin are refused (the state error) before they touch the engine: after the cost
    evaluation of the reconstruction and the refused calls, the SIRT step gives the bits of an engine that never made them."""
    N, P, Nx = 16, 5, 3
    ang = np.linspace(-70, 70, P)
    b = ref64.Matrix(N, ang).fp(S.phantom(Nx, N)).astype(F32)
    out = []
    for refused in (True, False):
        e = S.new_engine("A", nx=Nx, n=N, ang=ang)
        e.set_tilt_series(b)
        e.restart_recon()
        e.SIRT(2)
        dd = e.data_distance()                                  # the claim: G = A * RECON
        for call, args in S.REFUSED_WITHOUT_BEGIN.items() if refused else ():
            with pytest.raises(_lib.TomoError, match="error 3: .*begin has not been called"):      # TOMO_ERR_STATE
                e.be.c(call, *args)
        e.SIRT(1)
        out.append((dd, e.get_volume(), e.data_distance(), e.get_model_projections()))
    assert out[0][0] > 0 and np.abs(out[0][1]).max() > 0
    assert np.allclose([out[0][0], out[0][2]], [out[1][0], out[1][2]], rtol=RTOL, atol=0)
    assert np.array_equal(out[0][1], out[1][1]) and np.array_equal(out[0][3], out[1][3])


def _fista_run(writer, reuse):
    e = engine("C")
    e.set_option("fp_reuse", reuse)
    e.restart_recon()
    e.initialize_fista()
    e.SIRT(1)
    e.fista_momentum(0.0)
    e.data_distance()
    e.fista_project_yk()
    e.SIRT(1)
    e.fista_momentum(0.3)
    e.data_distance()
    done = e.fista_project_yk()
    assert done == bool(reuse)                                   # with fp_reuse the projection by linearity is in hand
    writer(e)
    v = e.get_volume(VOL_YK)
    e.SIRT(1)                                                    # on YK
    return v, e.get_volume(VOL_YK)


FISTA_WRITERS = {"set_yk": lambda e: e.set_volume(S.user_volume(e.Nslice_, e.Ny, 60), VOL_YK),
                 "fgp_on_yk": lambda e: e.tv_fgp(2, 0.01, vol=VOL_YK),
                 "scale_yk": lambda e: e.be.c("scale_volume", VOL_YK, 0.5),
                 "set_recon_slice": lambda e: e.set_recon(S.user_volume(1, e.Ny, 61)[0], 2),
                 "cross_into_recon": w_cross}


@pytest.mark.parametrize("name", list(FISTA_WRITERS))
def test_projection_by_linearity_is_dropped_by_a_writer(gpu, name):
    v1, y1 = _fista_run(FISTA_WRITERS[name], 1)
    v0, y0 = _fista_run(FISTA_WRITERS[name], 0)
    assert np.array_equal(v1, v0) and np.array_equal(y1, y0)
    ref64.assert_within("the step of the written yk", y1, *matrix("C").tomo_sirt_step(v1, series("C")))


# ---- (d) ---------------------------------------------------------------------------------------------------------------------------------
def _begin(e, kind):
    e.restart_recon()
    e.SIRT(2)
    e.copy_recon()
    if kind == "tv_deferred":
        return e.tv_gd_tracked(3, 0.05, defer=True)
    if kind == "snapshot":
        e.data_distance()
        e.be.scalars_snapshot()
        return lambda: e.be.scalars_snapshot_read()
    e.data_distance_begin()
    return lambda: (e.data_distance_end(),)


REDUCERS = {"tomo_dart_classify": lambda e: (np.array(e.dart_classify(S.THR, connectivity=26, seed=4, free_fraction=0.2)), e.dart_state()),
            "tomo_dart_class_stats": lambda e: (e.dart_class_stats(S.THR),),
            "tomo_sino_moments": lambda e: (e.sino_moments(SINO_B), e.sino_moments(SINO_G)),
            "tomo_sino_xcorr": lambda e: (e.sino_xcorr(SINO_B, SINO_G, 3),),
            "tomo_sino_axis_profile": lambda e: (e.sino_axis_profile(SINO_G),)}


@pytest.mark.parametrize("reducer", list(REDUCERS))
@pytest.mark.parametrize("kind", ["tv_deferred", "snapshot", "dd_begin"])
def test_reduction_users_while_work_is_pending(gpu, kind, reducer):
    """Neither side refuses; both deliver what the un-interleaved order delivers, and the engine goes on as a fresh one would."""
    a, b = engine("A"), engine("A")
    finish = _begin(a, kind)
    red_a = REDUCERS[reducer](a)                                 # while the item is pending
    pend_a = finish()
    finish = _begin(b, kind)
    pend_b = finish()                                            # the un-interleaved order
    red_b = REDUCERS[reducer](b)
    assert np.allclose(np.asarray(pend_a, np.float64), np.asarray(pend_b, np.float64), rtol=RTOL, atol=0), (pend_a, pend_b)
    for x, y in zip(red_a, red_b):
        assert np.array_equal(x, y)
    for e in (a, b):
        e.SIRT(1)
    assert np.array_equal(a.get_volume(), b.get_volume()) and np.array_equal(a.get_volume(VOL_TEMP), b.get_volume(VOL_TEMP))
    ref = ref64_dart.class_stats(b.get_volume(), S.THR)          # ... and the reducers' answers are the replay's, not only each other's
    assert np.array_equal(b.dart_class_stats(S.THR)[:, 1], ref[:, 1])


# ---- (e) ---------------------------------------------------------------------------------------------------------------------------------
def _prep(e, gid="A"):
    """The inputs of every stage step, set through the device calls (which neither allocate nor use the staging buffer)."""
    import torch
    dev = torch.device("cuda", e.gpuID)
    g = S.GEOM[gid]
    e.set_volume_tensor(torch.from_numpy(S.phantom(g["nx"], g["n"]) + S.user_volume(g["nx"], g["n"], 70) * F32(0.25)).to(dev))
    e.be.set_tilt_series_tensor(torch.from_numpy(series(gid)).to(dev))
    e.dart_classify(S.THR, connectivity=26, seed=9, free_fraction=0.2)
    torch.cuda.synchronize()


def _vol(e):
    return e.get_volume_tensor().cpu().numpy()


def _sino(e, which):
    return e.get_projections_tensor(which).cpu().numpy()


def _proj(e):
    mx = np.empty(e.Nproj, F32)
    e.be.c("sino_proj_max", SINO_B, _ptr(mx))
    e.be.c("sino_proj_scale", SINO_B, _ptr(mx), _ptr(np.linspace(1, 2, e.Nproj).astype(F32)))
    return mx, _sino(e, SINO_B)


STAGE_STEPS = [                                                  # (name, bytes of stage it needs at geometry A, the call)
    ("set_recon", 4096, lambda e: (e.set_recon(S.user_volume(1, e.Ny, 71)[0], 4), _vol(e))[1]),
    ("sino_affine", 432, lambda e: (e.sino_affine(SINO_B, SINO_USER0, S.affine_for(e.Nproj, e.Ny, e.Nslice_)), _sino(e, SINO_USER0))[1]),
    ("dart_state", 6144, lambda e: e.dart_state()),
    ("art_order", 1152, lambda e: (e.be.c("art_order", 0.6, _ptr(S.art_order(e.Nrow))), _vol(e))[1]),
    ("sino_shift", 144, lambda e: (e.sino_shift(SINO_B, SINO_USER0 + 1, S.shifts_for(e.Nproj), wrap=True), _sino(e, SINO_USER0 + 1))[1]),
    ("get_recon", 4096, lambda e: e.get_recon(2)),
    ("proj_max_scale", 72, _proj),
]


def test_stage_across_types_and_sizes(gpu):
    used = S.new_engine("A")
    sizes, got = [used.get_option("stage_bytes")], {}
    for name, need, call in STAGE_STEPS:
        _prep(used)
        got[name] = call(used)
        sizes.append(used.get_option("stage_bytes"))
        assert sizes[-1] >= need, (name, sizes)
    grown = sum(b > a for a, b in zip(sizes, sizes[1:]))
    assert sizes[0] == 0 and grown >= 2 and sizes[-1] == 6144 and sizes[-1] > STAGE_STEPS[-1][1], sizes   # grew twice, then used over-sized
    for name, need, call in STAGE_STEPS:                         # the same call on an engine whose stage it is the first to use
        f = S.new_engine("A")
        _prep(f)
        want = call(f)
        assert f.get_option("stage_bytes") == need, (name, f.get_option("stage_bytes"))
        for x, y in zip(got[name] if isinstance(want, tuple) else (got[name],), want if isinstance(want, tuple) else (want,)):
            assert np.array_equal(x, y), name
    rev = S.new_engine("A")                                      # the same calls, largest need first: no buffer is ever regrown
    for name, need, call in sorted(STAGE_STEPS, key=lambda s: -s[1]):
        _prep(rev)
        call(rev)
    assert rev.get_option("stage_bytes") == used.get_option("stage_bytes")
    assert rev.get_option("pool_bytes") == used.get_option("pool_bytes") > 0
    st = ref64_dart.state(_prep_volume(), S.THR, 26, 9, ref64_dart.free_threshold(0.2))
    assert np.array_equal(got["dart_state"], st)                 # ... and the right answer


def _prep_volume():
    g = S.GEOM["A"]
    return S.phantom(g["nx"], g["n"]) + S.user_volume(g["nx"], g["n"], 70) * F32(0.25)


def test_alignment_scratch_across_an_angle_count_change(gpu):
    ang13 = np.linspace(-65, 65, 13)
    b13, x = series("C", ang13), S.user_volume(32, 32, 80)
    used = engine("C")
    used.set_volume(x)
    first = S.align_calls(used)
    used.update_projection_angles(ang13 * np.pi / 180)
    used.set_tilt_series(b13)
    assert np.array_equal(used.get_volume(), x)
    got = S.align_calls(used)
    f = S.new_engine("C", ang=ang13)
    f.set_tilt_series(b13)
    f.set_volume(x)
    want = S.align_calls(f)
    assert S.xcorr_shifts(f) == (3, 16, 3) and got.keys() == want.keys()
    for k in want:
        assert np.array_equal(got[k], want[k]), k
    assert got["xcorr0"].shape == (13, 7, 7) and first["xcorr0"].shape == (9, 7, 7) and np.array_equal(got["xcorr0"], got["xcorr2"])
    assert used.get_option("pool_bytes") == f.get_option("pool_bytes") > 0
    mom = np.stack([b13.reshape(32, 13, 32).astype(np.float64).sum(axis=(0, 2))], axis=1)
    assert np.allclose(got["moments"][:, :1], mom, rtol=1e-12, atol=0)
