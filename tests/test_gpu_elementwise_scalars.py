"""Element-wise tests of the FP epilogues, the scalar reductions and the fusion kernels against the binary64 reference of tests/ref64.py.

FP epilogues.  RESID (Landweber), RESID_NORM (tomo_sirt), RESID_MUL (Cimmino): TOMO_SINO_R after one iteration.  DD
(tomo_data_distance_sq, and its aux-stream form): G and S_DD.  POISSON (tomo_poisson_residual): SINO_R and S_COST.  Each in the kernel
instances that carry it:

  instance            how it is chosen                                   slab (slices)        geometries
  rows  VEC 4/2/1     fp_tile = 0, fp_all_lpr = 0; VEC by sxc % 256 / 128  256 / 128 and 65 / 64  lin70, neg150 (64)
  rows_g LPR 16/32    fp_tile = 0, fp_all_lpr = 16 / 32                   128                  lin70, axes45
  tile  LPR 64/32/16  fp_tile_chunks_per_pass 4 / 2 / 1 on 5 chunks:      320                  lin70w
                      passes (4, 1) / (2, 2, 1) / 1 x 5: k_fp_tile_reduce<64 / 32 / 16>
  tile (default)      -                                                  128 / 64 / 1         axes45, neg150, p1_90
  strip, list         TOMO_FP_STRIP / TOMO_FP_LIST                        128                  lin70, axes45
  list (headline)     N = 512, P = 90                                     128                  DD and POISSON only

The engine's parallel-ray matrices have no empty rows on these geometries (every ray meets the image): the rowsum == 0 rule of
RESID_NORM is reached in tests/test_gpu_user_matrix.py, on matrices with empty and negative-sum rays.  Reuse paths (k_sino_resid): tomo_sirt after a data distance of the same volume, and the CGLS restart.

Reductions (S_DIFF, S_RMSE, S_L1, S_TV, S_GNORM) on volumes with sentinels (``ref64.with_sentinels``): each test asserts that
dropping or doubling any sentinel's term moves the sum by more than 10 bounds (S_GNORM: sentinels on a constant volume, since the
TV gradient does not grow with them; at N = 512 S_GNORM is not checked, its binary64 gradient being too large to hold).  Fusion kernels (k_mm_model, k_mm_update) for 1, 2, 3
and 8 elements, gamma 1, 1.6, 2, 0.5 and lamH 0, 0.7; k_proj_max / k_proj_scale bit for bit; the host's Lipschitz constants.

The tests print the largest ratio of error to bound they saw ("ratio ...") for the bounds built on the assumed accuracy of logf,
exp2f and log2f (ref64.LOGF_ULP, C_EXP, C_LOG).
"""
import numpy as np
import pytest

import ref64
from test_gpu_elementwise import FP_LIST, FP_ROWS, FP_STRIP, FP_TILE, GEOM, TV_CASES, TV_OPTS, engine, launches, matrix
from tomo_tv_amd import _lib
from tomo_tv_amd._lib import (S_COST, S_DD, S_DIFF, S_GNORM, S_L1, S_RMSE, S_TV, SINO_B, SINO_G, SINO_R, VOL_ORIGINAL, VOL_RECON,
                              VOL_TEMP)
from tomo_tv_amd.chemistry import multimodal
from tomo_tv_amd.engine import tomoengine

pytestmark = pytest.mark.gpu
F32 = np.float32

# (id, geometry, slices, instance)
EPI_CASES = [("lin70-rows_vec4", "lin70", 256, "vec"), ("lin70-rows_vec2", "lin70", 128, "vec"), ("lin70-rows_vec2_65", "lin70", 65, "vec"),
             ("lin70-rows_vec1", "lin70", 64, "vec"), ("neg150-rows_vec1", "neg150", 64, "vec"),
             ("lin70-rows_g16", "lin70", 128, "g16"), ("lin70-rows_g32", "lin70", 128, "g32"), ("axes45-rows_g16", "axes45", 128, "g16"),
             ("lin70w-tile_ncp4", "lin70w", 320, "tile4"), ("lin70w-tile_ncp2", "lin70w", 320, "tile2"),
             ("lin70w-tile_ncp1", "lin70w", 320, "tile1"), ("axes45-tile", "axes45", 128, "tile"), ("neg150-tile", "neg150", 64, "tile"),
             ("p1_90-tile", "p1_90", 1, "tile"), ("p1_90-rows_g16", "p1_90", 1, "g16"),
             ("lin70-strip", "lin70", 128, "strip"), ("axes45-strip", "axes45", 128, "strip"), ("neg150-strip", "neg150", 64, "strip"),
             ("lin70-list", "lin70", 128, "list"), ("axes45-list", "axes45", 128, "list")]
RATIOS = {}


def _note(key, r):
    RATIOS[key] = max(RATIOS.get(key, 0.0), r)
    print(f"ratio {key}: {RATIOS[key]:.3f}")


def _epi_engine(monkeypatch, gid, nx, inst):
    ang, N, _ = GEOM[gid]
    if inst in ("strip", "list"):
        return engine(monkeypatch, ang, N, nx, fp=inst)
    t = engine(monkeypatch, ang, N, nx)
    if inst == "vec" or inst in ("g16", "g32"):
        t.set_option("fp_tile", 0)
        t.set_option("fp_all_lpr", {"vec": 0, "g16": 16, "g32": 32}[inst])
        assert t.get_option("form_fp") == FP_ROWS
    else:
        t.set_option("fp_tile", 1)
        if inst != "tile":
            t.set_option("fp_tile_chunks_per_pass", int(inst[-1]))
        assert t.get_option("form_fp") == FP_TILE
    return t


def _epi_data(M, nx):
    x = ref64.dense_volume(nx, M.N, seed=40 + nx)
    b = ref64.signed_sino(nx, M.nrow, seed=41 + nx)
    bp = np.abs(ref64.signed_sino(nx, M.nrow, seed=42 + nx)) * F32(M.N / 4)
    bp[:, ::7] = 0                                                   # rows where b is 0
    return x, b, bp.astype(F32)


def _fp_launches(t, run):
    """(K_FP_TILE, K_FP_REDUCE) launches of run()."""
    n = {}

    def inner():
        n["r"] = launches(t, _lib.K_FP_REDUCE, run)
    n["t"] = launches(t, _lib.K_FP_TILE, inner)
    return n["t"], n["r"]


@pytest.mark.parametrize("cid,gid,nx,inst", EPI_CASES, ids=[c[0] for c in EPI_CASES])
def test_fp_epilogues_elementwise(gpu, monkeypatch, cid, gid, nx, inst):
    ang, N, _ = GEOM[gid]
    M = matrix(gid)
    x, b, bp = _epi_data(M, nx)
    t = _epi_engine(monkeypatch, gid, nx, inst)
    form = t.get_option("form_fp")
    nchunk = -(-nx // 64)
    if inst.startswith("tile") and inst != "tile":
        want_passes = -(-nchunk // int(inst[-1]))
    elif form in (FP_TILE, FP_STRIP, FP_LIST):
        want_passes = None                                           # the engine's own chunk count: at least one pass
    else:
        want_passes = 0
    if inst == "vec":                                                # k_fp_rows<VEC>: VEC from the computed width sxc
        sxc = nchunk * 64
        print("VEC", 4 if sxc % 256 == 0 else 2 if sxc % 128 == 0 else 1)
    t.set_tilt_series(b)

    def run(call):
        t.set_volume(x, VOL_RECON)
        nt, nr = _fp_launches(t, call)
        if want_passes is None:
            assert nt >= 1 and nt == nr, (nt, nr)
        elif form == FP_ROWS:
            assert nt == 0 and nr == 0, (nt, nr)
        else:
            assert nt == want_passes and nr == want_passes, (nt, nr, want_passes)
    # RESID (Landweber), RESID_NORM (tomo_sirt), RESID_MUL (Cimmino)
    for mode, call in (("resid", lambda: t.be.c("sirt_landweber", VOL_RECON, 0.01, 1)),
                       ("norm", lambda: t.be.c("sirt", VOL_RECON, 1)),
                       ("mul", lambda: t.be.c("sirt_cimmino", VOL_RECON, 0.5, 1))):
        run(call)
        ref, bound = M.residual(x, b, mode)
        ref64.assert_within(f"{cid} {mode}", t._sino(SINO_R), ref, bound)
    # DD: G and S_DD, on the main stream and on the aux stream
    g64, eg, s64, es = M.data_distance(x, b)
    for variant in ("main", "async"):
        if variant == "main":
            run(lambda: t.be.c("data_distance_sq", VOL_RECON))
        else:
            run(lambda: (t.be.c("data_distance_sq_async", VOL_RECON), t.be.c("async_wait")))
        ref64.assert_within(f"{cid} G {variant}", t._sino(SINO_G), g64, eg)
        ref64.assert_scalar(f"{cid} S_DD {variant}", t._scalar(S_DD), s64, es)
    # POISSON: SINO_R and S_COST
    t.set_tilt_series(bp)
    r64, er, c64, ec = M.poisson(x, bp)
    run(lambda: t.be.c("poisson_residual", VOL_RECON, SINO_B, SINO_R))
    got = t._sino(SINO_R)
    ref64.assert_within(f"{cid} poisson", got, r64, er)
    ref64.assert_scalar(f"{cid} S_COST", t._scalar(S_COST), c64, ec)
    _note("poisson cost (LOGF_ULP)", abs(t._scalar(S_COST) - c64) / ec)


def test_residual_reuse_paths(gpu, monkeypatch):
    """tomo_sirt right after a data distance of the same volume forms its residual from G (k_sino_resid<FP_RESID_NORM>: no FP launch),
    and so does the CGLS restart (k_sino_resid<FP_RESID>).  Both element-wise, and bit for bit what projecting again gives."""
    gid, nx = "axes45", 128
    ang, N, _ = GEOM[gid]
    M = matrix(gid)
    x, b, _ = _epi_data(M, nx)
    t = engine(monkeypatch, ang, N, nx)
    assert t.get_option("fp_reuse") == 1
    t.set_tilt_series(b)
    for mode, call in (("norm", lambda: t.be.c("sirt", VOL_RECON, 1)), ("resid", lambda: t.be.c("cgls", VOL_RECON, 0))):
        ref, bound = M.residual(x, b, mode)
        t.set_volume(x, VOL_RECON)
        t.be.c("data_distance_sq", VOL_RECON)
        assert _fp_launches(t, call) == (0, 0)
        reused = t._sino(SINO_R)
        ref64.assert_within(f"reuse {mode}", reused, ref, bound)
        t.set_volume(x, VOL_RECON)                                   # a fresh write: G no longer counts, the call projects
        assert _fp_launches(t, call)[1] >= 1
        assert np.array_equal(t._sino(SINO_R), reused), mode
    # the claim a copy inherits: G = A * RECON is A * TEMP as well, until TEMP is written
    t.set_volume(x, VOL_RECON)
    t.be.c("data_distance_sq", VOL_RECON)
    t.be.c("copy_volume", VOL_TEMP, VOL_RECON)
    step = lambda: t.be.c("sirt_data", VOL_TEMP, SINO_B, 1)
    assert _fp_launches(t, step) == (0, 0)
    t.set_volume(x, VOL_TEMP)
    assert _fp_launches(t, step)[1] == 1


# ---- the headline geometry ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big512():
    ang = np.linspace(-70, 70, 90)
    return ang, ref64.Matrix(512, ang)


def test_dd_and_poisson_at_the_headline_geometry(gpu, monkeypatch, big512):
    """N = 512, P = 90, 128 slices, list forms.  Slice s is base slice s % 4 times 2^k_s (k_s = (s // 4) % 8 - 4): A x scales exactly,
    so 4 binary64 projections give A x and its bound for the whole volume, and the whole-volume S_DD and S_COST are checked.
    Residual elements in slices 0, 63, 64, 127."""
    ang, M = big512
    N, nx = 512, 128
    base = ref64.dense_volume(4, N, seed=50)
    k = (np.arange(nx) // 4) % 8 - 4
    scale = np.ldexp(1.0, k)
    x = (base[np.arange(nx) % 4] * scale[:, None, None].astype(F32)).astype(F32)
    y4, e4, _ = M.fp_bound(base)
    y, ey = y4[np.arange(nx) % 4] * scale[:, None], e4[np.arange(nx) % 4] * scale[:, None]
    rng = np.random.default_rng(51)
    b = (y * rng.uniform(0.9, 1.1, y.shape) + rng.uniform(-0.5, 0.5, y.shape)).astype(F32)
    bp = np.abs(b)
    bp[:, ::7] = 0
    t = engine(monkeypatch, ang, N, nx, fp="list")
    t.set_volume(x, VOL_RECON)
    t.set_tilt_series(b)
    t.be.c("data_distance_sq", VOL_RECON)
    g64, eg, s64, es = M.data_distance(None, b, yb=(y, ey))
    sl = [0, 63, 64, 127]
    G = t._sino(SINO_G)
    ref64.assert_within("G", G[sl], g64[sl], eg[sl])
    ref64.assert_scalar("S_DD", t._scalar(S_DD), s64, es)
    t.set_tilt_series(bp)
    t.be.c("poisson_residual", VOL_RECON, SINO_B, SINO_R)
    r64, er, c64, ec = M.poisson(None, bp, yb=(y, ey))
    ref64.assert_within("poisson", t._sino(SINO_R)[sl], r64[sl], er[sl])
    ref64.assert_scalar("S_COST", t._scalar(S_COST), c64, ec)
    _note("poisson cost (LOGF_ULP)", abs(t._scalar(S_COST) - c64) / ec)


# ---- reductions with sentinels ----------------------------------------------------------------------------------------------------------
RED_CASES = TV_CASES + [(32, 320), (512, 128)]


def _margin(name, terms, bound):
    """Every sentinel's term, dropped or doubled, moves the sum by more than 10 bounds."""
    nx, n = terms.shape[:2]
    for p in ref64.sentinel_positions(nx, n):
        assert abs(terms[p]) > 10 * bound, (name, p, float(terms[p]), bound)


@pytest.mark.parametrize("N,Nx", RED_CASES, ids=[f"N{n}-nx{x}" for n, x in RED_CASES])
def test_reductions_with_sentinels(gpu, N, Nx):
    x = ref64.with_sentinels(ref64.dense_volume(Nx, N, seed=N + Nx))
    y = ref64.dense_volume(Nx, N, seed=N + Nx + 1)
    t = tomoengine(Nx, N, np.array([0.3]))
    eps = 1e-6
    t.tv_eps = eps
    t.set_volume(x, VOL_RECON)
    t.set_volume(y, VOL_TEMP)
    t.set_volume(y, VOL_ORIGINAL)
    d = x.astype(np.float64) - y
    s, es = ref64.sqdiff(x, y)
    _margin("S_DIFF", d * d, es)
    t.matrix_2norm()
    ref64.assert_scalar("S_DIFF", t._scalar(S_DIFF), s, es)
    t.rmse()
    ref64.assert_scalar("S_RMSE", t._scalar(S_RMSE), s, es)
    xs = (x - F32(1.0)).astype(F32)                                  # signed values for the L1 norm
    s, es = ref64.l1(xs)
    _margin("S_L1", np.abs(xs.astype(np.float64)), es)
    t.set_volume(xs, VOL_RECON)
    t.l1_norm()
    ref64.assert_scalar("S_L1", t._scalar(S_L1), s, es)
    # TV value: tomo_tv, the TV before descent of tv_gd under each kernel, the input TV of FGP in each form
    tv, etv = ref64.tv_value(x, eps)
    xv = x.astype(np.float64)
    terms = np.sqrt(np.float32(eps) + sum((xv - np.roll(xv, -1, a)) ** 2 for a in range(3)))
    _margin("S_TV", terms, etv)
    t.set_volume(x, VOL_RECON)
    ref64.assert_scalar("S_TV tomo_tv", t.tv(), tv, etv)
    if N < 512:                                                      # (the binary64 gradient of 512^2 x 128 would need ~5 GB)
        gn, egn = ref64.tv_gnorm(x, eps)
        # the TV gradient is scale-free (|g| <= 4 sqrt(3) whatever the sentinel), so its sentinels sit on a constant volume, where
        # g is 0 away from them: a second volume for the S_GNORM margin
        xc = ref64.with_sentinels(np.ones((Nx, N, N), F32))
        gnc, egnc = ref64.tv_gnorm(xc, eps)
        g, _ = ref64.tv_grad(xc.astype(np.float64), float(np.float32(eps)))
        _margin("S_GNORM", g * g, egnc)
    opts = TV_OPTS if N < 512 else TV_OPTS[:1]
    for name, march4, tz in opts:
        t.set_option("tv_march4", march4)
        t.set_option("tv_tz", tz)
        if N < 512:
            for vol, ref, bound in ((x, gn, egn), (xc, gnc, egnc)):
                t.set_volume(vol, VOL_RECON)
                t.be.c("halo_local", VOL_RECON)                      # tomo_tv_grad reads the caller's halo planes
                t.be.c("tv_grad", eps)
                ref64.assert_scalar(f"S_GNORM {name}", t._scalar(S_GNORM), ref, bound)
        t.set_volume(x, VOL_RECON)
        ref64.assert_scalar(f"S_TV tv_gd {name}", t.tv_gd(1, 0.01), tv, etv)
    tv6, etv6 = ref64.tv_value(x, 1e-6)
    for name, fused, pair in (("pair", 1, 1), ("fused", 1, 0), ("unfused", 0, 0))[: 3 if N < 512 else 1]:
        t.set_option("fgp_fused", fused)
        t.set_option("fgp_pair", pair)
        t.set_volume(x, VOL_RECON)
        ref64.assert_scalar(f"S_TV fgp {name}", t.tv_fgp(3, 0.02), tv6, etv6)


# ---- fusion kernels --------------------------------------------------------------------------------------------------------------------
def fusion_volumes(nel, shape, seed, negative=False):
    """Per-element volumes with exact zeros, subnormals, values down to 1e-30 and up to 1e3 (and negative voxels if asked)."""
    rng = np.random.default_rng(seed)
    xs = []
    for _ in range(nel):
        v = np.exp(rng.uniform(np.log(1e-3), np.log(1e3), shape)).astype(F32)
        flat = v.reshape(-1)
        k = flat.size
        flat[rng.choice(k, k // 16, replace=False)] = 0
        flat[rng.choice(k, k // 32, replace=False)] = np.exp(rng.uniform(np.log(1e-30), np.log(1e-3), k // 32)).astype(F32)
        flat[rng.choice(k, k // 64, replace=False)] = (rng.integers(1, 2 ** 23, k // 64) * 2.0 ** -149).astype(F32)
        flat[:4] = [0, 1.4e-45, 1e-30, 1e3]
        if negative:
            flat[rng.choice(k, k // 16, replace=False)] *= -1
        xs.append(v)
    return xs


def _check_special(name, got, ref, bound):
    """Non-finite reference values (the rules at x == 0) exactly, the rest under the bound."""
    fin = np.isfinite(ref)
    if not np.array_equal(got[~fin], ref[~fin], equal_nan=True):
        bad = np.argwhere((got != ref) & ~fin)[:5]
        raise AssertionError(f"{name}: special values differ at {bad.tolist()}")
    ref64.assert_within(name, got[fin], ref[fin], bound[fin])
    return ref64.ratio(got[fin], ref[fin], bound[fin])


@pytest.mark.parametrize("nel", [1, 2, 3, 8])
def test_fusion_kernels_elementwise(gpu, nel):
    """k_mm_model and k_mm_update called as chemistry.py calls them, on a 65-slice slab (padding slices included).  The engine's rule
    where the reference has inf * 0: at x_e == 0, gamma < 1 and lamH != 0 the new value is +inf where w_e (upd - model) > 0 and 0
    elsewhere (fmaxf(NaN, 0) = 0); with lamH == 0 (poisson_ML) no power is formed and the step is max(0, x_e - c u_e)."""
    Nx, N = 65, 16
    ang = np.linspace(-60, 60, 5)
    dev = multimodal(Nx, N, nel, np.deg2rad(ang), np.deg2rad(ang))
    w = np.linspace(0.3, 1.7, nel).astype(F32)
    shape = (Nx, N, N)
    rng = np.random.default_rng(nel)
    for g in (1.0, 1.6, 2.0, 0.5):
        xs = fusion_volumes(nel, shape, seed=nel * 10 + int(g * 10), negative=True)
        dev.set_volume(np.stack(xs))
        dev.ce.be.mm_model(dev._x, w, g, dev.he.be, dev.MODEL)
        got = dev.he.get_volume(dev.MODEL)
        ref, bound = ref64.mm_model(xs, w, g)
        r = _check_special(f"model nel {nel} gamma {g}", got, ref, bound)
        if g != 1.0:
            _note("pow model (C_EXP, C_LOG)", r)
        xs = fusion_volumes(nel, shape, seed=nel * 10 + int(g * 10) + 1)
        us = [rng.uniform(-2, 2, shape).astype(F32) for _ in range(nel)]
        upd, model = rng.uniform(0, 3, shape).astype(F32), rng.uniform(0, 3, shape).astype(F32)
        upd.reshape(-1)[:64] = model.reshape(-1)[:64]                 # upd == model at zero voxels too
        for lamH in (0.0, 0.7):
            dev.set_volume(np.stack(xs))
            for e in range(nel):
                dev.ce.set_volume(us[e], int(dev._u[e]))
            dev.he.set_volume(upd, dev.UPD)
            dev.he.set_volume(model, dev.MODEL)
            dev.ce.be.mm_update(dev._x, dev._u, w, g, 0.05, lamH, dev.he.be, dev.UPD, dev.MODEL)
            got = dev.get_volume()
            for e, (ref, bound) in enumerate(ref64.mm_update(xs, us, w, g, 0.05, lamH, upd, model)):
                r = _check_special(f"update nel {nel} gamma {g} lamH {lamH} e {e}", got[e], ref, bound)
                if g != 1.0 and lamH != 0:
                    _note("pow update (C_EXP, C_LOG)", r)


def test_poisson_ml_from_zero_at_gamma_below_one(gpu):
    """ChemicalTomo's Poisson-ML step from a zero start at gamma 0.5 against oracle/multimodal.py (no HAADF term, so gamma plays no
    part).  Before the fix every zero voxel stayed 0 (x^(gamma-1) = inf times lamH * 0 = NaN, clamped to 0)."""
    from test_gpu_chemistry import TOL, make_case
    from conftest import rel_l2
    dev, ref, gt = make_case(gamma=0.5)
    assert dev.get_volume().max() == 0
    for it in range(5):
        c_dev, c_ref = dev.poisson_ml(0.05), ref.poisson_ml(0.05)
        assert abs(c_dev - c_ref) <= 2e-5 * abs(c_ref), (it, c_dev, c_ref)
    vol = dev.get_volume()
    assert vol.max() > 0
    assert rel_l2(vol, ref.recon) < TOL


# ---- per-projection max / scale, Lipschitz constants ------------------------------------------------------------------------------------
@pytest.mark.parametrize("Nx", [65, 3])
def test_proj_max_and_scale_bit_for_bit(gpu, Nx):
    """k_proj_max leaves the padding slices out (on 65 slices, 63 padding slices of zeros): a projection whose values are all negative
    has a negative max.  k_proj_scale is (b / div_p) * mul_p, each step correctly rounded."""
    ang, N = np.linspace(-60, 60, 6), 16
    P = len(ang)
    t = tomoengine(Nx, N, np.deg2rad(ang))
    rng = np.random.default_rng(Nx)
    s = rng.uniform(-3, 2, (Nx, P * N)).astype(F32)
    s[:, N:2 * N] = -np.abs(s[:, N:2 * N]) - F32(0.5)
    s[:, 3 * N:4 * N] = -np.abs(s[:, 3 * N:4 * N]) - F32(2.0)
    t.set_tilt_series(s)
    m = np.empty(P, F32)
    t.be.c("sino_proj_max", SINO_B, _lib_ptr(m))
    want = ref64.proj_max(s, P, N)
    assert want[1] < 0 and want[3] < 0
    assert np.array_equal(m, want), (m, want)
    div, mul = (want + F32(5)).astype(F32), np.linspace(0.5, 2, P).astype(F32)
    t.be.c("sino_proj_scale", SINO_B, _lib_ptr(div), _lib_ptr(mul))
    assert np.array_equal(t.get_projections(), ref64.proj_scale(s, P, N, div, mul))


def _lib_ptr(a):
    from tomo_tv_amd.engine import _ptr
    return _ptr(a)


@pytest.mark.parametrize("gid", list(GEOM))
def test_lipschitz_constants(gpu, gid):
    import ctypes
    ang, N, _ = GEOM[gid]
    M = matrix(gid)
    t = tomoengine(1, N, np.deg2rad(ang))
    L, eL = M.lipschitz()
    ref64.assert_scalar(f"lipschitz {gid}", t.get_lipschitz(), L, eL)
    Lc = ctypes.c_float(0)
    _lib.check(t.be.L.tomo_lipschitz_cimmino(t.be.h, ctypes.byref(Lc)))
    L, eL = M.lipschitz(cimmino=True)
    ref64.assert_scalar(f"lipschitz_cimmino {gid}", Lc.value, L, eL)
