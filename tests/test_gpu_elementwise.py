"""Element-wise tests of every projector, SART and TV form against the binary64 reference of tests/ref64.py.

Two kinds of check:

* One-hot structure (exact).  FP and BP are linear and the slices independent: a one-hot voxel at pixel j_s in slice s projects to
  column j_s of A, BIT FOR BIT (each ray sum has one non-zero term); a one-hot ray i_s back-projects to row i_s of A.  Every other
  element, padding included, must be exactly 0.  The engine's parallel-ray matrices hold no duplicate (row, col) entries (asserted:
  ``Matrix.duplicates == 0``); were there any, the expected value would be their float32 sum under the ref64 bound instead.
* Dense data under the per-element bounds of ref64: values in [0.5, 1.5] with a different offset per slice (every face, border voxel
  and the first and last slice non-zero), signed residuals and sinograms.

Every test asserts the form that actually ran (``get_option("form_fp" / "form_bp" / "form_sart")``); the parametrization ids name it.

Geometry table (angles in degrees; N rays; Nx slices):

  id          angles                              N    Nx   FP forms                 BP forms          edge classes
  lin70       linspace(-70, 70, 9)                32   128  list strip tile rows     list tile all     control, one 128-slice piece
  lin70w      linspace(-70, 70, 9)                32   320  tile with 1 / 2 / 3      -                 5 chunks of 64: 5 / 3 / 2 passes
                                                            chunks per pass                            (asserted by the launch log)
  lin70x      linspace(-70, 70, 9)                32   256  (ART chain only)         -                 4 chunks of 64: the per-row kernels at
                                                                                                       vector width 4 where the slab is ONE
                                                                                                       chain of launches (two halves: width 2)
  lin70       (list asked for on Nx = 192, 129)   32        strip (fallback)         tile (fallback)   no whole 128-slice pieces
  axes45      -90 -67 -45 -20 0 20 45 67 90       33   128  list strip tile rows     list tile all     exact 0 / +-45 / +-90, odd N
  half180     0 ... 180 step 1 (181 angles)       31   128  list strip tile rows     list tile all     beyond +-90, many strip passes
  p193        linspace(-80, 80, 193)              32   128  strip                    tile (refused     just over the BP-list limit
                                                                                     list: fallback)
  dose_sym    0, +-3, ..., +-60 (unsorted)        32   192  strip tile rows          tile all          unsorted, 3 chunks of 64
  repeat      -40 -10 15 15 50                    8    65   tile rows                tile all          repeated angle, 65 slices
  neg150      linspace(-150, -30, 11)             96   64   strip tile rows          tile all          5 angles beyond -90, one at -90
  p1_45       45                                  129  63   tile rows                tile all          P = 1, N = 129, 63 slices
  p1_90       90                                  8    1    tile rows                tile all          P = 1, one slice
  big512      linspace(-70, 70, 90)               512  128  list                     list              headline geometry (sampled)

SART (one sweep, the angles in the order given): resident (N % 8 == 0; one launch, no fallback) / tile / angle on lin70, axes45
(angle, tile), dose_sym, repeat, neg150, and resident at N = 512.  tomo_sirt, Landweber and Cimmino on lin70, axes45, dose_sym; the
ART chain there and on lin70x in its tile-fused and per-angle forms (the launch log tells them apart).  tv_gd(1) with the kernels
k_tv_march4 (tz 8; its update pass also streamed, tracked and both), k_tv_grad_reg<8> and k_tv_grad_reg<4>, and FGP with 2 and 3
iterations in each form (pair, fused, unfused), on N in {8, 31, 32, 33, 96} x Nx in {1, 63, 64, 65, 129} (the predicated edge forms:
nx % 64 != 0, n % 8 != 0).
"""
import ctypes

import numpy as np
import pytest

import oracle
import ref64
from tomo_tv_amd import _lib
from tomo_tv_amd._lib import S_DIFF, VOL_ORIGINAL, VOL_RECON, VOL_TEMP
from tomo_tv_amd.engine import _ptr, ctvlib, system_matrix, tomoengine

pytestmark = pytest.mark.gpu

FP_ROWS, FP_TILE, FP_STRIP, FP_LIST = 0, 1, 2, 3
BP_ALL, BP_TILE, BP_LIST = 0, 1, 2
SART_ANGLE, SART_TILE, SART_RESIDENT = 0, 1, 2
FP_CODE = {"rows": FP_ROWS, "tile": FP_TILE, "tile1": FP_TILE, "tile2": FP_TILE, "tile3": FP_TILE, "strip": FP_STRIP, "list": FP_LIST}
BP_CODE = {"all": BP_ALL, "tile": BP_TILE, "list": BP_LIST}

GEOM = {
    "lin70": (np.linspace(-70, 70, 9), 32, 128),
    "lin70w": (np.linspace(-70, 70, 9), 32, 320),
    "lin70x": (np.linspace(-70, 70, 9), 32, 256),
    "axes45": (np.array([-90.0, -67.0, -45.0, -20.0, 0.0, 20.0, 45.0, 67.0, 90.0]), 33, 128),
    "half180": (np.arange(0.0, 181.0, 1.0), 31, 128),
    "p193": (np.linspace(-80, 80, 193), 32, 128),
    "dose_sym": (np.array([0.0] + [s * a for a in range(3, 61, 3) for s in (1, -1)]), 32, 192),
    "repeat": (np.array([-40.0, -10.0, 15.0, 15.0, 50.0]), 8, 65),
    "neg150": (np.linspace(-150, -30, 11), 96, 64),
    "p1_45": (np.array([45.0]), 129, 63),
    "p1_90": (np.array([90.0]), 8, 1),
}
FP_CASES = [("lin70", f) for f in ("list", "strip", "tile", "rows")] + [("lin70w", f) for f in ("tile1", "tile2", "tile3")] + \
           [(g, f) for g in ("axes45", "half180") for f in ("list", "strip", "tile", "rows")] + [("p193", "strip")] + \
           [(g, f) for g in ("dose_sym", "neg150") for f in ("strip", "tile", "rows")] + \
           [(g, f) for g in ("repeat", "p1_45", "p1_90") for f in ("tile", "rows")]
BP_CASES = [(g, f) for g in ("lin70", "axes45", "half180") for f in ("list", "tile", "all")] + [("p193", "tile")] + \
           [(g, f) for g in ("dose_sym", "repeat", "neg150", "p1_45", "p1_90") for f in ("tile", "all")]

_MATRIX = {}


def matrix(gid):
    if gid not in _MATRIX:
        ang, N, _ = GEOM[gid]
        _MATRIX[gid] = ref64.Matrix(N, ang)
        assert _MATRIX[gid].duplicates == 0
    return _MATRIX[gid]


def engine(monkeypatch, ang, N, Nx, fp=None, bp=None, A=None):
    """A tomoengine running the named FP / BP form (asserted); ``A``: a ctvlib engine of that matrix (load_A) instead."""
    if fp in ("list", "strip"):
        monkeypatch.setenv("TOMO_FP_STRIP", "1")
        monkeypatch.setenv("TOMO_FP_LIST", "1" if fp == "list" else "0")
    if A is None:
        t = tomoengine(Nx, N, np.asarray(ang) * np.pi / 180)
    else:
        t = ctvlib(Nx, N, len(ang))
        t.load_A(A)
    monkeypatch.delenv("TOMO_FP_STRIP", raising=False)
    monkeypatch.delenv("TOMO_FP_LIST", raising=False)
    if fp in ("tile", "tile1", "tile2", "tile3"):
        t.set_option("fp_tile", 1)
        if fp != "tile":
            t.set_option("fp_tile_chunks_per_pass", int(fp[-1]))
    elif fp == "rows":
        t.set_option("fp_tile", 0)
    if bp == "tile":
        t.set_option("bp_list", 0)
    elif bp == "all":
        t.set_option("bp_tile", 0)
    if fp is not None:
        assert t.get_option("form_fp") == FP_CODE[fp], (fp, t.get_option("form_fp"))
    if bp is not None:
        assert t.get_option("form_bp") == BP_CODE[bp], (bp, t.get_option("form_bp"))
    return t


def fp_of(t, x):
    t.set_volume(x, VOL_ORIGINAL)
    t.create_projections()
    return t.get_projections()


def bp_of(t, r):
    t.set_tilt_series(r)
    t.back_projection_of_tilt_series()
    return t.get_volume()


def onehot_fp(t, M, Nx, cols):
    """Forward-project one-hot volumes, Nx columns per launch: every output bit for bit."""
    for k0 in range(0, len(cols), Nx):
        js = cols[k0:k0 + Nx]
        x = np.zeros((Nx, M.ncol), np.float32)
        x[np.arange(len(js)), js] = 1.0
        got = fp_of(t, x.reshape(Nx, M.N, M.N))
        want = np.zeros((Nx, M.nrow), np.float32)
        for s, j in enumerate(js):
            want[s] = M.dense_column_f32(j)
        if not np.array_equal(got, want):
            bad = np.argwhere(got != want)[:5]
            raise AssertionError(f"one-hot FP: {int((got != want).sum())} wrong elements, first (slice, row) {bad.tolist()} "
                                 f"(pixels {[int(js[b[0]]) if b[0] < len(js) else None for b in bad]}): "
                                 f"got {[float(got[tuple(b)]) for b in bad]}, want {[float(want[tuple(b)]) for b in bad]}")


def onehot_bp(t, M, Nx, rows):
    for k0 in range(0, len(rows), Nx):
        rs = rows[k0:k0 + Nx]
        r = np.zeros((Nx, M.nrow), np.float32)
        r[np.arange(len(rs)), rs] = 1.0
        got = bp_of(t, r).reshape(Nx, M.ncol)
        want = np.zeros((Nx, M.ncol), np.float32)
        for s, i in enumerate(rs):
            want[s] = M.dense_row_f32(i)
        if not np.array_equal(got, want):
            bad = np.argwhere(got != want)[:5]
            raise AssertionError(f"one-hot BP: {int((got != want).sum())} wrong elements, first (slice, pixel) {bad.tolist()} "
                                 f"(rays {[int(rs[b[0]]) if b[0] < len(rs) else None for b in bad]}): "
                                 f"got {[float(got[tuple(b)]) for b in bad]}, want {[float(want[tuple(b)]) for b in bad]}")


def dense_fp_check(t, M, Nx, orc_slices=None):
    x = ref64.dense_volume(Nx, M.N, seed=M.N + Nx)
    y = fp_of(t, x)
    sl = np.arange(Nx) if orc_slices is None else np.asarray(orc_slices)
    y64, bound, ax = M.fp_bound(x[sl])
    print(f"ratio FP dense: {ref64.ratio(y[sl], y64, bound):.3f}")
    ref64.assert_within("FP", y[sl], y64, bound)
    orc = oracle.ctvlib(len(sl), M.N, M.P)
    orc.A = oracle.CSR(M.nrow, M.ncol, *M.csr())
    orc.original_volume = np.ascontiguousarray(x[sl])
    orc.create_projections()
    ref64.assert_typical("FP", y[sl], orc.b, y64, ax)


def dense_bp_check(t, M, Nx, orc_slices=None):
    r = ref64.signed_sino(Nx, M.nrow, seed=M.N + 3 * Nx)
    v = bp_of(t, r)
    sl = np.arange(Nx) if orc_slices is None else np.asarray(orc_slices)
    v64, bound, ar = M.bp_bound(r[sl])
    print(f"ratio BP dense: {ref64.ratio(v[sl], v64, bound):.3f}")
    ref64.assert_within("BP", v[sl], v64, bound)
    orc = oracle.ctvlib(len(sl), M.N, M.P)
    orc.A = oracle.CSR(M.nrow, M.ncol, *M.csr())
    ref64.assert_typical("BP", v[sl], orc.back_projection(r[sl]), v64, ar)


def launches(t, kernel, run):
    """How many launches of ``kernel`` (tomo_tv_amd._lib.K_*) ``run()`` makes on engine ``t`` (the engine's launch log)."""
    L = _lib.load()
    _lib.check(L.tomo_profile_enable(t.be.h, kernel, 1))
    run()
    n, ms = ctypes.c_int64(0), ctypes.c_double(0)
    _lib.check(L.tomo_profile_read(t.be.h, kernel, ctypes.byref(n), ctypes.byref(ms)))
    _lib.check(L.tomo_profile_enable(t.be.h, kernel, 0))
    return int(n.value)


# ---- FP / BP: every form, every edge class ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gid,form", FP_CASES, ids=[f"{g}-fp_{f}" for g, f in FP_CASES])
def test_forward_projector_elementwise(gpu, monkeypatch, gid, form):
    ang, N, Nx = GEOM[gid]
    M = matrix(gid)
    t = engine(monkeypatch, ang, N, Nx, fp=form)
    if form[-1].isdigit():                                 # the passes the forced chunk count gives: ceil(64-slice chunks / count)
        ncp, nchunk = int(form[-1]), -(-Nx // 64)
        assert launches(t, _lib.K_FP_TILE, lambda: fp_of(t, np.zeros((Nx, N, N), np.float32))) == -(-nchunk // ncp)
    onehot_fp(t, M, Nx, np.arange(M.ncol))                 # every column of A
    dense_fp_check(t, M, Nx)


@pytest.mark.parametrize("Nx", [192, 129])
def test_list_forms_fall_back_where_the_slab_is_no_whole_128_slice_pieces(gpu, monkeypatch, Nx):
    """The list forms need whole 128-slice pieces (sxc % 128 == 0): asked for on 192 (129 -> 192 padded) slices, the strip FP and the
    tile BP run -- and are element-wise right there."""
    ang, N, _ = GEOM["lin70"]
    M = matrix("lin70")
    monkeypatch.setenv("TOMO_FP_STRIP", "1")
    monkeypatch.setenv("TOMO_FP_LIST", "1")
    t = tomoengine(Nx, N, ang * np.pi / 180)
    assert t.get_option("fp_strip") == 1 and t.get_option("fp_list") == 1 and t.get_option("bp_list") == 1
    assert t.get_option("form_fp") == FP_STRIP and t.get_option("form_bp") == BP_TILE
    onehot_fp(t, M, Nx, np.arange(M.ncol))
    onehot_bp(t, M, Nx, np.arange(M.nrow))
    dense_fp_check(t, M, Nx)
    dense_bp_check(t, M, Nx)


@pytest.mark.parametrize("gid,form", BP_CASES, ids=[f"{g}-bp_{f}" for g, f in BP_CASES])
def test_back_projector_elementwise(gpu, monkeypatch, gid, form):
    ang, N, Nx = GEOM[gid]
    M = matrix(gid)
    t = engine(monkeypatch, ang, N, Nx, bp=form)
    onehot_bp(t, M, Nx, np.arange(M.nrow))                 # every row of A
    dense_bp_check(t, M, Nx)


def test_bp_list_refused_over_192_angles(gpu, monkeypatch):
    """P = 193: the list back projector keeps no bounds for so many angles; asking for it runs the tile form."""
    ang, N, Nx = GEOM["p193"]
    t = engine(monkeypatch, ang, N, Nx)
    assert t.get_option("bp_list") == 1 and t.get_option("bp_list_ready") == 0
    assert t.get_option("form_bp") == BP_TILE


@pytest.fixture(scope="module")
def big512():
    ang = np.linspace(-70, 70, 90)
    return ang, ref64.Matrix(512, ang)


@pytest.mark.parametrize("form", ["fp_list", "bp_list"])
def test_list_projectors_at_the_headline_geometry(gpu, monkeypatch, big512, form):
    """N = 512, P = 90, 128 slices (list forms): one-hot at every border pixel / the first and last ray of every angle and ~2000
    random ones; dense data checked in slices 0, 63, 64, 127 (the chunk edges)."""
    ang, M = big512
    N, Nx = 512, 128
    rng = np.random.default_rng(12)
    t = engine(monkeypatch, ang, N, Nx, fp="list", bp="list")
    if form == "fp_list":
        yy, zz = np.divmod(np.arange(M.ncol), N)
        border = np.nonzero((yy == 0) | (zz == 0) | (yy == N - 1) | (zz == N - 1))[0]
        cols = np.concatenate([border, rng.choice(M.ncol, 2000, replace=False)])
        onehot_fp(t, M, Nx, cols)
        dense_fp_check(t, M, Nx, orc_slices=[0, 63, 64, 127])
    else:
        ends = np.concatenate([np.arange(M.P) * N, np.arange(M.P) * N + N - 1])
        rows = np.concatenate([ends, rng.choice(M.nrow, 2000, replace=False)])
        onehot_bp(t, M, Nx, rows)
        dense_bp_check(t, M, Nx, orc_slices=[0, 63, 64, 127])


# ---- SIRT-type steps ------------------------------------------------------------------------------------------------------------------
STEP_GEOM = ["lin70", "axes45", "dose_sym"]


def _step_data(M, Nx):
    x = ref64.dense_volume(Nx, M.N, seed=21)
    b = (M.fp(ref64.dense_volume(Nx, M.N, seed=22)) * 1.02).astype(np.float32)
    return x, b


@pytest.mark.parametrize("gid", STEP_GEOM)
def test_sirt_landweber_cimmino_step_elementwise(gpu, monkeypatch, gid):
    ang, N, Nx = GEOM[gid]
    M = matrix(gid)
    x, b = _step_data(M, Nx)
    t = engine(monkeypatch, ang, N, Nx)
    assert t.get_option("form_fp") in (FP_TILE, FP_STRIP, FP_LIST) and t.get_option("form_bp") in (BP_TILE, BP_LIST, BP_ALL)
    t.set_tilt_series(b)
    t.set_volume(x, VOL_RECON)
    t.SIRT(1)
    ref, bound = M.tomo_sirt_step(x, b)
    ref64.assert_within("tomo_sirt", t.get_volume(), ref, bound)
    A = system_matrix(N, ang)
    for kind, beta in (("landweber", 0.01), ("cimmino", 0.5)):
        c = ctvlib(Nx, N, M.P)
        c.load_A(A)
        c.set_tilt_series(b)
        c.set_volume(x, VOL_RECON)
        if kind == "cimmino":
            c.cimminos_method()
            ref, bound = M.cimmino_step(x, b, beta)
        else:
            ref, bound = M.landweber_step(x, b, beta)
        c.SIRT(beta)
        ref64.assert_within(kind, c.get_volume(), ref, bound)


# tile1: the tile-fused form as ONE chain of launches ("sart_streams" = 1; by default a slab of an even number of 64-slice chunks
# runs as two half-slab chains, whose per-row kernels take the vector width that divides the half: 2 at 256 slices, 4 as one chain)
ART_CASES = [(g, v) for g in STEP_GEOM for v in ("tile", "angle")] + [("lin70x", "tile1"), ("lin70x", "angle")]


@pytest.mark.parametrize("gid,variant", ART_CASES, ids=[f"{g}-art_chain_{v}" for g, v in ART_CASES])
def test_art_chain_elementwise(gpu, gid, variant):
    """The chained ART sweep (k_art_chain): its tile-fused form (one k_sart_tile FP, then P - 1 fused steps: asserted by the launch
    log) and its per-angle form (FP + chain + BP per angle: no fused step)."""
    ang, N, Nx = GEOM[gid]
    M = matrix(gid)
    x, b = _step_data(M, Nx)
    sl = [0, Nx // 2, Nx - 1]
    c = ctvlib(Nx, N, M.P)
    c.load_A(system_matrix(N, ang))
    c.set_option("art_chain", 1)
    c.set_option("art_tile", 0 if variant == "angle" else 1)
    if variant == "tile1":
        c.set_option("sart_streams", 1)
    assert c.get_option("art_chain_ready") == 1
    c.set_tilt_series(b)
    c.set_volume(x, VOL_RECON)
    c.row_inner_product()
    fused = launches(c, _lib.K_SART_FUSED, lambda: c.ART(0.6))
    if variant == "tile1":
        assert fused == M.P - 1, fused
    elif variant == "tile":
        assert fused > 0 and fused % (M.P - 1) == 0, fused
    else:
        assert fused == 0
    got = c.get_volume()[sl]
    orc = oracle.ctvlib(len(sl), N, M.P)
    orc.A = oracle.CSR(M.nrow, M.ncol, *M.csr())
    orc.set_tilt_series(b[sl])
    orc.recon[:] = x[sl]
    orc.row_inner_product()
    orc.ART(0.6)
    ref64.assert_seq("ART chain", got, orc.recon, M.art(x[sl], b[sl], 0.6))


# ---- SART sweeps ----------------------------------------------------------------------------------------------------------------------
SART_CASES = [("lin70", "resident"), ("lin70", "tile"), ("lin70", "angle"), ("axes45", "tile"), ("axes45", "angle"),
              ("dose_sym", "resident"), ("dose_sym", "tile"), ("repeat", "resident"), ("repeat", "angle"), ("neg150", "resident"),
              ("neg150", "tile")]


def _sart_check(t, M, x, b, form, sl, beta=0.7, order=None):
    """One sweep (tomo_sart: what ``tomoengine.SART`` calls) in the named form, the angles in ``order`` (None: as given).  Beyond the
    three public forms: "coop" / "coop_own" = the tile chain with the residual rows formed inside the next tile step ("sart_coop";
    _own: every workgroup forms its own rows), "walk" = the fused ray-walk step ("sart_tile" = 0; reported as ANGLE)."""
    if form == "resident":
        t.set_option("sart_resident", 1)
    elif form in ("tile", "coop", "coop_own"):
        t.set_option("sart_resident", 0)
        t.set_option("sart_coop", 0 if form == "tile" else 1)
        if form == "coop_own":
            t.set_option("sart_coop_spin", -1)
    elif form == "walk":
        t.set_option("sart_resident", 0)
        t.set_option("sart_tile", 0)
    else:
        t.set_option("sart_fused", 0)
    code = {"resident": SART_RESIDENT, "tile": SART_TILE, "coop": SART_TILE, "coop_own": SART_TILE, "walk": SART_ANGLE, "angle": SART_ANGLE}[form]
    assert t.get_option("form_sart") == code, (form, t.get_option("form_sart"))
    t.set_tilt_series(b)
    t.set_volume(x, VOL_RECON)
    o = None if order is None else np.ascontiguousarray(order, np.int32)
    count = {}

    def sweep():
        count["fused"] = launches(t, _lib.K_SART_FUSED, lambda: t.be.c("sart", VOL_RECON, float(beta), 1, None if o is None else _ptr(o)))
    n = launches(t, _lib.K_SART_RESIDENT, sweep)
    got = t.get_volume()[sl]
    if form == "walk":
        assert count["fused"] > 0                       # fused ray-walk steps, not one FP + one BP launch per angle
    if form == "resident":
        assert n == 1 and t.get_option("sart_resident_fallbacks") == 0
    else:
        assert n == 0
    orc = oracle.ctvlib(len(sl), M.N, M.P)
    orc.A = oracle.CSR(M.nrow, M.ncol, *M.csr())
    orc.set_tilt_series(b[sl])
    orc.recon[:] = x[sl]
    orc.SART(beta, 1, order=o)
    ref = M.sart(x[sl], b[sl], beta, order=o)
    print(f"ratio SART sweep: {ref64.ratio(got, ref, ref64.seq_bound(orc.recon, ref)):.3f}")
    ref64.assert_seq(f"SART {form}", got, orc.recon, ref)
    return got, orc.recon


@pytest.mark.parametrize("gid,form", SART_CASES, ids=[f"{g}-sart_{f}" for g, f in SART_CASES])
def test_sart_sweep_elementwise(gpu, monkeypatch, gid, form):
    ang, N, Nx = GEOM[gid]
    M = matrix(gid)
    x, b = _step_data(M, Nx)
    t = engine(monkeypatch, ang, N, Nx)
    _sart_check(t, M, x, b, form, np.arange(Nx))


def test_resident_sart_at_the_headline_geometry(gpu, monkeypatch, big512):
    ang, M = big512
    Nx = 128
    x = ref64.dense_volume(Nx, 512, seed=31)
    b = (ref64.dense_volume(Nx, 512, seed=32).mean() * M.rowsum[None, :] * np.linspace(0.9, 1.1, Nx)[:, None]).astype(np.float32)
    t = engine(monkeypatch, ang, 512, Nx)
    _sart_check(t, M, x, b, "resident", [0, 63, 64, 127])


# ---- TV descent and FGP ------------------------------------------------------------------------------------------------------------------
TV_CASES = [(8, 1), (31, 63), (32, 64), (33, 65), (96, 129), (32, 129), (31, 1)]
# (kernel that runs, tv_march4, tv_tz): with tv_tz = 4 both passes run k_tv_grad_reg<4> whatever tv_march4 says
TV_OPTS = [("march4_tz8", 1, 8), ("reg_tz8", 0, 8), ("reg_tz4", 1, 4)]
# ... and (sart_nt, tracked), the other instances of the march's update pass: sart_nt = 1 streams its accesses at any slab size (-1: by
# size, none of these); tracked: tv_gd_tracked, whose last update pass also forms the step norm and writes the snapshot
TV_UPDATE_OPTS = [o + (-1, False) for o in TV_OPTS] + \
                 [("march4_tz8_nt", 1, 8, 1, False), ("march4_tz8_tracked", 1, 8, -1, True), ("march4_tz8_nt_tracked", 1, 8, 1, True)]


def _tv_input(Nx, N):
    return ref64.dense_volume(Nx, N, seed=N * 1000 + Nx)


@pytest.mark.parametrize("N,Nx", TV_CASES, ids=[f"N{n}-nx{x}" for n, x in TV_CASES])
def test_tv_gd_elementwise(gpu, N, Nx):
    x = _tv_input(Nx, N)
    eps, dpocs = 1e-6, 0.02 * np.sqrt(x.size)
    orc = oracle.ctvlib(Nx, N, 1)
    orc.tv_eps = eps
    orc.recon[:] = x
    orc.tv_gd(1, dpocs)
    t64 = ref64.tv_gd(x, 1, dpocs, eps)
    for name, march4, tz, nt, tracked in TV_UPDATE_OPTS:
        t = tomoengine(Nx, N, np.array([0.3]))
        t.tv_eps = eps
        t.set_option("tv_march4", march4)
        t.set_option("tv_tz", tz)
        t.set_option("sart_nt", nt)
        t.set_volume(x, VOL_RECON)
        if tracked:                                        # the snapshot (TEMP) holds the volume before the step
            t.set_volume(x, VOL_TEMP)
            t.tv_gd_tracked(1, dpocs)
        else:
            t.tv_gd(1, dpocs)
        got = t.get_volume()
        ref64.assert_seq(f"tv_gd {name}", got, orc.recon, t64)
        if tracked:                                        # ... then the new volume, and S_DIFF the squared norm of the step taken
            assert np.array_equal(t.get_volume(VOL_TEMP), got), name
            ref64.assert_scalar(f"S_DIFF tv_gd {name}", t._scalar(S_DIFF), *ref64.sqdiff(got, x))


@pytest.mark.parametrize("iters", [2, 3])
@pytest.mark.parametrize("N,Nx", TV_CASES, ids=[f"N{n}-nx{x}" for n, x in TV_CASES])
def test_fgp_elementwise(gpu, N, Nx, iters):
    """FGP in its three forms.  Pair form: 2 iterations run the final pair pass alone (k_fgp_fused2<FINAL>), 3 iterations a pair step
    (k_fgp_fused2, what every call of 3 and more iterations runs) and then the one-iteration end pass."""
    x = _tv_input(Nx, N)
    lam = 0.02
    orc = oracle.ctvlib(Nx, N, 1)
    orc.recon[:] = x
    orc.tv_fgp(iters, lam)
    g64 = ref64.tv_fgp(x, iters, lam)
    for name, fused, pair in (("pair", 1, 1), ("fused", 1, 0), ("unfused", 0, 0)):
        t = tomoengine(Nx, N, np.array([0.3]))
        t.set_option("fgp_fused", fused)
        t.set_option("fgp_pair", pair)
        t.set_volume(x, VOL_RECON)
        t.tv_fgp(iters, lam)
        ref64.assert_seq(f"fgp {name} x{iters}", t.get_volume(), orc.recon, g64)
