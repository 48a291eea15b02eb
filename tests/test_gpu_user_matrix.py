"""Element-wise tests of engines built from a CALLER'S matrix (``ctvlib.load_A`` / ``update_proj_angles``: tomo_create_from_matrix)
against the binary64 reference of tests/ref64.py, on the matrix families of tests/user_matrices.py:

  dead      empty rays (rowsum == 0: the first / last ray, middle rays, one whole angle) and pixels no angle crosses (colsum == 0)
  gain      per-ray factors (row sums no longer the chord length)
  signed    one angle negated: row sums and per-angle column sums < 0 (``> 0`` against ``!= 0``)
  messy     dead + duplicate (row, col) triplets (the last assignment wins), explicit 0.0 / -0.0 weights, entries that end as 0, shuffled
  shuffled  rays permuted inside every angle: a pixel's two rays are no neighbours (no ART chain, no resident sweep, no SART tiles)

on the geometries lin70 (N 32, 128 slices), axes45 (N 33, 128) -- every family -- and repeat (N 8, 65 slices), neg150 (N 96, 64) -- dead
and messy.  The reference is ``ref64.Matrix`` of ``canonical(A)`` (tests/test_user_matrices_cpu.py: the oracle's loadA keeps exactly
that); the engine is fed the raw triplets.  Which table builders take which family is established on the CPU by
tests/native/user_matrix_check and pinned in ``user_matrices.EXPECTED``; every test asserts the engine's ``*_ready`` options and the
form that ran against that table.  No tolerance is new: every bound is one of ref64's, evaluated on the canonical matrix, and every
"unchanged" / "zero" assertion is exact.

Worst error-to-bound ratios seen on an MI355X over the whole file (observations, printed as "ratio ..."; none was used to set a bound):
FP dense 0.130, BP dense 0.143; residual resid 0.144, norm 0.128, mul 0.132; tomo_sirt 0.055 (the same in the list, tile and voxel-driven
back projector), landweber 0.212, cimmino 0.063; SART sweep 0.259 and ART sweep 0.190 (of the oracle's yardstick ``seq_bound``);
pdhg_sino_dual 0.577; pdhg_tv_step x 0.449, xbar 0.482, p 0.277.  The one-hot checks are exact.  ``row_inner_product`` has no read-back:
its table is checked through the Cimmino step, the Cimmino constant and the ART sweeps.

Not asserted here: that moving an idle angle inside a sweep's order changes no bit -- it does, in rounding: the first angle of a tile
sweep is projected by another kernel instance than the later ones.  The exact statement is made on a matrix whose angles are ALL idle
(``test_angles_without_a_positive_row_sum_leave_the_volume``).
"""
import numpy as np
import pytest

import oracle
import ref64
import ref64_pdhg as R
import user_matrices as um
from test_gpu_elementwise import (BP_ALL, BP_TILE, FP_ROWS, FP_TILE, GEOM, SART_ANGLE, _sart_check, _step_data,
                                  dense_bp_check, dense_fp_check, engine, launches, onehot_bp, onehot_fp)
from test_gpu_pdhg import P0, UVOL, X, XBAR, dense_inputs, get_p, put
from tomo_tv_amd import _lib
from tomo_tv_amd._lib import SINO_R, SINO_USER0, VOL_RECON
from tomo_tv_amd.engine import _ptr, ctvlib, system_matrix

pytestmark = pytest.mark.gpu
assert all(np.array_equal(GEOM[g][0], um.GEOM[g][0]) and GEOM[g][1:] == um.GEOM[g][1:] for g in um.GEOM)      # (the CPU tests take theirs from user_matrices)
F32 = np.float32
IDS = [f"{f}-{g}" for f, g in um.CASES]
RATIOS = {}
_CASE = {}


def _note(key, got, ref, bound):
    RATIOS[key] = max(RATIOS.get(key, 0.0), ref64.ratio(got, ref, bound))
    print(f"ratio {key}: {RATIOS[key]:.3f}")


class Case:
    """One (family, geometry): the raw triplets, the binary64 matrix of their canonical form, and what the family must reach --
    asserted from the matrix alone, before any engine exists."""

    def __init__(self, name, gid):
        self.name, self.gid = name, gid
        self.ang, self.N, self.Nx = GEOM[gid]
        self.P = self.ang.size
        self.own = system_matrix(self.N, self.ang)
        self.A = um.family(name, self.own, self.N, self.P)
        self.M, self.dropped = um.reference(self.N, self.ang, self.A)
        um.assert_reaches(name, self.N, self.P, um.properties(self.M), self.dropped)
        self.exp = um.EXPECTED[name, gid]
        M = self.M
        self.dead_rows = np.nonzero(M.rowsum <= 0)[0]              # rays whose normalised residual is 0 by rule
        self.dead_pix = np.nonzero(M.colsum <= 0)[0]               # pixels no all-angle step may move
        self.idle_angles = [i for i in range(self.P) if np.all(M.rowsum[i * self.N:(i + 1) * self.N] <= 0)]   # removed / negated


def case(name, gid):
    if (name, gid) not in _CASE:
        _CASE[name, gid] = Case(name, gid)
    return _CASE[name, gid]


def assert_ready(t, c):
    """The engine's answers are the host check's (user_matrices.EXPECTED)."""
    assert t.get_option("art_chain_ready") == c.exp["art_chain_ok"]
    assert t.get_option("sart_resident_ready") == c.exp["sart_resident_ok"]
    assert t.get_option("bp_list_ready") == c.exp["bp_list_ok"]


def fp_forms(c):
    whole = (-(-c.Nx // 64) * 64) % 128 == 0                       # the list forms need whole 128-slice pieces
    return (["list"] if c.exp["fp_list_ok"] and whole else []) + (["strip"] if c.exp["fp_strip_ok"] else []) + ["tile", "rows"]


def bp_forms(c):
    whole = (-(-c.Nx // 64) * 64) % 128 == 0
    return (["list"] if c.exp["bp_list_ok"] and whole else []) + (["tile"] if c.exp["bp_tile_ok"] else []) + ["all"]


def sart_forms(c):
    return (["resident"] if c.exp["sart_resident_ok"] else []) + (["tile"] if c.exp["sart_tile_ok"] else []) + ["angle"]


def sample(c, n_all, special, seed):
    """All of 0 .. n_all - 1 for N <= 33; at N = 96 the special ones and a seeded sample."""
    if c.N <= 33:
        return np.arange(n_all)
    rng = np.random.default_rng(seed)
    return np.unique(np.concatenate([np.asarray(special, np.int64), rng.choice(n_all, 384, replace=False)]))


def touched(c):
    """(pixels, rays) of the entries the family changed against the engine's own matrix: removed, duplicated, zeroed."""
    key = lambda A: A[0].astype(np.int64) * c.M.ncol + A[1].astype(np.int64)   # noqa: E731
    C = um.canonical(c.A, c.M.ncol)
    own = dict(zip(key(c.own).tolist(), c.own[2].tolist()))
    new = dict(zip(key(C).tolist(), C[2].tolist()))
    diff = [k for k in set(own) | set(new) if own.get(k) != new.get(k)]
    d = np.asarray(sorted(diff)[::max(1, len(diff) // 1500)], np.int64)
    return d % c.M.ncol, d // c.M.ncol


def _forms_table(kind):
    out = []
    for f, g in um.CASES:
        exp = um.EXPECTED[f, g]
        whole = (-(-GEOM[g][2] // 64) * 64) % 128 == 0
        if kind == "fp":
            forms = (["list"] if exp["fp_list_ok"] and whole else []) + (["strip"] if exp["fp_strip_ok"] else []) + ["tile", "rows"]
        elif kind == "bp":
            forms = (["list"] if exp["bp_list_ok"] and whole else []) + (["tile"] if exp["bp_tile_ok"] else []) + ["all"]
        else:
            forms = (["resident"] if exp["sart_resident_ok"] else []) + (["tile"] if exp["sart_tile_ok"] else []) + ["angle"]
        out += [(f, g, form) for form in forms]
    return out


FP_CASES, BP_CASES, SART_CASES = _forms_table("fp"), _forms_table("bp"), _forms_table("sart")


# ---- FP / BP in every form the builders serve ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,gid,form", FP_CASES, ids=[f"{f}-{g}-fp_{m}" for f, g, m in FP_CASES])
def test_forward_projector_on_a_user_matrix(gpu, monkeypatch, name, gid, form):
    c = case(name, gid)
    M = c.M
    assert form in fp_forms(c)
    t = engine(monkeypatch, c.ang, c.N, c.Nx, fp=form, A=c.A)      # (asserts form_fp)
    assert_ready(t, c)
    if form in ("list", "strip"):
        assert t.get_option("fp_strip_ready") == c.exp["fp_strip_ok"] and (form != "list" or t.get_option("fp_list_ready") == c.exp["fp_list_ok"])
    yy, zz = np.divmod(np.arange(M.ncol), c.N)
    border = np.nonzero((yy == 0) | (zz == 0) | (yy == c.N - 1) | (zz == c.N - 1))[0]
    cols = sample(c, M.ncol, np.concatenate([border, c.dead_pix, touched(c)[0]]), 1)
    # one-hot, bit for bit: a removed row or column is exactly 0, a duplicated entry its last value, a zero weight 0
    onehot_fp(t, M, c.Nx, cols)
    dense_fp_check(t, M, c.Nx)


@pytest.mark.parametrize("name,gid,form", BP_CASES, ids=[f"{f}-{g}-bp_{m}" for f, g, m in BP_CASES])
def test_back_projector_on_a_user_matrix(gpu, monkeypatch, name, gid, form):
    c = case(name, gid)
    M = c.M
    assert form in bp_forms(c)
    t = engine(monkeypatch, c.ang, c.N, c.Nx, bp=form, A=c.A)      # (asserts form_bp)
    assert_ready(t, c)
    ends = np.concatenate([np.arange(c.P) * c.N, np.arange(c.P) * c.N + c.N - 1])
    rows = sample(c, M.nrow, np.concatenate([ends, c.dead_rows, touched(c)[1]]), 2)
    onehot_bp(t, M, c.Nx, rows)
    dense_bp_check(t, M, c.Nx)


def test_forms_a_builder_refuses_fall_back(gpu, monkeypatch):
    """Rays shuffled: the list back projector and the SART tile / resident tables do not exist; asked for, the tile back projector and
    the ray-walk sweep run (by their codes), and the ART chain is not ready."""
    c = case("shuffled", "lin70")
    monkeypatch.setenv("TOMO_FP_STRIP", "1")
    monkeypatch.setenv("TOMO_FP_LIST", "1")
    t = ctvlib(c.Nx, c.N, c.P)
    t.load_A(c.A)
    assert t.get_option("bp_list") == 1 and t.get_option("bp_list_ready") == 0 and t.get_option("form_bp") == BP_TILE
    assert t.get_option("sart_resident_ready") == 0 and t.get_option("form_sart") == SART_ANGLE and t.get_option("art_chain_ready") == 0
    t.set_option("bp_tile", 0)
    assert t.get_option("form_bp") == BP_ALL


# ---- residual epilogues: the rowsum > 0 rule ----------------------------------------------------------------------------------------------
# the instances EPI_CASES (test_gpu_elementwise_scalars.py) names per geometry: lin70 rows VEC 2 / rows_g 16, 32 / strip / list (and the
# default tile), axes45 rows_g 16 / tile / strip / list, neg150 (64 slices) rows VEC 1 / tile / strip; repeat (65 slices -> 128: VEC 2) is
# not in that table: every instance its slab can run
EPI = [(f, g, inst) for f in ("dead", "signed", "messy") for g, insts in (("lin70", ("vec", "g16", "g32", "tile", "strip", "list")),
                                                                          ("axes45", ("g16", "tile", "strip", "list"))) for inst in insts] + \
      [(f, g, inst) for f in ("dead", "messy") for g, insts in (("neg150", ("vec", "tile", "strip")),
                                                                ("repeat", ("vec", "g16", "tile", "strip", "list"))) for inst in insts]


@pytest.mark.parametrize("name,gid,inst", EPI, ids=[f"{f}-{g}-{i}" for f, g, i in EPI])
def test_residual_epilogues_on_a_user_matrix(gpu, monkeypatch, name, gid, inst):
    c = case(name, gid)
    M = c.M
    if inst in ("strip", "list"):
        t = engine(monkeypatch, c.ang, c.N, c.Nx, fp=inst, A=c.A)
    else:
        t = engine(monkeypatch, c.ang, c.N, c.Nx, fp="tile" if inst == "tile" else "rows", A=c.A)
        if inst != "tile":
            t.set_option("fp_all_lpr", {"vec": 0, "g16": 16, "g32": 32}[inst])
            assert t.get_option("form_fp") == FP_ROWS
        else:
            assert t.get_option("form_fp") == FP_TILE
    x = ref64.dense_volume(c.Nx, c.N, seed=40 + c.Nx)
    b = ref64.signed_sino(c.Nx, M.nrow, seed=41 + c.Nx)
    assert len(c.dead_rows) and np.all(b[:, c.dead_rows] != 0)
    t.set_tilt_series(b)
    for mode, call in (("resid", lambda: t.be.c("sirt_landweber", VOL_RECON, 0.01, 1)), ("norm", lambda: t.be.c("sirt", VOL_RECON, 1)),
                       ("mul", lambda: t.be.c("sirt_cimmino", VOL_RECON, 0.5, 1))):
        t.set_volume(x, VOL_RECON)
        call()
        got = t._sino(SINO_R)
        ref, bound = M.residual(x, b, mode)
        _note(f"residual {mode}", got, ref, bound)
        ref64.assert_within(f"{name} {gid} {inst} {mode}", got, ref, bound)
        if mode == "norm":                                          # rowsum <= 0: exactly 0, whatever b holds there
            assert not got[:, c.dead_rows].any()


# ---- SIRT-type steps and the host tables -------------------------------------------------------------------------------------------------
def _signed_start(c):
    """The step data of the own-matrix tests, with negative values on every pixel no angle crosses (and a few others)."""
    x, b = _step_data(c.M, c.Nx)
    x = x.copy()
    x[::3].reshape(-1, c.M.ncol)[:, c.dead_pix] *= F32(-1)
    x[1::5, c.N // 2, ::4] *= F32(-1)
    return x, b


@pytest.mark.parametrize("name,gid", um.CASES, ids=IDS)
def test_sirt_landweber_cimmino_on_a_user_matrix(gpu, monkeypatch, name, gid):
    c = case(name, gid)
    M = c.M
    x, b = _signed_start(c)
    keep = np.maximum(x.reshape(c.Nx, -1)[:, c.dead_pix], 0)
    t = engine(monkeypatch, c.ang, c.N, c.Nx, A=c.A)
    assert_ready(t, c)
    t.set_tilt_series(b)
    for kind, beta in (("tomo_sirt", None), ("landweber", 0.01), ("cimmino", 0.5)):
        t.set_volume(x, VOL_RECON)
        if kind == "tomo_sirt":
            t.be.c("sirt", VOL_RECON, 1)
            ref, bound = M.tomo_sirt_step(x, b)
        elif kind == "landweber":
            t.be.c("sirt_landweber", VOL_RECON, beta, 1)
            ref, bound = M.landweber_step(x, b, beta)
        else:
            t.be.c("sirt_cimmino", VOL_RECON, beta, 1)
            ref, bound = M.cimmino_step(x, b, beta)
        got = t.get_volume()
        _note(kind, got, ref, bound)
        ref64.assert_within(f"{name} {gid} {kind}", got, ref, bound)
        assert np.array_equal(got.reshape(c.Nx, -1)[:, c.dead_pix], keep), kind     # colsum <= 0: max(0, x), exactly
    # the host tables (in the negated angle weight and row sum are both negative: every term of A^T (A 1) stays positive)
    ref64.assert_scalar("lipschitz", t.get_lipschitz(), *M.lipschitz())
    t.cimminos_method()
    ref64.assert_scalar("lipschitz cimmino", t.lipschits(), *M.lipschitz(cimmino=True))


SIRT_BP = [(f, g, m) for f, g, m in BP_CASES if f in ("dead", "signed", "messy")]


@pytest.mark.parametrize("name,gid,form", SIRT_BP, ids=[f"{f}-{g}-bp_{m}" for f, g, m in SIRT_BP])
def test_tomo_sirt_column_rule_in_every_bp_form(gpu, monkeypatch, name, gid, form):
    """The colsum > 0 rule of the list, tile and voxel-driven back projectors (k_bp_list, k_bp_tile, k_bp_all), each with pixels whose
    column sum is 0: one tomo_sirt step under its bound, those pixels max(0, x) exactly."""
    c = case(name, gid)
    x, b = _signed_start(c)
    keep = np.maximum(x.reshape(c.Nx, -1)[:, c.dead_pix], 0)
    t = engine(monkeypatch, c.ang, c.N, c.Nx, bp=form, A=c.A)      # (asserts form_bp)
    t.set_tilt_series(b)
    t.set_volume(x, VOL_RECON)
    t.be.c("sirt", VOL_RECON, 1)
    ref, bound = c.M.tomo_sirt_step(x, b)
    got = t.get_volume()
    _note(f"tomo_sirt bp_{form}", got, ref, bound)
    ref64.assert_within(f"{name} {gid} tomo_sirt bp_{form}", got, ref, bound)
    assert np.array_equal(got.reshape(c.Nx, -1)[:, c.dead_pix], keep)


# ---- SART sweeps ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,gid,form", SART_CASES, ids=[f"{f}-{g}-sart_{m}" for f, g, m in SART_CASES])
def test_sart_sweep_on_a_user_matrix(gpu, monkeypatch, name, gid, form):
    """One sweep in natural order and one in a seeded order (tomo_sart's order argument) under the oracle's yardstick; pixels no angle
    crosses keep max(0, x) exactly."""
    c = case(name, gid)
    M = c.M
    x, b = _step_data(M, c.Nx)
    x = x.copy()
    x[::3].reshape(-1, M.ncol)[:, c.dead_pix] *= F32(-1)          # (pixels without rays: they enter no projection)
    keep = np.maximum(x.reshape(c.Nx, -1)[:, c.dead_pix], 0)
    sl = np.arange(c.Nx) if c.N <= 33 else np.array([0, 31, 63])
    t = engine(monkeypatch, c.ang, c.N, c.Nx, A=c.A)
    assert_ready(t, c)
    perm = np.random.default_rng(17).permutation(c.P)
    for o in (None, perm):
        got, _ = _sart_check(t, M, x, b, form, sl, order=o)
        assert np.array_equal(got.reshape(len(sl), -1)[:, c.dead_pix], keep[sl])


# the other instances of the rowsum > 0 rule in a sweep: st_resid_row (the rows formed inside the next tile step: "sart_coop", also with
# every workgroup forming its own) and k_resid_finish behind the fused ray-walk step, whose walk lists hold messy's explicit zeros and
# the orphans next to them
SART_MORE = [(f, g, m) for f, g in (("dead", "lin70"), ("signed", "lin70"), ("messy", "axes45"), ("messy", "repeat")) for m in ("coop", "coop_own", "walk")]


@pytest.mark.parametrize("name,gid,form", SART_MORE, ids=[f"{f}-{g}-sart_{m}" for f, g, m in SART_MORE])
def test_sart_sweep_cooperative_and_ray_walk_on_a_user_matrix(gpu, monkeypatch, name, gid, form):
    c = case(name, gid)
    M = c.M
    assert c.exp["sart_tile_ok"] == 1 and len(c.dead_rows)
    x, b = _step_data(M, c.Nx)
    x = x.copy()
    x[::3].reshape(-1, M.ncol)[:, c.dead_pix] *= F32(-1)
    keep = np.maximum(x.reshape(c.Nx, -1)[:, c.dead_pix], 0)
    t = engine(monkeypatch, c.ang, c.N, c.Nx, A=c.A)
    for o in (None, np.random.default_rng(17).permutation(c.P)):
        got, _ = _sart_check(t, M, x, b, form, np.arange(c.Nx), order=o)
        assert np.array_equal(got.reshape(c.Nx, -1)[:, c.dead_pix], keep)


@pytest.mark.parametrize("form", ["resident", "tile", "angle"])
def test_angles_without_a_positive_row_sum_leave_the_volume(gpu, monkeypatch, form):
    """A matrix of two angles, one removed and one negated (``user_matrices.idle_pair``): every normalised residual is 0 by the
    rowsum > 0 rule, so a SART sweep in either order and a tomo_sirt step leave max(0, x), bit for bit."""
    ang, N, Nx = GEOM["lin70"]
    ang = ang[:2]
    A = um.idle_pair(system_matrix(N, ang), N)
    M, _ = um.reference(N, ang, A)
    assert np.all(M.rowsum <= 0) and np.count_nonzero(M.rowsum < 0) == N and um.signs_are_safe(M)
    x = ref64.dense_volume(Nx, N, seed=21)
    x[::3, :, ::5] *= F32(-1)
    b = ref64.signed_sino(Nx, M.nrow, seed=22)
    assert np.all(b != 0)
    t = engine(monkeypatch, ang, N, Nx, A=A)
    assert t.get_option("sart_resident_ready") == um.EXPECTED_IDLE["sart_resident_ok"]
    for o in (None, np.array([1, 0])):
        got, _ = _sart_check(t, M, x, b, form, np.arange(Nx), order=o)
        assert np.array_equal(got, np.maximum(x, 0)), form
    t.set_volume(x, VOL_RECON)
    t.be.c("sirt", VOL_RECON, 1)
    assert np.array_equal(t.get_volume(), np.maximum(x, 0))
    assert not t._sino(SINO_R).any()


# ---- ART ------------------------------------------------------------------------------------------------------------------------------------
ART = [(f, g, v) for g in ("lin70", "axes45") for f in ("dead", "gain", "messy") for v in ("tile", "angle")] + \
      [("shuffled", "lin70", "rows"), ("shuffled", "axes45", "rows")]


def _art_oracle(c, x, b, sl, order=None):
    orc = oracle.ctvlib(len(sl), c.N, c.P)
    orc.load_A(c.A)                                                # the raw triplets
    orc.set_tilt_series(b[sl])
    orc.recon[:] = x[sl]
    orc.row_inner_product()
    orc.ART(0.6, order=order)
    return orc.recon


@pytest.mark.parametrize("name,gid,variant", ART, ids=[f"{f}-{g}-art_{v}" for f, g, v in ART])
def test_art_sweep_on_a_user_matrix(gpu, name, gid, variant):
    c = case(name, gid)
    M = c.M
    x, b = _step_data(M, c.Nx)
    sl = [0, c.Nx // 2, c.Nx - 1]
    t = ctvlib(c.Nx, c.N, c.P)
    t.load_A(c.A)
    t.set_option("art_chain", 1)
    t.set_option("art_tile", 0 if variant == "angle" else 1)
    assert t.get_option("art_chain_ready") == c.exp["art_chain_ok"] == (0 if variant == "rows" else 1)
    t.set_tilt_series(b)
    t.set_volume(x, VOL_RECON)
    t.row_inner_product()
    fused = launches(t, _lib.K_SART_FUSED, lambda: t.ART(0.6))
    if variant == "tile":
        assert fused > 0 and fused % (c.P - 1) == 0, fused
    else:
        # The launch log has no id for the ART kernels: the per-angle chain and the row-sequential kernel both show as "no fused
        # step".  What tells them apart is the engine's own condition for the chain, art_chain_ready (asserted above): 0 on the
        # shuffled rays, so tomo_art_order can only have launched k_art.
        assert fused == 0, fused
    ref = M.art(x[sl], b[sl], 0.6)
    print(f"ratio ART sweep: {ref64.ratio(t.get_volume()[sl], ref, ref64.seq_bound(_art_oracle(c, x, b, sl), ref)):.3f}")
    ref64.assert_seq(f"ART {variant}", t.get_volume()[sl], _art_oracle(c, x, b, sl), M.art(x[sl], b[sl], 0.6))


@pytest.mark.parametrize("name", ["own", "dead", "messy", "signed", "shuffled"])
def test_art_in_a_row_order(gpu, name):
    """tomo_art_order with a seeded row order (the row-sequential kernel), on lin70: the families, and the engine's own matrix with the
    chain switched off."""
    c = case("dead" if name == "own" else name, "lin70")
    A = c.own if name == "own" else c.A
    M = ref64.Matrix(c.N, c.ang, A=um.canonical(A, c.N * c.N))
    x, b = _step_data(M, c.Nx)
    sl = [0, c.Nx // 2, c.Nx - 1]
    order = np.ascontiguousarray(np.random.default_rng(23).permutation(M.nrow), np.int32)
    t = ctvlib(c.Nx, c.N, c.P)
    t.load_A(A)
    t.set_option("art_chain", 0)
    t.set_tilt_series(b)
    t.row_inner_product()
    orc = oracle.ctvlib(len(sl), c.N, c.P)
    orc.load_A(A)
    orc.set_tilt_series(b[sl])
    orc.row_inner_product()
    for o in (order, None):
        t.set_volume(x, VOL_RECON)
        if o is None:
            t.ART(0.6)
        else:
            t.be.c("art_order", 0.6, _ptr(o))
        orc.recon[:] = x[sl]
        orc.ART(0.6, order=o)
        ref64.assert_seq(f"ART order {name}", t.get_volume()[sl], orc.recon, M.art(x[sl], b[sl], 0.6, order=o))


# ---- shuffled rays: the fallbacks, element-wise ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gid", ["lin70", "axes45"])
def test_shuffled_rays_run_the_fallback_kernels(gpu, monkeypatch, gid):
    """The ray-walk sweep of a user matrix (its tables built at creation: the engine has no angles to rebuild them from) and the
    voxel-driven back projector, through tomo_sart and tomo_sirt."""
    c = case("shuffled", gid)
    M = c.M
    x, b = _step_data(M, c.Nx)
    t = engine(monkeypatch, c.ang, c.N, c.Nx, bp="all", A=c.A)
    assert t.get_option("form_bp") == BP_ALL and t.get_option("form_sart") == SART_ANGLE and t.get_option("sart_resident_ready") == 0
    t.set_tilt_series(b)
    t.set_volume(x, VOL_RECON)
    n = launches(t, _lib.K_SART_FUSED, lambda: t.be.c("sart", VOL_RECON, 0.7, 1, None))
    assert n > 0                                                   # the fused ray-walk steps, not one FP + one BP per angle
    orc = oracle.ctvlib(c.Nx, c.N, c.P)
    orc.load_A(c.A)
    orc.set_tilt_series(b)
    orc.recon[:] = x
    orc.SART(0.7, 1)
    ref64.assert_seq("SART ray-walk", t.get_volume(), orc.recon, M.sart(x, b, 0.7))
    t.set_volume(x, VOL_RECON)
    t.be.c("sirt", VOL_RECON, 1)
    ref, bound = M.tomo_sirt_step(x, b)
    ref64.assert_within("tomo_sirt (BP all)", t.get_volume(), ref, bound)


# ---- preconditioned PDHG ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,gid", [(f, g) for f in ("dead", "signed") for g in ("lin70", "axes45")])
def test_preconditioned_pdhg_on_a_user_matrix(gpu, name, gid):
    c = case(name, gid)
    M = c.M
    nx = 65
    t = ctvlib(nx, c.N, c.P)
    t.load_A(c.A)
    rowsum, colsum = R.tables_f32(M)
    assert np.array_equal(rowsum <= 0, M.rowsum <= 0) and np.array_equal(colsum == 0, M.colsum == 0)
    q, g, b = (ref64.signed_sino(nx, M.nrow, s + nx) for s in (1, 2, 3))
    QS, GS, BS = SINO_USER0, SINO_USER0 + 1, SINO_USER0 + 2
    for slot, v in ((QS, q), (GS, g), (BS, b)):
        t.be.c("set_sinogram", slot, _ptr(v))
    ref, bound = R.sino_dual_bound(q, g, b, rowsum=rowsum)
    t.pdhg_sino_dual(QS, GS, BS, sigma=0.07, precond=True)
    got = t._sino(QS)
    _note("pdhg_sino_dual", got, ref, bound)
    ref64.assert_within("sino_dual", got, ref, bound)
    assert np.array_equal(got[:, c.dead_rows], q[:, c.dead_rows])  # S = 0 exactly: q <- (q + 0) / 1
    lam = 0.5
    x, xbar, u, p = dense_inputs(nx, c.N, lam, 7)
    put(t, x=x, xbar=xbar, u=u, p=p)
    ref, bound = R.tv_step_bound(x, xbar, u, p, 0.5, lam, 1.0, colsum=colsum)
    t.pdhg_tv_step(X, XBAR, UVOL, P0, sigma=0.3, tau=0.2, lam=lam, theta=1.0, precond=True)
    for nm, gg, rr, bb in zip(("x", "xbar", "p"), (t.get_volume(X), t.get_volume(XBAR), get_p(t)), ref, bound):
        _note(f"pdhg_tv_step {nm}", gg, rr, bb)
        ref64.assert_within(f"tv_step {nm}", gg, rr, bb)


# ---- update_proj_angles -------------------------------------------------------------------------------------------------------------------
def test_update_proj_angles_to_a_user_matrix_keeps_the_volume(gpu, monkeypatch):
    c = case("dead", "lin70")
    t = ctvlib(c.Nx, c.N, c.P)
    t.load_A(c.own)
    x = ref64.dense_volume(c.Nx, c.N, seed=3)
    t.set_volume(x, VOL_RECON)
    t.update_proj_angles(c.A, c.P)
    assert np.array_equal(t.get_volume().view(np.uint32), x.view(np.uint32))
    assert_ready(t, c)
    onehot_fp(t, c.M, c.Nx, np.arange(c.M.ncol))
    t.set_volume(x, VOL_RECON)
    t.forward_projection()
    y64, bound, _ = c.M.fp_bound(x)
    ref64.assert_within("FP of the kept volume", t.get_model_projections(), y64, bound)
