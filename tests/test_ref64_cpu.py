"""The binary64 reference (tests/ref64.py) and its per-element bounds: the float32 oracle passes every bound on the geometries the
GPU element-wise tests use, and every check fails on oracle outputs that were deliberately corrupted (a lost, mis-weighted or
misplaced entry, slices swapped or lost, a SART angle swapped or skipped, a TV / FGP step with a different boundary rule on one face).
"""
import numpy as np
import pytest

import oracle
import ref64
from tomo_tv_amd.engine import system_matrix

# (angle set, N, slices): the angle sets of tests/test_gpu_elementwise.py at CPU-sized N
ANGLES = {
    "lin70": np.linspace(-70, 70, 9),
    "axes45": np.array([-90.0, -67.0, -45.0, -20.0, 0.0, 20.0, 45.0, 67.0, 90.0]),
    "half180": np.arange(0.0, 181.0, 1.0),
    "dose_sym": np.array([0.0] + [s * a for a in range(3, 61, 3) for s in (1, -1)]),
    "repeat": np.array([-40.0, -10.0, 15.0, 15.0, 50.0]),
    "neg150": np.linspace(-150, -30, 11),
    "p1_45": np.array([45.0]),
    "p1_90": np.array([90.0]),
}
CASES = [("lin70", 32, 3), ("axes45", 31, 2), ("half180", 8, 2), ("dose_sym", 33, 2), ("repeat", 16, 3), ("neg150", 32, 2),
         ("p1_45", 8, 3), ("p1_90", 33, 2)]


def _setup(name, N, nx):
    ang = ANGLES[name]
    A = system_matrix(N, ang)
    M = ref64.Matrix(N, ang, A=A)
    orc = oracle.ctvlib(nx, N, ang.size)
    orc.load_A(A)
    return M, orc


@pytest.mark.parametrize("name,N,nx", CASES, ids=[c[0] for c in CASES])
def test_oracle_within_projector_bounds(name, N, nx):
    M, orc = _setup(name, N, nx)
    assert M.duplicates == 0
    x = ref64.dense_volume(nx, N, seed=1)
    orc.original_volume = x.copy()
    orc.create_projections()
    y64, bound, ax = M.fp_bound(x)
    ref64.assert_within("oracle FP", orc.b, y64, bound)
    ref64.assert_typical("oracle FP", orc.b, orc.b, y64, ax)
    r = ref64.signed_sino(nx, M.nrow, seed=2)
    v64, vb, ar = M.bp_bound(r)
    v = orc.back_projection(r)
    ref64.assert_within("oracle BP", v, v64, vb)
    ref64.assert_typical("oracle BP", v, v, v64, ar)


@pytest.mark.parametrize("name,N,nx", CASES[:4], ids=[c[0] for c in CASES[:4]])
def test_oracle_within_step_bounds(name, N, nx):
    """tomo_sirt (row / column normalised), Landweber and Cimmino steps under the carried first-order bound; SART sweep, tv_gd and
    FGP under the oracle yardstick (which the oracle meets by construction: here the binary64 ports are checked against it)."""
    M, orc = _setup(name, N, nx)
    x = ref64.dense_volume(nx, N, seed=3)
    b = (M.fp(ref64.dense_volume(nx, N, seed=4)) * 1.02).astype(np.float32)
    orc.set_tilt_series(b)
    for kind in ("norm", "landweber", "cimmino"):
        orc.recon[:] = x
        if kind == "norm":
            orc.SIRT_norm(1)
            ref, bound = M.tomo_sirt_step(x, b)
        elif kind == "landweber":
            orc.SIRT(0.01)
            ref, bound = M.landweber_step(x, b, 0.01)
        else:
            orc.cimminos_method()
            orc.SIRT(0.5)
            ref, bound = M.cimmino_step(x, b, 0.5)
        ref64.assert_within(kind, orc.recon, ref, bound)
    order = np.random.default_rng(5).permutation(M.P).astype(np.int32)
    orc.recon[:] = x
    orc.SART(0.7, 1, order=order)
    s64 = M.sart(x, b, 0.7, order)
    assert np.abs(orc.recon - s64).max() <= 1e-4 * np.abs(s64).max()
    ref64.assert_seq("oracle SART", orc.recon, orc.recon, s64)
    orc.recon[:] = x
    orc.row_inner_product()
    orc.ART(0.6)
    a64 = M.art(x, b, 0.6)
    assert np.abs(orc.recon - a64).max() <= 1e-4 * np.abs(a64).max()


def test_tv_ports_match_the_oracle():
    nx, N = 5, 12
    x = ref64.dense_volume(nx, N, seed=6)
    orc = oracle.ctvlib(nx, N, 1)
    t64 = ref64.tv_gd(x, 2, 0.3, 1e-6)
    orc.tv_eps = 1e-6                                  # (the oracle's own binary64 descent takes eps from tv_eps)
    f64_c = orc.tv_gd_f64(2, 0.3, start=x)
    assert np.array_equal(t64.astype(np.float32), f64_c) or np.abs(t64 - f64_c).max() <= ref64.U * np.abs(t64).max()
    orc.recon[:] = x
    orc.tv_fgp(3, 0.05)
    g64 = ref64.tv_fgp(x, 3, 0.05)
    assert np.abs(orc.recon - g64).max() <= 1e-5 * np.abs(g64).max()


# ---- the checks have teeth ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fp_case():
    N, nx = 16, 4
    ang = np.linspace(-60, 60, 5)
    A = system_matrix(N, ang)
    M = ref64.Matrix(N, ang, A=A)
    orc = oracle.ctvlib(nx, N, ang.size)
    orc.load_A(A)
    x = ref64.dense_volume(nx, N, seed=7)
    orc.original_volume = x.copy()
    orc.create_projections()
    r = ref64.signed_sino(nx, M.nrow, seed=8)
    return M, x, orc.b.copy(), r, orc.back_projection(r)


def _border_entry(M, wmin=0.05):
    y, z = M.cols // M.N, M.cols % M.N
    border = (y == 0) | (z == 0) | (y == M.N - 1) | (z == M.N - 1)
    k = np.nonzero(border & (M.w32 >= wmin))[0]
    return int(k[len(k) // 2])


def _corruptions(arr, M, k, fwd, data):
    """The four corrupted copies of an FP (fwd) or BP output."""
    out = {}
    rr, cc, w = int(M.rows[k]), int(M.cols[k]), M.w32[k]
    lost = arr.reshape(len(arr), -1).copy()
    scaled = lost.copy()
    big = int(np.argmax(M.w32))
    rb, cb, wb = int(M.rows[big]), int(M.cols[big]), M.w32[big]
    src = data.reshape(len(data), -1)
    if fwd:
        lost[:, rr] -= w * src[:, cc]
        scaled[:, rb] += np.float32(wb * 2.0 ** -10) * src[:, cb]
    else:
        lost[:, cc] -= w * src[:, rr]
        scaled[:, cb] += np.float32(wb * 2.0 ** -10) * src[:, rb]
    out["lost_border_entry"] = lost.reshape(arr.shape)
    out["weight_scaled"] = scaled.reshape(arr.shape)
    sw = arr.copy()
    sw[[1, 2]] = sw[[2, 1]]
    out["slices_swapped"] = sw
    z = arr.copy()
    z[-1] = 0
    out["last_slice_zero"] = z
    return out


@pytest.mark.parametrize("kind", ["lost_border_entry", "weight_scaled", "slices_swapped", "last_slice_zero"])
def test_projector_bounds_catch_corruption(fp_case, kind):
    M, x, y, r, v = fp_case
    k = _border_entry(M)
    y64, yb, _ = M.fp_bound(x)
    v64, vb, _ = M.bp_bound(r)
    ref64.assert_within("FP", y, y64, yb)              # the clean outputs pass ...
    ref64.assert_within("BP", v, v64, vb)
    with pytest.raises(AssertionError):                # ... the corrupted ones do not
        ref64.assert_within("FP", _corruptions(y, M, k, True, x)[kind], y64, yb)
    with pytest.raises(AssertionError):
        ref64.assert_within("BP", _corruptions(v, M, k, False, r)[kind], v64, vb)


def test_typical_check_catches_a_worse_accumulation(fp_case):
    """An accumulation that loses a few bits everywhere (every sum rounded to 20 bits) passes the worst-case bound but not the typical one."""
    M, x, y, _, _ = fp_case
    y64, yb, ax = M.fp_bound(x)
    m, e = np.frexp(y64)
    coarse = np.ldexp(np.round(m * 2.0 ** 20) / 2.0 ** 20, e).astype(np.float32)
    ref64.assert_typical("FP", y, y, y64, ax)
    with pytest.raises(AssertionError):
        ref64.assert_typical("FP", coarse, y, y64, ax)


@pytest.fixture(scope="module")
def sart_case():
    N, nx = 16, 3
    ang = np.array([0.0, 3.0, -3.0, 6.0, -6.0, 9.0, -9.0])
    A = system_matrix(N, ang)
    M = ref64.Matrix(N, ang, A=A)
    orc = oracle.ctvlib(nx, N, ang.size)
    orc.load_A(A)
    x = ref64.dense_volume(nx, N, seed=9)
    b = (M.fp(ref64.dense_volume(nx, N, seed=10))).astype(np.float32)
    orc.set_tilt_series(b)
    orc.recon[:] = x
    orc.SART(0.8, 1)
    return M, x, b, orc.recon.copy(), M.sart(x, b, 0.8)


@pytest.mark.parametrize("kind", ["swap_two_angles", "skip_one_angle"])
def test_sart_yardstick_catches_a_wrong_order(sart_case, kind):
    M, x, b, got, s64 = sart_case
    ref64.assert_seq("SART", got, got, s64)
    order = list(range(M.P))
    if kind == "swap_two_angles":
        order[2], order[3] = order[3], order[2]
    else:
        del order[4]
    bad = M.sart(x, b, 0.8, order).astype(np.float32)
    with pytest.raises(AssertionError):
        ref64.assert_seq("SART", bad, got, s64)


@pytest.mark.parametrize("axis,side", [(a, s) for a in range(3) for s in ("lo", "hi")])
def test_tv_yardsticks_catch_a_wrong_boundary_rule_on_one_face(axis, side):
    nx, N = 6, 10
    x = ref64.dense_volume(nx, N, seed=11)
    orc = oracle.ctvlib(nx, N, 1)
    orc.tv_eps = 1e-6
    orc.recon[:] = x
    orc.tv_gd(1, 0.2)
    t64 = ref64.tv_gd(x, 1, 0.2, 1e-6)
    ref64.assert_seq("tv_gd", orc.recon, orc.recon, t64)
    with pytest.raises(AssertionError):
        ref64.assert_seq("tv_gd", ref64.tv_gd(x, 1, 0.2, 1e-6, wrong_face=(axis, side)).astype(np.float32), orc.recon, t64)
    orc.recon[:] = x
    orc.tv_fgp(2, 0.05)
    g64 = ref64.tv_fgp(x, 2, 0.05)
    ref64.assert_seq("fgp", orc.recon, orc.recon, g64)
    with pytest.raises(AssertionError):
        ref64.assert_seq("fgp", ref64.tv_fgp(x, 2, 0.05, wrong_face=(axis, side)).astype(np.float32), orc.recon, g64)


# ---- FP epilogues, scalar reductions, fusion steps -------------------------------------------------------------------------------------
F32 = np.float32


def _orc_fp(M, x):
    """The float32 oracle's A x."""
    orc = oracle.ctvlib(len(x), M.N, M.P)
    orc.A = oracle.CSR(M.nrow, M.ncol, *M.csr())
    orc.original_volume = np.ascontiguousarray(x, F32)
    orc.create_projections()
    return orc, orc.b.copy()


def _orc_epilogues(M, x, b):
    """The five epilogues in float32 from the oracle's projection (the kernels' expressions)."""
    orc, a = _orc_fp(M, x)
    rs32 = _orc_fp(M, np.ones((1, M.N, M.N), F32))[1][0]          # A 1 in float32
    orc.row_inner_product()
    d = (b - a).astype(F32)
    with np.errstate(divide="ignore", invalid="ignore"):
        norm = np.where(rs32 > 0, d / rs32, F32(0)).astype(F32)
    mul = (d * orc.innerProduct).astype(F32)
    dd = float(np.sum(((a - b).astype(F32) ** 2).astype(np.float64)))
    eps = F32(0.1)
    pr = ((a - b) / (a + eps)).astype(F32)
    cost = float(np.sum((a - b * np.log(a + eps, dtype=F32)).astype(np.float64)))
    return dict(a=a, resid=d, norm=norm, mul=mul, dd=dd, pr=pr, cost=cost, rs32=rs32)


def _poisson_data(M, nx, seed):
    b = np.abs(ref64.signed_sino(nx, M.nrow, seed=seed)) * F32(M.N / 4)
    b[:, ::7] = 0                                                   # rows where b is 0
    return b.astype(F32)


@pytest.mark.parametrize("name,N,nx", CASES, ids=[c[0] for c in CASES])
def test_oracle_within_epilogue_bounds(name, N, nx):
    M, _ = _setup(name, N, nx)
    x = ref64.dense_volume(nx, N, seed=12)
    b = ref64.signed_sino(nx, M.nrow, seed=13)
    o = _orc_epilogues(M, x, b)
    for mode, key in (("resid", "resid"), ("norm", "norm"), ("mul", "mul")):
        ref, bound = M.residual(x, b, mode)
        ref64.assert_within(mode, o[key], ref, bound)
    zero = M.rowsum == 0
    assert np.all(o["norm"][:, zero] == 0)
    g, eg, s, es = M.data_distance(x, b)
    ref64.assert_within("G", o["a"], g, eg)
    ref64.assert_scalar("S_DD", o["dd"], s, es)
    bp = _poisson_data(M, nx, 14)
    o = _orc_epilogues(M, x, bp)
    r, er, c, ec = M.poisson(x, bp)
    ref64.assert_within("poisson residual", o["pr"], r, er)
    ref64.assert_scalar("S_COST", o["cost"], c, ec)


@pytest.fixture(scope="module")
def epi_case():
    M, _ = _setup("lin70", 32, 3)
    x = ref64.dense_volume(3, 32, seed=15)
    b = ref64.signed_sino(3, M.nrow, seed=16)
    return M, x, b, _orc_epilogues(M, x, b)


EPI_CORRUPT = [("resid", "sign_flip"), ("norm", "sign_flip"), ("mul", "sign_flip"), ("norm", "neighbour_rowsum"),
               ("mul", "neighbour_rowsum")]


@pytest.mark.parametrize("mode,kind", EPI_CORRUPT, ids=[f"{m}-{k}" for m, k in EPI_CORRUPT])
def test_epilogue_bounds_catch_corruption(epi_case, mode, kind):
    M, x, b, o = epi_case
    ref, bound = M.residual(x, b, mode)
    good = o[mode]
    ref64.assert_within(mode, good, ref, bound)
    bad = good.copy()
    if kind == "sign_flip":
        i = int(np.argmax(np.abs(good[1])))
        bad[1, i] = -bad[1, i]
    else:
        f = o["rs32"] if mode == "norm" else (M.rowinner.astype(F32))
        fn = np.roll(f, 1)                                          # the neighbouring row's factor
        d = o["resid"]
        with np.errstate(divide="ignore", invalid="ignore"):
            bad = np.where(fn > 0, d / fn, 0).astype(F32) if mode == "norm" else (d * fn).astype(F32)
    with pytest.raises(AssertionError):
        ref64.assert_within(mode, bad, ref, bound)


def test_poisson_and_dd_bounds_catch_corruption(epi_case):
    M, x, _, _ = epi_case
    bp = _poisson_data(M, 3, 17)
    o = _orc_epilogues(M, x, bp)
    r, er, c, ec = M.poisson(x, bp)
    bad = o["pr"].copy()
    i = int(np.argmax(np.abs(bad[2])))
    bad[2, i] = -bad[2, i]
    with pytest.raises(AssertionError):
        ref64.assert_within("poisson", bad, r, er)
    a = o["a"]
    k = int(np.argmax(a[0]))
    term = float(a[0, k]) - float(bp[0, k]) * float(np.log(np.float64(a[0, k]) + ref64.EPS_POISSON))
    with pytest.raises(AssertionError):                              # one term left out of the cost
        ref64.assert_scalar("S_COST", o["cost"] - term, c, ec)
    _, _, s, es = M.data_distance(x, bp)
    d = (a - bp).astype(np.float64)
    with pytest.raises(AssertionError):                              # the last real slice left out
        ref64.assert_scalar("S_DD", o["dd"] - float(np.sum(d[-1] ** 2)), s, es)


def _f32_sqdiff_terms(a, b):
    return (((a - b).astype(F32)) ** 2).astype(F32).astype(np.float64)


def _tv_terms_f32(x, eps):
    """The float32 TV value terms of k_tv_value / orc_tv."""
    x = np.asarray(x, F32)
    s = (F32(eps) + ((x - np.roll(x, -1, 0)) ** 2).astype(F32)).astype(F32)
    s = (s + ((x - np.roll(x, -1, 1)) ** 2).astype(F32)).astype(F32)
    s = (s + ((x - np.roll(x, -1, 2)) ** 2).astype(F32)).astype(F32)
    return np.sqrt(s).astype(np.float64)


def _tv_grad_f32(x, eps):
    """The TV gradient of ctvlib.cpp:431-447 evaluated in float32 (every operation rounded), the kernels' expression."""
    x = np.asarray(x, F32)
    eps = F32(eps)

    def S(a, ax, d):
        return np.roll(a, -d, ax)

    def D(c, a1, a2, a3):
        return np.sqrt(eps + (c - a1) * (c - a1) + (c - a2) * (c - a2) + (c - a3) * (c - a3))
    c = x
    xp, yp, zp = S(x, 0, 1), S(x, 1, 1), S(x, 2, 1)
    xm, ym, zm = S(x, 0, -1), S(x, 1, -1), S(x, 2, -1)
    g = (((c - xp) + (c - yp)) + (c - zp)) / D(c, xp, yp, zp)
    g = g + (c - xm) / D(xm, c, S(xm, 1, 1), S(xm, 2, 1))
    g = g + (c - ym) / D(ym, S(ym, 0, 1), c, S(ym, 2, 1))
    g = g + (c - zm) / D(zm, S(zm, 0, 1), S(zm, 1, 1), c)
    return g.astype(F32)


REDUCTION_SHAPES = [(5, 12), (66, 8), (3, 9)]


@pytest.mark.parametrize("nx,N", REDUCTION_SHAPES)
def test_oracle_within_reduction_bounds(nx, N):
    x = ref64.with_sentinels(ref64.dense_volume(nx, N, seed=18))
    y = ref64.dense_volume(nx, N, seed=19)
    s, es = ref64.sqdiff(x, y)
    ref64.assert_scalar("S_DIFF", float(np.sum(_f32_sqdiff_terms(x, y))), s, es)
    s, es = ref64.l1(x - F32(1.0))
    ref64.assert_scalar("S_L1", float(np.sum(np.abs((x - F32(1.0)).astype(np.float64)))), s, es)
    orc = oracle.ctvlib(nx, N, 1)
    orc.tv_eps = 1e-6
    orc.recon[:] = x
    s, es = ref64.tv_value(x, 1e-6)
    ref64.assert_scalar("S_TV", orc.tv(), s, es)
    ref64.assert_scalar("S_TV", float(np.sum(_tv_terms_f32(x, 1e-6))), s, es)
    g32 = _tv_grad_f32(x, 1e-6).astype(np.float64)
    s, es = ref64.tv_gnorm(x, 1e-6)
    ref64.assert_scalar("S_GNORM", float(np.sum((g32 * g32).astype(F32).astype(np.float64))), s, es)


def test_tv_gd_still_matches_the_oracle_after_factoring_the_gradient():
    nx, N = 4, 10
    x = ref64.dense_volume(nx, N, seed=20)
    orc = oracle.ctvlib(nx, N, 1)
    orc.tv_eps = 1e-6
    f64_c = orc.tv_gd_f64(2, 0.3, start=x)
    t64 = ref64.tv_gd(x, 2, 0.3, 1e-6)
    assert np.abs(t64 - f64_c).max() <= ref64.U * np.abs(t64).max()


@pytest.mark.parametrize("kind", ["drop_float4", "drop_last_slice", "double_last_slice", "drop_sentinel_chunk2"])
def test_reduction_bounds_catch_dropped_or_doubled_terms(kind):
    """One float4 group (4 consecutive slices of one pixel, the volume's storage order), the last real slice, or the sentinel at the
    start of the second 64-slice chunk, dropped from or added twice to S_DIFF, S_L1, S_TV and S_GNORM."""
    nx, N = 66, 8
    x = ref64.with_sentinels(ref64.dense_volume(nx, N, seed=21))
    y = ref64.dense_volume(nx, N, seed=22)
    terms = {"S_DIFF": (_f32_sqdiff_terms(x, y), ref64.sqdiff(x, y)),
             "S_L1": (np.abs(x.astype(np.float64)), ref64.l1(x)),
             "S_TV": (_tv_terms_f32(x, 1e-6), ref64.tv_value(x, 1e-6))}
    g32 = _tv_grad_f32(x, 1e-6).astype(np.float64)
    terms["S_GNORM"] = ((g32 * g32).astype(F32).astype(np.float64), ref64.tv_gnorm(x, 1e-6))
    for name, (t, (s, es)) in terms.items():
        ref64.assert_scalar(name, float(np.sum(t)), s, es)
        if kind == "drop_float4":
            delta = -float(np.sum(t[0:4, 0, 0]))                        # the float4 of pixel 0 holding the first sentinel
        elif kind == "drop_last_slice":
            delta = -float(np.sum(t[-1]))
        elif kind == "double_last_slice":
            delta = float(np.sum(t[-1]))
        else:
            delta = -float(t[64, 0, 0])
        assert abs(delta) > 10 * es, (name, kind, delta, es)          # the sentinels keep the margin wide
        with pytest.raises(AssertionError):
            ref64.assert_scalar(name, float(np.sum(t)) + delta, s, es)


def test_tv_value_catches_a_clamped_face():
    nx, N = 6, 10
    x = ref64.with_sentinels(ref64.dense_volume(nx, N, seed=23))
    s, es = ref64.tv_value(x, 1e-6)
    for axis in range(3):
        bad, _ = ref64.tv_value(x, 1e-6, wrong_face=(axis, "hi"))
        with pytest.raises(AssertionError):
            ref64.assert_scalar("S_TV", bad, s, es)
        gbad, _ = ref64.tv_gnorm(x, 1e-6, wrong_face=(axis, "hi"))
        s2, es2 = ref64.tv_gnorm(x, 1e-6)
        with pytest.raises(AssertionError):
            ref64.assert_scalar("S_GNORM", gbad, s2, es2)


# ---- fusion kernels ----------------------------------------------------------------------------------------------------------------
def fusion_volumes(nel, shape, seed, negative=False):
    """Per-element volumes with exact zeros, subnormals, values down to 1e-30 and up to 1e3 (and negative voxels if asked)."""
    rng = np.random.default_rng(seed)
    xs = []
    for e in range(nel):
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


def _mm_model_f32(xs, w, g):
    """oracle/multimodal.py: model()."""
    acc = np.zeros(xs[0].shape, F32)
    for e in range(len(xs)):
        acc = (acc + F32(w[e]) * (xs[e] if g == 1 else np.power(xs[e], F32(g), dtype=F32))).astype(F32)
    return acc


def _mm_update_f32(xs, us, w, g, c, lamH, upd=None, model=None, corrupt=None):
    """oracle/multimodal.py: the updates of data_fusion (lamH != 0) and poisson_ml (lamH == 0), in float32."""
    out = []
    g, c, lamH = F32(g), F32(c), F32(lamH)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for e in range(len(xs)):
            x, u = xs[e], us[e]
            if lamH == 0:
                v = (x - (c * u).astype(F32)).astype(F32)
            else:
                uh = (F32(w[e]) * (upd - model).astype(F32)).astype(F32)
                if g != 1:
                    pw = np.power(x, g if corrupt == "pow_gamma" else g - F32(1.0), dtype=F32)
                    uh = ((g * pw).astype(F32) * uh).astype(F32)
                v = (x - ((c * u).astype(F32) - (lamH * uh).astype(F32))).astype(F32)
            out.append(v if corrupt == "no_clamp" else np.fmax(v, F32(0)))
    return out


@pytest.mark.parametrize("g", [1.0, 1.6, 2.0, 0.5])
@pytest.mark.parametrize("nel", [1, 3, 8])
def test_oracle_within_fusion_bounds(nel, g):
    shape = (3, 8, 8)
    w = np.linspace(0.3, 1.7, nel).astype(F32)
    xs = fusion_volumes(nel, shape, seed=nel * 10, negative=(g == 2.0))
    ref, bound = ref64.mm_model(xs, w, g)
    ref64.assert_within("model", _mm_model_f32(xs, w, g), ref, bound)
    xs = fusion_volumes(nel, shape, seed=nel * 10 + 1)
    rng = np.random.default_rng(nel)
    us = [rng.uniform(-2, 2, shape).astype(F32) for _ in range(nel)]
    upd, model = rng.uniform(0, 3, shape).astype(F32), rng.uniform(0, 3, shape).astype(F32)
    upd.reshape(-1)[:8] = model.reshape(-1)[:8]                       # D == 0 at a zero voxel as well
    for lamH in (0.0, 0.7):
        got = _mm_update_f32(xs, us, w, g, 0.05, lamH, upd, model)
        for e, (r, b) in enumerate(ref64.mm_update(xs, us, w, g, 0.05, lamH, upd, model)):
            fin = np.isfinite(r)
            assert np.array_equal(got[e][~fin], r[~fin]), (e, lamH)
            ref64.assert_within(f"update e{e} lamH {lamH}", got[e][fin], r[fin], b[fin])


@pytest.mark.parametrize("kind", ["swap_weights", "pow_gamma", "no_clamp"])
def test_fusion_bounds_catch_corruption(kind):
    nel, shape, g = 3, (2, 8, 8), 1.6
    w = np.array([0.2, 0.5, 0.9], F32)
    xs = fusion_volumes(nel, shape, seed=5)
    rng = np.random.default_rng(6)
    us = [rng.uniform(-2, 2, shape).astype(F32) for _ in range(nel)]
    upd, model = rng.uniform(0, 3, shape).astype(F32), rng.uniform(0, 3, shape).astype(F32)
    if kind == "swap_weights":
        ref, bound = ref64.mm_model(xs, w, g)
        ref64.assert_within("model", _mm_model_f32(xs, w, g), ref, bound)
        with pytest.raises(AssertionError):
            ref64.assert_within("model", _mm_model_f32(xs, w[[1, 0, 2]], g), ref, bound)
        return
    refs = ref64.mm_update(xs, us, w, g, 0.05, 0.7, upd, model)
    bad = _mm_update_f32(xs, us, w, g, 0.05, 0.7, upd, model, corrupt=kind)
    with pytest.raises(AssertionError):
        for e, (r, b) in enumerate(refs):
            ref64.assert_within("update", bad[e], r, b)


def test_proj_max_and_scale_are_exact_and_catch_the_padding():
    """k_proj_max leaves the padding slices out: on a sinogram whose projections are all negative, a max that counted the (zero)
    padding would return 0."""
    P, N, nx = 4, 6, 5
    rng = np.random.default_rng(7)
    s = rng.uniform(-3, 2, (nx, P * N)).astype(F32)
    s[:, N:2 * N] = -np.abs(s[:, N:2 * N]) - F32(0.5)                 # projection 1 all negative
    m = ref64.proj_max(s, P, N)
    assert m[1] < 0 and np.array_equal(m, s.reshape(nx, P, N).max(axis=(0, 2)))
    padded = np.maximum(m, 0)
    assert not np.array_equal(padded, m)
    div, mul = m + F32(5), np.linspace(0.5, 2, P).astype(F32)
    out = ref64.proj_scale(s, P, N, div, mul)
    blk = (s.reshape(nx, P, N) / div[None, :, None]).astype(F32) * mul[None, :, None]
    assert np.array_equal(out, blk.astype(F32).reshape(nx, P * N))


@pytest.mark.parametrize("name,N", [("lin70", 32), ("axes45", 33), ("neg150", 32), ("p1_90", 16)])
def test_oracle_lipschitz_within_bound(name, N):
    M, orc = _setup(name, N, 1)
    L, eL = M.lipschitz()
    ref64.assert_scalar("lipschitz", orc.lipschits(), L, eL)
    orc.cimminos_method()
    L, eL = M.lipschitz(cimmino=True)
    ref64.assert_scalar("lipschitz_cimmino", orc.lipschits(), L, eL)
    with pytest.raises(AssertionError):                               # the second largest column instead
        v = np.bincount(M.cols, M.vals * (M.rowsum * M.rowinner)[M.rows], M.ncol)
        ref64.assert_scalar("lipschitz_cimmino", np.sort(v)[-2] if np.sort(v)[-2] != v.max() else v.max() * (1 - 1e-4), L, eL)


# ---- CGLS, the WBP row filter, the FISTA passes ----------------------------------------------------------------------------------------
# the one-step shapes of tests/test_gpu_elementwise_misc.py (N, P, slices)
CGLS_SHAPES = [(8, 3, 3), (9, 4, 130), (8, 3, 513), (8, 3, 1025), (33, 5, 449)]


def _cgls_setup(N, P, nx):
    ang = np.linspace(-70, 70, P)
    M = ref64.Matrix(N, ang)
    return M, ref64.cgls_sino(M, nx, seed=N + nx)


def _sumsq_f32(v, rpb=None, drop=None, phases=1):
    """k_slice_sumsq + _finish on (slices, rows): float32 squares summed in double.  ``drop = "last_block"``: the last (short) block of
    ``rpb`` rows left out; ``drop = "phase"``: the 8-row groups of row phase 1 of ``phases`` left out in every block."""
    m = v.shape[1]
    keep = np.ones(m, bool)
    if drop == "last_block":
        keep[(-(-m // rpb) - 1) * rpb:] = False
    elif drop == "phase":
        r = np.arange(m)
        keep[((r % rpb) // 8) % phases == 1] = False
    sq = (v * v).astype(F32).astype(np.float64)
    return sq[:, keep].sum(axis=1)


def _cgls_first_f32(M, b, coef=None, drop_z=None, drop_w=None, rpb_z=None, rpb_w=None, phases=1):
    """The first CGLS step from zero in float32 as the kernels form it; ``coef(alpha)``: the coefficient each slice is handed."""
    orc, _ = _orc_fp(M, np.zeros((len(b), M.N, M.N), F32))
    z = orc.back_projection(b)
    orc.recon[:] = z
    orc.forward_projection()
    w = orc.g.copy()
    gam = _sumsq_f32(z.reshape(len(b), -1), rpb_z, drop_z, phases)
    den = _sumsq_f32(w, rpb_w, drop_w, phases)
    alpha = np.where(den > 0, gam / np.where(den > 0, den, 1), 0).astype(F32)
    if coef is not None:
        alpha = coef(alpha)
    return np.maximum((alpha[:, None, None] * z).astype(F32), F32(0))


@pytest.mark.parametrize("N,P,nx", CGLS_SHAPES, ids=[f"N{c[0]}-nx{c[2]}" for c in CGLS_SHAPES])
def test_cgls_inputs_separate_alpha_and_the_f32_step_is_inside_its_bound(N, P, nx):
    M, b = _cgls_setup(N, P, nx)
    x1, bound, alpha, rel = M.cgls_first_step(b)
    zs = ref64.cgls_zero_slice(nx)
    assert zs % 4 == 1 and not b[zs].any() and alpha[zs] == 0 and np.count_nonzero(alpha == 0) == 1
    assert ref64.alpha_separation(alpha, rel) > 1.0
    sl = ref64.slice_sample(nx)
    assert {0, nx - 1, zs} <= set(sl.tolist()) and all(k in sl and k - 1 in sl for k in range(64, nx, 64))
    if nx >= 8:
        assert {int(s) % 4 for s in sl if s != zs} == {0, 1, 2, 3}            # every lane of a float4 group, the zero slice aside
    got = _cgls_first_f32(M, b)
    ref64.assert_within("cgls first step", got, x1, bound)
    assert not got[zs].any() and not x1[zs].any() and not bound[zs].any()
    # the same step through Matrix.cgls (alpha rounded to float32 there)
    xa, al, _ = M.cgls(None, b, 1, slices=sl)
    assert np.abs(xa - x1[sl]).max() <= 2 * ref64.U * np.abs(x1).max() and np.allclose(al[0], alpha[sl], rtol=2 * ref64.U, atol=0)


@pytest.fixture(scope="module")
def cgls_case():
    M, b = _cgls_setup(9, 4, 130)
    return (M, b) + M.cgls_first_step(b)


@pytest.mark.parametrize("kind", ["neighbour_slice", "neighbour_group", "one_grid_stride"])
def test_cgls_bound_catches_a_coefficient_from_the_wrong_slice(cgls_case, kind):
    """The coefficient of slice s + 1, of the next float4 group (s + 4), and of the group an unrounded capped grid would reach on its
    second trip ((8192 * 256) % (sx / 4) groups on, in the padded row of sx = 192 coefficients)."""
    M, b, x1, bound, alpha, rel = cgls_case
    nx, sx = len(b), 192
    shift = {"neighbour_slice": 1, "neighbour_group": 4, "one_grid_stride": 4 * ((8192 * 256) % (sx // 4))}[kind]
    assert shift % sx != 0

    def coef(a):
        pad = np.zeros(sx, F32)
        pad[:nx] = a
        return np.roll(pad, -shift)[:nx]
    bad = _cgls_first_f32(M, b, coef=coef)
    with pytest.raises(AssertionError):
        ref64.assert_within("cgls", bad, x1, bound)
    # ... and in every single slice on its own (the zero slice aside: any coefficient times z = 0 is 0)
    err = (np.abs(bad - x1) > bound).reshape(nx, -1).any(axis=1)
    zs = ref64.cgls_zero_slice(nx)
    assert err[np.arange(nx) != zs].all()


@pytest.mark.parametrize("kind", ["last_block_z", "last_block_w", "phase_z", "phase_w"])
def test_cgls_bound_catches_rows_left_out_of_the_slice_sums(kind):
    """N = 33: the pixel sum has 18 blocks of 61 rows, the last one short (52 rows); its row phases take alternate groups of 8 rows."""
    N, P, nx = 33, 5, 6
    M, b = _cgls_setup(N, P, nx)
    x1, bound, _, _ = M.cgls_first_step(b)
    mz, mw = N * N, N * P
    rz, rw = -(-mz // ((mz + 63) // 64)), -(-mw // ((mw + 63) // 64))
    assert (rz, mz - 17 * rz) == (61, 52)
    ref64.assert_within("cgls", _cgls_first_f32(M, b, rpb_z=rz, rpb_w=rw, phases=2), x1, bound)
    kw = dict(rpb_z=rz, rpb_w=rw, phases=2)
    kw["drop_" + kind[-1]] = "last_block" if kind.startswith("last") else "phase"
    with pytest.raises(AssertionError):
        ref64.assert_within("cgls", _cgls_first_f32(M, b, **kw), x1, bound)


def test_cgls_sequential_yardstick_catches_a_wrong_coefficient():
    N, P, nx = 8, 3, 9
    M, b = _cgls_setup(N, P, nx)
    x0 = (F32(0.1) * ref64.dense_volume(nx, N, seed=30)).astype(F32)
    orc, _ = _orc_fp(M, x0)

    def fp(v):
        orc.recon[:] = v
        orc.forward_projection()
        return orc.g.copy()
    good = ref64.cgls_f32(fp, orc.back_projection, x0, b, 3)
    x64, al, be = M.cgls(x0, b, 3)
    assert al.shape == (3, nx) and be.shape == (3, nx)
    ref64.assert_seq("cgls", good, good, x64)
    assert np.abs(good - x64).max() <= 1e-4 * np.abs(x64).max()
    sub, _, _ = M.cgls(x0, b, 3, slices=[2, 7])                        # the slices are independent
    assert np.array_equal(sub, x64[[2, 7]])
    bad = ref64.cgls_f32(fp, orc.back_projection, x0[[1, 0] + list(range(2, nx))], b, 3)   # two slices' starts exchanged
    with pytest.raises(AssertionError):
        ref64.assert_seq("cgls", bad, good, x64)
    sw = ref64.cgls_f32(fp, lambda r: np.roll(orc.back_projection(r), 1, axis=0), x0, b, 3)   # every slice handed its neighbour's z
    with pytest.raises(AssertionError):
        ref64.assert_seq("cgls", sw, good, x64)


def _filter_f32(b, taps, P, N, kind=None):
    """k_filter_rows in float32 (one multiply-add per tap, k ascending).  ``kind``: "tap_plus_one" reads h[|j - k| + 1] (0 past the
    end), "chunk0" lets the slices of the second 64-slice chunk read the first chunk's input, "next_projection" takes the last ray
    of a projection from the next one (the element one past the row)."""
    h = np.asarray(taps, F32)
    s = np.asarray(b, F32).reshape(len(b), P, N)
    if kind == "chunk0":
        s = s.copy()
        n2 = min(64, len(b) - 64)
        s[64:64 + n2] = s[:n2]
    hp = np.concatenate([h, [F32(0)]])
    out = np.zeros_like(s)
    for j in range(N):
        acc = np.zeros(s.shape[:2], F32)
        for k in range(N):
            d = abs(j - k) + (1 if kind == "tap_plus_one" else 0)
            col = s[:, :, k]
            if kind == "next_projection" and k == N - 1:
                col = np.roll(s[:, :, 0], -1, axis=1)
            acc = (acc + (hp[d] * col).astype(F32)).astype(F32)
        out[:, :, j] = acc
    return out.reshape(len(b), P * N)


def _random_taps(N, seed):
    rng = np.random.default_rng(seed)
    return (rng.permutation(np.geomspace(1.0, 1e-3, N)) * rng.choice([-1.0, 1.0], N)).astype(F32)


@pytest.mark.parametrize("taps", ["ram-lak", "random"])
def test_filter_rows_bound_holds_and_catches_wrong_indices(taps):
    from tomo_tv_amd.engine import fbp_filter_taps
    N, P, nx = 9, 3, 70
    h = np.asarray(fbp_filter_taps(N, "ram-lak"), F32) if taps == "ram-lak" else _random_taps(N, 1)
    assert taps == "ram-lak" or len(set(np.abs(h).tolist())) == N
    b = ref64.signed_sino(nx, P * N, seed=31)
    ref, bound = ref64.filter_rows(b, h, P, N)
    idx = np.abs(np.arange(N)[:, None] - np.arange(N)[None, :])
    direct = (h.astype(np.float64)[idx][None, None] * b.reshape(nx, P, 1, N).astype(np.float64)).sum(axis=3)
    assert np.abs(direct.reshape(nx, -1) - ref).max() <= 1e-12
    ref64.assert_within("filter", _filter_f32(b, h, P, N), ref, bound)
    for kind in ("tap_plus_one", "chunk0", "next_projection"):
        with pytest.raises(AssertionError):
            ref64.assert_within("filter", _filter_f32(b, h, P, N, kind), ref, bound)


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _soft_inputs(l):
    l = F32(l)
    up, dn = np.nextafter(l, F32(4)), np.nextafter(l, F32(-1))
    rng = np.random.default_rng(32)
    special = np.array([l, -l, 0.0, -0.0, 1e-40, -1e-40, up, -up, dn, -dn, 2.0 ** -149, -2.0 ** -126], F32)
    return np.concatenate([special, rng.uniform(-2, 2, 500).astype(F32)])


@pytest.mark.parametrize("l", [0.3, 0.0])
def test_soft_threshold_is_exact_and_catches_a_wrong_comparison_or_sign(l):
    v = _soft_inputs(l)
    lf = F32(l)
    want = ref64.soft_threshold(v, l)
    assert want.dtype == F32
    plain = (np.sign(v) * np.maximum(np.abs(v) - lf, F32(0))).astype(F32)   # the textbook form: the same values (signs of zero apart)
    assert np.array_equal(want, plain)
    assert not np.signbit(want[want == 0]).any()                            # every zero is +0
    if l == 0.0:
        assert want[4] == v[4] != 0 and want[10] == v[10] != 0              # the subnormals survive
    a = np.abs(v)
    ge = np.where(a >= lf, np.copysign((a - lf).astype(F32), v), F32(0)).astype(F32)     # >= for >
    assert np.array_equal(ge, want)                                         # equal as values ...
    diff = _bits(ge) != _bits(want)                                         # ... the bit patterns tell: -0 at v == -l (and at -0 for l == 0)
    assert diff.any() and np.all((a[diff] == lf) & np.signbit(v[diff]))
    nosign = np.where(a > lf, (a - lf).astype(F32), F32(0)).astype(F32)     # the sign dropped
    assert not np.array_equal(_bits(nosign), _bits(want)) and not np.array_equal(nosign, want)


def _momentum_f32(r, old, beta, fma=False):
    beta = F32(beta)
    d = (r - old).astype(F32)
    if fma:                                                                 # beta * d is exact in binary64: one rounding of the sum
        return (beta.astype(np.float64) * d.astype(np.float64) + r.astype(np.float64)).astype(F32)
    return (r + (beta * d).astype(F32)).astype(F32)


@pytest.mark.parametrize("beta", [0.0, 0.37, 0.999])
def test_momentum_bound_holds_and_catches_exchanged_operands(beta):
    rng = np.random.default_rng(33)
    r = rng.uniform(-2, 2, (5, 8, 8)).astype(F32)
    old = (r + rng.uniform(-0.3, 0.3, r.shape)).astype(F32)
    old[0] = r[0]                                                           # no step where nothing moved
    for fn in (ref64.momentum, ref64.sino_extrapolate):
        y, bound = fn(r, old, beta)
        for fma in (False, True):
            ref64.assert_within("momentum", _momentum_f32(r, old, beta, fma), y, bound)
        assert np.abs(bound).max() <= 4 * ref64.U * np.abs(y).max() + 1e-30   # a few u
        if beta == 0.0:
            assert np.array_equal(y, r.astype(np.float64))
        with pytest.raises(AssertionError):                                 # old and r exchanged
            ref64.assert_within("momentum", _momentum_f32(old, r, beta), y, bound)
