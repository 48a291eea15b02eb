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
