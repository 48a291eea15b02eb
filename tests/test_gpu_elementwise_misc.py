"""Element-wise tests of the per-slice CGLS helpers, the WBP row filter and the FISTA passes against tests/ref64.py.

Every case asserts, from its shape, that it reaches the path it is listed for (the launchers' own arithmetic, restated here: a change
of a cap or a threshold there fails the assertion instead of silently ending the coverage).  sx = the slices rounded up to 64.

CGLS (k_slice_sumsq / _finish / _ratio / _axpy / _xpay), angles linspace(-70, 70, P):

  N    P  Nx    sx    per  what it reaches
  8    3  3     64    64   four row phases that meet in LDS; m = 64 (pixels) and 24 (rays)
  9    4  130   192   64   odd row counts 81 / 36: ragged 8-row trips, a short last row block
  8    3  513   576   128  two row phases; two workgroups along x, the second partly dead
  8    3  1025  1088  256  one row phase; two workgroups along x, the second partly dead
  33   5  449   512   128  exactly filled; m = 1089: 18 row blocks, the last one short
  212  3  130   192   64   k_slice_axpy / _xpay at the capped grid (8190 blocks, unit 3): a second grid-stride trip

  one step from zero: a-priori bound (Matrix.cgls_first_step), the zero slice exactly 0; the inputs' per-slice alpha differ between
  neighbouring slices by more than 100 bounds of alpha (asserted before the GPU is touched).  3 steps, called twice, from
  0.1 * dense_volume: seq_bound against cgls_f32 on the first four shapes.

WBP filter (k_filter_rows<VEC>; tomo_fbp called directly, SINO_R read back), ram-lak taps and random taps (all distinct, 1 .. 1e-3):

  N   P  Nx   VEC  nchunk
  9   3  129  1    3       81 waves: the last workgroup has 3 surplus waves
  16  2  384  2    3
  8   3  512  4    2
  48  4  2    1    1       (the shape of test_gpu_parity's WBP tests)

  SINO_R against filter_rows; the volume against scale * A^T (the device's own filtered rows), positivity 0 and 1.

FISTA passes (k_soft_threshold, k_scale, k_clamp, k_momentum, k_sino_extrapolate) at N = 8, Nx = 3 and N = 64, Nx = 1025 (n4 = 1 114 112
float4 > 4096 * 256: the second trip of the capped grid; its elements are ten times the first trip's).  Soft threshold, scale
and clamp bit for bit; the momentum's three buffers (first step, aliased step, after a caller wrote RECON_OLD); the projection of
the extrapolated point from the device's own two projections (61 angles at the large shape: the sinogram pass takes a second trip).

Worst error-to-bound ratios seen on an MI355X (the tests print them as "ratio ..."), none of them used to set a bound:

  CGLS first step   0.032  (of the a-priori bound: worst-case sums over 2 P + 16 entries, SAFETY 1.5)
  CGLS sequential   0.668  (of seq_bound: 4 x the float32 oracle's own worst error of the slice)
  filter            0.327
  momentum          0.987  (three roundings, each can reach u: about four million elements come close to all three)
  extrapolate       0.988
"""
import numpy as np
import pytest

import oracle
import ref64
from test_gpu_elementwise import engine
from tomo_tv_amd._lib import SINO_B, SINO_G, SINO_R, SINO_YK_MODEL, VOL_RECON, VOL_RECON_OLD, VOL_YK
from tomo_tv_amd.engine import _ptr, fbp_filter_taps

pytestmark = pytest.mark.gpu
F32 = np.float32
RATIOS = {}
GRID_1D_CAP = 4096          # grid_1d(): blocks of 256 float4
SLICE_GRID_CAP = 8192       # slice_grid(): blocks of 256 float4, rounded down to a multiple of sx / 64


def _note(key, r):
    RATIOS[key] = max(RATIOS.get(key, 0.0), r)
    print(f"ratio {key}: {RATIOS[key]:.3f}")


def _sx(Nx):
    return -(-Nx // 64) * 64


def _angles(P):
    return np.linspace(-70, 70, P)


_MATRIX = {}


def _matrix(N, P):
    if (N, P) not in _MATRIX:
        _MATRIX[N, P] = ref64.Matrix(N, _angles(P))
        assert _MATRIX[N, P].duplicates == 0
    return _MATRIX[N, P]


def _engine(monkeypatch, N, P, Nx):
    return engine(monkeypatch, _angles(P), N, Nx)


# ---- CGLS ---------------------------------------------------------------------------------------------------------------------------------
# (N, P, Nx, per, row phases, workgroups along x, partly dead, short last row block of the pixel sums)
CGLS_CASES = [(8, 3, 3, 64, 4, 1, True, False), (9, 4, 130, 64, 4, 1, True, True), (8, 3, 513, 128, 2, 2, True, False),
              (8, 3, 1025, 256, 1, 2, True, False), (33, 5, 449, 128, 2, 1, False, True)]
CGLS_IDS = [f"N{c[0]}-P{c[1]}-nx{c[2]}-per{c[3]}" for c in CGLS_CASES]


def _sumsq_layout(Nx, m):
    """slice_sumsq() / k_slice_sumsq for m rows: (per, row phases, workgroups along x, dead float4 columns, row blocks, rows per block,
    rows of the last block)."""
    cols = _sx(Nx) // 4
    per = 256 if cols >= 256 else 128 if cols >= 128 else 64
    gx = -(-cols // per)
    nby = min(1024, max(1, (m + 63) // 64))
    rpb = -(-m // nby)
    return per, 256 // per, gx, gx * per - cols, nby, rpb, m - (nby - 1) * rpb


_CGLS_DATA = {}


def _cgls_data(N, P, Nx):
    """(matrix, sinogram): computed once per shape, never modified."""
    if (N, P, Nx) not in _CGLS_DATA:
        M = _matrix(N, P)
        b = ref64.cgls_sino(M, Nx, seed=N + Nx)
        b.setflags(write=False)
        _CGLS_DATA[N, P, Nx] = (M, b)
    return _CGLS_DATA[N, P, Nx]


@pytest.mark.parametrize("N,P,Nx,per,phases,gx,dead,short", CGLS_CASES, ids=CGLS_IDS)
def test_cgls_first_step_elementwise(gpu, monkeypatch, N, P, Nx, per, phases, gx, dead, short):
    lay = _sumsq_layout(Nx, N * N)
    assert lay[:3] == (per, phases, gx) and (lay[3] > 0) == dead and (0 < lay[6] < lay[5]) == short, lay
    if (N, Nx) == (9, 130):
        assert lay[5] % 8 != 0 and _sumsq_layout(Nx, N * P)[5] % 8 != 0          # ragged 8-row trips in both sums
    if (N, Nx) == (33, 449):
        assert lay[3] == 0 and lay[4] == 18
    M, b = _cgls_data(N, P, Nx)
    x1, bound, alpha, rel = M.cgls_first_step(b)
    zs = ref64.cgls_zero_slice(Nx)
    assert zs % 4 in (1, 2) and not b[zs].any() and alpha[zs] == 0 and np.count_nonzero(alpha == 0) == 1
    sep = ref64.alpha_separation(alpha, rel)
    print(f"alpha separation / (100 bounds): {sep:.2f}")
    assert sep > 1.0                                                              # before the GPU is touched
    t = _engine(monkeypatch, N, P, Nx)
    t.set_tilt_series(b)
    t.be.c("cgls", VOL_RECON, 1)                                                  # from the zero volume
    got = t.get_volume()
    assert np.isfinite(got).all()
    assert not got[zs].any(), "the zero slice"
    _note("cgls first step", ref64.ratio(got, x1, bound))
    ref64.assert_within("cgls first step", got, x1, bound)


def _oracle_cgls(M, x0, b, niter):
    orc = oracle.ctvlib(len(b), M.N, M.P)
    orc.A = oracle.CSR(M.nrow, M.ncol, *M.csr())

    def fp(v):
        orc.recon[:] = v
        orc.forward_projection()
        return orc.g.copy()
    return ref64.cgls_f32(fp, orc.back_projection, x0, b, niter)


@pytest.mark.parametrize("N,P,Nx,per,phases,gx,dead,short", CGLS_CASES[:4], ids=CGLS_IDS[:4])
def test_cgls_three_steps_twice_elementwise(gpu, monkeypatch, N, P, Nx, per, phases, gx, dead, short):
    """3 steps from 0.1 * dense_volume, called twice (every call restarts, like the reference's): the float32 oracle iteration is the
    yardstick of the binary64 one."""
    assert _sumsq_layout(Nx, N * N)[:3] == (per, phases, gx)
    M, b = _cgls_data(N, P, Nx)
    x0 = (F32(0.1) * ref64.dense_volume(Nx, N, seed=N + Nx + 7)).astype(F32)
    t = _engine(monkeypatch, N, P, Nx)
    t.set_tilt_series(b)
    t.set_volume(x0, VOL_RECON)
    x32, x64 = x0, x0
    for call in range(2):
        t.be.c("cgls", VOL_RECON, 3)
        got = t.get_volume()
        x32 = _oracle_cgls(M, x32, b, 3)
        x64, _, _ = M.cgls(x64, b, 3)
        _note("cgls sequential", ref64.ratio(got, x64, ref64.seq_bound(x32, x64)))
        ref64.assert_seq(f"cgls call {call}", got, x32, x64)


def test_cgls_capped_grid_with_a_unit_that_is_no_power_of_two(gpu, monkeypatch):
    """k_slice_axpy / k_slice_xpay on a volume of more float4 than the capped grid covers in one trip, sx / 64 = 3: the grid is
    rounded down to 8190 blocks so that a thread meets its own four coefficients again on the second trip.  The slices compared are
    ``ref64.slice_sample`` (the whole volume is fetched); the coefficient an unrounded grid would hand a second-trip element comes from
    the float4 group (8192 * 256) % (sx / 4) further on: those partner slices' alpha are computed too and must differ."""
    N, P, Nx = 212, 3, 130
    sx = _sx(Nx)
    n4, unit = N * N * sx // 4, sx // 64
    assert n4 > SLICE_GRID_CAP * 256 and unit == 3 and unit & (unit - 1) != 0
    grid = SLICE_GRID_CAP // unit * unit
    assert grid == 8190 and (grid * 256) % (sx // 4) == 0 and n4 > grid * 256
    shift = 4 * ((SLICE_GRID_CAP * 256) % (sx // 4))                              # slices, of an unrounded grid's stride
    assert shift % sx != 0
    first2 = -(-grid * 256 // (sx // 4))                                          # pixels from here on are wholly on the second trip
    M, b = _cgls_data(N, P, Nx)
    sl = ref64.slice_sample(Nx)
    partner = [(s + shift) % sx for s in sl]
    both = np.array(sorted(set(sl) | {p for p in partner if p < Nx}))
    x1, bound, alpha, rel = M.cgls_first_step(b[both])
    at = {int(s): k for k, s in enumerate(both)}
    zs = ref64.cgls_zero_slice(Nx)
    assert zs in at and alpha[at[zs]] == 0
    for s, p in zip(sl, partner):                                                 # (a partner in the padding has coefficient 0)
        if s != zs and p < Nx and p != zs:
            a, c = alpha[at[s]], alpha[at[p]]
            assert abs(a - c) / max(a, c) > 100 * max(rel[at[s]], rel[at[p]]), (s, p)
    k = [at[int(s)] for s in sl]
    x1, bound = x1[k], bound[k]
    tail = x1.reshape(len(sl), -1)[:, first2:]
    assert (np.abs(tail).max(axis=1) > 0)[sl != zs].all()                         # the second trip writes non-zero voxels
    t = _engine(monkeypatch, N, P, Nx)
    t.set_tilt_series(b)
    t.be.c("cgls", VOL_RECON, 1)
    got = t.get_volume()
    assert np.isfinite(got).all() and not got[zs].any()
    _note("cgls first step", ref64.ratio(got[sl], x1, bound))
    ref64.assert_within("cgls capped grid", got[sl], x1, bound)


# ---- WBP row filter -------------------------------------------------------------------------------------------------------------------------
FILTER_CASES = [(9, 3, 129, 1, 3), (16, 2, 384, 2, 3), (8, 3, 512, 4, 2), (48, 4, 2, 1, 1)]


def random_taps(N, seed):
    """N distinct taps, magnitudes from 1 down to 1e-3 in random order, random signs."""
    rng = np.random.default_rng(seed)
    h = (rng.permutation(np.geomspace(1.0, 1e-3, N)) * rng.choice([-1.0, 1.0], N)).astype(F32)
    assert len(set(np.abs(h).tolist())) == N
    return h


@pytest.mark.parametrize("N,P,Nx,VEC,nchunk", FILTER_CASES, ids=[f"N{c[0]}-nx{c[2]}-vec{c[3]}" for c in FILTER_CASES])
def test_wbp_filter_rows_elementwise(gpu, monkeypatch, N, P, Nx, VEC, nchunk):
    sxc = _sx(Nx)
    assert (4 if sxc % 256 == 0 else 2 if sxc % 128 == 0 else 1) == VEC and sxc // (64 * VEC) == nchunk
    waves = N * P * nchunk
    if (N, Nx) == (9, 129):
        assert waves == 81 and -(-waves // 4) * 4 - waves == 3                    # surplus waves in the last workgroup
    M = _matrix(N, P)
    b = ref64.signed_sino(Nx, M.nrow, seed=N + Nx)
    t = _engine(monkeypatch, N, P, Nx)
    t.set_tilt_series(b)
    scale = F32(np.pi / P)
    for name, taps in (("ram-lak", fbp_filter_taps(N, "ram-lak")), ("random", random_taps(N, N + Nx))):
        taps = np.ascontiguousarray(taps, F32)
        f64, fb = ref64.filter_rows(b, taps, P, N)
        for positivity in (0, 1):
            t.be.c("fbp", _ptr(taps), float(scale), positivity)
            g = t._sino(SINO_R)
            _note("filter", ref64.ratio(g, f64, fb))
            ref64.assert_within(f"filter {name}", g, f64, fb)
            assert np.array_equal(t._sino(SINO_B), b)                             # the tilt series is only read
            v64, vb, _ = M.bp_bound(g)                                            # A^T of the device's own filtered rows
            ref = float(scale) * v64
            bound = float(scale) * vb + 2 * ref64.U * np.abs(ref)
            got = t.get_volume()
            if positivity:
                assert got.min() >= 0
                ref = np.maximum(ref, 0.0)
            else:
                assert got.min() < 0                                              # negative voxels survive
            ref64.assert_within(f"wbp volume {name} positivity {positivity}", got, ref, bound)


# ---- FISTA and element-wise passes ------------------------------------------------------------------------------------------------------
PASS_SHAPES = [(8, 3), (64, 1025)]
PASS_IDS = ["N8-nx3", "N64-nx1025"]


def _second_trip_pixel(rows, Nx, must):
    """The first row (pixel, or ray) whose float4 all lie on the second trip of a grid_1d() pass over ``rows`` rows, None if the pass
    has one trip; ``must``: the shape is there to reach the second trip."""
    sx4 = _sx(Nx) // 4
    n4 = rows * sx4
    if must:
        assert n4 > GRID_1D_CAP * 256, n4
    if n4 <= GRID_1D_CAP * 256:
        return None
    assert n4 <= 2 * GRID_1D_CAP * 256
    return -(-GRID_1D_CAP * 256 // sx4)


def _two_trip_volume(N, Nx, seed, signed=True):
    """Magnitudes in [0.1, 1) on the first trip, ten times that (values the first trip never has) on the second."""
    rng = np.random.default_rng(seed)
    v = rng.uniform(0.1, 1.0, (Nx, N * N))
    if signed:
        v *= rng.choice([-1.0, 1.0], v.shape)
    p2 = _second_trip_pixel(N * N, Nx, N == 64)
    if p2 is not None:
        v[:, p2:] *= 10.0
    return v.astype(F32).reshape(Nx, N, N)


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


@pytest.mark.parametrize("N,Nx", PASS_SHAPES, ids=PASS_IDS)
def test_soft_threshold_scale_and_clamp_bit_for_bit(gpu, monkeypatch, N, Nx):
    t = _engine(monkeypatch, N, 3, Nx)
    lam = F32(0.3)
    up, dn = np.nextafter(lam, F32(1)), np.nextafter(lam, F32(0))
    special = np.array([lam, -lam, 0.0, -0.0, 1e-40, -1e-40, up, -up, dn, -dn, 2 * lam, -2 * lam, 2.0 ** -149, 2.0 ** -126], F32)
    assert special[4] != 0 and np.signbit(special[3])
    for l in (lam, F32(0.0)):
        x = _two_trip_volume(N, Nx, seed=N + 1)
        flat = x.reshape(Nx, -1)
        k = min(Nx, len(special))
        for pix in (0, N * N // 2, N * N - 1):                                    # the special values on both trips, in every float4 lane
            flat[:k, pix] = special[:k]
            flat[Nx - k:, (pix + 1) % (N * N)] = special[:k]
        if Nx < len(special):
            flat[0, 2:2 + len(special)] = special
        t.set_volume(x, VOL_RECON)
        assert np.array_equal(_bits(t.get_volume()), _bits(x))                    # the transfers keep -0 and the subnormals
        t.be.c("soft_threshold", VOL_RECON, float(l))                             # the raw entry: no positivity after it
        got, want = t.get_volume(), ref64.soft_threshold(x, l)
        assert (want < 0).any() and (want == 0).any()
        bad = np.argwhere(_bits(got) != _bits(want))
        assert bad.size == 0, (float(l), bad[:5].tolist(), [float(got[tuple(i)]) for i in bad[:5]], [float(want[tuple(i)]) for i in bad[:5]])
    x = _two_trip_volume(N, Nx, seed=N + 2)
    t.set_volume(x, VOL_RECON)
    t.be.c("scale_volume", VOL_RECON, 0.37)
    want = (x * F32(0.37)).astype(F32)
    assert np.array_equal(t.get_volume(), want)
    t.positivity()
    assert np.array_equal(t.get_volume(), np.maximum(want, F32(0))) and (want < 0).any()


@pytest.mark.parametrize("beta", [0.0, 0.37, 0.999])
@pytest.mark.parametrize("N,Nx", PASS_SHAPES, ids=PASS_IDS)
def test_fista_momentum_elementwise(gpu, monkeypatch, N, Nx, beta):
    """Step 1: RECON_OLD a volume of its own.  Step 2: RECON_OLD is RECON (a flag in the engine), and the new point lands in the buffer
    RECON has left.  Step 3: the caller wrote RECON_OLD in between.  After each: YK = r + beta (r - old) within the bound, RECON and
    RECON_OLD the prox result r bit for bit."""
    t = _engine(monkeypatch, N, 3, Nx)
    vols = [_two_trip_volume(N, Nx, seed=10 * N + k, signed=(k % 2 == 1)) for k in range(6)]
    t.set_volume(vols[0], VOL_RECON)
    t.initialize_fista()
    old = vols[1]
    t.set_volume(old, VOL_RECON_OLD)
    for step, r in enumerate(vols[2:5]):
        if step == 2:
            old = vols[5]
            t.set_volume(old, VOL_RECON_OLD)
        t.set_volume(r, VOL_YK)
        t.fista_momentum(beta)
        y64, bound = ref64.momentum(r, old, beta)
        got = t.get_volume(VOL_YK)
        _note("momentum", ref64.ratio(got, y64, bound))
        ref64.assert_within(f"momentum step {step}", got, y64, bound)
        if beta == 0.0:
            assert np.array_equal(got, r)
        assert np.array_equal(t.get_volume(VOL_RECON), r), step
        assert np.array_equal(t.get_volume(VOL_RECON_OLD), r), step
        assert np.array_equal(t.get_volume(VOL_YK), got), step                    # (reading the three changed none of them)
        old = r


@pytest.mark.parametrize("N,Nx,P", [(8, 3, 3), (64, 1025, 61)], ids=PASS_IDS)
def test_fista_project_yk_elementwise(gpu, monkeypatch, N, Nx, P):
    """SINO_YK_MODEL against (1 + beta) A r - beta A r_old formed in binary64 from the device's own two projections; the beta == 0
    forms bit for bit; and the projection the pass saves for the next step bit for bit: the step after it projects a zero volume with
    beta = 1, which makes the result the saved projection's negative exactly."""
    _second_trip_pixel(N * P, Nx, N == 64)                                        # the sinogram pass: P = 61 rays' worth of float4
    t = _engine(monkeypatch, N, P, Nx)
    t.set_tilt_series(ref64.signed_sino(Nx, N * P, seed=3))
    assert t.get_option("fp_reuse") == 1
    t.set_volume(_two_trip_volume(N, Nx, 70, signed=False), VOL_RECON)
    t.initialize_fista()
    prev = None
    for step, beta in enumerate((0.0, 0.37, 0.0, 0.999, 1.0)):
        r = _two_trip_volume(N, Nx, 71 + step, signed=False) if beta != 1.0 else np.zeros((Nx, N, N), F32)
        t.set_volume(r, VOL_YK)
        t.fista_momentum(beta)
        t.data_distance()
        assert t.fista_project_yk(), step                                         # (step 0: the shortcut of a first step with beta == 0)
        q = t._sino(SINO_YK_MODEL)
        g = t.get_model_projections()                                             # G stays A r
        if step == 0:
            assert g.any()
        if beta == 0.0:
            assert np.array_equal(q, g), step
        elif beta == 1.0:
            assert not g.any() and prev.any() and np.array_equal(q, -prev)        # the saved projection, bit for bit
        else:
            q64, bound = ref64.sino_extrapolate(g, prev, beta)
            _note("extrapolate", ref64.ratio(q, q64, bound))
            ref64.assert_within(f"extrapolate step {step}", q, q64, bound)
        prev = g
