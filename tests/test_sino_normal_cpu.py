"""The per-projection similarity matching without a GPU: the binary64 statement of the 21 sums (tests/ref64_sino_normal.py) against
plain loops, the binary32 replay of the kernel's arithmetic inside the bound and three deliberately wrong replays outside it, the host
helpers of ``align``, the ABI, the Python refusals, and the recovery of a known warp by the binary64 replay of the loop."""
import functools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import ref64_affine as RF
import ref64_sino_normal as SN
import sequences_affine3d  # noqa: F401  (the rows of the other features: the closure check below needs the whole table)
import sequences_register3d  # noqa: F401
import sequences_sino_normal  # noqa: F401  (registers this feature's row of the call-sequence closure table)
from conftest import ROOT
from test_bin_cpu import mixed

# (shift, rotation in degrees, magnification) of the replay tests
MAPS = [((1.5, -2.25), 1.3, 1.02), ((0.3, -0.6), -4.0, 0.97), ((0.5, 0.0), 8.0, 1.0), ((-1.5, 0.25), 0.7, 1.05), ((2.0, -1.5), -2.0, 1.0)]
IDENT = np.array([1.0, 0, 0, 0, 1.0, 0])

# What the binary64 replay of the loop reaches on the committed fixture (``ref64_sino_normal.recovery_case``, margin 2, start at the
# identity, default tolerances): worst (shift error in pixels, rotation error in degrees, magnification error) over the
# projections.  It converges at the default tolerances in 4 iterations at both shapes.
RECORDED = {(70, 33, 5): (3.52e-3, 2.25e-2, 4.67e-4), (40, 48, 4): (7.47e-3, 6.34e-2, 1.65e-4)}


def smooth(P, N, ns, seed):
    """per projection a few Gaussian blobs on a slope: both gradient components and the residual are non-trivial"""
    rng = np.random.default_rng(seed)
    r, s = np.meshgrid(np.arange(N, dtype=np.float64), np.arange(ns, dtype=np.float64), indexing="ij")
    out = []
    for _ in range(P):
        X = 0.02 * r - 0.01 * s
        for _ in range(4):
            c, w = (rng.uniform(0.25 * N, 0.75 * N), rng.uniform(0.25 * ns, 0.75 * ns)), rng.uniform(0.15, 0.3) * min(N, ns)
            X = X + rng.uniform(0.5, 1.5) * np.exp(-((r - c[0]) ** 2 + (s - c[1]) ** 2) / (2 * w * w))
        out.append(X)
    return np.array(out, np.float32)


def maps(N, ns):
    d, rot, mag = zip(*MAPS)
    return RF.matrices(np.array(d), rot, mag, N, ns)


@pytest.mark.parametrize("shape", [(5, 6), (6, 5)])
def test_statement_equals_the_loops(shape):
    N, ns = shape
    P = len(MAPS) + 2
    Fv, Gv = mixed((P, N, ns), N).astype(np.float64), mixed((P, N, ns), ns + 7).astype(np.float64)
    M = np.vstack([maps(N, ns), IDENT, [1, 0, -1, 0, 1, 1]])
    for margin in (0, 1):
        a, b = SN.normal(Fv, Gv, M, margin), SN.normal_loops(Fv, Gv, M, margin)
        assert np.allclose(a, b, rtol=1e-12, atol=1e-12) and np.array_equal(a[:, 15], b[:, 15]), margin
    ident = SN.normal(Fv, Fv, np.tile(IDENT, (P, 1)), 0)
    assert np.all(ident[:, 15] == (N - 1) * (ns - 1)) and not ident[:, 14].any() and not ident[:, 10:14].any()   # the last row and slice never count
    far = SN.normal(Fv, Gv, np.tile([1, 0, 3.0 * N, 0, 1, 0], (P, 1)), 0)
    assert not far.any()


def test_replay_is_inside_the_bound_and_wrong_replays_are_outside():
    N, ns = 14, 17
    P = len(MAPS)
    Fv, Gv = smooth(P, N, ns, 70), smooth(P, N, ns, 80)
    M = maps(N, ns)
    ref, bnd, _ = SN.bound(Fv, Gv, M, 1)
    assert np.allclose(ref, SN.normal(Fv, Gv, M, 1), rtol=1e-14, atol=0)
    r = SN.ratios(SN.normal_replay_f32(Fv, Gv, M, 1), ref, bnd)
    print(f"replay: worst error / bound per projection {np.round(r.max(axis=1), 4)}, samples that count {ref[:, 15].astype(int)}")
    assert r.max() <= 1.0 and np.all(ref[:, 15] > N * ns // 8)
    for wrong in ("swapped_gradient", "corner", "zero_padded"):
        rw = SN.ratios(SN.normal_replay_f32(Fv, Gv, M, 1, **{wrong: True}), ref, bnd)
        assert np.all(rw.max(axis=1) > 1.0), (wrong, rw.max(axis=1))


def test_replay_copies_samples_on_whole_pixel_maps():
    """identity and a whole-pixel shift: w is a copy, so the count and the sums of w carry the summation term alone"""
    P, N, ns = 2, 9, 11
    Fv, Gv = smooth(P, N, ns, 3), smooth(P, N, ns, 4)
    M = np.array([IDENT, [1, 0, -2, 0, 1, 1]], np.float64)
    ref, _, summ = SN.bound(Fv, Gv, M, 0)
    got = SN.normal_replay_f32(Fv, Gv, M, 0)
    assert np.array_equal(got[:, 15], ref[:, 15]) and np.all(np.abs(got[:, 16:] - ref[:, 16:]) <= summ[:, 16:])
    assert ref[0, 15] == (N - 1) * (ns - 1) and ref[1, 15] == (N - 2) * (ns - 2)   # rows r >= 2; slices s + 2 <= ns - 1
    # a coordinate just below a whole pixel whose fraction rounds to 1 IS that pixel with t = 0: the identity moved by -2^-30 counts
    # row 0 and slice 0 and copies the identity's samples (the statement, with the exact floor, does not: its "near" term says so)
    tiny = np.array([[1, 0, -2.0 ** -30, 0, 1, -2.0 ** -30]] * P)
    near, same = SN.normal_replay_f32(Fv, Gv, tiny, 0), SN.normal_replay_f32(Fv, Gv, np.tile(IDENT, (P, 1)), 0)
    assert np.array_equal(near[:, 14:], same[:, 14:]) and np.all(near[:, 15] == (N - 1) * (ns - 1))
    rt, bt, _ = SN.bound(Fv, Gv, tiny, 0)
    assert SN.ratios(near, rt, bt).max() <= 1.0 and np.all(bt[:, 15] >= N + ns - 1)        # (the statement counts rows 1 .. N - 1 instead)


def test_host_helpers():
    from tomo_tv_amd.align import affine_matrices, compose_similarity_increment, decode_similarity, similarity_increment, unpack_similarity_normal
    N, ns = 33, 70
    d, rot, mag = (np.array(v) for v in zip(*MAPS))
    M = affine_matrices(d, rot, mag, N, ns)
    assert np.allclose(M, maps(N, ns), rtol=0, atol=1e-12)
    sh, ro, ma = decode_similarity(M, N, ns)                                   # decode o affine_matrices = identity
    assert np.allclose(sh, d, rtol=0, atol=1e-12) and np.allclose(ro, rot, rtol=0, atol=1e-12) and np.allclose(ma, mag, rtol=0, atol=1e-12)
    assert np.allclose(affine_matrices(sh, ro, ma, N, ns), M, rtol=0, atol=1e-12)
    assert compose_similarity_increment(M, np.zeros((len(M), 4)), N, ns).tobytes() == M.tobytes()      # a zero step: bit for bit
    delta = np.array([[0.3, -0.2, 0.01, 0.002]] * len(M))
    delta[2] = 0.0
    out = compose_similarity_increment(M, delta, N, ns)
    assert np.allclose(out, SN.compose(M, delta, N, ns), rtol=0, atol=1e-13) and out[2].tobytes() == M[2].tobytes()
    # a pure shift increment moves the source position by it; a rotation and a magnification keep the centre of the moving image
    I = np.tile(IDENT, (1, 1))
    assert np.allclose(compose_similarity_increment(I, [[1, 2, 0, 0]], N, ns)[0], (1, 0, 1, 0, 1, 2))
    c = np.array([0.5 * (N - 1), 0.5 * (ns - 1)])
    turned = compose_similarity_increment(I, [[0, 0, 0.1, 0.05]], N, ns)[0].reshape(2, 3)
    assert np.allclose(turned[:, :2] @ c + turned[:, 2], c, atol=1e-12)
    quarter = compose_similarity_increment(I, [[0, 0, np.pi / 2, 0]], N, ns)[0].reshape(2, 3)[:, :2]   # +r towards +s
    assert np.allclose(quarter @ [1, 0], [0, 1], atol=1e-15)
    # the sense of the increment against affine_matrices: omega turns the SOURCE position, so the content turns by -omega, and
    # e^lambda scales the source position, so the content shrinks
    _, ro2, ma2 = decode_similarity(compose_similarity_increment(I, [[0, 0, np.deg2rad(2.0), np.log(1.25)]], N, ns), N, ns)
    assert np.allclose(ro2, -2.0, atol=1e-12) and np.allclose(ma2, 0.8, atol=1e-12)
    # the linear part stays a scaled rotation through 50 compositions
    rng = np.random.default_rng(0)
    Mk = M.copy()
    for _ in range(50):
        Mk = compose_similarity_increment(Mk, rng.uniform(-0.2, 0.2, (len(M), 4)) * [1, 1, 1, 0.1], N, ns)
    for a in range(len(M)):
        A = Mk[a].reshape(2, 3)[:, :2]
        k = np.linalg.det(A)
        assert np.allclose(A @ A.T, k * np.eye(2), rtol=0, atol=1e-12 * max(1.0, k)) and k > 0
    # the step: H delta = -b per projection, with damping (H + damping diag H) delta = -b; switched-off parameters stay exactly put
    Q = rng.normal(size=(3, 9, 4))
    H, b = np.einsum("pij,pik->pjk", Q, Q), rng.normal(size=(3, 4))
    dl = similarity_increment(H, b)
    assert np.allclose(np.einsum("pjk,pk->pj", H, dl), -b, atol=1e-12)
    dd = similarity_increment(H, b, 0.5)
    assert all(np.allclose((H[a] + 0.5 * np.diag(np.diag(H[a]))) @ dd[a], -b[a], atol=1e-12) for a in range(3))
    for kw, keep in ((dict(rotation=False), [0, 1, 3]), (dict(magnification=False), [0, 1, 2]), (dict(rotation=False, magnification=False), [0, 1])):
        dk = similarity_increment(H, b, **kw)
        off = [k for k in range(4) if k not in keep]
        assert not dk[:, off].any() and all(np.allclose(H[a][np.ix_(keep, keep)] @ dk[a, keep], -b[a, keep], atol=1e-12) for a in range(3))
        Mo = compose_similarity_increment(I, dk[:1], N, ns)
        _, ro3, ma3 = decode_similarity(Mo, N, ns)
        assert (2 in keep or ro3[0] == 0.0) and (3 in keep or ma3[0] == 1.0)
    sing = H.copy()
    sing[1][:, 3], sing[1][3, :] = sing[1][:, 2].copy(), sing[1][2, :].copy()
    sing[1][3, 3] = sing[1][2, 2]
    nanH, infb = H.copy(), b.copy()
    nanH[2, 0, 0], infb[0, 1] = np.nan, np.inf
    for bad, who in (((nanH, b), "projection 2"), ((H, infb), "projection 0"), ((sing, b), "projection 1")):
        with pytest.raises(ValueError, match=who):
            similarity_increment(*bad)
    for bad in ((H, b, -1.0), (H[0], b[0]), (np.zeros((3, 4, 4)), b, 1.0)):
        with pytest.raises(ValueError):
            similarity_increment(*bad)
    assert np.all(np.isfinite(similarity_increment(sing, b, 0.1)))
    assert np.all(np.isfinite(similarity_increment(sing, b, rotation=False)))           # the singular pair is no longer in the system
    # a projection that is not active is not looked at (the loop's converged projections) and gets a zero step
    da = similarity_increment(sing, b, active=[True, False, True])
    assert not da[1].any() and np.array_equal(da[[0, 2]], dl[[0, 2]])
    assert not similarity_increment(nanH, infb, active=[False, True, False])[[0, 2]].any()
    with pytest.raises(ValueError):
        similarity_increment(H, b, active=[True, False])
    # the unpacking of the 21 sums: this file's statement of it
    out = rng.normal(size=(4, 21)) ** 2
    out[:, 15], out[3] = [5, 9, 1, 0], 0.0
    out[:, 16:18] += 10.0
    Hu, bu, ssd, cnt, ncc = unpack_similarity_normal(out)
    H2, b2, ssd2, cnt2, ncc2 = SN.unpack(out)
    assert np.array_equal(Hu, H2) and np.array_equal(Hu, Hu.transpose(0, 2, 1)) and np.array_equal(bu, b2) and np.array_equal(ssd, ssd2)
    assert np.array_equal(cnt, cnt2) and cnt.dtype == np.int64 and np.allclose(ncc, ncc2, rtol=1e-14, atol=0) and ncc[3] == 0.0


class FakeEngine:
    """``sino_affine_normal`` by the binary64 statement: what ``match_projections`` needs of an engine"""
    def __init__(self, F, G):
        self.F, self.G = F, G
        self.Nproj, self.Ny, self.Nslice_ = F.shape[0], F.shape[1], F.shape[2]
        self.calls = 0

    def sino_affine_normal(self, fixed, moving, M, margin=1):
        from tomo_tv_amd.align import unpack_similarity_normal
        self.calls += 1
        return unpack_similarity_normal(SN.normal(self.F, self.G, M, margin))


def test_python_refusals_come_before_the_library(monkeypatch):
    from tomo_tv_amd import _lib, engine, inprocess, reconstructor

    def boom(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "load", boom)

    class Untouchable:
        def __getattr__(self, name):
            boom()
    sharded = object.__new__(engine.tomoengine)
    sharded.comm, sharded.sub_slabs, sharded.be = object(), 1, None
    subslab = object.__new__(engine.tomoengine)
    subslab.comm, subslab.sub_slabs, subslab.be = None, 2, object.__new__(engine._GroupBackend)
    whole = object.__new__(engine.tomoengine)
    whole.comm, whole.sub_slabs, whole.be = None, 1, object.__new__(engine._SlabBackend)
    for e in (sharded, subslab, whole):
        e.Nproj, e.Ny, e.Nslice_ = 3, 12, 10
    I = np.tile(IDENT, (3, 1))
    for eng in (sharded, subslab):
        with pytest.raises(NotImplementedError):
            eng.sino_affine_normal(1, 2, I)
    nan = I.copy()
    nan[1, 2] = np.nan
    for M in (I[:2], np.zeros((3, 5)), np.zeros(18), nan, np.where(np.isnan(nan), np.inf, nan)):
        with pytest.raises(ValueError):
            whole.sino_affine_normal(1, 2, M)
    for margin in (-1, 5, 6):                                                       # 2 * 5 >= 10 slices
        with pytest.raises(ValueError):
            whole.sino_affine_normal(1, 2, I, margin=margin)
    with pytest.raises(NotImplementedError):
        object.__new__(engine._GroupBackend).c("sino_affine_normal", 1, 2, None, 1, None)
    with pytest.raises(NotImplementedError):
        inprocess.InProcessMultiGPU.sino_affine_normal(None, 1, 2, I)
    # the loop's own refusals, on an engine that must not be asked
    from tomo_tv_amd.align import match_projections
    for kw in (dict(M0=np.zeros((2, 6))), dict(M0=nan), dict(max_iter=-1), dict(tol_shift=-1.0), dict(tol_deg=np.nan), dict(tol_mag=-1e-9)):
        with pytest.raises(ValueError):
            match_projections(whole, 1, 2, **kw)
    # the driver: leave_one_out with a recon callback, and an object whose engine is sharded
    rec = object.__new__(reconstructor.TomoGPU)
    rec.tomo, rec._align_kept, rec.Nangles = sharded, True, 3
    with pytest.raises(NotImplementedError):
        rec.refine_alignment_affine()
    rec.tomo = object()
    with pytest.raises(NotImplementedError):
        rec.refine_alignment_affine()
    sharded.be = subslab.be = whole.be = None                                       # (nothing to destroy)


def test_symbols_in_header_library_and_table():
    from tomo_tv_amd import _lib
    import sequences as S
    import test_abi_cpu
    src = open(os.path.join(ROOT, "include", "tomo_hip.h")).read()
    L = _lib.load()
    name = "tomo_sino_affine_normal"
    assert re.search(r"\bint %s\s*\(" % name, src) and hasattr(L, name)
    assert _lib.SIGNATURES[name] == [_lib._p, _lib._i, _lib._i, _lib._p, _lib._i, _lib._p]
    ident, out = IDENT.copy(), np.zeros(21)
    assert L.tomo_sino_affine_normal(None, 0, 1, ident.ctypes.data, 1, out.ctypes.data) == 1 and L.tomo_last_error()
    # the header declares exactly what the library exports
    nm = shutil.which("nm")
    assert nm, "binutils' nm is needed to list the library's exports"
    sym = subprocess.run([nm, "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = sorted(set(re.findall(r" T (tomo_\w+)$", sym, re.M)))
    declared = test_abi_cpu.declared_symbols()
    assert len(exported) == len(declared) and exported == declared
    names = S.header_prototypes(src)
    assert set(sequences_sino_normal.ROWS) <= set(names) and S.closure_errors(names) == []
    for phrase in ("all four tap positions lie inside G_a", "[0..9] the upper triangle of J^T J, row-major", "q_r g_s - q_s g_r, q_r g_r + q_s g_s",
                   "tomo_sino_xcorr, tomo_sino_affine_normal and tomo_sino_axis_profile may be called"):
        assert phrase in src, phrase


# ---- the loop ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def recovery(shape):
    """the fixture and the binary64 replay of the loop on it (margin 2, from the identity, default tolerances, at most 30 iterations)"""
    Fv, Gv, Mt, truth = SN.recovery_case(shape)
    M, hist = SN.gauss_newton(Fv, Gv, max_iter=30, margin=2)
    return dict(F=Fv, G=Gv, M_true=Mt, truth=truth, M=M, hist=hist, err=SN.recovery_error(M, truth, shape[1], shape[0]))


@pytest.mark.parametrize("shape", SN.RECOVERY_SHAPES)
def test_recovery_by_the_binary64_replay(shape):
    """Recorded (RECORDED above): the replay's own error on the committed fixture; asserted against twice that."""
    c = recovery(shape)
    ns, N, P = shape
    d, rot, mag = c["truth"]
    assert np.all(np.abs(d) <= 1.5) and np.all(np.abs(rot) <= 2.0) and np.all(np.abs(mag - 1.0) <= 0.02) and len(rot) == P
    print(f"{shape}: shift error {c['err'][0]:.3e} px, rotation error {c['err'][1]:.3e} degrees, magnification error {c['err'][2]:.3e}; "
          f"{len(c['hist']['step'])} iterations, converged {c['hist']['converged']}, ncc {np.round(c['hist']['ncc'][0], 4)} -> "
          f"{np.round(c['hist']['ncc'][-1], 5)}")
    assert all(e <= 2.0 * r for e, r in zip(c["err"], RECORDED[shape]))
    assert c["hist"]["converged"].all() and len(c["hist"]["step"]) < 30                # the replay does converge at the default tolerances
    assert np.all(c["hist"]["ssd"][-1] < 0.05 * c["hist"]["ssd"][0]) and np.all(c["hist"]["ncc"][-1] > c["hist"]["ncc"][0])
    # align.match_projections on the statement is this file's loop: the same evaluations, the same maps
    from tomo_tv_amd.align import match_projections
    fake = FakeEngine(c["F"], c["G"])
    res = match_projections(fake, 1, 2, max_iter=30, margin=2)
    assert fake.calls == len(c["hist"]["step"]) and res["converged"].all()
    assert np.allclose(res["M"], c["M"], rtol=0, atol=1e-12)
    assert np.allclose(res["shift"], SN.decode(c["M"], N, ns)[0], rtol=0, atol=1e-10)
    # switched-off parameters stay exactly put through the loop, and a projection that has converged keeps its map
    res0 = match_projections(FakeEngine(c["F"], c["G"]), 1, 2, max_iter=6, margin=2, rotation=False, magnification=False)
    assert not res0["rotation_deg"].any() and np.all(res0["magnification"] == 1.0)
    assert np.all(res0["M"][:, [0, 1, 3, 4]] == [1.0, 0.0, 0.0, 1.0])
    one = match_projections(FakeEngine(c["F"], c["G"]), 1, 2, M0=np.where(np.arange(P)[:, None] == 0, c["M"], SN.identity(P)), max_iter=2,
                            tol_shift=0.05, tol_deg=0.05, tol_mag=1e-3, margin=2)
    assert one["converged"][0] and not one["step"][1][0].any()                        # frozen after its first (small) step
    far = np.tile([1, 0, 0.95 * N, 0, 1, 0], (P, 1)).astype(np.float64)
    far[1:] = SN.identity(P)[1:]
    with pytest.raises(RuntimeError, match=r"projections \[0\]"):
        match_projections(FakeEngine(c["F"], c["G"]), 1, 2, M0=far, margin=2)
