"""Affine resampling and the tilt-axis estimate without a GPU: the binary32 replay of the kernel's arithmetic against the binary64
statement and its derived bound (tests/ref64_affine.py), three deliberately wrong replays, ``align.affine_matrices``, the estimator on
the replayed case, ``TomoGPU``'s bookkeeping on an engine restated in numpy, and the ABI."""
import os
import re

import numpy as np
import pytest

import ref64_affine as F
import ref64_align as RA
from conftest import ROOT


def params(P, seed, span=3.0):
    """random rotations in +-10 degrees, magnifications in [0.9, 1.1], fractional shifts (binary32 numbers)"""
    rng = np.random.default_rng(seed)
    return (rng.uniform(-span, span, (P, 2)).astype(np.float32).astype(np.float64), rng.uniform(-10.0, 10.0, P), rng.uniform(0.9, 1.1, P))


@pytest.fixture(scope="module", params=[(8, 8), (33, 70)], ids=["8x8", "33x70"])
def case(request):
    N, ns = request.param
    P = 4
    X = np.random.default_rng(N + ns).random((P, N, ns), dtype=np.float32)
    sh, rot, mag = params(P, 17 + N)
    M = F.matrices(sh, rot, mag, N, ns)
    ref, _ = F.affine(X, M)
    return X, sh, rot, mag, M, ref, F.bound(X, M)


def test_kernel_replay_is_inside_the_bound(case):
    X, sh, rot, mag, M, ref, bound = case
    err = np.abs(F.affine_replay_f32(X, M).astype(np.float64) - ref)
    print(f"worst error / bound: {np.max(err / np.maximum(bound, 1e-300)):.3f}")
    assert np.all(err <= bound)
    # a rounding bound, not slack: a millionth of the largest sample
    assert np.all(bound <= 2e-6 * float(X.max()))


@pytest.mark.parametrize("wrong", ["transpose", "corner", "flip_sign"])
def test_bound_catches_a_wrong_replay(case, wrong):
    X, sh, rot, mag, M, ref, bound = case
    N, ns = X.shape[1:]
    bad = F.affine_replay_f32(X, F.matrices(sh, rot, mag, N, ns, **{wrong: True})).astype(np.float64)
    assert np.any(np.abs(bad - ref) > bound)
    assert np.mean(np.abs(bad - ref) > bound) > 0.5


def test_statement_is_the_definition_written_out():
    """a few elements of the binary64 statement by hand: taps, weights, zero outside"""
    X = np.random.default_rng(2).random((1, 6, 5))
    M = np.array([[1.0, 0.0, 0.25, 0.0, 1.0, -0.5]])           # r' = r + 0.25, s' = s - 0.5
    out, mag = F.affine(X, M)
    want = 0.75 * (0.5 * X[0, 2, 1] + 0.5 * X[0, 2, 2]) + 0.25 * (0.5 * X[0, 3, 1] + 0.5 * X[0, 3, 2])
    assert abs(out[0, 2, 2] - want) < 1e-15 and abs(mag[0, 2, 2] - want) < 1e-15
    assert abs(out[0, 5, 0] - 0.75 * 0.5 * X[0, 5, 0]) < 1e-15      # row 6 and slice -1 are outside: zero
    assert np.array_equal(F.affine(X, np.array([[1.0, 0, 0, 0, 1.0, 0]]))[0], X)
    assert not F.affine(X, np.array([[1.0, 0, 100.0, 0, 1.0, 0]]))[0].any()
    assert not F.affine(X, np.array([[1e300, 1e300, 0.0, -1e300, 0, 0]]))[0][0, 1:].any()
    assert np.array_equal(F.profile(X)[0], X[0].sum(axis=0))


def test_affine_matrices():
    from tomo_tv_amd.align import affine_matrices
    N, ns, P = 33, 70, 5
    sh, rot, mag = params(P, 3)
    # rotation 0, magnification 1: exact translations, scalars broadcast
    M = affine_matrices(sh, 0.0, 1.0, N, ns)
    assert M.shape == (P, 6) and M.dtype == np.float64
    assert np.array_equal(M, np.stack([np.ones(P), np.zeros(P), -sh[:, 0], np.zeros(P), np.ones(P), -sh[:, 1]], axis=1))
    assert np.array_equal(affine_matrices(sh, np.zeros(P), np.ones(P), N, ns), M)
    assert np.array_equal(affine_matrices(sh, 360.0, 1.0, N, ns), M)
    # ... which compose with the shifts exactly as the shift statement does
    X = np.random.default_rng(5).random((P, N, ns), dtype=np.float32)
    got, gmag = F.affine(X, M)
    ref, rmag = RA.shift(X, sh, wrap=False)
    assert np.all(np.abs(got - ref) <= 1e-15 * rmag) and np.all(np.abs(gmag - rmag) <= 1e-15 * rmag)
    # the general form is the definition (tests/ref64_affine.py: matrices), per projection and with scalars
    assert np.allclose(affine_matrices(sh, rot, mag, N, ns), F.matrices(sh, rot, mag, N, ns), rtol=0, atol=1e-12)
    assert np.allclose(affine_matrices(sh, 7.5, 1.05, N, ns), F.matrices(sh, 7.5, 1.05, N, ns), rtol=0, atol=1e-12)
    # quarter turns: cos and sin are the exact 0 and +-1, and on a square image +90 degrees is np.rot90, element for element
    for deg, lin in ((90.0, (0.0, 1.0, -1.0, 0.0)), (180.0, (-1.0, 0.0, 0.0, -1.0)), (270.0, (0.0, -1.0, 1.0, 0.0)), (-90.0, (0.0, -1.0, 1.0, 0.0))):
        m = affine_matrices(np.zeros((1, 2)), deg, 1.0, 16, 16)[0]
        assert (m[0], m[1], m[3], m[4]) == lin and m[2] == np.round(m[2]) and m[5] == np.round(m[5]), deg
    Q = np.random.default_rng(6).random((3, 16, 16))
    out, _ = F.affine(Q, affine_matrices(np.zeros((3, 2)), 90.0, 1.0, 16, 16))
    assert all(np.array_equal(out[a], np.rot90(Q[a])) for a in range(3))
    # the sense: +phi moves a sample on the +r side of the centre towards +s
    Z = np.zeros((1, 33, 33))
    Z[0, 28, 16] = 1.0
    out, _ = F.affine(Z, affine_matrices(np.zeros((1, 2)), 10.0, 1.0, 33, 33))
    _, r_cm, s_cm = RA.moments(out)[0] / out.sum()
    assert s_cm > 16.5 and r_cm < 28.0
    with pytest.raises(ValueError):
        affine_matrices(sh, 0.0, 0.0, N, ns)


@pytest.fixture(scope="module")
def axis():
    ang, clean, X = F.axis_case()
    c = F.AXIS_CASE
    return ang, clean, X, F.estimate(X, np.zeros((c["nproj"], 2)), c["search_deg"], c["step_deg"])


def test_estimator_replay_finds_the_injected_rotation(axis):
    """(Nslice, N, P) = (32, 32, 9), every projection rotated by phi0 = 3 degrees: the binary64 replay returns -phi0 within half a
    grid step, from an interior grid minimum; the series before the rotation scores two orders below the best candidate's neighbours"""
    ang, clean, X, (rot, k, border, g, sc) = axis
    c = F.AXIS_CASE
    print(f"replay: grid minimum {g[k]} (index {k}), after the parabola {rot:.6f}; scores beside it {sc[k - 1]:.3e} {sc[k]:.3e} {sc[k + 1]:.3e}")
    assert abs(rot + c["phi0"]) <= 0.5 * c["step_deg"] and not border
    assert k == F.AXIS_REPLAY["index"] and abs(rot - F.AXIS_REPLAY["rotation"]) < 1e-3
    assert abs(rot - g[k]) <= 0.5 * c["step_deg"]
    # zero border: nothing of the rotated series reaches the image's edge, and the clean series is a common-line series
    assert not X[:, :2].any() and not X[:, -2:].any() and not X[:, :, :2].any() and not X[:, :, -2:].any()
    assert F.score(F.profile(clean), F.score_border(c["n"], c["search_deg"])) < 0.05 * sc[k]


def test_package_estimator_pieces_equal_the_statement(axis):
    from tomo_tv_amd import align
    ang, clean, X, (rot, k, border, g, sc) = axis
    c = F.AXIS_CASE
    assert np.array_equal(align.axis_grid(c["search_deg"], c["step_deg"]), g) and len(g) == 41 and g[0] == -10.0 and g[-1] == 10.0
    H = align.axis_score_border(c["n"], c["search_deg"])
    assert H == F.score_border(c["n"], c["search_deg"]) == 3
    prof = F.profile(X)
    assert abs(align.axis_score(prof, H) - F.score(prof, H)) <= 1e-12 * F.score(prof, H)
    got = align.axis_minimum(g, sc)
    assert got[1:] == (k, border) and abs(got[0] - rot) < 1e-12
    # a minimum on the grid's border: flagged, not refined
    assert align.axis_minimum(g, np.arange(len(g), dtype=np.float64)) == (g[0], 0, True) == F.minimum(g, np.arange(len(g), dtype=np.float64))
    assert align.axis_minimum(g, -np.arange(len(g), dtype=np.float64))[1:] == (len(g) - 1, True)
    # the parabola: exact for a parabola, clamped to half a step
    assert abs(align.axis_minimum(g, (g - 1.2) ** 2)[0] - 1.2) < 1e-12
    with pytest.raises(ValueError):
        align.axis_score(prof, 16)


class NumpyEngine:
    """the five engine calls ``TomoGPU``'s alignment uses, restated with the binary64 statements; records what was called"""

    def __init__(self, X):
        self.P, self.N, self.ns = X.shape
        self.slots, self.calls = {}, []

    def _align_one_engine(self):
        pass

    def set_tilt_series(self, b):
        self.slots[0] = RA.images(b, self.N).astype(np.float64)

    def sino_shift(self, src, dst, shifts, wrap=False):
        self.calls.append(("shift", src, dst))
        self.slots[dst] = RA.shift(self.slots[src], np.asarray(shifts, np.float32), wrap=wrap)[0]

    def sino_affine(self, src, dst, M):
        self.calls.append(("affine", src, dst))
        self.slots[dst] = F.affine(self.slots[src], M)[0]

    def sino_axis_profile(self, which):
        return F.profile(self.slots[which])


def numpy_rec(X):
    from tomo_tv_amd.reconstructor import TomoGPU
    rec = object.__new__(TomoGPU)
    rec.tomo = NumpyEngine(X)
    rec.set_tilt_series(np.ascontiguousarray(X.transpose(2, 1, 0)))
    return rec


def test_tomogpu_alignment_bookkeeping(axis):
    from tomo_tv_amd import align
    from tomo_tv_amd._lib import SINO_B
    ang, clean, X, (rot, k, border, g, sc) = axis
    P, N, ns = X.shape
    rec = numpy_rec(X)
    eng = rec.tomo
    sh = np.array([[1.5, -2.25]] * P)
    # nothing stored, no keyword: today's calls and nothing else
    rec.set_alignment(sh)
    assert eng.calls == [("shift", SINO_B, rec.ALIGN_SLOT), ("shift", rec.ALIGN_SLOT, SINO_B)]
    assert all(np.array_equal(v, w) for v, w in zip(rec.get_alignment_rotation(), (np.zeros(P), np.ones(P))))
    with pytest.raises(ValueError):
        rec.set_alignment(sh, wrap=True, rotation_deg=1.0)
    assert getattr(rec, "_align_rot", None) is None                       # the refused call stored nothing
    # the estimator equals the statement's, uses the scratch slot and leaves the series alone until it applies
    del eng.calls[:]
    before = eng.slots[SINO_B].copy()
    got = rec.estimate_tilt_axis_rotation(F.AXIS_CASE["search_deg"], F.AXIS_CASE["step_deg"], apply=False)
    assert len({rec.ALIGN_SLOT, rec.ALIGN_MODEL_SLOT, rec.ALIGN_SCRATCH_SLOT, SINO_B}) == 4
    assert eng.calls == [("affine", rec.ALIGN_SLOT, rec.ALIGN_SCRATCH_SLOT)] * len(g) and np.array_equal(eng.slots[SINO_B], before)
    want = F.estimate(X, sh, F.AXIS_CASE["search_deg"], F.AXIS_CASE["step_deg"])
    assert abs(got - want[0]) < 1e-9 and np.allclose(rec.align_axis_scores[1], want[4], rtol=1e-9, atol=0) and not rec.align_axis_at_border
    assert np.array_equal(rec.align_axis_scores[0], g) and getattr(rec, "_align_rot", None) is None
    # apply: one affine pass of the series as given by the shifts and the rotation together; both remembered
    got = rec.estimate_tilt_axis_rotation(F.AXIS_CASE["search_deg"], F.AXIS_CASE["step_deg"])
    assert eng.calls[-1] == ("affine", rec.ALIGN_SLOT, SINO_B)
    assert np.array_equal(eng.slots[SINO_B], F.affine(X, align.affine_matrices(sh, got, 1.0, N, ns))[0])
    assert np.array_equal(rec.get_alignment(), sh) and np.array_equal(rec.get_alignment_rotation()[0], np.full(P, got))
    # a later call that names no rotation keeps it (no compounding: the kept copy again), a magnification joins it
    sh2 = sh + 0.5
    rec.set_alignment(sh2)
    assert np.array_equal(eng.slots[SINO_B], F.affine(X, align.affine_matrices(sh2, got, 1.0, N, ns))[0])
    rec.set_alignment(sh2, magnification=1.05)
    assert np.array_equal(eng.slots[SINO_B], F.affine(X, align.affine_matrices(sh2, got, 1.05, N, ns))[0])
    assert np.array_equal(rec.get_alignment_rotation()[1], np.full(P, 1.05))
    with pytest.raises(ValueError):
        rec.set_alignment(sh2, wrap=True)
    with pytest.raises(ValueError):
        rec.estimate_tilt_axis_rotation(search_deg=80.0)
    # a new series drops everything
    rec.set_tilt_series(np.ascontiguousarray(X.transpose(2, 1, 0)))
    assert not rec._align_kept and rec._align_shifts is None and rec._align_rot is None


def test_symbols_in_header_library_and_table():
    from tomo_tv_amd import _lib
    src = open(os.path.join(ROOT, "include", "tomo_hip.h")).read()
    L = _lib.load()
    for name, nargs in (("tomo_sino_affine", 4), ("tomo_sino_axis_profile", 3)):
        assert re.search(r"\bint %s\s*\(" % name, src), name
        assert hasattr(L, name) and len(_lib.SIGNATURES[name]) == nargs
        args = [None if t is _lib._p else 0 for t in _lib.SIGNATURES[name]]
        assert getattr(L, name)(*args) == 1 and L.tomo_last_error()      # null engine: TOMO_ERR_ARG, no crash
    assert "m00 r + m01 s + m02" in src and "copies the" in src


def test_sharded_and_group_classes_refuse_the_new_calls():
    from tomo_tv_amd import engine, inprocess
    sharded = object.__new__(engine.tomoengine)
    sharded.comm, sharded.sub_slabs, sharded.be = object(), 1, None
    subslab = object.__new__(engine.tomoengine)
    subslab.comm, subslab.sub_slabs, subslab.be = None, 2, object.__new__(engine._GroupBackend)
    for eng in (sharded, subslab):
        eng.Nproj = eng.Nslice_ = 3
        for call in (lambda: eng.sino_affine(0, 3, np.zeros((3, 6))), lambda: eng.sino_axis_profile(0)):
            with pytest.raises(NotImplementedError):
                call()
    group = object.__new__(engine._GroupBackend)
    for name in ("sino_affine", "sino_axis_profile"):
        with pytest.raises(NotImplementedError):
            group.c(name, 0, None)
        with pytest.raises(NotImplementedError):
            getattr(inprocess.InProcessMultiGPU, name)(None, 0)
