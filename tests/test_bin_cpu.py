"""Binning and prolongation without a GPU: the binary64 statements (tests/ref64_bin.py) against plain loops, the binary32 replays of
the kernels' arithmetic against the derived bounds, three deliberately wrong replays, the scale convention against the oracle's
matrices, projection matching over a pyramid replayed on the CPU, ``TomoGPU``'s new drivers on an engine restated in numpy, the ABI."""
import os
import re

import numpy as np
import pytest

import ref64_align as RA
import ref64_bin as B
from conftest import ROOT


def mixed(shape, seed):
    return (np.random.default_rng(seed).random(shape, dtype=np.float32) - np.float32(0.4)) * np.float32(3.0)


CONST = np.float32(0.7).view(np.uint32).__and__(np.uint32(0xFFFFFFF0)).view(np.float32)      # 0.7 with its last 4 mantissa bits cleared
CASES = [(2, 8, 5, 3), (2, 16, 130, 2), (4, 12, 70, 3), (4, 16, 64, 2), (4, 8, 7, 2)]       # (f, N, Nslice, P); the last has k = 3


@pytest.mark.parametrize("f,N,ns,P", CASES)
def test_statements_equal_the_loops_and_replays_are_inside_the_bounds(f, N, ns, P):
    X, V = mixed((P, N, ns), N + ns), mixed((ns, N, N), N + ns + 1)
    sb, sbound = B.bin_sino(X, f)
    vb, vbound = B.bin_volume(V, f)
    assert sb.shape == (P, N // f, -(-ns // f)) and vb.shape == (-(-ns // f), N // f, N // f)
    if N * ns <= 16 * 70:
        assert np.allclose(sb, B.bin_sino_loops(X, f), rtol=1e-14, atol=1e-15) and np.allclose(vb, B.bin_volume_loops(V, f), rtol=1e-14, atol=1e-15)
    for got, ref, bound in ((B.bin_replay_f32(X, f), sb, sbound), (B.bin_replay_f32(V, f, volume=True), vb, vbound)):
        err = np.abs(got.astype(np.float64) - ref)
        print(f"bin: worst error / bound {np.max(err / np.maximum(bound, 1e-300)):.3f}")
        assert np.all(err <= bound)
        assert np.all(bound <= 64 * 2.0 ** -24 * float(np.abs(X).max() + np.abs(V).max()))      # a rounding bound, not slack
    C = mixed((-(-ns // f), N // f, N // f), 5 * N)
    ref, bound = B.prolong(C, f, ns)
    assert ref.shape == (ns, N, N)
    if N * ns <= 12 * 70:
        assert np.allclose(ref, B.prolong_loops(C, f, ns), rtol=1e-13, atol=1e-14)
    err = np.abs(B.prolong_replay_f32(C, f, ns).astype(np.float64) - ref)
    print(f"prolong: worst error / bound {np.max(err / np.maximum(bound, 1e-300)):.3f}")
    assert np.all(err <= bound) and np.all(bound <= 13 * 2.0 ** -24 * float(np.abs(C).max()))


@pytest.mark.parametrize("f,N,ns,P", [c for c in CASES if c[2] % c[0]])
def test_bound_catches_a_partial_bin_scaled_as_a_full_one(f, N, ns, P):
    X = mixed((P, N, ns), 3)
    ref, bound = B.bin_sino(X, f)
    bad = np.abs(B.bin_replay_f32(X, f, partial_as_full=True).astype(np.float64) - ref) > bound
    assert not bad[:, :, :-1].any() and np.mean(bad[:, :, -1]) > 0.9
    V = mixed((ns, N, N), 4)
    ref, bound = B.bin_volume(V, f)
    bad = np.abs(B.bin_replay_f32(V, f, volume=True, partial_as_full=True).astype(np.float64) - ref) > bound
    assert not bad[:-1].any() and np.mean(bad[-1]) > 0.9


@pytest.mark.parametrize("wrong", [dict(half_cell=False), dict(clamp=False)], ids=["no_half_cell", "no_clamp"])
@pytest.mark.parametrize("f", [2, 4])
def test_bound_catches_wrong_prolongation_taps(f, wrong):
    C = mixed((5, 4, 4), 9) + np.float32(2.0)
    ref, bound = B.prolong(C, f, 5 * f - 1)
    bad = np.abs(B.prolong_replay_f32(C, f, 5 * f - 1, **wrong).astype(np.float64) - ref) > bound
    assert bad.any()
    if "half_cell" in wrong:
        assert np.mean(bad) > 0.5
    else:
        assert bad[0].all() and bad[:, 0].all() and bad[:, :, 0].all()        # the faces the clamp serves


def test_bit_identities_of_the_replays():
    for f in (2, 4):
        const = np.full((3, 4, 4), np.float32(0.3))
        assert np.all(B.prolong_replay_f32(const, f, 3 * f - 1) == np.float32(0.3))
        edge = B.prolong_replay_f32(mixed((3, 4, 4), 1), f, 3 * f)
        C = mixed((3, 4, 4), 1)
        assert edge[0, 0, 0] == C[0, 0, 0] and edge[-1, -1, -1] == C[-1, -1, -1]        # all three axes clamped: a copy
        # the sum is sequential: j * const must be a binary32 number for j <= f k, so the constant keeps 4 spare mantissa bits
        X = np.full((2, 8, 4 * f + 1), CONST)
        out = B.bin_replay_f32(X, f)
        assert np.all(out[:, :, :-1] == CONST / np.float32(f)) and out[0, 0, -1] == CONST / np.float32(f)        # k = f and k = 1
        # an Inf sample: its bin is Inf, its clamped copies are Inf, nothing beside a clamped copy is NaN because of the clamp
        X[1, 3, 2] = np.inf
        out = B.bin_replay_f32(X, f)
        assert np.isinf(out[1, 3 // f, 2 // f]) and np.isfinite(out).sum() == out.size - 1
        C[0, 0, 0] = np.inf
        fine = B.prolong_replay_f32(C, f, 3 * f)
        assert np.all(fine[:f // 2, :f // 2, :f // 2] == np.inf)


def dense(N, ang):
    import oracle
    A3 = oracle.parallel_ray(N, np.asarray(ang, np.float64))
    A = np.zeros((len(ang) * N, N * N))
    np.add.at(A, (A3[0].astype(int), A3[1].astype(int)), A3[2].astype(np.float64))
    return A


def scale_gap(f, N, ns, ang):
    """max |A_coarse bin_volume(x) - bin_sino(A_fine x)| relative to the largest coarse sample"""
    V = np.random.default_rng(N).random((ns, N, N))
    Af, Ac = dense(N, ang), dense(N // f, ang)
    fine = np.stack([(Af @ V[s].ravel()).reshape(len(ang), N) for s in range(ns)], axis=2)             # X[a][r][s]
    Vc = B.bin_volume(V, f)[0]
    coarse = np.stack([(Ac @ Vc[s].ravel()).reshape(len(ang), N // f) for s in range(Vc.shape[0])], axis=2)
    want = B.bin_sino(fine, f)[0]
    return float(np.abs(coarse - want).max() / np.abs(want).max())


@pytest.mark.parametrize("f,N,ns", [(2, 16, 5), (4, 16, 6)])
def test_scale_convention_against_the_oracles_matrices(f, N, ns):
    """At 0 and 90 degrees a ray runs along a pixel row: projecting the binned volume with the coarse matrix IS binning the fine
    projections (mean of f x k samples divided by f), to the rounding of the binary32 matrix entries.  At an oblique angle the two
    differ by the discretisation of the strip model only (printed, recorded in DESIGN 8g, not asserted)."""
    gap = scale_gap(f, N, ns, [0.0, 90.0])
    print(f"f = {f}: axis-aligned gap {gap:.3e}, at 33 degrees {scale_gap(f, N, ns, [33.0]):.3e}")
    assert gap <= 1e-6


# ---- projection matching over a pyramid, replayed --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pyr():
    c = B.PYRAMID_CASE
    ang, clean, X, inj = B.pyramid_case()
    return c, ang, X, inj, B.pyramid_replay(ang, X, c["pyramid"], c["nouter"], c["max_shift"], c["niter"])


def test_one_level_cannot_recover_what_the_pyramid_does(pyr):
    c, ang, X, inj, (hist, pks, borders) = pyr
    assert np.abs(inj).max() == c["span"] > 2 * c["max_shift"]
    h1, _, b1 = B.pyramid_replay(ang, X, (1,), c["nouter"], c["max_shift"], c["niter"])
    r1 = RA.gauge_residual(h1[-1], inj, ang)
    print("one level: flagged per pass", [int(b.sum()) for b in b1], "left outside the gauge", np.abs(r1[0]).max(), np.abs(r1[1]).max())
    assert b1[0].sum() >= 5 and max(np.abs(r1[0]).max(), np.abs(r1[1]).max()) > c["max_shift"]
    rr, rs = RA.gauge_residual(hist[-1], inj, ang)
    print("pyramid: flagged per pass", [int(b.sum()) for b in borders], "left outside the gauge", np.abs(rr).max(), np.abs(rs).max())
    assert len(hist) == 3 * c["nouter"] and np.abs(rr).max() <= 1.0 and np.abs(rs).max() <= 1.0
    for k, pk in enumerate(pks):                                       # peaks of a level are whole multiples of its factor
        assert np.array_equal(pk % c["pyramid"][k // c["nouter"]], np.zeros_like(pk))


# ---- TomoGPU on an engine restated in numpy ------------------------------------------------------------------------------------------
class NumpyEngine:
    """the engine calls ``binned``, ``coarse_to_fine`` and ``refine_alignment`` use: the oracle's SIRT and projector, the binary64
    correlation and shift, the binary32 replay of the binning, the binary64 prolongation; every call is logged with its level"""

    def __init__(self, ns, N, ang, log, level=1):
        import oracle
        self.ns, self.N, self.ang, self.P, self.calls, self.level = ns, N, np.asarray(ang, np.float64), len(ang), log, level
        self.o = oracle.ctvlib(ns, N, self.P)
        self.o.load_A(oracle.parallel_ray(N, self.ang))
        self.slots = {}

    def _log(self, *what):
        self.calls.append((self.level,) + what)

    def _align_one_engine(self):
        pass

    def initialize_SIRT(self):
        pass

    initialize_FP = initialize_SIRT

    def set_tilt_series(self, b):
        self.slots[0] = RA.images(b, self.N).astype(np.float32)

    def binned_engine(self, f):
        self._log("binned_engine", f)
        return NumpyEngine(-(-self.ns // f), self.N // f, self.ang, self.calls, self.level * f)

    def bin_sinogram_to(self, coarse, f, src=0, dst=0):
        self._log("bin", f)
        assert coarse.level == self.level * f
        coarse.slots[dst] = B.bin_replay_f32(self.slots[src], f)

    def prolong_volume_to(self, fine, f, src=0, dst=0):
        self._log("prolong", f)
        assert self.level == fine.level * f
        fine.o.recon[:] = B.prolong(self.o.recon, f, fine.ns)[0].astype(np.float32)

    def restart_recon(self):
        self._log("restart")
        self.o.restart_recon()

    def SIRT(self, n=1):
        self._log("SIRT", n)
        self.o.set_tilt_series(RA.packed(self.slots[0]))
        self.o.SIRT_norm(n)

    def data_distance(self):
        self.o.set_tilt_series(RA.packed(self.slots[0]))
        return self.o.data_distance(normalize=False)

    def forward_projection(self):
        self._log("fp")
        self.o.forward_projection()
        self.slots[1] = RA.images(self.o.g, self.N)

    def sino_xcorr(self, a, b, S, subtract_mean=True):
        self._log("xcorr", a, b, S)
        return RA.xcorr(self.slots[a], self.slots[b], S, subtract_mean)

    def sino_shift(self, src, dst, shifts, wrap=False):
        self._log("shift", src, dst)
        self.slots[dst] = RA.shift(self.slots[src], np.asarray(shifts, np.float32), wrap=wrap)[0].astype(np.float32)


def numpy_rec(ang, X):
    from tomo_tv_amd.reconstructor import TomoGPU
    rec = object.__new__(TomoGPU)
    rec.tomo = NumpyEngine(X.shape[2], X.shape[1], ang, [])
    rec.verbose = False
    rec.set_tilt_series(np.ascontiguousarray(np.asarray(X).transpose(2, 1, 0)))
    return rec


@pytest.fixture(scope="module")
def small():
    c = dict(RA.PLAIN_CASE, nslice=13, n=16, nproj=7)
    ang, clean, X, inj = RA.refine_case(c)
    return ang, clean, X


def test_binned_builds_the_coarse_object_on_the_engine(small):
    ang, clean, X = small
    rec = numpy_rec(ang, clean)
    for f in (2, 4):
        c = rec.binned(f)
        assert (c.Nslice, c.Nray, c.Nangles) == (-(-13 // f), 16 // f, 7) and c.tomo.level == f and c.recon is None
        assert np.array_equal(c.tomo.slots[0], B.bin_replay_f32(clean, f))
        assert rec.tomo.calls[-2:] == [(1, "binned_engine", f), (1, "bin", f)]
        assert c.get_alignment().shape == (7, 2) and not c.get_alignment().any()
    for bad in (3, 1, 8):
        with pytest.raises(ValueError):
            rec.binned(bad)
    odd = numpy_rec(ang, clean[:, :14])
    with pytest.raises(ValueError):
        odd.binned(4)
    assert odd.binned(2).Nray == 7


def test_coarse_to_fine_composes_the_engine_calls(small):
    ang, clean, X = small
    rec = numpy_rec(ang, clean)
    costs = rec.coarse_to_fine((4, 2), Niter=(3, 2, 1))
    assert [len(c) for c in costs] == [3, 2, 1] and rec.cost is costs[2]
    assert rec.tomo.calls == [(1, "binned_engine", 4), (1, "bin", 4), (4, "restart")] + [(4, "SIRT", 1)] * 3 + \
        [(1, "binned_engine", 2), (1, "bin", 2), (4, "prolong", 2)] + [(2, "SIRT", 1)] * 2 + [(2, "prolong", 2), (1, "SIRT", 1)]
    # the same by hand, from zero: the warm start is what the last level continues from (no restart in between)
    import oracle
    lv = {f: oracle.ctvlib(-(-13 // f), 16 // f, 7) for f in (4, 2, 1)}
    for f, o in lv.items():
        o.load_A(oracle.parallel_ray(16 // f, ang))
        o.set_tilt_series(RA.packed(clean if f == 1 else B.bin_replay_f32(clean, f)))
    lv[4].SIRT_norm(3)
    lv[2].recon[:] = B.prolong(lv[4].recon, 2, 7)[0]
    lv[2].SIRT_norm(2)
    lv[1].recon[:] = B.prolong(lv[2].recon, 2, 13)[0]
    lv[1].SIRT_norm(1)
    assert np.array_equal(rec.tomo.o.recon, lv[1].recon) and costs[2][0] == lv[1].data_distance(normalize=False)
    # a later call re-uses the kept objects (no new engine) and bins the series again; a new series drops them
    kept = dict(rec._pyramid)
    del rec.tomo.calls[:]
    rec.coarse_to_fine((2,), Niter=(1, 1))
    assert rec._pyramid[2] is kept[2] and not any(c[1] == "binned_engine" for c in rec.tomo.calls) and rec.tomo.calls[0] == (1, "bin", 2)
    rec.set_tilt_series(np.ascontiguousarray(clean.transpose(2, 1, 0)))
    assert rec._pyramid == {}
    for kw in (dict(factors=(2, 4)), dict(factors=(3,), Niter=(1, 1)), dict(Niter=(1, 1)), dict(alg="CGLS"), dict(factors=(4, 4))):
        with pytest.raises(ValueError):
            rec.coarse_to_fine(**kw)


def test_refine_alignment_pyramid_follows_the_replay_and_none_is_the_plain_path(small):
    from tomo_tv_amd._lib import SINO_B, SINO_G
    ang, clean, X = small
    few = lambda r: r.sirt_calls.append(r.tomo.level) or (r.tomo.restart_recon(), r.tomo.SIRT(5))   # noqa: E731
    from tomo_tv_amd.reconstructor import TomoGPU
    TomoGPU.sirt_calls = []
    try:
        rec = numpy_rec(ang, X)
        total = rec.refine_alignment(Nouter=2, max_shift=2, recon=few, subpixel=False, pyramid=(4, 2, 1))
        hist, pks, borders = B.pyramid_replay(ang, X, (4, 2, 1), 2, 2, 5)
        assert TomoGPU.sirt_calls == [4, 4, 2, 2, 1, 1]                   # recon is handed the level's object
        assert len(rec.align_history) == len(rec.align_peaks) == len(rec.align_int_peaks) == len(rec.align_at_border) == 6
        for k in range(6):
            assert np.array_equal(rec.align_peaks[k], pks[k]) and np.array_equal(rec.align_history[k], hist[k]), k
            assert np.array_equal(rec.align_int_peaks[k], pks[k]) and np.array_equal(rec.align_at_border[k], borders[k])
        assert np.array_equal(total, hist[-1]) and np.array_equal(rec.tomo.slots[SINO_B], RA.shift_int(X, total))
        assert any(p.any() for p in pks[:2]) and all(not (p % 4).any() for p in pks[:2])
        # pyramid=None and pyramid=(1,): today's pass, call for call -- no coarse object, nothing binned
        logs = []
        for kw in (dict(), dict(pyramid=None), dict(pyramid=(1,))):
            r = numpy_rec(ang, X)
            r.refine_alignment(Nouter=2, max_shift=2, recon=few, subpixel=False, **kw)
            logs.append((list(r.tomo.calls), r.get_alignment()))
            assert r._pyramid == {}
        one = [(1, "restart"), (1, "SIRT", 5), (1, "fp"), (1, "xcorr", SINO_G, SINO_B, 2), (1, "shift", rec.ALIGN_SLOT, SINO_B)]
        assert logs[0][0] == [(1, "shift", SINO_B, rec.ALIGN_SLOT)] + one * 2
        assert logs[1][0] == logs[0][0] == logs[2][0] and np.array_equal(logs[1][1], logs[0][1]) and np.array_equal(logs[2][1], logs[0][1])
        with pytest.raises(ValueError):
            rec.refine_alignment(pyramid=(3,))
    finally:
        del TomoGPU.sirt_calls


def test_symbols_in_header_library_and_table():
    from tomo_tv_amd import _lib
    src = open(os.path.join(ROOT, "include", "tomo_hip.h")).read()
    L = _lib.load()
    for name in ("tomo_sino_bin", "tomo_volume_bin", "tomo_volume_prolong"):
        assert re.search(r"\bint %s\s*\(" % name, src), name
        assert hasattr(L, name) and _lib.SIGNATURES[name] == [_lib._p, _lib._i, _lib._p, _lib._i, _lib._i]
        assert getattr(L, name)(None, 0, None, 0, 2) == 1 and L.tomo_last_error()      # null engines: TOMO_ERR_ARG, no crash
    assert "1 / (f^2 k)" in src and "ordinary cell" in src and "clamped edge copies" in src


def test_sharded_group_and_inprocess_classes_refuse():
    from tomo_tv_amd import engine, inprocess
    sharded = object.__new__(engine.tomoengine)
    sharded.comm, sharded.sub_slabs, sharded.be = object(), 1, None
    subslab = object.__new__(engine.tomoengine)
    subslab.comm, subslab.sub_slabs, subslab.be = None, 2, object.__new__(engine._GroupBackend)
    whole = object.__new__(engine.tomoengine)
    whole.comm, whole.sub_slabs, whole.be = None, 1, object.__new__(engine._SlabBackend)
    for eng in (sharded, subslab):
        for call in (eng.bin_sinogram_to, eng.bin_volume_to, eng.prolong_volume_to):
            with pytest.raises(NotImplementedError):
                call(whole, 2)
        with pytest.raises(NotImplementedError):
            whole.bin_sinogram_to(eng, 2)                                              # ... as the partner too
        with pytest.raises(NotImplementedError):
            eng.binned_engine(2)
    group = object.__new__(engine._GroupBackend)
    for name in ("sino_bin", "volume_bin", "volume_prolong"):
        with pytest.raises(NotImplementedError):
            group.c(name, 0, None, 0, 2)
    for name in ("bin_sinogram_to", "bin_volume_to", "prolong_volume_to"):
        with pytest.raises(NotImplementedError):
            getattr(inprocess.InProcessMultiGPU, name)(None, whole, 2)
    whole.be = None                                                                    # (nothing to destroy)
    subslab.be = None
