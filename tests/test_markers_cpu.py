"""Marker alignment without a GPU: the plain statements of tests/ref64_markers.py against brute force, the a-priori bound against the
binary32 replay (and against the form the kernel must not use), the host rules of tomo_tv_amd/align.py, the ABI of the two calls, and
the yardstick of the GPU end-to-end test."""
import os
import re

import numpy as np
import pytest

import ref64
import ref64_affine
import ref64_markers as R
import sequences as S
import sequences_markers as SM
from conftest import ROOT
from tomo_tv_amd import align

F32 = np.float32
CALLS = ("tomo_sino_template_ncc", "tomo_sino_peaks")


def series(P, N, ns, seed, pedestal=3.0):
    rng = np.random.default_rng(seed)
    return (rng.uniform(0.5, 1.5, (P, N, ns)) + pedestal * np.arange(1, P + 1)[:, None, None]).astype(F32)


@pytest.mark.parametrize("Rt", [1, 2, 3])
def test_ncc_statement_against_a_double_loop(Rt):
    X, T = series(2, 9, 8, Rt), SM.template(Rt)
    X[1, 5:, 3:] = F32(2.5)                                                         # a flat corner: zeroed by the floor
    got, _, band = R.ncc(X, T, 1e-6)
    t = R.prepare_template(T).astype(np.float64)
    assert abs((t * t).sum() - 1) < 1e-6 and abs(t.sum()) < 1e-6
    W = 2 * Rt + 1
    want = np.zeros(X.shape)
    for a in range(2):
        for r in range(Rt, 9 - Rt):
            for s in range(Rt, 8 - Rt):
                w = X[a, r - Rt:r + Rt + 1, s - Rt:s + Rt + 1].astype(np.float64)
                d = w - w.mean()
                v = (d * d).sum()
                want[a, r, s] = (t * d).sum() / np.sqrt(v) if v > float(F32(1e-6) * F32(W * W)) else 0.0
    assert np.allclose(got, want, rtol=1e-12, atol=1e-14) and not band.any() and np.abs(got).max() <= 1 + 1e-12
    if Rt < 3:
        assert not got[1, 5 + Rt:9 - Rt, 3 + Rt:8 - Rt].any()
    assert not R.ncc(series(1, 4, 9, 0), SM.template(2))[0].any()                    # an image smaller than the template: all zero


@pytest.mark.parametrize("Rt", [1, 2, 5, 8])
def test_bound_holds_for_the_replay_and_not_for_the_cancelling_form(Rt):
    """pedestals 100, 200, 300 under noise of width 1: sumsq - sum^2 / W loses (x / d)^2 = 1e4 .. 1e5 ulps, the bound allows about W"""
    X, T = series(3, 33, 40, 11 + Rt, pedestal=100.0), SM.template(Rt)
    want, bound, band = R.ncc(X, T, 1e-4)
    assert not band.any() and np.all(np.isfinite(bound)) and bound.max() < 1e-3
    err = np.abs(R.ncc_replay32(X, T, 1e-4) - want)
    wrong = np.abs(R.ncc_wrong32(X, T, 1e-4) - want)
    print(f"R={Rt}: replay worst error / bound {np.max(err / np.maximum(bound, 1e-300)):.3f}, cancelling form "
          f"{np.max(wrong / np.maximum(bound, 1e-300)):.1f}")
    assert np.all(err <= bound)
    assert np.any(wrong > bound)


def brute_peaks(X, radius, thr):
    P, N, ns = X.shape
    out = np.zeros(X.shape, bool)
    for a in range(P):
        for r in range(N):
            for s in range(ns):
                x = X[a, r, s]
                ok = bool(x >= thr)
                for rr in range(max(0, r - radius), min(N, r + radius + 1)):
                    for ss in range(max(0, s - radius), min(ns, s + radius + 1)):
                        if (rr, ss) != (r, s):
                            ok = ok and bool(x > X[a, rr, ss] if (rr, ss) < (r, s) else x >= X[a, rr, ss])
                out[a, r, s] = ok
    return out


@pytest.mark.parametrize("radius", [1, 2, 3])
def test_peak_rule_against_brute_force(radius):
    rng = np.random.default_rng(radius)
    X = rng.integers(0, 4, (3, 9, 11)).astype(F32)
    X[0, 4, 3:8] = 9.0                                                               # a plateau
    X[1, 2, 2] = X[1, 2, 2 + radius] = X[1, 2 + radius + 1, 2] = 8.0                  # ties inside and just outside the window
    X[1, 0, 0] = X[1, 8, 10] = 7.0                                                   # image corners
    X[2, 5, 5] = np.nan
    for thr in (0.0, 3.0, 8.0):
        with np.errstate(invalid="ignore"):
            want = brute_peaks(X, radius, thr)
        assert np.array_equal(R.peak_mask(X, radius, thr), want)
        n, rec = R.peaks(X, radius, thr)
        assert np.array_equal(n, want.sum((1, 2)))
    assert R.peak_mask(X, radius, 0.0)[0, 4, 3] and not R.peak_mask(X, radius, 0.0)[0, 4, 4:8].any()      # the first of a plateau only
    assert not R.peak_mask(X, radius, 0.0)[2, 5 - radius:5 + radius + 1, 5 - radius:5 + radius + 1].any()  # nothing next to a NaN
    n, rec = R.peaks(X, 1, 3.0)
    r0 = rec[1][0]
    assert tuple(r0[:2]) == (0, 0) and np.array_equal(r0[2:7].view(F32), [7.0, 7.0, X[1, 1, 0], 7.0, X[1, 0, 1]]) and r0[7] == 0
    assert all(np.all(np.diff(r[:, 0] * 11 + r[:, 1]) > 0) for r in rec)


def test_positions_and_template():
    rec = np.zeros((2, 8), np.int32)
    rec[0, :2], rec[1, :2] = (4, 7), (0, 3)
    rec[0, 2:7] = np.array([1.0, 0.5, 0.75, 0.25, 0.25], F32).view(np.int32)
    rec[1, 2:7] = np.array([1.0, 1.0, 0.5, 0.5, 0.75], F32).view(np.int32)            # on the border r = 0: the upper neighbour repeats x
    pos = align.marker_positions(rec)
    assert np.array_equal(pos, R.positions(rec)) and pos[0, 0] == 4 + 0.5 * (0.5 - 0.75) / (0.5 - 2 + 0.75) and pos[0, 1] == 7.0
    assert align.marker_positions(rec, (9, 9))[1, 0] == 0.0 and align.marker_positions(rec, (9, 9))[1, 1] == pos[1, 1]
    T = align.marker_template(2.0, 4)
    assert T.shape == (9, 9) and T[4, 4] == 1 and T[0, 0] == 0 and T[4, 6] == 0.5 and np.array_equal(T, T.T) and np.array_equal(T, T[::-1])
    assert abs(T.sum() - np.pi * 4) < 0.2 and np.array_equal(align.marker_template(2.0, 4, bright=False), -T)
    for bad in ((0.0, 3), (9.0, 2), (2.0, 0)):
        with pytest.raises(ValueError):
            align.marker_template(*bad)


def test_detector_coordinate_against_the_forward_projection():
    """single-voxel phantoms on both sides of both axes: the peak of the projected row within 0.5 px of the prediction at every angle"""
    N, ang = 16, np.linspace(-70, 70, 8)
    M, U = ref64.Matrix(N, ang), align.marker_detector_coordinate(ang, N)
    for iy, iz in ((3, 4), (12, 5), (4, 12), (11, 11), (8, 2), (2, 8)):
        v = np.zeros((1, N, N), F32)
        v[0, iy, iz] = 1
        b = R.images(M.fp(v), N)[:, :, 0]
        pred = 0.5 * (N - 1) + U @ np.array([iy - 0.5 * (N - 1), iz - 0.5 * (N - 1)])
        assert np.all(np.abs(np.argmax(b, axis=1) - pred) <= 0.5), (iy, iz)
        assert np.all(np.abs((b * np.arange(N)).sum(1) / b.sum(1) - pred) <= 0.5)


def synthetic(J=6, P=15, N=64, ns=70, phi_deg=2.0, seed=1):
    rng = np.random.default_rng(seed)
    ang = np.linspace(-70, 70, P)
    mk = np.column_stack([rng.uniform(-20, 20, J), rng.uniform(-20, 20, J), rng.uniform(-30, 30, J)])
    d = rng.uniform(-4, 4, (P, 2))
    c, U, t = np.array([0.5 * (N - 1), 0.5 * (ns - 1)]), align.marker_detector_coordinate(ang, N), np.deg2rad(phi_deg)
    Rm = np.array([[np.cos(t), -np.sin(t)], [np.sin(t), np.cos(t)]])
    tracks = [np.array([(a, *(Rm.T @ (np.array([U[a] @ mk[j, :2], mk[j, 2]]) - d[a]) + c)) for a in range(P)]) for j in range(J)]
    return ang, mk, d, tracks


def test_solve_markers_exact_noisy_and_refusals():
    N, ns = 64, 70
    ang, mk, d, tracks = synthetic()
    out = align.solve_markers(tracks, ang, N, ns)
    dg, (al, be, ga) = align.marker_gauge(d, ang)
    assert np.array_equal(dg, R.remove_gauge(d, ang))
    assert np.abs(out["shifts"] - dg).max() < 1e-9 and abs(out["rotation_deg"] - 2.0) < 1e-9 and out["residual_rms"] < 1e-9
    assert np.abs(out["markers"] - (mk + np.array([be, -al, -ga]))).max() < 1e-9
    assert np.abs(align.marker_gauge(out["shifts"], ang)[0] - out["shifts"]).max() < 1e-12        # the result carries no gauge mode
    # the shifts go straight into affine_matrices: an observation lands on the model
    Mx = align.affine_matrices(out["shifts"], out["rotation_deg"], 1.0, N, ns)
    a, r, s = tracks[2][5]
    q = np.array([0.5 * (N - 1) + align.marker_detector_coordinate(ang, N)[int(a)] @ out["markers"][2, :2], 0.5 * (ns - 1) + out["markers"][2, 2]])
    m = Mx[int(a)].reshape(2, 3)
    assert np.allclose(m[:, :2] @ q + m[:, 2], (r, s), atol=1e-9)
    off = align.solve_markers(tracks, ang, N, ns, rotation=False)
    assert off["rotation_deg"] == 0.0 and off["residual_rms"] > 0.1
    # noise of sigma 0.1: within five standard deviations of the least-squares covariance sigma^2 (J^T J)^+ of the gauge-free shifts
    sigma, rng = 0.1, np.random.default_rng(2)
    noisy = [np.column_stack([t[:, 0], t[:, 1:] + rng.normal(0, sigma, (len(t), 2))]) for t in tracks]
    got = align.solve_markers(noisy, ang, N, ns)
    P, J = len(ang), len(tracks)
    U, c = align.marker_detector_coordinate(ang, N), np.array([0.5 * (N - 1), 0.5 * (ns - 1)])
    rows = []
    for j, t in enumerate(tracks):
        for a, r, s in t:
            o = np.array([r, s]) - c
            q = np.deg2rad(2.0)
            dq = np.array([-np.sin(q) * o[0] - np.cos(q) * o[1], np.cos(q) * o[0] - np.sin(q) * o[1]])
            for k in range(2):
                row = np.zeros(3 * J + 2 * P + 1)
                if k == 0:
                    row[3 * j:3 * j + 2] = -U[int(a)]
                else:
                    row[3 * j + 2] = -1.0
                row[3 * J + 2 * int(a) + k] = 1.0
                row[-1] = dq[k]
                rows.append(row)
    Jm = np.array(rows)
    cov = sigma ** 2 * np.linalg.pinv(Jm.T @ Jm)
    t = np.deg2rad(ang)
    B = np.stack([np.cos(t), np.sin(t)], axis=1)
    Gr, Gs = np.eye(P) - B @ np.linalg.pinv(B), np.eye(P) - np.full((P, P), 1.0 / P)
    ir, is_ = 3 * J + 2 * np.arange(P), 3 * J + 2 * np.arange(P) + 1
    sd_r = np.sqrt(np.diag(Gr @ cov[np.ix_(ir, ir)] @ Gr.T))
    sd_s = np.sqrt(np.diag(Gs @ cov[np.ix_(is_, is_)] @ Gs.T))
    err = np.abs(got["shifts"] - dg)
    print(f"noise 0.1: worst shift error / sd {max(np.max(err[:, 0] / sd_r), np.max(err[:, 1] / sd_s)):.2f}, phi error / sd "
          f"{abs(np.deg2rad(got['rotation_deg'] - 2.0)) / np.sqrt(cov[-1, -1]):.2f}, residual rms {got['residual_rms']:.3f}")
    assert np.all(err[:, 0] <= 5 * sd_r) and np.all(err[:, 1] <= 5 * sd_s)
    assert abs(np.deg2rad(got["rotation_deg"] - 2.0)) <= 5 * np.sqrt(cov[-1, -1])
    assert 0.05 < got["residual_rms"] < 0.2
    with pytest.raises(ValueError, match="three markers"):
        align.solve_markers(tracks[:2], ang, N, ns)
    with pytest.raises(ValueError, match="rank"):
        align.solve_markers([t[t[:, 0] != 4] for t in tracks], ang, N, ns)                 # projection 4 seen by nobody
    with pytest.raises(ValueError, match="rank"):
        align.solve_markers([t[:1] for t in tracks[:3]] + tracks[3:], ang, N, ns)         # three markers seen once only


def test_link_markers_misses_spurious_and_crossing():
    N = 64
    ang, mk, d, tracks = synthetic()
    # two markers whose sinusoids cross: the same slice but for 3 samples, y and z mirrored
    ang2, P = np.linspace(-70, 70, 15), 15
    U, c = align.marker_detector_coordinate(ang2, N), 0.5 * (N - 1)
    pair = [np.array([(a, c + U[a] @ yz, sl) for a in range(P)]) for yz, sl in (((12.0, 6.0), 30.0), ((-12.0, 6.0), 33.0))]
    assert np.any(np.diff(np.sign(pair[0][:, 1] - pair[1][:, 1])) != 0)                     # they do cross in r
    got = align.link_markers([np.array([p[a, 1:] for p in pair]) for a in range(P)], ang2, N, 5.0, P)
    assert len(got) == 2 and all(any(np.array_equal(g, p) for p in pair) for g in got)
    # shifted projections, missed detections, a spurious detection
    rng = np.random.default_rng(0)
    pos = [np.array([t[a, 1:] for t in tracks]) for a in range(P)]
    pos[3] = np.delete(pos[3], 2, axis=0)                                                   # marker 2 missed in projection 3 ...
    pos[11] = np.delete(pos[11], 0, axis=0)                                                 # ... marker 0 in projection 11
    pos[5] = np.vstack([pos[5], [5.0, 5.0]])                                                # a detection that belongs to nobody
    pos = [p[rng.permutation(len(p))] for p in pos]
    got = align.link_markers(pos, ang, N, 6.0, 10)
    assert len(got) == 6
    for g in got:
        j = [k for k, t in enumerate(tracks) if np.array_equal(t[7], g[g[:, 0] == 7][0])][0]
        keep = np.ones(P, bool)
        keep[3], keep[11] = j != 2, j != 0
        assert np.array_equal(g, tracks[j][keep])
    assert len(align.link_markers(pos, ang, N, 6.0, 15)) == 4                               # the two with a miss fall below min_views
    far = [p.copy() for p in pos]
    for a in (9, 10, 11, 12, 13, 14):
        far[a] = np.zeros((0, 2))                                                           # nothing detected: the tracks end after the misses
    assert all(len(g) <= 9 for g in align.link_markers(far, ang, N, 6.0, 3))


def test_end_to_end_yardstick():
    """The whole pipeline in binary64 on ``ref64.Matrix(64, angles).fp`` of the bead phantom (ref64_markers.E2E), distorted in
    binary64 (ref64_affine.affine) by the seeded shifts and the 2 degree rotation: all 6 beads in all 15 projections, residual rms
    0.189 px; against the gauge-removed truth the largest shift error is 0.2308 px and the rotation error 0.1377 degrees (the bias
    of a 3-point parabola on the correlation of a bilinearly resampled 2-voxel bead).  These are the records E2E_SHIFT_ERR = 0.231
    and E2E_PHI_ERR = 0.138 the GPU test doubles.  The binary32 replay of the correlation moves the result by 2e-7 px."""
    c = R.E2E
    b = R.images(ref64.Matrix(c["N"], c["angles"]).fp(R.bead_phantom()), c["N"])
    _, M, d_true, phi_true = R.e2e_distortion()
    assert np.abs(d_true).max() <= 4 * np.sqrt(2)
    X = ref64_affine.affine(b, M)[0].astype(F32)
    T = align.marker_template(c["marker_radius"], c["R"])
    out = R.pipeline(R.ncc(X, T, 0.0)[0])
    assert np.all(out["n_detected"] == 6) and [len(t) for t in out["tracks"]] == [15] * 6
    s_err, p_err = np.abs(out["shifts"] - R.remove_gauge(d_true, c["angles"])).max(), abs(out["rotation_deg"] - phi_true)
    print(f"binary64 pipeline: shift error {s_err:.4f} px, rotation error {p_err:.4f} degrees, residual rms {out['residual_rms']:.4f} px")
    assert s_err <= R.E2E_SHIFT_ERR and p_err <= R.E2E_PHI_ERR                               # the records hold ...
    assert s_err >= 0.9 * R.E2E_SHIFT_ERR and p_err >= 0.9 * R.E2E_PHI_ERR                   # ... and are not padded
    replay = R.pipeline(R.ncc_replay32(X, T, 0.0))
    assert np.abs(replay["shifts"] - out["shifts"]).max() < 1e-5 and abs(replay["rotation_deg"] - out["rotation_deg"]) < 1e-5


def test_header_declares_and_library_exports_the_two_calls():
    from tomo_tv_amd import _lib
    text = open(os.path.join(ROOT, "include", "tomo_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    L = _lib.load()
    for name in CALLS:
        assert re.search(r"\bint\s+%s\s*\(\s*tomo_engine\s*\*" % name, src), name
        assert hasattr(L, name) and name in _lib.SIGNATURES, name
    assert L.tomo_sino_template_ncc(None, 0, 1, None, 1, 0.0) == 1 and L.tomo_sino_peaks(None, 0, 1, 0.0, 1, None, None) == 1
    assert L.tomo_last_error()                                                               # a null engine: TOMO_ERR_ARG, no crash
    import sequences_affine3d, sequences_condition, sequences_register3d, sequences_sino_normal, sequences_tilt  # noqa: F401, E401
    names = S.header_prototypes(text)
    assert set(SM.ROWS) == set(CALLS) <= set(names) and S.closure_errors(names) == []
    from tomo_tv_amd.reconstructor import TomoGPU
    assert TomoGPU.MARKER_NCC_SLOT == align.MARKER_NCC_SLOT not in (TomoGPU.ALIGN_SLOT, TomoGPU.ALIGN_SCRATCH_SLOT, TomoGPU.ALIGN_MODEL_SLOT,
                                                                   align.TILT_SCRATCH_SLOT)
