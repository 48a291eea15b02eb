"""The projection phase of the volume-resident SART sweep (k_sart_resident, tomo_tv_amd/csrc/sart_resident.hip.h) at the smallest
shapes where its scheduling can go wrong: how the cells of an angle are requested and consumed inside a pass (sets of pixels in
flight while others are in use), what happens at the first and last step of a sweep, and which waves serve the tile sums.

Every case holds the resident sweep to the streamed chain of the same engine ("sart_resident" = 0) with the bounds of
tests/test_gpu_sart_resident.py: 1e-6 on the volume (the two forms add a ray sum in different orders, ~1e-7 apart), 1e-5 on the
tracked step norm.
"""
import numpy as np
import pytest

from tomo_tv_amd._lib import VOL_ORIGINAL, VOL_RECON
from tomo_tv_amd.engine import tomoengine
from tomo_tv_amd.phantom import ellipsoids, tilt_angles

pytestmark = pytest.mark.gpu


def _engine(ns, n, nproj, resident):
    t = tomoengine(ns, n, np.deg2rad(tilt_angles(nproj)))
    t.set_option("sart_resident", resident)
    t.set_volume(ellipsoids(ns, n, seed=11), VOL_ORIGINAL)
    t.create_projections()
    b = t.get_projections()
    rng = np.random.default_rng(3)
    t.set_tilt_series((b * (1.0 + 0.05 * rng.standard_normal(b.shape)) + 0.5).astype(np.float32))
    return t


def _rel(a, b):
    return float(np.linalg.norm(a.astype(np.float64) - b) / max(np.linalg.norm(b), 1e-30))


def _sweep(ns, n, nproj, sweeps, resident, tracked=False, spin=None):
    t = _engine(ns, n, nproj, resident)
    if resident:
        assert t.get_option("sart_resident_ready") == 1 and t.get_option("form_sart") == 2
    if spin is not None:
        t.set_option("sart_resident_spin", spin)
    nrm = None
    if tracked:
        t.copy_recon()
        nrm = t.SART_tracked(0.7, sweeps)
    else:
        t.SART(0.7, sweeps)
    return t, t.get_volume(VOL_RECON), nrm


@pytest.mark.parametrize("ns,n,nproj,sweeps", [
    (64, 64, 3, 1),      # four tiles; three steps: the look-ahead of two angles runs off the end at both ends of the sweep
    (64, 64, 1, 1),      # steps == 1: one forward and one back projection, nothing to look ahead to
    (64, 72, 5, 2),      # N a multiple of 8 but not of 32: the edge tiles hold blocks outside the image, whose waves still serve tile sums
])
def test_projection_phase_equals_streamed_sweep(gpu, ns, n, nproj, sweeps):
    _, want, _ = _sweep(ns, n, nproj, sweeps, 0)
    t, got, _ = _sweep(ns, n, nproj, sweeps, 1)
    assert t.get_option("sart_resident_fallbacks") == 0
    assert np.isfinite(got).all() and got.max() > 0
    assert _rel(got, want) <= 1e-6, _rel(got, want)


def test_projection_phase_two_chunks_tracked(gpu):
    """N = 128, P = 7, 128 slices: two chunks (the cell sets are reused across the chunk boundary) and the tracked store."""
    ns, n, nproj = 128, 128, 7
    _, want, want_nrm = _sweep(ns, n, nproj, 2, 0, tracked=True)
    t, got, nrm = _sweep(ns, n, nproj, 2, 1, tracked=True)
    assert t.get_option("sart_resident_fallbacks") == 0
    assert _rel(got, want) <= 1e-6, _rel(got, want)
    assert abs(nrm - want_nrm) <= 1e-5 * abs(want_nrm), (nrm, want_nrm)
    assert t.matrix_2norm() == 0.0          # the snapshot volume is the swept volume after a tracked sweep


def test_projection_phase_gives_up_with_cells_in_flight(gpu):
    """N = 64, P = 4, every wait gives up at its first look ("sart_resident_spin" = 0): no chunk commits while cell loads are
    outstanding, and the streamed chain redoes the sweep -- the result is the streamed engine's."""
    ns, n, nproj = 64, 64, 4
    _, want, _ = _sweep(ns, n, nproj, 2, 0)
    t, got, _ = _sweep(ns, n, nproj, 2, 1, spin=0)
    assert t.get_option("sart_resident_fallbacks") == 1
    assert t.get_option("sart_resident_fallback_chunks") == 1
    assert _rel(got, want) <= 1e-6, _rel(got, want)
