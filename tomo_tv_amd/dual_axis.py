"""``DualAxisTomo`` -- reconstruction from two tilt series about perpendicular axes (an extension; the reference has one axis).

A single series leaves a missing wedge; a second one about the perpendicular axis shrinks it to a pyramid.  Every slice shares one
system matrix, so the second axis needs no new projector: it is a second ordinary engine whose slices run along the other axis, and
the volume is carried between the two layouts on the device (``tomoengine.cross_volume_to``; include/tomo_hip.h: tomo_volume_cross).

Convention.  The public volume is ``X[s][y][z]``; series A tilts about ``s`` (``TomoGPU``'s axis 0), the beam at zero tilt runs along
``y``, and series B tilts about ``z``:

* ``seriesA`` is ``(N, N, Pa)`` = [s][ray][angle], exactly what ``TomoGPU`` takes;
* ``seriesB`` is ``(N, N, Pb)`` = [z][ray][angle] with the rays of B running along ``s``.

At zero tilt the two series' projections are transposes of each other, ``P_B[z, ray=s] = P_A[s, ray=z]``.  Bringing measured data to
this convention (mirrors, quarter turns, the in-plane rotation that makes the second axis exactly perpendicular:
``TomoGPU.set_alignment(rotation_deg=...)``) is the caller's job; the 3-D shift between the two series is not registered here.
"""
import numpy as np

from ._lib import S_DD, VOL_RECON
from .reconstructor import TomoGPU, _device_tensor


class DualAxisTomo:

    def __init__(self, anglesA, seriesA, anglesB, seriesB, gpu_id=-1):
        """Angles in degrees; the series as numpy arrays or device tensors (as ``TomoGPU``).  Both series must be cubes' worth of
        data, ``(N, N, Pa)`` and ``(N, N, Pb)`` with one N: ``ValueError`` otherwise.  ``.a`` and ``.b`` are two ``TomoGPU`` objects on
        one device whose alignment and binning methods stay usable per series; the volume of record is ``.a``'s reconstruction."""
        sa, sb = tuple(seriesA.shape), tuple(seriesB.shape)
        if len(sa) != 3 or len(sb) != 3 or sa[0] != sa[1] or sb[0] != sb[1] or sa[0] != sb[0]:
            raise ValueError(f"dual-axis reconstruction needs two series (N, N, Pa) and (N, N, Pb) of one N: got {sa} and {sb}")
        if gpu_id < 0:
            t = _device_tensor(seriesA)
            gpu_id = t.device.index if t is not None else 0
        self.N = int(sa[0])
        self.a = TomoGPU(anglesA, seriesA, gpu_id=gpu_id)
        self.b = TomoGPU(anglesB, seriesB, gpu_id=gpu_id)
        self.cost = None

    # ---- the volume between the two layouts --------------------------------------------------------------------------------------
    def _a_to_b(self):
        self.a.tomo.cross_volume_to(self.b.tomo)

    def _b_to_a(self):
        self.b.tomo.cross_volume_to(self.a.tomo)

    def _enqueue_dd(self):
        """||A_A x - b_A||^2 and ||A_B cross(x) - b_B||^2 into the two engines' scalar slots; both volumes hold x.  No host wait."""
        self.a.tomo.be.c("data_distance_sq", VOL_RECON)
        self.b.tomo.be.c("data_distance_sq", VOL_RECON)

    def _read_dd(self):
        return float(np.sqrt(self.a.tomo._scalar(S_DD))), float(np.sqrt(self.b.tomo._scalar(S_DD)))

    def data_distance(self):
        """``(||A_A x - b_A||, ||A_B cross(x) - b_B||)`` of the volume of record (carried into B's layout first)."""
        self._a_to_b()
        self._enqueue_dd()
        return self._read_dd()

    def restart_recon(self):
        self.a.tomo.restart_recon()
        self.b.tomo.restart_recon()

    # ---- drivers -------------------------------------------------------------------------------------------------------------------
    def _alternate(self, Niter, step_a, step_b, show_convergence, restart):
        self.cost = np.zeros((int(Niter), 2))
        if restart:
            self.restart_recon()
        for i in range(int(Niter)):
            step_a()
            self._a_to_b()
            step_b()
            self._b_to_a()                       # the four steps are enqueued back to back: the engines' streams order themselves
            if show_convergence:
                self._enqueue_dd()
                self.cost[i] = self._read_dd()
        return self.cost

    def sirt(self, Niter=100, beta=None, show_convergence=True, restart=True):
        """Alternating Landweber from zero (``restart=False``: from the volume of record as it stands, e.g. between two calls of
        ``tv_fgp``).  Each iteration: x <- max(0, x + t_A A_A^T (b_A - A_A x)) on A, the volume carried to B,
        the same step with A_B, b_B, t_B on B, the volume carried back.  ``t = 1 / L`` (``L`` = the engine's Lipschitz bound,
        ``get_lipschitz``) or ``beta / L`` when ``beta`` is given.  Returns the (Niter, 2) array of ``(dd_a, dd_b)`` after every
        iteration, read once per iteration (zeros without ``show_convergence``; nothing is then read back at all)."""
        ta, tb = self.a.tomo, self.b.tomo
        f = 1.0 if beta is None else float(beta)
        step_a, step_b = f / ta.get_lipschitz(), f / tb.get_lipschitz()
        return self._alternate(Niter, lambda: ta.be.c("sirt_landweber", VOL_RECON, step_a, 1),
                               lambda: tb.be.c("sirt_landweber", VOL_RECON, step_b, 1), show_convergence, restart)

    def sart(self, Niter=100, beta=1.0, init="sequential", show_convergence=True, restart=True):
        """The same alternation with one SART sweep (all angles of the series, relaxation ``beta``) per axis and iteration."""
        ta, tb = self.a.tomo, self.b.tomo
        ta.initialize_SART(init)
        tb.initialize_SART(init)
        return self._alternate(Niter, lambda: ta.SART(beta, 1), lambda: tb.SART(beta, 1), show_convergence, restart)

    def combine(self, weight=0.5):
        """The classic merge of two tomograms reconstructed independently (``.a.sirt(...)``, ``.b.sirt(...)``):
        RECON_A <- (1 - weight) RECON_A + weight cross(RECON_B), as a scaling of A's volume followed by one fused multiply-add."""
        w = float(weight)
        self.a.tomo.be.c("scale_volume", VOL_RECON, 1.0 - w)
        self.b.tomo.cross_axpy_volume_to(self.a.tomo, w)

    # regularisation acts on the volume of record, so a caller can interleave it with the drivers' iterations
    def tv_fgp(self, iters, lam):
        return self.a.tomo.tv_fgp(iters, lam)

    def tv_gd(self, ng, dPOCS):
        return self.a.tomo.tv_gd(ng, dPOCS)

    def get_recon(self, as_tensor=False):
        """A's volume ``X[s][y][z]``: (N, N, N) float64, or with ``as_tensor`` a float32 torch tensor on the device."""
        return self.a.get_recon(as_tensor=as_tensor)
