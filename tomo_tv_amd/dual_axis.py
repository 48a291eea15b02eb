"""``DualAxisTomo`` -- reconstruction from two tilt series about perpendicular axes (an extension; the reference has one axis).

A single series leaves a missing wedge; a second one about the perpendicular axis shrinks it to a pyramid.  Every slice shares one
system matrix, so the second axis needs no new projector: it is a second ordinary engine whose slices run along the other axis, and
the volume is carried between the two layouts on the device (``tomoengine.cross_volume_to``; include/tomo_hip.h: tomo_volume_cross).

Convention.  The public volume is ``X[s][y][z]``; series A tilts about ``s`` (``TomoGPU``'s axis 0), the beam at zero tilt runs along
``y``, and series B tilts about ``z``:

* ``seriesA`` is ``(N, N, Pa)`` = [s][ray][angle], exactly what ``TomoGPU`` takes;
* ``seriesB`` is ``(N, N, Pb)`` = [z][ray][angle] with the rays of B running along ``s``.

At zero tilt the two series' projections are transposes of each other, ``P_B[z, ray=s] = P_A[s, ray=z]``.  Bringing measured data to
this convention (mirrors, quarter turns) is the caller's job.  Two measured series are never related by the exact transpose: the
pose of the second series relative to the first -- a small rigid motion in all three axes -- is applied by every driver once it is
set (``set_registration``, from fiducials or an external registration) or estimated from the two tomograms on the device
(``estimate_registration``: intensity-based Gauss-Newton, optionally coarse to fine).
"""
import numpy as np

from ._lib import S_DD, VOL_RECON, VOL_USER0
from .align import affine_matrix_3d, rotation_3d
from .reconstructor import TomoGPU, _device_tensor


def registration_maps(N, rotation_deg=(0, 0, 0), shift=(0, 0, 0), matrix=None):
    """The maps of a registration T = (rotation R about the centre of an N^3 volume, then ``+shift``), checked: ``None`` for the
    identity, else ``R``, ``shift`` and the two destination-to-source matrices of ``tomoengine.volume_affine_to``: ``to_a`` moves
    content by T (crossed B volume -> A's frame), ``to_b`` by T^-1 (volume of record -> what series B sees, before the cross)."""
    rot, d = np.asarray(rotation_deg, np.float64), np.asarray(shift, np.float64)
    if rot.shape != (3,) or d.shape != (3,) or not np.all(np.isfinite(rot)) or not np.all(np.isfinite(d)):
        raise ValueError("rotation_deg and shift must be three finite numbers each")
    if matrix is None:
        R = rotation_3d(rot)
    else:
        R = np.asarray(matrix, np.float64)
        if R.shape != (3, 3) or not np.all(np.isfinite(R)):
            raise ValueError("matrix must be a finite 3 x 3 rotation")
        if not np.allclose(R @ R.T, np.eye(3), rtol=0, atol=1e-9) or np.linalg.det(R) < 0:
            raise ValueError("matrix must be a proper rotation (R R^T = 1, det R = +1)")
    if np.array_equal(R, np.eye(3)) and not d.any():
        return None
    shape = (int(N),) * 3
    return dict(R=R.copy(), shift=d.copy(), to_a=affine_matrix_3d(shift=d, src_shape=shape, matrix=R),
                to_b=affine_matrix_3d(shift=-(R.T @ d), src_shape=shape, matrix=R.T))


class DualAxisTomo:

    # user slots the drivers clobber once a registration is set: resampling scratch (on A) and B's volume before its step (on B)
    VOL_SCRATCH, VOL_SAVED = VOL_USER0 + 38, VOL_USER0 + 39

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
        self._reg = None

    # ---- the pose of the second series ----------------------------------------------------------------------------------------------
    def set_registration(self, rotation_deg=(0, 0, 0), shift=(0, 0, 0), matrix=None):
        """The rigid motion T that takes series B's content, after the nominal cross, into A's frame: a rotation about the volume
        centre (``rotation_deg`` = (about s, about y, about z) in A's (s, y, z) axes, or the 3 x 3 ``matrix``; senses as in
        ``align.affine_matrix_3d``) followed by ``+shift`` voxels, so that ``x_A = T(cross(x_B))`` and series B measures
        ``cross(T^-1 x_A)``.  ``ValueError`` for wrong shapes or non-finite values.  The identity (the default) switches the
        registration off: every driver then issues exactly the calls of an object that never had one.  With a registration the
        drivers use the user slots ``VOL_SCRATCH`` (A) and ``VOL_SAVED`` (B) as scratch."""
        self._reg = registration_maps(self.N, rotation_deg, shift, matrix)

    def get_registration(self):
        """``(R, shift)`` of ``set_registration``: the 3 x 3 rotation and the shift in voxels (the identity and zeros when none is set)."""
        if self._reg is None:
            return np.eye(3), np.zeros(3)
        return self._reg["R"].copy(), self._reg["shift"].copy()

    def estimate_registration(self, pyramid=(1,), max_iter=30, margin=1, apply=True, **kw):
        """Estimate the registration from the two tomograms: B's reconstruction is crossed into A's ``VOL_SCRATCH`` and registered
        onto A's reconstruction by intensity-based Gauss-Newton (``align.register_volumes``: fixed = A's ``VOL_RECON``, moving = the
        scratch slot), so the result is directly the ``(R, shift)`` of ``set_registration``, ``x_A = T(cross(x_B))``.  BOTH
        reconstructions must already exist (``dual.a.sirt(..)``, ``dual.b.sirt(..)``, each series on its own): nothing is
        reconstructed here.  The iteration starts from the registration currently set.  ``pyramid`` lists the binning factors of
        the levels, falling to 1 -- ``(1,)``, ``(2, 1)``, ``(4, 2, 1)``: a coarser level runs on the binned engine that ``self.a`` keeps per factor
        (the one ``coarse_to_fine`` uses: built once, its reconstruction is left alone), which receives both volumes in its user
        slots ``VOL_SCRATCH`` and ``VOL_SAVED`` through ``bin_volume_to``; between levels the shift is scaled by the ratio of the
        factors and the rotation carried as it is.  ``max_iter`` and ``margin`` hold per level; ``kw`` goes to
        ``align.register_volumes`` (``tol_shift``, ``tol_deg``, ``damping``).  With ``apply`` the estimate is set
        (``set_registration(matrix=R, shift=shift)``); without, the object's registration stays as it was (A's ``VOL_SCRATCH`` is
        overwritten either way).  -> the dict of the finest level, plus ``levels``: the (factor, dict) pairs of every level."""
        from .align import register_volumes
        factors = [int(f) for f in pyramid]
        if not factors or factors[-1] != 1 or any(f not in (1, 2, 4) for f in factors) or any(a <= b for a, b in zip(factors, factors[1:])):
            raise ValueError("pyramid must list falling factors out of 4, 2, 1 and end with 1: (1,), (2, 1), (4, 1) or (4, 2, 1)")
        if any(self.N % f for f in factors):
            raise ValueError(f"N = {self.N} is not divisible by every factor of {tuple(factors)}")
        ta, tb = self.a.tomo, self.b.tomo
        Rm, d = self.get_registration()
        tb.cross_volume_to(ta, src=VOL_RECON, dst=self.VOL_SCRATCH)
        levels = []
        for f in factors:
            n = self.N // f
            M0 = affine_matrix_3d(shift=d / f, src_shape=(n, n, n), matrix=Rm)
            if f == 1:
                res = register_volumes(ta, ta, M0, max_iter=max_iter, margin=margin, fixed_vol=VOL_RECON, moving_vol=self.VOL_SCRATCH, **kw)
            else:
                coarse = self.a._coarse(f).tomo
                ta.bin_volume_to(coarse, f, src=VOL_RECON, dst=self.VOL_SCRATCH)
                ta.bin_volume_to(coarse, f, src=self.VOL_SCRATCH, dst=self.VOL_SAVED)
                res = register_volumes(coarse, coarse, M0, max_iter=max_iter, margin=margin, fixed_vol=self.VOL_SCRATCH,
                                       moving_vol=self.VOL_SAVED, **kw)
            Rm, d = res["R"], res["shift"] * f
            levels.append((f, res))
        out = dict(levels[-1][1], levels=levels)
        if apply:
            self.set_registration(matrix=out["R"], shift=out["shift"])
        return out

    # ---- the volume between the two layouts --------------------------------------------------------------------------------------
    def _a_to_b(self):
        """B's reconstruction = the volume of record as series B sees it: cross(x), or with a registration cross(T^-1 x)."""
        if self._reg is None:
            self.a.tomo.cross_volume_to(self.b.tomo)
            return
        ta = self.a.tomo
        ta.volume_affine_to(ta, self._reg["to_b"], src=VOL_RECON, dst=self.VOL_SCRATCH)
        ta.cross_volume_to(self.b.tomo, src=self.VOL_SCRATCH, dst=VOL_RECON)

    def _b_to_a(self):
        self.b.tomo.cross_volume_to(self.a.tomo)

    def _b_step_into_a(self, step_b):
        """With a registration: B steps on its copy of the volume of record, and only the INCREMENT comes back, by linearity:
        x <- max(0, x + T cross(B new - B before)).  The volume of record itself is never interpolated, so nothing blurs from one
        round trip to the next.  The difference is formed before the interpolation (the crossed new volume, then one fused
        multiply-add with -1 times the crossed saved copy, which is exact wherever the step changed a voxel by less than a factor of
        two): one resampling per iteration instead of two, and its rounding error scales with the increment, not with the volume."""
        ta, tb = self.a.tomo, self.b.tomo
        self._a_to_b()
        tb.be.c("copy_volume", self.VOL_SAVED, VOL_RECON)
        step_b()
        tb.cross_volume_to(ta, src=VOL_RECON, dst=self.VOL_SCRATCH)
        tb.cross_axpy_volume_to(ta, -1.0, src=self.VOL_SAVED, dst=self.VOL_SCRATCH)
        ta.volume_affine_axpy_to(ta, self._reg["to_a"], 1.0, clamp=True, src=self.VOL_SCRATCH, dst=VOL_RECON)

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
            if self._reg is None:
                self._a_to_b()
                step_b()
                self._b_to_a()                   # the four steps are enqueued back to back: the engines' streams order themselves
            else:
                self._b_step_into_a(step_b)
            if show_convergence:
                if self._reg is not None:
                    self._a_to_b()               # B still holds its own step: give it the volume of record before measuring
                self._enqueue_dd()
                self.cost[i] = self._read_dd()
        return self.cost

    def sirt(self, Niter=100, beta=None, show_convergence=True, restart=True):
        """Alternating Landweber from zero (``restart=False``: from the volume of record as it stands, e.g. between two calls of
        ``tv_fgp``).  Each iteration: x <- max(0, x + t_A A_A^T (b_A - A_A x)) on A, the volume carried to B,
        the same step with A_B, b_B, t_B on B, the volume carried back.  ``t = 1 / L`` (``L`` = the engine's Lipschitz bound,
        ``get_lipschitz``) or ``beta / L`` when ``beta`` is given.  Returns the (Niter, 2) array of ``(dd_a, dd_b)`` after every
        iteration, read once per iteration (zeros without ``show_convergence``; nothing is then read back at all).
        With a registration (``set_registration``) B steps on cross(T^-1 x) and only its increment is brought back,
        x <- max(0, x + T cross(B new - B before)): the volume of record is interpolated zero times per iteration.  Unlike the
        unregistered driver this leaves the two engines inconsistent when nothing is measured (``show_convergence=False``): B's
        reconstruction then holds B's own last step, not cross(T^-1 x); ``data_distance()`` carries the volume of record over
        again before it measures.  The user slots ``VOL_SCRATCH`` of A and ``VOL_SAVED`` of B (VOL_USER0 + 38, + 39) are overwritten."""
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
        RECON_A <- (1 - weight) RECON_A + weight cross(RECON_B), as a scaling of A's volume followed by one fused multiply-add.
        With a registration: + weight T(cross(RECON_B)), the crossed volume resampled into A's frame inside the multiply-add."""
        w = float(weight)
        self.a.tomo.be.c("scale_volume", VOL_RECON, 1.0 - w)
        if self._reg is None:
            self.b.tomo.cross_axpy_volume_to(self.a.tomo, w)
            return
        ta = self.a.tomo
        self.b.tomo.cross_volume_to(ta, src=VOL_RECON, dst=self.VOL_SCRATCH)
        ta.volume_affine_axpy_to(ta, self._reg["to_a"], w, src=self.VOL_SCRATCH, dst=VOL_RECON)

    # regularisation acts on the volume of record, so a caller can interleave it with the drivers' iterations
    def tv_fgp(self, iters, lam):
        return self.a.tomo.tv_fgp(iters, lam)

    def tv_gd(self, ng, dPOCS):
        return self.a.tomo.tv_gd(ng, dPOCS)

    def get_recon(self, as_tensor=False):
        """A's volume ``X[s][y][z]``: (N, N, N) float64, or with ``as_tensor`` a float32 torch tensor on the device."""
        return self.a.get_recon(as_tensor=as_tensor)
