"""``TomoGPU`` -- the public reconstruction API of tomofusion/gpu/reconstructor.py:11-215 on the HIP engine.

Same constructor and driver methods (``sirt``, ``sart``, ``fista``, ``asd_pocs``, ``kl_divergence``, ``get_recon``), plus ``pdhg_tv``;
the matplotlib/Tk viewers of the reference are not part of the hot path.  Broken reference drivers are implemented
to the semantics of their canonical loops:
``fista`` is the textbook x_k = prox_TV(SIRT(y_k)) + momentum, ``asd_pocs`` follows examples/sim_ASD.py:66-94.
"""
import ctypes

import numpy as np

from . import _lib, align, pytvlib
from ._lib import S_DD, S_DIFF2, SINO_B, SINO_G, SINO_PACKED, SINO_PUBLIC, SINO_USER0, VOL_RECON, VOL_TEMP, VOL_USER0, VOL_YK
from .engine import is_tensor, multigpuengine, tomoengine


def _device_tensor(a):
    """``a`` as a torch tensor if it is one or exports DLPack from a GPU (``torch.from_dlpack`` takes it without a copy); None for
    numpy arrays and everything else that lives on the host, which keep the host path."""
    if isinstance(a, np.ndarray):
        return None
    if not is_tensor(a):
        if not hasattr(a, "__dlpack_device__") or a.__dlpack_device__()[0] == 1:      # 1 = kDLCPU
            return None
        import torch
        a = torch.from_dlpack(a)
    return a if a.is_cuda else None


def dart_thresholds(levels):
    """The thresholds between K ascending grey levels: the midpoints of adjacent levels, formed in binary64, as float32 (K - 1,)."""
    g = np.asarray(levels, dtype=np.float64).ravel()
    return (0.5 * (g[:-1] + g[1:])).astype(np.float32)


def particles_to_keep(voxels, min_voxels):
    """The table ``keep_components`` takes, (K + 1,) bool: entry k is true where component k has at least ``min_voxels`` voxels
    (entry 0, the background's, is true)."""
    return np.concatenate([[True], np.asarray(voxels, dtype=np.int64) >= int(min_voxels)])


def particle_table(stats):
    """The records of ``component_stats`` as the dict ``TomoGPU.label_particles`` returns (centroids and diameters in binary64)."""
    v = stats["voxels"].astype(np.float64)
    return {"count": int(stats.size), "voxels": stats["voxels"].astype(np.int64),
            "centroid": np.stack([stats["sum_s"] / v, stats["sum_y"] / v, stats["sum_z"] / v], axis=1).reshape(-1, 3),
            "bbox": np.stack([np.stack([stats["min_s"], stats["min_y"], stats["min_z"]], axis=1),
                              np.stack([stats["max_s"], stats["max_y"], stats["max_z"]], axis=1)], axis=1).reshape(-1, 2, 3).astype(np.int64),
            "surface": stats["surface"].astype(np.int64), "equivalent_diameter": np.cbrt(6.0 * v / np.pi),
            "first": stats["first"].astype(np.int64)}


def device_count():
    """List of visible GPU ids (tomofusion/__init__.py:10-18)."""
    return list(range(_lib.device_count()))


def determine_gpu_config(gpu_id=-1):
    """tomofusion/__init__.py:21-34: 'multigpu' whenever no device was named (``gpu_id < 0``) and there is more than one to use --
    several visible GPUs in a plain process (the engine then spreads the slices over them by itself, one host thread per device:
    ``inprocess.py``) or a ``torch.distributed`` job of several ranks (one slab per rank).  ``TOMO_SINGLE_GPU=1`` keeps a plain
    process on one device."""
    import os
    n = len(device_count())
    if n == 0:
        raise ValueError("An AMD GPU is needed for this package!")
    if gpu_id >= 0:
        return "singleconfig"
    from .inprocess import process_group_world
    if process_group_world() > 1:
        return "multigpu"
    if n > 1 and os.environ.get("TOMO_SINGLE_GPU", "0") != "1":
        return "multigpu"
    return "singleconfig"


def _on_rank_threads(fn):
    """Run a driver loop ON the rank threads of the in-process multi-GPU facade instead of forwarding every engine call of the loop
    through it.  A forwarded call costs a queue hand-off to one host thread per device and back (bench.py `inprocess_facade`: 25 us at
    2 devices, 80 us at 8) and an ASD-POCS iteration makes ~7 of them: 0.55 ms of host time per 2.4-ms step at 8 GPUs.  Every rank
    thread runs the same Python loop on its own slab engine -- exactly what the ranks of a torchrun job do (the scalars every rank
    reads are all-reduced, so all ranks take the same decisions) -- and the facade is crossed ONCE per driver call.  The result
    vectors of rank 0's loop are copied back to this object."""
    import copy
    import functools

    @functools.wraps(fn)
    def driver(self, *args, **kw):
        from .inprocess import InProcessMultiGPU
        t = self.tomo
        if not isinstance(t, InProcessMultiGPU) or getattr(self, "_on_rank", False):
            return fn(self, *args, **kw)
        clones = []
        for eng in t._engines:
            c = copy.copy(self)
            c.tomo, c._on_rank = eng, True
            clones.append(c)
        before = dict(self.__dict__)
        out = t._world.run(lambda r: fn(clones[r], *args, **kw))
        # whatever rank 0's loop set or replaced on its clone (cost, dd_vec, tv_vec, ... -- not the engine, not the marker)
        for name, val in clones[0].__dict__.items():
            if name in ("tomo", "_on_rank"):
                continue
            if name not in before or before[name] is not val:
                setattr(self, name, val)
        return out[0]
    return driver


class TomoGPU:

    def __init__(self, tiltAngles, tiltSeries=None, gpu_id=-1, verbose=False, sub_slabs=1):
        """tiltAngles in degrees, tiltSeries (Nslice, Nray, Nangles) with axis 0 = tilt axis: a numpy array, or a torch tensor on the
        GPU (or any object ``torch.from_dlpack`` takes from one), which is handed to the engine without a host copy; with no
        ``gpu_id`` named and no process group the engine is then built on the tensor's device.  ``sub_slabs=K`` (an extension,
        single GPU): run the volume as K sub-slab engines side by side on the GPU (engine.py: ``_GroupBackend``)."""
        pytvlib.check_hip()
        tiltAngles = np.asarray(tiltAngles, dtype=np.float64)
        self.Nslice, self.Nray, self.Nangles = tiltSeries.shape
        if tiltAngles.size != self.Nangles:
            raise ValueError("tiltAngles and tiltSeries disagree on the number of projections")
        t = _device_tensor(tiltSeries)
        if t is not None and gpu_id < 0:
            from .inprocess import process_group_world
            if process_group_world() == 1:
                gpu_id = t.device.index
        config = determine_gpu_config(gpu_id)
        if config == "singleconfig":
            self.tomo = tomoengine(self.Nslice, self.Nray, np.deg2rad(tiltAngles), device=max(gpu_id, 0), sub_slabs=sub_slabs)
        else:
            self.tomo = multigpuengine(self.Nslice, self.Nray, np.deg2rad(tiltAngles))
        self.verbose = verbose
        self._tilt_deg = tiltAngles.ravel().copy()
        self.set_tilt_series(tiltSeries)
        self.recon = None
        self.cost = None

    def set_tilt_series(self, tiltSeries):
        self.Nslice, self.Nray, self.Nangles = tiltSeries.shape
        self.recon = None
        self._align_kept, self._align_shifts, self._align_rot = False, None, None      # a new series: nothing kept, nothing applied
        self._pyramid = {}                                                             # ... and no binned copy of the old one
        self._align_wrap, self._conditioning = False, None                             # ... and nothing done to its intensities
        t = _device_tensor(tiltSeries)
        if t is None:
            self.tomo.set_tilt_series(pytvlib.pack_tilt_series(tiltSeries))
        else:
            pytvlib.load_tilt_series_tensor(self.tomo, t)

    # ---- drivers (gpu/reconstructor.py:61-192) ---------------------------------------------------------
    @_on_rank_threads
    def _run_iterative(self, alg, Niter, show_convergence=True):
        self.cost = np.zeros(Niter)
        self.tomo.restart_recon()
        for i in range(Niter):
            pytvlib.run(self.tomo, alg)
            if show_convergence:
                self.cost[i] = self.tomo.data_distance()
        return self.cost

    def sart(self, Niter=150, init="sequential", show_convergence=True):
        if init not in pytvlib.sart_orders():
            init = "sequential"
        pytvlib.initialize_algorithm(self.tomo, "SART", init)
        return self._run_iterative("SART", Niter, show_convergence)

    def sirt(self, Niter=150, show_convergence=True):
        pytvlib.initialize_algorithm(self.tomo, "SIRT")
        return self._run_iterative("SIRT", Niter, show_convergence)

    def cgls(self, Niter=100, show_convergence=True):
        pytvlib.initialize_algorithm(self.tomo, "CGLS")
        return self._run_iterative("CGLS", Niter, show_convergence)

    # ---- positioning the tomogram (an extension: engine.py volume_affine_to; include/tomo_hip.h: tomo_volume_affine) ---------------
    def reorient(self, rotation_deg=(0, 0, 0), shift=(0, 0, 0), magnification=1.0):
        """Resample the reconstruction in place by a rigid motion plus scaling (``align.affine_matrix_3d``: rotation about the volume
        centre by ``rotation_deg`` = (about s, about y, about z), ``magnification``, then ``+shift`` voxels; trilinear, zeros move in
        from outside), e.g. to take out the pitch of a slab-shaped sample before segmentation or ``dart``.  One interpolation on the
        device through the scratch volume ``VOL_TEMP`` (the slot of ``copy_recon``), which is clobbered.  Returns the 12 entries of
        the destination-to-source map it used.  Afterwards the reconstruction is a POSITIONED tomogram: it no longer belongs to the
        tilt series (its projections are not the data's), so continuing an iterative run from it is the caller's risk.
        ``ValueError`` for wrong shapes or non-finite values; one whole-volume engine only (``NotImplementedError`` for sharded and
        sub-slab objects)."""
        M = align.affine_matrix_3d(rotation_deg, shift, magnification, src_shape=(self.Nslice, self.Nray, self.Nray))
        t = self._bin_engine()
        t.volume_affine_to(t, M, src=VOL_RECON, dst=VOL_TEMP)
        t.be.c("copy_volume", VOL_RECON, VOL_TEMP)
        return M

    # ---- binning and coarse-to-fine reconstruction (an extension: engine.py bin_sinogram_to / prolong_volume_to) ----------------
    def _bin_engine(self):
        t = self.tomo
        if not hasattr(t, "_align_one_engine"):
            raise NotImplementedError("binning runs on one whole-volume engine")
        t._align_one_engine()
        return t

    def binned(self, factor):
        """A new ``TomoGPU`` of shape (ceil(Nslice / f), Nray / f, Nangles), f = ``factor`` (2 or 4), with the same angles on the same
        device, whose tilt series is this object's current series (sinogram slot B, alignment included) binned on the device: the
        mean of f x k samples divided by f, so that a reconstruction of it is the f-fold binned volume in the same units.  No host
        copy of the series is made.  ``ValueError`` when ``Nray % factor != 0`` (the rays of the two grids would not line up)."""
        f = int(factor)
        if f not in (2, 4):
            raise ValueError("factor must be 2 or 4")
        if self.Nray % f != 0:
            raise ValueError(f"Nray = {self.Nray} is not divisible by the factor {f}")
        t = self._bin_engine()
        c = object.__new__(TomoGPU)
        c.Nslice, c.Nray, c.Nangles = -(-self.Nslice // f), self.Nray // f, self.Nangles
        c.tomo = t.binned_engine(f)
        c.verbose, c.recon, c.cost = getattr(self, "verbose", False), None, None
        c._align_kept, c._align_shifts, c._align_rot, c._pyramid = False, None, None, {}
        t.bin_sinogram_to(c.tomo, f)
        return c

    def _coarse(self, factor):
        """The binned object of ``factor``, kept on ``self`` from its first use (its tables cost about 1 / f^2 of this engine's) until
        ``set_tilt_series``; its series is binned again from the current one on every call (alignment may have moved it)."""
        f = int(factor)
        kept = self.__dict__.setdefault("_pyramid", {})
        if f in kept:
            self._bin_engine().bin_sinogram_to(kept[f].tomo, f)
        else:
            kept[f] = self.binned(f)
        return kept[f]

    def coarse_to_fine(self, factors=(4, 2), Niter=(30, 20, 10), alg="SIRT"):
        """Reconstruct from zero at the coarsest of ``factors``, interpolate the result into the next level's reconstruction
        (``prolong_volume_to``), run that level's iterations from there, and so on down to full resolution: ``Niter`` has one entry
        per factor and a last one for this object.  ``alg`` is "SIRT" or "SART".  Returns the per-level cost arrays (the data distance
        after every iteration, each at its own level); this object's ``cost`` is the last of them."""
        factors = [int(f) for f in factors]
        Niter = [int(n) for n in Niter]
        if alg not in ("SIRT", "SART"):
            raise ValueError("alg must be 'SIRT' or 'SART'")
        if len(Niter) != len(factors) + 1:
            raise ValueError("Niter needs len(factors) + 1 entries: one per factor and one for full resolution")
        steps = factors + [1]
        if any(f not in (2, 4) for f in factors) or any(a // b not in (2, 4) or a % b for a, b in zip(steps, steps[1:])):
            raise ValueError("factors must fall from level to level in steps of 2 or 4: (4, 2), (4,) or (2,)")
        self._bin_engine()
        costs, prev, prev_f = [], None, None
        for f, n in zip(steps, Niter):
            rec = self if f == 1 else self._coarse(f)
            pytvlib.initialize_algorithm(rec.tomo, alg)
            if prev is None:
                rec.tomo.restart_recon()
            else:
                prev.tomo.prolong_volume_to(rec.tomo, prev_f // f)
            rec.cost = np.zeros(n)
            for i in range(n):
                pytvlib.run(rec.tomo, alg)
                rec.cost[i] = rec.tomo.data_distance()
            costs.append(rec.cost)
            prev, prev_f = rec, f
        return costs

    @_on_rank_threads
    def wbp(self, filter="ram-lak"):
        if filter not in pytvlib.wbp_filters():
            filter = "ram-lak"
        pytvlib.initialize_algorithm(self.tomo, "FBP", filter)
        pytvlib.run(self.tomo, "FBP")

    @_on_rank_threads
    def kl_divergence(self, Niter=100, lambda_param=0.1):
        self.tomo.restart_recon()
        pytvlib.initialize_algorithm(self.tomo, "kl-divergence")
        self.cost = np.zeros(Niter)
        for i in range(Niter):
            self.cost[i] = pytvlib.run(self.tomo, "kl-divergence", lambda_param)
        return self.cost

    @_on_rank_threads
    def fista(self, Niter=100, momentum=True, lambda_param=0.1, nTViter=10, show_convergence=True):
        """gpu/reconstructor.py:121-155 with the TV prox actually feeding the iterate (quirk Q6)."""
        t = self.tomo
        pytvlib.initialize_algorithm(t, "fista")
        if not momentum:
            t.remove_momentum()
        self.cost = np.zeros(Niter)
        t0 = 1.0
        for k in range(Niter):
            pytvlib.run(t, "fista")                       # gradient step on yk (or recon without momentum)
            if momentum:
                t.tv_fgp(nTViter, lambda_param, vol=VOL_YK)   # the prox acts on the stepped point, in place ...
                tk = 0.5 * (1 + np.sqrt(1 + 4 * t0 ** 2))
                t.fista_momentum((t0 - 1) / tk)               # ... and its result is what momentum extrapolates
                t0 = tk
            else:
                t.tv_fgp(nTViter, lambda_param)
            if show_convergence:
                self.cost[k] = 0.5 * t.data_distance() ** 2 + lambda_param * t.tv()
                if momentum:
                    t.fista_project_yk()                      # the cost's A r gives the next step's A yk by linearity
        return self.cost

    @_on_rank_threads
    def pdhg_tv(self, Niter=100, lambda_param=0.1, theta=1.0, precond=True, ratio=1.0, show_convergence=True):
        """Chambolle-Pock (primal-dual hybrid gradient) for min_{x >= 0} 1/2 |Ax - b|^2 + lambda |grad x|_{2,1}: no inner loop, one
        forward projection, one back projection and one fused stencil pass per iteration.  ``precond=True`` (default) uses the
        diagonal step sizes of Pock and Chambolle (2011), which need no Lipschitz estimate; ``precond=False`` the scalar ones,
        tau sigma (L_A + 12) = 1, with ``ratio`` moving weight from sigma to tau.  Runs on one whole-volume engine or on a volume
        sharded over ranks or devices (one ring exchange of 5 planes per iteration); not on ``sub_slabs``.

        With ``show_convergence`` the cost is ``0.5 * data_distance()**2 + lambda_param * tv()`` exactly as ``fista`` reports it.
        ``tv()`` is the periodic, eps-smoothed value while the iteration minimises the Neumann one (no wrap-around, no eps);
        FISTA with the FGP prox has the same mismatch."""
        t = self.tomo
        if not hasattr(t, "_pdhg_one_engine"):
            raise NotImplementedError("pdhg_tv runs on one whole-volume engine")
        t._pdhg_one_engine()
        pytvlib.initialize_algorithm(t, "pdhg")
        t.restart_recon()
        t.pdhg_begin()
        self.cost = np.zeros(Niter)
        if not show_convergence:
            pytvlib.run(t, "pdhg", lambda_param, Niter, theta=theta, precond=precond, ratio=ratio)
            return self.cost
        for k in range(Niter):
            pytvlib.run(t, "pdhg", lambda_param, 1, theta=theta, precond=precond, ratio=ratio)
            self.cost[k] = 0.5 * t.data_distance() ** 2 + lambda_param * t.tv()
        return self.cost

    @_on_rank_threads
    def asd_pocs(self, Niter=100, eps=0.025, beta0=0.25, beta_reduce=0.9985, r_max=0.95, nTViter=10, alpha=0.2,
                 alpha_reduce=0.95, show_convergence=True, normalize_dd=True, init="sequential"):
        """examples/sim_ASD.py:66-94 == demo.ipynb cell 25 (the reference method itself is broken, quirk Q7).

        ``normalize_dd``: divide the data distance by Nslice*Nrow as the CPU path does (ctvlib.cpp:275), which is
        what the default ``eps`` presumes (quirk Q5)."""
        t = self.tomo
        pytvlib.initialize_algorithm(t, "asd-pocs", init)
        t.initialize_recon_copy()
        t.restart_recon()
        beta = beta0
        self.dd_vec, self.tv_vec = np.zeros(Niter), np.zeros(Niter)
        dPOCS = 0.0
        norm = float(t.Nslice_ * t.Nrow) if normalize_dd else 1.0
        t.copy_recon()
        pending = None              # (iteration, its SART step norm or None, the deferred read of its scalars)

        def collect(dPOCS):
            """The scalars of the iteration whose read-back is in flight, and the step-length rule they feed (sim_ASD.py:90-94)."""
            j, dp, get = pending
            if dp is None:
                self.tv_vec[j], dg, dd2, dp2 = get()
                dp = float(np.sqrt(dp2))
            else:
                self.tv_vec[j], dg, dd2 = get()
            self.dd_vec[j] = float(np.sqrt(dd2)) / norm
            if dg > dp * r_max and self.dd_vec[j] > eps:
                dPOCS *= alpha_reduce
            return dPOCS
        for i in range(Niter):
            # sim_ASD.py:68-78: copy_recon; SART; dp = matrix_2norm; copy_recon -- the step norm and the new snapshot
            # (TEMP) come out of the sweep's last back-projection pass; TEMP == recon holds on entry.  Only the first
            # iteration needs dp at once (it sets the TV step length); later ones leave it on the device until the
            # iteration's scalars are read together: one all-reduce and one read-back per iteration -- and that read-back
            # is collected only AFTER the next sweep has been enqueued (the scalars of iteration i steer nothing before the
            # TV steps of iteration i+1), so the device never waits for the host between two iterations.
            if i == 0:
                dp0 = t.SART_tracked(beta)
                dPOCS = dp0 * alpha
            else:
                dp0 = None
                t.SART_tracked(beta, defer=True)
                dPOCS = collect(dPOCS)
            beta *= beta_reduce
            # the residual of the SART result is independent of the TV descent: evaluate it on the snapshot (TEMP)
            # on the engine's second stream while the TV steps run
            t.data_distance_begin()
            # sim_ASD.py:84-88: tv_gd; dg = matrix_2norm (and the copy_recon that opens the next iteration)
            pending = (i, dp0, t.tv_gd_tracked(nTViter, dPOCS, extra=(S_DD,) if i == 0 else (S_DD, S_DIFF2), defer=True))
        if pending is not None:
            collect(dPOCS)
        return self.dd_vec, self.tv_vec

    # ---- alignment of the tilt series (an extension: the reference centres by mass on the host, cpu/utils/logger.py:237-252) ----
    ALIGN_SLOT = SINO_USER0          # sinogram slot that keeps the series as it was given
    ALIGN_MODEL_SLOT = SINO_USER0 + 39   # the last user slot: the leave-one-out model projections (refine_alignment)
    ALIGN_SCRATCH_SLOT = SINO_USER0 + 38  # the candidates of estimate_tilt_axis_rotation

    def _align_engine(self):
        t = self.tomo
        if not hasattr(t, "_align_one_engine"):
            raise NotImplementedError("alignment runs on one whole-volume engine")
        t._align_one_engine()
        if not self._align_kept:
            # the series as given, kept on the device: every later shift resamples THIS copy, so interpolation never compounds
            # (a whole-pixel shift of zero copies bit for bit).  Only set_tilt_series of THIS object drops the copy: a caller that
            # replaces the series through self.tomo directly must call set_tilt_series instead, or the old series is resampled
            t.sino_shift(SINO_B, self.ALIGN_SLOT, np.zeros((self.Nangles, 2), np.float32))
            self._align_kept = True
        return t

    def get_alignment(self):
        """Total shifts (Nangles, 2) of (dr, ds) -- along the rays, along the tilt axis -- applied to the series as it was given."""
        return np.zeros((self.Nangles, 2)) if self._align_shifts is None else np.array(self._align_shifts, np.float64)

    def _align_resample(self, t, shifts, wrap=False, dst=SINO_B, rotation_deg=None):
        """The one place that resamples the series as given (``ALIGN_SLOT``) into ``dst``: by ``sino_shift`` while no rotation or
        magnification is stored, else by ONE affine pass that combines the stored rotation and magnification (or the candidate
        ``rotation_deg``) with the shifts -- rotation and shifts never compound their interpolation.  The shifts are rounded to
        binary32 on both paths, so a stored rotation of 0 with magnification 1 gives the bits of the shift path."""
        stored = getattr(self, "_align_rot", None)
        if stored is None and rotation_deg is None:
            t.sino_shift(self.ALIGN_SLOT, dst, shifts, wrap=wrap)
            if dst == SINO_B:
                self._align_wrap = bool(wrap)          # what the conditioning drivers re-apply (_conditioned)
            return
        if wrap:
            raise ValueError("wrap=True cannot be combined with a rotation or magnification: the affine pass has no wrap form")
        rot, mag = stored if stored is not None else (0.0, 1.0)
        sh = np.asarray(shifts, np.float32).astype(np.float64)
        t.sino_affine(self.ALIGN_SLOT, dst, align.affine_matrices(sh, rot if rotation_deg is None else rotation_deg, mag, self.Nray, self.Nslice))
        if dst == SINO_B:
            self._align_wrap = False

    def set_alignment(self, shifts, wrap=False, *, rotation_deg=None, magnification=None):
        """Apply total shifts to the series as it was given (not on top of earlier ones): projection a moves by (dr, ds) =
        ``shifts[a]`` in the sense of ``np.roll``, bilinear for fractions, zeros (or with ``wrap`` the other edge) moving in.

        ``rotation_deg`` / ``magnification`` (a scalar or one value per projection): the content is first rotated by
        ``+rotation_deg`` about the image centre ((Nray-1)/2, (Nslice-1)/2), counter-clockwise from the r axis towards the s axis,
        and scaled by ``magnification`` (``align.affine_matrices``); the series as given is resampled ONCE by the combined map.  Both
        are remembered (``get_alignment_rotation``) and kept by later calls that name neither, ``refine_alignment`` included, until
        ``set_tilt_series``; a keyword left ``None`` keeps its stored value (0 and 1 if there is none).  ``wrap`` must be False once a
        rotation or magnification is stored or given."""
        t = self._align_engine()
        shifts = np.array(shifts, np.float64).reshape(self.Nangles, 2)
        stored = getattr(self, "_align_rot", None)
        if rotation_deg is not None or magnification is not None or stored is not None:
            if wrap:
                raise ValueError("wrap=True cannot be combined with a rotation or magnification: the affine pass has no wrap form")
            rot, mag = stored if stored is not None else (np.zeros(self.Nangles), np.ones(self.Nangles))
            if rotation_deg is not None:
                rot = np.array(np.broadcast_to(np.asarray(rotation_deg, np.float64), (self.Nangles,)))
            if magnification is not None:
                mag = np.array(np.broadcast_to(np.asarray(magnification, np.float64), (self.Nangles,)))
            if not (np.all(np.isfinite(rot)) and np.all(np.isfinite(mag)) and np.all(mag > 0)):
                raise ValueError("rotation_deg must be finite and magnification positive and finite")
            self._align_rot = (rot, mag)
        self._align_resample(t, shifts, wrap=wrap)
        self._align_shifts = shifts
        return self.get_alignment()

    def get_alignment_rotation(self):
        """``(rotation_deg, magnification)``, each (Nangles,) float64, applied to the series as it was given (zeros and ones if
        none was set)."""
        stored = getattr(self, "_align_rot", None)
        if stored is None:
            return np.zeros(self.Nangles), np.ones(self.Nangles)
        return np.array(stored[0], np.float64), np.array(stored[1], np.float64)

    def estimate_tilt_axis_rotation(self, search_deg=10.0, step_deg=0.5, apply=True):
        """In-plane rotation that brings the tilt axis onto the slice index, by the common-line property: for a parallel-beam series
        whose axis runs along s, the mass of slice s, c_a[s] = sum_r X_a[r][s], is the same in every projection a.  For every
        candidate phi = k ``step_deg`` in [-``search_deg``, ``search_deg``] the series as given is resampled by the current shifts (and
        stored magnification) and phi into sinogram slot ``ALIGN_SCRATCH_SLOT`` (``sino_affine``), its profile taken
        (``sino_axis_profile``) and scored by sum_s Var_a(c_a[s]) / sum_s mean_a(c_a[s])^2 over the slices H <= s < Nslice - H,
        H = ceil(Nray/2 sin(search_deg)), which zero fill never reaches (``ValueError`` if none is left).  The grid minimum is refined
        by a 3-point parabola clamped to +-1/2 step; a minimum on the grid's border is not refined and sets
        ``self.align_axis_at_border`` (widen the search).  Returns the rotation ``set_alignment(rotation_deg=...)`` should receive, one
        value for the whole series, and with ``apply`` passes it on with the current shifts.  ``self.align_axis_scores`` keeps
        ``(grid, scores)``.  No reconstruction is needed.

        Assumes a background near zero at the image borders (content that a rotation moves across the border changes the masses)
        and a series already centred: run it after ``align_center_of_mass``, before ``refine_alignment``."""
        t = self._align_engine()
        H = align.axis_score_border(self.Nray, search_deg)
        if self.Nslice - 2 * H <= 0:
            raise ValueError(f"no slice is left between the borders of {H} slices: lower search_deg")
        grid = align.axis_grid(search_deg, step_deg)
        shifts = self.get_alignment()
        scores = np.zeros(len(grid))
        for k, phi in enumerate(grid):
            self._align_resample(t, shifts, dst=self.ALIGN_SCRATCH_SLOT, rotation_deg=float(phi))
            scores[k] = align.axis_score(t.sino_axis_profile(self.ALIGN_SCRATCH_SLOT), H)
        rot, _, self.align_axis_at_border = align.axis_minimum(grid, scores)
        self.align_axis_scores = (grid, scores)
        if apply:
            self.set_alignment(shifts, rotation_deg=rot)
        return rot

    def align_center_of_mass(self):
        """The reference's rule per projection (cpu/utils/logger.py:237-252): roll, with wrap-around, so that the integer-truncated
        centre of mass lands on ``size // 2`` of both axes.  Replaces the engine's tilt series; returns the (Nangles, 2) integer
        shifts (dr, ds)."""
        t = self._align_engine()
        shifts = align.center_of_mass_shifts(t.sino_moments(self.ALIGN_SLOT), self.Nray, self.Nslice)
        self.set_alignment(shifts, wrap=True)
        return shifts

    # ---- conditioning of the series as given (an extension of cpu/utils/logger.py:93, which subtracts a background on the host before
    # it centres; include/tomo_hip.h: tomo_sino_window_stats / tomo_sino_median / tomo_sino_intensity; the rules are in align.py) ----
    @property
    def conditioning(self):
        """What the conditioning drivers have done to the series since ``set_tilt_series``, per projection: ``gain`` and ``offset``
        (the series as given went through ``gain * x + offset`` in total, outlier replacement aside) and ``replaced``, the number
        of samples ``despeckle`` replaced."""
        c = getattr(self, "_conditioning", None)
        if c is None:
            c = self._conditioning = dict(gain=np.ones(self.Nangles), offset=np.zeros(self.Nangles), replaced=np.zeros(self.Nangles, np.int64))
        return {k: v.copy() for k, v in c.items()}

    def _conditioned(self, t):
        """The series as given (``ALIGN_SLOT``) has changed: resample it again by the alignment in force (the shifts, the stored
        rotation and magnification, the ``wrap`` last used), and drop what was derived from the old series."""
        self._align_resample(t, self.get_alignment(), wrap=getattr(self, "_align_wrap", False))
        self._pyramid = {}
        self.recon = None

    def _apply_intensity(self, t, gain, offset, clamp=False):
        t.sino_intensity(self.ALIGN_SLOT, self.ALIGN_SLOT, gain, offset, clamp=clamp)
        self.conditioning                                # (creates the record)
        c = self._conditioning
        c["offset"] = np.asarray(gain, np.float64) * c["offset"] + np.asarray(offset, np.float64)
        c["gain"] = np.asarray(gain, np.float64) * c["gain"]
        self._conditioned(t)

    def subtract_background(self, window=None, clamp=False):
        """Subtract from every projection of the series as given the mean of its samples in ``window`` = ``(r0, r1, s0, s1)``, rays
        r0 <= r < r1 and slices s0 <= s < s1; ``None`` is the reference's first-quarter corner (cpu/utils/logger.py:255-263,
        ``align.background_window``).  With ``clamp`` negative results become 0.  An outlier inside the window enters its mean.  The current alignment is re-applied.  Returns the
        (Nangles,) backgrounds removed (the offset applied is their binary32 rounding, negated)."""
        t = self._align_engine()
        r0, r1, s0, s1 = align.background_window(self.Nray, self.Nslice) if window is None else (int(v) for v in window)
        st = t.sino_window_stats(self.ALIGN_SLOT, (r0, r1, s0, s1))
        mean = st[:, 0] / float((r1 - r0) * (s1 - s0))
        offset = -mean.astype(np.float32)
        self._apply_intensity(t, np.ones(self.Nangles, np.float32), offset, clamp=clamp)
        return -offset.astype(np.float64)

    def despeckle(self, n_sigma=6.0, radius=1, passes=1):
        """Replace outliers ("hot pixels", X-ray hits) of the series as given by the median of their (2 ``radius`` + 1)^2
        neighbourhood: per pass one measuring ``sino_median``, the thresholds ``align.despeckle_thresholds(stats, n_sigma)`` (per
        projection ``n_sigma`` Gaussian sigmas, estimated from the mean absolute deviation from the local median), one replacing call
        into ``ALIGN_SCRATCH_SLOT`` and a move back.  The current alignment is re-applied.  Returns the (Nangles,) int64 numbers of
        samples replaced, summed over the passes."""
        if int(passes) < 1:
            raise ValueError("passes must be at least 1")
        t = self._align_engine()
        total = np.zeros(self.Nangles, np.int64)
        for _ in range(int(passes)):
            th = align.despeckle_thresholds(t.sino_median(self.ALIGN_SLOT, radius=radius), n_sigma)
            st = t.sino_median(self.ALIGN_SLOT, self.ALIGN_SCRATCH_SLOT, radius=radius, thresh=th)
            t.sino_intensity(self.ALIGN_SCRATCH_SLOT, self.ALIGN_SLOT, 1.0, 0.0)
            total += st[:, 4].astype(np.int64)
        self.conditioning
        self._conditioning["replaced"] = self._conditioning["replaced"] + total
        self._conditioned(t)
        return total

    def normalize_intensity(self, mode="mass"):
        """Scale every projection of the series as given so that all have the same total mass, the mean of the masses before
        (``align.mass_gains``: a parallel-beam projection of one object has the same mass at every tilt).  ``"mass"`` is the only
        mode.  The current alignment is re-applied.  Returns the (Nangles,) gains applied (binary32 values)."""
        if mode != "mass":
            raise ValueError(f"unknown mode {mode!r}: 'mass' is the only one")
        t = self._align_engine()
        gain = align.mass_gains(t.sino_moments(self.ALIGN_SLOT)).astype(np.float32)
        self._apply_intensity(t, gain, np.zeros(self.Nangles, np.float32))
        return gain.astype(np.float64)

    def condition(self, background=True, despeckle=True, normalize=True, **kw):
        """``subtract_background``, ``despeckle`` and ``normalize_intensity`` in that order (the reference's step first, then the two
        it lacks), each unless switched off; the keywords ``window`` and ``clamp`` go to the first, ``n_sigma``, ``radius`` and
        ``passes`` to the second, ``mode`` to the third.  Returns ``{"background": ..., "replaced": ..., "gain": ...}`` with what each
        step that ran returned."""
        known = {"window", "clamp", "n_sigma", "radius", "passes", "mode"}
        if set(kw) - known:
            raise TypeError(f"unknown keyword(s) {sorted(set(kw) - known)}")
        pick = lambda *names: {k: kw[k] for k in names if k in kw}  # noqa: E731
        out = {}
        if background:
            out["background"] = self.subtract_background(**pick("window", "clamp"))
        if despeckle:
            out["replaced"] = self.despeckle(**pick("n_sigma", "radius", "passes"))
        if normalize:
            out["gain"] = self.normalize_intensity(**pick("mode"))
        return out

    # ---- marker (fiducial / feature) alignment: detection on the device (include/tomo_hip.h: tomo_sino_template_ncc /
    # tomo_sino_peaks), tracking and the least-squares model in align.py.  An extension: the reference has none. -----------------
    MARKER_NCC_SLOT = align.MARKER_NCC_SLOT   # SINO_USER0 + 36: the correlation of the series as given with the marker template

    def align_markers(self, marker_radius=2.0, R=None, bright=True, threshold=0.5, peak_radius=None, search_radius=6.0, min_views=None,
                      rotation=True, apply=True):
        """First alignment from tracked markers, without a reconstruction: the series as given is correlated with an anti-aliased disc
        of radius ``marker_radius`` samples (``align.marker_template``; window radius ``R``, default ceil(marker_radius) + 2, at most
        8; ``bright=False`` for dark markers) into sinogram slot ``MARKER_NCC_SLOT``; its local maxima >= ``threshold`` within
        ``peak_radius`` (default ``R``) are the detections, refined to sub-pixel positions (``align.marker_positions``), followed
        through the series (``align.link_markers`` with ``search_radius``; tracks with fewer than ``min_views`` views, default half
        the projections, are dropped) and fitted by ``align.solve_markers``: marker positions, one shift per projection and, with
        ``rotation``, the in-plane rotation of the tilt axis.  With ``apply`` the result goes to
        ``set_alignment(shifts, rotation_deg=phi)``, which resamples the series as given once.  -> dict: ``shifts`` (Nangles, 2),
        ``rotation_deg``, ``markers`` (J, 3) of (y, z, sigma), ``tracks``, ``residual_rms`` (pixels: how good the alignment is),
        ``n_detected`` (Nangles,); also kept as ``self.marker_alignment``."""
        t = self._align_engine()
        R = int(np.ceil(float(marker_radius))) + 2 if R is None else int(R)
        peak_radius = R if peak_radius is None else int(peak_radius)
        min_views = max(3, (self.Nangles + 1) // 2) if min_views is None else int(min_views)
        t.sino_template_ncc(self.ALIGN_SLOT, self.MARKER_NCC_SLOT, align.marker_template(marker_radius, R, bright))
        count, records = t.sino_peaks(self.MARKER_NCC_SLOT, peak_radius, threshold)
        positions = [align.marker_positions(rec, (self.Nray, self.Nslice)) for rec in records]
        tracks = align.link_markers(positions, self._tilt_deg, self.Nray, search_radius, min_views)
        out = align.solve_markers(tracks, self._tilt_deg, self.Nray, self.Nslice, rotation=rotation)
        out = dict(shifts=out["shifts"], rotation_deg=out["rotation_deg"], markers=out["markers"], tracks=tracks,
                   residual_rms=out["residual_rms"], n_detected=count.astype(np.int64))
        self.marker_alignment = out
        if apply:
            self.set_alignment(out["shifts"], rotation_deg=out["rotation_deg"])
            self._pyramid = {}                     # binned copies and a reconstruction of the series as it was aligned before
            self.recon = None
        return out

    def _model_leave_one_out(self, niter):
        """Into sinogram slot ``ALIGN_MODEL_SLOT``: for every projection a, projection a of a SIRT reconstruction (``niter`` iterations
        from zero) that never saw projection a.  One engine does it: before every SIRT step the data of projection a are replaced by
        the model's own projection a, so that its residual is zero and only the other projections shape the volume.  The series goes
        through torch tensors on the engine's device (plumbing: two sinogram copies per step); B is put back as it was."""
        t = self.tomo
        pytvlib.initialize_algorithm(t, "SIRT")
        b = t.get_projections_tensor(SINO_B, SINO_PUBLIC)
        work, model = b.clone(), b.clone()
        for a in range(self.Nangles):
            work.copy_(b)
            t.set_tilt_series_tensor(work, SINO_PUBLIC)
            t.restart_recon()
            for _ in range(int(niter)):
                t.forward_projection()
                work[:, :, a] = t.get_projections_tensor(SINO_G, SINO_PUBLIC)[:, :, a]
                t.set_tilt_series_tensor(work, SINO_PUBLIC)
                t.SIRT(1)
            t.forward_projection()
            model[:, :, a] = t.get_projections_tensor(SINO_G, SINO_PUBLIC)[:, :, a]
        t.set_tilt_series_tensor(b, SINO_PUBLIC)
        t.be.set_tilt_series_tensor(model, SINO_PUBLIC, self.ALIGN_MODEL_SLOT)
        return self.ALIGN_MODEL_SLOT

    def _align_pass(self, t, f, shifts, max_shift, recon, subpixel, leave_one_out, loo_iters):
        """One pass of projection matching at binning factor ``f`` (1: on this object itself): model, correlation, peaks times f, new
        totals, the series as given resampled by them, bookkeeping.  -> the new total shifts."""
        rec = self if f == 1 else self._coarse(f)
        ct = t if f == 1 else rec.tomo
        if leave_one_out:
            model = rec._model_leave_one_out(loo_iters)
        else:
            recon(rec)
            ct.forward_projection()
            model = SINO_G
        C = ct.sino_xcorr(model, SINO_B, int(max_shift))
        peaks, border = align.find_peaks(C, subpixel)
        int_peaks = peaks if not subpixel else align.find_peaks(C, False)[0]
        if f != 1:
            peaks, int_peaks = peaks * f, int_peaks * f
        self.align_int_peaks.append(int_peaks)
        shifts = shifts - peaks
        m = shifts[:, 1].mean()
        shifts[:, 1] -= m if subpixel else np.round(m)
        self._align_resample(t, shifts)
        self._align_shifts = shifts.copy()
        self.align_peaks.append(peaks)
        self.align_history.append(shifts.copy())
        self.align_at_border.append(border)
        return shifts

    def refine_alignment(self, Nouter=5, max_shift=8, recon=None, subpixel=True, leave_one_out=False, loo_iters=20, pyramid=None):
        """Projection matching.  Every outer pass reconstructs (``recon(self)``; default 20 SIRT iterations), projects the result,
        correlates each model projection with the measured one over shifts in [-max_shift, max_shift]^2 (``sino_xcorr``), moves the
        total shift of every projection against the peak it found and resamples the series AS GIVEN by the new totals (zeros move
        in).  The mean of ds -- a translation of the volume along the tilt axis, which no projection can see -- is removed; without
        ``subpixel`` peaks and the removed mean are whole pixels, so the series is only ever copied, never interpolated.  The
        translation of the volume across the tilt axis (dr_a = x cos(theta_a) + y sin(theta_a)) is left where the data put it.
        A peak on the window's border keeps its integer position and is flagged in ``self.align_at_border`` (per pass, per angle):
        raise ``max_shift`` or pre-align by ``align_center_of_mass``.  Returns the total (Nangles, 2) shifts; ``self.align_history``
        holds them after every pass, ``self.align_peaks`` the peaks and ``self.align_int_peaks`` the whole-pixel maxima they refine.
        The series as given is kept in sinogram slot ``ALIGN_SLOT`` from the first alignment call on and dropped only by
        ``set_tilt_series`` of this object: replace the series through it, not through ``self.tomo``.

        ``leave_one_out``: the model of projection a comes from a SIRT reconstruction (``loo_iters`` iterations, ``recon`` is not used)
        that never saw projection a.  With few projections the plain form stalls -- the reconstruction reproduces every measured
        projection where it lies, so its model correlates best at zero shift (at 9 projections of 32 x 32 slices no peak leaves
        (0, 0)) -- and this form does not; it costs ``Nangles`` reconstructions per pass and needs torch.

        ``pyramid``: binning factors, coarsest first, e.g. ``(4, 2, 1)``; ``Nouter`` passes run per level.  A pass at factor f bins the
        current series into the kept coarse object (``binned``), reconstructs and projects THERE (``recon`` is called with the coarse
        object; ``leave_one_out`` works per level), correlates there with the same ``max_shift`` -- which reaches f * max_shift
        full-resolution pixels -- and multiplies the peaks by f.  Totals, history, peaks and the resampling of the series as given stay
        in full-resolution pixels; the lists get one entry per pass over all levels.  Factor 1 is the plain pass; ``None`` (default)
        is ``(1,)``."""
        t = self._align_engine()
        if leave_one_out and recon is not None:
            raise ValueError("leave_one_out reconstructs by itself (loo_iters SIRT iterations): recon is not used")
        if recon is None:
            recon = lambda rec: rec.sirt(20, show_convergence=False)  # noqa: E731
        levels = (1,) if pyramid is None else tuple(int(f) for f in pyramid)
        if not levels or any(f not in (1, 2, 4) for f in levels):
            raise ValueError("pyramid holds binning factors 4, 2 or 1, coarsest first")
        shifts = self.get_alignment()
        self.align_history, self.align_at_border, self.align_peaks, self.align_int_peaks = [], [], [], []
        for f in levels:
            for _ in range(int(Nouter)):
                shifts = self._align_pass(t, f, shifts, max_shift, recon, subpixel, leave_one_out, loo_iters)
        return self.get_alignment()

    def refine_alignment_affine(self, Nouter=3, recon=None, rotation=True, magnification=True, leave_one_out=False, loo_iters=20,
                                max_iter=20, margin=2, damping=0.0):
        """Projection matching by intensity: per projection a shift, an in-plane rotation and a magnification, estimated by
        Gauss-Newton on the device (``align.match_projections``, ``tomoengine.sino_affine_normal``).  Every outer pass reconstructs
        (``recon(self)``; default 20 SIRT iterations; or with ``leave_one_out`` the model of ``refine_alignment``, ``loo_iters`` SIRT
        iterations that never saw the projection), projects the result and matches the series AS GIVEN (``ALIGN_SLOT``) to that model,
        starting from the stored shifts, rotation and magnification (``align.affine_matrices``).  Three gauges are removed from the
        result: the mean of ds (a translation of the volume along the tilt axis, as in ``refine_alignment``); the mean of the
        rotation increment of the pass (a common in-plane rotation is the tilt-axis direction: ``estimate_tilt_axis_rotation`` finds
        it); the mean of the log-magnification increment (a common magnification only rescales the volume).  The new totals are
        stored and the series as given is resampled ONCE by them; ``get_alignment()`` / ``get_alignment_rotation()`` report them.
        ``rotation=False`` / ``magnification=False`` remove that parameter from the fit: its stored values stay bit-identical.
        Returns ``(shifts, rotation_deg, magnification)``; ``self.align_affine_history`` holds that triple after every pass and
        ``self.align_affine_cost`` per pass a dict of the per-evaluation ``ssd`` and ``ncc`` and of ``converged``.

        Capture range: the matching follows the image gradient, so it finds a distortion of about a pixel, a few at most, at the
        image border (a rotation of 1 degree moves the border of a 512-pixel image by 4.5 pixels); there is no pyramid.  Run it
        after ``align_center_of_mass`` / ``refine_alignment`` have brought the shifts within that range.  With few projections the
        plain form stalls as ``refine_alignment``'s does: use ``leave_one_out``."""
        t = self._align_engine()
        if leave_one_out and recon is not None:
            raise ValueError("leave_one_out reconstructs by itself (loo_iters SIRT iterations): recon is not used")
        if recon is None:
            recon = lambda rec: rec.sirt(20, show_convergence=False)  # noqa: E731
        shifts = self.get_alignment()
        self.align_affine_history, self.align_affine_cost = [], []
        for _ in range(int(Nouter)):
            if leave_one_out:
                model = self._model_leave_one_out(loo_iters)
            else:
                recon(self)
                t.forward_projection()
                model = SINO_G
            rot, mag = self.get_alignment_rotation()
            M0 = align.affine_matrices(shifts, rot, mag, self.Nray, self.Nslice)
            res = align.match_projections(t, model, self.ALIGN_SLOT, M0, max_iter=max_iter, margin=margin, damping=damping,
                                          rotation=rotation, magnification=magnification)
            shifts = res["shift"].copy()
            shifts[:, 1] -= shifts[:, 1].mean()
            if rotation:
                drot = res["rotation_deg"] - rot
                rot = rot + (drot - drot.mean())
            if magnification:
                dlog = np.log(res["magnification"]) - np.log(mag)
                mag = mag * np.exp(dlog - dlog.mean())
            if rotation or magnification:
                self._align_rot = (rot, mag)
            self._align_resample(t, shifts)
            self._align_shifts = shifts.copy()
            self.align_affine_history.append((shifts.copy(), rot.copy(), mag.copy()))
            self.align_affine_cost.append(dict(ssd=res["ssd"], ncc=res["ncc"], converged=res["converged"]))
        return self.get_alignment(), *self.get_alignment_rotation()

    # ---- refinement of the tilt angles (an extension: the reference takes them as given; engine.py volume_rot_derivative /
    # sino_tilt_normal, align.match_tilt_angles) -----------------------------------------------------------------------------
    def get_tilt_angles(self):
        """The tilt angles in degrees the engine projects with: those of the constructor until ``refine_tilt_angles`` (or
        ``tomo.update_projection_angles``) replaces them."""
        rad = getattr(self.tomo, "_ctor_kw", {}).get("angles_rad")
        if rad is not None:
            return np.rad2deg(np.asarray(rad, np.float64).ravel())
        return np.array(self._tilt_deg, np.float64)

    def _set_tilt_angles(self, deg):
        """New angles for this object's engine (``update_projection_angles``: the tables are rebuilt, the volumes move over).  The
        sinogram slots do NOT survive a rebuild, so the two the alignment state lives in -- the series in ``SINO_B`` and, once an
        alignment call has kept it, the series as given in ``ALIGN_SLOT`` -- are carried across, as device tensors where torch sees
        the device (a copy of bits either way).  Every kept binned object has the old angles and is dropped."""
        t = self.tomo
        keep = [SINO_B] + ([self.ALIGN_SLOT] if getattr(self, "_align_kept", False) else [])
        try:
            import torch
            on_device = torch.cuda.is_available() and torch.cuda.device_count() > t.gpuID
        except ImportError:
            on_device = False
        saved = [(s, t.get_projections_tensor(s) if on_device else t._sino_local(s)) for s in keep]
        t.update_projection_angles(np.deg2rad(np.asarray(deg, np.float64)))
        for s, x in saved:
            if on_device:
                t.be.set_tilt_series_tensor(x, SINO_PACKED, s)
            else:
                t.be.c("set_sinogram", int(s), x.ctypes.data_as(ctypes.c_void_p))
        self._pyramid = {}

    def refine_tilt_angles(self, Nouter=3, recon=None, damping=1.0, max_step_deg=5.0, margin=1, factor=1, apply=True):
        """Refine the tilt angle of every projection by Gauss-Newton matching on the device.  Every pass reconstructs at the current
        angles (``recon(self)``; default 100 SIRT iterations from zero -- NOT the 20 of the shift and affine refinements: the step
        reads the residual b - A x, and a residual that is mostly the iteration's own remaining error points nowhere.  In binary64
        at 32 x 32, 31 projections, +-4 degrees, 20 iterations per pass left the rms angle error at 2.1 of 2.2 degrees and then
        raised it, 50 and 100 lowered it to 0.79 and 0.76 after one pass), forms the rotational derivative volume D x = X d_Y x - Y d_X x
        (``volume_rot_derivative``), projects x and D x -- A (D x) is the derivative of every projection by its own angle -- and
        reduces per projection <b - A x, A D x> and <A D x, A D x> (``align.match_tilt_angles``, ``sino_tilt_normal``).  The step of
        angle p is their quotient times ``damping``, clipped to ``max_step_deg``; the mean of the steps of a pass is removed (a
        common offset is a rotation of the volume about the tilt axis, which the data cannot see: ``align.tilt_increment``).  The new
        angles are applied through ``update_projection_angles`` before the next pass.  Returns the total angles in degrees;
        ``self.tilt_history`` holds them after every pass, ``self.tilt_cost`` per pass a dict of ``rr`` (per projection, sum of
        (b - A x)^2 over the samples ``margin`` inside the image), ``count`` and ``data_distance`` (||A x - b|| of the pass's
        reconstruction, BEFORE its step); ``get_tilt_angles()`` reports the current angles.  Stored shifts, rotation and
        magnification are not touched.  ``apply=False`` leaves the engine with the angles it had on entry (they are put back).

        ``factor`` = 2 or 4: reconstruction, derivative and sums run on the kept binned object (``binned``): angles do not depend on
        resolution, and a rebuild of the coarse tables costs about 1 / factor^2 of this engine's.  Only the coarse object changes
        angles between passes; this object's engine is rebuilt ONCE at the end.  ``recon`` is then called with the coarse object.
        ``margin`` is in full-resolution pixels: the coarse object leaves out ``margin // factor`` of its own.

        Overwrites on the engine it runs on: the reconstruction, ``VOL_TEMP`` (the derivative volume), ``SINO_G`` and sinogram slot
        ``align.TILT_SCRATCH_SLOT``.  A rebuild carries ``SINO_B`` and ``ALIGN_SLOT`` across and drops every kept binned object.

        Capture range: the step is a linearisation in the angle, good while the angle error moves the outermost detail by about a
        pixel or two (1 degree is 0.28 pixel at the border of a 32-pixel image, 4.5 pixels at 512); errors far below a pixel at the
        border are below what the data resolve.  One whole-volume engine only (``NotImplementedError`` otherwise)."""
        t = self._bin_engine()
        f = int(factor)
        if f not in (1, 2, 4):
            raise ValueError("factor must be 1, 2 or 4")
        if int(Nouter) < 0:
            raise ValueError("Nouter must not be negative")
        if recon is None:
            recon = lambda rec: rec.sirt(100, show_convergence=False)  # noqa: E731
        start = self.get_tilt_angles()
        ang = start.copy()
        self.tilt_history, self.tilt_cost = [], []
        moved = False                     # the engine of this object (f == 1) or of the coarse one no longer has ``start``
        for k in range(int(Nouter)):
            rec = self if f == 1 else self._coarse(f)          # (bins the current series into the kept coarse object)
            recon(rec)
            rd, dd, rr, count = align.match_tilt_angles(rec.tomo, SINO_B, VOL_RECON, margin=int(margin) // f)
            dist = rec.tomo.data_distance()
            ang = ang + align.tilt_increment(rd, dd, damping, max_step_deg)
            self.tilt_history.append(ang.copy())
            self.tilt_cost.append(dict(rr=rr, count=count, data_distance=dist))
            if k < int(Nouter) - 1:
                if f == 1:
                    self._set_tilt_angles(ang)
                else:
                    rec.tomo.update_projection_angles(np.deg2rad(ang))     # its series is binned again by the next pass
                moved = True
        if apply and self.tilt_history:
            self._set_tilt_angles(ang)
        elif moved:
            if f == 1:
                self._set_tilt_angles(start)
            else:
                self._pyramid.pop(f, None)
        return ang.copy()

    # ---- DART: discrete tomography (an extension; Batenburg & Sijbers 2011; engine.py dart_*) -------------------------------------
    def _dart_engine(self):
        t = self.tomo
        if not hasattr(t, "_dart_one_engine"):
            raise NotImplementedError("DART runs on one whole-volume engine, not on a volume sharded over devices")
        t._dart_one_engine()
        return t

    def _recon_range(self):
        """(min, max) of the current reconstruction: a torch reduction on the device where torch sees it, else on the host."""
        t = self.tomo
        try:
            import torch
            on_device = torch.cuda.is_available() and torch.cuda.device_count() > t.gpuID
        except ImportError:
            on_device = False
        if on_device:
            x = t.get_volume_tensor(VOL_RECON)
            return float(x.min()), float(x.max())
        x = t.get_volume(VOL_RECON)
        return float(x.min()), float(x.max())

    def estimate_grey_levels(self, K, iters=20):
        """K grey levels of the current reconstruction by 1-D Lloyd (k-means) iterations: start at ``linspace(min, max, K)``; per
        iteration the thresholds are the midpoints of adjacent levels and every level moves to the mean of its class
        (``dart_class_stats``: sums and counts in binary64 on the device); an empty class keeps its level.  -> float64 array (K,)."""
        t = self._dart_engine()
        K = int(K)
        if not 1 <= K <= 16:
            raise ValueError("K must be 1..16")
        lo, hi = self._recon_range()
        levels = np.linspace(lo, hi, K)
        for _ in range(int(iters)):
            if K == 1 or not np.all(np.diff(levels.astype(np.float32)) > 0):
                break                                                   # a constant volume: nothing to separate
            st = t.dart_class_stats(dart_thresholds(levels))
            new = np.where(st[:, 1] > 0, st[:, 0] / np.maximum(st[:, 1], 1.0), levels)
            if np.array_equal(new, levels):
                break
            levels = new
        return levels

    def dart(self, grey_levels, Niter=20, arm_iters=10, init_iters=50, fix_probability=0.85, smoothing=0.1, connectivity=26, seed=0,
             segment=True):
        """DART (Batenburg & Sijbers, IEEE TIP 20(9), 2011) for an object made of K known grey levels.

        ``grey_levels``: K ascending values, or an int K: the levels are then estimated from the current reconstruction
        (``estimate_grey_levels``, after the initial SIRT run below).  The thresholds are the midpoints of adjacent levels.
        If the reconstruction is all zero (the ``restart_recon`` state) ``init_iters`` SIRT iterations make the starting point.
        Then, ``Niter`` times: segment the reconstruction (``dart_classify``: boundary voxels are free, and every other voxel with
        probability 1 - ``fix_probability``, drawn from ``seed_k = (seed * 0x9E3779B1 + k) mod 2^32``); set the fixed voxels to
        their grey level; run ``arm_iters`` SIRT iterations in which the fixed voxels are put back after every one (``dart_arm``);
        move every free voxel by ``smoothing`` towards the mean of its 26 neighbours (skipped at 0; the smoother writes into
        volume slot ``VOL_USER0`` and the result is copied back, so WHATEVER THE CALLER KEPT IN ``VOL_USER0`` IS OVERWRITTEN).  With ``segment`` the loop ends with one more segmentation without random voxels and ``dart_restore(everywhere=True)``,
        which sets EVERY voxel, boundary included, to the grey level of its label: the volume then holds only the K values.
        ``get_dart_labels()`` gives the labels of the last segmentation.

        -> dict of arrays, one entry per iteration: ``data_distance`` (||A x - b|| after the iteration), ``n_free``, ``n_boundary``;
        ``grey_levels`` holds the levels used.  ``self.cost`` is replaced by the ``data_distance`` array, as the other drivers do."""
        t = self._dart_engine()
        pytvlib.initialize_algorithm(t, "SIRT")
        lo, hi = self._recon_range()
        if lo == 0.0 and hi == 0.0:
            t.SIRT(int(init_iters))
        if isinstance(grey_levels, (bool, np.bool_)):
            raise TypeError("grey_levels must be a sequence of grey levels or an int K, not a bool")
        if isinstance(grey_levels, (int, np.integer)):
            levels = self.estimate_grey_levels(int(grey_levels))
        else:
            levels = np.asarray(grey_levels, dtype=np.float64).ravel()
        grey = levels.astype(np.float32)
        if grey.size < 1 or grey.size > 16 or not np.all(np.isfinite(grey)) or not np.all(np.diff(grey) > 0):
            raise ValueError("grey_levels must be 1..16 finite, strictly ascending values (as float32)")
        thr = dart_thresholds(levels)
        free_fraction = 1.0 - float(fix_probability)
        if not 0.0 <= free_fraction <= 1.0:
            raise ValueError("fix_probability must lie in [0, 1]")
        Niter = int(Niter)
        out = {"data_distance": np.zeros(Niter), "n_free": np.zeros(Niter, np.int64), "n_boundary": np.zeros(Niter, np.int64),
               "grey_levels": levels.copy()}
        for k in range(Niter):
            seed_k = (int(seed) * 0x9E3779B1 + k) & 0xffffffff
            out["n_free"][k], out["n_boundary"][k] = t.dart_classify(thr, VOL_RECON, connectivity, seed_k, free_fraction)
            t.dart_restore(grey)
            t.dart_arm(int(arm_iters), grey)
            if smoothing != 0:
                t.dart_smooth(VOL_RECON, VOL_USER0, float(smoothing))
                t.be.c("copy_volume", VOL_RECON, VOL_USER0)
            out["data_distance"][k] = t.data_distance()
        if segment:
            t.dart_classify(thr, VOL_RECON, connectivity, 0, 0.0)
            t.dart_restore(grey, everywhere=True)
        self.cost = out["data_distance"]
        return out

    def get_dart_labels(self):
        """(Nslice, Nray, Nray) uint8: the label (index into the grey levels) of every voxel in the last segmentation."""
        return self._dart_engine().dart_state() & _lib.DART_LABEL_MASK

    # ---- particles: connected components of the thresholded reconstruction (an extension; engine.py *_components) -----------------
    def _components_engine(self):
        t = self.tomo
        if not hasattr(t, "_components_one_engine"):
            raise NotImplementedError("component labelling runs on one whole-volume engine, not on a volume sharded over devices")
        t._components_one_engine()
        return t

    def label_particles(self, threshold=None, level=None, connectivity=26, min_voxels=1, fill=0.0):
        """The particle table of the current reconstruction: its connected components (6 or 26 neighbours) on the device.

        Foreground is ``x >= threshold``; ``threshold=None`` takes the midpoint of the two levels of ``estimate_grey_levels(2)``.
        ``level=(g, tol)`` selects ``g - tol <= x <= g + tol`` instead: one grey level of a DART result.  ``min_voxels > 1`` sets
        the components with fewer voxels to ``fill`` IN THE RECONSTRUCTION (``keep_components``) and labels again, so that the
        numbers stay contiguous.  -> dict: ``count`` K and, per particle in label order (ascending smallest voxel index, the
        numbering of ``scipy.ndimage.label``), ``voxels``, ``centroid`` (K, 3) float64 in (s, y, z), ``bbox`` (K, 2, 3) inclusive
        min / max, ``surface`` (voxels with a face neighbour outside the particle), ``equivalent_diameter`` (of the sphere with
        ``voxels``) and ``first``.  ``get_particle_labels()`` gives the label volume."""
        t = self._components_engine()
        if level is not None:
            if threshold is not None:
                raise ValueError("give a threshold or a level, not both")
            g, tol = (float(v) for v in level)
            if not tol >= 0.0:
                raise ValueError("the tolerance of a level must not be negative")
            lo, hi = g - tol, g + tol
        else:
            if threshold is None:
                threshold = float(np.mean(self.estimate_grey_levels(2)))
            lo, hi = float(threshold), float("inf")
        if int(min_voxels) < 1:
            raise ValueError("min_voxels must be at least 1")
        t.label_components(VOL_RECON, lo, hi, connectivity)
        st = t.component_stats()
        keep = particles_to_keep(st["voxels"], min_voxels)
        if not keep[1:].all():
            t.keep_components(VOL_RECON, keep, fill)
            t.label_components(VOL_RECON, lo, hi, connectivity)
            st = t.component_stats()
        return particle_table(st)

    def get_particle_labels(self):
        """(Nslice, Nray, Nray) int32: 0 for background, k for the voxels of particle k of the last ``label_particles``."""
        return self._components_engine().component_labels()

    def _tensor_engine(self):
        if not hasattr(self.tomo, "get_volume_tensor") or getattr(self.tomo, "comm", None) is not None:
            raise NotImplementedError("as_tensor needs the whole volume on one device: a sharded engine hands out its local slab "
                                      "(tomo.get_volume_tensor), the gathering calls return numpy")
        return self.tomo

    def get_recon(self, as_tensor=False, dtype=None):
        """(Nslice, Nray, Nray) float64 like the reference (gpu/reconstructor.py:207-215).  ``as_tensor=True``: a torch tensor on the
        engine's device instead (``dtype`` torch.float32 by default, or torch.float64), converted on the device, no host copy."""
        if as_tensor:
            return self._tensor_engine().get_volume_tensor(VOL_RECON, dtype=dtype)
        self.recon = self.tomo.get_volume(VOL_RECON).astype(np.float64)
        return self.recon

    def get_projections(self, as_tensor=False, dtype=None):
        """The tilt series the engine holds, (Nslice, Nray, Nangles) as it was given (the reference's stub: gpu/reconstructor.py:217):
        numpy float32, or with ``as_tensor=True`` a torch tensor on the engine's device."""
        if as_tensor:
            return self._tensor_engine().get_projections_tensor(SINO_B, SINO_PUBLIC, dtype=dtype)
        b = self.tomo.get_projections()
        return np.ascontiguousarray(b.reshape(self.Nslice, self.Nangles, self.Nray).transpose(0, 2, 1))
