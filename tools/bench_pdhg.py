#!/usr/bin/env python3
"""Time a Chambolle-Pock iteration (tomo_pdhg) and its fused pass (k_pdhg_tv) beside the FISTA iteration and k_fgp_fused2 of the
same session; optionally list the cost per iteration of PDHG (both step modes) and FISTA on one phantom.  ``--slabs K``: the fused SLAB
pass and one whole iteration on K slab engines of one device instead (the sharded form without a second GPU).

One engine, seeded phantom as tools/run_config.py.  Whole iterations: the host clock around K enqueued iterations closed by a
synchronise (one call enqueues all K; warm-up first; the median of --reps repeats).  Kernels: the engine's HIP-event launch log
(tomo_profile_*).  Bytes: 44 per voxel for k_pdhg_tv, 28 per voxel and PAIR of iterations for k_fgp_fused2; roof 8.0 TB/s."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tomo_tv_amd import _lib, pytvlib                                          # noqa: E402
from tomo_tv_amd._lib import K_FGP_GRAD, K_PDHG_TV, VOL_ORIGINAL, VOL_YK       # noqa: E402
from tomo_tv_amd.engine import tomoengine                                      # noqa: E402
from tomo_tv_amd.phantom import ellipsoids, tilt_angles                        # noqa: E402

ROOF = 8.0e12


def kernel_ms(t, kernel, run):
    L = _lib.load()
    _lib.check(L.tomo_profile_enable(t.be.h, kernel, 1))
    run()
    n, ms = ctypes.c_int64(0), ctypes.c_double(0)
    _lib.check(L.tomo_profile_read(t.be.h, kernel, ctypes.byref(n), ctypes.byref(ms)))
    _lib.check(L.tomo_profile_enable(t.be.h, kernel, 0))
    return int(n.value), float(ms.value)


def timed(t, run, reps):
    out = []
    for _ in range(reps):
        t.synchronize()
        t0 = time.perf_counter()
        run()
        t.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out))


def fista_steps(t, k, lam, ntv, st):
    for _ in range(k):
        pytvlib.run(t, "fista")
        t.tv_fgp(ntv, lam, vol=VOL_YK)
        tk = 0.5 * (1 + np.sqrt(1 + 4 * st["t0"] ** 2))
        t.fista_momentum((st["t0"] - 1) / tk)
        st["t0"] = tk


ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=512)
ap.add_argument("--nslice", type=int, default=512)
ap.add_argument("--nproj", type=int, default=90)
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--lam", type=float, default=0.1)
ap.add_argument("--converge", type=int, default=0, help="also list the cost of this many iterations of PDHG (both modes) and FISTA")
ap.add_argument("--out", default="")
ap.add_argument("--slabs", type=int, default=0, help="K >= 2: time the fused SLAB pass and one whole iteration on K slab engines of this device instead")
a = ap.parse_args()


def run_slabs(a):
    """The volume as K slab engines on ONE device and one stream (the ring of tests/local_ring.py without the threads): per slab engine
    the fused slab pass (k_pdhg_tv<.., SLAB>, from the launch log) and, on the host clock, one whole iteration of all K engines
    {plane exchange by device copies, forward projection, dual sinogram, back projection, slab pass}."""
    from tomo_tv_amd.distributed import slab_partition
    K = a.slabs
    ang = np.deg2rad(tilt_angles(a.nproj))
    x = ellipsoids(a.nslice, a.n)
    eng = []
    for r in range(K):
        first, cnt = slab_partition(a.nslice, K, r)
        t = tomoengine(cnt, a.n, ang)
        t.be.enable_torch()                                                    # binds the plane tensors, runs on torch's stream
        t.be.c("set_slab_edges", int(r == 0), int(r == K - 1))
        t.set_volume(x[first:first + cnt], VOL_ORIGINAL)
        t.create_projections()
        eng.append(t)

    def exchange():
        for r, t in enumerate(eng):
            first, last, _, _ = t.be.pdhg_planes()
            eng[(r + 1) % K].be.pdhg_planes()[2].copy_(last)
            eng[(r - 1) % K].be.pdhg_planes()[3].copy_(first)

    def iterate(k, precond):
        for _ in range(k):
            exchange()
            for t in eng:
                t.be.c("pdhg_slab_iter", float(a.lam), 1.0, int(precond), 1.0, -1)

    def sync():
        for t in eng:
            t.synchronize()
    res = dict(shape=[a.nslice, a.n, a.n], nproj=a.nproj, iters=a.iters, reps=a.reps, slabs=K, slab_slices=[t.nloc for t in eng])
    for precond in (True, False):
        for t in eng:
            t.restart_recon()
            t.be.c("pdhg_slab_begin")
        iterate(3, precond)
        out = []
        for _ in range(a.reps):
            sync()
            t0 = time.perf_counter()
            iterate(a.iters, precond)
            sync()
            out.append((time.perf_counter() - t0) * 1e3 / a.iters)
        per = []
        for t in eng:
            n, kms = kernel_ms(t, K_PDHG_TV, lambda: iterate(a.iters, precond))
            per.append(kms / max(n, 1) * 1e3)
        res["pdhg_precond%d" % precond] = dict(ms_per_iteration_all_slabs=float(np.median(out)), k_pdhg_tv_slab_us=per)
        print(f"pdhg slabs={K} precond={int(precond)}: {np.median(out):.3f} ms per iteration of all {K} slab engines (one stream); slab pass "
              + " / ".join(f"{u:.1f}" for u in per) + " us per slab engine")
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if a.slabs >= 2:
    run_slabs(a)
    sys.exit(0)

t = tomoengine(a.nslice, a.n, np.deg2rad(tilt_angles(a.nproj)))
t.set_volume(ellipsoids(a.nslice, a.n), VOL_ORIGINAL)
t.create_projections()
vox = a.nslice * a.n * a.n
res = dict(shape=[a.nslice, a.n, a.n], nproj=a.nproj, iters=a.iters, reps=a.reps)
for precond in (True, False):
    t.restart_recon()
    t.pdhg_begin()
    t.pdhg(3, a.lam, precond=precond)                                          # warm-up: allocations, first launches
    ms = timed(t, lambda: t.pdhg(a.iters, a.lam, precond=precond), a.reps) / a.iters
    n, kms = kernel_ms(t, K_PDHG_TV, lambda: t.pdhg(a.iters, a.lam, precond=precond))
    k_us = kms / max(n, 1) * 1e3
    res["pdhg_precond%d" % precond] = dict(ms_per_iteration=ms, k_pdhg_tv_us=k_us, k_pdhg_tv_roof_fraction=44.0 * vox / (k_us * 1e-6) / ROOF)
    print(f"pdhg precond={int(precond)}: {ms:.3f} ms per iteration; k_pdhg_tv {k_us:.1f} us = {44.0 * vox / (k_us * 1e-6) / 1e12:.2f} TB/s "
          f"({100 * 44.0 * vox / (k_us * 1e-6) / ROOF:.0f} % of the roof)")
t.restart_recon()
pytvlib.initialize_algorithm(t, "fista")
st = {"t0": 1.0}
fista_steps(t, 2, a.lam, 10, st)
ms = timed(t, lambda: fista_steps(t, a.iters, a.lam, 10, st), a.reps) / a.iters
n, kms = kernel_ms(t, K_FGP_GRAD, lambda: fista_steps(t, a.iters, a.lam, 10, st))
k_us = kms / max(n, 1) * 1e3
res["fista_ntv10"] = dict(ms_per_iteration=ms, k_fgp_fused_us=k_us, k_fgp_fused_roof_fraction=28.0 * vox / (k_us * 1e-6) / ROOF)
print(f"fista (nTViter=10, no cost evaluation): {ms:.3f} ms per iteration; fused FGP pass {k_us:.1f} us = {28.0 * vox / (k_us * 1e-6) / 1e12:.2f} TB/s "
      f"({100 * 28.0 * vox / (k_us * 1e-6) / ROOF:.0f} % of the roof on 28 B per voxel and pair)")
if a.converge:
    # The cost both drivers report: 0.5 |A x - b|^2 + lam tv() (periodic, eps-smoothed TV).  PDHG minimises the same data term with
    # the Neumann TV; FISTA's gradient step is the ASTRA-normalised SIRT update (x + C A^T R (b - A x)), so its fixed point minimises
    # the R-weighted data term, not this one.
    conv = {}
    for name in ("pdhg_precond", "pdhg_scalar", "fista"):
        t.restart_recon()
        c = np.zeros(a.converge)
        if name == "fista":
            pytvlib.initialize_algorithm(t, "fista")
            st = {"t0": 1.0}
        else:
            t.pdhg_begin()
        for k in range(a.converge):
            if name == "fista":
                fista_steps(t, 1, a.lam, 10, st)
            else:
                t.pdhg(1, a.lam, precond=name == "pdhg_precond")
            c[k] = 0.5 * t.data_distance() ** 2 + a.lam * t.tv()
        conv[name] = c.tolist()
        print(name, " ".join(f"{v:.5g}" for v in c[:: max(1, a.converge // 10)]), f"last {c[-1]:.6g}")
    res["cost"] = conv
if a.out:
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
