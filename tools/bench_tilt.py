#!/usr/bin/env python3
"""The two kernels of the tilt-angle refinement at 512 x 512 x 90 (``--nslice``, ``--n``, ``--nproj`` for another size) against the copy
ceiling measured in the same run: ``tomo_volume_rot_derivative`` (one volume read through a four-point stencil, one written) and
``tomo_sino_tilt_normal`` (three series read, nothing written), each next to a device-to-device copy of the same number of bytes it
moves at least (a copy of N bytes reads N and writes N: 2 N bytes of traffic).  The stand-alone figure of the copy ceiling is
tools/micro/copy_patterns.hip; the copy here is the yardstick of THIS run, on this device, at this size.

The derivative is enqueued ``reps`` times and waited for once; the sums wait for their 4 numbers per projection in every call, so their
time includes one stream wait and the second reduction stage.  Wall clock, the best of three rounds.  One whole pass of
``align.match_tilt_angles`` (derivative, two projections, sums) is timed beside them.  Needs a GPU: there is nothing to fall back to.
Writes profiles/tilt_refine.md (``--out``)."""
import argparse
import ctypes
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from tomo_tv_amd import _lib, align  # noqa: E402
from tomo_tv_amd._lib import SINO_B, SINO_PACKED, SINO_USER0, VOL_RECON, VOL_TEMP  # noqa: E402
from tomo_tv_amd.engine import tomoengine  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--nslice", type=int, default=512)
ap.add_argument("--n", type=int, default=512, help="rays per projection")
ap.add_argument("--nproj", type=int, default=90)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tilt_refine.md"))
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_tilt: no GPU")
dev = torch.device("cuda", 0)
ns, n, P = a.nslice, a.n, a.nproj
B_SLOT, G_SLOT, D_SLOT = SINO_USER0, SINO_USER0 + 1, SINO_USER0 + 2

eng = tomoengine(ns, n, np.deg2rad(np.linspace(-70, 70, P)), device=0)
L, h = _lib.load(), eng.be.h


def sync():
    eng.synchronize()
    torch.cuda.synchronize(dev)


def wall(fn, reps=a.reps):
    fn()
    sync()
    best = float("inf")
    for _ in range(3):
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        sync()
        best = min(best, (time.perf_counter() - t0) / reps)
    return best


gen = torch.Generator(device=dev).manual_seed(1)
eng.set_volume_tensor(torch.rand((ns, n, n), device=dev, generator=gen), VOL_RECON)
for slot in (SINO_B, B_SLOT, G_SLOT, D_SLOT):
    eng.be.set_tilt_series_tensor(torch.rand((ns, n * P), device=dev, generator=gen), SINO_PACKED, slot)
sync()

sx = -(-ns // 64) * 64                                 # the row pitch: padding slices are moved like real ones
vol_bytes, sino_bytes = 4 * n * n * sx, 4 * n * P * sx
out = np.empty((P, 4), np.float64)
po = out.ctypes.data_as(ctypes.c_void_p)


def copy_time(nbytes):
    """a device-to-device copy that moves ``nbytes`` in all (half read, half written)"""
    x = torch.empty(nbytes // 8, dtype=torch.float32, device=dev).normal_()
    y = torch.empty_like(x)
    return wall(lambda: y.copy_(x))


t_der = wall(lambda: _lib.check(L.tomo_volume_rot_derivative(h, VOL_RECON, VOL_TEMP)))
t_der_copy = copy_time(2 * vol_bytes)
t_sum = wall(lambda: _lib.check(L.tomo_sino_tilt_normal(h, B_SLOT, G_SLOT, D_SLOT, 1, po)))
t_sum_copy = copy_time(3 * sino_bytes)
t_pass = wall(lambda: align.match_tilt_angles(eng, SINO_B), reps=max(1, a.reps // 4))

rows = [("tomo_volume_rot_derivative", 2 * vol_bytes, t_der, t_der_copy), ("tomo_sino_tilt_normal", 3 * sino_bytes, t_sum, t_sum_copy)]
lines = [f"# The kernels of the tilt-angle refinement on the MI355X: {ns} slices x {n} rays x {P} projections", "",
         f"Wall clock around {a.reps} calls, best of three rounds, through the ctypes table.  `bytes` is the least traffic of the call (the",
         "derivative: one volume read, one written, the four neighbour rows counted once; the sums: three series read, the padded row",
         "pitch included).  `copy` is a device-to-device copy moving the same number of bytes, timed in the same run; the ratio is the call's",
         "time over the copy's.  The sums wait for the stream and run their second stage inside every call.", "",
         "| call | bytes, MB | time, ms | GB/s | copy of the same bytes, ms | copy GB/s | ratio |", "|---|---|---|---|---|---|---|"]
for name, nb, t, tc in rows:
    lines.append(f"| {name} | {nb / 1e6:.1f} | {t * 1e3:.3f} | {nb / t / 1e9:.0f} | {tc * 1e3:.3f} | {nb / tc / 1e9:.0f} | {t / tc:.2f} |")
    print(lines[-1], flush=True)
lines += ["", f"One evaluation (`align.match_tilt_angles`: derivative, two forward projections, sums): {t_pass * 1e3:.2f} ms.", "",
          "Not measured here: hardware counters of either kernel, the stand-alone copy ceiling of tools/micro/copy_patterns.hip, and the",
          "rebuild of the tables that `TomoGPU.refine_tilt_angles` pays once per pass at full resolution.", ""]
os.makedirs(os.path.dirname(a.out), exist_ok=True)
with open(a.out, "w") as f:
    f.write("\n".join(lines))
print("\n".join(lines))
