#!/usr/bin/env python3
"""DART kernels at 512^3 (``--n`` for another size): time per kernel with its algorithmic bytes (classify 5 B/voxel: 4 read, 1 state
byte written; restore 9 B: state + volume read, volume written; smooth 9 B: volume + state read, volume written) as a rate and as a
fraction of the copy ceiling (``--ceiling-GBps``: the read+write figure of tools/micro/copy_patterns.hip measured on the same device,
or a torch ``copy_`` probe run here when it is not given); one full DART iteration (classify, restore, ``arm_iters`` masked SIRT
iterations, smooth + copy back, data distance) against ``arm_iters`` plain SIRT iterations; and a torch baseline for the boundary
(label tensor, then ``max_pool3d`` of the labels and of their negation: boundary = local max != local min).

Times are wall clock around ``reps`` calls that end in a stream synchronise.  Needs a GPU: there is nothing to fall back to.
Writes profiles/dart.md (``--out``)."""
import argparse
import ctypes
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from tomo_tv_amd._lib import VOL_RECON, VOL_USER0  # noqa: E402
from tomo_tv_amd.engine import tomoengine  # noqa: E402
from tomo_tv_amd.phantom import tilt_angles  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=512, help="Nslice = Nray = n")
ap.add_argument("--angles", type=int, default=90)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--arm-iters", type=int, default=10)
ap.add_argument("--ceiling-GBps", type=float, default=None)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "dart.md"))
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_dart: no GPU")
dev = torch.device("cuda", 0)
n, P = a.n, a.angles
nvox = n ** 3
t = tomoengine(n, n, np.deg2rad(tilt_angles(P)), device=0)


def sync():
    t.synchronize()
    torch.cuda.synchronize(dev)


def wall(fn, reps=a.reps):
    fn()
    sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    sync()
    return (time.perf_counter() - t0) / reps


# a two-phase object with noise: both interior and boundary voxels, like a reconstruction in mid-run
g = torch.Generator(device=dev).manual_seed(1)
ax = torch.arange(n, device=dev, dtype=torch.float32) - (n - 1) / 2
r2 = ax[:, None, None] ** 2 + ax[None, :, None] ** 2 + ax[None, None, :] ** 2
x = (r2 < (0.35 * n) ** 2).float() + 0.1 * torch.randn((n, n, n), device=dev, generator=g)
t.set_volume_tensor(x, VOL_RECON)
t.set_volume_tensor((r2 < (0.35 * n) ** 2).float(), 2)
t.create_projections()
sync()

ceiling = a.ceiling_GBps
ceiling_src = "the best pattern of tools/micro/copy_patterns.hip (in-place read + write of a 512^3 volume), passed in"
if ceiling is None:
    src, dst = torch.empty(nvox, device=dev), torch.empty(nvox, device=dev)
    ceiling = 8.0 * nvox / wall(lambda: dst.copy_(src)) / 1e9
    ceiling_src = "torch copy_ of one volume, read + write (run here)"
    del src, dst

thr, grey = [0.5], [0.0, 1.0]
rows = []


def row(name, seconds, nbytes):
    rate = nbytes / seconds / 1e9 if nbytes else None
    rows.append((name, seconds * 1e3, nbytes / nvox if nbytes else None, rate, rate / ceiling if rate else None))
    print(rows[-1], flush=True)


thr_a = np.asarray(thr, np.float32)
grey_a = np.asarray(grey, np.float32)
thr_p, grey_p = thr_a.ctypes.data_as(ctypes.c_void_p), grey_a.ctypes.data_as(ctypes.c_void_p)
fthr = int(0.15 * 2 ** 32)
for C in (6, 26):
    row(f"k_dart_classify<{C}>", wall(lambda: t.be.c("dart_classify", VOL_RECON, thr_p, 1, C, 1, fthr)), 5 * nvox)
t.be.c("copy_volume", VOL_USER0, VOL_RECON)
row("k_dart_restore", wall(lambda: t.be.c("dart_restore", VOL_USER0, grey_p, 2)), 9 * nvox)
row("k_dart_smooth", wall(lambda: t.be.c("dart_smooth", VOL_RECON, VOL_USER0, 0.1)), 9 * nvox)
out = np.zeros((2, 2))
row("k_dart_class_stats (2 classes, waits)", wall(lambda: t.be.c("dart_class_stats", VOL_RECON, thr_p, 1, out.ctypes.data_as(ctypes.c_void_p))), 4 * nvox)


def torch_boundary():
    lab = (x >= 0.5).float()[None, None]
    mx = torch.nn.functional.max_pool3d(lab, 3, 1, 1)
    mn = -torch.nn.functional.max_pool3d(-lab, 3, 1, 1)
    return mx != mn


row("torch baseline: labels + 2 x max_pool3d (26-boundary, padding -inf = no wrap)", wall(torch_boundary, max(2, a.reps // 4)), 5 * nvox)


def dart_iteration():
    t.be.c("dart_classify", VOL_RECON, thr_p, 1, 26, 1, fthr)
    t.be.c("dart_restore", VOL_RECON, grey_p, 2)
    t.be.c("dart_arm", VOL_RECON, 0, a.arm_iters, grey_p, 2)
    t.be.c("dart_smooth", VOL_RECON, VOL_USER0, 0.1)
    t.be.c("copy_volume", VOL_RECON, VOL_USER0)
    t.data_distance()


t_iter = wall(dart_iteration, 3)
t_sirt = wall(lambda: t.be.c("sirt", VOL_RECON, a.arm_iters), 3)
lines = [f"# DART kernels on the MI355X: {n}^3, {P} angles", "",
         f"Copy ceiling {ceiling:.0f} GB/s: {ceiling_src}.  Wall clock around {a.reps} calls ending in a synchronise.", "",
         "| kernel | ms | algorithmic B/voxel | GB/s | of the copy ceiling |", "|---|---|---|---|---|"]
for name, ms, bpv, rate, frac in rows:
    lines.append(f"| {name} | {ms:.3f} | {bpv:.0f} | {rate:.0f} | {100 * frac:.0f} % |")
lines += ["", f"One DART iteration (classify, restore, {a.arm_iters} masked SIRT iterations, smooth, copy back, data distance): {t_iter * 1e3:.1f} ms; "
          f"{a.arm_iters} plain SIRT iterations: {t_sirt * 1e3:.1f} ms; overhead {100 * (t_iter / t_sirt - 1):.1f} %.", ""]
os.makedirs(os.path.dirname(a.out), exist_ok=True)
with open(a.out, "w") as f:
    f.write("\n".join(lines))
print("\n".join(lines))
