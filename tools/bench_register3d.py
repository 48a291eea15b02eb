#!/usr/bin/env python3
"""One Gauss-Newton evaluation of the 3-D registration at 512^3 (``--n`` for another size): ``tomo_volume_affine_normal`` for the
identity and for the 8 degree-plus-shift map of the registered dual-axis case, next to ``tomo_volume_affine`` with the same map in the
same run -- the yardstick: the same gathers, one more volume read (F) and no store.  The ratio of the two times is what is recorded.

Times are wall clock around ``reps`` calls, the best of three rounds; ``tomo_volume_affine_normal`` waits for its 32 numbers in every
call (that wait and the 256-byte read-back are inside its time), the resampling calls are enqueued back to back and waited for once.
Needs a GPU: there is nothing to fall back to.  Writes profiles/register3d.md (``--out``)."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from tomo_tv_amd._lib import VOL_RECON  # noqa: E402
from tomo_tv_amd.align import affine_matrix_3d  # noqa: E402
from tomo_tv_amd.engine import tomoengine  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=512, help="the cube's edge")
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "register3d.md"))
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_register3d: no GPU")
dev = torch.device("cuda", 0)
n = a.n
nvox = n ** 3
shape = (n, n, n)

ea = tomoengine(n, n, np.deg2rad([-30.0, 30.0]), device=0)        # the moving volume G / the source of the resampling
eb = tomoengine(n, n, np.deg2rad([-30.0, 30.0]), device=0)        # the fixed volume F / the destination


def sync():
    ea.synchronize()
    eb.synchronize()
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
ea.set_volume_tensor(torch.rand(shape, device=dev, generator=gen), VOL_RECON)
F = torch.rand(shape, device=dev, generator=gen)
sync()

maps = [("identity", affine_matrix_3d(src_shape=shape)),
        ("8 degrees about y + shift (1.5, 0, -2.25)", affine_matrix_3d((0, 8, 0), (1.5, 0, -2.25), src_shape=shape))]
rows = []
for name, M in maps:
    t_aff = wall(lambda: ea.volume_affine_to(eb, M))
    eb.set_volume_tensor(F, VOL_RECON)                             # the resampling overwrote the fixed engine's volume
    sync()
    t_norm = wall(lambda: eb.volume_affine_normal(ea, M, margin=1))
    count = eb.volume_affine_normal(ea, M, margin=1)[3]
    rows.append((name, t_aff * 1e3, t_norm * 1e3, t_norm / t_aff, count / nvox))
    print(rows[-1], flush=True)

lines = [f"# One evaluation of the 3-D registration's normal equations on the MI355X: {n}^3", "",
         f"Wall clock around {a.reps} calls, best of three rounds.  `tomo_volume_affine_normal` waits for its result in every call; the",
         "resampling calls are waited for once per round.  Both engines hold uniform random volumes; margin 1.", "",
         "| map | tomo_volume_affine, ms | tomo_volume_affine_normal, ms | ratio | voxels that count |", "|---|---|---|---|---|"]
for name, ta, tn, ratio, frac in rows:
    lines.append(f"| {name} | {ta:.3f} | {tn:.3f} | {ratio:.2f} | {100 * frac:.1f} % |")
lines += ["", "Algorithmic traffic: the resampling reads and writes a volume (8 B/voxel); the normal equations read two and write 8 KB per",
          "workgroup at most.  Per counting voxel the kernel adds about 45 binary64 fused multiply-adds (21 + 6 + 4 sums, the cross",
          "product and q) to the gather's arithmetic.", ""]
os.makedirs(os.path.dirname(a.out), exist_ok=True)
with open(a.out, "w") as f:
    f.write("\n".join(lines))
print("\n".join(lines))
