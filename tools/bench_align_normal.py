#!/usr/bin/env python3
"""One Gauss-Newton evaluation of the per-projection matching at 512 x 512 x 90 (``--nslice``, ``--n``, ``--nproj`` for another size):
``tomo_sino_affine_normal`` for the identity and for a general map (1.5 degrees, magnification 1.01, a sub-pixel shift), next to
``tomo_sino_affine`` with the same maps in the same run -- the yardstick: the same gathers, one more series read (F) and no store.  The
ratio of the two times is what is recorded.

Both C calls are timed through the ctypes table itself (``_lib.load()``), with the matrices and the output preallocated: no wrapper,
no unpacking.  Times are wall clock around ``reps`` calls, the best of three rounds; both calls wait for the stream in every call (the
normal equations for their 21 numbers per projection, the resampling because its matrices are read from the caller's memory).  What
the Python wrapper ``sino_affine_normal`` adds on the host (checks, ``align.unpack_similarity_normal``) is a column of its own.
Needs a GPU: there is nothing to fall back to.  Writes profiles/align_normal.md (``--out``)."""
import argparse
import ctypes
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from tomo_tv_amd import _lib  # noqa: E402
from tomo_tv_amd._lib import SINO_PACKED, SINO_USER0  # noqa: E402
from tomo_tv_amd.align import affine_matrices, unpack_similarity_normal  # noqa: E402
from tomo_tv_amd.engine import tomoengine  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--nslice", type=int, default=512)
ap.add_argument("--n", type=int, default=512, help="rays per projection")
ap.add_argument("--nproj", type=int, default=90)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_normal.md"))
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_align_normal: no GPU")
dev = torch.device("cuda", 0)
ns, n, P = a.nslice, a.n, a.nproj
F_SLOT, G_SLOT, D_SLOT = SINO_USER0, SINO_USER0 + 1, SINO_USER0 + 2

eng = tomoengine(ns, n, np.deg2rad(np.linspace(-70, 70, P)), device=0)


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
for slot in (F_SLOT, G_SLOT):
    eng.be.set_tilt_series_tensor(torch.rand((ns, n * P), device=dev, generator=gen), SINO_PACKED, slot)
sync()

maps = [("identity", affine_matrices(np.zeros((P, 2)), 0.0, 1.0, n, ns)),
        ("1.5 degrees, magnification 1.01, shift (0.3, -0.6)", affine_matrices(np.tile([0.3, -0.6], (P, 1)), 1.5, 1.01, n, ns))]
L, h = _lib.load(), eng.be.h
out = np.empty((P, 21), np.float64)
po = out.ctypes.data_as(ctypes.c_void_p)


def host_only(fn, reps=200):
    fn()
    best = float("inf")
    for _ in range(3):
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        best = min(best, (time.perf_counter() - t0) / reps)
    return best


rows = []
for name, M in maps:
    M = np.ascontiguousarray(M, np.float64)
    pm = M.ctypes.data_as(ctypes.c_void_p)
    t_aff = wall(lambda: _lib.check(L.tomo_sino_affine(h, G_SLOT, D_SLOT, pm)))
    t_norm = wall(lambda: _lib.check(L.tomo_sino_affine_normal(h, F_SLOT, G_SLOT, pm, 2, po)))
    t_wrap = wall(lambda: eng.sino_affine_normal(F_SLOT, G_SLOT, M, margin=2))
    t_unpack = host_only(lambda: unpack_similarity_normal(out))
    count = eng.sino_affine_normal(F_SLOT, G_SLOT, M, margin=2)[3]
    rows.append((name, t_aff * 1e3, t_norm * 1e3, t_norm / t_aff, t_wrap * 1e3, t_unpack * 1e3, float(count.sum()) / (ns * n * P)))
    print(rows[-1], flush=True)

lines = [f"# One evaluation of the per-projection matching's normal equations on the MI355X: {ns} slices x {n} rays x {P} projections", "",
         f"Wall clock around {a.reps} calls, best of three rounds.  The two C calls are timed through the ctypes table with preallocated",
         "matrices and output; both wait for the stream in every call.  `wrapper` is `tomoengine.sino_affine_normal` (the C call plus checks",
         "and unpacking on the host), `unpack` is `align.unpack_similarity_normal` alone, host only.  Both slots hold uniform random series;",
         "margin 2.", "",
         "| map | tomo_sino_affine, ms | tomo_sino_affine_normal, ms | ratio of the C calls | wrapper, ms | unpack, ms | samples that count |",
         "|---|---|---|---|---|---|---|"]
for name, ta, tn, ratio, tw, tu, frac in rows:
    lines.append(f"| {name} | {ta:.3f} | {tn:.3f} | {ratio:.2f} | {tw:.3f} | {tu:.3f} | {100 * frac:.1f} % |")
lines += ["", "Algorithmic traffic: the resampling reads and writes a series (8 B/sample); the normal equations read two and write 168 B per",
          "workgroup.  Per counting sample the kernel adds 23 binary64 fused multiply-adds or additions (10 + 4 + 7 sums, J[2], J[3]) and",
          "three products to the gather's arithmetic.", ""]
os.makedirs(os.path.dirname(a.out), exist_ok=True)
with open(a.out, "w") as f:
    f.write("\n".join(lines))
print("\n".join(lines))
