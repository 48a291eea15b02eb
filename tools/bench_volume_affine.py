#!/usr/bin/env python3
"""The 3-D affine resampling of a volume at 512^3 (``--n`` for another size): ``tomo_volume_affine`` (8 B/voxel algorithmic: one read,
one write) and ``tomo_volume_affine_axpy`` (12 B/voxel) as a rate and as a share of the copy ceiling, for the identity, a 5 degree
rotation about s, about y and about z, the 8 degree-plus-shift map of the registered dual-axis case, and the pure permutation through
the affine kernel against ``tomo_volume_cross`` followed by a near-identity affine (the composed route of ``DualAxisTomo``).

The ceiling is the best read+write figure of ``tools/micro/copy_patterns <n> <n>`` (hipcc -O3 --offload-arch=gfx950
tools/micro/copy_patterns.hip), run here as a child process in the same run when the program exists (``--copy-patterns``), else a
torch ``copy_`` probe.  Times are wall clock around ``reps`` calls that end in a synchronise of both engines, the best of three
rounds.  Needs a GPU: there is nothing to fall back to.  Writes profiles/volume_affine.md (``--out``)."""
import argparse
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from tomo_tv_amd._lib import VOL_RECON, VOL_USER0  # noqa: E402
from tomo_tv_amd.align import affine_matrix_3d  # noqa: E402
from tomo_tv_amd.engine import tomoengine  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=512, help="the cube's edge")
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--copy-patterns", default=os.path.join(ROOT, "tools", "micro", "copy_patterns"))
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "volume_affine.md"))
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_volume_affine: no GPU")
dev = torch.device("cuda", 0)
n = a.n
nvox = n ** 3
shape = (n, n, n)

patterns = []
if os.path.exists(a.copy_patterns):
    out = subprocess.run([a.copy_patterns, str(n), str(n)], capture_output=True, text=True, timeout=300).stdout
    patterns = [(m.group(1).strip(), float(m.group(2))) for m in re.finditer(r"^(.*?)\s+[\d.]+ us\s+(\d+) GB/s$", out, re.M)]
    print(out, flush=True)

ea = tomoengine(n, n, np.deg2rad([-30.0, 30.0]), device=0)
eb = tomoengine(n, n, np.deg2rad([-30.0, 30.0]), device=0)


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


x = torch.rand(shape, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
ea.set_volume_tensor(x, VOL_RECON)
eb.set_volume_tensor(x, VOL_RECON)
sync()
src, dst = torch.empty(nvox, device=dev), torch.empty(nvox, device=dev)
torch_copy = 8.0 * nvox / wall(lambda: dst.copy_(src)) / 1e9
del src, dst
if patterns:
    ceiling, ceiling_src = max(p[1] for p in patterns), f"the best pattern of tools/micro/copy_patterns {n} {n} in this run (in-place read + write)"
else:
    ceiling, ceiling_src = torch_copy, "torch copy_ of one volume, read + write (tools/micro/copy_patterns was not built)"

rows = []


def row(name, seconds, bpv):
    rate = bpv * nvox / seconds / 1e9
    rows.append((name, seconds * 1e3, bpv, rate, rate / ceiling))
    print(rows[-1], flush=True)


SCR = VOL_USER0
maps = [("identity", affine_matrix_3d(src_shape=shape)),
        ("5 degrees about s", affine_matrix_3d((5, 0, 0), src_shape=shape)),
        ("5 degrees about y", affine_matrix_3d((0, 5, 0), src_shape=shape)),
        ("5 degrees about z", affine_matrix_3d((0, 0, 5), src_shape=shape)),
        ("8 degrees about y + shift (1.5, 0, -2.25)", affine_matrix_3d((0, 8, 0), (1.5, 0, -2.25), src_shape=shape))]
for name, M in maps:
    row(f"tomo_volume_affine, {name}", wall(lambda: ea.volume_affine_to(eb, M)), 8)
name, M = maps[-1]
row(f"tomo_volume_affine_axpy (clamp), {name}", wall(lambda: ea.volume_affine_axpy_to(eb, M, 0.5, clamp=True)), 12)
row(f"tomo_volume_affine within one engine, {name}", wall(lambda: ea.volume_affine_to(ea, M, dst=SCR)), 8)
perm = np.array([0, 0, 1, 0, 0, 1, 0, 0, 1, 0, 0, 0], np.float64)
row("pure permutation through the affine kernel", wall(lambda: ea.volume_affine_to(eb, perm)), 8)
near = np.asarray(M, np.float64).reshape(3, 4)
direct = near[[2, 1, 0], :].ravel()                                              # the permutation after the near-identity map: one call
row("near-permutation, direct (one affine call)", wall(lambda: ea.volume_affine_to(eb, direct)), 8)
row("near-permutation, composed (tomo_volume_cross + near-identity affine within the destination)",
    wall(lambda: (ea.cross_volume_to(eb, dst=SCR), eb.volume_affine_to(eb, M, src=SCR, dst=VOL_RECON))), 8)
row("tomo_volume_cross alone", wall(lambda: ea.cross_volume_to(eb)), 8)
row("torch copy_ of one volume", 8.0 * nvox / torch_copy / 1e9, 8)

lines = [f"# 3-D affine resampling of a volume on the MI355X: {n}^3", "",
         f"Copy ceiling {ceiling:.0f} GB/s: {ceiling_src}.  Wall clock around {a.reps} calls ending in a synchronise, best of three rounds.",
         "GB/s is the algorithmic traffic (8 B/voxel: one read, one write; 12 B/voxel for the fused multiply-add form) over that time; the",
         "composed route is charged 8 B/voxel too, so that its row compares with the direct one.", "",
         "| call | ms | algorithmic B/voxel | GB/s | of the copy ceiling |", "|---|---|---|---|---|"]
for name, ms, bpv, rate, frac in rows:
    lines.append(f"| {name} | {ms:.3f} | {bpv} | {rate:.0f} | {100 * frac:.0f} % |")
if patterns:
    lines += ["", f"`copy_patterns {n} {n}` in the same run:", "", "| pattern | GB/s |", "|---|---|"] + [f"| {p} | {r:.0f} |" for p, r in patterns]
near_identity = [frac for name, _, _, _, frac in rows if name.startswith("tomo_volume_affine, ") and "identity" not in name]
if near_identity and min(near_identity) < 0.5:
    lines += ["", f"The near-identity maps reach {100 * min(near_identity):.0f} - {100 * max(near_identity):.0f} % of the copy ceiling, below half of it.",
              "SUPPOSED, not backed by a `rocprofv3 --pmc FETCH_SIZE` / `WRITE_SIZE` run: what binds is the tap loads per lane -- eight 4-byte",
              "gathers per voxel, 32 per 16 bytes stored, each with 64-bit address arithmetic and three bounds predicates -- and, for",
              "rotations about y or z, the smaller cache-line reuse between consecutive lanes (their taps spread over more source rows",
              "than under a rotation about s); not the HBM bytes, which the identity row moves at a multiple of that rate."]
lines.append("")
os.makedirs(os.path.dirname(a.out), exist_ok=True)
with open(a.out, "w") as f:
    f.write("\n".join(lines))
print("\n".join(lines))
