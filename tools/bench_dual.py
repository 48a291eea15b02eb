#!/usr/bin/env python3
"""The dual-axis volume transpose at 512^3 (``--n`` for another size): ``tomo_volume_cross`` (8 B/voxel: one read, one write) and
``tomo_volume_cross_axpy`` (12 B/voxel: two reads, one write) as a rate and as a fraction of the copy ceiling, next to
``torch.permute(2, 1, 0).contiguous()`` on a tensor of the same size (8 B/voxel).

The ceiling is the best read+write figure of ``tools/micro/copy_patterns <n> <n>`` (hipcc -O3 --offload-arch=gfx950
tools/micro/copy_patterns.hip), run here as a child process in the same run when the program exists (``--copy-patterns``), else a
torch ``copy_`` probe.  Times are wall clock around ``reps`` calls that end in a synchronise of both engines, the best of three
rounds.  Needs a GPU: there is nothing to fall back to.  Writes profiles/dual_axis.md (``--out``)."""
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

from tomo_tv_amd._lib import VOL_RECON  # noqa: E402
from tomo_tv_amd.engine import tomoengine  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=512, help="the cube's edge")
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--copy-patterns", default=os.path.join(ROOT, "tools", "micro", "copy_patterns"))
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dual_axis.md"))
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_dual: no GPU")
dev = torch.device("cuda", 0)
n = a.n
nvox = n ** 3

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


x = torch.rand((n, n, n), device=dev, generator=torch.Generator(device=dev).manual_seed(1))
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


row("tomo_volume_cross (k_volume_cross<false>)", wall(lambda: ea.cross_volume_to(eb)), 8)
row("tomo_volume_cross_axpy, clamp (k_volume_cross<true>)", wall(lambda: ea.cross_axpy_volume_to(eb, 0.5, clamp=True)), 12)
row("both ways back to back (A -> B, B -> A), per call", wall(lambda: (ea.cross_volume_to(eb), eb.cross_volume_to(ea))) / 2, 8)
row("torch permute(2, 1, 0).contiguous()", wall(lambda: x.permute(2, 1, 0).contiguous()), 8)
row("torch copy_ of one volume", 8.0 * nvox / torch_copy / 1e9, 8)

lines = [f"# Dual-axis volume transpose on the MI355X: {n}^3", "",
         f"Copy ceiling {ceiling:.0f} GB/s: {ceiling_src}.  Wall clock around {a.reps} calls ending in a synchronise, best of three rounds.", "",
         "| call | ms | algorithmic B/voxel | GB/s | of the copy ceiling |", "|---|---|---|---|---|"]
for name, ms, bpv, rate, frac in rows:
    lines.append(f"| {name} | {ms:.3f} | {bpv} | {rate:.0f} | {100 * frac:.0f} % |")
if patterns:
    lines += ["", f"`copy_patterns {n} {n}` in the same run:", "", "| pattern | GB/s |", "|---|---|"] + [f"| {p} | {r:.0f} |" for p, r in patterns]
lines.append("")
os.makedirs(os.path.dirname(a.out), exist_ok=True)
with open(a.out, "w") as f:
    f.write("\n".join(lines))
print("\n".join(lines))
