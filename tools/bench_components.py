#!/usr/bin/env python3
"""Connected components at 512^3 and 1024 x 512^2 (``--shapes``): label, stats and keep on a sparse-particle phantom (a few hundred
spheres, 26-connectivity) and on uniform noise thresholded near the site-percolation densities (0.31 with 6 neighbours, 0.10 with
26), each as a time, as bytes of the label array moved once (4 B/voxel) per second against the copy ceiling, and against the host
route of before (``get_volume`` + ``scipy.ndimage.label``, where scipy is installed; run once).

The copy ceiling is measured in the same run: the best pattern of tools/micro/copy_patterns (built with hipcc beside its source),
started as a child process before this one opens the device; without that binary, a torch ``copy_`` of one volume.
Times are wall clock around ``reps`` calls that end in a stream synchronise (label and stats wait by themselves).
Needs a GPU: there is nothing to fall back to.  Writes profiles/components.md (``--out``)."""
import argparse
import ctypes
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="512x512,1024x512", help="Nslice x N, comma separated")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--spheres", type=int, default=300)
ap.add_argument("--no-host", action="store_true", help="skip the host route")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "components.md"))
a = ap.parse_args()

ceiling, ceiling_src = None, ""
exe = os.path.join(ROOT, "tools", "micro", "copy_patterns")
if os.path.exists(exe):
    p = subprocess.run([exe, "512", "512"], capture_output=True, text=True, timeout=300)
    rates = [float(m) for m in re.findall(r"(\d+) GB/s", p.stdout)]
    if p.returncode == 0 and rates:
        ceiling, ceiling_src = max(rates), "the best pattern of tools/micro/copy_patterns (in-place read + write of a 512^3 volume), run first"

import torch  # noqa: E402

from tomo_tv_amd._lib import VOL_RECON, VOL_USER0  # noqa: E402
from tomo_tv_amd.engine import tomoengine  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("bench_components: no GPU")
dev = torch.device("cuda", 0)
try:
    import scipy.ndimage as ndi
except ImportError:
    ndi = None


def wall(fn, sync, reps):
    fn()
    sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    sync()
    return (time.perf_counter() - t0) / reps


if ceiling is None:
    src, dst = torch.empty(512 ** 3, device=dev), torch.empty(512 ** 3, device=dev)
    ceiling = 8.0 * 512 ** 3 / wall(lambda: dst.copy_(src), lambda: torch.cuda.synchronize(dev), 10) / 1e9
    ceiling_src = "torch copy_ of a 512^3 volume, read + write (run here: tools/micro/copy_patterns was not built)"
    del src, dst


def spheres(ns, n, count):
    gen = torch.Generator(device="cpu").manual_seed(3)
    x = torch.zeros((ns, n, n), device=dev)
    for _ in range(count):
        r = int(torch.randint(3, 11, (1,), generator=gen))
        c = [int(torch.randint(r, m - r, (1,), generator=gen)) for m in (ns, n, n)]
        ax = [torch.arange(-r, r + 1, device=dev, dtype=torch.float32)] * 3
        ball = (ax[0][:, None, None] ** 2 + ax[1][None, :, None] ** 2 + ax[2][None, None, :] ** 2 <= r * r).float()
        v = x[c[0] - r:c[0] + r + 1, c[1] - r:c[1] + r + 1, c[2] - r:c[2] + r + 1]
        torch.maximum(v, ball, out=v)
    return x


lines = ["# Connected components on the MI355X", "",
         f"Copy ceiling {ceiling:.0f} GB/s: {ceiling_src}.  Wall clock around {a.reps} calls ending in a synchronise; the rate counts the",
         "label array once (4 B/voxel), so `of ceiling` = (the time a copy of the labels would take) / (the time taken).", ""]
for shape in a.shapes.split(","):
    ns, n = (int(v) for v in shape.split("x"))
    nvox = ns * n * n
    t = tomoengine(ns, n, np.deg2rad([0.0, 30.0]), device=0)
    sync = t.synchronize
    gen = torch.Generator(device=dev).manual_seed(1)
    noise = torch.rand((ns, n, n), device=dev, generator=gen)
    cases = [("spheres", spheres(ns, n, a.spheres), 26), ("noise 0.31", (noise < 0.31).float(), 6), ("noise 0.10", (noise < 0.10).float(), 26)]
    del noise
    lines += [f"## Nslice {ns}, N {n} ({nvox / 2 ** 20:.0f} Mi voxels)", "",
              "| volume | connectivity | K | call | ms | GB/s (labels once) | of ceiling | host route s | speed-up |", "|---|---|---|---|---|---|---|---|---|"]
    for name, x, conn in cases:
        t.set_volume_tensor(x, VOL_RECON)
        K = t.label_components(VOL_RECON, 0.5, 1.5, conn)
        host = None
        if ndi is not None and not a.no_host:
            t0 = time.perf_counter()
            lab, Kh = ndi.label(t.get_volume(VOL_RECON) >= 0.5, structure=ndi.generate_binary_structure(3, 1 if conn == 6 else 3))
            host = time.perf_counter() - t0
            assert Kh == K, (Kh, K)
            del lab
        t_label = wall(lambda: t.label_components(VOL_RECON, 0.5, 1.5, conn), sync, a.reps)

        def stats():
            t.be.c("components_label", VOL_RECON, 0.5, 1.5, conn, kref)          # the measurements are cached per labelling
            return t.component_stats()
        kref = ctypes.byref(ctypes.c_int64(0))
        t._n_components = K
        t_stats = wall(stats, sync, a.reps) - t_label
        keep = np.ones(K + 1, bool)
        keep[1::2] = False
        t.be.c("copy_volume", VOL_USER0, VOL_RECON)
        t.label_components(VOL_USER0, 0.5, 1.5, conn)
        t_keep = wall(lambda: t.keep_components(VOL_USER0, keep, 0.0), sync, a.reps)
        for call, sec in (("label", t_label), ("stats", t_stats), ("keep", t_keep)):
            rate = 4.0 * nvox / sec / 1e9
            hs = f"{host:.2f}" if host is not None and call == "label" else ""
            sp = f"{host / sec:.0f} x" if host is not None and call == "label" else ""
            lines.append(f"| {name} | {conn} | {K} | {call} | {sec * 1e3:.2f} | {rate:.0f} | {100 * rate / ceiling:.1f} % | {hs} | {sp} |")
            print(lines[-1], flush=True)
        del x
    lines.append("")
    t.release_components()
    t.be.close()
    del t, cases
    torch.cuda.empty_cache()
if ndi is None:
    lines += ["scipy is not installed here: the host route was not timed.", ""]
os.makedirs(os.path.dirname(a.out), exist_ok=True)
with open(a.out, "w") as f:
    f.write("\n".join(lines))
print("\n".join(lines))
