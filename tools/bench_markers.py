#!/usr/bin/env python3
"""The marker-detection calls at 512 x 512 x 90 and 1024 x 1024 x 120 (slices x rays x projections) against the copy ceiling measured
in the same process: ``tomo_sino_template_ncc`` at template radius 2, 4 and 8 and ``tomo_sino_peaks`` on its result, beside
  * a copy of the same slot as ``tomo_sino_intensity`` with gain 1 and offset 0: 8 bytes per sample, the ceiling of any pass that
    reads a series and writes one;
  * the same correlation written with torch (``conv2d`` for the window sums, the sums of squares and the template product): what a
    user would write -- the cancelling form, whose accuracy the kernel does not share.
Every call is warmed up, then timed as wall clock around ``reps`` calls that end in a device synchronise, five rounds: the table gives
the median round and the range.  ``tomo_sino_peaks`` waits for its counts in every call (a clear, the kernel, two read-backs and the
host sort are inside its time).  Needs a GPU: there is nothing to fall back to.  Writes profiles/markers.md (``--out``)."""
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
from tomo_tv_amd._lib import SINO_PACKED, SINO_USER0  # noqa: E402
from tomo_tv_amd.engine import tomoengine  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="512x512x90,1024x1024x120", help="comma-separated Nslice x Nray x Nproj")
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "markers.md"))
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_markers: no GPU")
dev = torch.device("cuda", 0)
SRC, DST = SINO_USER0, SINO_USER0 + 1


def measure(fn, sync, reps):
    """-> (median, min, max) seconds per call over the rounds"""
    fn()
    sync()
    t = []
    for _ in range(a.rounds):
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        sync()
        t.append((time.perf_counter() - t0) / reps)
    return float(np.median(t)), min(t), max(t)


def torch_ncc(x, t):
    """x[P][N][ns], t the prepared template (zero mean, unit norm) -> the valid part of the correlation, by window sums"""
    W = t.shape[0]
    ones = torch.ones((1, 1, W, W), device=x.device)
    s1 = torch.nn.functional.conv2d(x[:, None], ones)
    s2 = torch.nn.functional.conv2d(x[:, None] * x[:, None], ones)
    c = torch.nn.functional.conv2d(x[:, None], t[None, None])
    v = s2 - s1 * s1 / (W * W)
    return torch.where(v > 0, c / torch.sqrt(v.clamp_min(1e-30)), torch.zeros_like(c))


lines = ["# The marker-detection calls on the MI355X against the copy ceiling of the same run", "",
         f"Wall clock around {a.reps} calls ending in a device synchronise, {a.rounds} rounds: the median round, with the range.  `bytes` is the",
         "least traffic of the call with the padded row pitch included (8 per sample for a pass that reads a series and writes one, 4 for one",
         "that only reads).  `of ceiling` is the time an 8-byte-per-sample copy takes for the call's bytes -- `tomo_sino_intensity` with gain 1,",
         "offset 0 of the same run, scaled by bytes -- over the call's time: 1.00 is the speed of that copy.  The series: uniform noise with",
         "one bright disc of radius 2 per 64 x 64 samples; the peaks are taken at threshold 0.5 with the template's radius.", ""]
for size in a.sizes.split(","):
    ns, n, P = (int(v) for v in size.split("x"))
    eng = tomoengine(ns, n, np.deg2rad(np.linspace(-70, 70, P)), device=0)
    L, h = _lib.load(), eng.be.h

    def sync():
        eng.synchronize()
        torch.cuda.synchronize(dev)

    gen = torch.Generator(device=dev).manual_seed(1)
    img = torch.rand((P, n, ns), device=dev, generator=gen) * 0.25
    r, s = torch.meshgrid(torch.arange(n, device=dev), torch.arange(ns, device=dev), indexing="ij")
    img += ((((r % 64) - 31.5) ** 2 + ((s % 64) - 31.5) ** 2) <= 4.0).float()[None]
    x = img.permute(2, 0, 1).reshape(ns, P * n).contiguous()                  # [s][angle][ray]: the packed host layout
    eng.be.set_tilt_series_tensor(x, SINO_PACKED, SRC)
    sync()
    sx = -(-ns // 64) * 64
    samples = n * P * sx
    unit = np.tile(np.array([1.0, 0.0], np.float32), (P, 1))
    pu = unit.ctypes.data_as(ctypes.c_void_p)
    c = _lib.check
    rows = [("copy: tomo_sino_intensity, gain 1, offset 0", 8, lambda: c(L.tomo_sino_intensity(h, SRC, DST, pu, 0)))]
    count = np.zeros(P, np.int32)
    cap = 4 * (-(-n // 64)) * (-(-ns // 64))
    rec = np.zeros((P, cap, 8), np.int32)
    pc, pr = count.ctypes.data_as(ctypes.c_void_p), rec.ctypes.data_as(ctypes.c_void_p)
    for R in (2, 4, 8):
        T = np.ascontiguousarray(align.marker_template(2.0, R), np.float32)
        pt = T.ctypes.data_as(ctypes.c_void_p)
        rows.append((f"tomo_sino_template_ncc, R = {R}", 8, lambda pt=pt, R=R, T=T: c(L.tomo_sino_template_ncc(h, SRC, DST, pt, R, 1e-6))))
        rows.append((f"tomo_sino_peaks of it, radius {R}", 4, lambda R=R: c(L.tomo_sino_peaks(h, DST, R, 0.5, cap, pc, pr))))
    torch_rows = []
    for R in (2, 4, 8):
        T = align.marker_template(2.0, R)
        t = T - T.mean()
        t = torch.tensor(t / np.sqrt((t * t).sum()), dtype=torch.float32, device=dev)
        torch_rows.append((f"torch: conv2d NCC (sumsq - sum^2 / W), R = {R}", 8, lambda t=t: torch_ncc(img, t)))
    lines += [f"## {ns} slices x {n} rays x {P} projections (pitch {sx}: {samples / 1e6:.1f} M samples per series)", "",
              "| call | bytes, MB | time, ms (range) | GB/s | of ceiling |", "|---|---|---|---|---|"]
    per_byte = None
    for name, bps, fn in rows + torch_rows:
        is_torch = name.startswith("torch")
        nbytes, reps = (bps * n * P * ns, max(1, a.reps // 10)) if is_torch else (bps * samples, a.reps)
        med, lo, hi = measure(fn, sync, reps)
        if per_byte is None:
            per_byte = med / nbytes                     # the first row is the ceiling
        lines.append(f"| {name} | {nbytes / 1e6:.1f} | {med * 1e3:.3f} ({lo * 1e3:.3f} .. {hi * 1e3:.3f}) | {nbytes / med / 1e9:.0f} | "
                     f"{per_byte * nbytes / med:.2f} |")
        print(lines[-1], flush=True)
    lines += ["", f"peaks found per projection at the last radius: {int(count.min())} .. {int(count.max())} (capacity {cap})", ""]
    del eng, x, img
    torch.cuda.empty_cache()
lines += ["Not measured here: hardware counters of these kernels (LDS and instruction issue, cache hit rates); the copy row is the",
          "yardstick of THIS run, on this device, at these sizes.", ""]
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    f.write("\n".join(lines))
print("\n".join(lines))
