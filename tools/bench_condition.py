#!/usr/bin/env python3
"""The conditioning calls at 512 x 512 x 90 and 1024 x 1024 x 120 (slices x rays x projections) against the copy ceiling measured in the
same process: ``tomo_sino_median`` (radius 1 and 2, measuring and replacing), ``tomo_sino_intensity`` and ``tomo_sino_window_stats``
(the whole image), beside
  * a copy of the same slot, as ``tomo_sino_intensity`` with gain 1 and as a plain ``hipMemcpyDtoD``: 8 bytes per sample, the ceiling
    of any pass that reads a series and writes one;
  * the same median written with torch (replicate padding, ``unfold`` twice, ``median`` over the window) on the device tensor: what a
    user would write.
Every call is warmed up, then timed as wall clock around ``reps`` calls that end in a device synchronise, five rounds: the table gives
the median round and the range.  The median and the statistics wait for their sums in every call (one stream wait and the second
reduction stage are inside their time).  Needs a GPU: there is nothing to fall back to.  Writes profiles/sino_condition.md (``--out``)."""
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
from tomo_tv_amd.engine import tomoengine  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="512x512x90,1024x1024x120", help="comma-separated Nslice x Nray x Nproj")
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sino_condition.md"))
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_condition: no GPU")
dev = torch.device("cuda", 0)
hip = ctypes.CDLL("libamdhip64.so")
hip.hipMemcpyDtoD.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
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


def torch_median(x, R):
    """x[P][N][ns] -> the (2R+1)^2 median with a replicated border"""
    W = 2 * R + 1
    p = torch.nn.functional.pad(x[:, None], (R, R, R, R), mode="replicate")[:, 0]
    return p.unfold(1, W, 1).unfold(2, W, 1).reshape(*x.shape, W * W).median(-1).values


lines = ["# The conditioning calls on the MI355X against the copy ceiling of the same run", "",
         f"Wall clock around {a.reps} calls ending in a device synchronise, {a.rounds} rounds: the median round, with the range.  `bytes` is the",
         "least traffic of the call with the padded row pitch included (8 per sample for a pass that reads a series and writes one, 4 for one",
         "that only reads).  `of ceiling` is the time an 8-byte-per-sample copy takes for the call's bytes -- `tomo_sino_intensity` with gain 1,",
         "offset 0 of the same run, scaled by bytes -- over the call's time: 1.00 is the speed of that copy.  The median and the statistics",
         "wait for their sums inside every call.", ""]
for size in a.sizes.split(","):
    ns, n, P = (int(v) for v in size.split("x"))
    eng = tomoengine(ns, n, np.deg2rad(np.linspace(-70, 70, P)), device=0)
    L, h = _lib.load(), eng.be.h

    def sync():
        eng.synchronize()
        torch.cuda.synchronize(dev)

    gen = torch.Generator(device=dev).manual_seed(1)
    x = torch.rand((ns, n * P), device=dev, generator=gen) + 0.5
    for slot in (SRC, DST):
        eng.be.set_tilt_series_tensor(x, SINO_PACKED, slot)
    sync()
    sx = -(-ns // 64) * 64
    samples = n * P * sx
    out = np.empty((P, 5), np.float64)
    po = out.ctypes.data_as(ctypes.c_void_p)
    th = np.full(P, 0.25, np.float32)
    pt = th.ctypes.data_as(ctypes.c_void_p)
    unit = np.tile(np.array([1.0, 0.0], np.float32), (P, 1))
    go = np.tile(np.array([1.25, -0.5], np.float32), (P, 1))
    pu, pg = unit.ctypes.data_as(ctypes.c_void_p), go.ctypes.data_as(ctypes.c_void_p)
    c = _lib.check
    raw_a = torch.empty(samples, dtype=torch.float32, device=dev).normal_()
    raw_b = torch.empty_like(raw_a)

    def dtod():
        assert hip.hipMemcpyDtoD(raw_b.data_ptr(), raw_a.data_ptr(), 4 * samples) == 0

    rows = [("copy: tomo_sino_intensity, gain 1, offset 0", 8, lambda: c(L.tomo_sino_intensity(h, SRC, DST, pu, 0))),
            ("copy: hipMemcpyDtoD", 8, dtod),
            ("tomo_sino_intensity, clamp", 8, lambda: c(L.tomo_sino_intensity(h, SRC, DST, pg, 1))),
            ("tomo_sino_intensity, in place", 8, lambda: c(L.tomo_sino_intensity(h, DST, DST, pu, 0))),
            ("tomo_sino_window_stats, whole image", 4, lambda: c(L.tomo_sino_window_stats(h, SRC, 0, n, 0, ns, po))),
            ("tomo_sino_median, radius 1, measuring", 4, lambda: c(L.tomo_sino_median(h, SRC, -1, 1, None, po))),
            ("tomo_sino_median, radius 1, replacing", 8, lambda: c(L.tomo_sino_median(h, SRC, DST, 1, pt, po))),
            ("tomo_sino_median, radius 2, measuring", 4, lambda: c(L.tomo_sino_median(h, SRC, -1, 2, None, po))),
            ("tomo_sino_median, radius 2, replacing", 8, lambda: c(L.tomo_sino_median(h, SRC, DST, 2, pt, po)))]
    img = torch.rand((P, n, ns), device=dev, generator=gen)
    torch_rows = [(f"torch: pad, unfold, median, radius {R}", 8, (lambda R=R: torch_median(img, R))) for R in (1, 2)]
    lines += [f"## {ns} slices x {n} rays x {P} projections (pitch {sx}: {samples / 1e6:.1f} M samples per series)", "",
              "| call | bytes, MB | time, ms (range) | GB/s | of ceiling |", "|---|---|---|---|---|"]
    per_byte = None
    for name, bps, fn in rows + torch_rows:
        is_torch = name.startswith("torch")
        if is_torch:                                    # the torch median moves ns real slices, not the pitch
            nbytes, reps = bps * n * P * ns, max(1, a.reps // 10)
        else:
            nbytes, reps = bps * samples, a.reps
        med, lo, hi = measure(fn, sync, reps)
        if per_byte is None:
            per_byte = med / nbytes                     # the first row is the ceiling
        lines.append(f"| {name} | {nbytes / 1e6:.1f} | {med * 1e3:.3f} ({lo * 1e3:.3f} .. {hi * 1e3:.3f}) | {nbytes / med / 1e9:.0f} | "
                     f"{per_byte * nbytes / med:.2f} |")
        print(lines[-1], flush=True)
    lines.append("")
    del eng, x, raw_a, raw_b, img
    torch.cuda.empty_cache()
lines += ["Not measured here: hardware counters of any of these kernels (instruction issue, cache hit rates), and the stand-alone copy",
          "ceiling of tools/micro/copy_patterns.hip; the copy rows are the yardstick of THIS run, on this device, at these sizes.", ""]
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    f.write("\n".join(lines))
print("\n".join(lines))
