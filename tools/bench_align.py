#!/usr/bin/env python3
"""Alignment kernels at 512 x 512 x 90: ``sino_xcorr`` for S = 8 and S = 16 and ``sino_shift``, against a torch baseline on the same
device (FFT cross-correlation of the mean-subtracted, zero-padded images, cropped to the window) and against the correlation's
LDS / VALU bound.

Every figure is the median of ``--reps`` timed calls after ``--warmup`` untimed ones, with the spread (min, max, interquartile
range) beside it.  The engine calls end in a stream synchronise and a read-back of the window (Nangles (2S+1)^2 doubles), so they
are timed by wall clock around the call -- the time a caller sees; the torch baseline is timed the same way, read-back of its
window included.  Writes ``profiles/align_xcorr.md`` (``--out``).  The figures are whole calls (moment passes, finalize and read-back
included); the kernels alone come from a second run of this tool under ``rocprofv3 --kernel-trace --stats`` (``--reps 30 --out``
somewhere else), whose ``k_sino_*`` rows are added to the profile as its last section.  ``--affine`` times ``sino_affine`` (3 degrees)
and ``sino_axis_profile`` instead, beside ``sino_shift`` on the same tensors and torch ``grid_sample``, and writes
``profiles/align_affine.md``.  Needs a GPU: there is nothing to fall back to."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from tomo_tv_amd._lib import SINO_B, SINO_PUBLIC, SINO_USER0  # noqa: E402
from tomo_tv_amd.engine import tomoengine  # noqa: E402
from tomo_tv_amd.phantom import tilt_angles  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--shape", type=int, nargs=3, default=[512, 512, 90], metavar=("NSLICE", "NRAY", "NANGLES"))
ap.add_argument("--reps", type=int, default=300, help="timed calls per figure (300 calls of 1-2 ms: 0.3-0.7 s of timed work)")
ap.add_argument("--warmup", type=int, default=20)
ap.add_argument("--affine", action="store_true", help="time sino_affine (3 degrees) and sino_axis_profile beside sino_shift and a torch "
                "grid_sample baseline instead, and write profiles/align_affine.md")
ap.add_argument("--out", default=None, help="default: profiles/align_xcorr.md, with --affine profiles/align_affine.md")
a = ap.parse_args()
if a.out is None:
    a.out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "align_affine.md" if a.affine else "align_xcorr.md")
ns, n, P = a.shape
dev = torch.device("cuda", 0)

# the MI355X figures the bound is computed from (LDS 128 B/clk/CU for 4-byte reads, 256 CUs, ~2.4 GHz; one 64-lane FMA per SIMD
# every 2 clocks... taken as 4 SIMDs x 32 lanes per clock)
CUS, CLK, LDS_B32_PER_CLK, FMA_LANES_PER_CLK = 256, 2.4e9, 32, 128
TILES = {8: (8, 9, 9), 16: (16, 11, 11)}          # S -> (S_MAX, TU, TV) of the launcher


def bound_ms(S):
    smax, tu, tv = TILES[S]
    w = 2 * smax + 1
    up, vp = -(-w // tu) * tu, -(-w // tv) * tv
    rows, lanes = P * n, -(-ns // 64) * 64
    fma = rows * lanes * up * vp                                   # lane-FMAs issued (padded window)
    reads = rows * lanes * (up // tu) * (vp // tv) * (tu + tv)     # 4-byte LDS reads per lane
    return fma / (CUS * FMA_LANES_PER_CLK * CLK) * 1e3, reads / (CUS * LDS_B32_PER_CLK * CLK) * 1e3, fma


def timed(fn):
    for _ in range(a.warmup):
        fn()
    t = []
    for _ in range(a.reps):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(dev)
        t.append((time.perf_counter() - t0) * 1e3)
    t = np.sort(np.array(t))
    return dict(median=float(np.median(t)), min=float(t[0]), max=float(t[-1]), iqr=float(np.percentile(t, 75) - np.percentile(t, 25)))


def fmt(r):
    return f"{r['median']:.3f} ms (min {r['min']:.3f}, max {r['max']:.3f}, IQR {r['iqr']:.3f})"


eng = tomoengine(ns, n, np.deg2rad(tilt_angles(P)), device=0)
rng = np.random.default_rng(1)
ta = torch.from_numpy(rng.random((ns, n, P), dtype=np.float32)).to(dev)
tb = torch.roll(ta, shifts=(3, -2), dims=(0, 1)) + 0.01 * torch.from_numpy(rng.random((ns, n, P), dtype=np.float32)).to(dev)
eng.be.set_tilt_series_tensor(ta, SINO_PUBLIC, SINO_B)
eng.be.set_tilt_series_tensor(tb, SINO_PUBLIC, SINO_USER0)
A = ta.permute(2, 1, 0).contiguous()             # [a][r][s]
B = tb.permute(2, 1, 0).contiguous()


def torch_xcorr(S):
    """FFT correlation of the mean-subtracted images zero-padded to (N + S, Nslice + S), cropped to the window, read back"""
    a0, b0 = A - A.mean((1, 2), keepdim=True), B - B.mean((1, 2), keepdim=True)
    shape = (n + S, ns + S)
    F = torch.fft.irfft2(torch.conj(torch.fft.rfft2(a0, s=shape)) * torch.fft.rfft2(b0, s=shape), s=shape)
    idx_u = torch.arange(-S, S + 1, device=dev) % shape[0]
    idx_v = torch.arange(-S, S + 1, device=dev) % shape[1]
    return F[:, idx_u][:, :, idx_v].double().cpu().numpy()


def bench_affine():
    """``sino_affine`` at 3 degrees and ``sino_axis_profile`` beside ``sino_shift`` with fractional shifts (the same bytes: one read and
    one write of the sinogram) and torch ``grid_sample`` (bilinear, zeros outside, align_corners) on the same images"""
    import torch.nn.functional as Fn
    from tomo_tv_amd.align import affine_matrices
    pitch = -(-ns // 64) * 64
    nbytes = 2 * P * n * pitch * 4
    sh = rng.uniform(-8, 8, (P, 2)).astype(np.float32)
    M = affine_matrices(sh, 3.0, 1.0, n, ns)
    dst = SINO_USER0 + 1
    k_aff = timed(lambda: eng.sino_affine(SINO_B, dst, M))
    got = eng.get_projections_tensor(dst, SINO_PUBLIC).permute(2, 1, 0).contiguous()          # [a][r][s]
    M_id = affine_matrices(np.zeros((P, 2)), 0.0, 1.0, n, ns)
    k_id = timed(lambda: eng.sino_affine(SINO_B, dst, M_id))
    k_sh = timed(lambda: eng.sino_shift(SINO_B, dst, sh))
    k_pr = timed(lambda: eng.sino_axis_profile(SINO_B))
    # grid_sample: x indexes the last axis (s), y the one before (r), normalised to [-1, 1] with align_corners=True
    Mt = torch.from_numpy(M).to(dev)
    r, s = torch.meshgrid(torch.arange(n, device=dev, dtype=torch.float64), torch.arange(ns, device=dev, dtype=torch.float64), indexing="ij")
    rp = Mt[:, 0, None, None] * r + Mt[:, 1, None, None] * s + Mt[:, 2, None, None]
    sp = Mt[:, 3, None, None] * r + Mt[:, 4, None, None] * s + Mt[:, 5, None, None]
    grid = torch.stack([2 * sp / (ns - 1) - 1, 2 * rp / (n - 1) - 1], dim=-1).float()

    def torch_affine():
        out = Fn.grid_sample(A[:, None], grid, mode="bilinear", padding_mode="zeros", align_corners=True)
        return out

    agree = float((torch_affine()[:, 0] - got).abs().max() / got.abs().max())
    t_gs = timed(torch_affine)
    ratio = k_aff["median"] / k_sh["median"]
    out = ["# Alignment kernels: `sino_affine` and `sino_axis_profile`", "",
           f"`tools/bench_align.py --affine`, {torch.cuda.get_device_name(0)}, (Nslice, Nray, Nangles) = ({ns}, {n}, {P}); median of {a.reps} "
           f"calls after {a.warmup} warm-up calls, wall clock around a call that ends in a stream synchronise (whole calls: table upload, "
           "kernel, synchronise; the profile also its finalize and the read-back of Nangles x Nslice doubles).", "",
           f"* `sino_affine`, rotation 3 degrees with fractional shifts: {fmt(k_aff)}: {nbytes / k_aff['median'] / 1e6:.0f} GB/s of its algorithmic "
           f"bytes (one read, one write of the sinogram: {nbytes / 1e6:.0f} MB)",
           f"* `sino_affine`, identity (every element takes the copy path): {fmt(k_id)}",
           f"* `sino_shift`, the same fractional shifts, the same tensors: {fmt(k_sh)}: {nbytes / k_sh['median'] / 1e6:.0f} GB/s",
           f"* affine / shift = {ratio:.2f}.  Both move the same bytes; the affine pass adds per element four binary64 FMAs, two floors, two "
           "conversions and per-lane (not per-angle) weights and branch conditions, and its source rows are not the destination's: at 3 "
           f"degrees a 64-slice wave reads from about {1 + int(np.ceil(64 * np.sin(np.deg2rad(3.0))))} source rows per tap row.  Which of the "
           "two carries the difference is NOT MEASURED (no counter run)",
           f"* torch `grid_sample` (bilinear, zeros outside, binary32 coordinates precomputed outside the timed call): {fmt(t_gs)}; largest "
           f"difference to the kernel {agree:.2e} of the largest sample; grid_sample / affine = {t_gs['median'] / k_aff['median']:.2f}",
           f"* `sino_axis_profile`: {fmt(k_pr)}: {nbytes / 2 / k_pr['median'] / 1e6:.0f} GB/s of one read of the sinogram ({nbytes / 2e6:.0f} MB)",
           "", "The kernels alone (under `rocprofv3 --kernel-trace --stats`): NOT MEASURED.", ""]
    print("\n".join(out), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(out))


if a.affine:
    bench_affine()
    sys.exit(0)

lines = ["# Alignment kernels: `sino_xcorr` and `sino_shift`", "",
         f"`tools/bench_align.py`, {torch.cuda.get_device_name(0)}, (Nslice, Nray, Nangles) = ({ns}, {n}, {P}); median of {a.reps} calls after "
         f"{a.warmup} warm-up calls, wall clock around a call that ends in a stream synchronise and the read-back of the window.", ""]
for S in (8, 16):
    C = eng.sino_xcorr(SINO_B, SINO_USER0, S)
    T = torch_xcorr(S)
    agree = float(np.max(np.abs(C - T)) / np.max(np.abs(C)))
    k = timed(lambda: eng.sino_xcorr(SINO_B, SINO_USER0, S))
    t = timed(lambda: torch_xcorr(S))
    k0 = timed(lambda: eng.sino_xcorr(SINO_B, SINO_USER0, S, subtract_mean=False))
    valu, lds, fma = bound_ms(S)
    bound = max(valu, lds)
    ratio = t["median"] / k["median"]
    lines += [f"## S = {S}", "",
              f"* `sino_xcorr` (means, correlation, finalize, read-back): {fmt(k)}",
              f"* the same without the two moment passes (`subtract_mean=False`: correlation, finalize, read-back): {fmt(k0)}",
              f"* torch FFT baseline: {fmt(t)}; largest difference of the two windows {agree:.2e} of the peak",
              f"* torch / kernel = {ratio:.2f} -- the kernel is {'faster' if ratio > 1 else 'SLOWER than the torch baseline'}",
              f"* bound: VALU {valu:.3f} ms ({fma / 1e9:.1f} G lane-FMAs), LDS {lds:.3f} ms -> {bound:.3f} ms; the call reaches "
              f"{100 * bound / k['median']:.0f} % of it ({2 * fma / k['median'] / 1e9:.1f} TFLOP/s), without the moment passes "
              f"{100 * bound / k0['median']:.0f} %.  These are whole calls; the kernels alone are in the last section", ""]
    print("\n".join(lines[-7:]), flush=True)
m = timed(lambda: eng.sino_moments(SINO_B))
lines += ["## `sino_moments`", "", f"* {fmt(m)} (one moment pass, its finalize and the read-back of Nangles x 3 doubles)", ""]
print("\n".join(lines[-2:]), flush=True)
sh = rng.uniform(-8, 8, (P, 2)).astype(np.float32)
r = timed(lambda: eng.sino_shift(SINO_B, SINO_USER0 + 1, sh))
nbytes = 2 * P * n * (-(-ns // 64) * 64) * 4
lines += ["## `sino_shift` (bilinear, fractional shifts, no wrap)", "",
          f"* {fmt(r)}: {nbytes / r['median'] / 1e6:.0f} GB/s of its algorithmic bytes (one read, one write of the sinogram: {nbytes / 1e6:.0f} MB)", ""]
print("\n".join(lines[-3:]), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    f.write("\n".join(lines))
