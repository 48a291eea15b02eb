#!/usr/bin/env python3
"""Data in / out of an engine: the host path (numpy: ``pack_tilt_series`` + ``set_tilt_series``, ``get_recon``) against the device
path (torch tensors: ``set_tilt_series_tensor(SINO_PUBLIC)``, ``get_volume_tensor``), per step, with the bytes each moves over the
device's memory system and a plain device copy of the same bytes (torch ``copy_``, the probe of tools/micro/mall_write.py) beside it.

Host-path times are wall clock around calls that end in a stream synchronise; device-path times are wall clock around ``reps`` calls
followed by a synchronise of the engine's and torch's streams.  Needs a GPU: there is nothing to fall back to."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from tomo_tv_amd import pytvlib  # noqa: E402
from tomo_tv_amd._lib import SINO_B, SINO_PUBLIC, VOL_RECON  # noqa: E402
from tomo_tv_amd.engine import tomoengine  # noqa: E402
from tomo_tv_amd.phantom import tilt_angles  # noqa: E402

CONFIGS = {"512": (512, 512, 90), "1024x128": (128, 1024, 120)}          # (Nslice, Nray, Nangles)

ap = argparse.ArgumentParser()
ap.add_argument("--config", action="append", choices=sorted(CONFIGS), help="default: 512")
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--host-reps", type=int, default=3)
ap.add_argument("--out", default=None, help="write the figures as JSON here")
a = ap.parse_args()
dev = torch.device("cuda", 0)
results = []


def wall(fn, reps, sync):
    fn()
    sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    sync()
    return (time.perf_counter() - t0) / reps


for name in a.config or ["512"]:
    nx, n, P = CONFIGS[name]
    sx = (nx + 63) // 64 * 64
    t0 = time.perf_counter()
    t = tomoengine(nx, n, np.deg2rad(tilt_angles(P)), device=0)
    print(f"[{name}] Nslice {nx} Nray {n} Nangles {P}: engine created in {time.perf_counter() - t0:.1f} s", flush=True)
    rng = np.random.default_rng(1)
    ts = rng.random((nx, n, P), dtype=np.float32)
    ts_dev = torch.from_numpy(ts).to(dev)

    def sync():
        t.synchronize()
        torch.cuda.synchronize(dev)

    rows = []

    def row(step, path, seconds, device_bytes, note=""):
        r = {"config": name, "step": step, "path": path, "ms": seconds * 1e3, "device_GBps": device_bytes / seconds / 1e9 if device_bytes else None,
             "note": note}
        rows.append(r)
        rate = f"{r['device_GBps']:9.1f} GB/s" if device_bytes else " " * 14
        print(f"[{name}] {step:22s} {path:8s} {r['ms']:10.3f} ms {rate}  {note}", flush=True)

    def copy_probe(nbytes):
        src = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
        dst = torch.empty_like(src)
        return wall(lambda: dst.copy_(src), a.reps, lambda: torch.cuda.synchronize(dev))

    # ---- tilt series in -------------------------------------------------------------------------------------------------
    sino_dev_bytes = (nx + sx) * n * P * 4                                    # read [nx][m] float32, write [m][sx]
    row("tilt series in", "host", wall(lambda: t.set_tilt_series(pytvlib.pack_tilt_series(ts)), a.host_reps, sync), 0,
        "pack_tilt_series (numpy) + H2D into the staging buffer + k_transpose_in")
    packed = pytvlib.pack_tilt_series(ts)
    row("tilt series in", "host", wall(lambda: t.set_tilt_series(packed), a.host_reps, sync), 0, "set_tilt_series alone (already packed)")
    want = t._sino_local(SINO_B)
    row("tilt series in", "device", wall(lambda: t.set_tilt_series_tensor(ts_dev, SINO_PUBLIC), a.reps, sync), sino_dev_bytes,
        "k_io_in<float, PUBLIC>")
    assert np.array_equal(t._sino_local(SINO_B), want), "device path differs from the host path"
    row("tilt series in", "copy", copy_probe(sino_dev_bytes // 2), sino_dev_bytes // 2 * 2, "torch copy_ of as many bytes")

    # ---- reconstruction out ---------------------------------------------------------------------------------------------
    t.initialize_SIRT()
    t.SIRT(1)
    vol32 = (nx + sx) * n * n * 4
    vol64 = sx * n * n * 4 + nx * n * n * 8
    row("recon out", "host", wall(lambda: t.get_volume(VOL_RECON).astype(np.float64), a.host_reps, sync), 0,
        "get_recon: k_transpose_out + D2H + float64 copy on the host")
    row("recon out", "host", wall(lambda: t.get_volume(VOL_RECON), a.host_reps, sync), 0, "get_volume alone (float32)")
    ref = t.get_volume(VOL_RECON)
    out32 = torch.empty((nx, n, n), dtype=torch.float32, device=dev)
    row("recon out float32", "device", wall(lambda: t.get_volume_tensor(VOL_RECON, out=out32), a.reps, sync), vol32, "k_io_out<float>")
    assert np.array_equal(out32.cpu().numpy(), ref)
    out64 = torch.empty((nx, n, n), dtype=torch.float64, device=dev)
    row("recon out float64", "device", wall(lambda: t.get_volume_tensor(VOL_RECON, out=out64), a.reps, sync), vol64, "k_io_out<double>")
    assert np.array_equal(out64.cpu().numpy(), ref.astype(np.float64))
    del out64
    row("recon out float32", "copy", copy_probe(vol32 // 2), vol32 // 2 * 2, "torch copy_ of as many bytes")
    row("volume in float32", "device", wall(lambda: t.set_volume_tensor(out32, VOL_RECON), a.reps, sync), vol32, "k_io_in<float>")
    assert np.array_equal(t.get_volume(VOL_RECON), ref)
    results += rows
    del t, ts_dev, out32
    torch.cuda.empty_cache()

if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"tool": "tools/bench_io.py", "device": torch.cuda.get_device_name(0), "reps": a.reps, "host_reps": a.host_reps,
                   "rows": results}, f, indent=1)
