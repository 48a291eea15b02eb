"""Run by test_gpu_dual.py in a child process: an engine bound to a one-rank RCCL communicator (tomo_comm_unique_id / tomo_comm_init, as a
C host would) is refused by tomo_volume_cross and tomo_volume_cross_axpy with TOMO_ERR_STATE, as the source and as the destination,
nothing is written, and both calls work again once the communicator is gone."""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ref64_dual as D  # noqa: E402
from tomo_tv_amd import _lib  # noqa: E402
from tomo_tv_amd.engine import tomoengine  # noqa: E402

V0, V1, STATE, N = 5, 6, 3, 8
L = _lib.load()
a = tomoengine(N, N, np.deg2rad(np.linspace(-60, 60, 2)))
b = tomoengine(N, N, np.deg2rad(np.linspace(-50, 40, 3)))
x = np.random.default_rng(2).uniform(-1, 1, (N, N, N)).astype(np.float32)
a.set_volume(x, V0)
b.set_volume(x, V1)
idbuf = (ctypes.c_ubyte * 128)()
_lib.check(L.tomo_comm_unique_id(idbuf))
_lib.check(L.tomo_comm_init(b.be.h, idbuf, 1, 0))
for src, sv, dst, dv in ((a.be.h, V0, b.be.h, V1), (b.be.h, V1, a.be.h, V0)):
    assert L.tomo_volume_cross(src, sv, dst, dv) == STATE and b"communicator" in L.tomo_last_error()
    assert L.tomo_volume_cross_axpy(src, sv, dst, dv, 0.5, 0) == STATE and b"communicator" in L.tomo_last_error()
assert np.array_equal(a.get_volume(V0).view(np.uint32), x.view(np.uint32))   # nothing was written
assert np.array_equal(b.get_volume(V1).view(np.uint32), x.view(np.uint32))
_lib.check(L.tomo_comm_destroy(b.be.h))
a.cross_volume_to(b, src=V0, dst=V1)
assert np.array_equal(b.get_volume(V1).view(np.uint32), D.cross(x).view(np.uint32))
print("DUAL_COMM_REFUSED_OK")
