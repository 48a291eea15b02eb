"""Run by test_gpu_affine3d.py in a child process: an engine bound to a one-rank RCCL communicator (tomo_comm_unique_id / tomo_comm_init,
as a C host would) is refused by tomo_volume_affine and tomo_volume_affine_axpy with TOMO_ERR_STATE, as the source, as the destination
and as both, nothing is written, and both calls work again once the communicator is gone."""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tomo_tv_amd import _lib  # noqa: E402
from tomo_tv_amd.engine import tomoengine  # noqa: E402

V0, V1, STATE, N = 5, 6, 3, 8
L = _lib.load()
a = tomoengine(N, N, np.deg2rad(np.linspace(-60, 60, 2)))
b = tomoengine(N + 2, N, np.deg2rad(np.linspace(-50, 40, 3)))
x, w = (np.random.default_rng(k).uniform(-1, 1, (n, N, N)).astype(np.float32) for k, n in ((2, N), (3, N + 2)))
a.set_volume(x, V0)
b.set_volume(w, V1)
ident = np.eye(3, 4).ravel()
m = ident.ctypes.data_as(ctypes.c_void_p)
idbuf = (ctypes.c_ubyte * 128)()
_lib.check(L.tomo_comm_unique_id(idbuf))
_lib.check(L.tomo_comm_init(b.be.h, idbuf, 1, 0))
for src, sv, dst, dv in ((a.be.h, V0, b.be.h, V1), (b.be.h, V1, a.be.h, V0), (b.be.h, V1, b.be.h, V0)):
    assert L.tomo_volume_affine(src, sv, dst, dv, m) == STATE and b"communicator" in L.tomo_last_error()
    assert L.tomo_volume_affine_axpy(src, sv, dst, dv, m, 0.5, 0) == STATE and b"communicator" in L.tomo_last_error()
assert np.array_equal(a.get_volume(V0).view(np.uint32), x.view(np.uint32))   # nothing was written
assert np.array_equal(b.get_volume(V1).view(np.uint32), w.view(np.uint32))
_lib.check(L.tomo_comm_destroy(b.be.h))
a.volume_affine_to(b, ident, src=V0, dst=V1)
ref = np.zeros_like(w)
ref[:N] = x
assert np.array_equal(b.get_volume(V1).view(np.uint32), ref.view(np.uint32))
print("AFFINE3D_COMM_REFUSED_OK")
