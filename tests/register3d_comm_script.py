"""Run by test_gpu_register3d.py in a child process: an engine bound to a one-rank RCCL communicator (tomo_comm_unique_id /
tomo_comm_init, as a C host would) is refused by tomo_volume_affine_normal with TOMO_ERR_STATE, as the fixed engine, as the moving
one and as both, and the call works again once the communicator is gone."""
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
ident, out = np.eye(3, 4).ravel(), np.full(32, -1.0)
m, o = ident.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p)
idbuf = (ctypes.c_ubyte * 128)()
_lib.check(L.tomo_comm_unique_id(idbuf))
_lib.check(L.tomo_comm_init(b.be.h, idbuf, 1, 0))
for fx, fv, mv_e, mv in ((a.be.h, V0, b.be.h, V1), (b.be.h, V1, a.be.h, V0), (b.be.h, V1, b.be.h, V1)):
    assert L.tomo_volume_affine_normal(fx, fv, mv_e, mv, m, 0, o) == STATE and b"communicator" in L.tomo_last_error()
assert np.all(out == -1.0)                                                    # nothing was written
_lib.check(L.tomo_comm_destroy(b.be.h))
H, g, ssd, count, ncc = a.volume_affine_normal(b, ident, margin=0, fixed_vol=V0, moving_vol=V1)
assert count == N * (N - 1) ** 2 and np.isfinite(H).all() and ssd > 0         # all N slices of a have their second tap inside b's N + 2
print("REGISTER3D_COMM_REFUSED_OK")
