"""Run by test_gpu_sino_normal.py in a child process: an engine bound to a one-rank RCCL communicator (tomo_comm_unique_id /
tomo_comm_init, as a C host would) is refused by tomo_sino_affine_normal with TOMO_ERR_STATE, and the call works again once the
communicator is gone."""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tomo_tv_amd import _lib  # noqa: E402
from tomo_tv_amd.engine import tomoengine  # noqa: E402

STATE, N, NS, P = 3, 8, 10, 3
L = _lib.load()
e = tomoengine(NS, N, np.deg2rad(np.linspace(-50, 40, P)))
b = np.random.default_rng(2).uniform(-1, 1, (NS, N * P)).astype(np.float32)
e.be.c("set_sinogram", 3, b.ctypes.data_as(ctypes.c_void_p))
ident, out = np.tile([1.0, 0, 0, 0, 1.0, 0], (P, 1)), np.full((P, 21), -1.0)
m, o = ident.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p)
idbuf = (ctypes.c_ubyte * 128)()
_lib.check(L.tomo_comm_unique_id(idbuf))
_lib.check(L.tomo_comm_init(e.be.h, idbuf, 1, 0))
assert L.tomo_sino_affine_normal(e.be.h, 3, 3, m, 0, o) == STATE and b"communicator" in L.tomo_last_error()
assert np.all(out == -1.0)                                                    # nothing was written
_lib.check(L.tomo_comm_destroy(e.be.h))
H, g, ssd, count, ncc = e.sino_affine_normal(3, 3, ident, margin=0)
assert np.all(count == (N - 1) * (NS - 1)) and np.isfinite(H).all() and not ssd.any() and not g.any()
print("SINO_NORMAL_COMM_REFUSED_OK")
