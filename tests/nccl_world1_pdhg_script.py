"""Run by test_gpu_pdhg_sharded.py in a child process: the native whole call of the slab-sharded Chambolle-Pock loop (tomo_comm_pdhg:
niter x {one RCCL group of self-sends, one iteration}) on a one-rank communicator against tomo_pdhg on a plain engine of the same
shape, in both step modes.  The communicator is made through the C ABI alone (tomo_comm_unique_id / tomo_comm_init), as a C host would."""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ref64  # noqa: E402
import ref64_pdhg as R  # noqa: E402
from tomo_tv_amd import _lib  # noqa: E402
from tomo_tv_amd._lib import S_DIFF, VOL_RECON, VOL_YK  # noqa: E402
from tomo_tv_amd.engine import tomoengine  # noqa: E402

N, NX, NITER, LAM = 32, 65, 6, 0.125
ang = np.linspace(-70, 70, 9)
b = ref64.Matrix(N, ang).fp(R.block_phantom(NX, N)).astype(np.float32)
L = _lib.load()


def engine():
    t = tomoengine(NX, N, ang * np.pi / 180)
    t.set_tilt_series(b)
    t.restart_recon()
    return t


for precond in (0, 1):
    plain = engine()
    plain.pdhg_begin()
    plain.pdhg(NITER, LAM, precond=bool(precond), slot=S_DIFF)
    want = (plain.get_volume(VOL_RECON), plain.get_volume(VOL_YK), plain._scalar(S_DIFF))
    t = engine()
    h = t.be.h
    idbuf = (ctypes.c_ubyte * 128)()
    _lib.check(L.tomo_comm_unique_id(idbuf))
    _lib.check(L.tomo_comm_init(h, idbuf, 1, 0))
    assert L.tomo_comm_pdhg(h, 1, LAM, 1.0, precond, 1.0, -1) == 3           # before tomo_pdhg_slab_begin
    assert L.tomo_pdhg_begin(h) == 3 and b"whole-volume" in L.tomo_last_error()     # the whole-volume calls keep refusing a communicator
    _lib.check(L.tomo_pdhg_slab_begin(h))
    _lib.check(L.tomo_comm_pdhg(h, NITER - 2, LAM, 1.0, precond, 1.0, -1))
    _lib.check(L.tomo_comm_pdhg_exchange(h))                                 # the step-wise composition of the same call
    _lib.check(L.tomo_pdhg_slab_iter(h, LAM, 1.0, precond, 1.0, -1))
    _lib.check(L.tomo_comm_pdhg(h, 1, LAM, 1.0, precond, 1.0, S_DIFF))
    rounds = ctypes.c_int(0)
    _lib.check(L.tomo_get_option(h, b"comm_rounds", ctypes.byref(rounds)))
    assert rounds.value == NITER, rounds.value                               # one round per iteration
    got = (t.get_volume(VOL_RECON), t.get_volume(VOL_YK), t.be.scalars()[S_DIFF])
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and want[0].any(), precond
    assert abs(got[2] - want[2]) <= 1e-12 * want[2], (got[2], want[2])
    _lib.check(L.tomo_comm_destroy(h))
print("NCCL_WORLD1_PDHG_OK")
