"""Run by test_gpu_dart.py in a child process: an engine bound to a one-rank RCCL communicator (tomo_comm_unique_id / tomo_comm_init, as a
C host would) refuses every tomo_dart_* call with TOMO_ERR_STATE -- before a classify and, for a state made before the communicator
was bound, after one -- and computes again once the communicator is gone."""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ref64_dart as R  # noqa: E402
from tomo_tv_amd import _lib  # noqa: E402
from tomo_tv_amd.engine import tomoengine  # noqa: E402

V0, V1, STATE = 5, 6, 3
L = _lib.load()
t = tomoengine(5, 12, np.deg2rad(np.linspace(-60, 60, 3)))
h = t.be.h
rng = np.random.default_rng(2)
x = rng.uniform(0, 1, (5, 12, 12)).astype(np.float32)
t.set_volume(x, V0)
thr = (ctypes.c_float * 3)(0.2, 0.5, 0.8)
grey = (ctypes.c_float * 4)(0.0, 0.3, 0.6, 1.0)
out, st = (ctypes.c_double * 32)(), (ctypes.c_uint8 * x.size)()
_lib.check(L.tomo_dart_classify(h, V0, thr, 3, 26, 0, 0))                 # a state in hand: the communicator alone must refuse
idbuf = (ctypes.c_ubyte * 128)()
_lib.check(L.tomo_comm_unique_id(idbuf))
_lib.check(L.tomo_comm_init(h, idbuf, 1, 0))
calls = [lambda: L.tomo_dart_classify(h, V0, thr, 3, 26, 0, 0), lambda: L.tomo_dart_restore(h, V0, grey, 4),
         lambda: L.tomo_dart_segment(h, V0, grey, 4), lambda: L.tomo_dart_arm(h, V0, 0, 1, grey, 4),
         lambda: L.tomo_dart_smooth(h, V0, V1, 0.1), lambda: L.tomo_dart_class_stats(h, V0, thr, 3, out),
         lambda: L.tomo_dart_get_state(h, st)]
for i, f in enumerate(calls):
    assert f() == STATE, i
    assert b"communicator" in L.tomo_last_error(), i
assert np.array_equal(t.get_volume(V0).view(np.uint32), x.view(np.uint32))   # nothing was written
_lib.check(L.tomo_comm_destroy(h))
want = R.state(x, np.array(thr[:], np.float32), 26, 0, 0)
assert np.array_equal(t.dart_state(), want)                                  # the state of before, untouched
_lib.check(L.tomo_dart_classify(h, V0, thr, 3, 6, 0, 0))
assert np.array_equal(t.dart_state(), R.state(x, np.array(thr[:], np.float32), 6, 0, 0))
print("DART_COMM_REFUSED_OK")
