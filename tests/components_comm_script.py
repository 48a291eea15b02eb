"""Run by test_gpu_components.py in a child process: an engine bound to a one-rank RCCL communicator (tomo_comm_unique_id /
tomo_comm_init, as a C host would) refuses tomo_components_label, _get_labels, _stats and _keep with TOMO_ERR_STATE -- also with a
labelling made before the communicator was bound -- and labels again once the communicator is gone."""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ref64_components as R  # noqa: E402
from tomo_tv_amd import _lib  # noqa: E402
from tomo_tv_amd.engine import tomoengine  # noqa: E402

V0, STATE = 5, 3
L = _lib.load()
t = tomoengine(5, 12, np.deg2rad(np.linspace(-60, 60, 3)))
h = t.be.h
x = (np.random.default_rng(2).random((5, 12, 12)) < 0.3).astype(np.float32)
t.set_volume(x, V0)
want, K, _ = R.components(x, 0.5, 1.5, 6)
assert t.label_components(V0, 0.5, 1.5, 6) == K                            # a labelling in hand: the communicator alone must refuse
idbuf = (ctypes.c_ubyte * 128)()
_lib.check(L.tomo_comm_unique_id(idbuf))
_lib.check(L.tomo_comm_init(h, idbuf, 1, 0))
k = ctypes.c_int64(-7)
lab = np.full(x.shape, -7, np.int32)
rec = np.zeros(K, R.DTYPE)
tab = np.zeros(K + 1, np.uint8)
calls = [lambda: L.tomo_components_label(h, V0, 0.5, 1.5, 26, ctypes.byref(k)), lambda: L.tomo_components_get_labels(h, lab.ctypes.data),
         lambda: L.tomo_components_stats(h, K, rec.ctypes.data), lambda: L.tomo_components_keep(h, V0, tab.ctypes.data, K + 1, 9.0)]
for i, f in enumerate(calls):
    assert f() == STATE, i
    assert b"communicator" in L.tomo_last_error(), i
assert k.value == -7 and np.all(lab == -7) and not rec.view(np.uint8).any()
assert np.array_equal(t.get_volume(V0).view(np.uint32), x.view(np.uint32))   # nothing was written
_lib.check(L.tomo_comm_destroy(h))
assert np.array_equal(t.component_labels(), want)                            # the labelling of before, untouched
want26, K26, st26 = R.components(x, 0.5, 1.5, 26)
assert t.label_components(V0, 0.5, 1.5, 26) == K26 and np.array_equal(t.component_labels(), want26)
assert np.array_equal(t.component_stats(), st26)
print("COMPONENTS_COMM_REFUSED_OK")
