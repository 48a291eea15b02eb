"""The slab-sharded Chambolle-Pock entry points without a GPU: exported, declared with a reference citation, null-safe; the Python
surface a sharded caller needs exists and ``TomoGPU.pdhg_tv`` kept its signature."""
import inspect
import os
import re

from conftest import ROOT

NEW = {"tomo_bind_pdhg_halo": (None, None, None, None, None), "tomo_pdhg_slab_pack": (None, 5, 8),
       "tomo_pdhg_slab_tv_step": (None, 5, 6, 7, 8, 0.1, 0.1, 0.1, 1.0, 0, -1), "tomo_pdhg_slab_begin": (None,),
       "tomo_pdhg_slab_iter": (None, 0.1, 1.0, 1, 1.0, -1), "tomo_comm_pdhg_exchange": (None,),
       "tomo_comm_pdhg": (None, 1, 0.1, 1.0, 1, 1.0, -1)}


def test_new_symbols_are_exported_and_reject_a_null_engine():
    from tomo_tv_amd import _lib
    L = _lib.load()
    for name, args in NEW.items():
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name]) == len(args), name
        assert getattr(L, name)(*args) != 0, name
        assert L.tomo_last_error(), name


def test_header_declares_them_with_a_reference_citation():
    src = open(os.path.join(ROOT, "include", "tomo_hip.h")).read()
    for name in NEW:
        m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int " + name + r"\(", src, flags=re.S)
        assert m, f"{name}: no declaration with a comment in front of it"
        assert re.search(r"mpi_ctvlib\.cpp:400-422", m.group(1)), f"{name}: the comment does not cite the ring it replaces"


def test_python_surface():
    from tomo_tv_amd.engine import _SlabBackend, tomoengine
    from tomo_tv_amd.reconstructor import TomoGPU
    for name in ("pdhg_planes", "pdhg_slab_pack", "pdhg_exchange"):
        assert callable(getattr(tomoengine, name)), name
    assert callable(_SlabBackend.pdhg_planes)
    sig = inspect.signature(TomoGPU.pdhg_tv)
    assert str(sig) == "(self, Niter=100, lambda_param=0.1, theta=1.0, precond=True, ratio=1.0, show_convergence=True)"
