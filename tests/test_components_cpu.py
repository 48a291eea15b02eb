"""Connected components without a GPU: the plain statement of tests/ref64_components.py against a brute-force flood fill, against
scipy.ndimage.label where scipy is installed, its measurements against loops; the ABI of the five calls; the closure table; the host
rules of ``TomoGPU.label_particles``."""
import ctypes
import os
import re

import numpy as np
import pytest

import ref64_components as R
import sequences as S
import sequences_components as SC
from conftest import ROOT

CALLS = ("tomo_components_label", "tomo_components_get_labels", "tomo_components_stats", "tomo_components_keep", "tomo_components_release")


def flood(fg, connectivity):
    """labels by a stack-based flood fill started at every unlabelled foreground voxel in index order"""
    lab = np.zeros(fg.shape, np.int32)
    offs, K = R.offsets(connectivity), 0
    for start in zip(*np.nonzero(fg)):
        if lab[start]:
            continue
        K += 1
        lab[start] = K
        stack = [start]
        while stack:
            v = stack.pop()
            for o in offs:
                w = tuple(a + b for a, b in zip(v, o))
                if all(0 <= c < n for c, n in zip(w, fg.shape)) and fg[w] and not lab[w]:
                    lab[w] = K
                    stack.append(w)
    return lab, K


def tiny_volumes():
    yield "empty", np.zeros((3, 5, 5), np.float32)
    yield "full", np.ones((3, 5, 5), np.float32)
    yield "checker", SC.checkerboard((3, 6, 6))
    yield "edge", SC.touching_blocks((4, 8, 8), False)
    yield "corner", SC.touching_blocks((4, 8, 8), True)
    yield "serpentine", SC.serpentine((3, 8, 8))
    yield "path", SC.serpentine_path((5, 8, 8))
    yield "nowrap", SC.no_wrap((3, 16, 16))
    for seed in range(3):
        yield f"random{seed}", SC.random_volume((4, 7, 9), 0.3, seed)


@pytest.mark.parametrize("connectivity", [6, 26])
def test_reference_against_a_flood_fill(connectivity):
    for name, x in tiny_volumes():
        fg = R.foreground(x, SC.LO, SC.HI)
        lab, K = R.label(fg, connectivity)
        want, Kw = flood(fg, connectivity)
        assert K == Kw and np.array_equal(lab, want), name
    # what the constructions promise
    assert R.label(R.foreground(SC.checkerboard((3, 6, 6)), SC.LO, SC.HI), connectivity)[1] == (54 if connectivity == 6 else 1)
    for corner in (False, True):
        assert R.label(SC.touching_blocks((4, 8, 8), corner) > 0, connectivity)[1] == (2 if connectivity == 6 else 1)
    for shape in ((5, 16, 16), (70, 16, 16), (5, 24, 24)):
        for make in (SC.serpentine, SC.serpentine_path):
            x = make(shape)
            assert R.label(x > 0, connectivity)[1] == 1, (shape, make.__name__)
        even = (shape[0] + 1) // 2 / shape[0]                                          # the share of slices that carry a snake of the path
        assert 0.45 < SC.serpentine(shape).mean() < 0.6 and 0.45 * even < SC.serpentine_path(shape).mean() < 0.6 * even
    assert R.label(SC.no_wrap((5, 16, 16)) > 0, connectivity)[1] == 8


def test_foreground_rule():
    x = np.array([0.25, 0.75, np.nextafter(np.float32(0.25), np.float32(0)), np.nextafter(np.float32(0.75), np.float32(1)), np.nan, np.inf,
                  -np.inf, 0.5], np.float32)
    assert R.foreground(x, 0.25, 0.75).tolist() == [True, True, False, False, False, False, False, True]
    assert R.foreground(x, -np.inf, np.inf).tolist() == [True] * 4 + [False, True, True, True]


@pytest.mark.parametrize("connectivity", [6, 26])
@pytest.mark.parametrize("shape", [(1, 16, 16), (5, 16, 16), (70, 16, 16), (130, 12, 12)])
@pytest.mark.parametrize("density", [0.2, 0.35, 0.5])
def test_reference_against_scipy(shape, density, connectivity):
    ndi = pytest.importorskip("scipy.ndimage")
    fg = SC.random_volume(shape, density, 7) > 0
    want, Kw = ndi.label(fg, structure=ndi.generate_binary_structure(3, 1 if connectivity == 6 else 3))
    lab, K = R.label(fg, connectivity)
    assert K == Kw and np.array_equal(lab, want)


@pytest.mark.parametrize("connectivity, density", [(6, 0.3), (26, 0.12)])
def test_measurements_against_loops(connectivity, density):
    x = SC.random_volume((4, 7, 9), density, 5)
    lab, K, st = R.components(x, SC.LO, SC.HI, connectivity)
    assert K > 3 and st.dtype.itemsize == 72
    for k in range(1, K + 1):
        vox = [v for v in zip(*np.nonzero(lab == k))]
        r = st[k - 1]
        assert r["voxels"] == len(vox)
        for i, n in enumerate("syz"):
            c = [v[i] for v in vox]
            assert (r["sum_" + n], r["min_" + n], r["max_" + n]) == (sum(c), min(c), max(c))
        assert r["first"] == min((s * 7 + y) * 9 + z for s, y, z in vox)
        surf = 0
        for v in vox:
            for o in R.offsets(6):
                w = tuple(a + b for a, b in zip(v, o))
                if not all(0 <= c < n for c, n in zip(w, lab.shape)) or lab[w] == 0:
                    surf += 1
                    break
        assert r["surface"] == surf
    assert np.all(np.diff(st["first"]) > 0)                                            # the numbering rule
    table = np.concatenate([[True], st["voxels"] >= 3])
    kept = R.keep(x, lab, table, -2.0)
    assert np.array_equal(kept == -2.0, np.isin(lab, 1 + np.flatnonzero(st["voxels"] < 3))) and np.array_equal(kept[kept != -2.0], x[kept != -2.0])


def test_header_declares_and_library_exports_the_five_calls():
    from tomo_tv_amd import _lib
    text = open(os.path.join(ROOT, "include", "tomo_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    L = _lib.load()
    for name in CALLS:
        assert re.search(r"\bint\s+%s\s*\(\s*tomo_engine\s*\*" % name, src), name
        assert hasattr(L, name) and name in _lib.SIGNATURES, name
    k = ctypes.c_int64(0)
    buf = (ctypes.c_uint8 * 72)()
    assert L.tomo_components_label(None, 0, 0.0, 1.0, 26, ctypes.byref(k)) == 1 and L.tomo_components_get_labels(None, buf) == 1
    assert L.tomo_components_stats(None, 1, buf) == 1 and L.tomo_components_keep(None, 0, buf, 1, 0.0) == 1
    assert L.tomo_components_release(None) == 1 and L.tomo_last_error()                # a null engine: TOMO_ERR_ARG, no crash
    # the record of the header, field by field, is the numpy dtype
    m = re.search(r"typedef struct tomo_component \{(.*?)\} tomo_component;", src, re.S)
    fields = []
    for ctype, names in re.findall(r"(int64_t|int32_t)\s+([^;]+);", m.group(1)):
        fields += [(n.strip(), "<i8" if ctype == "int64_t" else "<i4") for n in names.split(",")]
    assert fields == _lib.COMPONENT_FIELDS and np.dtype(_lib.COMPONENT_FIELDS).itemsize == 72


def test_the_closure_table_has_no_errors():
    import sequences_affine3d, sequences_condition, sequences_markers, sequences_register3d, sequences_sino_normal, sequences_tilt  # noqa: F401, E401
    names = S.header_prototypes(open(os.path.join(ROOT, "include", "tomo_hip.h")).read())
    assert set(SC.ROWS) == set(CALLS) <= set(names) and S.closure_errors(names) == []


class FakeEngine:
    """the engine calls of ``TomoGPU.label_particles`` on the reference"""

    def __init__(self, x):
        self.x, self.calls = np.array(x, np.float32), []

    def _components_one_engine(self):
        pass

    def label_components(self, vol, lo, hi, connectivity=26):
        self.calls.append(("label", lo, hi, connectivity))
        self.lab, K, self.st = R.components(self.x, lo, hi, connectivity)
        return K

    def component_stats(self):
        return self.st

    def component_labels(self):
        return self.lab

    def keep_components(self, vol, keep, fill=0.0):
        self.calls.append(("keep", fill))
        assert len(keep) == self.st.size + 1
        self.x = R.keep(self.x, self.lab, keep, fill)


def test_label_particles_post_processing():
    from tomo_tv_amd.reconstructor import TomoGPU, particle_table, particles_to_keep
    x = np.zeros((6, 12, 12), np.float32)
    x[1:4, 2:5, 2:5] = 1.0                                  # 27 voxels, centre (2, 3, 3)
    x[4, 8, 8:10] = 1.0                                     # 2 voxels
    x[0, 0, 11] = 2.0                                       # 1 voxel of another grey level
    g = object.__new__(TomoGPU)
    g.tomo = FakeEngine(x)
    out = g.label_particles(threshold=0.5, connectivity=6)
    assert out["count"] == 3 and out["voxels"].tolist() == [1, 27, 2] and out["first"].tolist() == [11, 144 + 24 + 2, 4 * 144 + 96 + 8]
    assert np.array_equal(out["centroid"], [[0, 0, 11], [2, 3, 3], [4, 8, 8.5]]) and out["centroid"].dtype == np.float64
    assert np.array_equal(out["bbox"][1], [[1, 2, 2], [3, 4, 4]]) and out["surface"].tolist() == [1, 26, 2]
    assert np.allclose(out["equivalent_diameter"], np.cbrt(6 * np.array([1, 27, 2]) / np.pi), rtol=1e-15)
    assert g.tomo.calls == [("label", 0.5, float("inf"), 6)]
    assert np.array_equal(g.get_particle_labels(), R.label(x >= 0.5, 6)[0])
    # one grey level of a discrete result
    g.tomo = FakeEngine(x)
    assert g.label_particles(level=(1.0, 0.25))["voxels"].tolist() == [27, 2]
    # min_voxels: the smaller ones are removed from the volume, then labelled again
    g.tomo = FakeEngine(x)
    out = g.label_particles(threshold=0.5, min_voxels=3, fill=-1.0)
    assert out["count"] == 1 and out["voxels"].tolist() == [27] and [c[0] for c in g.tomo.calls] == ["label", "keep", "label"]
    assert g.tomo.x[0, 0, 11] == -1.0 and g.tomo.x[4, 8, 8] == -1.0 and g.tomo.x[2, 3, 3] == 1.0
    assert particles_to_keep([5, 2, 3], 3).tolist() == [True, True, False, True]
    empty = particle_table(np.zeros(0, R.DTYPE))
    assert empty["count"] == 0 and empty["centroid"].shape == (0, 3) and empty["bbox"].shape == (0, 2, 3)
    for bad in (dict(threshold=0.5, level=(1.0, 0.1)), dict(level=(1.0, -0.1)), dict(threshold=0.5, min_voxels=0)):
        with pytest.raises(ValueError):
            g.label_particles(**bad)
