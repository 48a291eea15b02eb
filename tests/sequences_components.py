"""Rows of the call-sequence closure table (tests/sequences.py: CLASSIFICATION) for the connected-component entry points, and the volumes
and call sequence their tests share.  ``tomo_components_label`` reads a volume through the read-only view and writes only the engine's
label state (buffers of their own, no lane, no staging buffer); ``tomo_components_get_labels`` and ``tomo_components_stats`` read that
state back; ``tomo_components_keep`` writes a caller-named volume through ``get_vol`` like the DART writers, its table through the
staging buffer in stream order.  Imported by the test modules of this feature, hence registered whenever the suite is collected."""
import numpy as np

import sequences as S

ROWS = {"tomo_components_label": ("state", "internal: the engine's label state (labels, root counts, records); reads the volume through get_vol_ro"),
        "tomo_components_get_labels": ("query", ""),
        "tomo_components_stats": ("query", ""),
        "tomo_components_keep": ("vol stage", "excluded: writes a caller-named slot through get_vol; test_gpu_components holds its used-engine and claim "
                                 "tests (test_used_engine_gives_a_fresh_engines_labels, test_the_new_calls_leave_a_later_sirt_run_alone)"),
        "tomo_components_release": ("query", "")}
S.CLASSIFICATION.update(ROWS)

F32 = np.float32
LO, HI = 0.5, 1.5                                       # the band of the 0 / 1 volumes below


def random_volume(shape, density, seed):
    return (np.random.default_rng(seed).random(shape) < density).astype(F32)


def checkerboard(shape):
    s, y, z = np.indices(shape)
    return ((s + y + z) % 2 == 0).astype(F32)


def touching_blocks(shape, corner):
    """two blocks that share only an edge (a line along s), or with ``corner`` only a corner point (where there are two slices)"""
    ns, n, _ = shape
    a, h = n // 2, max(1, ns // 2)
    x = np.zeros(shape, F32)
    if corner:
        x[:h, 2:a, 2:a] = 1
        x[h:, a:n - 2, a:n - 2] = 1
    else:
        x[:, 2:a, 2:a] = 1
        x[:, a:n - 2, a:n - 2] = 1
    return x


def serpentine(shape):
    """every slice: the even rows whole, joined at alternating ends by one voxel of the odd row between them; odd slices mirrored in
    z.  One component of about half the voxels that visits every row of every slice."""
    ns, n, _ = shape
    x = np.zeros(shape, F32)
    x[:, 0::2, :] = 1
    for j, y in enumerate(range(1, n - 1, 2)):
        x[:, y, n - 1 if j % 2 == 0 else 0] = 1
    x[1::2] = x[1::2, :, ::-1]
    return x


def serpentine_path(shape):
    """ONE path: the snake of ``serpentine`` in the even slices only, successive snakes joined end to end through a single voxel of
    the odd slice between them (alternately at the snake's end and at its start): the longest chain of parent links the size allows
    under 6-connectivity, a quarter of the voxels."""
    ns, n, _ = shape
    x = np.zeros(shape, F32)
    x[0::2, 0::2, :] = 1
    rows = list(range(1, n - 1, 2))
    for j, y in enumerate(rows):
        x[0::2, y, n - 1 if j % 2 == 0 else 0] = 1
    last = n - 2 if n % 2 == 0 else n - 1                 # the last even row, and the end the snake leaves it at
    end = (last, 0 if (last // 2) % 2 == 1 else n - 1)
    for k, s in enumerate(range(1, ns - 1, 2)):
        x[(s,) + (end if k % 2 == 0 else (0, 0))] = 1
    return x


def no_wrap(shape):
    """pieces on opposite faces, and on the two ends of consecutive rows, that only a periodic neighbour (or a run that crosses a row
    end in the linear index) would join"""
    ns, n, _ = shape
    x = np.zeros(shape, F32)
    x[0, 4:6, 4:6] = 1
    if ns >= 3:
        x[ns - 1, 4:6, 4:6] = 1
    x[:, 0, 8:10] = 1
    x[:, n - 1, 8:10] = 1
    x[ns // 2, 10:12, 0] = 1
    x[ns // 2, 10:12, n - 1] = 1
    x[ns // 2, 7, n - 1] = 1
    x[ns // 2, 8, 0] = 1
    return x


def special_values(shape, seed):
    """values in [0, 1] with voxels exactly at the bounds 0.25 and 0.75, one ulp outside them, NaN and both infinities"""
    rng = np.random.default_rng(seed)
    x = rng.random(shape).astype(F32)
    flat = x.reshape(-1)
    pick = rng.choice(flat.size, size=min(flat.size, 21), replace=False)
    lo, hi = F32(0.25), F32(0.75)
    vals = [lo, hi, np.nextafter(lo, F32(0)), np.nextafter(hi, F32(1)), F32(np.nan), F32(np.inf), F32(-np.inf)]
    for i, p in enumerate(pick):
        flat[p] = vals[i % len(vals)]
    return x


def component_calls(e, x, vol, lo=LO, hi=HI):
    """Every component entry point on engine ``e`` with volume ``x`` in slot ``vol``; -> the results, for the tests that compare them."""
    out = {}
    for c in (6, 26):
        e.set_volume(x, vol)
        out[f"K{c}"] = np.array([e.label_components(vol, lo, hi, c)])
        out[f"labels{c}"] = e.component_labels()
        st = e.component_stats()
        out[f"stats{c}"] = st.view(np.uint8)
        table = np.concatenate([[True], st["voxels"] >= 3])
        e.keep_components(vol, table, -2.0)
        out[f"kept{c}"] = e.get_volume(vol)
    e.release_components()
    return out
