"""Rows of the call-sequence closure table (tests/sequences.py: CLASSIFICATION) for the marker-detection entry points, and the call
sequence their used-engine test runs.  ``tomo_sino_template_ncc`` writes a caller-named sinogram slot through ``sino_slot``, which
drops the claim on G where G is the destination, like every slot accessor; its template goes through the staging buffer in stream
order.  ``tomo_sino_peaks`` writes no slot (a read-only view); its counters are cleared in stream order by the call that reads them
and its records are sorted on the host.  Imported by the test modules of this feature, hence registered whenever the suite is
collected."""
import numpy as np

import sequences as S
from tomo_tv_amd._lib import SINO_B, SINO_USER0

ROWS = {"tomo_sino_template_ncc": ("sino stage", "excluded: writes a caller-named slot; test_gpu_markers holds its used-engine and claim tests "
                                   "(test_used_engine_gives_a_fresh_engines_bits, test_the_new_calls_leave_a_later_sirt_run_alone)"),
        "tomo_sino_peaks": ("reduce", "excluded: no lane, a buffer of its own cleared by every call; test_gpu_markers runs it on a used engine "
                            "(test_used_engine_gives_a_fresh_engines_bits)")}
S.CLASSIFICATION.update(ROWS)


def template(R):
    """a disc with a negative surround: entries of both signs, not symmetric under a transpose"""
    g = np.arange(-R, R + 1, dtype=np.float64)
    T = np.where(g[:, None] ** 2 + g[None, :] ** 2 <= (0.6 * R) ** 2, 1.0, -0.25)
    T[0, :] += 0.125 * np.arange(2 * R + 1)
    return T.astype(np.float32)


def marker_calls(e):
    """Both marker entry points on the tilt series of engine ``e``; -> the results, for the tests that compare them."""
    U = SINO_USER0 + 7
    out = {}
    for R in (1, 3):
        e.sino_template_ncc(SINO_B, U + R, template(R), var_floor=1e-6)
        out[f"ncc{R}"] = e._sino(U + R)
        count, rec = e.sino_peaks(U + R, R, 0.25, capacity=4)
        out[f"count{R}"] = count
        out[f"records{R}"] = np.concatenate(rec)
    count, rec = e.sino_peaks(SINO_B, 2, 0.5)
    out["count_b"], out["records_b"] = count, np.concatenate(rec)
    return out
