"""Rows of the call-sequence closure table (tests/sequences.py: CLASSIFICATION) for the conditioning entry points, and the call
sequence their used-engine test runs.  ``tomo_sino_window_stats`` and a measuring ``tomo_sino_median`` write no slot (read-only
views) and are reduction users of the alignment family's own partial sums, every entry of which is written by the call that reads it.
A replacing ``tomo_sino_median`` and ``tomo_sino_intensity`` write a caller-named sinogram slot through ``sino_slot``, which drops
the claim on G where G is the destination, like every slot accessor; the table they upload goes through the staging buffer in stream
order.  Imported by the test modules of this feature, hence registered whenever the suite is collected."""
import numpy as np

import sequences as S
from tomo_tv_amd._lib import SINO_B, SINO_USER0

ROWS = {"tomo_sino_window_stats": ("reduce", "excluded: no lane, the alignment family's partial buffer; test_gpu_condition runs it on a used engine next to its "
                                   "siblings (test_used_engine_gives_a_fresh_engines_bits)"),
        "tomo_sino_median": ("sino stage reduce", "excluded: writes a caller-named slot, no lane; test_gpu_condition holds its used-engine and claim tests "
                             "(test_used_engine_gives_a_fresh_engines_bits, test_the_new_calls_leave_a_later_sirt_run_alone)"),
        "tomo_sino_intensity": ("sino stage", "excluded: writes a caller-named slot; test_gpu_condition holds its used-engine and claim tests "
                                "(test_used_engine_gives_a_fresh_engines_bits, test_the_new_calls_leave_a_later_sirt_run_alone)")}
S.CLASSIFICATION.update(ROWS)


def condition_calls(e):
    """Every conditioning entry point on the tilt series of engine ``e``; -> the results, for the tests that compare them."""
    P, U = e.Nproj, SINO_USER0 + 4
    out = {"stats": e.sino_window_stats(SINO_B), "corner": e.sino_window_stats(SINO_B, (0, max(1, e.Ny // 4), 0, max(1, e.Nslice_ // 4)))}
    for R in (1, 2):
        out[f"measure{R}"] = e.sino_median(SINO_B, radius=R)
        th = (np.float32(0.02) * (1 + np.arange(P))).astype(np.float32)
        out[f"replace{R}"] = e.sino_median(SINO_B, U + R, radius=R, thresh=th)
        out[f"median{R}"] = e._sino(U + R)
    e.sino_intensity(SINO_B, U + 3, np.linspace(0.5, 1.5, P), np.linspace(-0.25, 0.25, P), clamp=True)
    e.sino_intensity(U + 3, U + 3, -1.25, 0.125)
    out["intensity"] = e._sino(U + 3)
    return out
