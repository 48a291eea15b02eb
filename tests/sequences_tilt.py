"""Rows of the call-sequence closure table (tests/sequences.py: CLASSIFICATION) for the entry points of the tilt-angle refinement.
``tomo_volume_rot_derivative`` writes a volume through ``get_vol`` like every volume writer, so a claim on the model sinogram is
dropped by the version it bumps; its claim and used-engine tests live in tests/test_gpu_tilt.py.  ``tomo_sino_tilt_normal`` writes no
slot (three read-only views) and is a reduction user of the alignment family's own partial sums, every entry of which is written by
the call that reads it.  Imported by the test modules of this feature, hence registered whenever the suite is collected."""
import sequences as S

ROWS = {"tomo_volume_rot_derivative": ("vol", "excluded: test_gpu_tilt holds its claim and used-engine tests (test_claim_is_dropped_by_a_derivative_into_the_projected_volume, test_used_engine_gives_a_fresh_engines_bits)"),
        "tomo_sino_tilt_normal": ("reduce", "excluded: no lane, the alignment family's partial buffer; test_gpu_tilt runs it back to back and next to "
                                  "its siblings (test_used_engine_gives_a_fresh_engines_bits)")}
S.CLASSIFICATION.update(ROWS)
