"""Row of the call-sequence closure table (tests/sequences.py: CLASSIFICATION) for the entry point of the per-projection matching.
``tomo_sino_affine_normal`` writes no slot (both sinograms are read-only views, the claim on the model sinogram stays); it is a
reduction user of the alignment family's own partial sums, every entry of which is written by the call that reads it.  Its
back-to-back, claim and pending-work tests live in tests/test_gpu_sino_normal.py, so it carries an ``excluded:`` reason.  Imported by
the test modules of this feature, hence registered whenever the suite is collected."""
import sequences as S

ROWS = {"tomo_sino_affine_normal": ("reduce", "excluded: no lane, the alignment family's partial buffer; test_gpu_sino_normal runs it back to back "
                                    "and under pending work (test_repeats_bit_for_bit_and_changes_nothing, test_while_work_is_pending)")}
S.CLASSIFICATION.update(ROWS)
