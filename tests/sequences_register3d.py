"""Row of the call-sequence closure table (tests/sequences.py: CLASSIFICATION) for the entry point of the 3-D registration.
``tomo_volume_affine_normal`` writes no slot (both volumes are read-only views); it is a reduction user, but of no lane of the engine:
its partial sums live in a buffer of its own, every row of which is written by the call that reads it.  Its back-to-back and claim tests
live in tests/test_gpu_register3d.py, so it carries an ``excluded:`` reason.  Imported by the test modules of this feature, hence
registered whenever the suite is collected."""
import sequences as S

ROWS = {"tomo_volume_affine_normal": ("reduce", "excluded: no lane, a partial buffer of its own; test_gpu_register3d runs it back to back "
                                      "with other calls (test_repeats_bit_for_bit_and_changes_nothing)")}
S.CLASSIFICATION.update(ROWS)
