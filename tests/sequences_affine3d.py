"""Rows of the call-sequence closure table (tests/sequences.py: CLASSIFICATION) for the entry points of the 3-D affine resampling.
The closure test asks for a row per ``int tomo_*(tomo_engine *...)`` prototype; these two are writers of a volume slot whose claim
test lives in tests/test_gpu_affine3d.py (test_claim_is_dropped_by_a_resampled_volume), so they carry an ``excluded:`` reason like
``tomo_volume_prolong``.  Imported by the test modules of this feature, hence registered whenever the suite is collected."""
import sequences as S

_CLAIM = "excluded: test_gpu_affine3d holds its claim test (test_claim_is_dropped_by_a_resampled_volume)"
ROWS = {"tomo_volume_affine": ("vol", _CLAIM), "tomo_volume_affine_axpy": ("vol", _CLAIM)}
S.CLASSIFICATION.update(ROWS)
