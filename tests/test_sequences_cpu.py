"""Closure of the call-sequence tables (tests/sequences.py): every engine entry point of include/tomo_hip.h is classified, every writer
is in section (c) of tests/test_gpu_sequences.py and every reduction user in section (d), or excluded with a written reason.  A new
ABI entry point without a row fails here, on any machine."""
import os

import sequences as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    with open(os.path.join(ROOT, "include", "tomo_hip.h")) as f:
        return f.read()


def test_every_entry_point_is_classified():
    names = S.header_prototypes(_header())
    assert len(names) > 130 and len(set(names)) == len(names), len(names)
    assert S.closure_errors(names) == []


def test_a_new_prototype_or_a_dropped_row_is_noticed():
    text = _header()
    names = S.header_prototypes(text + "\nint tomo_dummy_writer(tomo_engine *e, int vol);\n")
    assert S.closure_errors(names) == ["tomo_dummy_writer: no row in tests/sequences.py CLASSIFICATION"]
    names = S.header_prototypes(text)
    for victim in ("tomo_dart_smooth", "tomo_get_dims"):
        table = {k: v for k, v in S.CLASSIFICATION.items() if k != victim}
        assert any(e.startswith(victim + ":") for e in S.closure_errors(names, table)), victim
    # a writer that loses its section (c) entry and has no reason, a reduction user outside section (d), a reason that is none
    table = dict(S.CLASSIFICATION, tomo_sirt=("vol", ""), tomo_l1_norm=("reduce", ""), tomo_cgls=("vol", "excluded: old"))
    errs = S.closure_errors(names, table)
    assert sum(e.startswith(("tomo_sirt:", "tomo_l1_norm:", "tomo_cgls:")) for e in errs) >= 3, errs


def test_the_pair_matrix_is_as_large_as_promised():
    pairs = S.pairs()
    assert len(S.DISTURBERS) >= 10 and len(S.PROBES) >= 11
    at_a = {(d, p) for g, d, p in pairs if g in ("A", "C")}
    assert at_a == {(d, p) for d in S.DISTURBERS for p in S.PROBES}
    assert {p for g, d, p in pairs if g == "B"} == set(S.FORM_PROBES)
    assert len(set(pairs)) == len(pairs)


def test_sections_c_and_d_hold_a_case_for_every_entry_of_their_tables():
    """The case dicts of tests/test_gpu_sequences.py against the tables (importing that module needs no GPU)."""
    import test_gpu_sequences as G
    assert set(G.WRITERS) | {"tomo_adopt_volumes"} == set(S.CLAIM_VOLUME_WRITERS) | set(S.CLAIM_SINO_WRITERS)
    assert G.test_claim_is_dropped_by_a_new_geometry is not None          # the case of tomo_adopt_volumes
    assert set(G.REDUCERS) == set(S.LANE_REDUCERS)
