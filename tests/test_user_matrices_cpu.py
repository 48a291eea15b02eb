"""The matrix families of tests/user_matrices.py, checked without a GPU: each family reaches the edges it is listed for (counted on the
binary64 matrix alone), ``canonical`` is what the oracle's loadA keeps, and the host table builders take every family -- replayed by
tests/native/user_matrix_check under AddressSanitizer + UBSan -- with exactly the answers the GPU test pins
(``user_matrices.EXPECTED``)."""
import os
import subprocess

import numpy as np
import pytest

import oracle
import ref64
import user_matrices as um
from user_matrices import GEOM
from tomo_tv_amd.engine import system_matrix

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = [f"{f}-{g}" for f, g in um.CASES]
_CACHE = {}


def case(name, gid):
    if (name, gid) not in _CACHE:
        ang, N, Nx = GEOM[gid]
        A = um.family(name, system_matrix(N, ang), N, ang.size)
        M, dropped = um.reference(N, ang, A)
        _CACHE[name, gid] = (A, M, dropped)
    return _CACHE[name, gid]


@pytest.fixture(scope="module")
def checker():
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "native"), "-s", "usermat"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return os.path.join(ROOT, "tests", "native", "build", "san_user_matrix_check")


@pytest.mark.parametrize("name,gid", um.CASES, ids=IDS)
def test_family_reaches_what_it_is_listed_for(name, gid):
    ang, N, _ = GEOM[gid]
    A, M, dropped = case(name, gid)
    um.assert_reaches(name, N, ang.size, um.properties(M), dropped)
    if name in ("dead", "messy"):
        rows, pix, angle = um.dead_parts(N, ang.size)
        assert not M.row_nnz[rows[0]] or name == "messy"                   # (messy puts an explicit zero into a dead ray)
        assert np.all(M.rowsum[rows] == 0) and np.all(M.colsum[pix] == 0) and np.all(M.rowsum[angle * N:(angle + 1) * N] == 0)
    if name == "signed":
        i = um.SIGNED_ANGLE
        assert np.all(M.rowsum[i * N:(i + 1) * N] < 0) and np.all(um.angle_colsum(M, i) <= 0) and np.any(um.angle_colsum(M, i) < 0)
    # float32 sums in any order take the sign of the binary64 sums: the > 0 rules of the kernels and of ref64 agree by construction
    assert um.signs_are_safe(M)


@pytest.mark.parametrize("name,gid", um.CASES, ids=IDS)
def test_canonical_is_what_the_oracle_keeps(name, gid):
    ang, N, _ = GEOM[gid]
    A, M, dropped = case(name, gid)
    csr = oracle.load_A(A, M.nrow, M.ncol)                                 # the raw triplets: orc_csr_from_coo is last-wins
    ptr, idx, val = M.csr()
    assert csr.nnz == A.shape[1] - dropped
    assert np.array_equal(csr.ptr, ptr) and np.array_equal(csr.idx, idx)
    assert np.array_equal(csr.val.view(np.uint32), val.view(np.uint32))    # bit for bit: -0.0 stays -0.0


def test_canonical_keeps_the_last_assignment_and_explicit_zeros():
    A = np.array([[1, 0, 1, 1, 0, 1], [2, 3, 0, 2, 3, 1], [5.0, 1.0, 7.0, 6.0, 0.0, -0.0]], np.float32)
    C = um.canonical(A, 4)
    assert C.tolist() == [[0.0, 1.0, 1.0, 1.0], [3.0, 0.0, 1.0, 2.0], [0.0, 7.0, -0.0, 6.0]]
    assert np.signbit(C[2, 2])
    M = ref64.Matrix(2, np.zeros(2), A=C)
    assert M.duplicates == 0 and ref64.Matrix(2, np.zeros(2), A=A).duplicates == 2


def test_messy_changes_the_result_through_last_wins():
    """Some duplicated entries end with the second value, some with the first, and the killed entries end as explicit zeros."""
    ang, N, _ = GEOM["lin70"]
    A, M, dropped = case("messy", "lin70")
    D = um.canonical(um.dead(system_matrix(N, ang), N, ang.size), N * N)
    key = {(int(r), int(c)): w for r, c, w in D.T}
    changed = sum(1 for r, c, w in um.canonical(A, N * N).T if (int(r), int(c)) in key and key[int(r), int(c)] != w and w != 0)
    killed = sum(1 for r, c, w in um.canonical(A, N * N).T if (int(r), int(c)) in key and w == 0)
    assert 0 < changed < dropped - 3 and killed == 3


def test_art_reference_takes_a_row_order():
    ang, N, _ = GEOM["repeat"]
    A, M, _ = case("messy", "repeat")
    x = ref64.dense_volume(2, N, seed=5)
    b = ref64.signed_sino(2, M.nrow, seed=6)
    order = np.random.default_rng(3).permutation(M.nrow)
    orc = oracle.ctvlib(2, N, ang.size)
    orc.load_A(A)
    orc.set_tilt_series(b)
    orc.row_inner_product()
    for o in (None, order):
        orc.recon[:] = x
        orc.ART(0.6, order=o)
        ref = M.art(x, b, 0.6, order=o)
        assert np.abs(orc.recon - ref).max() < 1e-4
    assert np.abs(M.art(x, b, 0.6, order=order) - M.art(x, b, 0.6)).max() > 1e-3


@pytest.mark.parametrize("name,gid", um.CASES, ids=IDS)
def test_table_builders_take_the_family(checker, tmp_path, name, gid):
    ang, N, Nx = GEOM[gid]
    A, _, _ = case(name, gid)
    path = str(tmp_path / "triplets.bin")
    um.write_triplets(path, N, ang.size, -(-Nx // 64), A)
    r = subprocess.run([checker, path, "q"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = r.stdout.strip().splitlines()[-1]
    got = {k: int(v) for k, v in (kv.split("=") for kv in line.split())}
    assert got == um.EXPECTED[name, gid], line


def test_table_builders_take_two_idle_angles(checker, tmp_path):
    ang, N, Nx = GEOM["lin70"]
    A = um.idle_pair(system_matrix(N, ang[:2]), N)
    M, _ = um.reference(N, ang[:2], A)
    assert np.all(M.rowsum <= 0) and np.all(M.colsum <= 0) and um.signs_are_safe(M)
    path = str(tmp_path / "idle.bin")
    um.write_triplets(path, N, 2, -(-Nx // 64), A)
    r = subprocess.run([checker, path, "q"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = r.stdout.strip().splitlines()[-1]
    assert {k: int(v) for k, v in (kv.split("=") for kv in line.split())} == um.EXPECTED_IDLE, line
