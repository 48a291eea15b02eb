"""Matrix families for the tests of engines built from a caller's matrix (``ctvlib.load_A`` / ``update_proj_angles``).

numpy only, deterministic; imported by the GPU tests (tests/test_gpu_user_matrix.py) and the CPU tests
(tests/test_user_matrices_cpu.py).  Every family maps the engine's own float32 ``(3, nnz)`` triplets of N rays and P angles
(``system_matrix(N, angles)``: row = angle * N + ray, col = y * N + z) to new raw triplets -- what the engine and the oracle are
fed.  ``canonical(A)`` is what the engine must then hold: the last assignment of a repeated (row, col) wins, rows sorted by column,
explicit zeros kept as entries.  ``ref64.Matrix`` is built from the canonical triplets (``reference``).

  dead      every entry removed of: the first ray of angle 0, the last ray of the last angle, one middle ray of every third
            angle, one whole angle, a border pixel, the pixel at a 16 x 16 tile corner, an interior 3 x 3 block.  Ray windows only
            shrink.
  gain      every ray's weights times a per-ray float32 factor in [0.5, 2]; half of the factors are powers of two.
  signed    one whole angle negated exactly: its row sums and its per-angle column sums are < 0, nothing else changes sign.
  messy     ``dead``, plus duplicates of ~5 % of the entries with another value, explicit 0.0 / -0.0 weights on pixels the ray does
            not otherwise touch (among them dead pixels, a dead ray and the dead angle), entries whose first assignment is
            non-zero and whose last is 0 -- and the whole triplet list shuffled.
  shuffled  the rays permuted inside every angle (the matrix of test_matrix_whose_ray_windows_defeat_the_tile_kernels).
"""
import numpy as np

FAMILIES = ("dead", "gain", "signed", "messy", "shuffled")
# (angles in degrees, N rays, slices): the four geometries of tests/test_gpu_elementwise.py's GEOM table that the families run on
GEOM = {
    "lin70": (np.linspace(-70, 70, 9), 32, 128),
    "axes45": (np.array([-90.0, -67.0, -45.0, -20.0, 0.0, 20.0, 45.0, 67.0, 90.0]), 33, 128),
    "repeat": (np.array([-40.0, -10.0, 15.0, 15.0, 50.0]), 8, 65),
    "neg150": (np.linspace(-150, -30, 11), 96, 64),
}


def _rc(A):
    return A[0].astype(np.int64), A[1].astype(np.int64)


def dead_parts(N, P):
    """(rows, pixels, angle) that ``dead`` removes: sinogram rows, pixel numbers, and the whole angle among the rows."""
    angle = P // 2
    rows = {0, (P - 1) * N + N - 1}
    rows |= {i * N + min(N - 1, N // 2 + i // 3) for i in range(0, P, 3)}
    rows |= {angle * N + j for j in range(N)}
    c = min(16, N - 1)
    q = N // 4
    pix = {0 * N + N // 3, c * N + c} | {(q + dy) * N + q + dz for dy in range(3) for dz in range(3)}
    return np.array(sorted(rows)), np.array(sorted(pix)), angle


def dead(A, N, P):
    rows, pix, _ = dead_parts(N, P)
    r, c = _rc(A)
    keep = ~np.isin(r, rows) & ~np.isin(c, pix)
    return np.ascontiguousarray(A[:, keep])


def gain_factors(N, P):
    rng = np.random.default_rng(1000 + 7 * N + P)
    f = rng.uniform(0.5, 2.0, N * P).astype(np.float32)
    f[::2] = np.array([0.5, 1.0, 2.0], np.float32)[rng.integers(0, 3, f[::2].size)]
    return f


def gain(A, N, P):
    out = A.copy()
    out[2] = (A[2] * gain_factors(N, P)[A[0].astype(np.int64)]).astype(np.float32)
    return out


SIGNED_ANGLE = 1


def signed(A, N, P):
    out = A.copy()
    sel = (A[0].astype(np.int64) // N) == SIGNED_ANGLE
    out[2, sel] = -A[2, sel]
    return out


def shuffled(A, N, P):
    rng = np.random.default_rng(9)
    perm = np.concatenate([i * N + rng.permutation(N) for i in range(P)])
    out = A.copy()
    out[0] = perm[A[0].astype(np.int64)].astype(np.float32)
    return out


def messy(A, N, P):
    D = dead(A, N, P)
    rows, pix, angle = dead_parts(N, P)
    rng = np.random.default_rng(2000 + 11 * N + P)
    r, c = _rc(D)
    nnz = D.shape[1]
    ncol = N * N
    have = set((r * ncol + c).tolist())
    # duplicates with another value (which of the two is the last is settled by the shuffle below)
    dup = rng.choice(nnz, max(4, nnz // 20), replace=False)
    dups = D[:, dup].copy()
    dups[2] = (dups[2] * np.float32(0.75) + np.float32(0.125)).astype(np.float32)
    # explicit zeros where the ray has no entry: a dead pixel from a live ray, a live pixel from a dead ray and from the dead angle,
    # and one ray in eight on a random pixel
    live_row = int(r[nnz // 3])
    zr = [live_row, live_row, int(rows[0]), angle * N + N // 2]
    zc = [int(pix[0]), int(pix[1]), int(c[nnz // 2]), int(c[nnz // 2 + 1])]
    for row in rng.choice(N * P, max(4, N * P // 8), replace=False):
        col = int(rng.integers(0, ncol))
        if int(row) * ncol + col not in have:
            zr.append(int(row))
            zc.append(col)
    zeros = np.zeros((3, len(zr)), np.float32)
    zeros[0], zeros[1] = zr, zc
    zeros[2, 1::2] = -0.0
    # entries that end as 0: first assignment non-zero, last assignment 0 (never one of the duplicated entries)
    cand = np.setdiff1d(np.arange(nnz), dup)
    kill = rng.choice(cand, 3, replace=False)
    kills = D[:, kill].copy()
    kills[2] = 0.0
    out = np.concatenate([D, dups, zeros, kills], axis=1)
    out = out[:, rng.permutation(out.shape[1])]
    ro, co = _rc(out)
    for k in kill:                                         # the zero assignment must come last
        at = np.nonzero((ro == r[k]) & (co == c[k]))[0]
        assert at.size == 2
        if out[2, at[1]] != 0:
            out[2, at[0]], out[2, at[1]] = out[2, at[1]], out[2, at[0]]
    return np.ascontiguousarray(out)


def family(name, A, N, P):
    return {"dead": dead, "gain": gain, "signed": signed, "messy": messy, "shuffled": shuffled}[name](A, N, P)


def canonical(A, ncol=None):
    """The matrix the engine must hold for the raw triplets A: the last assignment of a (row, col) wins, rows sorted by column,
    explicit zeros kept.  float32 (3, nnz')."""
    r, c = _rc(A)
    ncol = int(c.max()) + 1 if ncol is None else int(ncol)
    key = r * ncol + c
    order = np.argsort(key, kind="stable")
    k = key[order]
    last = np.ones(k.size, bool)
    last[:-1] = k[1:] != k[:-1]
    return np.ascontiguousarray(A[:, order[last]])


def reference(N, angles_deg, A):
    """(``ref64.Matrix`` of ``canonical(A)``, the number of assignments that canonical dropped)."""
    import ref64
    C = canonical(A, N * N)
    M = ref64.Matrix(N, angles_deg, A=C)
    assert M.duplicates == 0
    return M, A.shape[1] - C.shape[1]


def properties(M):
    """What a family reaches, counted on a ``ref64.Matrix``: rows with rowsum == 0 / < 0, pixels with colsum == 0 / <= 0, explicit
    zero weights, the most non-zero rays of one angle through one pixel, whether every pixel's two rays of an angle are neighbours
    (the ART chain's condition), and the (angle, pixel) cells whose only entries are zeros."""
    nz = M.w32 != 0
    ang = M.rows // M.N
    cell = ang[nz] * M.ncol + M.cols[nz]
    ray = (M.rows % M.N)[nz]
    cnt = np.bincount(cell, minlength=M.P * M.ncol)
    lo = np.full(M.P * M.ncol, M.N, np.int64)
    hi = np.full(M.P * M.ncol, -1, np.int64)
    np.minimum.at(lo, cell, ray)
    np.maximum.at(hi, cell, ray)
    two = cnt == 2
    zcell = np.unique(ang[~nz] * M.ncol + M.cols[~nz])
    return dict(rows_zero=int(np.count_nonzero(M.rowsum == 0)), rows_negative=int(np.count_nonzero(M.rowsum < 0)),
                pixels_zero=int(np.count_nonzero(M.colsum == 0)), pixels_nonpositive=int(np.count_nonzero(M.colsum <= 0)),
                zero_weights=int(np.count_nonzero(~nz)), max_rays_per_cell=int(cnt.max()),
                chain=bool(np.all(hi[two] - lo[two] == 1)), zero_only_cells=int(np.count_nonzero(cnt[zcell] == 0)))


def angle_colsum(M, i):
    """The column sums of angle i alone (binary64): the SART divisor of that angle."""
    sel = (M.rows // M.N) == i
    return np.bincount(M.cols[sel], M.vals[sel], M.ncol)


def signs_are_safe(M):
    """True where no row sum, all-angle column sum or per-angle column sum of M lies so close to 0 that a float32 sum in any order
    could take another sign than the binary64 sum: |sum| > gamma(entries + 2) sum |w| wherever sum |w| > 0."""
    import ref64
    aw = np.abs(M.vals)

    def ok(s, a, n):
        return bool(np.all((a == 0) | (np.abs(s) > ref64.gamma(n + 2) * a)))
    good = ok(M.rowsum, np.bincount(M.rows, aw, M.nrow), M.row_nnz) and ok(M.colsum, np.bincount(M.cols, aw, M.ncol), M.col_nnz)
    for i in range(M.P):
        sel = (M.rows // M.N) == i
        good = good and ok(angle_colsum(M, i), np.bincount(M.cols[sel], aw[sel], M.ncol), 2)
    return good


def write_triplets(path, N, P, nchunk, A):
    """The raw triplets as tests/native/user_matrix_check reads them: int32 N, P, nchunk (64-slice chunks of the slab), int64 nnz,
    then the float32 rows, columns and values."""
    with open(path, "wb") as f:
        np.array([N, P, nchunk], np.int32).tofile(f)
        np.array([A.shape[1]], np.int64).tofile(f)
        np.ascontiguousarray(A, np.float32).tofile(f)


# ---- the cases and what the host builders answer on them ---------------------------------------------------------------------------
# (family, geometry of tests/test_gpu_elementwise.py: GEOM)
CASES = [(f, g) for g in ("lin70", "axes45") for f in FAMILIES] + [(f, g) for g in ("repeat", "neg150") for f in ("dead", "messy")]
# The answers of the table builders, as tests/native/user_matrix_check prints them (the CPU test compares this table with the program's
# output; the GPU test asserts the engine's *_ready options and forms against it).  Every builder takes every family but these: the
# resident sweep needs N % 8 == 0, and with the rays shuffled a pixel's two rays are no neighbours (no ART chain, no resident sweep), a
# 16 x 16 tile's ray window exceeds the 26 rows of the SART tile and list back projector; the 40-row window of the tile back projector
# still holds all N <= 40 rays.
_ALL = dict(tables_ok=1, art_chain_ok=1, fp_strip_ok=1, fp_list_ok=1, sart_tile_ok=1, sart_resident_ok=1, bp_tile_ok=1, bp_list_ok=1)
EXPECTED = {}
for _f, _g in CASES:
    EXPECTED[_f, _g] = dict(_ALL, sart_resident_ok=0 if _g == "axes45" else 1)
    if _f == "shuffled":
        EXPECTED[_f, _g].update(art_chain_ok=0, sart_tile_ok=0, sart_resident_ok=0, bp_list_ok=0)


def assert_reaches(name, N, P, props, dropped):
    """The family reaches what it is listed for (counts from ``properties`` and ``reference``)."""
    assert props["max_rays_per_cell"] <= 2, props
    rows, pix, _ = dead_parts(N, P)
    if name in ("dead", "messy"):
        assert props["rows_zero"] == len(rows) and props["pixels_zero"] == len(pix) == 11 and props["rows_negative"] == 0, props
        assert props["chain"], props
    if name == "dead":
        assert dropped == 0 and props["zero_weights"] == 0
    if name == "messy":
        assert dropped >= 4 and props["zero_weights"] >= 7 and props["zero_only_cells"] >= 4, (dropped, props)
    if name == "gain":
        assert props["rows_zero"] == props["rows_negative"] == props["pixels_nonpositive"] == dropped == 0 and props["chain"], props
    if name == "signed":
        assert props["rows_negative"] == N and props["rows_zero"] == 0 and dropped == 0 and props["chain"], props
    if name == "shuffled":
        assert not props["chain"] and props["rows_zero"] == props["rows_negative"] == dropped == 0, props


def idle_pair(A2, N):
    """From the engine's own matrix of TWO angles: angle 0 removed entirely, angle 1 negated -- no ray has a positive sum, so every
    SART, SIRT or ART step must leave max(0, x), exactly."""
    out = A2[:, (A2[0].astype(np.int64) // N) == 1].copy()
    out[2] = -out[2]
    return np.ascontiguousarray(out)


EXPECTED_IDLE = dict(_ALL)          # on lin70's first two angles (N = 32)
