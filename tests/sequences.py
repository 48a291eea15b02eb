"""Tables of the call-sequence tests (tests/test_gpu_sequences.py) and of their closure check (tests/test_sequences_cpu.py).

An engine is a long-lived state machine: projection claims (``vol_version``, ``g_valid``, ``yk_claim``, ``mom``), the ``old_is_recon``
flag, three reduction lanes, pending snapshots and evaluations, scratch shared by unrelated features (``stage``, ``al_part``,
``al_out``, TEMP, YK, the dual fields).  A *disturber* runs every entry point of one feature family on an engine; a *probe* is a short
run of one algorithm that records every intermediate result.  ``probe(used engine)`` must give the bits of ``probe(fresh engine)``.

Importing this module touches neither the library nor a GPU (the CPU closure check imports it).
"""
import contextlib
import os

import numpy as np

from tomo_tv_amd._lib import (S_DD, S_DIFF, SINO_B, SINO_G, SINO_PUBLIC, SINO_USER0, VOL_RECON, VOL_RECON_OLD, VOL_TEMP, VOL_USER0,
                              VOL_YK)

F32 = np.float32
FP_LIST, BP_LIST, SART_ANGLE, SART_TILE, SART_RESIDENT = 3, 2, 0, 1, 2

# A: the geometry of the pdhg isolation test.  B: whole 128-slice pieces, so that the list projectors run, and the resident and tile
# sweeps.  C: A as a cube -- tomo_volume_cross refuses anything else, so the dual-axis disturber runs there.
GEOM = {"A": dict(n=32, nx=6, ang=np.linspace(-70, 70, 9), lists=False),
        "B": dict(n=64, nx=128, ang=np.linspace(-70, 70, 16), lists=True),
        "C": dict(n=32, nx=32, ang=np.linspace(-70, 70, 9), lists=False)}
THR, GREYS = np.array([0.5, 1.5], F32), np.array([0.0, 1.0, 2.0], F32)


@contextlib.contextmanager
def _env(**kw):
    saved = {k: os.environ.get(k) for k in kw}
    os.environ.update(kw)
    try:
        yield
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def new_engine(gid, nx=None, n=None, ang=None):
    from tomo_tv_amd.engine import tomoengine
    g = GEOM[gid]
    args = (nx or g["nx"], n or g["n"], np.asarray(g["ang"] if ang is None else ang) * np.pi / 180)
    if g["lists"] and nx is None and n is None:
        with _env(TOMO_FP_STRIP="1", TOMO_FP_LIST="1"):
            return tomoengine(*args)
    return tomoengine(*args)


def phantom(nx, n):
    """Two boxes of different height per slice on a zero background (the block phantom of the pdhg tests): grey levels 0, 1, 2."""
    x = np.zeros((nx, n, n), F32)
    for s in range(nx):
        a = n // 4 + (s % 3)
        x[s, a:a + n // 3, n // 5:n // 5 + n // 2] = 1.0
        x[s, n // 2:n // 2 + n // 4, n // 2 + (s % 2):n // 2 + n // 3] = 2.0
    return x


def user_volume(nx, n, seed):
    return np.random.default_rng(seed).uniform(0.25, 1.75, (nx, n, n)).astype(F32)


def shifts_for(P, seed=3):
    return np.random.default_rng(seed).uniform(-2.5, 2.5, (P, 2)).astype(F32)


def affine_for(P, n, nx):
    """A small in-plane rotation about the image centre plus a sub-pixel shift, one matrix per projection."""
    m = np.zeros((P, 6))
    for a in range(P):
        t = np.deg2rad(1.5 + 0.25 * a)
        c, s, cr, cs = np.cos(t), np.sin(t), (n - 1) / 2, (nx - 1) / 2
        m[a] = (c, -s, cr - c * cr + s * cs + 0.3, s, c, cs - s * cr - c * cs - 0.2)
    return m


# ---- disturbers: fn(engine, gid, b) -> True when SINO_B was written (the harness then sets the tilt series again) -----------------------
def d_pdhg_precond(e, gid, b):
    e.pdhg_begin()
    e.pdhg(2, 0.125, precond=True, slot=S_DIFF)
    U = VOL_USER0 + 10
    e.pdhg_tv_step(U, U + 1, U + 2, U + 3, lam=0.1, precond=True, slot=S_DIFF)
    e.pdhg_sino_dual(SINO_USER0 + 6, SINO_G, SINO_B, precond=True)


def d_pdhg_scalar(e, gid, b):
    e.pdhg_begin()
    e.pdhg(2, 0.125, precond=False, ratio=0.5)
    U = VOL_USER0 + 10
    e.pdhg_tv_step(U, U + 1, U + 2, U + 3, sigma=0.3, tau=0.2, lam=0.1, precond=False)
    e.pdhg_sino_dual(SINO_USER0 + 6, SINO_G, SINO_B, sigma=0.07, precond=False)


def d_dart(e, gid, b):
    e.SIRT(3)
    n6 = e.dart_classify(THR, connectivity=6, seed=1, free_fraction=0.1)
    n26 = e.dart_classify(THR, connectivity=26, seed=2, free_fraction=0.2)
    assert n6[1] > 0 and n26[1] >= n6[1], (n6, n26)          # the disturber is not vacuous: there is a boundary
    e.dart_arm(2, GREYS)
    e.dart_restore(GREYS)
    e.dart_smooth(VOL_RECON, VOL_USER0 + 7, 0.3)
    e.dart_class_stats(THR)
    e.dart_state()
    e.dart_restore(GREYS, everywhere=True)


def xcorr_shifts(e):
    """3, then the widest window the engine takes (16 where min(Nray, Nslice) allows it), then 3 again: al_part regrows and is then
    used while larger than needed."""
    return (3, min(16, min(e.Ny, e.Nslice_) - 1), 3)


def align_calls(e):
    """Every alignment entry point; -> the results, for the tests that compare them."""
    out = {"moments": e.sino_moments(SINO_B)}
    e.forward_projection()
    for k, S in enumerate(xcorr_shifts(e)):
        out[f"xcorr{k}"] = e.sino_xcorr(SINO_B, SINO_G, S)
    sh = shifts_for(e.Nproj)
    e.sino_shift(SINO_B, SINO_USER0 + 1, sh, wrap=False)
    e.sino_shift(SINO_B, SINO_USER0 + 2, sh, wrap=True)
    e.sino_affine(SINO_B, SINO_USER0 + 3, affine_for(e.Nproj, e.Ny, e.Nslice_))
    out["profile"] = e.sino_axis_profile(SINO_B)
    for k in (1, 2, 3):
        out[f"sino{k}"] = e._sino(SINO_USER0 + k)
    return out


def d_align(e, gid, b):
    e.SIRT(1)
    align_calls(e)


def d_bin(e, gid, b):
    from tomo_tv_amd.engine import tomoengine
    g = GEOM[gid]
    e.SIRT(1)
    coarse = e.binned_engine(2)                                # the engine under test as the fine side
    e.bin_sinogram_to(coarse, 2)
    e.bin_volume_to(coarse, 2)
    coarse.prolong_volume_to(e, 2, dst=VOL_USER0 + 8)
    coarse.prolong_volume_to(e, 2)
    fine = tomoengine(2 * g["nx"] - 1, 2 * g["n"], g["ang"] * np.pi / 180)   # ... and as the coarse side (a trailing partial bin)
    fine.set_volume(user_volume(2 * g["nx"] - 1, 2 * g["n"], 21))
    fine.be.c("forward_projection", VOL_RECON, SINO_B)
    fine.bin_sinogram_to(e, 2, dst=SINO_USER0 + 4)
    fine.bin_sinogram_to(e, 2)
    fine.bin_volume_to(e, 2, dst=VOL_USER0 + 9)
    fine.bin_volume_to(e, 2)
    e.prolong_volume_to(fine, 2)
    e.synchronize(), fine.synchronize(), coarse.synchronize()
    return True


def d_dual(e, gid, b):
    from tomo_tv_amd.engine import tomoengine
    g = GEOM[gid]
    other = tomoengine(g["n"], g["n"], np.linspace(-60, 60, 7) * np.pi / 180)
    e.SIRT(1)
    e.cross_volume_to(other)                                   # as the source
    e.cross_axpy_volume_to(other, 0.5, clamp=True)
    other.cross_volume_to(e, dst=VOL_USER0 + 9)                # as the destination
    other.cross_axpy_volume_to(e, 0.25, clamp=False)
    other.cross_volume_to(e)
    e.synchronize(), other.synchronize()


def d_io(e, gid, b):
    import torch
    dev = torch.device("cuda", e.gpuID)
    side = torch.cuda.Stream(dev)
    gen = torch.Generator(device=dev).manual_seed(7)
    with torch.cuda.stream(side):
        v = torch.rand((e.Nslice_, e.Ny, e.Nz), dtype=torch.float64, device=dev, generator=gen)
        s = torch.rand((e.Nslice_, e.Ny, e.Nproj), dtype=torch.float64, device=dev, generator=gen)
        e.set_volume_tensor(v, VOL_USER0 + 4)
        e.set_volume_tensor(v)
        e.get_volume_tensor(VOL_RECON, dtype=torch.float64)
        e.be.set_tilt_series_tensor(s, SINO_PUBLIC, which=SINO_USER0 + 5)
        e.be.set_tilt_series_tensor(s, SINO_PUBLIC, which=SINO_G)
        e.be.set_tilt_series_tensor(s, SINO_PUBLIC, which=SINO_B)
        e.get_projections_tensor(SINO_B, SINO_PUBLIC, dtype=torch.float64)
        e.get_projections_tensor(SINO_G, SINO_PUBLIC, dtype=torch.float64)
    side.synchronize()
    e.synchronize()
    return True


def d_chem(e, gid, b):
    he = new_engine(gid)
    e.be.share_stream_with(he.be)                              # the engine under test carries the elements and owns the stream
    U = VOL_USER0
    for k in range(4):
        e.set_volume(user_volume(e.Nslice_, e.Ny, 30 + k), U + k)
    he.set_volume(user_volume(e.Nslice_, e.Ny, 40), U + 1)
    xv, uv, w = np.array([U, U + 1], np.int32), np.array([U + 2, U + 3], np.int32), np.array([0.7, 1.3], F32)
    e.be.mm_model(xv, w, 1.6, he.be, U)
    e.be.mm_update(xv, uv, w, 1.6, 0.01, 0.1, he.be, U + 1, U)
    e.synchronize()
    he.be.close()


def fista_mid_state(e):
    """initialize_fista, then two rounds of {SIRT step, momentum, cost, projection by linearity}; stops with old_is_recon, yk_claim and
    mom all live (the second tomo_fista_project_yk says it formed A yk)."""
    e.initialize_fista()
    e.SIRT(1)
    e.fista_momentum(0.0)
    e.data_distance()
    e.fista_project_yk()
    e.SIRT(1)
    e.fista_momentum(0.3)
    e.data_distance()
    assert e.fista_project_yk(), "the projection of the extrapolated point was not formed: the state is not the one intended"


def d_fista_mid(e, gid, b):
    fista_mid_state(e)


def d_deferred(e, gid, b):
    e.SIRT(1)
    e.copy_recon()
    e.tv_gd_tracked(3, 0.05, defer=True)                       # the deferred read is never taken
    e.data_distance_begin()
    e.data_distance_end()
    e.be.scalars_snapshot()
    e.be.scalars_snapshot_read()
    e.data_distance_begin()
    e.tv_gd_tracked(2, 0.05, extra=(S_DD,), defer=True)        # ... and one more is left pending for good


DISTURBERS = {"pdhg_precond": d_pdhg_precond, "pdhg_scalar": d_pdhg_scalar, "dart": d_dart, "align": d_align, "bin": d_bin,
              "dual": d_dual, "device_io": d_io, "chemistry": d_chem, "fista_mid": d_fista_mid, "deferred": d_deferred}
CUBE_ONLY = {"dual"}                                           # tomo_volume_cross takes cubes: this row runs at geometry C


def restore_inputs(e, b, wrote_b):
    """The documented inputs of a run, and nothing else: the tilt series where the disturber overwrote it, a zero start, and the
    host-side target switch of the reference's engine (tomoengine.cpp: momentum), which FISTA leaves on by design."""
    if wrote_b:
        e.set_tilt_series(b)
    e.remove_momentum()
    e.restart_recon()


# ---- probes: fn(engine, gid) -> {name: array}; names starting with "s_" are double sums (compared at rtol 1e-12) ---------------------
def _check_projector_forms(e, gid):
    if GEOM[gid]["lists"]:
        assert e.get_option("form_fp") == FP_LIST and e.get_option("form_bp") == BP_LIST, (e.get_option("form_fp"), e.get_option("form_bp"))


def p_sirt(e, gid):
    _check_projector_forms(e, gid)
    o = {}
    e.SIRT(1)
    o["x1"] = e.get_volume()
    o["s_dd1"] = np.array([e.data_distance()])
    e.SIRT(1)                                                  # starts from the claim the cost evaluation left
    o["x2"] = e.get_volume()
    o["s_dd2"] = np.array([e.data_distance()])
    o["g"] = e.get_model_projections()
    return o


def p_cgls(e, gid):
    _check_projector_forms(e, gid)
    o = {}
    e.CGLS(1)
    o["x1"] = e.get_volume()
    o["s_dd1"] = np.array([e.data_distance()])
    e.CGLS(1)
    o["x2"] = e.get_volume()
    return o


def _p_sart(form):
    def probe(e, gid):
        if form == SART_RESIDENT:
            assert e.get_option("sart_resident_ready") == 1
            e.set_option("sart_resident", 1)
        elif form == SART_TILE:
            e.set_option("sart_resident", 0)
        else:
            e.set_option("sart_fused", 0)
        assert e.get_option("form_sart") == form, e.get_option("form_sart")
        o = {}
        e.SART(0.7, 1)
        o["x1"] = e.get_volume()
        e.SART(0.7, 1)
        o["x2"] = e.get_volume()
        if form == SART_RESIDENT:
            assert e.get_option("sart_resident_fallbacks") == 0
        return o
    return probe


def art_order(nrow):
    return np.ascontiguousarray(np.random.default_rng(5).permutation(nrow), dtype=np.int32)


def p_art(e, gid):
    assert e.get_option("art_chain_ready") == 1
    e.be.c("art", 0.6)
    return {"x1": e.get_volume()}


def p_art_random(e, gid):
    from tomo_tv_amd.engine import _ptr
    order = art_order(e.Nrow)
    e.be.c("art_order", 0.6, _ptr(order))
    return {"x1": e.get_volume()}


FISTA_LAM, FISTA_TV = 0.01, 3


def p_fista(e, gid):
    """Three iterations of TomoGPU.fista, step by step: the second gradient step starts from the claim a copy inherits (beta = 0), the
    third from the projection formed by linearity."""
    o, cost, t0 = {}, [], 1.0
    e.initialize_fista()
    for k in range(3):
        e.SIRT(1)
        o[f"step{k}"] = e.get_volume(VOL_YK)
        e.tv_fgp(FISTA_TV, FISTA_LAM, vol=VOL_YK)
        tk = 0.5 * (1 + np.sqrt(1 + 4 * t0 ** 2))
        e.fista_momentum((t0 - 1) / tk)
        t0 = tk
        cost.append(0.5 * e.data_distance() ** 2 + FISTA_LAM * e.tv())
        o[f"done{k}"] = np.array([e.fista_project_yk()])
        o[f"recon{k}"], o[f"yk{k}"], o[f"old{k}"] = e.get_volume(), e.get_volume(VOL_YK), e.get_volume(VOL_RECON_OLD)
    o["s_cost"] = np.array(cost)
    e.remove_momentum()
    return o


def p_asd_pocs(e, gid):
    from tomo_tv_amd.reconstructor import TomoGPU
    g = object.__new__(TomoGPU)
    g.tomo = e
    dd, tv = g.asd_pocs(Niter=2, nTViter=3)
    return {"s_dd": dd, "s_tv": tv, "x": e.get_volume(), "temp": e.get_volume(VOL_TEMP)}


def p_fgp(e, gid):
    o = {}
    e.SIRT(1)
    o["x0"] = e.get_volume()
    o["s_tv1"] = np.array([e.tv_fgp(3, 0.02)])
    o["x1"] = e.get_volume()
    o["s_tv2"] = np.array([e.tv_fgp(3, 0.02)])
    o["x2"] = e.get_volume()
    return o


def p_pdhg(e, gid):
    e.pdhg_begin()
    e.pdhg(2, 0.125, precond=True, slot=S_DIFF)
    return {"x": e.get_volume(), "xbar": e.get_volume(VOL_YK), "s_diff": np.array([e._scalar(S_DIFF)])}


def p_wbp(e, gid):
    _check_projector_forms(e, gid)
    e.initialize_FBP("ram-lak")
    e.FBP(True)
    return {"x": e.get_volume()}


def p_poisson(e, gid):
    _check_projector_forms(e, gid)
    o = {}
    e.SIRT(1)
    o["x0"] = e.get_volume()
    o["s_cost"] = np.array([e.poisson_ML(0.1)])
    o["x1"] = e.get_volume()
    return o


def p_dd(e, gid):
    _check_projector_forms(e, gid)
    o = {}
    e.SIRT(1)
    o["x0"] = e.get_volume()
    o["s_dd"] = np.array([e.data_distance()])
    o["g"] = e.get_model_projections()
    return o


PROBES = {"sirt": p_sirt, "cgls": p_cgls, "sart_resident": _p_sart(SART_RESIDENT), "sart_tile": _p_sart(SART_TILE),
          "sart_angle": _p_sart(SART_ANGLE), "art": p_art, "art_random": p_art_random, "fista": p_fista, "asd_pocs": p_asd_pocs,
          "tv_fgp": p_fgp, "pdhg": p_pdhg, "wbp": p_wbp, "poisson_ml": p_poisson, "data_distance": p_dd}
# the probes whose kernel form differs at geometry B (list projectors, resident / tile sweeps, the tile-fused ART chain)
FORM_PROBES = ("sirt", "cgls", "sart_resident", "sart_tile", "sart_angle", "art", "wbp", "poisson_ml", "data_distance")


def pairs():
    """(geometry, disturber, probe) of section (a): everything at A (the dual row at the cube C), the form-dependent probes again at B
    (without the dual row: B is not a cube)."""
    out = []
    for d in DISTURBERS:
        gid = "C" if d in CUBE_ONLY else "A"
        out += [(gid, d, p) for p in PROBES]
        if d not in CUBE_ONLY:
            out += [("B", d, p) for p in FORM_PROBES]
    return out


# ---- section (c): the writers between a claim and the step that could use it; section (d): the newer reduction users ------------------
CLAIM_VOLUME_WRITERS = ("tomo_dart_restore", "tomo_dart_segment", "tomo_dart_arm", "tomo_dart_smooth", "tomo_volume_bin",
                        "tomo_volume_cross", "tomo_volume_cross_axpy", "tomo_mm_update", "tomo_pdhg", "tomo_set_slice",
                        "tomo_adopt_volumes")
CLAIM_SINO_WRITERS = ("tomo_sino_shift", "tomo_sino_affine", "tomo_sino_bin", "tomo_set_sinogram_device")
LANE_REDUCERS = ("tomo_dart_classify", "tomo_dart_class_stats", "tomo_sino_moments", "tomo_sino_xcorr", "tomo_sino_axis_profile")
# section (c), refused calls: writers that refuse a call for the engine's state (no begin) -- entry (without "tomo_") -> arguments; the
# refusal comes before any claim changes, so the step that follows behaves as on an engine that never made the call
REFUSED_WITHOUT_BEGIN = {"fgp_end": (3,), "fgp_fused_end": (0.02,)}

# ---- the closure table: every `int tomo_*(tomo_engine *...)` of include/tomo_hip.h -------------------------------------------------------
# name -> (classes, note).  Classes: "vol" writes a volume slot, "sino" writes a sinogram slot, "reduce" reduction user, "stage" user
# of the staging buffer, "state" writes buffers of the engine that are no slot (dual fields, halo planes, saved projections) or
# planes of the caller, "query" pure query / lifecycle.  A "vol" / "sino" entry must be in section (c) and EVERY "reduce" entry, a
# writer's too, in section (d), or carry a note that starts with "excluded:" and gives the reason in one line; a "state" entry says in
# a note that starts with "internal:" what it writes.
_OLD_CLAIM = "excluded: predates the claims' tests (test_gpu_parity: test_projection_reuse_is_bit_identical_and_never_stale)"
_OLD_REDUCE = "excluded: a main-lane reduction of the original engine (test_gpu_elementwise_scalars), enqueued in stream order"
_SLAB = "excluded: step form of a sharded slab; engines with a communicator are out of scope (test_gpu_sharded_tv / _pdhg_sharded)"
_IO = "excluded: the device setters' claim test is test_gpu_device_io (left alone by design)"
CLASSIFICATION = {
    "tomo_destroy": ("query", ""), "tomo_set_stream": ("query", ""), "tomo_synchronize": ("query", ""), "tomo_get_device": ("query", ""),
    "tomo_get_dims": ("query", ""), "tomo_get_stream": ("query", ""), "tomo_set_option": ("query", ""), "tomo_get_option": ("query", ""),
    "tomo_lipschitz": ("query", ""), "tomo_row_inner_product": ("query", ""), "tomo_lipschitz_cimmino": ("query", ""),
    "tomo_release_geometry": ("query", ""), "tomo_async_wait": ("query", ""), "tomo_bind_scalar_buffer": ("query", ""),
    "tomo_bind_halo": ("query", ""), "tomo_wait_for": ("query", ""), "tomo_set_slab_edges": ("query", ""),
    "tomo_tv_set_target": ("query", ""), "tomo_bind_fgp_halo": ("query", ""), "tomo_bind_fgp_halo2": ("query", ""),
    "tomo_bind_pdhg_halo": ("query", ""), "tomo_sart_chain_count": ("query", ""), "tomo_profile_enable": ("query", ""),
    "tomo_profile_read": ("query", ""), "tomo_profile_read2": ("query", ""), "tomo_profile_intervals": ("query", ""),
    "tomo_comm_init": ("query", ""), "tomo_comm_share": ("query", ""), "tomo_comm_destroy": ("query", ""), "tomo_comm_info": ("query", ""),
    "tomo_read_scalars": ("query", ""), "tomo_scalars_snapshot": ("query", ""), "tomo_scalars_snapshot_read": ("query", ""),
    "tomo_comm_read_scalars": ("query", ""), "tomo_comm_scalars_snapshot": ("query", ""), "tomo_fista_project_yk": ("state", "internal: the saved projection g_prev and A * yk in g_yk; SINO_G and its claim stay (section (c), FISTA analogue)"),
    "tomo_halo_pack": ("state", "internal: one boundary plane into a device buffer of the caller"), "tomo_halo_pack_both": ("state", "internal: both boundary planes into device buffers of the caller"), "tomo_halo_local": ("state", "internal: the engine's halo planes, from its own volume"), "tomo_halo_from": ("state", "internal: the engine's halo planes, from the neighbours' volumes"),
    "tomo_scalar_sum_from": ("state", "internal: one slot of the scalar buffer"), "tomo_comm_exchange_halo": ("state", "internal: the halo planes, by RCCL"), "tomo_comm_fgp_exchange": ("state", "internal: the FGP planes, by RCCL"),
    "tomo_comm_fgp_exchange2": ("state", "internal: the two-deep FGP planes, by RCCL"), "tomo_comm_pdhg_exchange": ("state", "internal: the pdhg planes, by RCCL"), "tomo_pdhg_slab_pack": ("state", "internal: the send planes of the slab pass"),
    # the staging buffer's users (section (e) runs them in a row)
    "tomo_set_tilt_series": ("sino stage", _OLD_CLAIM), "tomo_set_sinogram": ("sino stage", _OLD_CLAIM),
    "tomo_get_sinogram": ("stage", ""), "tomo_set_volume": ("vol stage", _OLD_CLAIM), "tomo_get_volume": ("stage", ""),
    "tomo_set_slice": ("vol stage", ""), "tomo_get_slice": ("stage", ""), "tomo_sino_proj_max": ("stage", ""),
    "tomo_sino_proj_scale": ("sino stage", "excluded: scales a caller-named slot in place; test_gpu_chemistry covers it next to the claim"),
    "tomo_art_order": ("vol stage", _OLD_CLAIM), "tomo_dart_get_state": ("stage", ""),
    "tomo_sino_shift": ("sino stage", ""), "tomo_sino_affine": ("sino stage", ""),
    # device I/O
    "tomo_set_volume_device": ("vol", _IO), "tomo_get_volume_device": ("query", ""), "tomo_set_sinogram_device": ("sino", ""),
    "tomo_get_sinogram_device": ("query", ""),
    # writers of the original engine
    "tomo_restart_recon": ("vol", _OLD_CLAIM), "tomo_copy_volume": ("vol", _OLD_CLAIM),
    "tomo_copy_volume_from": ("vol", "excluded: section (b) checks it under old_is_recon; the claim follows get_vol like tomo_set_volume"),
    "tomo_adopt_volumes": ("vol", ""), "tomo_forward_projection": ("sino", _OLD_CLAIM), "tomo_back_projection": ("vol", _OLD_CLAIM),
    "tomo_sirt_landweber": ("vol", _OLD_CLAIM), "tomo_sirt_cimmino": ("vol", _OLD_CLAIM), "tomo_sirt": ("vol", _OLD_CLAIM),
    "tomo_sirt_data": ("vol", _OLD_CLAIM), "tomo_sart": ("vol", _OLD_CLAIM), "tomo_sart_data": ("vol", _OLD_CLAIM),
    "tomo_sart_tracked": ("vol reduce", _OLD_CLAIM), "tomo_cgls": ("vol", _OLD_CLAIM), "tomo_fbp": ("vol", _OLD_CLAIM),
    "tomo_art": ("vol", _OLD_CLAIM), "tomo_poisson_ml": ("vol reduce", _OLD_CLAIM), "tomo_poisson_residual": ("sino reduce", _OLD_CLAIM),
    "tomo_scale_volume": ("vol", _OLD_CLAIM), "tomo_positivity": ("vol", _OLD_CLAIM), "tomo_soft_threshold": ("vol", _OLD_CLAIM),
    "tomo_fista_momentum": ("vol", _OLD_CLAIM),
    "tomo_data_distance_sq": ("sino reduce", _OLD_CLAIM), "tomo_data_distance_sq_async": ("sino reduce", _OLD_CLAIM),
    "tomo_diff_norm_sq": ("reduce", _OLD_REDUCE), "tomo_sino_diff_norm_sq": ("reduce", _OLD_REDUCE), "tomo_l1_norm": ("reduce", _OLD_REDUCE),
    # alignment, binning, dual-axis, DART
    "tomo_sino_moments": ("reduce", ""), "tomo_sino_xcorr": ("reduce", ""), "tomo_sino_axis_profile": ("reduce", ""),
    "tomo_sino_bin": ("sino", ""), "tomo_volume_bin": ("vol", ""),
    "tomo_volume_prolong": ("vol", "excluded: test_gpu_bin already holds its claim test (left alone by design)"),
    "tomo_volume_cross": ("vol", ""), "tomo_volume_cross_axpy": ("vol", ""),
    "tomo_dart_classify": ("reduce", ""), "tomo_dart_restore": ("vol", ""), "tomo_dart_segment": ("vol", ""), "tomo_dart_arm": ("vol", ""),
    "tomo_dart_smooth": ("vol", ""), "tomo_dart_class_stats": ("reduce", ""),
    # TV, FGP: writers of the original engine
    "tomo_tv_partial": ("reduce", _OLD_REDUCE), "tomo_tv_grad": ("reduce", _OLD_REDUCE), "tomo_tv_grad_tv": ("reduce", _OLD_REDUCE),
    "tomo_tv_update": ("vol", _OLD_CLAIM), "tomo_tv_update_planes": ("vol", _OLD_CLAIM), "tomo_tv_grad_planes": ("reduce", _OLD_REDUCE),
    "tomo_tv_halo_apply": ("state", "internal: advances the engine's halo planes"), "tomo_tv_update_tracked": ("vol reduce", _OLD_CLAIM), "tomo_fgp_begin": ("state", "internal: clears the FGP dual field P"),
    "tomo_fgp_begin_vol": ("state", "internal: clears the FGP dual field P"), "tomo_fgp_obj": ("state", "internal: the FGP field D (the TV gradient buffer)"), "tomo_fgp_grad": ("state", "internal: the FGP dual field P"), "tomo_fgp_end": ("vol", _OLD_CLAIM),
    "tomo_fgp_fused_begin": ("state", "internal: clears P and fills the send planes"), "tomo_fgp_fused_step": ("state", "internal: the FGP dual field P and the send planes"), "tomo_fgp_fused_step2": ("state", "internal: the FGP dual field P and the send planes"),
    "tomo_fgp_fused_end": ("vol", _OLD_CLAIM), "tomo_fgp_fused_last": ("vol", _OLD_CLAIM), "tomo_tv": ("reduce", _OLD_REDUCE),
    "tomo_tv_gd": ("vol reduce", _OLD_CLAIM), "tomo_tv_gd_tracked": ("vol reduce", _OLD_CLAIM), "tomo_tv_fgp": ("vol reduce", _OLD_CLAIM),
    "tomo_tv_fgp_vol": ("vol reduce", _OLD_CLAIM), "tomo_comm_tv_gd": ("vol reduce", _SLAB),
    # Chambolle-Pock
    "tomo_pdhg_sino_dual": ("sino", "excluded: writes the caller-named dual sinogram; asking for G drops the claim (get_sino), as for every slot accessor"),
    "tomo_pdhg_tv_step": ("vol reduce", "excluded: step form on caller-named slots; tomo_pdhg (section (c)) runs the same pass on RECON"),
    "tomo_pdhg_begin": ("vol", "excluded: writes YK and the engine-owned dual fields only; section (c) runs it before tomo_pdhg"),
    "tomo_pdhg": ("vol reduce", "excluded: (its reduction) the optional step norm is a main-lane sum in stream order, test_gpu_pdhg; the write is in section (c)"), "tomo_pdhg_slab_tv_step": ("vol reduce", _SLAB), "tomo_pdhg_slab_sino_dual": ("sino", _SLAB),
    "tomo_pdhg_slab_begin": ("vol", _SLAB), "tomo_pdhg_slab_iter": ("vol reduce", _SLAB), "tomo_comm_pdhg": ("vol reduce", _SLAB),
    # multimodal
    "tomo_mm_model": ("vol", "excluded: writes the model volume of the OTHER engine; tomo_mm_update (section (c)) writes this engine's"),
    "tomo_mm_update": ("vol", ""),
}
CLASSES = {"vol", "sino", "reduce", "stage", "state", "query"}


def header_prototypes(text):
    """The names of the `int tomo_*(tomo_engine *...)` prototypes in the text of include/tomo_hip.h."""
    import re
    return re.findall(r"^\s*int\s+(tomo_\w+)\s*\(\s*tomo_engine\s*\*", text, re.M)


def closure_errors(names, table=None):
    """What is wrong with the table for these prototype names (an empty list: nothing)."""
    table = CLASSIFICATION if table is None else table
    errs = [f"{n}: no row in tests/sequences.py CLASSIFICATION" for n in names if n not in table]
    errs += [f"{n}: a row without a prototype in the header" for n in table if n not in names]
    covered_c = set(CLAIM_VOLUME_WRITERS) | set(CLAIM_SINO_WRITERS)
    for n, (classes, note) in table.items():
        cl = set(classes.split())
        if not cl or cl - CLASSES:
            errs.append(f"{n}: unknown class in {classes!r}")
        if "query" in cl and len(cl) > 1:
            errs.append(f"{n}: a pure query cannot also be {classes!r}")
        one_line = len(note) > 20 and "\n" not in note
        excluded, internal = note.startswith("excluded:") and one_line, note.startswith("internal:") and one_line
        if note and not (excluded or internal):
            errs.append(f"{n}: a note must be 'excluded: <one-line reason>' or 'internal: <what is written>'")
        if ("state" in cl) != internal:
            errs.append(f"{n}: the class 'state' and a note 'internal: ...' go together")
        if cl & {"vol", "sino"} and n not in covered_c and not excluded:
            errs.append(f"{n}: writes a slot but is neither in section (c) nor excluded with a reason")
        if "reduce" in cl and n not in LANE_REDUCERS and not excluded:
            errs.append(f"{n}: a reduction user that is neither in section (d) nor excluded with a reason")
    errs += [f"{n}: listed in section (c) but not classified as a writer" for n in covered_c
             if n in table and not set(table[n][0].split()) & {"vol", "sino"}]
    errs += [f"{n}: listed in section (d) but not classified as a reduction user" for n in LANE_REDUCERS
             if n in table and "reduce" not in table[n][0].split()]
    return errs
