// engine_fgp.inc -- part of tomo_engine.hip (ONE translation unit: the kernels are templates and asm blocks in headers; the host side is
// split by topic into files that tomo_engine.hip includes in order).  This part: C ABI: FGP-TV prox: the Obj / Grad pair, the fused
// iteration (one, two, and one with the result), the whole-call forms and the plane bindings of a sharded slab.
// The faces of the slab a pass works on, passed to every launcher: global edges of the volume (first / last), or faces inside it, which
// read and write the bound planes (deep: the two-slice-deep set).  The C entries take them from the engine (tomo_set_slab_edges,
// tomo_bind_fgp_halo); the whole-call form works on the whole volume whatever the engine has been told.
struct FgpFaces { int first, last; float *lo, *hi, *send_first, *send_last; bool deep; bool sharded() const { return !(first && last); } };
static FgpFaces fgp_faces(const tomo_engine *e) { return FgpFaces{e->is_first, e->is_last, e->fgp_lo, e->fgp_hi, e->fgp_send_first, e->fgp_send_last, e->fgp_planes2}; }
static const FgpFaces FGP_WHOLE{1, 1, nullptr, nullptr, nullptr, nullptr, false};
static int fgp_need(bool begun, const char *call) { return begun ? TOMO_OK : fail(TOMO_ERR_STATE, std::string(call) + " has not been called"); }

int tomo_bind_fgp_halo(tomo_engine *e, void *lo, void *hi, void *send_first, void *send_last)
{
    NEED(e);
    if (!lo || !hi || !send_first || !send_last) return fail(TOMO_ERR_ARG, "null plane buffer");
    HIPCHK(hipStreamSynchronize(e->stream));
    e->fgp_lo = (float *)lo; e->fgp_hi = (float *)hi; e->fgp_send_first = (float *)send_first; e->fgp_send_last = (float *)send_last; e->fgp_planes2 = false;
    return TOMO_OK;
}

// the two-slice-deep set (k_fgp_fused2<.., SHARDED>): lo 5 planes [P1(-1), A(-1), P2(-1), P3(-1), P1(-2)], hi 8 planes
// [A, P1, P2, P3](nx), [..](nx + 1), send_first 8 planes [A, P1, P2, P3](0), [..](1), send_last 5 planes [P1(nx-1), A(nx-1), P2(nx-1),
// P3(nx-1), P1(nx-2)].  The one-deep planes of tomo_bind_fgp_halo are the prefixes (1 / 4 / 4 / 1), so both step forms run on it.
int tomo_bind_fgp_halo2(tomo_engine *e, void *lo, void *hi, void *send_first, void *send_last)
{
    int rc = tomo_bind_fgp_halo(e, lo, hi, send_first, send_last);
    if (!rc) e->fgp_planes2 = true;
    return rc;
}

// ---- step form: Obj / Grad pair -----------------------------------------------------------------------------------------------------
static int fgp_begin_impl(tomo_engine *e, int vol, bool zero_p)
{
    NEED(e);
    float *d, *p; int rc; if ((rc = get_vol(e, vol, &d))) return rc;
    e->fgp_target = vol;
    if (zero_p) {   // step form: D and P start as zero fields (tv_fgp.cu:216-227); the fused form needs neither
        if ((rc = get_scratch(e, &e->tvg, &d))) return rc;
        HIPCHK(hipMemsetAsync(d, 0, e->vol_elems() * sizeof(float), e->stream));
    }
    for (int i = 0; i < 3; ++i) {
        if ((rc = get_scratch(e, &e->fgp_p[i], &p))) return rc;
        if (zero_p) HIPCHK(hipMemsetAsync(p, 0, e->vol_elems() * sizeof(float), e->stream));
    }
    return TOMO_OK;
}
int tomo_fgp_begin(tomo_engine *e) { return fgp_begin_impl(e, TOMO_VOL_RECON, true); }
int tomo_fgp_begin_vol(tomo_engine *e, int vol) { return fgp_begin_impl(e, vol, true); }

// d <- a - lambda div P; lo: the plane below slice 0 where the slab's first face is inside the volume
static int fgp_obj(tomo_engine *e, const float *a, float *d, const float *lo, int first, float lambda)
{
    ProfScope ps(e, TOMO_K_FGP_OBJ);
    hipLaunchKernelGGL(k_fgp_obj, dim3(tv_grid(e)), dim3(256), 0, e->stream, a, d, e->fgp_p[0], e->fgp_p[1], e->fgp_p[2], lo, first, lambda, e->n, e->nx, e->sx);
    LAUNCHCHK();
    return TOMO_OK;
}
static int fgp_grad(tomo_engine *e, const float *hi, int last, float lambda)
{
    ProfScope ps(e, TOMO_K_FGP_GRAD);
    hipLaunchKernelGGL(k_fgp_grad, dim3(tv_grid(e)), dim3(256), 0, e->stream, e->tvg, e->fgp_p[0], e->fgp_p[1], e->fgp_p[2], hi, last, 1.0f / (26.0f * lambda), e->n, e->nx, e->sx);
    LAUNCHCHK();
    return TOMO_OK;
}
// the prox result lands in the volume: D is the zero-filled buffer when no iteration ran, exactly like d_update (tv_fgp.cu:223,272)
static int fgp_end(tomo_engine *e)
{
    if (int rc = fgp_need(e->tvg, "tomo_fgp_begin")) return rc;
    e->claims.prox_landed(e->fgp_target);
    HIPCHK(hipMemcpyAsync(e->vol[e->fgp_target], e->tvg, e->vol_elems() * sizeof(float), hipMemcpyDeviceToDevice, e->stream));
    return TOMO_OK;
}
int tomo_fgp_obj(tomo_engine *e, float lambda)
{
    NEED(e);
    if (int rc = fgp_need(e->tvg && e->fgp_p[2], "tomo_fgp_begin")) return rc;
    return fgp_obj(e, e->vol[e->fgp_target], e->tvg, e->halo_lo, e->is_first, lambda);
}
int tomo_fgp_grad(tomo_engine *e, float lambda)
{
    NEED(e);
    if (int rc = fgp_need(e->tvg && e->fgp_p[2], "tomo_fgp_begin")) return rc;
    return fgp_grad(e, e->halo_hi, e->is_last, lambda);
}
int tomo_fgp_end(tomo_engine *e, int iters) { (void)iters; NEED(e); return fgp_end(e); }

// ---- fused FGP iteration, step form (single slab and slab-sharded) ------------------------------------------------------
static int fgp_fused_begin(tomo_engine *e, int vol, const FgpFaces &fc)
{
    if (fc.sharded() && !fc.lo) return fail(TOMO_ERR_STATE, "slab-sharded fused FGP needs tomo_bind_fgp_halo");
    int rc; if ((rc = fgp_begin_impl(e, vol, false))) return rc;     // the first iteration takes P = 0 as known
    float *q; for (int i = 0; i < 3; ++i) if ((rc = get_scratch(e, &e->fgp_q[i], &q))) return rc;
    if (fc.sharded()) {
        auto pack = [&](float *dst, int slice) { hipLaunchKernelGGL(k_halo_pack, dim3((unsigned)((e->npix + 255) / 256)), dim3(256), 0, e->stream, e->vol[vol], dst, (int)e->npix, e->sx, slice); };
        pack(fc.send_first, 0);           // plane 0 of send_first: the first slice of the prox input (constant over the call)
        // the deep set: A of slice 1 (send_first plane 4) and of the last slice (send_last plane 1)
        if (fc.deep && e->nx >= 2) { pack(fc.send_first + 4 * e->npix, 1); pack(fc.send_last + e->npix, e->nx - 1); }
        LAUNCHCHK();
    }
    return TOMO_OK;
}

// What the fused passes share besides the "begun?" check (fgp_need): the launch on fgp_grid, reading P and writing Q, which then change
// places (final: the pass wrote the call's result instead, into Q1, which changes places with the target's buffer: the old one is scratch now).
extern "C++" template <class K, class Edge>      // (this file is included inside the extern "C" block of the ABI)
static int launch_fgp_fused(tomo_engine *e, int prof, K kernel, int tz, int nchunk, float lambda, int first_iteration, const Edge &ed, bool final = false)
{
    const int yseg = 32;                                 // (16 ... 64 within 3 %; 128 and more lose to the tail)
    {
        ProfScope ps(e, prof);
        hipLaunchKernelGGL(kernel, dim3(fgp_grid(e->n, nchunk, tz, yseg)), dim3(256), 0, e->stream, e->vol[e->fgp_target], e->fgp_p[0], e->fgp_p[1], e->fgp_p[2],
                           e->fgp_q[0], e->fgp_q[1], e->fgp_q[2], lambda, 1.0f / (26.0f * lambda), e->n, e->nx, e->sx, yseg, first_iteration ? 1 : 0, ed);
    }
    LAUNCHCHK();
    if (final) { std::swap(e->vol[e->fgp_target], e->fgp_q[0]); e->claims.prox_landed(e->fgp_target); }
    else for (int k = 0; k < 3; ++k) std::swap(e->fgp_p[k], e->fgp_q[k]);
    return TOMO_OK;
}

static int fgp_fused_step(tomo_engine *e, float lambda, int first_iteration, const FgpFaces &fc)
{
    if (int rc = fgp_need(e->fgp_q[2] && e->fgp_p[2], "tomo_fgp_fused_begin")) return rc;
    const bool sh = fc.sharded();
    const FgpEdge ed{sh ? fc.lo : nullptr, sh ? fc.hi : nullptr, sh ? fc.send_first : nullptr, sh ? fc.send_last : nullptr, fc.first, fc.last};
    return sh ? launch_fgp_fused(e, TOMO_K_FGP_GRAD, k_fgp_fused<true>, TVL_TZ, e->sxc / 64, lambda, first_iteration, ed)
              : launch_fgp_fused(e, TOMO_K_FGP_GRAD, k_fgp_fused<false>, TVL_TZ, e->sxc / 64, lambda, first_iteration, ed);
}

// two iterations in one pass (k_fgp_fused2: P stays on chip between them).  A sharded slab needs the two-slice-deep planes
// (tomo_bind_fgp_halo2, exchanged once before the call: tomo_comm_fgp_exchange2) and at least two slices on EVERY slab of the ring.
static int fgp_fused_step2(tomo_engine *e, float lambda, int first_iteration, const FgpFaces &fc)
{
    if (int rc = fgp_need(e->fgp_q[2] && e->fgp_p[2], "tomo_fgp_fused_begin")) return rc;
    const int nchunk = (e->nx + F2_SC - 1) / F2_SC;
    if (!fc.sharded()) return launch_fgp_fused(e, TOMO_K_FGP_GRAD, k_fgp_fused2<false, false>, F2_TZ, nchunk, lambda, first_iteration, Fgp2Edge{});
    if (!fc.deep || !fc.lo) return fail(TOMO_ERR_STATE, "a sharded tomo_fgp_fused_step2 needs the two-slice-deep planes (tomo_bind_fgp_halo2)");
    if (e->nx < 2) return fail(TOMO_ERR_STATE, "a sharded tomo_fgp_fused_step2 needs at least two slices per slab");
    return launch_fgp_fused(e, TOMO_K_FGP_GRAD, k_fgp_fused2<false, true>, F2_TZ, nchunk, lambda, first_iteration, Fgp2Edge{fc.lo, fc.hi, fc.send_first, fc.send_last, fc.first, fc.last});
}

// one more iteration AND the call's result in one pass (k_fgp_fused2<true>): D of the iteration's P, which is never stored.  Whole-volume slabs only.
static int fgp_fused_last(tomo_engine *e, float lambda, int first_iteration, const FgpFaces &fc)
{
    if (int rc = fgp_need(e->fgp_q[2] && e->fgp_p[2], "tomo_fgp_fused_begin")) return rc;
    if (fc.sharded()) return fail(TOMO_ERR_STATE, "tomo_fgp_fused_last is for a slab that is the whole volume");
    if (e->fgp_target < 0 || e->fgp_target >= TOMO_VOL_SLOTS) return fail(TOMO_ERR_STATE, "no target volume");
    return launch_fgp_fused(e, TOMO_K_FGP_OBJ, k_fgp_fused2<true, false>, F2_TZ, (e->nx + F2_SC - 1) / F2_SC, lambda, first_iteration, Fgp2Edge{}, true);
}

// the last iteration only needs D (tv_fgp.cu:272), written straight over the target volume
static int fgp_fused_end(tomo_engine *e, float lambda, const FgpFaces &fc)
{
    if (int rc = fgp_need(e->fgp_p[2], "tomo_fgp_fused_begin")) return rc;
    e->claims.prox_landed(e->fgp_target);
    float *a = e->vol[e->fgp_target];
    return fgp_obj(e, a, a, fc.sharded() ? fc.lo : e->halo_lo, fc.first, lambda);
}

int tomo_fgp_fused_begin(tomo_engine *e, int vol) { NEED(e); return fgp_fused_begin(e, vol, fgp_faces(e)); }
int tomo_fgp_fused_step(tomo_engine *e, float lambda, int first_iteration) { NEED(e); return fgp_fused_step(e, lambda, first_iteration, fgp_faces(e)); }
int tomo_fgp_fused_step2(tomo_engine *e, float lambda, int first_iteration) { NEED(e); return fgp_fused_step2(e, lambda, first_iteration, fgp_faces(e)); }
int tomo_fgp_fused_last(tomo_engine *e, float lambda, int first_iteration) { NEED(e); return fgp_fused_last(e, lambda, first_iteration, fgp_faces(e)); }
int tomo_fgp_fused_end(tomo_engine *e, float lambda) { NEED(e); return fgp_fused_end(e, lambda, fgp_faces(e)); }

// ---- whole-call form: the slab is the whole volume ----------------------------------------------------------------------------------
int tomo_tv_fgp(tomo_engine *e, int iters, float lambda) { return tomo_tv_fgp_vol(e, TOMO_VOL_RECON, iters, lambda); }
int tomo_tv_fgp_vol(tomo_engine *e, int vol, int iters, float lambda)
{
    int rc = tomo_tv(e, vol, 1e-6f); if (rc) return rc;    // tv_fgp.cu:170-189,231-238 (refuses a null engine)
    if (e->fgp_fused && iters > 1) {
        // iterations 0..iters-2: one fused kernel each (D stays on chip); the last iteration only needs D
        rc = fgp_fused_begin(e, vol, FGP_WHOLE);
        int i = 0;
        if (e->fgp_pair) for (; i + 2 < iters && !rc; i += 2) rc = fgp_fused_step2(e, lambda, i == 0, FGP_WHOLE);     // pairs, P kept on chip between
        if (e->fgp_pair && i + 2 == iters) return rc ? rc : fgp_fused_last(e, lambda, i == 0, FGP_WHOLE);              // an odd iteration out and the result: one pass
        for (; i + 1 < iters && !rc; ++i) rc = fgp_fused_step(e, lambda, i == 0, FGP_WHOLE);
        return rc ? rc : fgp_fused_end(e, lambda, FGP_WHOLE);
    }
    rc = fgp_begin_impl(e, vol, true);
    for (int i = 0; i < iters && !rc; ++i) if (!(rc = fgp_obj(e, e->vol[e->fgp_target], e->tvg, e->halo_lo, 1, lambda))) rc = fgp_grad(e, e->halo_hi, 1, lambda);
    return rc ? rc : fgp_end(e);
}
