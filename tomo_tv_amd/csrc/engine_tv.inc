// engine_tv.inc -- part of tomo_engine.hip (ONE translation unit: the kernels are templates and asm blocks in headers; the host side is
// split by topic into files that tomo_engine.hip includes in order).  This part: C ABI: TV value / gradient / descent, the sub-slab group's halo calls, FGP (Obj / Grad pair, fused steps, whole-call forms).

// ---- TV -----------------------------------------------------------------------------------------------------------------
static int field_ptr(tomo_engine *e, int field, float **out)
{
    if (field == TOMO_FIELD_FGP_D) return get_scratch(e, &e->tvg, out);
    if (field == TOMO_FIELD_FGP_P1) return get_scratch(e, &e->fgp_p[0], out);
    return get_vol_ro(e, field, out);   // halo packs and fills only read
}

int tomo_bind_halo(tomo_engine *e, void *device_lo, void *device_hi)
{
    NEED(e);
    HIPCHK(hipStreamSynchronize(e->stream));
    e->halo_lo = device_lo ? (float *)device_lo : e->halo_lo_own;
    e->halo_hi = device_hi ? (float *)device_hi : e->halo_hi_own;
    return TOMO_OK;
}

int tomo_halo_pack(tomo_engine *e, int field, int last, void *device_dst)
{
    NEED(e);
    float *x; int rc; if ((rc = field_ptr(e, field, &x))) return rc;
    if (!device_dst) return fail(TOMO_ERR_ARG, "null destination");
    hipLaunchKernelGGL(k_halo_pack, dim3((unsigned)((e->npix + 255) / 256)), dim3(256), 0, e->stream, x, (float *)device_dst, (int)e->npix, e->sx, last ? e->nx - 1 : 0);
    LAUNCHCHK();
    return TOMO_OK;
}

int tomo_halo_pack_both(tomo_engine *e, int field, void *first_plane, void *last_plane)
{
    NEED(e);
    float *x; int rc; if ((rc = field_ptr(e, field, &x))) return rc;
    if (!first_plane || !last_plane) return fail(TOMO_ERR_ARG, "null destination");
    // k_halo_wrap(x, lo, hi): lo <- last slice, hi <- slice 0
    hipLaunchKernelGGL(k_halo_wrap, dim3((unsigned)((e->npix + 255) / 256)), dim3(256), 0, e->stream, x, (float *)last_plane, (float *)first_plane, (int)e->npix, e->sx, e->nx);
    LAUNCHCHK();
    return TOMO_OK;
}

int tomo_halo_local(tomo_engine *e, int field)
{
    NEED(e);
    float *x; int rc; if ((rc = field_ptr(e, field, &x))) return rc;
    // below slice 0 sits the last slice, above the last slice sits slice 0
    hipLaunchKernelGGL(k_halo_wrap, dim3((unsigned)((e->npix + 255) / 256)), dim3(256), 0, e->stream, x, e->halo_lo, e->halo_hi, (int)e->npix, e->sx, e->nx);
    LAUNCHCHK();
    return TOMO_OK;
}

// ---- several slab engines on ONE device (tomo_tv_amd/engine.py: _GroupBackend) ------------------------------------------------
// A slab can be run as K sub-slabs, each a complete engine with its own allocations and stream: the dependent launch chains of
// the sub-slabs (a SART sweep is 180 of them) then fill each other's launch gaps and kernel tails.  Slices only couple in the 3-D
// TV stencils and in the global sums; these three calls are what the coupling needs.

// e's stream waits for everything enqueued on other's stream so far
int tomo_wait_for(tomo_engine *e, tomo_engine *other)
{
    NEED(e);
    if (!other) return fail(TOMO_ERR_ARG, "null engine");
    if (other->device != e->device) return fail(TOMO_ERR_ARG, "engines on different devices");
    if (other == e || other->stream == e->stream) return TOMO_OK;
    if (!other->ev_peer) HIPCHK(hipEventCreateWithFlags(&other->ev_peer, hipEventDisableTiming));
    HIPCHK(hipEventRecord(other->ev_peer, other->stream));
    HIPCHK(hipStreamWaitEvent(e->stream, other->ev_peer, 0));
    return TOMO_OK;
}

// e's halo planes from its neighbours' volumes: lo = LAST slice of lo_src's field, hi = FIRST slice of hi_src's field (the
// caller orders the streams: tomo_wait_for).  The ring of sub-slabs of one volume gives the periodic wrap of ctvlib.cpp:348,421.
int tomo_halo_from(tomo_engine *e, int field, tomo_engine *lo_src, tomo_engine *hi_src)
{
    NEED(e);
    if (!lo_src || !hi_src) return fail(TOMO_ERR_ARG, "null engine");
    if (lo_src->n != e->n || hi_src->n != e->n || lo_src->device != e->device || hi_src->device != e->device) return fail(TOMO_ERR_ARG, "engines differ in image size or device");
    float *xl, *xh; int rc;
    if ((rc = field_ptr(lo_src, field, &xl)) || (rc = field_ptr(hi_src, field, &xh))) return rc;
    dim3 grid((unsigned)((e->npix + 255) / 256));
    hipLaunchKernelGGL(k_halo_pack, grid, dim3(256), 0, e->stream, xl, e->halo_lo, (int)e->npix, lo_src->sx, lo_src->nx - 1);
    hipLaunchKernelGGL(k_halo_pack, grid, dim3(256), 0, e->stream, xh, e->halo_hi, (int)e->npix, hi_src->sx, 0);
    LAUNCHCHK();
    return TOMO_OK;
}

// scalar dst_slot of e = sum over the engines' src_slot partial sums, on e's stream (caller orders the streams)
int tomo_scalar_sum_from(tomo_engine *e, int dst_slot, tomo_engine **srcs, int n, int src_slot)
{
    NEED(e);
    if (!srcs || n < 1 || n > 8 || dst_slot < 0 || dst_slot >= TOMO_S_COUNT || src_slot < 0 || src_slot >= TOMO_S_COUNT) return fail(TOMO_ERR_ARG, "bad argument");
    SumSrc s{};
    s.n = n;
    for (int i = 0; i < n; ++i) { if (!srcs[i] || srcs[i]->device != e->device) return fail(TOMO_ERR_ARG, "bad source engine"); s.p[i] = srcs[i]->d_scal + src_slot; }
    hipLaunchKernelGGL(k_sum_doubles, dim3(1), dim3(1), 0, e->stream, s, e->d_scal + dst_slot);
    LAUNCHCHK();
    return TOMO_OK;
}

int tomo_set_slab_edges(tomo_engine *e, int is_first, int is_last)
{
    if (!e) return fail(TOMO_ERR_ARG, "null engine");
    e->is_first = is_first ? 1 : 0; e->is_last = is_last ? 1 : 0;
    return TOMO_OK;
}

static int tv_grid(tomo_engine *e)
{
    int64_t items = e->npix * (e->sx / 64);
    return (int)std::min<int64_t>((items + 3) / 4, 256 * 16);
}

// TV of a volume with the halo planes as they are (step form: the caller has exchanged or wrapped them)
int tomo_tv_partial(tomo_engine *e, int vol, float eps)
{
    NEED(e);
    float *x; int rc; if ((rc = get_vol_ro(e, vol, &x))) return rc;
    Halo h{e->halo_lo, e->halo_hi};
    if (e->tv_lds != 8 && e->tv_lds != 1) {   // direct-global stencil (reads x twice)
        if ((rc = reduce_begin(e))) return rc;
        hipLaunchKernelGGL(k_tv_value, dim3(tv_grid(e)), dim3(256), 0, e->stream, x, h, e->d_part, eps, e->n, e->nx, e->sx);
        LAUNCHCHK();
        return reduce_end(e, TOMO_S_TV);
    }
    // the march of the gradient kernels without their gradient half: x is read once
    if (!e->d_part_tv) { if ((rc = dev_alloc(e, ENGINE, (void **)&e->d_part_tv, NPART * sizeof(double), true))) return rc; }
    if ((rc = reduce_begin(e, tv_lane(e)))) return rc;
    const int yseg = 32;
    if (e->tv_lds == 1 && e->tv_march4 && e->nx % 64 == 0 && e->n % 8 == 0) {
        // the value alone from the branch-free march (round 3): the R loop without the gradient half
        hipLaunchKernelGGL((k_tv_march4<8, true, TVM_VALUE, false>), dim3(tv_march_grid(e->n, 8, e->sxc / 64, (e->n + yseg - 1) / yseg)), dim3(256), 0, e->stream, x, h, (double *)nullptr, eps, e->n, e->nx, e->sx, yseg, e->d_part_tv, TvUpd{});
    } else if (e->tv_lds == 1) {
        hipLaunchKernelGGL((k_tv_grad_reg<8, true, false>), dim3(tv_march_grid(e->n, 8, e->sxc / 64, (e->n + yseg - 1) / yseg)), dim3(256), 0, e->stream, x, h, (float *)nullptr, (double *)nullptr, eps, e->n, e->nx, e->sx, yseg, e->d_part_tv, TvUpd{});
    } else {
        dim3 grid((unsigned)(((e->n + 7) / 8) * (e->sxc / 64)), (unsigned)((e->n + yseg - 1) / yseg));
        hipLaunchKernelGGL((k_tv_grad_lds<8, true, false>), grid, dim3(256), 0, e->stream, x, h, (float *)nullptr, (double *)nullptr, eps, e->n, e->nx, e->sx, yseg, e->d_part_tv);
    }
    LAUNCHCHK();
    return reduce_end(e, tv_lane(e), TOMO_S_TV);
}

// Rows a wave of the register march walks.  32 at a full slab (8 chunks x 64 z-blocks x 16 segments = 8192 waves at 512^3);
// a thin slab of a multi-GPU run has too few waves at that length (64 slices: 1024 waves, 4 per CU), so the segments
// shrink until there are ~8 waves per SIMD lane group again -- the 2 halo rows a segment re-reads cost less than the idle CUs.
static int tv_rows_per_wave(const tomo_engine *e, int tz)
{
    if (e->tv_yseg > 0) return e->tv_yseg;
    const int64_t cols = (int64_t)((e->n + tz - 1) / tz) * (e->sxc / 64);
    int yseg = 32;
    while (yseg > TV_YSEG_MIN && cols * ((e->n + yseg - 1) / yseg) < TV_WAVES_WANTED) yseg >>= 1;
    return yseg;
}

static int tv_grad_impl(tomo_engine *e, float eps, bool with_tv, float *g_first = nullptr, float *g_last = nullptr)
{
    NEED(e);
    float *x, *g; int rc;
    if ((rc = get_vol(e, e->tv_target, &x))) return rc;
    if ((rc = get_scratch(e, &e->tvg, &g))) return rc;
    if ((rc = reduce_begin(e))) return rc;
    Halo h{e->halo_lo, e->halo_hi};
    if ((g_first || g_last) && !(e->tv_lds == 1 && e->tv_recompute)) return fail(TOMO_ERR_STATE, "gradient planes need the recompute form of the TV march (tv_lds = 1, tv_recompute = 1)");
    if (with_tv && e->tv_lds != 8 && e->tv_lds != 1) with_tv = false;
    if (with_tv) {
        if (!e->d_part_tv) { if ((rc = dev_alloc(e, ENGINE, (void **)&e->d_part_tv, NPART * sizeof(double), true))) return rc; }
        if ((rc = reduce_begin(e, tv_lane(e)))) return rc;
    }
    {
        ProfScope ps(e, TOMO_K_TV_GRAD);
        e->tv_last_eps = eps;
        double *part_tv = with_tv ? e->d_part_tv : nullptr;
        if (e->tv_lds == 1 && e->tv_recompute) {   // sum g^2 (and TV) only: the update pass re-evaluates g (TVM_UPDATE)
            TvUpd gp{};
            gp.wrap_lo = g_last; gp.wrap_hi = g_first;      // g's last / first slice (slab-sharded descent), or null
            const int tz = e->tv_tz == 4 ? 4 : 8, yseg = tv_rows_per_wave(e, tz);
            dim3 grid(tv_march_grid(e->n, tz, e->sxc / 64, (e->n + yseg - 1) / yseg));
            const bool edge = e->nx % 64 != 0 || e->n % 8 != 0;      // lanes without a voxel exist: the march's predicated form
            with_flag(with_tv, [&](auto W) {
                if (tz == 8 && e->tv_march4) with_flag(edge, [&](auto E) {
                    hipLaunchKernelGGL((k_tv_march4<8, W(), TVM_NORM, E()>), grid, dim3(256), 0, e->stream, x, h, e->d_part, eps, e->n, e->nx, e->sx, yseg, part_tv, gp);
                });
                else with_int<4, 8>(tz, [&](auto TZ) {
                    hipLaunchKernelGGL((k_tv_grad_reg<TZ(), W(), true, TVM_NORM>), grid, dim3(256), 0, e->stream, x, h, (float *)nullptr, e->d_part, eps, e->n, e->nx, e->sx, yseg, part_tv, gp);
                });
            });
        } else if (e->tv_lds == 1) {   // register march (k_tv_grad_reg): one wave per (z block, chunk, y segment)
            int yseg = 32;   // 8 .. 64 rows per wave measured the same; longer segments leave too few waves
            dim3 grid(tv_march_grid(e->n, 8, e->sxc / 64, (e->n + yseg - 1) / yseg));
            with_flag(with_tv, [&](auto W) {
                hipLaunchKernelGGL((k_tv_grad_reg<8, W()>), grid, dim3(256), 0, e->stream, x, h, g, e->d_part, eps, e->n, e->nx, e->sx, yseg, part_tv, TvUpd{});
            });
        } else if (e->tv_lds) {
            int yseg = 32;
            if (e->tv_lds == 16) {      // (no folded value: with_tv is off)
                dim3 grid((unsigned)(((e->n + 15) / 16) * (e->sxc / 64)), (unsigned)((e->n + yseg - 1) / yseg));
                hipLaunchKernelGGL((k_tv_grad_lds<16, false>), grid, dim3(256), 0, e->stream, x, h, g, e->d_part, eps, e->n, e->nx, e->sx, yseg, (double *)nullptr);
            } else {
                dim3 grid((unsigned)(((e->n + 7) / 8) * (e->sxc / 64)), (unsigned)((e->n + yseg - 1) / yseg));
                with_flag(with_tv, [&](auto W) {
                    hipLaunchKernelGGL((k_tv_grad_lds<8, W()>), grid, dim3(256), 0, e->stream, x, h, g, e->d_part, eps, e->n, e->nx, e->sx, yseg, part_tv);
                });
            }
        } else {
            hipLaunchKernelGGL(k_tv_grad, dim3(tv_grid(e)), dim3(256), 0, e->stream, x, h, g, e->d_part, eps, e->n, e->nx, e->sx);
        }
    }
    LAUNCHCHK();
    if (with_tv && (rc = reduce_end(e, tv_lane(e), TOMO_S_TV))) return rc;
    return reduce_end(e, TOMO_S_GNORM);
}

int tomo_tv_set_target(tomo_engine *e, int vol)
{
    NEED(e);
    float *x;
    int rc = get_vol(e, vol, &x);
    if (rc) return rc;
    e->tv_target = vol;
    return TOMO_OK;
}

int tomo_tv_grad(tomo_engine *e, float eps) { return tv_grad_impl(e, eps, false); }
int tomo_tv_grad_tv(tomo_engine *e, float eps)
{
    if (e && e->tv_lds != 8 && e->tv_lds != 1) {   // kernels without the folded value: a separate pass
        int rc = tomo_tv_partial(e, e->tv_target, eps);
        return rc ? rc : tv_grad_impl(e, eps, false);
    }
    return tv_grad_impl(e, eps, true);
}

// Slab-sharded descent, one communication round per inner iteration: the norm pass also leaves the gradient's first and last
// slice in caller buffers (what the neighbours need to advance their halo planes themselves: tomo_tv_halo_apply).
int tomo_tv_grad_planes(tomo_engine *e, float eps, int with_tv, void *g_first, void *g_last)
{
    if (!g_first || !g_last) return fail(TOMO_ERR_ARG, "null plane buffer");
    return tv_grad_impl(e, eps, with_tv != 0, (float *)g_first, (float *)g_last);
}

// halo planes <- the neighbours' update of those slices: halo - (dPOCS g)/||g|| (clamped), with the received gradient planes
// g_lo (the lower neighbour's last slice) and g_hi (the upper neighbour's first slice).  Call it AFTER the update pass (which
// still reads the old planes).
int tomo_tv_halo_apply(tomo_engine *e, float dPOCS, int clamp, const void *g_lo, const void *g_hi)
{
    NEED(e);
    if (!g_lo || !g_hi) return fail(TOMO_ERR_ARG, "null plane buffer");
    hipLaunchKernelGGL(k_halo_apply, dim3((unsigned)((e->npix + 255) / 256)), dim3(256), 0, e->stream, e->halo_lo, e->halo_hi,
                       (const float *)g_lo, (const float *)g_hi, gnorm_ptr(e), dPOCS, clamp, (int)e->npix);
    LAUNCHCHK();
    return TOMO_OK;
}

// the engine's pair of halo planes that is NOT in use (the second pair is allocated on first use): what a pass that still reads the
// planes in use writes the next ones into
static int halo_other_pair(tomo_engine *e, float **lo, float **hi)
{
    int rc;
    if (!e->halo_lo_alt) {
        if ((rc = dev_alloc(e, ENGINE, (void **)&e->halo_lo_alt, e->npix * sizeof(float), true))) return rc;
        if ((rc = dev_alloc(e, ENGINE, (void **)&e->halo_hi_alt, e->npix * sizeof(float), true))) return rc;
    }
    *lo = e->halo_lo == e->halo_lo_own ? e->halo_lo_alt : e->halo_lo_own;
    *hi = e->halo_hi == e->halo_hi_own ? e->halo_hi_alt : e->halo_hi_own;
    return TOMO_OK;
}

// wrap: also write the new last / first slice into the engine's halo planes (single slab, periodic); plane_last /
// plane_first: into caller buffers instead (slab-sharded: the planes the ring exchange sends next)
// hg_lo / hg_hi (slab-sharded descent): the gradient planes received from the ring neighbours; the halo planes are advanced with them
// (k_halo_apply's expression) -- inside the update pass where it can write a second pair of planes ("tv_halo_fold", the march4 form, the
// engine's own planes), by a k_halo_apply launch behind it otherwise
static int tv_update_impl(tomo_engine *e, float dPOCS, int clamp, int track_vol, int slot, bool wrap = false,
                          float *plane_last = nullptr, float *plane_first = nullptr, const float *hg_lo = nullptr, const float *hg_hi = nullptr)
{
    NEED(e);
    float *x, *g, *track = nullptr; int rc;
    if ((rc = get_vol(e, e->tv_target, &x))) return rc;
    if ((rc = get_scratch(e, &e->tvg, &g))) return rc;
    if (track_vol >= 0) {
        if (track_vol == e->tv_target) return fail(TOMO_ERR_ARG, "the tracked volume must differ from the one descended");
        if (slot < 0 || slot >= TOMO_S_COUNT) return fail(TOMO_ERR_ARG, "bad scalar slot");
        if ((rc = get_vol(e, track_vol, &track))) return rc;
        // an evaluation in flight on the second stream may still read the tracked volume (ASD-POCS: the data distance
        // of the snapshot): order this write behind it on the device; tomo_async_wait later is still valid
        if ((rc = order_after_async(e))) return rc;
        if ((rc = reduce_begin(e))) return rc;
    }
    if (e->tv_lds == 1 && e->tv_recompute) {
        // recompute-and-update pass: reads x (+ the halo planes the norm pass used), writes x_new into the second buffer,
        // which then becomes the volume.  The wrapped planes of x_new go to a second pair of halo buffers (this pass still
        // reads the old ones), swapped in afterwards; halo buffers bound by the caller are refreshed by a gather launch.
        float *alt;
        if ((rc = get_scratch(e, &e->tv_alt, &alt))) return rc;
        const bool own_halo = e->halo_lo == e->halo_lo_own || e->halo_lo == e->halo_lo_alt;
        float *wl = plane_last, *wh = plane_first;
        if (wrap && own_halo && (rc = halo_other_pair(e, &wl, &wh))) return rc;
        Halo h{e->halo_lo, e->halo_hi};
        TvUpd up{alt, gnorm_ptr(e), dPOCS, clamp, track, wl, wh, slab_streams(e) ? 1 : 0, nullptr, nullptr, nullptr, nullptr};
        const bool fold = hg_lo && hg_hi && (e->tv_halo_fold < 0 ? e->sxc >= 128 : e->tv_halo_fold != 0) && own_halo && !wrap && e->tv_tz != 4 && e->tv_march4;
        if (fold) {
            up.hg_lo = hg_lo; up.hg_hi = hg_hi;
            if ((rc = halo_other_pair(e, &up.ho_lo, &up.ho_hi))) return rc;
        }
        {
            ProfScope ps(e, TOMO_K_TV_UPDATE);
            const int tz = e->tv_tz == 4 ? 4 : 8, yseg = tv_rows_per_wave(e, tz);
            dim3 grid(tv_march_grid(e->n, tz, e->sxc / 64, (e->n + yseg - 1) / yseg));
            const bool edge = e->nx % 64 != 0 || e->n % 8 != 0;
            if (tz == 8 && e->tv_march4) with_flag(edge, [&](auto E) { with_flag(track != nullptr, [&](auto T) { with_flag(up.stream != 0, [&](auto S) {
                hipLaunchKernelGGL((k_tv_march4<8, false, TVM_UPDATE, E(), T(), S()>), grid, dim3(256), 0, e->stream, x, h, e->d_part, e->tv_last_eps, e->n, e->nx, e->sx, yseg, (double *)nullptr, up);
            }); }); });
            else with_int<4, 8>(tz, [&](auto TZ) {
                hipLaunchKernelGGL((k_tv_grad_reg<TZ(), false, true, TVM_UPDATE>), grid, dim3(256), 0, e->stream, x, h, (float *)nullptr, e->d_part, e->tv_last_eps, e->n, e->nx, e->sx, yseg, (double *)nullptr, up);
            });
        }
        LAUNCHCHK();
        e->vol[e->tv_target] = alt; e->tv_alt = x;              // the updated volume lives in the partner buffer
        if (wrap && own_halo) { e->halo_lo = wl; e->halo_hi = wh; }
        else if (wrap) { if ((rc = tomo_halo_local(e, e->tv_target))) return rc; }
        if (fold) { e->halo_lo = up.ho_lo; e->halo_hi = up.ho_hi; }
        else if (hg_lo && hg_hi && (rc = tomo_tv_halo_apply(e, dPOCS, clamp, hg_lo, hg_hi))) return rc;
        return track ? reduce_end(e, slot) : TOMO_OK;
    }
    int64_t n4 = e->vol_elems() / 4;
    {
        ProfScope ps(e, TOMO_K_TV_UPDATE);
        float *wl = wrap ? e->halo_lo : plane_last, *wh = wrap ? e->halo_hi : plane_first;
        double *part = track ? e->d_part : nullptr;
        with_flag(track != nullptr, [&](auto T) {
            hipLaunchKernelGGL(k_tv_update<T()>, dim3(grid_1d(n4)), dim3(256), 0, e->stream, (f4 *)x, (const f4 *)g, gnorm_ptr(e), dPOCS, clamp, n4, (f4 *)track, part, wl, wh, e->nx, e->sx / 4);
        });
    }
    LAUNCHCHK();
    if (hg_lo && hg_hi && (rc = tomo_tv_halo_apply(e, dPOCS, clamp, hg_lo, hg_hi))) return rc;
    return track ? reduce_end(e, slot) : TOMO_OK;
}

int tomo_tv_update(tomo_engine *e, float dPOCS, int clamp) { return tv_update_impl(e, dPOCS, clamp, -1, 0); }

int tomo_tv_update_planes(tomo_engine *e, float dPOCS, int clamp, void *first_plane, void *last_plane)
{
    if (!first_plane || !last_plane) return fail(TOMO_ERR_ARG, "null plane buffer");
    return tv_update_impl(e, dPOCS, clamp, -1, 0, false, (float *)last_plane, (float *)first_plane);
}

int tomo_tv_update_tracked(tomo_engine *e, float dPOCS, int clamp, int track_vol, int slot)
{
    return tv_update_impl(e, dPOCS, clamp, track_vol, slot);
}

int tomo_fgp_begin(tomo_engine *e) { return tomo_fgp_begin_vol(e, TOMO_VOL_RECON); }

static int fgp_begin_impl(tomo_engine *e, int vol, bool zero_p)
{
    NEED(e);
    float *d, *p; int rc;
    if ((rc = get_vol(e, vol, &d))) return rc;
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

int tomo_fgp_begin_vol(tomo_engine *e, int vol) { return fgp_begin_impl(e, vol, true); }

int tomo_fgp_obj(tomo_engine *e, float lambda)
{
    NEED(e);
    if (!e->tvg || !e->fgp_p[2]) return fail(TOMO_ERR_STATE, "tomo_fgp_begin has not been called");
    ProfScope ps(e, TOMO_K_FGP_OBJ);
    hipLaunchKernelGGL(k_fgp_obj, dim3(tv_grid(e)), dim3(256), 0, e->stream, e->vol[e->fgp_target], e->tvg, e->fgp_p[0], e->fgp_p[1], e->fgp_p[2], e->halo_lo, e->is_first, lambda, e->n, e->nx, e->sx);
    LAUNCHCHK();
    return TOMO_OK;
}

int tomo_fgp_grad(tomo_engine *e, float lambda)
{
    NEED(e);
    if (!e->tvg || !e->fgp_p[2]) return fail(TOMO_ERR_STATE, "tomo_fgp_begin has not been called");
    float multip = 1.0f / (26.0f * lambda);
    ProfScope ps(e, TOMO_K_FGP_GRAD);
    hipLaunchKernelGGL(k_fgp_grad, dim3(tv_grid(e)), dim3(256), 0, e->stream, e->tvg, e->fgp_p[0], e->fgp_p[1], e->fgp_p[2], e->halo_hi, e->is_last, multip, e->n, e->nx, e->sx);
    LAUNCHCHK();
    return TOMO_OK;
}

int tomo_fgp_end(tomo_engine *e, int iters)
{
    if (e) e->claims.prox_landed(e->fgp_target);   // the prox result lands in the volume

    NEED(e);
    if (!e->tvg) return fail(TOMO_ERR_STATE, "tomo_fgp_begin has not been called");
    (void)iters;  // D is the zero-filled buffer when no iteration ran, exactly like d_update (tv_fgp.cu:223,272)
    HIPCHK(hipMemcpyAsync(e->vol[e->fgp_target], e->tvg, e->vol_elems() * sizeof(float), hipMemcpyDeviceToDevice, e->stream));
    return TOMO_OK;
}

int tomo_tv(tomo_engine *e, int vol, float eps)
{
    int rc;
    if ((rc = tomo_halo_local(e, vol))) return rc;
    return tomo_tv_partial(e, vol, eps);
}

static int tv_gd_impl(tomo_engine *e, int ng, float dPOCS, float eps, int track_vol, int slot)
{
    int rc;
    if (!e) return fail(TOMO_ERR_ARG, "null engine");
    // the TV value before descent comes out of the first gradient pass (its denominators are the TV integrand)
    const bool fold_tv = ng > 0 && (e->tv_lds == 8 || e->tv_lds == 1);
    if (fold_tv) { if ((rc = tomo_halo_local(e, e->tv_target))) return rc; }
    else if ((rc = tomo_tv(e, e->tv_target, eps))) return rc;
    for (int g = 0; g < ng; ++g) {
        // single slab: every descent step but the last also writes the wrapped halo planes of its result
        if ((rc = tv_grad_impl(e, eps, fold_tv && g == 0))) return rc;
        if ((rc = tv_update_impl(e, dPOCS, g == ng - 1, g == ng - 1 ? track_vol : -1, slot, g < ng - 1))) return rc;
    }
    if (ng <= 0) {
        if ((rc = tomo_positivity(e, e->tv_target))) return rc;
        if (track_vol >= 0) {
            if ((rc = tomo_diff_norm_sq(e, e->tv_target, track_vol, slot))) return rc;
            return tomo_copy_volume(e, track_vol, e->tv_target);
        }
    }
    return TOMO_OK;
}

int tomo_tv_gd(tomo_engine *e, int ng, float dPOCS, float eps) { return tv_gd_impl(e, ng, dPOCS, eps, -1, 0); }

int tomo_tv_gd_tracked(tomo_engine *e, int ng, float dPOCS, float eps, int track_vol, int slot)
{
    if (track_vol < 0) return fail(TOMO_ERR_ARG, "bad tracked volume");
    return tv_gd_impl(e, ng, dPOCS, eps, track_vol, slot);
}

int tomo_tv_fgp(tomo_engine *e, int iters, float lambda) { return tomo_tv_fgp_vol(e, TOMO_VOL_RECON, iters, lambda); }

// ---- fused FGP iteration, step form (single slab and slab-sharded) ------------------------------------------------------
int tomo_bind_fgp_halo(tomo_engine *e, void *lo, void *hi, void *send_first, void *send_last)
{
    NEED(e);
    if (!lo || !hi || !send_first || !send_last) return fail(TOMO_ERR_ARG, "null plane buffer");
    HIPCHK(hipStreamSynchronize(e->stream));
    e->fgp_lo = (float *)lo; e->fgp_hi = (float *)hi; e->fgp_send_first = (float *)send_first; e->fgp_send_last = (float *)send_last;
    e->fgp_planes2 = false;
    return TOMO_OK;
}

// the two-slice-deep set (k_fgp_fused2<.., SHARDED>): lo 5 planes [P1(-1), A(-1), P2(-1), P3(-1), P1(-2)], hi 8 planes
// [A, P1, P2, P3](nx), [..](nx + 1), send_first 8 planes [A, P1, P2, P3](0), [..](1), send_last 5 planes [P1(nx-1), A(nx-1), P2(nx-1),
// P3(nx-1), P1(nx-2)].  The one-deep planes of tomo_bind_fgp_halo are the prefixes (1 / 4 / 4 / 1), so both step forms run on it.
int tomo_bind_fgp_halo2(tomo_engine *e, void *lo, void *hi, void *send_first, void *send_last)
{
    int rc = tomo_bind_fgp_halo(e, lo, hi, send_first, send_last);
    if (rc) return rc;
    e->fgp_planes2 = true;
    return TOMO_OK;
}

// sharded: slab faces that are not global edges read / write the bound planes
static bool fgp_sharded(const tomo_engine *e) { return !(e->is_first && e->is_last); }

int tomo_fgp_fused_begin(tomo_engine *e, int vol)
{
    int rc;
    if ((rc = fgp_begin_impl(e, vol, false))) return rc;     // the first iteration takes P = 0 as known
    float *q;
    for (int i = 0; i < 3; ++i) if ((rc = get_scratch(e, &e->fgp_q[i], &q))) return rc;
    if (fgp_sharded(e)) {
        if (!e->fgp_lo) return fail(TOMO_ERR_STATE, "slab-sharded fused FGP needs tomo_bind_fgp_halo");
        // plane 0 of send_first: the first slice of the prox input (constant over the call)
        hipLaunchKernelGGL(k_halo_pack, dim3((unsigned)((e->npix + 255) / 256)), dim3(256), 0, e->stream, e->vol[vol], e->fgp_send_first, (int)e->npix, e->sx, 0);
        LAUNCHCHK();
        if (e->fgp_planes2 && e->nx >= 2) {      // the deep set: A of slice 1 (send_first plane 4) and of the last slice (send_last plane 1)
            hipLaunchKernelGGL(k_halo_pack, dim3((unsigned)((e->npix + 255) / 256)), dim3(256), 0, e->stream, e->vol[vol], e->fgp_send_first + 4 * e->npix, (int)e->npix, e->sx, 1);
            hipLaunchKernelGGL(k_halo_pack, dim3((unsigned)((e->npix + 255) / 256)), dim3(256), 0, e->stream, e->vol[vol], e->fgp_send_last + e->npix, (int)e->npix, e->sx, e->nx - 1);
            LAUNCHCHK();
        }
    }
    return TOMO_OK;
}

int tomo_fgp_fused_step(tomo_engine *e, float lambda, int first_iteration)
{
    NEED(e);
    if (!e->fgp_q[2] || !e->fgp_p[2]) return fail(TOMO_ERR_STATE, "tomo_fgp_fused_begin has not been called");
    const int yseg = 32;
    const int nzb = (e->n + TVL_TZ - 1) / TVL_TZ, nys = (e->n + yseg - 1) / yseg, nchunk = e->sxc / 64;
    // one workgroup per item; an XCD-aligned grid when the z blocks split evenly over the 8 XCDs (k_fgp_fused's item map)
    dim3 grid((nzb & 7) == 0 ? 8u * (unsigned)((nzb >> 3) * nchunk * nys) : (unsigned)(nzb * nchunk * nys));
    const float multip = 1.0f / (26.0f * lambda);
    FgpEdge ed{};
    ed.first = e->is_first; ed.last = e->is_last;
    if (fgp_sharded(e)) { ed.p1_lo = e->fgp_lo; ed.hi = e->fgp_hi; ed.send_first = e->fgp_send_first; ed.send_last = e->fgp_send_last; }
    {
        ProfScope ps(e, TOMO_K_FGP_GRAD);
        with_flag(fgp_sharded(e), [&](auto SH) {
            hipLaunchKernelGGL(k_fgp_fused<SH()>, grid, dim3(256), 0, e->stream, e->vol[e->fgp_target], e->fgp_p[0], e->fgp_p[1], e->fgp_p[2],
                               e->fgp_q[0], e->fgp_q[1], e->fgp_q[2], lambda, multip, e->n, e->nx, e->sx, yseg, first_iteration ? 1 : 0, ed);
        });
    }
    LAUNCHCHK();
    for (int k = 0; k < 3; ++k) std::swap(e->fgp_p[k], e->fgp_q[k]);
    return TOMO_OK;
}

// two iterations in one pass (k_fgp_fused2: P stays on chip between them).  A sharded slab needs the two-slice-deep planes
// (tomo_bind_fgp_halo2, exchanged once before the call: tomo_comm_fgp_exchange2) and at least two slices on EVERY slab of the ring.
int tomo_fgp_fused_step2(tomo_engine *e, float lambda, int first_iteration)
{
    NEED(e);
    if (!e->fgp_q[2] || !e->fgp_p[2]) return fail(TOMO_ERR_STATE, "tomo_fgp_fused_begin has not been called");
    if (fgp_sharded(e) && (!e->fgp_planes2 || !e->fgp_lo)) return fail(TOMO_ERR_STATE, "a sharded tomo_fgp_fused_step2 needs the two-slice-deep planes (tomo_bind_fgp_halo2)");
    if (fgp_sharded(e) && e->nx < 2) return fail(TOMO_ERR_STATE, "a sharded tomo_fgp_fused_step2 needs at least two slices per slab");
    const int yseg = 32;                                 // (16 ... 64 within 3 %; 128 and more lose to the tail)
    const int nzb = (e->n + F2_TZ - 1) / F2_TZ, nys = (e->n + yseg - 1) / yseg, nchunk = (e->nx + F2_SC - 1) / F2_SC;
    dim3 grid((nzb & 7) == 0 ? 8u * (unsigned)((nzb >> 3) * nchunk * nys) : (unsigned)(nzb * nchunk * nys));
    const float multip = 1.0f / (26.0f * lambda);
    {
        ProfScope ps(e, TOMO_K_FGP_GRAD);
        const Fgp2Edge ed = fgp_sharded(e) ? Fgp2Edge{e->fgp_lo, e->fgp_hi, e->fgp_send_first, e->fgp_send_last, e->is_first, e->is_last} : Fgp2Edge{};
        with_flag(fgp_sharded(e), [&](auto SH) {
            hipLaunchKernelGGL((k_fgp_fused2<false, SH()>), grid, dim3(256), 0, e->stream, e->vol[e->fgp_target], e->fgp_p[0], e->fgp_p[1], e->fgp_p[2],
                               e->fgp_q[0], e->fgp_q[1], e->fgp_q[2], lambda, multip, e->n, e->nx, e->sx, yseg, first_iteration ? 1 : 0, ed);
        });
    }
    LAUNCHCHK();
    for (int k = 0; k < 3; ++k) std::swap(e->fgp_p[k], e->fgp_q[k]);
    return TOMO_OK;
}

// one more iteration AND the call's result in one pass (k_fgp_fused2<true>): D of the iteration's P, which is never stored; the
// result is written to a scratch volume that then changes places with the target's buffer.  Whole-volume slabs only.
int tomo_fgp_fused_last(tomo_engine *e, float lambda, int first_iteration)
{
    NEED(e);
    if (!e->fgp_q[2] || !e->fgp_p[2]) return fail(TOMO_ERR_STATE, "tomo_fgp_fused_begin has not been called");
    if (fgp_sharded(e)) return fail(TOMO_ERR_STATE, "tomo_fgp_fused_last is for a slab that is the whole volume");
    if (e->fgp_target < 0 || e->fgp_target >= TOMO_VOL_SLOTS) return fail(TOMO_ERR_STATE, "no target volume");
    const int yseg = 32;
    const int nzb = (e->n + F2_TZ - 1) / F2_TZ, nys = (e->n + yseg - 1) / yseg, nchunk = (e->nx + F2_SC - 1) / F2_SC;
    dim3 grid((nzb & 7) == 0 ? 8u * (unsigned)((nzb >> 3) * nchunk * nys) : (unsigned)(nzb * nchunk * nys));
    const float multip = 1.0f / (26.0f * lambda);
    {
        ProfScope ps(e, TOMO_K_FGP_OBJ);
        hipLaunchKernelGGL((k_fgp_fused2<true, false>), grid, dim3(256), 0, e->stream, e->vol[e->fgp_target], e->fgp_p[0], e->fgp_p[1], e->fgp_p[2],
                           e->fgp_q[0], e->fgp_q[1], e->fgp_q[2], lambda, multip, e->n, e->nx, e->sx, yseg, first_iteration ? 1 : 0, Fgp2Edge{});
    }
    LAUNCHCHK();
    std::swap(e->vol[e->fgp_target], e->fgp_q[0]);         // the prox result's buffer becomes the volume; the old one is scratch now
    e->claims.prox_landed(e->fgp_target);
    return TOMO_OK;
}

// the last iteration only needs D (tv_fgp.cu:272), written straight over the target volume
int tomo_fgp_fused_end(tomo_engine *e, float lambda)
{
    if (e) e->claims.prox_landed(e->fgp_target);   // the prox result lands in the volume

    NEED(e);
    if (!e->fgp_p[2]) return fail(TOMO_ERR_STATE, "tomo_fgp_fused_begin has not been called");
    ProfScope ps(e, TOMO_K_FGP_OBJ);
    float *a = e->vol[e->fgp_target];
    hipLaunchKernelGGL(k_fgp_obj, dim3(tv_grid(e)), dim3(256), 0, e->stream, a, a, e->fgp_p[0], e->fgp_p[1], e->fgp_p[2],
                       fgp_sharded(e) ? e->fgp_lo : e->halo_lo, e->is_first, lambda, e->n, e->nx, e->sx);
    LAUNCHCHK();
    return TOMO_OK;
}

int tomo_tv_fgp_vol(tomo_engine *e, int vol, int iters, float lambda)
{
    int rc;
    if ((rc = tomo_tv(e, vol, 1e-6f))) return rc;    // tv_fgp.cu:170-189,231-238
    const bool fused = e && e->fgp_fused && iters > 1;
    int f = e->is_first, l = e->is_last;
    e->is_first = e->is_last = 1;
    if (fused) {
        // iterations 0..iters-2: one fused kernel each (D stays on chip); the last iteration only needs D
        rc = tomo_fgp_fused_begin(e, vol);
        int i = 0;
        if (e->fgp_pair) for (; i + 2 < iters && !rc; i += 2) rc = tomo_fgp_fused_step2(e, lambda, i == 0);     // pairs, P kept on chip between
        if (e->fgp_pair && i + 2 == iters) {              // an odd iteration out and the result: one pass
            if (!rc) rc = tomo_fgp_fused_last(e, lambda, i == 0);
        } else {
            for (; i + 1 < iters && !rc; ++i) rc = tomo_fgp_fused_step(e, lambda, i == 0);
            if (!rc) rc = tomo_fgp_fused_end(e, lambda);
        }
        e->is_first = f; e->is_last = l;
        return rc;
    }
    rc = fgp_begin_impl(e, vol, true);
    for (int i = 0; i < iters && !rc; ++i) {
        if ((rc = tomo_fgp_obj(e, lambda)) || (rc = tomo_fgp_grad(e, lambda))) break;
    }
    e->is_first = f; e->is_last = l;
    if (rc) return rc;
    return tomo_fgp_end(e, iters);
}
