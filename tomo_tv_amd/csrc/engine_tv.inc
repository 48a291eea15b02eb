// engine_tv.inc -- part of tomo_engine.hip (ONE translation unit: the kernels are templates and asm blocks in headers; the host side is
// split by topic into files that tomo_engine.hip includes in order).  This part: C ABI: the halo calls, the sub-slab group's coupling calls, TV value / gradient / update / descent.
// Which kernel runs is select_tv's answer (tv_form.h).  A pass receives what it uses -- eps, the address of ||g||^2, the halo planes it reads
// and may replace -- and only the C entries read those from the engine.
static int field_ptr(tomo_engine *e, int field, float **out)
{
    if (field == TOMO_FIELD_FGP_D) return get_scratch(e, &e->tvg, out);
    if (field == TOMO_FIELD_FGP_P1) return get_scratch(e, &e->fgp_p[0], out);
    return get_vol_ro(e, field, out);   // halo packs and fills only read
}

struct HaloPair { float *lo, *hi; };       // the plane below slice 0 and the plane above the last slice
// lo <- the last slice of x, hi <- slice 0: the periodic wrap of a single slab
static int halo_wrap(tomo_engine *e, const float *x, HaloPair h)
{
    hipLaunchKernelGGL(k_halo_wrap, dim3((unsigned)((e->npix + 255) / 256)), dim3(256), 0, e->stream, x, h.lo, h.hi, (int)e->npix, e->sx, e->nx);
    LAUNCHCHK();
    return TOMO_OK;
}

int tomo_bind_halo(tomo_engine *e, void *device_lo, void *device_hi)
{
    NEED(e);
    HIPCHK(hipStreamSynchronize(e->stream));
    e->halo_lo = device_lo ? (float *)device_lo : e->halo_lo_own; e->halo_hi = device_hi ? (float *)device_hi : e->halo_hi_own;
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
    return halo_wrap(e, x, HaloPair{(float *)last_plane, (float *)first_plane});
}

int tomo_halo_local(tomo_engine *e, int field)
{
    NEED(e);
    float *x; int rc; if ((rc = field_ptr(e, field, &x))) return rc;
    return halo_wrap(e, x, HaloPair{e->halo_lo, e->halo_hi});     // below slice 0 sits the last slice, above the last slice sits slice 0
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

// ---- the launchers: one per kernel family (select_tv says which runs) ------------------------------------------------------------
static TvShape tv_shape(const tomo_engine *e) { return TvShape{e->n, e->nx, e->sxc}; }
static TvForm tv_form(const tomo_engine *e) { return select_tv(e->tv, tv_shape(e)); }
static int tv_grid(tomo_engine *e) { return (int)std::min<int64_t>((e->npix * (e->sx / 64) + 3) / 4, 256 * 16); }

// direct-global stencil (reads x twice): the gradient into g, or the value alone (g = null); sums into the main lane's partial sums
static void launch_tv_direct(tomo_engine *e, const float *x, Halo h, float *g, float eps)
{
    if (g) hipLaunchKernelGGL(k_tv_grad, dim3(tv_grid(e)), dim3(256), 0, e->stream, x, h, g, e->d_part, eps, e->n, e->nx, e->sx);
    else hipLaunchKernelGGL(k_tv_value, dim3(tv_grid(e)), dim3(256), 0, e->stream, x, h, e->d_part, eps, e->n, e->nx, e->sx);
}

// LDS march: the gradient into g (the TV value folded in with 8 columns per workgroup only), or the value alone (g = null)
static void launch_tv_lds(tomo_engine *e, const TvPass &p, bool with_tv, const float *x, Halo h, float *g, float eps, double *part, double *part_tv)
{
    const dim3 grid((unsigned)(((e->n + p.tz - 1) / p.tz) * (e->sxc / 64)), (unsigned)((e->n + p.yseg - 1) / p.yseg));
    auto lds = [&](auto k) { hipLaunchKernelGGL(k, grid, dim3(256), 0, e->stream, x, h, g, part, eps, e->n, e->nx, e->sx, p.yseg, part_tv); };
    if (!g) lds(k_tv_grad_lds<8, true, false>);
    else if (p.family == TV_LDS16) lds(k_tv_grad_lds<16, false>);
    else with_flag(with_tv, [&](auto W) { lds(k_tv_grad_lds<8, W()>); });
}

// Register march, every pass of it, one wave per (z block, chunk, y segment): k_tv_march4 where the pass says so, else k_tv_grad_reg.
// mode: TVM_VALUE the TV value alone (the march without its gradient half: x is read once; k_tv_march4 only without edge lanes);
// TVM_STORE the gradient into g; TVM_NORM sum g^2 (and TV) only; TVM_UPDATE re-evaluates g and writes up.x_out.
static void launch_tv_march(tomo_engine *e, const TvPass &p, int mode, bool with_tv, const float *x, Halo h, float *g, float eps, double *part,
                            double *part_tv, const TvUpd &up)
{
    const dim3 grid(tv_march_grid(e->n, p.tz, e->sxc / 64, (e->n + p.yseg - 1) / p.yseg));
    const bool m4 = p.family == TV_MARCH4;
    auto march4 = [&](auto k) { hipLaunchKernelGGL(k, grid, dim3(256), 0, e->stream, x, h, part, eps, e->n, e->nx, e->sx, p.yseg, part_tv, up); };
    auto reg = [&](auto k) { hipLaunchKernelGGL(k, grid, dim3(256), 0, e->stream, x, h, g, part, eps, e->n, e->nx, e->sx, p.yseg, part_tv, up); };
    if (mode == TVM_VALUE) { if (m4) march4(k_tv_march4<8, true, TVM_VALUE, false>); else reg(k_tv_grad_reg<8, true, false>); }
    else if (mode == TVM_STORE) with_flag(with_tv, [&](auto W) { reg(k_tv_grad_reg<8, W()>); });
    else if (mode == TVM_NORM) with_flag(with_tv, [&](auto W) {
        if (m4) with_flag(p.edge, [&](auto E) { march4(k_tv_march4<8, W(), TVM_NORM, E()>); });
        else with_int<4, 8>(p.tz, [&](auto TZ) { reg(k_tv_grad_reg<TZ(), W(), true, TVM_NORM>); });
    });
    else if (m4) with_flag(p.edge, [&](auto E) { with_flag(up.track != nullptr, [&](auto T) { with_flag(up.stream != 0, [&](auto S) {
        march4(k_tv_march4<8, false, TVM_UPDATE, E(), T(), S()>);
    }); }); });
    else with_int<4, 8>(p.tz, [&](auto TZ) { reg(k_tv_grad_reg<TZ(), false, true, TVM_UPDATE>); });
}

// ---- value, gradient, update: each receives eps, the address of ||g||^2 and the halo planes it uses; only the C entries read them from the engine
static int tv_value_impl(tomo_engine *e, int vol, Halo h, float eps)
{
    float *x; int rc; if ((rc = get_vol_ro(e, vol, &x))) return rc;
    const TvPass p = tv_form(e).value;
    const bool direct = p.family == TV_DIRECT;       // sums into the main lane; the marches into the TV lane
    if (!direct && !e->d_part_tv && (rc = dev_alloc(e, ENGINE, (void **)&e->d_part_tv, NPART * sizeof(double), true))) return rc;
    const Lane ln = direct ? main_lane(e) : tv_lane(e);
    if ((rc = reduce_begin(e, ln))) return rc;
    if (direct) launch_tv_direct(e, x, h, nullptr, eps);
    else if (p.family == TV_LDS8) launch_tv_lds(e, p, true, x, h, nullptr, eps, nullptr, e->d_part_tv);
    else launch_tv_march(e, p, TVM_VALUE, true, x, h, nullptr, eps, nullptr, e->d_part_tv, TvUpd{});
    LAUNCHCHK();
    return reduce_end(e, ln, TOMO_S_TV);
}

// TV of a volume with the halo planes as they are (step form: the caller has exchanged or wrapped them)
int tomo_tv_partial(tomo_engine *e, int vol, float eps) { NEED(e); return tv_value_impl(e, vol, Halo{e->halo_lo, e->halo_hi}, eps); }

// sum g^2 into TOMO_S_GNORM (and, with_tv, the TV value into TOMO_S_TV); g itself is stored only by the forms whose update pass reads it.
// g_first / g_last: the gradient's first and last slice into these buffers as well (the recompute form's norm pass only)
static int tv_grad_impl(tomo_engine *e, float eps, bool with_tv, Halo h, float *g_first = nullptr, float *g_last = nullptr)
{
    const TvForm f = tv_form(e);
    if ((g_first || g_last) && !f.planes) return fail(TOMO_ERR_STATE, "gradient planes need the recompute form of the TV march (tv_lds = 1, tv_recompute = 1)");
    float *x, *g; int rc;
    if ((rc = get_vol(e, e->tv_target, &x)) || (rc = get_scratch(e, &e->tvg, &g))) return rc;
    with_tv = with_tv && f.carries_tv;
    if (with_tv && !e->d_part_tv && (rc = dev_alloc(e, ENGINE, (void **)&e->d_part_tv, NPART * sizeof(double), true))) return rc;
    if ((rc = reduce_begin(e)) || (with_tv && (rc = reduce_begin(e, tv_lane(e))))) return rc;
    {
        ProfScope ps(e, TOMO_K_TV_GRAD);
        double *part_tv = with_tv ? e->d_part_tv : nullptr;
        TvUpd gp{}; gp.wrap_lo = g_last; gp.wrap_hi = g_first;      // g's last / first slice (slab-sharded descent), or null
        if (f.recompute) launch_tv_march(e, f.descent, TVM_NORM, with_tv, x, h, nullptr, eps, e->d_part, part_tv, gp);   // the update pass re-evaluates g
        else if (f.descent.family == TV_REG) launch_tv_march(e, f.descent, TVM_STORE, with_tv, x, h, g, eps, e->d_part, part_tv, gp);
        else if (f.descent.family == TV_DIRECT) launch_tv_direct(e, x, h, g, eps);
        else launch_tv_lds(e, f.descent, with_tv, x, h, g, eps, e->d_part, part_tv);
    }
    LAUNCHCHK();
    if (with_tv && (rc = reduce_end(e, tv_lane(e), TOMO_S_TV))) return rc;
    return reduce_end(e, TOMO_S_GNORM);
}

int tomo_tv_set_target(tomo_engine *e, int vol)
{
    NEED(e);
    float *x; int rc; if ((rc = get_vol(e, vol, &x))) return rc;
    e->tv_target = vol;
    return TOMO_OK;
}

// The step-form entries.  eps carries from the gradient call to the update call that follows it (the update pass of the recompute form
// evaluates the gradient again): tv_last_eps, which only they read.
static int tv_grad_entry(tomo_engine *e, float eps, bool with_tv, float *g_first = nullptr, float *g_last = nullptr)
{
    NEED(e);
    const int rc = tv_grad_impl(e, eps, with_tv, Halo{e->halo_lo, e->halo_hi}, g_first, g_last);
    if (!rc) e->tv_last_eps = eps;
    return rc;
}

int tomo_tv_grad(tomo_engine *e, float eps) { return tv_grad_entry(e, eps, false); }
int tomo_tv_grad_tv(tomo_engine *e, float eps)
{
    NEED(e);
    const bool carries = tv_form(e).carries_tv;      // kernels without the folded value: a separate pass
    if (!carries) { int rc = tomo_tv_partial(e, e->tv_target, eps); if (rc) return rc; }
    return tv_grad_entry(e, eps, carries);
}
// Slab-sharded descent, one communication round per inner iteration: the norm pass also leaves the gradient's first and last slice in caller
// buffers (what the neighbours need to advance their halo planes themselves: tomo_tv_halo_apply).
int tomo_tv_grad_planes(tomo_engine *e, float eps, int with_tv, void *g_first, void *g_last)
{
    return (!g_first || !g_last) ? fail(TOMO_ERR_ARG, "null plane buffer") : tv_grad_entry(e, eps, with_tv != 0, (float *)g_first, (float *)g_last);
}

// halo planes <- the neighbours' update of those slices: halo - (dPOCS g)/||g|| (clamped), with the received gradient planes
// g_lo (the lower neighbour's last slice) and g_hi (the upper neighbour's first slice).  Call it AFTER the update pass (which still reads the old planes).
static int halo_apply(tomo_engine *e, HaloPair h, const float *g_lo, const float *g_hi, const double *gnorm2, float dPOCS, int clamp)
{
    hipLaunchKernelGGL(k_halo_apply, dim3((unsigned)((e->npix + 255) / 256)), dim3(256), 0, e->stream, h.lo, h.hi, g_lo, g_hi, gnorm2, dPOCS, clamp, (int)e->npix);
    LAUNCHCHK();
    return TOMO_OK;
}
int tomo_tv_halo_apply(tomo_engine *e, float dPOCS, int clamp, const void *g_lo, const void *g_hi)
{
    NEED(e);
    if (!g_lo || !g_hi) return fail(TOMO_ERR_ARG, "null plane buffer");
    return halo_apply(e, HaloPair{e->halo_lo, e->halo_hi}, (const float *)g_lo, (const float *)g_hi, e->d_scal + e->gnorm_slot, dPOCS, clamp);
}

// The engine owns two pairs of halo planes (the second is allocated on first use): *out = the partner of the pair h, what a pass that
// still reads h writes the next planes into.  Planes bound by the caller have no partner.
static int halo_partner(tomo_engine *e, HaloPair h, HaloPair *out)
{
    int rc;
    if (!e->halo_lo_alt && ((rc = dev_alloc(e, ENGINE, (void **)&e->halo_lo_alt, e->npix * sizeof(float), true)) ||
                            (rc = dev_alloc(e, ENGINE, (void **)&e->halo_hi_alt, e->npix * sizeof(float), true)))) return rc;
    *out = HaloPair{h.lo == e->halo_lo_own ? e->halo_lo_alt : e->halo_lo_own, h.hi == e->halo_hi_own ? e->halo_hi_alt : e->halo_hi_own};
    return TOMO_OK;
}

// x <- x - (dPOCS g)/||g|| with ||g||^2 at gnorm2.  halo: the planes the gradient pass read; on return the planes in use.  wrap: the pass also
// leaves the new last / first slice as the halo planes (single slab, periodic); plane_last / plane_first: in caller buffers instead (the planes
// the ring exchange sends next).  hg_lo / hg_hi (slab-sharded descent): the gradient planes received from the ring neighbours; the halo planes
// are advanced with them (k_halo_apply's expression) -- inside the update pass where tv_folds_halo says so, by a k_halo_apply launch behind it
// otherwise.  The recompute form still reads `halo` while it writes: new planes of the engine's own pair go to its partner, which `halo` names
// afterwards; planes bound by the caller are refreshed in place by a launch behind the pass.
static int tv_update_impl(tomo_engine *e, float eps, const double *gnorm2, HaloPair &halo, float dPOCS, int clamp, int track_vol, int slot, bool wrap = false,
                          float *plane_last = nullptr, float *plane_first = nullptr, const float *hg_lo = nullptr, const float *hg_hi = nullptr)
{
    float *x, *g, *track = nullptr; int rc;
    if (track_vol >= 0 && track_vol == e->tv_target) return fail(TOMO_ERR_ARG, "the tracked volume must differ from the one descended");
    if (track_vol >= 0 && (slot < 0 || slot >= TOMO_S_COUNT)) return fail(TOMO_ERR_ARG, "bad scalar slot");
    if (track_vol >= TOMO_VOL_SLOTS) return fail(TOMO_ERR_ARG, "bad volume id");
    if ((rc = get_vol(e, e->tv_target, &x)) || (rc = get_scratch(e, &e->tvg, &g))) return rc;
    // an evaluation in flight on the second stream may still read the tracked volume (ASD-POCS: the data distance of the snapshot): order this
    // write behind it on the device; tomo_async_wait later is still valid
    if (track_vol >= 0 && ((rc = get_vol(e, track_vol, &track)) || (rc = order_after_async(e)) || (rc = reduce_begin(e)))) return rc;
    const TvForm f = tv_form(e);
    const bool advance = hg_lo && hg_hi;     // (with both planes or not at all)
    if (f.recompute) {
        // recompute-and-update pass: reads x (+ the halo planes the norm pass used), writes x_new into the second buffer, which then becomes the volume
        float *alt; if ((rc = get_scratch(e, &e->tv_alt, &alt))) return rc;
        const bool own = halo.lo == e->halo_lo_own || halo.lo == e->halo_lo_alt, fold = advance && tv_folds_halo(f, e->tv, tv_shape(e), own, wrap);
        HaloPair next{nullptr, nullptr};
        if (((wrap && own) || fold) && (rc = halo_partner(e, halo, &next))) return rc;
        TvUpd up{alt, gnorm2, dPOCS, clamp, track, wrap && own ? next.lo : plane_last, wrap && own ? next.hi : plane_first, slab_streams(e) ? 1 : 0, nullptr, nullptr, nullptr, nullptr};
        if (fold) { up.hg_lo = hg_lo; up.hg_hi = hg_hi; up.ho_lo = next.lo; up.ho_hi = next.hi; }
        { ProfScope ps(e, TOMO_K_TV_UPDATE); launch_tv_march(e, f.descent, TVM_UPDATE, false, x, Halo{halo.lo, halo.hi}, nullptr, eps, e->d_part, nullptr, up); }
        LAUNCHCHK();
        e->vol[e->tv_target] = alt; e->tv_alt = x;              // the updated volume lives in the partner buffer
        if (next.lo) halo = next;
        else if (wrap && (rc = halo_wrap(e, alt, halo))) return rc;
        if (advance && !fold && (rc = halo_apply(e, halo, hg_lo, hg_hi, gnorm2, dPOCS, clamp))) return rc;
        return track ? reduce_end(e, slot) : TOMO_OK;
    }
    int64_t n4 = e->vol_elems() / 4;
    {
        ProfScope ps(e, TOMO_K_TV_UPDATE);
        float *wl = wrap ? halo.lo : plane_last, *wh = wrap ? halo.hi : plane_first;
        auto update = [&](auto k) { hipLaunchKernelGGL(k, dim3(grid_1d(n4)), dim3(256), 0, e->stream, (f4 *)x, (const f4 *)g, gnorm2, dPOCS, clamp, n4, (f4 *)track, track ? e->d_part : nullptr, wl, wh, e->nx, e->sx / 4); };
        if (track) update(k_tv_update<true>); else update(k_tv_update<false>);
    }
    LAUNCHCHK();
    if (advance && (rc = halo_apply(e, halo, hg_lo, hg_hi, gnorm2, dPOCS, clamp))) return rc;
    return track ? reduce_end(e, slot) : TOMO_OK;
}

// step form: eps as the last tomo_tv_grad* left it, ||g||^2 from the engine's slot, the engine's planes (which stay: no wrap, no advance)
static int tv_update_entry(tomo_engine *e, float dPOCS, int clamp, int track_vol, int slot, float *plane_last = nullptr, float *plane_first = nullptr)
{
    NEED(e);
    HaloPair h{e->halo_lo, e->halo_hi};
    return tv_update_impl(e, e->tv_last_eps, e->d_scal + e->gnorm_slot, h, dPOCS, clamp, track_vol, slot, false, plane_last, plane_first);
}
int tomo_tv_update(tomo_engine *e, float dPOCS, int clamp) { return tv_update_entry(e, dPOCS, clamp, -1, 0); }
int tomo_tv_update_tracked(tomo_engine *e, float dPOCS, int clamp, int track_vol, int slot) { return tv_update_entry(e, dPOCS, clamp, track_vol, slot); }
int tomo_tv_update_planes(tomo_engine *e, float dPOCS, int clamp, void *first_plane, void *last_plane)
{
    return (!first_plane || !last_plane) ? fail(TOMO_ERR_ARG, "null plane buffer") : tv_update_entry(e, dPOCS, clamp, -1, 0, (float *)last_plane, (float *)first_plane);
}

int tomo_tv(tomo_engine *e, int vol, float eps) { int rc = tomo_halo_local(e, vol); return rc ? rc : tomo_tv_partial(e, vol, eps); }

static int tv_gd_impl(tomo_engine *e, int ng, float dPOCS, float eps, int track_vol, int slot)
{
    NEED(e);
    int rc;      // the TV value before descent comes out of the first gradient pass (its denominators are the TV integrand)
    const bool fold_tv = ng > 0 && tv_form(e).carries_tv;
    if (fold_tv) { if ((rc = tomo_halo_local(e, e->tv_target))) return rc; }
    else if ((rc = tomo_tv(e, e->tv_target, eps))) return rc;
    if (ng > 0) e->tv_last_eps = eps;
    for (int g = 0; g < ng; ++g) {
        // single slab: every descent step but the last also writes the wrapped halo planes of its result
        HaloPair h{e->halo_lo, e->halo_hi};
        if ((rc = tv_grad_impl(e, eps, fold_tv && g == 0, Halo{h.lo, h.hi}))) return rc;
        rc = tv_update_impl(e, eps, e->d_scal + e->gnorm_slot, h, dPOCS, g == ng - 1, g == ng - 1 ? track_vol : -1, slot, g < ng - 1);
        e->halo_lo = h.lo; e->halo_hi = h.hi;
        if (rc) return rc;
    }
    if (ng <= 0) {
        if ((rc = tomo_positivity(e, e->tv_target))) return rc;
        if (track_vol >= 0) return (rc = tomo_diff_norm_sq(e, e->tv_target, track_vol, slot)) ? rc : tomo_copy_volume(e, track_vol, e->tv_target);
    }
    return TOMO_OK;
}

int tomo_tv_gd(tomo_engine *e, int ng, float dPOCS, float eps) { return tv_gd_impl(e, ng, dPOCS, eps, -1, 0); }
int tomo_tv_gd_tracked(tomo_engine *e, int ng, float dPOCS, float eps, int track_vol, int slot)
{
    return track_vol < 0 ? fail(TOMO_ERR_ARG, "bad tracked volume") : tv_gd_impl(e, ng, dPOCS, eps, track_vol, slot);
}
