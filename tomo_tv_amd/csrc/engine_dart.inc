// engine_dart.inc -- DART discrete tomography: segmentation with boundary and random free set, masked restore, the masked SIRT
// iterations of an update step, the masked smoother, per-class sums.
// Part of tomo_engine.hip (included inside its extern "C" block, after engine_bin.inc); kernels: kernels_dart.hip.h.
//
// One whole-volume engine only (the NEED_ALIGN rule): the label stencil of a slab would need its neighbours' boundary planes.  The
// state buffer (one byte per voxel) and the partial sums of the class statistics belong to the engine's registry, are allocated on
// first use and kept.  Everything that can be refused is refused before anything is enqueued or any engine state is touched.

// the rule of NEED_ALIGN (a usable engine without a communicator) under DART's name, then the 32-bit voxel index
#define NEED_DART(e) do { NEED(e); if ((e)->comm) return fail(TOMO_ERR_STATE, "DART runs on one whole-volume engine: this engine has a communicator"); if ((uint64_t)(e)->nx * (uint64_t)(e)->npix >= ((uint64_t)1 << 32)) return fail(TOMO_ERR_ARG, "DART indexes voxels with 32 bits: Nslice * N * N must be below 2^32"); } while (0)

static int dart_vol_id(int id) { return (id < 0 || id >= TOMO_VOL_SLOTS) ? fail(TOMO_ERR_ARG, "bad volume id") : TOMO_OK; }

static int dart_thresholds(const float *thr_host, int nthr, DartThr *out)
{
    if (nthr < 0 || nthr > 15) return fail(TOMO_ERR_ARG, "the number of thresholds must be 0..15");
    if (nthr > 0 && !thr_host) return fail(TOMO_ERR_ARG, "null thresholds");
    for (int i = 0; i < 15; ++i) out->t[i] = INFINITY;
    for (int i = 0; i < nthr; ++i) {
        if (!std::isfinite(thr_host[i])) return fail(TOMO_ERR_ARG, "non-finite threshold");
        if (i && !(thr_host[i] > thr_host[i - 1])) return fail(TOMO_ERR_ARG, "the thresholds must be strictly ascending");
        out->t[i] = thr_host[i];
    }
    return TOMO_OK;
}

// the grey levels of a call that follows a classify: one per label of the state
static int dart_greys(const tomo_engine *e, const float *grey_host, int nlevels, DartGrey *out)
{
    if (!grey_host) return fail(TOMO_ERR_ARG, "null grey levels");
    if (e->dart_nthr < 0) return fail(TOMO_ERR_STATE, "no segmentation in hand (tomo_dart_classify)");
    if (nlevels != e->dart_nthr + 1) return fail(TOMO_ERR_ARG, "the state has " + std::to_string(e->dart_nthr + 1) + " labels, got " + std::to_string(nlevels) + " grey levels");
    for (int i = 0; i < 16; ++i) out->g[i] = i < nlevels ? grey_host[i] : 0.f;
    return TOMO_OK;
}

// rows per wave of the two marches: about one round of resident waves, at least 8 rows (each segment loads two more than it writes)
static int dart_yseg(const tomo_engine *e, int tz)
{
    const int64_t cols = (int64_t)((e->n + tz - 1) / tz) * (e->sx / 64);
    const int64_t nys = std::max<int64_t>(1, (TV_WAVES_WANTED + cols - 1) / cols);
    return (int)std::min<int64_t>(e->n, std::max<int64_t>(TV_YSEG_MIN, (e->n + nys - 1) / nys));
}
static unsigned dart_grid(const tomo_engine *e, int tz, int yseg)
{
    const int64_t items = (int64_t)((e->n + tz - 1) / tz) * (e->sx / 64) * ((e->n + yseg - 1) / yseg);
    return (unsigned)((items + 3) / 4);
}

static int dart_restore_launch(tomo_engine *e, float *x, const DartGrey &g, bool all)
{
    const int64_t nvec = (int64_t)e->vol_elems() / 4;
    const dim3 grid((unsigned)grid_1d(nvec)), block(256);
    if (all) hipLaunchKernelGGL((k_dart_restore<true>), grid, block, 0, e->stream, x, (const uint8_t *)e->dart_state, g, nvec, e->nx, e->sx);
    else hipLaunchKernelGGL((k_dart_restore<false>), grid, block, 0, e->stream, x, (const uint8_t *)e->dart_state, g, nvec, e->nx, e->sx);
    LAUNCHCHK();
    return TOMO_OK;
}

int tomo_dart_classify(tomo_engine *e, int vol, const float *thr_host, int nthr, int connectivity, uint32_t seed, uint32_t free_threshold)
{
    NEED_DART(e);
    DartThr thr; int rc;
    if ((rc = dart_vol_id(vol)) || (rc = dart_thresholds(thr_host, nthr, &thr))) return rc;
    if (connectivity != 6 && connectivity != 26) return fail(TOMO_ERR_ARG, "connectivity must be 6 or 26");
    float *x;
    if ((rc = get_vol_ro(e, vol, &x))) return rc;
    if (!e->dart_state) { if ((rc = dev_alloc(e, ENGINE, (void **)&e->dart_state, e->vol_elems(), false))) return rc; }
    if (!e->d_part_tv) { if ((rc = dev_alloc(e, ENGINE, (void **)&e->d_part_tv, NPART * sizeof(double), true))) return rc; }
    const Lane lf = main_lane(e), lb = tv_lane(e);       // two reductions of the main stream open at once: the TV sum's lane takes the second
    if ((rc = reduce_begin(e, lf)) || (rc = reduce_begin(e, lb))) return rc;
    const int yseg = dart_yseg(e, 8);
    const dim3 grid(dart_grid(e, 8, yseg)), block(256);
    if (connectivity == 6) hipLaunchKernelGGL((k_dart_classify<6>), grid, block, 0, e->stream, (const float *)x, e->dart_state, thr, nthr, seed, free_threshold, e->n, e->nx, e->sx, yseg, lf.part, lb.part);
    else hipLaunchKernelGGL((k_dart_classify<26>), grid, block, 0, e->stream, (const float *)x, e->dart_state, thr, nthr, seed, free_threshold, e->n, e->nx, e->sx, yseg, lf.part, lb.part);
    LAUNCHCHK();
    e->dart_nthr = nthr;                                 // from here on the buffer holds THIS call's state, whatever a later launch returns
    if ((rc = reduce_end(e, lf, TOMO_S_DART_FREE))) return rc;
    return reduce_end(e, lb, TOMO_S_DART_BOUNDARY);
}

static int dart_restore(tomo_engine *e, int vol, const float *grey_host, int nlevels, bool all)
{
    NEED_DART(e);
    DartGrey g; int rc;
    if ((rc = dart_vol_id(vol)) || (rc = dart_greys(e, grey_host, nlevels, &g))) return rc;
    if ((rc = order_after_async(e))) return rc;
    float *x;
    if ((rc = get_vol(e, vol, &x))) return rc;
    return dart_restore_launch(e, x, g, all);
}

int tomo_dart_restore(tomo_engine *e, int vol, const float *grey_host, int nlevels) { return dart_restore(e, vol, grey_host, nlevels, false); }
int tomo_dart_segment(tomo_engine *e, int vol, const float *grey_host, int nlevels) { return dart_restore(e, vol, grey_host, nlevels, true); }

int tomo_dart_arm(tomo_engine *e, int vol, int sino_b, int niter, const float *grey_host, int nlevels)
{
    NEED_DART(e);
    DartGrey g; int rc;
    if ((rc = dart_vol_id(vol)) || (rc = dart_greys(e, grey_host, nlevels, &g))) return rc;
    if (sino_b < 0 || sino_b >= TOMO_SINO_SLOTS) return fail(TOMO_ERR_ARG, "bad sinogram id");
    if (niter < 0) return fail(TOMO_ERR_ARG, "negative iteration count");
    for (int it = 0; it < niter; ++it) {
        if ((rc = tomo_sirt_data(e, vol, sino_b, 1))) return rc;
        float *x;
        if ((rc = get_vol(e, vol, &x)) || (rc = dart_restore_launch(e, x, g, false))) return rc;
    }
    return TOMO_OK;
}

int tomo_dart_smooth(tomo_engine *e, int src, int dst, float beta)
{
    NEED_DART(e);
    int rc;
    if ((rc = dart_vol_id(src)) || (rc = dart_vol_id(dst))) return rc;
    if (src == dst) return fail(TOMO_ERR_ARG, "source and destination must be different volume slots");
    if (!(beta >= 0.f && beta <= 1.f)) return fail(TOMO_ERR_ARG, "beta must lie in [0, 1]");
    if (e->dart_nthr < 0) return fail(TOMO_ERR_STATE, "no segmentation in hand (tomo_dart_classify)");
    if ((rc = order_after_async(e))) return rc;
    float *s, *d;
    // dst first: where RECON_OLD still shares RECON's buffer (Claims::write) and the two are src and dst, get_vol makes the copy real,
    // so that two different slot ids are two different buffers by the time src is looked up -- nothing is left to refuse from here on
    if ((rc = get_vol(e, dst, &d)) || (rc = get_vol_ro(e, src, &s))) return rc;
    const int yseg = dart_yseg(e, DART_SMOOTH_TZ);
    hipLaunchKernelGGL((k_dart_smooth<DART_SMOOTH_TZ>), dim3(dart_grid(e, DART_SMOOTH_TZ, yseg)), dim3(256), 0, e->stream, (const float *)s, d,
                       (const uint8_t *)e->dart_state, beta, e->n, e->nx, e->sx, yseg);
    LAUNCHCHK();
    return TOMO_OK;
}

int tomo_dart_class_stats(tomo_engine *e, int vol, const float *thr_host, int nthr, double *out_host)
{
    NEED_DART(e);
    DartThr thr; int rc;
    if ((rc = dart_vol_id(vol)) || (rc = dart_thresholds(thr_host, nthr, &thr))) return rc;
    if (!out_host) return fail(TOMO_ERR_ARG, "null output");
    float *x;
    if ((rc = get_vol_ro(e, vol, &x))) return rc;
    if (!e->dart_part) { if ((rc = dev_alloc(e, ENGINE, (void **)&e->dart_part, (size_t)(DART_STATS_BLOCKS + 1) * 32 * sizeof(double), false))) return rc; }
    const int64_t nvec = (int64_t)e->vol_elems() / 4;
    const int nblk = (int)std::min<int64_t>(DART_STATS_BLOCKS, (nvec + 255) / 256), nc = nthr + 1;
    double *out = e->dart_part + (size_t)DART_STATS_BLOCKS * 32;
    const dim3 grid(nblk), block(256);
    if (nc <= 2) hipLaunchKernelGGL((k_dart_class_stats<2>), grid, block, 0, e->stream, (const float *)x, thr, nthr, nvec, e->nx, e->sx, e->dart_part);
    else if (nc <= 4) hipLaunchKernelGGL((k_dart_class_stats<4>), grid, block, 0, e->stream, (const float *)x, thr, nthr, nvec, e->nx, e->sx, e->dart_part);
    else if (nc <= 8) hipLaunchKernelGGL((k_dart_class_stats<8>), grid, block, 0, e->stream, (const float *)x, thr, nthr, nvec, e->nx, e->sx, e->dart_part);
    else hipLaunchKernelGGL((k_dart_class_stats<16>), grid, block, 0, e->stream, (const float *)x, thr, nthr, nvec, e->nx, e->sx, e->dart_part);
    LAUNCHCHK();
    return reduce_tail([&] { hipLaunchKernelGGL(k_sum_rows_tree, dim3(2 * nc), dim3(256), 0, e->stream, (const double *)e->dart_part, out, nblk, 32); },
                       e, out, out_host, (size_t)2 * nc * sizeof(double));
}

int tomo_dart_get_state(tomo_engine *e, uint8_t *out_host)
{
    NEED_DART(e);
    if (!out_host) return fail(TOMO_ERR_ARG, "null output");
    if (e->dart_nthr < 0) return fail(TOMO_ERR_STATE, "no segmentation in hand (tomo_dart_classify)");
    const size_t bytes = (size_t)e->nx * e->npix;
    int rc;
    if ((rc = ensure_stage(e, bytes))) return rc;
    hipLaunchKernelGGL(k_dart_state_out, dim3((unsigned)((e->npix + 63) / 64), (unsigned)(e->sx / 64)), dim3(256), 0, e->stream,
                       (const uint8_t *)e->dart_state, (uint8_t *)e->stage, e->npix, e->nx, e->sx);
    LAUNCHCHK();
    HIPCHK(hipMemcpyAsync(out_host, e->stage, bytes, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return TOMO_OK;
}
