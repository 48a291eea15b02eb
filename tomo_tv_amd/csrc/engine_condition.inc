// engine_condition.inc -- conditioning of a tilt series: window statistics, outlier removal by a local median, per-projection gain
// and offset (tomo_sino_window_stats, tomo_sino_median, tomo_sino_intensity).
// Part of tomo_engine.hip (included inside its extern "C" block, after engine_tilt.inc, whose NEED_WHOLE it uses, with al_ensure and
// reduce_tail of engine_align.inc); kernels: kernels_condition.hip.h.
//
// One whole-volume engine only, like the other alignment calls: the sums are per projection over ALL slices and the median's window
// crosses slab boundaries.  Everything that can be refused is refused before anything is enqueued or allocated.  Source slots are
// read-only views (no claim on TOMO_SINO_G is dropped); the destination goes through sino_slot, which drops the claim where it is G.

static int cond_slot_ok(int id) { return id >= 0 && id < TOMO_SINO_SLOTS; }

int tomo_sino_window_stats(tomo_engine *e, int sino, int r0, int r1, int s0, int s1, double *out_host)
{
    NEED_WHOLE(e);
    if (!out_host) return fail(TOMO_ERR_ARG, "null output");
    if (!cond_slot_ok(sino)) return fail(TOMO_ERR_ARG, "bad sinogram id");
    if (r0 < 0 || r1 > e->n || r0 >= r1 || s0 < 0 || s1 > e->nx || s0 >= s1) return fail(TOMO_ERR_ARG, "the window is empty or leaves the image");
    { int rc_ = order_after_async(e); if (rc_) return rc_; }
    float *g; int rc;
    if ((rc = sino_slot_ro(e, sino, &g))) return rc;
    const int nblk = (r1 - r0 + WS_ROWS - 1) / WS_ROWS;
    if ((rc = al_ensure(e, (void **)&e->al_part, &e->al_part_bytes, (size_t)e->np * nblk * 4 * sizeof(double)))) return rc;
    if ((rc = al_ensure(e, (void **)&e->al_out, &e->al_out_bytes, (size_t)e->np * 4 * sizeof(double)))) return rc;
    hipLaunchKernelGGL(k_sino_window_stats, dim3(nblk, e->np), dim3(256), 0, e->stream, (const float *)g, e->al_part, e->n, e->sx, r0, r1, s0, s1);
    LAUNCHCHK();
    return reduce_tail([&] { hipLaunchKernelGGL(k_window_stats_finish, dim3((e->np * 4 + 255) / 256), dim3(256), 0, e->stream,
                                                (const double *)e->al_part, e->al_out, e->np, nblk); },
                       e, e->al_out, out_host, (size_t)e->np * 4 * sizeof(double));
}

int tomo_sino_median(tomo_engine *e, int src, int dst, int radius, const float *thresh_host, double *out_host)
{
    NEED_WHOLE(e);
    if (!out_host) return fail(TOMO_ERR_ARG, "null output");
    if (!cond_slot_ok(src)) return fail(TOMO_ERR_ARG, "bad sinogram id");
    if (radius != 1 && radius != 2) return fail(TOMO_ERR_ARG, "radius must be 1 or 2");
    if (thresh_host) {
        if (!cond_slot_ok(dst)) return fail(TOMO_ERR_ARG, "bad sinogram id");
        if (src == dst) return fail(TOMO_ERR_ARG, "source and destination must be different sinogram slots");
        for (int a = 0; a < e->np; ++a) if (!(thresh_host[a] >= 0.f)) return fail(TOMO_ERR_ARG, "a threshold is negative or NaN");
    } else if (dst != -1) return fail(TOMO_ERR_ARG, "a measuring call (no thresholds) writes nothing: its destination must be -1");
    { int rc_ = order_after_async(e); if (rc_) return rc_; }
    float *s, *d = nullptr; int rc;
    if (thresh_host && (rc = sino_slot(e, dst, &d))) return rc;
    if ((rc = sino_slot_ro(e, src, &s))) return rc;
    const int nchunk = (e->nx + 63) / 64, nrb = (e->n + MD_ROWS - 1) / MD_ROWS, nblk = nrb * nchunk;
    if ((rc = al_ensure(e, (void **)&e->al_part, &e->al_part_bytes, (size_t)e->np * nblk * 5 * sizeof(double)))) return rc;
    if ((rc = al_ensure(e, (void **)&e->al_out, &e->al_out_bytes, (size_t)e->np * 5 * sizeof(double)))) return rc;
    if (thresh_host) {
        if ((rc = ensure_stage(e, (size_t)e->np * sizeof(float)))) return rc;
        HIPCHK(hipMemcpyAsync(e->stage, thresh_host, (size_t)e->np * sizeof(float), hipMemcpyHostToDevice, e->stream));
    }
    const dim3 grid(nchunk, nrb, e->np), block(256);
    with_int<1, 2>(radius, [&](auto R) { with_flag(thresh_host != nullptr, [&](auto REPLACE) {
        hipLaunchKernelGGL((k_sino_median<R(), REPLACE()>), grid, block, 0, e->stream, (const float *)s, d, (const float *)e->stage, e->al_part,
                           e->n, e->nx, e->sx);
    }); });
    LAUNCHCHK();
    return reduce_tail([&] { hipLaunchKernelGGL(k_sum_rows_ascending, dim3((e->np * 5 + 255) / 256), dim3(256), 0, e->stream,
                                                (const double *)e->al_part, e->al_out, e->np, nblk, 5, (float *)nullptr, 0.0); },
                       e, e->al_out, out_host, (size_t)e->np * 5 * sizeof(double));       // its wait also covers the thresholds, read from the caller's host memory
}

// Enqueued, no wait.  The table goes through the engine's own host copy: an unpinned source of hipMemcpyAsync is consumed before the
// call returns, so neither the caller's memory nor the copy has to outlive it, and the device table (the staging buffer) is reused
// in stream order.
int tomo_sino_intensity(tomo_engine *e, int src, int dst, const float *gain_offset_host, int clamp)
{
    NEED_WHOLE(e);
    if (!gain_offset_host) return fail(TOMO_ERR_ARG, "null gains and offsets");
    if (!cond_slot_ok(src) || !cond_slot_ok(dst)) return fail(TOMO_ERR_ARG, "bad sinogram id");
    for (int i = 0; i < 2 * e->np; ++i) if (!std::isfinite(gain_offset_host[i])) return fail(TOMO_ERR_ARG, "non-finite gain or offset");
    { int rc_ = order_after_async(e); if (rc_) return rc_; }
    float *s, *d; int rc;
    if ((rc = sino_slot(e, dst, &d))) return rc;
    if (src == dst) s = d;
    else if ((rc = sino_slot_ro(e, src, &s))) return rc;
    if ((rc = ensure_stage(e, (size_t)e->np * sizeof(float2)))) return rc;
    e->cond_tab.assign(gain_offset_host, gain_offset_host + 2 * (size_t)e->np);
    HIPCHK(hipMemcpyAsync(e->stage, e->cond_tab.data(), (size_t)e->np * sizeof(float2), hipMemcpyHostToDevice, e->stream));
    const int blocks = (int)std::min<int64_t>(((int64_t)e->n * (e->sx / 4) + 255) / 256, 2048);
    with_flag(clamp != 0, [&](auto CLAMP) {
        hipLaunchKernelGGL((k_sino_intensity<CLAMP()>), dim3(blocks, e->np), dim3(256), 0, e->stream, (const float *)s, d, (const float2 *)e->stage,
                           e->n, e->nx, e->sx);
    });
    LAUNCHCHK();
    return TOMO_OK;
}
