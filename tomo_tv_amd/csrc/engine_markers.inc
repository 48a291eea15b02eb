// engine_markers.inc -- marker detection on a tilt series: template correlation and local maxima (tomo_sino_template_ncc,
// tomo_sino_peaks).
// Part of tomo_engine.hip (included inside its extern "C" block, after engine_condition.inc, whose cond_slot_ok it uses, with
// NEED_WHOLE of engine_tilt.inc and al_ensure of engine_align.inc); kernels: kernels_markers.hip.h.
//
// One whole-volume engine only, like the other alignment calls: a window crosses slab boundaries.  Everything that can be refused
// is refused before anything is enqueued or allocated.  Source slots are read-only views (no claim on TOMO_SINO_G is dropped); the
// destination goes through sino_slot, which drops the claim where it is G.

static int marker_radius_ok(int R) { return R >= 1 && R <= MK_RMAX; }

// Enqueued, no wait.  The template is normalised here in binary64 and goes through the engine's own host copy and the staging
// buffer in stream order, like the table of tomo_sino_intensity.
int tomo_sino_template_ncc(tomo_engine *e, int src, int dst, const float *template_host, int R, float var_floor)
{
    NEED_WHOLE(e);
    if (!template_host) return fail(TOMO_ERR_ARG, "null template");
    if (!cond_slot_ok(src) || !cond_slot_ok(dst)) return fail(TOMO_ERR_ARG, "bad sinogram id");
    if (src == dst) return fail(TOMO_ERR_ARG, "source and destination must be different sinogram slots");
    if (!marker_radius_ok(R)) return fail(TOMO_ERR_ARG, "the template radius must lie in 1..8");
    if (!(var_floor >= 0.f)) return fail(TOMO_ERR_ARG, "var_floor is negative or NaN");
    const int W2 = (2 * R + 1) * (2 * R + 1);
    double mean = 0.0, ss = 0.0;
    for (int k = 0; k < W2; ++k) {
        if (!std::isfinite(template_host[k])) return fail(TOMO_ERR_ARG, "non-finite template");
        mean += (double)template_host[k];
    }
    mean /= W2;
    for (int k = 0; k < W2; ++k) { const double t = (double)template_host[k] - mean; ss += t * t; }
    if (!(ss > 0.0)) return fail(TOMO_ERR_ARG, "the template is constant");
    { int rc_ = order_after_async(e); if (rc_) return rc_; }
    float *s, *d; int rc;
    if ((rc = sino_slot(e, dst, &d))) return rc;
    if ((rc = sino_slot_ro(e, src, &s))) return rc;
    if ((rc = ensure_stage(e, (size_t)W2 * sizeof(float)))) return rc;
    const double scale = 1.0 / std::sqrt(ss);
    e->mk_tmpl.resize(W2);
    for (int k = 0; k < W2; ++k) e->mk_tmpl[k] = (float)(((double)template_host[k] - mean) * scale);
    HIPCHK(hipMemcpyAsync(e->stage, e->mk_tmpl.data(), (size_t)W2 * sizeof(float), hipMemcpyHostToDevice, e->stream));
    const dim3 grid(e->sx / 64, (e->n + MK_ROWS - 1) / MK_ROWS, e->np);
    hipLaunchKernelGGL(k_sino_template_ncc, grid, dim3(256), 0, e->stream, (const float *)s, d, (const float *)e->stage, R,
                       var_floor * (float)W2, e->n, e->nx, e->sx);
    LAUNCHCHK();
    return TOMO_OK;
}

// Waits.  Device buffer: one counter per projection (256-byte aligned block), then the records, min(capacity, Nray * Nslice) per
// projection.  The counts come back first; then only the records that exist, and the host sorts every projection's by row-major
// index (unique, hence one result whatever order the atomics gave).
int tomo_sino_peaks(tomo_engine *e, int sino, int radius, float threshold, int capacity, int *count_host, int *records_host)
{
    NEED_WHOLE(e);
    if (!count_host || !records_host) return fail(TOMO_ERR_ARG, "null output");
    if (!cond_slot_ok(sino)) return fail(TOMO_ERR_ARG, "bad sinogram id");
    if (!marker_radius_ok(radius)) return fail(TOMO_ERR_ARG, "the peak radius must lie in 1..8");
    if (std::isnan(threshold)) return fail(TOMO_ERR_ARG, "the threshold is NaN");
    if (capacity < 1) return fail(TOMO_ERR_ARG, "capacity must be at least 1");
    { int rc_ = order_after_async(e); if (rc_) return rc_; }
    float *g; int rc;
    if ((rc = sino_slot_ro(e, sino, &g))) return rc;
    const int dcap = (int)std::min<int64_t>(capacity, (int64_t)e->n * e->nx);
    const size_t head = ((size_t)e->np * sizeof(int) + 255) / 256 * 256, rec_bytes = (size_t)dcap * 8 * sizeof(int);
    if ((rc = al_ensure(e, &e->mk_buf, &e->mk_bytes, head + (size_t)e->np * rec_bytes))) return rc;
    int *cnt = (int *)e->mk_buf;
    int4 *rec = (int4 *)((char *)e->mk_buf + head);
    HIPCHK(hipMemsetAsync(cnt, 0, (size_t)e->np * sizeof(int), e->stream));
    const dim3 grid((e->nx + 63) / 64, (e->n + MK_ROWS - 1) / MK_ROWS, e->np);
    hipLaunchKernelGGL(k_sino_peaks, grid, dim3(256), 0, e->stream, (const float *)g, cnt, rec, radius, threshold, dcap, e->n, e->nx, e->sx);
    LAUNCHCHK();
    HIPCHK(hipMemcpyAsync(count_host, cnt, (size_t)e->np * sizeof(int), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    int kmax = 0;
    for (int a = 0; a < e->np; ++a) kmax = std::max(kmax, std::min(count_host[a], dcap));
    if (!kmax) return TOMO_OK;
    struct Rec { int w[8]; };
    static_assert(sizeof(Rec) == 32, "eight 32-bit words");
    e->mk_host.resize((size_t)e->np * kmax * 8);
    HIPCHK(hipMemcpy2DAsync(e->mk_host.data(), (size_t)kmax * sizeof(Rec), rec, rec_bytes, (size_t)kmax * sizeof(Rec), e->np, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    const int nx = e->nx;
    for (int a = 0; a < e->np; ++a) {
        const int k = std::min(count_host[a], dcap);
        Rec *r = (Rec *)e->mk_host.data() + (size_t)a * kmax;
        std::sort(r, r + k, [nx](const Rec &p, const Rec &q) { return (int64_t)p.w[0] * nx + p.w[1] < (int64_t)q.w[0] * nx + q.w[1]; });
        std::memcpy(records_host + (size_t)a * capacity * 8, r, (size_t)k * sizeof(Rec));
    }
    return TOMO_OK;
}
