// engine_components.inc -- connected components of a thresholded volume: labels 1..K, per-component measurements, removal of
// chosen components (tomo_components_*).
// Part of tomo_engine.hip (included inside its extern "C" block, after engine_dart.inc, whose dart_vol_id it uses); kernels:
// kernels_components.hip.h.
//
// One whole-volume engine only, by the rule and in the words of the DART calls: a component crosses slab boundaries.  The label state
// (one int32 per real voxel in the public order [Nslice][Ny][Nz], one root count per 256 voxels, K records) belongs to the engine's
// registry, is allocated by tomo_components_label and kept until tomo_components_release.  Everything that can be refused is refused
// before anything is enqueued or allocated.

#define NEED_CC(e) do { NEED(e); if ((e)->comm) return fail(TOMO_ERR_STATE, "component labelling runs on one whole-volume engine: this engine has a communicator"); if ((uint64_t)(e)->nx * (uint64_t)(e)->npix >= ((uint64_t)1 << 31)) return fail(TOMO_ERR_ARG, "component labels are 32-bit: Nslice * N * N must be below 2^31"); } while (0)

static int cc_need_labels(const tomo_engine *e) { return e->cc_count < 0 ? fail(TOMO_ERR_STATE, "no labelling in hand (tomo_components_label)") : TOMO_OK; }

int tomo_components_label(tomo_engine *e, int vol, float lo, float hi, int connectivity, int64_t *count)
{
    NEED_CC(e);
    int rc;
    if (!count) return fail(TOMO_ERR_ARG, "null count");
    if ((rc = dart_vol_id(vol))) return rc;
    if (connectivity != 6 && connectivity != 26) return fail(TOMO_ERR_ARG, "connectivity must be 6 or 26");
    if (std::isnan(lo) || std::isnan(hi)) return fail(TOMO_ERR_ARG, "a bound is NaN");
    if (lo > hi) return fail(TOMO_ERR_ARG, "lo is above hi");
    float *x;
    if ((rc = get_vol_ro(e, vol, &x))) return rc;
    const int npix = (int)e->npix, nvox = e->nx * npix, nblk = (nvox + 255) / 256;
    if (!e->cc_label) { if ((rc = dev_alloc(e, ENGINE, (void **)&e->cc_label, (size_t)nvox * sizeof(int), false))) return rc; }
    if (!e->cc_counts) { if ((rc = dev_alloc(e, ENGINE, (void **)&e->cc_counts, ((size_t)nblk + 1) * sizeof(int), false))) return rc; }
    e->cc_count = -1;                                    // from here on the buffer holds THIS call's work: no labelling until it is complete
    e->cc_stats_done = false;
    const dim3 tiles((unsigned)((npix + 63) / 64), (unsigned)(e->sx / 64)), vox((unsigned)nblk), block(256);
    hipLaunchKernelGGL(k_cc_init, tiles, block, 0, e->stream, (const float *)x, e->cc_label, lo, hi, e->n, npix, e->nx, e->sx);
    LAUNCHCHK();
    if (connectivity == 6) hipLaunchKernelGGL((k_cc_merge<6>), vox, block, 0, e->stream, e->cc_label, e->n, npix, nvox);
    else hipLaunchKernelGGL((k_cc_merge<26>), vox, block, 0, e->stream, e->cc_label, e->n, npix, nvox);
    LAUNCHCHK();
    hipLaunchKernelGGL(k_cc_flatten, vox, block, 0, e->stream, e->cc_label, e->cc_counts, nvox);
    LAUNCHCHK();
    hipLaunchKernelGGL(k_cc_scan, dim3(1), dim3(1024), 0, e->stream, e->cc_counts, nblk);
    LAUNCHCHK();
    int K = 0;
    HIPCHK(hipMemcpyAsync(&K, e->cc_counts + nblk, sizeof(int), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    if ((size_t)K > e->cc_rec_cap) {                     // the stream is idle: the old records can go
        if (e->cc_rec) e->pool.release(e->cc_rec);
        e->cc_rec_cap = 0;
        if ((rc = dev_alloc(e, ENGINE, (void **)&e->cc_rec, (size_t)K * sizeof(CcRecord), false))) return rc;
        e->cc_rec_cap = (size_t)K;
    }
    if (K) {
        hipLaunchKernelGGL(k_cc_number, vox, block, 0, e->stream, e->cc_label, (const int *)e->cc_counts, e->cc_rec, nvox);
        LAUNCHCHK();
    }
    hipLaunchKernelGGL(k_cc_relabel, vox, block, 0, e->stream, e->cc_label, nvox);
    LAUNCHCHK();
    if (K) {
        hipLaunchKernelGGL(k_cc_roots, dim3((unsigned)((K + 255) / 256)), block, 0, e->stream, e->cc_label, (const CcRecord *)e->cc_rec, K);
        LAUNCHCHK();
    }
    HIPCHK(hipStreamSynchronize(e->stream));
    e->cc_count = K;
    *count = K;
    return TOMO_OK;
}

int tomo_components_get_labels(tomo_engine *e, int32_t *labels_host)
{
    NEED_CC(e);
    if (!labels_host) return fail(TOMO_ERR_ARG, "null output");
    if (int rc = cc_need_labels(e)) return rc;
    HIPCHK(hipMemcpyAsync(labels_host, e->cc_label, (size_t)e->nx * e->npix * sizeof(int), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return TOMO_OK;
}

// The measurements are taken by the first call after a labelling and kept with it.
int tomo_components_stats(tomo_engine *e, int64_t capacity, tomo_component *records_host)
{
    NEED_CC(e);
    static_assert(sizeof(tomo_component) == sizeof(CcRecord), "the record of the header and the kernels' are one layout");
    if (capacity < 0) return fail(TOMO_ERR_ARG, "negative capacity");
    if (capacity > 0 && !records_host) return fail(TOMO_ERR_ARG, "null output");
    if (int rc = cc_need_labels(e)) return rc;
    const int64_t K = e->cc_count, nout = std::min<int64_t>(K, capacity);
    if (!K) return TOMO_OK;
    if (!e->cc_stats_done) {
        const int yb = 16;
        const int64_t items = (int64_t)e->nx * ((e->n + yb - 1) / yb) * ((e->n + 63) / 64);
        hipLaunchKernelGGL(k_cc_stats, dim3((unsigned)((items + 3) / 4)), dim3(256), 0, e->stream, (const int *)e->cc_label, e->cc_rec, e->n, e->nx, yb);
        LAUNCHCHK();
        e->cc_stats_done = true;
    }
    if (nout) HIPCHK(hipMemcpyAsync(records_host, e->cc_rec, (size_t)nout * sizeof(CcRecord), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return TOMO_OK;
}

// Enqueued, no wait.  The table goes through the engine's own host copy and the staging buffer in stream order.
int tomo_components_keep(tomo_engine *e, int vol, const uint8_t *keep_host, int64_t n, float fill)
{
    NEED_CC(e);
    int rc;
    if (!keep_host) return fail(TOMO_ERR_ARG, "null table");
    if ((rc = dart_vol_id(vol)) || (rc = cc_need_labels(e))) return rc;
    if (n != e->cc_count + 1) return fail(TOMO_ERR_ARG, "the labelling has " + std::to_string(e->cc_count) + " components: the table must have one entry more, got " + std::to_string(n));
    if ((rc = order_after_async(e))) return rc;
    float *x;
    if ((rc = get_vol(e, vol, &x)) || (rc = ensure_stage(e, (size_t)n))) return rc;
    e->cc_keep.assign(keep_host, keep_host + n);
    HIPCHK(hipMemcpyAsync(e->stage, e->cc_keep.data(), (size_t)n, hipMemcpyHostToDevice, e->stream));
    const int npix = (int)e->npix;
    hipLaunchKernelGGL(k_cc_keep, dim3((unsigned)((npix + 63) / 64), (unsigned)(e->sx / 64)), dim3(256), 0, e->stream, x, (const int *)e->cc_label,
                       (const uint8_t *)e->stage, fill, npix, e->nx, e->sx);
    LAUNCHCHK();
    return TOMO_OK;
}

// Allowed on any engine (there is nothing to refuse in giving memory back); without a labelling it does nothing.
int tomo_components_release(tomo_engine *e)
{
    if (!e) return fail(TOMO_ERR_ARG, "null engine");
    HIPCHK(hipSetDevice(e->device));
    if (e->cc_label || e->cc_counts || e->cc_rec) HIPCHK(hipStreamSynchronize(e->stream));
    if (e->cc_label) e->pool.release(e->cc_label);
    if (e->cc_counts) e->pool.release(e->cc_counts);
    if (e->cc_rec) e->pool.release(e->cc_rec);
    e->cc_rec_cap = 0;
    e->cc_count = -1;
    e->cc_stats_done = false;
    return TOMO_OK;
}
