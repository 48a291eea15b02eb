// engine_api.inc -- part of tomo_engine.hip (ONE translation unit: the kernels are templates and asm blocks in headers; the host side is
// split by topic into files that tomo_engine.hip includes in order).  This part: C ABI: lifetime, data in / out, projections, SIRT / Poisson-ML / CGLS / WBP (SART and ART: engine_sart.inc), the multimodal steps, scalars.


const char *tomo_last_error(void) { return g_err.c_str(); }

int tomo_device_count(int *count)
{
    if (!count) return fail(TOMO_ERR_ARG, "null count");
    int n = 0;
    hipError_t err = hipGetDeviceCount(&n);
    if (err != hipSuccess) { n = 0; (void)hipGetLastError(); }
    *count = n;
    return TOMO_OK;
}

int tomo_system_matrix(int nray, int nproj, const double *angles_rad, int64_t cap, float *rows, float *cols,
                       float *vals, int64_t *nnz)
{
    if (!angles_rad || !nnz) return fail(TOMO_ERR_ARG, "null argument");
    int rc = check_dims(1, nray, nproj);
    if (rc) return rc;
    Coo m;
    build_parallel_ray(nray, nproj, angles_rad, m);
    *nnz = m.ptr[m.nrow];
    if (cap == 0) return TOMO_OK;
    if (cap < *nnz || !rows || !cols || !vals) return fail(TOMO_ERR_ARG, "output capacity too small");
    for (int64_t r = 0; r < m.nrow; ++r)
        for (int64_t k = m.ptr[r]; k < m.ptr[r + 1]; ++k) { rows[k] = (float)r; cols[k] = (float)m.col[k]; vals[k] = m.val[k]; }
    return TOMO_OK;
}

int tomo_create(int nslice, int nray, int nproj, const double *angles_rad, int device, tomo_engine **out)
{
    if (!angles_rad || !out) return fail(TOMO_ERR_ARG, "null argument");
    int rc = check_dims(nslice, nray, nproj);
    if (rc) return rc;
    tomo_engine *e = new_engine(nslice, nray, nproj, device);
    const double t_begin = std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
    e->angles.assign(angles_rad, angles_rad + nproj);
    Coo m;
    build_parallel_ray(nray, nproj, angles_rad, m);
    return finish_create(e, m, out, t_begin);
}

int tomo_create_from_matrix(int nslice, int nray, int nproj, int64_t nnz, const float *rows, const float *cols,
                            const float *vals, int device, tomo_engine **out)
{
    if (!rows || !cols || !vals || !out) return fail(TOMO_ERR_ARG, "null argument");
    int rc = check_dims(nslice, nray, nproj);
    if (rc) return rc;
    const double t_begin = std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
    Coo m;
    std::string err;
    if (!coo_from_triplets((int64_t)nray * nproj, (int64_t)nray * nray, nnz, rows, cols, vals, m, err))
        return fail(TOMO_ERR_ARG, err);
    tomo_engine *e = new_engine(nslice, nray, nproj, device);
    return finish_create(e, m, out, t_begin);
}

// every device buffer that depends on the tilt geometry (tables, sinograms, scratch sized by it); volumes stay
static void free_geometry(tomo_engine *e)
{
    e->pool.release_life(GEOMETRY);
    e->rs_ok = false; e->rs_angs_cap = 0; e->rs_angs_host.clear(); e->seg_ready = false;
    e->pdhg_begun = false;
    e->claims.geometry_released();
    e->geometry_released = true;
}

// wait for everything the engine has enqueued (its stream, its second stream, every sub-stream): no evaluation is pending then
static int quiesce(tomo_engine *e)
{
    HIPCHK(hipStreamSynchronize(e->stream));
    if (e->aux) HIPCHK(hipStreamSynchronize(e->aux));
    for (int u = 0; u < tomo_engine::MAX_CHAINS; ++u) if (e->sub_stream[u]) HIPCHK(hipStreamSynchronize(e->sub_stream[u]));
    e->async_pending = false;
    return TOMO_OK;
}

static int same_slab(const tomo_engine *a, const tomo_engine *b)
{
    return a->nx != b->nx || a->n != b->n || a->sx != b->sx || a->device != b->device ? fail(TOMO_ERR_ARG, "engines differ in slab shape or device") : TOMO_OK;
}

int tomo_destroy(tomo_engine *e)
{
    if (!e) return TOMO_OK;
    (void)hipSetDevice(e->device);
    (void)quiesce(e);                               // (teardown goes on whatever a wait answers)
    if (e->aux) { (void)hipStreamDestroy(e->aux); (void)hipEventDestroy(e->ev_fork); (void)hipEventDestroy(e->ev_join); }
    for (int u = 0; u < tomo_engine::MAX_CHAINS; ++u) if (e->sub_stream[u]) { (void)hipStreamDestroy(e->sub_stream[u]); (void)hipEventDestroy(e->ev_sjoin[u]); }
    comm_release(e);
    if (e->ev_sfork) (void)hipEventDestroy(e->ev_sfork);
    if (e->ev_peer) (void)hipEventDestroy(e->ev_peer);
    if (e->ev_io) (void)hipEventDestroy(e->ev_io);
    if (e->ev_snap) (void)hipEventDestroy(e->ev_snap);
    if (e->h_snap) (void)hipHostFree(e->h_snap);
    if (e->rs_abort) (void)hipHostFree(e->rs_abort);
    if (e->rs_done) (void)hipHostFree(e->rs_done);
    e->pool.release_all();
    for (auto &p : e->prof) { for (auto ev : p.ev) (void)hipEventDestroy(ev); if (p.ref) (void)hipEventDestroy(p.ref); }
    if (e->own_stream && e->stream) (void)hipStreamDestroy(e->stream);
    delete e;
    return TOMO_OK;
}

// Rebuilding the tilt geometry with the reconstruction kept (tomoengine::update_projection_angles, tomoengine.cpp:128-149;
// ctvlib::update_proj_angles, ctvlib.cpp:317-333): release the old engine's tables and sinograms, create the new engine,
// let it adopt the old engine's volumes (pointers move, nothing is copied), destroy the old engine.
int tomo_release_geometry(tomo_engine *e)
{
    NEED(e);
    if (int rc = quiesce(e)) return rc;
    free_geometry(e);
    return TOMO_OK;
}

int tomo_adopt_volumes(tomo_engine *dst, tomo_engine *src)
{
    if (!dst || !src) return fail(TOMO_ERR_ARG, "null engine");
    if (int rc = same_slab(dst, src)) return rc;
    HIPCHK(hipSetDevice(dst->device));
    if (int rc = quiesce(src)) return rc;           // nothing of src may still be reading the volumes that move
    HIPCHK(hipStreamSynchronize(dst->stream));
    for (int i = 0; i < TOMO_VOL_SLOTS; ++i) {      // (an error return in here leaves the volumes before i moved: it cannot fire for engines whose volumes are their own)
        if (!src->vol[i]) continue;
        if (dst->vol[i] && dst->pool.release(dst->vol[i])) return fail(TOMO_ERR_STATE, "a volume of the adopting engine is not its own");
        if (src->pool.move_to(dst->pool, src->vol[i], (void **)&dst->vol[i])) return fail(TOMO_ERR_STATE, "a volume of the adopted engine is not its own");
        src->vol[i] = nullptr;                     // (its entry's slot may be the partner of a swap: move_to nulls only a slot that held the address)
    }
    dst->claims.adopt(src->claims);
    return TOMO_OK;
}

int tomo_set_stream(tomo_engine *e, void *hip_stream)
{
    NEED(e);
    HIPCHK(hipStreamSynchronize(e->stream));
    if (e->own_stream) { HIPCHK(hipStreamDestroy(e->stream)); e->own_stream = false; }
    e->stream = (hipStream_t)hip_stream;
    return TOMO_OK;
}

int tomo_synchronize(tomo_engine *e) { NEED(e); HIPCHK(hipStreamSynchronize(e->stream)); return TOMO_OK; }
int tomo_get_device(tomo_engine *e, int *device) { if (!e || !device) return fail(TOMO_ERR_ARG, "null"); *device = e->device; return TOMO_OK; }
int tomo_get_dims(tomo_engine *e, int *nslice, int *nray, int *nproj, int64_t *nnz)
{
    if (!e) return fail(TOMO_ERR_ARG, "null engine");
    if (nslice) *nslice = e->nx;
    if (nray) *nray = e->n;
    if (nproj) *nproj = e->np;
    if (nnz) *nnz = e->nnz;
    return TOMO_OK;
}

// ---- data in / out ---------------------------------------------------------------------------------------
static int upload(tomo_engine *e, const float *host, float *dst, int64_t m)
{
    size_t bytes = (size_t)e->nx * m * sizeof(float);
    int rc = ensure_stage(e, bytes);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(e->stage, host, bytes, hipMemcpyHostToDevice, e->stream));
    dim3 grid((unsigned)((m + 31) / 32), (unsigned)((e->sx + 31) / 32)), block(256);
    hipLaunchKernelGGL(k_transpose_in, grid, block, 0, e->stream, e->stage, dst, e->nx, m, e->sx);
    LAUNCHCHK();
    HIPCHK(hipStreamSynchronize(e->stream));
    return TOMO_OK;
}

static int download(tomo_engine *e, const float *src, float *host, int64_t m)
{
    size_t bytes = (size_t)e->nx * m * sizeof(float);
    int rc = ensure_stage(e, bytes);
    if (rc) return rc;
    dim3 grid((unsigned)((m + 31) / 32), (unsigned)((e->sx + 31) / 32)), block(256);
    hipLaunchKernelGGL(k_transpose_out, grid, block, 0, e->stream, src, e->stage, e->nx, m, e->sx);
    LAUNCHCHK();
    HIPCHK(hipMemcpyAsync(host, e->stage, bytes, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return TOMO_OK;
}

int tomo_set_sinogram(tomo_engine *e, int which, const float *b)
{
    NEED(e);
    if (!b) return fail(TOMO_ERR_ARG, "null sinogram");
    float *dst; int rc = sino_slot(e, which, &dst); if (rc) return rc;
    return upload(e, b, dst, e->nrows);
}

int tomo_set_tilt_series(tomo_engine *e, const float *b) { return tomo_set_sinogram(e, TOMO_SINO_B, b); }

int tomo_get_sinogram(tomo_engine *e, int which, float *out)
{
    NEED(e);
    if (!out) return fail(TOMO_ERR_ARG, "null output");
    if (which == TOMO_SINO_YK_MODEL) {                   // the extrapolated point's projection, while it is one
        const float *yk = projection_in_hand(e, TOMO_VOL_YK);
        if (!yk) return fail(TOMO_ERR_STATE, "no projection of the extrapolated point in hand (tomo_fista_project_yk)");
        return download(e, yk, out, e->nrows);
    }
    float *src;
    int rc = sino_slot(e, which, &src);
    if (rc) return rc;
    return download(e, src, out, e->nrows);
}

int tomo_set_volume(tomo_engine *e, int vol, const float *data)
{
    NEED(e);
    { int rc_ = order_after_async(e); if (rc_) return rc_; }
    float *dst; int rc = get_vol(e, vol, &dst); if (rc) return rc;
    if (!data) return fail(TOMO_ERR_ARG, "null volume");
    return upload(e, data, dst, e->npix);
}

int tomo_get_volume(tomo_engine *e, int vol, float *data)
{
    NEED(e);
    float *src; int rc = get_vol_ro(e, vol, &src); if (rc) return rc;
    if (!data) return fail(TOMO_ERR_ARG, "null volume");
    return download(e, src, data, e->npix);
}

int tomo_set_slice(tomo_engine *e, int vol, int s, const float *img)
{
    NEED(e);
    { int rc_ = order_after_async(e); if (rc_) return rc_; }
    float *dst; int rc = get_vol(e, vol, &dst); if (rc) return rc;
    if (s < 0 || s >= e->nx || !img) return fail(TOMO_ERR_ARG, "slice index out of range");
    if ((rc = ensure_stage(e, e->npix * sizeof(float)))) return rc;
    HIPCHK(hipMemcpyAsync(e->stage, img, e->npix * sizeof(float), hipMemcpyHostToDevice, e->stream));
    hipLaunchKernelGGL(k_scatter_slice, dim3((unsigned)((e->npix + 255) / 256)), dim3(256), 0, e->stream, e->stage, dst, e->npix, e->sx, s);
    LAUNCHCHK();
    HIPCHK(hipStreamSynchronize(e->stream));
    return TOMO_OK;
}

int tomo_get_slice(tomo_engine *e, int vol, int s, float *img)
{
    NEED(e);
    float *src; int rc = get_vol_ro(e, vol, &src); if (rc) return rc;
    if (s < 0 || s >= e->nx || !img) return fail(TOMO_ERR_ARG, "slice index out of range");
    if ((rc = ensure_stage(e, e->npix * sizeof(float)))) return rc;
    hipLaunchKernelGGL(k_gather_slice, dim3((unsigned)((e->npix + 255) / 256)), dim3(256), 0, e->stream, src, e->stage, e->npix, e->sx, s);
    LAUNCHCHK();
    HIPCHK(hipMemcpyAsync(img, e->stage, e->npix * sizeof(float), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return TOMO_OK;
}

// ---- data in / out of device buffers of the caller (no staging buffer, no host wait) ------------------------------------------
// (check_device_buffer, io_fence, io_args, io_launch: engine_launch.inc)
int tomo_set_volume_device(tomo_engine *e, int vol, const void *dev, int dtype, int64_t nelems, void *hip_stream)
{
    NEED(e);
    int rc = io_args(e, dev, dtype, TOMO_SINO_PACKED, nelems, e->npix); if (rc) return rc;
    if ((rc = order_after_async(e))) return rc;
    float *dst; if ((rc = get_vol(e, vol, &dst))) return rc;
    return io_launch<true>(e, const_cast<void *>(dev), dst, e->npix, dtype, TOMO_SINO_PACKED, (hipStream_t)hip_stream);
}

int tomo_get_volume_device(tomo_engine *e, int vol, void *dev, int dtype, int64_t nelems, void *hip_stream)
{
    NEED(e);
    int rc = io_args(e, dev, dtype, TOMO_SINO_PACKED, nelems, e->npix); if (rc) return rc;
    float *src; if ((rc = get_vol_ro(e, vol, &src))) return rc;
    return io_launch<false>(e, dev, src, e->npix, dtype, TOMO_SINO_PACKED, (hipStream_t)hip_stream);
}

int tomo_set_sinogram_device(tomo_engine *e, int which, const void *dev, int dtype, int layout, int64_t nelems, void *hip_stream)
{
    NEED(e);
    int rc = io_args(e, dev, dtype, layout, nelems, e->nrows); if (rc) return rc;
    if ((rc = order_after_async(e))) return rc;      // (an evaluation on the second stream may still read B or G)
    float *dst; if ((rc = sino_slot(e, which, &dst))) return rc;
    return io_launch<true>(e, const_cast<void *>(dev), dst, e->nrows, dtype, layout, (hipStream_t)hip_stream);
}

int tomo_get_sinogram_device(tomo_engine *e, int which, void *dev, int dtype, int layout, int64_t nelems, void *hip_stream)
{
    NEED(e);
    int rc = io_args(e, dev, dtype, layout, nelems, e->nrows); if (rc) return rc;
    float *src;
    if (which == TOMO_SINO_YK_MODEL) {                   // the extrapolated point's projection, while it is one
        src = const_cast<float *>(projection_in_hand(e, TOMO_VOL_YK));
        if (!src) return fail(TOMO_ERR_STATE, "no projection of the extrapolated point in hand (tomo_fista_project_yk)");
    } else if ((rc = sino_slot(e, which, &src))) return rc;
    return io_launch<false>(e, dev, src, e->nrows, dtype, layout, (hipStream_t)hip_stream);
}

int tomo_restart_recon(tomo_engine *e)
{
    NEED(e);
    { int rc_ = order_after_async(e); if (rc_) return rc_; }
    HIPCHK(hipMemsetAsync(e->vol[TOMO_VOL_RECON], 0, e->vol_elems() * sizeof(float), e->stream));
    if (e->vol[TOMO_VOL_YK]) HIPCHK(hipMemsetAsync(e->vol[TOMO_VOL_YK], 0, e->vol_elems() * sizeof(float), e->stream));
    if (e->vol[TOMO_VOL_RECON_OLD]) HIPCHK(hipMemsetAsync(e->vol[TOMO_VOL_RECON_OLD], 0, e->vol_elems() * sizeof(float), e->stream));
    e->claims.restarted();
    return TOMO_OK;
}

int tomo_copy_volume(tomo_engine *e, int dst, int src)
{
    NEED(e);
    { int rc_ = order_after_async(e); if (rc_) return rc_; }
    float *d, *s; int rc;
    const bool g_src = g_is_projection_of(e, src);
    if ((rc = get_vol(e, dst, &d)) || (rc = get_vol_ro(e, src, &s))) return rc;
    if (d != s) HIPCHK(hipMemcpyAsync(d, s, e->vol_elems() * sizeof(float), hipMemcpyDeviceToDevice, e->stream));
    e->claims.copied(dst, src, g_src);
    return TOMO_OK;
}

// ---- projector ------------------------------------------------------------------------------------------------
int tomo_forward_projection(tomo_engine *e, int vol, int sino)
{
    NEED(e);
    { int rc_ = order_after_async(e); if (rc_) return rc_; }
    float *x, *g; int rc;
    if ((rc = get_vol_ro(e, vol, &x))) return rc;
    if ((rc = sino_slot(e, sino, &g))) return rc;
    if ((rc = launch_fp_all<FP_STORE>(e, x, nullptr, g))) return rc;
    if (sino == TOMO_SINO_G) e->claims.g_projected_from(vol);
    return TOMO_OK;
}

int tomo_back_projection(tomo_engine *e, int sino, int vol)
{
    NEED(e);
    float *x, *g; int rc;
    if ((rc = get_vol(e, vol, &x))) return rc;
    if ((rc = sino_slot(e, sino, &g))) return rc;
    return launch_bp_all(e, x, g, nullptr, 0.f, 1.f, 0);
}

int tomo_lipschitz(tomo_engine *e, float *L) { if (!e || !L) return fail(TOMO_ERR_ARG, "null"); *L = e->lipschitz; return TOMO_OK; }
int tomo_lipschitz_cimmino(tomo_engine *e, float *L) { if (!e || !L) return fail(TOMO_ERR_ARG, "null"); *L = e->lipschitz_cimmino; return TOMO_OK; }
int tomo_row_inner_product(tomo_engine *e) { if (!e) return fail(TOMO_ERR_ARG, "null engine"); return TOMO_OK; /* built with the tables */ }

// ---- reconstruction steps -----------------------------------------------------------------------------------------
int tomo_sirt_landweber(tomo_engine *e, int vol, float beta, int niter)
{
    NEED(e);
    float *x, *r; int rc;
    if ((rc = get_vol(e, vol, &x)) || (rc = get_sino(e, &e->sino[TOMO_SINO_R], &r))) return rc;
    for (int it = 0; it < niter; ++it) {
        if ((rc = launch_fp_all<FP_RESID>(e, x, e->sino[TOMO_SINO_B], r))) return rc;
        if ((rc = launch_bp_all(e, x, r, nullptr, 1.f, beta, 1))) return rc;
    }
    return TOMO_OK;
}

// ctvlib::SIRT(beta) with cimminos_method() active: x += A^T M (b - A x) * beta/Nrow, M = diag(|A_i|^2) (sic: the
// reference multiplies by the row norms, quirk Q10), then positivity   ctvlib.cpp:212-216, 245-251
int tomo_sirt_cimmino(tomo_engine *e, int vol, float beta, int niter)
{
    NEED(e);
    float *x, *r; int rc;
    if ((rc = get_vol(e, vol, &x)) || (rc = get_sino(e, &e->sino[TOMO_SINO_R], &r))) return rc;
    for (int it = 0; it < niter; ++it) {
        if ((rc = launch_fp_all<FP_RESID_MUL>(e, x, e->sino[TOMO_SINO_B], r, e->d_rowinner))) return rc;   // the epilogue's per-row factor: |A_i|^2
        if ((rc = launch_bp_all(e, x, r, nullptr, 1.f, beta / (float)e->nrows, 1))) return rc;
    }
    return TOMO_OK;
}

int tomo_sirt(tomo_engine *e, int vol, int niter) { return tomo_sirt_data(e, vol, TOMO_SINO_B, niter); }

int tomo_sirt_data(tomo_engine *e, int vol, int sino_b, int niter)
{
    NEED(e);
    float *x, *r, *b; int rc;
    const float *have = (niter > 0 && sino_b != TOMO_SINO_G) ? projection_in_hand(e, vol) : nullptr;   // A * this volume, as it stands
    const bool reuse = have != nullptr;
    if (reuse) { if ((rc = order_after_async(e))) return rc; }                            // (an evaluation on the second stream made it)
    if ((rc = get_vol(e, vol, &x)) || (rc = get_sino(e, &e->sino[TOMO_SINO_R], &r)) || (rc = sino_slot(e, sino_b, &b))) return rc;
    for (int it = 0; it < niter; ++it) {
        if (it == 0 && reuse) { if ((rc = launch_sino_resid<FP_RESID_NORM>(e, b, have, r))) return rc; }
        else if ((rc = launch_fp_all<FP_RESID_NORM>(e, x, b, r))) return rc;
        if ((rc = launch_bp_all(e, x, r, e->d_colsum_all, 1.f, 1.f, 1))) return rc;
    }
    return TOMO_OK;
}

int tomo_poisson_ml(tomo_engine *e, float lambda)
{
    int rc;
    if ((rc = tomo_poisson_residual(e, TOMO_VOL_RECON, TOMO_SINO_B, TOMO_SINO_R))) return rc;
    float *x;
    if ((rc = get_vol(e, TOMO_VOL_RECON, &x))) return rc;
    return launch_bp_all(e, x, e->sino[TOMO_SINO_R], nullptr, 1.f, -(lambda / e->lipschitz), 1);
}

int tomo_poisson_residual(tomo_engine *e, int vol, int sino_b, int sino_out)
{
    NEED(e);
    float *x, *b, *r; int rc;
    if ((rc = get_vol(e, vol, &x)) || (rc = sino_slot(e, sino_b, &b)) || (rc = sino_slot(e, sino_out, &r))) return rc;
    if ((rc = reduce_begin(e))) return rc;
    if ((rc = launch_fp_all<FP_POISSON>(e, x, b, r))) return rc;
    return reduce_end(e, TOMO_S_COST);
}

// ---- CGLS (TomoGPU.cgls; ASTRA CCudaCglsAlgorithm in the reference: tomoengine.cpp:207-229) -------------------------
// Standard CGLS on min ||A x - b||, restarted from the current volume at every call exactly like the reference
// (algo_cgls->initialize per call), independently per slice (alpha, beta are per-slice scalars), positivity at the end.
static int slice_sumsq(tomo_engine *e, const float *v, int64_t m, double *sums)
{
    const int cols = e->sx / 4, per = cols >= 256 ? 256 : (cols >= 128 ? 128 : 64);
    const int nby = (int)std::min<int64_t>(1024, std::max<int64_t>(1, (m + 63) / 64));   // workgroups along the rows
    const int rpb = (int)((m + nby - 1) / nby);
    if (!e->cg_part) { int rc = dev_alloc(e, ENGINE, (void **)&e->cg_part, (size_t)1024 * e->sx * sizeof(double), false); if (rc) return rc; }
    dim3 grid((unsigned)((cols + per - 1) / per), (unsigned)nby);
    hipLaunchKernelGGL(k_slice_sumsq, grid, dim3(256), 0, e->stream, v, e->cg_part, m, e->sx, rpb);
    LAUNCHCHK();
    hipLaunchKernelGGL(k_slice_sumsq_finish, dim3((e->sx + 255) / 256), dim3(256), 0, e->stream, (const double *)e->cg_part, sums, nby, e->sx);
    LAUNCHCHK();
    return TOMO_OK;
}

// grid of the per-slice axpy kernels: its stride (blocks * 256 float4) must be a multiple of sx/4 so that a thread keeps its
// slice group; sx is a multiple of 64, so sx/4 divides 256 * (sx/4) / gcd -- simply take a block count that is a multiple of sx/64
static unsigned slice_grid(const tomo_engine *e, int64_t n4)
{
    const int64_t unit = std::max(1, e->sx / 64);          // blocks per 4 rows... 256 float4 = 1024 floats = 1024/sx rows
    int64_t b = std::min<int64_t>((n4 + 255) / 256, 8192);
    b = std::max<int64_t>(unit, (b / unit) * unit);
    return (unsigned)b;
}

int tomo_cgls(tomo_engine *e, int vol, int niter)
{
    NEED(e);
    float *x, *r, *b, *w; int rc;
    const bool reuse_g = g_is_projection_of(e, vol);        // the restart's A x is already in G (a data_distance of this volume)
    if (reuse_g) { if ((rc = order_after_async(e))) return rc; }
    if ((rc = get_vol(e, vol, &x)) || (rc = get_sino(e, &e->sino[TOMO_SINO_R], &r)) || (rc = sino_slot(e, TOMO_SINO_B, &b))) return rc;
    if ((rc = get_scratch(e, &e->cg_p, &w)) || (rc = get_scratch(e, &e->cg_z, &w))) return rc;
    if ((rc = get_sino(e, &e->cg_w, &w))) return rc;
    if (!e->cg_sums) { if ((rc = dev_alloc(e, ENGINE, (void **)&e->cg_sums, 2 * e->sx * sizeof(double), true))) return rc; }
    if (!e->cg_coef) { if ((rc = dev_alloc(e, ENGINE, (void **)&e->cg_coef, e->sx * sizeof(float), true))) return rc; }
    double *gam = e->cg_sums, *tmp = e->cg_sums + e->sx;
    const int64_t nv = (int64_t)e->vol_elems(), ns = (int64_t)e->sino_elems();
    auto ratio = [&](const double *num, const double *den) {
        hipLaunchKernelGGL(k_slice_ratio, dim3((e->sx + 255) / 256), dim3(256), 0, e->stream, num, den, e->cg_coef, e->sx);
    };
    // r = b - A x ; z = A^T r ; p = z ; gamma = |z|^2
    if (reuse_g) { if ((rc = launch_sino_resid<FP_RESID>(e, b, e->sino[TOMO_SINO_G], r))) return rc; }
    else if ((rc = launch_fp_all<FP_RESID>(e, x, b, r))) return rc;
    if ((rc = launch_bp_all(e, e->cg_z, r, nullptr, 0.f, 1.f, 0))) return rc;
    HIPCHK(hipMemcpyAsync(e->cg_p, e->cg_z, nv * sizeof(float), hipMemcpyDeviceToDevice, e->stream));
    if ((rc = slice_sumsq(e, e->cg_z, e->npix, gam))) return rc;
    for (int it = 0; it < niter; ++it) {
        // w = A p ; alpha = gamma / |w|^2 ; x += alpha p ; r -= alpha w
        if ((rc = launch_fp_all<FP_STORE>(e, e->cg_p, nullptr, e->cg_w))) return rc;
        if ((rc = slice_sumsq(e, e->cg_w, e->nrows, tmp))) return rc;
        ratio(gam, tmp);
        hipLaunchKernelGGL(k_slice_axpy, dim3(slice_grid(e, nv / 4)), dim3(256), 0, e->stream, (f4 *)x, (const f4 *)e->cg_p, (const f4 *)e->cg_coef, 1.f, nv / 4, e->sx / 4);
        hipLaunchKernelGGL(k_slice_axpy, dim3(slice_grid(e, ns / 4)), dim3(256), 0, e->stream, (f4 *)r, (const f4 *)e->cg_w, (const f4 *)e->cg_coef, -1.f, ns / 4, e->sx / 4);
        // z = A^T r ; beta = |z|^2 / gamma ; gamma = |z|^2 ; p = z + beta p
        if ((rc = launch_bp_all(e, e->cg_z, r, nullptr, 0.f, 1.f, 0))) return rc;
        if ((rc = slice_sumsq(e, e->cg_z, e->npix, tmp))) return rc;
        ratio(tmp, gam);
        HIPCHK(hipMemcpyAsync(gam, tmp, e->sx * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
        hipLaunchKernelGGL(k_slice_xpay, dim3(slice_grid(e, nv / 4)), dim3(256), 0, e->stream, (f4 *)e->cg_p, (const f4 *)e->cg_z, (const f4 *)e->cg_coef, nv / 4, e->sx / 4);
        LAUNCHCHK();
    }
    return tomo_positivity(e, vol);
}

// ---- WBP / FBP (TomoGPU.wbp; ASTRA CCudaFilteredBackProjectionAlgorithm: tomoengine.cpp:317-347) ----------------------
// recon = scale * A^T (h * b): h = real-space filter taps h[0..N-1] (symmetric), built by the host for the named filter.
int tomo_fbp(tomo_engine *e, const float *taps_host, float scale, int apply_positivity)
{
    NEED(e);
    if (!taps_host) return fail(TOMO_ERR_ARG, "null filter");
    float *x, *b, *g; int rc;
    if ((rc = get_vol(e, TOMO_VOL_RECON, &x)) || (rc = sino_slot(e, TOMO_SINO_B, &b)) || (rc = get_sino(e, &e->sino[TOMO_SINO_R], &g))) return rc;
    if (!e->fbp_h) { if ((rc = dev_alloc(e, GEOMETRY, (void **)&e->fbp_h, e->n * sizeof(float), false))) return rc; }
    HIPCHK(hipMemcpyAsync(e->fbp_h, taps_host, e->n * sizeof(float), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    int nchunk = e->sxc / (64 * e->vec);
    int64_t waves = e->nrows * nchunk;
    dim3 grid((unsigned)((waves + 3) / 4)), block(256);
    with_vec(e->vec, [&](auto V) {
        hipLaunchKernelGGL((k_filter_rows<V()>), grid, block, 0, e->stream, b, g, e->fbp_h, e->n, (int)e->nrows, e->sx, nchunk);
    });
    LAUNCHCHK();
    return launch_bp_all(e, x, g, nullptr, 0.f, scale, apply_positivity ? 1 : 0);
}

int tomo_scale_volume(tomo_engine *e, int vol, float factor)
{
    NEED(e);
    { int rc_ = order_after_async(e); if (rc_) return rc_; }
    float *x; int rc; if ((rc = get_vol(e, vol, &x))) return rc;
    int64_t n4 = e->vol_elems() / 4;
    hipLaunchKernelGGL(k_scale, dim3(grid_1d(n4)), dim3(256), 0, e->stream, (f4 *)x, factor, n4);
    LAUNCHCHK();
    return TOMO_OK;
}

int tomo_sino_diff_norm_sq(tomo_engine *e, int a, int b, int slot)
{
    NEED(e);
    if (slot < 0 || slot >= TOMO_S_COUNT) return fail(TOMO_ERR_ARG, "bad scalar slot");
    float *pa, *pb; int rc;
    if ((rc = sino_slot(e, a, &pa)) || (rc = sino_slot(e, b, &pb))) return rc;
    if ((rc = reduce_begin(e))) return rc;
    int64_t n4 = e->sino_elems() / 4;
    hipLaunchKernelGGL(k_sqdiff, dim3(grid_1d(n4)), dim3(256), 0, e->stream, (const f4 *)pa, (const f4 *)pb, e->d_part, n4);
    LAUNCHCHK();
    return reduce_end(e, slot);
}

// per-projection maximum over (slices, rays): multimodal::rescale_projections (multimodal.cpp:323-327)
int tomo_sino_proj_max(tomo_engine *e, int sino, float *out_host)
{
    NEED(e);
    float *g; int rc; if ((rc = sino_slot(e, sino, &g))) return rc;
    if (!out_host) return fail(TOMO_ERR_ARG, "null output");
    if ((rc = ensure_stage(e, e->np * sizeof(float)))) return rc;
    hipLaunchKernelGGL(k_proj_max, dim3(e->np), dim3(256), 0, e->stream, g, e->stage, e->n, e->nx, e->sx);
    LAUNCHCHK();
    HIPCHK(hipMemcpyAsync(out_host, e->stage, e->np * sizeof(float), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return TOMO_OK;
}

int tomo_sino_proj_scale(tomo_engine *e, int sino, const float *div_host, const float *mul_host)
{
    NEED(e);
    float *g; int rc; if ((rc = sino_slot(e, sino, &g))) return rc;
    if (!div_host || !mul_host) return fail(TOMO_ERR_ARG, "null factors");
    if ((rc = ensure_stage(e, 2 * e->np * sizeof(float)))) return rc;
    HIPCHK(hipMemcpyAsync(e->stage, div_host, e->np * sizeof(float), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(e->stage + e->np, mul_host, e->np * sizeof(float), hipMemcpyHostToDevice, e->stream));
    hipLaunchKernelGGL(k_proj_scale, dim3(e->np), dim3(256), 0, e->stream, g, e->stage, e->n, e->sx);
    LAUNCHCHK();
    HIPCHK(hipStreamSynchronize(e->stream));
    return TOMO_OK;
}

// copy a volume between two engines of the same slab shape on one device (used when the tilt geometry is rebuilt:
// tomoengine::update_projection_angles, tomoengine.cpp:128-149, keeps the reconstruction)
int tomo_copy_volume_from(tomo_engine *dst, int dst_vol, tomo_engine *src, int src_vol)
{
    if (!dst || !src) return fail(TOMO_ERR_ARG, "null engine");
    int rc = same_slab(dst, src); if (rc) return rc;
    HIPCHK(hipSetDevice(dst->device));
    float *d, *s;
    if ((rc = get_vol(dst, dst_vol, &d)) || (rc = get_vol(src, src_vol, &s))) return rc;
    HIPCHK(hipStreamSynchronize(src->stream));
    HIPCHK(hipMemcpyAsync(d, s, dst->vol_elems() * sizeof(float), hipMemcpyDeviceToDevice, dst->stream));
    HIPCHK(hipStreamSynchronize(dst->stream));
    return TOMO_OK;
}

int tomo_get_stream(tomo_engine *e, void **out) { if (!e || !out) return fail(TOMO_ERR_ARG, "null"); *out = (void *)e->stream; return TOMO_OK; }

// ---- multimodal (ChemicalTomo) element-wise steps: two engines of equal slab size on one device/stream ----
static int mm_check(tomo_engine *a, tomo_engine *b, int nel)
{
    if (!a || !b) return fail(TOMO_ERR_ARG, "null engine");
    if (int rc = same_slab(a, b)) return rc;
    if (a->stream != b->stream) return fail(TOMO_ERR_STATE, "engines must share one stream (tomo_set_stream)");
    if (nel < 1 || nel > MM_MAX_EL) return fail(TOMO_ERR_ARG, "element count out of range");
    return TOMO_OK;
}

// model = Sigma * x^gamma = sum_e w_e x_e^gamma      multimodal.cpp:425-427 (fuse), :459-460
int tomo_mm_model(tomo_engine *ce, const int32_t *xvols, int nel, const float *w, float gamma, tomo_engine *he, int model_vol)
{
    int rc = mm_check(ce, he, nel); if (rc) return rc;
    HIPCHK(hipSetDevice(ce->device));
    MMArgs a{};
    a.nel = nel; a.gamma = gamma;
    for (int i = 0; i < nel; ++i) { float *p; if ((rc = get_vol(ce, xvols[i], &p))) return rc; a.x[i] = p; a.w[i] = w[i]; }
    float *m; if ((rc = get_vol(he, model_vol, &m))) return rc;
    int64_t n4 = ce->vol_elems() / 4;
    hipLaunchKernelGGL(k_mm_model, dim3(grid_1d(n4)), dim3(256), 0, ce->stream, a, (f4 *)m, n4);
    LAUNCHCHK();
    return TOMO_OK;
}

// x_e <- max(0, x_e - (lamC_over_L * uC_e - lamH * gamma x_e^(gamma-1) w_e (upd - model)))   multimodal.cpp:435-438,471
int tomo_mm_update(tomo_engine *ce, const int32_t *xvols, const int32_t *uvols, int nel, const float *w, float gamma,
                   float lamC_over_L, float lamH, tomo_engine *he, int upd_vol, int model_vol)
{
    int rc = mm_check(ce, he, nel); if (rc) return rc;
    HIPCHK(hipSetDevice(ce->device));
    MMArgs a{};
    a.nel = nel; a.gamma = gamma;
    for (int i = 0; i < nel; ++i) {
        float *p, *u;
        if ((rc = get_vol(ce, xvols[i], &p)) || (rc = get_vol(ce, uvols[i], &u))) return rc;
        a.x[i] = p; a.u[i] = u; a.w[i] = w[i];
    }
    float *upd = nullptr, *m = nullptr;
    if (lamH != 0.f) { if ((rc = get_vol(he, upd_vol, &upd)) || (rc = get_vol(he, model_vol, &m))) return rc; }
    int64_t n4 = ce->vol_elems() / 4;
    hipLaunchKernelGGL(k_mm_update, dim3(grid_1d(n4)), dim3(256), 0, ce->stream, a, (const f4 *)upd, (const f4 *)m, lamC_over_L, lamH, n4);
    LAUNCHCHK();
    return TOMO_OK;
}

int tomo_positivity(tomo_engine *e, int vol)
{
    NEED(e);
    { int rc_ = order_after_async(e); if (rc_) return rc_; }
    float *x; int rc; if ((rc = get_vol(e, vol, &x))) return rc;
    int64_t n4 = e->vol_elems() / 4;
    hipLaunchKernelGGL(k_clamp, dim3(grid_1d(n4)), dim3(256), 0, e->stream, (f4 *)x, n4);
    LAUNCHCHK();
    return TOMO_OK;
}

int tomo_soft_threshold(tomo_engine *e, int vol, float lambda)
{
    NEED(e);
    float *x; int rc; if ((rc = get_vol(e, vol, &x))) return rc;
    int64_t n4 = e->vol_elems() / 4;
    hipLaunchKernelGGL(k_soft_threshold, dim3(grid_1d(n4)), dim3(256), 0, e->stream, (f4 *)x, lambda, n4);
    LAUNCHCHK();
    return TOMO_OK;
}

int tomo_fista_momentum(tomo_engine *e, float beta)
{
    NEED(e);
    // recon <- yk is a rotation of the two buffers, recon_old <- recon a flag (get_vol), and yk_new = r + beta (r - old) lands in
    // the buffer recon has just left -- which, from the second step on, is also where `old` sits (old == recon then): the step
    // reads two volumes and writes one (round 2: two reads, three stores: 645 us at 512^3).  Same expression, same bits.
    { int rc_ = order_after_async(e); if (rc_) return rc_; }
    float *x, *yk, *old; int rc;
    if ((rc = get_vol_ro(e, TOMO_VOL_RECON, &x)) || (rc = get_vol_ro(e, TOMO_VOL_YK, &yk))) return rc;
    if ((rc = get_vol_ro(e, TOMO_VOL_RECON_OLD, &old))) return rc;   // (x itself where recon_old's content IS recon's)
    int64_t n4 = e->vol_elems() / 4;
    hipLaunchKernelGGL(k_momentum, dim3(grid_1d(n4)), dim3(256), 0, e->stream, (const f4 *)yk, (const f4 *)old, (f4 *)x, beta, n4);
    LAUNCHCHK();
    e->vol[TOMO_VOL_RECON] = yk;                          // the prox result r
    e->vol[TOMO_VOL_YK] = x;                              // r + beta (r - old), written over the buffer recon has left
    e->claims.nesterov_step(beta);                        // recon_old == r, not stored
    return TOMO_OK;
}

// FISTA's next gradient step projects yk = r + beta (r - r_old).  The driver has just projected r for its cost
// (gpu/reconstructor.py:121-155: data_distance after every iteration) and projected r_old one iteration earlier, and the projector
// is linear: A yk = (1 + beta) A r - beta A r_old, a pass over two sinograms (94 MB) instead of a projection of the volume.  Call it
// after data_distance(recon); it does nothing unless every piece is provably in place (G = A recon as it stands, recon / yk /
// recon_old untouched since the last tomo_fista_momentum, the saved A r_old from the very iterate recon_old holds), and then leaves
// G = A yk with the claim the next tomo_sirt on yk picks up ("fp_reuse").  *done = 1 when the projection was formed.  Not
// bit-identical to projecting yk (rounding of the combination, ~1e-7 of |b|): parity tests hold it to the oracle at 1e-5 like
// every other path.
int tomo_fista_project_yk(tomo_engine *e, int *done)
{
    NEED(e);
    if (done) *done = 0;
    const Claims::Linearity how = e->claims.linearity_begin(e->sino[TOMO_SINO_G] != nullptr);
    if (how == Claims::REFUSED) return TOMO_OK;
    { int rc_ = order_after_async(e); if (rc_) return rc_; }
    int rc; float *p, *q;
    if ((rc = get_sino(e, &e->g_prev, &p)) || (rc = get_sino(e, &e->g_yk, &q))) return rc;
    const float *g = e->sino[TOMO_SINO_G];
    const int64_t n4 = (int64_t)e->sino_elems() / 4;
    if (how == Claims::FORM) {   // q = A yk = (1 + beta) A r - beta A r_old; p = A r (the saved projection of the next step): one pass
        hipLaunchKernelGGL(k_sino_extrapolate, dim3(grid_1d(n4)), dim3(256), 0, e->stream, (const VecOf<4>::T *)g, (VecOf<4>::T *)p, (VecOf<4>::T *)q, e->claims.beta(), n4);
        LAUNCHCHK();
    } else {
        HIPCHK(hipMemcpyAsync(p, g, e->sino_elems() * sizeof(float), hipMemcpyDeviceToDevice, e->stream));   // first step: only save A r
    }
    // G is untouched: it stays A * recon, with its claim, and get_model_projections() returns what the reference's would
    if (e->claims.linearity_end(how) && done) *done = 1;
    return TOMO_OK;
}

// ---- scalars --------------------------------------------------------------------------------------------------------
// A x into G and |A x - b|^2 into TOMO_S_DD on lane ln.  (A buffer allocated in here is cleared on the main stream: the caller of another
// lane has them all in place before it forks.)
static int data_distance_on(tomo_engine *e, const Lane &ln, int vol)
{
    float *x, *g; int rc;
    if ((rc = get_vol_ro(e, vol, &x)) || (rc = get_sino(e, &e->sino[TOMO_SINO_G], &g))) return rc;
    if ((rc = reduce_begin(e, ln))) return rc;
    if ((rc = launch_fp_all<FP_DD>(e, ln, x, e->sino[TOMO_SINO_B], g))) return rc;
    e->claims.g_projected_from(vol);                    // FP_DD also stores g = A x
    return reduce_end(e, ln, TOMO_S_DD);
}

int tomo_data_distance_sq(tomo_engine *e, int vol)
{
    NEED(e);
    return data_distance_on(e, main_lane(e), vol);
}

// The data distance of a volume that the main sequence no longer modifies (e.g. the TEMP copy) can be evaluated on
// a second stream while the main stream goes on (ASD-POCS: the residual of the SART result next to the TV descent).
int tomo_data_distance_sq_async(tomo_engine *e, int vol)
{
    NEED(e);
    if (e->async_pending) return fail(TOMO_ERR_STATE, "an asynchronous evaluation is already in flight");
    if (!e->aux) {
        HIPCHK(hipStreamCreateWithFlags(&e->aux, hipStreamNonBlocking));
        HIPCHK(hipEventCreateWithFlags(&e->ev_fork, hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&e->ev_join, hipEventDisableTiming));
        if (int rc = dev_alloc(e, ENGINE, (void **)&e->d_part_aux, NPART * sizeof(double), true)) return rc;
    }
    float *tmp; int rc;
    if ((rc = get_vol_ro(e, vol, &tmp)) || (rc = get_sino(e, &e->sino[TOMO_SINO_G], &tmp))) return rc;   // allocate on the main stream
    HIPCHK(hipEventRecord(e->ev_fork, e->stream));
    HIPCHK(hipStreamWaitEvent(e->aux, e->ev_fork, 0));
    if ((rc = data_distance_on(e, aux_lane(e), vol))) return rc;
    HIPCHK(hipEventRecord(e->ev_join, e->aux));
    e->async_pending = true;
    return TOMO_OK;
}

int tomo_async_wait(tomo_engine *e)
{
    NEED(e);
    if (e->async_pending) {
        HIPCHK(hipStreamWaitEvent(e->stream, e->ev_join, 0));
        e->async_pending = false;
    }
    return TOMO_OK;
}

int tomo_diff_norm_sq(tomo_engine *e, int a, int b, int slot)
{
    NEED(e);
    if (slot < 0 || slot >= TOMO_S_COUNT) return fail(TOMO_ERR_ARG, "bad scalar slot");
    float *pa, *pb; int rc;
    if ((rc = get_vol_ro(e, a, &pa)) || (rc = get_vol_ro(e, b, &pb))) return rc;
    if ((rc = reduce_begin(e))) return rc;
    int64_t n4 = e->vol_elems() / 4;
    hipLaunchKernelGGL(k_sqdiff, dim3(grid_1d(n4)), dim3(256), 0, e->stream, (const f4 *)pa, (const f4 *)pb, e->d_part, n4);
    LAUNCHCHK();
    return reduce_end(e, slot);
}

int tomo_l1_norm(tomo_engine *e, int vol)
{
    NEED(e);
    float *x; int rc; if ((rc = get_vol_ro(e, vol, &x))) return rc;
    if ((rc = reduce_begin(e))) return rc;
    int64_t n4 = e->vol_elems() / 4;
    hipLaunchKernelGGL(k_l1, dim3(grid_1d(n4)), dim3(256), 0, e->stream, (const f4 *)x, e->d_part, n4);
    LAUNCHCHK();
    return reduce_end(e, TOMO_S_L1);
}

int tomo_read_scalars(tomo_engine *e, double *out, int count)
{
    NEED(e);
    if (!out || count < 0 || count > TOMO_S_COUNT) return fail(TOMO_ERR_ARG, "bad scalar count");
    { int rc = tomo_async_wait(e); if (rc) return rc; }
    HIPCHK(hipMemcpyAsync(out, e->d_scal, count * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return TOMO_OK;
}

// The scalars of an iteration without a pipeline bubble: the copy is enqueued behind the kernels that produce them, the host
// goes on enqueueing (the next SART sweep) and collects the values later (tomo_scalars_snapshot_read waits on the event only).
int tomo_scalars_snapshot(tomo_engine *e)
{
    NEED(e);
    { int rc = tomo_async_wait(e); if (rc) return rc; }        // device-side ordering behind the second stream's evaluation
    if (!e->h_snap) {
        HIPCHK(hipHostMalloc((void **)&e->h_snap, TOMO_S_COUNT * sizeof(double), hipHostMallocDefault));
        HIPCHK(hipEventCreateWithFlags(&e->ev_snap, hipEventDisableTiming));
    }
    hipLaunchKernelGGL(k_scalars_to_host, dim3(1), dim3(64), 0, e->stream, (const double *)e->d_scal, e->h_snap, (int)TOMO_S_COUNT);
    LAUNCHCHK();
    HIPCHK(hipEventRecord(e->ev_snap, e->stream));
    e->snap_pending = true;
    return TOMO_OK;
}

int tomo_scalars_snapshot_read(tomo_engine *e, double *out, int count)
{
    NEED(e);
    if (!out || count < 0 || count > TOMO_S_COUNT) return fail(TOMO_ERR_ARG, "bad scalar count");
    if (!e->snap_pending) return fail(TOMO_ERR_STATE, "no scalar snapshot in flight");
    HIPCHK(hipEventSynchronize(e->ev_snap));
    std::memcpy(out, e->h_snap, count * sizeof(double));
    e->snap_pending = false;
    return TOMO_OK;
}

int tomo_bind_scalar_buffer(tomo_engine *e, void *device_doubles)
{
    NEED(e);
    HIPCHK(hipStreamSynchronize(e->stream));
    e->d_scal = device_doubles ? (double *)device_doubles : e->d_scal_own;
    return TOMO_OK;
}
