// engine_register3d.inc -- the Gauss-Newton normal equations of a rigid registration of two volumes (tomo_volume_affine_normal).
// Part of tomo_engine.hip (included inside its extern "C" block, after engine_affine3d.inc); kernel: kernels_register3d.hip.h.
//
// The rules of engine_affine3d.inc: whole-volume engines on one device, everything that can be refused is refused before anything is
// enqueued; with two engines the kernels run on the fixed engine's stream behind an event of the moving engine's, and the moving
// engine's stream then waits for them.  Both volumes are read-only views (get_vol_ro): no version moves, no claim is dropped, and the
// fixed and the moving volume may be one slot of one engine.  The workgroups' partial sums live in reg_part of the FIXED engine,
// [RG_BLOCKS + 1][32] doubles allocated at the first call (the last row: the result); every row that is read was written by the same
// call, so the buffer is never cleared.  The call waits for its 32 numbers.

int tomo_volume_affine_normal(tomo_engine *fixed, int fixed_vol, tomo_engine *moving, int moving_vol, const double *m_host, int margin,
                              double *out_host)
{
    if (!fixed || !moving) return fail(TOMO_ERR_ARG, "null engine");
    if (!m_host) return fail(TOMO_ERR_ARG, "null matrix");
    if (!out_host) return fail(TOMO_ERR_ARG, "null output");
    if (fixed_vol < 0 || fixed_vol >= TOMO_VOL_SLOTS || moving_vol < 0 || moving_vol >= TOMO_VOL_SLOTS) return fail(TOMO_ERR_ARG, "bad volume id");
    if (fixed->device != moving->device) return fail(TOMO_ERR_ARG, "the engines live on different devices");
    for (int i = 0; i < 12; ++i) if (!std::isfinite(m_host[i])) return fail(TOMO_ERR_ARG, "non-finite matrix entry");
    if (margin < 0) return fail(TOMO_ERR_ARG, "negative margin");
    NEED_ALIGN(moving);
    NEED_ALIGN(fixed);
    if (!(fixed->is_first && fixed->is_last) || !(moving->is_first && moving->is_last))
        return fail(TOMO_ERR_STATE, "registration needs whole volumes: an engine is a slab of a larger one (tomo_set_slab_edges)");
    if (2 * (int64_t)margin >= std::min(fixed->nx, fixed->n))
        return fail(TOMO_ERR_ARG, "the margin leaves no voxel of the fixed volume (2 * margin >= a size)");
    int rc;
    float *f, *g;
    if ((rc = get_vol_ro(fixed, fixed_vol, &f)) || (rc = get_vol_ro(moving, moving_vol, &g))) return rc;
    if (!fixed->reg_part) { if ((rc = dev_alloc(fixed, ENGINE, (void **)&fixed->reg_part, (size_t)(RG_BLOCKS + 1) * RG_SUMS * sizeof(double), false))) return rc; }
    if ((rc = bin_fence_in(moving, fixed))) return rc;
    Affine3 M;
    std::memcpy(M.m, m_host, sizeof M.m);
    const int nblk = (int)std::min<int64_t>(RG_BLOCKS, (fixed->npix + AF_ROWS - 1) / AF_ROWS);
    double *out = fixed->reg_part + (size_t)RG_BLOCKS * RG_SUMS;
    hipLaunchKernelGGL(k_volume_affine_normal, dim3(nblk), dim3(256), 0, fixed->stream, (const float *)f, (const float *)g, M, moving->nx,
                       moving->n, moving->sx, fixed->nx, fixed->n, fixed->sx, margin, fixed->reg_part);
    hipError_t launched = hipGetLastError();
    if (launched == hipSuccess) {
        hipLaunchKernelGGL(k_affine_normal_finish, dim3(RG_SUMS), dim3(256), 0, fixed->stream, (const double *)fixed->reg_part, out, nblk);
        launched = hipGetLastError();
    }
    rc = io_fence(fixed, fixed->stream, moving->stream);       // the fence goes back even when a launch failed
    HIPCHK(launched);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(out_host, out, RG_SUMS * sizeof(double), hipMemcpyDeviceToHost, fixed->stream));
    HIPCHK(hipStreamSynchronize(fixed->stream));
    return TOMO_OK;
}
