// engine_register3d.inc -- the Gauss-Newton normal equations of a rigid registration of two volumes (tomo_volume_affine_normal).
// Part of tomo_engine.hip (included inside its extern "C" block, after engine_affine3d.inc); kernel: kernels_register3d.hip.h.
//
// Whole-volume engines on one device, neither a slab of a larger volume; refusal and ordering: the pair rules of engine_bin.inc, the
// fixed engine in the place of the destination (the kernels run on its stream).  Both volumes are read-only views (get_vol_ro): no
// version moves, no claim is dropped, and the fixed and the moving volume may be one slot of one engine.  The workgroups' partial
// sums live in reg_part of the FIXED engine, [RG_BLOCKS + 1][32] doubles allocated at the first call (the last row: the result);
// every row that is read was written by the same call, so the buffer is never cleared.  The call waits for its 32 numbers.

int tomo_volume_affine_normal(tomo_engine *fixed, int fixed_vol, tomo_engine *moving, int moving_vol, const double *m_host, int margin,
                              double *out_host)
{
    const Pair p{moving, fixed, moving_vol, fixed_vol, false, "registration"};
    int rc;
    if ((rc = pair_check(p, PAIR_ENGINES))) return rc;
    if (!m_host) return fail(TOMO_ERR_ARG, "null matrix");
    if (!out_host) return fail(TOMO_ERR_ARG, "null output");
    if ((rc = pair_check(p, PAIR_SLOTS | PAIR_DEVICE))) return rc;
    for (int i = 0; i < 12; ++i) if (!std::isfinite(m_host[i])) return fail(TOMO_ERR_ARG, "non-finite matrix entry");
    if (margin < 0) return fail(TOMO_ERR_ARG, "negative margin");
    if ((rc = pair_check(p, PAIR_STATE))) return rc;
    if (2 * (int64_t)margin >= std::min(fixed->nx, fixed->n))
        return fail(TOMO_ERR_ARG, "the margin leaves no voxel of the fixed volume (2 * margin >= a size)");
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
    // the fence goes back to the moving engine even when a launch failed: the tail sees to it
    return reduce_tail([&] { hipLaunchKernelGGL(k_sum_rows_tree, dim3(RG_SUMS), dim3(256), 0, fixed->stream, (const double *)fixed->reg_part, out, nblk, RG_SUMS); },
                       fixed, out, out_host, RG_SUMS * sizeof(double), hipGetLastError(), moving);
}
