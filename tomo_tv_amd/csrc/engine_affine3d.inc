// engine_affine3d.inc -- a volume resampled by a 3-D affine map between two engines, or between two slots of one engine
// (tomo_volume_affine, tomo_volume_affine_axpy).
// Part of tomo_engine.hip (included inside its extern "C" block, after engine_dual.inc); kernel: kernels_affine3d.hip.h.
//
// Whole-volume engines on one device; neither may be a slab of a larger volume: the taps of a slab's boundary voxels live on its
// neighbours.  The sizes of the two engines are free.  Refusal, slot bookkeeping and ordering: the pair rules of engine_bin.inc; with
// one engine both fences fall away and the kernel runs on its stream alone.  The matrix travels as a kernel argument: no staging
// buffer, no host wait.

static int affine3d_pair(tomo_engine *src, tomo_engine *dst, int src_vol, int dst_vol, const double *m_host)
{
    const Pair p{src, dst, src_vol, dst_vol, false, "resampling"};
    if (int rc = pair_check(p, PAIR_ENGINES)) return rc;
    if (!m_host) return fail(TOMO_ERR_ARG, "null matrix");
    if (int rc = pair_check(p, PAIR_SLOTS)) return rc;
    if (src == dst && src_vol == dst_vol) return fail(TOMO_ERR_ARG, "within one engine the source and the destination must be two slots");
    if (int rc = pair_check(p, PAIR_DEVICE)) return rc;
    for (int i = 0; i < 12; ++i) if (!std::isfinite(m_host[i])) return fail(TOMO_ERR_ARG, "non-finite matrix entry");
    return pair_check(p, PAIR_STATE);
}

static int affine3d_launch(bool axpy, tomo_engine *src, int src_vol, tomo_engine *dst, int dst_vol, const double *m_host, float a, int clamp)
{
    int rc = affine3d_pair(src, dst, src_vol, dst_vol, m_host); if (rc) return rc;
    // the destination first: within one engine, a write access to RECON or RECON_OLD makes RECON_OLD's own copy real (get_vol), and
    // only then is the read-only view of the source the buffer that will still hold it when the kernel runs
    float *s, *d;
    if ((rc = get_vol(dst, dst_vol, &d)) || (rc = get_vol_ro(src, src_vol, &s))) return rc;
    if (s == d) return fail(TOMO_ERR_ARG, "the source and the destination slot share one buffer");
    if ((rc = bin_fence_in(src, dst))) return rc;
    Affine3 M;
    std::memcpy(M.m, m_host, sizeof M.m);
    const dim3 grid((unsigned)((dst->npix + AF_ROWS - 1) / AF_ROWS)), block(256);
    if (axpy) hipLaunchKernelGGL((k_volume_affine<true>), grid, block, 0, dst->stream, (const float *)s, d, M, src->nx, src->n, src->sx, dst->nx, dst->n, dst->sx, a, clamp ? 1 : 0);
    else hipLaunchKernelGGL((k_volume_affine<false>), grid, block, 0, dst->stream, (const float *)s, d, M, src->nx, src->n, src->sx, dst->nx, dst->n, dst->sx, 0.f, 0);
    LAUNCHCHK();
    return io_fence(dst, dst->stream, src->stream);
}

int tomo_volume_affine(tomo_engine *src, int src_vol, tomo_engine *dst, int dst_vol, const double *m_host)
{
    return affine3d_launch(false, src, src_vol, dst, dst_vol, m_host, 0.f, 0);
}

int tomo_volume_affine_axpy(tomo_engine *src, int src_vol, tomo_engine *dst, int dst_vol, const double *m_host, float a, int clamp)
{
    return affine3d_launch(true, src, src_vol, dst, dst_vol, m_host, a, clamp);
}
