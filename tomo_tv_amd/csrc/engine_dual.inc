// engine_dual.inc -- dual-axis tomography: the volume of one engine in the layout of an engine with the perpendicular tilt axis
// (tomo_volume_cross, tomo_volume_cross_axpy).
// Part of tomo_engine.hip (included inside its extern "C" block, after engine_bin.inc); kernel: kernels_dual.hip.h.
//
// Two whole-volume engines on one device, both cubes of the same N; neither may be a slab of a larger volume: crossing a slab is an
// all-to-all between the ranks.  Refusal, slot bookkeeping and ordering: the pair rules of engine_bin.inc.

static int cross_pair(tomo_engine *src, tomo_engine *dst, int src_vol, int dst_vol)
{
    const Pair p{src, dst, src_vol, dst_vol, false, "crossing the tilt axes"};
    if (int rc = pair_check(p, PAIR_ENGINES)) return rc;
    if (src == dst) return fail(TOMO_ERR_ARG, "the source and the destination engine must be two engines");
    if (int rc = pair_check(p, PAIR_SLOTS | PAIR_DEVICE)) return rc;
    if (src->nx != src->n || dst->nx != dst->n)
        return fail(TOMO_ERR_ARG, "both engines must hold a cube (Nslice == Nray): " + std::to_string(src->nx) + " x " + std::to_string(src->n) + "^2 and " +
                                      std::to_string(dst->nx) + " x " + std::to_string(dst->n) + "^2");
    if (src->n != dst->n) return fail(TOMO_ERR_ARG, "the engines differ in N (" + std::to_string(src->n) + " and " + std::to_string(dst->n) + ")");
    return pair_check(p, PAIR_STATE);
}

static int cross_launch(bool axpy, tomo_engine *src, int src_vol, tomo_engine *dst, int dst_vol, float a, int clamp)
{
    int rc = cross_pair(src, dst, src_vol, dst_vol); if (rc) return rc;
    float *s, *d;
    if ((rc = get_vol_ro(src, src_vol, &s)) || (rc = get_vol(dst, dst_vol, &d))) return rc;
    if ((rc = bin_fence_in(src, dst))) return rc;
    const int tiles_z = dst->sx / DX_T, tiles_s = (dst->n + DX_T - 1) / DX_T;
    const dim3 grid((unsigned)((int64_t)tiles_z * tiles_s * dst->n)), block(256);
    if (axpy) hipLaunchKernelGGL((k_volume_cross<true>), grid, block, 0, dst->stream, (const float *)s, d, dst->n, dst->sx, tiles_z, tiles_s, a, clamp ? 1 : 0);
    else hipLaunchKernelGGL((k_volume_cross<false>), grid, block, 0, dst->stream, (const float *)s, d, dst->n, dst->sx, tiles_z, tiles_s, 0.f, 0);
    LAUNCHCHK();
    return io_fence(dst, dst->stream, src->stream);
}

int tomo_volume_cross(tomo_engine *src, int src_vol, tomo_engine *dst, int dst_vol)
{
    return cross_launch(false, src, src_vol, dst, dst_vol, 0.f, 0);
}

int tomo_volume_cross_axpy(tomo_engine *src, int src_vol, tomo_engine *dst, int dst_vol, float a, int clamp)
{
    return cross_launch(true, src, src_vol, dst, dst_vol, a, clamp);
}
