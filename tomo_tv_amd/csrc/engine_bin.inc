// engine_bin.inc -- resampling between two engines whose grids differ by a factor F = 2 or 4: sinogram and volume binning (fine ->
// coarse), trilinear prolongation (coarse -> fine).
// Part of tomo_engine.hip (included inside its extern "C" block, after engine_align.inc); kernels: kernels_bin.hip.h.
//
// Two whole-volume engines on one device (the NEED_ALIGN rule for both).  Everything that can be refused is refused before anything is
// enqueued or any engine state is touched, so a refused call leaves both engines as they were.  The kernel runs on the destination
// engine's stream, ordered behind the source engine's stream and the source stream behind it, by events (io_fence): no host wait.

// a sinogram slot that is only read: allocated (zero) on first use like any slot, but asking for G does not drop its claim
static int sino_slot_ro(tomo_engine *e, int id, float **out)
{
    if (id < 0 || id >= TOMO_SINO_SLOTS) return fail(TOMO_ERR_ARG, "bad sinogram id");
    if (!e->sino[id]) { int rc = dev_alloc(e, GEOMETRY, (void **)&e->sino[id], e->sino_elems() * sizeof(float), true); if (rc) return rc; }
    *out = e->sino[id];
    return TOMO_OK;
}

// the geometry rule of the three calls; sino: the engines must also agree on the number of projections
static int bin_pair(tomo_engine *fine, tomo_engine *coarse, int factor, bool sino, int fine_slot, int coarse_slot)
{
    if (!fine || !coarse) return fail(TOMO_ERR_ARG, "null engine");
    if (fine == coarse) return fail(TOMO_ERR_ARG, "the fine and the coarse engine must be two engines");
    if (factor != 2 && factor != 4) return fail(TOMO_ERR_ARG, "factor must be 2 or 4");
    const int nslots = sino ? (int)TOMO_SINO_SLOTS : (int)TOMO_VOL_SLOTS;
    if (fine_slot < 0 || fine_slot >= nslots || coarse_slot < 0 || coarse_slot >= nslots) return fail(TOMO_ERR_ARG, sino ? "bad sinogram id" : "bad volume id");
    if (fine->device != coarse->device) return fail(TOMO_ERR_ARG, "the engines live on different devices");
    if (fine->n != factor * coarse->n)
        return fail(TOMO_ERR_ARG, "Nray of the fine engine (" + std::to_string(fine->n) + ") is not factor * Nray of the coarse one (" + std::to_string(coarse->n) + ")");
    if (coarse->nx != (fine->nx + factor - 1) / factor)
        return fail(TOMO_ERR_ARG, "Nslice of the coarse engine (" + std::to_string(coarse->nx) + ") is not ceil(Nslice of the fine one / factor)");
    if (sino && fine->np != coarse->np) return fail(TOMO_ERR_ARG, "the engines differ in the number of projections");
    NEED_ALIGN(fine);
    NEED_ALIGN(coarse);
    return TOMO_OK;
}

// src's stream -> (kernel on dst's stream) -> src's stream
static int bin_fence_in(tomo_engine *src, tomo_engine *dst)
{
    int rc;
    if ((rc = order_after_async(src)) || (rc = order_after_async(dst))) return rc;
    return io_fence(dst, src->stream, dst->stream);
}

int tomo_sino_bin(tomo_engine *fine, int sino, tomo_engine *coarse, int coarse_sino, int factor)
{
    int rc = bin_pair(fine, coarse, factor, true, sino, coarse_sino); if (rc) return rc;
    float *s, *d;
    if ((rc = sino_slot_ro(fine, sino, &s)) || (rc = sino_slot(coarse, coarse_sino, &d))) return rc;
    if ((rc = bin_fence_in(fine, coarse))) return rc;
    const int64_t rows = coarse->nrows;
    const dim3 grid((unsigned)((rows + 3) / 4), (unsigned)(coarse->sx / 64)), block(256);
    if (factor == 2) hipLaunchKernelGGL((k_sino_bin<2>), grid, block, 0, coarse->stream, (const float *)s, d, rows, fine->nx, fine->sx, coarse->nx, coarse->sx);
    else hipLaunchKernelGGL((k_sino_bin<4>), grid, block, 0, coarse->stream, (const float *)s, d, rows, fine->nx, fine->sx, coarse->nx, coarse->sx);
    LAUNCHCHK();
    return io_fence(coarse, coarse->stream, fine->stream);
}

int tomo_volume_bin(tomo_engine *fine, int vol, tomo_engine *coarse, int coarse_vol, int factor)
{
    int rc = bin_pair(fine, coarse, factor, false, vol, coarse_vol); if (rc) return rc;
    float *s, *d;
    if ((rc = get_vol_ro(fine, vol, &s)) || (rc = get_vol(coarse, coarse_vol, &d))) return rc;
    if ((rc = bin_fence_in(fine, coarse))) return rc;
    const dim3 grid((unsigned)((coarse->npix + 3) / 4), (unsigned)(coarse->sx / 64)), block(256);
    if (factor == 2) hipLaunchKernelGGL((k_volume_bin<2>), grid, block, 0, coarse->stream, (const float *)s, d, coarse->n, fine->nx, fine->sx, coarse->nx, coarse->sx);
    else hipLaunchKernelGGL((k_volume_bin<4>), grid, block, 0, coarse->stream, (const float *)s, d, coarse->n, fine->nx, fine->sx, coarse->nx, coarse->sx);
    LAUNCHCHK();
    return io_fence(coarse, coarse->stream, fine->stream);
}

int tomo_volume_prolong(tomo_engine *coarse, int vol, tomo_engine *fine, int fine_vol, int factor)
{
    int rc = bin_pair(fine, coarse, factor, false, fine_vol, vol); if (rc) return rc;
    float *s, *d;
    if ((rc = get_vol_ro(coarse, vol, &s)) || (rc = get_vol(fine, fine_vol, &d))) return rc;
    if ((rc = bin_fence_in(coarse, fine))) return rc;
    const int64_t groups = (int64_t)(coarse->n + 1) * (coarse->n + 1);
    const dim3 grid((unsigned)((groups + 3) / 4), (unsigned)(fine->sx / 64)), block(256);
    if (factor == 2) hipLaunchKernelGGL((k_volume_prolong<2>), grid, block, 0, fine->stream, (const float *)s, d, coarse->n, coarse->nx, coarse->sx, fine->nx, fine->sx);
    else hipLaunchKernelGGL((k_volume_prolong<4>), grid, block, 0, fine->stream, (const float *)s, d, coarse->n, coarse->nx, coarse->sx, fine->nx, fine->sx);
    LAUNCHCHK();
    return io_fence(fine, fine->stream, coarse->stream);
}
