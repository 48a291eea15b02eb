// engine_bin.inc -- resampling between two engines whose grids differ by a factor F = 2 or 4: sinogram and volume binning (fine ->
// coarse), trilinear prolongation (coarse -> fine).
// Part of tomo_engine.hip (included inside its extern "C" block, after engine_align.inc); kernels: kernels_bin.hip.h.
//
// The rules of every call on a pair of engines -- these three, engine_dual.inc, engine_affine3d.inc, engine_register3d.inc -- are stated
// here.  Two whole-volume engines on one device (the NEED_ALIGN rule for both; the later families also refuse a slab of a larger
// volume).  Everything that can be refused is refused before anything is enqueued or any engine state is touched, so a refused call
// leaves both engines as they were.  The kernel runs on the destination engine's stream, ordered behind the source engine's stream and
// the source stream behind it, by events (bin_fence_in before, io_fence after): no host wait.

// The checks the pair calls share.  A call names the steps it wants done now and puts its own checks between them, so that a call
// with several faults reports the one it always reported; within one pair_check the steps run in the order of their values.
// PAIR_STATE is NEED_ALIGN for a, then for b, then -- where `whole` names the operation -- neither engine a slab of a larger volume.
enum { PAIR_ENGINES = 1, PAIR_SLOTS = 2, PAIR_DEVICE = 4, PAIR_STATE = 8 };
struct Pair { tomo_engine *a, *b; int slot_a, slot_b; bool sino; const char *whole; };

static int pair_check(const Pair &p, int steps)
{
    if ((steps & PAIR_ENGINES) && (!p.a || !p.b)) return fail(TOMO_ERR_ARG, "null engine");
    const int nslots = p.sino ? (int)TOMO_SINO_SLOTS : (int)TOMO_VOL_SLOTS;
    if ((steps & PAIR_SLOTS) && (p.slot_a < 0 || p.slot_a >= nslots || p.slot_b < 0 || p.slot_b >= nslots))
        return fail(TOMO_ERR_ARG, p.sino ? "bad sinogram id" : "bad volume id");
    if ((steps & PAIR_DEVICE) && p.a->device != p.b->device) return fail(TOMO_ERR_ARG, "the engines live on different devices");
    if (!(steps & PAIR_STATE)) return TOMO_OK;
    NEED_ALIGN(p.a);
    NEED_ALIGN(p.b);
    if (p.whole && (!(p.a->is_first && p.a->is_last) || !(p.b->is_first && p.b->is_last)))
        return fail(TOMO_ERR_STATE, std::string(p.whole) + " needs whole volumes: an engine is a slab of a larger one (tomo_set_slab_edges)");
    return TOMO_OK;
}

// the geometry rule of the three calls; sino: the engines must also agree on the number of projections
static int bin_pair(tomo_engine *fine, tomo_engine *coarse, int factor, bool sino, int fine_slot, int coarse_slot)
{
    const Pair p{fine, coarse, fine_slot, coarse_slot, sino, nullptr};
    if (int rc = pair_check(p, PAIR_ENGINES)) return rc;
    if (fine == coarse) return fail(TOMO_ERR_ARG, "the fine and the coarse engine must be two engines");
    if (factor != 2 && factor != 4) return fail(TOMO_ERR_ARG, "factor must be 2 or 4");
    if (int rc = pair_check(p, PAIR_SLOTS | PAIR_DEVICE)) return rc;
    if (fine->n != factor * coarse->n)
        return fail(TOMO_ERR_ARG, "Nray of the fine engine (" + std::to_string(fine->n) + ") is not factor * Nray of the coarse one (" + std::to_string(coarse->n) + ")");
    if (coarse->nx != (fine->nx + factor - 1) / factor)
        return fail(TOMO_ERR_ARG, "Nslice of the coarse engine (" + std::to_string(coarse->nx) + ") is not ceil(Nslice of the fine one / factor)");
    if (sino && fine->np != coarse->np) return fail(TOMO_ERR_ARG, "the engines differ in the number of projections");
    return pair_check(p, PAIR_STATE);
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
