// engine_tilt.inc -- refinement of the per-projection tilt angles: the rotational derivative of a volume and the per-projection sums
// of the angle step (tomo_volume_rot_derivative, tomo_sino_tilt_normal).
// Part of tomo_engine.hip (included inside its extern "C" block, after engine_align.inc, whose NEED_ALIGN, al_ensure and reduce_tail
// it uses); kernels: kernels_tilt.hip.h.
//
// One whole-volume engine only, like the other alignment calls: the derivative's stencil lies inside a slice and would not mind a
// slab, but the sums are per projection over ALL slices, and nothing adds them across slabs.  Everything that can be refused is
// refused before anything is enqueued.

#define NEED_WHOLE(e) do { NEED_ALIGN(e); if (!((e)->is_first && (e)->is_last)) return fail(TOMO_ERR_STATE, "alignment runs on one whole-volume engine: this engine is a slab of a larger volume (tomo_set_slab_edges)"); } while (0)

int tomo_volume_rot_derivative(tomo_engine *e, int src_vol, int dst_vol)
{
    NEED_WHOLE(e);
    if (src_vol < 0 || src_vol >= TOMO_VOL_SLOTS || dst_vol < 0 || dst_vol >= TOMO_VOL_SLOTS) return fail(TOMO_ERR_ARG, "bad volume id");
    if (src_vol == dst_vol) return fail(TOMO_ERR_ARG, "the source and the destination must be two volume slots");
    const int64_t blocks = ((int64_t)e->npix * (e->sx / 4) + 255) / 256;
    if (blocks > INT32_MAX) return fail(TOMO_ERR_ARG, "the volume is too large for one launch");
    { int rc_ = order_after_async(e); if (rc_) return rc_; }
    // the destination first (the rule of engine_affine3d.inc): a write access to RECON or RECON_OLD makes RECON_OLD's own copy real,
    // and only then is the read-only view of the source the buffer that will still hold it when the kernel runs
    float *s, *d; int rc;
    if ((rc = get_vol(e, dst_vol, &d)) || (rc = get_vol_ro(e, src_vol, &s))) return rc;
    if (s == d) return fail(TOMO_ERR_ARG, "the source and the destination slot share one buffer");
    hipLaunchKernelGGL(k_vol_rot_derivative, dim3((unsigned)blocks), dim3(256), 0, e->stream, (const float *)s, d, e->n, e->sx);
    LAUNCHCHK();
    return TOMO_OK;
}

// The three slots are read-only views (no claim on TOMO_SINO_G is dropped, no version moves) and may coincide.  The workgroups'
// partial sums go to al_part, the result to al_out ([np][4] doubles); the call waits for them.
int tomo_sino_tilt_normal(tomo_engine *e, int b_sino, int g_sino, int d_sino, int margin, double *out_host)
{
    NEED_WHOLE(e);
    if (!out_host) return fail(TOMO_ERR_ARG, "null output");
    for (int id : {b_sino, g_sino, d_sino}) if (id < 0 || id >= TOMO_SINO_SLOTS) return fail(TOMO_ERR_ARG, "bad sinogram id");
    if (margin < 0) return fail(TOMO_ERR_ARG, "negative margin");
    if (2 * (int64_t)margin >= std::min(e->n, e->nx)) return fail(TOMO_ERR_ARG, "the margin leaves no sample of a projection (2 * margin >= a size)");
    { int rc_ = order_after_async(e); if (rc_) return rc_; }
    float *b, *g, *d; int rc;
    if ((rc = sino_slot_ro(e, b_sino, &b)) || (rc = sino_slot_ro(e, g_sino, &g)) || (rc = sino_slot_ro(e, d_sino, &d))) return rc;
    const int nblk = (e->n + TN_ROWS - 1) / TN_ROWS;
    if ((rc = al_ensure(e, (void **)&e->al_part, &e->al_part_bytes, (size_t)e->np * nblk * TN_SUMS * sizeof(double)))) return rc;
    if ((rc = al_ensure(e, (void **)&e->al_out, &e->al_out_bytes, (size_t)e->np * TN_SUMS * sizeof(double)))) return rc;
    hipLaunchKernelGGL(k_sino_tilt_normal, dim3(nblk, e->np), dim3(256), 0, e->stream, (const float *)b, (const float *)g, (const float *)d,
                       e->n, e->nx, e->sx, margin, e->al_part);
    LAUNCHCHK();
    return reduce_tail([&] { hipLaunchKernelGGL(k_sum_rows_ascending, dim3((e->np * TN_SUMS + 255) / 256), dim3(256), 0, e->stream,
                                                (const double *)e->al_part, e->al_out, e->np, nblk, TN_SUMS, (float *)nullptr, 0.0); },
                       e, e->al_out, out_host, (size_t)e->np * TN_SUMS * sizeof(double));
}
