// engine_align.inc -- tilt-series alignment: per-angle moments, windowed cross-correlation, resampling by per-angle shifts or affine
// maps, the normal equations of a per-projection similarity matching, per-slice mass profiles.
// Part of tomo_engine.hip (included inside its extern "C" block, after engine_api.inc); kernels: kernels_align.hip.h, kernels_align_normal.hip.h.
//
// One whole-volume engine only: a shift along the tilt axis moves samples across slab boundaries, so an engine bound to a
// communicator refuses (TOMO_ERR_STATE).  The buffers (partial sums, moments, means, the window) belong to the engine's registry and
// are kept: after the first call of a given size nothing is allocated.

static int al_ensure(tomo_engine *e, void **p, size_t *have, size_t bytes)
{
    if (*have >= bytes) return TOMO_OK;
    if (*p) { HIPCHK(hipStreamSynchronize(e->stream)); e->pool.release(*p); *p = nullptr; *have = 0; }
    if (int rc = dev_alloc(e, ENGINE, p, bytes, false)) return rc;
    *have = bytes;
    return TOMO_OK;
}

#define NEED_ALIGN(e) do { NEED(e); if ((e)->comm) return fail(TOMO_ERR_STATE, "alignment runs on one whole-volume engine: this engine has a communicator"); } while (0)

// The tail of every call that sums in two stages (kernels_geom.hip.h) and hands the result to the caller: the second stage (finish()
// launches it on e's stream) behind a first stage that was launched well, the copy of the result to the caller's memory, and the wait
// for it.  With a partner the first stage read a volume of another engine: the fence back to the partner's stream follows the
// launches and goes back even when one of them failed.
extern "C++" {
template <class Finish>
static int reduce_tail(Finish &&finish, tomo_engine *e, const double *dev, double *host, size_t bytes, hipError_t launched = hipSuccess,
                       tomo_engine *partner = nullptr)
{
    if (launched == hipSuccess) { finish(); launched = hipGetLastError(); }
    const int rc = partner ? io_fence(e, e->stream, partner->stream) : TOMO_OK;
    HIPCHK(launched);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return TOMO_OK;
}
}

// the moments of sinogram g, first stage: the workgroups' triples into al_part; enqueued, no wait
static int al_moments_part(tomo_engine *e, const float *g)
{
    const int nblk = (e->n + AL_MROWS - 1) / AL_MROWS;
    int rc;
    if ((rc = al_ensure(e, (void **)&e->al_part, &e->al_part_bytes, (size_t)e->np * nblk * 3 * sizeof(double)))) return rc;
    if (!e->al_mom) { if ((rc = dev_alloc(e, GEOMETRY, (void **)&e->al_mom, (size_t)2 * e->np * 3 * sizeof(double), false))) return rc; }
    if (!e->al_mean) { if ((rc = dev_alloc(e, GEOMETRY, (void **)&e->al_mean, (size_t)2 * e->np * sizeof(float), false))) return rc; }
    hipLaunchKernelGGL(k_sino_moments, dim3(nblk, e->np), dim3(256), 0, e->stream, g, e->al_part, e->n, e->nx, e->sx);
    LAUNCHCHK();
    return TOMO_OK;
}

// second stage: the moments into al_mom[which] ([np][3] doubles) and the means into al_mean[which] ([np] floats), in the one launch
static void al_moments_finish(tomo_engine *e, int which)
{
    hipLaunchKernelGGL(k_sum_rows_ascending, dim3((e->np * 3 + 255) / 256), dim3(256), 0, e->stream, (const double *)e->al_part,
                       e->al_mom + (size_t)which * e->np * 3, e->np, (e->n + AL_MROWS - 1) / AL_MROWS, 3, e->al_mean + (size_t)which * e->np,
                       (double)e->n * (double)e->nx);
}

// both stages; enqueued, no wait
static int al_moments(tomo_engine *e, const float *g, int which)
{
    if (int rc = al_moments_part(e, g)) return rc;
    al_moments_finish(e, which);
    LAUNCHCHK();
    return TOMO_OK;
}

int tomo_sino_moments(tomo_engine *e, int sino, double *out_host)
{
    NEED_ALIGN(e);
    if (!out_host) return fail(TOMO_ERR_ARG, "null output");
    { int rc_ = order_after_async(e); if (rc_) return rc_; }
    float *g; int rc;
    if ((rc = sino_slot(e, sino, &g)) || (rc = al_moments_part(e, g))) return rc;
    return reduce_tail([&] { al_moments_finish(e, 0); }, e, e->al_mom, out_host, (size_t)e->np * 3 * sizeof(double));
}

int tomo_sino_xcorr(tomo_engine *e, int sino_a, int sino_b, int max_shift, int subtract_mean, double *out_host)
{
    NEED_ALIGN(e);
    if (!out_host) return fail(TOMO_ERR_ARG, "null output");
    const int S = max_shift;
    if (S < 1 || S > 16 || S > std::min(e->n, e->nx) - 1) return fail(TOMO_ERR_ARG, "max_shift must be 1..16 and at most min(Nray, Nslice) - 1");
    { int rc_ = order_after_async(e); if (rc_) return rc_; }
    float *A, *B; int rc;
    if ((rc = sino_slot(e, sino_a, &A)) || (rc = sino_slot(e, sino_b, &B))) return rc;
    const float *mA = nullptr, *mB = nullptr;
    if (subtract_mean) {
        if ((rc = al_moments(e, A, 0)) || (rc = al_moments(e, B, 1))) return rc;
        mA = e->al_mean; mB = e->al_mean + e->np;
    }
    const int smax = S <= 4 ? 4 : (S <= 8 ? 8 : 16), wm = 2 * smax + 1, w = 2 * S + 1;
    const int nchunk = (e->nx + 63) / 64, ncg = (nchunk + AL_KC - 1) / AL_KC, nrb = (e->n + AL_R - 1) / AL_R, nblk = nrb * ncg;
    if ((rc = al_ensure(e, (void **)&e->al_part, &e->al_part_bytes, (size_t)e->np * nblk * wm * wm * sizeof(double)))) return rc;
    if ((rc = al_ensure(e, (void **)&e->al_out, &e->al_out_bytes, (size_t)e->np * 33 * 33 * sizeof(double)))) return rc;
    const dim3 grid(ncg, nrb, e->np), block(256);
    if (smax == 4) hipLaunchKernelGGL((k_sino_xcorr<4, 9, 9>), grid, block, 0, e->stream, A, B, mA, mB, e->al_part, e->n, e->nx, e->sx, nchunk);
    else if (smax == 8) hipLaunchKernelGGL((k_sino_xcorr<8, 9, 9>), grid, block, 0, e->stream, A, B, mA, mB, e->al_part, e->n, e->nx, e->sx, nchunk);
    else hipLaunchKernelGGL((k_sino_xcorr<16, 11, 11>), grid, block, 0, e->stream, A, B, mA, mB, e->al_part, e->n, e->nx, e->sx, nchunk);
    LAUNCHCHK();
    return reduce_tail([&] { hipLaunchKernelGGL(k_sino_xcorr_finish, dim3((e->np * w * w + 255) / 256), dim3(256), 0, e->stream,
                                                (const double *)e->al_part, e->al_out, e->np, nblk, smax, S); },
                       e, e->al_out, out_host, (size_t)e->np * w * w * sizeof(double));
}

// The axis split of kernels_geom.hip.h on the host, applied to -d, with the wrap and the pin of k that only this call needs:
// -d = k + t with k = floor(-d) and t in [0, 1).  k and the binary64 fraction are exact (d is a binary32 number); rounded to binary32
// the fraction of a tiny positive d (1 - 2^-30, say) becomes 1, which is the whole-pixel shift k + 1 and is passed on as such, so
// that the kernel's copy path takes it -- never a two-tap form with weights 0 and 1.  Without wrap a k beyond the image on either
// side is pinned just outside it (every tap is then outside: zeros); with wrap it is taken modulo size.
static void al_split(float d, int size, int wrap, int *k, float *t)
{
    const double nd = -(double)d;
    double fl = std::floor(nd);
    *t = (float)(nd - fl);
    if (*t >= 1.f) { *t = 0.f; fl += 1.0; }
    if (wrap) { double m = std::fmod(fl, (double)size); if (m < 0) m += size; *k = (int)m; }
    else *k = (int)std::max(-(double)size - 2.0, std::min((double)size + 2.0, fl));
}

int tomo_sino_shift(tomo_engine *e, int src, int dst, const float *shifts_host, int wrap)
{
    NEED_ALIGN(e);
    if (!shifts_host) return fail(TOMO_ERR_ARG, "null shifts");
    if (src == dst) return fail(TOMO_ERR_ARG, "source and destination must be different sinogram slots");
    for (int i = 0; i < 2 * e->np; ++i) if (!std::isfinite(shifts_host[i])) return fail(TOMO_ERR_ARG, "non-finite shift");
    { int rc_ = order_after_async(e); if (rc_) return rc_; }
    float *s, *d; int rc;
    if ((rc = sino_slot(e, src, &s)) || (rc = sino_slot(e, dst, &d))) return rc;
    if ((rc = ensure_stage(e, (size_t)e->np * sizeof(int4)))) return rc;
    std::vector<int4> tab(e->np);
    for (int a = 0; a < e->np; ++a) {
        float tr, ts;
        al_split(shifts_host[2 * a], e->n, wrap, &tab[a].x, &tr);
        al_split(shifts_host[2 * a + 1], e->nx, wrap, &tab[a].y, &ts);
        std::memcpy(&tab[a].z, &tr, 4); std::memcpy(&tab[a].w, &ts, 4);
    }
    HIPCHK(hipMemcpyAsync(e->stage, tab.data(), (size_t)e->np * sizeof(int4), hipMemcpyHostToDevice, e->stream));
    const int blocks = (int)std::min<int64_t>(((int64_t)e->n * e->sx + 255) / 256, 1024);
    const dim3 grid(blocks, e->np), block(256);
    if (wrap) hipLaunchKernelGGL((k_sino_shift<true>), grid, block, 0, e->stream, (const float *)s, d, (const int4 *)e->stage, e->n, e->nx, e->sx);
    else hipLaunchKernelGGL((k_sino_shift<false>), grid, block, 0, e->stream, (const float *)s, d, (const int4 *)e->stage, e->n, e->nx, e->sx);
    LAUNCHCHK();
    HIPCHK(hipStreamSynchronize(e->stream));        // the table is read from this call's host memory
    return TOMO_OK;
}

int tomo_sino_affine(tomo_engine *e, int src, int dst, const double *m_host)
{
    NEED_ALIGN(e);
    if (!m_host) return fail(TOMO_ERR_ARG, "null matrices");
    if (src == dst) return fail(TOMO_ERR_ARG, "source and destination must be different sinogram slots");
    for (int i = 0; i < 6 * e->np; ++i) if (!std::isfinite(m_host[i])) return fail(TOMO_ERR_ARG, "non-finite matrix entry");
    { int rc_ = order_after_async(e); if (rc_) return rc_; }
    float *s, *d; int rc;
    if ((rc = sino_slot(e, src, &s)) || (rc = sino_slot(e, dst, &d))) return rc;
    if ((rc = ensure_stage(e, (size_t)e->np * 6 * sizeof(double)))) return rc;
    HIPCHK(hipMemcpyAsync(e->stage, m_host, (size_t)e->np * 6 * sizeof(double), hipMemcpyHostToDevice, e->stream));
    const int blocks = (int)std::min<int64_t>(((int64_t)e->n * e->sx + 255) / 256, 1024);
    hipLaunchKernelGGL(k_sino_affine, dim3(blocks, e->np), dim3(256), 0, e->stream, (const float *)s, d, (const double *)e->stage, e->n, e->nx, e->sx);
    LAUNCHCHK();
    HIPCHK(hipStreamSynchronize(e->stream));        // the table is read from the caller's host memory
    return TOMO_OK;
}

// The Gauss-Newton normal equations of every projection (kernels_align_normal.hip.h).  Everything that can be refused is refused before
// anything is enqueued.  Both slots are read-only views: no claim is dropped, no version moves, and they may be one slot.  The
// workgroups' partial sums go to al_part, the result to al_out with the matrices behind it ([np][21] then [np][6] doubles): every
// entry that is read was written by the same call.  The call waits for its 21 * np numbers.
int tomo_sino_affine_normal(tomo_engine *e, int fixed_sino, int moving_sino, const double *m_host, int margin, double *out_host)
{
    NEED_ALIGN(e);
    if (!m_host) return fail(TOMO_ERR_ARG, "null matrices");
    if (!out_host) return fail(TOMO_ERR_ARG, "null output");
    if (fixed_sino < 0 || fixed_sino >= TOMO_SINO_SLOTS || moving_sino < 0 || moving_sino >= TOMO_SINO_SLOTS) return fail(TOMO_ERR_ARG, "bad sinogram id");
    for (int i = 0; i < 6 * e->np; ++i) if (!std::isfinite(m_host[i])) return fail(TOMO_ERR_ARG, "non-finite matrix entry");
    if (margin < 0) return fail(TOMO_ERR_ARG, "negative margin");
    if (2 * (int64_t)margin >= std::min(e->n, e->nx)) return fail(TOMO_ERR_ARG, "the margin leaves no sample of a projection (2 * margin >= a size)");
    if (!(e->is_first && e->is_last)) return fail(TOMO_ERR_STATE, "alignment runs on one whole-volume engine: this engine is a slab of a larger volume (tomo_set_slab_edges)");
    { int rc_ = order_after_async(e); if (rc_) return rc_; }
    float *f, *g; int rc;
    if ((rc = sino_slot_ro(e, fixed_sino, &f)) || (rc = sino_slot_ro(e, moving_sino, &g))) return rc;
    const int nblk = (e->n + SN_ROWS - 1) / SN_ROWS;
    if ((rc = al_ensure(e, (void **)&e->al_part, &e->al_part_bytes, (size_t)e->np * nblk * SN_SUMS * sizeof(double)))) return rc;
    if ((rc = al_ensure(e, (void **)&e->al_out, &e->al_out_bytes, (size_t)e->np * (SN_SUMS + 6) * sizeof(double)))) return rc;
    double *mat = e->al_out + (size_t)e->np * SN_SUMS;
    HIPCHK(hipMemcpyAsync(mat, m_host, (size_t)e->np * 6 * sizeof(double), hipMemcpyHostToDevice, e->stream));
    hipLaunchKernelGGL(k_sino_affine_normal, dim3(nblk, e->np), dim3(256), 0, e->stream, (const float *)f, (const float *)g, (const double *)mat,
                       e->n, e->nx, e->sx, margin, e->al_part);
    LAUNCHCHK();
    return reduce_tail([&] { hipLaunchKernelGGL(k_sum_rows_ascending, dim3((e->np * SN_SUMS + 255) / 256), dim3(256), 0, e->stream,
                                                (const double *)e->al_part, e->al_out, e->np, nblk, SN_SUMS, (float *)nullptr, 0.0); },
                       e, e->al_out, out_host, (size_t)e->np * SN_SUMS * sizeof(double));       // its wait also covers the matrices, read from the caller's host memory
}

int tomo_sino_axis_profile(tomo_engine *e, int sino, double *out_host)
{
    NEED_ALIGN(e);
    if (!out_host) return fail(TOMO_ERR_ARG, "null output");
    { int rc_ = order_after_async(e); if (rc_) return rc_; }
    float *g; int rc;
    if ((rc = sino_slot(e, sino, &g))) return rc;
    const int nblk = (e->n + AL_PROWS - 1) / AL_PROWS, nchunk = (e->nx + 63) / 64;
    if ((rc = al_ensure(e, (void **)&e->al_part, &e->al_part_bytes, (size_t)e->np * nblk * e->nx * sizeof(double)))) return rc;
    if ((rc = al_ensure(e, (void **)&e->al_out, &e->al_out_bytes, (size_t)e->np * e->nx * sizeof(double)))) return rc;
    hipLaunchKernelGGL(k_sino_axis_profile, dim3(nchunk, nblk, e->np), dim3(256), 0, e->stream, (const float *)g, e->al_part, e->n, e->nx, e->sx);
    LAUNCHCHK();
    return reduce_tail([&] { hipLaunchKernelGGL(k_sum_rows_ascending, dim3((e->np * e->nx + 255) / 256), dim3(256), 0, e->stream,
                                                (const double *)e->al_part, e->al_out, e->np, nblk, e->nx, (float *)nullptr, 0.0); },
                       e, e->al_out, out_host, (size_t)e->np * e->nx * sizeof(double));
}
