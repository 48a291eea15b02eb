// engine_pdhg.inc -- part of tomo_engine.hip (ONE translation unit; see engine_tv.inc).  This part: C ABI of the Chambolle-Pock
// iteration for min_{x >= 0} 1/2 |Ax - b|^2 + lambda |grad x|_{2,1} (kernels_pdhg.hip.h): the two step forms over caller-named slots
// and the whole-call form of one whole-volume engine; then the same for a slab of a sharded volume (tomo_pdhg_slab_*).

// a slab of a sharded volume has entry points of its own (tomo_pdhg_slab_*, below; tomo_comm_pdhg*, engine_comm.inc), which read the
// neighbours' p and xbar from the planes of tomo_bind_pdhg_halo
static int pdhg_whole_volume(const tomo_engine *e)
{
    if (e->comm) return fail(TOMO_ERR_STATE, "pdhg_tv runs on one whole-volume engine: this engine has a communicator");
    if (!(e->is_first && e->is_last)) return fail(TOMO_ERR_STATE, "pdhg_tv runs on one whole-volume engine: this slab is not both the first and the last (tomo_set_slab_edges)");
    return TOMO_OK;
}

// step sizes of the scalar mode: tau sigma (L_A + 12) = 1, ratio moves weight from sigma to tau (evaluated in double, rounded once)
static void pdhg_scalar_steps(const tomo_engine *e, float ratio, float *sigma, float *tau)
{
    const double s = std::sqrt((double)e->lipschitz + 12.0), r = (double)ratio;
    *tau = (float)(r / s);
    *sigma = (float)(1.0 / (r * s));
}

static int pdhg_sino_launch(tomo_engine *e, float *q, const float *g, const float *b, float sigma, int precond)
{
    const int64_t n4 = (int64_t)e->sino_elems() / 4;
    with_flag(precond != 0, [&](auto PRE) {
        hipLaunchKernelGGL(k_pdhg_sino<PRE()>, dim3(grid_1d(n4)), dim3(256), 0, e->stream, (f4 *)q, (const f4 *)g, (const f4 *)b, e->d_rowsum, sigma, n4, e->sx / 4);
    });
    LAUNCHCHK();
    return TOMO_OK;
}

static int pdhg_sino_dual_slots(tomo_engine *e, int q_sino, int g_sino, int b_sino, float sigma, int precond)
{
    int rc;
    if (q_sino == g_sino || q_sino == b_sino || g_sino == b_sino) return fail(TOMO_ERR_ARG, "tomo_pdhg_sino_dual: the three sinogram slots must differ");
    if (!precond && !(sigma > 0.f)) return fail(TOMO_ERR_ARG, "tomo_pdhg_sino_dual: sigma must be positive in scalar mode");
    float *q, *g, *b;
    if ((rc = sino_slot(e, q_sino, &q)) || (rc = sino_slot(e, g_sino, &g)) || (rc = sino_slot(e, b_sino, &b))) return rc;
    return pdhg_sino_launch(e, q, g, b, sigma, precond);
}

int tomo_pdhg_sino_dual(tomo_engine *e, int q_sino, int g_sino, int b_sino, float sigma, int precond)
{
    NEED(e);
    int rc;
    if ((rc = pdhg_whole_volume(e))) return rc;
    return pdhg_sino_dual_slots(e, q_sino, g_sino, b_sino, sigma, precond);
}

// The fused pass on buffers: x in place; xbar and p0..p2 land in the engine's second buffers, which then change places with the
// buffers behind the handles (fgp_p / fgp_q do the same), so the handles name the new fields afterwards.
// A slab with a face inside the volume (the callers have made sure that its planes exist) runs the SLAB form.
static bool pdhg_sharded(const tomo_engine *e) { return !(e->is_first && e->is_last); }

static int pdhg_tv_launch(tomo_engine *e, float *x, float **xbar, const float *u, float **p[3], float sigma, float tau, float lambda, float theta,
                          int precond, int slot)
{
    int rc;
    float *alt[4];
    for (int k = 0; k < 4; ++k) if ((rc = get_scratch(e, &e->pdhg_alt[k], &alt[k]))) return rc;
    if (slot >= 0 && (rc = reduce_begin(e))) return rc;
    PdhgArgs A{x, *xbar, u, *p[0], *p[1], *p[2], alt[0], alt[1], alt[2], alt[3], e->d_colsum_all, precond ? 0.5f : sigma, tau, lambda, theta};
    const int yseg = tv_rows_per_wave(e->tv, tv_shape(e), PD_TZ);
    dim3 grid(tv_march_grid(e->n, PD_TZ, e->sxc / 64, (e->n + yseg - 1) / yseg));
    {
        ProfScope ps(e, TOMO_K_PDHG_TV);
        const bool slab = pdhg_sharded(e);
        const PdhgSlab E = slab ? PdhgSlab{e->pdhg_lo, e->pdhg_hi, e->pdhg_send_first, e->pdhg_send_last, e->is_first, e->is_last} : PdhgSlab{};
        with_flag(precond != 0, [&](auto PRE) { with_flag(slot >= 0, [&](auto SUM) { with_flag(slab, [&](auto SLAB) {
            hipLaunchKernelGGL((k_pdhg_tv<PRE(), SUM(), SLAB()>), grid, dim3(256), 0, e->stream, A, e->d_part, e->n, e->nx, e->sx, yseg, E);
        }); }); });
    }
    LAUNCHCHK();
    std::swap(*xbar, e->pdhg_alt[0]);
    for (int k = 0; k < 3; ++k) std::swap(*p[k], e->pdhg_alt[1 + k]);
    return slot >= 0 ? reduce_end(e, slot) : TOMO_OK;
}

static int pdhg_check_steps(float sigma, float tau, float lambda, int precond, int slot)
{
    if (!(lambda > 0.f)) return fail(TOMO_ERR_ARG, "pdhg: lambda must be positive");
    if (!precond && (!(sigma > 0.f) || !(tau > 0.f))) return fail(TOMO_ERR_ARG, "pdhg: sigma and tau must be positive in scalar mode");
    if (slot < -1 || slot >= TOMO_S_COUNT) return fail(TOMO_ERR_ARG, "pdhg: bad scalar slot (-1 = none)");
    return TOMO_OK;
}

static int pdhg_tv_step_slots(tomo_engine *e, int x_vol, int xbar_vol, int u_vol, int p_vol0, float sigma, float tau, float lambda, float theta,
                              int precond, int slot)
{
    int rc;
    const int ids[6] = {x_vol, xbar_vol, u_vol, p_vol0, p_vol0 + 1, p_vol0 + 2};
    for (int i = 0; i < 6; ++i) {
        if (ids[i] < 0 || ids[i] >= TOMO_VOL_SLOTS) return fail(TOMO_ERR_ARG, "tomo_pdhg_tv_step: volume slot out of range");
        for (int j = 0; j < i; ++j) if (ids[i] == ids[j]) return fail(TOMO_ERR_ARG, "tomo_pdhg_tv_step: the volume slots overlap");
    }
    if ((rc = pdhg_check_steps(sigma, tau, lambda, precond, slot))) return rc;
    if ((rc = order_after_async(e))) return rc;
    float *x, *u, *t;
    if ((rc = get_vol(e, x_vol, &x)) || (rc = get_vol_ro(e, u_vol, &u))) return rc;
    for (int i = 1; i < 6; ++i) if (i != 2 && (rc = get_vol(e, ids[i], &t))) return rc;     // written: allocated, versions bumped
    float **p[3] = {&e->vol[ids[3]], &e->vol[ids[4]], &e->vol[ids[5]]};
    return pdhg_tv_launch(e, x, &e->vol[xbar_vol], u, p, sigma, tau, lambda, theta, precond, slot);
}

int tomo_pdhg_tv_step(tomo_engine *e, int x_vol, int xbar_vol, int u_vol, int p_vol0, float sigma, float tau, float lambda, float theta,
                      int precond, int slot)
{
    NEED(e);
    int rc;
    if ((rc = pdhg_whole_volume(e))) return rc;
    return pdhg_tv_step_slots(e, x_vol, xbar_vol, u_vol, p_vol0, sigma, tau, lambda, theta, precond, slot);
}

// p = 0, q = 0, xbar = x: the state tomo_pdhg iterates on, kept across calls until the next begin
static int pdhg_begin_state(tomo_engine *e)
{
    int rc;
    float *t;
    for (int k = 0; k < 3; ++k) {
        if ((rc = get_scratch(e, &e->pdhg_p[k], &t))) return rc;
        HIPCHK(hipMemsetAsync(t, 0, e->vol_elems() * sizeof(float), e->stream));
    }
    if ((rc = get_sino(e, &e->pdhg_q, &t))) return rc;
    HIPCHK(hipMemsetAsync(t, 0, e->sino_elems() * sizeof(float), e->stream));
    if ((rc = tomo_copy_volume(e, TOMO_VOL_YK, TOMO_VOL_RECON))) return rc;
    e->pdhg_begun = true;
    return TOMO_OK;
}

int tomo_pdhg_begin(tomo_engine *e)
{
    NEED(e);
    int rc;
    if ((rc = pdhg_whole_volume(e))) return rc;
    return pdhg_begin_state(e);
}

// niter iterations; `between` (may be empty) runs before each of them: the plane exchange of a slab
static int pdhg_loop(tomo_engine *e, int niter, float lambda, float theta, int precond, float ratio, int slot, const std::function<int()> &between)
{
    int rc;
    if (!e->pdhg_begun || !e->pdhg_q || !e->pdhg_p[2]) return fail(TOMO_ERR_STATE, "tomo_pdhg_begin has not been called");
    if (niter < 0) return fail(TOMO_ERR_ARG, "tomo_pdhg: negative iteration count");
    if (!precond && !(ratio > 0.f)) return fail(TOMO_ERR_ARG, "tomo_pdhg: ratio must be positive");
    float sigma = 0.5f, tau = 1.f;
    if (!precond) pdhg_scalar_steps(e, ratio, &sigma, &tau);
    if ((rc = pdhg_check_steps(sigma, tau, lambda, precond, slot))) return rc;
    if (!e->sino[TOMO_SINO_B]) return fail(TOMO_ERR_STATE, "tomo_pdhg: no tilt series");
    for (int it = 0; it < niter; ++it) {
        if (between && (rc = between())) return rc;
        // 1. g = A xbar (into the residual scratch: the model sinogram G and its claim stay as they are), q <- (q + S (g - b)) / (1 + S)
        if ((rc = tomo_forward_projection(e, TOMO_VOL_YK, TOMO_SINO_R))) return rc;
        if ((rc = pdhg_sino_launch(e, e->pdhg_q, e->sino[TOMO_SINO_R], e->sino[TOMO_SINO_B], sigma, precond))) return rc;
        // 2. u = A^T q
        float *x, *u, *t;
        if ((rc = get_vol(e, TOMO_VOL_TEMP, &u))) return rc;
        if ((rc = launch_bp_all(e, u, e->pdhg_q, nullptr, 0.f, 1.f, 0))) return rc;
        // 3. the fused pass
        if ((rc = get_vol(e, TOMO_VOL_RECON, &x)) || (rc = get_vol(e, TOMO_VOL_YK, &t))) return rc;
        float **p[3] = {&e->pdhg_p[0], &e->pdhg_p[1], &e->pdhg_p[2]};
        if ((rc = pdhg_tv_launch(e, x, &e->vol[TOMO_VOL_YK], u, p, sigma, tau, lambda, theta, precond, it == niter - 1 ? slot : -1))) return rc;
    }
    return TOMO_OK;
}

int tomo_pdhg(tomo_engine *e, int niter, float lambda, float theta, int precond, float ratio, int slot)
{
    NEED(e);
    int rc;
    if ((rc = pdhg_whole_volume(e))) return rc;
    return pdhg_loop(e, niter, lambda, theta, precond, ratio, slot, nullptr);
}

// ---- a slab of a sharded volume ------------------------------------------------------------------------------------------
// The forward projection, the dual sinogram and the back projection are slice-local; the fused pass reads the neighbours' slices from
// the lo / hi planes and leaves this slab's boundary fields in the send planes (k_pdhg_tv<.., SLAB>).  A slab that is both first and
// last runs the whole-volume kernel and needs no planes.
int tomo_bind_pdhg_halo(tomo_engine *e, void *lo, void *hi, void *send_first, void *send_last)
{
    NEED(e);
    if (!lo || !hi || !send_first || !send_last) return fail(TOMO_ERR_ARG, "null plane buffer");
    HIPCHK(hipStreamSynchronize(e->stream));
    e->pdhg_lo = (float *)lo; e->pdhg_hi = (float *)hi; e->pdhg_send_first = (float *)send_first; e->pdhg_send_last = (float *)send_last;
    return TOMO_OK;
}

static int comm_buffers(tomo_engine *e);        // engine_comm.inc: an engine with a communicator that has bound nothing gets planes of its own
static int pdhg_planes(tomo_engine *e)
{
    if (!e->pdhg_lo && e->comm) { int rc = comm_buffers(e); if (rc) return rc; }
    if (!e->pdhg_lo && pdhg_sharded(e)) return fail(TOMO_ERR_STATE, "a slab of a sharded volume needs its planes (tomo_bind_pdhg_halo)");
    return TOMO_OK;
}

static int pdhg_pack(tomo_engine *e, const float *xbar, float *const p[3])
{
    if (!e->pdhg_lo) return TOMO_OK;            // a whole-volume slab without planes: nobody to send to
    const dim3 grid((unsigned)((e->npix + 255) / 256));
    hipLaunchKernelGGL(k_halo_pack, grid, dim3(256), 0, e->stream, xbar, e->pdhg_send_first, (int)e->npix, e->sx, 0);
    hipLaunchKernelGGL(k_halo_pack, grid, dim3(256), 0, e->stream, xbar, e->pdhg_send_last, (int)e->npix, e->sx, e->nx - 1);
    for (int k = 0; k < 3; ++k)
        hipLaunchKernelGGL(k_halo_pack, grid, dim3(256), 0, e->stream, (const float *)p[k], e->pdhg_send_last + (size_t)(1 + k) * e->npix, (int)e->npix, e->sx, e->nx - 1);
    LAUNCHCHK();
    return TOMO_OK;
}

int tomo_pdhg_slab_pack(tomo_engine *e, int xbar_vol, int p_vol0)
{
    NEED(e);
    int rc;
    if ((rc = pdhg_planes(e))) return rc;
    float *xbar, *p[3];
    if ((rc = get_vol_ro(e, xbar_vol, &xbar))) return rc;
    for (int k = 0; k < 3; ++k) if ((rc = get_vol_ro(e, p_vol0 + k, &p[k]))) return rc;
    return pdhg_pack(e, xbar, p);
}

int tomo_pdhg_slab_tv_step(tomo_engine *e, int x_vol, int xbar_vol, int u_vol, int p_vol0, float sigma, float tau, float lambda, float theta,
                           int precond, int slot)
{
    NEED(e);
    int rc;
    if ((rc = pdhg_planes(e))) return rc;
    return pdhg_tv_step_slots(e, x_vol, xbar_vol, u_vol, p_vol0, sigma, tau, lambda, theta, precond, slot);
}

int tomo_pdhg_slab_sino_dual(tomo_engine *e, int q_sino, int g_sino, int b_sino, float sigma, int precond)
{
    NEED(e);
    return pdhg_sino_dual_slots(e, q_sino, g_sino, b_sino, sigma, precond);
}

int tomo_pdhg_slab_begin(tomo_engine *e)
{
    NEED(e);
    int rc;
    if ((rc = pdhg_planes(e)) || (rc = pdhg_begin_state(e))) return rc;
    return pdhg_pack(e, e->vol[TOMO_VOL_YK], e->pdhg_p);
}

int tomo_pdhg_slab_iter(tomo_engine *e, float lambda, float theta, int precond, float ratio, int slot)
{
    NEED(e);
    int rc;
    if ((rc = pdhg_planes(e))) return rc;
    return pdhg_loop(e, 1, lambda, theta, precond, ratio, slot, nullptr);
}
