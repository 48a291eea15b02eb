// engine_sart.inc -- part of tomo_engine.hip (ONE translation unit: the kernels are templates and asm blocks in headers; the host side is
// split by topic into files that tomo_engine.hip includes in order).  This part: the SART and ART sweeps: the launch chains of a sweep
// (run_chains), the launchers of their steps, the four forms of a SART sweep (select_sart names the one that runs) and their C ABI.
// (It holds templates, so it stands before the extern "C" block: its entry points take C linkage from their declarations in tomo_hip.h.)

// A sweep over a slab as one chain of launches on the engine's stream (tile step -> residual finish -> tile step ...: ~5.7 us of idle
// chip after each and a tail of partly filled CUs at the end of each), or as two chains over two sub-slabs (64-slice chunks, equal
// halves) on two streams: slices are independent, and each stream's short kernels and launch boundaries disappear under the other
// stream's tile step (round 2, 512 slices: 23.4 -> 22.1 ms per ASD-POCS step).  The sub-slabs run their per-row kernels at the widest
// vector that fits (k_bp_angle writes its roundings out, so every width gives the same bits).  A sweep is then 2 x ~180 launches of ~100 us kernels: one host thread cannot enqueue both chains
// fast enough to keep both streams fed (measured: 19.4 ms per sweep against 19.9 on one stream), so the second chain is enqueued
// by a second host thread (18.0 ms: what two independent engines on two Python threads reach).
// "sart_streams": 2 = always (when the slab has two chunks), 1 = never, 0 = auto: equal halves, and not when a pixel's row of
// slices is a multiple of 4 KB -- the two halves of such rows land on the same memory channels (1024 slices: 48.5 against 42.9 ms
// per ASD-POCS step; 128 / 256 / 512 / 768 slices: -2.6 / -3.3 / -5.5 / -5.3 %).
// chains a sweep of this engine's slab runs as, under the current "sart_streams" (also what tomo_sart_chain_count reports)
static int chain_count(const tomo_engine *e)
{
    const int units = e->sxc / 64;
    const bool two = e->sart_streams >= 2 || (e->sart_streams == 0 && units % 2 == 0 && (e->sx * sizeof(float)) % 4096 != 0);
    if (!(two && units >= 2)) return 1;
    if (e->sart_streams > 2) return std::min(std::min(e->sart_streams, (int)tomo_engine::MAX_CHAINS), units);
    return 2;   // "sart_streams" = 3 / 4: that many chains (measured at 512 slices: 2 chains 22.4 ms per step, 3: 24.1, 4: 22.7)
}

// the widest vector of the per-row kernels that fits the 64-slice chunks [c0, c0 + nc)
static int chunk_vec(int c0, int nc) { return (c0 % 4 == 0 && nc % 4 == 0) ? 4 : (c0 % 2 == 0 && nc % 2 == 0) ? 2 : 1; }

template <class Chain>
static int run_chains(tomo_engine *e, const Chain &chain)
{
    const int units = e->sxc / 64;                       // 64-slice chunks; a sub-slab's per-row kernels use the widest vector that fits
    const int nch = chain_count(e);
    if (nch < 2) return chain(whole(e));
    if (!e->ev_sfork) HIPCHK(hipEventCreateWithFlags(&e->ev_sfork, hipEventDisableTiming));
    for (int u = 0; u < nch; ++u)
        if (!e->sub_stream[u]) {
            HIPCHK(hipStreamCreateWithFlags(&e->sub_stream[u], hipStreamNonBlocking));
            HIPCHK(hipEventCreateWithFlags(&e->ev_sjoin[u], hipEventDisableTiming));
        }
    HIPCHK(hipEventRecord(e->ev_sfork, e->stream));
    Sub sbs[tomo_engine::MAX_CHAINS];
    for (int u = 0, c0 = 0; u < nch; ++u) {
        const int nc = units / nch + (u < units % nch ? 1 : 0);
        sbs[u] = Sub{e->sub_stream[u], c0, nc, chunk_vec(c0, nc)};
        c0 += nc;
    }
    for (int u = 0; u < nch; ++u) HIPCHK(hipStreamWaitEvent(e->sub_stream[u], e->ev_sfork, 0));
    int rcs[tomo_engine::MAX_CHAINS] = {TOMO_OK, TOMO_OK, TOMO_OK, TOMO_OK};
    std::string errs[tomo_engine::MAX_CHAINS];
    for (int u = 1; u < nch; ++u) {                        // chains 1.. are enqueued by the engine's persistent helper threads
        if (!e->chain_helper[u]) {
            e->chain_helper[u].reset(new ChainHelper());
            e->chain_helper[u]->start(e->device);
        }
        e->chain_helper[u]->submit([&, u]() {
            rcs[u] = chain(sbs[u]);
            if (rcs[u]) errs[u] = g_err;                  // the error text is thread-local
        });
    }
    rcs[0] = chain(sbs[0]);
    for (int u = 1; u < nch; ++u) e->chain_helper[u]->wait();
    for (int u = 1; u < nch; ++u) if (rcs[u] && !rcs[0]) { rcs[0] = rcs[u]; g_err = errs[u]; }
    for (int u = 0; u < nch; ++u)
        if (hipEventRecord(e->ev_sjoin[u], e->sub_stream[u]) != hipSuccess && !rcs[0]) rcs[0] = fail(TOMO_ERR_HIP, "hipEventRecord(sub-slab join)");
    for (int u = 0; u < nch; ++u) HIPCHK(hipStreamWaitEvent(e->stream, e->ev_sjoin[u], 0));
    return rcs[0];
}

int tomo_sart_chain_count(tomo_engine *e, int *count) { if (!e || !count) return fail(TOMO_ERR_ARG, "null"); *count = chain_count(e); return TOMO_OK; }

// ---- the launchers of a sweep's steps (b = the data sinogram the residual rows are formed against) ---------------------------------
// the chained ART's back projection of angle `angle` (k_bp_art); a = the rows k_art_chain left, all angles
static int launch_bp_art(tomo_engine *e, const Sub &sb, float *x, int angle, const float *a, float beta)
{
    const int vec = sub_vec(e, sb);
    const Chunks ch = chunks64(e, sb);
    const int nchunk = ch.n / vec, ngroups = (int)((e->npix + BP_PPW - 1) / BP_PPW);
    dim3 grid((unsigned)(((int64_t)ngroups * nchunk + 3) / 4));
    with_vec(vec, [&](auto V) {
        hipLaunchKernelGGL((k_bp_art<V(), BP_PPW>), grid, dim3(256), 0, sb.stream, x, e->d_cell + (size_t)angle * e->npix, a + (size_t)angle * e->n * e->sx, beta,
                           (int)e->npix, e->sx, ngroups, nchunk, slab_streams(e) ? 1 : 0, ch.c0 / vec);
    });
    LAUNCHCHK();
    return TOMO_OK;
}

// residual rows of angle `next` from the partial sums in `partial` and their row lists (k_resid_finish); sum: plain row sums instead
// (chained ART: k_art_chain forms the residuals)
static int launch_resid_finish(tomo_engine *e, const Sub &sb, const float *partial, const uint32_t *row_first, const uint32_t *row_nseg, int next, const float *b, float *r, bool sum = false)
{
    const Chunks ch = chunks64(e, sb);
    const int vec = sub_vec(e, sb), nchunk = ch.n / vec;
    dim3 grid((unsigned)((int64_t)e->n * nchunk)), block(256);
    with_vec(vec, [&](auto V) { with_flag(sum, [&](auto S) {
        hipLaunchKernelGGL((k_resid_finish<V(), S()>), grid, block, 0, sb.stream, partial, row_first, row_nseg, b, e->d_rowsum, r, next * e->n, e->n, nchunk, e->sx, ch.c0 / vec);
    }); });
    LAUNCHCHK();
    return TOMO_OK;
}

// segmented per-angle step: FUSED -> BP(prev) + FP(next); else plain FP(next).  Leaves the residual rows of `next` in r.
template <bool FUSED>
static int launch_sart_seg(tomo_engine *e, const float *x_old, float *x_new, int prev, int next, const float *b, float *r, float beta)
{
    if (!e->seg_partial)
        if (int rc = dev_alloc(e, GEOMETRY, (void **)&e->seg_partial, (size_t)std::max<uint32_t>(1, e->max_items) * e->sx * sizeof(float), true)) return rc;
    const int nchunk = e->sxc / (64 * e->vec);
    uint32_t b0 = e->h_seg_exec_ptr[next], b1 = e->h_seg_exec_ptr[next + 1];
    int L = (int)((b1 - b0) / 8);
    const SegItemD *exec = e->d_seg_exec + b0;
    const CellD *cell = FUSED ? e->d_cell + (size_t)prev * e->npix : nullptr;
    const float *rp = FUSED ? r + (size_t)prev * e->n * e->sx : nullptr;
    if (L > 0) {
        ProfScope ps(e, FUSED ? TOMO_K_SART_FUSED : TOMO_K_FP_ANGLE);
        dim3 grid((unsigned)(8 * (int64_t)L * nchunk)), block(64);
        with_vec(e->vec, [&](auto V) {
            hipLaunchKernelGGL((k_sart_seg<V(), 8, FUSED>), grid, block, 0, e->stream, x_old, x_new, exec, L, e->d_went, cell, rp, beta, e->seg_partial, e->sx);
        });
        LAUNCHCHK();
    }
    return launch_resid_finish(e, whole(e), e->seg_partial, e->d_row_first, e->d_row_nseg, next, b, r);
}

// function attributes and the partial-sum buffers of the tile form (k_sart_tile), set up on the caller's thread and stream
static int sart_tile_prepare(tomo_engine *e, bool coop)
{
    if (!e->attr_st) {
        const void *forms[] = {(const void *)k_sart_tile<true, false, true>, (const void *)k_sart_tile<true, false, false>,
                               (const void *)k_sart_tile<false, false, true>, (const void *)k_sart_tile<false, false, false>,
                               (const void *)k_sart_tile<true, true, true>, (const void *)k_sart_tile<true, true, false>,
                               (const void *)k_sart_tile<true, false, true, true>, (const void *)k_sart_tile<true, false, false, true>};
        for (const void *f : forms) HIPCHK(hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, ST_LDS_V * 16));
        e->attr_st = true;
    }
    const size_t pbytes = (size_t)std::max<uint32_t>(1, e->st_max_ids) * e->sx * sizeof(float);
    if (!e->st_partial)
        if (int rc = dev_alloc(e, GEOMETRY, (void **)&e->st_partial, pbytes, true)) return rc;
    if (coop && !e->st_partial2) {
        int rc;
        if ((rc = dev_alloc(e, GEOMETRY, (void **)&e->st_partial2, pbytes, true))) return rc;
        if ((rc = dev_alloc(e, GEOMETRY, (void **)&e->st_flags, (size_t)e->n * (e->sxc / 64) * sizeof(uint32_t), true))) return rc;
        // workgroups that start together: the reducer duty is dealt to that many (2 per CU by LDS; any value is correct)
        int per_cu = 0; hipDeviceProp_t prop;
        HIPCHK(hipGetDeviceProperties(&prop, e->device));
        HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void *)k_sart_tile<true, true, true>, ST_THREADS, ST_LDS_V * 16));
        e->st_resident = std::max(1, per_cu) * std::max(1, prop.multiProcessorCount);
    }
    return TOMO_OK;
}

// tile form of the per-angle step (k_sart_tile; sart_tile_prepare has run): FUSED -> BP(prev) + FP(next), in place; else plain
// FP(next).  Leaves the residual rows of `next` in r; finish = false leaves the partial sums of `next` in `partial` for the next link's reducer duty (cooperative chain)
// ART: the fused step of the chained ART sweep (r = the rows k_art_chain left for `prev`; the finish stores plain row sums into
// fp_out, from which k_art_chain forms the rows of `next`)
template <bool FUSED, bool ART = false>
static int launch_sart_tile(tomo_engine *e, const Sub &sb, float *x, int prev, int next, const float *b, float *r, float beta,
                            float *partial = nullptr, bool finish = true, int64_t key = -1, float *fp_out = nullptr)
{
    const Chunks ch = chunks64(e, sb);
    const size_t nt = (size_t)e->st_ntiles;
    if (!partial) partial = e->st_partial;
    {
        ProfScope ps(e, FUSED ? TOMO_K_SART_FUSED : TOMO_K_FP_ANGLE, sb.stream, key);
        dim3 grid((unsigned)(8 * ((e->st_ntiles + 7) / 8) * ch.n)), block(ST_THREADS);
        with_flag(slab_streams(e), [&](auto NT) {
            hipLaunchKernelGGL((k_sart_tile<FUSED, false, NT(), ART && FUSED>), grid, block, ST_LDS_V * 16, sb.stream, x, x,
                               FUSED ? e->d_st_cell + (size_t)prev * nt * ST_PIX : nullptr, FUSED ? e->d_st_win + (size_t)prev * nt : nullptr,
                               FUSED ? r + (size_t)prev * e->n * e->sx : nullptr, beta,
                               e->d_st_seg + (size_t)next * nt * ST_MAXSEG, e->d_st_segid + (size_t)next * nt * ST_MAXSEG, e->d_st_ent, partial,
                               e->n, e->sx, e->st_tiles_z, e->st_ntiles, ch.n, ch.c0, e->sart_skip_same, StCoop{});
        });
        LAUNCHCHK();
    }
    if (ART) return launch_resid_finish(e, sb, partial, e->d_st_row_first, e->d_st_row_nseg, next, b, fp_out, true);
    return finish ? launch_resid_finish(e, sb, partial, e->d_st_row_first, e->d_st_row_nseg, next, b, r) : TOMO_OK;
}

// cooperative link: residual rows of `prev` from p_read (reducer duty of the first workgroups), BP(prev) + FP(next) -> p_write
static int launch_sart_coop(tomo_engine *e, const Sub &sb, float *x, int prev, int next, const float *b, float *r, float beta,
                            const float *p_read, float *p_write, uint32_t epoch, int64_t key = -1)
{
    const Chunks ch = chunks64(e, sb);
    const size_t nt = (size_t)e->st_ntiles;
    ProfScope ps(e, TOMO_K_SART_FUSED, sb.stream, key);
    const unsigned nblocks = (unsigned)(8 * ((e->st_ntiles + 7) / 8) * ch.n);
    StCoop co;
    co.p_read = p_read; co.row_first = e->d_st_row_first + (size_t)prev * e->n; co.row_nseg = e->d_st_row_nseg + (size_t)prev * e->n;
    co.b = b + (size_t)prev * e->n * e->sx; co.rowsum = e->d_rowsum + (size_t)prev * e->n; co.r_out = r + (size_t)prev * e->n * e->sx;
    co.flags = e->st_flags; co.epoch = epoch; co.nitems = e->n * ch.n; co.nchunk_all = e->sxc / 64; co.spin = e->sart_coop_spin;
    co.nred = (int)std::min<unsigned>(nblocks, (unsigned)std::max(1, e->st_resident));
    with_flag(slab_streams(e), [&](auto NT) {
        hipLaunchKernelGGL((k_sart_tile<true, true, NT()>), dim3(nblocks), dim3(ST_THREADS), ST_LDS_V * 16, sb.stream, x, x,
                           e->d_st_cell + (size_t)prev * nt * ST_PIX, e->d_st_win + (size_t)prev * nt, r + (size_t)prev * e->n * e->sx, beta,
                           e->d_st_seg + (size_t)next * nt * ST_MAXSEG, e->d_st_segid + (size_t)next * nt * ST_MAXSEG, e->d_st_ent, p_write,
                           e->n, e->sx, e->st_tiles_z, e->st_ntiles, ch.n, ch.c0, e->sart_skip_same, co);
    });
    LAUNCHCHK();
    return TOMO_OK;
}

// ---- a SART sweep --------------------------------------------------------------------------------------------------------------
// What a sweep works on, whatever its form.  Read-only once built: the helper threads of run_chains share it.
struct AngleSeq {   // at(k): the angle of step k, under the caller's permutation of the np angles (null: natural order)
    const int32_t *order; int np;
    int at(int64_t k) const { const int q = (int)(k % np); return order ? order[q] : q; }
};
struct Sweep {
    float *x, *r;            // the swept volume (in place), the residual sinogram
    const float *b;          // the data sinogram
    float *track;            // null, or the tracked volume: the last back projection sums ||x_new - track||^2 and copies x_new into it
    float beta; int64_t steps; AngleSeq seq;     // steps > 0
};

// ANGLE, the reference structure: one forward projection + one back-projection update per angle
static int sweep_angles(tomo_engine *e, const Sweep &s)
{
    for (int64_t k = 0; k < s.steps; ++k) {
        const int i = s.seq.at(k);
        {
            ProfScope ps(e, TOMO_K_FP_ANGLE);
            if (int rc = launch_fp<FP_RESID_NORM>(e, s.x, i * e->n, e->n, s.b, s.r)) return rc;
        }
        if (int rc = launch_bp_angle(e, whole(e), s.x, i, s.r, s.beta, k == s.steps - 1 ? s.track : nullptr)) return rc;
    }
    return TOMO_OK;
}

// TILE, one chain over the sub-slab sb, in place: FP(a0) ; [BP(a_k-1) + FP(a_k)] for every consecutive pair ; BP(a_last).  coop: the
// cooperative chain (k_sart_tile COOP): the links alternate the two partial buffers, link k publishes with epoch0 + k
static int tile_chain(tomo_engine *e, const Sweep &s, const Sub &sb, bool coop, uint32_t epoch0)
{
    const int last = s.seq.at(s.steps - 1);
    int rc = launch_sart_tile<false>(e, sb, s.x, 0, s.seq.at(0), s.b, s.r, s.beta, nullptr, !coop);       // link 0 (coop: its sums stay in st_partial)
    for (int64_t k = 1; k < s.steps && !rc; ++k) {
        const int prev = s.seq.at(k - 1), next = s.seq.at(k);
        if (coop) {
            float *pk = (k & 1) ? e->st_partial2 : e->st_partial, *pk1 = (k & 1) ? e->st_partial : e->st_partial2;   // P[k&1], P[(k-1)&1]
            rc = launch_sart_coop(e, sb, s.x, prev, next, s.b, s.r, s.beta, pk1, pk, epoch0 + (uint32_t)k, k);
        } else if (prev == next) {      // single-angle geometry: the residual rows read and written would be the same
            if (!(rc = launch_bp_angle(e, sb, s.x, prev, s.r, s.beta))) rc = launch_sart_tile<false>(e, sb, s.x, 0, next, s.b, s.r, s.beta);
        } else rc = launch_sart_tile<true>(e, sb, s.x, prev, next, s.b, s.r, s.beta, nullptr, true, k);
    }
    if (!rc && coop) rc = launch_resid_finish(e, sb, ((s.steps - 1) & 1) ? e->st_partial2 : e->st_partial, e->d_st_row_first, e->d_st_row_nseg, last, s.b, s.r);
    return rc ? rc : launch_bp_angle(e, sb, s.x, last, s.r, s.beta, s.track);          // link `steps`
}

// TILE over the whole slab (as one chain or several), or over the chunk ranges {c0, nc} a resident launch left
static int sweep_tiles(tomo_engine *e, const Sweep &s, const std::vector<std::pair<int, int>> *ranges = nullptr)
{
    // the cooperative chain needs consecutive angles to differ (np >= 2) and whole 64-slice chunks
    const bool coop = e->sart_coop && e->np >= 2 && s.steps >= 2 && !ranges;
    if (int rc = sart_tile_prepare(e, coop)) return rc;
    const uint32_t epoch0 = e->st_epoch + 1;             // (both sub-slab chains alike)
    if (coop) e->st_epoch += (uint32_t)(s.steps + 1);
    if (!ranges) return run_chains(e, [&](const Sub &sb) { return tile_chain(e, s, sb, coop, epoch0); });
    for (const auto &rg : *ranges)       // one after the other on the engine's stream (they share the partial-sum buffer)
        if (int rc = tile_chain(e, s, Sub{e->stream, rg.first, rg.second, chunk_vec(rg.first, rg.second)}, false, epoch0)) return rc;
    return TOMO_OK;
}

// SEG, the ray-walk form (k_sart_seg): each fused step reads one buffer and writes the other, so the swept volume may end in the
// partner buffer: e->vol[vol] and e->sart_alt then change places
static int sweep_seg(tomo_engine *e, const Sweep &s, int vol)
{
    float *alt, *cur = s.x; int rc;
    // the ray-walk form's tables (built at creation only where it is the expected form), the partner buffer
    if ((rc = ensure_seg_tables(e)) || (rc = get_scratch(e, &e->sart_alt, &alt))) return rc;
    if ((rc = launch_sart_seg<false>(e, cur, nullptr, 0, s.seq.at(0), s.b, s.r, s.beta))) return rc;
    for (int64_t k = 1; k < s.steps; ++k) {
        const int prev = s.seq.at(k - 1), next = s.seq.at(k);
        if (prev == next) {   // single-angle geometry: the residual rows read and written would be the same
            if ((rc = launch_bp_angle(e, whole(e), cur, prev, s.r, s.beta)) || (rc = launch_fp<FP_RESID_NORM>(e, cur, next * e->n, e->n, s.b, s.r))) return rc;
            continue;
        }
        if ((rc = launch_sart_seg<true>(e, cur, alt, prev, next, s.b, s.r, s.beta))) return rc;
        std::swap(cur, alt);
    }
    const int last = s.seq.at(s.steps - 1);
    if ((rc = launch_bp_angle(e, whole(e), cur, last, s.r, s.beta, s.track))) return rc;
    if (cur != s.x) { e->vol[vol] = cur; e->sart_alt = s.x; }   // the swept volume now lives in the partner buffer
    return TOMO_OK;
}

// ---- RESIDENT: the sweep as one launch of the volume-resident kernel (sart_resident.hip.h) -----------------------------------------
// Every workgroup of the launch must be on the chip at once (they wait for one another's ray sums), and a workgroup fills a CU:
// two such launches side by side -- two engines on one device, on two streams -- could each get part of the chip and wait for the
// rest until their spins run out.  So the resident launches of one device form a chain: each waits for the event the one before
// it (any engine, any stream) recorded.  Other kernels may overlap freely: they finish by themselves.
static std::mutex g_rs_mu;
static hipEvent_t g_rs_last[64] = {};

// RESIDENT: one launch, the slab read and written once.  The call waits for the launch -- one host wait per sweep (~10 us against a
// sweep of milliseconds) is what knowing costs -- and the 64-slice chunks the launch did not store (the device was shared) go to the
// streamed chain.  The counters (tags, commit words, sequence number, sit-out) are the ledger's: e->rs, sart_host.h.
static int launch_sart_resident(tomo_engine *e, const Sweep &s)
{
    std::vector<std::pair<int, int>> failed;              // chunk ranges {c0, nc}
    if (s.steps > (int64_t)1 << 24) return fail(TOMO_ERR_ARG, "too many SART steps in one call");
    if (e->device < 0 || e->device >= 64) return fail(TOMO_ERR_ARG, "device index");
    const int nc = e->sxc / 64;                           // the whole slab: every launch adds to every chunk's commit word
    const int groups = std::max(1, std::min(e->rs_groups, nc)), rounds = (nc + groups - 1) / groups;
    std::vector<int> angs((size_t)s.steps);               // the angle of every step, on the device (an unchanged sequence stays where it is)
    for (int64_t k = 0; k < s.steps; ++k) angs[(size_t)k] = s.seq.at(k);
    if (angs != e->rs_angs_host) {
        HIPCHK(hipStreamSynchronize(e->stream));          // (a sweep in flight may still read the old sequence; rare: the first sweep, a new order)
        if ((size_t)s.steps > e->rs_angs_cap) {
            if (e->d_rs_angs) { e->pool.release(e->d_rs_angs); e->rs_angs_cap = 0; }
            if (int rc = dev_alloc(e, GEOMETRY, (void **)&e->d_rs_angs, (size_t)s.steps * sizeof(int), false)) return rc;
            e->rs_angs_cap = (size_t)s.steps;
        }
        HIPCHK(hipMemcpy(e->d_rs_angs, angs.data(), (size_t)s.steps * sizeof(int), hipMemcpyHostToDevice));
        e->rs_angs_host.swap(angs);
    }
    const RsLedger::Launch l = e->rs.begin(rounds, s.steps);
    if (l.clear_tags) {
        HIPCHK(hipMemsetAsync(e->rs_pb, 0, e->rs_pb_bytes, e->stream));
        HIPCHK(hipMemsetAsync(e->rs_rb, 0, e->rs_rb_bytes, e->stream));
    }
    if (l.clear_commit) HIPCHK(hipMemsetAsync(e->d_rs_commit, 0, (size_t)nc * sizeof(unsigned), e->stream));
    if (l.clear_done) std::memset(e->rs_done, 0, (size_t)nc * sizeof(int));
    RsArgs A{};
    A.x = s.x; A.b = s.b; A.rowsum = e->d_rowsum; A.hdr = e->d_rs_hdr; A.cell = e->d_rs_cell; A.ts = e->d_rs_ts; A.rl = e->d_rs_rl;
    A.pb = e->rs_pb; A.rb = e->rs_rb; A.angs = e->d_rs_angs; A.track = s.track; A.part = e->d_part; A.abort_word = e->d_rs_abort; A.abort_host = e->rs_abort;
    A.commit = e->d_rs_commit; A.done_host = e->rs_done; A.seq = l.seq; A.commit_base = l.commit_base; A.test_fail = e->rs_test_fail;
    A.n = e->n; A.sx = e->sx; A.np = e->np; A.ntiles = e->rs_ntiles; A.tiles = e->rs_tiles; A.rpt = e->rs_rpt; A.steps = (int)s.steps; A.chunk0 = 0; A.nchunk = nc;
    A.epoch0 = l.epoch0; A.spin_limit = e->rs_spin_limit; A.beta = s.beta; A.prof = nullptr;
    {
        std::lock_guard<std::mutex> lk(g_rs_mu);
        hipEvent_t &last = g_rs_last[e->device];
        if (!last) HIPCHK(hipEventCreateWithFlags(&last, hipEventDisableTiming));
        else HIPCHK(hipStreamWaitEvent(e->stream, last, 0));
        {
            ProfScope ps(e, TOMO_K_SART_RESIDENT);
            hipLaunchKernelGGL(k_sart_resident, dim3((unsigned)(e->rs_ntiles * groups)), dim3(RS_THREADS), 0, e->stream, A);
            LAUNCHCHK();
        }
        HIPCHK(hipEventRecord(last, e->stream));
    }
    // the verdict: which chunks carry this launch's sequence number
    HIPCHK(hipStreamSynchronize(e->stream));
    int nfailed = 0;
    for (int c = 0; c < nc; ++c) {
        if (e->rs_done[c] == (int)l.seq) continue;
        ++nfailed;
        if (!failed.empty() && failed.back().first + failed.back().second == c) ++failed.back().second;
        else failed.emplace_back(c, 1);
    }
    e->rs.finish(nfailed, e->rs_ntiles, nfailed ? *e->rs_abort : 0);
    if (nfailed) {
        *e->rs_abort = 0;
        HIPCHK(hipMemsetAsync(e->d_rs_abort, 0, sizeof(int), e->stream));
    }
    return failed.empty() ? TOMO_OK : sweep_tiles(e, s, &failed);
}

// track_vol >= 0: the last back-projection of the sweep also leaves ||x_new - track||^2 in scalar `slot` and copies x_new
// into track_vol (tomo_sart_tracked)
static int sart_impl(tomo_engine *e, int vol, int sino_b, float beta, int niter, const int32_t *order, int track_vol, int slot)
{
    NEED(e);
    Sweep s{};
    float *b; int rc;
    if ((rc = get_vol(e, vol, &s.x)) || (rc = get_sino(e, &e->sino[TOMO_SINO_R], &s.r)) || (rc = sino_slot(e, sino_b, &b))) return rc;
    s.b = b; s.beta = beta; s.steps = (int64_t)niter * e->np; s.seq = AngleSeq{order, e->np};
    if (track_vol >= 0) {
        if (track_vol == vol) return fail(TOMO_ERR_ARG, "the tracked volume must differ from the swept one");
        if (slot < 0 || slot >= TOMO_S_COUNT) return fail(TOMO_ERR_ARG, "bad scalar slot");
        if ((rc = get_vol(e, track_vol, &s.track))) return rc;
        if (s.steps <= 0) {   // nothing is swept: the plain pair of passes
            return (rc = tomo_diff_norm_sq(e, vol, track_vol, slot)) ? rc : tomo_copy_volume(e, track_vol, vol);
        }
        if ((rc = reduce_begin(e))) return rc;
    }
    if (order && !is_permutation(order, e->np)) return fail(TOMO_ERR_ARG, "SART order is not a permutation of the angles");
    if (s.steps <= 0) return TOMO_OK;
    const SartChoice ch = select_sart(e);
    if (ch.no_tables) return fail(TOMO_ERR_STATE, "\"sart_resident\" = 1, but this engine has no tables of the resident sweep (N not a multiple of 8, more 32 x 32 tiles than CUs, or a matrix whose ray windows do not fit)");
    if (ch.sits_out) --e->rs.skip;
    switch (ch.form) {
    case SART_ANGLE: rc = sweep_angles(e, s); break;
    case SART_SEG: rc = sweep_seg(e, s, vol); break;
    case SART_TILE: rc = sweep_tiles(e, s); break;
    case SART_RESIDENT: rc = launch_sart_resident(e, s); break;
    }
    if (rc) return rc;
    return s.track ? reduce_end(e, slot) : TOMO_OK;
}

int tomo_sart(tomo_engine *e, int vol, float beta, int niter, const int32_t *order) { return sart_impl(e, vol, TOMO_SINO_B, beta, niter, order, -1, 0); }
int tomo_sart_data(tomo_engine *e, int vol, int sino_b, float beta, int niter, const int32_t *order) { return sart_impl(e, vol, sino_b, beta, niter, order, -1, 0); }
int tomo_sart_tracked(tomo_engine *e, int vol, int sino_b, float beta, int niter, const int32_t *order, int track_vol, int slot) { return sart_impl(e, vol, sino_b, beta, niter, order, track_vol, slot); }

// ---- ART -----------------------------------------------------------------------------------------------------------------------
int tomo_art(tomo_engine *e, float beta) { return tomo_art_order(e, beta, nullptr); }

int tomo_art_order(tomo_engine *e, float beta, const int32_t *order_host)
{
    NEED(e);
    float *x;
    { int rc_ = get_vol(e, TOMO_VOL_RECON, &x); if (rc_) return rc_; }
    int32_t *d_order = nullptr;
    if (order_host) {
        if (!is_permutation(order_host, e->nrows)) return fail(TOMO_ERR_ARG, "row order is not a permutation");
        int rc = ensure_stage(e, e->nrows * sizeof(int32_t)); if (rc) return rc;
        HIPCHK(hipMemcpyAsync(e->stage, order_host, e->nrows * sizeof(int32_t), hipMemcpyHostToDevice, e->stream));
        d_order = (int32_t *)e->stage;
    }
    if (!order_host && e->art_chain && e->art_chain_ok) {
        // natural order: one angle = forward projection + recurrence along the rays + back-projection (k_art_chain)
        float *d, *a; int rc;
        if ((rc = get_sino(e, &e->sino[TOMO_SINO_G], &d)) || (rc = get_sino(e, &e->sino[TOMO_SINO_R], &a))) return rc;
        const float *b = e->sino[TOMO_SINO_B];
        if (e->art_tile && e->sart_tile && e->st_ok && e->np >= 1) {
            // the same fused steps as the SART sweep: FP(a0); [BP_art(a_k-1) + FP(a_k)] ...; BP_art(a_last), the residual rows of
            // each angle formed by k_art_chain from the tile step's row sums.  Per angle 228 instead of 323 us at 512^3.
            if ((rc = sart_tile_prepare(e, false))) return rc;
            auto chain = [&](const Sub &sb) -> int {        // one sub-slab's (or the whole slab's) chain of launches
                const Chunks ch = chunks64(e, sb);
                for (int i = 0; i < e->np; ++i) {
                    int rc2 = i == 0 ? launch_sart_tile<false, true>(e, sb, x, 0, 0, b, a, beta, nullptr, true, -1, d)
                                     : launch_sart_tile<true, true>(e, sb, x, i - 1, i, b, a, beta, nullptr, true, i, d);
                    if (rc2) return rc2;
                    hipLaunchKernelGGL(k_art_chain, dim3((unsigned)ch.n), dim3(64 * ART_CW), 0, sb.stream, d, b, e->d_rowinner, e->d_rowcross, a, beta, i * e->n, e->n, e->sx, ch.c0);
                    LAUNCHCHK();
                }
                return launch_bp_art(e, sb, x, e->np - 1, a, beta);
            };
            if ((rc = run_chains(e, chain))) return rc;
            return tomo_positivity(e, TOMO_VOL_RECON);
        }
        for (int i = 0; i < e->np; ++i) {
            if ((rc = launch_fp<FP_STORE>(e, x, i * e->n, e->n, nullptr, d))) return rc;
            hipLaunchKernelGGL(k_art_chain, dim3((unsigned)(e->sx / 64)), dim3(64 * ART_CW), 0, e->stream, d, b, e->d_rowinner, e->d_rowcross, a, beta, i * e->n, e->n, e->sx, 0);
            LAUNCHCHK();
            if ((rc = launch_bp_art(e, whole(e), x, i, a, beta))) return rc;
        }
        return tomo_positivity(e, TOMO_VOL_RECON);
    }
    hipLaunchKernelGGL(k_art, dim3(e->sxc / 64), dim3(64 * ART_WAVES), 0, e->stream, x, e->d_rptr, e->d_rent, e->sino[TOMO_SINO_B], e->d_rowinner, beta, (int)e->nrows, e->sx, d_order);
    LAUNCHCHK();
    int rc = tomo_positivity(e, TOMO_VOL_RECON);
    if (!rc && order_host) HIPCHK(hipStreamSynchronize(e->stream));   // the staging buffer holds the order until the sweep is done
    return rc;
}
