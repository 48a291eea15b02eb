// engine_options.inc -- part of tomo_engine.hip (ONE translation unit: the kernels are templates and asm blocks in headers; the host side is
// split by topic into files that tomo_engine.hip includes in order).  This part: C ABI: tomo_get_option / tomo_set_option and the per-kernel launch log (tomo_profile_*).

int tomo_get_option(tomo_engine *e, const char *name, int *value)
{
    if (!e || !name || !value) return fail(TOMO_ERR_ARG, "null argument");
    if (std::strcmp(name, "fp_strip") == 0) { *value = e->fp_strip; return TOMO_OK; }
    if (std::strcmp(name, "fp_strip_ready") == 0) { *value = e->fs_ok ? 1 : 0; return TOMO_OK; }
    if (std::strcmp(name, "fp_strip_slots") == 0) { *value = e->fs_ok ? e->fs_kused : 0; return TOMO_OK; }
    if (std::strcmp(name, "fp_tile") == 0) { *value = e->fp_tile; return TOMO_OK; }
    if (std::strcmp(name, "bp_tile") == 0) { *value = e->bp_tile; return TOMO_OK; }
    if (std::strcmp(name, "bp_list") == 0) { *value = e->bp_list; return TOMO_OK; }
    if (std::strcmp(name, "fgp_pair") == 0) { *value = e->fgp_pair; return TOMO_OK; }
    if (std::strcmp(name, "fp_list") == 0) { *value = e->fp_list; return TOMO_OK; }
    if (std::strcmp(name, "fp_list_ready") == 0) { *value = e->fl_ok ? 1 : 0; return TOMO_OK; }
    if (std::strcmp(name, "bp_list_ready") == 0) { *value = e->bl_ok ? 1 : 0; return TOMO_OK; }
    if (std::strcmp(name, "fp_reuse") == 0) { *value = e->claims.reuse(); return TOMO_OK; }
    if (std::strcmp(name, "art_chain_ready") == 0) { *value = e->art_chain_ok ? 1 : 0; return TOMO_OK; }     // natural-order ART runs as the chain
    if (std::strcmp(name, "sart_tile") == 0) { *value = e->sart_tile; return TOMO_OK; }
    if (std::strcmp(name, "sart_resident") == 0) { *value = e->sart_resident; return TOMO_OK; }
    if (std::strcmp(name, "sart_resident_ready") == 0) { *value = e->rs_ok ? 1 : 0; return TOMO_OK; }
    if (std::strcmp(name, "sart_resident_active") == 0) { *value = (e->rs_ok && e->sart_resident != 0) ? 1 : 0; return TOMO_OK; }
    if (std::strcmp(name, "sart_resident_spin") == 0) { *value = (int)std::min<uint32_t>(e->rs_spin_limit, 0x7FFFFFFFu); return TOMO_OK; }
    if (std::strcmp(name, "sart_resident_fallbacks") == 0) { *value = e->rs.fallbacks; return TOMO_OK; }            // sweeps that needed the streamed chain
    if (std::strcmp(name, "sart_resident_fallback_chunks") == 0) { *value = e->rs.fallback_chunks; return TOMO_OK; } // ... and the 64-slice chunks it swept
    if (std::strcmp(name, "sart_resident_skip") == 0) { *value = e->rs.skip; return TOMO_OK; }                       // sweeps the resident form still sits out
    if (std::strcmp(name, "sart_resident_last_code") == 0) { *value = e->rs.last_code; return TOMO_OK; }             // 1 residual rows, 2 tile sums (0: the commit)
    if (std::strcmp(name, "table_kib") == 0) { *value = (int)std::min<size_t>(e->table_bytes >> 10, 0x7FFFFFFF); return TOMO_OK; }   // device tables built at creation
    if (std::strcmp(name, "create_ms") == 0) { *value = (int)std::min(e->create_ms + 0.5, 2147483647.0); return TOMO_OK; }           // what creating this engine took
    if (std::strcmp(name, "stage_bytes") == 0) { *value = (int)std::min<size_t>(e->stage_bytes, 0x7FFFFFFF); return TOMO_OK; }   // staging buffer of the host data calls (0: never allocated)
    if (std::strcmp(name, "pool_bytes") == 0) { *value = (int)std::min<size_t>(e->pool.bytes(), 0x7FFFFFFF); return TOMO_OK; }   // the registry's live allocations, summed
    if (std::strcmp(name, "tv_halo_fold") == 0) { *value = e->tv.halo_fold; return TOMO_OK; }
    if (std::strcmp(name, "form_fp") == 0) { *value = select_forms(e).fp; return TOMO_OK; }
    if (std::strcmp(name, "form_bp") == 0) { *value = select_forms(e).bp; return TOMO_OK; }
    if (std::strcmp(name, "form_sart") == 0) { *value = select_forms(e).sart; return TOMO_OK; }
    if (std::strcmp(name, "rccl_version") == 0) { *value = g_rccl.version; return TOMO_OK; }     // 0 until a communicator has been opened
    if (std::strcmp(name, "comm_rounds") == 0) { *value = (int)std::min<int64_t>(e->comm_rounds, 0x7FFFFFFF); return TOMO_OK; }
    return fail(TOMO_ERR_ARG, std::string("unknown option ") + name);
}

int tomo_set_option(tomo_engine *e, const char *name, int value)
{
    if (!e || !name) return fail(TOMO_ERR_ARG, "null argument");
    if (std::strcmp(name, "fgp_fused") == 0) { e->fgp_fused = value ? 1 : 0; return TOMO_OK; }
    if (std::strcmp(name, "fgp_pair") == 0) { e->fgp_pair = value ? 1 : 0; return TOMO_OK; }
    if (std::strcmp(name, "sart_fused") == 0) { e->sart_fused = value ? 1 : 0; return TOMO_OK; }
    if (std::strcmp(name, "fp_all_lpr") == 0) { e->fp_all_lpr = (value == 16 || value == 32) ? value : 0; return TOMO_OK; }
    if (std::strcmp(name, "art_chain") == 0) { e->art_chain = value ? 1 : 0; return TOMO_OK; }
    if (std::strcmp(name, "sart_tile") == 0) { e->sart_tile = value ? 1 : 0; return TOMO_OK; }
    if (std::strcmp(name, "sart_resident") == 0) { e->sart_resident = value < 0 ? -1 : (value ? 1 : 0); e->rs.skip = e->rs.backoff = 0; return TOMO_OK; }
    if (std::strcmp(name, "sart_resident_spin") == 0) { e->rs_spin_limit = value < 0 ? (1u << 21) : (uint32_t)value; return TOMO_OK; }   // polls before a wait gives up (< 0: the default; tests: tiny, 0 = at the first look)
    if (std::strcmp(name, "sart_resident_test_fail") == 0) { e->rs_test_fail = std::max(0, value); return TOMO_OK; }   // tests: chunk + 1 that refuses to commit
    if (std::strcmp(name, "fp_reuse") == 0) { e->claims.set_reuse(value != 0); return TOMO_OK; }
    if (std::strcmp(name, "sart_streams") == 0) { e->sart_streams = value >= 2 ? std::min(value, (int)tomo_engine::MAX_CHAINS) : (value == 1 ? 1 : 0); return TOMO_OK; }
    if (std::strcmp(name, "art_tile") == 0) { e->art_tile = value ? 1 : 0; return TOMO_OK; }
    if (std::strcmp(name, "sart_skip_same") == 0) { e->sart_skip_same = value ? 1 : 0; return TOMO_OK; }
    if (std::strcmp(name, "sart_nt") == 0) { e->sart_nt = value < 0 ? -1 : (value ? 1 : 0); return TOMO_OK; }
    if (std::strcmp(name, "sart_coop") == 0) { e->sart_coop = value ? 1 : 0; return TOMO_OK; }
    if (std::strcmp(name, "sart_coop_spin") == 0) { e->sart_coop_spin = value < 0 ? -1 : value; return TOMO_OK; }
    if (std::strcmp(name, "bp_tile") == 0) { e->bp_tile = value ? 1 : 0; return TOMO_OK; }
    if (std::strcmp(name, "bp_list") == 0) { e->bp_list = value ? 1 : 0; return TOMO_OK; }
    if (std::strcmp(name, "bp_list_band") == 0) { e->bp_list_band = value ? 1 : 0; return TOMO_OK; }
    if (std::strcmp(name, "fp_list") == 0) { e->fp_list = value ? 1 : 0; return TOMO_OK; }
    // all-angle FP form: "fp_strip" = 1 (default) sheared strips; asking for "fp_tile" = 1 / 0 explicitly selects the tile-stationary /
    // the ray-driven form (and takes the strips out of the way until "fp_strip" = 1 is set again)
    if (std::strcmp(name, "fp_strip") == 0) { e->fp_strip = value ? 1 : 0; return TOMO_OK; }
    if (std::strcmp(name, "fp_tile") == 0) { e->fp_tile = value ? 1 : 0; e->fp_strip = 0; return TOMO_OK; }
    if (std::strcmp(name, "fp_tile_chunks_per_pass") == 0) {   // any count >= 1 (0 = from the scratch cap); before the first projection
        if (value < 0 || fp_scratch_exists(e)) return fail(TOMO_ERR_STATE, "fp_tile_chunks_per_pass must be set before the first projection");
        e->ft_ncp_forced = value; fp_forget_plans(e); return TOMO_OK;
    }
    if (std::strcmp(name, "fp_tile_scratch_mib") == 0) {   // cap of the partial-sum scratch; takes effect before the first all-angle FP
        if (value <= 0 || fp_scratch_exists(e)) return fail(TOMO_ERR_STATE, "fp_tile_scratch_mib must be positive and set before the first projection");
        e->ft_scratch_cap = (size_t)value << 20; fp_forget_plans(e); return TOMO_OK;
    }
    if (std::strcmp(name, "tv_gnorm_slot") == 0) {
        if (value < 0 || value >= TOMO_S_COUNT) return fail(TOMO_ERR_ARG, "bad scalar slot");
        e->gnorm_slot = value; return TOMO_OK;
    }
    if (std::strcmp(name, "tv_tz") == 0) { e->tv.tz = value == 4 ? 4 : 8; return TOMO_OK; }
    if (std::strcmp(name, "tv_halo_fold") == 0) { e->tv.halo_fold = value < 0 ? -1 : (value ? 1 : 0); return TOMO_OK; }
    if (std::strcmp(name, "tv_march4") == 0) { e->tv.march4 = value ? 1 : 0; return TOMO_OK; }
    if (std::strcmp(name, "tv_yseg") == 0) { e->tv.yseg = value < 0 ? 0 : value; return TOMO_OK; }
    if (std::strcmp(name, "tv_recompute") == 0) { e->tv.recompute = value ? 1 : 0; return TOMO_OK; }
    if (std::strcmp(name, "tv_lds") == 0) { e->tv.lds = value; return TOMO_OK; }   // 1 register march, 8 / 16 LDS march (z-columns per workgroup), 0 direct
    return fail(TOMO_ERR_ARG, std::string("unknown option ") + name);
}

// ---- measurement ------------------------------------------------------------------------------------------------------------
int tomo_profile_enable(tomo_engine *e, int kernel, int on)
{
    NEED(e);
    if (kernel < 0 || kernel >= PROF_MAX_KERNELS) return fail(TOMO_ERR_ARG, "bad kernel id");
    HIPCHK(hipStreamSynchronize(e->stream));
    e->prof[kernel].on = on != 0;
    e->prof[kernel].stride = on > 1 ? (unsigned)on : 1u;     // on = N > 1: bracket every N-th launch only
    e->prof[kernel].seen = 0;
    e->prof[kernel].used = 0;
    e->prof[kernel].dropped = 0;
    if (on) {
        if (!e->prof[kernel].ref) HIPCHK(hipEventCreate(&e->prof[kernel].ref));
        HIPCHK(hipEventRecord(e->prof[kernel].ref, e->stream));
    }
    return TOMO_OK;
}

// busy_ms (may be null): time during which AT LEAST ONE launch of the kernel was executing (union of the launch intervals
// on the common time base) -- with the SART sweep on two streams two launches of one kernel overlap, and sum / launches
// is then the duration of a launch that shares the chip, not the chip's rate
int tomo_profile_read2(tomo_engine *e, int kernel, int64_t *launches, double *total_ms, double *busy_ms)
{
    NEED(e);
    if (kernel < 0 || kernel >= PROF_MAX_KERNELS || !launches || !total_ms) return fail(TOMO_ERR_ARG, "bad argument");
    HIPCHK(hipStreamSynchronize(e->stream));
    for (int u = 0; u < tomo_engine::MAX_CHAINS; ++u) if (e->sub_stream[u]) HIPCHK(hipStreamSynchronize(e->sub_stream[u]));
    if (e->aux) HIPCHK(hipStreamSynchronize(e->aux));
    ProfSlot &p = e->prof[kernel];
    double tot = 0;
    std::vector<std::pair<float, float>> iv;
    for (size_t i = 0; i + 1 < p.used; i += 2) {
        float ms = 0;
        HIPCHK(hipEventElapsedTime(&ms, p.ev[i], p.ev[i + 1]));
        tot += ms;
        if (busy_ms && p.ref) {
            float t0 = 0;
            HIPCHK(hipEventElapsedTime(&t0, p.ref, p.ev[i]));
            iv.emplace_back(t0, t0 + ms);
        }
    }
    if (busy_ms) {
        std::sort(iv.begin(), iv.end());
        double busy = 0; float run_a = 0, run_b = -1;
        for (auto &q : iv) {
            if (run_b < run_a || q.first > run_b) { if (run_b >= run_a) busy += run_b - run_a; run_a = q.first; run_b = q.second; }
            else run_b = std::max(run_b, q.second);
        }
        if (run_b >= run_a) busy += run_b - run_a;
        *busy_ms = busy;
    }
    *launches = (int64_t)(p.used / 2);
    *total_ms = tot;
    p.used = 0;
    if (p.dropped) {   // never report an average over a silently truncated log
        std::string msg = std::to_string(p.dropped) + " launches were not recorded (event log full)";
        p.dropped = 0;
        return fail(TOMO_ERR_STATE, msg);
    }
    return TOMO_OK;
}

// the launch intervals of a kernel [t0, t1) in ms since ref_engine's log of the same kernel was switched on (engines of a slab
// group share one device: their events are on one time base); does not reset the log
int tomo_profile_intervals(tomo_engine *e, int kernel, tomo_engine *ref_engine, double *t0, double *t1, int cap, int *count)
{
    NEED(e);
    if (kernel < 0 || kernel >= PROF_MAX_KERNELS || !ref_engine || !count) return fail(TOMO_ERR_ARG, "bad argument");
    HIPCHK(hipStreamSynchronize(e->stream));
    ProfSlot &p = e->prof[kernel];
    hipEvent_t ref = ref_engine->prof[kernel].ref;
    if (!ref) return fail(TOMO_ERR_STATE, "the reference engine's log is not enabled");
    int n = (int)(p.used / 2);
    *count = n;
    if (!t0 || !t1 || cap < n) return cap == 0 ? TOMO_OK : fail(TOMO_ERR_ARG, "interval buffers too small");
    for (int i = 0; i < n; ++i) {
        float a = 0, d = 0;
        HIPCHK(hipEventElapsedTime(&a, ref, p.ev[2 * i]));
        HIPCHK(hipEventElapsedTime(&d, p.ev[2 * i], p.ev[2 * i + 1]));
        t0[i] = a; t1[i] = a + d;
    }
    return TOMO_OK;
}

int tomo_profile_read(tomo_engine *e, int kernel, int64_t *launches, double *total_ms)
{
    return tomo_profile_read2(e, kernel, launches, total_ms, nullptr);
}
