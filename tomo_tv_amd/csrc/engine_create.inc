// engine_create.inc -- part of tomo_engine.hip (ONE translation unit: the kernels are templates and asm blocks in headers; the host side is
// split by topic into files that tomo_engine.hip includes in order).  This part: creation: host tables -> device (finish_create_impl), teardown on failure.

// ---- creation ----------------------------------------------------------------------------------------------
// host tables are released as soon as they are on the device (peak host memory: a few times nnz * 8 bytes per engine,
// and one process per GPU builds its own)
template <class V> static void release(V &v) { V().swap(v); }

// Host tables onto the device.  A Tab names one: the member that will hold it, the host data, and the least size of its allocation (what the
// kernels may address of a table that can be empty, or prefetch behind its end); tab() makes one of a vector, or of a pointer and its bytes.
struct Tab { void **slot; const void *host; size_t bytes, min_bytes; };
template <class D, class T> static Tab tab(D **slot, const std::vector<T> &v, size_t min_elems = 0) { return Tab{(void **)slot, v.data(), v.size() * sizeof(T), min_elems * sizeof(T)}; }
template <class D> static Tab tab(D **slot, const void *host, size_t bytes) { return Tab{(void **)slot, host, bytes, 0}; }
// each table allocated (the geometry's memory) and then copied, in the order given; the first error ends it
static int upload_tables(tomo_engine *e, std::initializer_list<Tab> tabs)
{
    for (const Tab &t : tabs) {
        int rc = dev_alloc(e, GEOMETRY, t.slot, std::max(t.bytes, t.min_bytes), false);
        if (rc) return rc;
        HIPCHK(hipMemcpy(*t.slot, t.host, t.bytes, hipMemcpyHostToDevice));
    }
    return TOMO_OK;
}

// matrix entries as the kernels load them: {offset, the weight's bits}
template <class O>
static std::vector<uint2> pack_entries(const O *off, const float *w, size_t n)
{
    std::vector<uint2> ent(n);
    for (size_t k = 0; k < n; ++k) { uint32_t bits; std::memcpy(&bits, &w[k], 4); ent[k] = make_uint2((uint32_t)off[k], bits); }
    return ent;
}

// Walk lists + equal-sized segment items of the ray-walk SART step (k_sart_seg): the form of matrices whose tile tables do not exist and
// of "sart_tile" = 0.  Round 6: where the tile tables exist and the engine knows its angles, these tables are built on first use
// (ensure_seg_tables) instead of at creation -- 0.19 of 2.3 s at 512^2 x 90, 0.93 of 9.4 s at 1024^2 x 120, 0.25 / 1.4 GB of device
// memory; TOMO_EAGER_TABLES = 1 builds them at creation as before.  (The other fallback families stay eager: whether they CAN serve a
// geometry -- st_ok, fb_ok, fl_ok ... -- is the outcome of their build, and select_forms needs those answers.)
static int build_seg_tables(tomo_engine *e, const Coo &m, Tables &t)
{
    int rc;
    build_walk(m, e->n, e->np, t);
    {
        const std::vector<uint2> went = pack_entries(t.walk_pix.data(), t.walk_w.data(), t.walk_pix.size());
        if ((rc = upload_tables(e, {tab(&e->d_wptr, t.walk_ptr), tab(&e->d_went, went, 1)}))) return rc;
    }
    {
        const int seg_len = 32;   // visits per work item: 16/32/64/128 measured 222/224/233/242 us per fused step at 512^3
        build_segments(e->n, e->np, seg_len, t);
        static_assert(sizeof(Tables::SegItem) == sizeof(SegItemD), "segment item layout");
        e->h_seg_exec_ptr = t.seg_exec_ptr;
        e->max_items = t.max_items_per_angle;
        if ((rc = upload_tables(e, {tab(&e->d_seg_exec, t.seg_exec, 1), tab(&e->d_row_first, t.row_first), tab(&e->d_row_nseg, t.row_nseg)}))) return rc;
        release(t.walk_pix); release(t.walk_w); release(t.walk_ptr); release(t.seg_exec); release(t.row_first); release(t.row_nseg);
    }
    e->seg_ready = true;
    return TOMO_OK;
}

static int ensure_seg_tables(tomo_engine *e)
{
    if (e->seg_ready) return TOMO_OK;
    if (e->angles.empty()) return fail(TOMO_ERR_STATE, "the ray-walk tables were not built and the engine does not know its angles");
    Coo m;
    build_parallel_ray(e->n, e->np, e->angles.data(), m);
    sort_rows(m);
    Tables t;
    std::string err;
    if (!build_tables(m, e->n, e->np, t, err)) return fail(TOMO_ERR_GEOMETRY, err);
    return build_seg_tables(e, m, t);
}

static int finish_create_impl(tomo_engine *e, Coo &m, tomo_engine **out)
{
    Tables t;
    std::string err;
    const bool timing = std::getenv("TOMO_BUILD_TIMING") != nullptr;      // per-phase wall clock of the table builders to stderr
    auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    double t_last = now();
    auto lap = [&](const char *what) { if (timing) { double x = now(); std::fprintf(stderr, "tomo_create: %-32s %.3f s\n", what, x - t_last); t_last = x; } };
    sort_rows(m);
    lap("sort_rows");
    if (!build_tables(m, e->n, e->np, t, err)) return fail(TOMO_ERR_GEOMETRY, err);
    lap("build_tables");
    e->nnz = m.ptr[m.nrow];
    if (e->nnz >= (int64_t)0xFFFFFFFFu) return fail(TOMO_ERR_ARG, "matrix too large for 32-bit entry offsets");
    e->lipschitz = t.lipschitz;
    e->lipschitz_cimmino = t.lipschitz_cimmino;
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking));
    e->own_stream = true;

    std::vector<uint32_t> ptr32(m.nrow + 1);
    for (int64_t r = 0; r <= m.nrow; ++r) ptr32[r] = (uint32_t)m.ptr[r];
    std::vector<uint2> ent = pack_entries(m.col.data(), m.val.data(), (size_t)e->nnz);
    int rc;
    if ((rc = upload_tables(e, {tab(&e->d_rptr, ptr32), tab(&e->d_rent, ent, 1), tab(&e->d_rowsum, t.rowsum), tab(&e->d_rowinner, t.rowinner),
                                tab(&e->d_colsum_all, t.colsum_all), tab(&e->d_rowcross, t.rowcross), tab(&e->d_cell, t.cell)}))) return rc;
    e->art_chain_ok = t.art_chain_ok;      // (the cells go up here: build_tables wrote them, every later builder only reads them)
    lap("csr / cells upload");
    {
        build_tiles(m, e->n, e->np, FT_TY, FT_TZ, 256, t);
        static_assert(Tables::TILE_SLOTS == FT_SLOTS && Tables::TILE_BATCH == FT_BATCH, "tile stream shape");
        e->ft_tiles_z = t.tiles_z; e->ft_ntiles = t.tiles_y * t.tiles_z;
        e->ft.nseg = t.tile_nseg;
        std::vector<uint2> tent = pack_entries(t.tile_off.data(), t.tile_w.data(), t.tile_off.size());
        if ((rc = upload_tables(e, {tab(&e->d_ft_slot_ptr, t.tile_slot_ptr), tab(&e->d_ft_slot_seg0, t.tile_slot_seg0, 1), tab(&e->d_ft_tent, tent),
                                    tab(&e->ft.d_rsptr, t.rseg_ptr), tab(&e->ft.d_rsidx, t.rseg_idx)}))) return rc;
        release(tent); release(t.tile_off); release(t.tile_w); release(t.rseg_idx); release(t.rseg_ptr); release(t.tile_slot_ptr); release(t.tile_slot_seg0);
        lap("build_tiles + upload");
        {   // sheared-strip tables of the all-angle FP; a geometry they cannot hold (a user matrix whose rays are no lines) keeps the tile form
            std::string why;
            static_assert(Tables::FS_W == FS_W && Tables::FS_H == FS_H && Tables::FS_WAVES == FS_WAVES && Tables::FS_GROUPS == FS_GROUPS, "strip shape");
            static_assert(sizeof(Tables::FsItem) == sizeof(FsItemD), "strip item layout");
            // Measured (round 4, MI355X, FP alone, strips against tiles; strips cut into segments of 16 tiles): 1024 x 512^2 x 90 2.53 / 2.87 ms,
            // 512^3 x 90 1.32 / 1.44, 128 x 1024^2 x 120 1.71 / 1.83, 1024^3 x 120 12.1 / 14.6 -- and 256 x 512^2 0.71 / 0.70, 64 x 512^2 0.235 / 0.196,
            // 256^3 x 60 0.143 / 0.122: an item is a sequential march of up to 16 tiles, and the form pays once a launch has several rounds
            // of them over the 512 resident workgroups: passes (~6.5 with the shear's overhang) x strips x segments x chunks >= 3000.
            // TOMO_FP_STRIP = 0 / 1 overrides the rule (tests build the tables at small sizes).
            const int fs_tiles = (e->n + FS_H - 1) / FS_H, fs_seglen = std::max(4, std::min(16, fs_tiles / 2));
            const double fs_wgs = 6.5 * ((double)e->n / FS_W) * ((fs_tiles + fs_seglen - 1) / fs_seglen) * (e->sxc / 64);
            bool want = e->n >= 384 && fs_wgs >= 3000.0;
            if (const char *env = std::getenv("TOMO_FP_STRIP")) want = std::atoi(env) != 0;
            e->fs_ok = want && build_fp_strips(m, e->n, e->np, 256, e->sxc / 64, t, why);
            if (e->fs_ok) {
                e->fs_nitems = (int)t.fs_item.size(); e->fs_kused = t.fs_kused; e->fs.nseg = t.fs_nseg;
                static_assert(sizeof(uint2) == sizeof(uint64_t), "entry layout");
                if ((rc = upload_tables(e, {tab(&e->d_fs_items, t.fs_item), tab(&e->d_fs_orient, t.fs_orient), tab(&e->d_fs_shift, t.fs_shift), tab(&e->d_fs_cnt, t.fs_cnt),
                                            tab(&e->d_fs_gstart, t.fs_gstart), tab(&e->d_fs_gseg0, t.fs_gseg0), tab(&e->d_fs_ent, t.fs_ent.get(), t.fs_ent_n * sizeof(uint2)),
                                            tab(&e->fs.d_rsptr, t.fs_rseg_ptr), tab(&e->fs.d_rsidx, t.fs_rseg_idx)}))) return rc;
                if ((rc = dev_alloc(e, GEOMETRY, (void **)&e->d_fs_zero, 256, true))) return rc;
            }
            t.fs_ent.reset(); t.fs_ent_n = 0; release(t.fs_cnt); release(t.fs_rseg_idx); release(t.fs_rseg_ptr); release(t.fs_gstart); release(t.fs_gseg0);
        }
        lap("build_fp_strips + upload");
        {   // the same strips as wave-uniform entry lists (k_fp_list); by the same rule (TOMO_FP_LIST = 0 / 1 overrides it)
            std::string why;
            static_assert(Tables::FL_W == FL_W && Tables::FL_TH == FL_TH && Tables::FL_WAVES == FL_WAVES && Tables::FL_BATCH == FL_BATCH && Tables::FL_PIXB == FL_PIXB, "list shape");
            static_assert(sizeof(Tables::FlItem) == sizeof(FlItemD), "list item layout");
            bool want = e->fs_ok;
            if (const char *env = std::getenv("TOMO_FP_LIST")) want = std::atoi(env) != 0;
            e->fl_ok = want && build_fp_lists(m, e->n, e->np, t, why);
            // The waves of a workgroup meet at a barrier after every tile, so a tile costs its busiest wave; build_fp_lists deals the rays
            // to the waves by load (fl_balance = mean / max batches per wave and tile: 0.89-0.90 on the BASELINE geometries).  Measured
            // (MI355X, FP alone, lists against strips): 512^3 x 90 1.12 / 1.22 ms, 512^3 x 70 0.92 / 1.06, 128 x 512^2 x 90 0.35 / 0.39,
            // 256^3 x 60 0.138 / 0.147, 128 x 1024^2 x 120 1.58 / 1.58.  A geometry that cannot be balanced keeps the strips.
            if (e->fl_ok && !std::getenv("TOMO_FP_LIST") && t.fl_balance < 0.8) e->fl_ok = false;
            if (e->fl_ok) {
                e->fl_nitems = (int)t.fl_item.size(); e->fl.nseg = t.fl_nseg; e->fl.pairs = true;   // whole 128-slice pieces
                if ((rc = upload_tables(e, {tab(&e->d_fl_items, t.fl_item), tab(&e->d_fl_orient, t.fl_orient), tab(&e->d_fl_shift, t.fl_shift),
                                            tab(&e->d_fl_ent, t.fl_ent.get(), t.fl_ent_n * sizeof(uint2)), tab(&e->d_fl_ptr, t.fl_ptr), tab(&e->d_fl_fent, t.fl_flush),
                                            tab(&e->d_fl_fptr, t.fl_fptr), tab(&e->fl.d_rsptr, t.fl_rseg_ptr), tab(&e->fl.d_rsidx, t.fl_rseg_idx)}))) return rc;
                if ((rc = dev_alloc(e, GEOMETRY, (void **)&e->d_fl_zero, 512, true))) return rc;
            }
            t.fl_ent.reset(); t.fl_ent_n = 0; release(t.fl_flush); release(t.fl_ptr); release(t.fl_fptr); release(t.fl_rseg_ptr); release(t.fl_rseg_idx); release(t.fl_item); release(t.fl_shift);
        }
        lap("build_fp_lists + upload");
        build_sart_tiles(m, e->n, e->np, ST_TY, ST_TZ, ST_MAXR, 256, t);
        static_assert(Tables::ST_MAXSEG == ST_MAXSEG, "segment slots per tile");
        e->st_ok = t.st_ok;
        if (e->st_ok) {
            e->st_ntiles = t.st_tiles; e->st_tiles_z = t.st_tiles_z; e->st_max_ids = t.st_max_ids;
            const std::vector<uint2> sent = pack_entries(t.st_off.data(), t.st_w.data(), t.st_off.size());
            if ((rc = upload_tables(e, {tab(&e->d_st_cell, t.st_cell), tab(&e->d_st_win, t.st_win), tab(&e->d_st_segid, t.st_segid), tab(&e->d_st_seg, t.st_seg),
                                        tab(&e->d_st_ent, sent), tab(&e->d_st_row_first, t.st_row_first), tab(&e->d_st_row_nseg, t.st_row_nseg)}))) return rc;
        }
        release(t.st_cell); release(t.st_off); release(t.st_w); release(t.st_seg); release(t.st_segid); release(t.st_win);
        lap("build_sart_tiles + upload");
        if (!e->st_ok || e->angles.empty() || std::getenv("TOMO_EAGER_TABLES")) {      // else: on first use (ensure_seg_tables)
            if ((rc = build_seg_tables(e, m, t))) return rc;
        }
        lap("build_walk + build_segments + upload");
        {   // tables of the volume-resident sweep (resident.cpp); TOMO_SART_RESIDENT = 0 leaves them out
            static_assert(Resident::T == RS_T && Resident::WAVES == RS_WAVES && Resident::MAXWIN == RS_MAXWIN && Resident::RL == RS_RL && Resident::USABLE == RS_USABLE &&
                          Resident::TSN == 8 && Resident::SINK == 14 && sizeof(Resident::Hdr) == sizeof(RsHdrD), "k_sart_resident geometry (resident.h)");
            bool want = e->n % 8 == 0;
            if (const char *env = std::getenv("TOMO_SART_RESIDENT")) want = want && std::atoi(env) != 0;
            e->rs_ok = false;
            if (want) {
                hipDeviceProp_t prop;
                HIPCHK(hipGetDeviceProperties(&prop, e->device));
                e->rs_cus = prop.multiProcessorCount;
                Resident R;
                build_sart_resident(e->n, e->np, t, e->rs_cus, R);
                // every workgroup of a launch must be on the chip at once: the runtime's own count of workgroups per CU for this kernel
                // (registers, LDS) has to cover the launch; and the chunks of a sweep that could not finish go to the tile chain
                // (a runtime that cannot answer admits nothing: the sweep is an option, the engine is not -- rs_ok stays false)
                int per_cu = 0;
                if (R.ok && hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void *)k_sart_resident, RS_THREADS, 0) != hipSuccess) {
                    (void)hipGetLastError();
                    per_cu = 0;
                }
                if (R.ok && e->st_ok && (int64_t)per_cu * e->rs_cus >= R.ntiles) {
                    e->rs_ntiles = R.ntiles; e->rs_tiles = R.tiles; e->rs_rpt = R.rpt;
                    e->rs_groups = std::max(1, std::min(per_cu * e->rs_cus / R.ntiles, e->sxc / 64));
                    e->rs_pb_bytes = (size_t)e->rs_groups * R.ntiles * RS_MAXWIN * 64 * sizeof(rs_u64);
                    e->rs_rb_bytes = (size_t)e->rs_groups * e->np * e->n * 64 * sizeof(rs_u64);
                    if ((rc = upload_tables(e, {tab(&e->d_rs_hdr, R.hdr), tab(&e->d_rs_cell, R.cell), tab(&e->d_rs_ts, R.ts), tab(&e->d_rs_rl, R.rl)}))) return rc;
                    if ((rc = dev_alloc(e, GEOMETRY, (void **)&e->rs_pb, e->rs_pb_bytes, true)) || (rc = dev_alloc(e, GEOMETRY, (void **)&e->rs_rb, e->rs_rb_bytes, true))) return rc;     // tag 0 = never written
                    if (!e->rs_abort) { HIPCHK(hipHostMalloc((void **)&e->rs_abort, sizeof(int), hipHostMallocMapped)); *e->rs_abort = 0; }
                    if ((rc = dev_alloc(e, GEOMETRY, (void **)&e->d_rs_abort, sizeof(int), true)) || (rc = dev_alloc(e, GEOMETRY, (void **)&e->d_rs_commit, (size_t)(e->sxc / 64) * sizeof(unsigned), true))) return rc;
                    if (!e->rs_done) { HIPCHK(hipHostMalloc((void **)&e->rs_done, (size_t)(e->sxc / 64) * sizeof(int), hipHostMallocMapped)); }
                    std::memset(e->rs_done, 0, (size_t)(e->sxc / 64) * sizeof(int));
                    e->rs.epoch = 0; e->rs.seq = 0; e->rs.commit_base = 0; e->rs.commit_dirty = false;
                    e->rs_ok = true;
                }
            }
        }
        lap("build_sart_resident + upload");
        build_bp_tiles(e->n, e->np, FT_TY, FT_TZ, FB_A, FB_MAXR, 256, 2 * FB_A, t);   // the cell ring prefetches up to angle P + 2*FB_A - 2
        static_assert(sizeof(Tables::TileCell) == sizeof(uint4), "tile cell layout");
        e->fb_ok = t.bp_tile_ok && e->np <= FB_MAX_PROJ;
        e->bl_ok = false;
        if (e->fb_ok) {
            if ((rc = upload_tables(e, {tab(&e->d_fb_cell, t.bp_cell), tab(&e->d_fb_win, t.bp_win)}))) return rc;
            release(t.bp_cell);
        }
        lap("build_bp_tiles + upload");
        static_assert(BL_TY == Tables::BL_TY && BL_TZ == Tables::BL_TZ && BL_WAVES == Tables::BL_WAVES && BL_A == Tables::BL_A && BL_MAXR == Tables::BL_MAXR &&
                      BL_ROWB == Tables::BL_ROWB && BL_BATCH == Tables::BL_BATCH, "k_bp_list geometry (sysmat.h)");
        build_bp_lists(e->n, e->np, BL_TY, BL_TZ, BL_A, BL_MAXR, BL_ROWB, BL_WAVES, BL_BATCH, Tables::BL_REGS, t);
        // (k_bp_list keeps a stage's list bounds and window words per lane; its staging offsets are 32-bit)
        e->bl_ok = t.bl_ok && (e->np + BL_A - 1) / BL_A <= 64;
        if (e->bl_ok) {
            const size_t nent = (size_t)(t.bl_nbatch + 1) * BL_BATCH;
            e->bl_tiles_z = (e->n + BL_TZ - 1) / BL_TZ;
            e->bl_ntiles = ((e->n + BL_TY - 1) / BL_TY) * e->bl_tiles_z;
            if ((rc = upload_tables(e, {tab(&e->d_bl_ent, t.bl_ent.get(), nent * sizeof(uint4)), tab(&e->d_bl_ptr, t.bl_ptr), tab(&e->d_bl_win, t.bl_win)}))) return rc;
            t.bl_ent.reset();
        }
        release(t.bl_win); release(t.bl_ptr);
    }
    lap("build_bp_lists + upload");
    static_assert(sizeof(Cell) == sizeof(CellD), "cell layout");
    e->table_bytes = e->pool.bytes();              // what follows are fields, not tables
    if ((rc = dev_alloc(e, ENGINE, (void **)&e->d_scal_own, TOMO_S_COUNT * sizeof(double), true)) || (rc = dev_alloc(e, ENGINE, (void **)&e->d_part, NPART * sizeof(double), true))) return rc;
    e->d_scal = e->d_scal_own;
    if ((rc = dev_alloc(e, ENGINE, (void **)&e->halo_lo_own, e->npix * sizeof(float), true)) || (rc = dev_alloc(e, ENGINE, (void **)&e->halo_hi_own, e->npix * sizeof(float), true))) return rc;
    e->halo_lo = e->halo_lo_own; e->halo_hi = e->halo_hi_own;
    float *tmp;
    if ((rc = get_vol(e, TOMO_VOL_RECON, &tmp)) || (rc = get_sino(e, &e->sino[TOMO_SINO_B], &tmp))) return rc;
    HIPCHK(hipStreamSynchronize(e->stream));
    *out = e;
    return TOMO_OK;
}

extern "C" int tomo_destroy(tomo_engine *e);

// a half-built engine is torn down again (device buffers, stream) and the first error is the one reported
static int finish_create(tomo_engine *e, Coo &m, tomo_engine **out, double t_begin)
{
    int rc = finish_create_impl(e, m, out);
    e->create_ms = (std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count() - t_begin) * 1e3;
    if (rc) {
        std::string first = g_err;
        tomo_destroy(e);
        g_err = first;
    }
    return rc;
}

static tomo_engine *new_engine(int nslice, int nray, int nproj, int device)
{
    tomo_engine *e = new tomo_engine();
    e->nx = nslice; e->n = nray; e->np = nproj; e->device = device;
    e->sxc = ((nslice + 63) / 64) * 64;
    e->vec = (e->sxc % 256 == 0) ? 4 : (e->sxc % 128 == 0) ? 2 : 1;
    // Row pitch = computed width.  A pixel's row of slices that is a multiple of 4 KB (1024 slices) makes two sweep chains striding over
    // alternate halves of the rows alias the memory channels (round 2: 51.3 against 40.6 ms per sweep at 1024 slices), so such a slab
    // runs ONE chain (chain_count, engine_sart.inc).  Round 4 measured 64 slices of padding on the pitch so that it can run two: 1024^3 x 120 ASD-POCS
    // step 208.7 ms against 206.6 ms with one chain on the plain pitch -- no gain; the environment hook of that experiment is gone
    // (round 5, ADVICE r4: several launches size their work from the pitch, so a padded pitch was not safe to ship).
    e->sx = e->sxc;
    e->npix = (int64_t)nray * nray;
    e->nrows = (int64_t)nray * nproj;
    return e;
}

static int check_dims(int nslice, int nray, int nproj)
{
    if (nslice <= 0 || nray <= 0 || nproj <= 0) return fail(TOMO_ERR_ARG, "Nslice, Nray and Nproj must be positive");
    if (nray > 4096) return fail(TOMO_ERR_ARG, "Nray > 4096 not supported (float32 index storage limit of parallelRay)");
    return TOMO_OK;
}
