// engine_launch.inc -- part of tomo_engine.hip (ONE translation unit: the kernels are templates and asm blocks in headers; the host side is
// split by topic into files that tomo_engine.hip includes in order).  This part: which kernel family runs (select_forms, select_sart) and the
// launch helpers of the projectors (the steps of a SART sweep are in engine_sart.inc).  The forward projectors take the Lane they run on; the three
// partial-sum families of the all-angle one (tile, strip, list) differ in their main kernel only and share one pass loop (fp_passes).  Last: the
// checks, the stream ordering and the launch of the data calls on device buffers of the caller (tomo_set_*_device / tomo_get_*_device).

// ---- run-time value -> template argument ----------------------------------------------------------------------
// The ONE way a run-time value picks a kernel instantiation: f is called with a std::integral_constant of the value (the last
// of Vs where v is none of them) and launches inside, reading it as V().  Nest only parameters whose every combination exists.
template <int V0, int... Vs, class F>
static void with_int(int v, F &&f)
{
    if constexpr (sizeof...(Vs) == 0) f(std::integral_constant<int, V0>{});
    else if (v == V0) f(std::integral_constant<int, V0>{});
    else with_int<Vs...>(v, f);
}
template <class F> static void with_vec(int vec, F &&f) { with_int<4, 2, 1>(vec, f); }
template <class F> static void with_flag(bool b, F &&f) { if (b) f(std::true_type{}); else f(std::false_type{}); }

// the 64-slice chunks a launch covers: the sub-slab's, else the whole slab's
struct Chunks { int n, c0; };
static Chunks chunks64(const tomo_engine *e, const Sub &sb) { return sb.nc ? Chunks{sb.nc, sb.c0} : Chunks{e->sxc / 64, 0}; }

// ---- projector launches -------------------------------------------------------------------------------------
// Every projector takes the Lane it runs on (stream, partial sums of the epilogue's scalar, scratch index); the overloads without
// one run on the main lane.
// lpr: 0 = wide form (64*vec slices per workgroup, scalar table walk); 16 / 32 = narrow-chunk form with that
// many lanes per ray (k_fp_rows_g).  rowfac: the per-row factor of the epilogue.  Null means "the row sums" (d_rowsum), here and in
// launch_fp_all: a caller that names another table passes one that exists (d_rowinner is uploaded with the geometry).
template <int MODE>
static int launch_fp(tomo_engine *e, const Lane &ln, const float *x, int row0, int nrows, const float *b, float *out, int lpr = 0, const float *rowfac = nullptr)
{
    if (!rowfac) rowfac = e->d_rowsum;
    if (lpr == 16 || lpr == 32) {
        int R = 64 / lpr;
        int nchunk = e->sxc / (lpr * 4);
        int64_t waves = (int64_t)((nrows + R - 1) / R) * nchunk;
        dim3 grid((unsigned)((waves + 3) / 4)), block(256);
        with_int<16, 32>(lpr, [&](auto L) {
            hipLaunchKernelGGL((k_fp_rows_g<L(), MODE>), grid, block, 0, ln.stream, x, e->d_rptr, e->d_rent, b, rowfac, out, ln.part, row0, nrows, e->sx, nchunk);
        });
        LAUNCHCHK();
        return TOMO_OK;
    }
    int vec = e->vec;
    int nchunk = e->sxc / (64 * vec);
    dim3 grid((unsigned)((int64_t)nrows * nchunk)), block(256);
    with_vec(vec, [&](auto V) {
        hipLaunchKernelGGL((k_fp_rows<V(), MODE>), grid, block, 0, ln.stream, x, e->d_rptr, e->d_rent, b, rowfac, out, ln.part, row0, nrows, e->sx);
    });
    LAUNCHCHK();
    return TOMO_OK;
}
template <int MODE>
static int launch_fp(tomo_engine *e, const float *x, int row0, int nrows, const float *b, float *out, int lpr = 0, const float *rowfac = nullptr)
{
    return launch_fp<MODE>(e, main_lane(e), x, row0, nrows, b, out, lpr, rowfac);
}

// the row sums of chunks [c0, c0 + ncp) from the family's partial sums in the lane's scratch
template <int MODE>
static void launch_fp_reduce(tomo_engine *e, const Lane &ln, const FpFamily &f, const float *b, const float *rowfac, float *out, int c0, int ncp)
{
    int lpr = (ncp % 4 == 0) ? 64 : (ncp % 2 == 0) ? 32 : 16;
    int64_t items = (int64_t)e->nrows * (ncp * 16 / lpr);
    int64_t waves = (items + 64 / lpr - 1) / (64 / lpr);
    dim3 grid((unsigned)((waves + 3) / 4)), block(256);
    with_int<64, 32, 16>(lpr, [&](auto L) {
        hipLaunchKernelGGL((k_fp_tile_reduce<L(), MODE>), grid, block, 0, ln.stream, f.part[ln.idx], f.d_rsptr, f.d_rsidx, b, rowfac, out, ln.part, (int)e->nrows, e->sx, c0, ncp);
    });
}

// Chunks per pass of an all-angle FP whose scratch takes nseg partial rows per 64-slice chunk: what "ft_scratch_cap" holds (or the
// forced count), rounded down to whole 64- or 32-lane spans of the reduce; pairs: whole 128-slice pieces, a forced count too.
static int plan_ncp(const tomo_engine *e, uint32_t nseg, bool pairs)
{
    const int nchunk = e->sxc / 64, least = pairs ? 2 : 1;
    const size_t per_chunk = (size_t)std::max<uint32_t>(1, nseg) * 64 * sizeof(float);
    int ncp = (int)std::min<size_t>(nchunk, std::max<size_t>(least, e->ft_scratch_cap / per_chunk));
    if (e->ft_ncp_forced > 0) ncp = std::min(nchunk, std::max(least, e->ft_ncp_forced));
    if (e->ft_ncp_forced > 0 && !pairs) return ncp;
    if (ncp >= 4) return ncp & ~3;
    return pairs || ncp >= 2 ? 2 : ncp;
}

// the options that plan_ncp reads may change until a scratch has been sized by them
static bool fp_scratch_exists(const tomo_engine *e)
{
    for (const FpFamily *f : {&e->ft, &e->fs, &e->fl}) if (f->part[0] || f->part[1]) return true;
    return false;
}
static void fp_forget_plans(tomo_engine *e) { e->ft.ncp = e->fs.ncp = e->fl.ncp = 0; }

// The pass loop of the three families: the slab's chunks in passes of f.ncp (planned here on first use), each pass the family's main
// kernel -- launch_main(part, c0, ncp) writes the partial sums of chunks [c0, c0 + ncp) -- and then the reduce with the epilogue,
// both on the lane's stream.  The scratch is one pass large, one per lane that projects, allocated on that lane's first use.
template <int MODE, class F>
static int fp_passes(tomo_engine *e, const Lane &ln, FpFamily &f, const float *b, const float *rowfac, float *out, F &&launch_main)
{
    const int nchunk = e->sxc / 64;
    if (!f.ncp) f.ncp = plan_ncp(e, f.nseg, f.pairs);
    float *&part = f.part[ln.idx];
    if (!part) {
        if (int rc = dev_alloc(e, GEOMETRY, (void **)&part, (size_t)std::max<uint32_t>(1, f.nseg) * f.ncp * 64 * sizeof(float), false)) return rc;
    }
    for (int c0 = 0; c0 < nchunk; c0 += f.ncp) {
        const int ncp = std::min(f.ncp, nchunk - c0);              // (pairs: even, the slab is whole 128-slice pieces)
        {
            ProfScope ps(e, TOMO_K_FP_TILE, ln.stream);
            launch_main(part, c0, ncp);
            LAUNCHCHK();
        }
        {
            ProfScope ps(e, TOMO_K_FP_REDUCE, ln.stream);
            launch_fp_reduce<MODE>(e, ln, f, b, rowfac, out, c0, ncp);
            LAUNCHCHK();
        }
    }
    return TOMO_OK;
}

// all-angle FP, tile-stationary form (k_fp_tile + k_fp_tile_reduce)
template <int MODE>
static int launch_fp_tile(tomo_engine *e, const Lane &ln, const float *x, const float *b, float *out, const float *rowfac)
{
    if (!e->attr_fp) {   // per engine: the attribute belongs to the (function, device) pair
        HIPCHK(hipFuncSetAttribute((const void *)k_fp_tile, hipFuncAttributeMaxDynamicSharedMemorySize, FT_LDS_BYTES));
        e->attr_fp = true;
    }
    return fp_passes<MODE>(e, ln, e->ft, b, rowfac, out, [&](float *part, int c0, int ncp) {
        dim3 grid((unsigned)(8 * ((e->ft_ntiles + 7) / 8) * ncp)), block(FT_THREADS);
        hipLaunchKernelGGL(k_fp_tile, grid, block, FT_LDS_BYTES, ln.stream, x, e->d_ft_slot_ptr, e->d_ft_slot_seg0, e->d_ft_tent, part,
                           e->n, e->sx, e->ft_tiles_z, e->ft_ntiles, c0, ncp);
    });
}

// all-angle FP, sheared-strip form (k_fp_strip + k_fp_tile_reduce on the strips' row lists)
template <int MODE>
static int launch_fp_strip(tomo_engine *e, const Lane &ln, const float *x, const float *b, float *out, const float *rowfac)
{
    return fp_passes<MODE>(e, ln, e->fs, b, rowfac, out, [&](float *part, int c0, int ncp) {
        dim3 grid((unsigned)(8 * ((e->fs_nitems + 7) / 8) * ncp)), block(FS_THREADS);
        with_int<8, 12, 16>(e->fs_kused <= 8 ? 8 : e->fs_kused <= 12 ? 12 : 16, [&](auto K) {
            hipLaunchKernelGGL((k_fp_strip<K()>), grid, block, 0, ln.stream, x, e->d_fs_items, e->d_fs_orient, e->d_fs_shift, e->d_fs_cnt,
                               e->d_fs_gstart, e->d_fs_gseg0, e->d_fs_ent, part, e->n, e->sx, e->fs_nitems, c0, ncp, e->d_fs_zero);
        });
    });
}

// all-angle FP, sheared strips as wave-uniform entry lists (k_fp_list + k_fp_tile_reduce on the lists' row lists)
template <int MODE>
static int launch_fp_list(tomo_engine *e, const Lane &ln, const float *x, const float *b, float *out, const float *rowfac)
{
    if (!e->attr_fl) {
        HIPCHK(hipFuncSetAttribute((const void *)k_fp_list, hipFuncAttributeMaxDynamicSharedMemorySize, FL_LDS_BYTES));
        e->attr_fl = true;
    }
    return fp_passes<MODE>(e, ln, e->fl, b, rowfac, out, [&](float *part, int c0, int ncp) {
        dim3 grid((unsigned)(8 * ((e->fl_nitems + 7) / 8) * (ncp / 2))), block(FL_THREADS);
        hipLaunchKernelGGL(k_fp_list, grid, block, FL_LDS_BYTES, ln.stream, x, e->d_fl_items, e->d_fl_orient, e->d_fl_shift, e->d_fl_ent, e->d_fl_ptr,
                           e->d_fl_fent, e->d_fl_fptr, part, e->n, e->sx, e->fl_nitems, c0 / 2, ncp / 2, ncp, e->d_fl_zero);
    });
}

// ---- which form runs ---------------------------------------------------------------------------------------------------------
// ONE place decides which kernel family an operation of this engine uses, from what finish_create_impl could build for the geometry
// (the *_ok flags), the slab's shape and the options in force; the launchers below ask it, and so can a host
// (tomo_get_option "form_fp" / "form_bp" / "form_sart": the TOMO_FORM_* codes of include/tomo_hip.h).
//   all-angle forward projection   LIST   the sheared strips as wave-uniform entry lists (k_fp_list): slab = whole 128-slice pieces,
//                                         tables built (N >= 384 and >= 3000 strip workgroups, or TOMO_FP_LIST = 1), balance >= 0.8
//                                  STRIP  k_fp_strip: the same geometry rule where the slab is no multiple of 128 slices or the lists
//                                         could not be balanced
//                                  TILE   k_fp_tile + k_fp_tile_reduce: small images and thin slabs (the default there), user matrices
//                                         whose rays are no lines
//                                  ROWS   ray-driven k_fp_rows / k_fp_rows_g: "fp_tile" = 0 only
//   all-angle back projection      LIST   k_bp_list: whole 128-slice pieces, P <= 192;  TILE  k_bp_tile: other slabs, P <= FB_MAX_PROJ;
//                                  ALL    voxel-driven k_bp_all: the fallback
//   SART sweep (select_sart)       RESIDENT  k_sart_resident: N a multiple of 8, one 32 x 32 tile per CU, ray windows fit (resident.cpp);
//                                            after a launch that could not finish it sits out some sweeps, which run as TILE
//                                  TILE      k_sart_tile chain + k_resid_finish: N = 1024, fallbacks, "sart_resident" = 0
//                                  SEG       ray-walk k_sart_seg + k_resid_finish, the volume in a ping-pong pair: no tile tables or
//                                            "sart_tile" = 0 (reported as ANGLE: the public codes name three families)
//                                  ANGLE     one FP + one BP launch per angle: "sart_fused" = 0
enum SartForm { SART_ANGLE, SART_SEG, SART_TILE, SART_RESIDENT };
// form: what the next sweep runs;  sits_out: ... TILE in place of RESIDENT, and that sweep uses up one of the sit-outs (rs.skip);
// no_tables: "sart_resident" = 1 insists on tables this engine does not have: the sweep is an error, raised before any launch
struct SartChoice { SartForm form; bool sits_out, no_tables; };
static SartChoice select_sart(const tomo_engine *e)
{
    if (!e->sart_fused) return {SART_ANGLE, false, false};
    if (e->sart_resident != 0 && e->rs_ok) {          // (the resident tables exist only where the tile tables do)
        const bool sits_out = e->rs.skip > 0 && e->sart_resident != 1;
        return {sits_out ? SART_TILE : SART_RESIDENT, sits_out, false};
    }
    return {(e->sart_tile && e->st_ok) ? SART_TILE : SART_SEG, false, e->sart_resident == 1};
}

struct Forms { int fp, bp, sart; };
static Forms select_forms(const tomo_engine *e)
{
    Forms f;
    const SartChoice s = select_sart(e);
    f.fp = (e->fp_strip && e->fp_list && e->fl_ok && e->sxc % 128 == 0) ? TOMO_FORM_FP_LIST
         : (e->fp_strip && e->fs_ok) ? TOMO_FORM_FP_STRIP
         : e->fp_tile ? TOMO_FORM_FP_TILE : TOMO_FORM_FP_ROWS;
    f.bp = (e->bp_tile && e->bl_ok && e->bp_list && e->sxc % 128 == 0) ? TOMO_FORM_BP_LIST
         : (e->bp_tile && e->fb_ok) ? TOMO_FORM_BP_TILE : TOMO_FORM_BP_ALL;
    f.sart = (s.form == SART_RESIDENT || s.sits_out) ? TOMO_FORM_SART_RESIDENT      // (the family the engine is set to, sitting out or not)
           : s.form == SART_TILE ? TOMO_FORM_SART_TILE : TOMO_FORM_SART_ANGLE;
    return f;
}

// all-angle FP in the form select_forms names
template <int MODE>
static int launch_fp_all(tomo_engine *e, const Lane &ln, const float *x, const float *b, float *out, const float *rowfac = nullptr)
{
    if (!rowfac) rowfac = e->d_rowsum;
    switch (select_forms(e).fp) {
    case TOMO_FORM_FP_LIST: return launch_fp_list<MODE>(e, ln, x, b, out, rowfac);
    case TOMO_FORM_FP_STRIP: return launch_fp_strip<MODE>(e, ln, x, b, out, rowfac);
    case TOMO_FORM_FP_TILE: return launch_fp_tile<MODE>(e, ln, x, b, out, rowfac);
    default: return launch_fp<MODE>(e, ln, x, 0, (int)e->nrows, b, out, e->fp_all_lpr, rowfac);
    }
}
template <int MODE>
static int launch_fp_all(tomo_engine *e, const float *x, const float *b, float *out, const float *rowfac = nullptr)
{
    return launch_fp_all<MODE>(e, main_lane(e), x, b, out, rowfac);
}

// residual rows from a projection already in G (fp_reuse)
template <int MODE>
static int launch_sino_resid(tomo_engine *e, const float *b, const float *g, float *out)
{
    const int64_t n4 = (int64_t)e->sino_elems() / 4;
    hipLaunchKernelGGL((k_sino_resid<MODE>), dim3(grid_1d(n4)), dim3(256), 0, e->stream, b, g, e->d_rowsum, out, n4, e->sx / 4);
    LAUNCHCHK();
    return TOMO_OK;
}

// A slab larger than the Infinity Cache is streamed (non-temporal tile accesses); a smaller one stays cached between the
// launches of consecutive angles and keeps plain accesses (see st_xload / st_xstore).  "sart_nt": 0 never, 1 always, -1 by size.
static bool slab_streams(const tomo_engine *e)
{
    if (e->sart_nt >= 0) return e->sart_nt != 0;
    return (size_t)e->npix * e->sx * sizeof(float) >= ((size_t)192 << 20);
}

constexpr int BP_PPW = 4;

// the SART update of angle `angle` from its rows of the residual sinogram r (k_bp_angle)
static int launch_bp_angle(tomo_engine *e, const Sub &sb, float *x, int angle, const float *r, float beta, float *track = nullptr)
{
    ProfScope ps(e, TOMO_K_BP_ANGLE, sb.stream);
    const int vec = sub_vec(e, sb);              // (a sub-slab is whole multiples of 64*vec slices)
    const Chunks ch = chunks64(e, sb);
    const int nchunk = ch.n / vec, ngroups = (int)((e->npix + BP_PPW - 1) / BP_PPW);
    dim3 grid((unsigned)(((int64_t)ngroups * nchunk + 3) / 4)), block(256);
    double *part = track ? e->d_part : nullptr;  // tracked: the caller brackets with reduce_begin / reduce_end
    with_vec(vec, [&](auto V) { with_flag(track != nullptr, [&](auto T) {
        hipLaunchKernelGGL((k_bp_angle<V(), BP_PPW, T()>), grid, block, 0, sb.stream, x, e->d_cell + (size_t)angle * e->npix, r + (size_t)angle * e->n * e->sx, beta, (int)e->npix, e->sx,
                           ngroups, nchunk, track, part, ch.c0 / vec);
    }); });
    LAUNCHCHK();
    return TOMO_OK;
}

static int launch_bp_all(tomo_engine *e, float *x, const float *r, const float *colsum, float alpha, float beta, int clamp)
{
    const int form = select_forms(e).bp;
    if (form == TOMO_FORM_BP_LIST) {     // entry lists: whole pairs of 64-slice chunks
        if (!e->attr_bp2) {
            HIPCHK(hipFuncSetAttribute((const void *)k_bp_list, hipFuncAttributeMaxDynamicSharedMemorySize, BL_LDS_BYTES));
            e->attr_bp2 = true;
        }
        const int nchunk2 = e->sxc / 128;
        ProfScope ps(e, TOMO_K_BP_TILE);
        dim3 grid((unsigned)(8 * ((e->bl_ntiles + 7) / 8) * nchunk2)), block(BL_THREADS);
        hipLaunchKernelGGL(k_bp_list, grid, block, BL_LDS_BYTES, e->stream, x, e->d_bl_ent, e->d_bl_ptr, e->d_bl_win, r, colsum, alpha, beta, clamp,
                           e->np, e->n, e->sx, e->bl_tiles_z, e->bl_ntiles, nchunk2, e->bp_list_band);
        LAUNCHCHK();
        return TOMO_OK;
    }
    if (form == TOMO_FORM_BP_TILE) {
        if (!e->attr_bp) {
            HIPCHK(hipFuncSetAttribute((const void *)k_bp_tile, hipFuncAttributeMaxDynamicSharedMemorySize, FB_LDS_BYTES + FB_MAX_PROJ * 4));
            e->attr_bp = true;
        }
        const int nchunk64 = e->sxc / 64;
        ProfScope ps(e, TOMO_K_BP_TILE);
        dim3 grid((unsigned)(8 * ((e->ft_ntiles + 7) / 8) * nchunk64)), block(FT_THREADS);
        hipLaunchKernelGGL(k_bp_tile, grid, block, FB_LDS_BYTES + e->np * 4, e->stream, x, e->d_fb_cell, e->d_fb_win, r, colsum, alpha, beta, clamp,
                           e->np, e->n, e->sx, e->ft_tiles_z, e->ft_ntiles, nchunk64);
        LAUNCHCHK();
        return TOMO_OK;
    }
    int nchunk = e->sxc / (64 * e->vec);
    int ngroups = (int)((e->npix + BP_PPW - 1) / BP_PPW);
    int64_t waves = (int64_t)ngroups * nchunk;
    dim3 grid((unsigned)((waves + 3) / 4)), block(256);
    with_vec(e->vec, [&](auto V) {
        hipLaunchKernelGGL((k_bp_all<V(), BP_PPW>), grid, block, 0, e->stream, x, e->d_cell, r, colsum, alpha, beta, clamp, e->np, e->n, (int)e->npix, e->sx, ngroups, nchunk);
    });
    LAUNCHCHK();
    return TOMO_OK;
}

// ---- data in / out of device buffers of the caller (tomo_set_*_device / tomo_get_*_device, engine_api.inc) -----------------------
// ext must be plain device memory of the engine's device, `bytes` long from ext on: asked of the runtime before anything is enqueued
static int check_device_buffer(tomo_engine *e, const void *ext, size_t bytes)
{
    if (!ext) return fail(TOMO_ERR_ARG, "null device pointer");
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, ext) != hipSuccess) {
        (void)hipGetLastError();
        return fail(TOMO_ERR_ARG, "the pointer is not known to the HIP runtime (pageable host memory?)");
    }
    if (at.type != hipMemoryTypeDevice) return fail(TOMO_ERR_ARG, "the pointer is not plain device memory (pinned, managed or unregistered host memory)");
    if (at.device != e->device) return fail(TOMO_ERR_ARG, "the buffer lives on device " + std::to_string(at.device) + ", the engine on device " + std::to_string(e->device));
    hipDeviceptr_t base = nullptr; size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, const_cast<void *>(ext)) != hipSuccess) { (void)hipGetLastError(); return TOMO_OK; }   // (no range known: the type check stands alone)
    if ((const char *)ext + bytes > (const char *)base + size) return fail(TOMO_ERR_ARG, "the buffer's allocation ends before nelems elements");
    return TOMO_OK;
}

// Both streams are ordered both ways around the kernel, by events on the device: the engine's stream starts behind what the caller's
// stream did to the buffer (produced it; filled or freed what a get overwrites), the caller's stream continues behind the kernel (consumes a
// get; may overwrite or free what a set read).  The same stream on both sides needs neither.
static int io_fence(tomo_engine *e, hipStream_t from, hipStream_t to)
{
    if (from == to) return TOMO_OK;
    if (!e->ev_io) HIPCHK(hipEventCreateWithFlags(&e->ev_io, hipEventDisableTiming));
    HIPCHK(hipEventRecord(e->ev_io, from));
    HIPCHK(hipStreamWaitEvent(to, e->ev_io, 0));
    return TOMO_OK;
}

static int io_args(tomo_engine *e, const void *ext, int dtype, int layout, int64_t nelems, int64_t m)
{
    if (dtype != TOMO_F32 && dtype != TOMO_F64) return fail(TOMO_ERR_ARG, "bad dtype (TOMO_F32 or TOMO_F64)");
    if (layout != TOMO_SINO_PACKED && layout != TOMO_SINO_PUBLIC) return fail(TOMO_ERR_ARG, "bad layout (TOMO_SINO_PACKED or TOMO_SINO_PUBLIC)");
    if (nelems != (int64_t)e->nx * m) return fail(TOMO_ERR_ARG, "nelems is " + std::to_string(nelems) + ", the slab has " + std::to_string((int64_t)e->nx * m) + " elements");
    if (m > 0x7FFFFFFF) return fail(TOMO_ERR_ARG, "more than 2^31 rows");
    return check_device_buffer(e, ext, (size_t)nelems * (dtype == TOMO_F64 ? sizeof(double) : sizeof(float)));
}

// the conversion kernel between ext ([nx][m], dtype, layout) and dev ([m][sx]) on the engine's stream, fenced against `caller`
template <bool IN>
static int io_launch(tomo_engine *e, void *ext, float *dev, int64_t m, int dtype, int layout, hipStream_t caller)
{
    int rc = io_fence(e, caller, e->stream);
    if (rc) return rc;
    const dim3 grid((unsigned)((m + IO_TJ - 1) / IO_TJ), (unsigned)(e->sx / IO_TS)), block(256);
    const size_t esz = dtype == TOMO_F64 ? sizeof(double) : sizeof(float);
    const bool vec = m % 4 == 0 && (uintptr_t)ext % (4 * esz) == 0;
    with_flag(dtype == TOMO_F64, [&](auto f64) { with_flag(layout == TOMO_SINO_PUBLIC, [&](auto pub) { with_flag(vec, [&](auto v) {
        using T = std::conditional_t<decltype(f64)::value, double, float>;
        if constexpr (IN) hipLaunchKernelGGL((k_io_in<T, decltype(pub)::value, decltype(v)::value>), grid, block, 0, e->stream, (const T *)ext, dev, e->nx, m, e->sx, e->np, e->n);
        else hipLaunchKernelGGL((k_io_out<T, decltype(pub)::value, decltype(v)::value>), grid, block, 0, e->stream, dev, (T *)ext, e->nx, m, e->sx, e->np, e->n);
    }); }); });
    LAUNCHCHK();
    return io_fence(e, e->stream, caller);
}
