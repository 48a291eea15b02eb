// tomo_engine.hip -- engine state + C ABI (include/tomo_hip.h) over the kernels in kernels.hip.h.
//
// Mirrors the method surface of the reference's `tomoengine` (tomofusion/gpu/utils/tomoengine.{hpp,cpp}) and
// `ctvlib` (tomofusion/cpu/utils/ctvlib.{hpp,cpp}); each entry point cites the lines it replaces in the header.
// Unlike the reference (host-resident volume, cudaMalloc + H2D + D2H inside every call) all fields stay
// resident in HBM for the life of the engine.
#include "../../include/tomo_hip.h"
#include "kernels.hip.h"
#include "sart_resident.hip.h"
#include "sysmat.h"
#include "resident.h"
#include "dev_pool.h"
#include "claims.h"
#include "sart_host.h"
#include "tv_form.h"

#include <dlfcn.h>
#if __has_include(<rccl/rccl.h>)
#include <rccl/rccl.h>
#else
// A ROCm install without the RCCL development headers still builds the engine: librccl is only ever opened with dlopen
// (rccl_load), so the handful of opaque types and constants of its C API that the tomo_comm_* entries use are restated here
// (nccl.h: ncclUniqueId is 128 opaque bytes; ncclFloat32 = 7, ncclFloat64 = 8, ncclSum = 0, ncclSuccess = 0).
#define NCCL_UNIQUE_ID_BYTES 128
typedef struct ncclComm *ncclComm_t;
typedef struct { char internal[NCCL_UNIQUE_ID_BYTES]; } ncclUniqueId;
typedef enum { ncclSuccess = 0 } ncclResult_t;
typedef enum { ncclFloat32 = 7, ncclFloat64 = 8 } ncclDataType_t;
typedef enum { ncclSum = 0 } ncclRedOp_t;
#endif

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <functional>
#include <memory>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <thread>
#include <string>
#include <vector>

using namespace tomo;

static thread_local std::string g_err;
static int fail(int code, const std::string &msg) { g_err = msg; return code; }

#define HIPCHK(call)                                                                                      \
    do {                                                                                                  \
        hipError_t _e = (call);                                                                           \
        if (_e != hipSuccess)                                                                             \
            return fail(TOMO_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(_e));                 \
    } while (0)
#define LAUNCHCHK() HIPCHK(hipGetLastError())
#define NEED(e) do { if (!(e)) return fail(TOMO_ERR_ARG, "null engine"); if ((e)->geometry_released) return fail(TOMO_ERR_STATE, "engine geometry was released"); HIPCHK(hipSetDevice((e)->device)); } while (0)
enum { PROF_MAX_KERNELS = 12, PROF_MAX_EVENTS = 1 << 19 };   // 262144 launches per kernel id between two reads

struct ProfSlot {
    bool on = false;
    unsigned stride = 1, seen = 0;   // every stride-th launch is bracketed (an event pair costs ~3 us of command-processor time)
    std::vector<hipEvent_t> ev;  // pairs
    hipEvent_t ref = nullptr;    // recorded when the log is switched on: launches on different streams share this time base
    size_t used = 0, dropped = 0;   // dropped: launches that could not be recorded (tomo_profile_read reports them)
};

// A persistent host thread that enqueues the launch chain of one sub-slab (run_chains).  Round 2 started and joined a std::thread
// per sweep (50-100 us of host time on the path of a 4 ms step of a 64-slice slab); this one is started once per
// engine and sleeps on a condition variable between sweeps.
struct ChainHelper {
    std::thread th;
    std::mutex mu;
    std::condition_variable cv;
    std::function<void()> job;
    bool has_job = false, done = true, stop = false;
    void start(int device)
    {
        th = std::thread([this, device]() {
            (void)hipSetDevice(device);
            std::unique_lock<std::mutex> lk(mu);
            for (;;) {
                cv.wait(lk, [this] { return has_job || stop; });
                if (stop) return;
                has_job = false;
                lk.unlock();
                job();
                lk.lock();
                done = true;
                cv.notify_all();
            }
        });
    }
    void submit(std::function<void()> f)
    {
        std::lock_guard<std::mutex> lk(mu);
        job = std::move(f);
        has_job = true;
        done = false;
        cv.notify_all();
    }
    void wait()
    {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [this] { return done; });
    }
    ~ChainHelper()
    {
        if (th.joinable()) {
            { std::lock_guard<std::mutex> lk(mu); stop = true; }
            cv.notify_all();
            th.join();
        }
    }
};

// the allocator of every engine's DevPool: the only raw device allocation and release of the engine
static int pool_alloc(void **p, size_t bytes) { HIPCHK(hipMalloc(p, bytes)); return TOMO_OK; }
static void pool_free(void *p) { (void)hipFree(p); }

// One partial-sum family of the all-angle forward projector (k_fp_tile / k_fp_strip / k_fp_list): the main kernel writes nseg
// partial row sums per 64-slice chunk into the scratch of the lane it runs on, k_fp_tile_reduce gathers them through the row
// lists rsptr / rsidx.  ncp chunks go into one pass (planned on first use, plan_ncp; 0 = not planned yet) and size the scratch.
struct FpFamily {
    uint32_t nseg = 0;
    int ncp = 0;
    bool pairs = false;                           // works on whole pairs of chunks (128-slice pieces)
    float *part[2] = {nullptr, nullptr};          // scratch, [lane]: allocated when that lane first projects
    uint32_t *d_rsptr = nullptr, *d_rsidx = nullptr;
};

struct CommRef;
struct tomo_engine;
static void comm_release(tomo_engine *e);
struct tomo_engine {
    int nx = 0, n = 0, np = 0, sx = 0, sxc = 0, vec = 1, device = 0;   // sx = row pitch, sxc = computed width
    int64_t npix = 0, nrows = 0, nnz = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    // tables
    uint32_t *d_rptr = nullptr;
    uint2 *d_rent = nullptr;
    float *d_rowsum = nullptr, *d_rowinner = nullptr, *d_colsum_all = nullptr, *d_rowcross = nullptr;
    bool art_chain_ok = false;
    int art_chain = 1;                            // natural-order ART: per-angle FP + ray recurrence + BP instead of row steps
    CellD *d_cell = nullptr;
    uint32_t *d_wptr = nullptr;                   // walk lists of the fused SART step
    uint2 *d_went = nullptr;
    float lipschitz = 0.f, lipschitz_cimmino = 0.f;
    int sart_fused = 1;                      // 1: SART sweep as a chain of fused BP+FP steps; 0: separate FP and BP per angle
    int fp_all_lpr = 16;
    // The six "tv_*" switches, read by select_tv / tv_folds_halo (tv_form.h) and the option calls only.
    // recompute: a tv_gd inner iteration as "norm pass (no store) + recompute-and-update pass into a second buffer" instead
    // of "gradient pass (store g) + update pass": one volume write instead of two (HBM writes are the scarce resource)
    // tz: z-columns per wave of the register march (8 or 4); yseg: its rows per wave, 0 = by slab size (tv_rows_per_wave);
    // march4: norm / update passes by k_tv_march4 (no row rotation) instead of k_tv_grad_reg
    // halo_fold (slab-sharded descent): the update pass advances the halo planes itself (lanes 1..8 of the packed edge registers: one 32-byte load of
    // the received gradient plane and one store per row and plane) instead of a k_halo_apply launch per inner iteration.  -1 = automatic:
    // where the slab has two chunks or more.  Measured (round 6, bench.py --force-dist, world-1 RCCL group): 128 slices 3.53 against 3.62 ms
    // per step; 64 slices (ONE chunk: every wave of the pass holds both planes) 2.04 against 2.01 -- so a one-chunk slab keeps the launch.
    // (The first form, one lane looping over the row's eight pixels: 2.165 against 2.012 at 64 slices.)  1 / 0 force it.
    TvOptions tv;
    int gnorm_slot = TOMO_S_GNORM;                // scalar slot the TV update takes ||g||^2 from (slab groups: TOMO_S_GNORM_ALL)
    hipEvent_t ev_peer = nullptr;                 // tomo_wait_for: "everything enqueued on this engine so far"
    hipEvent_t ev_io = nullptr;                   // tomo_set_*_device / tomo_get_*_device: orders the caller's stream and the engine's
    float tv_last_eps = 1e-6f;                    // step form: eps of the last tomo_tv_grad*, which the tomo_tv_update* that follows passes on
    float *tv_alt = nullptr, *halo_lo_alt = nullptr, *halo_hi_alt = nullptr;
    // fp_all_lpr: all-angle FP: lanes per ray of the narrow-chunk form (0 = wide form)
    SegItemD *d_seg_exec = nullptr;
    std::vector<uint32_t> h_seg_exec_ptr;
    uint32_t *d_row_first = nullptr, *d_row_nseg = nullptr;
    float *seg_partial = nullptr;
    uint32_t max_items = 0;
    bool seg_ready = false;                       // the walk / segment tables above are on the device (built at creation or on first use)
    std::vector<double> angles;                   // the tilt angles of an engine created from angles (tomo_create): tables built on first use come from them
    float *sart_alt = nullptr;                    // ping-pong partner of the volume being swept
    // tile-stationary all-angle FP (k_fp_tile): its family record and tables; k_bp_tile walks the same tile grid (ft_tiles_z, ft_ntiles)
    int fp_tile = 1, ft_tiles_z = 0, ft_ntiles = 0;
    FpFamily ft;
    uint32_t *d_ft_slot_ptr = nullptr, *d_ft_slot_seg0 = nullptr;
    uint2 *d_ft_tent = nullptr;
    // sheared-strip all-angle FP (k_fp_strip, round 4): ray sums resident in registers, ~5 partial sums per ray instead of ~27
    int fp_strip = 1, fs_nitems = 0, fs_kused = 0;
    bool fs_ok = false;
    FpFamily fs;
    FsItemD *d_fs_items = nullptr;
    int *d_fs_orient = nullptr, *d_fs_shift = nullptr;
    uint4 *d_fs_cnt = nullptr;
    uint32_t *d_fs_gstart = nullptr, *d_fs_gseg0 = nullptr;
    uint2 *d_fs_ent = nullptr;
    float *d_fs_zero = nullptr;                   // 256 bytes of zeros: what a strip tile's pixels outside the image are staged from
    // ... and as wave-uniform entry lists (k_fp_list) when the slab is a whole number of 128-slice pieces
    int fp_list = 1, fl_nitems = 0;
    bool fl_ok = false, attr_fl = false;
    FpFamily fl;
    FlItemD *d_fl_items = nullptr;
    int *d_fl_orient = nullptr, *d_fl_shift = nullptr;
    uint2 *d_fl_ent = nullptr, *d_fl_fent = nullptr;
    uint32_t *d_fl_ptr = nullptr, *d_fl_fptr = nullptr;
    float *d_fl_zero = nullptr;
    bool attr_fp = false, attr_bp = false, attr_st = false;   // dynamic-LDS limits raised on this engine's device
    int sart_streams = 0;                        // chains a SART / ART sweep runs as: 0 = automatic, 1 = one, 2..4 = that many (chain_count, run_chains)
    static constexpr int MAX_CHAINS = 4;
    hipStream_t sub_stream[MAX_CHAINS] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t ev_sfork = nullptr, ev_sjoin[MAX_CHAINS] = {nullptr, nullptr, nullptr, nullptr};
    std::unique_ptr<ChainHelper> chain_helper[MAX_CHAINS];   // [u]: the thread that enqueues chain u (u >= 1), started on first use
    int sart_tile = 1;                            // fused SART step on streamed image tiles (k_sart_tile) when the geometry allows it
    bool st_ok = false;
    int st_ntiles = 0, st_tiles_z = 0;
    uint32_t st_max_ids = 0;
    uint4 *d_st_cell = nullptr;
    uint32_t *d_st_win = nullptr, *d_st_segid = nullptr, *d_st_row_first = nullptr, *d_st_row_nseg = nullptr;
    uint2 *d_st_seg = nullptr, *d_st_ent = nullptr;
    float *st_partial = nullptr, *st_partial2 = nullptr;   // tile partial sums; the second buffer of the cooperative chain (links alternate)
    uint32_t *st_flags = nullptr;                          // [ray of an angle][64-slice chunk]: epoch of the launch that published the residual row
    uint32_t st_epoch = 0;
    // "sart_coop" = 1: residual rows inside the tile step (k_sart_tile COOP) instead of one k_resid_finish launch per angle.
    // Off by default -- measured (round 2, 512^2 x 90): the step kernel grows by what the dropped launch and its two
    // boundaries cost (221 vs 210 us at 512 slices: 27.3 ms per ASD-POCS step either way) and by more on thin slabs
    // (64 slices: 37.0 vs 30.8 us, 5.25 vs 4.87 ms per step): the first workgroups cannot start their voxel update before
    // the rows exist, so the reduction is serial either way and only moves inside the launch.
    int sart_coop = 0, sart_coop_spin = 4096, st_resident = 0;
    // "sart_resident" (round 5): the sweep as ONE launch of k_sart_resident -- a 64-slice chunk of the whole image stays in the chip's
    // vector registers over all angles of the sweep and the workgroups exchange only ray sums (sart_resident.hip.h).  -1 = automatic
    // (whenever the tables exist: N a multiple of 8 with at most one 32 x 32 tile per CU, a matrix whose ray windows fit), 0 = never
    // (the streamed tile steps), 1 = insist (an error where the tables do not exist).
    int sart_resident = -1;
    bool rs_ok = false;
    int rs_ntiles = 0, rs_tiles = 0, rs_rpt = 0, rs_groups = 0, rs_cus = 0;
    RsHdrD *d_rs_hdr = nullptr;
    uint4 *d_rs_cell = nullptr;
    uint2 *d_rs_ts = nullptr;
    uint16_t *d_rs_rl = nullptr;
    rs_u64 *rs_pb = nullptr, *rs_rb = nullptr;     // granules {value, tag}: tile sums, residual rows
    size_t rs_pb_bytes = 0, rs_rb_bytes = 0;
    int *d_rs_angs = nullptr; size_t rs_angs_cap = 0;   // angle of every step of the sweep in flight, and the steps it has room for
    std::vector<int> rs_angs_host;                 // (what d_rs_angs holds: an unchanged sequence is not uploaded again)
    int *rs_abort = nullptr, *d_rs_abort = nullptr; // pinned host word / device word a workgroup sets when a bounded spin gave up
    // fail-safe (round 6): a chunk is stored by all of its workgroups or by none (rs_commit); d_rs_commit = the chunks' commit words,
    // rs_done = pinned [chunk]: the sequence number of the launch that stored it.  Chunks that did not commit are swept by the streamed
    // chain, and the resident form then sits out rs.skip sweeps (doubling up to 64 while the failures go on; "sart_resident" = 1 insists)
    unsigned *d_rs_commit = nullptr;
    int *rs_done = nullptr;
    RsLedger rs;                                   // the launches' counters: tags, commit base, sequence number, sit-out (sart_host.h)
    int rs_test_fail = 0;                          // tests: chunk + 1 that refuses to commit
    uint32_t rs_spin_limit = 1u << 21;             // polls before a wait of the resident kernel gives up
    size_t table_bytes = 0;                        // device bytes of the tables built at creation (everything but volumes, sinograms, halos)
    double create_ms = 0.0;                        // wall clock of the creation (matrix, tables, uploads)
    int art_tile = 1;                              // chained ART sweep as fused tile steps (k_sart_tile ART) instead of k_fp_rows + k_bp_art per angle
    int sart_skip_same = 1;                        // k_sart_tile stores only the 256-byte pieces whose bits changed (in place)
    int sart_nt = -1;                              // tile accesses: -1 streaming form by slab size (slab_streams), 0 plain, 1 streaming
    int bp_tile = 1;                              // tile-stationary all-angle BP (k_bp_tile) when the geometry allows it
    int bp_list = 1;                              // ... in its entry-list form (k_bp_list) when the slab is whole pairs of 64-slice chunks
    bool attr_bp2 = false, bl_ok = false;
    int bp_list_band = 0;                         // k_bp_list: 1 = an XCD owns a contiguous band of tiles (see the kernel)
    uint4 *d_bl_ent = nullptr;                    // k_bp_list: entry batches and the first batch of every (tile, stage, wave) list
    uint32_t *d_bl_ptr = nullptr, *d_bl_win = nullptr;
    int bl_tiles_z = 0, bl_ntiles = 0;
    bool fb_ok = false;
    uint4 *d_fb_cell = nullptr;
    uint32_t *d_fb_win = nullptr;
    int ft_ncp_forced = 0;                        // chunks per pass of every FP family, forced (tests); 0 = what ft_scratch_cap holds
    size_t ft_scratch_cap = (size_t)8 << 30;      // >= 4 chunks per pass up to 1024^2 x 120 (one pass measured 12 % faster than one chunk per pass)
    // fields
    float *vol[TOMO_VOL_SLOTS] = {};
    float *sino[TOMO_SINO_SLOTS] = {};
    int fgp_target = TOMO_VOL_RECON;
    int tv_target = TOMO_VOL_RECON;               // volume the tv_gd / tv_grad / tv_update forms act on (tomo_tv_set_target)
    float *cg_p = nullptr, *cg_z = nullptr, *cg_w = nullptr, *fbp_h = nullptr;   // CGLS direction / A^T r / A p; WBP kernel
    double *cg_sums = nullptr;                    // 2*sx per-slice sums
    double *cg_part = nullptr;                    // 1024 x sx: the workgroups' partial sums of a per-slice reduction
    float *cg_coef = nullptr;                     // sx per-slice coefficients
    float *tvg = nullptr;                         // TV gradient tensor; doubles as FGP "D"
    float *fgp_p[3] = {nullptr, nullptr, nullptr};
    float *fgp_q[3] = {nullptr, nullptr, nullptr};   // ping-pong partners for the fused FGP iteration
    int fgp_fused = 1;
    int fgp_pair = 1;                             // ... two iterations per pass (k_fgp_fused2) where the slab is not sharded
    // Chambolle-Pock (engine_pdhg.inc): the dual field and dual sinogram of the whole-call form, and the second buffers of the
    // fused pass (xbar, p0..p2), which change places with the buffers of the fields it wrote
    float *pdhg_p[3] = {nullptr, nullptr, nullptr}, *pdhg_alt[4] = {nullptr, nullptr, nullptr, nullptr}, *pdhg_q = nullptr;
    bool pdhg_begun = false;
    // planes of the slab-sharded fused pass (caller-owned device buffers, tomo_bind_pdhg_halo): lo 4, hi 1, send_first 1, send_last 4
    float *pdhg_lo = nullptr, *pdhg_hi = nullptr, *pdhg_send_first = nullptr, *pdhg_send_last = nullptr;
    float *stage = nullptr;
    size_t stage_bytes = 0;
    // alignment (engine_align.inc): the workgroups' partial sums, per-angle moments [2][np][3] and means [2][np], the window read back
    double *al_part = nullptr, *al_mom = nullptr, *al_out = nullptr;
    float *al_mean = nullptr;
    size_t al_part_bytes = 0, al_out_bytes = 0;
    std::vector<float> cond_tab;                  // conditioning (engine_condition.inc): the host copy of the last {gain, offset} table enqueued
    // marker detection (engine_markers.inc): the host copy of the last normalised template enqueued; the peak counters and records on
    // the device (kept, grown on demand) and the host block the records are sorted in
    std::vector<float> mk_tmpl;
    void *mk_buf = nullptr;
    size_t mk_bytes = 0;
    std::vector<int> mk_host;
    // DART (engine_dart.inc): one state byte per voxel, the number of thresholds it was made with (-1: no segmentation yet), and the
    // class statistics' partial sums [DART_STATS_BLOCKS + 1][16][2] (the last row: the result)
    uint8_t *dart_state = nullptr;
    int dart_nthr = -1;
    double *dart_part = nullptr;
    // connected components (engine_components.inc): one int32 label per real voxel in the public order, the root counts of every 256
    // voxels (then their prefix sums and K), the K records and the room they have, K itself (-1: no labelling), whether the records
    // hold the measurements of this labelling yet, and the host copy of the last keep table enqueued
    int *cc_label = nullptr, *cc_counts = nullptr;
    CcRecord *cc_rec = nullptr;
    size_t cc_rec_cap = 0;
    int64_t cc_count = -1;
    bool cc_stats_done = false;
    std::vector<uint8_t> cc_keep;
    // registration (engine_register3d.inc): the workgroups' partial sums of the normal equations [RG_BLOCKS + 1][32] (the last row: the result)
    double *reg_part = nullptr;
    // scalars
    double *d_scal = nullptr, *d_scal_own = nullptr, *d_part = nullptr, *d_part_aux = nullptr, *d_part_tv = nullptr;
    double *h_snap = nullptr;          // pinned: tomo_scalars_snapshot
    hipEvent_t ev_snap = nullptr;
    bool snap_pending = false;
    bool part_open[3] = {false, false, false};   // [Lane::idx]: a reduction into that lane's partial sums is in flight (see reduce_begin)
    hipStream_t aux = nullptr;                    // second stream for work that is independent of the main sequence
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    bool async_pending = false;
    struct CommRef *comm = nullptr;               // native RCCL communicator (tomo_comm_init / tomo_comm_share); see the comm section
    int64_t comm_rounds = 0;                      // RCCL rounds (one ncclGroup or one lone collective) this engine has enqueued: bench.py's rccl_rounds_per_step
    float *comm_send_first = nullptr, *comm_send_last = nullptr, *comm_g_lo = nullptr, *comm_g_hi = nullptr;   // N*N planes
    float *comm_fgp = nullptr;                    // the engine's own planes of the fused FGP exchange when the host binds none
    float *comm_pdhg = nullptr;                   // ... and of the slab-sharded Chambolle-Pock pass (10 planes)
    double *comm_scal = nullptr;                  // TOMO_S_COUNT doubles: the all-reduced copy of the scalar buffer
    // which projections are in hand and whether RECON_OLD shares RECON's buffer: the write versions and every claim made on them (claims.h)
    Claims claims;
    // FISTA: the projection of the extrapolated point by linearity (tomo_fista_project_yk)
    float *g_prev = nullptr;                      // A * (the iterate before the last Nesterov step)
    float *g_yk = nullptr;                        // A * yk formed by linearity; G itself stays A * recon (tomoengine.cpp:410-427,459)
    bool geometry_released = false;               // tomo_release_geometry: only tomo_adopt_volumes / tomo_destroy remain valid
    // halos
    float *halo_lo = nullptr, *halo_hi = nullptr, *halo_lo_own = nullptr, *halo_hi_own = nullptr;
    // planes of the fused slab-sharded FGP iteration (caller-owned device buffers, tomo_bind_fgp_halo)
    float *fgp_lo = nullptr, *fgp_hi = nullptr, *fgp_send_first = nullptr, *fgp_send_last = nullptr;
    bool fgp_planes2 = false;                     // the bound planes are the two-slice-deep set (5 / 8 / 8 / 5 planes: tomo_bind_fgp_halo2)
    int is_first = 1, is_last = 1;
    ProfSlot prof[PROF_MAX_KERNELS];
    std::mutex prof_mu;
    size_t vol_elems() const { return (size_t)npix * sx; }
    size_t sino_elems() const { return (size_t)nrows * sx; }
    // every device allocation of the engine (dev_pool.h).  Caller-bound buffers and the aliases of owned ones (d_scal, halo_lo / halo_hi,
    // fgp_lo ..., pdhg_lo ...) are never registered.
    DevPool pool{pool_alloc, pool_free};
};

constexpr DevPool::Life GEOMETRY = DevPool::GEOMETRY, COMM = DevPool::COMM, ENGINE = DevPool::ENGINE;
// *p = a new device buffer of the engine, owned by its pool; zero: cleared on the engine's stream
static int dev_alloc(tomo_engine *e, DevPool::Life life, void **p, size_t bytes, bool zero)
{
    if (int rc = e->pool.alloc(life, p, bytes)) return rc;
    if (zero) HIPCHK(hipMemsetAsync(*p, 0, bytes ? bytes : 4, e->stream));
    return TOMO_OK;
}

// ---- a projection already in hand is not computed again -------------------------------------------------------------------
// The reference's drivers evaluate `data_distance()` after every SIRT / CGLS step (gpu/reconstructor.py:61-71, show_convergence
// defaults to True) and the next step starts by projecting the very same volume; multimodal::data_fusion projects the model
// volume for its cost and then starts a SIRT run from a copy of it (multimodal.cpp:452-470).  The engine remembers which volume
// (slot and write-version) the model sinogram G was projected from; a SIRT / CGLS call whose volume is still that one forms its
// first residual from G instead of projecting again -- the same kernels produced G, so the bits are the same ("fp_reuse" = 0
// switches it off).  The bookkeeping is the engine's Claims record (claims.h); the accessors below are where it meets the buffers.
static bool g_is_projection_of(const tomo_engine *e, int vol) { return e->claims.g_is_projection_of(vol, e->sino[TOMO_SINO_G] != nullptr); }

// the sinogram that holds A * (volume vol as it stands), or nullptr: G through its claim, or the extrapolated point's own buffer
static const float *projection_in_hand(const tomo_engine *e, int vol)
{
    const Claims::Source s = e->claims.projection_in_hand(vol, e->sino[TOMO_SINO_G] != nullptr, e->g_yk != nullptr);
    return s == Claims::FROM_G ? e->sino[TOMO_SINO_G] : s == Claims::FROM_G_YK ? e->g_yk : nullptr;
}

// After a Nesterov step recon_old == recon (tomoengine.cpp:381-384 copies the prox result into both).  The step keeps that as a
// FLAG instead of a second store (Claims::nesterov_step: the logical content of RECON_OLD is RECON's; its own buffer is stale), so the
// step reads two volumes and writes one.  Whoever may WRITE recon, or touches recon_old, goes through get_vol, which first makes
// the copy real; readers of recon use get_vol_ro and leave the flag alone.
static int get_vol_ro(tomo_engine *e, int id, float **out)
{
    if (id < 0 || id >= TOMO_VOL_SLOTS) return fail(TOMO_ERR_ARG, "bad volume id");
    id = e->claims.read_slot(id);
    if (!e->vol[id]) { int rc = dev_alloc(e, ENGINE, (void **)&e->vol[id], e->vol_elems() * sizeof(float), true); if (rc) return rc; }
    *out = e->vol[id];
    return TOMO_OK;
}

static int get_vol(tomo_engine *e, int id, float **out)
{
    if (id < 0 || id >= TOMO_VOL_SLOTS) return fail(TOMO_ERR_ARG, "bad volume id");
    if (e->claims.write(id)) {                          // RECON_OLD shared RECON's buffer until now: make the copy real
        float *src, *dst; int rc;
        if ((rc = get_vol_ro(e, TOMO_VOL_RECON, &src)) || (rc = get_vol_ro(e, TOMO_VOL_RECON_OLD, &dst))) return rc;
        HIPCHK(hipMemcpyAsync(dst, src, e->vol_elems() * sizeof(float), hipMemcpyDeviceToDevice, e->stream));
    }
    return get_vol_ro(e, id, out);
}

static int get_sino(tomo_engine *e, float **slot, float **out)
{
    if (slot == &e->sino[TOMO_SINO_G]) e->claims.g_touched();
    if (!*slot) { int rc = dev_alloc(e, GEOMETRY, (void **)slot, e->sino_elems() * sizeof(float), true); if (rc) return rc; }
    *out = *slot;
    return TOMO_OK;
}

static int sino_slot(tomo_engine *e, int id, float **out)
{
    if (id < 0 || id >= TOMO_SINO_SLOTS) return fail(TOMO_ERR_ARG, "bad sinogram id");
    return get_sino(e, &e->sino[id], out);
}

// a sinogram slot that is only read: allocated (zero) on first use like any slot, but asking for G does not drop its claim
static int sino_slot_ro(tomo_engine *e, int id, float **out)
{
    if (id < 0 || id >= TOMO_SINO_SLOTS) return fail(TOMO_ERR_ARG, "bad sinogram id");
    if (!e->sino[id]) { int rc = dev_alloc(e, GEOMETRY, (void **)&e->sino[id], e->sino_elems() * sizeof(float), true); if (rc) return rc; }
    *out = e->sino[id];
    return TOMO_OK;
}

static int get_scratch(tomo_engine *e, float **slot, float **out)
{
    if (!*slot) { int rc = dev_alloc(e, ENGINE, (void **)slot, e->vol_elems() * sizeof(float), true); if (rc) return rc; }
    *out = *slot;
    return TOMO_OK;
}

// A write to a volume or to the re-projection G on the main stream must not overtake an evaluation still reading them
// on the second stream (tomo_data_distance_sq_async): order the main stream behind it.  No-op when nothing is pending.
static int order_after_async(tomo_engine *e)
{
    if (e->async_pending) HIPCHK(hipStreamWaitEvent(e->stream, e->ev_join, 0));
    return TOMO_OK;
}

static int ensure_stage(tomo_engine *e, size_t bytes)
{
    if (e->stage_bytes >= bytes) return TOMO_OK;
    if (e->stage) { HIPCHK(hipStreamSynchronize(e->stream)); e->pool.release(e->stage); e->stage_bytes = 0; }
    if (int rc = dev_alloc(e, ENGINE, (void **)&e->stage, bytes, false)) return rc;
    e->stage_bytes = bytes;
    return TOMO_OK;
}

// ---- profiling brackets (bench.py roofline: HIP events on the launch stream) --------------------------
// Where a launch goes: the engine's stream and the whole slab, or one sub-slab (64-slice chunks [c0, c0 + nc)) on its own
// stream.  Passed explicitly so that two host threads can enqueue the two sub-slab chains of a SART sweep side by side.
struct Sub {
    hipStream_t stream; int c0 = 0, nc = 0;
    int vec = 0;       // vector width of the per-row kernels on this sub-slab (0: the engine's); divides c0 and nc
};
static int sub_vec(const tomo_engine *e, const Sub &sb) { return sb.nc && sb.vec ? sb.vec : e->vec; }
static Sub whole(const tomo_engine *e) { return Sub{e->stream}; }

// Where a projection or a reduction of the whole slab runs: the stream, the partial sums its scalar is gathered in, and the index that
// picks the lane's FP scratch (FpFamily::part) and its open flag (part_open).  Passed explicitly: the main sequence and the evaluation
// on the second stream (tomo_data_distance_sq_async) go through the same launchers side by side.  The TV sum is a second reduction
// of the main stream that is open at the same time as the main one: a lane of its own that never projects.
struct Lane { hipStream_t stream; double *part; int idx; };
static Lane main_lane(const tomo_engine *e) { return Lane{e->stream, e->d_part, 0}; }
static Lane aux_lane(const tomo_engine *e) { return Lane{e->aux, e->d_part_aux, 1}; }
static Lane tv_lane(const tomo_engine *e) { return Lane{e->stream, e->d_part_tv, 2}; }

struct ProfScope {
    tomo_engine *e; int k; hipEvent_t stop = nullptr; hipStream_t st;
    // key >= 0: the launch's position in its chain (the two sub-slab chains of a SART sweep then bracket the SAME links, so
    // that the overlap of sibling launches can be seen); key < 0: every stride-th launch in arrival order
    ProfScope(tomo_engine *e_, int k_, hipStream_t st_ = nullptr, int64_t key = -1) : e(e_), k(k_), st(st_ ? st_ : e_->stream)
    {
        ProfSlot &p = e->prof[k];
        if (!p.on) return;
        hipEvent_t start;
        {
            std::lock_guard<std::mutex> lk(e->prof_mu);       // two threads may log launches of one kernel
            if (p.stride > 1 && ((key >= 0 ? (uint64_t)key : (uint64_t)p.seen++) % p.stride) != 0) return;
            if (p.used + 2 > p.ev.size()) {
                if (p.ev.size() >= PROF_MAX_EVENTS) { ++p.dropped; return; }
                hipEvent_t a, b;
                if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) { ++p.dropped; return; }
                p.ev.push_back(a); p.ev.push_back(b);
            }
            start = p.ev[p.used];
            stop = p.ev[p.used + 1];
            p.used += 2;
        }
        (void)hipEventRecord(start, st);
    }
    ~ProfScope() { if (stop) (void)hipEventRecord(stop, st); }
};

// ---- reductions ------------------------------------------------------------------------------------------
// The partial-sum buffers are zero between reductions: they are allocated zeroed and k_finalize clears what it has read,
// so a reduction costs no memset launch.  Only a reduction that was abandoned half-way (an error return between begin
// and end) leaves its buffer marked open, and the next begin clears it.
static int reduce_begin(tomo_engine *e, const Lane &ln)
{
    bool &open = e->part_open[ln.idx];
    if (open) HIPCHK(hipMemsetAsync(ln.part, 0, NPART * sizeof(double), ln.stream));
    open = true;
    return TOMO_OK;
}
static int reduce_end(tomo_engine *e, const Lane &ln, int slot)
{
    hipLaunchKernelGGL(k_finalize, dim3(1), dim3(NPART), 0, ln.stream, ln.part, e->d_scal + slot);
    LAUNCHCHK();
    e->part_open[ln.idx] = false;
    return TOMO_OK;
}
static int reduce_begin(tomo_engine *e) { return reduce_begin(e, main_lane(e)); }
static int reduce_end(tomo_engine *e, int slot) { return reduce_end(e, main_lane(e), slot); }

static int grid_1d(int64_t n4) { int64_t b = (n4 + 255) / 256; return (int)std::min<int64_t>(std::max<int64_t>(b, 1), 4096); }

#include "engine_launch.inc"
#include "engine_create.inc"
#include "engine_sart.inc"

extern "C" {

#include "engine_api.inc"
#include "engine_tv.inc"
#include "engine_fgp.inc"
#include "engine_pdhg.inc"
#include "engine_align.inc"
#include "engine_tilt.inc"
#include "engine_condition.inc"
#include "engine_markers.inc"
#include "engine_bin.inc"
#include "engine_dual.inc"
#include "engine_affine3d.inc"
#include "engine_register3d.inc"
#include "engine_dart.inc"
#include "engine_components.inc"
#include "engine_comm.inc"
#include "engine_options.inc"

}  // extern "C"
