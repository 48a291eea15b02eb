/*
 * tomo_hip.h -- C ABI of libtomo_hip.so, the MI355X (gfx950) engine for the hot path of
 * jtschwar/tomo_TV: parallel-beam forward projection, voxel-driven back-projection, SIRT/SART
 * updates and the 3-D TV kernels, behind the reference's `tomoengine` / `ctvlib` method surface.
 *
 * This is the drop-in boundary: every entry point names the reference interface it replaces
 * (paths relative to the reference tree).  Plain pointers and sizes only.  Host arrays use the
 * reference's layouts:
 *     volume    float32 [Nslice][Ny][Nz]                 (container/Matrix3D.cpp:20-23)
 *     sinogram  float32 [Nslice][Nproj*Nray], index angle*Nray+ray   (gpu/reconstructor.py:54-56)
 * Device-resident state lives inside the opaque engine (slab-interleaved layout).
 *
 * Every function returns 0 on success or a tomo_status code; tomo_last_error() gives the text.
 * One engine = one device slab of slices; calls on one engine must be serialised by the caller.
 */
#ifndef TOMO_HIP_H
#define TOMO_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct tomo_engine tomo_engine;

enum tomo_status { TOMO_OK = 0, TOMO_ERR_ARG = 1, TOMO_ERR_HIP = 2, TOMO_ERR_STATE = 3, TOMO_ERR_GEOMETRY = 4 };

/* volumes held by the engine (tomoengine.hpp:44: recon, temp_recon, original_volume, yk, recon_old) */
enum tomo_volume { TOMO_VOL_RECON = 0, TOMO_VOL_TEMP = 1, TOMO_VOL_ORIGINAL = 2, TOMO_VOL_YK = 3, TOMO_VOL_RECON_OLD = 4,
                   TOMO_VOL_COUNT = 5,
                   TOMO_VOL_USER0 = 5,      /* caller-managed extra volumes (per-element tomograms of Matrix4D, multimodal.hpp) */
                   TOMO_VOL_SLOTS = 5 + 40 };
/* sinograms held by the engine (tomoengine.hpp:53: b = measured, g = re-projection) */
enum tomo_sinogram { TOMO_SINO_B = 0, TOMO_SINO_G = 1, TOMO_SINO_R = 2 /* residual scratch */,
                     TOMO_SINO_USER0 = 3,   /* caller-managed extra sinograms (per-element bChem, multimodal.hpp) */
                     TOMO_SINO_SLOTS = 3 + 40,
                     /* read-only pseudo-slot of tomo_get_sinogram: A * yk as tomo_fista_project_yk formed it (TOMO_ERR_STATE when
                      * no such projection is in hand); TOMO_SINO_G itself always stays A * recon (tomoengine.cpp:410-427,459) */
                     TOMO_SINO_YK_MODEL = 1000 };

/* slots of the device scalar buffer (doubles); each holds THIS slab's partial sum */
enum tomo_scalar { TOMO_S_DD = 0,      /* sum (A x - b)^2            data_distance  */
                   TOMO_S_DIFF = 1,    /* sum (recon - temp)^2       matrix_2norm   */
                   TOMO_S_TV = 2,      /* sum sqrt(eps + |grad|^2)   tv / tv_gd / tv_fgp return value */
                   TOMO_S_GNORM = 3,   /* sum g^2 of the TV gradient (one tv_gd inner iteration) */
                   TOMO_S_RMSE = 4,    /* sum (recon - original)^2   rmse           */
                   TOMO_S_COST = 5,    /* Poisson-ML cost            poisson_ML     */
                   TOMO_S_L1 = 6,      /* sum |recon|                l1_norm        */
                   TOMO_S_GNORM_ALL = 8, /* sum g^2 over the sub-slab engines of a slab group (tomo_scalar_sum_from) */
                   TOMO_S_DIFF2 = 7,   /* a second step-norm slot: ASD-POCS keeps the SART step norm here until the
                                          iteration's scalars are read together (one all-reduce, one read-back) */
                   TOMO_S_DART_FREE = 9,      /* free voxels of the last tomo_dart_classify (an exact integer) */
                   TOMO_S_DART_BOUNDARY = 10, /* boundary voxels of the last tomo_dart_classify */
                   TOMO_S_COUNT = 16 };

const char *tomo_last_error(void);

/* GPU count; replaces tomofusion/__init__.py:10-18 (pycuda device_count). */
int tomo_device_count(int *count);

/* Host-only system matrix: drop-in for parallelRay(Nside, angles) of tomofusion/cpu/utils/pytvlib.py:8-121.
 * angles_rad[i] must be angle_deg*pi/180 evaluated in double.  Writes up to cap entries of (row, col, val)
 * as float32 in parallelRay's generation order and the entry count to *nnz (call with cap = 0 to size). */
int tomo_system_matrix(int nray, int nproj, const double *angles_rad, int64_t cap,
                       float *rows, float *cols, float *vals, int64_t *nnz);

/* tomoengine(Nslice, Nray, angles) -- gpu/utils/tomoengine.cpp:48-84.  Builds the line-intersection system
 * matrix of parallelRay for these angles and uploads its ray (CSR) and per-angle voxel tables. */
int tomo_create(int nslice, int nray, int nproj, const double *angles_rad, int device, tomo_engine **out);

/* ctvlib(Nslice, Nray, Nproj) + load_A(A) -- cpu/utils/ctvlib.cpp:28-48, 309-315.  A given as the three
 * float32 rows of parallelRay's output.  The matrix must have at most two rays of one angle per pixel. */
int tomo_create_from_matrix(int nslice, int nray, int nproj, int64_t nnz, const float *rows, const float *cols,
                            const float *vals, int device, tomo_engine **out);

int tomo_destroy(tomo_engine *e);

/* Run all work of this engine on an existing HIP stream (hipStream_t), e.g. torch's current stream. */
int tomo_set_stream(tomo_engine *e, void *hip_stream);
int tomo_synchronize(tomo_engine *e);
int tomo_get_device(tomo_engine *e, int *device);                       /* tomoengine.cpp:92-95 get_gpu_id */
int tomo_get_dims(tomo_engine *e, int *nslice, int *nray, int *nproj, int64_t *nnz);

/* ---- data in / out ------------------------------------------------------------------------------- */
int tomo_set_tilt_series(tomo_engine *e, const float *b);               /* tomoengine.cpp:101 setTiltSeries */
int tomo_set_sinogram(tomo_engine *e, int which, const float *b);       /* multimodal.cpp:150-151 set_haadf/chem_tilt_series */
int tomo_get_sinogram(tomo_engine *e, int which, float *out);           /* :454-458 get_projections / get_model_projections */
int tomo_set_volume(tomo_engine *e, int vol, const float *data);        /* all slices at once */
int tomo_get_volume(tomo_engine *e, int vol, float *data);
int tomo_set_slice(tomo_engine *e, int vol, int s, const float *img);   /* :104-106 setOriginalVolume / setRecon */
int tomo_get_slice(tomo_engine *e, int vol, int s, float *img);         /* :452 getRecon */
/* ---- the same data calls on DEVICE buffers of the caller --------------------------------------------------------------------
 * For a host that already has the tilt series on the GPU, or wants the reconstruction there (the reference only ever hands over
 * host arrays: gpu/reconstructor.py:54-56 packs and uploads, :207-215 downloads and converts).  `dev` is plain device memory of
 * the engine's device holding `nelems` elements of `dtype`, dense: a volume as [Nslice][Ny][Nz], a sinogram in `layout`.  The
 * conversion kernel reads or writes the caller's buffer directly: no staging buffer is allocated or touched, and the call does
 * not wait on the host.  `hip_stream` (hipStream_t, NULL = the default stream) is the stream on which the caller produced the
 * data (set) or will consume it (get): the engine's stream is ordered behind it before the kernel and it is ordered behind the
 * engine's stream after the kernel, with events on the device, so the caller may also overwrite or free a buffer it has set from
 * that stream.  The same stream as the engine's (tomo_set_stream) needs no event.
 * Checked before anything is enqueued, TOMO_ERR_ARG otherwise: dtype and layout are one of the constants; nelems is Nslice*Ny*Nz
 * (volume) or Nslice*Nproj*Nray (sinogram); hipPointerGetAttributes knows `dev` as device memory (not pinned, managed or pageable
 * host memory, not NULL) of the engine's device, and its allocation holds nelems elements from `dev` on.
 * A set writes the padding slices of the engine's layout as zero; a get writes nothing outside the nelems elements.  Slot
 * bookkeeping (write versions, the model sinogram's claim, the FISTA state) is that of the host calls. */
enum tomo_dtype { TOMO_F32 = 0,             /* float32 */
                  TOMO_F64 = 1 };           /* float64: rounded to nearest even on the way in (a C cast), exact on the way out */
enum tomo_sino_layout { TOMO_SINO_PACKED = 0,   /* [Nslice][Nproj][Nray]: the host calls' layout, index angle*Nray+ray */
                        TOMO_SINO_PUBLIC = 1 }; /* [Nslice][Nray][Nproj]: what TomoGPU is given (gpu/reconstructor.py:54-56 transposes it) */
int tomo_set_volume_device(tomo_engine *e, int vol, const void *dev, int dtype, int64_t nelems, void *hip_stream);
int tomo_get_volume_device(tomo_engine *e, int vol, void *dev, int dtype, int64_t nelems, void *hip_stream);
int tomo_set_sinogram_device(tomo_engine *e, int which, const void *dev, int dtype, int layout, int64_t nelems, void *hip_stream);
/* which = TOMO_SINO_YK_MODEL reads as in tomo_get_sinogram */
int tomo_get_sinogram_device(tomo_engine *e, int which, void *dev, int dtype, int layout, int64_t nelems, void *hip_stream);
int tomo_restart_recon(tomo_engine *e);                                 /* :462-468 restart_recon */
int tomo_copy_volume(tomo_engine *e, int dst, int src);                 /* :404 copy_recon = (TEMP <- RECON) */
/* volume of another engine with the same slab shape (rebuilding the tilt geometry keeps the reconstruction:
 * tomoengine::update_projection_angles, tomoengine.cpp:128-149) */
int tomo_copy_volume_from(tomo_engine *dst, int dst_vol, tomo_engine *src, int src_vol);
/* the same rebuild without a copy and with one set of tables in memory: release the old engine's tables and sinograms
 * (only tomo_adopt_volumes / tomo_destroy remain valid on it), create the new engine, move the volumes over
 * (ctvlib::update_proj_angles, ctvlib.cpp:317-333, keeps recon across a matrix change as well) */
int tomo_release_geometry(tomo_engine *e);
int tomo_adopt_volumes(tomo_engine *dst, tomo_engine *src);

/* ---- projector -------------------------------------------------------------------------------------- */
int tomo_forward_projection(tomo_engine *e, int vol, int sino);         /* :416-427 forwardProjection; :109-126 create_projections */
int tomo_back_projection(tomo_engine *e, int sino, int vol);            /* :279-291 back_projection: vol = A^T sino */
int tomo_lipschitz(tomo_engine *e, float *L);                           /* ctvlib.cpp:194-202 lipschits; tomoengine.cpp:369-371 */
int tomo_row_inner_product(tomo_engine *e);                             /* ctvlib.cpp:234-242 normalization */
int tomo_lipschitz_cimmino(tomo_engine *e, float *L);                   /* ctvlib.cpp:198-199: max(A^T M A 1), M = diag(|A_i|^2) */

/* ---- reconstruction steps --------------------------------------------------------------------------- */
/* ctvlib::SIRT(beta): x = max(0, x + beta A^T (b - A x))   ctvlib.cpp:205-221.  vol = RECON or YK. */
int tomo_sirt_landweber(tomo_engine *e, int vol, float beta, int niter);
/* ctvlib::SIRT(beta) after cimminos_method(): x = max(0, x + A^T M (b - A x) beta/Nrow), M_ii = |A_i|^2 -- the
 * reference multiplies by the row norms (quirk Q10); reproduced as written   ctvlib.cpp:212-216, 245-251 */
int tomo_sirt_cimmino(tomo_engine *e, int vol, float beta, int niter);
/* tomoengine::SIRT(nIter) (ASTRA SIRT, min-constraint 0): x = max(0, x + C A^T R (b - A x))  tomoengine.cpp:181-205 */
int tomo_sirt(tomo_engine *e, int vol, int niter);
/* the same with the measured data in any sinogram slot: multimodal::SIRT(e, s, nIter)  multimodal.cpp:339-358 */
int tomo_sirt_data(tomo_engine *e, int vol, int sino_b, int niter);
/* tomoengine::SART(beta, nIter): nIter sweeps of per-angle updates, order[] = angle permutation or NULL
 * (sequential)  tomoengine.cpp:151-179 */
int tomo_sart(tomo_engine *e, int vol, float beta, int niter, const int32_t *order);
int tomo_sart_data(tomo_engine *e, int vol, int sino_b, float beta, int niter, const int32_t *order); /* multimodal.cpp:377-396 */
/* The sweep of tomo_sart_data whose last back-projection also leaves ||x_new - track_vol||^2 in scalar `slot` and
 * copies x_new into track_vol: the `matrix_2norm()` + `copy_recon()` pair that follows the SART sweep in the ASD-POCS
 * loop (examples/sim_ASD.py:70-78, gpu/reconstructor.py:168-176) without two more passes over the slab. */
int tomo_sart_tracked(tomo_engine *e, int vol, int sino_b, float beta, int niter, const int32_t *order, int track_vol, int slot);
/* tomoengine::CGLS(nIter): CGLS restarted from the current volume, per slice, then positivity  tomoengine.cpp:207-229 */
int tomo_cgls(tomo_engine *e, int vol, int niter);
/* tomoengine::FBP(apply_positivity): recon = scale * A^T (taps * b), taps[0..Nray-1] = symmetric real-space filter
 * (built by the host for the named filter, pytvlib.py:33-36)  tomoengine.cpp:317-347 */
int tomo_fbp(tomo_engine *e, const float *taps_host, float scale, int apply_positivity);
/* ctvlib::ART(beta): row-action Kaczmarz sweep + positivity  ctvlib.cpp:137-155 */
int tomo_art(tomo_engine *e, float beta);
/* ctvlib::randART(beta) with the rows visited in the given permutation (the reference's loop, ctvlib.cpp:158-179,
 * rewrites its own counter and draws from an unseedable device: quirk Q9)  */
int tomo_art_order(tomo_engine *e, float beta, const int32_t *order_host);
/* tomoengine::poisson_ML(lambda): cost accumulates in TOMO_S_COST  tomoengine.cpp:231-246, 293-315 */
int tomo_poisson_ml(tomo_engine *e, float lambda);
/* out = (A x - b)/(A x + 0.1), cost sum(Ax - b log(Ax + 0.1)) -> TOMO_S_COST   multimodal.cpp:284-292, 466-473 */
int tomo_poisson_residual(tomo_engine *e, int vol, int sino_b, int sino_out);
int tomo_scale_volume(tomo_engine *e, int vol, float factor);           /* multimodal.cpp:307-309 rescale_tomograms */
int tomo_positivity(tomo_engine *e, int vol);                           /* ctvlib.cpp:224-231 */
int tomo_soft_threshold(tomo_engine *e, int vol, float lambda);         /* matrix_ops.cu:64-75 */
int tomo_fista_momentum(tomo_engine *e, float beta);                    /* tomoengine.cpp:381-384 */
/* A yk = (1 + beta) A recon - beta A recon_old by linearity, from the projections the driver's cost evaluation made anyway
 * (gpu/reconstructor.py:121-155): call after tomo_data_distance_sq(RECON); a no-op unless provably valid; *done = 1 when the model
 * sinogram now holds A yk and the next tomo_sirt(YK) will start from it.  That projection is dropped by any write to YK and by any
 * write-intent access of RECON (the caller has left the iteration it was formed in): the next tomo_sirt(YK) then projects again */
int tomo_fista_project_yk(tomo_engine *e, int *done);

/* ---- scalar reductions: partial sums of this slab land in the device scalar buffer ------------------
 * The sums are binary64 and gathered through 256 partial-sum slots by atomic additions, so a value is reproducible to the rounding of
 * the order of those additions (the tests compare such values at 1e-12 relative: a figure chosen far above the 2^-53 of one
 * rounding, not a measured one).  The projector's sums (TOMO_S_DD, TOMO_S_COST) and the tracked back-projection's give every WAVE a slot
 * of its own: in a launch of at most 256 waves no two additions meet in one slot, so by construction the value does not depend on
 * the order in which the waves finish (larger launches share slots and vary in the last bits as before). */
int tomo_data_distance_sq(tomo_engine *e, int vol);                     /* tomoengine.cpp:410-413 -> TOMO_S_DD (also fills G) */
/* the same evaluation on a second stream, for a volume the main sequence no longer writes (e.g. the TEMP copy);
 * tomo_async_wait (also implied by tomo_read_scalars) orders the main stream behind it */
int tomo_data_distance_sq_async(tomo_engine *e, int vol);
int tomo_async_wait(tomo_engine *e);
int tomo_diff_norm_sq(tomo_engine *e, int a, int b, int slot);          /* :407 matrix_2norm, :433 rmse */
int tomo_sino_diff_norm_sq(tomo_engine *e, int a, int b, int slot);     /* multimodal.cpp:489 (g - bh).norm() */
int tomo_sino_proj_max(tomo_engine *e, int sino, float *out_host);      /* multimodal.cpp:323-327: max per projection */
int tomo_sino_proj_scale(tomo_engine *e, int sino, const float *div_host, const float *mul_host); /* b <- b/div[p]*mul[p] */
int tomo_l1_norm(tomo_engine *e, int vol);                              /* :436 l1_norm -> TOMO_S_L1 */

/* ---- tilt-series alignment ------------------------------------------------------------------------------------------------
 * The reference aligns on the host, one image at a time, by the centre of mass (cpu/utils/logger.py:237-252: integer roll so that
 * the centre of mass lands on size // 2); the first three calls do that on the resident series and add what projection matching
 * needs, the last two take out an in-plane rotation (a tilt axis that does not run along the detector columns).  Projection a of a sinogram slot is the image X_a[r][s], ray r in [0, Nray), slice s in [0, Nslice).  A shift (dr, ds)
 * moves content by +d: dst_a[r][s] = src_a(r - dr, s - ds), the sense of np.roll.  One whole-volume engine only: an engine bound
 * to a communicator returns TOMO_ERR_STATE.  All three wait for their result; results are bit-identical from run to run.
 *   tomo_sino_moments: out_host[a] = {sum X_a, sum r X_a, sum s X_a} over the real samples, in binary64.
 *   tomo_sino_xcorr:   out_host[a][u + S][v + S] = sum_{r,s} (A_a[r][s] - mA_a)(B_a[r + u][s + v] - mB_a), S = max_shift, over the
 *       (r, s) with both samples inside the image; mA, mB the per-angle means (0 with subtract_mean = 0).  1 <= S <= 16 and
 *       S <= min(Nray, Nslice) - 1.  Not divided by the overlap: the entry at (u, v) sums (Nray - |u|)(Nslice - |v|) products, which
 *       leans the peak towards zero shift by the factor (1 - |u|/Nray)(1 - |v|/Nslice) -- 3 % per axis at S = 16, Nray = 512, large
 *       for stacks only a few S thin -- exactly like the FFT correlation of zero-padded images.
 *   tomo_sino_shift:   bilinear resampling by shifts_host[a] = {dr, ds}; samples outside the image are 0, or wrap around (wrap = 1).
 *       A whole-pixel shift reproduces the source bits; a shift beyond the image without wrap gives zeros.  src != dst.
 *   tomo_sino_affine:  dst_a[r][s] = bilinear(src_a)(r', s') with r' = m00 r + m01 s + m02, s' = m10 r + m11 s + m12 and
 *       m_host[a] = {m00, m01, m02, m10, m11, m12} in binary64: the map from a destination sample to its source position (in-plane
 *       rotation about any centre, magnification and shift in ONE interpolation).  Taps outside [0, Nray) x [0, Nslice) are 0; there
 *       is no wrap form.  The coordinates are evaluated in binary64, fma(m00, r, fma(m01, s, m02)), and split there into floor and
 *       fraction; only the fraction is rounded to binary32, and a zero fraction drops its tap.  Hence: an identity matrix copies the
 *       source bits; a pure translation {1, 0, -dr, 0, 1, -ds} gives the bits of tomo_sino_shift(wrap = 0) for the same (binary32)
 *       shift, fractions included; a whole-pixel map (quarter turns, flips) copies samples, and an Inf next to a copied sample never
 *       becomes NaN.  src != dst.
 *   tomo_sino_axis_profile: out_host[a][s] = sum_r X_a[r][s], in binary64 from the first sample, added in a fixed order.  For a
 *       parallel-beam series whose tilt axis runs along s this mass of slice s is the same in every projection a.
 *   tomo_sino_affine_normal: one Gauss-Newton evaluation of an intensity-based matching of every projection by a shift, an in-plane
 *       rotation and a magnification, in one pass.  F_a = projection a of fixed_sino (the model), G_a = projection a of moving_sino (the
 *       series as given); m_host[a] is the destination-to-source map of tomo_sino_affine: sample (r, s) of F_a has the position
 *       p = (r', s') in G_a, evaluated by the same binary64 chain and split the same way (a fraction that rounds to 1 is the next whole
 *       pixel with t = 0).  A sample counts when (a) all four tap positions lie inside G_a, 0 <= i and i + 1 <= size - 1 on both axes
 *       with i the first tap AFTER that split (a coordinate in [-2^-25, 0) is pixel 0 with t = 0 and can count; stricter than the
 *       zero padding of tomo_sino_affine), and (b) margin <= r <= Nray - 1 - margin and margin <= s <= Nslice - 1 -
 *       margin.  A sample that does not count loads no tap and adds nothing: an Inf or a NaN there, or in a sample of G that is no tap
 *       of a counting sample, stays out; padding slices are never read as data.  Per counting sample, in binary32: w = the four-tap
 *       expression of tomo_sino_affine with every product and every sum rounded once (no fused multiply-add; a zero fraction drops
 *       its tap, so whole-pixel maps copy bits -- for fractional maps the bits of tomo_sino_affine's own output are NOT promised, since
 *       that kernel's plain expression is the compiler's to fuse) and (g_r, g_s) = the derivative of the
 *       bilinear interpolant of the cell, g_r = (1 - ts)(x10 - x00) + ts (x11 - x01), g_s = (1 - tr)(x01 - x00) + tr (x11 - x10), the
 *       first term a product and the second a fused multiply-add (the exact order: kernels_align_normal.hip.h); at t = 0 the one-sided
 *       derivative towards the second tap.  Then in binary64: res = w - F, q = p - c_G with c_G = ((Nray - 1) / 2, (Nslice - 1) / 2),
 *       J = (g_r, g_s, q_r g_s - q_s g_r, q_r g_r + q_s g_s), the derivative of G(c_G + e^lambda Rot(omega)(p - c_G) + t) by
 *       (t_r, t_s, omega, lambda) at zero.  out_host[a] = the sums over the counting samples of projection a:
 *       [0..9] the upper triangle of J^T J, row-major;  [10..13] J^T res;  [14] sum res^2;  [15] the count;  [16..18] sum F^2, sum w^2,
 *       sum F w;  [19..20] sum F, sum w.  With no counting sample all 21 are +0.0, and the other projections are unaffected.  Two
 *       fixed-order reduction stages, no atomics: the same bits from call to call.  Both slots are only read (no claim on
 *       TOMO_SINO_G is dropped, no write version moves); fixed_sino == moving_sino is allowed.  Waits for its result.
 *       TOMO_ERR_ARG also for margin < 0 or 2 * margin >= Nray or Nslice; TOMO_ERR_STATE also for a slab of a larger volume
 *       (tomo_set_slab_edges) and for released geometry.  A refused call enqueues nothing.
 * TOMO_ERR_ARG: bad slot, src == dst, max_shift out of range, a null pointer, a non-finite shift or matrix entry. */
int tomo_sino_moments(tomo_engine *e, int sino, double *out_host);      /* [Nproj][3]   logger.py:237-247 */
int tomo_sino_xcorr(tomo_engine *e, int sino_a, int sino_b, int max_shift, int subtract_mean, double *out_host); /* [Nproj][2S+1][2S+1] */
int tomo_sino_shift(tomo_engine *e, int src, int dst, const float *shifts_host, int wrap);   /* logger.py:249-250 */
int tomo_sino_affine(tomo_engine *e, int src, int dst, const double *m_host);                /* [Nproj][6] */
int tomo_sino_affine_normal(tomo_engine *e, int fixed_sino, int moving_sino, const double *m_host /* [Nproj][6] */, int margin,
                            double *out_host /* [Nproj][21] */);                             /* waits */
int tomo_sino_axis_profile(tomo_engine *e, int sino, double *out_host);                      /* [Nproj][Nslice] */

/* ---- refinement of the per-projection tilt angles (kernels_tilt.hip.h; the drivers are align.match_tilt_angles and
 * TomoGPU.refine_tilt_angles) ----------------------------------------------------------------------------------------------
 * The reference takes the tilt angles as given (tomoengine.cpp:128-149 only replaces them); these two calls are what estimating them
 * needs.  In the convention of the system matrix (cpu/utils/pytvlib.py:8-121: pixel i * N + j of a slice at X = j - (N - 1) / 2,
 * Y = (N - 1) / 2 - i; ray t of angle theta through (t cos, t sin) along (-sin, cos)) the derivative of a projection by its own angle
 * is the projection of ONE volume, d g_theta / d theta = A_theta (D f) with D f = X d_Y f - Y d_X f.  One whole-volume engine, like the
 * alignment calls above: TOMO_ERR_STATE on an engine with a communicator, a slab of a larger volume (tomo_set_slab_edges) or released
 * geometry.  A refused call enqueues nothing and writes nothing.
 *   tomo_volume_rot_derivative: dst = D src per slice, central differences (f[+1] - f[-1]) / 2 across the pixel grid, taken as 0 in
 *       the direction that crosses the border (rows 0 and N - 1 for d_Y, columns 0 and N - 1 for d_X).  Binary32, every operation
 *       rounded once: dy = f[i - 1][j] - f[i + 1][j], dx = f[i][j + 1] - f[i][j - 1], q = (0.5 Y) dx, dst = fma(0.5 X, dy, -q); the
 *       halved coordinates are exact.  A constant slice gives exact zeros; padding stays zero.  Enqueued on the engine's stream, no
 *       wait.  TOMO_ERR_ARG: a bad slot, src_vol == dst_vol.
 *   tomo_sino_tilt_normal: one pass over three sinogram slots, the data b, the model g and the derivative d.  out_host[a] =
 *       {sum (b - g) d, sum d^2, sum (b - g)^2, the count} over the samples of projection a with margin <= ray <= Nray - 1 - margin and
 *       margin <= slice <= Nslice - 1 - margin, in binary64 from the first sample (the products by fused multiply-add); a sample that
 *       does not count is not looked at.  The Gauss-Newton step of angle a is out[a][0] / out[a][1] radians.  Two fixed-order
 *       reduction stages, no atomics: the same bits from call to call.  The slots are only read (no claim on TOMO_SINO_G is dropped)
 *       and may coincide.  Waits for its result.  TOMO_ERR_ARG: a bad slot, a null pointer, margin < 0 or 2 * margin >= Nray or Nslice. */
int tomo_volume_rot_derivative(tomo_engine *e, int src_vol, int dst_vol);
int tomo_sino_tilt_normal(tomo_engine *e, int b_sino, int g_sino, int d_sino, int margin, double *out_host /* [Nproj][4] */);  /* waits */

/* ---- conditioning of the tilt series (kernels_condition.hip.h; the drivers are TomoGPU.subtract_background / despeckle /
 * normalize_intensity / condition) -------------------------------------------------------------------------------------------
 * The reference cleans every measured image on the host before it centres it (cpu/utils/logger.py:93): background_subtract
 * (cpu/utils/logger.py:255-263) removes the mean of the image's first-quarter corner.  These three calls do that on the resident series
 * and add the two steps electron tomography takes for granted, outlier ("hot pixel", X-ray) removal by a local median and a gain
 * per projection.  Conventions of the alignment block: projection a of a slot is the image X_a[r][s], 0 <= r < Nray, 0 <= s < Nslice;
 * padding slices are never read as data and stay zero in whatever is written.  One whole-volume engine only: TOMO_ERR_STATE on an
 * engine with a communicator, a slab of a larger volume (tomo_set_slab_edges) or released geometry.  A refused call enqueues nothing and
 * writes nothing.  Source slots are only read (no claim on TOMO_SINO_G is dropped unless G is the destination).
 *   tomo_sino_window_stats: out_host[a] = {sum X, sum X^2, min X, max X} over r0 <= r < r1, s0 <= s < s1 of projection a.  The sums
 *       in binary64 from the first sample, the square a binary64 product of the converted sample; two fixed-order reduction stages,
 *       no atomics: the same bits from call to call.  The mean of the window [0, Nray / 4) x [0, Nslice / 4) is the background of
 *       cpu/utils/logger.py:255-263.  Waits for its result.  TOMO_ERR_ARG: an empty window or one that leaves the image.
 *   tomo_sino_median: m = the median of the (2 radius + 1)^2 samples around (r, s) of projection a of src, radius 1 or 2 (the 5th
 *       smallest of 9, the 13th smallest of 25), indices clamped to the image: the border is replicated, projections never mix.  A
 *       selection, never an average: m is one of the samples (among tied zeros the sign is unspecified).  d = x - m, one binary32
 *       subtraction.  out_host[a] = {sum d, sum |d|, sum d^2, the number of samples, the number replaced} in binary64, summed like
 *       the window statistics.  thresh_host == NULL only measures: nothing is written, dst must be -1, the number replaced is 0.
 *       Otherwise dst = (|d| > thresh_host[a]) ? m : x, compared in binary32, src != dst: +Inf copies the source bits, 0 gives the
 *       median image.  Inputs are taken as finite: a NaN makes the values of the windows it lies in unspecified and nothing else.
 *       Waits for its result.  TOMO_ERR_ARG: radius not 1 or 2, a negative or NaN threshold, src == dst, dst != -1 when measuring.
 *   tomo_sino_intensity: dst = fma(gain_a, x, offset_a), one fused operation, gain_offset_host[a] = {gain_a, offset_a}; with
 *       clamp != 0 followed by max(0, .) (a NaN or -0 gives +0).  src == dst is allowed; gain 1 with offset 0 copies.  Enqueued on the
 *       engine's stream, no wait (the table is consumed before the call returns).  TOMO_ERR_ARG: a non-finite gain or offset.
 * TOMO_ERR_ARG also: a bad slot, a null pointer. */
int tomo_sino_window_stats(tomo_engine *e, int sino, int r0, int r1, int s0, int s1, double *out_host /* [Nproj][4] */);   /* waits; logger.py:255-263 */
int tomo_sino_median(tomo_engine *e, int src, int dst, int radius, const float *thresh_host /* [Nproj] or NULL */,
                     double *out_host /* [Nproj][5] */);                                     /* waits */
int tomo_sino_intensity(tomo_engine *e, int src, int dst, const float *gain_offset_host /* [Nproj][2] */, int clamp);   /* logger.py:261 */

/* ---- marker (fiducial / feature) detection (kernels_markers.hip.h; the driver is TomoGPU.align_markers, the tracking and the
 * least-squares model are tomo_tv_amd/align.py: link_markers, solve_markers) --------------------------------------------------
 * An extension: the reference has no marker alignment.  Conventions of the conditioning block: projection a of a slot is the image
 * X_a[r][s], 0 <= r < Nray, 0 <= s < Nslice; padding slices are never read as data and are zero in whatever is written; projections
 * never mix.  One whole-volume engine only: TOMO_ERR_STATE on an engine with a communicator, a slab of a larger volume
 * (tomo_set_slab_edges) or released geometry.  A refused call enqueues nothing and writes nothing.  Source slots are only read (no
 * claim on TOMO_SINO_G is dropped unless G is the destination).  No floating-point atomics: the same bits from call to call.
 *   tomo_sino_template_ncc: the zero-mean normalised cross-correlation of every projection with one (2R+1) x (2R+1) template,
 *       template_host[k][j] at ray offset k - R and slice offset j - R, W = (2R+1)^2.  The library forms t = T - mean(T) scaled to
 *       sum t^2 = 1 in binary64 and rounds it to binary32.  For a sample whose whole window lies inside the image, in binary32, every
 *       operation rounded on its own and the window walked in row-major order from 0:  m = (sum x) / W;  c = sum t (x - m);
 *       v = sum (x - m)^2;  dst = c / sqrt(v) where v > var_floor * W (one binary32 product), else 0.  A sample whose window leaves
 *       the image gets 0 (so a projection smaller than the template is all zero).  Enqueued on the engine's stream, no wait (the
 *       template is consumed before the call returns).  TOMO_ERR_ARG: R outside 1..8, src == dst, a constant or non-finite template,
 *       a negative or NaN var_floor.
 *   tomo_sino_peaks: the local maxima of every projection.  (r, s) is a peak iff x >= threshold and, for every other sample
 *       (r', s') of its (2 radius + 1)^2 window clipped to the image, x > x' where (r', s') precedes (r, s) in row-major (r, s)
 *       order and x >= x' where it follows: of a plateau exactly the first sample.  A NaN is never a peak, nor is a sample with a NaN
 *       in its window.  count_host[a] = the true number of peaks of projection a, whatever capacity is.  records_host[a][k], for
 *       k < min(count_host[a], capacity), = eight 32-bit words: r, s (int32), the binary32 values at (r, s), (r-1, s), (r+1, s),
 *       (r, s-1), (r, s+1) -- a neighbour outside the image repeated as the centre value -- and a zero; sorted by r * Nslice + s
 *       ascending.  Where count_host[a] > capacity the records of that projection are unspecified (call again with the capacity the
 *       counts ask for); records past the count are not written.  Waits for its result.  TOMO_ERR_ARG: radius outside 1..8, a NaN
 *       threshold, capacity < 1.
 * TOMO_ERR_ARG also: a bad slot, a null pointer. */
int tomo_sino_template_ncc(tomo_engine *e, int src, int dst, const float *template_host /* [2R+1][2R+1] */, int R, float var_floor);
int tomo_sino_peaks(tomo_engine *e, int sino, int radius, float threshold, int capacity, int *count_host /* [Nproj] */,
                    int *records_host /* [Nproj][capacity][8] */);                           /* waits */

/* ---- binning and prolongation between two engines (coarse-to-fine drivers) --------------------------------------------------
 * `fine` and `coarse` are two different whole-volume engines on one device whose grids differ by factor = f, 2 or 4:
 *     fine Nray == f * coarse Nray,   coarse Nslice == ceil(fine Nslice / f),   and for tomo_sino_bin the same Nproj.
 * Nray must be divisible by f because the rule on rays is exact: parallelRay puts the rays at linspace(-(N-1)/2, (N-1)/2, N), and the
 * centre of the fine rays f r', ..., f r' + f - 1 is f times coarse ray r' of an N/f geometry.  Nslice need not be: the trailing coarse
 * slice takes the k < f fine slices that exist.
 * Scale.  A coarse voxel is the MEAN of the fine voxels it covers, and the coarse engine's matrix measures chord lengths in coarse
 * pixels, each f fine pixels long.  A ray through the binned volume therefore collects 1/f of what the f fine rays it replaces collect
 * on average: a coarse sample is the mean of its f * k fine samples divided by f, i.e. (sum of the f * k samples) * 1 / (f^2 k), for
 * full bins (k = f: 1 / f^3) and for the trailing partial bin (k < f) alike.  With it A_coarse bin(x) == bin(A_fine x) to rounding at
 * 0 and 90 degrees, where a ray runs along a pixel row, and up to the discretisation of the strip model elsewhere.
 *   tomo_sino_bin:   dst_a[r'][s'] = c * sum_{i<f} sum_{j<k} src_a[f r' + i][f s' + j],  k = min(f, Nslice - f s'),  c = 1 / (f^2 k)
 *       rounded to binary32; the sum in binary32 in ascending (i, j) order, then one multiply by c.
 *   tomo_volume_bin: dst[y'][z'][s'] = c * sum over the f x f x k block in ascending (y, z, s) order, the same c: the mean.
 *   tomo_volume_prolong: cell-centred trilinear interpolation with clamp-to-edge, coarse `vol` into fine `fine_vol`.  Per axis the
 *       fine index i sits at u = (i + 0.5) / f - 0.5; the taps are floor(u) and floor(u) + 1, clamped to the coarse range, and
 *       t = u - floor(u) (1/4 or 3/4 at f = 2, an odd eighth at f = 4).  Each lerp is fma(t, b - a, a), along s, then z, then y; where
 *       the clamp makes a and b the same sample it is copied.  The trailing partial coarse slice is treated as an ordinary cell.
 *       Nothing is rescaled: means carry the same units.
 * Hence, bit for bit: a constant volume prolongs to the same constant; a clamped edge copies (an Inf there stays an Inf); a constant
 * sinogram bins to const / f wherever k is a power of two and the partial sums j * const, j <= f k, are binary32 numbers (any constant
 * with log2(f k) spare low mantissa bits: the sum is sequential, and 3 * const already rounds for a constant that uses all 24); the
 * pitch padding of the destination is written as zero; no source sample at slice index >= Nslice enters a result; the same bits from
 * run to run.  An Inf in a bin gives Inf, never NaN.
 * Ordering: the kernel runs on the destination engine's stream, which first waits (by an event, on the device) for what the source
 * engine's stream has enqueued; the source engine's stream then waits for the kernel.  No host wait, and nothing to synchronise before
 * the next call on either engine.  The destination counts as written (as after tomo_set_volume / tomo_set_sinogram); the source is read.
 * TOMO_ERR_ARG: a null engine, the same engine twice, factor not 2 or 4, a bad slot, different devices, sizes that break the rule
 * above.  TOMO_ERR_STATE: an engine bound to a communicator or whose geometry was released.  A refused call has enqueued nothing and
 * leaves both engines usable. */
int tomo_sino_bin(tomo_engine *fine, int sino, tomo_engine *coarse, int coarse_sino, int factor);
int tomo_volume_bin(tomo_engine *fine, int vol, tomo_engine *coarse, int coarse_vol, int factor);
int tomo_volume_prolong(tomo_engine *coarse, int vol, tomo_engine *fine, int fine_vol, int factor);

/* ---- dual-axis tomography: one volume shared by two engines with perpendicular tilt axes ------------------------------------
 * A second tilt series about the perpendicular axis shrinks the missing wedge to a pyramid.  Every slice shares one system matrix and
 * the lanes index slices, so the second axis needs no new projector: it needs a second ordinary engine whose "slices" run along the
 * other axis, and the volume carried from one engine's layout into the other's.
 * Geometry.  At zero tilt the rays of parallelRay (cpu/utils/pytvlib.py:8-121) run along the image's row index and ray j meets column
 * j.  For the public volume X[s][y][z] the first tilt axis is s, the beam at zero tilt runs along y, and the perpendicular second axis
 * is z.  Engine B therefore has slice index z, row index y (still the beam) and column index s:
 *     X_B[z][y][s] = X_A[s][y][z],    b_B[z] = A_B vec(X[:, :, z]^T)  (the image with rows y and columns s).
 * Both engines must hold a cube, Nslice == Nray == N, of the same N; Nproj may differ.  At zero tilt the two series' projections are
 * transposes of each other, P_B[z][ray = s] = P_A[s][ray = z].  Mirrors and quarter turns of measured data are the caller's job.
 *   tomo_volume_cross:      dst[z][y][s] = src[s][y][z].  A copy of bits: NaN payloads, +-Inf, -0.0 and denormals survive.  dst is not read.
 *   tomo_volume_cross_axpy: dst[z][y][s] = fmaf(a, src[s][y][z], dst[z][y][s]), one rounding, then fmaxf(., 0) when clamp != 0.
 *       IEEE arithmetic throughout: a = 0 leaves a finite-source element's dst bits (except that -0.0 + 0.0 = +0.0), a = 0 against
 *       an Inf source gives NaN (0 * Inf), Inf stays Inf for a != 0.  fmaxf returns its other operand for a NaN, so with clamp a NaN
 *       result is stored as 0 -- the rule of every clamp of this engine (tomo_positivity).
 * Both write the pitch padding of the destination as zero, read no source element at slice index >= N, and give the same bits from
 * run to run.  Ordering and bookkeeping are those of tomo_volume_bin above: the kernel runs on the destination engine's stream, which
 * first waits (by an event, on the device) for what the source engine's stream has enqueued; the source's stream then waits for the
 * kernel.  No host wait.  The destination counts as written (its claim "G = A * vol" is dropped); the source is read.
 * TOMO_ERR_ARG: a null engine, the same engine twice, a bad slot, different devices, an engine that is not a cube, different N.
 * TOMO_ERR_STATE: an engine bound to a communicator, one that is a slab of a larger volume (tomo_set_slab_edges), or one whose geometry
 * was released -- crossing a sharded volume is an all-to-all between the ranks and is not provided.  A refused call has enqueued nothing
 * and leaves both engines usable. */
int tomo_volume_cross(tomo_engine *src, int src_vol, tomo_engine *dst, int dst_vol);
int tomo_volume_cross_axpy(tomo_engine *src, int src_vol, tomo_engine *dst, int dst_vol, float a, int clamp);

/* ---- a volume resampled by a 3-D affine map (positioning a tomogram; the pose of the second series of a dual-axis set) ----------
 * Two measured tilt series are never related by the exact transpose above: the grid is turned by hand, and the two tomograms differ
 * by a small rigid motion in all three axes.  These two calls apply such a motion (they do not estimate it): the volume counterpart of
 * tomo_sino_affine, rotation, magnification and shift in ONE trilinear interpolation.
 * Both volumes are addressed in their engine's public index order X[s][y][z].  m_host = {m00, m01, m02, m03, m10, .., m13, m20, ..,
 * m23}, a row-major 3 x 4 matrix in binary64, maps a DESTINATION voxel (s, y, z) to its SOURCE position (s', y', z') -- the
 * convention of tomo_sino_affine:
 *     s' = fma(m00, s, fma(m01, y, fma(m02, z, m03))),  y' = fma(m10, s, fma(m11, y, fma(m12, z, m13))),  z' = fma(m20, s, fma(m21, y, fma(m22, z, m23)))
 *   tomo_volume_affine:      dst[s][y][z] = trilinear(src)(s', y', z').  Taps outside [0, Nslice_src) x [0, N_src) x [0, N_src) are 0;
 *       there is no wrap form.  dst is not read.
 *   tomo_volume_affine_axpy: dst[s][y][z] = fmaf(a, that value, dst[s][y][z]), one rounding, then fmaxf(., 0) when clamp != 0: the
 *       rules of tomo_volume_cross_axpy, its NaN and Inf behaviour included (a = 0 against an Inf value gives NaN; with clamp a NaN
 *       result is stored as 0).
 * Arithmetic.  Each coordinate is evaluated in binary64 as the chain of three fused multiply-adds written above and split there
 * into floor and fraction.  Only the fraction t is rounded to binary32; a fraction that rounds to 1 is the next whole voxel with
 * t = 0.  Per axis the binary32 weights are w0 = 1 - t and w1 = t.  An axis whose fraction is zero keeps only its first tap, with
 * w0 = 1 exactly: the dropped tap is neither loaded nor multiplied.  With x[dy][dz][ds] the tap at (floor s' + ds, floor y' + dy,
 * floor z' + dz), the kept taps are combined in ascending (dy, dz, ds) order, ds fastest, every operation rounded once:
 *     o = ((wy[0] * wz[0]) * ws[0]) * x[0][0][0];  then for every further kept tap  o = fmaf((wy[dy] * wz[dz]) * ws[ds], x[dy][dz][ds], o)
 * and a voxel whose three fractions are all zero takes the bits of its single tap.  A coordinate outside (-1, size) has no tap inside
 * and gives 0.  Hence, bit for bit: an identity matrix on equal sizes copies the source (NaN payloads, -0.0 and denormals survive);
 * the permutation {0,0,1,0, 0,1,0,0, 1,0,0,0} between two cube engines gives the bits of tomo_volume_cross; a whole-voxel translation
 * copies samples and stores zeros where it runs out; quarter turns and flips copy samples; an Inf next to a copied sample never
 * becomes NaN.  One producer and one fixed expression per output word, no atomics: the same bits from run to run.
 * Engines.  src and dst are whole-volume engines on one device; their sizes may differ and need not be cubes.  They may be two
 * engines, or THE SAME engine with two different slots.  Both calls write the pitch padding of the destination as zero and read no
 * source element at slice index >= Nslice.  Ordering and bookkeeping are those of tomo_volume_cross: the source is read, the
 * destination counts as written (its claim "G = A * vol" is dropped); with two engines the kernel runs on the destination engine's
 * stream, which first waits (by an event, on the device) for what the source engine's stream has enqueued, and the source's stream
 * then waits for the kernel; with one engine the kernel runs on that engine's stream alone.  No host wait in either case: m_host is
 * read before the call returns.
 * TOMO_ERR_ARG: a null engine or pointer, a bad slot, the same engine with src_vol == dst_vol, different devices, a non-finite
 * matrix entry.  TOMO_ERR_STATE: an engine bound to a communicator, one that is a slab of a larger volume (tomo_set_slab_edges), or
 * one whose geometry was released.  A refused call has enqueued nothing and leaves both engines usable. */
int tomo_volume_affine(tomo_engine *src, int src_vol, tomo_engine *dst, int dst_vol, const double *m_host /* [12] */);
int tomo_volume_affine_axpy(tomo_engine *src, int src_vol, tomo_engine *dst, int dst_vol, const double *m_host, float a, int clamp);

/* ---- the 3-D rigid registration of two tomograms: the Gauss-Newton normal equations of one map ----------------------------------
 * The pose that the two calls above apply is ESTIMATED by minimising sum (G(M x) - F(x))^2 over the six rigid parameters; this call
 * evaluates, for one map, everything an iteration needs, in one pass over the fixed volume F (the loop itself is 32 numbers of host
 * arithmetic per iteration: tomo_tv_amd/align.py, register_volumes).  m_host is the destination-to-source map of tomo_volume_affine
 * with the same convention: the grid of F is the destination, the moving volume G the source, p = M x the position in G of the
 * voxel x = (s, y, z) of F, by the same chain of fused multiply-adds and the same split into floor and binary32 fraction.
 * A voxel counts only if (a) all eight tap positions lie inside G, 0 <= floor and floor + 1 <= size - 1 on every axis (stricter than
 * the zero padding above), and (b) x lies at least `margin` voxels from each face of F.  A voxel that does not count is not read
 * into anything: an Inf or a NaN in it, or in a voxel of G that is no tap of a counting voxel, stays out of the sums.
 * Per counting voxel: w = the trilinear value with the arithmetic and tap order stated above; g = (g_s, g_y, g_z) = the gradient of
 * the trilinear interpolant of the cell at the fractions, in binary32 from the same eight taps -- per component the four tap
 * differences along that axis, weighted by the products of the two other axes' weights, the first term a product and the three
 * others fused multiply-adds in ascending order of the two other axes' offsets (the exact order: kernels_register3d.hip.h);
 * r = w - F(x) and q = p - c_G with c_G = (size - 1) / 2 per axis of G, in binary64;
 *     J = (g_s, g_y, g_z, q_y g_z - q_z g_y, q_z g_s - q_s g_z, q_s g_y - q_y g_s)   in binary64,
 * the derivative of G(c_G + Rot(omega)(p - c_G) + t) by (t, omega) at zero.  out_host receives the sums over the counting voxels,
 * products and accumulation in binary64:  [0..20] the upper triangle of J^T J, row-major;  [21..26] J^T r;  [27] sum r^2;  [28] the
 * count;  [29..31] sum F^2, sum w^2, sum F w (for a normalised correlation).  No atomics, two stages in a fixed order: the same bits
 * from call to call.  With no counting voxel every sum is +0.0.
 * Both volumes are only read: no claim is dropped, and F and G may be two engines, two slots of one engine, or one and the same
 * slot.  With two engines the kernels run on the fixed engine's stream behind an event of the moving engine's stream, which then
 * waits for them; the call waits for its result.
 * TOMO_ERR_ARG: a null engine or pointer, a bad slot, different devices, a non-finite matrix entry, margin < 0 or 2 * margin >= a
 * size of F.  TOMO_ERR_STATE: an engine bound to a communicator, one that is a slab of a larger volume, or one whose geometry was
 * released.  A refused call has enqueued nothing and leaves both engines usable. */
int tomo_volume_affine_normal(tomo_engine *fixed, int fixed_vol, tomo_engine *moving, int moving_vol, const double *m_host /* [12] */,
                              int margin, double *out_host /* [32] */);   /* waits */

/* ---- DART: discrete tomography for objects made of a few known grey levels ----------------------------------------------------
 * K. J. Batenburg, J. Sijbers, "DART: a practical reconstruction algorithm for discrete tomography", IEEE Trans. Image Process.
 * 20(9), 2011, pp. 2542-2553.  The reference has no DART; these calls are its building blocks on the resident volume, and
 * TomoGPU.dart (reconstructor.py) is the loop: segment -> fix the interior at its grey level -> SIRT on the free voxels -> smooth.
 * A voxel v = (s, y, z) of a volume has slice s in [0, Nslice) and y, z in [0, N).  Neighbours are NOT periodic (unlike the TV
 * calls): a neighbour outside the volume does not exist.  The engine owns one STATE byte per voxel, made by tomo_dart_classify and
 * used by the other calls: bits 0-3 label, bit 6 boundary, bit 7 free.
 *   tomo_dart_classify: label(v) = the number of thresholds t_i, i < nthr, with x(v) >= t_i, compared in binary32 (NaN: 0; +Inf:
 *       nthr).  0 <= nthr <= 15, thresholds finite and strictly ascending.  boundary(v) = some existing neighbour w of v has
 *       label(w) != label(v); connectivity 6 = the faces, 26 = faces, edges and corners.  free(v) = boundary(v) || h(v) <
 *       free_threshold with h(v) = mix(mix(idx) ^ seed), idx = (s N + y) N + z in uint32 arithmetic and
 *       mix(a): a ^= a >> 16; a *= 0x7feb352d; a ^= a >> 15; a *= 0x846ca68b; a ^= a >> 16  -- a counter-based draw: the same set for
 *       the same seed on any machine; free_threshold = 0 gives no random voxels, p * 2^32 a fraction p of them.  The numbers of free
 *       and of boundary voxels land in TOMO_S_DART_FREE / TOMO_S_DART_BOUNDARY as exact integers.  Reads `vol`; enqueued, no wait.
 *   tomo_dart_restore:  x(v) = grey_host[label(v)] where v is not free; a free voxel keeps its bits.  nlevels = the state's nthr + 1.
 *   tomo_dart_segment:  the same for EVERY voxel, free or not: the volume then holds only the grey levels (the final segmentation).
 *   tomo_dart_arm:      niter x { one iteration of tomo_sirt_data(e, vol, sino_b, 1) (the ASTRA SIRT step of tomoengine::SIRT,
 *       gpu/utils/tomoengine.cpp:189-205); tomo_dart_restore }: SIRT whose fixed voxels are put back to their grey level after EVERY
 *       iteration, so the residual of the fixed part is absorbed by the free voxels alone.  The SIRT kernels are the ones of
 *       tomo_sirt_data, untouched.  Enqueued without a host wait.
 *   tomo_dart_smooth:   dst(v) = fma(beta, m - x, x) for a free voxel, x = src(v), m = (the sum of the existing 26 neighbours of v in
 *       src) * (1 / count): the sum in binary32 from the first term in ascending (dy, dz, ds) order without the centre, free and fixed
 *       neighbours alike, 1 / count rounded once to binary32; a fixed voxel copies the bits of src.  src != dst, 0 <= beta <= 1.
 *   tomo_dart_class_stats: out_host[c] = {sum of x(v), number of v} over the voxels with label(v) = c, c <= nthr (the label rule of
 *       tomo_dart_classify for the thresholds given here; no state is needed or changed), in binary64, added in a fixed order in two
 *       stages.  A voxel that is not finite is COUNTED in its class but NOT summed (the mean of the finite ones stays usable).  Waits.
 *   tomo_dart_get_state: the state bytes as [Nslice][Ny][Nz].  Waits.
 * Hence, bit for bit: tomo_dart_arm with every voxel free (free_threshold = 2^32 - 1 leaves out only h = 2^32 - 1) gives the bits of
 * tomo_sirt_data(e, vol, sino_b, niter); with no voxel free it leaves a restored volume as it is; beta = 0 copies src; an Inf
 * beside a fixed voxel never makes it NaN; the same state, counts, sums and volumes from run to run.  The pitch padding of a volume
 * is written as zero and of the state as 0, and no sample at slice index >= Nslice enters a result.
 * Bookkeeping: a volume written by restore, segment, arm or smooth counts as written (as after tomo_set_volume: its version moves on
 * and a claim "G = A * vol" is dropped); classify and class_stats only read.
 * One whole-volume engine only (a slab would need its neighbours' label planes): TOMO_ERR_STATE for an engine bound to a
 * communicator or whose geometry was released, and for restore, segment, arm, smooth or get_state before any classify.
 * TOMO_ERR_ARG: a null pointer, a bad slot, src == dst, nthr outside 0..15, nlevels != the state's nthr + 1, thresholds that are not
 * finite and strictly ascending, connectivity other than 6 or 26, beta not in [0, 1] (NaN included), niter < 0, or
 * Nslice * N * N >= 2^32.  A refused call has enqueued nothing and leaves the engine usable. */
int tomo_dart_classify(tomo_engine *e, int vol, const float *thr_host, int nthr, int connectivity,
                       uint32_t seed, uint32_t free_threshold);
int tomo_dart_restore(tomo_engine *e, int vol, const float *grey_host, int nlevels);
int tomo_dart_segment(tomo_engine *e, int vol, const float *grey_host, int nlevels);
int tomo_dart_arm(tomo_engine *e, int vol, int sino_b, int niter, const float *grey_host, int nlevels);
int tomo_dart_smooth(tomo_engine *e, int src, int dst, float beta);
int tomo_dart_class_stats(tomo_engine *e, int vol, const float *thr_host, int nthr, double *out_host); /* [nthr+1][2], waits */
int tomo_dart_get_state(tomo_engine *e, uint8_t *out_host);  /* [Nslice][Ny][Nz], waits */

/* ---- Connected components of a thresholded volume: labels, per-component measurements, removal of components ----------------------
 * The reference has no counterpart (its users label the downloaded volume on the host); these calls close the workflow on the
 * resident volume, and TomoGPU.label_particles (reconstructor.py) is the driver.  A voxel v = (s, y, z) as for the DART calls;
 * its public linear index is p = (s N + y) N + z.
 *   foreground: fg(v) = lo <= x(v) && x(v) <= hi, compared in binary32: a NaN voxel is never foreground; lo = -Inf and hi = +Inf are
 *       allowed.  The pitch padding of a volume is never foreground and never read.
 *   connectivity: 6 = the faces, 26 = faces, edges and corners.  Neighbours are NOT periodic.
 *   numbering: the components are numbered 1..K in ascending order of their smallest p; background is 0 (the numbering of
 *       scipy.ndimage.label).  The rule fixes every label whatever the order in which the kernels' atomics arrive.
 *   tomo_components_label: labels slot `vol` (read only) into the engine's label state -- one int32 per voxel, a root count per
 *       256 voxels and K records, allocated here and kept -- and returns K in *count.  Waits.
 *   tomo_components_get_labels: the labels as [Nslice][Ny][Nz] int32.  Waits.
 *   tomo_components_stats: records 1..min(K, capacity) in component order; nothing beyond them is written.  All fields are integers,
 *       hence exact in any order of accumulation: voxels; sum_s, sum_y, sum_z (the centroid is sum / voxels, formed by the host);
 *       the bounding box min_* .. max_* (inclusive); first = the component's smallest p; surface = the number of its voxels with at
 *       least one of the SIX face neighbours background or outside the volume, whatever connectivity labelled it.  The measurements
 *       are taken by the first call after a labelling and kept with it.  Sums of intensities are not offered: a floating-point sum
 *       over an arbitrary voxel set has no fixed order without a sort.  Waits.
 *   tomo_components_keep: x(v) = fill where label(v) > 0 && !keep_host[label(v)]; every other voxel keeps its bits (it is not
 *       written).  n must be K + 1 (entry 0, the background's, is not read).  The label state is NOT changed: label again for
 *       contiguous numbers.  Enqueued, no wait; the table goes through the staging buffer in stream order.
 *   tomo_components_release: frees the label state (4 bytes per voxel); allowed on any engine, a no-op without a state.
 * The same labels, K and records from run to run and on a used engine as on a fresh one.
 * TOMO_ERR_STATE: get_labels, stats or keep without a labelling; an engine bound to a communicator, or one whose geometry was
 * released (one whole-volume engine only, as for the DART calls: the Python classes refuse slabs of a larger volume before the call).
 * TOMO_ERR_ARG: a null engine or pointer, a bad slot, connectivity other than 6 or 26, a NaN bound or lo > hi, n != K + 1, a negative
 * capacity, or Nslice * N * N >= 2^31 (label + 1 must fit int32).  A refused call has enqueued and allocated nothing. */
typedef struct tomo_component {
    int64_t voxels, sum_s, sum_y, sum_z, surface, first;
    int32_t min_s, min_y, min_z, max_s, max_y, max_z;
} tomo_component;                                            /* 72 bytes; _lib.COMPONENT_DTYPE mirrors it */
int tomo_components_label(tomo_engine *e, int vol, float lo, float hi, int connectivity, int64_t *count);   /* waits */
int tomo_components_get_labels(tomo_engine *e, int32_t *labels_host);   /* [Nslice][Ny][Nz], waits */
int tomo_components_stats(tomo_engine *e, int64_t capacity, tomo_component *records_host);   /* waits */
int tomo_components_keep(tomo_engine *e, int vol, const uint8_t *keep_host, int64_t n, float fill);
int tomo_components_release(tomo_engine *e);
int tomo_read_scalars(tomo_engine *e, double *out, int count);          /* synchronises the stream */
/* the same without a pipeline bubble: _snapshot enqueues the copy of all slots behind the kernels that produce them (and behind
 * an evaluation in flight on the second stream) and returns; _read waits for that copy only.  The ASD-POCS drivers enqueue the
 * next SART sweep in between (the scalars of iteration i decide nothing before the TV steps of iteration i+1:
 * examples/sim_ASD.py:90-94). */
int tomo_scalars_snapshot(tomo_engine *e);
int tomo_scalars_snapshot_read(tomo_engine *e, double *out, int count);
/* Pending work and the other reduction users.  Three things can be in flight between two calls: a tomo_scalars_snapshot not yet read,
 * a tomo_data_distance_sq_async not yet waited for, and the scalars of a tomo_tv_gd_tracked whose read-back the host has deferred
 * (a snapshot).  tomo_dart_classify, tomo_dart_class_stats, tomo_sino_moments, tomo_sino_xcorr, tomo_sino_affine_normal and tomo_sino_axis_profile may be called
 * while any of them is: none refuses, none cancels the pending item or changes what it delivers, and both sides deliver what the
 * un-interleaved order delivers, bit for bit.  They run on the engine's stream behind everything enqueued so far; a snapshot is a copy that was
 * enqueued BEFORE them, so it keeps the slot values of that moment (TOMO_S_DART_* of a later classify are not in it); the evaluation
 * on the second stream owns its own partial sums and only TOMO_S_DD, which none of the six writes, and the alignment calls (which
 * may read TOMO_SINO_G) first order the engine's stream behind it.  The six C calls leave the evaluation pending.  tomo_read_scalars, however,
 * implies tomo_async_wait, as stated above: a host that fetches TOMO_S_DART_* with it after tomo_dart_classify (the Python wrapper
 * does) has thereby COMPLETED the evaluation -- its TOMO_S_DD is the same value -- and a later tomo_async_wait is a no-op.  Only ONE snapshot can
 * be pending: a second tomo_scalars_snapshot replaces the first. */
int tomo_bind_scalar_buffer(tomo_engine *e, void *device_doubles);      /* >= TOMO_S_COUNT doubles, e.g. a torch tensor */

/* ---- 3-D total variation ---------------------------------------------------------------------------- */
/* Slices of a slab have neighbours on other ranks: two device buffers of Nray*Nray floats hold the slice
 * below the first local slice (lo) and above the last (hi).  tomo_halo_local fills them from this slab
 * (periodic wrap = single-rank behaviour of ctvlib.cpp:348,421-422); a distributed caller packs, exchanges
 * (mpi_ctvlib.cpp:400-422) and leaves the received planes in the bound buffers. */
int tomo_bind_halo(tomo_engine *e, void *device_lo, void *device_hi);
int tomo_halo_pack(tomo_engine *e, int field, int last, void *device_dst); /* field: tomo_volume or TOMO_FIELD_* */
int tomo_halo_pack_both(tomo_engine *e, int field, void *first_plane, void *last_plane);  /* both planes, one launch */
int tomo_halo_local(tomo_engine *e, int field);
enum tomo_field { TOMO_FIELD_FGP_D = 100, TOMO_FIELD_FGP_P1 = 101 };
/* Several slab engines on ONE device (a slab run as K sub-slabs, each with its own allocations and stream, so that their
 * dependent launch chains overlap): the three calls the coupling of the sub-slabs needs -- stream ordering, halo planes taken
 * straight from the neighbours' volumes (ring of sub-slabs = the periodic wrap of ctvlib.cpp:348,421; mpi_ctvlib.cpp:400-422
 * does it with MPI), and the sum of the engines' partial sums on the device (mpi_ctvlib.cpp:547 MPI_Allreduce).
 * "tv_gnorm_slot" (tomo_set_option) names the scalar slot the TV update reads ||g||^2 from. */
int tomo_wait_for(tomo_engine *e, tomo_engine *other);
int tomo_halo_from(tomo_engine *e, int field, tomo_engine *lo_src, tomo_engine *hi_src);
int tomo_scalar_sum_from(tomo_engine *e, int dst_slot, tomo_engine **srcs, int n, int src_slot);
/* global-edge flags for the non-periodic FGP stencil (tv_fgp.cu:57,81) */
int tomo_set_slab_edges(tomo_engine *e, int is_first, int is_last);

/* the volume the tv_gd / tv_grad / tv_update forms descend (default RECON): multimodal::tv_gd_4D runs the same descent
 * on every element's tomogram (multimodal.cpp:494, chemistry/utils/regularizers/tv_gd.cu:208-296) */
int tomo_tv_set_target(tomo_engine *e, int vol);
/* step forms (use the halo buffers as they are) */
int tomo_tv_partial(tomo_engine *e, int vol, float eps);                /* tv_gd.cu:27-47 -> TOMO_S_TV */
int tomo_tv_grad(tomo_engine *e, float eps);                            /* ctvlib.cpp:415-449 -> TOMO_S_GNORM */
/* the same pass, also the TV value of recon -> TOMO_S_TV (tv_gd.cu:177-183: the value "before descent") */
int tomo_tv_grad_tv(tomo_engine *e, float eps);
int tomo_tv_update(tomo_engine *e, float dPOCS, int clamp);             /* ctvlib.cpp:452-458 (+461 when clamp) */
/* the same step, also leaving the new first and last slice in two device planes (N*N floats each): what the ring
 * exchange of the slab-sharded descent sends before the next gradient pass, without a gather launch */
int tomo_tv_update_planes(tomo_engine *e, float dPOCS, int clamp, void *first_plane, void *last_plane);
/* one communication round per inner iteration instead of two (mpi_ctvlib.cpp:400-422 exchanges the slices, :455 reduces the
 * norm): the norm pass also leaves the gradient's first / last slice in device buffers; they travel with the all-reduce of
 * sum g^2, and every rank advances its halo planes itself (same expression as the update pass, same bits) */
int tomo_tv_grad_planes(tomo_engine *e, float eps, int with_tv, void *g_first, void *g_last);
int tomo_tv_halo_apply(tomo_engine *e, float dPOCS, int clamp, const void *g_lo, const void *g_hi);
/* the same step, also ||recon_new - track_vol||^2 -> scalar `slot` and track_vol = recon_new (sim_ASD.py:86-88) */
int tomo_tv_update_tracked(tomo_engine *e, float dPOCS, int clamp, int track_vol, int slot);
int tomo_fgp_begin(tomo_engine *e);                                     /* tv_fgp.cu:216-227 */
int tomo_fgp_begin_vol(tomo_engine *e, int vol);                        /* one element of cuda_tv_fgp_4D (chemistry/.../tv_fgp.cu:192) */
int tomo_fgp_obj(tomo_engine *e, float lambda);                         /* :44-65 + :143-154 */
int tomo_fgp_grad(tomo_engine *e, float lambda);                        /* :67-115 */
int tomo_fgp_end(tomo_engine *e, int iters);                            /* :272 */
/* Fused FGP iteration, step form: Obj + nonneg + Grad + Proj of tv_fgp.cu:244-268 in one pass (28 instead of 48
 * bytes per voxel) with ONE ring exchange per iteration when the volume is slab-sharded.  Caller-owned device planes
 * (Nray*Nray floats each): lo = P1 of the slice below this slab; hi = 4 planes {A, P1, P2, P3} of the slice above;
 * send_first = the same 4 planes of this slab's first slice and send_last = P1 of its last slice, written by
 * begin (A) and by every step (P) -- the caller exchanges send_last -> next.lo and send_first -> prev.hi before each
 * step and before end (tv_fgp.cu:57,81 need exactly these neighbours; mpi_ctvlib.cpp:400-422 is the reference ring). */
int tomo_bind_fgp_halo(tomo_engine *e, void *lo, void *hi, void *send_first, void *send_last);
/* The two-slice-deep set, for TWO fused iterations per pass on slabs (round 6; tv_fgp.cu:57,81 name the neighbours): lo 5 planes
 * [P1(-1), A(-1), P2(-1), P3(-1), P1(-2)], hi 8 planes [A, P1, P2, P3](nx), [A, P1, P2, P3](nx + 1), send_first 8 planes (my slices
 * 0 and 1: [A, P1, P2, P3] each), send_last 5 planes [P1(nx-1), A(nx-1), P2(nx-1), P3(nx-1), P1(nx-2)].  The one-deep planes above
 * are the prefixes (1 / 4 / 4 / 1 planes), so tomo_fgp_fused_step and _end run on the same buffers. */
int tomo_bind_fgp_halo2(tomo_engine *e, void *lo, void *hi, void *send_first, void *send_last);
int tomo_fgp_fused_begin(tomo_engine *e, int vol);
int tomo_fgp_fused_step(tomo_engine *e, float lambda, int first_iteration);
int tomo_fgp_fused_step2(tomo_engine *e, float lambda, int first_iteration);   /* TWO iterations in one pass (P stays on chip between
                                                                                * them; the same bits as two steps).  On a slab of a sharded
                                                                                * volume: tomo_bind_fgp_halo2, one two-deep exchange before
                                                                                * it, at least two slices on every slab of the ring */
int tomo_fgp_fused_end(tomo_engine *e, float lambda);                   /* the last iteration: D over the input volume */
int tomo_fgp_fused_last(tomo_engine *e, float lambda, int first_iteration);   /* one more step AND the end in one pass (the same bits);
                                                                               * whole-volume slabs only */

/* whole-call forms for a single slab (= the reference's single-GPU calls) */
int tomo_tv(tomo_engine *e, int vol, float eps);                        /* tomoengine.cpp:439-442 tv_3D -> TOMO_S_TV */
int tomo_tv_gd(tomo_engine *e, int ng, float dPOCS, float eps);         /* :445 tv_gd_3D; TV before descent -> TOMO_S_TV */
int tomo_tv_gd_tracked(tomo_engine *e, int ng, float dPOCS, float eps, int track_vol, int slot); /* last step tracked */
int tomo_tv_fgp(tomo_engine *e, int iters, float lambda);               /* :448-450 tv_fgp_3D; TV of input -> TOMO_S_TV */
int tomo_tv_fgp_vol(tomo_engine *e, int vol, int iters, float lambda);  /* multimodal.cpp:497 tv_fgp_4D, one element */

/* ---- Chambolle-Pock (PDHG) for  min_{x >= 0} 1/2 |Ax - b|^2 + lambda |grad x|_{2,1} ---------------------------------------
 * The reference's unfinished counterpart is gpu/utils/regularizers/tv_chambolle.cu (in its tree, not compiled); the arithmetic
 * here is this project's own.  Index convention x[s][y][z], the three axes alike, Neumann ends: (grad x)_a[i] = x[i + 1_a] - x[i]
 * where i_a < n_a - 1, else 0; (div p)[i] = sum_a p_a[i] - p_a[i - 1_a] with p_a[-1] = 0 and p_a = 0 at the last index of axis a
 * (written as 0 whatever was read), so <grad x, p> = <x, -div p> exactly.  One iteration (theta = 1 by default):
 *     g = A xbar;  q <- (q + S (g - b)) / (1 + S);  u = A^T q;
 *     p <- a / max(1, |a|_2 / lambda), a = p + s_grad grad xbar;  x_new = max(0, x - T (u - div p));  xbar <- x_new + theta (x_new - x)
 * precond = 0: S = s_grad = sigma, T = tau, tau sigma (L_A + 12) <= 1 (L_A = tomo_lipschitz, 12 >= |grad|^2).  precond = 1 (diagonal,
 * Pock-Chambolle 2011, alpha = 1): S_i = 1 / rowsum_i (0 for an empty ray), s_grad = 1/2, T_j = 1 / (colsum_j + d_j), d_j = the
 * difference rows that touch voxel j (0..6); sigma and tau are not read.
 * All four calls run on the engine's stream and never synchronise; they return TOMO_ERR_STATE on an engine with a communicator or
 * whose slab is not both first and last (tomo_set_slab_edges): a slab of a sharded volume has the tomo_pdhg_slab_* / tomo_comm_pdhg*
 * calls below, which read the neighbours' p and xbar from halo planes. */
/* step 1 on sinogram slots (q may be TOMO_SINO_USER0 + k); tv_chambolle.cu has no data term: the dual sinogram is new here */
int tomo_pdhg_sino_dual(tomo_engine *e, int q_sino, int g_sino, int b_sino, float sigma, int precond);
/* step 3 as ONE fused pass over caller-named volume slots (counterpart of the dual / primal kernels sketched in tv_chambolle.cu):
 * p lives in p_vol0 .. p_vol0 + 2 (axis s, y, z).  After the call the named slots hold the new fields, whatever buffers were swapped
 * underneath.  slot >= 0: also sum (x_new - x)^2 -> that scalar; -1: none.  44 bytes per voxel. */
int tomo_pdhg_tv_step(tomo_engine *e, int x_vol, int xbar_vol, int u_vol, int p_vol0, float sigma, float tau, float lambda,
                      float theta, int precond, int slot);
/* whole-call form (the loop tv_chambolle.cu was meant to drive): tomo_pdhg_begin sets p = 0, q = 0, xbar = RECON; tomo_pdhg runs niter
 * iterations on RECON, YK (xbar), TEMP (u), an engine-owned dual field and dual sinogram (TOMO_SINO_R holds A xbar), which are
 * kept across calls until the next begin.  Scalar mode: tau = ratio / sqrt(L_A + 12), sigma = 1 / (ratio sqrt(L_A + 12)).
 * slot: as above, of the last iteration. */
int tomo_pdhg_begin(tomo_engine *e);
int tomo_pdhg(tomo_engine *e, int niter, float lambda, float theta, int precond, float ratio, int slot);
/* ---- the same on a slab of a volume sharded along the tilt axis --------------------------------------------------------------
 * Only the fused pass couples slices (grad along s, div along s); the projections and the dual sinogram are slice-local.  The
 * neighbours' slices reach it through caller-owned device planes of Nray*Nray floats, dense [y][z] (the reference's sharded engine
 * exchanges whole boundary slices the same way: cpu/utils/mpi_ctvlib.cpp:400-422):
 *     lo          4 planes [xbar, p0, p1, p2] of the slice below this slab        hi         1 plane, xbar of the slice above
 *     send_last   4 planes [xbar, p0, p1, p2] of this slab's last slice           send_first 1 plane, xbar of its slice 0
 * The caller moves send_last -> next.lo and send_first -> prev.hi before each step: 5 N^2 floats per rank and iteration, one round.
 * The pass itself leaves the new boundary fields in the send planes (no pack launch per iteration); a neighbour's dual step is
 * re-evaluated from its planes with the same float32 operations, so the sharded result has the bits of the whole-volume pass.
 * A face flagged as the volume's end (tomo_set_slab_edges) reads and writes no plane.  An engine with a communicator that has bound
 * nothing gets planes of its own.  mpi_ctvlib.cpp:400-422 is the ring these replace. */
int tomo_bind_pdhg_halo(tomo_engine *e, void *lo, void *hi, void *send_first, void *send_last);
/* both send buffers from named volume slots (before the first step, or after a start from fields the pass did not write);
 * the boundary slices mpi_ctvlib.cpp:400-422 sends */
int tomo_pdhg_slab_pack(tomo_engine *e, int xbar_vol, int p_vol0);
/* tomo_pdhg_tv_step on a slab: same arguments and checks; honours the slab edges, reads lo / hi as they are (mpi_ctvlib.cpp:400-422
 * fills them), leaves the new boundary fields in the send buffers; `slot` receives THIS slab's partial sum.  A slab that is both first
 * and last needs no planes and gives the bits of tomo_pdhg_tv_step; TOMO_ERR_STATE where planes are needed and none are bound. */
int tomo_pdhg_slab_tv_step(tomo_engine *e, int x_vol, int xbar_vol, int u_vol, int p_vol0, float sigma, float tau, float lambda,
                           float theta, int precond, int slot);
/* tomo_pdhg_sino_dual on a slab (slice-local: no plane, no exchange) */
int tomo_pdhg_slab_sino_dual(tomo_engine *e, int q_sino, int g_sino, int b_sino, float sigma, int precond);
/* the state of tomo_pdhg_begin (p = 0, q = 0, xbar = RECON) plus the send buffers packed from it (mpi_ctvlib.cpp:400-422) */
int tomo_pdhg_slab_begin(tomo_engine *e);
/* ONE iteration of tomo_pdhg without the exchange, which the caller runs before it (mpi_ctvlib.cpp:400-422): forward projection of
 * xbar, dual sinogram, back projection, the fused slab pass.  Arguments as tomo_pdhg's; TOMO_ERR_STATE before tomo_pdhg_slab_begin.
 * The scalar step sizes come from the engine's L_A (tomo_lipschitz), which depends on the 2-D matrix only: every rank derives the
 * same sigma and tau without an all-reduce. */
int tomo_pdhg_slab_iter(tomo_engine *e, float lambda, float theta, int precond, float ratio, int slot);

/* ---- multimodal (ChemicalTomo) element-wise steps ---------------------------------------------------------
 * Two engines with the same slab shape on one device and stream: `ce` carries the chemical geometry and the
 * per-element tomograms, `he` the HAADF geometry, the model volume Sigma*x^gamma and the SIRT-updated model.
 * Sigma (fusion_helper.py:5-32) is pixel-diagonal with one weight per element, passed as w[nel]. */
int tomo_get_stream(tomo_engine *e, void **hip_stream);
int tomo_mm_model(tomo_engine *ce, const int32_t *xvols, int nel, const float *w, float gamma, tomo_engine *he,
                  int model_vol);                                       /* multimodal.cpp:425-427 */
int tomo_mm_update(tomo_engine *ce, const int32_t *xvols, const int32_t *uvols, int nel, const float *w, float gamma,
                   float lamC_over_L, float lamH, tomo_engine *he, int upd_vol, int model_vol); /* :435-438, :471-476 */

/* Engine options (A/B switches for measurement; defaults are the fast paths):
 *   "sart_fused" (1): run a SART sweep as FP(a0), [BP(a_k)+FP(a_k+1)] fused steps, BP(a_last) instead of separate
 *                     FP/BP launches per angle (same arithmetic per voxel; 8 instead of 12 bytes per voxel-angle)
 *   "tv_lds" (1):     TV gradient kernel: 1 = register march (one wave = 8 z-columns x 64 slices, rows in registers,
 *                     slice neighbours by DPP; bit-identical to the LDS march and 13 % faster), 8 / 16 = LDS march with that
 *                     many z-columns per workgroup, 0 = direct-global stencil
 *   "tv_recompute" (1): a tv_gd inner iteration as "norm pass (sum g^2, nothing stored) + update pass that re-evaluates g and writes
 *                     x_new into a second buffer" instead of "gradient pass (store g) + update pass (read x, g; write x)": one volume
 *                     write instead of two -- HBM writes are the scarce resource (3 TB/s against ~6 for reads); bit-identical
 *   "fgp_fused" (1):  one fused kernel per FGP iteration (single slab)
 *   "fgp_pair" (1):   ... and two iterations per pass where the slab is the whole volume (k_fgp_fused2: 28 bytes per voxel for two
 *                     iterations; the same bits); 0 = one iteration per pass
 *   "art_chain" (1):  tomo_art in natural row order as per-angle FP + ray recurrence + BP (k_art_chain) instead of
 *                     row-by-row steps (k_art, which still serves tomo_art_order with a permutation)
 *   "art_tile" (1):   the chained ART sweep as fused tile steps (BP of the previous angle + FP of the next in k_sart_tile's ART
 *                     form, k_art_chain between them) instead of k_fp_rows + k_art_chain + k_bp_art per angle: 19.2 against
 *                     26.0 ms per sweep at 512^3 x 90
 *   "sart_tile" (1):  fused SART steps on image tiles streamed through LDS (k_sart_tile, in place) instead of the ray-walk
 *                     form (k_sart_seg); equal at 512 slices per GPU, 14-18 % faster on slabs of <= 128 slices
 *   "sart_streams" (0): the SART sweep of a slab as two sub-slabs (64-slice chunks, equal halves) on two streams, the second
 *                     chain enqueued by a second host thread: slices are independent, each stream fills the other's launch
 *                     boundaries and residual-row kernels.  2 = whenever the slab has two chunks, 1 = never, 0 = automatic:
 *                     equal halves and not when a pixel's row of slices is a multiple of 4 KB (measured per ASD-POCS step:
 *                     -2.6 / -3.3 / -5.5 / -5.3 % at 128 / 256 / 512 / 768 slices, +13 % at 1024).  A sub-slab runs its per-row
 *                     kernels at the widest vector that fits its chunks; results are bit-identical to the one-chain sweep
 *   "sart_skip_same" (1): k_sart_tile (in place) leaves out the store of a 256-byte piece (pixel x 64 slices) whose bits did
 *                     not change (clamped zeros, zero residuals): same memory image, fewer HBM writes; gain depends on the data
 *   "sart_nt" (-1):   cache policy of k_sart_tile's voxel accesses: 1 = streamed (non-temporal loads, write-through
 *                     non-temporal stores: -9 % per sweep at 512^3), 0 = plain, -1 = streamed when the slab exceeds 192 MB
 *                     (a slab that fits the Infinity Cache is faster with plain accesses)
 *   "sart_coop" (0):  1 = the residual rows of an angle are formed inside the next tile step by its first workgroups
 *                     instead of one k_resid_finish launch per angle (bit-identical; measured no faster);
 *                     "sart_coop_spin" (4096): polls before a workgroup forms its rows itself (< 0: always, for tests)
 *   "tv_yseg" (0):    rows a wave of the TV register march walks; 0 = 32, shortened on thin slabs until >= 8192 waves
 *   "tv_march4" (1):  norm / update passes of tv_gd by k_tv_march4 (row slots renamed over a 4x unrolled loop, packed edge
 *                     values: no register rotation; -10 % per inner iteration, bit-identical) instead of k_tv_grad_reg
 *   "fp_tile" (1):    all-angle forward projection from LDS-resident image tiles (k_fp_tile + k_fp_tile_reduce);
 *                     0 = ray-driven form selected by "fp_all_lpr"
 *   "fp_tile_scratch_mib" (8192): cap of the tile projector's partial-sum scratch; a larger volume is projected in
 *                     several passes over groups of 64-slice chunks (set before the first projection)
 *   "fp_tile_chunks_per_pass" (0): that number of 64-slice chunks per pass instead (0 = derived from the cap)
 *   "bp_tile" (1):    all-angle back-projection from LDS-staged residual-row windows (k_bp_tile; bit-identical to the
 *                     pixel-driven k_bp_all it replaces; used when every tile's ray window fits, else k_bp_all)
 *   "bp_list" (1):    ... in its entry-list form (k_bp_list: one scalar-loaded entry per nonzero weight, accumulators picked by
 *                     the VGPR index mode; same bits) when the engine built the lists ("bp_list_ready" of tomo_get_option) and
 *                     the slab is a whole number of 128-slice pieces; 0 = k_bp_tile
 *   "fp_all_lpr" (16): ray-driven all-angle forward projection with 16 lanes x float4 per ray and 64-slice chunks
 *                     (0 = wide form)
 *   "fp_reuse" (1):   a tomo_sirt / tomo_sirt_data / tomo_cgls call whose volume is exactly what the model sinogram was last
 *                     projected from (tomo_forward_projection into TOMO_SINO_G, tomo_data_distance_sq; tracked by slot and
 *                     write-version, inherited by tomo_copy_volume) starts from that sinogram instead of projecting again:
 *                     bit-identical.  Also gates tomo_fista_project_yk.  0 = every projection recomputed
 *   "fp_strip" (1):   all-angle forward projection by sheared strips with the ray sums resident in registers (k_fp_strip) when the
 *                     engine built the strip tables (large slabs; "fp_strip_ready" of tomo_get_option); setting "fp_tile"
 *                     explicitly also sets "fp_strip" = 0, so that the tile / ray-driven forms can be selected
 *   "fp_list" (1):    ... the strips as wave-uniform entry lists (k_fp_list: one angle per wave, one accumulator per ray picked by
 *                     the VGPR index mode) when the engine built them ("fp_list_ready": where the strips are built and a tile's
 *                     work spreads evenly enough over the waves; TOMO_FP_LIST = 0 / 1 overrides) and the slab is a whole number
 *                     of 128-slice pieces; 0 = k_fp_strip
 *   "sart_resident" (-1): the SART sweep as ONE launch of the volume-resident kernel (k_sart_resident: a 64-slice chunk of the whole
 *                     image stays in vector registers over all angles, the workgroups exchange ray sums).  -1 = automatic: wherever
 *                     the tables exist ("sart_resident_ready": N a multiple of 8, at most one 32 x 32 tile per CU, ray windows that
 *                     fit, the tile tables of the streamed chain built too); after a sweep that could not finish (below) the form sits
 *                     out 1, 2, 4 ... 64 sweeps before it is tried again.  0 = never (the streamed chain k_sart_tile), 1 = insist:
 *                     an error where the tables do not exist, no sitting out.  Setting it clears the sitting-out state.
 *                     FAIL-SAFE: every workgroup of the launch must be on the chip at once.  Where that cannot happen (another
 *                     process or a long kernel of the caller holds CUs) the waits run out, the affected 64-slice chunks are NOT
 *                     stored -- a chunk is stored by all of its workgroups or by none -- and tomo_sart / tomo_sart_tracked sweep
 *                     them with the streamed chain before they return: the call returns TOMO_OK with the sweep done (the
 *                     reference's sweep either happens or errors before touching recon, tomoengine.cpp:162-179).  The call waits
 *                     for the launch on the host (that is what knowing costs: ~10 us per sweep)
 *   "sart_resident_spin" (2097152): polls (~1 us each) a wait of the resident sweep makes before it gives up; < 0 = the default,
 *                     0 = every wait gives up at its first unsuccessful look (tests)
 *   "sart_resident_test_fail" (0): tests: chunk + 1 whose first workgroup refuses to commit (that chunk goes to the streamed chain) */
int tomo_set_option(tomo_engine *e, const char *name, int value);
/* read back a switch, or a fact about the engine: "fp_strip", "fp_list", "fp_tile", "bp_tile", "bp_list", "fgp_pair", "fp_reuse", "sart_tile", and
 * "fp_list_ready" (1: the list form of the strips was built),
 * "art_chain_ready" (1: every pixel's two rays of an angle are neighbours, so a natural-order ART sweep runs as the chain, k_art_chain,
 * where "art_chain" = 1; 0: it runs row by row, k_art),
 * "bp_list_ready" (1: the entry lists of k_bp_list were built: every tile's ray windows fit and there are at most 192 angles),
 * "fp_strip_ready" (1: the sheared-strip tables were built at creation -- by the slab-size rule or TOMO_FP_STRIP=1 -- so
 * "fp_strip" = 1 takes effect), "fp_strip_slots" (accumulator slots per lane group the strip kernel runs with),
 * "comm_rounds" (RCCL rounds -- one ncclGroup or one lone collective each -- this engine has enqueued since creation),
 * "rccl_version" (ncclGetVersion's code of the librccl the library opened, e.g. 22707; 0 before the first communicator),
 * "sart_resident", "sart_resident_ready" (the tables of the volume-resident SART sweep were built), "sart_resident_active"
 * (ready and not switched off), "sart_resident_spin", "sart_resident_fallbacks" (sweeps of this engine that needed the streamed chain
 * for chunks the resident launch did not store), "sart_resident_fallback_chunks" (how many 64-slice chunks that were),
 * "sart_resident_skip" (sweeps the resident form still sits out), "sart_resident_last_code" (what the last give-up waited for:
 * 1 residual rows, 2 tile sums, 0 the commit),
 * "table_kib" (device memory of the tables built at creation: every kernel family's, eagerly), "create_ms" (what creation took),
 * "stage_bytes" (bytes of the staging buffer the HOST data calls copy through, clamped to 2^31 - 1; 0 = never allocated: the device
 * data calls, tomo_set_volume_device ..., neither allocate nor use it),
 * "pool_bytes" (the sizes of every live device allocation of the engine's registry, summed and clamped to 2^31 - 1: two engines of one
 * geometry that made the same calls with the same sizes hold the same number, in whatever order the sizes came -- a scratch buffer
 * that is regrown is released first, none is held twice; an engine that holds 2 GiB or more reads as 2^31 - 1, where an equality of
 * two engines says nothing),
 * "form_fp" / "form_bp" / "form_sart": which kernel family the all-angle forward projection, the all-angle back projection and the
 * SART sweep of THIS engine run as under the options in force (tomo_form; one function of the engine decides it for the launchers
 * and for this query: tomo_engine.hip select_forms) */
typedef enum { TOMO_FORM_FP_ROWS = 0, TOMO_FORM_FP_TILE = 1, TOMO_FORM_FP_STRIP = 2, TOMO_FORM_FP_LIST = 3,
               TOMO_FORM_BP_ALL = 0, TOMO_FORM_BP_TILE = 1, TOMO_FORM_BP_LIST = 2,
               TOMO_FORM_SART_ANGLE = 0, TOMO_FORM_SART_TILE = 1, TOMO_FORM_SART_RESIDENT = 2 } tomo_form;
int tomo_get_option(tomo_engine *e, const char *name, int *value);
/* ---- native communicator: the slab-sharded path over RCCL on the engine's own stream ---------------------------------------
 * Replaces, for a C / C++ host as for the Python one, the MPI calls of the reference's sharded CPU engine (mpi_ctvlib.cpp:400-422
 * ring exchange of boundary slices, :455 / :547 MPI_Allreduce of the norms) and the OpenMP-over-GPUs loop of multigpuengine.cpp:
 * one engine per rank holding rank's slab (tomo_create with the slab's slice count), one communicator shared by the rank's
 * engines.  librccl is opened with dlopen on first use.  Rank 0 makes the 128-byte id and hands it to the others by any means
 * (MPI_Bcast, torch.distributed.broadcast, a file); tomo_comm_init is collective over the group. */
int tomo_comm_unique_id(void *id128);
int tomo_comm_init(tomo_engine *e, const void *id128, int world, int rank);   /* also sets the slab's global-edge flags */
int tomo_comm_share(tomo_engine *e, tomo_engine *other);                       /* another engine of the same rank and device */
int tomo_comm_destroy(tomo_engine *e);
int tomo_comm_info(tomo_engine *e, int *world, int *rank);                     /* world = 0: no communicator */
/* boundary slices of a field into the ring neighbours' halo planes: pack + ONE group of 2 sends and 2 receives */
int tomo_comm_exchange_halo(tomo_engine *e, int field);
/* every scalar slot summed over the ranks (into a copy: the buffer keeps the slab's partial sums), read back; and the
 * non-blocking form collected by tomo_scalars_snapshot_read */
int tomo_comm_read_scalars(tomo_engine *e, double *out, int count);
int tomo_comm_scalars_snapshot(tomo_engine *e);
/* slab-sharded tv_gd / tv_gd_tracked (track_vol < 0: plain), whole call: per inner iteration ONE group {all-reduce of sum g^2 +
 * the gradient's boundary planes to both neighbours}; every rank advances its halo planes itself.  TOMO_S_TV keeps the slab's
 * share of the TV value before descent. */
int tomo_comm_tv_gd(tomo_engine *e, int ng, float dPOCS, float eps, int track_vol, int slot);
/* the plane exchange between two fused FGP iterations (buffers of tomo_bind_fgp_halo) */
int tomo_comm_fgp_exchange(tomo_engine *e);
/* ... and before a PAIR of them (tomo_fgp_fused_step2 on slabs): the two-slice-deep planes of tomo_bind_fgp_halo2, one round per two iterations */
int tomo_comm_fgp_exchange2(tomo_engine *e);
/* the plane exchange before an iteration of the slab-sharded Chambolle-Pock loop (buffers of tomo_bind_pdhg_halo, or the engine's
 * own): ONE group, 1 plane towards prev and 4 towards next -- the ring of mpi_ctvlib.cpp:400-422 */
int tomo_comm_pdhg_exchange(tomo_engine *e);
/* slab-sharded tomo_pdhg, whole call: niter x {that exchange, tomo_pdhg_slab_iter} on the engine's stream (mpi_ctvlib.cpp:400-422 per
 * iteration); `slot` keeps this slab's partial sum of the last iteration.  TOMO_ERR_STATE without a communicator or before
 * tomo_pdhg_slab_begin. */
int tomo_comm_pdhg(tomo_engine *e, int niter, float lambda, float theta, int precond, float ratio, int slot);

/* launch chains a SART / ART sweep of this engine's slab runs as under the current "sart_streams" (1 = one chain on the
 * engine's stream; 2..4 = that many sub-slabs of 64-slice chunks on their own streams).  What the reference hides inside
 * ASTRA's run(Nproj*nIter) (tomoengine.cpp:162-179); bench.py derives the bytes one launch moves from it. */
int tomo_sart_chain_count(tomo_engine *e, int *count);

/* ---- measurement hooks (bench.py) -------------------------------------------------------------------
 * While enabled, every launch of the named kernel is bracketed by HIP events on the engine's stream (on = N > 1: every N-th
 * launch only -- an event pair costs about 3 us of command-processor time, 0.7 ms per ASD-POCS step when all ~210 launches of
 * a step are bracketed); tomo_profile_read synchronises, returns the count and summed device time of the bracketed launches,
 * and resets the log. */
enum tomo_kernel_id { TOMO_K_BP_ANGLE = 0, TOMO_K_FP_ANGLE = 1, TOMO_K_TV_GRAD = 2, TOMO_K_TV_UPDATE = 3,
                      TOMO_K_FGP_OBJ = 4, TOMO_K_FGP_GRAD = 5 /* also the fused FGP iteration */, TOMO_K_SART_FUSED = 6,
                      TOMO_K_FP_TILE = 7, TOMO_K_BP_TILE = 8, TOMO_K_FP_REDUCE = 9,
                      TOMO_K_SART_RESIDENT = 10 /* one launch = one whole SART sweep of the slab (volume-resident form) */,
                      TOMO_K_PDHG_TV = 11 /* the fused pass of a Chambolle-Pock iteration */ };
int tomo_profile_enable(tomo_engine *e, int kernel, int on);
int tomo_profile_read(tomo_engine *e, int kernel, int64_t *launches, double *total_ms);
/* the same, also busy_ms = time during which at least one launch of the kernel was executing (union of the launch
 * intervals): the SART sweep runs as two sub-slabs on two streams ("sart_streams"), so two launches of a kernel overlap */
int tomo_profile_read2(tomo_engine *e, int kernel, int64_t *launches, double *total_ms, double *busy_ms);
/* launch intervals [t0, t1) in ms on the time base of ref_engine's log (engines of a slab group); cap = 0 only counts */
int tomo_profile_intervals(tomo_engine *e, int kernel, tomo_engine *ref_engine, double *t0, double *t1, int cap, int *count);

#ifdef __cplusplus
}
#endif
#endif /* TOMO_HIP_H */
