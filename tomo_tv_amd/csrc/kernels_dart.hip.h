// kernels_dart.hip.h -- DART discrete tomography (Batenburg & Sijbers, IEEE Trans. Image Process. 20(9), 2011): segmentation into grey
// levels with the label-boundary stencil and the random free set, masked restore, masked 3 x 3 x 3 smoother, per-class sums
// Part of kernels.hip.h (include that, not this).
//
// Volumes are [y][z][s], slice s fastest, pitch sx a multiple of 64 floats; the state buffer is one byte per voxel with the same
// [pix][sx] indexing: bits 0-3 the label, bit 6 boundary, bit 7 free.  The slices nx .. sx-1 of a row are padding: every kernel here
// writes them as zero (volumes) or as state 0, and none takes a sample at s >= nx into a result (by a select, never a product with 0).
// Neighbours are NOT periodic: unlike the TV kernels a neighbour outside [0, nx) x [0, n) x [0, n) does not exist.
//
// The two stencils (k_dart_classify, k_dart_smooth) keep the structure of k_tv_march4: lane = slice, a wave owns one 64-slice chunk and
// TZ z-columns (+ one column on either side) and marches along y with three rows in registers whose roles rotate by name; the s -/+ 1
// neighbours are wave shifts (DPP), and what lies beyond the chunk's two edges comes from the adjacent chunk through one packed
// register per row and edge (lane j = column j), read with v_readlane into the shift's `old` operand.
// The same bits from run to run: every volume element is one fixed sequence of operations and the class sums are added in a fixed
// order in two stages.  The one exception to "fixed order" are the two COUNTS of k_dart_classify, which go through block_accumulate
// like the engine's other scalars (one binary64 atomicAdd per workgroup, in arrival order): the addends are integers whose total is
// below 2^32, so every partial sum is exact and the order cannot show.
#pragma once

namespace tomo {

enum { DART_LABEL_MASK = 15, DART_BOUNDARY = 64, DART_FREE = 128 };
struct DartThr { float t[15]; };      // thresholds, strictly ascending; entries >= nthr are not read
struct DartGrey { float g[16]; };     // grey level of every label

__device__ __forceinline__ uint32_t dart_mix(uint32_t a)
{
    a ^= a >> 16; a *= 0x7feb352du; a ^= a >> 15; a *= 0x846ca68bu; a ^= a >> 16;
    return a;
}

// label(v) = #{i < nthr : v >= t_i} for K values at once (a NaN compares false: 0; +Inf: nthr).  The thresholds are wave-uniform
// kernel arguments; the loop over them is the outer one, so a threshold is fetched once for the K compares.
template <int K> __device__ __forceinline__ void dart_labels(const float (&v)[K], int (&lab)[K], const DartThr &thr, int nthr)
{
#pragma unroll
    for (int k = 0; k < K; ++k) lab[k] = 0;
#pragma unroll
    for (int i = 0; i < 15; ++i) {
        if (i >= nthr) break;
        const float t = thr.t[i];
#pragma unroll
        for (int k = 0; k < K; ++k) lab[k] += v[k] >= t ? 1 : 0;
    }
}

__device__ __forceinline__ int dart_shr(int old, int v) { return __builtin_amdgcn_update_dpp(old, v, 0x138, 0xf, 0xf, false); }   // lane l <- l-1; lane 0 keeps old
__device__ __forceinline__ int dart_shl(int old, int v) { return __builtin_amdgcn_update_dpp(old, v, 0x130, 0xf, 0xf, false); }   // lane l <- l+1; lane 63 keeps old

// the wave's work item: 64-slice chunk bs, z-block bz, y-segment ys
__device__ __forceinline__ bool dart_item(int n, int sx, int yseg, int tz, int &bs, int &bz, int &ys)
{
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int nzb = (n + tz - 1) / tz, nchunk = sx >> 6, nys = (n + yseg - 1) / yseg;
    const int64_t item = (int64_t)blockIdx.x * 4 + wave;
    bs = (int)(item % nchunk); bz = (int)((item / nchunk) % nzb); ys = (int)(item / ((int64_t)nchunk * nzb));
    return ys < nys;
}

// ---- k_dart_classify -------------------------------------------------------------------------------------------------------
// state(v) = label | boundary << 6 | free << 7 with
//   boundary(v) = some EXISTING C-neighbour w (C = 6: faces; 26: faces, edges, corners) has label(w) != label(v)
//   free(v)     = boundary(v) || h(v) < free_threshold,   h(v) = mix(mix(idx) ^ seed),   idx = (s N + y) N + z as uint32
// and the number of free and of boundary voxels summed into part_free / part_bnd (block_accumulate: integers below 2^32, exact
// in binary64 in any order; the launcher's k_finalize makes the scalars).
//
// One pass over x: a value is labelled once, when its row is loaded.  The label travels as the pair p = {label, 15 - label} of
// 16-bit halves, so that ONE packed minimum (v_pk_min_u16) carries both the minimum and the maximum label of a neighbourhood, and
// the neighbourhood is separable: along s when the row is loaded (two wave shifts), along z once per row, along y per output --
// boundary <=> min != max <=> lo + hi != 15.  A neighbour that does not exist is left out: along s the voxel's own pair stands in for
// it (neutral: it is part of the minimum anyway), along z and y the term is skipped under a wave-uniform condition.
typedef unsigned short dart_p2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ dart_p2 dart_pmin(dart_p2 a, dart_p2 b) { return __builtin_elementwise_min(a, b); }
__device__ __forceinline__ int dart_pi(dart_p2 a) { return __builtin_bit_cast(int, a); }
__device__ __forceinline__ dart_p2 dart_ip(int a) { return __builtin_bit_cast(dart_p2, a); }

template <int C>
__global__ __launch_bounds__(256) void k_dart_classify(const float *__restrict__ x, uint8_t *__restrict__ state, DartThr thr, int nthr,
                                                       uint32_t seed, uint32_t free_threshold, int n, int nx, int sx, int yseg,
                                                       double *__restrict__ part_free, double *__restrict__ part_bnd)
{
    static_assert(C == 6 || C == 26, "connectivity");
    constexpr int TZ = 8;
    const int lane = threadIdx.x & 63;
    int bs, bz, ys;
    uint32_t nfree = 0, nbnd = 0;
    if (dart_item(n, sx, yseg, TZ, bs, bz, ys)) {
        const int y0 = ys * yseg, y1 = min(y0 + yseg, n);
        const int z0 = bz * TZ, s0 = bs * 64, s = s0 + lane;
        const bool lo_in = s0 > 0, hi_in = s0 + 64 < nx;        // the slice below / above the chunk exists
        const int zl = z0 - 1 + lane;                           // the column whose edge values this lane gathers (lane < TZ + 2)
        const bool zl_ok = lane < TZ + 2 && zl >= 0 && zl < n;
        // a row in registers: E = the voxels' own pairs (columns 1 .. TZ), G = what the row gives to an output of its column when it
        // is the centre row (C = 26: also when it is the row above or below, where C = 6 takes E)
        dart_p2 E0[TZ], E1[TZ], E2[TZ], G0[TZ], G1[TZ], G2[TZ];
        float raw[TZ + 4];                                      // the next row as loaded: columns 0 .. TZ+1, then the two packed edges
        auto fetch = [&](int y) __attribute__((always_inline)) {
            const float *rowp = x + (size_t)y * n * sx;
#pragma unroll
            for (int j = 0; j < TZ + 2; ++j) {
                const int z = z0 - 1 + j;
                raw[j] = (z >= 0 && z < n) ? rowp[(size_t)z * sx + (unsigned)s] : 0.f;
            }
            raw[TZ + 2] = (lo_in && zl_ok) ? rowp[(size_t)zl * sx + (unsigned)(s0 - 1)] : 0.f;
            raw[TZ + 3] = (hi_in && zl_ok) ? rowp[(size_t)zl * sx + (unsigned)(s0 + 64)] : 0.f;
        };
        // raw -> E, G of the row
        auto digest = [&](dart_p2 *E, dart_p2 *G) __attribute__((always_inline)) {
            int lab[TZ + 4];
            dart_labels<TZ + 4>(raw, lab, thr, nthr);
            dart_p2 e[TZ + 2], es[TZ + 2];
            const int pe = lab[TZ + 2] | (15 - lab[TZ + 2]) << 16, pf = lab[TZ + 3] | (15 - lab[TZ + 3]) << 16;
#pragma unroll
            for (int j = 0; j < TZ + 2; ++j) {
                const int ei = lab[j] | (15 - lab[j]) << 16;
                e[j] = dart_ip(ei);
                if (C == 6 && (j == 0 || j == TZ + 1)) continue;                    // the outer columns only give their own pair
                const int left = dart_shr(lo_in ? __builtin_amdgcn_readlane(pe, j) : ei, ei);
                int right = dart_shl(hi_in ? __builtin_amdgcn_readlane(pf, j) : ei, ei);
                if (!hi_in) right = s + 1 < nx ? right : ei;                        // the ragged chunk: slice s + 1 is padding
                es[j] = dart_pmin(e[j], dart_pmin(dart_ip(left), dart_ip(right)));
            }
#pragma unroll
            for (int j = 1; j <= TZ; ++j) {
                dart_p2 g = es[j];
                if (z0 + j - 2 >= 0) g = dart_pmin(g, C == 26 ? es[j - 1] : e[j - 1]);
                if (z0 + j < n) g = dart_pmin(g, C == 26 ? es[j + 1] : e[j + 1]);
                E[j - 1] = e[j]; G[j - 1] = g;
            }
        };
        // one step of the march: row yn (loaded by the step before) is digested into (En, Gn), row yn + 1 is requested, and row yn - 1
        // (Ec, Gc), which now has both neighbours (Em, Gm) and (En, Gn), is written
        auto step = [&](int yn, dart_p2 *En, dart_p2 *Gn, const dart_p2 *Ec, const dart_p2 *Gc, const dart_p2 *Em, const dart_p2 *Gm)
                        __attribute__((always_inline)) {
            if (yn >= 0 && yn < n) digest(En, Gn);
            if (yn + 1 <= y1 && yn + 1 < n) fetch(yn + 1);
            const int y = yn - 1;
            if (y < y0) return;
            const bool up = y > 0, dn = y + 1 < n;
#pragma unroll
            for (int j = 0; j < TZ; ++j) {
                const int z = z0 + j;
                if (z >= n) break;
                dart_p2 f = Gc[j];
                if (up) f = dart_pmin(f, C == 26 ? Gm[j] : Em[j]);
                if (dn) f = dart_pmin(f, C == 26 ? Gn[j] : En[j]);
                const uint32_t lab = Ec[j].x;
                const bool bnd = (uint32_t)f.x + (uint32_t)f.y != 15u;
                const uint32_t idx = ((uint32_t)s * (uint32_t)n + (uint32_t)y) * (uint32_t)n + (uint32_t)z;
                const bool fr = bnd || dart_mix(dart_mix(idx) ^ seed) < free_threshold;
                const bool real = s < nx;
                state[((size_t)y * n + z) * sx + (unsigned)s] = real ? (uint8_t)(lab | (bnd ? DART_BOUNDARY : 0) | (fr ? DART_FREE : 0)) : (uint8_t)0;
                nbnd += real && bnd; nfree += real && fr;
            }
        };
        int yn = y0 - 1;
        if (yn < 0) yn = y0;             // no row above the volume: the first step digests row y0 and writes nothing (y0 - 1 < y0)
        fetch(yn);
        for (; yn <= y1; yn += 3) {
            step(yn, E0, G0, E2, G2, E1, G1);
            if (yn + 1 <= y1) step(yn + 1, E1, G1, E0, G0, E2, G2);
            if (yn + 2 <= y1) step(yn + 2, E2, G2, E1, G1, E0, G0);
        }
    }
    block_accumulate((double)nfree, part_free);
    __syncthreads();
    block_accumulate((double)nbnd, part_bnd);
}

// ---- k_dart_restore --------------------------------------------------------------------------------------------------------
// x(v) = grey[label(v)] where v is not free (ALL: everywhere -- the final segmentation); a free voxel keeps its bits; padding = 0.
// Four slices per thread: one 4-byte load of the state, one 16-byte load and store of x.  The grey levels sit in LDS (a per-lane
// index into a kernel argument would go through scratch).
template <bool ALL>
__global__ __launch_bounds__(256) void k_dart_restore(float *__restrict__ x, const uint8_t *__restrict__ state, DartGrey grey, int64_t nvec,
                                                      int nx, int sx)
{
    __shared__ float g[16];
    if (threadIdx.x == 0) {
#pragma unroll
        for (int c = 0; c < 16; ++c) g[c] = grey.g[c];
    }
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * 256) {
        const int s = (int)((i * 4) % sx);
        const uint32_t st = reinterpret_cast<const uint32_t *>(state)[i];
        VecOf<4>::T v = reinterpret_cast<VecOf<4>::T *>(x)[i];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t b = (st >> (8 * k)) & 255u;
            if (ALL || !(b & DART_FREE)) v[k] = g[b & DART_LABEL_MASK];
            if (s + k >= nx) v[k] = 0.f;
        }
        reinterpret_cast<VecOf<4>::T *>(x)[i] = v;
    }
}

// ---- k_dart_smooth (src != dst) ----------------------------------------------------------------------------------------------
// free voxel:  dst = fma(beta, m - x, x),  m = (sum of the existing 26 neighbours of src) * (1 / count)
// fixed voxel: dst = the bits of src;  padding: 0.
// The sum runs in binary32 from the first term in ascending (dy, dz, ds) order without the centre, free and fixed neighbours alike;
// count = ny nz ns - 1 with n. = the 1, 2 or 3 positions that exist along that axis, and 1 / count is rounded once (__fdiv_rn).  A
// neighbour that does not exist enters the sum as +0.  That leaves every bit of dst as if it had been skipped: a + 0 == a for every
// a but -0, so the two sums can only differ in the sign of a sum that is zero, m then is a zero of either sign, and for x != 0
// m - x == -x either way while for x == +-0 fma(beta, +-0, x) with beta >= 0 is +0 unless every term is -0 in both forms.
// A voxel without any neighbour (a 1 x 1 x 1 volume) is copied.  The result of a fixed voxel is a select of the source value, so an
// Inf beside it (whose sum is Inf or NaN) cannot reach it.
constexpr int DART_SMOOTH_TZ = 4;     // z-columns per wave: three rows x (TZ + 2) columns x {s-1, s, s+1} live in registers
template <int TZ>
__global__ __launch_bounds__(256) void k_dart_smooth(const float *__restrict__ x, float *__restrict__ dst, const uint8_t *__restrict__ state,
                                                     float beta, int n, int nx, int sx, int yseg)
{
    const int lane = threadIdx.x & 63;
    int bs, bz, ys;
    if (!dart_item(n, sx, yseg, TZ, bs, bz, ys)) return;
    const int y0 = ys * yseg, y1 = min(y0 + yseg, n);
    const int z0 = bz * TZ, s0 = bs * 64, s = s0 + lane;
    const bool lo_in = s0 > 0, hi_in = s0 + 64 < nx, real = s < nx;
    const int zl = z0 - 1 + lane;
    const bool zl_ok = lane < TZ + 2 && zl >= 0 && zl < n;
    const int ns = 1 + (s > 0) + (s + 1 < nx);
    // a row in registers: the values of columns 0 .. TZ+1 at slices s-1, s, s+1 (0 where the voxel does not exist)
    float L0[TZ + 2], C0[TZ + 2], R0[TZ + 2], L1[TZ + 2], C1[TZ + 2], R1[TZ + 2], L2[TZ + 2], C2[TZ + 2], R2[TZ + 2];
    float raw[TZ + 4];
    auto fetch = [&](int y) __attribute__((always_inline)) {
        const float *rowp = x + (size_t)y * n * sx;
#pragma unroll
        for (int j = 0; j < TZ + 2; ++j) {
            const int z = z0 - 1 + j;
            raw[j] = (real && z >= 0 && z < n) ? rowp[(size_t)z * sx + (unsigned)s] : 0.f;
        }
        raw[TZ + 2] = (lo_in && zl_ok) ? rowp[(size_t)zl * sx + (unsigned)(s0 - 1)] : 0.f;
        raw[TZ + 3] = (hi_in && zl_ok) ? rowp[(size_t)zl * sx + (unsigned)(s0 + 64)] : 0.f;
    };
    auto digest = [&](bool exists, float *L, float *Cc, float *R) __attribute__((always_inline)) {
        const int pe = __builtin_bit_cast(int, raw[TZ + 2]), pf = __builtin_bit_cast(int, raw[TZ + 3]);
#pragma unroll
        for (int j = 0; j < TZ + 2; ++j) {
            const int c = __builtin_bit_cast(int, raw[j]);
            // (hi_in false: lane 63 takes +0 -- slice s0 + 64 does not exist; a lane whose slice s + 1 is padding shifts in the 0 loaded there)
            const int l = dart_shr(__builtin_amdgcn_readlane(pe, j), c), r = dart_shl(__builtin_amdgcn_readlane(pf, j), c);
            L[j] = exists ? __builtin_bit_cast(float, l) : 0.f;
            Cc[j] = exists ? raw[j] : 0.f;
            R[j] = exists ? __builtin_bit_cast(float, r) : 0.f;
        }
    };
    auto step = [&](int yn, float *Ln, float *Cn, float *Rn, const float *Lc, const float *Cc, const float *Rc, const float *Lm,
                    const float *Cm, const float *Rm) __attribute__((always_inline)) {
        digest(yn >= 0 && yn < n, Ln, Cn, Rn);
        if (yn + 1 <= y1 && yn + 1 < n) fetch(yn + 1);
        const int y = yn - 1;
        if (y < y0) return;
        const int ny = 1 + (y > 0) + (y + 1 < n);
#pragma unroll
        for (int j = 1; j <= TZ; ++j) {
            const int z = z0 + j - 1;
            if (z >= n) break;
            const int nz = 1 + (z > 0) + (z + 1 < n);
            float acc = 0.f;
            acc += Lm[j - 1]; acc += Cm[j - 1]; acc += Rm[j - 1];
            acc += Lm[j]; acc += Cm[j]; acc += Rm[j];
            acc += Lm[j + 1]; acc += Cm[j + 1]; acc += Rm[j + 1];
            acc += Lc[j - 1]; acc += Cc[j - 1]; acc += Rc[j - 1];
            acc += Lc[j]; acc += Rc[j];
            acc += Lc[j + 1]; acc += Cc[j + 1]; acc += Rc[j + 1];
            acc += Ln[j - 1]; acc += Cn[j - 1]; acc += Rn[j - 1];
            acc += Ln[j]; acc += Cn[j]; acc += Rn[j];
            acc += Ln[j + 1]; acc += Cn[j + 1]; acc += Rn[j + 1];
            const int count = ny * nz * ns - 1;
            const float xc = Cc[j];
            const float m = __fmul_rn(acc, __fdiv_rn(1.f, (float)count));
            const float sm = __fmaf_rn(beta, __fsub_rn(m, xc), xc);
            const size_t at = ((size_t)y * n + z) * sx + (unsigned)s;
            const bool fr = (state[at] & DART_FREE) != 0 && count > 0;
            dst[at] = real ? (fr ? sm : xc) : 0.f;
        }
    };
    int yn = y0 - 1;
    if (yn < 0) yn = y0;                 // no row above the volume: the first step digests row y0 against a row of zeros (ny = 2)
    fetch(yn);
#pragma unroll
    for (int j = 0; j < TZ + 2; ++j) { L1[j] = C1[j] = R1[j] = 0.f; L2[j] = C2[j] = R2[j] = 0.f; }
    for (; yn <= y1; yn += 3) {
        step(yn, L0, C0, R0, L2, C2, R2, L1, C1, R1);
        if (yn + 1 <= y1) step(yn + 1, L1, C1, R1, L0, C0, R0, L2, C2, R2);
        if (yn + 2 <= y1) step(yn + 2, L2, C2, R2, L1, C1, R1, L0, C0, R0);
    }
}

// ---- k_dart_class_stats ------------------------------------------------------------------------------------------------------
// out[c] = {sum of x, count} over the real voxels of class c (the label rule of k_dart_classify), in binary64.  A voxel that is not
// finite is counted in its class (NaN: class 0; +Inf: the last; -Inf: class 0) but NOT summed: one such voxel would otherwise
// make the mean of its class useless.
// Two stages in a fixed order (kernels_geom.hip.h): a thread adds the voxels it strides over in ascending order into acc[c][2] =
// {sum, count}, the workgroup's sums go to part[block][c][2] (block_sum_row) and k_sum_rows_tree adds the workgroups' rows.
constexpr int DART_STATS_BLOCKS = 1024;

template <int NC>
__global__ __launch_bounds__(256) void k_dart_class_stats(const float *__restrict__ x, DartThr thr, int nthr, int64_t nvec, int nx, int sx,
                                                          double *__restrict__ part)
{
    double acc[2 * NC];
#pragma unroll
    for (int k = 0; k < 2 * NC; ++k) acc[k] = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * 256) {
        const int s = (int)((i * 4) % sx);
        const VecOf<4>::T q = reinterpret_cast<const VecOf<4>::T *>(x)[i];
        const float v[4] = {q[0], q[1], q[2], q[3]};
        int lab[4];
        dart_labels<4>(v, lab, thr, nthr);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const bool real = s + k < nx;
            const double a = (real && fabsf(v[k]) < INFINITY) ? (double)v[k] : 0.0;
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                const bool in = real && lab[k] == c;
                acc[2 * c] += in ? a : 0.0;
                acc[2 * c + 1] += in ? 1.0 : 0.0;
            }
        }
    }
    block_sum_row<2 * NC>(acc, part + (size_t)blockIdx.x * 32);
}

// ---- k_dart_state_out: the state buffer [pix][sx] as the host's [Nslice][Ny][Nz] bytes ------------------------------------------
// a workgroup moves 64 pixels x 64 slices through LDS (pitch 65 bytes)
__global__ __launch_bounds__(256) void k_dart_state_out(const uint8_t *__restrict__ state, uint8_t *__restrict__ out, int64_t npix, int nx, int sx)
{
    __shared__ uint8_t tile[64][65];
    const int64_t p0 = (int64_t)blockIdx.x * 64;
    const int s0 = blockIdx.y * 64, c = threadIdx.x & 63, r = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int64_t p = p0 + 4 * k + r;
        tile[4 * k + r][c] = p < npix ? state[(size_t)p * sx + s0 + c] : (uint8_t)0;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int s = s0 + 4 * k + r;
        const int64_t p = p0 + c;
        if (s < nx && p < npix) out[(size_t)s * npix + p] = tile[c][4 * k + r];
    }
}

}  // namespace tomo
