// kernels_bin.hip.h -- resampling between a fine grid and a grid F times coarser (F = 2 or 4): binning of sinograms and volumes,
// trilinear prolongation of volumes
// Part of kernels.hip.h (include that, not this).
//
// Both layouts are [row][slice] with the slice index fastest and a pitch that is a multiple of 64 floats; buffers are 256-byte
// aligned.  The slices nx .. pitch-1 of a row are padding: every kernel here writes them as zero in its destination and none takes a
// source sample at slice index >= nx into a result (the guard is a select, not a product with 0, so an Inf or NaN in the padding would
// not reach a sum).  No atomics, no LDS; every output element is one fixed sequence of binary32 operations, so the bits are the same
// from run to run.
//
// Scale (include/tomo_hip.h has the derivation): a coarse voxel is the MEAN of its F x F x k fine voxels; a coarse sinogram sample is
// the mean of its F x k fine samples divided by F, because the coarse matrix measures chord lengths in coarse pixels.  k = F for a
// full bin and k = Nslice - F s' < F for the trailing partial one; both means are (sum) * 1 / (F^2 k).
#pragma once

namespace tomo {

// 1 / (F^2 k) rounded to binary32, k in 1 .. F: constants the compiler folds (1/48 at F = 4, k = 3 is the only inexact one)
template <int F> __device__ __forceinline__ float bin_scale(int k)
{
    return k == 1 ? 1.f / (F * F) : k == 2 ? 1.f / (F * F * 2) : k == 3 ? 1.f / (F * F * 3) : 1.f / (F * F * 4);
}

// the F consecutive fine slices F s' .. F s' + F - 1 of a row as one 8- or 16-byte load (the pitch is a multiple of 64 floats and
// F s' + F <= pitch wherever s' is a real coarse slice, so the load is aligned and inside the row); v[j] for j >= k is not used
template <int F> __device__ __forceinline__ void bin_load(const float *__restrict__ p, float (&v)[F])
{
    if constexpr (F == 2) { const float2 q = *reinterpret_cast<const float2 *>(p); v[0] = q.x; v[1] = q.y; }
    else { const float4 q = *reinterpret_cast<const float4 *>(p); v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w; }
}

// ---- sinogram: dst_a[r'][s'] = c(s') * sum_{i < F} sum_{j < k(s')} src_a[F r' + i][F s' + j],  c = 1 / (F^2 k) -----------------------
// Lane = coarse slice; a wave takes one destination row (coarse row d = a * Nc + r' reads the fine rows F d .. F d + F - 1, because
// N = F Nc), a workgroup four consecutive rows.  Per fine row a wave reads 64 F consecutive floats (512 B or 1 KiB) and writes 256 B.
// The sum runs in binary32 in ascending (i, j) order from the first sample, then one multiply by c.
template <int F>
__global__ __launch_bounds__(256) void k_sino_bin(const float *__restrict__ src, float *__restrict__ dst, int64_t rows_c, int nx_f, int sx_f,
                                                  int nx_c, int sx_c)
{
    const int lane = threadIdx.x & 63, sc = blockIdx.y * 64 + lane;
    const int64_t d = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (d >= rows_c || sc >= sx_c) return;
    float o = 0.f;
    if (sc < nx_c) {
        const int k = min(F, nx_f - F * sc);
        const float *p = src + (size_t)(F * d) * sx_f + F * sc;
        float acc = 0.f;
#pragma unroll
        for (int i = 0; i < F; ++i) {
            float v[F];
            bin_load<F>(p + (size_t)i * sx_f, v);
#pragma unroll
            for (int j = 0; j < F; ++j) if (j < k) acc += v[j];
        }
        o = acc * bin_scale<F>(k);
    }
    dst[(size_t)d * sx_c + sc] = o;
}

// ---- volume: dst[y'][z'][s'] = the mean of src[F y' + i][F z' + j][F s' + l], i, j < F, l < k(s') -----------------------------------
// Lane = coarse slice; a wave takes one coarse pixel (y', z'), i.e. F^2 fine rows.  Ascending (y, z, s) order in binary32, then one
// multiply by 1 / (F^2 k).
template <int F>
__global__ __launch_bounds__(256) void k_volume_bin(const float *__restrict__ src, float *__restrict__ dst, int n_c, int nx_f, int sx_f,
                                                    int nx_c, int sx_c)
{
    const int lane = threadIdx.x & 63, sc = blockIdx.y * 64 + lane;
    const int64_t d = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (d >= (int64_t)n_c * n_c || sc >= sx_c) return;
    float o = 0.f;
    if (sc < nx_c) {
        const int yc = (int)(d / n_c), zc = (int)(d - (int64_t)yc * n_c), n_f = F * n_c;
        const int k = min(F, nx_f - F * sc);
        float acc = 0.f;
#pragma unroll
        for (int i = 0; i < F; ++i)
#pragma unroll
            for (int j = 0; j < F; ++j) {
                float v[F];
                bin_load<F>(src + ((size_t)(F * yc + i) * n_f + (F * zc + j)) * sx_f + F * sc, v);
#pragma unroll
                for (int l = 0; l < F; ++l) if (l < k) acc += v[l];
            }
        o = acc * bin_scale<F>(k);
    }
    dst[(size_t)d * sx_c + sc] = o;
}

// ---- prolongation: cell-centred trilinear interpolation with clamp-to-edge ------------------------------------------------------
// Per axis the fine index i sits at u = (i + 0.5) / F - 0.5 of the coarse grid; its taps are floor(u) and floor(u) + 1, clamped to the
// coarse range, its weight t = u - floor(u) (1/4 or 3/4 at F = 2, an odd eighth at F = 4: exact).  A lerp is fma(t, b - a, a); where
// the clamp makes both taps the same sample the sample is copied (the same bits for finite values, and an Inf stays an Inf instead of
// Inf - Inf).  Applied along s, then z, then y.  The trailing coarse slice is an ordinary cell even where it averaged fewer than F fine
// slices.
//
// The fine indices F g - F/2 .. F g + F/2 - 1 of an axis share the taps (g - 1, g), g in 0 .. Nc: a wave takes one such group (gy, gz)
// and 64 fine slices, loads the two s-taps of the four coarse rows once, forms the four s-lerps once and writes the up to F^2 fine rows
// of the group from them -- the re-use of the coarse rows is in registers.  Lane = fine slice: neighbouring lanes read the same or
// neighbouring coarse samples (64 / F + 1 distinct floats per row and wave), served by one or two cache lines.
template <int F> __device__ __forceinline__ void prolong_axis(int i, int nc, int &a, int &b, float &t)
{
    const float u = ((float)i + 0.5f) * (1.f / F) - 0.5f, fl = floorf(u);
    t = u - fl;
    a = min(max((int)fl, 0), nc - 1);
    b = min(max((int)fl + 1, 0), nc - 1);
}
__device__ __forceinline__ float prolong_lerp(float t, float a, float b, bool same) { return same ? a : fmaf(t, b - a, a); }

template <int F>
__global__ __launch_bounds__(256) void k_volume_prolong(const float *__restrict__ src, float *__restrict__ dst, int n_c, int nx_c, int sx_c,
                                                        int nx_f, int sx_f)
{
    const int lane = threadIdx.x & 63, s = blockIdx.y * 64 + lane, ng = n_c + 1, n_f = F * n_c;
    const int64_t g = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (g >= (int64_t)ng * ng || s >= sx_f) return;
    const int gy = (int)(g / ng), gz = (int)(g - (int64_t)gy * ng);
    const int ya = max(gy - 1, 0), yb = min(gy, n_c - 1), za = max(gz - 1, 0), zb = min(gz, n_c - 1);
    float v[2][2] = {{0.f, 0.f}, {0.f, 0.f}};
    const bool real = s < nx_f;
    if (real) {
        int sa, sb; float ts;
        prolong_axis<F>(s, nx_c, sa, sb, ts);
#pragma unroll
        for (int iy = 0; iy < 2; ++iy)
#pragma unroll
            for (int iz = 0; iz < 2; ++iz) {
                const float *row = src + ((size_t)(iy ? yb : ya) * n_c + (iz ? zb : za)) * sx_c;
                v[iy][iz] = prolong_lerp(ts, row[sa], row[sb], sa == sb);
            }
    }
#pragma unroll
    for (int py = -F / 2; py < F / 2; ++py) {
        const int y = F * gy + py;
        if (y < 0 || y >= n_f) continue;
        int a0, b0; float ty;
        prolong_axis<F>(y, n_c, a0, b0, ty);
#pragma unroll
        for (int pz = -F / 2; pz < F / 2; ++pz) {
            const int z = F * gz + pz;
            if (z < 0 || z >= n_f) continue;
            int a1, b1; float tz;
            prolong_axis<F>(z, n_c, a1, b1, tz);
            float o = 0.f;
            if (real) {
                const float lo = prolong_lerp(tz, v[0][0], v[0][1], a1 == b1), hi = prolong_lerp(tz, v[1][0], v[1][1], a1 == b1);
                o = prolong_lerp(ty, lo, hi, a0 == b0);
            }
            dst[((size_t)y * n_f + z) * sx_f + s] = o;
        }
    }
}

}  // namespace tomo
