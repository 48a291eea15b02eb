// kernels_geom.hip.h -- what the geometry families share (alignment, per-projection matching, 3-D resampling, registration, DART class
// sums): the split of a coordinate into tap and fraction, the bilinear and the trilinear value, the workgroup's sum of its threads'
// binary64 accumulators, and the two second stages that add the workgroups' rows.  Each rule is stated here once.
// Part of kernels.hip.h (include that, not this; it stands before kernels_align.hip.h).
#pragma once

namespace tomo {

// ---- the axis split -------------------------------------------------------------------------------------------------------------
// A binary64 coordinate c is split into k = floor(c) and the fraction c - k in binary64; only the fraction is rounded to binary32, and
// a fraction that rounds to 1 (c just below a whole number) is the next whole sample: first tap k + 1, t = 0.  The taps are i and
// i + 1 with the weights (1 - t, t).  The host's al_split (engine_align.inc) applies the same rule to -shift.
// What is accepted differs, and the difference is behaviour:
//   SPLIT_ZERO_PAD         c in (-1, size): at least one tap can lie inside [0, size), the others read as 0 (k_sino_affine,
//                          k_volume_affine).  Outside that range there is no tap, and no conversion to int (a NaN lands there).
//   SPLIT_INSIDE           both taps inside, judged AFTER the split: c in (-1, size), then 0 <= i and i + 1 <= size - 1.  A c in
//                          [-2^-25, 0) is sample 0 with t = 0 and is taken (k_sino_affine_normal).
//   SPLIT_INSIDE_FROM_ZERO both taps inside, c judged BEFORE the split: c in [0, size), then i + 1 <= size - 1.  A c in [-2^-25, 0)
//                          is refused (k_volume_affine_normal).
enum SplitRule { SPLIT_ZERO_PAD, SPLIT_INSIDE, SPLIT_INSIDE_FROM_ZERO };

template <SplitRule RULE> __device__ __forceinline__ bool axis_split(double c, int size, int &i, float &t)
{
    if (!((RULE == SPLIT_INSIDE_FROM_ZERO ? c >= 0.0 : c > -1.0) && c < (double)size)) return false;
    const double f = floor(c);
    t = (float)(c - f);
    i = (int)f;
    if (t >= 1.f) { t = 0.f; ++i; }
    if constexpr (RULE == SPLIT_ZERO_PAD) return true;
    return (RULE == SPLIT_INSIDE_FROM_ZERO || i >= 0) && i + 1 <= size - 1;
}

// the same with the weights in place of the fraction: w = (1 - t, t), and where t = 0 the second tap is not kept (two = false) and
// w[0] = 1 exactly
template <SplitRule RULE> __device__ __forceinline__ bool axis_split(double c, int size, int &i, float w[2], bool &two)
{
    float t;
    if (!axis_split<RULE>(c, size, i, t)) return false;
    two = t != 0.f;
    w[0] = two ? 1.f - t : 1.f;
    w[1] = t;
    return true;
}

// ---- the bilinear value of k_sino_shift and k_sino_affine -----------------------------------------------------------------------
// fetch(i, j) is the sample at row i, slice j (0, or the wrapped sample, outside the image: the caller's rule).  A zero fraction drops
// its second tap altogether, so a whole-pixel position copies the source value -- no 1 * x + 0 * y, which would turn an Inf next to x
// into NaN.  Plain operators: the compiler contracts products and sums into fused multiply-adds as it sees fit, and since both
// kernels instantiate this one expression they get the same contraction -- a pure translation through k_sino_affine has the bits of
// k_sino_shift by construction.  (k_sino_affine_normal evaluates the same formula without contraction: other bits.)
template <class Fetch> __device__ __forceinline__ float bilinear_value(Fetch &&fetch, int i, int j, float tr, float ts)
{
    if (tr == 0.f && ts == 0.f) return fetch(i, j);
    if (tr == 0.f) return (1.f - ts) * fetch(i, j) + ts * fetch(i, j + 1);
    if (ts == 0.f) return (1.f - tr) * fetch(i, j) + tr * fetch(i + 1, j);
    const float wr = 1.f - tr, ws = 1.f - ts;
    return (wr * ws) * fetch(i, j) + (wr * ts) * fetch(i, j + 1) + (tr * ws) * fetch(i + 1, j) + (tr * ts) * fetch(i + 1, j + 1);
}

// ---- the trilinear value of k_volume_affine and k_volume_affine_normal ------------------------------------------------------------
// tap(dy, dz, ds) is the sample at the first tap plus (dy, dz, ds); w* and k* are the weights and the "second tap kept" flags of
// axis_split.  The kept taps are combined in ascending (dy, dz, ds) order, ds fastest, every operation rounded once:
//     o = ((wy[0] * wz[0]) * ws[0]) * x[0][0][0];   then for every further kept tap   o = fmaf((wy[dy] * wz[dz]) * ws[ds], x, o)
// A tap that is not kept is not asked for, and three zero fractions copy the bits of the one tap.
template <class Tap>
__device__ __forceinline__ float trilinear_value(Tap &&tap, const float (&wy)[2], const float (&wz)[2], const float (&ws)[2], bool ky, bool kz,
                                                 bool ks)
{
    if (!ks && !ky && !kz) return tap(0, 0, 0);
    float o = __fmul_rn(__fmul_rn(__fmul_rn(wy[0], wz[0]), ws[0]), tap(0, 0, 0));
#pragma unroll
    for (int k = 1; k < 8; ++k) {
        const int dy = k >> 2, dz = (k >> 1) & 1, ds = k & 1;
        if ((dy && !ky) || (dz && !kz) || (ds && !ks)) continue;
        o = __fmaf_rn(__fmul_rn(__fmul_rn(wy[dy], wz[dz]), ws[ds]), tap(dy, dz, ds), o);
    }
    return o;
}

// ---- two-stage sums in a fixed order ----------------------------------------------------------------------------------------------
// No kernel of these families adds floats atomically: a thread adds its terms in index order in binary64, the workgroup adds its
// threads, a second kernel adds the workgroups.  The same bits from run to run.
//
// First stage, the workgroup's end: all 256 threads call it with their K sums.  Each sum goes through the wave tree (wave_sum), then
// the four waves are added in ascending order, ((w0 + w1) + w2) + w3, and thread k writes row[k]: one writer per value.
template <int K> __device__ __forceinline__ void block_sum_row(const double (&acc)[K], double *__restrict__ row)
{
    static_assert(K <= 256, "one thread per value");
    __shared__ double red[4][K];
    const int w = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const double v = wave_sum(acc[k]);
        if ((threadIdx.x & 63) == 0) red[w][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < K) {
        const int k = threadIdx.x;
        row[k] = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
    }
}

// Second stage for part[group][nblk][K]: out[g][k] = the group's rows added in ascending order, one thread per (g, k).  With mean
// set, mean[g] = out[g][0] / count rounded to binary32 (the moments: what the correlation subtracts while staging).
__global__ void k_sum_rows_ascending(const double *__restrict__ part, double *__restrict__ out, int groups, int nblk, int K,
                                     float *__restrict__ mean, double count)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= groups * K) return;
    const int g = i / K, k = i - K * g;
    double s = 0.0;
    for (int b = 0; b < nblk; ++b) s += part[((size_t)g * nblk + b) * K + k];
    out[i] = s;
    if (mean && k == 0) mean[g] = (float)(s / count);
}

// Second stage for part[nblk][stride] with many rows: one workgroup of 256 threads per output o = blockIdx.x; thread t adds the rows
// t, t + 256, ... in ascending order, then the threads are added as in block_sum_row.
__global__ __launch_bounds__(256) void k_sum_rows_tree(const double *__restrict__ part, double *__restrict__ out, int nblk, int stride)
{
    double v[1] = {0.0};
    for (int b = threadIdx.x; b < nblk; b += 256) v[0] += part[(size_t)b * stride + blockIdx.x];
    block_sum_row<1>(v, out + blockIdx.x);
}

}  // namespace tomo
