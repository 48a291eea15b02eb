// kernels_condition.hip.h -- conditioning of a tilt series on the sinogram layout: window statistics (the background of
// cpu/utils/logger.py:255-263), outlier removal by a local median, per-projection gain and offset
// Part of kernels.hip.h (include that, not this; it stands after kernels_geom.hip.h, whose two-stage sums it uses).
//
// The conventions are those of kernels_align.hip.h: projection a of a sinogram is the image X_a[r][s], ray r in [0, N), slice s in
// [0, Nslice): device row a * N + r, slice fastest, pitch sx.  The slices Nslice .. sx-1 are padding: never read as data, written as
// zero.  Lane = slice.  The sums are two-stage sums in a fixed order (block_sum_row, then k_sum_rows_ascending or
// k_window_stats_finish): no floating-point atomics, the same bits from call to call.
#pragma once
#include <utility>

namespace tomo {

// ---- the selection network --------------------------------------------------------------------------------------------------------
// Batcher's merge exchange (Knuth, TAOCP 5.2.2, Algorithm M) for n keys, generated at compile time as a list of compare-exchange
// pairs (lo, hi), lo < hi: after the list v[0] <= ... <= v[n-1].  The median kernel reads v[n / 2] only, and since a compare-exchange
// is one min and one max on registers, the halves that never reach that output are dead code to the compiler: what is left is a
// selection, not a sort.  A value that comes out is one of the values that went in (min and max pick, they never average).
struct ExchangeNet { int count; int lo[256], hi[256]; };

constexpr ExchangeNet merge_exchange(int n)
{
    ExchangeNet net{};
    int t = 0;
    while ((1 << t) < n) ++t;
    for (int p = t > 0 ? 1 << (t - 1) : 0; p > 0; p >>= 1) {
        int q = 1 << (t - 1), r = 0, d = p;
        for (;;) {
            for (int i = 0; i + d < n; ++i)
                if ((i & p) == r) { net.lo[net.count] = i; net.hi[net.count] = i + d; ++net.count; }
            if (q == p) break;
            d = q - p; q >>= 1; r = p;
        }
    }
    return net;
}

template <int N> struct NetOf { static constexpr ExchangeNet net = merge_exchange(N); };

template <int LO, int HI, int N> __device__ __forceinline__ void compare_exchange(float (&v)[N])
{
    static_assert(0 <= LO && LO < HI && HI < N, "a pair of the network");
    const float a = v[LO], b = v[HI];
    v[LO] = fminf(a, b);
    v[HI] = fmaxf(a, b);
}
template <int N, size_t... I> __device__ __forceinline__ void apply_net(float (&v)[N], std::index_sequence<I...>)
{
    (compare_exchange<NetOf<N>::net.lo[I], NetOf<N>::net.hi[I], N>(v), ...);
}
// the median of the N values (N odd); v is used up
template <int N> __device__ __forceinline__ float median_of(float (&v)[N])
{
    static_assert(N % 2 == 1 && N <= 25, "an odd window that the pair list holds");
    apply_net<N>(v, std::make_index_sequence<NetOf<N>::net.count>{});
    return v[N / 2];
}

// ---- local median: measure, or replace the outliers -------------------------------------------------------------------------------
// m = the median of the W x W samples around (r, s) of projection a, W = 2 R + 1, indices clamped to [0, N) x [0, Nslice): the border
// is replicated, projections never mix, slice Nslice - 1 never sees a padding slice.  d = x - m, one binary32 subtraction.  Per
// projection, in binary64 from the first sample: sum d, sum |d|, sum d^2 (the square a binary64 product of the converted d), the
// number of samples and the number replaced.  With REPLACE, dst = (|d| > thresh[a]) ? m : x, compared in binary32, and the padding
// slices of dst are written as zero; without it nothing but the sums is written.
//
// The form: workgroup (chunk, row block, a) takes 64 slices of MD_ROWS rays; each wave marches along r over
// MD_ROWS / 4 rays with the W rows of its window in registers (W x W values per lane), so a row is loaded once per wave and not W
// times.  The W values of a row are W loads of that row at the slices s - R .. s + R, clamped: each is one coalesced 256-byte request,
// the first of them brings the line in and the others hit the vector cache.  The march is unrolled W-fold so that the row a new load
// replaces is a fixed set of registers (no rotation moves).  A wave re-reads 2 R halo rows per MD_ROWS / 4 of its own (from L2).
constexpr int MD_ROWS = 64;

template <int R, bool REPLACE>
__global__ __launch_bounds__(256) void k_sino_median(const float *__restrict__ src, float *__restrict__ dst, const float *__restrict__ thresh,
                                                     double *__restrict__ part, int n, int nx, int sx)
{
    constexpr int W = 2 * R + 1, PER_WAVE = MD_ROWS / 4;
    const int a = blockIdx.z, rb = blockIdx.y, ch = blockIdx.x;
    const int wave = threadIdx.x >> 6, s = ch * 64 + (threadIdx.x & 63);
    const bool real = s < nx;
    const float *S = src + (size_t)a * n * sx;
    float *D = REPLACE ? dst + (size_t)a * n * sx : nullptr;
    const float thr = REPLACE ? thresh[a] : 0.f;
    int col[W];
#pragma unroll
    for (int j = 0; j < W; ++j) col[j] = min(max(s + j - R, 0), nx - 1);
    const int rs = rb * MD_ROWS + wave * PER_WAVE, re = min(n, rs + PER_WAVE);
    double acc[3] = {0.0, 0.0, 0.0};
    int count = 0, replaced = 0;
    float w[W][W];                                      // row rho of the window sits in w[(rho - r + R) % W] at the head r of an unrolled group
    if (rs < re) {
#pragma unroll
        for (int k = 0; k < W - 1; ++k) {
            const float *row = S + (size_t)min(max(rs - R + k, 0), n - 1) * sx;
#pragma unroll
            for (int j = 0; j < W; ++j) w[k][j] = row[col[j]];
        }
    }
    for (int r = rs; r < re; r += W) {
#pragma unroll
        for (int u = 0; u < W; ++u) {
            if (r + u < re) {                           // the same in every lane
                const float *row = S + (size_t)min(r + u + R, n - 1) * sx;
#pragma unroll
                for (int j = 0; j < W; ++j) w[(W - 1 + u) % W][j] = row[col[j]];
                float v[W * W];
#pragma unroll
                for (int k = 0; k < W; ++k)
#pragma unroll
                    for (int j = 0; j < W; ++j) v[k * W + j] = w[k][j];
                const float x = w[(R + u) % W][R], m = median_of<W * W>(v);
                const float d = __fsub_rn(x, m);
                if (real) {
                    const double dd = (double)d;
                    acc[0] += dd; acc[1] += fabs(dd); acc[2] += __dmul_rn(dd, dd);
                    ++count;
                }
                if constexpr (REPLACE) {
                    const bool rep = fabsf(d) > thr;
                    if (real && rep) ++replaced;
                    D[(size_t)(r + u) * sx + s] = real ? (rep ? m : x) : 0.f;
                }
            }
        }
    }
    const double sums[5] = {acc[0], acc[1], acc[2], (double)count, (double)replaced};
    block_sum_row<5>(sums, part + (((size_t)a * gridDim.y + rb) * gridDim.x + ch) * 5);
}

// ---- window statistics: sum X, sum X^2, min X, max X over r0 <= r < r1, s0 <= s < s1 of every projection ---------------------------
// Workgroup (blk, a) takes WS_ROWS rays of the window; wave w the rays rlo + w, rlo + w + 4, ..., a lane the slices s0 + lane,
// s0 + lane + 64, ...  The sums in binary64 from the first sample (the square a binary64 product of the converted sample), minimum
// and maximum in binary32 (exact in any order).  part[a][blk] = {sum, sum of squares, min, max}; k_window_stats_finish adds the first
// two over the workgroups in ascending order and takes the extrema of the other two.
constexpr int WS_ROWS = 32;

__global__ __launch_bounds__(256) void k_sino_window_stats(const float *__restrict__ g, double *__restrict__ part, int n, int sx, int r0, int r1,
                                                           int s0, int s1)
{
    __shared__ float ext[2][4];
    const int a = blockIdx.y, blk = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int rlo = r0 + blk * WS_ROWS, rhi = min(r1, rlo + WS_ROWS);
    const float *base = g + (size_t)a * n * sx;
    double acc[2] = {0.0, 0.0};
    float lo = INFINITY, hi = -INFINITY;
    for (int r = rlo + wave; r < rhi; r += 4)
        for (int s = s0 + lane; s < s1; s += 64) {
            const float x = base[(size_t)r * sx + s];
            const double xd = (double)x;
            acc[0] += xd; acc[1] += __dmul_rn(xd, xd);
            lo = fminf(lo, x); hi = fmaxf(hi, x);
        }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { lo = fminf(lo, __shfl_xor(lo, o, 64)); hi = fmaxf(hi, __shfl_xor(hi, o, 64)); }
    if (lane == 0) { ext[0][wave] = lo; ext[1][wave] = hi; }
    __syncthreads();
    double *row = part + ((size_t)a * gridDim.x + blk) * 4;
    if (threadIdx.x == 0) {
        row[2] = (double)fminf(fminf(ext[0][0], ext[0][1]), fminf(ext[0][2], ext[0][3]));
        row[3] = (double)fmaxf(fmaxf(ext[1][0], ext[1][1]), fmaxf(ext[1][2], ext[1][3]));
    }
    block_sum_row<2>(acc, row);
}

__global__ void k_window_stats_finish(const double *__restrict__ part, double *__restrict__ out, int np, int nblk)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= np * 4) return;
    const int a = i >> 2, k = i & 3;
    const double *p = part + (size_t)a * nblk * 4 + k;
    double v = p[0];
    for (int b = 1; b < nblk; ++b) {
        const double t = p[(size_t)b * 4];
        v = k < 2 ? v + t : (k == 2 ? fmin(v, t) : fmax(v, t));
    }
    out[i] = v;
}

// ---- gain and offset per projection -----------------------------------------------------------------------------------------------
// dst = fma(gain_a, x, offset_a), one fused operation; with CLAMP followed by max(0, .), spelled v > 0 ? v : 0 (a -0 and a NaN give
// +0).  tab[a] = {gain, offset}.  Four slices per lane (the pitch is a multiple of 64 floats: every float4 is aligned and inside one
// row); padding slices are written as zero whatever the offset.  src and dst may be the same buffer: an element is read and written
// by the same lane.
template <bool CLAMP>
__global__ __launch_bounds__(256) void k_sino_intensity(const float *src, float *dst, const float2 *__restrict__ tab, int n, int nx, int sx)
{
    const int a = blockIdx.y;
    const float2 t = tab[a];
    const float4 *S = reinterpret_cast<const float4 *>(src + (size_t)a * n * sx);
    float4 *D = reinterpret_cast<float4 *>(dst + (size_t)a * n * sx);
    const int sx4 = sx >> 2, total = n * sx4;
    auto one = [&](float x, int s) -> float {
        float v = __fmaf_rn(t.x, x, t.y);
        if constexpr (CLAMP) v = v > 0.f ? v : 0.f;
        return s < nx ? v : 0.f;
    };
    for (int idx = blockIdx.x * 256 + threadIdx.x; idx < total; idx += gridDim.x * 256) {
        const int s = (idx % sx4) * 4;
        const float4 x = S[idx];
        D[idx] = make_float4(one(x.x, s), one(x.y, s + 1), one(x.z, s + 2), one(x.w, s + 3));
    }
}

}  // namespace tomo
