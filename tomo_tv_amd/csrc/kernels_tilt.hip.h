// kernels_tilt.hip.h -- refinement of the per-projection tilt angles: the rotational derivative of a volume about the tilt axis
// (tomo_volume_rot_derivative) and the per-projection sums of the Gauss-Newton step of an angle (tomo_sino_tilt_normal).
// Part of kernels.hip.h (include that, not this; it follows kernels_geom.hip.h, whose two-stage sums it uses).
//
// The convention of the system matrix (sysmat.cpp; cpu/utils/pytvlib.py:8-121): the pixel of flat index i * N + j of a slice sits at
// X = j - (N - 1) / 2, Y = (N - 1) / 2 - i, and ray t of angle theta runs through (t cos, t sin) along (-sin, cos).  For
// g_theta(t) = int f ds this gives  d g_theta / d theta = int (X d_Y f - Y d_X f) ds:  the angle derivative of EVERY projection is the
// ordinary projection of one volume D f = X d_Y f - Y d_X f, formed slice by slice.  With the residual r_p = b_p - g_p and
// d_p = (A D f)_p the Gauss-Newton step of projection p is <r_p, d_p> / <d_p, d_p> radians.
#pragma once

namespace tomo {

// ---- dst = X d_Y f - Y d_X f ------------------------------------------------------------------------------------------------------
// Central differences across the pixel grid of a slice; a row index i grows against Y:
//     dy = f[i - 1][j] - f[i + 1][j]   (0 on the rows i = 0 and i = N - 1: no tap is loaded there)
//     dx = f[i][j + 1] - f[i][j - 1]   (0 on the columns j = 0 and j = N - 1)
// The order of operations per voxel, every one rounded once in binary32 (tests/ref64_tilt.py replays it):
//     two subtractions (dy, dx);  two multiplies by 0.5 * coordinate,  hx = 0.5 * X and hy = 0.5 * Y, which are exact (X and Y are
//     half-integers below 2^22, so the halves are quarter-integers that binary32 holds) and  q = hy * dx, which rounds;
//     one fused multiply-add  dst = fma(hx, dy, -q).
// Four roundings (dy, dx, q, the fma), none between hx * dy and the subtraction of q.  A constant slice gives dy = dx = 0 and an exact 0.
// Lane = slice: the four neighbours of a pixel are whole rows of the slab-interleaved layout, a thread takes four consecutive slices
// of one pixel (16-byte loads, a wave 1 KiB of one row), and the padding slices (zero in src) come out as zero.  At worst four reads
// and one write of 4 bytes per voxel reach HBM (the centre sample is never read); neighbouring rows are re-read from cache.
// grid = ceil(npix * sx / 4 / 256); 256 threads.  src != dst (the host refuses): a pass in place would read what it wrote.
__global__ __launch_bounds__(256) void k_vol_rot_derivative(const float *__restrict__ src, float *__restrict__ dst, int n, int sx)
{
    const int sx4 = sx >> 2;
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x, total = (size_t)n * n * sx4;
    if (idx >= total) return;
    const size_t pix = idx / sx4;
    const int i = (int)(pix / n), j = (int)(pix - (size_t)i * n);
    const float c = 0.5f * (float)(n - 1);
    const float hx = 0.5f * ((float)j - c), hy = 0.5f * (c - (float)i);
    const float4 *s = reinterpret_cast<const float4 *>(src) + idx;
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 dy = zero, dx = zero;
    if (i > 0 && i < n - 1) {
        const float4 up = s[-(ptrdiff_t)n * sx4], dn = s[(ptrdiff_t)n * sx4];
        dy = make_float4(__fsub_rn(up.x, dn.x), __fsub_rn(up.y, dn.y), __fsub_rn(up.z, dn.z), __fsub_rn(up.w, dn.w));
    }
    if (j > 0 && j < n - 1) {
        const float4 rt = s[sx4], lf = s[-sx4];
        dx = make_float4(__fsub_rn(rt.x, lf.x), __fsub_rn(rt.y, lf.y), __fsub_rn(rt.z, lf.z), __fsub_rn(rt.w, lf.w));
    }
    float4 o;
    o.x = __fmaf_rn(hx, dy.x, -__fmul_rn(hy, dx.x));
    o.y = __fmaf_rn(hx, dy.y, -__fmul_rn(hy, dx.y));
    o.z = __fmaf_rn(hx, dy.z, -__fmul_rn(hy, dx.z));
    o.w = __fmaf_rn(hx, dy.w, -__fmul_rn(hy, dx.w));
    reinterpret_cast<float4 *>(dst)[idx] = o;
}

// ---- the sums of the angle step ---------------------------------------------------------------------------------------------------
// B, G, D: three sinograms (data, model, derivative), X_a[r][s] with the engine's sizes and pitch.  A sample counts when
// margin <= r <= Nray - 1 - margin and margin <= s <= Nslice - 1 - margin; a sample that does not count adds nothing (a branch, never a
// product with 0: an Inf or a NaN there stays out), and padding slices never count.  Per counting sample in binary64:
//     res = (double)B - (double)G;  d = (double)D;
//     [0] += res * d   [1] += d * d   [2] += res * res   (each one fused multiply-add)   [3] += 1
// Shape and order as k_sino_affine_normal: workgroup (blk, a) takes the TN_ROWS rays [TN_ROWS blk, TN_ROWS (blk + 1)) of projection a, a
// thread the groups of four slices idx = threadIdx.x, threadIdx.x + 256, ... of them (ray idx / (sx / 4), slices 4 (idx % (sx / 4)) ...
// + 3, ascending), three 16-byte loads each; its four sums go through block_sum_row to part[a][blk][4] and k_sum_rows_ascending adds
// the workgroups of a projection.  No atomics: the same bits from call to call.  Nothing but part is written.
constexpr int TN_ROWS = 16;          // rays per workgroup of k_sino_tilt_normal
constexpr int TN_SUMS = 4;

// grid = (ceil(n / TN_ROWS), np); 256 threads
__global__ __launch_bounds__(256) void k_sino_tilt_normal(const float *__restrict__ B, const float *__restrict__ G, const float *__restrict__ D,
                                                          int n, int nx, int sx, int margin, double *__restrict__ part)
{
    double acc[TN_SUMS] = {0.0, 0.0, 0.0, 0.0};
    const int a = blockIdx.y, blk = blockIdx.x, sx4 = sx >> 2;
    const size_t base = (size_t)a * n * sx4;
    const float4 *Ba = reinterpret_cast<const float4 *>(B) + base, *Ga = reinterpret_cast<const float4 *>(G) + base,
                 *Da = reinterpret_cast<const float4 *>(D) + base;
    const int row0 = blk * TN_ROWS, items = min(TN_ROWS, n - row0) * sx4;
    const int slo = margin, shi = nx - 1 - margin;
    for (int idx = threadIdx.x; idx < items; idx += 256) {
        const int rr = idx / sx4, s0 = 4 * (idx - rr * sx4), r = row0 + rr;
        if (r < margin || r > n - 1 - margin || s0 > shi || s0 + 3 < slo) continue;
        const size_t at = (size_t)r * sx4 + (s0 >> 2);
        const float4 b4 = Ba[at], g4 = Ga[at], d4 = Da[at];
        const float bv[4] = {b4.x, b4.y, b4.z, b4.w}, gv[4] = {g4.x, g4.y, g4.z, g4.w}, dv[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (s0 + k < slo || s0 + k > shi) continue;
            const double res = (double)bv[k] - (double)gv[k], d = (double)dv[k];
            acc[0] = fma(res, d, acc[0]);
            acc[1] = fma(d, d, acc[1]);
            acc[2] = fma(res, res, acc[2]);
            acc[3] += 1.0;
        }
    }
    block_sum_row<TN_SUMS>(acc, part + ((size_t)a * gridDim.x + blk) * TN_SUMS);
}

}  // namespace tomo
