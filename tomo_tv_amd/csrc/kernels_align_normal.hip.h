// kernels_align_normal.hip.h -- the Gauss-Newton normal equations of an intensity-based similarity matching of every projection of a
// series against its model: gather, analytic gradient and the 4 x 4 reduction in one pass over the model (tomo_sino_affine_normal)
// Part of kernels.hip.h (include that, not this; it follows kernels_align.hip.h, whose layout and conventions it shares).
//
// F_a is projection a of the fixed sinogram (the model; the destination grid of tomo_sino_affine), G_a projection a of the moving one
// (the series as given; the source), both X_a[r][s] with the engine's sizes and pitch.  mat[a] = {m00, m01, m02, m10, m11, m12} maps a
// sample (r, s) of F_a to its position p = (r', s') in G_a: the chain of k_sino_affine, r' = fma(m00, r, fma(m01, s, m02)),
// s' = fma(m10, r, fma(m11, s, m12)) in binary64; each coordinate is split by axis_split<SPLIT_INSIDE> (kernels_geom.hip.h).
//
// Which samples count.  Both must hold: (a) all four tap positions lie inside G_a, 0 <= i and i + 1 <= size - 1 on both axes with i the
// first tap AFTER the split (so a coordinate just below 0 whose fraction rounds to 1 is pixel 0 and can count; stricter than the zero
// padding of k_sino_affine: a sample on the last row of G does not count even with t = 0); (b) margin <= r <= Nray - 1 - margin and margin <= s <= Nslice - 1 - margin.  A sample that does not count loads no tap and
// adds nothing (a branch, never a product with 0): an Inf or a NaN there, or in a sample of G that is no tap of a counting sample,
// stays out.  A counting sample loads all four taps x[di][dj] (di along r, dj along s), whatever its fractions.  Padding slices
// (s >= Nslice) are never read as data: they fail (b) as samples and (a) as taps.
//
// Per counting sample, in binary32 with every operation rounded once:
//   value     w   = the formula of bilinear_value, here with every product and every sum an operation of its own (no fused
//                 multiply-add: the intrinsics below say so; tests/ref64_affine.py replays the same operations).  The taps are needed
//                 for the gradient anyway.  This is the UNCONTRACTED evaluation: k_sino_affine's compiled bilinear_value is
//                 contracted into fused multiply-adds, so w is not bit-equal to what tomo_sino_affine writes for the same map:
//                   tr = ts = 0:  x00
//                   tr = 0:       (1 - ts) x00 + ts x01
//                   ts = 0:       (1 - tr) x00 + tr x10
//                   else:         ((wr ws) x00 + (wr ts) x01 + (tr ws) x10) + (tr ts) x11,  wr = 1 - tr, ws = 1 - ts, summed left to right
//   gradient  with the weights per axis u[0] = 1 - t, u[1] = t, and u[0] = 1 exactly where t = 0:
//             g_r = us[0] (x10 - x00);  then fmaf(us[1], x11 - x01, .)
//             g_s = ur[0] (x01 - x00);  then fmaf(ur[1], x11 - x10, .)
//   the derivative of the bilinear interpolant of the cell [i, i + 1] x [j, j + 1] at the fractions: at t = 0 the one-sided derivative
//   towards the second tap.
// and in binary64:
//   res = (double)w - (double)F_a(r, s);   q = p - c_G,  c_G = ((Nray - 1) / 2, (Nslice - 1) / 2),  p the coordinates as the chain gave them
//   J = (g_r, g_s, fma(q_r, g_s, -(q_s g_r)), fma(q_r, g_r, q_s g_s))
//   the derivative of G(c_G + e^lambda Rot(omega)(p - c_G) + t) by (t_r, t_s, omega, lambda) at 0.
// The 21 sums over the counting samples of projection a, each term added by one binary64 fused multiply-add (the products of two
// binary32 values are exact there, so only the sum rounds):
//   [0..9] the upper triangle of J^T J, row-major;  [10..13] J^T res;  [14] sum res^2;  [15] the count;  [16..18] sum F^2, sum w^2,
//   sum F w;  [19..20] sum F, sum w.
//
// Shape.  Lane = slice: workgroup (blk, a) takes the SN_ROWS rays [SN_ROWS blk, SN_ROWS (blk + 1)) of projection a, a thread the items
// idx = threadIdx.x, threadIdx.x + 256, ... of them (row idx / sx, slice idx % sx: a wave reads 64 consecutive slices of one row of F,
// 256 bytes, and gathers G through the cache hierarchy with 4-byte loads) and adds its samples in that order into 21 binary64 registers.
// The workgroup's 21 sums go to part[a][blk][21] (block_sum_row) and k_sum_rows_ascending adds the workgroups of a projection.  No
// atomics, no LDS but the 4 x 21 wave sums: the same bits from call to call.  Nothing but part and out is written.
#pragma once

namespace tomo {

constexpr int SN_ROWS = 16;          // rays per workgroup of k_sino_affine_normal
constexpr int SN_SUMS = 21;

// grid = (ceil(n / SN_ROWS), np); 256 threads
__global__ __launch_bounds__(256) void k_sino_affine_normal(const float *__restrict__ F, const float *__restrict__ G,
                                                            const double *__restrict__ mat, int n, int nx, int sx, int margin,
                                                            double *__restrict__ part)
{
    double acc[SN_SUMS];
#pragma unroll
    for (int k = 0; k < SN_SUMS; ++k) acc[k] = 0.0;
    const int a = blockIdx.y, blk = blockIdx.x;
    const double *m = mat + 6 * (size_t)a;
    const double m00 = m[0], m01 = m[1], m02 = m[2], m10 = m[3], m11 = m[4], m12 = m[5];
    const float *Fa = F + (size_t)a * n * sx, *Ga = G + (size_t)a * n * sx;
    const double cr = 0.5 * (double)(n - 1), cs = 0.5 * (double)(nx - 1);
    const int row0 = blk * SN_ROWS, items = min(SN_ROWS, n - row0) * sx;
    for (int idx = threadIdx.x; idx < items; idx += 256) {
        const int rr = idx / sx, s = idx - rr * sx, r = row0 + rr;
        if (r < margin || r > n - 1 - margin || s < margin || s > nx - 1 - margin) continue;
        const double rp = fma(m00, (double)r, fma(m01, (double)s, m02));
        const double sp = fma(m10, (double)r, fma(m11, (double)s, m12));
        int i, j;
        float tr, ts;
        if (!axis_split<SPLIT_INSIDE>(rp, n, i, tr) || !axis_split<SPLIT_INSIDE>(sp, nx, j, ts)) continue;
        // the four taps: all inside G_a by the rule above
        const float *g0 = Ga + (size_t)i * sx + j;
        const float x00 = g0[0], x01 = g0[1], x10 = g0[sx], x11 = g0[sx + 1];
        float w;
        const float ur0 = tr != 0.f ? __fsub_rn(1.f, tr) : 1.f, us0 = ts != 0.f ? __fsub_rn(1.f, ts) : 1.f;
        if (tr == 0.f && ts == 0.f) w = x00;
        else if (tr == 0.f) w = __fadd_rn(__fmul_rn(us0, x00), __fmul_rn(ts, x01));
        else if (ts == 0.f) w = __fadd_rn(__fmul_rn(ur0, x00), __fmul_rn(tr, x10));
        else {
            w = __fadd_rn(__fmul_rn(__fmul_rn(ur0, us0), x00), __fmul_rn(__fmul_rn(ur0, ts), x01));
            w = __fadd_rn(w, __fmul_rn(__fmul_rn(tr, us0), x10));
            w = __fadd_rn(w, __fmul_rn(__fmul_rn(tr, ts), x11));
        }
        const float gr = __fmaf_rn(ts, __fsub_rn(x11, x01), __fmul_rn(us0, __fsub_rn(x10, x00)));
        const float gs = __fmaf_rn(tr, __fsub_rn(x11, x10), __fmul_rn(ur0, __fsub_rn(x01, x00)));
        const double wd = (double)w, fd = (double)Fa[(size_t)r * sx + s], res = wd - fd;
        const double qr = rp - cr, qs = sp - cs;
        double J[4] = {(double)gr, (double)gs, 0.0, 0.0};
        J[2] = fma(qr, J[1], -(qs * J[0]));
        J[3] = fma(qr, J[0], qs * J[1]);
        int o = 0;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
#pragma unroll
            for (int q = p; q < 4; ++q) { acc[o] = fma(J[p], J[q], acc[o]); ++o; }
        }
#pragma unroll
        for (int p = 0; p < 4; ++p) acc[10 + p] = fma(J[p], res, acc[10 + p]);
        acc[14] = fma(res, res, acc[14]);
        acc[15] += 1.0;
        acc[16] = fma(fd, fd, acc[16]);
        acc[17] = fma(wd, wd, acc[17]);
        acc[18] = fma(fd, wd, acc[18]);
        acc[19] += fd;
        acc[20] += wd;
    }
    block_sum_row<SN_SUMS>(acc, part + ((size_t)a * gridDim.x + blk) * SN_SUMS);
}

}  // namespace tomo
