// kernels_register3d.hip.h -- the Gauss-Newton normal equations of an intensity-based rigid registration of two volumes: gather, analytic
// gradient and the 6 x 6 reduction in one pass over the fixed volume (tomo_volume_affine_normal)
// Part of kernels.hip.h (include that, not this; it follows kernels_affine3d.hip.h, whose Affine3, AF_ROWS and layout it shares).
//
// F is the fixed volume (the destination grid of tomo_volume_affine), G the moving one (the source); both [pixel = y N + z][slice s]
// with their own sizes and pitches.  A voxel x = (s, y, z) of F has the position p = M x in G: the coordinate chain of
// k_volume_affine, three fused multiply-adds per coordinate in binary64, the two inner links once per item of four voxels; each
// coordinate is split by axis_split<SPLIT_INSIDE_FROM_ZERO> (kernels_geom.hip.h).
//
// Which voxels count.  Both must hold: (a) all eight tap positions lie inside G: 0 <= c on every axis, judged on the coordinate
// itself BEFORE the split (0 <= floor(c), as tests/ref64_register3d.py states it: a c in [-2^-25, 0) does not count although its
// split would be voxel 0 with t = 0 -- k_sino_affine_normal's rule takes such a sample), and i + 1 <= size - 1 with i the first tap
// after the split (stricter than the zero padding of k_volume_affine: a voxel on the last plane of G does not count even with
// t = 0); (b) margin <= x <= size - 1 - margin on every axis of F.  A voxel that does not count loads no tap and adds nothing
// (a branch, never a product with 0): an Inf or a NaN there, or in a voxel of G that is no tap of a counting voxel, stays out.  A
// counting voxel loads all eight taps x[dy][dz][ds], whatever its fractions.
//
// Per counting voxel, in binary32 with every operation rounded once (weights per axis w[0] = 1 - t, w[1] = t, and w[0] = 1 exactly
// where t = 0, as axis_split gives them):
//   value     w   = trilinear_value of the kept taps (an axis with t = 0 keeps its first tap only): the bits of k_volume_affine.
//   gradient  g_s = (wy0 wz0) e00;  then fmaf(wy0 wz1, e01, .), fmaf(wy1 wz0, e10, .), fmaf(wy1 wz1, e11, .)
//                   with e[dy][dz] = x[dy][dz][1] - x[dy][dz][0]
//             g_y = (wz0 ws0) e00;  then fmaf(wz0 ws1, e01, .), fmaf(wz1 ws0, e10, .), fmaf(wz1 ws1, e11, .)
//                   with e[dz][ds] = x[1][dz][ds] - x[0][dz][ds]
//             g_z = (wy0 ws0) e00;  then fmaf(wy0 ws1, e01, .), fmaf(wy1 ws0, e10, .), fmaf(wy1 ws1, e11, .)
//                   with e[dy][ds] = x[dy][1][ds] - x[dy][0][ds]
//   the derivative of the trilinear interpolant of the cell [i, i + 1]^3 at the fractions: at t = 0 the one-sided derivative towards
//   the second tap.
// and in binary64:
//   r = (double)w - (double)F(x);   q = p - c_G,  c_G = (size - 1) / 2 per axis,  p the coordinate as the chain gave it
//   J = (g_s, g_y, g_z, fma(q_y, g_z, -(q_z g_y)), fma(q_z, g_s, -(q_s g_z)), fma(q_s, g_y, -(q_y g_s)))
//   the derivative of G(c_G + Rot(omega)(p - c_G) + t) by (t, omega) at 0.
// The 32 sums over the counting voxels, each term added by one binary64 fused multiply-add (the products of two binary32 values are
// exact there, so only the sum rounds):
//   [0..20] the upper triangle of J^T J, row-major;  [21..26] J^T r;  [27] sum r^2;  [28] the count;  [29..31] sum F^2, sum w^2, sum F w.
//
// Shape.  Lanes, items of four slices and AF_ROWS rows per block of rows as in k_volume_affine; F is read with one 16-byte load per
// item, G through the cache hierarchy with 4-byte loads.  The grid is capped at RG_BLOCKS workgroups, workgroup b takes the blocks of
// rows b, b + gridDim.x, ...: a thread adds its voxels in that order into 32 binary64 registers, the workgroup's sums go to part[b][32]
// (block_sum_row) and k_sum_rows_tree adds the workgroups' rows.  No atomics: the same bits from call to call.  Nothing but part and
// out is written.
#pragma once

namespace tomo {

constexpr int RG_BLOCKS = 1024;      // the most workgroups of k_volume_affine_normal: bounds part[RG_BLOCKS + 1][32] (the last row: the result)
constexpr int RG_SUMS = 32;

// grid.x = min(RG_BLOCKS, ceil(N_F^2 / AF_ROWS)); 256 threads
__global__ __launch_bounds__(256) void k_volume_affine_normal(const float *__restrict__ F, const float *__restrict__ G, Affine3 M, int nxs,
                                                              int ns, int sxs, int nxd, int nd, int sxd, int margin,
                                                              double *__restrict__ part)
{
    double acc[RG_SUMS];
#pragma unroll
    for (int k = 0; k < RG_SUMS; ++k) acc[k] = 0.0;
    const int quads = sxd >> 2, npix = nd * nd, nblk = (npix + AF_ROWS - 1) / AF_ROWS;
    const double cs = 0.5 * (double)(nxs - 1), cyz = 0.5 * (double)(ns - 1);
    for (int blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
        const int row0 = blk * AF_ROWS, items = min(AF_ROWS, npix - row0) * quads;
        for (int idx = threadIdx.x; idx < items; idx += 256) {
            const int r = idx / quads, s0 = 4 * (idx - r * quads), row = row0 + r;
            const int yi = row / nd, zi = row % nd;
            if (yi < margin || yi > nd - 1 - margin || zi < margin || zi > nd - 1 - margin) continue;
            if (s0 + 3 < margin || s0 > nxd - 1 - margin) continue;
            const double y = (double)yi, z = (double)zi;
            const double bs = fma(M.m[1], y, fma(M.m[2], z, M.m[3]));
            const double by = fma(M.m[5], y, fma(M.m[6], z, M.m[7]));
            const double bz = fma(M.m[9], y, fma(M.m[10], z, M.m[11]));
            const float4 f4 = *reinterpret_cast<const float4 *>(F + (size_t)row * sxd + s0);
            const float fv[4] = {f4.x, f4.y, f4.z, f4.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int s = s0 + k;
                if (s < margin || s > nxd - 1 - margin) continue;
                const double sd = (double)s;
                const double ps = fma(M.m[0], sd, bs), py = fma(M.m[4], sd, by), pz = fma(M.m[8], sd, bz);
                int is, iy, iz;
                float ws[2], wy[2], wz[2];
                bool ks, ky, kz;
                if (!axis_split<SPLIT_INSIDE_FROM_ZERO>(ps, nxs, is, ws, ks) || !axis_split<SPLIT_INSIDE_FROM_ZERO>(py, ns, iy, wy, ky) ||
                    !axis_split<SPLIT_INSIDE_FROM_ZERO>(pz, ns, iz, wz, kz))
                    continue;
                // the eight taps x[dy][dz][ds] at index dy 4 + dz 2 + ds: all inside G by the rule above
                const float *g0 = G + ((size_t)iy * ns + iz) * (size_t)sxs + is;
                const size_t oz = (size_t)sxs, oy = (size_t)ns * sxs;
                const float x[8] = {g0[0], g0[1], g0[oz], g0[oz + 1], g0[oy], g0[oy + 1], g0[oy + oz], g0[oy + oz + 1]};
                const float w = trilinear_value([&](int dy, int dz, int ds) { return x[dy * 4 + dz * 2 + ds]; }, wy, wz, ws, ky, kz, ks);
                float gs = __fmul_rn(__fmul_rn(wy[0], wz[0]), __fsub_rn(x[1], x[0]));
                gs = __fmaf_rn(__fmul_rn(wy[0], wz[1]), __fsub_rn(x[3], x[2]), gs);
                gs = __fmaf_rn(__fmul_rn(wy[1], wz[0]), __fsub_rn(x[5], x[4]), gs);
                gs = __fmaf_rn(__fmul_rn(wy[1], wz[1]), __fsub_rn(x[7], x[6]), gs);
                float gy = __fmul_rn(__fmul_rn(wz[0], ws[0]), __fsub_rn(x[4], x[0]));
                gy = __fmaf_rn(__fmul_rn(wz[0], ws[1]), __fsub_rn(x[5], x[1]), gy);
                gy = __fmaf_rn(__fmul_rn(wz[1], ws[0]), __fsub_rn(x[6], x[2]), gy);
                gy = __fmaf_rn(__fmul_rn(wz[1], ws[1]), __fsub_rn(x[7], x[3]), gy);
                float gz = __fmul_rn(__fmul_rn(wy[0], ws[0]), __fsub_rn(x[2], x[0]));
                gz = __fmaf_rn(__fmul_rn(wy[0], ws[1]), __fsub_rn(x[3], x[1]), gz);
                gz = __fmaf_rn(__fmul_rn(wy[1], ws[0]), __fsub_rn(x[6], x[4]), gz);
                gz = __fmaf_rn(__fmul_rn(wy[1], ws[1]), __fsub_rn(x[7], x[5]), gz);
                const double wd = (double)w, fd = (double)fv[k], res = wd - fd;
                const double qs = ps - cs, qy = py - cyz, qz = pz - cyz;
                double J[6] = {(double)gs, (double)gy, (double)gz, 0.0, 0.0, 0.0};
                J[3] = fma(qy, J[2], -(qz * J[1]));
                J[4] = fma(qz, J[0], -(qs * J[2]));
                J[5] = fma(qs, J[1], -(qy * J[0]));
                int o = 0;
#pragma unroll
                for (int a = 0; a < 6; ++a) {
#pragma unroll
                    for (int b = a; b < 6; ++b) { acc[o] = fma(J[a], J[b], acc[o]); ++o; }
                }
#pragma unroll
                for (int a = 0; a < 6; ++a) acc[21 + a] = fma(J[a], res, acc[21 + a]);
                acc[27] = fma(res, res, acc[27]);
                acc[28] += 1.0;
                acc[29] = fma(fd, fd, acc[29]);
                acc[30] = fma(wd, wd, acc[30]);
                acc[31] = fma(fd, wd, acc[31]);
            }
        }
    }
    block_sum_row<RG_SUMS>(acc, part + (size_t)blockIdx.x * RG_SUMS);
}

}  // namespace tomo
