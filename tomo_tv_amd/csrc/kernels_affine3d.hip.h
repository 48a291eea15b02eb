// kernels_affine3d.hip.h -- a volume resampled by a 3-D affine map: rotation, magnification and shift in one trilinear interpolation
// (tomo_volume_affine / tomo_volume_affine_axpy)
// Part of kernels.hip.h (include that, not this).
//
// Both volumes are [pixel = y N + z][slice s] with row pitch sx (a multiple of 64 floats, buffers 256-byte aligned); their sizes may
// differ.  m = {m00 .. m03, m10 .. m13, m20 .. m23} in binary64 maps a DESTINATION voxel (s, y, z) to its SOURCE position
//     s' = fma(m00, s, fma(m01, y, fma(m02, z, m03))),   y' = fma(m10, s, fma(m11, y, fma(m12, z, m13))),   z' likewise with m2*,
// three fused multiply-adds per coordinate, evaluated per voxel (the two inner links depend on the destination row alone and are
// formed once per lane item of four voxels: the same operations on the same operands, the same bits).  Each coordinate is split by
// axis_split<SPLIT_ZERO_PAD> into first tap, weights and the "second tap kept" flag, and the value is trilinear_value of the kept
// taps (both kernels_geom.hip.h): an axis whose fraction is zero keeps only its first tap -- the other is neither loaded nor
// multiplied.  A tap outside the source is 0 (not loaded); a coordinate outside (-1, size) has no tap inside and gives 0 (a NaN from
// Inf - Inf of huge finite entries lands there too).  Hence an identity, a permutation of the axes, a whole-voxel translation,
// quarter turns and flips copy samples bit for bit, and an Inf next to a copied sample stays out of the sum.
//
// Shape.  Lanes run along the destination's s, four consecutive slices per lane, one 16-byte store per lane: a 16-lane group writes
// 256 contiguous bytes of a destination row, over the whole pitch (the slices Nslice .. sx-1 are stored as zero by this same
// launch).  Workgroup b covers the AF_ROWS consecutive destination rows from AF_ROWS b on -- z fastest inside a y plane -- so the
// eight taps of neighbouring rows, and of neighbouring workgroups, meet the same cache lines.  The source is gathered through the
// cache hierarchy with 4-byte loads: for a first column near (1, 0, 0) consecutive lanes read consecutive words of a few source rows.
// A wave whose voxels all lie outside the source finds every tap predicate false and stores zeros without a load.  Nine binary64 FMAs
// per voxel as stated; issued per item of four voxels: 6 for the inner links (recomputed per item, not hoisted per row: a 512-slice
// row has 128 items) and 12 outer ones, 4.5 per voxel, beside eight loads per voxel and one 16-byte store per item.  No LDS, no
// scratch, no atomics; every output word has one producer and one fixed expression: the same bits from run to run.
#pragma once

namespace tomo {

constexpr int AF_ROWS = 8;       // destination rows per workgroup

struct Affine3 { double m[12]; };

// the interpolated source value at destination voxel (s, row): by, bz, bs are the row's inner links of the three chains
__device__ __forceinline__ float af_sample(const float *__restrict__ src, const Affine3 &M, double bs, double by, double bz, int s,
                                           int nxs, int ns, int sxs)
{
    const double sd = (double)s;
    int is, iy, iz;
    float ws[2], wy[2], wz[2];
    bool ks, ky, kz;
    if (!axis_split<SPLIT_ZERO_PAD>(fma(M.m[0], sd, bs), nxs, is, ws, ks) || !axis_split<SPLIT_ZERO_PAD>(fma(M.m[4], sd, by), ns, iy, wy, ky) ||
        !axis_split<SPLIT_ZERO_PAD>(fma(M.m[8], sd, bz), ns, iz, wz, kz))
        return 0.f;
    auto tap = [&](int dy, int dz, int ds) -> float {
        const int y = iy + dy, z = iz + dz, q = is + ds;
        if ((unsigned)y >= (unsigned)ns || (unsigned)z >= (unsigned)ns || (unsigned)q >= (unsigned)nxs) return 0.f;
        return src[((size_t)y * ns + z) * (size_t)sxs + q];
    };
    return trilinear_value(tap, wy, wz, ws, ky, kz, ks);
}

// AXPY = false: dst = value (dst is not read).  AXPY = true: dst = fmaf(a, value, dst), then fmaxf(., 0) when clamp -- fmaxf returns
// its other operand for a NaN, so a NaN result is clamped to 0 (k_volume_cross's rule).
// grid.x = ceil(N_dst^2 / AF_ROWS); 256 threads
template <bool AXPY>
__global__ __launch_bounds__(256) void k_volume_affine(const float *__restrict__ src, float *__restrict__ dst, Affine3 M, int nxs, int ns,
                                                       int sxs, int nxd, int nd, int sxd, float a, int clamp)
{
    const int quads = sxd >> 2, npix = nd * nd;
    const int row0 = blockIdx.x * AF_ROWS, items = min(AF_ROWS, npix - row0) * quads;
    for (int idx = threadIdx.x; idx < items; idx += 256) {
        const int r = idx / quads, s0 = 4 * (idx - r * quads), row = row0 + r;
        const double y = (double)(row / nd), z = (double)(row % nd);
        const double bs = fma(M.m[1], y, fma(M.m[2], z, M.m[3]));
        const double by = fma(M.m[5], y, fma(M.m[6], z, M.m[7]));
        const double bz = fma(M.m[9], y, fma(M.m[10], z, M.m[11]));
        float *q = dst + (size_t)row * sxd + s0;
        float v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = s0 + k < nxd ? af_sample(src, M, bs, by, bz, s0 + k, nxs, ns, sxs) : 0.f;
        if constexpr (AXPY) {
            const float4 d = *reinterpret_cast<const float4 *>(q);
            const float dd[4] = {d.x, d.y, d.z, d.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float f = __fmaf_rn(a, v[k], dd[k]);
                if (clamp) f = fmaxf(f, 0.f);
                v[k] = s0 + k < nxd ? f : 0.f;
            }
        }
        *reinterpret_cast<float4 *>(q) = make_float4(v[0], v[1], v[2], v[3]);
    }
}

}  // namespace tomo
