// kernels_dual.hip.h -- dual-axis tomography: the volume of one engine carried into the layout of an engine whose tilt axis is
// perpendicular to the first one's (tomo_volume_cross / tomo_volume_cross_axpy)
// Part of kernels.hip.h (include that, not this).
//
// Both engines hold a cube of N^3 voxels as [pixel = y N + z][slice s] with row pitch sx (a multiple of 64 floats, buffers 256-byte
// aligned).  Engine B's slice index is engine A's z and its column index is A's s; the beam direction y is shared:
//     dst[(y N + s) sx + z] = src[(y N + z) sx + s]
// i.e. for every y an N x N transpose of rows of sx floats.  Reading with the lanes along z (a whole plane between two lanes) is the
// uncoalesced access SURVEY 2b describes; here both sides run along the fastest index: a workgroup carries one 64 x 64 tile of one
// y-plane through LDS.  Source side: a 16-lane group reads 256 contiguous bytes of one source row (lanes along s), 16 bytes per
// lane.  Destination side: a 16-lane group writes 256 contiguous bytes of one destination row (lanes along z), 16 bytes per lane.
// The tile is kept with a row of 65 words: the row-wise word stores and the column-wise word loads of a 32-lane half then meet a bank
// twice at the most (the 16-byte global accesses fix four consecutive words per lane, so the eight distinct 4 c offsets of a half
// fold onto eight banks, two lanes each); the pass moves 16 KiB through LDS per 32 KiB of HBM traffic and is bound by the latter.
//
// A tile that lies inside the cube on both axes takes the path without any per-element guard (the choice is uniform for the
// workgroup).  An edge tile selects: no source word at slice index >= N or of a row z >= N is loaded, a destination row s >= N is
// not written, and the destination columns N .. sx-1 are stored as zero by this same launch (the tiles cover the whole pitch along z).
// The tile holds uint32 words, so `cross` moves bits: NaN payloads, -0.0 and denormals arrive as they left.  No atomics, no
// scratch; every output word has one producer and one fixed expression: the same bits from run to run.
#pragma once

namespace tomo {

constexpr int DX_T = 64, DX_P = DX_T + 1;      // tile edge, LDS row in words

// AXPY = false: dst = src^T (dst is not read).  AXPY = true: dst = fmaf(a, src^T, dst), then fmaxf(., 0) when clamp -- fmaxf
// returns its other operand for a NaN, so a NaN result is clamped to 0 (the rule of every clamp of this engine, k_positivity).
template <bool AXPY, bool FULL>
__device__ __forceinline__ void cross_tile(const float *__restrict__ src, float *__restrict__ dst, uint32_t *tile, int n, int sx,
                                           size_t plane, int z0, int s0, float a, int clamp)
{
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, r = w * 4 + (lane >> 4), c = 4 * (lane & 15);
    uint4 v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int z = z0 + i * 16 + r, s = s0 + c;
        const float *p = src + (plane + z) * (size_t)sx + s;
        if constexpr (FULL) v[i] = *reinterpret_cast<const uint4 *>(p);
        else {
            const bool row = z < n;
            v[i].x = row && s < n ? __float_as_uint(p[0]) : 0u;
            v[i].y = row && s + 1 < n ? __float_as_uint(p[1]) : 0u;
            v[i].z = row && s + 2 < n ? __float_as_uint(p[2]) : 0u;
            v[i].w = row && s + 3 < n ? __float_as_uint(p[3]) : 0u;
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        uint32_t *t = tile + (i * 16 + r) * DX_P + c;      // tile[z][s]
        t[0] = v[i].x; t[1] = v[i].y; t[2] = v[i].z; t[3] = v[i].w;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int sl = i * 16 + r, s = s0 + sl, z = z0 + c;       // destination row s, columns z .. z + 3
        if (!FULL && s >= n) continue;
        const uint32_t *t = tile + c * DX_P + sl;
        uint4 o = make_uint4(t[0], t[DX_P], t[2 * DX_P], t[3 * DX_P]);
        float *q = dst + (plane + s) * (size_t)sx + z;
        if constexpr (AXPY) {
            float4 d;
            if constexpr (FULL) d = *reinterpret_cast<const float4 *>(q);
            else { d.x = z < n ? q[0] : 0.f; d.y = z + 1 < n ? q[1] : 0.f; d.z = z + 2 < n ? q[2] : 0.f; d.w = z + 3 < n ? q[3] : 0.f; }
            float4 f = make_float4(__fmaf_rn(a, __uint_as_float(o.x), d.x), __fmaf_rn(a, __uint_as_float(o.y), d.y),
                                   __fmaf_rn(a, __uint_as_float(o.z), d.z), __fmaf_rn(a, __uint_as_float(o.w), d.w));
            if (clamp) { f.x = fmaxf(f.x, 0.f); f.y = fmaxf(f.y, 0.f); f.z = fmaxf(f.z, 0.f); f.w = fmaxf(f.w, 0.f); }
            o = make_uint4(__float_as_uint(f.x), __float_as_uint(f.y), __float_as_uint(f.z), __float_as_uint(f.w));
            if constexpr (!FULL) { if (z >= n) o.x = 0u; if (z + 1 >= n) o.y = 0u; if (z + 2 >= n) o.z = 0u; if (z + 3 >= n) o.w = 0u; }
        }
        *reinterpret_cast<uint4 *>(q) = o;
    }
}

// grid.x = (tiles along z over the whole pitch) * (tiles along s over N) * N planes; 256 threads
template <bool AXPY>
__global__ __launch_bounds__(256) void k_volume_cross(const float *__restrict__ src, float *__restrict__ dst, int n, int sx, int tiles_z,
                                                      int tiles_s, float a, int clamp)
{
    __shared__ uint32_t tile[DX_T * DX_P];
    const int tz = blockIdx.x % tiles_z, rest = blockIdx.x / tiles_z, ts = rest % tiles_s, y = rest / tiles_s;
    if (y >= n) return;
    const int z0 = tz * DX_T, s0 = ts * DX_T;
    const size_t plane = (size_t)y * n;
    if (z0 + DX_T <= n && s0 + DX_T <= n) cross_tile<AXPY, true>(src, dst, tile, n, sx, plane, z0, s0, a, clamp);
    else cross_tile<AXPY, false>(src, dst, tile, n, sx, plane, z0, s0, a, clamp);
}

}  // namespace tomo
