// kernels_markers.hip.h -- marker (fiducial / feature) detection on the sinogram layout: the zero-mean normalised cross-correlation
// of every projection with one small template, and the local maxima of a slot with their four neighbours
// Part of kernels.hip.h (include that, not this; it stands after kernels_condition.hip.h, whose layout conventions it keeps).
//
// Projection a of a sinogram is the image X_a[r][s], ray r in [0, N), slice s in [0, Nslice): device row a * N + r, slice fastest,
// pitch sx.  The slices Nslice .. sx-1 are padding: never read as data, written as zero.  Lane = slice.  Both kernels are selections
// plus, in the correlation, binary32 operations in one fixed order, each rounded on its own (no contraction to a fused multiply-add):
// the same bits from call to call, and a replay in numpy gives them too.  No floating-point atomics; the peak compaction adds 1 to an
// integer counter per projection, so the ORDER of the records is not fixed -- the host code sorts them (engine_markers.inc).
//
// The form: an LDS tile with halo.  Workgroup (chunk, row block, a) stages the MK_ROWS + 2 R rows of
// 64 + 2 R slices its 64 x MK_ROWS samples look at, once, with coalesced loads (a row is 256 + 8 R contiguous bytes), and every
// window access after that is an LDS read at consecutive addresses in consecutive lanes: conflict-free at any R.  The row march of
// k_sino_median keeps W x W values per lane in registers, 289 at R = 8 (one wave per SIMD at best) and one instance per R; the tile
// needs 33 registers at every R, so R is a run-time argument and there is one instance of each kernel.
#pragma once

namespace tomo {

constexpr int MK_ROWS = 32, MK_RMAX = 8, MK_PITCH = 64 + 2 * MK_RMAX, MK_TROWS = MK_ROWS + 2 * MK_RMAX;

// tile[i][j] = X_a[r0 - R + i][s0 - R + j] for 0 <= i < MK_ROWS + 2 R, 0 <= j < 64 + 2 R; 0 where that leaves the image (such an
// entry is never used as data: every user tests the indices against N and Nslice).  Wave w takes the rows w, w + 4, ...; ends in a
// barrier.
__device__ __forceinline__ void mk_load_tile(float (*tile)[MK_PITCH], const float *__restrict__ S, int r0, int s0, int R, int n, int nx, int sx)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, tw = 64 + 2 * R, th = MK_ROWS + 2 * R;
    for (int i = wave; i < th; i += 4) {
        const int r = r0 - R + i;
        for (int j = lane; j < tw; j += 64) {
            const int s = s0 - R + j;
            tile[i][j] = (r >= 0 && r < n && s >= 0 && s < nx) ? S[(size_t)r * sx + s] : 0.f;
        }
    }
    __syncthreads();
}

// ---- zero-mean normalised cross-correlation with one template ------------------------------------------------------------------------
// tmpl = the (2R+1) x (2R+1) template t, row-major [k][j] over (ray offset k - R, slice offset j - R), already zero-mean with
// sum t^2 = 1 (the host prepares it in binary64).  W = (2R+1)^2.  For a sample (r, s) whose window lies inside the image, over the
// window in row-major order and from 0:  sum += x;  m = sum / W;  then again in that order  d = x - m,  c += t * d,  v += d * d;
// dst = v > vmin ? c / sqrt(v) : 0, with vmin = var_floor * W formed on the host in binary32.  Every operation is one correctly
// rounded binary32 operation.  The mean goes first on purpose: sumsq - sum^2 / W cancels without a useful bound.  A sample whose
// window leaves the image, and every padding slice (the whole pitch is written), gets 0.
__global__ __launch_bounds__(256) void k_sino_template_ncc(const float *__restrict__ src, float *__restrict__ dst, const float *__restrict__ tmpl,
                                                           int R, float vmin, int n, int nx, int sx)
{
#pragma clang fp contract(off)
    __shared__ float tile[MK_TROWS][MK_PITCH];
    __shared__ float tt[(2 * MK_RMAX + 1) * (2 * MK_RMAX + 1)];
    const int a = blockIdx.z, r0 = blockIdx.y * MK_ROWS, s0 = blockIdx.x * 64;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, s = s0 + lane, W = 2 * R + 1;
    for (int k = threadIdx.x; k < W * W; k += 256) tt[k] = tmpl[k];
    mk_load_tile(tile, src + (size_t)a * n * sx, r0, s0, R, n, nx, sx);
    float *D = dst + (size_t)a * n * sx;
    const float fw = (float)(W * W);
    const bool cols_inside = s - R >= 0 && s + R < nx;
    for (int q = 0; q < MK_ROWS / 4; ++q) {
        const int i = wave * (MK_ROWS / 4) + q, r = r0 + i;
        if (r >= n) break;                                  // the same in every lane
        float out = 0.f;
        if (cols_inside && r - R >= 0 && r + R < n) {
            float sum = 0.f;
            for (int k = 0; k < W; ++k)
                for (int j = 0; j < W; ++j) sum = sum + tile[i + k][lane + j];
            const float m = sum / fw;
            float c = 0.f, v = 0.f;
            for (int k = 0; k < W; ++k)
                for (int j = 0; j < W; ++j) {
                    const float d = tile[i + k][lane + j] - m;
                    const float td = tt[k * W + j] * d, dd = d * d;
                    c = c + td;
                    v = v + dd;
                }
            if (v > vmin) out = c / sqrtf(v);
        }
        D[(size_t)r * sx + s] = out;
    }
}

// ---- local maxima with their four neighbours -------------------------------------------------------------------------------------------
// (r, s) of projection a is a peak iff x >= threshold and, for every other sample (r', s') of its (2 radius + 1)^2 window clipped
// to the image, x > x' where (r', s') precedes (r, s) in row-major (r, s) order and x >= x' where it follows: of a plateau exactly
// the first sample qualifies; a NaN is never a peak and no sample with a NaN in its window is one (every comparison with a NaN
// fails).  count[a] is raised by 1 per peak (an integer atomic), and a peak whose ticket k is below capacity writes record
// rec[a][k] = {r, s, x, x(r-1, s), x(r+1, s), x(r, s-1), x(r, s+1), 0}: eight 32-bit words, a neighbour outside the image repeated as
// x.  count[a] ends as the true number of peaks whatever capacity is.
__global__ __launch_bounds__(256) void k_sino_peaks(const float *__restrict__ src, int *__restrict__ count, int4 *__restrict__ rec, int R,
                                                    float threshold, int capacity, int n, int nx, int sx)
{
    __shared__ float tile[MK_TROWS][MK_PITCH];
    const int a = blockIdx.z, r0 = blockIdx.y * MK_ROWS, s0 = blockIdx.x * 64;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, s = s0 + lane;
    mk_load_tile(tile, src + (size_t)a * n * sx, r0, s0, R, n, nx, sx);
    if (s >= nx) return;
    for (int q = 0; q < MK_ROWS / 4; ++q) {
        const int i = wave * (MK_ROWS / 4) + q, r = r0 + i;
        if (r >= n) break;
        const float x = tile[i + R][lane + R];
        bool ok = x >= threshold;
        if (ok) {
            for (int dr = -R; dr <= R; ++dr) {
                if (r + dr < 0 || r + dr >= n) continue;
                for (int ds = -R; ds <= R; ++ds) {
                    if (s + ds < 0 || s + ds >= nx || (dr == 0 && ds == 0)) continue;
                    const float y = tile[i + R + dr][lane + R + ds];
                    ok = ok && ((dr < 0 || (dr == 0 && ds < 0)) ? x > y : x >= y);
                }
            }
        }
        if (ok) {
            const int k = atomicAdd(count + a, 1);
            if (k < capacity) {
                const float up = r > 0 ? tile[i + R - 1][lane + R] : x, down = r + 1 < n ? tile[i + R + 1][lane + R] : x;
                const float left = s > 0 ? tile[i + R][lane + R - 1] : x, right = s + 1 < nx ? tile[i + R][lane + R + 1] : x;
                int4 *p = rec + ((size_t)a * capacity + k) * 2;
                p[0] = make_int4(r, s, __float_as_int(x), __float_as_int(up));
                p[1] = make_int4(__float_as_int(down), __float_as_int(left), __float_as_int(right), 0);
            }
        }
    }
}

}  // namespace tomo
