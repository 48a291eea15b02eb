// kernels_align.hip.h -- tilt-series alignment on the sinogram layout: per-angle moments, windowed cross-correlation, resampling
// by shifts and by affine maps, per-slice mass profiles
// Part of kernels.hip.h (include that, not this: the families share helpers and constants in the order kernels.hip.h lists them).
//
// Projection a of a sinogram is the image X_a[r][s], ray r in [0, N), slice s in [0, Nslice): device row a * N + r, slice fastest,
// pitch sx.  The slices Nslice .. sx-1 are padding and are zero; every kernel here leaves them zero and none reads them as data.
// The sums are two-stage sums in a fixed order (kernels_geom.hip.h): the same bits from run to run.
#pragma once

namespace tomo {

// ---- per-angle moments: sum X, sum r X, sum s X over the real samples (cpu/utils/logger.py:237-247) ----------------------------
// Workgroup (blk, a) takes AL_MROWS rays of projection a.  A thread keeps one slice column (per = 64, 128 or 256 threads side by side
// on a row, the 256 / per row phases take alternate rows) and adds in binary64 from the first sample on: x, r * x and s * x are exact
// there, so the only roundings are binary64 additions.  One triple per workgroup (block_sum_row); k_sum_rows_ascending adds the
// workgroups' triples and forms the means.
constexpr int AL_MROWS = 32;

__global__ __launch_bounds__(256) void k_sino_moments(const float *__restrict__ g, double *__restrict__ part, int n, int nx, int sx)
{
    const int a = blockIdx.y, blk = blockIdx.x;
    const int per = sx >= 256 ? 256 : (sx >= 128 ? 128 : 64), phase = threadIdx.x / per, nphase = 256 / per, col = threadIdx.x % per;
    const int r0 = blk * AL_MROWS, r1 = min(n, r0 + AL_MROWS);
    const float *base = g + (size_t)a * n * sx;
    double acc[3] = {0.0, 0.0, 0.0};
    for (int r = r0 + phase; r < r1; r += nphase)
        for (int s = col; s < nx; s += per) {
            const double x = (double)base[(size_t)r * sx + s];
            acc[0] += x; acc[1] += (double)r * x; acc[2] += (double)s * x;
        }
    block_sum_row<3>(acc, part + ((size_t)a * gridDim.x + blk) * 3);
}

// ---- windowed cross-correlation ------------------------------------------------------------------------------------------------
// C_a(u, v) = sum_{r, s} (A_a[r][s] - mA_a) (B_a[r + u][s + v] - mB_a) over the (r, s) with both samples inside the image, for
// (u, v) in [-S_MAX, S_MAX]^2 (the launcher picks the smallest S_MAX >= S and k_sino_xcorr_finish keeps [-S, S]^2).  Not divided by
// the overlap: a window entry at |u|, |v| > 0 sums over (N - |u|)(Nslice - |v|) samples, which leans the peak towards zero shift
// by a factor (1 - |u| / N)(1 - |v| / Nslice) -- negligible for S << N, and what the FFT correlation of zero-padded images gives.
//
// Lane = slice.  Workgroup (cg, rb, a) owns the B rows rho in [AL_R rb, AL_R (rb + 1)) of projection a and the 64-slice chunks
// [AL_KC cg, AL_KC (cg + 1)); wave w owns 16 of those rows.  Per chunk it stages B - mB for its rows with a halo of slices (v shifts
// are then reads of consecutive lanes at a constant offset) and A - mA for the rows rho - u it can meet; whatever lies outside the
// image, the pitch padding included, is staged as 0 and so contributes nothing.  The (2 S_MAX + 1)^2 sums do not fit in registers:
// the window is cut into tiles of TU x TV entries, one pass per tile; per B row a pass reads TV window values and TU rows of A and
// issues TU * TV FMAs, (TU + TV) / (TU TV) LDS reads per FMA.  All LDS reads are 4-byte, consecutive lanes on consecutive banks.
// A lane's sum runs over its 16 rows of up to AL_KC chunks -- a binary32 FMA chain of at most 16 * AL_KC links -- then over the 64
// lanes in a tree of depth 6 (4 DPP steps inside a row of 16 lanes, the four rows pairwise), then over the four waves, the
// workgroups and the passes in binary64 in index order.  tests/ref64_align.py derives its error bound from exactly this order.
constexpr int AL_R = 64, AL_KC = 4;

template <int CTRL> __device__ __forceinline__ float al_dpp(float v)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, false));
}
// sum over the 64 lanes, the same bits in every lane that reads it (an addition commutes): quad_perm [1,0,3,2], [2,3,0,1],
// row_half_mirror, row_mirror, then the four rows of 16 as (0 + 1) + (2 + 3)
__device__ __forceinline__ float al_wave_sum(float v)
{
    v += al_dpp<0xB1>(v); v += al_dpp<0x4E>(v); v += al_dpp<0x141>(v); v += al_dpp<0x140>(v);
    auto row = [&](int l) { return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l)); };
    return (row(0) + row(16)) + (row(32) + row(48));
}

template <int S_MAX, int TU, int TV>
__global__ __launch_bounds__(256) void k_sino_xcorr(const float *__restrict__ A, const float *__restrict__ B,
                                                    const float *__restrict__ meanA, const float *__restrict__ meanB,
                                                    double *__restrict__ part, int n, int nx, int sx, int nchunk)
{
    constexpr int W = 2 * S_MAX + 1, NTU = (W + TU - 1) / TU, NTV = (W + TV - 1) / TV, UP = NTU * TU, VP = NTV * TV;
    constexpr int AROWS = AL_R + UP - 1, BW = 64 + VP - 1, ALO = UP - 1 - S_MAX;   // A rows rho0 - ALO ..; B slices c0 - S_MAX ..
    __shared__ float sA[AROWS * 64];
    __shared__ float sB[AL_R * BW];
    __shared__ float red[4][TU * TV];
    const int a = blockIdx.z, rb = blockIdx.y, cg = blockIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int rho0 = rb * AL_R;
    const float mA = meanA ? meanA[a] : 0.f, mB = meanB ? meanB[a] : 0.f;
    const float *Aa = A + (size_t)a * n * sx, *Ba = B + (size_t)a * n * sx;
    const int ch0 = cg * AL_KC, ch1 = min(nchunk, ch0 + AL_KC);
    const int i0 = 16 * wave, i1 = min(i0 + 16, n - rho0);          // this wave's B rows (LDS row index); rows past the image: none
    double *out = part + ((size_t)a * gridDim.y * gridDim.x + (size_t)rb * gridDim.x + cg) * (W * W);
    for (int t = 0; t < NTU * NTV; ++t) {
        const int ui0 = (t / NTV) * TU, vi0 = (t % NTV) * TV;       // this pass: u = ui0 + j - S_MAX, v = vi0 + k - S_MAX
        float acc[TU][TV];
#pragma unroll
        for (int j = 0; j < TU; ++j)
#pragma unroll
            for (int k = 0; k < TV; ++k) acc[j][k] = 0.f;
        for (int ch = ch0; ch < ch1; ++ch) {
            const int c0 = ch * 64;
            __syncthreads();                                        // the previous chunk's (and pass's) readers are done
            for (int i = wave; i < AROWS; i += 4) {
                const int r = rho0 - ALO + i, s = c0 + lane;
                sA[i * 64 + lane] = (r >= 0 && r < n && s < nx) ? Aa[(size_t)r * sx + s] - mA : 0.f;
            }
            for (int idx = threadIdx.x; idx < AL_R * BW; idx += 256) {
                const int i = idx / BW, j = idx - i * BW;
                const int rho = rho0 + i, s = c0 - S_MAX + j;
                sB[idx] = (rho < n && s >= 0 && s < nx) ? Ba[(size_t)rho * sx + s] - mB : 0.f;
            }
            __syncthreads();
            for (int i = i0; i < i1; ++i) {
                const float *pb = sB + i * BW + lane + vi0;
                const float *pa = sA + (i + UP - 1 - ui0) * 64 + lane;     // row rho - u of A: LDS row i + ALO - (ui0 + j - S_MAX)
                float b[TV], av[TU];
#pragma unroll
                for (int k = 0; k < TV; ++k) b[k] = pb[k];
#pragma unroll
                for (int j = 0; j < TU; ++j) av[j] = pa[-64 * j];
#pragma unroll
                for (int j = 0; j < TU; ++j)
#pragma unroll
                    for (int k = 0; k < TV; ++k) acc[j][k] = fmaf(av[j], b[k], acc[j][k]);
            }
        }
#pragma unroll
        for (int j = 0; j < TU; ++j)
#pragma unroll
            for (int k = 0; k < TV; ++k) {
                const float s = al_wave_sum(acc[j][k]);
                if (lane == 0) red[wave][j * TV + k] = s;
            }
        __syncthreads();
        if (threadIdx.x < TU * TV) {
            const int ui = ui0 + threadIdx.x / TV, vi = vi0 + threadIdx.x % TV;
            if (ui < W && vi < W)
                out[ui * W + vi] = (((double)red[0][threadIdx.x] + (double)red[1][threadIdx.x]) + (double)red[2][threadIdx.x]) + (double)red[3][threadIdx.x];
        }
    }
}

// C[a][u + S][v + S] = the workgroups' sums in ascending order; part holds windows of half-width smax per (angle, workgroup)
__global__ void k_sino_xcorr_finish(const double *__restrict__ part, double *__restrict__ C, int np, int nblk, int smax, int S)
{
    const int w = 2 * S + 1, wm = 2 * smax + 1;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= np * w * w) return;
    const int a = i / (w * w), q = i - a * w * w, u = q / w - S, v = q % w - S;
    const double *p = part + (size_t)a * nblk * wm * wm + (u + smax) * wm + (v + smax);
    double s = 0.0;
    for (int b = 0; b < nblk; ++b) s += p[(size_t)b * wm * wm];
    C[i] = s;
}

// ---- resampling by per-angle shifts (cpu/utils/logger.py:249-250 with WRAP and whole-pixel shifts) ------------------------------
// dst_a[r][s] = bilinear(src_a)(r - dr_a, s - ds_a).  The host splits -d into floor and fraction: tab[a] = {kr, ks, bits of tr, bits
// of ts}, so the four taps are rows r + kr, r + kr + 1 and slices s + ks, s + ks + 1 with weights (1 - tr, tr) x (1 - ts, ts).  A tap
// outside the image is 0, or with WRAP the sample modulo the image size (the host gives kr in [0, N), ks in [0, Nslice) then).  The
// value is bilinear_value (kernels_geom.hip.h): a whole-pixel shift copies the source value.  Padding slices of dst are written as zero.
template <bool WRAP>
__global__ __launch_bounds__(256) void k_sino_shift(const float *__restrict__ src, float *__restrict__ dst, const int4 *__restrict__ tab,
                                                    int n, int nx, int sx)
{
    const int a = blockIdx.y;
    const int4 t = tab[a];
    const int kr = t.x, ks = t.y;
    const float tr = __int_as_float(t.z), ts = __int_as_float(t.w);
    const float *S = src + (size_t)a * n * sx;
    float *D = dst + (size_t)a * n * sx;
    auto fetch = [&](int i, int j) -> float {
        if constexpr (WRAP) { if (i >= n) i -= n; if (j >= nx) j -= nx; }
        else if (i < 0 || i >= n || j < 0 || j >= nx) return 0.f;
        return S[(size_t)i * sx + j];
    };
    const int total = n * sx;
    for (int idx = blockIdx.x * 256 + threadIdx.x; idx < total; idx += gridDim.x * 256) {
        const int r = idx / sx, s = idx - r * sx;
        D[idx] = s < nx ? bilinear_value(fetch, r + kr, s + ks, tr, ts) : 0.f;
    }
}

// ---- resampling by per-angle affine maps (in-plane rotation, magnification, shift in one interpolation) -------------------------
// dst_a[r][s] = bilinear(src_a)(r', s') with r' = m00 r + m01 s + m02, s' = m10 r + m11 s + m12, mat[a] = {m00, m01, m02, m10, m11,
// m12} in binary64.  The layout and the grid are k_sino_shift's: lane = slice, s fastest, one 4-byte write per element, coalesced;
// the reads of a wave are the source row(s) its destination row maps to -- for the few degrees of a tilt-axis correction a wave's 64
// slices touch a handful of neighbouring source rows, 256-byte runs that the L2 serves.  The coordinates are binary64, evaluated
// per element as fma(m00, r, fma(m01, s, m02)) and split by axis_split<SPLIT_ZERO_PAD> (kernels_geom.hip.h).  Four binary64 FMAs,
// two floors and two conversions per element beside one read and one write: at half the binary32 rate still an order below the time
// the bytes take.  The value is the bilinear_value that k_sino_shift evaluates: an identity copies the source bits, a pure
// translation gives tomo_sino_shift's bits (wrap = 0) and an Inf next to a copied sample stays out of the sum.  A tap outside
// [0, n) x [0, nx) is 0; a coordinate outside (-1, n) x (-1, nx) has no tap inside and gives 0 (a NaN from Inf - Inf of huge finite
// entries lands here too).  Padding slices of dst are written as zero.
__global__ __launch_bounds__(256) void k_sino_affine(const float *__restrict__ src, float *__restrict__ dst, const double *__restrict__ mat,
                                                     int n, int nx, int sx)
{
    const int a = blockIdx.y;
    const double *m = mat + 6 * (size_t)a;
    const double m00 = m[0], m01 = m[1], m02 = m[2], m10 = m[3], m11 = m[4], m12 = m[5];
    const float *S = src + (size_t)a * n * sx;
    float *D = dst + (size_t)a * n * sx;
    auto fetch = [&](int i, int j) -> float {
        if (i < 0 || i >= n || j < 0 || j >= nx) return 0.f;
        return S[(size_t)i * sx + j];
    };
    const int total = n * sx;
    for (int idx = blockIdx.x * 256 + threadIdx.x; idx < total; idx += gridDim.x * 256) {
        const int r = idx / sx, s = idx - r * sx;
        float o = 0.f;
        if (s < nx) {
            const double rp = fma(m00, (double)r, fma(m01, (double)s, m02));
            const double sp = fma(m10, (double)r, fma(m11, (double)s, m12));
            int i, j;
            float tr, ts;
            if (axis_split<SPLIT_ZERO_PAD>(rp, n, i, tr) && axis_split<SPLIT_ZERO_PAD>(sp, nx, j, ts)) o = bilinear_value(fetch, i, j, tr, ts);
        }
        D[idx] = o;
    }
}

// ---- per-slice mass profile: c_a[s] = sum_r X_a[r][s] (the common line of a parallel-beam series: the same for every tilt) --------
// Workgroup (ch, blk, a) takes the 64 slices [64 ch, 64 ch + 64) of AL_PROWS rays of projection a.  Lane = slice: wave w adds rows
// r0 + w, r0 + w + 4, ... in ascending order, in binary64 from the first sample (a row read of a wave is 256 consecutive bytes); the
// four waves' sums are added in wave order, one value per (angle, workgroup, slice) -- lane-wise, with no sum across lanes, so this
// is not block_sum_row -- and k_sum_rows_ascending adds the workgroups' rows.
constexpr int AL_PROWS = 64;

__global__ __launch_bounds__(256) void k_sino_axis_profile(const float *__restrict__ g, double *__restrict__ part, int n, int nx, int sx)
{
    __shared__ double red[4][64];
    const int a = blockIdx.z, blk = blockIdx.y, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int s = blockIdx.x * 64 + lane;
    const int r0 = blk * AL_PROWS, r1 = min(n, r0 + AL_PROWS);
    const float *base = g + (size_t)a * n * sx;
    double acc = 0.0;
    if (s < nx)
        for (int r = r0 + w; r < r1; r += 4) acc += (double)base[(size_t)r * sx + s];
    red[w][lane] = acc;
    __syncthreads();
    if (w == 0 && s < nx) part[((size_t)a * gridDim.y + blk) * nx + s] = ((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane];
}

}  // namespace tomo
