// kernels_common.hip.h -- vector helpers, block reductions, layout conversion at the host boundary and at the device boundary
// Part of kernels.hip.h (include that, not this: the families share helpers and constants in the order kernels.hip.h lists them).
#pragma once

namespace tomo {


// ---- small vector helpers -----------------------------------------------------------------------
template <int V> struct VecOf;
template <> struct VecOf<1> { typedef float T; };
template <> struct VecOf<2> { typedef float T __attribute__((ext_vector_type(2))); };
template <> struct VecOf<4> { typedef float T __attribute__((ext_vector_type(4))); };

template <int V> __device__ __forceinline__ typename VecOf<V>::T vzero();
template <> __device__ __forceinline__ float vzero<1>() { return 0.f; }
template <> __device__ __forceinline__ VecOf<2>::T vzero<2>() { VecOf<2>::T v = {0.f, 0.f}; return v; }
template <> __device__ __forceinline__ VecOf<4>::T vzero<4>() { VecOf<4>::T v = {0.f, 0.f, 0.f, 0.f}; return v; }

template <int V> __device__ __forceinline__ float velem(const typename VecOf<V>::T &v, int i);
template <> __device__ __forceinline__ float velem<1>(const float &v, int) { return v; }
template <> __device__ __forceinline__ float velem<2>(const VecOf<2>::T &v, int i) { return v[i]; }
template <> __device__ __forceinline__ float velem<4>(const VecOf<4>::T &v, int i) { return v[i]; }

template <int V> __device__ __forceinline__ void vset(typename VecOf<V>::T &v, int i, float f);
template <> __device__ __forceinline__ void vset<1>(float &v, int, float f) { v = f; }
template <> __device__ __forceinline__ void vset<2>(VecOf<2>::T &v, int i, float f) { v[i] = f; }
template <> __device__ __forceinline__ void vset<4>(VecOf<4>::T &v, int i, float f) { v[i] = f; }

// ---- block reduction of a double into one of NPART partial slots ----------------------------------
constexpr int NPART = 256;

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

// all threads of a 256-thread block call this; one atomic per block
__device__ __forceinline__ void block_accumulate(double v, double *__restrict__ part)
{
    __shared__ double red[4];
    v = wave_sum(v);
    int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) red[w] = v;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(&part[blockIdx.x & (NPART - 1)], red[0] + red[1] + red[2] + red[3]);
}

// Non-temporal access by experiment bit (make EXTRA=-DTOMO_NT=<mask>); bits that paid are folded into NT_DEFAULT.
#ifndef TOMO_NT
#define TOMO_NT 0
#endif
#ifndef TOMO_NT_OFF   // experiment: bits of NT_DEFAULT switched off
#define TOMO_NT_OFF 0
#endif
constexpr int NT_DEFAULT = 32 | 256;   // 32: k_fp_tile partial sums (SIRT iteration -5 %); 256: k_fgp_fused outputs (-4 %)
template <int BIT, typename T>
__device__ __forceinline__ T nt_ld(const T *p)
{
    if constexpr (((TOMO_NT | NT_DEFAULT) & ~TOMO_NT_OFF & BIT) != 0) return __builtin_nontemporal_load(p);
    else return *p;
}
template <int BIT, typename T>
__device__ __forceinline__ void nt_st(T v, T *p)
{
    if constexpr (((TOMO_NT | NT_DEFAULT) & ~TOMO_NT_OFF & BIT) != 0) {
        __builtin_nontemporal_store(v, p);
    } else *p = v;
}

__global__ void k_finalize(double *__restrict__ part, double *__restrict__ dst)
{
    double v = part[threadIdx.x];  // launched with NPART threads
    part[threadIdx.x] = 0.0;       // leave the buffer ready for the next reduction (no memset launch per reduction)
    __shared__ double red[NPART / 64];
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0;
        for (int i = 0; i < NPART / 64; ++i) s += red[i];
        *dst = s;
    }
}

// ---- layout conversion at the host boundary -------------------------------------------------------
// host [ns][m]  ->  device [m][sx]   (padding slices written as zero)
__global__ __launch_bounds__(256) void k_transpose_in(const float *__restrict__ src, float *__restrict__ dst,
                                                       int ns, int64_t m, int sx)
{
    __shared__ float tile[32][33];
    int64_t m0 = (int64_t)blockIdx.x * 32;
    int s0 = blockIdx.y * 32;
    int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
    for (int r = ty; r < 32; r += 8) {
        int s = s0 + r;
        int64_t mm = m0 + tx;
        tile[r][tx] = (s < ns && mm < m) ? src[(int64_t)s * m + mm] : 0.f;
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
        int64_t mm = m0 + r;
        int s = s0 + tx;
        if (mm < m && s < sx) dst[mm * sx + s] = tile[tx][r];
    }
}

// device [m][sx] -> host [ns][m]
__global__ __launch_bounds__(256) void k_transpose_out(const float *__restrict__ src, float *__restrict__ dst,
                                                        int ns, int64_t m, int sx)
{
    __shared__ float tile[32][33];
    int64_t m0 = (int64_t)blockIdx.x * 32;
    int s0 = blockIdx.y * 32;
    int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int r = ty; r < 32; r += 8) {
        int64_t mm = m0 + r;
        int s = s0 + tx;
        tile[r][tx] = (mm < m && s < sx) ? src[mm * sx + s] : 0.f;
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
        int s = s0 + r;
        int64_t mm = m0 + tx;
        if (s < ns && mm < m) dst[(int64_t)s * m + mm] = tile[tx][r];
    }
}

// ---- layout conversion at the device boundary (tomo_set_*_device / tomo_get_*_device) ------------------------------------
// The caller's buffer ext is dense [ns][m] of T (float or double), the engine's dev is [m][sx] floats.  With PUBLIC the caller's
// sinogram is [s][ray][angle]: column j = ray * nang + angle of ext is row angle * nray + ray of dev, so the pack of
// pytvlib.pack_tilt_series is a permutation of the ROWS dev is addressed by -- ext is still read along its contiguous index and
// dev still written along slices.  A workgroup moves 32 columns x 64 slices as two 32 x 32 tiles through LDS; every thread moves
// four consecutive columns on the ext side and four consecutive slices on the dev side (16 bytes of float each; VEC: as one access,
// which needs m % 4 == 0 and a 16-byte aligned ext).  Tile pitch 33: in a 32-lane group of a ds_read_b32 / ds_write_b32 eight
// lanes x 4 columns of four consecutive rows fall on banks 4 l + r + const (mod 32), all distinct, on either side.
constexpr int IO_TJ = 32, IO_TS = 64;

template <typename T> struct IoVec4;
template <> struct IoVec4<float> { typedef float T __attribute__((ext_vector_type(4))); };
template <> struct IoVec4<double> { typedef double T __attribute__((ext_vector_type(4))); };

template <bool PUBLIC>
__device__ __forceinline__ int64_t io_row(int64_t j, int nang, int nray)
{
    if constexpr (PUBLIC) { uint32_t ray = (uint32_t)j / (uint32_t)nang, ang = (uint32_t)j - ray * (uint32_t)nang; return (int64_t)ang * nray + ray; }
    else return j;
}

// ext -> dev; T = double rounds to nearest even (the conversion of a C cast); slices ns <= s < sx are written as zero
template <typename T, bool PUBLIC, bool VEC>
__global__ __launch_bounds__(256) void k_io_in(const T *__restrict__ ext, float *__restrict__ dev, int ns, int64_t m, int sx,
                                               int nang, int nray)
{
    __shared__ float tile[2][32][33];
    const int64_t j0 = (int64_t)blockIdx.x * IO_TJ;
    const int s0 = blockIdx.y * IO_TS;
    const int r = threadIdx.x >> 3, c = (threadIdx.x & 7) * 4;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int s = s0 + 32 * h + r;
        const int64_t j = j0 + c;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (s < ns) {
            const T *p = ext + (int64_t)s * m + j;
            if constexpr (VEC) {
                if (j < m) { typename IoVec4<T>::T q = *reinterpret_cast<const typename IoVec4<T>::T *>(p); for (int k = 0; k < 4; ++k) v[k] = (float)q[k]; }
            } else {
                for (int k = 0; k < 4; ++k) if (j + k < m) v[k] = (float)p[k];
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) tile[h][r][c + k] = v[k];
    }
    __syncthreads();
    const int64_t j = j0 + r;
    if (j >= m) return;
    float *q = dev + io_row<PUBLIC>(j, nang, nray) * sx + s0 + c;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        VecOf<4>::T v = {tile[h][c][r], tile[h][c + 1][r], tile[h][c + 2][r], tile[h][c + 3][r]};
        *reinterpret_cast<VecOf<4>::T *>(q + 32 * h) = v;
    }
}

// dev -> ext; writes ext[s][j] for s < ns, j < m only
template <typename T, bool PUBLIC, bool VEC>
__global__ __launch_bounds__(256) void k_io_out(const float *__restrict__ dev, T *__restrict__ ext, int ns, int64_t m, int sx,
                                                int nang, int nray)
{
    __shared__ float tile[2][32][33];
    const int64_t j0 = (int64_t)blockIdx.x * IO_TJ;
    const int s0 = blockIdx.y * IO_TS;
    const int r = threadIdx.x >> 3, c = (threadIdx.x & 7) * 4;
    if (j0 + r < m) {
        const float *q = dev + io_row<PUBLIC>(j0 + r, nang, nray) * sx + s0 + c;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            VecOf<4>::T v = *reinterpret_cast<const VecOf<4>::T *>(q + 32 * h);
#pragma unroll
            for (int k = 0; k < 4; ++k) tile[h][c + k][r] = v[k];
        }
    }
    __syncthreads();
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int s = s0 + 32 * h + r;
        const int64_t j = j0 + c;
        if (s >= ns || j >= m) continue;
        T *p = ext + (int64_t)s * m + j;
        if constexpr (VEC) {
            typename IoVec4<T>::T o = {(T)tile[h][r][c], (T)tile[h][r][c + 1], (T)tile[h][r][c + 2], (T)tile[h][r][c + 3]};
            *reinterpret_cast<typename IoVec4<T>::T *>(p) = o;
        } else {
            for (int k = 0; k < 4; ++k) if (j + k < m) p[k] = (T)tile[h][r][c + k];
        }
    }
}

__global__ void k_scatter_slice(const float *__restrict__ img, float *__restrict__ vol, int64_t m, int sx, int s)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < m) vol[i * sx + s] = img[i];
}

__global__ void k_gather_slice(const float *__restrict__ vol, float *__restrict__ img, int64_t m, int sx, int s)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < m) img[i] = vol[i * sx + s];
}

// vector register blocks the asm loops of the list projectors and of the resident sweep bind (v[64:127], s[36:67] ...)
typedef float v2f __attribute__((ext_vector_type(2)));
typedef float v32f __attribute__((ext_vector_type(32)));
typedef uint32_t u16v __attribute__((ext_vector_type(16)));

}  // namespace tomo
