// kernels_pdhg.hip.h -- Chambolle-Pock (PDHG) iteration for  min_{x >= 0} 1/2 |Ax - b|^2 + lambda |grad x|_{2,1}
// Part of kernels.hip.h (include that, not this).
//
// One iteration = forward projection of xbar, k_pdhg_sino (dual sinogram), back projection, k_pdhg_tv (everything else).
// Conventions (x[s][y][z], all three axes alike, Neumann ends):
//   (grad x)_a[i] = x[i + 1_a] - x[i] where i_a < n_a - 1, else 0;   (div p)[i] = sum_a p_a[i] - p_a[i - 1_a], p_a[-1] = 0.
//   p_a at the last index of axis a is 0 by construction: the kernel writes 0 there whatever it read, and the divergence uses the new p,
//   so <grad x, p> = <x, -div p> holds exactly.  Padding slices (s >= nx) are no one's neighbour and are written as 0.
// Every float32 operation below is spelled out (__fmaf_rn, __fdiv_rn, __fsqrt_rn ...): the dual step is evaluated at a voxel by the
// wave that owns it AND by the waves that need it as a minus-neighbour, and both must produce the same bits.
#pragma once

namespace tomo {

constexpr int PD_TZ = 8;           // z-columns a wave owns (it evaluates the dual step on PD_TZ + 1: column z0 - 1 again)

struct PdhgArgs {
    float *x;                      // primal iterate, updated in place (only its own voxel reads it)
    const float *xbar, *u, *p0, *p1, *p2;   // extrapolated point, A^T q, the dual field (axis s, y, z)
    float *xbar_out, *q0, *q1, *q2;         // second buffers: neighbouring waves still read the old xbar and p
    const float *colsum;           // diagonal mode: sum_i |A_ij| per pixel
    float sigma, tau, lambda, theta;
};

// p_new = a / max(1, |a|_2 / lambda),  a_a = p_a + sigma (xbar[i + 1_a] - xbar[i])  (0 where the difference row does not exist)
__device__ __forceinline__ void pdhg_dual(float c, float cs, float cy, float cz, float p0, float p1, float p2, bool ms, bool my, bool mz,
                                          float sigma, float lambda, float &o0, float &o1, float &o2)
{
    const float a0 = ms ? __fmaf_rn(sigma, __fsub_rn(cs, c), p0) : 0.f;
    const float a1 = my ? __fmaf_rn(sigma, __fsub_rn(cy, c), p1) : 0.f;
    const float a2 = mz ? __fmaf_rn(sigma, __fsub_rn(cz, c), p2) : 0.f;
    const float nn = __fmaf_rn(a2, a2, __fmaf_rn(a1, a1, __fmul_rn(a0, a0)));
    const float r = __fdiv_rn(__fsqrt_rn(nn), lambda);
    const float inv = __fdiv_rn(1.f, fmaxf(1.f, r));
    o0 = __fmul_rn(a0, inv); o1 = __fmul_rn(a1, inv); o2 = __fmul_rn(a2, inv);
}

// ---- the fused pass: dual step, divergence, primal step, extrapolation ----------------------------------------------------------
// The barrier-free register march of k_tv_grad_reg: one wave = PD_TZ z-columns x 64 slices (lane = slice), rows marched along y.
//   slice neighbours   DPP wave shifts inside the chunk; beyond its edges the values are gathered once per row into packed registers
//                      (lane j = column j) and reach lane 0 / lane 63 through v_readlane + the DPP `old` operand.  p_new_s at the
//                      slice below the chunk is ONE packed evaluation of the dual step per row for all columns
//   y - 1              p_new_y of the previous row stays in registers; a segment's first row evaluates row y0 - 1 once, storing nothing
//   z - 1              p_new_z of the previous column stays in a register; column z0 - 1 is evaluated again by this wave
// Traffic per voxel: x, xbar, p0..p2, u read and x, xbar, p0..p2 written once = 44 B (the re-read halo columns and rows hit in L2).
// SUM: also sum (x_new - x)^2 into the partial-sum buffer.  PRECOND: T = 1 / (colsum + d), d = the difference rows that touch the voxel.
template <bool PRECOND, bool SUM>
__global__ __launch_bounds__(256) void k_pdhg_tv(PdhgArgs A, double *__restrict__ part, int n, int nx, int sx, int yseg)
{
    constexpr int TZ = PD_TZ;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int nzb = (n + TZ - 1) / TZ, nchunk = (nx + 63) >> 6, nys = (n + yseg - 1) / yseg;
    double acc = 0.0;
    // item = (y segment, z block, chunk), chunk fastest, an XCD-contiguous band of z blocks where they split evenly (k_tv_grad_reg's map)
    int bs, bz, ys;
    if ((nzb & 7) == 0) {
        const int zpx = nzb >> 3;
        const int64_t li = (int64_t)(blockIdx.x >> 3) * 4 + wave;
        bs = (int)(li % nchunk); bz = (int)(blockIdx.x & 7) * zpx + (int)((li / nchunk) % zpx); ys = (int)(li / ((int64_t)nchunk * zpx));
    } else {
        const int64_t item = (int64_t)blockIdx.x * 4 + wave;
        bs = (int)(item % nchunk); bz = (int)((item / nchunk) % nzb); ys = (int)(item / ((int64_t)nchunk * nzb));
    }
    if (ys < nys) {
        const int y0 = ys * yseg, y1 = min(y0 + yseg, n);
        const int z0 = bz * TZ, s0 = bs * 64, s = s0 + lane;
        const bool has_lo = s0 > 0, has_hi = s0 + 64 < nx;          // wave-uniform: the chunk has a neighbour below / above
        const bool valid = s < nx, ms = s < nx - 1;
        int zc[TZ + 2];                                             // columns z0 - 1 .. z0 + TZ, clamped into the image (masks decide what counts)
#pragma unroll
        for (int j = 0; j < TZ + 2; ++j) zc[j] = min(max(z0 - 1 + j, 0), n - 1);
        const int zlraw = z0 - 1 + min(lane, TZ + 1), zl = min(max(zlraw, 0), n - 1);      // packed registers: lane j = column j
        const bool mzl = zlraw >= 0 && zlraw < n - 1;
        auto shr = [&](float old, float v) {                        // lane l <- lane l-1 ; lane 0 keeps `old`
            return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, old), __builtin_bit_cast(int, v), 0x138, 0xf, 0xf, false));
        };
        auto shl = [&](float old, float v) {                        // lane l <- lane l+1 ; lane 63 keeps `old`
            return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, old), __builtin_bit_cast(int, v), 0x130, 0xf, 0xf, false));
        };
        auto lanev = [&](float v, int j) { return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), j)); };
        const int ystart = y0 > 0 ? y0 - 1 : 0;
        float c0[TZ + 2], cp[TZ + 2], pyp[TZ + 1];
#pragma unroll
        for (int j = 0; j <= TZ; ++j) pyp[j] = 0.f;                 // p_new_y of row y - 1 (row -1: 0)
#pragma unroll
        for (int j = 0; j < TZ + 2; ++j) c0[j] = A.xbar[(size_t)(ystart * n + zc[j]) * sx + (unsigned)s];
        float PE0 = has_lo ? A.xbar[(size_t)(ystart * n + zl) * sx + (unsigned)(s0 - 1)] : 0.f;   // xbar at slice s0 - 1, packed
        for (int y = ystart; y < y1; ++y) {
            const bool emit = y >= y0, my = y < n - 1;
            const int yn = min(y + 1, n - 1);
#pragma unroll
            for (int j = 0; j < TZ + 2; ++j) cp[j] = A.xbar[(size_t)(yn * n + zc[j]) * sx + (unsigned)s];
            const size_t pl = (size_t)(y * n + zl) * sx;
            // p_new_s at slice s0 - 1 of this row, all columns at once
            float PEp = 0.f, phs = 0.f;
            if (has_lo) {
                PEp = A.xbar[(size_t)(yn * n + zl) * sx + (unsigned)(s0 - 1)];
                const float pc = A.xbar[pl + (unsigned)s0];
                const float kz = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, PE0), 0x101, 0xf, 0xf, false));   // row_shl:1 -> column j + 1
                float o1, o2;
                pdhg_dual(PE0, pc, PEp, kz, A.p0[pl + (unsigned)(s0 - 1)], A.p1[pl + (unsigned)(s0 - 1)], A.p2[pl + (unsigned)(s0 - 1)],
                          true, my, mzl, A.sigma, A.lambda, phs, o1, o2);
            }
            const float PH = has_hi ? A.xbar[pl + (unsigned)(s0 + 64)] : 0.f;      // xbar at slice s0 + 64, packed
            float pzp = 0.f;                                        // p_new_z of column z - 1 (column -1: 0)
#pragma unroll
            for (int j = 0; j <= TZ; ++j) {
                const int z = z0 - 1 + j;
                if (z < 0 || z >= n) continue;                      // wave-uniform
                const size_t at = (size_t)(y * n + z) * sx + (unsigned)s;
                const float cs = shl(lanev(PH, j), c0[j]);
                float n0, n1, n2;
                pdhg_dual(c0[j], cs, cp[j], c0[j + 1], A.p0[at], A.p1[at], A.p2[at], ms, my, z < n - 1, A.sigma, A.lambda, n0, n1, n2);
                if (j >= 1) {
                    if (emit) {
                        const float psm = shr(lanev(phs, j), n0);  // p_new_s at slice s - 1 (slice -1: 0, phs is 0 without a chunk below)
                        const float dv = __fadd_rn(__fadd_rn(__fsub_rn(n0, s > 0 ? psm : 0.f), __fsub_rn(n1, pyp[j])), __fsub_rn(n2, pzp));
                        float T = A.tau;
                        if (PRECOND) {
                            const int d = (s > 0) + (s < nx - 1) + (y > 0) + (y < n - 1) + (z > 0) + (z < n - 1);
                            const float den = __fadd_rn(A.colsum[y * n + z], (float)d);
                            T = den > 0.f ? __fdiv_rn(1.f, den) : 0.f;
                        }
                        const float xo = A.x[at];
                        const float xn = fmaxf(__fmaf_rn(-T, __fsub_rn(A.u[at], dv), xo), 0.f);
                        const float dx = __fsub_rn(xn, xo);
                        if (SUM && valid) acc += (double)__fmul_rn(dx, dx);
                        A.x[at] = valid ? xn : 0.f;
                        A.xbar_out[at] = valid ? __fmaf_rn(A.theta, dx, xn) : 0.f;
                        A.q0[at] = valid ? n0 : 0.f;
                        A.q1[at] = valid ? n1 : 0.f;
                        A.q2[at] = valid ? n2 : 0.f;
                    }
                    pyp[j] = n1;
                }
                pzp = n2;
            }
#pragma unroll
            for (int j = 0; j < TZ + 2; ++j) c0[j] = cp[j];
            PE0 = PEp;
        }
    }
    if (SUM) block_accumulate(acc, part);
}

// ---- dual sinogram: q <- (q + S (g - b)) / (1 + S),  S = sigma, or 1 / rowsum per ray (0 for an empty ray) ------------------------
template <bool PRECOND>
__global__ __launch_bounds__(256) void k_pdhg_sino(f4 *__restrict__ q, const f4 *__restrict__ g, const f4 *__restrict__ b,
                                                    const float *__restrict__ rowsum, float sigma, int64_t n4, int sx4)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        float sg = sigma;
        if (PRECOND) { const float rs = rowsum[i / sx4]; sg = rs > 0.f ? __fdiv_rn(1.f, rs) : 0.f; }
        const float den = __fadd_rn(1.f, sg);
        const f4 qv = q[i], gv = g[i], bv = b[i];
        f4 r;
#pragma unroll
        for (int k = 0; k < 4; ++k) r[k] = __fdiv_rn(__fmaf_rn(sg, __fsub_rn(gv[k], bv[k]), qv[k]), den);
        q[i] = r;
    }
}

}  // namespace tomo
