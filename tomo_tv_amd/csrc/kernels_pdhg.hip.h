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

// SLAB: the planes of a slab of a sharded volume, dense [y][z] (n * n floats each).  The slice below the slab (lo = xbar, p0, p1, p2)
// and xbar of the slice above (hi) stand in for the neighbours' slices; the pass leaves what the neighbours need next in send_first
// (xbar_new of slice 0) and send_last (xbar_new, p0_new, p1_new, p2_new of slice nx - 1).  first / last: the slab holds the volume's end.
struct PdhgSlab {
    const float *lo, *hi;
    float *send_first, *send_last;
    int first, last;
};

// the same, left as a and 1 / max(1, |a|_2 / lambda): p_new = a * inv
__device__ __forceinline__ void pdhg_dual_parts(float c, float cs, float cy, float cz, float p0, float p1, float p2, bool ms, bool my, bool mz,
                                                float sigma, float lambda, float &a0, float &a1, float &a2, float &inv)
{
    a0 = ms ? __fmaf_rn(sigma, __fsub_rn(cs, c), p0) : 0.f;
    a1 = my ? __fmaf_rn(sigma, __fsub_rn(cy, c), p1) : 0.f;
    a2 = mz ? __fmaf_rn(sigma, __fsub_rn(cz, c), p2) : 0.f;
    const float nn = __fmaf_rn(a2, a2, __fmaf_rn(a1, a1, __fmul_rn(a0, a0)));
    inv = __fdiv_rn(1.f, fmaxf(1.f, __fdiv_rn(__fsqrt_rn(nn), lambda)));
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
// SLAB: a slab face that is not the volume's end is a chunk edge whose neighbour slice lies in a plane: chunk 0 evaluates p_new_s of the
//   slice below from the lo planes (the packed evaluation, same bits as the neighbour's own), and xbar of the slice above reaches the
//   lane of slice nx - 1 through lane 63's packed register (nx % 64 == 0) or stands in for the padding slice nx in that lane's upper
//   neighbour (a partial chunk: that lane stores 0 like every padding lane).  d counts the difference rows of the global volume.
template <bool PRECOND, bool SUM, bool SLAB>
__global__ __launch_bounds__(256) void k_pdhg_tv(PdhgArgs A, double *__restrict__ part, int n, int nx, int sx, int yseg, PdhgSlab E)
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
        const bool valid = s < nx, ms = s < nx - 1 || (SLAB && s == nx - 1 && !E.last);
        const bool lo_pl = SLAB && s0 == 0 && !E.first;            // wave-uniform: slice s0 - 1 is the lo planes
        const bool hi_pl = SLAB && !has_hi && !E.last;             // wave-uniform: slice nx is the hi plane ...
        const bool hi_edge = hi_pl && s0 + 64 == nx, hi_mid = hi_pl && s0 + 64 > nx;   // ... beyond lane 63, or at the lane of slice nx
        const bool below = s > 0 || (SLAB && !E.first), above = s < nx - 1 || (SLAB && !E.last);   // the difference rows along s exist
        const int npix = n * n;
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
        if (SLAB && lo_pl) PE0 = E.lo[ystart * n + zl];
        if (SLAB && hi_mid) {
            const float h = E.hi[ystart * n + zl];
#pragma unroll
            for (int j = 0; j < TZ + 2; ++j) c0[j] = s == nx ? lanev(h, j) : c0[j];
        }
        for (int y = ystart; y < y1; ++y) {
            const bool emit = y >= y0, my = y < n - 1;
            const int yn = min(y + 1, n - 1);
#pragma unroll
            for (int j = 0; j < TZ + 2; ++j) cp[j] = A.xbar[(size_t)(yn * n + zc[j]) * sx + (unsigned)s];
            if (SLAB && hi_mid) {
                const float h = E.hi[yn * n + zl];
#pragma unroll
                for (int j = 0; j < TZ + 2; ++j) cp[j] = s == nx ? lanev(h, j) : cp[j];
            }
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
            } else if (SLAB && lo_pl) {
                const int at = y * n + zl;
                PEp = E.lo[yn * n + zl];
                const float pc = A.xbar[pl];
                const float kz = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, PE0), 0x101, 0xf, 0xf, false));
                float o1, o2;
                pdhg_dual(PE0, pc, PEp, kz, E.lo[npix + at], E.lo[2 * npix + at], E.lo[3 * npix + at], true, my, mzl, A.sigma, A.lambda, phs, o1, o2);
            }
            float PH = has_hi ? A.xbar[pl + (unsigned)(s0 + 64)] : 0.f;            // xbar at slice s0 + 64, packed
            if (SLAB && hi_edge) PH = E.hi[y * n + zl];
            float pzp = 0.f;                                        // p_new_z of column z - 1 (column -1: 0)
#pragma unroll
            for (int j = 0; j <= TZ; ++j) {
                const int z = z0 - 1 + j;
                if (z < 0 || z >= n) continue;                      // wave-uniform
                const size_t at = (size_t)(y * n + z) * sx + (unsigned)s;
                const float cs = shl(lanev(PH, j), c0[j]);
                float n0, n1, n2, b0 = 0.f, b1 = 0.f, b2 = 0.f, binv = 0.f;
                if (SLAB) {
                    pdhg_dual_parts(c0[j], cs, cp[j], c0[j + 1], A.p0[at], A.p1[at], A.p2[at], ms, my, z < n - 1, A.sigma, A.lambda, b0, b1, b2, binv);
                    n0 = __fmul_rn(b0, binv); n1 = __fmul_rn(b1, binv); n2 = __fmul_rn(b2, binv);
                    asm volatile("" : "+v"(n0), "+v"(n1), "+v"(n2));       // the rounded products: nothing below may fuse them again
                } else {
                    pdhg_dual(c0[j], cs, cp[j], c0[j + 1], A.p0[at], A.p1[at], A.p2[at], ms, my, z < n - 1, A.sigma, A.lambda, n0, n1, n2);
                }
                if (j >= 1) {
                    if (emit) {
                        const float psm = shr(lanev(phs, j), n0);  // p_new_s at slice s - 1 (slice -1: 0, phs is 0 without a chunk below)
                        float dv;
                        if (SLAB) {
                            // The divergence of the whole-volume form, operation for operation.  The *_rn helpers are plain operators to
                            // the compiler, and in the SLAB = false code it fuses the product a * inv into the subtraction of the s term
                            // (and of the z term in the wave's last column, whose p_new_z no next column needs), so x_new sees
                            // unrounded products there.  A sharded run must give those bits (tests/test_gpu_pdhg_sharded.py holds the
                            // two forms together): spelled out here.
                            const float t0 = __fmaf_rn(b0, binv, -(below ? psm : 0.f));
                            const float t1 = n1 - pyp[j];
                            const float t2 = j == TZ ? __fmaf_rn(b2, binv, -pzp) : n2 - pzp;
                            dv = (t0 + t1) + t2;
                        } else {
                            dv = __fadd_rn(__fadd_rn(__fsub_rn(n0, below ? psm : 0.f), __fsub_rn(n1, pyp[j])), __fsub_rn(n2, pzp));
                        }
                        float T = A.tau;
                        if (PRECOND) {
                            const int d = below + above + (y > 0) + (y < n - 1) + (z > 0) + (z < n - 1);
                            const float den = __fadd_rn(A.colsum[y * n + z], (float)d);
                            T = den > 0.f ? __fdiv_rn(1.f, den) : 0.f;
                        }
                        const float xo = A.x[at];
                        const float xn = fmaxf(__fmaf_rn(-T, __fsub_rn(A.u[at], dv), xo), 0.f);
                        const float dx = __fsub_rn(xn, xo);
                        if (SUM && valid) acc += (double)__fmul_rn(dx, dx);
                        A.x[at] = valid ? xn : 0.f;
                        const float xb = __fmaf_rn(A.theta, dx, xn);
                        A.xbar_out[at] = valid ? xb : 0.f;
                        A.q0[at] = valid ? n0 : 0.f;
                        A.q1[at] = valid ? n1 : 0.f;
                        A.q2[at] = valid ? n2 : 0.f;
                        if (SLAB) {
                            const int pa = y * n + z;
                            if (s == 0 && !E.first) E.send_first[pa] = xb;
                            if (s == nx - 1 && !E.last) {
                                E.send_last[pa] = xb; E.send_last[npix + pa] = n0; E.send_last[2 * npix + pa] = n1; E.send_last[3 * npix + pa] = n2;
                            }
                        }
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
