// tv_form.h -- which TV kernel runs and on what grid: the host-only decision of engine_tv.inc / engine_fgp.inc (no HIP header, so the CPU
// checks it: tests/native/tv_form_check.cpp).  select_tv is the ONE place that reads the "tv_*" switches; the launchers ask the TvForm.
//   descent (gradient / norm + update): lds 1 + recompute: MARCH4 (tz 8 and march4) else REG (tz); lds 1 alone: REG (tz 8, g stored);
//                                       lds 16: LDS16; every other non-zero lds: LDS8; lds 0: DIRECT
//   value (tomo_tv_partial):            lds 1: MARCH4 (march4, no edge lanes) else REG; lds 8: LDS8; every other lds: DIRECT (k_tv_value)
// Two rules a reader would not guess (kept as they are):
//  * the value pass ignores "tv_tz": its march is always 8 columns wide, and k_tv_march4 runs it only on shapes without edge lanes;
//  * a non-zero lds other than 1, 8, 16 (say 4) descends by k_tv_grad_lds<8> like lds 8, but only lds 8 (and 1) fold the TV value into the
//    first gradient pass or evaluate it by their march: lds 4 takes its value from the direct stencil, like 16 and 0.
#pragma once
#include <cstdint>

namespace tomo {
constexpr int TV_YSEG_MIN = 8, TV_WAVES_WANTED = 4096;   // round 3: the march holds 4 waves per SIMD = 4096 resident waves: one full round
                                                         // (8192 before; 128 slices: 16 rows per wave 94.5 us per inner iteration against 8 rows ~100)
struct TvOptions { int lds = 1, recompute = 1, march4 = 1, tz = 8, yseg = 0, halo_fold = -1; };   // "tv_lds" ... "tv_halo_fold" (include/tomo_hip.h)
struct TvShape { int n, nx, sxc; };                      // image side, slices, computed width (whole 64-slice chunks)
enum TvFamily { TV_DIRECT, TV_LDS16, TV_LDS8, TV_REG, TV_MARCH4 };
// tz: z-columns per wave (REG, MARCH4) or workgroup (LDS); yseg: rows per wave / workgroup; edge: lanes without a voxel exist (the predicated
// form of k_tv_march4).  DIRECT has no items (0): its grid follows the voxel count.
struct TvPass { TvFamily family; int tz, yseg; bool edge; };
struct TvForm {
    TvPass descent, value;
    bool recompute;        // an inner iteration is "norm pass + recompute-and-update into the partner buffer", not "store g + k_tv_update"
    bool carries_tv;       // the first gradient pass can carry the TV value (else: a value pass of its own)
    bool planes;           // the norm pass can leave the gradient's first / last slice (tomo_tv_grad_planes)
};

// Rows a wave of the register march walks.  32 at a full slab (8 chunks x 64 z-blocks x 16 segments = 8192 waves at 512^3);
// a thin slab of a multi-GPU run has too few waves at that length (64 slices: 1024 waves, 4 per CU), so the segments
// shrink until there are ~8 waves per SIMD lane group again -- the 2 halo rows a segment re-reads cost less than the idle CUs.
inline int tv_rows_per_wave(const TvOptions &o, const TvShape &s, int tz)
{
    if (o.yseg > 0) return o.yseg;
    const int64_t cols = (int64_t)((s.n + tz - 1) / tz) * (s.sxc / 64);
    int yseg = 32;
    while (yseg > TV_YSEG_MIN && cols * ((s.n + yseg - 1) / yseg) < TV_WAVES_WANTED) yseg >>= 1;
    return yseg;
}

inline TvForm select_tv(const TvOptions &o, const TvShape &s)
{
    const bool edge = s.nx % 64 != 0 || s.n % 8 != 0, reg = o.lds == 1, rec = reg && o.recompute;
    const int tz = rec && o.tz == 4 ? 4 : 8;
    const TvPass direct{TV_DIRECT, 0, 0, false};
    TvForm f{};
    f.descent = rec ? TvPass{tz == 8 && o.march4 ? TV_MARCH4 : TV_REG, tz, tv_rows_per_wave(o, s, tz), edge}
              : reg ? TvPass{TV_REG, 8, 32, edge}      // 8 .. 64 rows per wave measured the same; longer segments leave too few waves
              : o.lds == 16 ? TvPass{TV_LDS16, 16, 32, edge} : o.lds ? TvPass{TV_LDS8, 8, 32, edge} : direct;
    f.value = reg ? TvPass{o.march4 && !edge ? TV_MARCH4 : TV_REG, 8, 32, edge} : o.lds == 8 ? TvPass{TV_LDS8, 8, 32, edge} : direct;
    f.recompute = f.planes = rec; f.carries_tv = reg || o.lds == 8;
    return f;
}

// The update pass advances the halo planes itself ("tv_halo_fold"; -1 = where the slab has two chunks or more) instead of a k_halo_apply
// launch behind it: k_tv_march4 only, on the engine's own planes (it writes the partner pair), and not while it also writes the wrap.
inline bool tv_folds_halo(const TvForm &f, const TvOptions &o, const TvShape &s, bool own_planes, bool wrap)
{
    return f.descent.family == TV_MARCH4 && (o.halo_fold < 0 ? s.sxc >= 128 : o.halo_fold != 0) && own_planes && !wrap;
}

// workgroups (4 waves) of the march kernels' item space (z blocks x chunks x y segments), for their XCD-aware item map (k_tv_grad_reg)
inline unsigned tv_march_grid(int n, int tz, int nchunk, int nys)
{
    const int nzb = (n + tz - 1) / tz;
    if ((nzb & 7) == 0) return 8u * (unsigned)(((int64_t)(nzb >> 3) * nchunk * nys + 3) / 4);
    return (unsigned)(((int64_t)nzb * nchunk * nys + 3) / 4);
}

// a fused FGP pass: one workgroup per (z block of tz columns, chunk, y segment); XCD-aligned when the z blocks split evenly over the 8 XCDs
inline unsigned fgp_grid(int n, int nchunk, int tz, int yseg)
{
    const int nzb = (n + tz - 1) / tz, nys = (n + yseg - 1) / yseg;
    return (nzb & 7) == 0 ? 8u * (unsigned)((nzb >> 3) * nchunk * nys) : (unsigned)(nzb * nchunk * nys);
}

}  // namespace tomo
