// Host-only check of the TV / FGP form decision (tomo_tv_amd/csrc/tv_form.h): select_tv, tv_folds_halo, tv_rows_per_wave and the grids of the
// march and fused FGP passes (the LDS passes' two-dimensional grid is written out in their launcher, from the pass's tz and yseg), for
// every combination of the six "tv_*" switches below on seven shapes, against a table of rules.  The rules are NOT computed by the header:
// each is restated from the launcher that decided it before the decision moved into select_tv -- engine_tv.inc and kernels_tv.hip.h as of
// commit de92016 ("Element-wise binary64 tests for engines built from a caller's matrix"); "L<n>" cites the line of that engine_tv.inc.
// Built with ASan + UBSan (tests/native/Makefile: san).  Usage: tv_form_check [quiet]
#include <cstdint>
#include <cstdio>
#include <initializer_list>
#include "tv_form.h"
using namespace tomo;

#define REQUIRE(c, ...) do { if (!(c)) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); return 1; } } while (0)

static int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// kernels_tv.hip.h L403-408 (tv_march_grid): one wave per (z block, chunk, y segment) item, four waves per workgroup; where the z blocks
// split evenly over the 8 XCDs every XCD gets its own whole number of workgroups
static unsigned want_march_grid(int n, int tz, int nchunk, int yseg)
{
    const int64_t nzb = ceil_div(n, tz), nys = ceil_div(n, yseg);
    if (nzb % 8 == 0) return (unsigned)(8 * ceil_div(nzb / 8 * nchunk * nys, 4));
    return (unsigned)ceil_div(nzb * nchunk * nys, 4);
}

// L144-151 (tv_rows_per_wave): the option if positive; else 32, halved while above 8 and the march would have fewer than 4096 waves
static int want_rows(int opt_yseg, int n, int sxc, int tz)
{
    if (opt_yseg > 0) return opt_yseg;
    for (int yseg = 32;; yseg /= 2)
        if (yseg == 8 || ceil_div(n, tz) * (sxc / 64) * ceil_div(n, yseg) >= 4096) return yseg;
}

// L493-495, L521-522, L546-547: one workgroup per (z block, chunk, y segment); 8 x the per-XCD count where the z blocks split evenly
static unsigned want_fgp_grid(int n, int nchunk, int tz, int yseg)
{
    const int nzb = (int)ceil_div(n, tz), nys = (int)ceil_div(n, yseg);
    return nzb % 8 == 0 ? 8u * (unsigned)(nzb / 8 * nchunk * nys) : (unsigned)(nzb * nchunk * nys);
}

static const char *name(TvFamily f) { return f == TV_DIRECT ? "DIRECT" : f == TV_LDS16 ? "LDS16" : f == TV_LDS8 ? "LDS8" : f == TV_REG ? "REG" : "MARCH4"; }

int main(int argc, char **)
{
    const bool quiet = argc > 1;
    const int shapes[7][3] = {{3, 1, 64}, {7, 5, 64}, {40, 70, 128}, {64, 64, 64}, {64, 128, 128}, {33, 130, 192}, {512, 512, 512}};
    const int ldss[5] = {0, 1, 4, 8, 16}, tzs[2] = {4, 8}, ysegs[3] = {0, 4, 32}, folds[3] = {-1, 0, 1};
    long cases = 0;
    for (const auto &sh : shapes) for (int lds : ldss) for (int rec = 0; rec < 2; ++rec) for (int m4 = 0; m4 < 2; ++m4) for (int otz : tzs)
    for (int oy : ysegs) for (int hf : folds) {
        const int n = sh[0], nx = sh[1], sxc = sh[2], nchunk = sxc / 64;
        TvOptions o; o.lds = lds; o.recompute = rec; o.march4 = m4; o.tz = otz; o.yseg = oy; o.halo_fold = hf;
        const TvShape s{n, nx, sxc};
        const TvForm f = select_tv(o, s);
        const bool edge = nx % 64 != 0 || n % 8 != 0;                           // L176, L307
#define CASE "n %d nx %d lds %d recompute %d march4 %d tz %d yseg %d"
#define ARGS n, nx, lds, rec, m4, otz, oy
        // ---- the descent passes (tv_grad_impl L153-209, tv_update_impl L271-335)
        const bool rec_form = lds == 1 && rec;                                   // L171, L287
        REQUIRE(f.recompute == rec_form, CASE ": recompute form", ARGS);
        REQUIRE(f.planes == rec_form, CASE ": gradient planes (L161)", ARGS);
        REQUIRE(f.carries_tv == (lds == 8 || lds == 1), CASE ": folded TV value (L162, L224, L415)", ARGS);
        TvFamily fam; int tz = 8, yseg = 32;
        if (rec_form) {
            tz = otz == 4 ? 4 : 8;                                               // L174, L305
            yseg = want_rows(oy, n, sxc, tz);                                    // L174, L305
            fam = (tz == 8 && m4) ? TV_MARCH4 : TV_REG;                          // L178, L308
        }
        else if (lds == 1) fam = TV_REG;                                         // L185-186: k_tv_grad_reg<8, W>, yseg = 32
        else if (lds == 16) { fam = TV_LDS16; tz = 16; }                         // L193: k_tv_grad_lds<16, false>, yseg = 32 (L192)
        else if (lds) fam = TV_LDS8;                                             // L191, L196-199: k_tv_grad_lds<8, W> for EVERY other non-zero lds
        else fam = TV_DIRECT;                                                    // L202-203: k_tv_grad
        REQUIRE(f.descent.family == fam, CASE ": descent family %s, the rule says %s", ARGS, name(f.descent.family), name(fam));
        if (fam != TV_DIRECT) {
            REQUIRE(f.descent.tz == tz && f.descent.yseg == yseg, CASE ": descent tz %d yseg %d, the rule says %d %d", ARGS, f.descent.tz, f.descent.yseg, tz, yseg);
            if (fam == TV_REG || fam == TV_MARCH4) {                             // L175, L187, L306
                REQUIRE(f.descent.edge == edge, CASE ": descent edge", ARGS);
                const unsigned g = tv_march_grid(n, tz, nchunk, (n + yseg - 1) / yseg);
                REQUIRE(g == want_march_grid(n, tz, nchunk, yseg), CASE ": descent grid %u", ARGS, g);
            }
        }
        // ---- the value pass (tomo_tv_partial L113-139): its own rule -- tv_tz and tv_recompute are not asked, k_tv_march4 only without edge lanes,
        // and every lds other than 1 and 8 (4 and 16 too) takes the direct stencil
        TvFamily vfam;
        if (lds != 8 && lds != 1) vfam = TV_DIRECT;                              // L118: k_tv_value
        else if (lds == 1 && m4 && nx % 64 == 0 && n % 8 == 0) vfam = TV_MARCH4; // L128: k_tv_march4<8, true, TVM_VALUE, false>
        else if (lds == 1) vfam = TV_REG;                                        // L131: k_tv_grad_reg<8, true, false>
        else vfam = TV_LDS8;                                                     // L133-135: k_tv_grad_lds<8, true, false>
        REQUIRE(f.value.family == vfam, CASE ": value family %s, the rule says %s", ARGS, name(f.value.family), name(vfam));
        if (vfam != TV_DIRECT) {
            REQUIRE(f.value.tz == 8 && f.value.yseg == 32, CASE ": value tz %d yseg %d (L127, L130, L132, L134)", ARGS, f.value.tz, f.value.yseg);
            REQUIRE(vfam != TV_MARCH4 || !f.value.edge, CASE ": the value march runs the unpredicated k_tv_march4 only", ARGS);
            if (vfam != TV_LDS8) REQUIRE(tv_march_grid(n, 8, nchunk, (n + 31) / 32) == want_march_grid(n, 8, nchunk, 32), CASE ": value march grid (L130, L132)", ARGS);
        }
        // ---- halo planes advanced inside the update pass (L298, inside the branch of L287; the received planes are the caller's business)
        for (int own = 0; own < 2; ++own) for (int wrap = 0; wrap < 2; ++wrap) {
            const bool want = rec_form && (hf < 0 ? sxc >= 128 : hf != 0) && own && !wrap && otz != 4 && m4;
            REQUIRE(tv_folds_halo(f, o, s, own != 0, wrap != 0) == want, CASE ": halo_fold %d own %d wrap %d: the rule says %d", ARGS, hf, own, wrap, (int)want);
        }
        // ---- rows per wave for any column count a caller names (engine_pdhg.inc asks with its own), and the fused FGP grids
        for (int t : {4, 8}) REQUIRE(tv_rows_per_wave(o, s, t) == want_rows(oy, n, sxc, t), CASE ": rows per wave at %d columns", ARGS, t);
        REQUIRE(fgp_grid(n, nchunk, 8, 32) == want_fgp_grid(n, nchunk, 8, 32), CASE ": k_fgp_fused grid (L493-495)", ARGS);
        REQUIRE(fgp_grid(n, (nx + 31) / 32, 8, 32) == want_fgp_grid(n, (nx + 31) / 32, 8, 32), CASE ": k_fgp_fused2 grid (L521-522, L546-547)", ARGS);
        ++cases;
    }
    REQUIRE(cases == 7L * 5 * 2 * 2 * 2 * 3 * 3, "%ld cases", cases);
    {   // hand-worked.  512^3, 8 columns: 64 z blocks x 8 chunks = 512 columns; 32 rows per wave -> 16 segments -> 8192 waves >= 4096: 32.
        // 64 slices x 512^2: 64 z blocks x 1 chunk = 64 columns; 32 rows -> 16 segments -> 1024 waves < 4096; 16 rows -> 32 segments -> 2048 < 4096;
        // 8 rows: the loop of L149 stops at TV_YSEG_MIN (64 x 64 = 4096 waves): 8.  128 slices: 128 columns; 32 -> 2048 < 4096; 16 -> 4096: 16.
        const TvOptions o;
        REQUIRE(o.lds == 1 && o.recompute == 1 && o.march4 == 1 && o.tz == 8 && o.yseg == 0 && o.halo_fold == -1, "the defaults of the engine");
        REQUIRE(tv_rows_per_wave(o, TvShape{512, 512, 512}, 8) == 32, "512^3: %d rows per wave", tv_rows_per_wave(o, TvShape{512, 512, 512}, 8));
        REQUIRE(tv_rows_per_wave(o, TvShape{512, 64, 64}, 8) == 8, "64 x 512^2: %d rows per wave", tv_rows_per_wave(o, TvShape{512, 64, 64}, 8));
        REQUIRE(tv_rows_per_wave(o, TvShape{512, 128, 128}, 8) == 16, "128 x 512^2: %d rows per wave", tv_rows_per_wave(o, TvShape{512, 128, 128}, 8));
        // grids by hand: 512^3 norm pass: 64 z blocks (8 per XCD) x 8 chunks x 16 segments = 8192 waves = 2048 workgroups; the FGP pair pass:
        // 64 z blocks x 16 chunks of 32 slices x 16 segments = 16384 workgroups; N = 7 (one z block, no XCD split), 5 slices: 1 x 1 x 1 wave -> 1
        REQUIRE(tv_march_grid(512, 8, 8, 16) == 2048 && fgp_grid(512, 16, 8, 32) == 16384 && tv_march_grid(7, 8, 1, 1) == 1 && fgp_grid(7, 1, 8, 32) == 1, "hand-worked grids");
    }
    if (!quiet) std::printf("tv_form: ok (%ld cases)\n", cases);
    return 0;
}
