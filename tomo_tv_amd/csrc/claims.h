// claims.h -- what the engine remembers so that it does not project a volume twice (host-only: no HIP header, no device pointer, so the
// CPU checks it: tests/native/claims_check.cpp).  Three facts, all resting on one write-version per volume slot:
//   the G claim      "the model sinogram G is A * (volume v as it stands)": made by a plain projection into G, inherited by a copy of v;
//   the alias        "RECON_OLD's content is RECON's, its own buffer is stale": made by the Nesterov step;
//   by linearity     "g_yk is A * YK formed by linearity" and "g_prev is A * (the previous iterate)": made by tomo_fista_project_yk.
// Conservative by construction: every write-intent access of a volume bumps its version, every access of G through the slot accessors
// drops the G claim, and only the steps below make a claim.  A stale claim gives a plausible volume, not an error: a new call that writes
// a volume or G goes through get_vol / get_vol_ro / sino_slot / sino_slot_ro (tomo_engine.hip), which call these steps, and through
// nothing else.  The buffers (G, g_prev, g_yk, the volumes) stay in the engine; where a rule needs "does the buffer exist" it is passed in.
#pragma once
#include <cstdint>
#include "../../include/tomo_hip.h"

namespace tomo {

class Claims {
public:
    enum Source { NONE, FROM_G, FROM_G_YK };           // which sinogram holds A * v
    enum Linearity { REFUSED, SAVE_ONLY, FORM };       // what tomo_fista_project_yk may do
    // "fp_reuse" = 0 switches every reuse off (the claims made so far go: none may survive a stretch in which nothing was tracked as a claim)
    bool reuse() const { return fp_reuse; }
    void set_reuse(bool on) { fp_reuse = on; g_clear(); yk_claim.valid = false; }
    // Volume v is about to be written (get_vol).  true: RECON_OLD still shares RECON's buffer and one of the two is v, so the caller first
    // copies RECON's buffer into RECON_OLD's (asked for exactly once: the alias ends here).
    bool write(int v)
    {
        ++vol_version[v];                               // the caller may write it
        // A REPRODUCIBILITY choice, not a staleness fix: g_yk is still exactly A * YK after a write to RECON (neither YK nor g_yk was touched;
        // a write to YK drops the claim through the version above).  But g_yk was formed by linearity and does not have the bits of a
        // projection of YK, and a run in which the caller steps in between tomo_fista_project_yk and the next tomo_sirt on YK is required to
        // give the bits of "fp_reuse" = 0 (tests/test_gpu_sequences.py, section (c)).  The FISTA driver never writes RECON there: no cost.
        if (v == TOMO_VOL_RECON) yk_claim.valid = false;
        const bool shared = old_is_recon && (v == TOMO_VOL_RECON || v == TOMO_VOL_RECON_OLD);
        if (shared) old_is_recon = false;
        return shared;
    }
    // the slot whose buffer a read of v resolves to (get_vol_ro): RECON while RECON_OLD is its alias -- a read-only view of the same content
    int read_slot(int v) const { return v == TOMO_VOL_RECON_OLD && old_is_recon ? (int)TOMO_VOL_RECON : v; }
    // someone asked for G through get_sino / sino_slot: whoever asks for G may overwrite it
    void g_touched() { g_clear(); }
    // G was projected plainly from v as it stands (tomo_forward_projection into G; FP_DD of tomo_data_distance_sq also stores g = A x)
    void g_projected_from(int v) { g_valid[0].vol = v; g_valid[0].ver = vol_version[v]; g_valid[1].vol = -1; }
    // is G = A * (v as it stands)?  have_g: the buffer of G exists (a released geometry took it along)
    bool g_is_projection_of(int v, bool have_g) const
    {
        if (!fp_reuse || v < 0 || v >= TOMO_VOL_SLOTS || !have_g) return false;
        return (g_valid[0].vol == v && g_valid[0].ver == vol_version[v]) || (g_valid[1].vol == v && g_valid[1].ver == vol_version[v]);
    }
    // the sinogram that holds A * (v as it stands): G through its claim, or the extrapolated point's own buffer
    Source projection_in_hand(int v, bool have_g, bool have_g_yk) const
    {
        if (g_is_projection_of(v, have_g)) return FROM_G;
        return fp_reuse && v == TOMO_VOL_YK && have_g_yk && yk_claim.valid && yk_claim.ver == vol_version[TOMO_VOL_YK] ? FROM_G_YK : NONE;
    }
    // dst <- src was copied (tomo_copy_volume).  g_was_src: g_is_projection_of(src), asked BEFORE the accessors ran (the write of dst
    // touches nothing of G, so what held for src then holds for both now): G = A * src = A * dst
    void copied(int dst, int src, bool g_was_src) { if (g_was_src && dst != src) { g_valid[1].vol = dst; g_valid[1].ver = vol_version[dst]; } }
    // tomo_restart_recon: RECON, YK and RECON_OLD are physically zero, so nothing is shared any more
    void restarted() { old_is_recon = false; bump3(); }
    // The prox result landed in volume v behind the accessors (the FGP calls store into, or swap, the target's buffer after their begin
    // call took it through write()): its content changed once more.  Out-of-range v (no target): nothing.
    void prox_landed(int v) { if (v >= 0 && v < TOMO_VOL_SLOTS) ++vol_version[v]; }
    // The Nesterov step has run (tomo_fista_momentum): RECON <- r = YK's content, YK <- r + beta (r - old), RECON_OLD <- r as a flag,
    // not a store.  Whoever may WRITE RECON, or touches RECON_OLD, goes through write(), which ends the alias; readers use read_slot().
    void nesterov_step(float beta)
    {
        // is the saved projection (linearity_end) A * (what RECON_OLD held going into this step)?  RECON_OLD was set to RECON by the last
        // step and neither has been touched since, and the projection was saved from that very RECON
        mom_p_ok = g_prev_valid && mom.set && vol_version[TOMO_VOL_RECON] == mom.ver_recon && vol_version[TOMO_VOL_RECON_OLD] == mom.ver_old
                   && g_prev_recon_ver == vol_version[TOMO_VOL_RECON];
        bump3();
        old_is_recon = true;                            // recon_old == r, not stored
        mom.beta = beta; mom.set = true;
        mom.ver_recon = vol_version[TOMO_VOL_RECON]; mom.ver_yk = vol_version[TOMO_VOL_YK]; mom.ver_old = vol_version[TOMO_VOL_RECON_OLD];
    }
    float beta() const { return mom.beta; }
    // tomo_fista_project_yk, first half.  Anything but REFUSED needs every piece provably in place: G = A * RECON as it stands, RECON and YK
    // untouched since the last Nesterov step.  FORM: the saved g_prev is A * r_old, so g_yk = (1 + beta) G - beta g_prev is A * YK;
    // SAVE_ONLY: it is not (first step), G is only saved.  Either way g_prev and g_yk are about to be overwritten: what they claimed goes.
    Linearity linearity_begin(bool have_g)
    {
        if (!fp_reuse || !g_is_projection_of(TOMO_VOL_RECON, have_g) || !mom.set) return REFUSED;
        if (vol_version[TOMO_VOL_RECON] != mom.ver_recon || vol_version[TOMO_VOL_YK] != mom.ver_yk) return REFUSED;
        const bool have_prev = mom_p_ok;
        yk_claim.valid = g_prev_valid = mom_p_ok = false;   // (mom_p_ok: g_prev stops being A * r_old, so a second call cannot form from it)
        return have_prev ? FORM : SAVE_ONLY;
    }
    // ... second half, after the pass ran: g_prev = A * RECON, saved for the next step.  G is untouched: it stays A * RECON, with its claim.
    // true: a projection of YK is in hand -- g_yk as formed, or G itself after a first step with beta == 0 (YK is r, bit for bit: the
    // claim a copy inherits)
    bool linearity_end(Linearity how)
    {
        g_prev_valid = true; g_prev_recon_ver = vol_version[TOMO_VOL_RECON];
        if (how == FORM) { yk_claim.valid = true; yk_claim.ver = vol_version[TOMO_VOL_YK]; return true; }
        if (mom.beta != 0.f) return false;
        g_valid[1].vol = TOMO_VOL_YK; g_valid[1].ver = vol_version[TOMO_VOL_YK];
        return true;
    }
    // the tilt geometry went, and G, g_prev and g_yk with it (free_geometry): the G claim dies with have_g, the rest here
    void geometry_released() { yk_claim.valid = false; g_prev_valid = mom_p_ok = mom.set = false; }
    // this record's engine took over every volume of src's (tomo_adopt_volumes): the alias comes along, every volume here is another one
    // now, and G is a projection of none of them.  src is left without volumes; its engine is destroyed next.
    void adopt(Claims &src)
    {
        old_is_recon = src.old_is_recon; src.old_is_recon = false;
        for (int i = 0; i < TOMO_VOL_SLOTS; ++i) ++vol_version[i];
        g_clear();
    }

private:
    void g_clear() { g_valid[0].vol = g_valid[1].vol = -1; }
    void bump3() { ++vol_version[TOMO_VOL_RECON]; ++vol_version[TOMO_VOL_YK]; ++vol_version[TOMO_VOL_RECON_OLD]; }
    uint64_t vol_version[TOMO_VOL_SLOTS] = {};
    struct { int vol = -1; uint64_t ver = 0; } g_valid[2];   // G is A * (volume vol at write-version ver); [1]: a second volume with the same content
    bool fp_reuse = true;
    struct { bool valid = false; uint64_t ver = 0; } yk_claim;   // g_yk is A * (volume YK at this write-version)
    bool g_prev_valid = false, mom_p_ok = false;        // g_prev is A * (RECON at g_prev_recon_ver); ... and that is r_old of the last step
    uint64_t g_prev_recon_ver = 0;
    struct { float beta = 0.f; uint64_t ver_recon = 0, ver_yk = 0, ver_old = 0; bool set = false; } mom;   // the last Nesterov step
    bool old_is_recon = false;                          // RECON_OLD's content is RECON's (nesterov_step; see write)
};

}  // namespace tomo
