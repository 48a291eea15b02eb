// Host-only check of the engine's projection claims (tomo_tv_amd/csrc/claims.h) against a small model of what the buffers hold.
// The model: every volume buffer holds a content token (a write mints a new one, a copy copies it), G holds "plain projection of
// token t" or something else, g_yk holds "formed by linearity for YK-token t, RECON not written since" or nothing, g_prev holds
// "plain projection of token t" or nothing.  Beside the buffers (P, what the kernels would read) the model keeps what a caller
// expects each slot to hold (L): the alias is sound while a read of every slot, resolved by the record, finds the expected token.
//   (a) seeded random walks over all steps and all slots, "fp_reuse" toggled along the way: after every step each claim the record
//       makes must hold in the model (soundness; the record may always claim less);
//   (b) the drivers' call sequences with the decisions written out as they were read off the engine's code: which steps reuse, which
//       single writer drops a claim, when the alias asks for its copy.
// The wrappers below are the engine's accessors and calls reduced to their claim steps, in the engine's order.  Two things are taken
// from the engine's protocol rather than checked: the prox's begin call takes its target through write() before the result lands (with
// RECON or RECON_OLD as the target, no Nesterov step and no tomo_fista_project_yk in between), and an engine whose volumes were adopted
// is destroyed (the walk replaces it by a new one).
// Usage: claims_check [quiet]     exit 1 with the seed and the index of the failing step
#include <cstdint>
#include <cstdio>
#include <initializer_list>
#include "claims.h"
using namespace tomo;

enum { RECON = TOMO_VOL_RECON, TEMP = TOMO_VOL_TEMP, YK = TOMO_VOL_YK, OLD = TOMO_VOL_RECON_OLD, NV = TOMO_VOL_SLOTS };

static uint64_t g_tokens = 0;
static uint64_t mint() { return ++g_tokens; }
static uint64_t g_seed = 0;
static long g_step = -1;                               // -1: a scripted sequence

struct Sys {
    Claims c;
    uint64_t P[NV], L[NV];
    bool reuse = true, have_g = false, have_g_yk = false;
    struct { bool plain = false; uint64_t tok = 0; } G;
    struct { bool valid = false; uint64_t tok = 0; bool recon_written = false; } gyk;
    struct { bool valid = false; uint64_t tok = 0; } gprev;
    struct { bool set = false; uint64_t r = 0, old = 0, yk = 0; float beta = 0.f; } mom;
    int made_real = 0;                                 // times write() asked for RECON_OLD's copy
    Sys() { for (int v = 0; v < NV; ++v) P[v] = L[v] = mint(); }
};

#define REQUIRE(c, ...) do { if (!(c)) { std::printf("FAIL %s:%d seed %llu step %ld: ", __FILE__, __LINE__, (unsigned long long)g_seed, g_step); std::printf(__VA_ARGS__); std::printf("\n"); return false; } } while (0)

// ---- the engine's accessors and calls, reduced to their claim steps -----------------------------------------------------------------
static uint64_t rd(Sys &s, int v) { return s.P[s.c.read_slot(v)]; }                      // get_vol_ro
static void wr(Sys &s, int v)                                                            // get_vol
{
    if (s.c.write(v)) { ++s.made_real; s.P[OLD] = s.P[RECON]; }
    if (v == RECON) s.gyk.recon_written = true;
}
static void set_volume(Sys &s, int v) { wr(s, v); s.P[v] = s.L[v] = mint(); }            // any call that rewrites v through get_vol
static void touch_g(Sys &s) { s.c.g_touched(); s.have_g = true; s.G.plain = false; }     // get_sino on G
static void project(Sys &s, int v)                                                       // tomo_forward_projection into G, tomo_data_distance_sq
{
    const uint64_t t = rd(s, v);
    touch_g(s);
    s.G.plain = true; s.G.tok = t;
    s.c.g_projected_from(v);
}
static bool g_is(Sys &s, int v) { return s.c.g_is_projection_of(v, s.have_g); }
static Claims::Source in_hand(Sys &s, int v) { return s.c.projection_in_hand(v, s.have_g, s.have_g_yk); }
static Claims::Source sirt(Sys &s, int v) { const Claims::Source h = in_hand(s, v); set_volume(s, v); return h; }   // tomo_sirt_data
static bool cgls(Sys &s, int v) { const bool h = g_is(s, v); set_volume(s, v); return h; }                           // tomo_cgls
static void copy(Sys &s, int dst, int src)                                               // tomo_copy_volume
{
    const bool g_src = g_is(s, src);
    wr(s, dst);
    const uint64_t t = rd(s, src);
    if (dst != src) { s.P[dst] = t; s.L[dst] = s.L[src]; }
    s.c.copied(dst, src, g_src);
}
static void restart(Sys &s)                                                              // tomo_restart_recon
{
    s.P[RECON] = s.P[YK] = s.P[OLD] = s.L[RECON] = s.L[YK] = s.L[OLD] = mint();
    s.gyk.recon_written = true;
    s.c.restarted();
}
static void prox_landed(Sys &s, int v) { s.P[v] = s.L[v] = mint(); if (v == RECON) s.gyk.recon_written = true; s.c.prox_landed(v); }
static void prox(Sys &s, int v) { wr(s, v); prox_landed(s, v); }                         // tomo_fgp_begin_vol ... tomo_fgp_end
static void momentum(Sys &s, float beta)                                                 // tomo_fista_momentum
{
    const uint64_t r = rd(s, YK), old = rd(s, OLD), yk = beta == 0.f ? r : mint();       // (beta == 0: yk is r, bit for bit)
    s.P[RECON] = s.L[RECON] = r;
    s.P[YK] = s.L[YK] = yk;
    s.L[OLD] = r;                                                                        // (its buffer keeps what it had)
    s.mom.set = true; s.mom.r = r; s.mom.old = old; s.mom.yk = yk; s.mom.beta = beta;
    s.gyk.recon_written = true;
    s.c.nesterov_step(beta);
}
// tomo_fista_project_yk: *how = what the record allowed; false: the model does not bear it out
static bool project_yk(Sys &s, Claims::Linearity *how, bool *done)
{
    *done = false;
    *how = s.c.linearity_begin(s.have_g);
    if (*how == Claims::REFUSED) return true;
    REQUIRE(s.reuse, "fp_reuse is off and the projection by linearity was not refused");
    REQUIRE(s.G.plain && s.G.tok == s.L[RECON], "linearity: G is not the plain projection of RECON as it stands");
    REQUIRE(s.mom.set && s.L[RECON] == s.mom.r && s.L[YK] == s.mom.yk, "linearity: RECON or YK is not what the last Nesterov step left");
    s.have_g_yk = true;
    if (*how == Claims::FORM) {
        REQUIRE(s.gprev.valid && s.gprev.tok == s.mom.old, "linearity: the saved projection is not A * (what RECON_OLD held going into the step)");
        s.gyk.valid = true; s.gyk.tok = s.L[YK]; s.gyk.recon_written = false;
    }
    s.gprev.valid = true; s.gprev.tok = s.G.tok;
    *done = s.c.linearity_end(*how);
    REQUIRE(!*done || in_hand(s, YK) != Claims::NONE, "linearity: done, and no projection of YK in hand");
    return true;
}
static void release_geometry(Sys &s)                                                     // free_geometry
{
    s.have_g = s.have_g_yk = s.G.plain = s.gyk.valid = s.gprev.valid = false;
    s.c.geometry_released();
}
static void adopt(Sys &dst, Sys &src)                                                    // tomo_adopt_volumes (every slot of src allocated)
{
    for (int v = 0; v < NV; ++v) { dst.P[v] = src.P[v]; dst.L[v] = src.L[v]; src.P[v] = src.L[v] = mint(); }
    dst.gyk.recon_written = true;
    dst.c.adopt(src.c);
}
static void set_reuse(Sys &s, bool on) { s.reuse = on; s.c.set_reuse(on); }

// ---- every claim the record makes holds in the model -------------------------------------------------------------------------------
static bool sound(Sys &s)
{
    REQUIRE(s.c.reuse() == s.reuse, "the fp_reuse getter");
    for (int v = 0; v < NV; ++v) {
        REQUIRE(rd(s, v) == s.L[v], "a read of slot %d finds token %llu, expected %llu", v, (unsigned long long)rd(s, v), (unsigned long long)s.L[v]);
        const Claims::Source h = in_hand(s, v);
        REQUIRE((h == Claims::FROM_G) == g_is(s, v), "slot %d: the two queries disagree about G", v);
        if (h == Claims::NONE) continue;
        REQUIRE(s.reuse, "slot %d: fp_reuse is off and a projection is offered", v);
        if (h == Claims::FROM_G) REQUIRE(s.have_g && s.G.plain && s.G.tok == s.L[v], "slot %d: G is not the plain projection of it as it stands", v);
        else REQUIRE(v == YK && s.have_g_yk && s.gyk.valid && s.gyk.tok == s.L[YK] && !s.gyk.recon_written, "g_yk is offered and is not A * YK, or RECON was written since");
    }
    REQUIRE(!g_is(s, -1) && !g_is(s, NV) && in_hand(s, -1) == Claims::NONE && in_hand(s, NV) == Claims::NONE, "a slot out of range");
    return true;
}

// ---- (a) random walks ---------------------------------------------------------------------------------------------------------
static uint64_t g_rng;
static uint32_t rnd(uint32_t n) { g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(g_rng >> 33) % n; }
static int any_slot() { return rnd(3) ? (int)rnd(6) : (int)rnd(NV); }                    // the fixed slots and USER0 mostly, every slot sometimes

struct Tally { long g_reused = 0, yk_reused = 0, formed = 0, saved = 0, made_real = 0, off = 0; };

static bool walk(uint64_t seed, long nsteps, Tally &tally)
{
    g_seed = seed; g_rng = seed * 0x9E3779B97F4A7C15ull + 1;
    Sys *sys[2] = {new Sys(), new Sys()};
    // fista: a stretch in which the first engine mostly goes round the FISTA driver's loop (phase: the next of its five calls), with
    // any other step thrown in now and then, so that the deep states are reached and disturbed
    bool ok = true, fista = false;
    uint32_t phase = 0;
    for (g_step = 0; ok && g_step < nsteps; ++g_step) {
        if (rnd(64) == 0) fista = !fista;
        const bool loop = fista && rnd(8);
        Sys &s = *sys[!loop && rnd(4) == 0];
        const int v = loop ? (int)YK : any_slot();
        const float beta = rnd(4) ? 0.25f + 0.125f * (float)rnd(4) : 0.f;
        const uint32_t op = loop ? 100 + phase++ % 5 : rnd(16);
        Claims::Linearity how; bool done;
        tally.off += !s.reuse;
        switch (op) {
        case 0: case 1: set_volume(s, v); break;
        case 2: touch_g(s); break;
        case 3: case 4: case 103: project(s, op == 103 ? RECON : v); break;
        case 5: case 100: { const Claims::Source h = sirt(s, op == 100 ? YK : v); tally.g_reused += h == Claims::FROM_G; tally.yk_reused += h == Claims::FROM_G_YK; break; }
        case 6: tally.g_reused += cgls(s, v); break;
        case 7: case 8: copy(s, v, any_slot()); break;
        case 9: if (rnd(4) == 0) restart(s); else (void)rd(s, v); break;
        // the prox's result landing: right behind its begin call, or with other calls in between -- drawn only for a target whose write()
        // does no more than bump a version (for RECON and RECON_OLD the begin call has to be the nearest write: see the head of this file)
        case 10: case 101: if (rnd(2) && v != RECON && v != OLD) prox_landed(s, v); else prox(s, v); break;
        case 11: case 102: momentum(s, beta); break;
        case 12: case 104:
            ok = project_yk(s, &how, &done);
            tally.formed += how == Claims::FORM; tally.saved += how == Claims::SAVE_ONLY;
            break;
        case 13: if (rnd(8) == 0) release_geometry(s); else project(s, RECON); break;
        case 14: if (rnd(8) == 0) { Sys &d = *sys[0], *src = sys[1]; adopt(d, *src); delete src; sys[1] = new Sys(); } else momentum(s, beta); break;
        case 15: if (!s.reuse || rnd(4) == 0) set_reuse(s, !s.reuse); else set_volume(s, RECON); break;
        }
        ok = ok && sound(*sys[0]) && sound(*sys[1]);
    }
    tally.made_real += sys[0]->made_real + sys[1]->made_real;
    delete sys[0]; delete sys[1];
    return ok;
}

// ---- (b) the drivers' sequences, decisions written out ---------------------------------------------------------------------------------
#define EXPECT(c) REQUIRE(c, "%s", #c)
#define PYK(s, want_how, want_done) do { Claims::Linearity how_; bool done_; if (!project_yk(s, &how_, &done_)) return false; \
                                         REQUIRE(how_ == (want_how) && done_ == (want_done), "project_yk: %d, done %d", (int)how_, (int)done_); } while (0)
// the state of TomoGPU.fista after its second iteration: G = A * RECON, g_yk = A * YK formed by linearity, RECON_OLD an alias
static bool fista_two(Sys &s)
{
    copy(s, YK, RECON); copy(s, OLD, RECON);                                             // initialize_fista
    EXPECT(sirt(s, YK) == Claims::NONE); prox(s, YK); momentum(s, 0.f); project(s, RECON);
    PYK(s, Claims::SAVE_ONLY, true);                    // the first one only saves; beta == 0: YK is RECON bit for bit, G is granted to YK
    EXPECT(in_hand(s, YK) == Claims::FROM_G && g_is(s, RECON));
    EXPECT(sirt(s, YK) == Claims::FROM_G); prox(s, YK); momentum(s, 0.28f); project(s, RECON);
    PYK(s, Claims::FORM, true);                         // from the second iteration on: formed by linearity
    EXPECT(in_hand(s, YK) == Claims::FROM_G_YK && g_is(s, RECON) && s.c.read_slot(OLD) == RECON);
    return sound(s);
}

static bool scripted()
{
    g_seed = 0; g_step = -1;
    {   // TomoGPU._run_iterative, SIRT: a step and its data distance; every step from the second on starts from G
        Sys s;
        for (int it = 0; it < 4; ++it) { EXPECT((sirt(s, RECON) == Claims::FROM_G) == (it > 0)); project(s, RECON); EXPECT(sound(s)); }
    }
    {   // ... CGLS: the restart of every call from the second on
        Sys s;
        for (int it = 0; it < 3; ++it) { EXPECT(cgls(s, RECON) == (it > 0)); project(s, RECON); EXPECT(sound(s)); }
    }
    {   // multimodal::data_fusion: project the model volume, copy it, SIRT on the copy inherits the claim (and the model keeps its own)
        Sys s;
        const int MODEL = TOMO_VOL_USER0, UPD = TOMO_VOL_USER0 + 1;
        set_volume(s, MODEL); project(s, MODEL); copy(s, UPD, MODEL);
        EXPECT(g_is(s, UPD) && g_is(s, MODEL) && sound(s));
        EXPECT(sirt(s, UPD) == Claims::FROM_G && !g_is(s, UPD) && g_is(s, MODEL));
        copy(s, MODEL, MODEL); EXPECT(!g_is(s, MODEL));                                  // a copy onto itself is a write-intent access: no claim left
    }
    {   // TomoGPU.fista with momentum, three iterations
        Sys s;
        if (!fista_two(s)) return false;
        EXPECT(sirt(s, YK) == Claims::FROM_G_YK && in_hand(s, YK) == Claims::NONE); prox(s, YK); momentum(s, 0.43f); project(s, RECON);
        PYK(s, Claims::FORM, true);
        PYK(s, Claims::SAVE_ONLY, false);               // asked twice: g_prev is A * RECON now, not A * r_old -- nothing to form from, and g_yk's claim goes
        EXPECT(in_hand(s, YK) == Claims::NONE && sound(s));
    }
    // between the G claim and its use, each single writer drops it
    for (int w = 0; w < 10; ++w) {
        Sys s, other;
        set_volume(s, TEMP); project(s, TEMP); EXPECT(g_is(s, TEMP));
        switch (w) {
        case 0: set_volume(s, TEMP); break;
        case 1: touch_g(s); break;
        case 2: prox_landed(s, TEMP); break;
        case 3: release_geometry(s); break;
        case 4: adopt(s, other); break;
        case 5: set_reuse(s, false); EXPECT(!g_is(s, TEMP)); set_reuse(s, true); break;
        case 6: (void)rd(s, TEMP); set_volume(s, RECON); copy(s, YK, TEMP); momentum(s, 0.3f); prox_landed(s, TOMO_VOL_USER0); restart(s); EXPECT(g_is(s, TEMP) && g_is(s, YK) == false); continue;   // none of these writes TEMP or touches G
        case 7: project(s, RECON); EXPECT(g_is(s, RECON) && !g_is(s, TEMP)); restart(s); EXPECT(!g_is(s, RECON)); continue;
        case 8: project(s, RECON); momentum(s, 0.3f); EXPECT(!g_is(s, RECON) && !g_is(s, YK) && !g_is(s, OLD)); continue;
        case 9: project(s, OLD); restart(s); EXPECT(!g_is(s, OLD)); continue;
        }
        EXPECT(!g_is(s, TEMP) && in_hand(s, TEMP) == Claims::NONE && sound(s));
    }
    // between tomo_fista_project_yk and the step on YK: a writer of YK or RECON (and the rest of the list) drops g_yk, an unrelated slot does not
    for (int w = 0; w < 12; ++w) {
        Sys s, other;
        if (!fista_two(s)) return false;
        bool kept = false;
        switch (w) {
        case 0: set_volume(s, YK); break;
        case 1: set_volume(s, RECON); break;            // (reproducibility, not staleness: see Claims::write)
        case 2: prox(s, YK); break;
        case 3: prox_landed(s, YK); break;
        case 4: restart(s); break;
        case 5: momentum(s, 0.4f); break;
        case 6: release_geometry(s); break;
        case 7: adopt(s, other); break;
        case 8: set_reuse(s, false); EXPECT(in_hand(s, YK) == Claims::NONE); set_reuse(s, true); break;
        case 9: set_volume(s, TEMP); copy(s, TOMO_VOL_USER0, YK); kept = true; break;
        case 10: touch_g(s); kept = true; break;        // g_yk is a buffer of its own: G's claim goes, this one stays
        case 11: set_volume(s, OLD); kept = true; break;   // ends the alias; YK and g_yk are what they were
        }
        EXPECT((in_hand(s, YK) == Claims::FROM_G_YK) == kept && sound(s));
    }
    {   // the saved projection: a write to RECON or RECON_OLD between two Nesterov steps leaves nothing to form from
        for (int w = 0; w < 3; ++w) {
            Sys s;
            if (!fista_two(s)) return false;
            (void)sirt(s, YK); prox(s, YK);
            if (w == 1) set_volume(s, RECON);
            if (w == 2) set_volume(s, OLD);
            momentum(s, 0.43f); project(s, RECON);
            PYK(s, w == 0 ? Claims::FORM : Claims::SAVE_ONLY, w == 0);
            EXPECT(sound(s));
        }
    }
    {   // the alias: reads of RECON_OLD resolve to RECON after the step; the first write to either slot asks once for the copy
        for (int first : {RECON, OLD}) {
            Sys s;
            set_volume(s, RECON); copy(s, YK, RECON); copy(s, OLD, RECON);
            EXPECT(s.c.read_slot(OLD) == OLD && s.made_real == 0);
            set_volume(s, YK); momentum(s, 0.3f);
            EXPECT(s.c.read_slot(OLD) == RECON && s.c.read_slot(RECON) == RECON && s.c.read_slot(YK) == YK && s.made_real == 0);
            set_volume(s, TEMP); set_volume(s, YK); (void)rd(s, OLD); project(s, OLD);
            EXPECT(s.c.read_slot(OLD) == RECON && s.made_real == 0 && sound(s));          // other slots and reads leave it alone
            set_volume(s, first);
            EXPECT(s.c.read_slot(OLD) == OLD && s.made_real == 1 && sound(s));
            EXPECT(g_is(s, OLD) == (first == RECON));   // RECON_OLD's content outlives a write to RECON, and so does G's claim on it
            set_volume(s, RECON); set_volume(s, OLD);
            EXPECT(s.made_real == 1);
            momentum(s, 0.3f); momentum(s, 0.3f);
            EXPECT(s.c.read_slot(OLD) == RECON && s.made_real == 1 && sound(s));          // a step on an aliased pair needs no copy either
            restart(s); set_volume(s, first);
            EXPECT(s.c.read_slot(OLD) == OLD && s.made_real == 1 && sound(s));            // a restart ends the alias: every buffer is zero, nothing to copy
        }
        Sys src, dst;                                   // adoption carries the flag to the adopting record and clears it in the source
        set_volume(src, YK); momentum(src, 0.3f);
        adopt(dst, src);
        EXPECT(dst.c.read_slot(OLD) == RECON && src.c.read_slot(OLD) == OLD && sound(dst) && sound(src));
        set_volume(dst, OLD);
        EXPECT(dst.made_real == 1 && src.made_real == 0 && sound(dst));
        adopt(src, dst);
        EXPECT(src.c.read_slot(OLD) == OLD && dst.c.read_slot(OLD) == OLD);
    }
    return true;
}

int main(int argc, char **)
{
    const bool quiet = argc > 1;
    if (!scripted()) return 1;
    Tally t;
    for (uint64_t seed = 1; seed <= 5; ++seed) if (!walk(seed, 40000, t)) return 1;
    g_step = -1;
    // the walks went where the claims are: a walk that never reuses, forms or aliases checks nothing
    if (t.g_reused < 1000 || t.yk_reused < 100 || t.formed < 200 || t.saved < 200 || t.made_real < 200 || t.off < 1000) {
        std::printf("FAIL: the walks were too shallow: %ld reuses of G, %ld of g_yk, %ld formed, %ld saved, %ld copies made real, %ld steps with fp_reuse off\n",
                    t.g_reused, t.yk_reused, t.formed, t.saved, t.made_real, t.off);
        return 1;
    }
    if (!quiet) std::printf("claims: ok (%ld reuses of G, %ld of g_yk, %ld formed, %ld saved, %ld copies made real, %ld steps with fp_reuse off)\n",
                            t.g_reused, t.yk_reused, t.formed, t.saved, t.made_real, t.off);
    return 0;
}
