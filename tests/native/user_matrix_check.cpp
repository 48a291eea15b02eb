// Host-only check of every table builder on a CALLER'S matrix (tomo_create_from_matrix: ctvlib.load_A / update_proj_angles).
// Reads raw float32 triplets (tests/user_matrices.py: write_triplets), runs what finish_create_impl runs -- coo_from_triplets, sort_rows,
// build_tables, build_walk, build_segments, build_tiles, build_fp_strips, build_fp_lists, build_sart_tiles, build_sart_resident,
// build_bp_tiles, build_bp_lists, with the kernels' constants -- and replays each table the way its kernel reads it, in double
// precision on one slice:
//   * sort_rows against an independent last-assignment-wins, sorted-by-column copy of the triplets (explicit zeros kept);
//   * the cell table against that copy (non-zero weights only, ascending ray);
//   * every table offset in range; the tile, strip and list streams hold exactly the non-zero entries of the matrix and reproduce A x;
//     the back-projection cells, lists and resident cells reproduce the cell table;
//   * the walk lists visit every pixel of an angle exactly once as owner and carry every entry of the matrix; the segment items cut
//     every walk list exactly once.
// A builder may refuse a matrix (the kernels then fall back): what each one answered is printed as one line of name=0/1 pairs, which
// tests/test_gpu_user_matrix.py pins.  Usage: user_matrix_check FILE [quiet]
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include "resident.h"
#include "sysmat.h"
using namespace tomo;

#define REQUIRE(c, ...) do { if (!(c)) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); return 1; } } while (0)
static inline float bitsf(uint32_t b) { float f; std::memcpy(&f, &b, 4); return f; }

// the kernels' geometry (kernels_fp.hip.h, kernels_bp.hip.h, kernels_sart.hip.h; engine_create.inc passes the same numbers)
static const int FT_TY = 32, FT_TZ = 16, PIXB = 256, FB_A = 4, FB_MAXR = 40, FB_MAX_PROJ = 4096, ST_TY = 16, ST_TZ = 16, ST_MAXR = 26, SEG_LEN = 32, CUS = 256;

struct Problem {
    int N = 0, P = 0, nchunk = 1;
    int64_t nrows = 0, npix = 0, nz = 0;   // nz: non-zero weights of the canonical matrix
    Coo m;
    std::vector<double> x, g, rr;          // a volume slice, A x, a sinogram slice
};

static int check_tile_fp(const Problem &pb, const Tables &t)
{
    const int N = pb.N, TY = FT_TY, TZ = FT_TZ, NS = Tables::TILE_SLOTS, NB = Tables::TILE_BATCH;
    const int tiles_z = t.tiles_z, ntiles = t.tiles_y * t.tiles_z;
    REQUIRE(t.tile_slot_ptr.size() == (size_t)ntiles * NS + 1 && t.tile_slot_seg0.size() == (size_t)ntiles * NS, "tile table sizes");
    REQUIRE(t.rseg_ptr.size() == (size_t)pb.nrows + 1, "row list size");
    std::vector<double> part(t.tile_nseg, 0.0);
    std::vector<int> seen(t.tile_nseg, 0);
    int64_t real = 0;
    for (int k = 0; k < ntiles; ++k) {
        const int y0 = (k / tiles_z) * TY, z0 = (k % tiles_z) * TZ;
        for (int q = 0; q < NS; ++q) {
            const size_t slot = (size_t)k * NS + q;
            uint32_t seg = t.tile_slot_seg0[slot];
            double acc = 0.0;
            REQUIRE(t.tile_slot_ptr[slot] <= t.tile_slot_ptr[slot + 1] && (size_t)t.tile_slot_ptr[slot + 1] * NB <= t.tile_off.size(), "stream bounds");
            for (uint32_t b = t.tile_slot_ptr[slot]; b < t.tile_slot_ptr[slot + 1]; ++b) {
                bool last = false;
                for (int j = 0; j < NB; ++j) {
                    const uint32_t off = t.tile_off[(size_t)b * NB + j]; const float w = t.tile_w[(size_t)b * NB + j];
                    if (j == 0) last = off >> 31; else REQUIRE((off >> 31) == (uint32_t)last, "flag differs inside batch %u", b);
                    const uint32_t lp = (off & 0x7FFFFFFFu) / PIXB;
                    REQUIRE((off & 0x7FFFFFFFu) % PIXB == 0 && lp <= (uint32_t)(TY * TZ), "bad offset");
                    if (lp == (uint32_t)(TY * TZ)) { REQUIRE(w == 0.f, "padding entry with weight"); continue; }
                    const int y = y0 + lp / TZ, z = z0 + lp % TZ;
                    REQUIRE(y < N && z < N, "entry outside the image");
                    acc += (double)w * pb.x[(int64_t)y * N + z];
                    if (w != 0.f) ++real;
                }
                if (last) { REQUIRE(seg < t.tile_nseg, "segment id out of range"); part[seg] = acc; seen[seg]++; acc = 0.0; ++seg; }
            }
            const uint32_t next = slot + 1 < (size_t)ntiles * NS ? t.tile_slot_seg0[slot + 1] : t.tile_nseg;
            REQUIRE(seg == next, "stream %zu ends at segment %u, next stream starts at %u", slot, seg, next);
        }
    }
    REQUIRE(real == pb.nz, "tile streams hold %ld non-zero entries, matrix has %ld", (long)real, (long)pb.nz);
    for (uint32_t s = 0; s < t.tile_nseg; ++s) REQUIRE(seen[s] == 1, "segment %u written %d times", s, seen[s]);
    std::vector<int> used(t.tile_nseg, 0);
    for (int64_t r = 0; r < pb.nrows; ++r) {
        double s = 0;
        REQUIRE(t.rseg_ptr[r] <= t.rseg_ptr[r + 1] && t.rseg_ptr[r + 1] <= t.tile_nseg, "row list bounds");
        for (uint32_t k = t.rseg_ptr[r]; k < t.rseg_ptr[r + 1]; ++k) { REQUIRE(t.rseg_idx[k] < t.tile_nseg, "row list id"); s += part[t.rseg_idx[k]]; used[t.rseg_idx[k]]++; }
        REQUIRE(std::fabs(s - pb.g[r]) <= 1e-9 * (1.0 + std::fabs(pb.g[r])), "tile FP of row %ld: %.12g vs %.12g", (long)r, s, pb.g[r]);
    }
    for (uint32_t s = 0; s < t.tile_nseg; ++s) REQUIRE(used[s] == 1, "segment %u used by %d rows", s, used[s]);
    return 0;
}

static double bp_ref(const Problem &pb, const Tables &t, int i, int y, int z)
{
    double ref = 0;
    if (y < pb.N && z < pb.N) {
        const Cell &cc = t.cell[(size_t)i * pb.npix + (int64_t)y * pb.N + z];
        if (cc.w0 != 0.f) ref += (double)cc.w0 * pb.rr[(int64_t)i * pb.N + cc.r0];
        if (cc.w1 != 0.f) ref += (double)cc.w1 * pb.rr[(int64_t)i * pb.N + cc.r1];
    }
    return ref;
}

static int check_tile_bp(const Problem &pb, const Tables &t)
{
    const int N = pb.N, P = pb.P, TY = FT_TY, TZ = FT_TZ, A = FB_A, MAXR = FB_MAXR;
    const int tiles_z = (N + TZ - 1) / TZ, ntiles = ((N + TY - 1) / TY) * tiles_z;
    const uint32_t zoff = (uint32_t)(A * MAXR) * PIXB;
    REQUIRE(t.bp_win.size() == (size_t)ntiles * P && t.bp_cell.size() >= (size_t)ntiles * P * TY * TZ, "bp tile table sizes");
    for (int k = 0; k < ntiles; ++k) {
        const int y0 = (k / tiles_z) * TY, z0 = (k % tiles_z) * TZ;
        for (int lp = 0; lp < TY * TZ; ++lp) {
            const int y = y0 + lp / TZ, z = z0 + lp % TZ;
            for (int i = 0; i < P; ++i) {
                const uint32_t w = t.bp_win[(size_t)k * P + i], lo = w & 0xFFFFu, nr = w >> 16;
                REQUIRE(nr <= (uint32_t)MAXR && lo + nr <= (uint32_t)N, "bad window");
                const Tables::TileCell &c = t.bp_cell[((size_t)k * P + i) * (TY * TZ) + lp];
                double acc = 0;
                for (int h = 0; h < 2; ++h) {
                    const uint32_t off = h ? c.off1 : c.off0; const float wt = h ? c.w1 : c.w0;
                    if (off == zoff) { REQUIRE(wt == 0.f, "zero row with weight"); continue; }
                    const uint32_t slot = off / ((uint32_t)MAXR * PIXB), j = (off / PIXB) % MAXR;
                    REQUIRE(off % PIXB == 0 && slot == (uint32_t)(i % A) && j < nr, "bad cell offset");
                    acc += (double)wt * pb.rr[(int64_t)i * N + lo + j];
                }
                REQUIRE(acc == bp_ref(pb, t, i, y, z), "tile BP of pixel (%d, %d) angle %d", y, z, i);
            }
        }
    }
    return 0;
}

static int check_sart_tiles(const Problem &pb, const Tables &t)
{
    const int N = pb.N, P = pb.P, SY = ST_TY, SZ = ST_TZ, SMAXR = ST_MAXR, MS = Tables::ST_MAXSEG, NB = Tables::TILE_BATCH;
    const int stz = t.st_tiles_z, snt = t.st_tiles;
    int64_t real = 0;
    for (int i = 0; i < P; ++i) {
        std::vector<double> ps(t.st_max_ids, 0.0);
        std::vector<int> wr(t.st_max_ids, 0);
        for (int k = 0; k < snt; ++k) {
            const int y0 = (k / stz) * SY, z0 = (k % stz) * SZ;
            bool ended = false;
            for (int q = 0; q < MS; ++q) {
                const uint32_t b0 = t.st_seg[(((size_t)i * snt + k) * MS + q) * 2], nb = t.st_seg[(((size_t)i * snt + k) * MS + q) * 2 + 1];
                if (nb == 0) { ended = true; continue; }
                REQUIRE(!ended, "segment slots of a tile are not contiguous");
                REQUIRE(((size_t)b0 + nb) * NB <= t.st_off.size(), "SART batches out of range");
                double acc = 0;
                for (uint32_t e = 0; e < nb * NB; ++e) {
                    const uint32_t off = t.st_off[(size_t)b0 * NB + e]; const float w = t.st_w[(size_t)b0 * NB + e];
                    const uint32_t lp = off / PIXB;
                    REQUIRE(off % PIXB == 0 && lp <= (uint32_t)(SY * SZ), "bad SART entry offset");
                    if (lp == (uint32_t)(SY * SZ)) { REQUIRE(w == 0.f, "padding with weight"); continue; }
                    const int y = y0 + lp / SZ, z = z0 + lp % SZ;
                    REQUIRE(y < N && z < N, "SART entry outside the image");
                    acc += (double)w * pb.x[(int64_t)y * N + z];
                    if (w != 0.f) ++real;
                }
                const uint32_t pid = t.st_segid[((size_t)i * snt + k) * MS + q];
                REQUIRE(pid < t.st_max_ids, "partial id out of range");
                ps[pid] = acc; wr[pid]++;
            }
            const uint32_t w = t.st_win[(size_t)i * snt + k], lo = w & 0xFFFFu, nr = w >> 16;
            REQUIRE(nr <= (uint32_t)SMAXR && lo + nr <= (uint32_t)N, "SART window");
            for (int lp = 0; lp < SY * SZ; ++lp) {
                const int y = y0 + lp / SZ, z = z0 + lp % SZ;
                const Tables::TileCell &c = t.st_cell[((size_t)i * snt + k) * (SY * SZ) + lp];
                double a = 0;
                for (int h = 0; h < 2; ++h) {
                    const uint32_t off = h ? c.off1 : c.off0; const float wt = h ? c.w1 : c.w0;
                    if (off == (uint32_t)SMAXR * PIXB) { REQUIRE(wt == 0.f, "zero row with weight"); continue; }
                    REQUIRE(off % PIXB == 0 && off / PIXB < nr, "bad SART cell offset");
                    a += (double)wt * pb.rr[(int64_t)i * N + lo + off / PIXB];
                }
                REQUIRE(a == bp_ref(pb, t, i, y, z), "SART tile BP of pixel (%d, %d) angle %d", y, z, i);
            }
        }
        for (int j = 0; j < N; ++j) {
            const int64_t r = (int64_t)i * N + j;
            double sum = 0;
            for (uint32_t q = t.st_row_first[r]; q < t.st_row_first[r] + t.st_row_nseg[r]; ++q) { REQUIRE(q < t.st_max_ids && wr[q] == 1, "row uses an unwritten partial"); sum += ps[q]; wr[q] = 2; }
            REQUIRE(std::fabs(sum - pb.g[r]) <= 1e-9 * (1.0 + std::fabs(pb.g[r])), "SART tile FP of row %ld", (long)r);
        }
        for (uint32_t q = 0; q < t.st_max_ids; ++q) REQUIRE(wr[q] != 1, "partial %u of angle %d belongs to no row", q, i);
    }
    REQUIRE(real == pb.nz, "SART tile streams hold %ld non-zero entries, matrix has %ld", (long)real, (long)pb.nz);
    return 0;
}

static int check_strips(const Problem &pb, const Tables &t)
{
    constexpr int W = Tables::FS_W, H = Tables::FS_H, WAVES = Tables::FS_WAVES, GROUPS = Tables::FS_GROUPS, NB = Tables::TILE_BATCH;
    const int N = pb.N;
    std::vector<double> part(t.fs_nseg, 0.0);
    std::vector<int> seen(t.fs_nseg, 0);
    int64_t real = 0;
    REQUIRE(t.fs_orient.size() == (size_t)t.fs_npass && t.fs_shift.size() == (size_t)t.fs_npass * N, "strip pass tables");
    for (size_t it = 0; it < t.fs_item.size(); ++it) {
        const Tables::FsItem &I = t.fs_item[it];
        REQUIRE(I.pass >= 0 && I.pass < t.fs_npass, "pass out of range");
        REQUIRE((size_t)I.g0 + GROUPS < t.fs_gstart.size() && (size_t)I.g0 + GROUPS < t.fs_gseg0.size(), "group tables");
        REQUIRE(((size_t)I.cnt0 + (size_t)I.ntiles * WAVES) * 16 <= t.fs_cnt.size(), "count table");
        const int o = t.fs_orient[I.pass];
        const int32_t *sh = t.fs_shift.data() + (size_t)I.pass * N;
        for (int grp = 0; grp < GROUPS; ++grp) {
            const int wave = grp >> 2;
            size_t b = t.fs_gstart[I.g0 + grp];
            uint32_t seg = t.fs_gseg0[I.g0 + grp];
            double acc[16] = {0};
            for (uint32_t tt = 0; tt < I.ntiles; ++tt) {
                const uint8_t *cnt = t.fs_cnt.data() + ((size_t)I.cnt0 + (size_t)tt * WAVES + wave) * 16;
                for (int k = 0; k < 16; ++k) {
                    REQUIRE(k < t.fs_kused || cnt[k] == 0, "slot %d beyond fs_kused = %d has batches", k, t.fs_kused);
                    const int h = cnt[k], units = (h + 1) >> 1;
                    for (int q = 0; q < units; ++q, ++b) {
                        const bool half = q >= (h >> 1);
                        bool last = false;
                        REQUIRE((b + 1) * NB <= t.fs_ent_n, "strip batch %zu beyond the stream", b);
                        for (int j = 0; j < NB; ++j) {
                            const size_t at = b * NB + j;
                            const uint32_t off = Tables::fs_off_of(t.fs_ent[at]); const float w = Tables::fs_w_of(t.fs_ent[at]);
                            if (j == 0) last = off >> 31; else REQUIRE((off >> 31) == (uint32_t)last, "flag differs inside batch %zu", b);
                            if (half && j >= NB / 2) { REQUIRE(t.fs_ent[at] == t.fs_ent[at - NB / 2], "half batch %zu is not stored twice", b); continue; }
                            const uint32_t lp = (off & 0x7FFFFFFFu) / PIXB;
                            REQUIRE((off & 0x7FFFFFFFu) % PIXB == 0 && lp <= (uint32_t)(W * H), "bad offset");
                            if (lp == (uint32_t)(W * H)) { REQUIRE(w == 0.f, "padding entry with weight"); continue; }
                            const int u = (int)(I.tile0 + tt) * H + (int)(lp / W);
                            REQUIRE(u < N, "march coordinate %d outside the image", u);
                            const int v = I.v0 + sh[u] + (int)(lp % W);
                            REQUIRE(v >= 0 && v < N, "cross coordinate %d outside the image", v);
                            acc[k] += (double)w * pb.x[o ? (int64_t)v * N + u : (int64_t)u * N + v];
                            if (w != 0.f) ++real;
                        }
                        if (last) { REQUIRE(seg < t.fs_nseg, "segment id out of range"); part[seg] = acc[k]; seen[seg]++; acc[k] = 0.0; ++seg; }
                    }
                }
            }
            for (int k = 0; k < 16; ++k) REQUIRE(acc[k] == 0.0, "item %zu group %d slot %d ends with an unflushed sum", it, grp, k);
            REQUIRE(b == t.fs_gstart[I.g0 + grp + 1] && seg == t.fs_gseg0[I.g0 + grp + 1], "stream of item %zu group %d does not meet the next", it, grp);
        }
    }
    REQUIRE(real == pb.nz, "strip streams hold %ld non-zero entries, matrix has %ld", (long)real, (long)pb.nz);
    for (uint32_t s = 0; s < t.fs_nseg; ++s) REQUIRE(seen[s] == 1, "partial sum %u written %d times", s, seen[s]);
    std::vector<int> used(t.fs_nseg, 0);
    REQUIRE(t.fs_rseg_ptr.size() == (size_t)pb.nrows + 1, "strip row lists");
    for (int64_t r = 0; r < pb.nrows; ++r) {
        double s = 0;
        for (uint32_t k = t.fs_rseg_ptr[r]; k < t.fs_rseg_ptr[r + 1]; ++k) { REQUIRE(k < t.fs_rseg_idx.size() && t.fs_rseg_idx[k] < t.fs_nseg, "row list id out of range"); s += part[t.fs_rseg_idx[k]]; used[t.fs_rseg_idx[k]]++; }
        REQUIRE(std::fabs(s - pb.g[r]) <= 1e-9 * (1.0 + std::fabs(pb.g[r])), "strip FP of row %ld: %.12g vs %.12g", (long)r, s, pb.g[r]);
    }
    for (uint32_t s = 0; s < t.fs_nseg; ++s) REQUIRE(used[s] == 1, "partial sum %u used %d times by the row lists", s, used[s]);
    return 0;
}

static int check_fp_lists(const Problem &pb, const Tables &t)
{
    constexpr int W = Tables::FL_W, TH = Tables::FL_TH, WAVES = Tables::FL_WAVES, ACC = Tables::FL_ACC, BATCH = Tables::FL_BATCH, LPIXB = Tables::FL_PIXB, REGS = Tables::FL_REGS;
    const int N = pb.N;
    std::vector<double> part(t.fl_nseg, 0.0);
    std::vector<int> written(t.fl_nseg, 0);
    int64_t real = 0;
    std::vector<double> tile((size_t)2 * W * TH);
    REQUIRE(t.fl_orient.size() == (size_t)t.fl_npass && t.fl_shift.size() == (size_t)t.fl_npass * N, "list pass tables");
    for (size_t it = 0; it < t.fl_item.size(); ++it) {
        const Tables::FlItem &I = t.fl_item[it];
        REQUIRE(I.pass >= 0 && I.pass < t.fl_npass && I.ntiles >= 1 && I.ntiles <= 64, "item %zu: pass %d, %u tiles", it, I.pass, I.ntiles);
        REQUIRE((size_t)I.lp0 + (size_t)I.ntiles * WAVES < t.fl_ptr.size() && (size_t)I.lp0 + (size_t)I.ntiles * WAVES < t.fl_fptr.size(), "list pointers of item %zu", it);
        const int o = t.fl_orient[I.pass];
        const int32_t *sh = t.fl_shift.data() + (size_t)I.pass * N;
        std::vector<double> acc((size_t)WAVES * ACC, 0.0);
        for (uint32_t tt = 0; tt < I.ntiles; ++tt) {
            for (int q = 0; q < W * TH; ++q) {
                const int u = (int)(I.tile0 + tt) * TH + q / W, vv = I.v0 + sh[std::min(u, N - 1)] + q % W;
                const bool ok = u < N && vv >= 0 && vv < N;
                tile[(size_t)(tt & 1) * W * TH + q] = ok ? pb.x[o ? (int64_t)vv * N + u : (int64_t)u * N + vv] : 0.0;
            }
            for (int w = 0; w < WAVES; ++w) {
                const size_t li = (size_t)I.lp0 + (size_t)tt * WAVES + w;
                REQUIRE(t.fl_ptr[li] <= t.fl_ptr[li + 1] && (size_t)t.fl_ptr[li + 1] * BATCH <= t.fl_ent_n, "list bounds");
                for (size_t e = (size_t)t.fl_ptr[li] * BATCH; e < (size_t)t.fl_ptr[li + 1] * BATCH; ++e) {
                    const uint32_t e0 = Tables::fs_off_of(t.fl_ent[e]); const float wt = Tables::fs_w_of(t.fl_ent[e]);
                    const uint32_t off = e0 & ~(uint32_t)(LPIXB - 1), reg = e0 & (uint32_t)(LPIXB - 1);
                    REQUIRE(off / LPIXB < (uint32_t)(2 * W * TH) && off / LPIXB / (W * TH) == (tt & 1), "entry reads pixel image %u of tile %u", off / LPIXB, tt);
                    REQUIRE(reg % REGS == 0 && reg / REGS < (uint32_t)ACC, "accumulator register %u", reg);
                    if (wt == 0.f) continue;                      // padding, or an explicit zero of the matrix: adds nothing
                    acc[(size_t)w * ACC + reg / REGS] += (double)wt * tile[off / LPIXB];
                    ++real;
                }
                REQUIRE(t.fl_fptr[li] <= t.fl_fptr[li + 1] && t.fl_fptr[li + 1] <= t.fl_flush.size(), "flush bounds");
                for (uint32_t fr = t.fl_fptr[li]; fr < t.fl_fptr[li + 1]; ++fr) {
                    const uint32_t reg = (uint32_t)t.fl_flush[fr], id = (uint32_t)(t.fl_flush[fr] >> 32);
                    REQUIRE(id == fr && id < t.fl_nseg, "partial-sum id %u of flush record %u", id, fr);
                    REQUIRE(reg % REGS == 0 && reg / REGS < (uint32_t)ACC, "flushed register %u", reg);
                    REQUIRE(!written[id], "partial sum %u written twice", id);
                    written[id] = 1;
                    part[id] = acc[(size_t)w * ACC + reg / REGS];
                    acc[(size_t)w * ACC + reg / REGS] = 0.0;
                }
            }
        }
        for (size_t k = 0; k < acc.size(); ++k) REQUIRE(acc[k] == 0.0, "item %zu ends with a sum left in accumulator %zu", it, k);
    }
    REQUIRE(real == pb.nz, "lists hold %ld of %ld non-zero matrix entries", (long)real, (long)pb.nz);
    for (uint32_t id = 0; id < t.fl_nseg; ++id) REQUIRE(written[id], "partial sum %u never written", id);
    std::vector<int> used(t.fl_nseg, 0);
    REQUIRE(t.fl_rseg_ptr.size() == (size_t)pb.nrows + 1, "list row lists");
    for (int64_t r = 0; r < pb.nrows; ++r) {
        double s = 0;
        for (uint32_t k = t.fl_rseg_ptr[r]; k < t.fl_rseg_ptr[r + 1]; ++k) { REQUIRE(k < t.fl_rseg_idx.size(), "row list"); const uint32_t id = t.fl_rseg_idx[k]; REQUIRE(id < t.fl_nseg && !used[id], "row list of ray %ld", (long)r); used[id] = 1; s += part[id]; }
        REQUIRE(std::fabs(s - pb.g[r]) <= 1e-9 * (1.0 + std::fabs(pb.g[r])), "list FP of row %ld: %.12g vs %.12g", (long)r, s, pb.g[r]);
    }
    for (uint32_t id = 0; id < t.fl_nseg; ++id) REQUIRE(used[id], "partial sum %u belongs to no ray", id);
    return 0;
}

static int check_bp_lists(const Problem &pb, const Tables &t)
{
    constexpr int TY = Tables::BL_TY, TZ = Tables::BL_TZ, WAVES = Tables::BL_WAVES, A = Tables::BL_A, MAXR = Tables::BL_MAXR, ROWB = Tables::BL_ROWB,
                  BATCH = Tables::BL_BATCH, REGS = Tables::BL_REGS, PPW = TY * TZ / WAVES;
    const int N = pb.N, P = pb.P;
    const int tiles_z = (N + TZ - 1) / TZ, ntiles = ((N + TY - 1) / TY) * tiles_z, nstage = (P + A - 1) / A;
    REQUIRE(t.bl_ptr.size() == (size_t)ntiles * nstage * WAVES + 1 && t.bl_win.size() == (size_t)ntiles * P, "table sizes");
    std::vector<uint8_t> seen((size_t)P * pb.npix, 0);
    uint64_t real = 0;
    for (int k = 0; k < ntiles; ++k) {
        const int y0 = (k / tiles_z) * TY, z0 = (k % tiles_z) * TZ;
        for (int s = 0; s < nstage; ++s)
            for (int w = 0; w < WAVES; ++w) {
                const size_t li = ((size_t)k * nstage + s) * WAVES + w;
                REQUIRE(t.bl_ptr[li] <= t.bl_ptr[li + 1] && t.bl_ptr[li + 1] <= t.bl_nbatch, "list bounds");
                int last_angle = -1;
                uint32_t last_ray = 0;
                for (size_t pr = (size_t)t.bl_ptr[li] * BATCH; pr < (size_t)t.bl_ptr[li + 1] * BATCH; ++pr) {
                    const uint32_t e0 = (uint32_t)t.bl_ent[2 * pr];
                    const uint32_t off = e0 & ~(uint32_t)(ROWB - 1);
                    const uint32_t buf = off / (A * MAXR * ROWB), in = off % (A * MAXR * ROWB), slot = in / (MAXR * ROWB), row = in % (MAXR * ROWB) / ROWB;
                    REQUIRE(buf == (uint32_t)(s & 1), "pair of stage %d in LDS buffer %u", s, buf);
                    const int i = s * A + (int)slot;
                    REQUIRE(i < P, "pair of an angle beyond the last");
                    const uint32_t win = t.bl_win[(size_t)k * P + i], lo = win & 0xFFFFu, nr = win >> 16;
                    REQUIRE(row < nr && lo + nr <= (uint32_t)N, "row %u outside the staged window of %u rows (tile %d angle %d)", row, nr, k, i);
                    const uint32_t ray = lo + row;
                    REQUIRE((uint32_t)(t.bl_ent[2 * pr + 1]) < (uint32_t)ROWB, "second half of a pair carries no offset");
                    for (int h = 0; h < 2; ++h) {
                        const uint32_t reg = (uint32_t)t.bl_ent[2 * pr + h] & (uint32_t)(ROWB - 1), wb = (uint32_t)(t.bl_ent[2 * pr + h] >> 32);
                        const float wt = bitsf(wb);
                        REQUIRE(reg % REGS == 0 && reg / REGS < (uint32_t)PPW, "accumulator register %u", reg);
                        if (wt == 0.f) { REQUIRE(reg == 0, "padding must go to accumulator 0"); continue; }
                        REQUIRE(i > last_angle || (i == last_angle && ray >= last_ray), "angles, and rows inside an angle, must ascend");
                        last_angle = i; last_ray = ray;
                        int ly, lz;
                        Tables::bl_pixel(w, (int)(reg / REGS), ly, lz);
                        const int y = y0 + ly, z = z0 + lz;
                        REQUIRE(y < N && z < N, "entry of a pixel outside the image");
                        const int64_t p = (int64_t)y * N + z;
                        const Cell &c = t.cell[(size_t)i * pb.npix + p];
                        uint8_t &st = seen[(size_t)i * pb.npix + p];
                        if (c.w0 != 0.f && st == 0 && ray == c.r0 && wt == c.w0) st = (c.w1 != 0.f) ? 1 : 2;
                        else if (c.w1 != 0.f && st == (c.w0 != 0.f ? 1 : 0) && ray == c.r1 && wt == c.w1) st = 2;
                        else REQUIRE(false, "entry (pixel %lld angle %d ray %u w %g) is not the next weight of its cell", (long long)p, i, ray, wt);
                        ++real;
                    }
                }
            }
    }
    uint64_t nnz = 0;
    for (int i = 0; i < P; ++i)
        for (int64_t p = 0; p < pb.npix; ++p) {
            const Cell &c = t.cell[(size_t)i * pb.npix + p];
            nnz += (c.w0 != 0.f) + (c.w1 != 0.f);
            REQUIRE(seen[(size_t)i * pb.npix + p] == ((c.w0 != 0.f || c.w1 != 0.f) ? 2 : 0), "cell (angle %d pixel %lld) not fully listed", i, (long long)p);
        }
    REQUIRE(real == nnz && (int64_t)nnz == pb.nz, "listed %llu of %llu weights (matrix %ld)", (unsigned long long)real, (unsigned long long)nnz, (long)pb.nz);
    return 0;
}

static int check_resident(const Problem &pb, const Tables &t, const Resident &R)
{
    constexpr int T = Resident::T, W = Resident::WAVES, Q = Resident::PPW;
    const int N = pb.N, P = pb.P, ntiles = R.ntiles;
    REQUIRE(R.tiles == (N + T - 1) / T && ntiles == R.tiles * R.tiles && R.rpt * ntiles >= N, "tile counts");
    REQUIRE(R.hdr.size() == (size_t)P * ntiles && R.cell.size() == (size_t)P * ntiles * W * Q * 4 && R.ts.size() == (size_t)P * ntiles * Resident::MAXWIN * Resident::TSN && R.rl.size() == (size_t)P * N * Resident::RL, "table sizes");
    int64_t nz_cells = 0;
    for (int i = 0; i < P; ++i) {
        const Cell *ci = t.cell.data() + (size_t)i * pb.npix;
        std::vector<double> tsum((size_t)ntiles * Resident::MAXWIN, 0.0);
        for (int k = 0; k < ntiles; ++k) {
            const Resident::Hdr &h = R.hdr[(size_t)i * ntiles + k];
            REQUIRE(h.nrays <= Resident::MAXWIN && h.jbase + h.nrays <= N, "window of tile %d angle %d", k, i);
            const int y0 = (k / R.tiles) * T, z0 = (k % R.tiles) * T;
            std::vector<double> pbuf((size_t)W * 16, 0.0);
            for (int w = 0; w < W; ++w) {
                const uint32_t *cc = R.cell.data() + (((size_t)i * ntiles + k) * W + w) * Q * 4;
                int top = -1;
                for (int q = 0; q < Q; ++q) {
                    int ly, lz; Resident::pixel(w, q, ly, lz);
                    const int y = y0 + ly, z = z0 + lz;
                    const uint32_t s0 = cc[q * 4];
                    const float w0 = bitsf(cc[q * 4 + 1]), w1 = bitsf(cc[q * 4 + 2]);
                    REQUIRE(s0 <= (uint32_t)Resident::SINK, "slot range");
                    REQUIRE((w0 != 0.f) == (s0 < (uint32_t)Resident::USABLE) && (w1 == 0.f || (w0 != 0.f && s0 + 1 < (uint32_t)Resident::USABLE)), "slots of tile %d wave %d pixel %d angle %d", k, w, q, i);
                    const float cs = w0 + w1, inv = 1.0f / (cs > 0.f ? cs : 1.0f);
                    REQUIRE(bitsf(cc[q * 4 + 3]) == inv, "divisor");
                    if (y >= N || z >= N) { REQUIRE(w0 == 0.f && w1 == 0.f, "weight outside the image"); continue; }
                    const Cell &c = ci[(int64_t)y * N + z];
                    const int base = h.jbase + h.dw[w];
                    if (c.w0 != 0.f) { REQUIRE(w0 == c.w0 && base + (int)s0 == (int)c.r0, "first ray of pixel (%d,%d) angle %d", y, z, i); ++nz_cells; }
                    else REQUIRE(w0 == 0.f, "phantom first weight");
                    if (c.w1 != 0.f) { REQUIRE(w1 == c.w1 && base + (int)s0 + 1 == (int)c.r1, "second ray of pixel (%d,%d) angle %d", y, z, i); ++nz_cells; }
                    else REQUIRE(w1 == 0.f, "phantom second weight");
                    pbuf[(size_t)w * 16 + s0] += (double)w0 * pb.x[(int64_t)y * N + z];
                    pbuf[(size_t)w * 16 + s0 + 1] += (double)w1 * pb.x[(int64_t)y * N + z];
                    if (w0 != 0.f) top = std::max(top, (int)s0);
                    if (w1 != 0.f) top = std::max(top, (int)s0 + 1);
                }
                REQUIRE(top < 0 || h.dw[w] + top < h.nrays, "a wave's window reaches beyond the tile's");
                REQUIRE(pbuf[(size_t)w * 16 + 14] == 0.0 && pbuf[(size_t)w * 16 + 15] == 0.0, "the sink rows must stay zero");
            }
            for (int r = 0; r < h.nrays; ++r) {
                const uint8_t *e = R.ts.data() + (((size_t)i * ntiles + k) * Resident::MAXWIN + r) * Resident::TSN;
                double acc = 0.0, all = 0.0;
                int prev = -1;
                bool padded = false;
                for (int c = 0; c < Resident::TSN; ++c) {
                    if (e[c] == Resident::TS_PAD) { padded = true; continue; }
                    REQUIRE(!padded, "entry behind the padding");
                    const int w = e[c] >> 4, sl = e[c] & 15;
                    REQUIRE(w > prev && sl < Resident::USABLE && h.dw[w] + sl == r, "tile-sum entry %d of ray %d tile %d angle %d", c, r, k, i);
                    acc += pbuf[(size_t)w * 16 + sl];
                    prev = w;
                }
                for (int w = 0; w < W; ++w) { const int sl = r - h.dw[w]; if ((unsigned)sl < (unsigned)Resident::USABLE) all += pbuf[(size_t)w * 16 + sl]; }
                REQUIRE(acc == all, "tile sum of ray %d tile %d angle %d misses a block", r, k, i);
                tsum[(size_t)k * Resident::MAXWIN + r] = acc;
            }
        }
        for (int j = 0; j < N; ++j) {
            const uint16_t *list = R.rl.data() + ((size_t)i * N + j) * Resident::RL;
            double got = 0.0;
            int prev_tile = -1, cnt = 0, holders = 0;
            for (int e = 0; e < Resident::RL; ++e) {
                if (list[e] == 0xFFFF) { for (int f = e; f < Resident::RL; ++f) REQUIRE(list[f] == 0xFFFF, "hole in a reducer list"); break; }
                const int tile = list[e] / Resident::MAXWIN, slot = list[e] % Resident::MAXWIN;
                REQUIRE(tile > prev_tile && tile < ntiles, "reducer list not ascending");
                const Resident::Hdr &h = R.hdr[(size_t)i * ntiles + tile];
                REQUIRE(h.jbase + slot == j && slot < h.nrays, "reducer entry names another ray");
                got += tsum[list[e]];
                prev_tile = tile; ++cnt;
            }
            for (int k = 0; k < ntiles; ++k) { const Resident::Hdr &h = R.hdr[(size_t)i * ntiles + k]; if (j >= h.jbase && j < h.jbase + h.nrays) ++holders; }
            REQUIRE(holders == cnt, "ray %d angle %d: %d windows hold it, %d listed", j, i, holders, cnt);
            const double want = pb.g[(int64_t)i * N + j];
            REQUIRE(std::fabs(got - want) <= 1e-10 * (1.0 + std::fabs(want)), "resident FP of ray %d angle %d: %.12g vs %.12g", j, i, got, want);
        }
    }
    REQUIRE(nz_cells == pb.nz, "%ld weights in the resident cells, %ld in the matrix", (long)nz_cells, (long)pb.nz);
    return 0;
}

static int check_walk(const Problem &pb, const Tables &t)
{
    const int N = pb.N, P = pb.P;
    REQUIRE(t.walk_ptr.size() == (size_t)pb.nrows + 1 && t.walk_ptr[pb.nrows] == t.walk_pix.size() && t.walk_w.size() == t.walk_pix.size(), "walk sizes");
    int64_t real = 0;
    for (int i = 0; i < P; ++i) {
        std::vector<int> owners(pb.npix, 0);
        for (int j = 0; j < N; ++j) {
            const int64_t r = (int64_t)i * N + j;
            REQUIRE(t.walk_ptr[r] <= t.walk_ptr[r + 1], "walk pointers descend");
            double s = 0;
            for (uint32_t k = t.walk_ptr[r]; k < t.walk_ptr[r + 1]; ++k) {
                const uint32_t p = t.walk_pix[k] & 0x7FFFFFFFu;
                REQUIRE((int64_t)p < pb.npix, "walk pixel out of range");
                if (t.walk_pix[k] >> 31) {
                    owners[p]++;
                    // the owner of a crossed pixel is the first ray of its cell; an un-crossed pixel is owned with weight 0
                    const Cell &c = t.cell[(size_t)i * pb.npix + p];
                    REQUIRE(c.w0 != 0.f ? (c.r0 == (uint32_t)j && t.walk_w[k] == c.w0) : t.walk_w[k] == 0.f, "owner visit of pixel %u angle %d ray %d", p, i, j);
                }
                s += (double)t.walk_w[k] * pb.x[p];
                if (t.walk_w[k] != 0.f) ++real;
            }
            REQUIRE(std::fabs(s - pb.g[r]) <= 1e-9 * (1.0 + std::fabs(pb.g[r])), "walk FP of row %ld", (long)r);
        }
        for (int64_t p = 0; p < pb.npix; ++p) REQUIRE(owners[p] == 1, "pixel %ld of angle %d has %d owner visits", (long)p, i, owners[p]);
    }
    REQUIRE(real == pb.nz, "walk lists hold %ld non-zero entries, matrix has %ld", (long)real, (long)pb.nz);
    // segment items: every walk list cut exactly once, ids below the angle's count
    REQUIRE(t.seg_exec_ptr.size() == (size_t)P + 1 && t.seg_exec_ptr[P] == t.seg_exec.size(), "segment item sizes");
    std::vector<uint8_t> cover(t.walk_pix.size(), 0);
    for (int i = 0; i < P; ++i) {
        REQUIRE((t.seg_exec_ptr[i + 1] - t.seg_exec_ptr[i]) % 8 == 0, "items of an angle are eight equal lists");
        std::vector<int> idseen(t.max_items_per_angle, 0);
        for (uint32_t q = t.seg_exec_ptr[i]; q < t.seg_exec_ptr[i + 1]; ++q) {
            const Tables::SegItem &I = t.seg_exec[q];
            if (I.id == 0xFFFFFFFFu) continue;
            REQUIRE(I.id < t.max_items_per_angle && !idseen[I.id], "item id %u", I.id);
            idseen[I.id] = 1;
            REQUIRE(I.kbeg < I.kend && I.kend <= t.walk_pix.size() && I.kend - I.kbeg <= (uint32_t)SEG_LEN, "item range");
            REQUIRE(I.kbeg >= t.walk_ptr[(size_t)i * N] && I.kend <= t.walk_ptr[(size_t)(i + 1) * N], "item outside its angle");
            for (uint32_t k = I.kbeg; k < I.kend; ++k) { REQUIRE(!cover[k], "walk visit %u in two items", k); cover[k] = 1; }
        }
    }
    for (size_t k = 0; k < cover.size(); ++k) REQUIRE(cover[k], "walk visit %zu in no item", k);
    for (int64_t r = 0; r < pb.nrows; ++r)
        REQUIRE(t.row_nseg[r] == (t.walk_ptr[r + 1] - t.walk_ptr[r] + SEG_LEN - 1) / SEG_LEN && t.row_first[r] + t.row_nseg[r] <= t.max_items_per_angle, "row segments of row %ld", (long)r);
    return 0;
}

int main(int argc, char **argv)
{
    REQUIRE(argc > 1, "usage: user_matrix_check FILE [quiet]");
    const bool quiet = argc > 2;
    Problem pb;
    std::vector<float> rows, cols, vals;
    int64_t nnz = 0;
    {
        FILE *f = std::fopen(argv[1], "rb");
        REQUIRE(f, "cannot open %s", argv[1]);
        int32_t hdr[3];
        REQUIRE(std::fread(hdr, 4, 3, f) == 3 && std::fread(&nnz, 8, 1, f) == 1, "short header");
        pb.N = hdr[0]; pb.P = hdr[1]; pb.nchunk = hdr[2];
        REQUIRE(pb.N > 0 && pb.N <= 4096 && pb.P > 0 && pb.nchunk > 0 && nnz >= 0 && nnz < (1 << 28), "bad header");
        rows.resize(nnz); cols.resize(nnz); vals.resize(nnz);
        REQUIRE(std::fread(rows.data(), 4, nnz, f) == (size_t)nnz && std::fread(cols.data(), 4, nnz, f) == (size_t)nnz && std::fread(vals.data(), 4, nnz, f) == (size_t)nnz, "short file");
        std::fclose(f);
    }
    const int N = pb.N, P = pb.P;
    pb.nrows = (int64_t)N * P; pb.npix = (int64_t)N * N;
    std::string err;
    REQUIRE(coo_from_triplets(pb.nrows, pb.npix, nnz, rows.data(), cols.data(), vals.data(), pb.m, err), "%s", err.c_str());
    sort_rows(pb.m);
    Coo &m = pb.m;
    {   // the canonical matrix, formed independently: stable order by (row, col), the last assignment of a run stays
        std::vector<int64_t> order(nnz);
        for (int64_t k = 0; k < nnz; ++k) order[k] = k;
        auto key = [&](int64_t k) { return (int64_t)rows[k] * pb.npix + (int64_t)cols[k]; };
        std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return key(a) < key(b); });
        int64_t o = 0, dropped = 0;
        REQUIRE(m.ptr.size() == (size_t)pb.nrows + 1 && m.ptr[0] == 0, "row pointers");
        for (int64_t k = 0; k < nnz; ++k) {
            if (k + 1 < nnz && key(order[k + 1]) == key(order[k])) { ++dropped; continue; }
            const int64_t r = (int64_t)rows[order[k]];
            REQUIRE(o < m.ptr[pb.nrows] && o >= m.ptr[r] && o < m.ptr[r + 1], "entry %ld of the canonical matrix is not in row %ld of the sorted one", (long)o, (long)r);
            REQUIRE(m.col[o] == (uint32_t)cols[order[k]] && std::memcmp(&m.val[o], &vals[order[k]], 4) == 0, "sort_rows: entry (%ld, %u) holds %g, the last assignment is %g", (long)r, m.col[o], m.val[o], vals[order[k]]);
            ++o;
        }
        REQUIRE(o == m.ptr[pb.nrows] && (int64_t)m.col.size() == o && (int64_t)m.val.size() == o, "sort_rows kept %ld entries, the canonical matrix has %ld", (long)m.ptr[pb.nrows], (long)o);
        if (!quiet) std::printf("N=%d P=%d nchunk=%d: %ld triplets, %ld dropped as earlier assignments\n", N, P, pb.nchunk, (long)nnz, (long)dropped);
    }
    for (int64_t k = 0; k < m.ptr[pb.nrows]; ++k) if (m.val[k] != 0.f) ++pb.nz;
    std::mt19937 rng(7); std::uniform_real_distribution<double> U(0.1, 1.0);
    pb.x.resize(pb.npix); pb.g.assign(pb.nrows, 0.0); pb.rr.resize(pb.nrows);
    for (auto &v : pb.x) v = U(rng);
    for (auto &v : pb.rr) v = U(rng) - 0.5;
    for (int64_t r = 0; r < pb.nrows; ++r) for (int64_t k = m.ptr[r]; k < m.ptr[r + 1]; ++k) pb.g[r] += (double)m.val[k] * pb.x[m.col[k]];
    Tables t;
    if (!build_tables(m, N, P, t, err)) { std::printf("tables_ok=0 (%s)\n", err.c_str()); return 0; }
    {   // cells: the non-zero weights of the matrix, ascending ray; the neighbour property
        std::vector<Cell> cell((size_t)P * pb.npix, Cell{0u, 0.f, 0u, 0.f});
        bool chain = true;
        for (int64_t r = 0; r < pb.nrows; ++r)
            for (int64_t k = m.ptr[r]; k < m.ptr[r + 1]; ++k) {
                if (m.val[k] == 0.f) continue;
                Cell &c = cell[(size_t)(r / N) * pb.npix + m.col[k]];
                if (c.w0 == 0.f) { c.r0 = (uint32_t)(r % N); c.w0 = m.val[k]; } else { REQUIRE(c.w1 == 0.f, "three rays through a cell"); c.r1 = (uint32_t)(r % N); c.w1 = m.val[k]; if (c.r1 != c.r0 + 1) chain = false; }
            }
        REQUIRE(std::memcmp(cell.data(), t.cell.data(), cell.size() * sizeof(Cell)) == 0, "cell table differs from the matrix");
        REQUIRE(chain == t.art_chain_ok, "art_chain_ok is %d, the cells say %d", (int)t.art_chain_ok, (int)chain);
        for (int64_t r = 0; r < pb.nrows; ++r) {
            float s = 0.f, q = 0.f;
            for (int64_t k = m.ptr[r]; k < m.ptr[r + 1]; ++k) { s += m.val[k]; q += m.val[k] * m.val[k]; }
            REQUIRE(s == t.rowsum[r] && q == t.rowinner[r], "row sums of row %ld", (long)r);
        }
    }
    const bool chain_ok = t.art_chain_ok;
    build_tiles(m, N, P, FT_TY, FT_TZ, PIXB, t);
    if (check_tile_fp(pb, t)) return 1;
    std::string why_s, why_l;
    const bool fs_ok = build_fp_strips(m, N, P, PIXB, pb.nchunk, t, why_s);
    if (fs_ok && check_strips(pb, t)) return 1;
    const bool fl_ok = build_fp_lists(m, N, P, t, why_l);
    if (fl_ok && check_fp_lists(pb, t)) return 1;
    build_sart_tiles(m, N, P, ST_TY, ST_TZ, ST_MAXR, PIXB, t);
    const bool st_ok = t.st_ok;
    if (st_ok && check_sart_tiles(pb, t)) return 1;
    build_walk(m, N, P, t);
    build_segments(N, P, SEG_LEN, t);
    if (check_walk(pb, t)) return 1;
    Resident R;
    if (N % 8 == 0) build_sart_resident(N, P, t, CUS, R);
    if (R.ok && check_resident(pb, t, R)) return 1;
    build_bp_tiles(N, P, FT_TY, FT_TZ, FB_A, FB_MAXR, PIXB, 2 * FB_A, t);
    const bool fb_ok = t.bp_tile_ok && P <= FB_MAX_PROJ;
    if (fb_ok && check_tile_bp(pb, t)) return 1;
    build_bp_lists(N, P, Tables::BL_TY, Tables::BL_TZ, Tables::BL_A, Tables::BL_MAXR, Tables::BL_ROWB, Tables::BL_WAVES, Tables::BL_BATCH, Tables::BL_REGS, t);
    const bool bl_ok = t.bl_ok && (P + Tables::BL_A - 1) / Tables::BL_A <= 64;
    if (t.bl_ok && check_bp_lists(pb, t)) return 1;
    if (!quiet) {
        if (!fs_ok) std::printf("build_fp_strips refused: %s\n", why_s.c_str());
        if (!fl_ok) std::printf("build_fp_lists refused: %s\n", why_l.c_str());
        if (N % 8 == 0 && !R.ok) std::printf("build_sart_resident refused: %s\n", R.why.c_str());
    }
    std::printf("tables_ok=1 art_chain_ok=%d fp_strip_ok=%d fp_list_ok=%d sart_tile_ok=%d sart_resident_ok=%d bp_tile_ok=%d bp_list_ok=%d\n",
                (int)chain_ok, (int)fs_ok, (int)fl_ok, (int)st_ok, (int)(R.ok && st_ok), (int)fb_ok, (int)bl_ok);
    return 0;
}
