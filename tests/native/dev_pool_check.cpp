// Host-only check of the engine's device-memory registry (tomo_tv_amd/csrc/dev_pool.h) with malloc / free as the allocator: lifetimes,
// swapped and rebound slots, the hand-over of an allocation between two pools, allocation from two threads.  Built with ASan + UBSan
// (tests/native/Makefile: san): a double free aborts at once, and the leak check at exit is the leak assertion.
// Usage: dev_pool_check [quiet]
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <set>
#include <thread>
#include "dev_pool.h"
using namespace tomo;

#define REQUIRE(c, ...) do { if (!(c)) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); return 1; } } while (0)

// the allocator: malloc / free, with the set of live blocks kept beside it so that "freed exactly once" and "survived" can be asked
static std::mutex g_mu;
static std::set<void *> g_live;
static int g_bad_free = 0;
static int host_alloc(void **p, size_t bytes)
{
    *p = std::malloc(bytes);
    if (!*p) return 2;
    std::lock_guard<std::mutex> lk(g_mu);
    g_live.insert(*p);
    return 0;
}
static void host_free(void *p)
{
    { std::lock_guard<std::mutex> lk(g_mu); if (!g_live.erase(p)) ++g_bad_free; }
    std::free(p);
}
static bool live(void *p) { std::lock_guard<std::mutex> lk(g_mu); return g_live.count(p) != 0; }
static size_t nlive() { std::lock_guard<std::mutex> lk(g_mu); return g_live.size(); }

int main(int argc, char **)
{
    const bool quiet = argc > 1;
    {   // lifetimes: the geometry goes and its slots are nulled, the engine's buffers stay until release_all
        DevPool pool(host_alloc, host_free);
        void *table[3] = {}, *sino = nullptr, *vol = nullptr, *scratch = nullptr, *plane = nullptr;
        for (int k = 0; k < 3; ++k) REQUIRE(pool.alloc(DevPool::GEOMETRY, &table[k], 100 + k) == 0, "alloc");
        REQUIRE(pool.alloc(DevPool::ENGINE, &vol, 4096) == 0 && pool.alloc(DevPool::GEOMETRY, &sino, 640) == 0 && pool.alloc(DevPool::ENGINE, &scratch, 4096) == 0, "alloc");
        REQUIRE(pool.bytes() == 100 + 101 + 102 + 4096 + 640 + 4096, "bytes() is the sum of the sizes asked for: %zu", pool.bytes());
        void *const t0 = table[0], *const t1 = table[1], *const t2 = table[2], *const s0 = sino, *const v0 = vol, *const c0 = scratch;
        pool.release_life(DevPool::GEOMETRY);
        REQUIRE(!live(t0) && !live(t1) && !live(t2) && !live(s0), "release_life(GEOMETRY) frees every geometry entry");
        REQUIRE(!table[0] && !table[1] && !table[2] && !sino, "... and nulls their slots");
        REQUIRE(live(v0) && live(c0) && vol == v0 && scratch == c0, "engine entries survive it");
        REQUIRE(pool.bytes() == 2 * 4096 && nlive() == 2, "what is left: %zu bytes, %zu blocks", pool.bytes(), nlive());
        pool.release_life(DevPool::GEOMETRY);                   // nothing left of that life: no second free
        REQUIRE(pool.alloc(DevPool::COMM, &plane, 64) == 0, "alloc");
        void *const p0 = plane;
        pool.release_life(DevPool::COMM);
        REQUIRE(!live(p0) && !plane && live(v0) && live(c0) && nlive() == 2, "release_life(COMM) frees the communicator's buffers alone");
        pool.release_all();
        REQUIRE(nlive() == 0 && g_bad_free == 0 && !vol && !scratch && pool.bytes() == 0, "release_all frees each of the rest once");
        pool.release_all();
        REQUIRE(g_bad_free == 0, "a second release_all frees nothing");
    }
    {   // a ping-pong pair whose members changed places (volume <-> tv_alt): each buffer freed once
        DevPool pool(host_alloc, host_free);
        void *vol = nullptr, *alt = nullptr;
        REQUIRE(pool.alloc(DevPool::ENGINE, &vol, 256) == 0 && pool.alloc(DevPool::ENGINE, &alt, 256) == 0, "alloc");
        void *const a = vol, *const b = alt;
        vol = b; alt = a;
        pool.release_all();
        REQUIRE(!live(a) && !live(b) && nlive() == 0 && g_bad_free == 0, "swapped slots: both freed, each once");
        REQUIRE(vol == b && alt == a, "a slot that holds another address is left alone");
    }
    {   // a slot rebound to a caller's buffer (tomo_bind_halo ...): the foreign buffer is neither freed nor nulled
        DevPool pool(host_alloc, host_free);
        void *halo = nullptr, *foreign = std::malloc(64);
        REQUIRE(pool.alloc(DevPool::ENGINE, &halo, 64) == 0, "alloc");
        void *const own = halo;
        halo = foreign;
        REQUIRE(pool.release(foreign) != 0, "release of a pointer the pool does not own is an error");
        pool.release_all();
        REQUIRE(!live(own) && halo == foreign && g_bad_free == 0, "the engine's own buffer went, the caller's stayed");
        static_cast<char *>(foreign)[63] = 1;                   // still writable: ASan would stop a use after free here
        std::free(foreign);
    }
    {   // release by address, unknown addresses, zero bytes
        DevPool pool(host_alloc, host_free);
        void *stage = nullptr, *empty = nullptr;
        int on_stack = 0;
        REQUIRE(pool.alloc(DevPool::ENGINE, &stage, 1000) == 0 && pool.alloc(DevPool::GEOMETRY, &empty, 0) == 0, "alloc");
        REQUIRE(empty != nullptr && live(empty), "a zero-byte allocation gives a valid pointer");
        static_cast<char *>(empty)[3] = 7;                      // ... of 4 bytes
        REQUIRE(pool.bytes() == 1000, "a zero-byte allocation counts as zero bytes");
        REQUIRE(pool.release(&on_stack) != 0 && pool.release(nullptr) != 0, "unknown pointer: an error return");
        void *const st = stage;
        REQUIRE(pool.release(stage) == 0 && !live(st) && stage == nullptr && pool.bytes() == 0, "release(ptr) frees and nulls the slot");
        REQUIRE(pool.release(st) != 0 && g_bad_free == 0, "a second release of the same address is an error, not a double free");
    }   // (the destructor releases `empty`)
    REQUIRE(nlive() == 0 && g_bad_free == 0, "the pool's destructor releases what is left");
    {   // adoption: an allocation changes owner (tomo_adopt_volumes); the source's teardown must not touch it
        struct Engine { void *vol = nullptr, *alt = nullptr; DevPool pool{host_alloc, host_free}; };
        Engine *src = new Engine(), dst;
        REQUIRE(src->pool.alloc(DevPool::ENGINE, &src->vol, 500) == 0 && src->pool.alloc(DevPool::ENGINE, &src->alt, 300) == 0, "alloc");
        void *const moved = src->alt, *const other = src->vol;
        src->vol = moved; src->alt = other;                     // the volume sits in the allocation made for the partner slot
        REQUIRE(dst.pool.move_to(src->pool, moved, &dst.vol) != 0, "move_to of a pointer the pool does not own is an error");
        REQUIRE(src->pool.move_to(dst.pool, src->vol, &dst.vol) == 0, "move_to");
        REQUIRE(dst.vol == moved && src->alt == other, "move_to fills the new slot and leaves a swapped old one alone");
        src->vol = nullptr;
        REQUIRE(src->pool.bytes() == 500 && dst.pool.bytes() == 300, "bytes() moves with the entry: %zu / %zu", src->pool.bytes(), dst.pool.bytes());
        REQUIRE(src->pool.release(moved) != 0, "the source no longer owns it");
        src->pool.release_all();
        REQUIRE(live(moved) && !live(other), "the source's release_all frees only what it still owns");
        delete src;                                             // the slot the entry was allocated into is gone with its engine: it was re-pointed
        dst.pool.release_all();
        REQUIRE(!live(moved) && dst.vol == nullptr && nlive() == 0 && g_bad_free == 0, "the destination's frees it, through the new slot");
    }
    {   // a scratch buffer that grows on demand (ensure_stage, al_ensure: keep while large enough, else release and allocate anew), used by
        // callers of different sizes in a row: every byte a caller asked for is writable (ASan), the old block is freed once, and
        // bytes() ends at the largest request whatever the order -- what "pool_bytes" compares between a used and a fresh engine
        struct Scratch { void *p = nullptr; size_t have = 0; };
        auto ensure = [](DevPool &pool, Scratch &s, size_t bytes) {
            if (s.have >= bytes) return 0;
            if (s.p) { if (pool.release(s.p)) return 1; s.have = 0; }
            if (int rc = pool.alloc(DevPool::ENGINE, &s.p, bytes)) return rc;
            s.have = bytes;
            return 0;
        };
        const size_t order_a[] = {4096, 432, 6144, 1152, 144, 4096, 72}, order_b[] = {6144, 4096, 4096, 1152, 432, 144, 72};
        size_t total[2] = {0, 0};
        int k = 0;
        for (const size_t *order : {order_a, order_b}) {
            DevPool pool(host_alloc, host_free);
            Scratch s;
            void *other = nullptr;
            REQUIRE(pool.alloc(DevPool::ENGINE, &other, 1000) == 0, "alloc");
            int grown = 0;
            for (int i = 0; i < 7; ++i) {
                void *const before = s.p;
                REQUIRE(ensure(pool, s, order[i]) == 0 && s.have >= order[i], "ensure(%zu)", order[i]);
                if (s.p != before) { ++grown; REQUIRE(!before || !live(before), "the outgrown block was freed"); }
                for (size_t b = 0; b < order[i]; ++b) static_cast<char *>(s.p)[b] = (char)i;      // the whole request is the caller's to write
                REQUIRE(pool.bytes() == 1000 + s.have && nlive() == 2, "one scratch block at a time: %zu bytes, %zu blocks", pool.bytes(), nlive());
            }
            REQUIRE(grown == (k == 0 ? 2 : 1) && s.have == 6144, "grown %d times to %zu", grown, s.have);
            total[k++] = pool.bytes();
        }
        REQUIRE(total[0] == total[1] && nlive() == 0 && g_bad_free == 0, "the same bytes in either order: %zu / %zu", total[0], total[1]);
    }
    {   // first-use allocations from the main thread and a chain helper thread at once: no entry lost
        DevPool pool(host_alloc, host_free);
        constexpr int N = 2000;
        static void *slots[2][N];
        int rcs[2] = {0, 0};
        auto work = [&](int w) { for (int k = 0; k < N; ++k) rcs[w] |= pool.alloc(k & 1 ? DevPool::GEOMETRY : DevPool::ENGINE, &slots[w][k], 8 + (size_t)w); };
        std::thread th(work, 1);
        work(0);
        th.join();
        REQUIRE(rcs[0] == 0 && rcs[1] == 0 && nlive() == 2 * N, "every allocation is live: %zu", nlive());
        REQUIRE(pool.bytes() == (size_t)N * 8 + (size_t)N * 9, "every allocation is registered: %zu bytes", pool.bytes());
        pool.release_life(DevPool::GEOMETRY);
        REQUIRE(nlive() == N, "half of them were the geometry's");
        for (int w = 0; w < 2; ++w) for (int k = 0; k < N; ++k) REQUIRE((slots[w][k] == nullptr) == ((k & 1) != 0), "slot %d of thread %d", k, w);
        pool.release_all();
        REQUIRE(nlive() == 0 && g_bad_free == 0, "and all are freed, each once");
    }
    if (!quiet) std::printf("dev_pool: ok\n");
    return 0;
}
