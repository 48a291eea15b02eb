// dev_pool.h -- the one owner of an engine's device allocations (host-only: no HIP header, the allocator is passed in).
// Ownership is keyed by the ADDRESS of an allocation: the engine's ping-pong pairs change places at run time, so which member holds an
// allocation at teardown depends on the call history.  An entry knows its member (`slot`) only to null it on release, and only if the
// member still holds the address: one that was swapped, or rebound to a caller's buffer, is left alone.
#pragma once
#include <cstddef>
#include <mutex>
#include <vector>

namespace tomo {

class DevPool {
public:
    enum Life { GEOMETRY, COMM, ENGINE };              // freed with the tilt geometry / with the communicator / only with the engine
    using AllocFn = int (*)(void **, size_t);          // 0 = success; any other value is handed back by alloc()
    using FreeFn = void (*)(void *);
    DevPool(AllocFn a, FreeFn f) : alloc_(a), free_(f) {}
    ~DevPool() { release_all(); }

    // *slot = a new allocation of `bytes` (zero bytes: 4, so that the pointer is valid); the allocator's code on failure
    int alloc(Life life, void **slot, size_t bytes)
    {
        void *p = nullptr;
        if (int rc = alloc_(&p, bytes ? bytes : 4)) return rc;
        std::lock_guard<std::mutex> lk(mu_);           // (the launch helpers allocate on first use, also from the chain helper threads)
        ents_.push_back(Entry{p, bytes, life, slot});
        *slot = p;
        return 0;
    }
    // -1: the pool does not own `ptr` (nothing is freed)
    int release(void *ptr) { return take(ptr, nullptr, nullptr); }
    // `ptr` changes owner: *slot, a member of the new owner, holds it from now on.  -1: not owned
    int move_to(DevPool &other, void *ptr, void **slot) { return &other == this ? -1 : take(ptr, &other, slot); }
    void release_life(Life life) { sweep(&life); }
    void release_all() { sweep(nullptr); }
    // the sizes asked for, summed over the live allocations
    size_t bytes() const
    {
        std::lock_guard<std::mutex> lk(mu_);
        size_t n = 0;
        for (const Entry &en : ents_) n += en.bytes;
        return n;
    }

private:
    struct Entry { void *ptr; size_t bytes; Life life; void **slot; };
    void unslot(const Entry &en) { if (*en.slot == en.ptr) *en.slot = nullptr; }
    int take(void *ptr, DevPool *to, void **slot)      // the entry leaves this pool: freed, or handed to `to` (one lock at a time)
    {
        std::unique_lock<std::mutex> lk(mu_);
        size_t k = 0;
        while (k < ents_.size() && ents_[k].ptr != ptr) ++k;
        if (k == ents_.size()) return -1;
        Entry en = ents_[k];
        ents_.erase(ents_.begin() + (std::ptrdiff_t)k);
        lk.unlock();
        unslot(en);
        if (!to) { free_(ptr); return 0; }
        std::lock_guard<std::mutex> lo(to->mu_);
        to->ents_.push_back(Entry{ptr, en.bytes, en.life, slot});
        *slot = ptr;
        return 0;
    }
    void sweep(const Life *life)                       // null: every entry
    {
        std::lock_guard<std::mutex> lk(mu_);
        size_t kept = 0;
        for (Entry &en : ents_) { if (!life || en.life == *life) { free_(en.ptr); unslot(en); } else ents_[kept++] = en; }
        ents_.resize(kept);
    }
    AllocFn alloc_;
    FreeFn free_;
    mutable std::mutex mu_;
    std::vector<Entry> ents_;
};

}  // namespace tomo
