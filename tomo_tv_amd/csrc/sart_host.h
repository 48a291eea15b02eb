// sart_host.h -- the host-only arithmetic of the SART / ART sweeps (no HIP header, so the CPU checks it: tests/native/sart_host_check.cpp):
// the permutation check of a caller's order, and the counters of the volume-resident launch (launch_sart_resident, engine_sart.inc).
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace tomo {

// order[0 .. n) names every index of [0, n) once
inline bool is_permutation(const int32_t *order, int64_t n)
{
    std::vector<char> seen((size_t)n, 0);
    for (int64_t q = 0; q < n; ++q) {
        if (order[q] < 0 || order[q] >= n || seen[order[q]]) return false;
        seen[order[q]] = 1;
    }
    return true;
}

// What the resident launches of one engine count.  A launch of `rounds` chunk rounds and `steps` steps tags its granules
// epoch0 + 1 ... epoch0 + rounds * steps (tag 0 = never written), expects every commit word at commit_base and adds the number of
// tiles to each when it commits, and stores seq (never 0) into the host done-word of every chunk it stored.
struct RsLedger {
    uint32_t epoch = 0, seq = 0, commit_base = 0;   // tags handed out so far; the last launch's number; what every commit word holds
    bool commit_dirty = false;                      // a launch did not commit: the words differ
    int skip = 0, backoff = 0;                      // sweeps the resident form still sits out; the length of the last sit-out
    int fallbacks = 0, fallback_chunks = 0;         // sweeps that needed the streamed chain, and the 64-slice chunks it swept
    int last_code = 0;                              // the wait that gave up in the last of them: 1 residual rows, 2 tile sums (0: the commit)
    // clear_*: due before the launch: both granule arrays, the commit words, the host done-words
    struct Launch { bool clear_tags, clear_commit, clear_done; uint32_t epoch0, seq, commit_base; };
    Launch begin(int rounds, int64_t steps)
    {
        Launch l{};
        const uint64_t need = (uint64_t)rounds * (uint64_t)steps;
        if ((uint64_t)epoch + need + 16 > 0xFFFFFFFFull) { l.clear_tags = true; epoch = 0; }   // the tags wrap: back to the state after creation
        // the commit words: cleared after a launch that did not commit, and before the count could reach the poison bit
        if (commit_dirty || commit_base > 0x7F000000u) { l.clear_commit = true; commit_base = 0; commit_dirty = false; }
        if (++seq >= 0x7FFFFFF0u) { l.clear_done = true; seq = 1; }
        l.epoch0 = epoch; l.seq = seq; l.commit_base = commit_base;
        epoch += (uint32_t)need;
        return l;
    }
    // the verdict: nfailed chunks were not stored (code: the abort word the launch left).  The resident form then sits out `skip`
    // sweeps, doubling up to 64 while the failures go on.
    void finish(int nfailed, int ntiles, int code)
    {
        if (!nfailed) { commit_base += (unsigned)ntiles; backoff = 0; return; }
        commit_dirty = true;
        last_code = code;
        ++fallbacks;
        fallback_chunks += nfailed;
        skip = backoff = std::min(64, std::max(1, 2 * backoff));
    }
};

}  // namespace tomo
