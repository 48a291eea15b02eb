// Host-only check of the SART sweeps' host arithmetic (tomo_tv_amd/csrc/sart_host.h): the permutation check of a caller's order and the
// counters of the volume-resident launch -- the wrap of the granule tags, the clear of the commit words, the restart of the sequence
// number and the sit-out after failed launches.  On the GPU these take billions of steps to reach; here the ledger starts just below each
// boundary.  The expected values restate the rules of launch_sart_resident independently (plain 64-bit arithmetic on a copy of the state).
// Built with ASan + UBSan (tests/native/Makefile: san).  Usage: sart_host_check [quiet]
#include <cstdint>
#include <cstdio>
#include <numeric>
#include <vector>
#include "sart_host.h"
using namespace tomo;

#define REQUIRE(c, ...) do { if (!(c)) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); return 1; } } while (0)

// Launches of (rounds, steps) from the ledger's present state: the tag clear fires exactly where the rule says, epoch0 restarts from 0
// there, and between two clears the tags handed out -- the kernel writes epoch0 + 1 ... epoch0 + rounds * steps -- are never 0, never past
// 32 bits, and no two launches share one (nor do the ranges [epoch0, epoch0 + rounds * steps) overlap).  Returns the clears seen, -1 on failure.
static int tags_run(RsLedger &L, int rounds, int64_t steps, int launches)
{
    const uint64_t need = (uint64_t)rounds * (uint64_t)steps;
    uint64_t run_end = L.epoch;                        // the end of the last range handed out since the last clear
    int clears = 0;
    for (int i = 0; i < launches; ++i) {
        const uint64_t before = L.epoch;
        const bool due = before + need + 16 > 0xFFFFFFFFull;
        const RsLedger::Launch l = L.begin(rounds, steps);
        if (l.clear_tags != due) { std::printf("FAIL tag clear at epoch %llu: %d, the rule says %d\n", (unsigned long long)before, (int)l.clear_tags, (int)due); return -1; }
        if (due) { ++clears; run_end = 0; if (l.epoch0 != 0) { std::printf("FAIL epoch0 = %u after a tag clear\n", l.epoch0); return -1; } }
        else if (l.epoch0 != before) { std::printf("FAIL epoch0 = %u, the ledger stood at %llu\n", l.epoch0, (unsigned long long)before); return -1; }
        const uint64_t first = (uint64_t)l.epoch0 + 1, last = (uint64_t)l.epoch0 + need;
        if (l.epoch0 < run_end || first == 0 || last > 0xFFFFFFFFull) { std::printf("FAIL tags [%llu, %llu] after a run that ended at %llu\n", (unsigned long long)first, (unsigned long long)last, (unsigned long long)run_end); return -1; }
        run_end = (uint64_t)l.epoch0 + need;
        if (L.epoch != run_end) { std::printf("FAIL the ledger stands at %u after a range that ends at %llu\n", L.epoch, (unsigned long long)run_end); return -1; }
        L.finish(0, 1, 0);
    }
    return clears;
}

int main(int argc, char **)
{
    const bool quiet = argc > 1;
    {   // the permutation check, over a few angles and over many rows
        std::vector<int32_t> id(9);
        std::iota(id.begin(), id.end(), 0);
        REQUIRE(is_permutation(id.data(), 9), "the identity is a permutation");
        const int32_t shuffled[9] = {4, 0, 8, 2, 6, 1, 7, 3, 5}, dup[9] = {4, 0, 8, 2, 6, 1, 7, 3, 4}, high[9] = {4, 0, 9, 2, 6, 1, 7, 3, 5}, neg[9] = {4, 0, 8, 2, 6, 1, 7, 3, -1};
        REQUIRE(is_permutation(shuffled, 9), "a shuffled order is a permutation");
        REQUIRE(!is_permutation(dup, 9), "a duplicate is rejected");
        REQUIRE(!is_permutation(high, 9), "an index out of range is rejected");
        REQUIRE(!is_permutation(neg, 9), "-1 is rejected");
        REQUIRE(is_permutation(shuffled, 0) && is_permutation(id.data(), 1) && !is_permutation(shuffled, 1), "lengths 0 and 1");
        std::vector<int32_t> rows(70000);
        for (size_t q = 0; q < rows.size(); ++q) rows[q] = (int32_t)((q * 7919) % rows.size());   // 7919 is prime to 70000
        REQUIRE(is_permutation(rows.data(), (int64_t)rows.size()), "a row order of an ART sweep");
        rows[123] = rows[60000];
        REQUIRE(!is_permutation(rows.data(), (int64_t)rows.size()), "... with one row named twice");
    }
    {   // a fresh ledger: the first launch clears nothing, starts the tags at 0 (first tag 1) and carries sequence number 1
        RsLedger L;
        const RsLedger::Launch l = L.begin(3, 90);
        REQUIRE(!l.clear_tags && !l.clear_commit && !l.clear_done, "nothing is cleared after creation");
        REQUIRE(l.epoch0 == 0 && l.seq == 1 && l.commit_base == 0 && L.epoch == 270, "epoch0 %u seq %u base %u epoch %u", l.epoch0, l.seq, l.commit_base, L.epoch);
    }
    // tag wrap: from just below 0xFFFFFFFF - 16 - rounds * steps across the boundary, for sweeps of several sizes
    for (const auto &shape : std::vector<std::pair<int, int64_t>>{{1, 1}, {3, 90}, {8, 900}, {2, (int64_t)1 << 24}}) {
        const uint64_t need = (uint64_t)shape.first * (uint64_t)shape.second;
        RsLedger L;
        L.epoch = (uint32_t)(0xFFFFFFFFull - 16 - 4 * need - need / 2);     // a few launches fit, then the boundary
        const int clears = tags_run(L, shape.first, shape.second, 12);
        REQUIRE(clears == 1, "%d x %lld: one tag clear in 12 launches across the boundary, got %d", shape.first, (long long)shape.second, clears);
        for (uint64_t start : {0xFFFFFFFFull - 16 - need - 1, 0xFFFFFFFFull - 16 - need, 0xFFFFFFFFull - 16 - need + 1}) {   // the last epoch that fits, and its neighbours
            RsLedger M;
            M.epoch = (uint32_t)start;
            const RsLedger::Launch l = M.begin(shape.first, shape.second);
            REQUIRE(l.clear_tags == (start + need + 16 > 0xFFFFFFFFull), "%d x %lld at epoch %llu", shape.first, (long long)shape.second, (unsigned long long)start);
            REQUIRE(l.clear_tags == (start == 0xFFFFFFFFull - 16 - need + 1), "only the last of the three is past the boundary");
        }
    }
    {   // commit base: +ntiles per committing launch, the clear due once it has passed 0x7F000000 -- and after any launch that did not commit
        const int ntiles = 256;
        RsLedger L;
        L.commit_base = 0x7F000000u - 3 * ntiles;
        for (int i = 0; i < 8; ++i) {
            const uint32_t before = L.commit_base;
            const bool due = before > 0x7F000000u;
            const RsLedger::Launch l = L.begin(1, 10);
            REQUIRE(l.clear_commit == due, "commit clear at base %u: %d, the rule says %d", before, (int)l.clear_commit, (int)due);
            REQUIRE(l.commit_base == (due ? 0u : before), "the launch expects the words at %u, got %u", due ? 0u : before, l.commit_base);
            REQUIRE(i != 4 || due, "the base passes 0x7F000000 with the fourth launch: the fifth clears");
            REQUIRE(l.commit_base + (uint64_t)ntiles < 0x80000000ull, "the count stays below the poison bit");
            L.finish(0, ntiles, 0);
            REQUIRE(L.commit_base == l.commit_base + ntiles && !L.commit_dirty, "a committing launch adds the tiles");
        }
        RsLedger::Launch l = L.begin(1, 10);
        const uint32_t base = l.commit_base;
        REQUIRE(!l.clear_commit && base > 0, "no clear in the middle of a run");
        L.finish(2, ntiles, 1);                                  // one launch that did not commit
        REQUIRE(L.commit_dirty && L.commit_base == base, "a failed launch marks the words and adds nothing");
        l = L.begin(1, 10);
        REQUIRE(l.clear_commit && l.commit_base == 0 && !L.commit_dirty, "... and the next launch clears them");
        L.finish(0, ntiles, 0);
        l = L.begin(1, 10);
        REQUIRE(!l.clear_commit && l.commit_base == (uint32_t)ntiles, "then the count goes on from the clear");
    }
    {   // sequence numbers: never 0, the done-words cleared and the count back at 1 where it would reach 0x7FFFFFF0
        RsLedger L;
        L.seq = 0x7FFFFFF0u - 4;
        uint32_t prev = L.seq;
        for (int i = 0; i < 8; ++i) {
            const bool due = (uint64_t)prev + 1 >= 0x7FFFFFF0u;
            const RsLedger::Launch l = L.begin(1, 10);
            REQUIRE(l.clear_done == due, "done-word clear after sequence number %u: %d, the rule says %d", prev, (int)l.clear_done, (int)due);
            REQUIRE(l.seq == (due ? 1u : prev + 1) && l.seq != 0 && (int)l.seq > 0 && l.seq == L.seq, "sequence number %u after %u", l.seq, prev);
            REQUIRE(i != 3 || due, "the fourth launch from 0x7FFFFFF0 - 4 restarts the count");
            prev = l.seq;
            L.finish(0, 1, 0);
        }
    }
    {   // failures: the sit-out doubles up to 64, one success resets it, the counters add up, the code is the one passed in
        RsLedger L;
        const int want[9] = {1, 2, 4, 8, 16, 32, 64, 64, 64};
        int chunks = 0;
        for (int i = 0; i < 9; ++i) {
            L.begin(2, 30);
            L.finish(i + 1, 100, 1 + i % 2);
            chunks += i + 1;
            REQUIRE(L.skip == want[i] && L.backoff == want[i], "sit-out after %d failures in a row: %d", i + 1, L.skip);
            REQUIRE(L.fallbacks == i + 1 && L.fallback_chunks == chunks && L.last_code == 1 + i % 2 && L.commit_dirty, "counters after %d failures", i + 1);
            L.skip = 0;                                           // (the sweeps in between used the sit-outs up)
        }
        L.begin(2, 30);
        L.finish(0, 100, 0);
        REQUIRE(L.backoff == 0 && L.skip == 0 && L.fallbacks == 9 && L.fallback_chunks == chunks && L.last_code == 1, "a success resets the back-off and keeps the history");
        L.begin(2, 30);
        L.finish(3, 100, 2);
        REQUIRE(L.skip == 1 && L.backoff == 1 && L.fallbacks == 10 && L.fallback_chunks == chunks + 3 && L.last_code == 2, "the next failure starts at 1 again");
    }
    if (!quiet) std::printf("sart_host: ok\n");
    return 0;
}
