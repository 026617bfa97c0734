// spl_exoncount_wave.h -- how a wave adds its 64 reads' bins and verdicts to the exon-bin counts (spl_exoncount.hip), written
// against spl_wave.h's primitives: the same source runs on the device and under tests/hostsim/wave_emul.h on a CPU
// (tests/test_exoncount_wave_host.py).
//
// A read adds to SEVERAL bins, and a hot exon takes tens of millions of reads; coordinate-sorted neighbours hit the same bins.
// The commit works in ROUNDS: in round j every lane of the wave offers its j-th bin (`next()` of its source: the second walk of
// its read, nothing is stored per lane), or IDLE when it has none left.  Within a round, RUNS of equal bins in lane order make ONE
// 64-bit add each -- the head / run logic of splgene::wave_run, which spl_gene_count's histogram uses too.  The wave goes on while
// a ballot says some lane still has a bin: a read over 70 bins costs its wave 70 rounds, whatever the other lanes hold.  The four
// verdict counters are a ballot and a popcount each, kept by lane c for counter c.  Integer sums: exact, whatever the order.
#ifndef SPL_EXONCOUNT_WAVE_H
#define SPL_EXONCOUNT_WAVE_H
#include <stdint.h>

#include "spl_genecount_wave.h"

namespace splexon {

constexpr uint32_t VERDICTS = 4u;          // counted, no feature, ambiguous, not counted (= SPL_EXON_* of spl_exoncount_rule.h)
constexpr uint32_t IDLE_VERDICT = 4u;      // a lane without a read
constexpr uint32_t NO_BIN = 0xFFFFFFFFu;   // what a source says that has no further bin

// Called by all 64 lanes.  verdict: this lane's; mine: lane c's running sum of verdict counter c (c < VERDICTS).
WV_DEV void wave_verdicts(uint32_t verdict, uint32_t &mine)
{
    const uint32_t lane = wv::lane();
#pragma unroll
    for (uint32_t c = 0; c < VERDICTS; ++c) {
        const uint64_t b = wv::ballot(verdict == c);
        if (lane == c) mine += wv::popc64(b);
    }
}

// Called by all 64 lanes.  src.next(): this lane's next bin, NO_BIN when it has none (and from then on); counts: n_bins 64-bit
// words in device memory.  A bin at or beyond n_bins is counted nowhere (there is none: said for the memory's sake).
template <class Source>
WV_DEV void wave_commit(Source &src, uint32_t n_bins, uint64_t *counts)
{
    for (;;) {
        const uint32_t bin = src.next();
        if (!wv::any(bin != NO_BIN)) break; // (uniform: every lane leaves in the same round)
        uint32_t length;
        if (splgene::wave_run(bin, length) && bin < n_bins) wv::mem_add64(&counts[bin], (uint64_t)length);
    }
}

} // namespace splexon
#endif
