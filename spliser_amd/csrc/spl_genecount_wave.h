// spl_genecount_wave.h -- how a wave adds its 64 results to the gene counts (spl_genecount.hip), written against spl_wave.h's
// primitives: the same source runs on the device and under tests/hostsim/wave_emul.h on a CPU (tests/test_genecount_wave_host.py).
//
// A histogram that survives hot genes: one gene can take tens of millions of reads, and a read a lane adding one to its gene's
// counter would queue all of them on one word.  Reads are coordinate-sorted, so neighbouring lanes mostly hold the same gene.
// Within a wave, RUNS of equal results in lane order are counted: a lane is a HEAD when it is lane 0 or when its result differs
// from the result of the lane before it; the run's length is the distance to the next head (the ballot of heads), or to the end of
// the wave; the head of a run of gene results makes ONE 64-bit add of that length.  Results that return to an earlier value
// (A B A) are three runs: nothing is searched for, and nothing depends on the order of the reads -- any order gives the same sums,
// a sorted one few adds.  The three special results (no feature, ambiguous, not counted) are a ballot and a popcount each, kept by
// lane c for counter c, as spl_strand_tally keeps its counters; a lane without a read holds SPL_GENE_IDLE, which is counted nowhere.
#ifndef SPL_GENECOUNT_WAVE_H
#define SPL_GENECOUNT_WAVE_H
#include <stdint.h>

#include "spl_wave.h"

namespace splgene {

constexpr uint32_t NO_FEATURE = 0xFFFFFFFCu, AMBIGUOUS = 0xFFFFFFFDu, NOT_COUNTED = 0xFFFFFFFEu, IDLE = 0xFFFFFFFFu; // (= SPL_GENE_* of spl_genecount_rule.h)
constexpr uint32_t SPECIALS = 3u;

// Called by all 64 lanes.  The runs of equal values in lane order: -> whether this lane is a run's head; length: the lanes of the
// run from this lane on (the whole run's for its head).  (spl_exoncount_wave.h counts its rounds of bins with it too.)
WV_DEV bool wave_run(uint32_t value, uint32_t &length)
{
    const uint32_t lane = wv::lane();
    const uint32_t before = wv::shfl_up(value, 1u); // (lane 0 gets its own back: it is a head whatever it holds)
    const uint64_t heads = wv::ballot(lane == 0u || before != value);
    const uint64_t above = lane < 63u ? heads >> (lane + 1u) : 0ull; // the heads behind this lane, the next one in bit 0
    length = above ? wv::ffs64(above) + 1u : 64u - lane;
    return ((heads >> lane) & 1ull) != 0ull;
}

// Called by all 64 lanes.  result: this lane's; counts: n_genes 64-bit words in device memory; mine: lane c's running sum of
// special counter c (c < SPECIALS).  A gene result at or beyond n_genes is counted nowhere (there is none: said for the memory's sake).
WV_DEV void wave_count(uint32_t result, uint32_t n_genes, uint64_t *counts, uint32_t &mine)
{
    const uint32_t lane = wv::lane();
    uint32_t length;
    if (wave_run(result, length) && result < n_genes) wv::mem_add64(&counts[result], (uint64_t)length);
#pragma unroll
    for (uint32_t c = 0; c < SPECIALS; ++c) {
        const uint64_t b = wv::ballot(result == NO_FEATURE + c);
        if (lane == c) mine += wv::popc64(b);
    }
}

} // namespace splgene
#endif
