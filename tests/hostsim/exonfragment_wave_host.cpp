// Test-only host build of the body of spl_exon_count_fragments_kernel (spliser_amd/csrc/spl_exoncount.hip) under the wave emulator:
// a wave of 64 fibers per 64 reads of one segment, each lane taking its read's sides and verdict from spl_exonfragment_rule.h and
// handing the MERGE of its two walks (spl_exon_merge) to splexon::wave_commit, as the kernel does -- over flat maps, where the
// kernel's have a top level in LDS.  tests/test_exonfragment_wave_host.py holds the sums and the adds that were made against the
// yardstick's plain loops.
#include <vector>

#define WAVE_EMUL_IMPLEMENTATION
#include "wave_emul.h"
// spl_wave.h's mem_add64 on the host: between two rendezvous the lanes run one after the other, so a plain read-modify-write is
// the atomic; every call is written down (the word's index and what was added), which is what the tests count
namespace wv {
static uint64_t *g_add_base = nullptr;
static std::vector<uint64_t> g_adds; // pairs: index, value
inline void mem_add64(uint64_t *p, uint64_t v)
{
    *p += v;
    g_adds.push_back((uint64_t)(p - g_add_base));
    g_adds.push_back(v);
}
} // namespace wv
#include "../../spliser_amd/csrc/spl_exoncount_wave.h"
#include "../../spliser_amd/csrc/spl_exonfragment_rule.h"

static_assert(SPL_EXON_NO_BIN == splexon::NO_BIN, "the merge's ended walk is the commit's lane without a bin");

namespace {
struct LaneFragmentBins {
    spl_exon_merge<spl_gene_ops_ptr, spl_gene_map_flat> merge;
    uint32_t next() { return merge.next(); }
};
} // namespace

// The n reads of one segment with its mate table; a wave per 64 of them, the lanes behind the last one idle.  counts: n_bins
// words, added to; tallies: 4 words, added to (what the lanes 0..3 kept).  adds (or null): capacity pairs (index, value) of the
// adds made, in the order they were made; *n_adds their number.  -> 0, or < 0 when a wave broke a rule of the emulator.
extern "C" int exonfragment_wave_run(int64_t n, const int32_t *pos, const uint16_t *flag, const uint32_t *cig_off, const uint32_t *cigar, int64_t n_ops_total, const uint32_t *mate,
                                     int32_t shift, int stranded, int64_t n_a, const int32_t *a_start, const uint32_t *a_code, int64_t n_b, const int32_t *b_start, const uint32_t *b_code,
                                     uint32_t n_bins, const uint32_t *bin_gene, uint64_t *counts, uint64_t *tallies, uint64_t *adds, uint64_t capacity, uint64_t *n_adds)
{
    wv::g_add_base = counts;
    wv::g_adds.clear();
    const spl_mate_reads reads{pos, flag, cig_off, cigar, n_ops_total};
    const spl_gene_map_flat map_a{n_a, a_start, a_code}, map_b{n_b, b_start, b_code};
    for (int64_t base = 0; base < n; base += 64) {
        uint32_t mine[64] = {0};
        const bool ok = wv::run_wave([&]() {
            const uint32_t lane = wv::lane();
            const int64_t r = base + lane;
            uint32_t m = 0u, verdict = SPL_EXON_IDLE;
            spl_exon_side lead{0u, 0u, 0, false}, other{0u, 0u, 0, false};
            if (r < n) {
                verdict = spl_exon_fragment_sides(reads, 0, n, r, mate, (int64_t)shift, stranded, &lead, &other);
                if (verdict == SPL_EXON_COUNTED) verdict = spl_exon_fragment_verdict<spl_gene_ops_ptr>(cigar, lead, other, map_a, map_b, bin_gene);
            }
            splexon::wave_verdicts(verdict, m);
            if (verdict != SPL_EXON_COUNTED) lead.n_ops = other.n_ops = 0u;
            LaneFragmentBins bins{spl_exon_merge<spl_gene_ops_ptr, spl_gene_map_flat>(cigar, lead, other, map_a, map_b)};
            splexon::wave_commit(bins, n_bins, counts);
            mine[lane] = m;
        });
        if (!ok) return -1;
        for (uint32_t c = 0; c < splexon::VERDICTS; ++c) tallies[c] += mine[c];
        for (uint32_t l = splexon::VERDICTS; l < 64u; ++l)
            if (mine[l]) return -2; // (only the lanes 0..3 keep a verdict counter)
    }
    const uint64_t made = wv::g_adds.size() / 2u;
    if (n_adds) *n_adds = made;
    for (uint64_t k = 0; adds && k < made && k < capacity; ++k) { adds[2 * k] = wv::g_adds[2 * k]; adds[2 * k + 1] = wv::g_adds[2 * k + 1]; }
    return 0;
}
