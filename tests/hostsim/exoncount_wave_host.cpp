// Test-only host build of spliser_amd/csrc/spl_exoncount_wave.h (how a wave of spl_exoncount.hip adds its 64 reads' bins and
// verdicts to the counts) under the wave emulator: a wave of 64 fibers per 64 reads, each lane's bins a list it hands out one by
// one as the kernel's second walk does; tests/test_exoncount_wave_host.py holds the sums and the adds that were made against plain
// loops.
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

namespace {
struct ListBins {
    const uint32_t *p, *end;
    uint32_t next() { return p < end ? *p++ : splexon::NO_BIN; }
};
} // namespace

// Reads 0 .. n: read i has the verdict verdicts[i] and the bins bins[off[i] .. off[i + 1]); a wave per 64 of them, the lanes behind
// the last one idle.  counts: n_bins words, added to; tallies: 4 words, added to (what the lanes 0..3 kept).  adds (or null):
// capacity pairs (index, value) of the adds made, in the order they were made; *n_adds their number.  -> 0, or < 0 when a wave
// broke a rule of the emulator.
extern "C" int exoncount_wave_run(const uint32_t *verdicts, const uint64_t *off, const uint32_t *bins, uint64_t n, uint32_t n_bins, uint64_t *counts, uint64_t *tallies, uint64_t *adds,
                                  uint64_t capacity, uint64_t *n_adds)
{
    wv::g_add_base = counts;
    wv::g_adds.clear();
    for (uint64_t base = 0; base < n; base += 64u) {
        uint32_t mine[64] = {0};
        const bool ok = wv::run_wave([&]() {
            const uint32_t lane = wv::lane();
            const bool have = base + lane < n;
            uint32_t m = 0u;
            splexon::wave_verdicts(have ? verdicts[base + lane] : splexon::IDLE_VERDICT, m);
            ListBins src{have ? bins + off[base + lane] : nullptr, have ? bins + off[base + lane + 1] : nullptr};
            splexon::wave_commit(src, n_bins, counts);
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
