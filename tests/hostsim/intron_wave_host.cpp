// Test-only host build of spliser_amd/csrc/spl_intron_wave.h (how a team of lanes of spl_intron.hip takes the trimmed depth of one
// intron: searches, stretches, the radix selection of both rank values, the sum) under the wave emulator: a wave of 64 fibers per
// intron, the shared memory a struct on the host; tests/test_intron_wave_host.py holds the results against the yardstick's
// base-by-base expansion.
#include <vector>

#define WAVE_EMUL_IMPLEMENTATION
#include "wave_emul.h"
// spl_wave.h's shared-memory adds on the host: between two rendezvous the lanes run one after the other, so a plain
// read-modify-write is the atomic
namespace wv {
inline uint32_t lds_add(uint32_t *p, uint32_t v) { const uint32_t o = *p; *p = o + v; return o; }
inline void lds_add64(uint64_t *p, uint64_t v) { *p += v; }
} // namespace wv
#include "../../spliser_amd/csrc/spl_intron_wave.h"

// Intron i has the pieces piece_off[i] .. piece_off[i + 1]; out: 4 words an intron.  -> 0, or < 0 when a wave broke a rule of the
// emulator.
extern "C" int intron_wave_run(const int32_t *bound_pos, const uint32_t *bound_depth, int64_t n_bound, int64_t n_introns, const int64_t *piece_off, const int32_t *piece_start,
                               const int32_t *piece_end, uint32_t trim_percent, int64_t *out)
{
    static splintron::Shared sh; // (kept from intron to intron, as a workgroup's is)
    const splintron::Depth depth{bound_pos, bound_depth, n_bound};
    for (int64_t i = 0; i < n_introns; ++i) {
        const splintron::Pieces pieces{piece_start + piece_off[i], piece_end + piece_off[i], piece_off[i + 1] - piece_off[i]};
        const bool ok = wv::run_wave([&]() { splintron::team_intron(wv::lane(), 64u, depth, pieces, trim_percent, &sh, out + 4 * i); });
        if (!ok) return -1;
    }
    return 0;
}
