// Test-only host build of spliser_amd/csrc/spl_dups_wave.h (the keep decision of spl_reads_dedup over spl_subsample_wave.h's tile
// bodies) under the wave emulator: a wave of 64 fibers per tile, the two launches one after the other as the device's stream runs
// them, the scan of the tiles' totals between them a plain loop; tests/test_duplicates_host.py holds the result against numpy's
// boolean mask.  Returns 0, or < 0 when a wave broke a rule of the emulator or the totals do not fit the room given.
#include <vector>

#define WAVE_EMUL_IMPLEMENTATION
#include "wave_emul.h"
#include "../../spliser_amd/csrc/spl_dups_wave.h"

extern "C" uint32_t dups_wave_tile() { return splsub::TILE; }

// The arguments of subsample_wave_run with `dup` (a byte per entry of the arrays) in the place of the seed and the threshold.
extern "C" int dups_wave_run(uint32_t n_seg, const int64_t *seg_first, const int64_t *seg_n, int64_t n_rec, int64_t n_ops, const int32_t *pos, const uint16_t *flag,
                             const uint32_t *cig_off, const uint32_t *cigar, const uint8_t *xs, const uint64_t *key, const uint8_t *dup, int64_t cap_rec, int64_t cap_ops,
                             int32_t *pos_out, uint16_t *flag_out, uint32_t *cig_off_out, uint32_t *cigar_out, uint8_t *xs_out, uint64_t *key_out, uint32_t *index_out,
                             int64_t *kept_out)
{
    std::vector<splsub::Seg> segs(n_seg);
    uint64_t n_tiles = 0;
    int64_t base = 0;
    for (uint32_t k = 0; k < n_seg; ++k) {
        segs[k] = splsub::Seg{seg_first[k], seg_n[k], base, n_tiles};
        n_tiles += (uint64_t)((seg_n[k] + splsub::TILE - 1) / splsub::TILE);
        base += seg_n[k];
    }
    const splsub::Src src{pos, flag, cig_off, cigar, xs, key, n_rec, n_ops};
    std::vector<uint32_t> rows(2 * (size_t)n_tiles + 1, 0u);
    for (uint64_t t = 0; t < n_tiles; ++t) {
        int64_t lo, hi, at;
        splsub::tile_range(segs.data(), n_seg, t, &lo, &hi, &at);
        if (!wv::run_wave([&]() { spldup::tile_count(src, lo, hi, dup, &rows[t], &rows[n_tiles + t]); })) return -1;
    }
    for (uint64_t t = 1; t < n_tiles; ++t) { rows[t] += rows[t - 1]; rows[n_tiles + t] += rows[n_tiles + t - 1]; }
    const int64_t kept = n_tiles ? rows[n_tiles - 1] : 0, kept_ops = n_tiles ? rows[2 * n_tiles - 1] : 0;
    if (kept > cap_rec || kept_ops > cap_ops) return -2;
    for (uint32_t k = 0; k < n_seg; ++k) {
        const uint64_t end = k + 1 < n_seg ? segs[k + 1].tile0 : n_tiles, begin = segs[k].tile0;
        kept_out[k] = (int64_t)(end ? rows[end - 1] : 0) - (int64_t)(begin ? rows[begin - 1] : 0);
        kept_out[n_seg + k] = (int64_t)(end ? rows[n_tiles + end - 1] : 0) - (int64_t)(begin ? rows[n_tiles + begin - 1] : 0);
    }
    const splsub::Dst dst{pos_out, flag_out, cig_off_out, cigar_out, xs_out, key_out, index_out, kept, kept_ops};
    cig_off_out[kept] = (uint32_t)kept_ops;
    for (uint64_t t = 0; t < n_tiles; ++t) {
        int64_t lo, hi, at;
        splsub::tile_range(segs.data(), n_seg, t, &lo, &hi, &at);
        const uint32_t read0 = t ? rows[t - 1] : 0u, op0 = t ? rows[n_tiles + t - 1] : 0u;
        if (!wv::run_wave([&]() { spldup::tile_write(src, dst, lo, hi, at, dup, read0, op0); })) return -3;
    }
    return 0;
}
