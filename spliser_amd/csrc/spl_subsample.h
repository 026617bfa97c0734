// spl_subsample.h -- what spl_subsample.hip's launches take (the kernels' bodies are spl_subsample_wave.h, the rule
// spl_subsample_rule.h): plain structures and C entry points, for spl_capi.cpp and the tests' host builds.
#ifndef SPL_SUBSAMPLE_H
#define SPL_SUBSAMPLE_H
#include <stdint.h>

namespace splsub {

constexpr uint32_t ROUNDS = 16u, TILE = 64u * ROUNDS; // (lane l has the reads l, l + 64, ... of its tile: coalesced)
constexpr uint32_t LANE_OPS = 8u;                     // a CIGAR of more ops than this is copied by the wave

// A segment of the source set: its reads are the arrays' entries first .. first + n, the reads base .. base + n of the set, and
// the tiles tile0 .. tile0 + ceil(n / TILE) of the call.
struct Seg { int64_t first, n, base; uint64_t tile0; };

struct Src {
    const int32_t *pos; const uint16_t *flag; const uint32_t *cig_off, *cigar;
    const uint8_t *xs; const uint64_t *key; // xs: or null
    int64_t n_rec, n_ops;
};
struct Dst {
    int32_t *pos; uint16_t *flag; uint32_t *cig_off, *cigar;
    uint8_t *xs; uint64_t *key; uint32_t *index; // xs: null where the source has none; index: the kept reads' numbers in the source set
    int64_t n_rec, n_ops;                        // what the arrays have room for: the totals of the scan
};

} // namespace splsub

extern "C" {
uint32_t spl_dev_subsample_tile(void);
// Launch 1 over the n_tiles tiles of d_segs: rows[t] = the reads tile t keeps, rows[n_tiles + t] = their ops.
int spl_dev_launch_subsample_count(const splsub::Src *src, const splsub::Seg *d_segs, uint32_t n_seg, uint64_t n_tiles, uint64_t salt, uint64_t threshold, uint32_t *rows, void *stream);
// Behind the inclusive scans of the two rows: ends[k], ends[n_seg + k] = the kept reads and ops up to segment k's last tile.
int spl_dev_launch_subsample_ends(const uint32_t *rows, const splsub::Seg *d_segs, uint32_t n_seg, uint64_t n_tiles, uint32_t *ends, void *stream);
// Launch 3: the kept reads into dst, whose n_rec and n_ops are the scans' last sums; cig_off[n_rec] = n_ops is written too.
int spl_dev_launch_subsample_write(const splsub::Src *src, const splsub::Dst *dst, const splsub::Seg *d_segs, uint32_t n_seg, uint64_t n_tiles, uint64_t salt, uint64_t threshold,
                                   const uint32_t *rows, void *stream);
}
#endif
