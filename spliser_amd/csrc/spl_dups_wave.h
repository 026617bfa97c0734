// spl_dups_wave.h -- the second keep decision of spl_subsample_wave.h's tile bodies: a byte a read, kept where it is 0
// (spl_reads_dedup: the bytes are spl_reads_duplicates' marks).  The same source runs as one wave per workgroup on the device
// (spl_dups.hip) and under tests/hostsim/wave_emul.h on a CPU (tests/hostsim/dups_wave_host.cpp; tests/test_duplicates_host.py holds
// it against numpy's boolean mask).
#ifndef SPL_DUPS_WAVE_H
#define SPL_DUPS_WAVE_H
#include <stdint.h>

#include "spl_subsample_wave.h"

namespace spldup {

struct MaskKeep {
    const uint8_t *dup; // a byte per entry of the arrays
    SPL_HD bool operator()(const splsub::Src &, int64_t i, uint64_t, uint32_t) const { return dup[i] == 0u; }
};

WV_DEV void tile_count(const splsub::Src &s, int64_t lo, int64_t hi, const uint8_t *dup, uint32_t *reads_out, uint32_t *ops_out)
{
    splsub::tile_count_by(s, lo, hi, MaskKeep{dup}, reads_out, ops_out);
}

WV_DEV void tile_write(const splsub::Src &s, const splsub::Dst &d, int64_t lo, int64_t hi, int64_t base, const uint8_t *dup, uint32_t read0, uint32_t op0)
{
    splsub::tile_write_by(s, d, lo, hi, base, MaskKeep{dup}, read0, op0);
}

} // namespace spldup
#endif
