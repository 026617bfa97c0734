// spl_flagstat.h -- internal: THE definition of the flagstat counters (spl_bam_set_flagstat), as spl_bam.h has the read filter's.
//
// Sixteen categories, each counted twice: for records that passed the sequencer's quality control and for those that failed it
// (FLAG 0x200).  The device's record scan (spl_inflate.hip), the host decoder (bam_reader.cpp) and the test hook
// spl_flagstat_add_host all call spl_flagstat_categories and nothing else.  A record is PRIMARY when neither 0x100 (secondary)
// nor 0x800 (supplementary) is set; a record with both counts as secondary only.
//
//    0 total                         every record
//    1 primary                       primary
//    2 secondary                     0x100
//    3 supplementary                 0x800 and not 0x100
//    4 duplicates                    0x400
//    5 primary duplicates            primary and 0x400
//    6 mapped                        not 0x4
//    7 primary mapped                primary and not 0x4
//    8 paired in sequencing          primary and 0x1
//    9 read1                         8 and 0x40
//   10 read2                         8 and 0x80
//   11 properly paired               8, 0x2 and not 0x4
//   12 with itself and mate mapped   8, not 0x4, not 0x8
//   13 singletons                    8, 0x8 and not 0x4
//   14 mate on a different chr       12 and next_tid != tid
//   15 ... with mapQ >= 5            14 and mapq >= 5
//
// (samtools flagstat's lines as of 1.13, restated; parity with the tool itself is not pinned by a test: DESIGN.md section 9.)
#ifndef SPL_FLAGSTAT_H
#define SPL_FLAGSTAT_H
#include <stdint.h>

#include "spl_bam.h"
#include "spl_inflate.h"

#define SPL_FS_CATEGORIES 16

// bit c = the record belongs to category c
SPL_BAM_HD inline uint32_t spl_flagstat_categories(uint32_t flag, int32_t tid, int32_t next_tid, uint32_t mapq)
{
    const uint32_t primary = (flag & 0x900u) == 0u ? 1u : 0u;
    const uint32_t mapped = (flag & 0x4u) == 0u ? 1u : 0u;
    const uint32_t dup = (flag >> 10) & 1u;
    const uint32_t secondary = (flag >> 8) & 1u;
    const uint32_t paired = primary & (flag & 1u);
    const uint32_t mate_unmapped = (flag >> 3) & 1u;
    const uint32_t both = paired & mapped & (mate_unmapped ^ 1u);
    const uint32_t apart = both & (next_tid != tid ? 1u : 0u);
    return 1u | primary << 1 | secondary << 2 | (((flag >> 11) & 1u) & (secondary ^ 1u)) << 3 | dup << 4 | (primary & dup) << 5 | mapped << 6 | (primary & mapped) << 7 |
           paired << 8 | (paired & ((flag >> 6) & 1u)) << 9 | (paired & ((flag >> 7) & 1u)) << 10 | (paired & ((flag >> 1) & 1u) & mapped) << 11 | both << 12 |
           (paired & mate_unmapped & mapped) << 13 | apart << 14 | (apart & (mapq >= 5u ? 1u : 0u)) << 15;
}

#if defined(__HIPCC__)
// The counters of one BGZF block on the device: word c = category c, QC-passed records in its low half, QC-failed in its high half.
// Neither half can carry: no more than SPL_BS_REC_CAP records begin in a block.
static_assert(SPL_BS_REC_CAP <= 0xffffu, "a block's flagstat counters are 16 bits wide");
SPL_BAM_HD inline void spl_flagstat_add_packed(uint32_t w[SPL_FS_CATEGORIES], uint32_t flag, int32_t tid, int32_t next_tid, uint32_t mapq)
{
    const uint32_t m = spl_flagstat_categories(flag, tid, next_tid, mapq), sh = (flag >> 9 & 1u) * 16u;
#pragma unroll
    for (uint32_t c = 0; c < SPL_FS_CATEGORIES; ++c) w[c] += ((m >> c) & 1u) << sh;
}
#endif

// ... and everywhere else: out32[2 * c + q], q = 1 for QC-failed records
inline void spl_flagstat_add(int64_t out32[2 * SPL_FS_CATEGORIES], uint32_t flag, int32_t tid, int32_t next_tid, uint32_t mapq)
{
    const uint32_t m = spl_flagstat_categories(flag, tid, next_tid, mapq), q = flag >> 9 & 1u;
    for (uint32_t c = 0; c < SPL_FS_CATEGORIES; ++c) out32[2u * c + q] += (int64_t)((m >> c) & 1u);
}

#endif
