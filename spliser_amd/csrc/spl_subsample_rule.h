// spl_subsample_rule.h -- which reads of a read set a SUBSAMPLE keeps, as straight-line C++: the rule of spl_reads_subsample
// (spl_subsample.hip) and of `saturation` / `junctions --subsample`.
//
// The kernels include this header with SPL_HD = __device__ __forceinline__.  It contains no HIP intrinsics, so that tests/ compile
// it with g++ too (spl_subsample_keep_host, tests/hostsim/subsample_rule_asan.cpp); the product never calls it on the host.
//
// Replaces `samtools view -s SEED.FRAC` in front of a second run of the whole pipeline, twenty times over for a saturation curve
// (RSeQC's junction_saturation.py makes one of junctions, from a sorted file, in a Python loop).  The reference has no counterpart.
//
// THE RULE.  A read's decision depends on its NAME and the SEED only:
//   k = the read's name key (spl_mate_rule.h);  if k == 0, "no name":  k = (uint64)(uint32)POS << 32 | (uint64)FLAG << 16 | (n_ops & 0xffff)
//   z = k ^ (seed * 0x9e3779b97f4a7c15)                                                       (all mod 2^64)
//   z = (z ^ z >> 30) * 0xbf58476d1ce4e5b9;  z = (z ^ z >> 27) * 0x94d049bb133111eb;  z ^= z >> 31           (splitmix64's finisher)
//   u = z >> 32                                                                                (32 bits)
//   keep  <=>  u < threshold,   threshold in 0 .. 2^32   (2^32 keeps every read, 0 none)
// POS is the file's 1-based position, before any shard shift.
//
// WHAT FOLLOWS, and what the tests hold:
//   * both mates of a pair share one decision, and so does every secondary and supplementary record of the same name -- as under
//     `samtools view -s`;
//   * for one seed the kept sets are NESTED: T1 <= T2 gives kept(T1) a subset of kept(T2) -- a descending chain of selections, each
//     from the one before, selects what each would have selected from the whole;
//   * the decision depends neither on the order of the reads nor on the container: the same reads as BAM, SAM text, BGZF text or a
//     shuffled BAM keep the same names.
//
// NOT INTENDED: parity with samtools' choice of reads (its hash of the name is another, and so is its seed).  It would mean nothing
// for a random subset; parity with RSeQC / samtools -s is not claimed.
#ifndef SPL_SUBSAMPLE_RULE_H
#define SPL_SUBSAMPLE_RULE_H

#include <stdint.h>

#ifndef SPL_HD
#define SPL_HD inline
#endif

#define SPL_SUBSAMPLE_ALL 0x100000000ull // the threshold that keeps every read

// The seed as the rule takes it, made once a call.
SPL_HD uint64_t spl_subsample_salt(uint64_t seed) { return seed * 0x9e3779b97f4a7c15ull; }

// A read without a name: what stands in for its key.
SPL_HD uint64_t spl_subsample_nameless_key(int64_t pos, uint32_t flag, uint32_t n_ops)
{
    return (uint64_t)(uint32_t)pos << 32 | (uint64_t)(flag & 0xffffu) << 16 | (uint64_t)(n_ops & 0xffffu);
}

// u of a key that is not 0 (or of a nameless read's stand-in).
SPL_HD uint32_t spl_subsample_draw(uint64_t key, uint64_t salt)
{
    uint64_t z = key ^ salt;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    z ^= z >> 31;
    return (uint32_t)(z >> 32);
}

SPL_HD bool spl_subsample_keep(uint64_t name_key, int64_t pos, uint32_t flag, uint32_t n_ops, uint64_t salt, uint64_t threshold)
{
    const uint64_t k = name_key ? name_key : spl_subsample_nameless_key(pos, flag, n_ops);
    return (uint64_t)spl_subsample_draw(k, salt) < threshold;
}

#endif // SPL_SUBSAMPLE_RULE_H
