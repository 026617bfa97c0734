// spl_sort_wave.h -- the bodies of the stable radix sort's kernels (spl_sort.hip), written against spl_wave.h's primitives: the
// same source runs as one wave per workgroup on the device and under tests/hostsim/wave_emul.h on a CPU
// (tests/test_sort_wave_host.py holds it against numpy's stable sort).
//
// What is sorted: 64-bit keys (reference id << 32 | POS of a placed record, spl_capi.cpp) with the record's index as payload,
// least significant digit first, 8 bits a pass, over only the digits that can differ (pass_shifts).  A pass is three launches:
//   1. part_histogram  the keys are cut into PARTS of whole tiles, a part per wave; its counts per digit, in LDS, go to
//                      hist[digit * parts + part]
//   2. digit_scan      a wave per digit: the exclusive sums of its row of hist, and the digit's total
//   3. part_scatter    a part per wave again: where each digit's keys of this part begin (the totals of the smaller digits, the
//                      row's entry), then tile by tile, 64 keys a round in file order: a key's place is its digit's running offset
//                      plus the number of lanes in front of it that hold the same digit -- counted by ballots, so the order of
//                      equal digits is the order of the input, which is what makes the pass STABLE (and an LSD sort correct)
// Nothing here depends on the order in which atomics arrive: the only atomic is the histogram's count.
#ifndef SPL_SORT_WAVE_H
#define SPL_SORT_WAVE_H
#include <stddef.h>
#include <stdint.h>

#include "spl_wave.h"

namespace splsort {

constexpr uint32_t RADIX_BITS = 8u, RADIX = 1u << RADIX_BITS;
constexpr uint32_t KEYS_PER_LANE = 16u, TILE = 64u * KEYS_PER_LANE; // (a tile: 16 rounds of 64 keys, lane l the keys l, l + 64, ...: coalesced)
constexpr uint32_t MAX_PARTS = 2048u;                              // (waves a launch: eight a CU; a part is as many tiles as that takes)
constexpr uint32_t MAX_PASSES = 8u;

// How n keys are cut: n_tiles tiles, parts of tiles_per_part consecutive tiles each (the last one may have fewer; none is empty).
struct Plan { uint64_t n_tiles, tiles_per_part; uint32_t parts; };
static inline Plan plan_for(uint64_t n, uint32_t max_parts)
{
    Plan p;
    p.n_tiles = (n + TILE - 1u) / TILE;
    if (max_parts < 1u) max_parts = 1u;
    const uint64_t want = p.n_tiles < max_parts ? p.n_tiles : max_parts;
    p.tiles_per_part = want ? (p.n_tiles + want - 1u) / want : 1u;
    p.parts = (uint32_t)(want ? (p.n_tiles + p.tiles_per_part - 1u) / p.tiles_per_part : 0u);
    return p;
}

// The passes of a key whose low word has low_bits bits that can differ and whose high word has high_bits: the shifts of the
// digits, least significant first.  (A five-chromosome genome of 30 Mb: 25 and 3 bits, 4 + 1 passes instead of 8.)
static inline uint32_t pass_shifts2(uint32_t low_bits, uint32_t high_bits, uint32_t *shifts)
{
    uint32_t k = 0;
    if (low_bits > 32u) low_bits = 32u;
    if (high_bits > 32u) high_bits = 32u;
    for (uint32_t s = 0; s < low_bits; s += RADIX_BITS) shifts[k++] = s;
    for (uint32_t s = 0; s < high_bits; s += RADIX_BITS) shifts[k++] = 32u + s;
    return k;
}
// ... of a key of key_bits bits (1..64)
static inline uint32_t pass_shifts(uint32_t key_bits, uint32_t *shifts) { return pass_shifts2(key_bits < 32u ? key_bits : 32u, key_bits > 32u ? key_bits - 32u : 0u, shifts); }

WV_DEV uint32_t digit_of(uint64_t key, uint32_t shift) { return (uint32_t)(key >> shift) & (RADIX - 1u); }

// Launch 1.  h: RADIX words of shared memory.
WV_DEV void part_histogram(const uint64_t *keys, uint64_t n, uint32_t shift, uint64_t tile0, uint64_t tile1, WV_SHARED_PTR(uint32_t) h, uint32_t *hist, uint32_t parts, uint32_t part)
{
    const uint32_t lane = wv::lane();
    for (uint32_t j = 0; j < RADIX / 64u; ++j) h[lane + 64u * j] = 0u;
    wv::sync();
    for (uint64_t t = tile0; t < tile1; ++t) {
        const uint64_t base = t * TILE + lane;
#pragma unroll
        for (uint32_t r = 0; r < KEYS_PER_LANE; ++r) {
            const uint64_t idx = base + 64u * r;
            if (idx < n) wv::lds_add(&h[digit_of(keys[idx], shift)], 1u);
        }
    }
    wv::sync();
    for (uint32_t j = 0; j < RADIX / 64u; ++j) hist[(size_t)(lane + 64u * j) * parts + part] = h[lane + 64u * j];
}

// Launch 2, and the scans of the gather (spl_sort.hip): row[0 .. count) becomes its exclusive prefix sums, *total_out their sum.
WV_DEV void digit_scan(uint32_t *row, uint32_t count, uint32_t *total_out)
{
    const uint32_t lane = wv::lane();
    uint32_t carry = 0u;
    for (uint32_t i = 0; i < count; i += 64u) {
        const uint32_t idx = i + lane;
        const uint32_t v = idx < count ? row[idx] : 0u;
        const uint32_t inc = wv::scan_add(v);
        if (idx < count) row[idx] = carry + inc - v;
        carry += wv::shfl(inc, 63u);
    }
    if (lane == 0u) *total_out = carry;
}

// Launch 3.  offs: RADIX words of shared memory.  perm_in = null: the keys are in file order, a key's payload is its index.
WV_DEV void part_scatter(const uint64_t *keys_in, const uint32_t *perm_in, uint64_t n, uint32_t shift, uint64_t tile0, uint64_t tile1, WV_SHARED_PTR(uint32_t) offs,
                         const uint32_t *hist, const uint32_t *totals, uint32_t parts, uint32_t part, uint64_t *keys_out, uint32_t *perm_out)
{
    const uint32_t lane = wv::lane();
    { // where this part's keys of each digit begin: lane l has the digits 4 l .. 4 l + 3
        uint32_t t4[RADIX / 64u], sum = 0u;
        for (uint32_t j = 0; j < RADIX / 64u; ++j) { t4[j] = totals[lane * (RADIX / 64u) + j]; sum += t4[j]; }
        uint32_t run = wv::scan_add(sum) - sum;
        for (uint32_t j = 0; j < RADIX / 64u; ++j) {
            const uint32_t d = lane * (RADIX / 64u) + j;
            offs[d] = run + hist[(size_t)d * parts + part];
            run += t4[j];
        }
    }
    wv::sync();
    const uint64_t in_front = lane ? (~0ull >> (64u - lane)) : 0ull; // the lanes below this one
    for (uint64_t t = tile0; t < tile1; ++t) {
        const uint64_t base = t * TILE + lane;
        uint64_t key[KEYS_PER_LANE];
        uint32_t val[KEYS_PER_LANE];
#pragma unroll
        for (uint32_t r = 0; r < KEYS_PER_LANE; ++r) { // (all of a tile's loads first: sixteen in flight a lane)
            const uint64_t idx = base + 64u * r;
            const bool have = idx < n;
            key[r] = have ? keys_in[idx] : 0ull;
            val[r] = have ? (perm_in ? perm_in[idx] : (uint32_t)idx) : 0u;
        }
#pragma unroll
        for (uint32_t r = 0; r < KEYS_PER_LANE; ++r) {
            const bool have = base + 64u * r < n;
            const uint32_t d = digit_of(key[r], shift);
            uint64_t same = wv::ballot(have); // the lanes that hold a key of the same digit
#pragma unroll
            for (uint32_t b = 0; b < RADIX_BITS; ++b) {
                const bool bit = (d >> b) & 1u;
                const uint64_t with = wv::ballot(have && bit);
                same &= bit ? with : ~with;
            }
            const uint32_t rank = wv::popc64(same & in_front), count = wv::popc64(same);
            const uint32_t at = have ? offs[d] : 0u;
            wv::sync();
            if (have && rank == 0u) offs[d] = at + count; // (the digit's first lane of the round: one writer a word)
            wv::sync();
            const uint64_t dst = (uint64_t)at + rank;
            if (have && dst < n) { keys_out[dst] = key[r]; perm_out[dst] = val[r]; } // (dst < n always: said for the memory's sake)
        }
    }
}

// ---- the scan of the gather: inclusive prefix sums of n 32-bit counts in place, device-wide, in the same parts -------------------
// 1. a part's sum
WV_DEV void part_sum(const uint32_t *v, uint64_t n, uint64_t tile0, uint64_t tile1, uint32_t *partial, uint32_t part)
{
    const uint32_t lane = wv::lane();
    uint32_t s = 0u;
    for (uint64_t t = tile0; t < tile1; ++t) {
        const uint64_t base = t * TILE + lane;
#pragma unroll
        for (uint32_t r = 0; r < KEYS_PER_LANE; ++r) { const uint64_t idx = base + 64u * r; if (idx < n) s += v[idx]; }
    }
    const uint32_t inc = wv::scan_add(s);
    if (lane == 63u) partial[part] = inc;
}
// 2. digit_scan over the parts' sums.  3. a part's inclusive sums, on top of what lies in front of the part
WV_DEV void part_rescan(uint32_t *v, uint64_t n, uint64_t tile0, uint64_t tile1, const uint32_t *partial, uint32_t part)
{
    const uint32_t lane = wv::lane();
    uint32_t carry = partial[part];
    for (uint64_t t = tile0; t < tile1; ++t) {
        const uint64_t base = t * TILE + lane;
        for (uint32_t r = 0; r < KEYS_PER_LANE; ++r) {
            const uint64_t idx = base + 64u * r;
            const uint32_t x = idx < n ? v[idx] : 0u;
            const uint32_t inc = wv::scan_add(x);
            if (idx < n) v[idx] = carry + inc;
            carry += wv::shfl(inc, 63u);
        }
    }
}

} // namespace splsort
#endif
