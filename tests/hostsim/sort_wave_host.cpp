// Test-only host build of spliser_amd/csrc/spl_sort_wave.h (the bodies of spl_sort.hip's kernels) under the wave emulator: a wave of
// 64 fibers per part, the launches of a pass one after the other as the device's stream runs them; tests/test_sort_wave_host.py
// holds the result against numpy's stable sort.  Every function returns 0, or < 0 when a wave broke a rule of the emulator.
#include <vector>

#define WAVE_EMUL_IMPLEMENTATION
#include "wave_emul.h"
// spl_wave.h's lds_add on the host (the emulator has lds_max and lds_or): between two rendezvous the lanes run one after the other,
// so a plain read-modify-write is the atomic
namespace wv {
inline uint32_t lds_add(uint32_t *p, uint32_t v) { const uint32_t o = *p; *p = o + v; return o; }
} // namespace wv
#include "../../spliser_amd/csrc/spl_sort_wave.h"

namespace {
// One pass as the device runs it: histogram, scan, scatter.  hist_out (or null): parts x 256 counts, [digit * parts + part], as
// launch 1 left them.
int one_pass(const uint64_t *keys_in, const uint32_t *perm_in, uint64_t n, uint32_t shift, uint32_t max_parts, uint64_t *keys_out, uint32_t *perm_out, uint32_t *hist_out)
{
    const splsort::Plan pl = splsort::plan_for(n, max_parts);
    std::vector<uint32_t> hist((size_t)splsort::RADIX * std::max<uint32_t>(pl.parts, 1u), 0u), totals(splsort::RADIX, 0u), lds(splsort::RADIX, 0u);
    for (uint32_t p = 0; p < pl.parts; ++p) {
        const uint64_t t0 = (uint64_t)p * pl.tiles_per_part, t1 = std::min(pl.n_tiles, t0 + pl.tiles_per_part);
        if (!wv::run_wave([&]() { splsort::part_histogram(keys_in, n, shift, t0, t1, lds.data(), hist.data(), pl.parts, p); })) return -1;
    }
    if (hist_out) for (size_t k = 0; k < (size_t)splsort::RADIX * pl.parts; ++k) hist_out[k] = hist[k];
    for (uint32_t d = 0; d < splsort::RADIX; ++d)
        if (!wv::run_wave([&]() { splsort::digit_scan(hist.data() + (size_t)d * pl.parts, pl.parts, &totals[d]); })) return -2;
    for (uint32_t p = 0; p < pl.parts; ++p) {
        const uint64_t t0 = (uint64_t)p * pl.tiles_per_part, t1 = std::min(pl.n_tiles, t0 + pl.tiles_per_part);
        if (!wv::run_wave([&]() { splsort::part_scatter(keys_in, perm_in, n, shift, t0, t1, lds.data(), hist.data(), totals.data(), pl.parts, p, keys_out, perm_out); })) return -3;
    }
    return 0;
}
} // namespace

extern "C" uint32_t sort_wave_tile() { return splsort::TILE; }
extern "C" uint32_t sort_wave_parts(uint64_t n, uint32_t max_parts) { return splsort::plan_for(n, max_parts).parts; }
extern "C" uint32_t sort_wave_passes(uint32_t key_bits, uint32_t *shifts8) { return splsort::pass_shifts(key_bits, shifts8); }

extern "C" int sort_wave_pass(const uint64_t *keys_in, const uint32_t *perm_in, uint64_t n, uint32_t shift, uint32_t max_parts, uint64_t *keys_out, uint32_t *perm_out, uint32_t *hist_out)
{
    return one_pass(keys_in, perm_in, n, shift, max_parts, keys_out, perm_out, hist_out);
}

// The whole sort, driven as spl_capi.cpp drives the device's: the passes of key_bits, two buffers taking turns.
extern "C" int sort_wave_keys(const uint64_t *keys, uint64_t n, uint32_t key_bits, uint32_t max_parts, uint32_t *perm_out)
{
    uint32_t shifts[splsort::MAX_PASSES];
    const uint32_t n_pass = splsort::pass_shifts(key_bits, shifts);
    std::vector<uint64_t> ka(keys, keys + n), kb(n);
    std::vector<uint32_t> pa(n), pb(n);
    for (uint32_t k = 0; k < n_pass; ++k) {
        const int rc = one_pass(ka.data(), k ? pa.data() : nullptr, n, shifts[k], max_parts, kb.data(), pb.data(), nullptr);
        if (rc) return rc;
        ka.swap(kb);
        pa.swap(pb);
    }
    for (uint64_t i = 0; i < n; ++i) perm_out[i] = n_pass ? pa[i] : (uint32_t)i;
    return 0;
}

// The device-wide scan of the gather: v[0 .. n) becomes its inclusive prefix sums.
extern "C" int sort_wave_scan(uint32_t *v, uint64_t n, uint32_t max_parts)
{
    const splsort::Plan pl = splsort::plan_for(n, max_parts);
    std::vector<uint32_t> partial(std::max<uint32_t>(pl.parts, 1u) + 1u, 0u);
    for (uint32_t p = 0; p < pl.parts; ++p) {
        const uint64_t t0 = (uint64_t)p * pl.tiles_per_part, t1 = std::min(pl.n_tiles, t0 + pl.tiles_per_part);
        if (!wv::run_wave([&]() { splsort::part_sum(v, n, t0, t1, partial.data(), p); })) return -1;
    }
    if (!wv::run_wave([&]() { splsort::digit_scan(partial.data(), pl.parts, &partial[pl.parts]); })) return -2;
    for (uint32_t p = 0; p < pl.parts; ++p) {
        const uint64_t t0 = (uint64_t)p * pl.tiles_per_part, t1 = std::min(pl.n_tiles, t0 + pl.tiles_per_part);
        if (!wv::run_wave([&]() { splsort::part_rescan(v, n, t0, t1, partial.data(), p); })) return -3;
    }
    return 0;
}
