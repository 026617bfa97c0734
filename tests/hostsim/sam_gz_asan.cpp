// sam_gz_asan.cpp -- the host's inflate-and-carry parser of compressed SAM text (csrc/spl_sam_zhost.h) with the rule of
// spl_sam_line.h behind it, for a build with -fsanitize=address,undefined (tests/test_samz_host.py compiles and runs it): the
// compressed file lies in a heap block of exactly its size, the lines are read where the walk's buffer holds them.
// Arguments: the compressed file; a file -- u32 min_mapq, require, exclude; u32 n_names, then per name u32 length and bytes --;
// the bytes of header in front of the first line; the longest line taken (SPL_SAM_WINDOW_BYTES).  Output: per line
// "0 flag tid pos n_ops", or "declined <line> <reason>" and nothing more; then "end <status> <largest buffer>".
// Host code only; never loaded into Python.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../spliser_amd/csrc/spl_sam_line.h"
#include "../../spliser_amd/csrc/spl_sam_zhost.h"

static bool get32(FILE *fh, uint32_t *v) { return fread(v, 4, 1, fh) == 1; }

int main(int argc, char **argv)
{
    if (argc != 5) return 2;
    FILE *fh = fopen(argv[1], "rb");
    if (!fh) return 2;
    fseek(fh, 0, SEEK_END);
    const size_t fsize = (size_t)ftell(fh);
    fseek(fh, 0, SEEK_SET);
    uint8_t *image = (uint8_t *)malloc(fsize ? fsize : 1);
    if (fsize && fread(image, 1, fsize, fh) != fsize) return 2;
    fclose(fh);
    fh = fopen(argv[2], "rb");
    if (!fh) return 2;
    spl_bam_filter filter;
    uint32_t n_names = 0;
    if (!get32(fh, &filter.min_mapq) || !get32(fh, &filter.require_flags) || !get32(fh, &filter.exclude_flags) || !get32(fh, &n_names)) return 2;
    std::vector<uint8_t> all;
    uint32_t *name_off = (uint32_t *)malloc(4 * ((size_t)n_names + 1));
    name_off[0] = 0;
    for (uint32_t k = 0; k < n_names; ++k) {
        uint32_t len = 0;
        if (!get32(fh, &len)) return 2;
        all.resize(all.size() + len);
        if (len && fread(all.data() + all.size() - len, 1, len, fh) != len) return 2;
        name_off[k + 1] = (uint32_t)all.size();
    }
    fclose(fh);
    uint8_t *blob = (uint8_t *)malloc(all.size() ? all.size() : 1);
    if (!all.empty()) memcpy(blob, all.data(), all.size());
    uint32_t n_slots = 4;
    while (n_slots < 2 * n_names) n_slots *= 2;
    uint32_t *slots = (uint32_t *)calloc(n_slots, 4);
    const spl_sam_names names = {slots, name_off, blob, n_slots, (int32_t)n_names};
    for (uint32_t k = 0; k < n_names; ++k) {
        uint32_t s = spl_sam_hash(blob + name_off[k], blob + name_off[k + 1]) & (n_slots - 1u);
        while (slots[s]) s = (s + 1u) & (n_slots - 1u);
        slots[s] = k + 1u;
    }
    const uint64_t skip = strtoull(argv[3], nullptr, 10);
    const size_t max_line = (size_t)strtoull(argv[4], nullptr, 10);
    int status = 0;
    size_t largest = 0;
    {
        splsamz::Inflater z;
        splsamz::Lines lines;
        if (!z.begin(image, fsize)) return 3;
        uint64_t line_no = 0;
        int32_t hint = -1;
        status = lines.walk(z, skip, max_line, [&](const uint8_t *p, const uint8_t *stop, bool nl) -> bool {
            ++line_no;
            if (lines.buf.size() > largest) largest = lines.buf.size();
            if ((size_t)(stop - p) + (nl ? 1u : 0u) > max_line) { printf("declined %llu %u\n", (unsigned long long)line_no, SPL_SAM_LONG_LINE); return false; }
            // (the rule may read its line's bytes and not one more: a copy of exactly the line's size says so)
            const size_t len = (size_t)(stop - p);
            uint8_t *block = (uint8_t *)malloc(len ? len : 1);
            uint8_t *line = len ? block : block + 1;
            if (len) memcpy(line, p, len);
            spl_sam_line ln;
            spl_sam_parse_line(line, line + len, names, hint, filter, true, &ln);
            free(block);
            if (ln.reason != SPL_SAM_OK) { printf("declined %llu %u\n", (unsigned long long)line_no, ln.reason); return false; }
            hint = ln.tid;
            printf("0 %u %d %d %u\n", ln.flag, ln.tid, ln.pos, ln.n_ops);
            return true;
        });
        if (lines.buf.size() > largest) largest = lines.buf.size();
    }
    printf("end %d %zu\n", status, largest);
    free(slots); free(blob); free(name_off); free(image);
    return 0;
}
