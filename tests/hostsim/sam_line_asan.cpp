// sam_line_asan.cpp -- the rule of spl_sam_line.h over lines that each lie in a heap block of exactly their size, for a build with
// -fsanitize=address,undefined (tests/test_samcases_host.py compiles and runs it): a read at or beyond a line's end, or beyond
// the names' table, is a heap-buffer-overflow there.  Argument: a file -- u32 min_mapq, require, exclude; u32 n_names, then per
// name u32 length and bytes; u32 n_lines, then per line u32 length and bytes.  Output: one line per input line, "reason" or
// "0 flag tid pos mapq next_tid verdict placed xs end n_ops op op ...".  Host code only; never loaded into Python.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../spliser_amd/csrc/spl_sam_line.h"

static bool get32(FILE *fh, uint32_t *v) { return fread(v, 4, 1, fh) == 1; }

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    FILE *fh = fopen(argv[1], "rb");
    if (!fh) return 2;
    spl_bam_filter filter;
    uint32_t n_names = 0, n_lines = 0;
    if (!get32(fh, &filter.min_mapq) || !get32(fh, &filter.require_flags) || !get32(fh, &filter.exclude_flags) || !get32(fh, &n_names)) return 2;
    // the table as spl_sam_open makes it, every array exactly its size
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
    if (!get32(fh, &n_lines)) return 2;
    int32_t hint = -1;
    for (uint32_t k = 0; k < n_lines; ++k) {
        uint32_t len = 0;
        if (!get32(fh, &len)) return 2;
        uint8_t *block = (uint8_t *)malloc(len ? len : 1);
        uint8_t *line = len ? block : block + 1; // (the empty line lies at its block's end: any read of it is beyond)
        if (len && fread(line, 1, len, fh) != len) return 2;
        spl_sam_line ln;
        spl_sam_parse_line(line, line + len, names, hint, filter, true, &ln);
        if (ln.reason != SPL_SAM_OK) printf("%u\n", ln.reason);
        else {
            hint = ln.tid;
            printf("0 %u %d %d %u %d %d %u %u %lld %u", ln.flag, ln.tid, ln.pos, ln.mapq, ln.next_tid, ln.verdict, (unsigned)ln.placed, (unsigned)ln.xs, (long long)ln.end, ln.n_ops);
            uint32_t *ops = (uint32_t *)malloc(ln.n_ops ? 4 * (size_t)ln.n_ops : 1), n = 0;
            int64_t ref_len = 0;
            bool has_n = false;
            if (ln.placed && !spl_sam_cigar(line + ln.cigar_at, line + ln.cigar_at + ln.cigar_len, ops, &n, &ref_len, &has_n)) return 3;
            if (n != ln.n_ops) return 3;
            for (uint32_t j = 0; j < n; ++j) printf(" %u", ops[j]);
            printf("\n");
            free(ops);
        }
        free(block);
    }
    free(slots); free(blob); free(name_off);
    fclose(fh);
    return 0;
}
