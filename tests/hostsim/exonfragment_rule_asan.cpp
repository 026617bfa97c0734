// exonfragment_rule_asan.cpp -- the fragment rule of spl_exonfragment_rule.h over one segment's arrays, its mate table, the two bin
// maps, the bins' genes and the list of merged bins each in a heap block of exactly its size, for a build with
// -fsanitize=address,undefined (the test compiles and runs it): a load or a store beyond any of them is a heap-buffer-overflow
// there, an int32 sum that should have been int64 a UBSan report.  The mate table is taken as it comes: indexes beyond the segment
// and a read that is its own mate are the test's to send.
// Input, a case a line: "shift stranded cap|pos ...|flag ...|cig_off ...|cigar ...|mate ...|a starts ...|a codes ...|b starts ...|
// b codes ...|bin genes ...".
// Output, three lines a case: every read's verdict (0 counted, -1 no feature, -2 ambiguous, -3 not counted, -4 silent), every
// read's number of distinct bins, and the counted leaders' merged bins as far as cap reaches.  Host code only; never loaded into Python.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../spliser_amd/csrc/spl_exonfragment_rule.h"

static std::vector<unsigned long long> numbers(const std::string &s)
{
    std::vector<unsigned long long> out;
    const char *p = s.c_str();
    char *end = nullptr;
    for (;;) {
        const unsigned long long v = strtoull(p, &end, 10);
        if (end == p) break;
        out.push_back(v);
        p = end;
    }
    return out;
}

template <class T> static T *exact_block(const std::vector<unsigned long long> &v)
{
    T *block = (T *)malloc(v.empty() ? 1 : v.size() * sizeof(T));
    for (size_t i = 0; i < v.size(); ++i) block[i] = (T)v[i];
    return block;
}

int main()
{
    std::string text;
    char buf[1 << 16];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, stdin)) > 0) text.append(buf, got);
    size_t at = 0;
    while (at < text.size()) {
        size_t nl = text.find('\n', at);
        if (nl == std::string::npos) nl = text.size();
        const std::string line = text.substr(at, nl - at);
        at = nl + 1;
        if (line.empty()) continue;
        std::string parts[11];
        int k = 0;
        for (char ch : line) {
            if (ch == '|') { if (++k > 10) break; }
            else parts[k] += ch;
        }
        if (k != 10) { fprintf(stderr, "not a case: %s\n", line.c_str()); return 2; }
        const std::vector<unsigned long long> head = numbers(parts[0]), pos = numbers(parts[1]), flag = numbers(parts[2]), off = numbers(parts[3]), ops = numbers(parts[4]),
                                              mt = numbers(parts[5]), as = numbers(parts[6]), ac = numbers(parts[7]), bs = numbers(parts[8]), bc = numbers(parts[9]),
                                              genes = numbers(parts[10]);
        const int64_t n = (int64_t)pos.size();
        if (head.size() != 3 || flag.size() != pos.size() || off.size() != pos.size() + 1 || mt.size() != pos.size() || as.size() != ac.size() || bs.size() != bc.size()) {
            fprintf(stderr, "not a case: %s\n", line.c_str());
            return 2;
        }
        int32_t *d_pos = exact_block<int32_t>(pos), *a_start = exact_block<int32_t>(as), *b_start = exact_block<int32_t>(bs);
        uint16_t *d_flag = exact_block<uint16_t>(flag);
        uint32_t *d_off = exact_block<uint32_t>(off), *d_ops = exact_block<uint32_t>(ops), *d_mate = exact_block<uint32_t>(mt);
        uint32_t *a_code = exact_block<uint32_t>(ac), *b_code = exact_block<uint32_t>(bc), *bin_gene = exact_block<uint32_t>(genes);
        const int64_t shift = (int64_t)(int32_t)head[0], cap = (int64_t)head[2];
        const int stranded = (int)head[1];
        int64_t *bins = (int64_t *)malloc(cap ? (size_t)cap * sizeof(int64_t) : 1);
        int64_t *verdict = (int64_t *)malloc(n ? (size_t)n * sizeof(int64_t) : 1), *n_hits = (int64_t *)malloc(n ? (size_t)n * sizeof(int64_t) : 1);
        const spl_mate_reads reads{d_pos, d_flag, d_off, d_ops, (int64_t)ops.size()};
        const spl_gene_map_flat map_a{(int64_t)as.size(), a_start, a_code}, map_b{(int64_t)bs.size(), b_start, b_code};
        int64_t used = 0;
        for (int64_t r = 0; r < n; ++r) {
            verdict[r] = -(int64_t)spl_exon_fragment_result(reads, n, r, d_mate, shift, stranded, map_a, map_b, bin_gene, bins + used, cap - used, &n_hits[r]);
            used = used + n_hits[r] < cap ? used + n_hits[r] : cap;
        }
        for (int64_t r = 0; r < n; ++r) printf("%s%lld", r ? " " : "", (long long)verdict[r]);
        printf("\n");
        for (int64_t r = 0; r < n; ++r) printf("%s%lld", r ? " " : "", (long long)n_hits[r]);
        printf("\n");
        for (int64_t j = 0; j < used; ++j) printf("%s%lld", j ? " " : "", (long long)bins[j]);
        printf("\n");
        free(d_pos); free(a_start); free(b_start); free(d_flag); free(d_off); free(d_ops); free(d_mate); free(a_code); free(b_code); free(bin_gene); free(bins); free(verdict); free(n_hits);
    }
    return 0;
}
