// exoncount_rule_asan.cpp -- the exon-bin rule of spl_exoncount_rule.h over the cases of tests/exoncases.py, a read's ops, the two
// bin maps, the bins' genes and the hit list each in a heap block of exactly its size, for a build with
// -fsanitize=address,undefined (the test compiles and runs it): a load or a store beyond any of them is a heap-buffer-overflow
// there, an int32 sum that should have been int64 a UBSan report.
// Input, a case a line: "flag pos shift stranded cap|ops ...|a starts ...|a codes ...|b starts ...|b codes ...|bin genes ...".
// Output, a line a case: the verdict (0 counted, -1 no feature, -2 ambiguous, -3 not counted), the number of hits, and the first
// `cap` of them.  Host code only; never loaded into Python.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../spliser_amd/csrc/spl_exoncount_rule.h"

static std::vector<long long> numbers(const std::string &s)
{
    std::vector<long long> out;
    const char *p = s.c_str();
    char *end = nullptr;
    for (;;) {
        const long long v = strtoll(p, &end, 10);
        if (end == p) break;
        out.push_back(v);
        p = end;
    }
    return out;
}

template <class T> static T *exact_block(const std::vector<long long> &v)
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
        std::string parts[7];
        int k = 0;
        for (char ch : line) {
            if (ch == '|') { if (++k > 6) break; }
            else parts[k] += ch;
        }
        if (k != 6) { fprintf(stderr, "not a case: %s\n", line.c_str()); return 2; }
        const std::vector<long long> head = numbers(parts[0]), ops = numbers(parts[1]), as = numbers(parts[2]), ac = numbers(parts[3]), bs = numbers(parts[4]), bc = numbers(parts[5]),
                                     genes = numbers(parts[6]);
        if (head.size() != 5 || head[4] < 0 || as.size() != ac.size() || bs.size() != bc.size()) { fprintf(stderr, "not a case: %s\n", line.c_str()); return 2; }
        uint32_t *d_ops = exact_block<uint32_t>(ops);
        int32_t *a_start = exact_block<int32_t>(as), *b_start = exact_block<int32_t>(bs);
        uint32_t *a_code = exact_block<uint32_t>(ac), *b_code = exact_block<uint32_t>(bc), *bin_gene = exact_block<uint32_t>(genes);
        const int64_t cap = (int64_t)head[4];
        int64_t *bins = (int64_t *)malloc(cap ? (size_t)cap * sizeof(int64_t) : 1), n_hits = 0;
        const uint32_t v = spl_exon_read_result((uint32_t)head[0], (int64_t)(int32_t)head[1], d_ops, (uint32_t)ops.size(), (int64_t)(int32_t)head[2], (int)head[3],
                                                spl_gene_map_flat{(int64_t)as.size(), a_start, a_code}, spl_gene_map_flat{(int64_t)bs.size(), b_start, b_code}, bin_gene, bins, cap, &n_hits);
        printf("%lld %lld", -(long long)v, (long long)n_hits);
        for (int64_t j = 0; j < n_hits && j < cap; ++j) printf(" %lld", (long long)bins[j]);
        printf("\n");
        free(d_ops); free(a_start); free(b_start); free(a_code); free(b_code); free(bin_gene); free(bins);
    }
    return 0;
}
