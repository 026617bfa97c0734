// genecount_rule_asan.cpp -- the gene-count rule of spl_genecount_rule.h over the corner cases of tests/genecases.py, a read's ops
// and the two gene maps each in a heap block of exactly its size, for a build with -fsanitize=address,undefined (the test compiles
// and runs it): a load beyond either is a heap-buffer-overflow there, an int32 sum that should have been int64 a UBSan report.
// Input, a case a line: "flag pos shift stranded|ops ...|a starts ...|a codes ...|b starts ...|b codes ...".  Output: the read's
// result, a line a case: the gene's index, -1 no feature, -2 ambiguous, -3 not counted.  Host code only; never loaded into Python.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../spliser_amd/csrc/spl_genecount_rule.h"

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
        std::string parts[6];
        int k = 0;
        for (char ch : line) {
            if (ch == '|') { if (++k > 5) break; }
            else parts[k] += ch;
        }
        if (k != 5) { fprintf(stderr, "not a case: %s\n", line.c_str()); return 2; }
        const std::vector<long long> head = numbers(parts[0]), ops = numbers(parts[1]), as = numbers(parts[2]), ac = numbers(parts[3]), bs = numbers(parts[4]), bc = numbers(parts[5]);
        if (head.size() != 4 || as.size() != ac.size() || bs.size() != bc.size()) { fprintf(stderr, "not a case: %s\n", line.c_str()); return 2; }
        uint32_t *d_ops = exact_block<uint32_t>(ops);
        int32_t *a_start = exact_block<int32_t>(as), *b_start = exact_block<int32_t>(bs);
        uint32_t *a_code = exact_block<uint32_t>(ac), *b_code = exact_block<uint32_t>(bc);
        const uint32_t r = spl_gene_read_result((uint32_t)head[0], (int64_t)(int32_t)head[1], d_ops, (uint32_t)ops.size(), (int64_t)(int32_t)head[2], (int)head[3],
                                                spl_gene_map_flat{(int64_t)as.size(), a_start, a_code}, spl_gene_map_flat{(int64_t)bs.size(), b_start, b_code});
        printf("%lld\n", r == SPL_GENE_NO_FEATURE ? -1ll : r == SPL_GENE_AMBIGUOUS ? -2ll : r == SPL_GENE_NOT_COUNTED ? -3ll : (long long)r);
        free(d_ops); free(a_start); free(b_start); free(a_code); free(b_code);
    }
    return 0;
}
