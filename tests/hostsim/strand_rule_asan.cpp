// strand_rule_asan.cpp -- the strandedness rule of spl_strand_rule.h over the edge cases of tests/test_strandedness_host.py, a read's
// ops and the cover map each in a heap block of exactly its size, for a build with -fsanitize=address,undefined (the test compiles
// and runs it): a load beyond either is a heap-buffer-overflow there, an int32 sum that should have been int64 a UBSan report.
// Input, a case a line: "flag pos xs|ops ...|starts ...|codes ...".  Output: the 14 counters of that one read, a line a case.
// Host code only; never loaded into Python.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../spliser_amd/csrc/spl_strand_rule.h"

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
    char line[1 << 16];
    while (fgets(line, sizeof line, stdin)) {
        std::string parts[4];
        int k = 0;
        for (const char *p = line; *p && *p != '\n'; ++p) {
            if (*p == '|') { if (++k > 3) break; }
            else parts[k] += *p;
        }
        if (k != 3) { fprintf(stderr, "not a case: %s", line); return 2; }
        const std::vector<long long> head = numbers(parts[0]), ops = numbers(parts[1]), starts = numbers(parts[2]), codes = numbers(parts[3]);
        if (head.size() != 3 || starts.size() != codes.size()) { fprintf(stderr, "not a case: %s", line); return 2; }
        uint32_t *d_ops = exact_block<uint32_t>(ops);
        int32_t *d_start = exact_block<int32_t>(starts);
        uint8_t *d_code = exact_block<uint8_t>(codes);
        const uint32_t bits = spl_strand_read_bits((uint32_t)head[0], (int64_t)(int32_t)head[1], d_ops, (uint32_t)ops.size(), (uint8_t)head[2], (int64_t)starts.size(), d_start, d_code);
        for (int c = 0; c < SPL_STRAND_COUNTERS; ++c) printf("%s%u", c ? " " : "", (bits >> c) & 1u);
        printf("\n");
        free(d_ops); free(d_start); free(d_code);
    }
    return 0;
}
