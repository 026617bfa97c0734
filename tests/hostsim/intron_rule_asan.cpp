// intron_rule_asan.cpp -- the intron rule of spl_intron_rule.h over cases of tests/introncases.py, the boundaries and the pieces each
// in a heap block of exactly its size, for a build with -fsanitize=address,undefined (the test compiles and runs it): a load
// beyond any of them is a heap-buffer-overflow there, an int32 sum that should have been int64 a UBSan report.
// Input, a case a line: "trim length|bound pos ...|bound depth ...|piece start ...|piece end ...".
// Output, a line a case: "flaw <piece> <why>" / "bound <entry>" when the checks refuse it, else L, covered, depth_n, depth_sum.
// Host code only; never loaded into Python.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../spliser_amd/csrc/spl_intron_rule.h"

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
        std::string parts[5];
        int k = 0;
        for (char ch : line) {
            if (ch == '|') { if (++k > 4) break; }
            else parts[k] += ch;
        }
        const std::vector<long long> head = numbers(parts[0]), bp = numbers(parts[1]), bd = numbers(parts[2]), ps = numbers(parts[3]), pe = numbers(parts[4]);
        if (k != 4 || head.size() != 2 || bp.size() != bd.size() || ps.size() != pe.size()) { fprintf(stderr, "not a case: %s\n", line.c_str()); return 2; }
        int32_t *bound_pos = exact_block<int32_t>(bp), *piece_start = exact_block<int32_t>(ps), *piece_end = exact_block<int32_t>(pe);
        uint32_t *bound_depth = exact_block<uint32_t>(bd);
        int why = 0;
        const int64_t flaw = spl_intron_piece_flaw(piece_start, piece_end, 0, (int64_t)ps.size(), (int64_t)head[1], &why);
        const int64_t bound = spl_intron_bound_flaw((int64_t)bp.size(), bound_pos);
        if (flaw >= 0) printf("flaw %lld %d\n", (long long)flaw, why);
        else if (bound >= 0) printf("bound %lld\n", (long long)bound);
        else {
            int64_t out4[4];
            spl_intron_depth_of((int64_t)bp.size(), bound_pos, bound_depth, (int64_t)ps.size(), piece_start, piece_end, (int)head[0], out4);
            printf("%lld %lld %lld %lld\n", (long long)out4[0], (long long)out4[1], (long long)out4[2], (long long)out4[3]);
        }
        free(bound_pos); free(bound_depth); free(piece_start); free(piece_end);
    }
    return 0;
}
