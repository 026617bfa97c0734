// subsample_rule_asan.cpp -- the rule of spl_subsample_rule.h over the read sets of tests/subsamplecases.py, every array in a heap
// block of exactly its size, for a build with -fsanitize=address,undefined (the test compiles and runs it): a load beyond an array
// is a heap-buffer-overflow there, a shift or a product the rule did not mean a UBSan report.  Input, a case a line:
//   "seed threshold|name keys ...|pos ...|flag ...|cig_off ..."
// Output, a line a case: 1 or 0 per read, kept or not.  Host code only; never loaded into Python.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "../../spliser_amd/csrc/spl_subsample_rule.h"

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
        std::string parts[5];
        int k = 0;
        for (char ch : line) {
            if (ch == '|') { if (++k > 4) break; }
            else parts[k] += ch;
        }
        if (k != 4) { fprintf(stderr, "not a case: %d fields\n", k); return 2; }
        const std::vector<unsigned long long> head = numbers(parts[0]), keys = numbers(parts[1]), pos = numbers(parts[2]), flag = numbers(parts[3]), off = numbers(parts[4]);
        const size_t n = keys.size();
        if (head.size() != 2 || pos.size() != n || flag.size() != n || off.size() != n + 1) { fprintf(stderr, "not a case: sizes\n"); return 2; }
        uint64_t *d_key = exact_block<uint64_t>(keys);
        int32_t *d_pos = exact_block<int32_t>(pos);
        uint16_t *d_flag = exact_block<uint16_t>(flag);
        uint32_t *d_off = exact_block<uint32_t>(off);
        const uint64_t salt = spl_subsample_salt(head[0]);
        for (size_t r = 0; r < n; ++r)
            printf("%s%d", r ? " " : "", spl_subsample_keep(d_key[r], (int64_t)d_pos[r], d_flag[r], d_off[r + 1] - d_off[r], salt, head[1]) ? 1 : 0);
        printf("\n");
        free(d_key); free(d_pos); free(d_flag); free(d_off);
    }
    return 0;
}
