// mate_rule_asan.cpp -- the rules of spl_mate_rule.h (the name key, the pair stage, a fragment's gene) over the paired read sets of
// tests/matecases.py, every array in a heap block of exactly its size, for a build with -fsanitize=address,undefined (the test
// compiles and runs it): a load beyond an array is a heap-buffer-overflow there, an int32 sum that should have been int64 a UBSan
// report.  Input, a case a line:
//   "shift stranded|pos ...|flag ...|cig_off ...|cigar ...|name keys ...|a starts ...|a codes ...|b starts ...|b codes ...|names in hex, one a word (- = empty) ..."
// Output, three lines a case: the mate of every read (4294967295: none); what every read adds (the gene's index, -1 no feature, -2
// ambiguous, -3 not counted, -4 nothing); the key of every name.  Host code only; never loaded into Python.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <utility>
#include <vector>

#include "../../spliser_amd/csrc/spl_mate_rule.h"

static std::vector<long long> numbers(const std::string &s)
{
    std::vector<long long> out;
    const char *p = s.c_str();
    char *end = nullptr;
    for (;;) {
        const long long v = (long long)strtoull(p, &end, 10); // (keys use all 64 bits; a '-' in front negates, as strtoll would)
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
        std::string parts[11];
        int k = 0;
        for (char ch : line) {
            if (ch == '|') { if (++k > 10) break; }
            else parts[k] += ch;
        }
        if (k != 10) { fprintf(stderr, "not a case: %d fields\n", k); return 2; }
        const std::vector<long long> head = numbers(parts[0]), pos = numbers(parts[1]), flag = numbers(parts[2]), off = numbers(parts[3]), cig = numbers(parts[4]), keys = numbers(parts[5]),
                                     as = numbers(parts[6]), ac = numbers(parts[7]), bs = numbers(parts[8]), bc = numbers(parts[9]);
        const size_t n = pos.size();
        if (head.size() != 2 || flag.size() != n || off.size() != n + 1 || keys.size() != n || as.size() != ac.size() || bs.size() != bc.size() || (size_t)off[n] != cig.size()) {
            fprintf(stderr, "not a case: sizes\n");
            return 2;
        }
        int32_t *d_pos = exact_block<int32_t>(pos);
        uint16_t *d_flag = exact_block<uint16_t>(flag);
        uint32_t *d_off = exact_block<uint32_t>(off), *d_cig = exact_block<uint32_t>(cig);
        uint64_t *d_key = exact_block<uint64_t>(keys);
        int32_t *a_start = exact_block<int32_t>(as), *b_start = exact_block<int32_t>(bs);
        uint32_t *a_code = exact_block<uint32_t>(ac), *b_code = exact_block<uint32_t>(bc);
        // the compaction and a stable sort, then the pair stage's body element by element
        std::vector<std::pair<uint64_t, uint32_t>> el;
        for (size_t r = 0; r < n; ++r)
            if (spl_mate_pairable(d_flag[r], (int64_t)d_pos[r], d_off[r + 1] - d_off[r], d_key[r])) el.push_back({spl_mate_sort_key(d_key[r], d_flag[r]), (uint32_t)r});
        std::stable_sort(el.begin(), el.end(), [](const std::pair<uint64_t, uint32_t> &a, const std::pair<uint64_t, uint32_t> &b) { return a.first < b.first; });
        std::vector<long long> sk, si;
        for (const auto &e : el) { sk.push_back((long long)e.first); si.push_back((long long)e.second); }
        uint64_t *s_keys = exact_block<uint64_t>(sk);
        uint32_t *s_index = exact_block<uint32_t>(si);
        uint32_t *mate = exact_block<uint32_t>(std::vector<long long>(n, (long long)SPL_MATE_NONE));
        for (size_t j = 0; j < el.size(); ++j) (void)spl_mate_pair_element(s_keys, s_index, (int64_t)el.size(), (int64_t)j, mate, (int64_t)n);
        for (size_t r = 0; r < n; ++r) printf("%s%u", r ? " " : "", mate[r]);
        printf("\n");
        const spl_mate_reads reads{d_pos, d_flag, d_off, d_cig, (int64_t)cig.size()};
        const spl_gene_map_flat map_a{(int64_t)as.size(), a_start, a_code}, map_b{(int64_t)bs.size(), b_start, b_code};
        for (size_t r = 0; r < n; ++r) {
            const uint32_t v = spl_gene_fragment_result<spl_gene_ops_ptr>(reads, 0, (int64_t)n, (int64_t)r, mate, (int64_t)head[0], (int)head[1], map_a, map_b);
            printf("%s%lld", r ? " " : "", v == SPL_GENE_NO_FEATURE ? -1ll : v == SPL_GENE_AMBIGUOUS ? -2ll : v == SPL_GENE_NOT_COUNTED ? -3ll : v == SPL_GENE_IDLE ? -4ll : (long long)v);
        }
        printf("\n");
        // names
        bool first = true;
        size_t w = 0;
        const std::string &names = parts[10];
        while (w < names.size()) {
            while (w < names.size() && names[w] == ' ') ++w;
            size_t e = w;
            while (e < names.size() && names[e] != ' ') ++e;
            if (e == w) break;
            const std::string word = names.substr(w, e - w);
            w = e;
            const size_t len = word == "-" ? 0 : word.size() / 2;
            uint8_t *bytes = (uint8_t *)malloc(len ? len : 1);
            for (size_t i = 0; i < len; ++i) bytes[i] = (uint8_t)strtoul(word.substr(2 * i, 2).c_str(), nullptr, 16);
            printf("%s%llu", first ? "" : " ", (unsigned long long)spl_name_key(bytes, len));
            first = false;
            free(bytes);
        }
        printf("\n");
        free(d_pos); free(d_flag); free(d_off); free(d_cig); free(d_key); free(a_start); free(b_start); free(a_code); free(b_code); free(s_keys); free(s_index); free(mate);
    }
    return 0;
}
