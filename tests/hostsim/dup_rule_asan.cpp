// dup_rule_asan.cpp -- the rule of spl_dup_rule.h over the segments of tests/dupcases.py, every array in a heap block of exactly its
// size, for a build with -fsanitize=address,undefined (the test compiles and runs it): a load beyond an array is a
// heap-buffer-overflow there, a shift or a sum the rule did not mean a UBSan report.  Input, a segment a line:
//   "pos ...|flag ...|cig_off ...|cigar ...|name keys ...|mate ..."
// Output, two lines a segment: per LEADING read "index:W0:W1:W2" in leader order; then 1 or 0 per read, marked or not, and behind a
// '|' the sizes of the groups in the sorted order.  Host code only; never loaded into Python.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../spliser_amd/csrc/spl_dup_rule.h"

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

template <class T, class V> static T *exact_block(const std::vector<V> &v)
{
    T *block = (T *)malloc(v.empty() ? 1 : v.size() * sizeof(T));
    for (size_t i = 0; i < v.size(); ++i) block[i] = (T)v[i];
    return block;
}

struct El { spl_dup_sig sig; uint32_t leader; };

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
        if (k != 5) { fprintf(stderr, "not a segment: %d fields\n", k); return 2; }
        const std::vector<unsigned long long> pos = numbers(parts[0]), flag = numbers(parts[1]), off = numbers(parts[2]), cigar = numbers(parts[3]), keys = numbers(parts[4]),
                                              mate = numbers(parts[5]);
        const size_t n = pos.size();
        if (flag.size() != n || off.size() != n + 1 || keys.size() != n || mate.size() != n || cigar.size() != off[n]) { fprintf(stderr, "not a segment: sizes\n"); return 2; }
        int32_t *d_pos = exact_block<int32_t>(pos);
        uint16_t *d_flag = exact_block<uint16_t>(flag);
        uint32_t *d_off = exact_block<uint32_t>(off), *d_cigar = exact_block<uint32_t>(cigar), *d_mate = exact_block<uint32_t>(mate);
        uint64_t *d_key = exact_block<uint64_t>(keys);
        const spl_read_view reads{d_pos, d_flag, d_off, d_cigar, (int64_t)off[n]};
        std::vector<El> el;
        for (size_t r = 0; r < n; ++r) {
            spl_frag_side me, its;
            if (spl_dup_sides(reads, 0, (int64_t)n, (int64_t)r, d_mate, &me, &its) != SPL_FRAG_LEADS) continue;
            const spl_dup_sig sig = spl_dup_signature(reads, me, its, d_key[r]);
            printf("%s%zu:%llu:%llu:%llu", el.empty() ? "" : " ", r, (unsigned long long)sig.w0, (unsigned long long)sig.w1, (unsigned long long)sig.w2);
            el.push_back(El{sig, (uint32_t)r});
        }
        printf("\n");
        std::stable_sort(el.begin(), el.end(), [](const El &a, const El &b) {
            return a.sig.w0 != b.sig.w0 ? a.sig.w0 < b.sig.w0 : a.sig.w1 != b.sig.w1 ? a.sig.w1 < b.sig.w1 : a.sig.w2 < b.sig.w2;
        });
        std::vector<uint64_t> w0, w1;
        std::vector<uint32_t> perm, leader;
        for (size_t j = 0; j < el.size(); ++j) { w0.push_back(el[j].sig.w0); w1.push_back(el[j].sig.w1); perm.push_back((uint32_t)j); leader.push_back(el[j].leader); }
        uint64_t *d_w0 = exact_block<uint64_t>(w0), *d_w1 = exact_block<uint64_t>(w1);
        uint32_t *d_perm = exact_block<uint32_t>(perm), *d_leader = exact_block<uint32_t>(leader);
        uint8_t *d_dup = (uint8_t *)calloc(n ? n : 1, 1);
        const int64_t n_el = (int64_t)el.size();
        std::string groups;
        for (int64_t j = 0; j < n_el; ++j) {
            (void)spl_dup_mark_element(d_w0, d_w1, d_perm, d_leader, n_el, j, d_mate, (int64_t)n, d_dup);
            if (j && spl_dup_same(d_w0, d_w1, j - 1, j)) continue;
            groups += " " + std::to_string((long long)(spl_dup_group_end(d_w0, d_w1, n_el, j) - j));
        }
        for (size_t r = 0; r < n; ++r) printf("%s%d", r ? " " : "", (int)d_dup[r]);
        printf("|%s\n", groups.c_str());
        free(d_pos); free(d_flag); free(d_off); free(d_cigar); free(d_mate); free(d_key); free(d_w0); free(d_w1); free(d_perm); free(d_leader); free(d_dup);
    }
    return 0;
}
