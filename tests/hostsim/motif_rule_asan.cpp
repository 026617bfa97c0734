// motif_rule_asan.cpp -- the rule of spl_motif_rule.h (FASTA text, motif codes, read strands) over inputs that each lie in a heap
// block of exactly their size, for a build with -fsanitize=address,undefined (the test compiles and runs it): a load beyond the
// text, the sequence or the reads' arrays is a heap-buffer-overflow there, an int32 sum that should have been int64 a UBSan report.
// The inputs are taken as they come: junctions in front of base 1 and beyond the sequence's end, CIGAR offsets that descend or point
// beyond the ops, a sequence of no bases, a text that ends in the middle of a header are the test's to send.
// Input: the path of a file, a case a line.
//   "F|<the text's bytes as hex>"
//   "R|shift|<the sequence's codes as hex, a code a byte>|pos ...|flag ...|cig_off ...|cigar ..."
//   "J|<codes as hex>|left ...|right ..."
// Output.  F: "E reason line", or a line "S n" and per sequence a line "<name as hex> length <codes as hex>".  R: two lines, every
// read's strand byte and the twelve sums.  J: one line, every row's code.  Host code only; never loaded into Python.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../spliser_amd/csrc/spl_motif_rule.h"

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

static int nibble(char c) { return c <= '9' ? c - '0' : c - 'a' + 10; }
static uint8_t *hex_block(const std::string &s, size_t *n_out)
{
    const size_t n = s.size() / 2;
    uint8_t *block = (uint8_t *)malloc(n ? n : 1);
    for (size_t i = 0; i < n; ++i) block[i] = (uint8_t)(nibble(s[2 * i]) << 4 | nibble(s[2 * i + 1]));
    *n_out = n;
    return block;
}
static void print_hex(const uint8_t *p, size_t n) { for (size_t i = 0; i < n; ++i) printf("%02x", p[i]); }

struct Sink {
    std::vector<std::string> names;
    std::vector<std::vector<uint8_t>> codes;
    bool header(const uint8_t *p, uint64_t n, int64_t)
    {
        const std::string s((const char *)p, (size_t)n);
        for (const std::string &have : names) if (have == s) return false;
        names.push_back(s);
        codes.emplace_back();
        return true;
    }
    void bases(const uint8_t *p, uint64_t n) { for (uint64_t k = 0; k < n; ++k) codes.back().push_back((uint8_t)splmotif::base_code(p[k])); }
};

struct Ops {
    const uint32_t *p;
    uint32_t operator()(uint32_t k) const { return p[k]; }
};

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: %s CASES\n", argv[0]); return 2; }
    FILE *fh = fopen(argv[1], "rb");
    if (!fh) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    std::string text;
    char buf[1 << 16];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, fh)) > 0) text.append(buf, got);
    fclose(fh);
    size_t at = 0;
    while (at < text.size()) {
        size_t nl = text.find('\n', at);
        if (nl == std::string::npos) nl = text.size();
        const std::string line = text.substr(at, nl - at);
        at = nl + 1;
        if (line.empty()) continue;
        std::vector<std::string> parts(1);
        for (char ch : line) {
            if (ch == '|') parts.emplace_back();
            else parts.back() += ch;
        }
        if (parts[0] == "F" && parts.size() == 2) {
            size_t n = 0;
            uint8_t *block = hex_block(parts[1], &n);
            Sink sink;
            int64_t bad_line = 0;
            const int reason = splmotif::fasta_scan(block, (int64_t)n, sink, &bad_line);
            if (reason != SPL_FASTA_OK) printf("E %d %lld\n", reason, (long long)bad_line);
            else {
                printf("S %zu\n", sink.names.size());
                for (size_t k = 0; k < sink.names.size(); ++k) {
                    print_hex((const uint8_t *)sink.names[k].data(), sink.names[k].size());
                    printf(" %zu ", sink.codes[k].size());
                    print_hex(sink.codes[k].data(), sink.codes[k].size());
                    printf("\n");
                }
            }
            free(block);
        } else if (parts[0] == "R" && parts.size() == 7) {
            size_t length = 0;
            uint8_t *codes = hex_block(parts[2], &length);
            const std::vector<long long> shift = numbers(parts[1]), pos = numbers(parts[3]), flag = numbers(parts[4]), off = numbers(parts[5]), ops = numbers(parts[6]);
            if (shift.size() != 1 || flag.size() != pos.size() || off.size() != pos.size() + 1) { fprintf(stderr, "not a case: %s\n", line.c_str()); return 2; }
            int32_t *d_pos = exact_block<int32_t>(pos);
            uint16_t *d_flag = exact_block<uint16_t>(flag);
            uint32_t *d_off = exact_block<uint32_t>(off), *d_ops = exact_block<uint32_t>(ops);
            long long tally[SPL_MOTIF_TALLY] = {0};
            for (size_t i = 0; i < pos.size(); ++i) {
                uint32_t c0, c1;
                splmotif::ops_span(d_off, (int64_t)i, (int64_t)ops.size(), c0, c1);
                splmotif::ReadMotifs m;
                splmotif::read_motifs(d_flag[i], (int64_t)d_pos[i] + shift[0], Ops{d_ops + c0}, c1 - c0, splmotif::BytePairs{codes}, (int64_t)length, m);
                printf("%s%d", i ? " " : "", (int)m.strand);
                for (int c = 0; c < 7; ++c) tally[c] += m.walks[c];
                if (m.cls) tally[m.cls] += 1;
                if (m.outside) tally[11] += 1;
            }
            printf("\n");
            for (int c = 0; c < SPL_MOTIF_TALLY; ++c) printf("%s%lld", c ? " " : "", tally[c]);
            printf("\n");
            free(codes); free(d_pos); free(d_flag); free(d_off); free(d_ops);
        } else if (parts[0] == "J" && parts.size() == 4) {
            size_t length = 0;
            uint8_t *codes = hex_block(parts[1], &length);
            const std::vector<long long> left = numbers(parts[2]), right = numbers(parts[3]);
            if (left.size() != right.size()) { fprintf(stderr, "not a case: %s\n", line.c_str()); return 2; }
            for (size_t i = 0; i < left.size(); ++i) {
                bool outside = false;
                printf("%s%u", i ? " " : "", splmotif::junction_code(splmotif::BytePairs{codes}, (int64_t)length, left[i], right[i], outside));
            }
            printf("\n");
            free(codes);
        } else { fprintf(stderr, "not a case: %s\n", line.c_str()); return 2; }
    }
    return 0;
}
