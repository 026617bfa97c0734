// covfragment_rule_asan.cpp -- the fragment rules of spl_covfragment_rule.h (coverage) and spl_junctionfragment_rule.h (junctions)
// over one segment's arrays and its mate table, each in a heap block of exactly its size, for a build with
// -fsanitize=address,undefined (the test compiles and runs it): a load or a store beyond any of them is a heap-buffer-overflow
// there, an int32 sum that should have been int64 a UBSan report.  The mate table and the CIGAR offsets are taken as they come:
// mate indexes at and beyond the segment, a read that is its own mate, offsets that descend or point beyond the ops and a mate
// without an op are the test's to send.
// Input: the path of a file, a case a line.
//   "C|shift length stranded strand cap|pos ...|flag ...|cig_off ...|cigar ...|mate ..."
//   "J|shift stranded min_anchor min_intron max_intron cap|pos ...|flag ...|cig_off ...|cigar ...|mate ...|xs ..."   (xs: empty unless stranded = 3)
// Output.  C, five lines: every read's status (1 contributed, 0 nothing to mark, -4 silent, -3 not participating), every read's number
// of intervals, every read's "past the end", the leaders' intervals "s e s e ..." as far as cap reaches, and the six totals.  Every
// participating read's blocks by the cursor are held to spl_cov_walk's here as well: a difference ends the program with status 3.
// J, three lines: every read's counted junctions, every read's duplicate carries, and the rows "l r strand al ar dup ..." as far as cap
// reaches.  Host code only; never loaded into Python.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../spliser_amd/csrc/spl_covfragment_rule.h"
#include "../../spliser_amd/csrc/spl_junctionfragment_rule.h"

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

struct Blocks {
    std::vector<int64_t> v;
    void operator()(int64_t s, int64_t e) { v.push_back(s); v.push_back(e); }
};

struct KeepIntervals {
    int64_t cap, used, n;
    int64_t *s, *e;
    void operator()(int64_t a, int64_t b) { if (used < cap) { s[used] = a; e[used] = b; ++used; } ++n; }
};

struct KeepRows {
    int stranded;
    int64_t cap, n, counted, dup;
    int64_t *rows;
    void operator()(int32_t l, int32_t r, uint32_t code, uint32_t al, uint32_t ar, bool is_dup)
    {
        if (n < cap) {
            int64_t *row = rows + 6 * n;
            row[0] = l; row[1] = r; row[2] = !stranded ? '?' : code == 0u ? '+' : code == 1u ? '-' : '?'; row[3] = al; row[4] = ar; row[5] = is_dup ? 1 : 0;
        }
        ++n;
        ++(is_dup ? dup : counted);
    }
};

template <class T> static void print_line(const T *v, int64_t n)
{
    for (int64_t k = 0; k < n; ++k) printf("%s%lld", k ? " " : "", (long long)v[k]);
    printf("\n");
}

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
        const bool cov = parts[0] == "C";
        if ((cov && parts.size() != 7) || (!cov && (parts[0] != "J" || parts.size() != 8))) { fprintf(stderr, "not a case: %s\n", line.c_str()); return 2; }
        const std::vector<long long> head = numbers(parts[1]), pos = numbers(parts[2]), flag = numbers(parts[3]), off = numbers(parts[4]), ops = numbers(parts[5]), mt = numbers(parts[6]);
        const int64_t n = (int64_t)pos.size();
        if (head.size() != (cov ? 5u : 6u) || flag.size() != pos.size() || off.size() != pos.size() + 1 || mt.size() != pos.size()) { fprintf(stderr, "not a case: %s\n", line.c_str()); return 2; }
        int32_t *d_pos = exact_block<int32_t>(pos);
        uint16_t *d_flag = exact_block<uint16_t>(flag);
        uint32_t *d_off = exact_block<uint32_t>(off), *d_ops = exact_block<uint32_t>(ops), *d_mate = exact_block<uint32_t>(mt);
        const spl_mate_reads reads{d_pos, d_flag, d_off, d_ops, (int64_t)ops.size()};
        int64_t *per_a = (int64_t *)malloc(n ? (size_t)n * sizeof(int64_t) : 1), *per_b = (int64_t *)malloc(n ? (size_t)n * sizeof(int64_t) : 1);
        int64_t *per_c = (int64_t *)malloc(n ? (size_t)n * sizeof(int64_t) : 1);
        if (cov) {
            const int64_t shift = head[0], length = head[1], cap = head[4];
            const int stranded = (int)head[2], strand = (int)head[3];
            int64_t *iv_s = (int64_t *)malloc(cap ? (size_t)cap * sizeof(int64_t) : 1), *iv_e = (int64_t *)malloc(cap ? (size_t)cap * sizeof(int64_t) : 1);
            KeepIntervals keep{cap, 0, 0, iv_s, iv_e};
            int64_t totals[6] = {0, 0, 0, 0, 0, 0};
            for (int64_t r = 0; r < n; ++r) {
                spl_cov_side lead, other;
                const uint32_t what = spl_cov_fragment_sides(reads, 0, n, r, d_mate, shift, stranded, strand, &lead, &other);
                per_a[r] = what == SPL_COVF_SILENT ? -4 : -3;
                per_b[r] = per_c[r] = 0;
                ++totals[1];
                if (what != SPL_COVF_NOT_PARTICIPATING) { // the cursor against the walk, block for block
                    Blocks by_walk, by_cursor;
                    int64_t covered = 0;
                    const uint32_t bits = spl_cov_walk(spl_gene_ops_ptr{d_ops + lead.c0}, lead.n_ops, lead.p, length, by_walk, &covered);
                    spl_cov_cursor<spl_gene_ops_ptr> cursor(spl_gene_ops_ptr{d_ops + lead.c0}, lead.n_ops, lead.p, length);
                    for (int64_t s, e; cursor.next(&s, &e);) by_cursor(s, e);
                    if (by_walk.v != by_cursor.v || (bits & SPL_COV_PAST_END) != (cursor.bits & SPL_COV_PAST_END)) { fprintf(stderr, "the cursor and the walk differ at read %lld\n", (long long)r); return 3; }
                }
                if (what != SPL_COVF_LEADS) continue;
                keep.n = 0;
                int64_t covered = 0;
                const uint32_t bits = spl_cov_fragment_walk<spl_gene_ops_ptr>(d_ops, lead, other, length, keep, &covered);
                per_a[r] = (bits & SPL_COV_CONTRIBUTED) ? 1 : 0;
                per_b[r] = keep.n;
                per_c[r] = (bits & SPL_COV_PAST_END) ? 1 : 0;
                totals[0] += keep.n;
                totals[2] += per_a[r];
                totals[3] += per_c[r];
                totals[4] += covered;
                totals[5] += (bits & SPL_COVF_PAIR) ? 1 : 0;
            }
            print_line(per_a, n);
            print_line(per_b, n);
            print_line(per_c, n);
            for (int64_t k = 0; k < keep.used; ++k) printf("%s%lld %lld", k ? " " : "", (long long)iv_s[k], (long long)iv_e[k]);
            printf("\n");
            print_line(totals, 6);
            free(iv_s); free(iv_e);
        } else {
            const std::vector<long long> xs = numbers(parts[7]);
            const int stranded = (int)head[1];
            const int64_t cap = head[5];
            if (stranded == 3 && xs.size() != pos.size()) { fprintf(stderr, "not a case: %s\n", line.c_str()); return 2; }
            uint8_t *d_xs = exact_block<uint8_t>(xs);
            int64_t *rows = (int64_t *)malloc(cap ? (size_t)cap * 6 * sizeof(int64_t) : 1);
            const spljw::Filter filter{(uint32_t)head[2], (uint32_t)head[3], (uint32_t)head[4]};
            KeepRows keep{stranded, cap, 0, 0, 0, rows};
            for (int64_t r = 0; r < n; ++r) {
                keep.counted = keep.dup = 0;
                (void)spljf::read_junctions(reads, stranded == 3 ? d_xs : nullptr, n, r, d_mate, (int32_t)head[0], stranded, filter, keep);
                per_a[r] = keep.counted;
                per_b[r] = keep.dup;
            }
            print_line(per_a, n);
            print_line(per_b, n);
            print_line(rows, 6 * (keep.n < cap ? keep.n : cap));
            free(d_xs); free(rows);
        }
        free(d_pos); free(d_flag); free(d_off); free(d_ops); free(d_mate); free(per_a); free(per_b); free(per_c);
    }
    return 0;
}
