// spl_motif_rule.h -- a junction's strand from the genome's splice motifs, stated once for the device (spl_genome.hip, spl_motif.hip)
// and the host (spl_genome_pack_host, spl_motif_read_strand_host; tests/hostsim/motif_rule_asan.cpp compiles it alone).  The
// yardstick is tests/motifcases.py, a restatement in Python written without this file.
//
// BASE CODES, four bits: A = 1, C = 2, G = 4, T = 8, either letter case (genomes are soft-masked); every other byte is 0.
//
// FASTA: a line that begins with '>' opens a sequence, its name the bytes behind '>' up to the first space, tab, CR or the line's
// end; every other line is a sequence line, every byte of it a base except one CR directly in front of the newline.  Lines may
// have any length, empty lines are skipped, a last line without a newline is taken, a sequence of no bases is legal.  Declined
// (the reasons below, with the 1-based line): bytes before the first '>', an empty name, a repeated name, no sequence at all,
// and a file that begins with gzip's magic.
//
// MOTIF CODE of a junction (l, r) in spl_junctions' site convention (l the last base before the intron, r the last intronic
// base, 1-based): the donor pair is bases l + 1, l + 2, the acceptor pair bases r - 1, r; the codes are those of column 5 of
// STAR's SJ.out.tab -- 1 GT..AG +, 2 CT..AC -, 3 GC..AG +, 4 CT..GC -, 5 AT..AC +, 6 GT..AT -, 0 everything else: a pair with a 0
// base, an intron shorter than 4, a pair outside [1, length].  Odd codes are '+', even ones that are not 0 are '-'.
//
// READ STRAND: over ALL N ops of the read, in spl_junction_walk.h's walk with the knobs 0, 0, 0 (the knobs decide what supports
// a junction, not what strand a read has): '+' with a '+' code and no '-' code, '-' for the mirror case, 0 otherwise.  A read
// that is unmapped (0x4), has POS < 1 or no N op gets 0: the reads spl_bam_set_aux_strand leaves at 0.  This is STAR's
// --outSAMstrandField intronMotif, except that reads of inconsistent motifs stay (and count under '?') where STAR removes them.
#ifndef SPL_MOTIF_RULE_H
#define SPL_MOTIF_RULE_H
#include <stdint.h>

#include "spl_junction_walk.h"
#include "spl_read_view.h"

#ifndef SPL_MOTIF_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define SPL_MOTIF_HD __host__ __device__ __forceinline__
#else
#define SPL_MOTIF_HD inline
#endif
#endif

#define SPL_MOTIF_TALLY 12 // junction walks by code 0 .. 6; reads '+', '-', conflicting, spliced without a canonical junction, with a pair outside

// why a FASTA is declined
#define SPL_FASTA_OK 0
#define SPL_FASTA_BEFORE_HEADER 1
#define SPL_FASTA_EMPTY_NAME 2
#define SPL_FASTA_REPEATED_NAME 3
#define SPL_FASTA_NO_SEQUENCE 4
#define SPL_FASTA_GZIP 5

// what a line is
#define SPL_FASTA_LINE_EMPTY 0
#define SPL_FASTA_LINE_HEADER 1
#define SPL_FASTA_LINE_BASES 2

namespace splmotif {

SPL_MOTIF_HD uint32_t base_code(uint32_t byte)
{
    switch (byte | 0x20u) {
    case 'a': return 1u;
    case 'c': return 2u;
    case 'g': return 4u;
    case 't': return 8u;
    default: return 0u;
    }
}

// A line is bytes [p, end), its newline not among them; has_newline: one follows.  -> the bytes that count: all but one CR in
// front of the newline.
SPL_MOTIF_HD uint64_t line_content(const uint8_t *p, const uint8_t *end, bool has_newline)
{
    uint64_t n = (uint64_t)(end - p);
    if (has_newline && n && p[n - 1] == '\r') --n;
    return n;
}
SPL_MOTIF_HD int line_kind(const uint8_t *p, uint64_t content) { return content == 0 ? SPL_FASTA_LINE_EMPTY : p[0] == '>' ? SPL_FASTA_LINE_HEADER : SPL_FASTA_LINE_BASES; }
// the name of a header line of `content` bytes: the bytes behind '>' up to the first space, tab or CR
SPL_MOTIF_HD uint64_t name_length(const uint8_t *p, uint64_t content)
{
    uint64_t n = 0;
    while (1 + n < content && p[1 + n] != ' ' && p[1 + n] != '\t' && p[1 + n] != '\r') ++n;
    return n;
}

SPL_MOTIF_HD uint32_t motif_code_of(uint32_t d1, uint32_t d2, uint32_t a1, uint32_t a2)
{
    switch (d1 | d2 << 4 | a1 << 8 | a2 << 12) {
    case 4u | 8u << 4 | 1u << 8 | 4u << 12: return 1u; // GT..AG
    case 2u | 8u << 4 | 1u << 8 | 2u << 12: return 2u; // CT..AC
    case 4u | 2u << 4 | 1u << 8 | 4u << 12: return 3u; // GC..AG
    case 2u | 8u << 4 | 4u << 8 | 2u << 12: return 4u; // CT..GC
    case 1u | 8u << 4 | 1u << 8 | 2u << 12: return 5u; // AT..AC
    case 4u | 8u << 4 | 1u << 8 | 8u << 12: return 6u; // GT..AT
    default: return 0u;
    }
}
SPL_MOTIF_HD int code_sign(uint32_t code) { return code == 0u ? 0 : (code & 1u) ? 1 : -1; }

// `pair(p, a, b)`: the codes of bases p and p + 1 (1-based, both inside the sequence) into a and b.
template <class Pair>
SPL_MOTIF_HD uint32_t junction_code(const Pair &pair, int64_t length, int64_t l, int64_t r, bool &outside)
{
    outside = false;
    if (r - l < 4) return 0u;
    if (l + 1 < 1 || r > length) { outside = true; return 0u; } // (r - l >= 4: the donor pair ends in front of r, the acceptor pair begins behind l)
    uint32_t d1, d2, a1, a2;
    pair(l + 1, d1, d2);
    pair(r - 1, a1, a2);
    return motif_code_of(d1, d2, a1, a2);
}

// a sequence with a code per byte (the host's form)
struct BytePairs {
    const uint8_t *codes;
    SPL_MOTIF_HD void operator()(int64_t p, uint32_t &a, uint32_t &b) const { a = codes[p - 1] & 15u; b = codes[p] & 15u; }
};
// ... and two codes per byte, base p in nibble p - 1, the low nibble first (the device's form): one load where the pair lies in a byte
struct NibblePairs {
    const uint8_t *packed;
    SPL_MOTIF_HD void operator()(int64_t p, uint32_t &a, uint32_t &b) const
    {
        const uint64_t i = (uint64_t)(p - 1);
        const uint32_t x = packed[i >> 1];
        if (i & 1u) { a = x >> 4; b = packed[(i >> 1) + 1u] & 15u; }
        else { a = x & 15u; b = x >> 4; }
    }
};

// A read's ops in the arrays: cigar[c0, c1) (spl_ops_of, spl_read_view.h: offsets that descend or point beyond the arrays' ops are
// an empty CIGAR).
SPL_HD void ops_span(const uint32_t *cig_off, int64_t i, int64_t n_ops_total, uint32_t &c0, uint32_t &c1)
{
    uint32_t n_ops;
    spl_ops_of(cig_off, i, n_ops_total, &c0, &n_ops);
    c1 = c0 + n_ops;
}

// what one read adds to the tally: its walks by code (a read has several), and the read's class
struct ReadMotifs {
    uint32_t walks[7];
    uint8_t strand;  // '+', '-' or 0
    uint32_t cls;    // SPL_MOTIF_TALLY index 7 .. 10 of the read's class, or 0: not spliced (not walked)
    bool outside;    // a pair of one of its junctions lies outside the sequence
};

// The rule for one read.  ops(k): its k-th op in BAM form; pos: POS (1-based) in the sequence's coordinates.
template <class Ops, class Pair>
SPL_MOTIF_HD void read_motifs(uint32_t flag, int64_t pos, const Ops &ops, uint32_t n_ops, const Pair &pair, int64_t length, ReadMotifs &out)
{
    for (int c = 0; c < 7; ++c) out.walks[c] = 0u;
    out.strand = 0; out.cls = 0u; out.outside = false;
    if ((flag & 4u) || pos < 1 || pos > (int64_t)SPL_COORD_MAX || n_ops == 0u) return;
    const spljw::Filter all{0u, 0u, 0u};
    spljw::Walk w;
    w.begin((int32_t)pos);
    spljw::Junction j;
    bool plus = false, minus = false, any = false;
    while (spljw::next(w, ops, n_ops, all, j)) {
        bool outside = false;
        const uint32_t code = junction_code(pair, length, (int64_t)j.l, (int64_t)j.r, outside);
        for (uint32_t c = 0; c < 7u; ++c) out.walks[c] += code == c ? 1u : 0u; // (no index that a register file cannot take)
        out.outside = out.outside || outside;
        plus = plus || code_sign(code) > 0;
        minus = minus || code_sign(code) < 0;
        any = true;
    }
    if (!any) return;
    if (plus && !minus) { out.strand = (uint8_t)'+'; out.cls = 7u; }
    else if (minus && !plus) { out.strand = (uint8_t)'-'; out.cls = 8u; }
    else if (plus && minus) out.cls = 9u;
    else out.cls = 10u;
}

// The FASTA rule over text in host memory.  sink.header(name, name_len, line) -> false when the name was seen before;
// sink.bases(p, n): n bytes of the open sequence.  -> SPL_FASTA_OK, or the reason with *bad_line the 1-based line.
template <class Sink>
inline int fasta_scan(const uint8_t *text, int64_t len, Sink &sink, int64_t *bad_line)
{
    *bad_line = 0;
    if (len >= 2 && text[0] == 0x1f && text[1] == 0x8b) { *bad_line = 1; return SPL_FASTA_GZIP; }
    int64_t line = 0, n_seq = 0;
    const uint8_t *p = text, *const stop = text + (len > 0 ? len : 0);
    while (p < stop) {
        ++line;
        const uint8_t *end = p;
        while (end < stop && *end != '\n') ++end;
        const bool has_newline = end < stop;
        const uint64_t content = line_content(p, end, has_newline);
        const int kind = line_kind(p, content);
        if (kind == SPL_FASTA_LINE_HEADER) {
            const uint64_t n = name_length(p, content);
            if (n == 0) { *bad_line = line; return SPL_FASTA_EMPTY_NAME; }
            if (!sink.header(p + 1, n, line)) { *bad_line = line; return SPL_FASTA_REPEATED_NAME; }
            ++n_seq;
        } else if (kind == SPL_FASTA_LINE_BASES) {
            if (n_seq == 0) { *bad_line = line; return SPL_FASTA_BEFORE_HEADER; }
            sink.bases(p, content);
        }
        p = has_newline ? end + 1 : end;
    }
    if (n_seq == 0) { *bad_line = line ? line : 1; return SPL_FASTA_NO_SEQUENCE; }
    return SPL_FASTA_OK;
}

} // namespace splmotif
#endif
