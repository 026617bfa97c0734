// spl_sam_line.h -- THE definition of how one line of SAM text is read (spl_sam_open): the device kernels (spl_sam.hip), the host
// parser (bam_reader.cpp: sam_host_worker) and the tests' stand-alone sanitizer program all call spl_sam_parse_line and nothing else, as
// spl_bam_aux.h is the one walk of a BAM record's aux area.
//
// The rule is STRICT: a file with any line it does not take is declined as a whole and read by the Python reader (samio.read_sam)
// as before this decoder existed, so nothing that was accepted stops being accepted.  For every file the rule takes, the arrays
// are samio.read_sam's and the counters are the BAM decoder's on the BAM of the same records.
//
//   line    the bytes up to, not including, '\n' (the file's last line may lack it); an empty line is declined; a line that
//           begins with '@' behind the first alignment line is declined (header lines are the host's, spl_sam_open); a line
//           that holds a carriage return is declined (read_sam reads text, where '\r' ends a line); at least 11 TAB-separated
//           columns
//   FLAG    1-5 digits, at most 65535;  POS 1-10 digits, at most 2^31 - 1;  MAPQ 1-3 digits, at most 255 -- digits only
//   RNAME   '*': the record is counted (n_records, flagstat) and not extracted; else a name of the header's @SQ lines (tid = its
//           index in header order), any other name is declined; a named reference at POS 0 is declined
//   CIGAR   '*': no ops; else one or more of (1-9 digits, value < 2^28, one letter of MIDNSHP=X) -> len << 4 | code; anything
//           else, 'B' included, is declined
//   RNEXT   '=': the line's own tid, '*': -1, a name: looked up, unknown: declined (flagstat's next_tid)
//   filter  spl_bam_filter_verdict on FLAG and MAPQ, flags first (spl_bam.h)
//   strand  samio.sam_aux_strand: 0 unless the CIGAR holds an N; else the value of the first column from the 12th on that begins
//           "XS:A:", if that value is exactly '+' or '-' followed by TAB or the line's end, else 0 ("XS:i:" is another field)
//   name    where the decode was asked for name keys (spl_bam_set_mate_keys): spl_name_key_sam of the line, the key of column 1 --
//           the bytes from the line's start to its first TAB -- by spl_mate_rule.h, taken by the caller for a line it extracts
//
// No byte at or beyond `end` is ever read: every load is preceded by the comparison that allows it.
#ifndef SPL_SAM_LINE_H
#define SPL_SAM_LINE_H
#include <stdint.h>

#include "spl_bam.h"
#define SPL_MATE_KEY_ONLY // (the name key alone: spl_name_key_sam, column 1 of a line the rule has taken)
#include "spl_mate_rule.h"
#undef SPL_MATE_KEY_ONLY

// why a line (a file) is declined; 0 = the line is taken
#define SPL_SAM_OK 0u
#define SPL_SAM_EMPTY 1u
#define SPL_SAM_LATE_HEADER 2u
#define SPL_SAM_COLUMNS 3u
#define SPL_SAM_BAD_FLAG 4u
#define SPL_SAM_BAD_RNAME 5u
#define SPL_SAM_BAD_POS 6u
#define SPL_SAM_BAD_MAPQ 7u
#define SPL_SAM_BAD_CIGAR 8u
#define SPL_SAM_BAD_RNEXT 9u
#define SPL_SAM_POS_ZERO 10u
#define SPL_SAM_LONG_LINE 11u  // (the decoders': a line, its newline counted, longer than a window: spl_sam_window_bytes, spl_bam.h)
#define SPL_SAM_TOO_MANY 12u   // (the driver's: the file's CIGAR ops or placed records do not fit 32 bits)
#define SPL_SAM_CR 13u         // a carriage return anywhere in the line: read_sam opens the file as text, where it ends a line
#define SPL_SAM_N_REASONS 14u

inline const char *spl_sam_reason_text(uint32_t reason)
{
    static const char *const text[SPL_SAM_N_REASONS] = {"is fine", "is empty", "is a header line behind the first alignment", "has fewer than 11 columns",
        "has a FLAG that is not 0..65535 in digits", "names a reference the header does not have", "has a POS that is not 0..2147483647 in digits",
        "has a MAPQ that is not 0..255 in digits", "has a CIGAR that is not '*' or ops of MIDNSHP=X below 2^28", "names a mate reference the header does not have",
        "has a reference and POS 0", "is longer than a window (SPL_SAM_WINDOW_BYTES)", "brings the file beyond 2^32 CIGAR operations or placed reads", "holds a carriage return"};
    return reason < SPL_SAM_N_REASONS ? text[reason] : "?";
}

// The header's reference names for a lane to look one up: an open-addressed table (slot = tid + 1, 0 = free; linear probing from
// the 32-bit FNV-1a hash of the name's bytes; n_slots a power of two, at least twice the names), the names' bytes end to end and
// where each begins (n + 1 offsets).  The names are unique (spl_sam_open).
struct spl_sam_names {
    const uint32_t *slots;
    const uint32_t *name_off;
    const uint8_t *blob;
    uint32_t n_slots;
    int32_t n;
};

SPL_BAM_HD inline uint32_t spl_sam_hash(const uint8_t *p, const uint8_t *end)
{
    uint32_t h = 2166136261u;
    for (; p < end; ++p) h = (h ^ *p) * 16777619u;
    return h;
}

SPL_BAM_HD inline bool spl_sam_name_is(const spl_sam_names &t, int32_t tid, const uint8_t *p, const uint8_t *end)
{
    const uint32_t a = t.name_off[tid], b = t.name_off[tid + 1];
    if ((uint64_t)(end - p) != (uint64_t)(b - a)) return false;
    for (uint32_t k = 0; k < b - a; ++k)
        if (t.blob[a + k] != p[k]) return false;
    return true;
}

// -> the tid of the name [p, end), or -2 when the header has none such.  hint: a tid to try first (the previous line's), or < 0.
SPL_BAM_HD inline int32_t spl_sam_lookup(const spl_sam_names &t, const uint8_t *p, const uint8_t *end, int32_t hint)
{
    if (hint >= 0 && hint < t.n && spl_sam_name_is(t, hint, p, end)) return hint; // (names are unique: spl_sam_open refuses a header that repeats one)
    if (!t.n_slots) return -2;
    uint32_t s = spl_sam_hash(p, end) & (t.n_slots - 1u);
    for (uint32_t k = 0; k < t.n_slots; ++k, s = (s + 1u) & (t.n_slots - 1u)) {
        const uint32_t v = t.slots[s];
        if (!v) return -2;
        if (spl_sam_name_is(t, (int32_t)(v - 1u), p, end)) return (int32_t)(v - 1u);
    }
    return -2;
}

// digits only, 1..max_digits of them, value <= limit -> true and *out
SPL_BAM_HD inline bool spl_sam_number(const uint8_t *p, const uint8_t *end, uint32_t max_digits, uint64_t limit, uint64_t *out)
{
    if (p >= end || (uint64_t)(end - p) > max_digits) return false;
    uint64_t v = 0;
    for (; p < end; ++p) {
        const uint32_t d = (uint32_t)*p - (uint32_t)'0';
        if (d > 9u) return false;
        v = v * 10u + d;
    }
    if (v > limit) return false;
    *out = v;
    return true;
}

SPL_BAM_HD inline int32_t spl_sam_op_code(uint8_t c)
{
    switch (c) {
    case 'M': return 0;
    case 'I': return 1;
    case 'D': return 2;
    case 'N': return 3;
    case 'S': return 4;
    case 'H': return 5;
    case 'P': return 6;
    case '=': return 7;
    case 'X': return 8;
    default: return -1;
    }
}

// The CIGAR column [p, end): its ops into out[0 ..) when out is not null (the caller has room for them: a first call with null
// counts), -> false when the column is not a CIGAR of the rule.  ref_len: the reference bases its ops cover (M D N = X).
SPL_BAM_HD inline bool spl_sam_cigar(const uint8_t *p, const uint8_t *end, uint32_t *out, uint32_t *n_out, int64_t *ref_len_out, bool *has_n_out)
{
    uint32_t n = 0;
    int64_t ref_len = 0;
    bool has_n = false;
    *n_out = 0;
    if (end - p == 1 && p[0] == '*') { *ref_len_out = 0; *has_n_out = false; return true; }
    if (p >= end) return false;
    while (p < end) {
        uint32_t v = 0, digits = 0;
        while (p < end && (uint32_t)*p - (uint32_t)'0' <= 9u) {
            if (++digits > 9u) return false;
            v = v * 10u + ((uint32_t)*p - (uint32_t)'0');
            ++p;
        }
        if (!digits || p >= end || v >= (1u << 28)) return false;
        const int32_t code = spl_sam_op_code(*p);
        if (code < 0) return false;
        ++p;
        if (out) out[n] = v << 4 | (uint32_t)code;
        if (code == 0 || code == 2 || code == 3 || code == 7 || code == 8) ref_len += v;
        has_n = has_n || code == 3;
        if (++n == 0u) return false; // (2^32 ops in one line: no line is that long, no counter wraps)
    }
    *n_out = n;
    *ref_len_out = ref_len;
    *has_n_out = has_n;
    return true;
}

// What the rule reads off one line.
struct spl_sam_line {
    uint32_t reason;      // SPL_SAM_*: the rest is meaningful when 0
    uint32_t flag, mapq;
    int32_t pos, tid, next_tid; // pos as in the text (1-based), tid = -1 for '*'
    uint32_t n_ops;
    uint32_t cigar_at, cigar_len; // where the CIGAR column lies, counted from the line's first byte
    int32_t verdict;      // spl_bam_filter_verdict of (flag, mapq), for every line
    uint8_t placed;       // a reference and a position: extracted when verdict == SPL_BAM_KEPT
    uint8_t xs;           // the strand byte (0 unless want_xs)
    int64_t end;          // the last reference base the read covers (placed lines)
};

SPL_BAM_HD inline void spl_sam_parse_line(const uint8_t *p, const uint8_t *end, const spl_sam_names &names, int32_t hint_tid, const spl_bam_filter &filter, bool want_xs,
                                          spl_sam_line *out)
{
    out->reason = SPL_SAM_OK;
    out->flag = out->mapq = 0;
    out->pos = 0;
    out->tid = out->next_tid = -1;
    out->n_ops = out->cigar_at = out->cigar_len = 0;
    out->verdict = SPL_BAM_KEPT;
    out->placed = 0;
    out->xs = 0;
    out->end = 0;
    if (p >= end) { out->reason = SPL_SAM_EMPTY; return; }
    if (p[0] == '@') { out->reason = SPL_SAM_LATE_HEADER; return; }
    // the first ten TABs: col[k] = where column k begins, col[k + 1] - 1 = its end (column 10, QUAL, ends at the eleventh TAB or the line's end)
    const uint8_t *col[11];
    col[0] = p;
    uint32_t n_col = 1;
    const uint8_t *q = p;
    bool cr = false;
    for (; q < end && n_col < 11u; ++q) {
        cr = cr || *q == '\r';
        if (*q == '\t') col[n_col++] = q + 1;
    }
    // ... and the rest of the line: QUAL, then the optional columns (the 12th on), the first "XS:A:" among them
    uint8_t xs = 0;
    {
        const uint8_t *f = nullptr; // where the column q is in begins, from the 12th on
        bool found = false;
        for (;; ++q) {
            if (q == end || *q == '\t') {
                if (f && !found && q - f >= 5 && f[0] == 'X' && f[1] == 'S' && f[2] == ':' && f[3] == 'A' && f[4] == ':') {
                    found = true;
                    xs = q - f == 6 && (f[5] == '+' || f[5] == '-') ? f[5] : (uint8_t)0;
                }
                if (q == end) break;
                f = q + 1;
            } else
                cr = cr || *q == '\r';
        }
    }
    if (cr) { out->reason = SPL_SAM_CR; return; }
    if (n_col < 11u) { out->reason = SPL_SAM_COLUMNS; return; }
    uint64_t v = 0;
    if (!spl_sam_number(col[1], col[2] - 1, 5, 65535u, &v)) { out->reason = SPL_SAM_BAD_FLAG; return; }
    out->flag = (uint32_t)v;
    const uint8_t *r0 = col[2], *r1 = col[3] - 1;
    if (r1 - r0 == 1 && r0[0] == '*') out->tid = -1;
    else {
        out->tid = spl_sam_lookup(names, r0, r1, hint_tid);
        if (out->tid < 0) { out->reason = SPL_SAM_BAD_RNAME; return; }
    }
    if (!spl_sam_number(col[3], col[4] - 1, 10, 2147483647u, &v)) { out->reason = SPL_SAM_BAD_POS; return; }
    out->pos = (int32_t)v;
    if (!spl_sam_number(col[4], col[5] - 1, 3, 255u, &v)) { out->reason = SPL_SAM_BAD_MAPQ; return; }
    out->mapq = (uint32_t)v;
    int64_t ref_len = 0;
    bool has_n = false;
    if (!spl_sam_cigar(col[5], col[6] - 1, nullptr, &out->n_ops, &ref_len, &has_n)) { out->reason = SPL_SAM_BAD_CIGAR; return; }
    out->cigar_at = (uint32_t)(col[5] - p);
    out->cigar_len = (uint32_t)(col[6] - 1 - col[5]);
    const uint8_t *m0 = col[6], *m1 = col[7] - 1;
    if (m1 - m0 == 1 && m0[0] == '=') out->next_tid = out->tid;
    else if (m1 - m0 == 1 && m0[0] == '*') out->next_tid = -1;
    else {
        out->next_tid = spl_sam_lookup(names, m0, m1, out->tid);
        if (out->next_tid < 0) { out->reason = SPL_SAM_BAD_RNEXT; return; }
    }
    if (out->tid >= 0 && out->pos == 0) { out->reason = SPL_SAM_POS_ZERO; return; }
    out->verdict = spl_bam_filter_verdict(filter, out->flag, out->mapq);
    out->placed = out->tid >= 0 ? 1 : 0;
    out->end = (int64_t)out->pos + (ref_len > 0 ? ref_len : 1) - 1;
    if (!out->placed) out->n_ops = 0; // (nothing of such a line is extracted)
    if (want_xs && has_n && out->placed) out->xs = xs;
}

#endif
