// Sanitizer driver for the host code that reads and writes text (no GPU needed): spl_bed_open / spl_gff_open and their accessors,
// the .SpliSER.tsv parser and the walk, tables and writer of spl_combine.cpp in the order native.Combine calls them, the row and
// bedGraph writers, the gene search, the two number formatters, and the host packer.  Built by tests/test_native_sanitizers.py
// with -fsanitize=address,undefined (and once more with -fsanitize=thread), linked with spl_host.cpp, spl_combine.cpp, spl_pack.cpp.
//
//   text_asan_driver <manifest> <work directory>
//
// The manifest has one job a line, fields separated by tabs: kind, name, then paths.  For every job the driver prints
// "kind <tab> name <tab> return code <tab> rows <tab> checksum" (between a first line "start" and a last "done <tab> jobs"); the test computes the same lines through the ordinary library
// (tests/textcases.py has the checksum's statement), so a job skipped or parsed differently here shows.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/spliser.h"
#include "../../spliser_amd/csrc/spl_pack.h"

static char g_err[1024];
int spl_set_error(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}
extern "C" const char *spl_last_error(void) { return g_err; }

namespace {

// CRC-32 as zlib.crc32 computes it (the test's side of the checksums), chained over the pieces of a job
const uint32_t CRC_OF_NOTHING = 0;
uint32_t crc32_of(const void *data, size_t n, uint32_t crc = 0)
{
    static uint32_t table[256];
    if (!table[1])
        for (uint32_t i = 0; i < 256; ++i) {
            uint32_t c = i;
            for (int k = 0; k < 8; ++k) c = (c & 1u) ? 0xedb88320u ^ (c >> 1) : c >> 1;
            table[i] = c;
        }
    const unsigned char *p = (const unsigned char *)data;
    crc = ~crc;
    for (size_t i = 0; i < n; ++i) crc = table[(crc ^ p[i]) & 0xffu] ^ (crc >> 8);
    return ~crc;
}
uint32_t crc32_of(const std::string &s, uint32_t crc = 0) { return crc32_of(s.data(), s.size(), crc); }

std::string slurp(const std::string &path)
{
    std::ifstream f(path, std::ios::binary);
    std::stringstream ss;
    ss << f.rdbuf();
    return ss.str();
}

void report(const char *kind, const std::string &name, int rc, long long rows, uint32_t sum)
{
    printf("%s\t%s\t%d\t%lld\t%08x\n", kind, name.c_str(), rc, rows, (unsigned)sum);
}

// ---- BED / GFF: open, every accessor, one text line per row (textcases.columns_text) ---------------------------------------------
void text_job(const std::string &kind, const std::string &name, const std::string &path)
{
    const bool gff = kind == "gff";
    spl_textfile *t = nullptr;
    const int rc = gff ? spl_gff_open(path.c_str(), &t) : spl_bed_open(path.c_str(), &t);
    if (rc != SPL_OK) {
        if (t) { fprintf(stderr, "%s: a handle came back with return code %d\n", path.c_str(), rc); exit(1); }
        report(kind.c_str(), name, rc, 0, CRC_OF_NOTHING);
        return;
    }
    const int64_t rows = spl_text_rows(t);
    const int32_t n_chrom = spl_text_n_chrom(t);
    const int32_t *chrom = spl_text_chrom(t);
    const int64_t *left = spl_text_i64(t, 0), *right = spl_text_i64(t, 1), *alpha = spl_text_i64(t, 2);
    const uint8_t *strand = spl_text_strand(t);
    const uint32_t *off = nullptr;
    const char *names = spl_text_names(t, &off);
    if (spl_text_chrom_name(t, -1) || spl_text_chrom_name(t, n_chrom)) { fprintf(stderr, "%s: a name outside the table\n", path.c_str()); exit(1); }
    std::string text;
    char num[128];
    for (int64_t i = 0; i < rows; ++i) {
        if (chrom[i] < 0 || chrom[i] >= n_chrom) { fprintf(stderr, "%s: row %lld names chromosome %d of %d\n", path.c_str(), (long long)i, chrom[i], n_chrom); exit(1); }
        text += spl_text_chrom_name(t, chrom[i]);
        if (gff) {
            snprintf(num, sizeof num, "\t%lld\t%lld\t%d\t", (long long)left[i], (long long)right[i], (int)strand[i]);
            text += num;
            text.append(names + off[i], off[i + 1] - off[i]);
            text += '\n';
        } else {
            snprintf(num, sizeof num, "\t%lld\t%lld\t%lld\t%d\n", (long long)left[i], (long long)right[i], (long long)alpha[i], (int)strand[i]);
            text += num;
        }
    }
    spl_text_close(t);
    report(kind.c_str(), name, rc, rows, crc32_of(text));
}

// ---- .SpliSER.tsv: what native.Combine does, for every run of textcases.COMBINE_RUNS ---------------------------------------------
struct Run { const char *gene; int shallow, cryptic; };
const char *QUERY_GENE = "GChr1_0";
const Run RUNS[8] = {{"All", 0, 0}, {"All", 0, 1}, {"All", 1, 0}, {"All", 1, 1}, {QUERY_GENE, 0, 0}, {QUERY_GENE, 0, 1}, {QUERY_GENE, 1, 0}, {QUERY_GENE, 1, 1}};

#define MUST(call) do { const int rc_ = (call); if (rc_ != SPL_OK) { fprintf(stderr, "%s: %s failed with %d: %s\n", name.c_str(), #call, rc_, g_err); exit(1); } } while (0)

void combine_job(const std::string &name, const std::vector<std::string> &paths, const std::string &work)
{
    const int32_t ns = (int32_t)paths.size();
    std::vector<const char *> cpaths, ctitles;
    std::vector<std::string> titles;
    for (int32_t i = 0; i < ns; ++i) titles.push_back("S" + std::to_string(i));
    for (int32_t i = 0; i < ns; ++i) { cpaths.push_back(paths[(size_t)i].c_str()); ctitles.push_back(titles[(size_t)i].c_str()); }
    const std::string out_path = work + "/driver.combined.tsv";
    uint32_t sum = CRC_OF_NOTHING;
    long long rows = 0;
    for (const Run &run : RUNS) {
        spl_combine *c = nullptr;
        const int rc = spl_combine_open(cpaths.data(), ns, &c);
        if (rc != SPL_OK) {
            if (c) { fprintf(stderr, "%s: a handle came back with return code %d\n", name.c_str(), rc); exit(1); }
            report("tsv", name, rc, 0, CRC_OF_NOTHING);
            return;
        }
        rows = spl_combine_rows(c, ns - 1);
        // the region order: first appearance over the samples' runs (textcases.first_appearance)
        std::vector<std::string> chroms;
        for (int32_t idx = 0; idx < ns; ++idx) {
            const int64_t n = spl_combine_region_runs(c, idx, nullptr, 0);
            std::vector<int32_t> ids((size_t)n + 1);
            spl_combine_region_runs(c, idx, ids.data(), n);
            for (int64_t k = 0; k < n; ++k) {
                const char *txt = spl_combine_text(c, ids[(size_t)k]);
                if (!txt) { fprintf(stderr, "%s: region id %d has no text\n", name.c_str(), ids[(size_t)k]); exit(1); }
                bool seen = false;
                for (const std::string &s : chroms) seen = seen || s == txt;
                if (!seen) chroms.push_back(txt);
            }
        }
        size_t text_bytes = 0;
        for (int32_t k = 0; k < spl_combine_n_texts(c); ++k) text_bytes += strlen(spl_combine_text(c, k));
        (void)text_bytes;
        std::vector<const char *> cchroms;
        for (const std::string &s : chroms) cchroms.push_back(s.c_str());
        if (run.shallow && strcmp(run.gene, "All") != 0) MUST(spl_combine_keep_gene(c, run.gene));
        MUST(spl_combine_merge(c, cchroms.data(), (int32_t)cchroms.size(), run.cryptic, run.gene, run.shallow, 1, 2, 0.1));
        const int64_t *pairs = nullptr;
        const int64_t n_skipped = spl_combine_skipped(c, &pairs);
        uint64_t touched = 0; // (unsigned: positions of 18 digits add up past 2^63)
        for (int64_t k = 0; k < 2 * n_skipped; ++k) touched += (uint64_t)pairs[k];
        for (int32_t idx = 0; idx < ns; ++idx) {
            for (int32_t k = 0; k < spl_combine_n_tables(c, idx); ++k) {
                spl_query_table t;
                MUST(spl_combine_table(c, idx, k, &t));
                touched += strlen(t.chrom);
                for (int64_t i = 0; i < t.n; ++i) {
                    touched += (uint64_t)t.pos[i] + (uint64_t)t.site[i] + t.strand[i];
                    for (uint32_t e = t.part_off[i]; e < t.part_off[i + 1]; ++e) touched += (uint64_t)t.part_pos[e];
                    for (uint32_t e = t.comp_off[i]; e < t.comp_off[i + 1]; ++e) touched += (uint64_t)t.comp_pos[e];
                }
                const std::vector<uint32_t> zeros((size_t)t.n + 1, 0u);
                MUST(spl_combine_answers(c, idx, t.n, t.site, zeros.data(), zeros.data()));
            }
        }
        MUST(spl_combine_write(c, out_path.c_str(), ctitles.data(), run.cryptic));
        char head[96];
        snprintf(head, sizeof head, "sites %lld %lld skipped %lld\n", (long long)spl_combine_n_sites(c), (long long)spl_combine_n_gap_sites(c), (long long)n_skipped);
        sum = crc32_of(std::string(head), sum);
        sum = crc32_of(slurp(out_path), sum);
        spl_combine_close(c);
        if (touched == 0x7fffffffffffffffull) printf("#\n"); // (the sums above are reads the sanitizer must see, nothing else)
    }
    report("tsv", name, 0, rows, sum);
}

// ---- the number formatters on a file of doubles -----------------------------------------------------------------------------------
void format_job(const std::string &kind, const std::string &name, const std::string &path)
{
    const std::string raw = slurp(path);
    const size_t n = raw.size() / sizeof(double);
    std::string text;
    char buf[64];
    for (size_t i = 0; i < n; ++i) {
        double x;
        memcpy(&x, raw.data() + i * sizeof(double), sizeof x);
        if (kind == "fixed") {
            for (int digits : {3, 5, 0, 6}) { MUST(spl_fmt_fixed(x, digits, buf)); text += buf; text += '\n'; }
        } else {
            MUST(spl_fmt_repr(x, buf));
            text += buf;
            text += '\n';
        }
    }
    report(kind.c_str(), name, 0, (long long)n, crc32_of(text));
}

// ---- the host packer: spl_pack_host (spl_capi.cpp, which needs the HIP runtime) restated on splpack::plan / emit ------------------
void pack_job(const std::string &name, const std::string &path)
{
    const std::string raw = slurp(path);
    int64_t n;
    memcpy(&n, raw.data(), 8);
    std::vector<int32_t> pos((size_t)n + 1);
    std::vector<uint16_t> flag((size_t)n + 1);
    std::vector<uint32_t> off((size_t)n + 1);
    size_t at = 8;
    memcpy(pos.data(), raw.data() + at, 4 * (size_t)n); at += 4 * (size_t)n;
    memcpy(flag.data(), raw.data() + at, 2 * (size_t)n); at += 2 * (size_t)n;
    memcpy(off.data(), raw.data() + at, 4 * ((size_t)n + 1)); at += 4 * ((size_t)n + 1);
    std::vector<uint32_t> cigar(off[(size_t)n]);                 // (exactly the ops: a read past them is a report)
    if (raw.size() != at + 4 * cigar.size()) { fprintf(stderr, "%s: %zu bytes, %zu expected\n", path.c_str(), raw.size(), at + 4 * cigar.size()); exit(1); }
    if (!cigar.empty()) memcpy(cigar.data(), raw.data() + at, 4 * cigar.size());
    std::string first;
    size_t n_chunks = 0;
    for (int threads : {1, 16}) {
        splpack::Source src;
        if (n) src.add(splpack::Part{pos.data(), flag.data(), off.data(), cigar.data(), n});
        splpack::Plan plan;
        splpack::plan(src, plan, threads);
        std::vector<uint8_t> rec((size_t)plan.rec_bytes, 0);
        std::vector<uint32_t> wide((size_t)plan.n_wide);
        uint32_t no_wide = 0;
        if (!plan.chunks.empty()) {
            // (several threads on ranges of chunks, as the uploads do)
            struct Job { const splpack::Source *src; const splpack::Plan *plan; uint8_t *rec; uint32_t *wide; } job{&src, &plan, rec.data(), wide.empty() ? &no_wide : wide.data()};
            splpack::parallel_for(plan.chunks.size(), threads, [](size_t c, void *arg) {
                const Job &j = *(const Job *)arg;
                splpack::emit(*j.src, *j.plan, c, c + 1, j.rec + j.plan->chunks[c].rec_off, j.wide + j.plan->chunks[c].wide_off);
            }, &job);
        }
        std::string all((const char *)plan.chunks.data(), sizeof(splpack::ChunkDesc) * plan.chunks.size());
        all.append((const char *)rec.data(), rec.size());
        all.append((const char *)wide.data(), 4 * wide.size());
        if (threads == 1) first = all;
        else if (all != first) { fprintf(stderr, "%s: 16 threads pack other bytes than one\n", name.c_str()); exit(1); }
        n_chunks = plan.chunks.size();
    }
    report("pack", name, 0, (long long)n_chunks, crc32_of(first));
}

// ---- small built-in jobs: the gene search, the two writers ------------------------------------------------------------------------
void search_jobs()
{
    struct Table { const char *name; std::vector<int64_t> left, right; std::string strand; };
    const Table tables[3] = {{"empty", {}, {}, ""}, {"one_gene", {10}, {20}, "+"}, {"equal_left", {10, 10, 10, 30}, {20, 40, 15, 50}, "+-+-"}};
    std::vector<int64_t> q_pos;
    std::vector<uint8_t> q_strand;
    for (int64_t p = 0; p < 60; p += 5)
        for (char s : {'+', '-', '?'}) { q_pos.push_back(p); q_strand.push_back((uint8_t)s); }
    for (const Table &t : tables)
        for (int stranded = 0; stranded < 2; ++stranded) {
            // (arrays of exactly n entries: a probe past the table is a report)
            std::vector<int64_t> left(t.left), right(t.right);
            std::vector<uint8_t> strand(t.strand.begin(), t.strand.end());
            std::vector<int32_t> out(q_pos.size(), 99);
            const int rc = spl_gene_search(left.data(), right.data(), strand.data(), (int64_t)left.size(), q_pos.data(), q_strand.data(), (int64_t)q_pos.size(), stranded, out.data());
            std::string text;
            for (int32_t v : out) text += std::to_string(v) + ",";
            report("search", std::string(t.name) + (stranded ? "_stranded" : "_unstranded"), rc, (long long)out.size(), crc32_of(text));
        }
}

void writer_jobs(const std::string &work)
{
    const std::string name = "writers";
    // spl_tsv_append_many: a chromosome "" of two rows, one of no rows, "c2" of one row with one partner position on two edges
    const int64_t pos_a[2] = {100, 150}, alpha_a[2] = {4, 0}, b2s_a[2] = {2, 0}, b2c_a[2] = {1, 0}, part_pos_a[1] = {200}, edge_a[1] = {4}, comp_a[1] = {300};
    const uint32_t one_off_a[3] = {0, 1, 1}, beta1_a[2] = {2, 0};
    const double sse_a[2] = {0.5, 0.0}, b2w_a[2] = {0.5, 0.0};
    const int64_t pos_c[1] = {7}, alpha_c[1] = {1}, b2s_c[1] = {0}, b2c_c[1] = {3}, part_pos_c[2] = {9, 9}, edge_c[2] = {1, 5}, comp_c[2] = {8, 9};
    const uint32_t strand_off_c[2] = {0, 1}, gene_off_c[2] = {0, 2}, two_off_c[2] = {0, 2}, beta1_c[1] = {0};
    const double sse_c[1] = {1.0}, b2w_c[1] = {5.0 / 3.0};
    spl_tsv_rows rows[3];
    memset(rows, 0, sizeof rows);
    rows[0].chrom = ""; rows[0].n_sites = 2; rows[0].pos = pos_a; rows[0].strand_blob = "+"; rows[0].strand_off = one_off_a; rows[0].gene_blob = "G";
    rows[0].gene_off = one_off_a; rows[0].sse = sse_a; rows[0].alpha = alpha_a; rows[0].beta1 = beta1_a; rows[0].beta2_simple = b2s_a; rows[0].beta2_cryptic = b2c_a;
    rows[0].beta2_weighted = b2w_a; rows[0].part_off = one_off_a; rows[0].part_pos = part_pos_a; rows[0].edge_cnt = edge_a; rows[0].comp_off = one_off_a; rows[0].comp_pos = comp_a;
    rows[1].chrom = "c1"; rows[1].n_sites = 0;
    rows[2].chrom = "c2"; rows[2].n_sites = 1; rows[2].pos = pos_c; rows[2].strand_blob = "-"; rows[2].strand_off = strand_off_c; rows[2].gene_blob = "NA";
    rows[2].gene_off = gene_off_c; rows[2].sse = sse_c; rows[2].alpha = alpha_c; rows[2].beta1 = beta1_c; rows[2].beta2_simple = b2s_c; rows[2].beta2_cryptic = b2c_c;
    rows[2].beta2_weighted = b2w_c; rows[2].part_off = two_off_c; rows[2].part_pos = part_pos_c; rows[2].edge_cnt = edge_c; rows[2].comp_off = two_off_c; rows[2].comp_pos = comp_c;
    for (int cryptic = 0; cryptic < 2; ++cryptic) {
        const std::string path = work + (cryptic ? "/append_cryptic.tsv" : "/append_plain.tsv");
        remove(path.c_str());
        MUST(spl_tsv_append_many(path.c_str(), 0, nullptr, cryptic));
        MUST(spl_tsv_append_many(path.c_str(), 3, rows, cryptic));
        report("append", cryptic ? "cryptic" : "plain", 0, 3, crc32_of(slurp(path)));
    }
    // spl_bedgraph_append: textcases.BEDGRAPH_RUNS
    const std::string path = work + "/driver.bedgraph";
    remove(path.c_str());
    const int32_t s0[2] = {0, 5}, e0[2] = {5, 9}, s2[3] = {10, 20, 30}, e2[3] = {20, 30, 31};
    const uint32_t d0[2] = {3, 0}, d2[3] = {1, 4000000000u, 7};
    MUST(spl_bedgraph_append(path.c_str(), "", 2, s0, e0, d0, 0));
    MUST(spl_bedgraph_append(path.c_str(), "c1", 0, nullptr, nullptr, nullptr, 0));
    MUST(spl_bedgraph_append(path.c_str(), "c1", 3, s2, e2, d2, 3));
    report("bedgraph", "runs", 0, 5, crc32_of(slurp(path)));
}

} // namespace

int main(int argc, char **argv)
{
    if (argc < 3) { fprintf(stderr, "usage: %s <manifest> <work directory>\n", argv[0]); return 2; }
    setvbuf(stdout, nullptr, _IOLBF, 0);   // (every line leaves at once: what ran before a report ends the program stays readable)
    printf("start\n");                     // (... and a sanitizer runtime that ends the program before main shows as such)
    const std::string work = argv[2];
    std::ifstream manifest(argv[1]);
    if (!manifest) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    std::string line;
    long long jobs = 0;
    while (std::getline(manifest, line)) {
        std::vector<std::string> f;
        size_t a = 0;
        for (;;) {
            const size_t b = line.find('\t', a);
            f.push_back(line.substr(a, b == std::string::npos ? b : b - a));
            if (b == std::string::npos) break;
            a = b + 1;
        }
        if (f.size() < 2) continue;
        const std::string &kind = f[0], &name = f[1];
        ++jobs;
        if ((kind == "bed" || kind == "gff") && f.size() == 3) text_job(kind, name, f[2]);
        else if (kind == "tsv" && f.size() >= 3) combine_job(name, std::vector<std::string>(f.begin() + 2, f.end()), work);
        else if ((kind == "fixed" || kind == "repr") && f.size() == 3) format_job(kind, name, f[2]);
        else if (kind == "pack" && f.size() == 3) pack_job(name, f[2]);
        else if (kind == "search") search_jobs();
        else if (kind == "writers") writer_jobs(work);
        else { fprintf(stderr, "manifest line not understood: %s\n", line.c_str()); return 2; }
    }
    printf("done\t%lld\n", jobs);
    return 0;
}
