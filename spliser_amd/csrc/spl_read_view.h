// spl_read_view.h -- the BAM-native arrays of a segment as a per-read rule reads them, and a read's ops as a walk takes them: stated
// once for every rule header and every kernel over those arrays.  The kernels include this header with SPL_HD = __device__
// __forceinline__; it contains no HIP intrinsics, so that the host and tests/ compile it too.
#ifndef SPL_READ_VIEW_H
#define SPL_READ_VIEW_H

#include <stdint.h>

#ifndef SPL_HD
#define SPL_HD inline
#endif

// A read's ops where they lie, as every walk takes them: ops(k) = the read's k-th op (BAM form).
struct spl_ops_ptr {
    const uint32_t *p;
    SPL_HD uint32_t operator()(uint32_t k) const { return p[k]; }
};

// Entry i's ops in the arrays: cigar[c0, c0 + *n_ops).  Offsets that descend or point beyond the arrays' n_ops_total ops are an
// empty CIGAR: whatever the memory holds, no op outside the cigar array is read.
SPL_HD void spl_ops_of(const uint32_t *cig_off, int64_t i, int64_t n_ops_total, uint32_t *c0_out, uint32_t *n_ops)
{
    const uint32_t c0 = cig_off[i];
    uint32_t c1 = cig_off[i + 1];
    if (c1 < c0 || (int64_t)c1 > n_ops_total) c1 = c0;
    *c0_out = c0;
    *n_ops = c1 - c0;
}

// One read of a fragment as a walk takes it: its ops (n_ops = 0: there is no such read), p = POS - 1 + shift, and its FLAG.
struct spl_frag_side {
    uint32_t c0, n_ops;
    int64_t p;
    uint32_t flag;
};

// The arrays: read r of a segment is entry first + r.
struct spl_read_view {
    const int32_t *pos;
    const uint16_t *flag;
    const uint32_t *cig_off, *cigar;
    int64_t n_ops_total; // the cigar array's size
    SPL_HD void ops_of(int64_t i, uint32_t *c0, uint32_t *n_ops) const { spl_ops_of(cig_off, i, n_ops_total, c0, n_ops); }
    // Entry i as a side; -> whether it takes part: takes(flag, POS, n_ops).
    template <class Takes>
    SPL_HD bool side_of(int64_t i, int64_t shift, const Takes &takes, spl_frag_side *out) const
    {
        const int64_t p1 = (int64_t)pos[i];
        out->flag = flag[i];
        ops_of(i, &out->c0, &out->n_ops);
        out->p = p1 - 1 + shift;
        return takes(out->flag, p1, out->n_ops);
    }
};
// (the names the two had where they were first written: the stand-alone sanitizer drivers under tests/hostsim say them)
typedef spl_ops_ptr spl_gene_ops_ptr;
typedef spl_read_view spl_mate_reads;

#endif // SPL_READ_VIEW_H
