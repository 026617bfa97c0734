// spl_bam_aux.h -- the transcript strand an aligner left in a BAM record's aux area (XS:A:+/-; regtools junctions extract -s XS).
// THE definition of how that area is read: the host decoder (bam_reader.cpp), both device extractions (spl_inflate.hip), the
// test hook spl_bam_aux_strand_host and the stand-alone sanitizer program of the tests all call this and nothing else.
#ifndef SPL_BAM_AUX_H
#define SPL_BAM_AUX_H
#include <stdint.h>

#if defined(__HIPCC__)
#define SPL_AUX_HD __host__ __device__
#else
#define SPL_AUX_HD
#endif

// A WALK over the fields of [aux, end), not a search for bytes: a field is a 2-byte tag and a 1-byte type, and its value is stepped
// over by its type (SAM specification 4.2.4) -- A c C one byte, s S two, i I f four, Z H to their NUL, B a subtype byte, a
// uint32 count and count elements of the subtype's size.  So the bytes "XS" inside a Z string or a B array are never taken for a
// tag, and an XS of another type (BWA writes XS:i, the suboptimal score) is stepped over like any field.
// -> the value of the FIRST field XS of type A when that value is '+' or '-'; 0 when it is anything else (regtools: '?'), when
// there is no such field, or when the area cannot be walked to it: an unknown type code (the specification's 'd' included: no
// length is known for it here), a string without its NUL, a value or array that would run past `end`.  No byte at or beyond
// `end` is ever read: every load is preceded by the comparison that allows it.
SPL_AUX_HD inline uint8_t spl_bam_aux_strand(const uint8_t *aux, const uint8_t *end)
{
    const uint8_t *p = aux;
    while (end - p >= 3) {
        const uint8_t t0 = p[0], t1 = p[1], ty = p[2];
        p += 3;
        uint64_t sz = 0;
        switch (ty) {
        case 'A':
            if (t0 == 'X' && t1 == 'S') {
                if (end - p < 1) return 0;
                const uint8_t v = p[0];
                return v == '+' || v == '-' ? v : (uint8_t)0;
            }
            sz = 1;
            break;
        case 'c': case 'C': sz = 1; break;
        case 's': case 'S': sz = 2; break;
        case 'i': case 'I': case 'f': sz = 4; break;
        case 'Z': case 'H': {
            const uint8_t *q = p;
            while (q < end && *q) ++q;
            if (q >= end) return 0; // (no NUL)
            sz = (uint64_t)(q - p) + 1;
            break;
        }
        case 'B': {
            if (end - p < 5) return 0;
            const uint8_t sub = p[0];
            const uint32_t n = (uint32_t)p[1] | ((uint32_t)p[2] << 8) | ((uint32_t)p[3] << 16) | ((uint32_t)p[4] << 24);
            uint64_t es;
            switch (sub) {
            case 'c': case 'C': es = 1; break;
            case 's': case 'S': es = 2; break;
            case 'i': case 'I': case 'f': es = 4; break;
            default: return 0;
            }
            sz = 5 + (uint64_t)n * es;
            break;
        }
        default:
            return 0; // unknown type: where the next field begins is not known
        }
        if ((uint64_t)(end - p) < sz) return 0;
        p += sz;
    }
    return 0;
}

#endif
