// aux_strand_asan.cpp -- the aux walk of spl_bam_aux.h over areas cut off at every byte, each in a heap block of exactly its
// size, for a build with -fsanitize=address,undefined (tests/test_aux_strand_host.py compiles and runs it): a read at or beyond
// `end` is a heap-buffer-overflow there.  Arguments: aux areas as hex strings.  Output: one line per area, the walk's answer for
// every cut 0..len as two hex digits each.  Host code only; never loaded into Python.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../spliser_amd/csrc/spl_bam_aux.h"

static int nibble(char c) { return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : -1; }

int main(int argc, char **argv)
{
    for (int a = 1; a < argc; ++a) {
        const size_t len = strlen(argv[a]) / 2;
        uint8_t *full = (uint8_t *)malloc(len ? len : 1);
        for (size_t i = 0; i < len; ++i) {
            const int hi = nibble(argv[a][2 * i]), lo = nibble(argv[a][2 * i + 1]);
            if (hi < 0 || lo < 0) { fprintf(stderr, "not hex: %s\n", argv[a]); return 2; }
            full[i] = (uint8_t)(hi * 16 + lo);
        }
        for (size_t cut = 0; cut <= len; ++cut) {
            uint8_t *block = (uint8_t *)malloc(cut ? cut : 1);
            uint8_t *part = cut ? block : block + 1; // (cut = 0: the empty area lies at the block's end, any read of it is beyond)
            if (cut) memcpy(part, full, cut);
            printf("%02x", (unsigned)spl_bam_aux_strand(part, part + cut));
            free(block);
        }
        printf("\n");
        free(full);
    }
    return 0;
}
