// Test-only host build of spliser_amd/csrc/spl_crc.h (the arithmetic behind spl_crc32_wave_kernel's tables): tests/test_crc_host.py
// holds it against zlib.
#include "../../spliser_amd/csrc/spl_crc.h"

extern "C" uint32_t crc_x2n(int k) { return splcrc::x2n_entry((uint32_t)k); }
extern "C" uint32_t crc_mulmod(uint32_t a, uint32_t b) { return splcrc::mulmod(a, b); }
