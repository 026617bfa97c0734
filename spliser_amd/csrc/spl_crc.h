// CRC32 (IEEE 802.3, reflected: what a BGZF block's trailer holds, RFC 1952 §8): the arithmetic the wave kernel's tables are made
// with (spl_crc_wave.h).  The CRC register is linear in the data over GF(2): the register of a stretch followed by m zero bytes is
// the register times x^(8m) modulo the polynomial (mulmod; zlib's crc32_combine does the same on the host).
//
// Shared by the kernel (spl_inflate.hip) and by the host build the CPU tests check against zlib (tests/hostsim/crc_host.cpp).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SPL_CRC_FN __host__ __device__ inline
#else
#define SPL_CRC_FN inline
#endif

namespace splcrc {

constexpr uint32_t POLY = 0xEDB88320u;
constexpr int N_X2N = 24; // x^(2^k), k < 24: exponents (bits of payload) below 2^24 -- a BGZF payload has 2^19 at most

// table[0][b] of the byte-wise method
SPL_CRC_FN uint32_t byte_entry(uint32_t b)
{
    uint32_t c = b;
    for (int k = 0; k < 8; ++k) c = (c & 1u) ? (POLY ^ (c >> 1)) : (c >> 1);
    return c;
}

// a · b modulo the polynomial; bit 31 is the coefficient of x^0 (the reflected order the register is kept in)
SPL_CRC_FN uint32_t mulmod(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
    for (int i = 0; i < 32; ++i) {
        p ^= b & (0u - (a >> 31));
        a <<= 1;
        b = (b >> 1) ^ (POLY & (0u - (b & 1u)));
    }
    return p;
}

// x^(2^k): k squarings of x
SPL_CRC_FN uint32_t x2n_entry(uint32_t k)
{
    uint32_t v = 0x40000000u; // x^1
    for (uint32_t j = 0; j < k; ++j) v = mulmod(v, v);
    return v;
}

} // namespace splcrc
