// spl_sam_zhost.h -- compressed SAM text on the host: gzip members inflated one after another (BGZF is a file of many), and the
// inflated text cut into lines with a carried partial line.  Host code only (zlib); used by spl_sam_open's header reader, by the
// host parser of a compressed file (bam_reader.cpp: sam_host_worker), by the device decoder's thread for plain gzip (spl_capi.cpp:
// SamZDecode) and by the sanitizer program tests/hostsim/sam_gz_asan.cpp, which has nothing else of the project in it.
//
// Memory: `Lines` holds one buffer of at most max_line + PIECE bytes -- the longest line the rule takes and the piece inflated
// behind it --, grown as lines ask for it: never the file, never more than two windows of text (max_line is SPL_SAM_WINDOW_BYTES).
#ifndef SPL_SAM_ZHOST_H
#define SPL_SAM_ZHOST_H
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <zlib.h>

#include <algorithm>
#include <vector>

namespace splsamz {

// The members of a gzip file (RFC 1952) from a byte range, as one stream of inflated bytes.  zlib checks every member's CRC32
// and ISIZE.  What follows a member must be another member: anything else is damage (status -1), as is input that ends inside one.
struct Inflater {
    z_stream zs;
    const uint8_t *in = nullptr;
    size_t n_in = 0, at = 0; // the range, and how much of it zlib has been given
    bool open = false, between = true; // (between: at a member's beginning, nothing of it read)
    int status = 0; // 0: more to come; 1: the last member has ended with the input; -1: damaged or truncated
    Inflater() { memset(&zs, 0, sizeof zs); }
    Inflater(const Inflater &) = delete;
    Inflater &operator=(const Inflater &) = delete;
    ~Inflater() { if (open) inflateEnd(&zs); }
    bool begin(const uint8_t *data, size_t n)
    {
        in = data; n_in = n; at = 0; status = 0; between = true;
        if (open) inflateEnd(&zs);
        memset(&zs, 0, sizeof zs);
        open = inflateInit2(&zs, 31) == Z_OK;
        if (!open) status = -1;
        return open;
    }
    size_t consumed() const { return at - zs.avail_in; } // bytes of the range read so far
    // up to cap inflated bytes into dst -> how many (fewer than cap only when status is no longer 0)
    size_t read(uint8_t *dst, size_t cap)
    {
        size_t made = 0;
        while (made < cap && status == 0) {
            if (zs.avail_in == 0 && at < n_in) {
                const size_t give = std::min<size_t>(n_in - at, (size_t)1 << 30);
                zs.next_in = const_cast<Bytef *>(in + at);
                zs.avail_in = (uInt)give;
                at += give;
            }
            if (zs.avail_in == 0) { status = between ? 1 : -1; break; } // (the input ends: at a member's end, or inside one)
            const size_t room = std::min<size_t>(cap - made, (size_t)1 << 30);
            zs.next_out = dst + made;
            zs.avail_out = (uInt)room;
            between = false;
            const int rc = inflate(&zs, Z_NO_FLUSH);
            made += room - zs.avail_out;
            if (rc == Z_STREAM_END) {
                between = true;
                if (zs.avail_in == 0 && at >= n_in) status = 1;
                else if (inflateReset(&zs) != Z_OK) status = -1;
            } else if (rc != Z_OK && !(rc == Z_BUF_ERROR && zs.avail_in == 0 && at < n_in)) status = -1; // (Z_BUF_ERROR with input left to give: no progress yet)
        }
        return made;
    }
};

// The inflated stream's lines, one call each: line(p, stop, has_newline) -> false to stop.  The first `skip` bytes of the stream
// (the header, which spl_sam_open has read) are passed over.  A line is handed out whole whatever its length up to max_line, its
// newline counted; one that is longer is handed out as far as it has been read (more than max_line bytes, has_newline false): the
// caller's rule declines it by its length, and the walk ends there.
struct Lines {
    static constexpr size_t PIECE = (size_t)1 << 20;
    std::vector<uint8_t> buf;
    // -> 0: every line handed out; 1: the caller stopped; -1: the data is damaged (after the lines in front of the damage)
    template <class F> int walk(Inflater &z, uint64_t skip, size_t max_line, F &&line)
    {
        const size_t piece = std::min(PIECE, std::max<size_t>(max_line, 64));
        size_t have = 0; // bytes of an unfinished line at the buffer's front
        for (;;) {
            if (buf.size() < have + piece) buf.resize(std::min(std::max(2 * buf.size(), have + piece), max_line + piece)); // (have <= max_line here: a piece's room at least)
            size_t got = z.read(buf.data() + have, buf.size() - have);
            const int status = z.status;
            if (skip) { // (the header's bytes: nothing is carried yet)
                const size_t drop = (size_t)std::min<uint64_t>(skip, got);
                memmove(buf.data(), buf.data() + drop, got - drop);
                got -= drop;
                skip -= drop;
            }
            const size_t n = have + got;
            size_t p = 0;
            for (size_t from = have; p < n;) { // (the carried bytes hold no newline: the search begins behind them)
                const uint8_t *nl = (const uint8_t *)memchr(buf.data() + from, '\n', n - from);
                if (!nl) break;
                if (!line(buf.data() + p, nl, true)) return 1;
                p = from = (size_t)(nl - buf.data()) + 1;
            }
            have = n - p;
            if (status == -1) return -1;
            if (have > max_line || (status == 1 && have)) { // too long whatever follows / the last line, without a newline
                if (!line(buf.data() + p, buf.data() + n, false)) return 1;
                if (status != 1) return 1; // (the caller did not stop at a line it cannot take: nothing more to hand out)
                have = 0;
            }
            if (status == 1) return 0;
            if (p) memmove(buf.data(), buf.data() + p, have);
        }
    }
};

} // namespace splsamz
#endif
