// spl_text_windows.h -- a mapped text cut into windows of whole lines: the one plan of every text source that goes up to the device
// a window at a time (spl_capi.cpp: SamDecode for plain SAM text, GenomeLoad for FASTA).  Host code only, nothing else of the
// project in it: the sanitizer program tests/hostsim/text_windows_asan.cpp includes it alone.
//
// A window is bytes [lo, hi) of the image, at most win_bytes of them, and ends behind the last '\n' among them; the last window
// ends with the text, newline or not.  The sources differ in ONE rule, what becomes of a line that fits no window (its newline
// counted):
//   STOP        (SAM)    the windows end in front of it and the plan says so: the caller declines the file at that line once the
//                        lines before it have been found good.
//   OWN_WINDOW  (FASTA)  it gets a window of its own, which ends behind its newline, or with the text where it has none.
#ifndef SPL_TEXT_WINDOWS_H
#define SPL_TEXT_WINDOWS_H
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

namespace spltext {

struct Window { uint64_t lo, hi; };
enum LongLine { STOP = 0, OWN_WINDOW = 1 };

// Bytes [begin, fsize) of `image` as windows, appended to `out` -> whether a line that fits no window stopped the plan (STOP only).
// The windows tile [begin, end) without gap or overlap; end = fsize unless the plan was stopped.
inline bool cut_windows(const uint8_t *image, uint64_t begin, uint64_t fsize, uint64_t win_bytes, LongLine rule, std::vector<Window> &out)
{
    for (uint64_t lo = begin; lo < fsize;) {
        uint64_t hi = fsize - lo > win_bytes ? lo + win_bytes : fsize;
        if (hi < fsize) {
            const void *nl = memrchr(image + lo, '\n', (size_t)(hi - lo));
            if (!nl) {
                if (rule == STOP) return true;
                nl = memchr(image + hi, '\n', (size_t)(fsize - hi));
            }
            hi = nl ? (uint64_t)((const uint8_t *)nl - image) + 1 : fsize;
        }
        out.push_back(Window{lo, hi});
        lo = hi;
    }
    return false;
}

} // namespace spltext
#endif
