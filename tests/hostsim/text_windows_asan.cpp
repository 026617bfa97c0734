// text_windows_asan.cpp -- the window plan of spl_text_windows.h over texts that each lie in a heap block of exactly their size, for a
// build with -fsanitize=address,undefined (the test compiles and runs it): a search for a newline that leaves the text -- in front
// of `begin`'s window, or behind the text's last byte where the last line has no newline -- is a heap-buffer-overflow there.
// Input: the path of a file, a case a line: "rule|begin|win_bytes|<the text's bytes as hex>" (rule 0: stop, 1: a window of its own).
// Output, a line a case: "long_line n lo hi lo hi ...".  Host code only, nothing else of the project; never loaded into Python.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "../../spliser_amd/csrc/spl_text_windows.h"

static int nibble(char c) { return c <= '9' ? c - '0' : c - 'a' + 10; }

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: %s CASES\n", argv[0]); return 2; }
    FILE *fh = fopen(argv[1], "rb");
    if (!fh) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    std::string all;
    char buf[1 << 16];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, fh)) > 0) all.append(buf, got);
    fclose(fh);
    for (size_t at = 0; at < all.size();) {
        size_t nl = all.find('\n', at);
        if (nl == std::string::npos) nl = all.size();
        const std::string line = all.substr(at, nl - at);
        at = nl + 1;
        if (line.empty()) continue;
        std::vector<std::string> parts(1);
        for (char ch : line) {
            if (ch == '|') parts.emplace_back();
            else parts.back() += ch;
        }
        if (parts.size() != 4 || parts[3].size() % 2) { fprintf(stderr, "not a case: %s\n", line.c_str()); return 2; }
        const int rule = atoi(parts[0].c_str());
        const uint64_t begin = strtoull(parts[1].c_str(), nullptr, 10), win_bytes = strtoull(parts[2].c_str(), nullptr, 10);
        const size_t n = parts[3].size() / 2;
        uint8_t *text = (uint8_t *)malloc(n ? n : 1); // (exactly the text: no byte behind it is the program's)
        for (size_t i = 0; i < n; ++i) text[i] = (uint8_t)(nibble(parts[3][2 * i]) << 4 | nibble(parts[3][2 * i + 1]));
        if ((rule != spltext::STOP && rule != spltext::OWN_WINDOW) || begin > n) { fprintf(stderr, "not a case: %s\n", line.c_str()); return 2; }
        std::vector<spltext::Window> windows;
        const bool long_line = spltext::cut_windows(n ? text : nullptr, begin, n, win_bytes, (spltext::LongLine)rule, windows);
        printf("%d %zu", long_line ? 1 : 0, windows.size());
        for (const spltext::Window &w : windows) printf(" %llu %llu", (unsigned long long)w.lo, (unsigned long long)w.hi);
        printf("\n");
        free(text);
    }
    return 0;
}
