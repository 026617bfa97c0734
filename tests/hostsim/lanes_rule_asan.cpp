// lanes_rule_asan.cpp -- the rule of spl_lanes.h (which lane a counting pass takes, which events it waits for) over call sequences
// read from standard input, in a program of its own for AddressSanitizer / UBSan (tests/test_lanes_asan.py).  A line:
//   two tail foreign n_tables n_sets | kind a b c kind a b c ...
// and per line one line out: the plan's 6 + 4 * 12 numbers a call, or "error".  The calls and the plan live in heap blocks of
// exactly their sizes.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../spliser_amd/csrc/spl_lanes.h"

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        const size_t bar = line.find('|');
        if (bar == std::string::npos) continue;
        std::istringstream head(line.substr(0, bar)), tail(line.substr(bar + 1));
        int two = 0, tl = 0, foreign = 0, n_tables = 0, n_sets = 0;
        head >> two >> tl >> foreign >> n_tables >> n_sets;
        std::vector<int32_t> v;
        long long x;
        while (tail >> x) v.push_back((int32_t)x);
        const int64_t n_calls = (int64_t)(v.size() / 4);
        const int64_t stride = 6 + 4 * SPL_LANE_MAX_OPS;
        int32_t *calls = (int32_t *)malloc(sizeof(int32_t) * 4 * (size_t)n_calls + 1);
        int64_t *out = (int64_t *)malloc(sizeof(int64_t) * (size_t)(stride * n_calls) + 1);
        for (int64_t k = 0; k < 4 * n_calls; ++k) calls[k] = v[(size_t)k];
        if (spl_lanes_plan(two, tl, foreign, n_tables, n_sets, n_calls, calls, out) != 0) printf("error\n");
        else {
            for (int64_t k = 0; k < stride * n_calls; ++k) {
                const int64_t row = k % stride, n_ops = out[k - row + 2];
                printf("%lld ", row < 6 + 4 * n_ops ? (long long)out[k] : 0ll); // (behind a call's ops: not written)
            }
            printf("\n");
        }
        free(calls);
        free(out);
    }
    return 0;
}
