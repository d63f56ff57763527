// cprows_check.cpp — host table of compact pricing's row-form tier rule
// (spx_cprows.h; DESIGN.md §4 "Compact pricing"): for a row limit and a list
// length, the chunks a row is read in, the columns in flight, the limit as
// SPX_CPRICE_ROWS resolves it within the rows of AS, and the LDS the slots
// add to a workgroup.  Prints one JSON object per query; tests/
// test_cprice_rows_cpu.py builds it and checks the table.  No device code.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/cprows_check.cpp -o tools/cprows_check
//   tools/cprows_check tier S LIMIT | limit ENV CAP | lds WAVES LIMIT | below LIMIT 0
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../simplex_method_gpu_amd/csrc/spx_cprows.h"

int main(int argc, char** argv) {
    if (argc == 4 && !std::strcmp(argv[1], "tier")) {
        const int nc = spx_cprows::chunks(std::atoi(argv[2]), std::atoi(argv[3]));
        std::printf("{\"nc\": %d, \"depth\": %d}\n", nc, spx_cprows::depth(nc));
        return 0;
    }
    if (argc == 4 && !std::strcmp(argv[1], "limit")) {
        const char* env = std::strcmp(argv[2], "unset") ? argv[2] : nullptr;
        std::printf("{\"limit\": %d}\n", (int)spx_cprows::limit_from(env, std::atoll(argv[3])));
        return 0;
    }
    if (argc == 4 && !std::strcmp(argv[1], "lds")) {
        const int limit = std::atoi(argv[3]);
        std::printf("{\"slot_doubles\": %d, \"lds_bytes\": %zu}\n", spx_cprows::slot_doubles(limit),
                    spx_cprows::lds_bytes(std::atoi(argv[2]), limit));
        return 0;
    }
    if (argc == 4 && !std::strcmp(argv[1], "below")) {
        std::printf("{\"limit\": %d}\n", spx_cprows::tier_below(std::atoi(argv[2])));
        return 0;
    }
    std::fprintf(stderr, "usage: cprows_check tier S LIMIT | limit ENV|unset CAP | lds WAVES LIMIT | below LIMIT 0\n");
    return 2;
}
