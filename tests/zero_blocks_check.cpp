// Prints, for every beta given on the command line and K = 1 .. 7, the leading zero blocks of the +-J thresholds as the library's host code
// computes them (rrrmc.jl_amd/csrc/host_plan.hpp: zero_blocks, zero_pattern) — one line "beta K pattern zb0 zb1 ..." each; and checks
// zero_pattern_covers on every pair of patterns.  HIP-free: built with g++ by tests/test_zero_blocks_cpu.py.
#include <cstdio>
#include <cstdlib>

#include "../rrrmc.jl_amd/csrc/host_plan.hpp"

using namespace rrrmc;

int main(int argc, char** argv)
{
    const int nblocks = 3;      // sparse_kernels.hpp: kSwBlocks
    for (int a = 1; a < argc; ++a) {
        const double beta = std::strtod(argv[a], nullptr);
        for (int K = 1; K <= 7; ++K) {
            int zb[4] = {0, 0, 0, 0};
            zero_blocks(beta, K, nblocks, zb);
            std::printf("%.17g %d %u", beta, K, zero_pattern(beta, K, nblocks));
            for (int n = 0; n < (K + 1) / 2; ++n) std::printf(" %d", zb[n]);
            std::printf("\n");
        }
    }
    for (uint32_t want = 0; want < 256u; ++want)
        for (uint32_t have = 0; have < 256u; ++have) {
            bool ok = true;
            for (int n = 0; n < 4; ++n) ok = ok && ((have >> (2 * n)) & 3u) <= ((want >> (2 * n)) & 3u);
            if (zero_pattern_covers(want, have) != ok) { std::fprintf(stderr, "zero_pattern_covers(%u, %u) is wrong\n", want, have); return 1; }
        }
    return 0;
}
