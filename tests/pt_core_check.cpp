// Stand-alone host program over rrrmc.jl_amd/csrc/pt_core.hpp (the HIP-free core of the replica exchange) and det_math.hpp's host det_exp:
// built with -ffp-contract=off -fsanitize=address,undefined by tests/test_exchange_cpu.py and run directly.  It reads a table of cases
// from the file named on its command line and prints what the library's rule gives for each; the test feeds the same table to the numpy
// restatement (tests/exchange_reference.py) and compares the two outputs line by line.  Numbers travel as C99 hexadecimal floats.
//
//   A beta_a beta_b Ea Eb seed round replica   ->  A <x> <u> <verdict>          the whole rule: x, the EXCHANGE stream's uniform, the verdict
//   X x u                                      ->  X <verdict>                  the verdict for a given x and uniform
//   M R beta_a beta_b seed round               ->  M <words> <w0> <w1> ...      the mask words of R replicas with the energies of table_energy()
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../rrrmc.jl_amd/csrc/det_math.hpp"
#include "../rrrmc.jl_amd/csrc/pt_core.hpp"

using namespace rrrmc;

// the energies of the mask cases: small integers of both signs, so that x takes both signs and zero (the test computes the same)
static double table_energy(int which, int64_t r) { return which == 0 ? (double)((r * 7) % 13 - 6) : (double)((r * 5) % 11 - 5); }

int main(int argc, char** argv)
{
    if (argc != 2) { std::fprintf(stderr, "usage: %s cases.txt\n", argv[0]); return 2; }
    std::FILE* f = std::fopen(argv[1], "r");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    char line[512];
    int n = 0;
    while (std::fgets(line, sizeof line, f)) {
        char kind = 0;
        char a[5][64];
        uint64_t seed = 0, round = 0;
        long long rep = 0;
        if (std::sscanf(line, " %c", &kind) != 1) continue;
        if (kind == 'A') {
            if (std::sscanf(line, " %*c %63s %63s %63s %63s %" SCNu64 " %" SCNu64 " %lld", a[0], a[1], a[2], a[3], &seed, &round, &rep) != 7) { std::fclose(f); return 3; }
            const double ba = std::strtod(a[0], nullptr), bb = std::strtod(a[1], nullptr), Ea = std::strtod(a[2], nullptr), Eb = std::strtod(a[3], nullptr);
            const double x = pt_x(ba, bb, Ea, Eb);
            const double u = pt_rand((uint32_t)seed, (uint32_t)(seed >> 32), round, (uint32_t)rep);
            std::printf("A %a %a %d\n", x, u, pt_accept(ba, bb, Ea, Eb, u) ? 1 : 0);
        } else if (kind == 'X') {
            if (std::sscanf(line, " %*c %63s %63s", a[0], a[1]) != 2) { std::fclose(f); return 3; }
            std::printf("X %d\n", pt_accept_x(std::strtod(a[0], nullptr), std::strtod(a[1], nullptr)) ? 1 : 0);
        } else if (kind == 'M') {
            long long R = 0;
            if (std::sscanf(line, " %*c %lld %63s %63s %" SCNu64 " %" SCNu64, &R, a[0], a[1], &seed, &round) != 5 || R < 1) { std::fclose(f); return 3; }
            const double ba = std::strtod(a[0], nullptr), bb = std::strtod(a[1], nullptr);
            std::vector<uint32_t> m((size_t)pt_mask_words(R), 0u);
            for (int64_t r = 0; r < R; ++r)
                if (pt_accept(ba, bb, table_energy(0, r), table_energy(1, r), pt_rand((uint32_t)seed, (uint32_t)(seed >> 32), round, (uint32_t)r)))
                    m[(size_t)pt_mask_word(r)] |= pt_mask_bit(r);
            int64_t cnt = 0;
            for (int64_t r = 0; r < R; ++r) cnt += pt_mask_get(m.data(), r) ? 1 : 0;
            std::printf("M %zu", m.size());
            for (uint32_t w : m) std::printf(" %08x", w);
            std::printf(" %lld\n", (long long)cnt);
        } else {
            std::fclose(f);
            return 3;
        }
        ++n;
    }
    std::fclose(f);
    std::printf("done %d\n", n);
    return 0;
}
