// Stand-alone check of the HIP-free Topological Local Entropy code (rrrmc.jl_amd/csrc/tle_core.hpp), meant to be built with
// -fsanitize=address,undefined (tests/test_tle_sanitize_cpu.py): the topology checks accept and refuse what the reference's constructor does
// without reading outside the lists, the neighbour program of random topologies visits exactly the sites of neighbors(X0, j) in its order,
// the level tables are sorted, unique and contain the level of every field pair, and every index of the class-code table stays in bounds.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../rrrmc.jl_amd/csrc/tle_core.hpp"

using namespace rrrmc;

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd()
{
    g_state ^= g_state << 13; g_state ^= g_state >> 7; g_state ^= g_state << 17;
    return g_state;
}
#define REQUIRE(c)                                                                                  \
    do {                                                                                            \
        if (!(c)) { std::printf("FAILED %s (line %d)\n", #c, __LINE__); std::exit(1); }              \
    } while (0)

struct Topo { int Nk; std::vector<int32_t> rowptr, cols; };

static Topo from_lists(const std::vector<std::vector<int>>& nb)
{
    Topo t;
    t.Nk = (int)nb.size();
    t.rowptr.push_back(0);
    for (const auto& n : nb) { for (int j : n) t.cols.push_back(j); t.rowptr.push_back((int32_t)t.cols.size()); }
    return t;
}

static int check(const Topo& t, int64_t* md, char* msg, size_t n)
{
    // exact-size copies, so that a read past either list is a heap overflow the sanitizer reports
    std::vector<int32_t> rp(t.rowptr), cl(t.cols);
    return tle_check_topology(t.Nk, rp.data(), cl.empty() ? nullptr : cl.data(), md, msg, n);
}

static std::vector<std::vector<int>> random_symmetric(int Nk, int percent)
{
    std::vector<std::vector<int>> nb((size_t)Nk);
    for (int i = 0; i < Nk; ++i)
        for (int j = i + 1; j < Nk; ++j)
            if ((int)(rnd() % 100) < percent) { nb[(size_t)i].push_back(j); nb[(size_t)j].push_back(i); }
    for (auto& n : nb)                                        // list order is part of the model: shuffle
        for (size_t a = n.size(); a > 1; --a) std::swap(n[a - 1], n[(size_t)(rnd() % a)]);
    return nb;
}

int main()
{
    char msg[256];
    int64_t md = -1;
    // ---- the constructor's checks ----
    REQUIRE(check(from_lists({{1, 2}, {0}, {0}}), &md, msg, sizeof msg) == 0 && md == 2);
    REQUIRE(check(from_lists({{}, {}, {}}), &md, msg, sizeof msg) == 0 && md == 0);
    REQUIRE(check(from_lists({{1}, {}, {0}}), &md, msg, sizeof msg) == 1 && std::strstr(msg, "not symmetrical"));
    REQUIRE(check(from_lists({{0, 1}, {0}}), &md, msg, sizeof msg) == 1 && std::strstr(msg, "contains itself"));
    REQUIRE(check(from_lists({{1, 2, 1}, {0}, {0}}), &md, msg, sizeof msg) == 1 && std::strstr(msg, "duplicated element 1 in neighb[1]"));
    REQUIRE(check(from_lists({{3}, {0}, {}}), &md, msg, sizeof msg) == 1 && std::strstr(msg, "between 1 and 3"));
    REQUIRE(check(from_lists({{-1}, {}, {}}), &md, msg, sizeof msg) == 1 && std::strstr(msg, "between 1 and 3"));
    { Topo t = from_lists({{1}, {0}}); t.rowptr[0] = 1; REQUIRE(check(t, &md, msg, sizeof msg) == 1); }
    { Topo t = from_lists({{1}, {0}}); t.rowptr[1] = 3; t.rowptr[2] = 2; REQUIRE(check(t, &md, msg, sizeof msg) == 1); }

    // ---- the neighbour program ----
    for (int trial = 0; trial < 40; ++trial) {
        const int Nk = 1 + (int)(rnd() % 24), M = 3 + (int)(rnd() % 7), rows = M + 1;
        const auto nb = random_symmetric(Nk, 10 + (int)(rnd() % 80));
        const Topo t = from_lists(nb);
        REQUIRE(check(t, &md, msg, sizeof msg) == 0);
        std::vector<int32_t> cl(t.cols);
        for (int j = 0; j < Nk * rows; ++j) {
            const int i = j / rows, k = j % rows;
            std::vector<int> ref;
            if (k == 0) {
                for (int q = 1; q <= M; ++q) ref.push_back(j + q);
                for (int i1 : nb[(size_t)i]) for (int q = 0; q < rows; ++q) ref.push_back(i1 * rows + q);
            } else {
                ref.push_back(j - k);
                for (int i1 : nb[(size_t)i]) { ref.push_back(i1 * rows); ref.push_back(i1 * rows + k); }
            }
            REQUIRE(tle_neighbor_count(M, t.rowptr.data(), j) == (int64_t)ref.size());
            std::vector<char> seen((size_t)(Nk * rows), 0);
            for (size_t q = 0; q < ref.size(); ++q) {
                const int y = tle_neighbor(M, cl.data() + t.rowptr[(size_t)i], i, k, (int)q);
                REQUIRE(y == ref[q] && y != j && y >= 0 && y < Nk * rows && !seen[(size_t)y]);
                seen[(size_t)y] = 1;
            }
        }
    }

    // ---- level and code tables ----
    const double gs[] = {0.75, 1.5, 0.0, -0.6, 0.31, 0.7}, ls[] = {0.25, 0.0, 0.8, 0.4, 0.17, 0.7};
    for (int M = 3; M <= 9; ++M)
        for (int c = 0; c < 6; ++c)
            for (int maxdeg : {0, 1, 4, 12}) {
                const double gT = gs[c], lT = ls[c];
                std::vector<double> dE;
                tle_tables(M, gT, lT, maxdeg, dE);
                REQUIRE(!dE.empty() && dE.size() <= (size_t)tle_len1(M) * (size_t)(2 * M * maxdeg + 1));
                for (size_t a = 0; a < dE.size(); ++a) REQUIRE(dE[a] >= 0 && (a == 0 || dE[a] > dE[a - 1]));
                std::vector<uint32_t> code;
                REQUIRE(tle_codes(M, gT, lT, maxdeg, dE, code));
                const int64_t mn = (int64_t)M * maxdeg, nc = 2 * mn + 1;
                REQUIRE(code.size() == (size_t)((2 * M + 1) * nc));
                const int L = (int)dE.size();
                for (int64_t lf1 = -M; lf1 <= M; ++lf1)
                    for (int64_t lf2 = -mn; lf2 <= mn; ++lf2) {
                        const bool centre = (lf1 - M) % 2 == 0, replica = (lf1 == 1 || lf1 == -1) && lf2 >= -maxdeg && lf2 <= maxdeg;
                        const uint32_t cd = code[(size_t)((lf1 + M) * nc + (lf2 + mn))];
                        if (!centre && !replica) continue;
                        REQUIRE(cd != kTleNoCode);
                        const double d = tle_delta0(2 * gT, 2 * lT, (int)lf1, (int)lf2);
                        const int a = (int)(cd & 0x3FFFFFFFu);
                        REQUIRE(a < L && dE[(size_t)a] == fabs(d));
                        REQUIRE(((cd & kTleCodeUp) != 0) == (d > 0) && ((cd & kTleCodeZero) != 0) == (d == 0));
                        for (int s = 0; s < 2; ++s) {
                            const int k = tle_class_of(cd, L, s);
                            REQUIRE(k >= 0 && k < 2 * L && (k >= L) == (d > 0 || (d == 0 && s == 1)));
                        }
                    }
            }
    std::printf("all invariants hold\n");
    return 0;
}
