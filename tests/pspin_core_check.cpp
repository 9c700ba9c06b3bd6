// Stand-alone check of the HIP-free 3-spin code (rrrmc.jl_amd/csrc/pspin_core.hpp and the first part of host_pspin.hpp), meant to be
// built with -fsanitize=address,undefined (tests/test_pspin3_sanitize_cpu.py): generated tables are partitions layer by layer and pass
// the validation, which refuses every kind of malformed table and every size beyond the limits; pspin_delta / pspin_energy over the
// 16-bit table equal the direct sum over the triples, at bit offsets 0, 1, 31 and 33 and at the limits N = 65 535, K = 16.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../rrrmc.jl_amd/csrc/philox.hpp"
#include "../rrrmc.jl_amd/csrc/pspin_core.hpp"
#define RRRMC_PSPIN_HOST_CORE_ONLY
#include "../rrrmc.jl_amd/csrc/host_pspin.hpp"

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

static int bit_at(const std::vector<uint32_t>& sp, int off, int x) { const int b = off + x; return (int)((sp[(size_t)(b >> 5)] >> (b & 31)) & 1u); }

// −Σ over the layers' triples of σσσ: the triple of (i, k) is counted where i is its smallest site
static long long direct_energy(int N, int K, const std::vector<int32_t>& A, const std::vector<uint32_t>& sp, int off)
{
    long long E = 0;
    for (int i = 0; i < N; ++i)
        for (int k = 0; k < K; ++k) {
            const int y = A[(size_t)i * 2 * K + 2 * k], z = A[(size_t)i * 2 * K + 2 * k + 1];
            if (i < y && i < z) E -= (2 * bit_at(sp, off, i) - 1) * (2 * bit_at(sp, off, y) - 1) * (2 * bit_at(sp, off, z) - 1);
        }
    return E;
}
static int direct_delta(int K, const std::vector<int32_t>& A, const std::vector<uint32_t>& sp, int off, int i)
{
    int d = 0;
    for (int k = 0; k < K; ++k)
        d += (2 * bit_at(sp, off, A[(size_t)i * 2 * K + 2 * k]) - 1) * (2 * bit_at(sp, off, A[(size_t)i * 2 * K + 2 * k + 1]) - 1);
    return 2 * (2 * bit_at(sp, off, i) - 1) * d;
}

static void check_instance(int N, int K, uint64_t seed, int nconf)
{
    char msg[256];
    REQUIRE(pspin_check_size(N, K, msg, sizeof msg) == 0);
    std::vector<int32_t> A((size_t)N * 2 * K, -1);
    pspin_generate(N, K, seed, A.data());
    // every layer is a partition: each site is the partner of exactly two others, and the triples close
    for (int k = 0; k < K; ++k) {
        std::vector<int> seen((size_t)N, 0);
        for (int i = 0; i < N; ++i) {
            const int y = A[(size_t)i * 2 * K + 2 * k], z = A[(size_t)i * 2 * K + 2 * k + 1];
            REQUIRE(y >= 0 && y < N && z >= 0 && z < N && y != z && y != i && z != i);
            seen[(size_t)y] += 1; seen[(size_t)z] += 1;
            const int32_t* ay = &A[(size_t)y * 2 * K + 2 * k];
            REQUIRE((ay[0] == i || ay[1] == i) && (ay[0] == z || ay[1] == z));
        }
        for (int i = 0; i < N; ++i) REQUIRE(seen[(size_t)i] == 2);
    }
    std::vector<uint16_t> tab((size_t)N * 2 * K);
    REQUIRE(pspin_validate(N, K, A.data(), tab.data(), msg, sizeof msg) == 0);
    const PspinTable T{tab.data(), N, K};
    const int offs[4] = {0, 1, 31, 33};
    for (int c = 0; c < nconf; ++c) {
        const int off = offs[c % 4];
        std::vector<uint32_t> sp((size_t)((off + N + 31) / 32));
        for (uint32_t& w : sp) w = (uint32_t)rnd();
        const PspinRowBits bits{sp.data(), off};
        const long long E = pspin_energy(T, bits);
        REQUIRE(E == direct_energy(N, K, A, sp, off));
        for (int q = 0; q < 64; ++q) {
            const int i = (int)(rnd() % (uint64_t)N);
            const int d = pspin_delta(T, i, bits);
            REQUIRE(d == direct_delta(K, A, sp, off, i));
            REQUIRE(d % 4 == (K % 2 ? 2 : 0) || d % 4 == (K % 2 ? -2 : 0));          // allΔE: multiples of 4 (K even), 2 mod 4 (K odd)
            const int b = off + i;
            sp[(size_t)(b >> 5)] ^= 1u << (b & 31);
            REQUIRE(pspin_energy(T, bits) == E + d);                              // ΔE is the change of the energy
            REQUIRE(pspin_delta(T, i, bits) == -d);
            sp[(size_t)(b >> 5)] ^= 1u << (b & 31);
        }
    }
}

static void check_refusals()
{
    char msg[256];
    REQUIRE(pspin_check_size(0, 1, msg, sizeof msg) == 1);
    REQUIRE(pspin_check_size(4, 1, msg, sizeof msg) == 3);
    REQUIRE(pspin_check_size(65538, 1, msg, sizeof msg) == 3);
    REQUIRE(pspin_check_size(65535, 16, msg, sizeof msg) == 0);
    REQUIRE(pspin_check_size(6, 17, msg, sizeof msg) == 3);
    REQUIRE(pspin_check_size(6, 0, msg, sizeof msg) == 3);
    const int N = 9, K = 2;
    std::vector<int32_t> good((size_t)N * 2 * K);
    pspin_generate(N, K, 5, good.data());
    REQUIRE(pspin_validate(N, K, good.data(), nullptr, msg, sizeof msg) == 0);
    auto bad = [&](size_t e, int32_t v) {
        std::vector<int32_t> A = good;
        A[e] = v;
        return pspin_validate(N, K, A.data(), nullptr, msg, sizeof msg);
    };
    REQUIRE(bad(0, -1) == 1);                                                     // out of range, below
    REQUIRE(bad(3, N) == 1);                                                      // out of range, above
    REQUIRE(bad(0, good[1]) == 1);                                                // the two partners equal
    REQUIRE(bad(0, 0) == 1);                                                      // a partner is the site itself
    {                                                                             // a well-formed slot that the partners do not return
        std::vector<int32_t> A = good;
        int32_t other = 1;
        while (other == A[0] || other == A[1]) ++other;
        A[0] = other;
        REQUIRE(pspin_validate(N, K, A.data(), nullptr, msg, sizeof msg) == 1);
        REQUIRE(std::strstr(msg, "not consistent") != nullptr);
    }
    {                                                                             // one layer given twice: every pair counts twice, and is consistent
        std::vector<int32_t> A((size_t)N * 4);
        std::vector<int32_t> one((size_t)N * 2);
        pspin_generate(N, 1, 11, one.data());
        for (int i = 0; i < N; ++i) { A[(size_t)i * 4] = A[(size_t)i * 4 + 2] = one[(size_t)i * 2]; A[(size_t)i * 4 + 1] = A[(size_t)i * 4 + 3] = one[(size_t)i * 2 + 1]; }
        REQUIRE(pspin_validate(N, 2, A.data(), nullptr, msg, sizeof msg) == 0);
        A[2] = A[1]; A[3] = A[0];                                                 // the partners swapped inside a slot: the same pair, still consistent
        REQUIRE(pspin_validate(N, 2, A.data(), nullptr, msg, sizeof msg) == 0);
    }
}

int main()
{
    check_refusals();
    const int shapes[][2] = {{3, 1}, {3, 2}, {6, 3}, {33, 4}, {96, 5}, {192, 16}, {999, 7}};
    for (const auto& s : shapes) check_instance(s[0], s[1], 1000 + (uint64_t)s[0], 8);
    check_instance(65535, 16, 7, 1);                                              // both limits at once
    {                                                                             // equal seeds give equal tables, unequal seeds differing ones
        std::vector<int32_t> a(96 * 10), b(96 * 10), c(96 * 10);
        pspin_generate(96, 5, 42, a.data()); pspin_generate(96, 5, 42, b.data()); pspin_generate(96, 5, 43, c.data());
        REQUIRE(a == b && a != c);
    }
    std::printf("all invariants hold\n");
    return 0;
}
