// Stand-alone check of the HIP-free K-SAT code (rrrmc.jl_amd/csrc/sat_core.hpp and the first part of host_sat.hpp), meant to be built
// with -fsanitize=address,undefined (tests/test_sat_sanitize_cpu.py): occurrence programs of random and degenerate instances keep every
// index in bounds, sat_delta / sat_row_energy through the program equal the direct clause count, at bit offsets 0, 1, 31 and 33.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../rrrmc.jl_amd/csrc/sat_core.hpp"
#define RRRMC_SAT_HOST_CORE_ONLY
#include "../rrrmc.jl_amd/csrc/host_sat.hpp"

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

struct Inst { int N, Mc, K; std::vector<int32_t> vars; std::vector<int8_t> lits; };

static int bit_at(const std::vector<uint32_t>& sp, int off, int x) { const int b = off + x; return (int)((sp[(size_t)(b >> 5)] >> (b & 31)) & 1u); }

static long long direct_energy(const Inst& I, const std::vector<uint32_t>& sp, int off)
{
    long long n = 0;
    for (int a = 0; a < I.Mc; ++a) {
        bool sat = false;
        for (int k = 0; k < I.K && I.vars[(size_t)(a * I.K + k)] >= 0; ++k)
            sat = sat || bit_at(sp, off, I.vars[(size_t)(a * I.K + k)]) == I.lits[(size_t)(a * I.K + k)];
        n += !sat;
    }
    return n;
}
static int direct_delta(const Inst& I, const std::vector<uint32_t>& sp, int off, int i)
{
    int d = 0;
    for (int a = 0; a < I.Mc; ++a) {
        int nsat = 0; bool has = false, own = false;
        for (int k = 0; k < I.K && I.vars[(size_t)(a * I.K + k)] >= 0; ++k) {
            const int v = I.vars[(size_t)(a * I.K + k)];
            const bool s = bit_at(sp, off, v) == I.lits[(size_t)(a * I.K + k)];
            nsat += s;
            if (v == i) { has = true; own = s; }
        }
        if (!has) continue;
        if (nsat == 0) d -= 1;
        else if (nsat == 1 && own) d += 1;
    }
    return d;
}

// a random instance: clause lengths 1 .. Kmax (ragged) or exactly Kmax; variables drawn from the first `span` ones
static Inst make(int N, int Mc, int Kmax, bool ragged, int span)
{
    Inst I{N, Mc, Kmax, std::vector<int32_t>((size_t)(Mc * Kmax), -1), std::vector<int8_t>((size_t)(Mc * Kmax), 0)};
    for (int a = 0; a < Mc; ++a) {
        int l = ragged ? 1 + (int)(rnd() % (uint64_t)Kmax) : Kmax;
        if (l > span) l = span;
        std::vector<char> used((size_t)span, 0);
        for (int k = 0; k < l;) { const int v = (int)(rnd() % (uint64_t)span); if (!used[(size_t)v]) { used[(size_t)v] = 1; ++k; } }
        int k = 0;
        for (int v = 0; v < span; ++v)
            if (used[(size_t)v]) { I.vars[(size_t)(a * Kmax + k)] = v; I.lits[(size_t)(a * Kmax + k)] = (int8_t)(rnd() & 1); ++k; }
    }
    return I;
}

static void check(const Inst& I)
{
    std::vector<uint32_t> off;
    std::vector<SatEntry> ent;
    int64_t mc = -1;
    char msg[256];
    REQUIRE(sat_build_program(I.N, I.Mc, I.K, I.vars.data(), I.lits.data(), off, ent, &mc, msg, sizeof msg) == 0);
    REQUIRE((int)off.size() == I.N + 1 && off[0] == 0 && off[(size_t)I.N] == ent.size());
    uint32_t deg = 0;
    for (int i = 0; i < I.N; ++i) {
        REQUIRE(off[(size_t)i] <= off[(size_t)i + 1]);
        deg = off[(size_t)i + 1] - off[(size_t)i] > deg ? off[(size_t)i + 1] - off[(size_t)i] : deg;
        for (uint32_t e = off[(size_t)i]; e < off[(size_t)i + 1]; ++e) {
            const int n = (int)((sat_entry_half(ent[e], 0) >> 1) & 7u);
            for (int k = 0; k < 7; ++k) {
                if (k < n) REQUIRE((int)sat_entry_half(ent[e], 1 + k) < I.N && (int)sat_entry_half(ent[e], 1 + k) != i);
                else REQUIRE(sat_entry_half(ent[e], 1 + k) == 0);
            }
        }
    }
    REQUIRE((int64_t)deg == mc);
    long long firsts = 0;
    for (const SatEntry& e : ent) firsts += sat_entry_first(e);
    REQUIRE(firsts == I.Mc);
    const SatTable T{off.data(), ent.data(), I.N};
    const int offs[4] = {0, 1, 31, 33};
    for (int o : offs) {
        // the row sits between other bits: exactly the words the row touches are allocated, so a read past it is a sanitizer error
        std::vector<uint32_t> sp((size_t)((o + I.N + 31) / 32), 0u);
        for (int rep = 0; rep < 3; ++rep) {
            for (uint32_t& w : sp) w = (uint32_t)rnd();
            REQUIRE(sat_row_energy(T, sp.data(), o) == direct_energy(I, sp, o));
            long long E = direct_energy(I, sp, o);
            for (int t = 0; t < 4 * I.N; ++t) {
                const int i = (int)(rnd() % (uint64_t)I.N);
                const int d = sat_delta(T, sp.data(), o, i);
                REQUIRE(d == direct_delta(I, sp, o, i));
                sp[(size_t)((o + i) >> 5)] ^= 1u << ((o + i) & 31);
                E += d;
            }
            REQUIRE(E == direct_energy(I, sp, o));
        }
    }
}

static int refuse(int N, int Mc, int K, std::vector<int32_t> vars, std::vector<int8_t> lits)
{
    std::vector<uint32_t> off;
    std::vector<SatEntry> ent;
    char msg[256];
    return sat_build_program(N, Mc, K, vars.data(), lits.data(), off, ent, nullptr, msg, sizeof msg);
}

int main()
{
    const int shapes[][5] = {{10, 42, 3, 0, 10}, {31, 130, 3, 0, 31}, {33, 264, 5, 0, 33}, {9, 20, 3, 0, 9}, {20, 90, 8, 1, 19}, {1, 3, 1, 0, 1},
                             {64, 200, 8, 1, 64}, {65, 300, 8, 0, 9}, {100, 1, 8, 0, 100}, {40, 500, 2, 1, 3}, {12, 60, 4, 0, 12}};
    for (const auto& s : shapes)
        for (int rep = 0; rep < 3; ++rep) check(make(s[0], s[1], s[2], s[3] != 0, s[4]));
    // the largest variable id and a variable in every clause of a long list
    {
        Inst I{kSatNmax, 300, 2, std::vector<int32_t>(600), std::vector<int8_t>(600)};
        for (int a = 0; a < 300; ++a) { I.vars[(size_t)(2 * a)] = a; I.vars[(size_t)(2 * a + 1)] = kSatNmax - 1; I.lits[(size_t)(2 * a)] = (int8_t)(a & 1); I.lits[(size_t)(2 * a + 1)] = 1; }
        std::vector<uint32_t> off; std::vector<SatEntry> ent; int64_t mc = 0; char msg[256];
        REQUIRE(sat_build_program(I.N, I.Mc, I.K, I.vars.data(), I.lits.data(), off, ent, &mc, msg, sizeof msg) == 0 && mc == 300);
        std::vector<uint32_t> sp((size_t)((I.N + 31) / 32), 0u);
        const SatTable T{off.data(), ent.data(), I.N};
        REQUIRE(sat_row_energy(T, sp.data(), 0) == 150);               // all spins 0: the even clauses hold by their first literal alone
        REQUIRE(sat_delta(T, sp.data(), 0, kSatNmax - 1) == -150 && sat_delta(T, sp.data(), 0, 0) == 1 && sat_delta(T, sp.data(), 0, 1) == -1);
    }
    // refusals: 1 = invalid argument, 3 = beyond the limits
    REQUIRE(refuse(5, 1, 3, {-1, -1, -1}, {0, 0, 0}) == 1);             // an empty clause
    REQUIRE(refuse(5, 1, 3, {0, 5, -1}, {0, 0, 0}) == 1);               // a variable out of range
    REQUIRE(refuse(5, 1, 3, {1, 1, 2}, {0, 0, 0}) == 1);                // a variable twice
    REQUIRE(refuse(5, 1, 3, {2, 1, 3}, {0, 0, 0}) == 1);                // unsorted
    REQUIRE(refuse(5, 1, 3, {1, -1, 3}, {0, 0, 0}) == 1);               // an entry after a pad
    REQUIRE(refuse(5, 1, 3, {1, 2, 3}, {0, 2, 0}) == 1);                // a literal bit above 1
    REQUIRE(refuse(5, 0, 3, {0}, {0}) == 1);
    REQUIRE(refuse(kSatNmax + 1, 1, 1, {0}, {0}) == 3);
    REQUIRE(refuse(20, 1, 9, {0, 1, 2, 3, 4, 5, 6, 7, 8}, {0, 0, 0, 0, 0, 0, 0, 0, 0}) == 3);
    REQUIRE(refuse(20, 1, 9, {0, 1, 2, 3, 4, 5, 6, 7, -1}, {0, 0, 0, 0, 0, 0, 0, 0, 0}) == 0);
    {
        std::vector<int32_t> v((size_t)(kSatDegMax + 1), 0);
        std::vector<int8_t> l((size_t)(kSatDegMax + 1), 0);
        REQUIRE(refuse(2, kSatDegMax + 1, 1, v, l) == 3);               // a variable in 65 536 clauses
        v.pop_back(); l.pop_back();
        REQUIRE(refuse(2, kSatDegMax, 1, v, l) == 0);
    }
    std::printf("all invariants hold\n");
    return 0;
}
