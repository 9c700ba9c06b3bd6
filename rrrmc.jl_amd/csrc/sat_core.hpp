// The HIP-free core of random K-SAT (src/graphs/SAT.jl): the per-variable occurrence program and the clause walk over it.  Compiles with
// hipcc (host and device) and with a plain C++ compiler (tests/sat_core_check.cpp runs it under the host sanitizers).
//
// GraphSAT: N variables, Mc clauses; clause a holds len_a <= 8 distinct variables A[a] with literal bits J[a]; literal k is satisfied iff
// s[A[a][k]] == J[a][k] (SAT.jl:207); energy = the number of clauses without a satisfied literal.  delta_energy(i) = #(clauses that i alone
// satisfies) − #(unsatisfied clauses containing i): the reference's ClauseCache (S, I, lfields; SAT.jl:189-320) is a pure function of the
// configuration — I[a][1] is only read when S[a] == 1, where it is the unique satisfier — so nothing is cached here.
//
// Occurrence program.  A CSR over T[i] (the clauses containing i, in clause order): off[i] .. off[i + 1] index 16-byte entries, one per
// occurrence: four 32-bit words holding eight halfwords (halfword k = bits 16 (k & 1) .. of word k >> 1), copied BY VALUE before they are
// decoded so that one entry is one 128-bit load (in the gfx950 build: global_load_dwordx4 per lane in sat_wave_kernel and
// sat_standard_kernel, s_load_dwordx4 where the address is provably uniform; profiles/r12/sat.md):
//   halfword 0     bit 0      the polarity J of i's own literal
//                  bits 1-3   the number of OTHER literals of the clause (0 .. 7)
//                  bits 4-10  their polarities
//                  bit 11     i is the clause's first (smallest) variable: the occurrence that counts the clause in `energy`
//   halfwords 1-7  the other variables (16 bits: N <= 65 535), unused ones 0
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define RRRMC_SAT_HD __host__ __device__
#else
#define RRRMC_SAT_HD
#endif

namespace rrrmc {

constexpr int kSatNmax = 65535;                             // variables (16-bit ids in an entry)
constexpr int kSatLenMax = 8;                               // literals of one clause
constexpr long long kSatMcMax = 1ll << 20;                  // clauses
constexpr int kSatDegMax = 65535;                           // |T[i]|

struct alignas(16) SatEntry { uint32_t w[4]; };
RRRMC_SAT_HD inline unsigned sat_entry_half(const SatEntry& e, int k) { return (e.w[k >> 1] >> (16 * (k & 1))) & 0xffffu; }
RRRMC_SAT_HD inline void sat_entry_set_half(SatEntry& e, int k, unsigned v) { e.w[k >> 1] |= (v & 0xffffu) << (16 * (k & 1)); }

struct SatTable {
    const uint32_t* off;                                    // [N + 1]
    const SatEntry* ent;                                    // [off[N]]
    int N;
};

// a replica-contiguous bit row that starts at bit `off` of `sp`
struct SatRowBits {
    const uint32_t* sp; int off;
    RRRMC_SAT_HD int operator()(int x) const { const int b = off + x; return (int)((sp[b >> 5] >> (b & 31)) & 1u); }
};

// one occurrence of a variable whose spin bit is si: +1 when it alone satisfies the clause, −1 when the clause is unsatisfied, else 0
template <class Bits>
RRRMC_SAT_HD inline int sat_entry_term(const SatEntry e, int si, const Bits& bit)
{
    const unsigned h = sat_entry_half(e, 0);
    const int n = (int)((h >> 1) & 7u);
    bool other = false;
    for (int k = 0; k < 7; ++k)
        if (k < n) other = other || bit((int)sat_entry_half(e, 1 + k)) == (int)((h >> (4 + k)) & 1u);
    if (other) return 0;
    return si == (int)(h & 1u) ? 1 : -1;
}
RRRMC_SAT_HD inline bool sat_entry_first(const SatEntry& e) { return ((e.w[0] >> 11) & 1u) != 0; }

// delta_energy(X, C, i) (SAT.jl:314-320, = −lfields[i]) from the configuration only
template <class Bits>
RRRMC_SAT_HD inline int sat_delta_bits(const SatTable& T, int i, const Bits& bit)
{
    const int si = bit(i);
    int d = 0;
    for (uint32_t e = T.off[i]; e < T.off[i + 1]; ++e) { const SatEntry en = T.ent[e]; d += sat_entry_term(en, si, bit); }
    return d;
}
// the unsatisfied clauses whose first variable is i
template <class Bits>
RRRMC_SAT_HD inline int sat_first_unsat(const SatTable& T, int i, const Bits& bit)
{
    const int si = bit(i);
    int n = 0;
    for (uint32_t e = T.off[i]; e < T.off[i + 1]; ++e) {
        const SatEntry en = T.ent[e];
        n += (sat_entry_first(en) && sat_entry_term(en, si, bit) < 0) ? 1 : 0;
    }
    return n;
}
// energy(X, C) (SAT.jl:189-236): the number of clauses without a satisfied literal
template <class Bits>
RRRMC_SAT_HD inline long long sat_energy_bits(const SatTable& T, const Bits& bit)
{
    long long n = 0;
    for (int i = 0; i < T.N; ++i) n += sat_first_unsat(T, i, bit);
    return n;
}

// the two over a bit row that may start at any bit offset: slice k of an ensemble is the row at k Nk of the slice-major copy
RRRMC_SAT_HD inline int sat_delta(const SatTable& T, const uint32_t* spins, int bit_offset, int i)
{
    return sat_delta_bits(T, i, SatRowBits{spins, bit_offset});
}
RRRMC_SAT_HD inline long long sat_row_energy(const SatTable& T, const uint32_t* spins, int bit_offset)
{
    return sat_energy_bits(T, SatRowBits{spins, bit_offset});
}

}  // namespace rrrmc
