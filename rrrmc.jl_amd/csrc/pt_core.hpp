// The HIP-free core of the replica exchange between two contexts (rrrmc_exchange_async): the accept rule, the uniform of
// the EXCHANGE stream, and where a replica's verdict sits in the swap mask.  No HIP runtime calls: compiles with hipcc (host and device)
// and with a plain C++ compiler (tests/pt_core_check.cpp runs it under the host sanitizers, with -ffp-contract=off like the library).
//
// Replica r of context a (held at beta_a, energy Ea) and replica r of context b (beta_b, Eb) trade configurations iff
//     x = (beta_a - beta_b) * (Ea - Eb)  >= 0   or   u < det_exp(x)
// with three roundings and no fused multiply-add: the Metropolis rule for the pair's joint Boltzmann weight, written like accept
// (src/RRRMC.jl:39).  A NaN x (an energy that is not finite) is rejected, as `x >= 0 || rand() < exp(x)` rejects it.
#pragma once
#include <stdint.h>

#include "det_math.hpp"
#include "philox.hpp"

namespace rrrmc {

constexpr uint32_t TAG_EXCHANGE = 14;         // counter (lo32(round), hi32(round), replica0 + r, TAG_EXCHANGE): words 0 and 1 make u

// 53-bit uniform in [0, 1) from words 0 and 1 of a Philox block
RRRMC_HD double pt_uniform(const Philox4& o)
{
    return (double)((((uint64_t)o.w[0] << 32) | o.w[1]) >> 11) * 0x1.0p-53;
}

// the uniform of global replica `replica` (replica0 + r) in exchange round `round`
RRRMC_HD double pt_rand(uint32_t k0, uint32_t k1, uint64_t round, uint32_t replica)
{
    return pt_uniform(philox4x32_10((uint32_t)round, (uint32_t)(round >> 32), replica, TAG_EXCHANGE, k0, k1));
}

// x of the rule: every operation rounds once (the library and the check program are built with -ffp-contract=off)
RRRMC_HD double pt_x(double beta_a, double beta_b, double Ea, double Eb)
{
    const double dB = beta_a - beta_b;
    const double dE = Ea - Eb;
    return dB * dE;
}

// the verdict for a given x and uniform
RRRMC_HD bool pt_accept_x(double x, double u) { return x >= 0.0 || u < det_exp(x); }

RRRMC_HD bool pt_accept(double beta_a, double beta_b, double Ea, double Eb, double u) { return pt_accept_x(pt_x(beta_a, beta_b, Ea, Eb), u); }

// the swap mask: one bit per replica, 32 to a word, mask32[pt_mask_words(R)]; bits of replicas >= R are never set
RRRMC_HD int64_t pt_mask_word(int64_t r) { return r >> 5; }
RRRMC_HD uint32_t pt_mask_bit(int64_t r) { return 1u << (uint32_t)(r & 31); }
RRRMC_HD int64_t pt_mask_words(int64_t R) { return (R + 31) >> 5; }
RRRMC_HD bool pt_mask_get(const uint32_t* mask32, int64_t r) { return (mask32[pt_mask_word(r)] & pt_mask_bit(r)) != 0u; }

// an integer model's energy in the model's own units as a double (lv_to_f64; the +-J model has mul = 1, div = 1)
RRRMC_HD double pt_units_to_f64(long long units, long long mul, double div) { return (double)(units * mul) / div; }

}  // namespace rrrmc
