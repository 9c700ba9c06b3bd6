// The HIP-free core of the regular 3-spin model (src/graphs/PSpin3.jl): the partner table, delta_energy and energy over it, the limits and
// the validation of an uploaded table.  Compiles with hipcc (host and device) and with a plain C++ compiler (tests/pspin_core_check.cpp
// runs it under the host sanitizers).
//
// GraphPSpin3(N, K): N spins, 3 | N; each of the K layers is a partition of the sites into N / 3 triples, all couplings +1.  A[i] holds
// 2K site ids: slots 2k, 2k + 1 (0-based) are the two partners of i in layer k (PSpin3.jl:32-43).
//   energy          = −Σ_triples σ σ σ                                   (an Int, PSpin3.jl:62-93)
//   delta_energy(i) = 2 σ_i Σ_k σ_y σ_z = 2 (2c − K),  c = #{k : s_i ⊻ s_y ⊻ s_z == 1}      (σ_i σ_y σ_z = +1 iff an odd number of the bits is set)
// The reference reads ΔE from LocalFields{Int} (lfields[i] = −ΔE(i), PSpin3.jl:86, :147-155), an exact integer function of the
// configuration: nothing is cached here, ΔE is recomputed from the spins and stays bit-identical.  A pair that two layers
// share counts twice; K even has moves with ΔE = 0.
//
// The table on the device: 16-bit ids, [N][2K]; the row of a site is K 32-bit words (partner y in the low half, z in the high half).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#if defined(__HIPCC__)
#define RRRMC_PSPIN_HD __host__ __device__
#else
#define RRRMC_PSPIN_HD
#endif

namespace rrrmc {

constexpr int kPspinNmax = 65535;                           // spins (16-bit ids)
constexpr int kPspinKmax = 16;                              // layers

// the wrapper of a PSpin3 model id: 0 the graph itself, 1 GraphAddFields(h, g), 2 GraphAddSubFields(h, g); -1 for every other model.
// A lookup of its own: the tables of af_models.hpp / ens_models.hpp / mixed_models.hpp keep their form.
constexpr int32_t kPspinModelBase = 105;                    // RRRMC_MODEL_PSPIN3, _PSPIN3_AF, _PSPIN3_ASF (include/rrrmc_hip.h)
constexpr int32_t pspin_wrap(int32_t model) { return model >= kPspinModelBase && model <= kPspinModelBase + 2 ? model - kPspinModelBase : -1; }
constexpr int32_t pspin_model(int32_t wrap) { return wrap >= 0 && wrap <= 2 ? kPspinModelBase + wrap : 0; }

struct PspinTable {
    const uint16_t* A;                                      // [N][2K]
    int N, K;
};

// a replica-contiguous bit row that starts at bit `off` of `sp`
struct PspinRowBits {
    const uint32_t* sp; int off;
    RRRMC_PSPIN_HD int operator()(int x) const { const int b = off + x; return (int)((sp[b >> 5] >> (b & 31)) & 1u); }
};

// c of site i: the layers whose triple has the product +1
template <class Bits>
RRRMC_PSPIN_HD inline int pspin_count(const PspinTable& T, int i, const Bits& bit)
{
    const uint16_t* a = T.A + (size_t)i * 2 * T.K;
    const int si = bit(i);
    int c = 0;
    for (int k = 0; k < T.K; ++k) c += si ^ bit((int)a[2 * k]) ^ bit((int)a[2 * k + 1]);
    return c;
}
// delta_energy(X, C, i) (PSpin3.jl:147-155, = −lfields[i]) from the configuration only
template <class Bits>
RRRMC_PSPIN_HD inline int pspin_delta(const PspinTable& T, int i, const Bits& bit) { return 2 * (2 * pspin_count(T, i, bit) - T.K); }
// energy(X, C) (PSpin3.jl:62-93): every triple is met by its three sites
template <class Bits>
RRRMC_PSPIN_HD inline long long pspin_energy(const PspinTable& T, const Bits& bit)
{
    long long n = 0;
    for (int i = 0; i < T.N; ++i) n -= 2 * pspin_count(T, i, bit) - T.K;
    return n / 3;
}

// (N, K) against the limits: 0, or 1 (invalid argument) / 3 (beyond the kernels' limits) with a message
inline int pspin_check_size(int64_t N, int64_t K, char* msg, size_t msg_len)
{
    if (N < 1) { snprintf(msg, msg_len, "GraphPSpin3: N must be >= 1, given: %lld", (long long)N); return 1; }
    if (N % 3 != 0) { snprintf(msg, msg_len, "N must be divisible by 3, given: %lld", (long long)N); return 3; }          // PSpin3.jl:24
    if (N > kPspinNmax) { snprintf(msg, msg_len, "N = %lld: the 3-spin kernels cover N <= %d (16-bit site ids)", (long long)N, kPspinNmax); return 3; }
    if (K < 1 || K > kPspinKmax) { snprintf(msg, msg_len, "K = %lld: the 3-spin kernels cover 1 <= K <= %d", (long long)K, kPspinKmax); return 3; }          // (K >= 1: PSpin3.jl:22)
    return 0;
}

// An uploaded table A [N][2K] (0-based): every id in range; the two partners of a slot distinct and different from i; consistent — for
// slot k of i = (y, z), y's list holds the pair {i, z} and z's list the pair {i, y} as often as i's list holds {y, z} —, which makes
// 3 | Σ lf (PSpin3.jl:88).  Fills the 16-bit table when `out` is given.  Returns as pspin_check_size.
inline int pspin_validate(int64_t N, int64_t K, const int32_t* A, uint16_t* out, char* msg, size_t msg_len)
{
    const int rcs = pspin_check_size(N, K, msg, msg_len);
    if (rcs) return rcs;
    const int64_t K2 = 2 * K;
    for (int64_t i = 0; i < N; ++i)
        for (int64_t k = 0; k < K; ++k) {
            const int32_t y = A[i * K2 + 2 * k], z = A[i * K2 + 2 * k + 1];
            if (y < 0 || y >= N || z < 0 || z >= N) {
                snprintf(msg, msg_len, "GraphPSpin3: site %lld, layer %lld: partner (%d, %d) out of range (N = %lld)", (long long)i, (long long)k, y, z, (long long)N);
                return 1;
            }
            if (y == z || y == i || z == i) {
                snprintf(msg, msg_len, "GraphPSpin3: site %lld, layer %lld: the triple (%lld, %d, %d) repeats a site", (long long)i, (long long)k, (long long)i, y, z);
                return 1;
            }
        }
    // how often the list of site a holds the unordered pair {b, c}
    auto count = [&](int64_t a, int32_t b, int32_t c) {
        int n = 0;
        for (int64_t k = 0; k < K; ++k) {
            const int32_t p = A[a * K2 + 2 * k], q = A[a * K2 + 2 * k + 1];
            n += ((p == b && q == c) || (p == c && q == b)) ? 1 : 0;
        }
        return n;
    };
    for (int64_t i = 0; i < N; ++i)
        for (int64_t k = 0; k < K; ++k) {
            const int32_t y = A[i * K2 + 2 * k], z = A[i * K2 + 2 * k + 1];
            const int n = count(i, y, z);
            if (count(y, (int32_t)i, z) != n || count(z, (int32_t)i, y) != n) {
                snprintf(msg, msg_len, "GraphPSpin3: the table is not consistent: site %lld lists the triple (%lld, %d, %d) %d time(s), its partners do not",
                         (long long)i, (long long)i, y, z, n);
                return 1;
            }
        }
    if (out)
        for (int64_t e = 0; e < N * K2; ++e) out[e] = (uint16_t)A[e];
    return 0;
}

}  // namespace rrrmc
