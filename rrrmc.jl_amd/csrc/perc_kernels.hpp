// gfx950 kernels for the binary perceptron (src/graphs/PercStep.jl, PercLinear.jl): N (odd) binary synapses trained on P random patterns ξ.
// GraphPercStep{Int}: energy = the number of misclassified patterns (PercStep.jl:88-111); GraphPercLinear{Float64}: energy =
// 2 Σ_a ((−Δ_a − 1) ÷ 2 + 1) / √N over the patterns with Δ_a < 0 (PercLinear.jl:88-115).  Used as the slice graph of the Robust Ensemble and
// the Local Entropy ensemble (re_kernels.hpp, le_kernels.hpp: GraphPercStepRE / GraphPercLinearRE / GraphPercStepLE / GraphPercLinearLE,
// src/REAliases.jl, src/LEAliases.jl) and, stand-alone, under standardMC (perc_standard_kernel below).
//
// State.  Per chain (and per slice of an ensemble): the stabilities Δs[a] = N − 2 Σ_i (s_i ⊻ ξ[a,i]) as int16 (|Δ| <= N <= 32 767)
// and the two boundary sets of the reference's Stabilities, p and m, as P-bit masks.  The reference keeps p and m as ArraySets
// (src/ArraySets.jl), whose member ORDER depends on the history of push! / delete!.  Nothing ever reads that order: delta_energy only sums
// an integer per member (PercStep.jl:163-168, PercLinear.jl:167-172), integer addition commutes, and update_cache! only tests and changes
// membership (PercStep.jl:125-140, PercLinear.jl:129-141).  Membership itself is a function of Δ alone — p = {Δ == 1}; m = {Δ == −1} (step)
// or {Δ < 0} (linear) — which the update rules keep: every branch of update_cache! moves a pattern into exactly the set its new Δ names
// (N is odd, so Δ is odd and never 0).  So a mask per set gives the same delta_energy bit for bit (tests/test_perc_cpu.py checks the masks
// against literal ArraySets over a random walk), and Δs and the masks are pure functions of the configuration: flipping a spin and flipping
// it back restores them, which is why the direct branch of rrrMC updates a slice only for an accepted move.  The reference's ξsi / last_move
// copy of one pattern column is an optimisation of its BitMatrix access and has no counterpart here.
//
// Patterns.  Column-major pcol[i][w] (bit b of word w = ξ[64 w + b, i]) for delta_energy and update_cache!, row-major prow[a][...] (the ξv
// chunks of the ABI as 32-bit words) for energy — the two representations of gen_ξ (PercStep.jl:19-29).
//
// delta_energy(move i, spin bit s): col = pcol[i] ⊻ s;  step: popc(p & ~col) − popc(m & col);  linear: popc(p & ~col) + popc(m & ~col) −
// popc(m & col), times 2 / √N.  update_cache! after the flip (new spin bit s): Δ_a += 2 − 4 col_a for every a, then the masks from the new Δ.
// WAVE = false: a loop of one thread.  WAVE = true: the workgroup is one wavefront whose 64 lanes ALL run the chain with identical values
// (wave-uniform control flow); lane l owns pattern 64 w + l of word w, and the two mask words are the wavefront's ballots.  Integer
// arithmetic only: both builds give the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rrr_kernels.hpp"   // sbit / sflip, kRrrThreads, site_of, rand53, det_exp

namespace rrrmc {

constexpr int kPercNmax = 32767;                            // synapses of one perceptron (int16 stabilities)
constexpr int kPercPmax = 4096;                             // patterns (64 mask words)

struct PercParams {
    const uint64_t* col;                                    // [Nk][PW]
    const uint32_t* row;                                    // [P][RW]      RW = 2 ceil(Nk / 64); bits beyond Nk are 0
    int16_t* ds;                                            // [R][rows][64 PW]   Δs (entries a >= P stay 0)
    uint64_t* pm; uint64_t* mm;                             // [R][rows][PW]      the sets p and m
    int P, PW, RW, rows;
    double sN;                                              // sqrt(Nk) (PercLinear.jl:59)
};

struct PercView {                                           // one chain's state (HBM/L2, or LDS in the WAVE build)
    const uint64_t* col;
    int16_t* ds; uint64_t* pm; uint64_t* mm;
    int P, PW;
    double sN;
};

__device__ __forceinline__ PercView perc_view(const PercParams& Q, int r)
{
    PercView v{};
    v.col = Q.col; v.P = Q.P; v.PW = Q.PW; v.sN = Q.sN;
    if (Q.ds) {
        v.ds = Q.ds + (size_t)r * Q.rows * 64 * Q.PW;
        v.pm = Q.pm + (size_t)r * Q.rows * Q.PW;
        v.mm = Q.mm + (size_t)r * Q.rows * Q.PW;
    }
    return v;
}
inline size_t perc_lds_bytes(int64_t rows, int64_t PW) { return (size_t)rows * (size_t)PW * (2 * 8 + 64 * 2); }

// 32 spins of the row that starts at bit `off`, from bit `off + 32 w`, masked to the row's Nk bits
__device__ __forceinline__ uint32_t perc_row_word(const uint32_t* sp, int off, int w, int Nk, int Nbits)
{
    const int b0 = off + 32 * w, q = b0 >> 5, sh = b0 & 31, rem = Nk - 32 * w;
    uint32_t bits = sp[q] >> sh;
    if (sh && 32 * (q + 1) < Nbits) bits |= sp[q + 1] << (32 - sh);
    if (rem < 32) bits &= (1u << rem) - 1u;
    return bits;
}
// Δ_a of the configuration in row `off / Nk` (PercStep.jl:100-101)
__device__ __forceinline__ int perc_stability(const PercParams& Q, const uint32_t* sp, int off, int Nk, int Nbits, int a)
{
    const uint32_t* xa = Q.row + (size_t)a * Q.RW;
    int cnt = 0;
    for (int w = 0; 32 * w < Nk; ++w) cnt += __popc(perc_row_word(sp, off, w, Nk, Nbits) ^ xa[w]);
    return Nk - 2 * cnt;
}
// a pattern's term of the energy in integer units: 1 (step), (−Δ − 1) ÷ 2 + 1 (linear) when Δ < 0
template <bool LIN> __device__ __forceinline__ int perc_cost(int d) { return d < 0 ? (LIN ? (-d - 1) / 2 + 1 : 1) : 0; }
template <bool LIN> __device__ __forceinline__ bool perc_in_m(int d) { return LIN ? d < 0 : d == -1; }
// integer units -> energy: E (step, ET = Int), 2E / sN (linear, PercLinear.jl:114)
template <bool LIN> __device__ __forceinline__ double perc_energy_of(long long n, double sN) { return LIN ? (double)(2 * n) / sN : (double)n; }

// energy(X, C) of one row, sequential, from the configuration only
template <bool LIN>
__device__ inline double perc_row_energy(const PercParams& Q, const uint32_t* sp, int off, int Nk, int Nbits)
{
    long long n = 0;
    for (int a = 0; a < Q.P; ++a) n += perc_cost<LIN>(perc_stability(Q, sp, off, Nk, Nbits, a));
    return perc_energy_of<LIN>(n, Q.sN);
}

// energy (PercStep.jl:88-111) of rows row0 .. rows-1 of one chain by a whole workgroup (blockDim a multiple of 64): Δs and the masks are
// written, the integer energy of row k is added to s_n[k] (zeroed by the caller, who also synchronises afterwards)
template <bool LIN>
__device__ inline void perc_init_rows(const PercParams& Q, const PercView& pv, const uint32_t* sp, int Nk, int Nbits, long long* s_n)
{
    const int Pp = 64 * Q.PW, tot = Q.rows * Pp, lane = (int)threadIdx.x & 63;
    for (int idx = (int)threadIdx.x; idx < tot; idx += (int)blockDim.x) {          // a wavefront covers one mask word: uniform trip counts
        const int k = idx / Pp, a = idx - k * Pp;
        const bool in = a < Q.P;
        const int d = in ? perc_stability(Q, sp, k * Nk, Nk, Nbits, a) : 0;
        pv.ds[idx] = (int16_t)d;
        const uint64_t p = __ballot(in && d == 1), m = __ballot(in && perc_in_m<LIN>(d));
        if (lane == 0) { pv.pm[idx >> 6] = p; pv.mm[idx >> 6] = m; }
        if (d < 0) atomicAdd(reinterpret_cast<unsigned long long*>(&s_n[k]), (unsigned long long)perc_cost<LIN>(d));
    }
}

// delta_energy (PercStep.jl:150-173, PercLinear.jl:154-177) of flipping synapse i of row k, whose spin bit is s
template <bool LIN>
__device__ __forceinline__ double perc_residual(const PercView& pv, int k, int i, int s)
{
    const uint64_t* c = pv.col + (size_t)i * pv.PW;
    const uint64_t* pm = pv.pm + (size_t)k * pv.PW;
    const uint64_t* mm = pv.mm + (size_t)k * pv.PW;
    const uint64_t sx = s ? ~0ull : 0ull;
    int d = 0;
    for (int w = 0; w < pv.PW; ++w) {
        const uint64_t cw = c[w] ^ sx, m = mm[w];
        d += __popcll(pm[w] & ~cw) - __popcll(m & cw);
        if constexpr (LIN) d += __popcll(m & ~cw);
    }
    if constexpr (LIN) return (double)(2 * d) / pv.sN;
    else return (double)d;
}

// update_cache! (PercStep.jl:113-143, PercLinear.jl:117-145) of row k after synapse i was flipped to the spin bit s
template <bool LIN, bool WAVE>
__device__ __forceinline__ void perc_update(const PercView& pv, int k, int i, int s)
{
    const uint64_t* c = pv.col + (size_t)i * pv.PW;
    int16_t* ds = pv.ds + (size_t)k * 64 * pv.PW;
    uint64_t* pm = pv.pm + (size_t)k * pv.PW;
    uint64_t* mm = pv.mm + (size_t)k * pv.PW;
    const uint64_t sx = s ? ~0ull : 0ull;
    if constexpr (WAVE) {
        const int lane = (int)threadIdx.x;
        for (int w = 0; w < pv.PW; ++w) {
            const uint64_t cw = c[w] ^ sx;
            const int a = 64 * w + lane;
            const bool in = a < pv.P;
            const int nd = in ? (int)ds[a] + 2 - 4 * (int)((cw >> lane) & 1ull) : 0;
            ds[a] = (int16_t)nd;
            const uint64_t p = __ballot(in && nd == 1), m = __ballot(in && perc_in_m<LIN>(nd));
            if (lane == 0) { pm[w] = p; mm[w] = m; }
        }
        __syncthreads();                                    // (one wavefront per workgroup) the masks are read by every lane
    } else {
        for (int w = 0; w < pv.PW; ++w) {
            const uint64_t cw = c[w] ^ sx;
            const int nb = pv.P - 64 * w < 64 ? pv.P - 64 * w : 64;
            uint64_t p = 0, m = 0;
            for (int b = 0; b < nb; ++b) {
                const int nd = (int)ds[64 * w + b] + 2 - 4 * (int)((cw >> b) & 1ull);
                ds[64 * w + b] = (int16_t)nd;
                p |= (uint64_t)(nd == 1) << b;
                m |= (uint64_t)perc_in_m<LIN>(nd) << b;
            }
            pm[w] = p; mm[w] = m;
        }
    }
}

// debug checks: Δs and the masks of rows row0 .. rows-1 equal what the configuration gives
template <bool LIN>
__device__ inline bool perc_state_bad(const PercParams& Q, const PercView& pv, const uint32_t* sp, int row0, int Nk, int Nbits)
{
    bool bad = false;
    for (int k = row0; k < Q.rows; ++k)
        for (int a = 0; a < Q.P; ++a) {
            const int d = perc_stability(Q, sp, k * Nk, Nk, Nbits, a);
            const int ip = (int)((pv.pm[(size_t)k * Q.PW + (a >> 6)] >> (a & 63)) & 1ull), im = (int)((pv.mm[(size_t)k * Q.PW + (a >> 6)] >> (a & 63)) & 1ull);
            bad = bad || d != pv.ds[(size_t)k * 64 * Q.PW + a] || ip != (d == 1) || im != (int)perc_in_m<LIN>(d);
        }
    return bad;
}

// ---- the stand-alone graphs: GraphPercStep(N, P), GraphPercLinear(N, P) under standardMC -----------------------------------------------
struct PercMcParams {
    PercParams pc;
    uint32_t* sp;                                           // [R][W] spins, bit i = synapse i (the context's configuration)
    double* E_cur; int64_t* stats; double* Es;              // [R], [R][2], [nsamples][R]
    int32_t* flag;
    double beta;
    uint64_t g0;
    int64_t iters, step;
    long long samp0;
    uint32_t k0, k1, replica0;
    int N, W, R;
};

constexpr int kPercInitThreads = 256;
// energy(X, C) and the Stabilities of every chain, one workgroup per chain
template <bool LIN>
__global__ __launch_bounds__(kPercInitThreads) void perc_init_kernel(PercMcParams P)
{
    __shared__ long long s_n;
    const int r = (int)blockIdx.x;
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    perc_init_rows<LIN>(P.pc, perc_view(P.pc, r), P.sp + (size_t)r * P.W, P.N, 32 * P.W, &s_n);
    __syncthreads();
    if (threadIdx.x == 0) {
        P.E_cur[r] = perc_energy_of<LIN>(s_n, P.pc.sN);
        P.stats[(size_t)r * 2] = 0; P.stats[(size_t)r * 2 + 1] = 0;
    }
}

// standardMC (src/RRRMC.jl:81-127), one thread per chain: the common SITE stream names the synapse, rand() < exp(-β ΔE) on the ACCEPT_F64
// stream.  E starts from E_cur (perc_init_kernel, or the run a resumed call continues).
template <bool LIN>
__global__ __launch_bounds__(kRrrThreads) void perc_standard_kernel(PercMcParams P)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= P.R) return;
    uint32_t* sp = P.sp + (size_t)r * P.W;
    const PercView pv = perc_view(P.pc, r);
    const uint32_t rep = P.replica0 + (uint32_t)r;
    double E = P.E_cur[r];
    int64_t accepted = 0, ns = 0;
    long long next_sample = P.samp0;
    for (int64_t it = 1; it <= P.iters; ++it) {
        if (it == next_sample) { next_sample += P.step; P.Es[ns * P.R + r] = E; ns += 1; }
        const uint64_t g = P.g0 + (uint64_t)it;
        const int i = (int)site_of(P.k0, P.k1, g, (uint32_t)P.N);
        const double dE = perc_residual<LIN>(pv, 0, i, sbit(sp, i));
        const double xx = -P.beta * dE;
        const bool acc = (xx >= 0.0) || (rand53(P.k0, P.k1, g, rep) < det_exp(xx));          // RRRMC.jl:39
        if (acc) {
            sflip(sp, i);
            perc_update<LIN, false>(pv, 0, i, sbit(sp, i));
            E += dE;
            accepted += 1;
        }
    }
    P.E_cur[r] = E;
    P.stats[(size_t)r * 2] = accepted; P.stats[(size_t)r * 2 + 1] = 0;
}

// debug mode (rrrmc_set_debug_checks): the tracked energy, Δs and the masks against the configuration
template <bool LIN>
__global__ __launch_bounds__(64) void perc_check_kernel(PercMcParams P)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= P.R) return;
    const uint32_t* sp = P.sp + (size_t)r * P.W;
    bool bad = perc_state_bad<LIN>(P.pc, perc_view(P.pc, r), sp, 0, P.N, 32 * P.W);
    // |ΔE| <= 1e-10 max(1, |E|), as le_check_kernel (a deliberate departure from the absolute 1e-10 of RRRMC.jl:250): GraphPercLinear's energy reaches 10^5 and more at N = 32 767 with thousands of violated
    // patterns, where the rounding of a hundred E += ΔE alone exceeds an absolute 1e-10 (the step graph's integers stay exact)
    const double E = perc_row_energy<LIN>(P.pc, sp, 0, P.N, 32 * P.W);
    const double d = E - P.E_cur[r], tol = 1e-10 * (E < -1.0 ? -E : E > 1.0 ? E : 1.0);
    bad = bad || !(d <= tol && d >= -tol);
    if (bad) { atomicAdd(&P.flag[0], 1); P.flag[1] = r; }
}

}  // namespace rrrmc
