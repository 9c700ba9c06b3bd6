// gfx950 kernels for random K-SAT (src/graphs/SAT.jl): GraphSAT(N, K, α) stand-alone under standardMC, and the helpers its slices use in
// the Robust Ensemble and the Local Entropy ensemble (re_kernels.hpp, le_kernels.hpp: GraphSATRE / GraphSATLE, src/REAliases.jl:77-92,
// src/LEAliases.jl:77-92).  The clause walk and the occurrence program are in sat_core.hpp: delta_energy is recomputed from the
// spins, there is no per-chain cache and no update_cache!.
//
// The site of an iteration comes from the common SITE stream, so every replica of a call walks the SAME occurrence list: table addresses
// are wave-uniform in both builds.
//   sat_standard_kernel  one thread per replica.  Spins in the transposed [W][R] word layout (word w of replica r at w R + r, as the
//                        dense-SK sampler keeps them), so the lanes of a wavefront read adjacent words; control flow is uniform.
//   sat_wave_kernel      one wavefront per replica (the "few replicas" pattern), the replica's spins in LDS.  Lane l evaluates occurrence
//                        base + l of the site — one entry load, <= 7 LDS bit reads — and ΔE = popc(ballot(sole)) − popc(ballot(unsat)),
//                        accumulated over passes of 64.  The draws of 64 iterations are made by the 64 lanes at once.  Accept is decided
//                        on wave-uniform values; lane 0 flips the bit.
// Integer ΔE, the same rand53 / det_exp: both builds give the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rrr_kernels.hpp"   // sbit / sflip, kRrrThreads, site_of, rand53, det_exp
#include "sat_core.hpp"

namespace rrrmc {

constexpr int kSatWaveWords = (kSatNmax + 31) / 32;         // LDS words of one replica's spins in the wave build (8 KiB)

struct SatMcParams {
    SatTable tab;
    uint32_t* sp;                                           // [R][W] spins, bit i = variable i (the context's configuration)
    uint32_t* spT;                                          // [W][R] the thread build's transposed copy
    double* E_cur; int64_t* stats; double* Es;              // [R], [R][2], [nsamples][R]
    int32_t* flag;
    double beta;
    uint64_t g0;
    int64_t iters, step;
    long long samp0;
    uint32_t k0, k1, replica0;
    int N, W, R;
};

// the transposed layout: bit x of replica r
struct SatColBits {
    const uint32_t* spT; int R, r;
    __device__ __forceinline__ int operator()(int x) const { return (int)((spT[(size_t)(x >> 5) * R + r] >> (x & 31)) & 1u); }
};
// a replica's spins in LDS (or any contiguous row starting at bit 0)
struct SatLdsBits {
    const uint32_t* sp;
    __device__ __forceinline__ int operator()(int x) const { return (int)((sp[x >> 5] >> (x & 31)) & 1u); }
};

// [R][W] <-> [W][R], one thread per word
__global__ __launch_bounds__(256) void sat_transpose_kernel(SatMcParams P, int back)
{
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (long long)P.R * P.W) return;
    const int w = (int)(e / P.R), r = (int)(e - (long long)w * P.R);
    if (back) P.sp[(size_t)r * P.W + w] = P.spT[e];
    else P.spT[e] = P.sp[(size_t)r * P.W + w];
}

// energy(X, C) of every replica (SAT.jl:189-236), one thread per replica
__global__ __launch_bounds__(64) void sat_init_kernel(SatMcParams P)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= P.R) return;
    P.E_cur[r] = (double)sat_row_energy(P.tab, P.sp + (size_t)r * P.W, 0);
    P.stats[(size_t)r * 2] = 0; P.stats[(size_t)r * 2 + 1] = 0;
}

// standardMC (src/RRRMC.jl:81-127), one thread per replica on the transposed spins.  E starts from E_cur (sat_init_kernel, or the run a
// resumed call continues).
__global__ __launch_bounds__(kRrrThreads) void sat_standard_kernel(SatMcParams P)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= P.R) return;
    const SatColBits bits{P.spT, P.R, r};
    const uint32_t rep = P.replica0 + (uint32_t)r;
    double E = P.E_cur[r];
    int64_t accepted = 0, ns = 0;
    long long next_sample = P.samp0;
    for (int64_t it = 1; it <= P.iters; ++it) {
        if (it == next_sample) { next_sample += P.step; P.Es[ns * P.R + r] = E; ns += 1; }
        const uint64_t g = P.g0 + (uint64_t)it;
        const int i = (int)site_of(P.k0, P.k1, g, (uint32_t)P.N);
        const double dE = (double)sat_delta_bits(P.tab, i, bits);
        const double xx = -P.beta * dE;
        const bool acc = (xx >= 0.0) || (rand53(P.k0, P.k1, g, rep) < det_exp(xx));          // RRRMC.jl:39
        if (acc) {
            P.spT[(size_t)(i >> 5) * P.R + r] ^= 1u << (i & 31);
            E += dE;
            accepted += 1;
        }
    }
    P.E_cur[r] = E;
    P.stats[(size_t)r * 2] = accepted; P.stats[(size_t)r * 2 + 1] = 0;
}

// standardMC, one wavefront (one workgroup of 64) per replica on the context's [R][W] spins
__global__ __launch_bounds__(64) void sat_wave_kernel(SatMcParams P)
{
    __shared__ uint32_t l_sp[kSatWaveWords];
    __shared__ int l_site[64];
    __shared__ double l_u[64];
    const int r = (int)blockIdx.x, lane = (int)threadIdx.x;
    uint32_t* g_sp = P.sp + (size_t)r * P.W;
    for (int w = lane; w < P.W; w += 64) l_sp[w] = g_sp[w];
    const SatLdsBits bits{l_sp};
    const uint32_t rep = P.replica0 + (uint32_t)r;
    double E = P.E_cur[r];
    int64_t accepted = 0, ns = 0;
    long long next_sample = P.samp0;
    for (int64_t base = 0; base < P.iters; base += 64) {
        __syncthreads();
        {
            const uint64_t gl = P.g0 + (uint64_t)(base + 1 + lane);
            l_site[lane] = (int)site_of(P.k0, P.k1, gl, (uint32_t)P.N);
            l_u[lane] = rand53(P.k0, P.k1, gl, rep);
        }
        __syncthreads();
        const int64_t it_end = base + 64 < P.iters ? base + 64 : P.iters;
        for (int64_t it = base + 1; it <= it_end; ++it) {
            if (it == next_sample) { next_sample += P.step; if (lane == 0) P.Es[ns * P.R + r] = E; ns += 1; }
            const int i = l_site[it - base - 1];
            const uint32_t e0 = P.tab.off[i], e1 = P.tab.off[i + 1];
            const int si = bits(i);
            int d = 0;
            for (uint32_t eb = e0; eb < e1; eb += 64) {
                const uint32_t e = eb + (uint32_t)lane;
                int term = 0;
                if (e < e1) { const SatEntry en = P.tab.ent[e]; term = sat_entry_term(en, si, bits); }
                d += __popcll(__ballot(term > 0)) - __popcll(__ballot(term < 0));
            }
            const double dE = (double)d;
            const double xx = -P.beta * dE;
            const bool acc = (xx >= 0.0) || (l_u[it - base - 1] < det_exp(xx));              // RRRMC.jl:39
            if (acc) {
                __syncthreads();                            // (one wavefront) every lane has read the bits of this iteration
                if (lane == 0) l_sp[i >> 5] ^= 1u << (i & 31);
                __syncthreads();
                E += dE;
                accepted += 1;
            }
        }
    }
    __syncthreads();
    for (int w = lane; w < P.W; w += 64) g_sp[w] = l_sp[w];
    if (lane == 0) {
        P.E_cur[r] = E;
        P.stats[(size_t)r * 2] = accepted; P.stats[(size_t)r * 2 + 1] = 0;
    }
}

// debug mode (rrrmc_set_debug_checks): the tracked energy against the configuration
__global__ __launch_bounds__(64) void sat_check_kernel(SatMcParams P)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= P.R) return;
    const double E = (double)sat_row_energy(P.tab, P.sp + (size_t)r * P.W, 0);
    if (E != P.E_cur[r]) { atomicAdd(&P.flag[0], 1); P.flag[1] = r; }
}

// ---- SAT slices of the ensembles: rows k Nk of the slice-major copy ----------------------------------------------------------------------
// the number of unsatisfied clauses of rows row0 .. rows-1 of one chain by a whole workgroup, added to s_n[k] (zeroed by the caller, who
// also synchronises afterwards)
__device__ inline void sat_init_rows(const SatTable& T, const uint32_t* sp, int Nk, int row0, int rows, long long* s_n)
{
    for (int idx = row0 * Nk + (int)threadIdx.x; idx < rows * Nk; idx += (int)blockDim.x) {
        const int k = idx / Nk, i = idx - k * Nk;
        const int n = sat_first_unsat(T, i, SatRowBits{sp, k * Nk});
        if (n) atomicAdd(reinterpret_cast<unsigned long long*>(&s_n[k]), (unsigned long long)n);
    }
}

}  // namespace rrrmc
