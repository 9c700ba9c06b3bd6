// gfx950 kernels for the regular 3-spin model (src/graphs/PSpin3.jl): GraphPSpin3(N, K) stand-alone under standardMC, and the helpers it
// uses as the g of GraphAddFields / GraphAddSubFields (af_kernels.hpp).  The partner table, delta_energy and energy are pspin_core.hpp's
// (DESIGN §4w): ΔE is recomputed from the spins, there is no per-chain cache and no update_cache!.
//
// The site of an iteration comes from the common SITE stream, the uniform from ACCEPT_F64, the verdict is that of every non-±J model:
// acc = (x >= 0) || (u < det_exp(x)), x = −β ΔE (RRRMC.jl:39) — β = +∞ with ΔE = 0 gives x = NaN and is rejected, as in the reference.
//   pspin_standard_kernel  one thread per chain.  Spins in the transposed [W][R] word layout (word w of chain r at w R + r), so the lanes
//                          of a wavefront — which all attempt the same site — read adjacent words; 2K + 1 word reads per attempt, the
//                          table row is wave-uniform.  The build for many chains.
//   pspin_wave_kernel      one wavefront per chain, the chain's spins in LDS.  The 64 lanes take 64 CONSECUTIVE iterations: lane l draws
//                          the site and the uniform of iteration base + 1 + l, gathers its 2K partner ids once (K words) and evaluates
//                          ΔE and the verdict against the LDS state at the start of the batch.  The wave then retires the 64 attempts in
//                          the chain's order: the verdicts are read wave-uniformly (one ballot), a rejected attempt changes nothing and
//                          is passed over, an accepted one at site j has lane 0 flip the bit, after which only the LATER lanes whose
//                          neighbourhood holds j (their site is j, or j is among their 2K ids) evaluate ΔE and the verdict again — for
//                          a lane whose site is j that re-evaluation flips the sign.  Energy samples are written from the running E in
//                          order.  The last batch of a call may be shorter than 64.  ("Run commuting attempts side by side, retire in
//                          the chain's order", the idea of spf_team_kernel, inside one wavefront.)
// Integer ΔE, the same rand53 / det_exp, E accumulated in the chain's order: both builds give the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rrr_kernels.hpp"   // kRrrThreads, site_of, rand53, det_exp
#include "pspin_core.hpp"

namespace rrrmc {

constexpr int kPspinWaveWords = 2 * ((kPspinNmax + 63) / 64);          // LDS words of one chain's spins in the wave build (8 KiB)

struct PspinMcParams {
    PspinTable tab;
    uint32_t* sp;                                           // [R][W] spins, bit i = site i (the context's configuration)
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

// the transposed layout: bit x of chain r
struct PspinColBits {
    const uint32_t* spT; int R, r;
    __device__ __forceinline__ int operator()(int x) const { return (int)((spT[(size_t)(x >> 5) * R + r] >> (x & 31)) & 1u); }
};
// a chain's spins in LDS
struct PspinLdsBits {
    const uint32_t* sp;
    __device__ __forceinline__ int operator()(int x) const { return (int)((sp[x >> 5] >> (x & 31)) & 1u); }
};

// [R][W] <-> [W][R], one thread per word
__global__ __launch_bounds__(256) void pspin_transpose_kernel(PspinMcParams P, int back)
{
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (long long)P.R * P.W) return;
    const int w = (int)(e / P.R), r = (int)(e - (long long)w * P.R);
    if (back) P.sp[(size_t)r * P.W + w] = P.spT[e];
    else P.spT[e] = P.sp[(size_t)r * P.W + w];
}

// energy(X, C) of every chain (PSpin3.jl:62-93), one thread per chain
__global__ __launch_bounds__(64) void pspin_init_kernel(PspinMcParams P)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= P.R) return;
    P.E_cur[r] = (double)pspin_energy(P.tab, PspinRowBits{P.sp + (size_t)r * P.W, 0});
    P.stats[(size_t)r * 2] = 0; P.stats[(size_t)r * 2 + 1] = 0;
}

// standardMC (src/RRRMC.jl:81-127), one thread per chain on the transposed spins.  E starts from E_cur (pspin_init_kernel, or the run a
// resumed call continues).
__global__ __launch_bounds__(kRrrThreads) void pspin_standard_kernel(PspinMcParams P)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= P.R) return;
    const PspinColBits bits{P.spT, P.R, r};
    const uint32_t rep = P.replica0 + (uint32_t)r;
    double E = P.E_cur[r];
    int64_t accepted = 0, ns = 0;
    long long next_sample = P.samp0;
    for (int64_t it = 1; it <= P.iters; ++it) {
        if (it == next_sample) { next_sample += P.step; P.Es[ns * P.R + r] = E; ns += 1; }
        const uint64_t g = P.g0 + (uint64_t)it;
        const int i = (int)site_of(P.k0, P.k1, g, (uint32_t)P.N);
        const double dE = (double)pspin_delta(P.tab, i, bits);
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

// standardMC, one wavefront (one workgroup of 64) per chain on the context's [R][W] spins; lane l owns iteration base + 1 + l of a batch
__global__ __launch_bounds__(64) void pspin_wave_kernel(PspinMcParams P)
{
    __shared__ uint32_t l_sp[kPspinWaveWords];
    const int r = (int)blockIdx.x, lane = (int)threadIdx.x;
    const int K = P.tab.K;
    uint32_t* g_sp = P.sp + (size_t)r * P.W;
    for (int w = lane; w < P.W; w += 64) l_sp[w] = g_sp[w];
    __syncthreads();
    const PspinLdsBits bits{l_sp};
    const uint32_t* rows = reinterpret_cast<const uint32_t*>(P.tab.A);          // a site's row: K words (y | z << 16)
    const uint32_t rep = P.replica0 + (uint32_t)r;
    double E = P.E_cur[r];
    int64_t accepted = 0, ns = 0;
    long long next_sample = P.samp0;
    // the samples due before iteration `lim` has been retired: E has not changed since the last retired accept
    auto samples_to = [&](long long lim) {
        while (next_sample <= lim) { if (lane == 0) P.Es[ns * P.R + r] = E; ns += 1; next_sample += P.step; }
    };
    for (int64_t base = 0; base < P.iters; base += 64) {
        const int n = (int)(P.iters - base < 64 ? P.iters - base : 64);          // a tail batch is shorter
        const bool live = lane < n;
        const uint64_t gl = P.g0 + (uint64_t)(base + 1 + lane);
        const int i = (int)site_of(P.k0, P.k1, gl, (uint32_t)P.N);
        const double u = rand53(P.k0, P.k1, gl, rep);
        uint32_t pr[kPspinKmax];
#pragma unroll
        for (int k = 0; k < kPspinKmax; ++k) pr[k] = k < K ? rows[(size_t)i * K + k] : 0u;
        auto delta = [&]() -> int {
            const int si = bits(i);
            int c = 0;
#pragma unroll
            for (int k = 0; k < kPspinKmax; ++k)
                if (k < K) c += si ^ bits((int)(pr[k] & 0xffffu)) ^ bits((int)(pr[k] >> 16));
            return 2 * (2 * c - K);
        };
        auto verdict = [&](int d) -> bool {
            const double xx = -P.beta * (double)d;
            return (xx >= 0.0) || (u < det_exp(xx));                                         // RRRMC.jl:39
        };
        int d = delta();
        bool acc = verdict(d);
        unsigned long long am = __ballot(acc && live);          // the accepted attempts not yet retired (wave-uniform)
        while (am) {
            const int t = __builtin_ctzll(am);                  // attempts before t are rejected at the current state: nothing to do
            samples_to((long long)(base + 1 + t));
            const int j = __builtin_amdgcn_readlane(i, t);
            const int dj = __builtin_amdgcn_readlane(d, t);
            __syncthreads();                                    // (one wavefront) every lane has read the bits it needed
            if (lane == 0) l_sp[j >> 5] ^= 1u << (j & 31);
            __syncthreads();
            E += (double)dj;
            accepted += 1;
            bool hit = i == j;
#pragma unroll
            for (int k = 0; k < kPspinKmax; ++k)
                if (k < K) hit = hit || (int)(pr[k] & 0xffffu) == j || (int)(pr[k] >> 16) == j;
            if (hit && lane > t && live) { d = delta(); acc = verdict(d); }
            am = __ballot(acc && live) & ~((2ull << t) - 1ull);          // lanes 0 .. t are retired
        }
        samples_to((long long)(base + n));
    }
    __syncthreads();
    for (int w = lane; w < P.W; w += 64) g_sp[w] = l_sp[w];
    if (lane == 0) {
        P.E_cur[r] = E;
        P.stats[(size_t)r * 2] = accepted; P.stats[(size_t)r * 2 + 1] = 0;
    }
}

// debug mode (rrrmc_set_debug_checks): the tracked energy against pspin_energy of the configuration
__global__ __launch_bounds__(64) void pspin_check_kernel(PspinMcParams P)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= P.R) return;
    const double E = (double)pspin_energy(P.tab, PspinRowBits{P.sp + (size_t)r * P.W, 0});
    if (E != P.E_cur[r]) { atomicAdd(&P.flag[0], 1); P.flag[1] = r; }
}

// ---- GraphPSpin3 as the g of a field wrapper: one row of N spins ---------------------------------------------------------------------------
// −Σ_i σ_i Σ_k σ_y σ_z of one chain by a whole workgroup, added to s_n[0] (zeroed by the caller, who also synchronises afterwards): three
// times the energy
__device__ inline void pspin_init_row(const PspinTable& T, const uint32_t* sp, long long* s_n)
{
    const PspinRowBits bits{sp, 0};
    for (int i = (int)threadIdx.x; i < T.N; i += (int)blockDim.x) {
        const int n = -(2 * pspin_count(T, i, bits) - T.K);
        if (n) atomicAdd(reinterpret_cast<unsigned long long*>(&s_n[0]), (unsigned long long)(long long)n);
    }
}

}  // namespace rrrmc
