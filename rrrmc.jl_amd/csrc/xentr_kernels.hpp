// gfx950 kernels for the cross-entropy perceptron (src/graphs/PercXEntr.jl): N (odd) binary synapses trained on P random patterns ξ,
// GraphPercXEntr{λ}{Float64}: energy = Σ_a Hs[Δ2i(Δ_a)] with Hs[k] = log(1 + exp(−2 λ Δ / √N)) for Δ = −N + 2k (PercXEntr.jl:65, :97-119).
// Stand-alone under standardMC (xentr_standard_kernel, xentr_wave_kernel below) and as the g of GraphAddFields / GraphAddSubFields
// (af_kernels.hpp), which is what opens rrrMC on it.
//
// State.  Per chain: the stabilities Δs[a] = N − 2 Σ_i (s_i ⊻ ξ[a,i]) as int16 (|Δ| <= N <= 32 767), a pure function of the
// configuration as in perc_kernels.hpp: flipping a spin and flipping it back restores them.  The reference's newΔs array and its swap
// (PercXEntr.jl:44-47, :127-130: update_cache! right after delta_energy of the same move takes the stabilities delta_energy wrote), its
// ξsi / last_move copy of one pattern column (:138, :173) and the justΔ flag are optimisations of its memory accesses: the values they
// yield are Δ_a + 2 − 4 (ξ[a,i] ⊻ s_i) either way.  They have no counterpart here.
//
// Unlike the two other perceptrons' (perc_kernels.hpp), this delta_energy is no sum of integers: PercXEntr.jl:177-186 is
//     ΔE = 0.0;  for a = 1:P  ΔE += Hs[Δ2i(newΔ_a)] − Hs[Δ2i(oldΔ_a)]  end
// — P rounded Float64 additions in pattern order, on every attempt.  The terms t_a = Hs[..] − Hs[..] (one rounded subtraction each) are
// independent and may be formed in any order or in parallel; the additions are made in the reference's order, one chain of P dependent
// adds.  The library is built with -ffp-contract=off: every operation below is its own rounded Float64 operation.
//
// The table Hs is an INPUT (rrrmc_set_loss_table): N + 1 finite doubles made by the caller, so that the trajectory does not depend on whose
// log and exp made it.  Index (Δ + N) >> 1 is in 0 .. N by construction: |Δ_a| <= N always, and a move that would leave the range does not
// exist (a pattern with Δ_a = N has no mismatching synapse to flip towards N + 2).
//
// Two builds, same operations in the same order, same bits:
//   thread (xentr_standard_kernel): one thread per chain, as perc_standard_kernel.  Δs of 64 chains are interleaved ([tile][a][lane]) so
//     that the lanes of a wavefront read one pattern's stabilities from consecutive addresses; each lane runs its own ordered sum.
//   wave (xentr_wave_kernel): one wavefront per chain, wave-uniform control flow as in perc_update<.., true>.  Lane l owns pattern 64 w + l:
//     the lanes form the t_a in parallel into an LDS term buffer, then every lane runs the ordered sum over the buffer (broadcast reads,
//     identical values in all lanes).  Δs, the term buffer and the spins live in LDS.
//   HS_LDS: the table is staged in LDS when it fits beside the rest (the wave build: and the chains are few enough for its footprint not to
//   cost resident wavefronts, host_xentr.hpp); otherwise (and under RRRMC_XENTR_NO_LDS=1) it stays in global memory.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "perc_kernels.hpp"  // PercParams (patterns, Δs), perc_stability, kPercNmax / kPercPmax
#include "rrr_kernels.hpp"   // sbit / sflip, kRrrThreads, site_of, rand53, det_exp

namespace rrrmc {

struct XentrParams {                                        // what GraphPercXEntr adds to PercParams
    const double* Hs;                                       // [N + 1]
    double* term;                                           // [R][64 PW] the term buffer of the wrappers' global-memory build (af_kernels.hpp), else null
    double hmax;                                            // the table's largest entry (the debug check's bound)
    int N;
};

struct XentrView {                                          // one chain's state; Δ_a at ds[a * stride]
    const uint64_t* col; const double* Hs;
    int16_t* ds; double* term;
    int P, PW, N, stride;
};

__device__ __forceinline__ int xentr_idx(int d, int N) { return (d + N) >> 1; }          // Δ2i (PercXEntr.jl:49), 0-based

// the stand-alone contexts' layout of Δs: tiles of 64 chains, pattern-major inside a tile
__device__ __forceinline__ int16_t* xentr_tile_ds(int16_t* ds, int r, int PW) { return ds + (size_t)(r >> 6) * 64 * PW * 64 + (r & 63); }
// a wrapper's chain: plain [R][64 PW] (PercParams::ds with rows = 1)
__device__ __forceinline__ XentrView xentr_view(const PercParams& Q, const XentrParams& X, int r)
{
    XentrView v{};
    v.col = Q.col; v.Hs = X.Hs; v.P = Q.P; v.PW = Q.PW; v.N = X.N; v.stride = 1;
    if (Q.ds) v.ds = Q.ds + (size_t)r * 64 * Q.PW;
    if (X.term) v.term = X.term + (size_t)r * 64 * Q.PW;
    return v;
}

// bytes of LDS the wave build takes: the term buffer, the table when it is staged, Δs; `spin_words` 32-bit words of spins behind them
__host__ __device__ inline size_t xentr_lds_bytes(int64_t N, int64_t PW, int64_t spin_words, bool hs)
{
    return (size_t)PW * 64 * 8 + (hs ? ((size_t)N + 1) * 8 : 0) + (size_t)PW * 64 * 2 + (size_t)spin_words * 4;
}

// energy (PercXEntr.jl:97-119) of one chain, sequential, from the configuration only
__device__ inline double xentr_row_energy(const PercParams& Q, const XentrParams& X, const uint32_t* sp, int Nbits)
{
    double E = 0.0;
    for (int a = 0; a < Q.P; ++a) E += X.Hs[xentr_idx(perc_stability(Q, sp, 0, X.N, Nbits, a), X.N)];
    return E;
}

// energy by a whole workgroup: Δs written (entries a >= P are 0), the P terms staged in s_t ([P] doubles of LDS), then added by thread 0 in
// pattern order; the result is returned to thread 0 only.  The caller synchronises afterwards.
__device__ inline double xentr_init_chain(const PercParams& Q, const XentrParams& X, int16_t* ds, int stride, const uint32_t* sp, int Nbits, double* s_t)
{
    const int Pp = 64 * Q.PW;
    for (int a = (int)threadIdx.x; a < Pp; a += (int)blockDim.x) {
        const int d = a < Q.P ? perc_stability(Q, sp, 0, X.N, Nbits, a) : 0;
        ds[(size_t)a * stride] = (int16_t)d;
        if (a < Q.P) s_t[a] = X.Hs[xentr_idx(d, X.N)];
    }
    __syncthreads();
    double E = 0.0;
    if (threadIdx.x == 0)
        for (int a = 0; a < Q.P; ++a) E += s_t[a];
    return E;
}

// delta_energy (PercXEntr.jl:165-193) of flipping synapse i, whose spin bit is s: one thread
__device__ __forceinline__ double xentr_residual(const XentrView& v, int i, int s)
{
    const uint64_t* c = v.col + (size_t)i * v.PW;
    const uint64_t sx = s ? ~0ull : 0ull;
    double dE = 0.0;
    for (int w = 0; w < v.PW; ++w) {
        const uint64_t cw = c[w] ^ sx;
        const int nb = v.P - 64 * w < 64 ? v.P - 64 * w : 64;          // patterns of a partial last word beyond P contribute nothing
        for (int b = 0; b < nb; ++b) {
            const int od = (int)v.ds[(size_t)(64 * w + b) * v.stride];
            const int nd = od + 4 * (int)((cw >> b) & 1ull) - 2;
            dE += v.Hs[xentr_idx(nd, v.N)] - v.Hs[xentr_idx(od, v.N)];
        }
    }
    return dE;
}
// ... and by a wavefront (the workgroup; all 64 lanes call it with identical arguments and get identical values)
__device__ __forceinline__ double xentr_residual_wave(const XentrView& v, int i, int s)
{
    const uint64_t* c = v.col + (size_t)i * v.PW;
    const uint64_t sx = s ? ~0ull : 0ull;
    const int lane = (int)threadIdx.x;
    // four pattern words at a time, their look-ups ahead of their stores: when the table is in LDS too, a store to the term buffer between
    // two look-ups makes every look-up wait for it (the compiler cannot tell the two LDS arrays apart)
    for (int w0 = 0; w0 < v.PW; w0 += 4) {
        double t[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int w = w0 + k, a = 64 * w + lane;
            t[k] = 0.0;
            if (a < v.P) {                                  // (a < P implies w < PW)
                const int od = (int)v.ds[a];
                const int nd = od + 4 * (int)(((c[w] ^ sx) >> lane) & 1ull) - 2;
                t[k] = v.Hs[xentr_idx(nd, v.N)] - v.Hs[xentr_idx(od, v.N)];
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (w0 + k < v.PW) v.term[64 * (w0 + k) + lane] = t[k];
    }
    __syncthreads();
    double dE = 0.0;
    int a = 0;
    for (; a + 4 <= v.P; a += 4) {                          // (the buffer is 16-byte aligned: two terms per read)
        const double2 x = *reinterpret_cast<const double2*>(v.term + a), y = *reinterpret_cast<const double2*>(v.term + a + 2);
        dE += x.x; dE += x.y; dE += y.x; dE += y.y;
    }
    for (; a < v.P; ++a) dE += v.term[a];
    __syncthreads();                                        // (the next call overwrites the buffer)
    return dE;
}

// update_cache! (PercXEntr.jl:121-151) after synapse i was flipped to the spin bit s: Δ_a += 2 − 4 (ξ[a,i] ⊻ s), the rule of perc_update
template <bool WAVE>
__device__ __forceinline__ void xentr_update(const XentrView& v, int i, int s)
{
    const uint64_t* c = v.col + (size_t)i * v.PW;
    const uint64_t sx = s ? ~0ull : 0ull;
    if constexpr (WAVE) {
        const int lane = (int)threadIdx.x;
        for (int w = 0; w < v.PW; ++w) {
            const int a = 64 * w + lane;
            if (a < v.P) v.ds[a] = (int16_t)((int)v.ds[a] + 2 - 4 * (int)(((c[w] ^ sx) >> lane) & 1ull));
        }
        __syncthreads();
    } else {
        for (int w = 0; w < v.PW; ++w) {
            const uint64_t cw = c[w] ^ sx;
            const int nb = v.P - 64 * w < 64 ? v.P - 64 * w : 64;
            for (int b = 0; b < nb; ++b) {
                int16_t* d = v.ds + (size_t)(64 * w + b) * v.stride;
                *d = (int16_t)((int)*d + 2 - 4 * (int)((cw >> b) & 1ull));
            }
        }
    }
}

// debug checks: Δs equal what the configuration gives, exactly
__device__ inline bool xentr_state_bad(const PercParams& Q, const XentrParams& X, const int16_t* ds, int stride, const uint32_t* sp, int Nbits)
{
    bool bad = false;
    for (int a = 0; a < Q.P; ++a) bad = bad || perc_stability(Q, sp, 0, X.N, Nbits, a) != (int)ds[(size_t)a * stride];
    return bad;
}
// ... and the tracked energy equals a fresh one within the rounding a run of `nacc` accepted moves can have gathered.  With u = 2^-53 and
// H = the table's largest entry (all entries are >= 0 up to rounding, so |t_a| <= H and every partial sum is <= P H in magnitude):
//   a fresh energy: P additions, each off by <= u P H                                  -> u P^2 H, at the start of the run and in the check;
//   one ΔE: P subtractions off by <= u H each, P additions off by <= u P H each         -> u P (P + 1) H;
//   one E += ΔE: |E| <= P H and |ΔE| <= P H                                             -> 2 u P H.
// Sum: u H (2 P^2 + nacc (P (P + 1) + 2 P)) <= u H P (P + 3) (nacc + 2).  Loose (errors do not all align); the exact check is the one on Δs.
__device__ __forceinline__ double xentr_energy_bound(int P, double hmax, long long nacc)
{
    return 0x1.0p-53 * hmax * (double)P * (double)(P + 3) * (double)(nacc + 2);
}

// ---- the stand-alone graph: GraphPercXEntr(N, P, λ) under standardMC --------------------------------------------------------------------
struct XentrMcParams {
    PercParams pc;                                          // patterns; ds = the tiled Δs ([ceil(R / 64)][64 PW][64])
    XentrParams xe;
    uint32_t* sp;                                           // [R][W] spins, bit i = synapse i (the context's configuration)
    double* E_cur; int64_t* stats; double* Es;              // [R], [R][2], [nsamples][R]
    int64_t* nacc;                                          // [R] accepted moves of the run (since the last xentr_init_kernel)
    int32_t* flag;
    double beta;
    uint64_t g0;
    int64_t iters, step;
    long long samp0;
    uint32_t k0, k1, replica0;
    int N, W, R;
};

constexpr int kXentrInitThreads = 256;
// energy(X, C) and the stabilities of every chain, one workgroup per chain
__global__ __launch_bounds__(kXentrInitThreads) void xentr_init_kernel(XentrMcParams P)
{
    __shared__ double s_t[kPercPmax];
    const int r = (int)blockIdx.x;
    const double E = xentr_init_chain(P.pc, P.xe, xentr_tile_ds(P.pc.ds, r, P.pc.PW), 64, P.sp + (size_t)r * P.W, 32 * P.W, s_t);
    if (threadIdx.x == 0) {
        P.E_cur[r] = E;
        P.stats[(size_t)r * 2] = 0; P.stats[(size_t)r * 2 + 1] = 0;
        P.nacc[r] = 0;
    }
}

// standardMC (src/RRRMC.jl:81-127), one thread per chain: the common SITE stream names the synapse, rand() < exp(-β ΔE) on the ACCEPT_F64
// stream.  E starts from E_cur (xentr_init_kernel, or the run a resumed call continues).
template <bool HS_LDS>
__global__ __launch_bounds__(kRrrThreads) void xentr_standard_kernel(XentrMcParams P)
{
    extern __shared__ __attribute__((aligned(16))) double xentr_hs[];
    if constexpr (HS_LDS) {
        for (int k = (int)threadIdx.x; k <= P.N; k += (int)blockDim.x) xentr_hs[k] = P.xe.Hs[k];
        __syncthreads();
    }
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= P.R) return;
    uint32_t* sp = P.sp + (size_t)r * P.W;
    XentrView v{};
    v.col = P.pc.col; v.Hs = HS_LDS ? xentr_hs : P.xe.Hs; v.P = P.pc.P; v.PW = P.pc.PW; v.N = P.N; v.stride = 64;
    v.ds = xentr_tile_ds(P.pc.ds, r, P.pc.PW);
    const uint32_t rep = P.replica0 + (uint32_t)r;
    double E = P.E_cur[r];
    int64_t accepted = 0, ns = 0;
    long long next_sample = P.samp0;
    for (int64_t it = 1; it <= P.iters; ++it) {
        if (it == next_sample) { next_sample += P.step; P.Es[ns * P.R + r] = E; ns += 1; }
        const uint64_t g = P.g0 + (uint64_t)it;
        const int i = (int)site_of(P.k0, P.k1, g, (uint32_t)P.N);
        const double dE = xentr_residual(v, i, sbit(sp, i));
        const double xx = -P.beta * dE;
        const bool acc = (xx >= 0.0) || (rand53(P.k0, P.k1, g, rep) < det_exp(xx));          // RRRMC.jl:39
        if (acc) {
            sflip(sp, i);
            xentr_update<false>(v, i, sbit(sp, i));
            E += dE;
            accepted += 1;
        }
    }
    P.E_cur[r] = E;
    P.stats[(size_t)r * 2] = accepted; P.stats[(size_t)r * 2 + 1] = 0;
    P.nacc[r] += accepted;
}

// the same chain by one wavefront: every lane holds the chain's scalars with identical values, lane 0 stores
template <bool HS_LDS>
__global__ __launch_bounds__(64) void xentr_wave_kernel(XentrMcParams P)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char xentr_lds[];
    const int lane = (int)threadIdx.x, r = (int)blockIdx.x;
    const int Pp = 64 * P.pc.PW, W = P.W;
    double* const term = reinterpret_cast<double*>(xentr_lds);                     // [Pp]
    double* const hs = term + Pp;                                                  // [N + 1] when staged
    int16_t* const ds = reinterpret_cast<int16_t*>(hs + (HS_LDS ? P.N + 1 : 0));   // [Pp]
    uint32_t* const sp = reinterpret_cast<uint32_t*>(ds + Pp);                     // [W]
    uint32_t* const g_sp = P.sp + (size_t)r * W;
    int16_t* const g_ds = xentr_tile_ds(P.pc.ds, r, P.pc.PW);
    if constexpr (HS_LDS)
        for (int k = lane; k <= P.N; k += 64) hs[k] = P.xe.Hs[k];
    for (int a = lane; a < Pp; a += 64) ds[a] = g_ds[(size_t)a * 64];
    for (int w = lane; w < W; w += 64) sp[w] = g_sp[w];
    __syncthreads();
    XentrView v{};
    v.col = P.pc.col; v.Hs = HS_LDS ? hs : P.xe.Hs; v.ds = ds; v.term = term; v.P = P.pc.P; v.PW = P.pc.PW; v.N = P.N; v.stride = 1;
    const uint32_t rep = P.replica0 + (uint32_t)r;
    double E = P.E_cur[r];
    int64_t accepted = 0, ns = 0;
    long long next_sample = P.samp0;
    for (int64_t it = 1; it <= P.iters; ++it) {
        if (it == next_sample) { next_sample += P.step; if (lane == 0) P.Es[ns * P.R + r] = E; ns += 1; }
        const uint64_t g = P.g0 + (uint64_t)it;
        const int i = (int)site_of(P.k0, P.k1, g, (uint32_t)P.N);
        const double dE = xentr_residual_wave(v, i, sbit(sp, i));
        const double xx = -P.beta * dE;
        const bool acc = (xx >= 0.0) || (rand53(P.k0, P.k1, g, rep) < det_exp(xx));          // RRRMC.jl:39
        if (acc) {
            if (lane == 0) sflip(sp, i);                    // (every lane has read the old bit: xentr_residual_wave ends with a barrier)
            __syncthreads();
            xentr_update<true>(v, i, sbit(sp, i));
            E += dE;
            accepted += 1;
        }
    }
    __syncthreads();
    for (int a = lane; a < Pp; a += 64) g_ds[(size_t)a * 64] = ds[a];
    for (int w = lane; w < W; w += 64) g_sp[w] = sp[w];
    if (lane == 0) {
        P.E_cur[r] = E;
        P.stats[(size_t)r * 2] = accepted; P.stats[(size_t)r * 2 + 1] = 0;
        P.nacc[r] += accepted;
    }
}

// debug mode (rrrmc_set_debug_checks): Δs against the configuration exactly, the tracked energy against a fresh one within xentr_energy_bound
__global__ __launch_bounds__(64) void xentr_check_kernel(XentrMcParams P)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= P.R) return;
    const uint32_t* sp = P.sp + (size_t)r * P.W;
    bool bad = xentr_state_bad(P.pc, P.xe, xentr_tile_ds(P.pc.ds, r, P.pc.PW), 64, sp, 32 * P.W);
    const double d = xentr_row_energy(P.pc, P.xe, sp, 32 * P.W) - P.E_cur[r], tol = xentr_energy_bound(P.pc.P, P.xe.hmax, P.nacc[r]);
    bad = bad || !(d <= tol && d >= -tol);
    if (bad) { atomicAdd(&P.flag[0], 1); P.flag[1] = r; }
}

// step_energy (PercXEntr.jl:205-213): the number of patterns with Δ_a < 0, from the configuration; one wavefront per chain
__global__ __launch_bounds__(64) void perc_step_energy_kernel(PercParams Q, const uint32_t* spins, int N, int W, int64_t* out)
{
    const int r = (int)blockIdx.x, lane = (int)threadIdx.x;
    const uint32_t* sp = spins + (size_t)r * W;
    int n = 0;
    for (int a0 = 0; a0 < Q.P; a0 += 64) {
        const int a = a0 + lane;
        n += __popcll(__ballot(a < Q.P && perc_stability(Q, sp, 0, N, 32 * W, a) < 0));
    }
    if (lane == 0) out[r] = n;
}

}  // namespace rrrmc
