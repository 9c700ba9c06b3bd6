// gfx950 kernels for GraphAddFields / GraphAddSubFields (src/graphs/AddFields.jl:16-123): a DoubleGraph whose inner graph X0 = GraphAF(h)
// is N independent external fields (energy Σ_i h_i σ_i, delta_energy −2 σ_i h_i, no neighbours) over one graph g of N spins — any of the
// nine slice kinds of re_kernels.hpp, GraphPercXEntr (xentr_kernels.hpp) or GraphPSpin3 (pspin_kernels.hpp), used as ONE slice (M = 1, so
// the ABI site order is the slice's own).
//   GraphAddFields    (sub = 0): E = energy(X0) + energy(g), ΔE = ΔE(X0) + ΔE(g), residual = ΔE(g)
//   GraphAddSubFields (sub = 1): E = energy(g),              ΔE = ΔE(g),          residual = ΔE(g) − ΔE(X0)
// Samplers: rrrMC(X::DoubleGraph) (src/RRRMC.jl:221-290) over DeltaECacheCont (src/DeltaE.jl:297-410) and the DynamicSampler
// (src/DynamicSamplers.jl) of X0, and standardMC (src/RRRMC.jl:81-127).  X0 has no neighbours: a move is ONE setindex!, whatever g is.
//
// Layout.  Per chain: ΔEs [N], the sampler's weights v [N2] and its partial-sum tree ps [N2] in heap order (node (lev, k) at
// (1 << lev) − 1 + k = the sum of its LEFT subtree, DynamicSamplers.jl:54-98; N2 = 2^levs, levs = ceil(log2 N); entry N2 − 1 unused), z,
// trefresh, acc_rate, E and g's own per-chain state where its kind has one.  Everything is in global memory between calls, which is what a
// resumed call continues from.
//
// af_rrr_kernel: one wavefront per chain; all 64 lanes run the chain with identical values (wave-uniform control flow), lane 0 stores.
// The lanes share what is independent inside a step: getel (DynamicSamplers.jl:130-152) reads up to six tree levels per round trip (lane =
// node of the subtree below the current node, walked through v_readlane, as cont_wave_kernel.hpp does); the <= 16 node additions of a
// setindex! (:159-176) go one level per lane — distinct nodes, so every node receives the reference's one addition —; refresh! (:84-98)
// gives every node to one lane, which sums the leaves of its left subtree in ascending order, and z is accumulated sequentially (as
// cw_refresh does; the reference's sum(v) is pairwise); the perceptron and committee machine updates are one pattern per lane
// (perc_update / comm_update<.., true>), and GraphPercXEntr's residual is the wave build of xentr_kernels.hpp: one term per lane, then the
// ordered sum by every lane (xentr_residual_wave).
// LDS = true: tree, weights, ΔEs, the spins and g's per-chain state live in LDS for the call; LDS = false: in global memory.  Same
// operations in the same order: the two builds give the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "re_kernels.hpp"         // ReParams, re_view, re_residual / re_slice_update / re_slice_view / re_slice_energy, the slice kinds
#include "sk_block_kernel.hpp"    // sk_readlane_f64
#include "mixed_models.hpp"       // MixedList: g = GraphMixed (SLICE = RE_MIXED; the device functions are mixed_kernels.hpp's)

namespace rrrmc {

struct AfParams {
    ReParams re;                                            // g as one slice (M = 1, Nk = N, sp = abi = the context's configuration); the call's
                                                            // scalars, zz / E_cur / acc_rate / stats / Es / flag
    const double* h;                                        // [N]      the fields
    double* dEs;                                            // [R][N]   DeltaECacheCont.ΔEs
    double* v;                                              // [R][N2]  DynamicSampler.v (zeros beyond N)
    double* ps;                                             // [R][N2]  DynamicSampler.ps, heap order
    long long* tref;                                        // [R]      DynamicSampler.trefresh
    int32_t* status;                                        // [2]      chains that met "Unrecoverable loss of precision detected in the dynamic sampler", one of them
    int sub, levs, N2;
    int xe_hs_lds;                                          // GraphPercXEntr in the LDS build: the loss table is staged too (it fits)
    MixedList mx;                                           // g = GraphMixed: the component list (n = 0 otherwise)
};

// bytes of LDS one chain takes in the LDS build, without g's per-chain state: tree and weights (16 N2), ΔEs, the spins
__host__ __device__ inline size_t af_lds_bytes(int64_t N, int64_t N2, int64_t W) { return (size_t)N2 * 16 + (size_t)N * 8 + (((size_t)W * 4 + 7) & ~(size_t)7); }

// delta_energy(X0, C, i) = -2 σ h (AddFields.jl:45-52)
__device__ __forceinline__ double af_delta0(const double* h, int i, int s) { return (double)(-2 * (2 * s - 1)) * h[i]; }

// energy(g, C) from the integer (or Float64) total that the slice helpers of re_init_kernel leave
template <int SLICE>
__device__ __forceinline__ double af_g_energy(const ReParams& P, long long n, double eskn)
{
    if constexpr (SLICE == RE_SK) { n /= 2; return (double)n / P.sN; }
    else if constexpr (SLICE == RE_SKN || SLICE == RE_PXE) return eskn;          // (a Float64 sum made in the reference's order)
    else if constexpr (kPercSlice<SLICE>) return perc_energy_of<SLICE == RE_PLIN>(n, P.pc.sN);
    else if constexpr (kCommSlice<SLICE> || SLICE == RE_SAT) return (double)n;
    else if constexpr (SLICE == RE_PSPIN3) return (double)(n / 3);                // every triple was met by its three sites (PSpin3.jl:88-89)
    else return 0.0;
}

// The start of a reference call (src/RRRMC.jl:237-240): E = energy(X, C) and g's own cache; with `cache`, DeltaECacheCont(X0, C, β) — ΔEs,
// the weights prior(β ΔE) and refresh! —, acc_rate = 0.5.  One workgroup per chain.
constexpr int kAfInitThreads = 256;
}  // namespace rrrmc
#include "mixed_kernels.hpp"      // g = GraphMixed: the hooks of af_rrr_kernel<RE_MIXED, LDS> and the mix's own kernels (they take AfParams)
namespace rrrmc {
template <int SLICE>
__global__ __launch_bounds__(kAfInitThreads) void af_init_kernel(AfParams A, int cache)
{
    __shared__ long long s_n[1];
    __shared__ double s_E[1];
    const ReParams& P = A.re;
    const int r = (int)blockIdx.x, tid = (int)threadIdx.x;
    const int N = P.N;
    uint32_t* sp = P.sp + (size_t)r * P.W;
    const RrrView v = re_view(P, sp, r);
    if (tid == 0) { s_n[0] = 0; s_E[0] = 0.0; }
    __syncthreads();
    if constexpr (SLICE == RE_SK) {
        for (int x = tid; x < N; x += kAfInitThreads)
            atomicAdd(reinterpret_cast<unsigned long long*>(&s_n[0]), (unsigned long long)(long long)(-(slice_delta(v, x) / 2)));
    } else if constexpr (SLICE == RE_SKN) {                 // SK.jl:212-237: lfields = 2 lf, lfields_last = 0, move_last = none
        for (int i = tid; i < N; i += kAfInitThreads) {
            const double* Ji = P.Jd + (size_t)i * N;
            const int si = sbit(sp, i);
            double lf = 0.0;
            for (int j = 0; j < N; ++j) lf += (double)(1 - 2 * (si ^ sbit(sp, j))) * Ji[j];
            v.slf[i] = 2 * lf;
            v.slf[(size_t)N + i] = lf;
        }
        __syncthreads();
        if (tid == 0) {
            double n = 0.0;
            for (int i = 0; i < N; ++i) n -= v.slf[(size_t)N + i];
            n /= 2;
            s_E[0] = n;
            v.smv[0] = -1;
            v.scur[0] = 0;
        }
        __syncthreads();
        for (int i = tid; i < N; i += kAfInitThreads) v.slf[(size_t)N + i] = 0.0;
    } else if constexpr (kPercSlice<SLICE>) {
        perc_init_rows<SLICE == RE_PLIN>(P.pc, perc_view(P.pc, r), sp, N, N, s_n);
    } else if constexpr (kCommSlice<SLICE>) {
        comm_init_rows<comm_kind_of_slice(SLICE)>(P.cm, comm_view<comm_kind_of_slice(SLICE)>(P.cm, r), sp, N, N, s_n);
    } else if constexpr (SLICE == RE_SAT) {
        sat_init_rows(P.sat, sp, N, 0, 1, s_n);
    } else if constexpr (SLICE == RE_PSPIN3) {
        pspin_init_row(P.ps3, sp, s_n);
    } else if constexpr (SLICE == RE_PXE) {
        __shared__ double s_t[kPercPmax];
        const double Eg = xentr_init_chain(P.pc, P.xe, P.pc.ds + (size_t)r * 64 * P.pc.PW, 1, sp, N, s_t);
        if (tid == 0) s_E[0] = Eg;
    }
    __syncthreads();
    if (cache) {
        double* dEs = A.dEs + (size_t)r * N;
        double* w = A.v + (size_t)r * A.N2;
        double* ps = A.ps + (size_t)r * A.N2;
        for (int i = tid; i < A.N2; i += kAfInitThreads) {
            double x = 0.0;
            if (i < N) {
                const double d = af_delta0(A.h, i, sbit(sp, i));
                dEs[i] = d;
                x = prior_of(P.beta * d);
            }
            w[i] = x;
        }
        __syncthreads();
        // refresh!: node (lev, k) = the sum of the elements of its left subtree, ascending, from 0.0
        const int levs = A.levs;
        for (int n = tid; n < A.N2 - 1; n += kAfInitThreads) {
            const int lev = 31 - __builtin_clz((unsigned)n + 1u), k = n + 1 - (1 << lev), half = 1 << (levs - 1 - lev), i0 = k << (levs - lev);
            double acc = 0.0;
            for (int e = 0; e < half; ++e) { const int i = i0 + e; if (i < N) acc += w[i]; }
            ps[n] = acc;
        }
        if (tid == 0) ps[A.N2 - 1] = 0.0;
    }
    if (tid == 0) {
        double E0 = 0.0;
        if (!A.sub)
            for (int i = 0; i < N; ++i) E0 += A.h[i] * (double)(2 * sbit(sp, i) - 1);          // AddFields.jl:33-43
        const double Eg = af_g_energy<SLICE>(P, s_n[0], s_E[0]);
        P.E_cur[r] = A.sub ? Eg : E0 + Eg;                  // AddFields.jl:81, :117
        if (cache) {
            const double* w = A.v + (size_t)r * A.N2;
            double z = 0.0;
            for (int i = 0; i < N; ++i) z += w[i];
            P.zz[r] = z;
            P.acc_rate[r] = 0.5;
            A.tref[r] = 0;
        }
        P.stats[(size_t)r * 2] = 0;
        P.stats[(size_t)r * 2 + 1] = 0;
    }
}

// rrrMC(X::DoubleGraph) on GraphAddFields / GraphAddSubFields, one wavefront per chain
template <int SLICE, bool LDS>
__global__ __launch_bounds__(64) void af_rrr_kernel(AfParams A)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char af_lds[];
    const ReParams& P = A.re;
    const int lane = (int)threadIdx.x, r = (int)blockIdx.x;
    const int N = P.N, N2 = A.N2, levs = A.levs, W = P.W;
    uint32_t* const g_sp = P.sp + (size_t)r * W;
    double* const g_dEs = A.dEs + (size_t)r * N;
    double* const g_v = A.v + (size_t)r * N2;
    double* const g_ps = A.ps + (size_t)r * N2;
    uint32_t* sp = g_sp; double* dEs = g_dEs; double* w = g_v; double* ps = g_ps;
    if constexpr (LDS) {
        ps = reinterpret_cast<double*>(af_lds);                                    // [N2]
        w = ps + N2;                                                               // [N2]
        dEs = w + N2;                                                              // [N]
        sp = reinterpret_cast<uint32_t*>(dEs + N);                                 // [W]
        for (int i = lane; i < N2; i += 64) { ps[i] = g_ps[i]; w[i] = g_v[i]; }
        for (int i = lane; i < N; i += 64) dEs[i] = g_dEs[i];
        for (int i = lane; i < W; i += 64) sp[i] = g_sp[i];
        __syncthreads();
    }
    RrrView v = re_view(P, sp, r);
    const auto g_pv = re_slice_view<SLICE>(P, r);                                  // PercView, CommView or SatTable
    auto pv = g_pv;
    [[maybe_unused]] MixedViews mv{};                                              // g = GraphMixed: the components' state stays in global memory
    if constexpr (SLICE == RE_MIXED) mv = mixed_views(P, A.mx, r);
    double* const g_slf = v.slf;
    [[maybe_unused]] unsigned char* const l_slice = af_lds + ((af_lds_bytes(N, N2, W) + 7) & ~(size_t)7);
    if constexpr (LDS && SLICE == RE_SKN) {
        v.slf = reinterpret_cast<double*>(l_slice);                                // [2][N]
        for (int i = lane; i < 2 * N; i += 64) v.slf[i] = g_slf[i];
        __syncthreads();
    }
    if constexpr (LDS && kPercSlice<SLICE>) {
        const int nw = P.pc.PW;                                                    // mask words, then 64 stabilities per word
        pv.pm = reinterpret_cast<uint64_t*>(l_slice);
        pv.mm = pv.pm + nw;
        pv.ds = reinterpret_cast<int16_t*>(pv.mm + nw);
        for (int i = lane; i < nw; i += 64) { pv.pm[i] = g_pv.pm[i]; pv.mm[i] = g_pv.mm[i]; }
        for (int i = lane; i < 64 * nw; i += 64) pv.ds[i] = g_pv.ds[i];
        __syncthreads();
    }
    if constexpr (LDS && SLICE == RE_PXE) {
        const int Pp = 64 * P.pc.PW;                                               // the term buffer (16-byte aligned), the table when it fits, Δs
        pv.term = reinterpret_cast<double*>(af_lds + ((af_lds_bytes(N, N2, W) + 15) & ~(size_t)15));
        double* const hs = pv.term + Pp;
        pv.ds = reinterpret_cast<int16_t*>(hs + (A.xe_hs_lds ? N + 1 : 0));
        if (A.xe_hs_lds) {
            for (int i = lane; i <= N; i += 64) hs[i] = g_pv.Hs[i];
            pv.Hs = hs;
        }
        for (int i = lane; i < Pp; i += 64) pv.ds[i] = g_pv.ds[i];
        __syncthreads();
    }
    if constexpr (LDS && kCommSlice<SLICE>) {
        const int nm = (int)comm_mk_row(P.cm.K2, P.cm.PW, comm_kind_of_slice(SLICE) == CK_QU), nd = (int)comm_ds_row(P.cm.K2, P.cm.PW, comm_kind_of_slice(SLICE) == CK_QU);
        pv.mk = reinterpret_cast<uint64_t*>(l_slice);
        pv.ds = reinterpret_cast<int16_t*>(pv.mk + nm);
        for (int i = lane; i < nm; i += 64) pv.mk[i] = g_pv.mk[i];
        for (int i = lane; i < nd; i += 64) pv.ds[i] = g_pv.ds[i];
        __syncthreads();
    }
    const uint32_t rep = P.replica0 + (uint32_t)r;
    const double beta = P.beta;
    double z = P.zz[r], E = P.E_cur[r], acc_rate = P.acc_rate[r];
    long long trefresh = A.tref[r];
    const long long tlim = N > 100 ? N : 100;
    int64_t accepted = P.stats[(size_t)r * 2], staged_its = P.stats[(size_t)r * 2 + 1], ns = 0;
    long long next_sample = P.samp0;
    int bad = 0;

    auto bcd = [](double x, int l) -> double { return sk_readlane_f64(x, l); };
    // refresh! (DynamicSamplers.jl:84-98)
    auto refresh = [&]() {
        __syncthreads();
        for (int n = lane; n < N2 - 1; n += 64) {
            const int lev = 31 - __builtin_clz((unsigned)n + 1u), k = n + 1 - (1 << lev), half = 1 << (levs - 1 - lev), i0 = k << (levs - lev);
            double acc = 0.0;
            for (int e = 0; e < half; ++e) { const int i = i0 + e; if (i < N) acc += w[i]; }
            ps[n] = acc;
        }
        double zz = 0.0;
        for (int i = 0; i < N; ++i) zz += w[i];
        z = zz;
        trefresh = 0;
        __syncthreads();
    };
    // setindex! (:159-176): the counter is tested before it advances; level `lane` of the tree takes its one addition
    auto setel = [&](int i, double x) {
        if (trefresh >= tlim) refresh();
        trefresh += 1;
        const double d = x - w[i];
        __syncthreads();                                                           // (every lane has read the old weight)
        if (lane == 0) w[i] = x;
        z += d;
        if (lane < levs && ((i >> (levs - 1 - lane)) & 1) == 0) ps[(1 << lane) - 1 + (i >> (levs - lane))] += d;
        __syncthreads();
    };
    // getel (:130-152); -1 = "Unrecoverable loss of precision"
    const int hj = 31 - __builtin_clz((unsigned)lane + 1u), hm = lane + 1 - (1 << hj);       // this lane's node of a subtree: level hj, index hm
    auto getel = [&](double x) -> int {
        x = bcd(x, 0);                                                             // (every lane computed the same draw: tell the compiler)
        for (;;) {
            x *= z;
            int k = 0;
            for (int l0 = 0; l0 < levs; l0 += 6) {
                const int wl = levs - l0 < 6 ? levs - l0 : 6;
                const double pn = lane < (1 << wl) - 1 ? ps[(1 << (l0 + hj)) - 1 + (k << hj) + hm] : 0.0;
                int cur = 0;
                for (int s = 0; s < wl; ++s) {
                    const double p = bcd(pn, cur);
                    if (x > p) { x -= p; cur = 2 * cur + 2; } else cur = 2 * cur + 1;
                }
                k = (k << wl) + (cur - ((1 << wl) - 1));
            }
            k = __builtin_amdgcn_readfirstlane(k);
            if (k >= N || w[k < N ? k : 0] == 0) {
                if (!(trefresh > 0)) return -1;
                refresh();
                continue;
            }
            return k;
        }
    };
    // the slice graph's update_cache!: the kinds whose update is written for one thread run it on lane 0
    auto g_update = [&](int move) {
        if constexpr (kWaveSlice<SLICE>) re_slice_update<SLICE, true>(v, pv, move, 0, move);
        else if constexpr (SLICE == RE_MIXED) mixed_update_follow<true>(A.mx, v, move);          // (the pure components: g_update_pure)
        else if constexpr (SLICE == RE_SKN) {
            __syncthreads();
            if (lane == 0) skn_update(v, move);
            __syncthreads();
        }
    };
    // GraphMixed: the components that are pure functions of the configuration, once per accepted move
    auto g_update_pure = [&]([[maybe_unused]] int move) {
        if constexpr (SLICE == RE_MIXED) mixed_update_pure<true>(A.mx, v, mv, move);
    };
    auto flip = [&](int move) {
        __syncthreads();                                                           // (every lane has read the old bit)
        if (lane == 0) sflip(sp, move);
        __syncthreads();
    };
    auto accept_c = [&](double c, double x, uint64_t g) {                          // accept(c, x), RRRMC.jl:40-44
        bool ok = (c >= 1 && x >= 0);
        if (!ok) {
            const double a = c * det_exp(x);
            ok = a >= 1;
            if (!ok) {
                const Philox4 o2 = philox4x32_10((uint32_t)g, (uint32_t)(g >> 32), rep, TAG_RRR | (1u << 8), P.k0, P.k1);
                ok = (double)((((uint64_t)o2.w[0] << 32) | o2.w[1]) >> 11) * 0x1.0p-53 < a;
            }
        }
        return ok;
    };
    // delta_energy_residual at the current configuration (AddFields.jl:83, :119)
    auto residual = [&](int move) -> double {
        double dg;
        if constexpr (SLICE == RE_MIXED) dg = mixed_residual<true>(A.mx, v, mv, move);
        else dg = re_residual<SLICE, true>(v, pv, move, 0, move);
        return A.sub ? dg - af_delta0(A.h, move, sbit(sp, move)) : dg;
    };

    for (int64_t it = 1; it <= P.iters; ++it) {
        if (it == next_sample) { next_sample += P.step; if (lane == 0) P.Es[ns * P.R + r] = E; ns += 1; }
        const uint64_t g = P.g0 + (uint64_t)it;
        const Philox4 o = philox4x32_10((uint32_t)g, (uint32_t)(g >> 32), rep, TAG_RRR, P.k0, P.k1);
        const int move = getel((double)((((uint64_t)o.w[0] << 32) | o.w[1]) >> 11) * 0x1.0p-53);       // rand_move, DeltaE.jl:326-332
        if (move < 0) { bad = 1; break; }
        const double dE0 = dEs[move];
        bool acc = false;
        if (acc_rate < P.staged_thr) {
            // step_rrr (RRRMC.jl:131-138): compute_staged! on X0 flips, looks and flips back; the list is the move alone
            staged_its += 1;
            const double dEp = -dE0, pp = prior_of(beta * dEp);
            double zp = z + (pp - w[move]);                                        // compute_reverse_probabilities!, DeltaE.jl:344-354
            if (zp < 2.2250738585072014e-308) zp = 2.2250738585072014e-308;
            if (zp > (double)N) zp = (double)N;
            const double c = z / zp;
            const double dE1 = residual(move);
            if (accept_c(c, -beta * dE1, g)) {
                flip(move);                                                        // spinflip!(X, C, move)
                g_update(move);
                g_update_pure(move);
                __syncthreads();
                if (lane == 0) dEs[move] = dEp;                                    // apply_staged!
                setel(move, pp);
                E += dE0 + dE1;
                accepted += 1;
                acc = true;
            }
        } else {
            // direct branch: apply_move! (DeltaE.jl:378-410), undone by a second apply_move! on rejection.  g's cache follows every flip
            // where it keeps an undo record (GraphSKNormal's swap); where it is a pure function of the configuration it is updated once,
            // for an accepted move
            const double dE1 = residual(move);
            for (int pass = 0; pass < 2; ++pass) {
                flip(move);
                if constexpr (!kWaveSlice<SLICE>) g_update(move);
                const double z0 = z;
                const double dn = af_delta0(A.h, move, sbit(sp, move));
                __syncthreads();
                if (lane == 0) dEs[move] = dn;
                setel(move, prior_of(beta * dn));
                const double cc = z0 / z;
                if (pass == 1) break;                                              // that was the undo
                if (accept_c(cc, -beta * dE1, g)) { E += dE0 + dE1; accepted += 1; acc = true; break; }
            }
            if constexpr (kWaveSlice<SLICE>) { if (acc) g_update(move); }
            if (acc) g_update_pure(move);
        }
        acc_rate = acc_rate * (1 - P.lambda) + (acc ? 1.0 : 0.0) * P.lambda;       // RRRMC.jl:281
    }
    __syncthreads();
    if (lane == 0) {
        P.zz[r] = z; P.E_cur[r] = E; P.acc_rate[r] = acc_rate;
        P.stats[(size_t)r * 2] = accepted; P.stats[(size_t)r * 2 + 1] = staged_its;
        A.tref[r] = trefresh;
        if (bad) { atomicAdd(&A.status[0], 1); A.status[1] = r; }
    }
    if constexpr (LDS) {
        for (int i = lane; i < N2; i += 64) { g_ps[i] = ps[i]; g_v[i] = w[i]; }
        for (int i = lane; i < N; i += 64) g_dEs[i] = dEs[i];
        for (int i = lane; i < W; i += 64) g_sp[i] = sp[i];
    }
    if constexpr (LDS && SLICE == RE_SKN) {
        for (int i = lane; i < 2 * N; i += 64) g_slf[i] = v.slf[i];
    }
    if constexpr (LDS && kPercSlice<SLICE>) {
        const int nw = P.pc.PW;
        for (int i = lane; i < nw; i += 64) { g_pv.pm[i] = pv.pm[i]; g_pv.mm[i] = pv.mm[i]; }
        for (int i = lane; i < 64 * nw; i += 64) g_pv.ds[i] = pv.ds[i];
    }
    if constexpr (LDS && SLICE == RE_PXE) {
        for (int i = lane; i < 64 * P.pc.PW; i += 64) g_pv.ds[i] = pv.ds[i];
    }
    if constexpr (LDS && kCommSlice<SLICE>) {
        const int nm = (int)comm_mk_row(P.cm.K2, P.cm.PW, comm_kind_of_slice(SLICE) == CK_QU), nd = (int)comm_ds_row(P.cm.K2, P.cm.PW, comm_kind_of_slice(SLICE) == CK_QU);
        for (int i = lane; i < nm; i += 64) g_pv.mk[i] = pv.mk[i];
        for (int i = lane; i < nd; i += 64) g_pv.ds[i] = pv.ds[i];
    }
}

// standardMC (src/RRRMC.jl:81-127), one thread per chain: the common SITE stream names the spin, rand() < exp(-β ΔE) on the ACCEPT_F64
// stream; ΔE = ΔE(X0) + ΔE(g) (AddFields.jl:85-88) or ΔE(g) (:121).  E starts from E_cur (af_init_kernel, or the run a resumed call continues).
template <int SLICE>
__global__ __launch_bounds__(kRrrThreads) void af_standard_kernel(AfParams A)
{
    const ReParams& P = A.re;
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= P.R) return;
    uint32_t* sp = P.sp + (size_t)r * P.W;
    const RrrView v = re_view(P, sp, r);
    const auto pv = re_slice_view<SLICE>(P, r);
    const uint32_t rep = P.replica0 + (uint32_t)r;
    double E = P.E_cur[r];
    int64_t accepted = 0, ns = 0;
    long long next_sample = P.samp0;
    for (int64_t it = 1; it <= P.iters; ++it) {
        if (it == next_sample) { next_sample += P.step; P.Es[ns * P.R + r] = E; ns += 1; }
        const uint64_t g = P.g0 + (uint64_t)it;
        const int i = (int)site_of(P.k0, P.k1, g, (uint32_t)P.N);
        const double dg = re_residual<SLICE>(v, pv, i, 0, i);
        const double dE = A.sub ? dg : af_delta0(A.h, i, sbit(sp, i)) + dg;
        const double xx = -P.beta * dE;
        const bool acc = (xx >= 0.0) || (rand53(P.k0, P.k1, g, rep) < det_exp(xx));          // RRRMC.jl:39
        if (acc) {
            sflip(sp, i);
            re_slice_update<SLICE, false>(v, pv, i, 0, i);
            E += dE;
            accepted += 1;
        }
    }
    P.E_cur[r] = E;
    P.stats[(size_t)r * 2] = accepted; P.stats[(size_t)r * 2 + 1] = 0;
}

// debug mode (rrrmc_set_debug_checks): after a sampler call every chain's energy(X, C) is re-evaluated from its configuration and compared
// with the tracked E (|ΔE| <= 1e-10 max(1, |E|): the reference's check, RRRMC.jl:250, has an absolute 1e-10; relative once |E| > 1 is a deliberate departure, see re_check_kernel); g's cache is held as its own family's check holds
// it; after rrrMC, ΔEs and the weights must equal their definitions on the final spins bit for bit.
template <int SLICE>
__global__ __launch_bounds__(64) void af_check_kernel(AfParams A, int cache)
{
    const ReParams& P = A.re;
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= P.R) return;
    const int N = P.N;
    const uint32_t* sp = P.sp + (size_t)r * P.W;
    const RrrView v = re_view(P, P.sp + (size_t)r * P.W, r);
    bool bad = false;
    double E0 = 0.0;
    if (!A.sub)
        for (int i = 0; i < N; ++i) E0 += A.h[i] * (double)(2 * sbit(sp, i) - 1);
    const double Eg = re_slice_energy<SLICE>(P, v, 0);
    const double E = A.sub ? Eg : E0 + Eg;
    const double d = E - P.E_cur[r], tol = 1e-10 * (E < -1.0 ? -E : E > 1.0 ? E : 1.0);          // relative once |E| > 1, as le_check_kernel
    bad = bad || !(d <= tol && d >= -tol);
    if constexpr (SLICE == RE_SKN) {
        for (int i = 0; i < N; ++i) {
            const int si = sbit(sp, i);
            const double* Ji = P.Jd + (size_t)i * N;
            double lf = 0.0;
            for (int j = 0; j < N; ++j) lf += (double)(1 - 2 * (si ^ sbit(sp, j))) * Ji[j];
            const double dd = v.slf[(size_t)v.scur[0] * N + i] - 2 * lf;
            bad = bad || !(dd <= 1e-10 * N && dd >= -1e-10 * N);
        }
    }
    if constexpr (kPercSlice<SLICE>) bad = bad || perc_state_bad<SLICE == RE_PLIN>(P.pc, perc_view(P.pc, r), sp, 0, N, N);
    if constexpr (kCommSlice<SLICE>) bad = bad || comm_state_bad<comm_kind_of_slice(SLICE)>(P.cm, comm_view<comm_kind_of_slice(SLICE)>(P.cm, r), sp, 0, N, N);
    if constexpr (SLICE == RE_PXE) bad = bad || xentr_state_bad(P.pc, P.xe, P.pc.ds + (size_t)r * 64 * P.pc.PW, 1, sp, N);
    if (cache) {
        const double* dEs = A.dEs + (size_t)r * N;
        const double* w = A.v + (size_t)r * A.N2;
        for (int i = 0; i < N; ++i) {
            const double de = af_delta0(A.h, i, sbit(sp, i));
            bad = bad || !(dEs[i] == de) || !(w[i] == prior_of(P.beta * de));
        }
        for (int i = N; i < A.N2; ++i) bad = bad || !(w[i] == 0.0);
    }
    if (bad) { atomicAdd(&P.flag[0], 1); P.flag[1] = r; }
}

}  // namespace rrrmc
