// gfx950 kernels for the Local Entropy ensemble (src/graphs/LE.jl): GraphLocalEntropy{M,γT,G} = the inner graph GraphLE{M,γT}, which couples
// each of M replicas of spin i to an explicit reference ("centre") spin, plus a centre graph Xc and M slice graphs X1[k] of one graph G —
// GraphEmpty (Graph0LE), binary GraphSK (GraphSKLE), GraphSKNormal, GraphEANormal (GraphEALE) (src/LEAliases.jl).  Samplers: rrrMC(X::DoubleGraph) (src/RRRMC.jl:221-290)
// over the DeltaECache{Float64,L} (src/DeltaE.jl:63-295), standardMC (src/RRRMC.jl:81-127), and the observables LEenergies / cenergy /
// distances (LE.jl:259-274, 309-318).
//
// Layout.  Spins cross the ABI in the reference's order j = i (M+1) + k: k = 0 is spin i of the centre, k >= 1 spin i of replica k
// (LE.jl:55-84).  The kernels work on a slice-major copy with M+1 rows, x = k Nk + i (row 0 the centre), which is RE's copy with M+1 rows:
// re_to_slices_kernel / re_from_slices_kernel and the slice helpers of re_kernels.hpp (re_residual, re_slice_update, re_slice_energy) run
// unchanged on it with ReParams::M = M + 1.  The classes, set members and positions are indexed by the ABI site j.
//
// GraphLE's integer cache is never stored: lfields[j] = σc σ_(i,k) for a replica site and σc μ_i (μ_i = Σ_k σ_(i,k)) for the centre, a
// function of the spins that update_cache! (LE.jl:92-154) and its move_last swap keep (tests/le_reference.py restates both and checks it).
// Only μ_i is stored.  The class of a site is a look-up by lfields ∈ [-M, M] in a table the host fills by evaluating findk (DeltaE.jl:26-60)
// literally on ΔE = 2γT lfields, with the `up` rule of DeltaE.jl:83: no shortcut to prove, γT = 0 included.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "re_kernels.hpp"   // ReParams, re_view, re_residual, re_slice_update, re_slice_energy, re_class_f, the ABI <-> slice-major copies

namespace rrrmc {

constexpr int kLeMmax = 31;                                 // replicas M of the ensemble (M + 1 rows)
constexpr int kLeLmax = kLeMmax / 2 + 2;                    // levels: L = M/2 + 2 (M even) or (M+1)/2 (M odd), <= 17 (M = 30)

// ReParams with the LE meaning of its fields: M = the number of ROWS of the slice-major copy (replicas + centre), N = Nk (M + 1),
// tab = allΔE(GraphLE) [L], ft = the class weights [L], etab unused, Eslice [R][M + 1] (row 0: cenergy), slf [R][2][M + 1][Nk] (row 0 unused:
// the centre graph's cache is never updated, LE.jl:231-233).
struct LeParams : ReParams {
    const uint8_t* ctab;                                    // [2 Mr + 1]  class code of lfields = -Mr .. Mr: a | 0x40 (ΔE > 0) | 0x80 (ΔE == 0)
    double g2;                                              // 2γT: ΔE0 = 2γT lfields (LE.jl:156-164)
    double gT;                                              // γT = γ / β: energy(X0) = n γT (LE.jl:55-84)
    int64_t* dist;                                          // [R][Mr][Mr]  distances
    int Mr;                                                 // replicas M
};

// class a + L up of a site whose GraphLE field is lf and whose spin bit is s (DeltaE.jl:80-86)
__device__ __forceinline__ int le_class(const uint8_t* ctab, int Mr, int L, int lf, int s)
{
    const int c = ctab[lf + Mr];
    const int up = (c & 0x40) != 0 || ((c & 0x80) != 0 && s == 1);
    return (c & 0x3f) + L * up;
}

// 32 spins of row `off / Nk` from bit `off + 32 w`, masked to the row (as slice_delta reads a row)
__device__ __forceinline__ uint32_t le_row_word(const uint32_t* sp, int off, int w, int Nk, int Nbits)
{
    const int b0 = off + 32 * w, q = b0 >> 5, sh = b0 & 31, rem = Nk - 32 * w;
    uint32_t bits = sp[q] >> sh;
    if (sh && 32 * (q + 1) < Nbits) bits |= sp[q + 1] << (32 - sh);
    if (rem < 32) bits &= (1u << rem) - 1u;
    return bits;
}

// energy(X::GraphLocalEntropy, C) (LE.jl:242-258: energy(X0) = n γT, then the M slices in k order; the centre's own energy is not part of it)
// and, with `cache`, the DeltaECache (DeltaE.jl:74-103: sites pushed in ABI order), one workgroup per replica.  The replica slices'
// GraphSKNormal caches are rebuilt as SK.jl:212-237 does (lfields = 2 lf, lfields_last = 0, move_last = none).
template <int SLICE>
__global__ __launch_bounds__(kReInitThreads) void le_init_kernel(LeParams P, int cache)
{
    __shared__ int s_cnt[2 * kLeLmax][kReInitThreads];
    __shared__ int s_tot[2 * kLeLmax];
    __shared__ long long s_n[kLeMmax + 1];
    __shared__ double s_E[kLeMmax + 1];
    __shared__ long long s_n0;
    const int r = (int)blockIdx.x, tid = (int)threadIdx.x;
    const int N = P.N, Nk = P.Nk, Mr = P.Mr, rows = P.M, L = P.L;
    uint32_t* sp = P.sp + (size_t)r * P.W;
    int8_t* mu = P.mu + (size_t)r * Nk;
    const RrrView v = re_view(P, sp, r);
    for (int k = tid; k < rows; k += kReInitThreads) s_n[k] = 0;
    if (tid == 0) s_n0 = 0;
    __syncthreads();
    for (int i = tid; i < Nk; i += kReInitThreads) {
        int m = 0;
        for (int k = 1; k < rows; ++k) m += 2 * sbit(sp, k * Nk + i) - 1;
        mu[i] = (int8_t)m;
        atomicAdd(reinterpret_cast<unsigned long long*>(&s_n0), (unsigned long long)(long long)(-(2 * sbit(sp, i) - 1) * m));
    }
    if constexpr (SLICE == RE_SK) {
        for (int x = Nk + tid; x < N; x += kReInitThreads)
            atomicAdd(reinterpret_cast<unsigned long long*>(&s_n[x / Nk]), (unsigned long long)(long long)(-(slice_delta(v, x) / 2)));
    } else if constexpr (SLICE == RE_SKN) {
        for (int x = Nk + tid; x < N; x += kReInitThreads) {
            const int k = x / Nk, i = x - k * Nk;
            const double* Ji = P.Jd + (size_t)i * Nk;
            const int si = sbit(sp, x);
            double lf = 0.0;
            for (int j = 0; j < Nk; ++j) lf += (double)(1 - 2 * (si ^ sbit(sp, k * Nk + j))) * Ji[j];
            v.slf[((size_t)0 * rows + k) * Nk + i] = 2 * lf;
            v.slf[((size_t)1 * rows + k) * Nk + i] = lf;
        }
        __syncthreads();
        for (int k = 1 + tid; k < rows; k += kReInitThreads) {
            double n = 0.0;
            for (int i = 0; i < Nk; ++i) n -= v.slf[((size_t)1 * rows + k) * Nk + i];
            n /= 2;
            s_E[k] = n;
        }
        for (int k = tid; k < rows; k += kReInitThreads) { v.smv[k] = -1; v.scur[k] = 0; }
        __syncthreads();
        for (int x = Nk + tid; x < N; x += kReInitThreads) v.slf[(size_t)rows * Nk + x] = 0.0;
    } else if constexpr (SLICE == RE_SPF) {
        spf_init_rows(P, v, sp, 1, rows, s_E);                                                // (row 0, the centre: its cache is never used)
    } else if constexpr (kPercSlice<SLICE>) {
        perc_init_rows<SLICE == RE_PLIN>(P.pc, perc_view(P.pc, r), sp, Nk, N, s_n);          // (row 0, the centre: built, never used)
    } else if constexpr (kCommSlice<SLICE>) {
        comm_init_rows<comm_kind_of_slice(SLICE)>(P.cm, comm_view<comm_kind_of_slice(SLICE)>(P.cm, r), sp, Nk, N, s_n);          // (likewise)
    } else if constexpr (SLICE == RE_SAT) {
        sat_init_rows(P.sat, sp, Nk, 1, rows, s_n);
    }
    __syncthreads();
    if (cache) {
        // classes of a contiguous block of ABI sites per thread, an exclusive scan of the per-class counts over the threads: site order
        // inside every class, as push! in site order leaves it
        uint8_t* cls = P.cls + (size_t)r * N;
        uint16_t* spos = P.spos + (size_t)r * N;
        uint16_t* sv = P.sv + (size_t)r * 2 * L * N;
        for (int k = 0; k < 2 * L; ++k) s_cnt[k][tid] = 0;
        const int per = (N + kReInitThreads - 1) / kReInitThreads, j0 = tid * per, j1 = j0 + per < N ? j0 + per : N;
        for (int j = j0; j < j1; ++j) {
            const int i = j / rows, k = j - i * rows, s = sbit(sp, k * Nk + i), sc = 2 * sbit(sp, i) - 1;
            const int c = le_class(P.ctab, Mr, L, k == 0 ? sc * mu[i] : sc * (2 * s - 1), s);
            cls[j] = (uint8_t)c;
            s_cnt[c][tid] += 1;
        }
        __syncthreads();
        if (tid < 2 * L) {
            int run = 0;
            for (int t = 0; t < kReInitThreads; ++t) { const int c = s_cnt[tid][t]; s_cnt[tid][t] = run; run += c; }
            s_tot[tid] = run;
        }
        __syncthreads();
        for (int j = j0; j < j1; ++j) {
            const int c = cls[j];
            const int p = s_cnt[c][tid]++;
            sv[(size_t)c * N + p] = (uint16_t)j;
            spos[j] = (uint16_t)p;
        }
    }
    if (tid == 0) {
        double E = (double)s_n0 * P.gT;
        for (int k = 1; k < rows; ++k) {
            if constexpr (SLICE == RE_SK) { long long n = s_n[k]; n /= 2; E += (double)n / P.sN; }
            else if constexpr (SLICE == RE_SKN || SLICE == RE_SPF) E += s_E[k];
            else if constexpr (kPercSlice<SLICE>) E += perc_energy_of<SLICE == RE_PLIN>(s_n[k], P.pc.sN);
            else if constexpr (kCommSlice<SLICE> || SLICE == RE_SAT) E += (double)s_n[k];
            else E += 0.0;
        }
        P.E_cur[r] = E;
        if (cache) {
            double z = 0.0;
            for (int k = 0; k < 2 * L; ++k) {
                P.st[(size_t)r * 2 * L + k] = s_tot[k];
                const double x = (double)s_tot[k] * re_class_f(P.ft, L, k);
                z += x;
                P.T[(size_t)r * 2 * L + k] = x;
            }
            P.zz[r] = z;
            P.acc_rate[r] = 0.5;
        }
        P.stats[(size_t)r * 2] = 0;
        P.stats[(size_t)r * 2 + 1] = 0;
    }
}

// bytes of LDS one replica takes in the LDS build below: spins, positions, classes, μ, set sizes, the RRR draws of 64 iterations
__host__ __device__ inline size_t le_rrr_lds_bytes(int64_t N, int64_t W, int64_t Nk)
{
    return (size_t)W * 4 + (((size_t)N * 2 + 3) & ~(size_t)3) + (((size_t)N + 3) & ~(size_t)3) + (((size_t)Nk + 3) & ~(size_t)3) +
           (size_t)2 * kLeLmax * 4 + (size_t)kRrrThreads * 8 * 4;
}

// rrrMC(X::DoubleGraph) (src/RRRMC.jl:221-290) on the Local Entropy ensemble; the builds and the register layout of the class weights are
// re_rrr_kernel's (LM >= L classes per half in registers, LDS = one wavefront per replica with its hot state in LDS).  Neighbours in the
// order of apply_move! / compute_staged! (LE.jl:166-174): a centre move's M replicas ascending, a replica move's centre; then the move.
// Perceptron and committee machine slices in the LDS build: as in re_rrr_kernel, their state is staged in LDS and all 64 lanes run the chain.
template <bool LDS, int LM, int SLICE>
__global__ __launch_bounds__(kRrrThreads) void le_rrr_kernel(LeParams P)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t le_lds[];
    int r;
    if constexpr (LDS) {
        r = (int)blockIdx.x;
    } else {
        r = blockIdx.x * blockDim.x + threadIdx.x;
        if (r >= P.R) return;
    }
    const int N = P.N, Nk = P.Nk, Mr = P.Mr, rows = P.M, L = P.L;
    uint32_t* const g_sp = P.sp + (size_t)r * P.W;
    int8_t* const g_mu = P.mu + (size_t)r * Nk;
    uint8_t* const g_cls = P.cls + (size_t)r * N;
    uint16_t* const g_spos = P.spos + (size_t)r * N;
    int32_t* const g_t = P.st + (size_t)r * 2 * L;
    uint16_t* const sv = P.sv + (size_t)r * 2 * L * N;
    uint32_t* sp = g_sp; int8_t* mu = g_mu; uint8_t* cls = g_cls; uint16_t* spos = g_spos; int32_t* t = g_t;
    uint32_t* l_rng = nullptr;
    if constexpr (LDS) {
        const int tid = (int)threadIdx.x, nt = (int)blockDim.x;
        uint32_t* l_sp = le_lds;                                                   // [W]
        uint16_t* l_spos = reinterpret_cast<uint16_t*>(l_sp + P.W);                // [N]
        uint8_t* l_cls = reinterpret_cast<uint8_t*>(l_spos) + ((2 * N + 3) & ~3);  // [N]
        int8_t* l_mu = reinterpret_cast<int8_t*>(l_cls + ((N + 3) & ~3));          // [Nk]
        int32_t* l_t = reinterpret_cast<int32_t*>(l_mu + ((Nk + 3) & ~3));         // [2 kLeLmax]
        l_rng = reinterpret_cast<uint32_t*>(l_t + 2 * kLeLmax);                    // [64][8]
        for (int i = tid; i < P.W; i += nt) l_sp[i] = g_sp[i];
        for (int i = tid; i < N; i += nt) { l_spos[i] = g_spos[i]; l_cls[i] = g_cls[i]; }
        for (int i = tid; i < Nk; i += nt) l_mu[i] = g_mu[i];
        if (tid < 2 * L) l_t[tid] = g_t[tid];
        __syncthreads();
        sp = l_sp; spos = l_spos; cls = l_cls; mu = l_mu; t = l_t;
    }
    const RrrView g_v = re_view(P, sp, r);
    RrrView v = g_v;
    if constexpr (LDS && SLICE == RE_SPF) {                                        // the rows' LocalFields behind the chain's own arrays, as in re_rrr_kernel
        if (P.spf_lds) spf_ens_attach(v, reinterpret_cast<char*>(le_lds) + ((le_rrr_lds_bytes(N, P.W, Nk) + 7) & ~(size_t)7), rows);
    }
    const auto g_pv = re_slice_view<SLICE>(P, r);                                  // PercView, or CommView for committee slices
    auto pv = g_pv;
    if constexpr (LDS && kPercSlice<SLICE>) {
        const int nw = rows * P.pc.PW;                                             // mask words, then 64 stabilities per word
        pv.pm = reinterpret_cast<uint64_t*>(reinterpret_cast<char*>(le_lds) + ((le_rrr_lds_bytes(N, P.W, Nk) + 7) & ~(size_t)7));
        pv.mm = pv.pm + nw;
        pv.ds = reinterpret_cast<int16_t*>(pv.mm + nw);
        for (int i = (int)threadIdx.x; i < nw; i += (int)blockDim.x) { pv.pm[i] = g_pv.pm[i]; pv.mm[i] = g_pv.mm[i]; }
        for (int i = (int)threadIdx.x; i < 64 * nw; i += (int)blockDim.x) pv.ds[i] = g_pv.ds[i];
        __syncthreads();
    }
    if constexpr (LDS && kCommSlice<SLICE>) {
        const int nm = rows * (int)comm_mk_row(P.cm.K2, P.cm.PW, comm_kind_of_slice(SLICE) == CK_QU), nd = rows * (int)comm_ds_row(P.cm.K2, P.cm.PW, comm_kind_of_slice(SLICE) == CK_QU);  // mask words, stabilities
        pv.mk = reinterpret_cast<uint64_t*>(reinterpret_cast<char*>(le_lds) + ((le_rrr_lds_bytes(N, P.W, Nk) + 7) & ~(size_t)7));
        pv.ds = reinterpret_cast<int16_t*>(pv.mk + nm);
        for (int i = (int)threadIdx.x; i < nm; i += (int)blockDim.x) pv.mk[i] = g_pv.mk[i];
        for (int i = (int)threadIdx.x; i < nd; i += (int)blockDim.x) pv.ds[i] = g_pv.ds[i];
        __syncthreads();
    }
    const bool worker = !LDS || threadIdx.x == 0 || kWaveSlice<SLICE>;
    const uint32_t rep = P.replica0 + (uint32_t)r;
    const double* tab = P.tab;
    const double* ft = P.ft;
    const uint8_t* ctab = P.ctab;
    double T[2 * LM];
#pragma unroll
    for (int q = 0; q < 2 * LM; ++q) T[q] = 0.0;
    for (int q = 0; q < 2 * L; ++q) {                                  // class q in register q (q < L) or q - L + LM
        const double x = P.T[(size_t)r * 2 * L + q];
        const int uq = q < L ? q : q - L + LM;
#pragma unroll
        for (int u = 0; u < 2 * LM; ++u) if (u == uq) T[u] = x;
    }
    double z = P.zz[r], E = P.E_cur[r], acc_rate = P.acc_rate[r];
    int64_t accepted = P.stats[(size_t)r * 2], staged_its = P.stats[(size_t)r * 2 + 1];
    int64_t ns = 0;
    long long next_sample = P.samp0;

    // ArraySet delete! / push! (ArraySets.jl:56-76)
    auto set_move = [&](int j, int k0, int k1) {
        const int p = spos[j];
        const int last = sv[(size_t)k0 * N + t[k0] - 1];
        sv[(size_t)k0 * N + p] = (uint16_t)last;
        spos[last] = (uint16_t)p;
        t[k0] -= 1;
        sv[(size_t)k1 * N + t[k1]] = (uint16_t)j;
        spos[j] = (uint16_t)t[k1];
        t[k1] += 1;
        cls[j] = (uint8_t)k1;
    };
    auto t_add = [&](double* A, int k, double d) {
#pragma unroll
        for (int u = 0; u < 2 * LM; ++u) if (u == k) A[u] += d;
    };
    auto t_sub = [&](double* A, int k, double d) {
#pragma unroll
        for (int u = 0; u < 2 * LM; ++u) if (u == k) A[u] -= d;
    };
    auto accept_c = [&](double c, double x, const uint32_t* q2, uint64_t g) {          // accept(c, x), RRRMC.jl:40-44
        bool ok = (c >= 1 && x >= 0);
        if (!ok) {
            const double a = c * det_exp(x);
            ok = a >= 1;
            if (!ok) {
                Philox4 o2;
                if constexpr (LDS) { o2.w[0] = q2[0]; o2.w[1] = q2[1]; }
                else o2 = philox4x32_10((uint32_t)g, (uint32_t)(g >> 32), rep, TAG_RRR | (1u << 8), P.k0, P.k1);
                ok = (double)((((uint64_t)o2.w[0] << 32) | o2.w[1]) >> 11) * 0x1.0p-53 < a;
            }
        }
        return ok;
    };
    // the neighbours' new classes for the configuration in sp / mu (or, staged, for the move applied in thought: sc / mu_i as given);
    // visit(y, k0, k1) for every neighbour whose class changes, in the reference's order
    auto neighbours = [&](int i, int km, int sc, int mui, auto&& visit) {
        const int jg = i * rows;
        if (km == 0) {
            for (int k = 1; k < rows; ++k) {
                const int sy = sbit(sp, k * Nk + i);
                const int k0 = cls[jg + k], k1 = le_class(ctab, Mr, L, sc * (2 * sy - 1), sy);
                if (k0 != k1) visit(jg + k, k0, k1);
            }
        } else {
            const int k0 = cls[jg], k1 = le_class(ctab, Mr, L, sc * mui, (sc + 1) >> 1);
            if (k0 != k1) visit(jg, k0, k1);
        }
    };

    for (int64_t base = 0; base < P.iters; base += (LDS ? kRrrThreads : P.iters)) {
    if constexpr (LDS) {
        __syncthreads();
        const uint64_t gl = P.g0 + (uint64_t)(base + 1 + (int64_t)threadIdx.x);
        const Philox4 a = philox4x32_10((uint32_t)gl, (uint32_t)(gl >> 32), rep, TAG_RRR, P.k0, P.k1);
        const Philox4 b = philox4x32_10((uint32_t)gl, (uint32_t)(gl >> 32), rep, TAG_RRR | (1u << 8), P.k0, P.k1);
        uint32_t* q = l_rng + threadIdx.x * 8;
        q[0] = a.w[0]; q[1] = a.w[1]; q[2] = a.w[2]; q[3] = a.w[3]; q[4] = b.w[0]; q[5] = b.w[1]; q[6] = b.w[2]; q[7] = b.w[3];
        __syncthreads();
    }
    const int64_t it_end = LDS ? (base + kRrrThreads < P.iters ? base + kRrrThreads : P.iters) : P.iters;
    if (worker)
    for (int64_t it = base + 1; it <= it_end; ++it) {
        if (it == next_sample) { next_sample += P.step; P.Es[ns * P.R + r] = E; ns += 1; }
        const uint64_t g = P.g0 + (uint64_t)it;
        const uint32_t* q2 = LDS ? l_rng + (it - base - 1) * 8 + 4 : nullptr;
        // rand_move (DeltaE.jl:146-167)
        Philox4 o;
        if constexpr (LDS) { const uint32_t* q = l_rng + (it - base - 1) * 8; o.w[0] = q[0]; o.w[1] = q[1]; o.w[2] = q[2]; o.w[3] = q[3]; }
        else o = philox4x32_10((uint32_t)g, (uint32_t)(g >> 32), rep, TAG_RRR, P.k0, P.k1);
        const double rr = (double)((((uint64_t)o.w[0] << 32) | o.w[1]) >> 11) * 0x1.0p-53 * z;
        // the classes in the reference's order 0 .. 2L-1: register u holds class u for u < L and class u - LM + L for u >= LM
        int k = -1, klast = 0;
        double cT = 0.0;
#pragma unroll
        for (int u = 0; u < 2 * LM; ++u) {
            const bool live = u < LM ? u < L : u - LM < L;
            if (live && k < 0) {
                cT += T[u];
                klast = u;
                if (rr < cT) k = u;
            }
        }
        if (k < 0) {                                                   // r < cT failed: walk back over the empty classes
            k = klast;
            bool found = false;
#pragma unroll
            for (int u = 2 * LM - 1; u >= 0; --u) {
                const bool live = u < LM ? u < L : u - LM < L;
                if (live && !found && u <= klast && T[u] != 0) { k = u; found = true; }
            }
        }
        const int kc = k < LM ? k : k - LM + L;                        // the reference's class index (0-based)
        const double dE0 = kc < L ? -tab[kc] : tab[kc - L];
        const uint64_t uu = ((uint64_t)o.w[2] << 32) | o.w[3];
        const int move = sv[(size_t)kc * N + (size_t)mulhi64(uu, (uint64_t)t[kc])];
        const int i = move / rows, km = move - i * rows, xm = km * Nk + i;
        // delta_energy_residual (LE.jl:276-290): 0.0 for the centre, the replica slice's delta_energy (not divided by M)
        const double dE1 = km == 0 ? 0.0 : re_residual<SLICE, LDS>(v, pv, xm, km, i);

        bool acc = false;
        if (acc_rate < P.staged_thr) {
            // staged branch: step_rrr (RRRMC.jl:131-138) = compute_staged! + compute_reverse_probabilities!, the list in order; the second
            // pass applies it
            staged_its += 1;
            const int s_old = sbit(sp, xm);
            const int sc_new = (2 * sbit(sp, i) - 1) * (km == 0 ? -1 : 1);
            const int mu_new = km == 0 ? mu[i] : mu[i] + 2 * (1 - 2 * s_old);
            double Tp[2 * LM];
#pragma unroll
            for (int u = 0; u < 2 * LM; ++u) Tp[u] = T[u];
            double zp = z;
            auto stage = [&](int, int k0, int k1) {
                const double f0 = re_class_f(ft, L, k0), f1 = re_class_f(ft, L, k1);
                t_sub(Tp, k0 < L ? k0 : k0 - L + LM, f0);
                t_add(Tp, k1 < L ? k1 : k1 - L + LM, f1);
                zp += f1 - f0;
            };
            neighbours(i, km, sc_new, mu_new, stage);
            { const int k0 = cls[move]; stage(move, k0, k0 >= L ? k0 - L : k0 + L); }
            const double c = z / zp;
            if (accept_c(c, -P.beta * dE1, q2, g)) {
                sflip(sp, xm);                                             // spinflip!(X, C, move)
                if (km != 0) { mu[i] = (int8_t)mu_new; re_slice_update<SLICE, LDS>(v, pv, xm, km, i); }
                neighbours(i, km, sc_new, mu_new, [&](int y, int k0, int k1) { set_move(y, k0, k1); });     // apply_staged!
                { const int k0 = cls[move]; set_move(move, k0, k0 >= L ? k0 - L : k0 + L); }
#pragma unroll
                for (int u = 0; u < 2 * LM; ++u) T[u] = Tp[u];
                z = zp;
                E += dE0 + dE1;
                accepted += 1;
                acc = true;
            }
        } else {
            // direct branch: apply_move! (DeltaE.jl:232-295), undone by a second apply_move! on rejection
            for (int pass = 0; pass < 2; ++pass) {
                sflip(sp, xm);
                if (km != 0) {
                    mu[i] = (int8_t)(mu[i] + 2 * (2 * sbit(sp, xm) - 1));
                    // the undo pass takes the slice's swap path (move_last == move); perceptron slices: once, below, when accepted
                    if constexpr (!kWaveSlice<SLICE>) re_slice_update<SLICE>(v, xm);
                }
                double zp = z;
                auto apply = [&](int y, int k0, int k1) {
                    const double f0 = re_class_f(ft, L, k0), f1 = re_class_f(ft, L, k1);
                    t_sub(T, k0 < L ? k0 : k0 - L + LM, f0);
                    t_add(T, k1 < L ? k1 : k1 - L + LM, f1);
                    zp += f1 - f0;
                    set_move(y, k0, k1);
                };
                neighbours(i, km, 2 * sbit(sp, i) - 1, mu[i], apply);
                { const int k0 = cls[move]; apply(move, k0, k0 >= L ? k0 - L : k0 + L); }
                const double cc = z / zp;
                z = zp;
                if (pass == 1) break;                                      // that was the undo
                if (accept_c(cc, -P.beta * dE1, q2, g)) { E += dE0 + dE1; accepted += 1; acc = true; break; }
            }
            if constexpr (kWaveSlice<SLICE>) { if (acc && km != 0) re_slice_update<SLICE, LDS>(v, pv, xm, km, i); }
        }
        acc_rate = acc_rate * (1 - P.lambda) + (acc ? 1.0 : 0.0) * P.lambda;          // RRRMC.jl:281
    }
    }
    if (worker) {
        for (int q = 0; q < 2 * L; ++q) {
            double x = 0.0;
#pragma unroll
            for (int u = 0; u < 2 * LM; ++u) if (u == (q < L ? q : q - L + LM)) x = T[u];
            P.T[(size_t)r * 2 * L + q] = x;
        }
        P.zz[r] = z; P.E_cur[r] = E; P.acc_rate[r] = acc_rate;
        P.stats[(size_t)r * 2] = accepted; P.stats[(size_t)r * 2 + 1] = staged_its;
    }
    if constexpr (LDS && kPercSlice<SLICE>) {
        __syncthreads();
        const int nw = rows * P.pc.PW;
        for (int i = (int)threadIdx.x; i < nw; i += (int)blockDim.x) { g_pv.pm[i] = pv.pm[i]; g_pv.mm[i] = pv.mm[i]; }
        for (int i = (int)threadIdx.x; i < 64 * nw; i += (int)blockDim.x) g_pv.ds[i] = pv.ds[i];
    }
    if constexpr (LDS && kCommSlice<SLICE>) {
        __syncthreads();
        const int nm = rows * (int)comm_mk_row(P.cm.K2, P.cm.PW, comm_kind_of_slice(SLICE) == CK_QU), nd = rows * (int)comm_ds_row(P.cm.K2, P.cm.PW, comm_kind_of_slice(SLICE) == CK_QU);
        for (int i = (int)threadIdx.x; i < nm; i += (int)blockDim.x) g_pv.mk[i] = pv.mk[i];
        for (int i = (int)threadIdx.x; i < nd; i += (int)blockDim.x) g_pv.ds[i] = pv.ds[i];
    }
    if constexpr (LDS && SLICE == RE_SPF) {
        if (P.spf_lds) spf_ens_detach(v, g_v, rows);
    }
    if constexpr (LDS) {
        __syncthreads();
        const int tid = (int)threadIdx.x, nt = (int)blockDim.x;
        for (int i = tid; i < P.W; i += nt) g_sp[i] = sp[i];
        for (int i = tid; i < N; i += nt) { g_spos[i] = spos[i]; g_cls[i] = cls[i]; }
        for (int i = tid; i < Nk; i += nt) g_mu[i] = mu[i];
        if (tid < 2 * L) g_t[tid] = t[tid];
    }
}

// standardMC (src/RRRMC.jl:81-127): delta_energy = 2γT lfields[j] + delta_energy_residual (LE.jl:156-164, 276-294); the SITE stream names
// ABI site j, rand() < exp(-β ΔE) on the ACCEPT_F64 stream.  E starts from E_cur (le_init_kernel, or the run a resumed call continues).
template <int SLICE>
__global__ __launch_bounds__(kRrrThreads) void le_standard_kernel(LeParams P)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= P.R) return;
    const int Nk = P.Nk, rows = P.M;
    uint32_t* sp = P.sp + (size_t)r * P.W;
    int8_t* mu = P.mu + (size_t)r * Nk;
    const RrrView v = re_view(P, sp, r);
    const auto pv = re_slice_view<SLICE>(P, r);
    const uint32_t rep = P.replica0 + (uint32_t)r;
    double E = P.E_cur[r];
    int64_t accepted = 0, ns = 0;
    long long next_sample = P.samp0;
    for (int64_t it = 1; it <= P.iters; ++it) {
        if (it == next_sample) { next_sample += P.step; P.Es[ns * P.R + r] = E; ns += 1; }
        const uint64_t g = P.g0 + (uint64_t)it;
        const int j = (int)site_of(P.k0, P.k1, g, (uint32_t)P.N);
        const int i = j / rows, k = j - i * rows, x = k * Nk + i;
        const int sg = 2 * sbit(sp, x) - 1, sc = 2 * sbit(sp, i) - 1;
        const int lf = k == 0 ? sc * mu[i] : sc * sg;
        const double dE = P.g2 * (double)lf + (k == 0 ? 0.0 : re_residual<SLICE>(v, pv, x, k, i));
        const double xx = -P.beta * dE;
        const bool acc = (xx >= 0.0) || (rand53(P.k0, P.k1, g, rep) < det_exp(xx));          // RRRMC.jl:39
        if (acc) {
            sflip(sp, x);
            if (k != 0) {
                mu[i] = (int8_t)(mu[i] - 2 * sg);
                re_slice_update<SLICE, false>(v, pv, x, k, i);
            }
            E += dE;
            accepted += 1;
        }
    }
    P.E_cur[r] = E;
    P.stats[(size_t)r * 2] = accepted; P.stats[(size_t)r * 2 + 1] = 0;
}

// The observables, read-only (unlike the reference's LEenergies / cenergy, which call energy and so reset the slice caches, this reads the
// configuration only: a hook that calls them does not change the run).  Threads e < R (M+1): energy of row k = e % (M+1) of replica e / (M+1)
// under the slice graph — row 0 is cenergy (LE.jl:271-274), rows 1..M LEenergies (:259-269).  Threads e - R (M+1) < R M M: distances
// (:309-318), the Hamming distance of replica rows k1 and k2, popcounts of the XOR of the rows.
template <int SLICE>
__global__ __launch_bounds__(64) void le_obs_kernel(LeParams P)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    const int rows = P.M, Mr = P.Mr, Nk = P.Nk;
    const int ne = P.R * rows;
    if (e < ne) {
        const int r = e / rows, k = e - r * rows;
        const RrrView v = re_view(P, P.sp + (size_t)r * P.W, r);
        P.Eslice[e] = re_slice_energy<SLICE>(P, v, k);
        return;
    }
    const int d = e - ne;
    if (d >= P.R * Mr * Mr) return;
    const int r = d / (Mr * Mr), q = d - r * Mr * Mr, k1 = q / Mr, k2 = q - k1 * Mr;
    const uint32_t* sp = P.sp + (size_t)r * P.W;
    int64_t n = 0;
    for (int w = 0; 32 * w < Nk; ++w)
        n += __popc(le_row_word(sp, (k1 + 1) * Nk, w, Nk, P.N) ^ le_row_word(sp, (k2 + 1) * Nk, w, Nk, P.N));
    P.dist[d] = n;
}

// debug mode (rrrmc_set_debug_checks): after a sampler call every replica's energy(X, C) is re-evaluated from its configuration and compared
// with the tracked E (|ΔE| <= 1e-10 max(1, |E|): the bound of RRRMC.jl:250, relative once |E| > 1 — the inner energy n γT reaches 10^4 and
// more at N = 65 535, where the rounding of E += ΔE0 alone exceeds an absolute 1e-10); μ, and after rrrMC every site's class, membership
// and the set sizes, must equal what the configuration gives; GraphSKNormal replica slices: the cached fields within 1e-10 Nk of recomputed
// ones.
template <int SLICE>
__global__ __launch_bounds__(64) void le_check_kernel(LeParams P, int cache)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= P.R) return;
    const int Nk = P.Nk, rows = P.M, Mr = P.Mr, L = P.L, N = P.N;
    const uint32_t* sp = P.sp + (size_t)r * P.W;
    const int8_t* mu = P.mu + (size_t)r * Nk;
    const RrrView v = re_view(P, P.sp + (size_t)r * P.W, r);
    bool bad = false;
    long long n0 = 0;
    for (int i = 0; i < Nk; ++i) {
        int m = 0;
        for (int k = 1; k < rows; ++k) m += 2 * sbit(sp, k * Nk + i) - 1;
        bad = bad || m != mu[i];
        n0 -= (2 * sbit(sp, i) - 1) * m;
    }
    double E = (double)n0 * P.gT;
    for (int k = 1; k < rows; ++k) E += re_slice_energy<SLICE>(P, v, k);
    const double d = E - P.E_cur[r], tol = 1e-10 * (E < -1.0 ? -E : E > 1.0 ? E : 1.0);
    bad = bad || !(d <= tol && d >= -tol);
    if constexpr (SLICE == RE_SKN) {
        for (int k = 1; k < rows; ++k)
            for (int i = 0; i < Nk; ++i) {
                const int si = sbit(sp, k * Nk + i);
                const double* Ji = P.Jd + (size_t)i * Nk;
                double lf = 0.0;
                for (int j = 0; j < Nk; ++j) lf += (double)(1 - 2 * (si ^ sbit(sp, k * Nk + j))) * Ji[j];
                const double dd = v.slf[((size_t)v.scur[k] * rows + k) * Nk + i] - 2 * lf;
                bad = bad || !(dd <= 1e-10 * Nk && dd >= -1e-10 * Nk);
            }
    }
    if constexpr (SLICE == RE_SPF) bad = bad || spf_state_bad(P, v, sp, 1, rows);
    if constexpr (kPercSlice<SLICE>) bad = bad || perc_state_bad<SLICE == RE_PLIN>(P.pc, perc_view(P.pc, r), sp, 1, Nk, N);
    if constexpr (kCommSlice<SLICE>) bad = bad || comm_state_bad<comm_kind_of_slice(SLICE)>(P.cm, comm_view<comm_kind_of_slice(SLICE)>(P.cm, r), sp, 1, Nk, N);
    if (cache) {
        int cnt[2 * kLeLmax];
        for (int k = 0; k < 2 * L; ++k) cnt[k] = 0;
        for (int j = 0; j < N; ++j) {
            const int i = j / rows, k = j - i * rows, s = sbit(sp, k * Nk + i), sc = 2 * sbit(sp, i) - 1;
            const int c = le_class(P.ctab, Mr, L, k == 0 ? sc * mu[i] : sc * (2 * s - 1), s);
            bad = bad || c != P.cls[(size_t)r * N + j] || P.sv[((size_t)r * 2 * L + c) * N + P.spos[(size_t)r * N + j]] != j;
            cnt[c] += 1;
        }
        for (int k = 0; k < 2 * L; ++k) bad = bad || cnt[k] != P.st[(size_t)r * 2 * L + k];
    }
    if (bad) { atomicAdd(&P.flag[0], 1); P.flag[1] = r; }
}

}  // namespace rrrmc
