// gfx950 kernels for the Robust Ensemble (src/graphs/RE.jl): GraphRobustEnsemble{M,γ,β,G} = the inner graph GraphRE{M,γ,β}, which couples
// the M replicas of every spin through μ_i = Σ_k σ_(i,k), plus M slices of one graph G — GraphEmpty (Graph0RE), binary GraphSK (GraphSKRE),
// GraphSKNormal (src/REAliases.jl:20-38), GraphEANormal (GraphEARE, :43-75), the pattern machines and GraphSAT.  Samplers: rrrMC(X::DoubleGraph) (src/RRRMC.jl:221-290) with the DeltaECache{Float64,L} over
// ArraySets (src/DeltaE.jl:63-295, src/ArraySets.jl), standardMC (src/RRRMC.jl:81-127), and REenergies (RE.jl:285-301).
//
// Layout.  Spins cross the ABI in the reference's order j = i M + k (spin i of replica k, RE.jl:76-95); the kernels work on a
// slice-major copy x = k Nk + i, so that a binary-SK slice is a contiguous bit row and its field one popcount row (slice_delta).  The
// classes, set members and positions are indexed by the ABI site j: the ArraySets hold the reference's site ids, so rand(aset) picks the
// same site.  GraphRE's cache (lfields[j] = σ_j fk(μ_i − σ_j), RE.jl:96-104) is a table look-up over the stored μ_i and never stored:
// update_cache! recomputes the whole group (RE.jl:139-160) and its move_last swap (:125-135) gives the same table values.
//
// Classes.  findk compares Float64s exactly (DeltaE.jl:53-60) and fk(−x) = −fk(x) holds exactly in IEEE arithmetic, so the level of a site
// is the integer |mū| / 2 (mū = μ_i − σ_j has the parity of M − 1); `up` is decided on the Float64 value as DeltaE.jl:83 does.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rrr_kernels.hpp"   // RrrView, sbit / sflip, slice_delta, skn_update, kRrrThreads, TAG_RRR, det_exp
#include "perc_kernels.hpp"  // the binary perceptron slices (PercParams, perc_residual, perc_update, perc_init_rows)
#include "xentr_kernels.hpp" // the cross-entropy perceptron as the g of a field wrapper (XentrParams, xentr_residual, xentr_update)
#include "comm_kernels.hpp"  // the binary committee machine slices (CommParams, comm_residual, comm_update, comm_init_rows)
#include "sat_kernels.hpp"   // the K-SAT slices (SatTable, sat_delta, sat_row_energy, sat_init_rows)
#include "pspin_kernels.hpp" // GraphPSpin3 as the g of a field wrapper (PspinTable, pspin_delta, pspin_energy, pspin_init_row)

namespace rrrmc {

enum ReSlice { RE_EMPTY = 0, RE_SK = 1, RE_SKN = 2,          // GraphEmpty (Graph0RE), binary GraphSK (GraphSKRE), GraphSKNormal
               RE_PSTEP = 3, RE_PLIN = 4,                    // GraphPercStep (GraphPercStepRE), GraphPercLinear (GraphPercLinearRE)
               RE_CSTEP = 5, RE_CRELU = 6,                   // GraphCommStep (GraphCommStepRE), GraphCommReLU (GraphCommReLURE)
               RE_SAT = 8,                                   // GraphSAT (GraphSATRE); 7 is unassigned, as in the ABI
               RE_CQU = 9,                                   // GraphCommQu (GraphCommQuRE)
               RE_PXE = 11,                                  // GraphPercXEntr: the g of GraphAddFields / GraphAddSubFields only (af_kernels.hpp); 10 is unassigned
               RE_SPF = 12,                                  // GraphEANormal / GraphRRGNormal: sparse Float64 couplings (GraphEARE, GraphEALE, GraphEATLE)
               RE_MIXED = 13,                                // GraphMixed: the g of the field wrappers over a mix only (mixed_kernels.hpp)
               RE_PSPIN3 = 14 };                             // GraphPSpin3: the g of the field wrappers made by rrrmc_ctx_create_pspin3 only (pspin_kernels.hpp)
template <int SLICE> constexpr bool kPercSlice = SLICE == RE_PSTEP || SLICE == RE_PLIN;
template <int SLICE> constexpr bool kCommSlice = SLICE == RE_CSTEP || SLICE == RE_CRELU || SLICE == RE_CQU;
// slices whose state is a pure function of the configuration, updated once per accepted move by the whole wavefront in the LDS builds
// (a K-SAT slice is not one: like the binary SK slice it keeps no state, its residual is recomputed from the spins by the worker thread)
template <int SLICE> constexpr bool kWaveSlice = kPercSlice<SLICE> || kCommSlice<SLICE> || SLICE == RE_PXE;
constexpr int kReMmax = 32;                                 // replicas of the ensemble; levels L = ceil(M / 2) <= 16

struct ReParams {
    // the slice graph, shared by the M slices
    const uint32_t* Jb; int Wk; double sN;                  // binary GraphSK: rows of J as 32-bit words, sqrt(Nk)
    const double* Jd;                                       // GraphSKNormal: [Nk][Nk]
    PercParams pc;                                          // perceptron slices: the shared patterns, every slice's Stabilities
    XentrParams xe;                                         // GraphPercXEntr (with pc): the loss table, the global build's term buffer
    CommParams cm;                                          // committee machine slices: the same for GraphCommStep / GraphCommReLU / GraphCommQu
    SatTable sat;                                           // K-SAT slices: the shared occurrence program (no per-slice state)
    PspinTable ps3;                                         // GraphPSpin3 under a field wrapper: the partner table (no per-chain state)
    double* slf;                                            // [R][2][M][Nk]  every slice's lfields / lfields_last (SK.jl:212-276)
    int32_t* smv;                                           // [R][M]         move_last of every slice (-1 = none)
    uint8_t* scur;                                          // [R][M]         which of the two arrays is `lfields`
    // sparse Float64 slices (GraphEANormal, GraphRRGNormal): the shared graph and every slice's LocalFields{Float64} (EA.jl:584-653)
    const int32_t* A; const double* Jf; int K;              // [Nk][K] neighbour table (ascending rows, a neighbour may repeat) and couplings
    double* flf;                                            // [R][M][Nk]     lfields of every slice
    double* fundo;                                          // [R][M][K+1]    the part of lfields_last the undo path reads
    int32_t* fml;                                           // [R][M]         move_last of every slice (-1 = none)
    int spf_lds;                                            // the LDS builds stage flf / fundo / fml in LDS (they fit behind the chain's arrays)
    // tables: host libm (rrrmc_re_tables) and the sampler's class weights
    const double* tab;                                      // [M]    ΔElist(GraphRE): fk(mū) for mū = -(M-1), -(M-3), ..., M-1 (RE.jl:53-56)
    const double* etab;                                     // [M+1]  log(2 cosh(γ μ)) / β for μ = -M, -M+2, ..., M (RE.jl:90-93)
    const double* ft;                                       // [L]    det_exp(-β allΔE[a]) (DeltaE.jl:91)
    // state
    uint32_t* abi;                                          // [R][W] spins in ABI site order (the context's configuration)
    uint32_t* sp;                                           // [R][W] slice-major working copy
    int8_t* mu;                                             // [R][Nk]      μ_i
    uint8_t* cls;                                           // [R][N]       DeltaECache.pos (a + L up), by ABI site
    uint16_t* sv;                                           // [R][2L][N]   ArraySet.v of every class
    uint16_t* spos;                                         // [R][N]       position of a site inside its set
    int32_t* st;                                            // [R][2L]      set sizes
    double* T;                                              // [R][2L]
    double* zz; double* E_cur; double* acc_rate;            // [R]
    int64_t* stats;                                         // [R][2]       accepted, staged iterations (this call)
    double* Es;                                             // [nsamples][R]
    double* Eslice;                                         // [R][M]       REenergies
    int32_t* flag;                                          // [2]          debug checks: failures, a failing replica
    double beta, staged_thr, lambda;
    uint64_t g0;
    int64_t iters, step;
    long long samp0;                                        // the call's first sample is taken before its iteration samp0
    uint32_t k0, k1, replica0;
    int Nk, M, L, N, W, R;
};

// the slice helpers of rrr_kernels.hpp work on a RrrView of the slice-major copy
__device__ __forceinline__ RrrView re_view(const ReParams& P, uint32_t* sp, int r)
{
    RrrView v{};
    v.sp = sp; v.N = P.N; v.Nk = P.Nk; v.M = P.M; v.K = 0; v.wide = 0;
    v.Jb = P.Jb; v.Wk = P.Wk; v.sN = P.sN;
    v.Jd = P.Jd;
    v.slf = P.slf ? P.slf + (size_t)r * 2 * P.M * P.Nk : nullptr;
    v.smv = P.smv ? P.smv + (size_t)r * P.M : nullptr;
    v.scur = P.scur ? P.scur + (size_t)r * P.M : nullptr;
    if (P.Jf) {
        v.A = P.A; v.K = P.K; v.Jf = P.Jf;
        v.flf = P.flf + (size_t)r * P.M * P.Nk;
        v.fundo = P.fundo + (size_t)r * P.M * (P.K + 1);
        v.fml = P.fml + (size_t)r * P.M;
    }
    v.nk_magic = (uint32_t)((0x100000000ull + (uint32_t)P.Nk - 1u) / (uint32_t)P.Nk);
    return v;
}

// delta_energy_residual (RE.jl:303-310) = delta_energy(X1[k], C1[k], i), NOT divided by M: 0 (GraphEmpty), lfields[i] / sqrt(Nk) (GraphSK,
// SK.jl:137-140, the integer field by popcounts), lfields[i] (GraphSKNormal, SK.jl:278-284), -lfields[i] (sparse Float64 slices, EA.jl:655-663)
template <int SLICE>
__device__ __forceinline__ double re_residual(const RrrView& v, int x, int k, int i)
{
    if constexpr (SLICE == RE_EMPTY) return 0.0;
    else if constexpr (SLICE == RE_SK) return (double)slice_delta(v, x) / v.sN;
    else if constexpr (SLICE == RE_SPF) return -v.flf[(size_t)k * v.Nk + i];
    else return v.slf[((size_t)v.scur[k] * v.M + k) * v.Nk + i];
}
// the slice graph's update_cache! after the bit flip (spinflip!(X1[k], C1[k], i), RE.jl:246-253); the binary SK field is recomputed.
// Sparse Float64 slices: GraphQuant's helper (rrr_kernels.hpp) on the same RrrView members, so that the move_last path and the order in
// which a repeated neighbour receives its bonds are written once.
template <int SLICE>
__device__ __forceinline__ void re_slice_update(const RrrView& v, int x)
{
    if constexpr (SLICE == RE_SKN) skn_update(v, x);
    else if constexpr (SLICE == RE_SPF) spf_slice_update(v, x);
}
// sparse Float64 slices in the LDS builds: bytes of one chain's flf / fundo / fml (rows = M, or M + 1 with a centre), their staging behind
// `lds` (8-byte aligned) and the copy back at the end of the call.  Called by the whole workgroup.
__host__ __device__ inline size_t spf_ens_lds_bytes(int64_t rows, int64_t Nk, int64_t K)
{
    return (size_t)8 * (size_t)rows * (size_t)(Nk + K + 1) + (size_t)4 * (size_t)rows;
}
__device__ inline void spf_ens_attach(RrrView& v, char* lds, int rows)
{
    const int nf = rows * v.Nk, nu = rows * (v.K + 1), tid = (int)threadIdx.x, nt = (int)blockDim.x;
    double* l_lf = reinterpret_cast<double*>(lds);
    double* l_undo = l_lf + nf;
    int32_t* l_ml = reinterpret_cast<int32_t*>(l_undo + nu);
    for (int q = tid; q < nf; q += nt) l_lf[q] = v.flf[q];
    for (int q = tid; q < nu; q += nt) l_undo[q] = v.fundo[q];
    for (int q = tid; q < rows; q += nt) l_ml[q] = v.fml[q];
    __syncthreads();
    v.flf = l_lf; v.fundo = l_undo; v.fml = l_ml;
}
__device__ inline void spf_ens_detach(const RrrView& v, const RrrView& g, int rows)
{
    const int nf = rows * v.Nk, nu = rows * (v.K + 1), tid = (int)threadIdx.x, nt = (int)blockDim.x;
    __syncthreads();
    for (int q = tid; q < nf; q += nt) g.flf[q] = v.flf[q];
    for (int q = tid; q < nu; q += nt) g.fundo[q] = v.fundo[q];
    for (int q = tid; q < rows; q += nt) g.fml[q] = v.fml[q];
}
// the same two with the perceptron slices (perc_kernels.hpp), whose state is not part of the RrrView; WAVE: the wavefront-wide update
template <int SLICE, bool WAVE = false>
__device__ __forceinline__ double re_residual(const RrrView& v, const PercView& pv, int x, int k, int i)
{
    if constexpr (kPercSlice<SLICE>) return perc_residual<SLICE == RE_PLIN>(pv, k, i, sbit(v.sp, x));
    else return re_residual<SLICE>(v, x, k, i);
}
template <int SLICE, bool WAVE>
__device__ __forceinline__ void re_slice_update(const RrrView& v, const PercView& pv, int x, int k, int i)
{
    if constexpr (kPercSlice<SLICE>) perc_update<SLICE == RE_PLIN, WAVE>(pv, k, i, sbit(v.sp, x));
    else re_slice_update<SLICE>(v, x);
}
// ... and with the committee machine slices (comm_kernels.hpp); WAVE: all 64 lanes call it with identical values (GraphCommQu shares
// the patterns among them)
template <int SLICE, bool WAVE = false>
__device__ __forceinline__ double re_residual(const RrrView& v, const CommView& cv, int x, int k, int i)
{
    static_assert(kCommSlice<SLICE>, "a CommView goes with a committee machine slice");
    return comm_residual<comm_kind_of_slice(SLICE), WAVE>(cv, k, i, sbit(v.sp, x));
}
template <int SLICE, bool WAVE>
__device__ __forceinline__ void re_slice_update(const RrrView& v, const CommView& cv, int x, int k, int i)
{
    static_assert(kCommSlice<SLICE>, "a CommView goes with a committee machine slice");
    comm_update<comm_kind_of_slice(SLICE), WAVE>(cv, k, i, sbit(v.sp, x));
}
// ... and with the cross-entropy perceptron (xentr_kernels.hpp), M = 1; WAVE: the wavefront forms the terms, every lane adds them in order
template <int SLICE, bool WAVE = false>
__device__ __forceinline__ double re_residual(const RrrView& v, const XentrView& xv, int x, int /*k*/, int i)
{
    static_assert(SLICE == RE_PXE, "a XentrView goes with GraphPercXEntr");
    if constexpr (WAVE) return xentr_residual_wave(xv, i, sbit(v.sp, x));
    else return xentr_residual(xv, i, sbit(v.sp, x));
}
template <int SLICE, bool WAVE>
__device__ __forceinline__ void re_slice_update(const RrrView& v, const XentrView& xv, int x, int /*k*/, int i)
{
    static_assert(SLICE == RE_PXE, "a XentrView goes with GraphPercXEntr");
    xentr_update<WAVE>(xv, i, sbit(v.sp, x));
}
// ... and with the K-SAT slices (sat_kernels.hpp): delta_energy from the row's spins, no update_cache!
template <int SLICE, bool WAVE = false>
__device__ __forceinline__ double re_residual(const RrrView& v, const SatTable& sv, int x, int /*k*/, int i)
{
    static_assert(SLICE == RE_SAT, "a SatTable goes with a K-SAT slice");
    return (double)sat_delta(sv, v.sp, x - i, i);
}
template <int SLICE, bool WAVE>
__device__ __forceinline__ void re_slice_update(const RrrView&, const SatTable&, int, int, int)
{
    static_assert(SLICE == RE_SAT, "a SatTable goes with a K-SAT slice");
}
// ... and with GraphPSpin3 (pspin_kernels.hpp), M = 1: delta_energy from the spins, no update_cache!
template <int SLICE, bool WAVE = false>
__device__ __forceinline__ double re_residual(const RrrView& v, const PspinTable& pt, int x, int /*k*/, int i)
{
    static_assert(SLICE == RE_PSPIN3, "a PspinTable goes with GraphPSpin3");
    return (double)pspin_delta(pt, i, PspinRowBits{v.sp, x - i});
}
template <int SLICE, bool WAVE>
__device__ __forceinline__ void re_slice_update(const RrrView&, const PspinTable&, int, int, int)
{
    static_assert(SLICE == RE_PSPIN3, "a PspinTable goes with GraphPSpin3");
}
// the view of one chain's slice state that the kernels pass to the two above
template <int SLICE, class PP>
__device__ __forceinline__ auto re_slice_view(const PP& P, int r)
{
    if constexpr (SLICE == RE_SAT) return P.sat;
    else if constexpr (SLICE == RE_PSPIN3) return P.ps3;
    else if constexpr (SLICE == RE_PXE) return xentr_view(P.pc, P.xe, r);
    else if constexpr (kCommSlice<SLICE>) return comm_view<comm_kind_of_slice(SLICE)>(P.cm, r);
    else return perc_view(P.pc, r);
}
// class of ABI site j with spin bit s, for the group's μ = mub + σ: a + L up (DeltaE.jl:80-86 with lfields[j] = σ_j fk(mū), RE.jl:101)
__device__ __forceinline__ int re_class(const double* tab, int M, int L, int mub, int s)
{
    const double dE = (double)(2 * s - 1) * tab[(mub + M - 1) >> 1];
    const int a = (mub < 0 ? -mub : mub) >> 1;
    const int up = dE > 0 || (dE == 0 && s == 1);
    return a + L * up;
}
__device__ __forceinline__ double re_class_f(const double* ft, int L, int k) { return k >= L ? ft[k - L] : 1.0; }     // get_class_f

// sparse Float64 slices: lf_x = the sum over row x of the table, in order, of -J σx σy for the slice whose spins start at bit `off` (EA.jl:590-600)
__device__ __forceinline__ double spf_site_lf(const ReParams& P, const uint32_t* sp, int off, int x)
{
    const int K = P.K, sx = 2 * sbit(sp, off + x) - 1;
    double fl = 0.0;
    for (int q = 0; q < K; ++q) {
        const int sy = 2 * sbit(sp, off + P.A[(size_t)x * K + q]) - 1;
        fl = fl - P.Jf[(size_t)x * K + q] * (double)sx * (double)sy;
    }
    return fl;
}
// ... their caches rebuilt as energy(X1[k], C1[k]) does (EA.jl:584-611) for rows k0 .. rows - 1, by a whole workgroup: lfields = 2 lf,
// E1 = (Σ_x lf_x) / 2 summed in site order into s_E[k], the undo record cleared, move_last = none (every row's, an unused centre row included)
__device__ inline void spf_init_rows(const ReParams& P, const RrrView& v, const uint32_t* sp, int k0, int rows, double* s_E)
{
    const int Nk = P.Nk, K = P.K, tid = (int)threadIdx.x, nt = (int)blockDim.x;
    for (int x = k0 * Nk + tid; x < rows * Nk; x += nt) {
        const int k = x / Nk;
        v.flf[x] = spf_site_lf(P, sp, k * Nk, x - k * Nk);
    }
    __syncthreads();
    for (int k = tid; k < rows; k += nt) {
        if (k >= k0) {
            double* lf = v.flf + (size_t)k * Nk;
            double E1 = 0.0;
            for (int x = 0; x < Nk; ++x) { const double fl = lf[x]; E1 = E1 + fl; lf[x] = 2.0 * fl; }
            s_E[k] = E1 / 2;
        }
        v.fml[k] = -1;
        for (int q = 0; q <= K; ++q) v.fundo[(size_t)k * (K + 1) + q] = 0.0;
    }
    __syncthreads();
}
// ... debug mode: the cached fields of rows k0 .. rows - 1 within 1e-10 K of recomputed ones
__device__ inline bool spf_state_bad(const ReParams& P, const RrrView& v, const uint32_t* sp, int k0, int rows)
{
    bool bad = false;
    for (int k = k0; k < rows; ++k)
        for (int x = 0; x < P.Nk; ++x) {
            const double dd = v.flf[(size_t)k * P.Nk + x] - 2 * spf_site_lf(P, sp, k * P.Nk, x);
            bad = bad || !(dd <= 1e-10 * P.K && dd >= -1e-10 * P.K);
        }
    return bad;
}

// energy(X1[k], C1[k]) of one slice from the slice-major spins: GraphSK n / sqrt(Nk) (SK.jl:62-96), GraphSKNormal recomputed in the
// reference's order (SK.jl:212-237); 0 for GraphEmpty.  Sequential (REenergies, debug checks).
template <int SLICE>
__device__ inline double re_slice_energy(const ReParams& P, const RrrView& v, int k)
{
    const int Nk = P.Nk;
    if constexpr (SLICE == RE_SK) {
        long long n = 0;
        for (int i = 0; i < Nk; ++i) n -= slice_delta(v, k * Nk + i) / 2;
        n /= 2;
        return (double)n / P.sN;
    } else if constexpr (SLICE == RE_SKN) {
        double n = 0.0;
        for (int i = 0; i < Nk; ++i) {
            const int si = sbit(v.sp, k * Nk + i);
            const double* Ji = P.Jd + (size_t)i * Nk;
            double lf = 0.0;
            for (int j = 0; j < Nk; ++j) lf += (double)(1 - 2 * (si ^ sbit(v.sp, k * Nk + j))) * Ji[j];
            n -= lf;
        }
        n /= 2;
        return n;
    } else if constexpr (SLICE == RE_SPF) {
        double E1 = 0.0;                                                  // EA.jl:584-611: lf_x in table order, summed in site order, halved
        for (int x = 0; x < Nk; ++x) E1 = E1 + spf_site_lf(P, v.sp, k * Nk, x);
        return E1 / 2;
    } else if constexpr (kPercSlice<SLICE>) {
        return perc_row_energy<SLICE == RE_PLIN>(P.pc, v.sp, k * Nk, Nk, P.N);
    } else if constexpr (kCommSlice<SLICE>) {
        return comm_row_energy<comm_kind_of_slice(SLICE)>(P.cm, v.sp, k * Nk, P.N);
    } else if constexpr (SLICE == RE_SAT) {
        return (double)sat_row_energy(P.sat, v.sp, k * Nk);
    } else if constexpr (SLICE == RE_PXE) {
        return xentr_row_energy(P.pc, P.xe, v.sp, P.N);
    } else if constexpr (SLICE == RE_PSPIN3) {
        return (double)pspin_energy(P.ps3, PspinRowBits{v.sp, k * Nk});
    } else {
        return 0.0;
    }
}

// ABI order <-> slice-major copy, one thread per output word
__global__ __launch_bounds__(256) void re_to_slices_kernel(ReParams P)
{
    const int w = blockIdx.x * blockDim.x + threadIdx.x, r = blockIdx.y;
    if (w >= P.W) return;
    const uint32_t* a = P.abi + (size_t)r * P.W;
    uint32_t word = 0u;
    for (int b = 0; b < 32; ++b) {
        const int x = 32 * w + b;
        if (x >= P.N) break;
        const int k = x / P.Nk, i = x - k * P.Nk, j = i * P.M + k;
        word |= ((a[j >> 5] >> (j & 31)) & 1u) << b;
    }
    P.sp[(size_t)r * P.W + w] = word;
}
__global__ __launch_bounds__(256) void re_from_slices_kernel(ReParams P)
{
    const int w = blockIdx.x * blockDim.x + threadIdx.x, r = blockIdx.y;
    if (w >= P.W) return;
    const uint32_t* s = P.sp + (size_t)r * P.W;
    uint32_t word = 0u;
    for (int b = 0; b < 32; ++b) {
        const int j = 32 * w + b;
        if (j >= P.N) break;
        const int i = j / P.M, k = j - i * P.M, x = k * P.Nk + i;
        word |= ((s[x >> 5] >> (x & 31)) & 1u) << b;
    }
    P.abi[(size_t)r * P.W + w] = word;
}

// energy(X::GraphRobustEnsemble, C) (RE.jl:265-283: energy(X0) summed left to right in i, then the slices in k order) and, with `cache`,
// the DeltaECache (DeltaE.jl:74-103: sites pushed in ABI order j = 1..N), one workgroup per replica.  The slice caches of GraphSKNormal are
// rebuilt as SK.jl:212-237 does (lfields = 2 lf, lfields_last = 0, move_last = none).
constexpr int kReInitThreads = 256;
template <int SLICE>
__global__ __launch_bounds__(kReInitThreads) void re_init_kernel(ReParams P, int cache)
{
    __shared__ int s_cnt[2 * (kReMmax / 2)][kReInitThreads];
    __shared__ int s_tot[2 * (kReMmax / 2)];
    __shared__ long long s_n[kReMmax];
    __shared__ double s_E[kReMmax];
    const int r = (int)blockIdx.x, tid = (int)threadIdx.x;
    const int N = P.N, Nk = P.Nk, M = P.M, L = P.L;
    uint32_t* sp = P.sp + (size_t)r * P.W;
    int8_t* mu = P.mu + (size_t)r * Nk;
    const RrrView v = re_view(P, sp, r);
    for (int k = tid; k < M; k += kReInitThreads) s_n[k] = 0;
    for (int i = tid; i < Nk; i += kReInitThreads) {
        int m = 0;
        for (int k = 0; k < M; ++k) m += 2 * sbit(sp, k * Nk + i) - 1;
        mu[i] = (int8_t)m;
    }
    __syncthreads();
    if constexpr (SLICE == RE_SK) {
        for (int x = tid; x < N; x += kReInitThreads)
            atomicAdd(reinterpret_cast<unsigned long long*>(&s_n[x / Nk]), (unsigned long long)(long long)(-(slice_delta(v, x) / 2)));
    } else if constexpr (SLICE == RE_SKN) {
        for (int x = tid; x < N; x += kReInitThreads) {
            const int k = x / Nk, i = x - k * Nk;
            const double* Ji = P.Jd + (size_t)i * Nk;
            const int si = sbit(sp, x);
            double lf = 0.0;
            for (int j = 0; j < Nk; ++j) lf += (double)(1 - 2 * (si ^ sbit(sp, k * Nk + j))) * Ji[j];
            v.slf[((size_t)0 * M + k) * Nk + i] = 2 * lf;
            v.slf[((size_t)1 * M + k) * Nk + i] = lf;
        }
        __syncthreads();
        for (int k = tid; k < M; k += kReInitThreads) {
            double n = 0.0;
            for (int i = 0; i < Nk; ++i) n -= v.slf[((size_t)1 * M + k) * Nk + i];
            n /= 2;
            s_E[k] = n;
            v.smv[k] = -1;
            v.scur[k] = 0;
        }
        __syncthreads();
        for (int x = tid; x < N; x += kReInitThreads) v.slf[(size_t)M * Nk + x] = 0.0;
    } else if constexpr (SLICE == RE_SPF) {
        spf_init_rows(P, v, sp, 0, M, s_E);
    } else if constexpr (kPercSlice<SLICE>) {
        perc_init_rows<SLICE == RE_PLIN>(P.pc, perc_view(P.pc, r), sp, Nk, N, s_n);
    } else if constexpr (kCommSlice<SLICE>) {
        comm_init_rows<comm_kind_of_slice(SLICE)>(P.cm, comm_view<comm_kind_of_slice(SLICE)>(P.cm, r), sp, Nk, N, s_n);
    } else if constexpr (SLICE == RE_SAT) {
        sat_init_rows(P.sat, sp, Nk, 0, M, s_n);
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
            const int i = j / M, k = j - i * M, s = sbit(sp, k * Nk + i);
            const int c = re_class(P.tab, M, L, mu[i] - (2 * s - 1), s);
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
        double E = 0.0;
        for (int i = 0; i < Nk; ++i) E -= P.etab[(mu[i] + M) >> 1];
        for (int k = 0; k < M; ++k) {
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
__host__ __device__ inline size_t re_rrr_lds_bytes(int64_t N, int64_t W, int64_t Nk)
{
    return (size_t)W * 4 + (((size_t)N * 2 + 3) & ~(size_t)3) + (((size_t)N + 3) & ~(size_t)3) + (((size_t)Nk + 3) & ~(size_t)3) +
           (size_t)kReMmax * 4 + (size_t)kRrrThreads * 8 * 4;
}

// rrrMC(X::DoubleGraph) (src/RRRMC.jl:221-290) on the Robust Ensemble.  LM >= L: the class weights T live in 2 LM registers (indexed only
// through unrolled selects: no scratch), classes L .. LM - 1 and L + L .. stay empty.
// LDS = false: one thread per replica, everything in HBM/L2.
// LDS = true:  one workgroup (one wavefront) per replica with the replica's spins, positions, classes, μ and set sizes staged in LDS; the
//   two Philox blocks of 64 iterations are computed by the whole wavefront, then lane 0 runs the chain (rrr_quant_kernel<true>'s pattern).
//   The member arrays (2 L N entries) stay in HBM/L2.  Same arithmetic, same order: the results are the thread build's.
//   Perceptron slices: the Stabilities of the M slices are staged in LDS too, and ALL 64 lanes run the chain with identical values, so
//   that the O(P) update_cache! of an accepted move is one pattern per lane (perc_update<.., true>); stores name one address wave-wide.
//   Committee machine slices (comm_kernels.hpp) the same way: their Δ1 / Δ2 and masks in LDS, comm_update<.., true>.
//   Sparse Float64 slices: lfields, the undo record and move_last of the M slices are staged in LDS when they fit (ReParams::spf_lds) and
//   written back at the end of the call; lane 0 runs update_cache! there (K + 1 LDS reads and writes instead of scattered HBM/L2 ones).
template <bool LDS, int LM, int SLICE>
__global__ __launch_bounds__(kRrrThreads) void re_rrr_kernel(ReParams P)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t re_lds[];
    int r;
    if constexpr (LDS) {
        r = (int)blockIdx.x;
    } else {
        r = blockIdx.x * blockDim.x + threadIdx.x;
        if (r >= P.R) return;
    }
    const int N = P.N, Nk = P.Nk, M = P.M, L = P.L, Mh = P.M >> 1;
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
        uint32_t* l_sp = re_lds;                                                   // [W]
        uint16_t* l_spos = reinterpret_cast<uint16_t*>(l_sp + P.W);                // [N]
        uint8_t* l_cls = reinterpret_cast<uint8_t*>(l_spos) + ((2 * N + 3) & ~3);  // [N]
        int8_t* l_mu = reinterpret_cast<int8_t*>(l_cls + ((N + 3) & ~3));          // [Nk]
        int32_t* l_t = reinterpret_cast<int32_t*>(l_mu + ((Nk + 3) & ~3));         // [kReMmax]
        l_rng = reinterpret_cast<uint32_t*>(l_t + kReMmax);                        // [64][8]
        for (int i = tid; i < P.W; i += nt) l_sp[i] = g_sp[i];
        for (int i = tid; i < N; i += nt) { l_spos[i] = g_spos[i]; l_cls[i] = g_cls[i]; }
        for (int i = tid; i < Nk; i += nt) l_mu[i] = g_mu[i];
        if (tid < 2 * L) l_t[tid] = g_t[tid];
        __syncthreads();
        sp = l_sp; spos = l_spos; cls = l_cls; mu = l_mu; t = l_t;
    }
    const RrrView g_v = re_view(P, sp, r);
    RrrView v = g_v;
    if constexpr (LDS && SLICE == RE_SPF) {                                        // the slices' LocalFields behind the chain's own arrays
        if (P.spf_lds) spf_ens_attach(v, reinterpret_cast<char*>(re_lds) + ((re_rrr_lds_bytes(N, P.W, Nk) + 7) & ~(size_t)7), M);
    }
    const auto g_pv = re_slice_view<SLICE>(P, r);                                  // PercView, or CommView for committee slices
    auto pv = g_pv;
    if constexpr (LDS && kPercSlice<SLICE>) {
        const int nw = M * P.pc.PW;                                                // mask words, then 64 stabilities per word
        pv.pm = reinterpret_cast<uint64_t*>(reinterpret_cast<char*>(re_lds) + ((re_rrr_lds_bytes(N, P.W, Nk) + 7) & ~(size_t)7));
        pv.mm = pv.pm + nw;
        pv.ds = reinterpret_cast<int16_t*>(pv.mm + nw);
        for (int i = (int)threadIdx.x; i < nw; i += (int)blockDim.x) { pv.pm[i] = g_pv.pm[i]; pv.mm[i] = g_pv.mm[i]; }
        for (int i = (int)threadIdx.x; i < 64 * nw; i += (int)blockDim.x) pv.ds[i] = g_pv.ds[i];
        __syncthreads();
    }
    if constexpr (LDS && kCommSlice<SLICE>) {
        const int nm = M * (int)comm_mk_row(P.cm.K2, P.cm.PW, comm_kind_of_slice(SLICE) == CK_QU), nd = M * (int)comm_ds_row(P.cm.K2, P.cm.PW, comm_kind_of_slice(SLICE) == CK_QU);     // mask words, stabilities
        pv.mk = reinterpret_cast<uint64_t*>(reinterpret_cast<char*>(re_lds) + ((re_rrr_lds_bytes(N, P.W, Nk) + 7) & ~(size_t)7));
        pv.ds = reinterpret_cast<int16_t*>(pv.mk + nm);
        for (int i = (int)threadIdx.x; i < nm; i += (int)blockDim.x) pv.mk[i] = g_pv.mk[i];
        for (int i = (int)threadIdx.x; i < nd; i += (int)blockDim.x) pv.ds[i] = g_pv.ds[i];
        __syncthreads();
    }
    const bool worker = !LDS || threadIdx.x == 0 || kWaveSlice<SLICE>;
    const uint32_t rep = P.replica0 + (uint32_t)r;
    const double* tab = P.tab;
    const double* ft = P.ft;
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
        const double dE0 = kc < L ? -tab[kc + Mh] : tab[kc - L + Mh];
        const uint64_t uu = ((uint64_t)o.w[2] << 32) | o.w[3];
        const int move = sv[(size_t)kc * N + (size_t)mulhi64(uu, (uint64_t)t[kc])];
        const int i = move / M, km = move - i * M, xm = km * Nk + i, jg = i * M;

        bool acc = false;
        if (acc_rate < P.staged_thr) {
            // staged branch: step_rrr (RRRMC.jl:131-138) = compute_staged! + compute_reverse_probabilities!, the list in order (the group
            // ascending without the move, then the move: CavityRange, RE.jl:175-206; DeltaE.jl:202-230); the second pass applies it
            staged_its += 1;
            const int s_old = sbit(sp, xm);
            const int munew = mu[i] + 2 * (1 - 2 * s_old);
            double Tp[2 * LM];
#pragma unroll
            for (int u = 0; u < 2 * LM; ++u) Tp[u] = T[u];
            double zp = z;
            for (int y = jg; y < jg + M; ++y) {
                if (y == move) continue;
                const int sy = sbit(sp, (y - jg) * Nk + i);
                const int k0 = cls[y], k1 = re_class(tab, M, L, munew - (2 * sy - 1), sy);
                if (k0 == k1) continue;
                const double f0 = re_class_f(ft, L, k0), f1 = re_class_f(ft, L, k1);
                t_sub(Tp, k0 < L ? k0 : k0 - L + LM, f0);
                t_add(Tp, k1 < L ? k1 : k1 - L + LM, f1);
                zp += f1 - f0;
            }
            {
                const int k0 = cls[move], k1 = k0 >= L ? k0 - L : k0 + L;
                const double f0 = re_class_f(ft, L, k0), f1 = re_class_f(ft, L, k1);
                t_sub(Tp, k0 < L ? k0 : k0 - L + LM, f0);
                t_add(Tp, k1 < L ? k1 : k1 - L + LM, f1);
                zp += f1 - f0;
            }
            const double c = z / zp;
            const double dE1 = re_residual<SLICE, LDS>(v, pv, xm, km, i);      // delta_energy_residual, RE.jl:303-310
            if (accept_c(c, -P.beta * dE1, q2, g)) {
                sflip(sp, xm);                                             // spinflip!(X, C, move)
                mu[i] = (int8_t)munew;
                re_slice_update<SLICE, LDS>(v, pv, xm, km, i);
                for (int y = jg; y < jg + M; ++y) {                        // apply_staged!
                    if (y == move) continue;
                    const int sy = sbit(sp, (y - jg) * Nk + i);
                    const int k0 = cls[y], k1 = re_class(tab, M, L, munew - (2 * sy - 1), sy);
                    if (k0 != k1) set_move(y, k0, k1);
                }
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
            const double dE1 = re_residual<SLICE, LDS>(v, pv, xm, km, i);
            for (int pass = 0; pass < 2; ++pass) {
                sflip(sp, xm);
                const int s_new = sbit(sp, xm);
                const int munew = mu[i] + 2 * (2 * s_new - 1);
                mu[i] = (int8_t)munew;
                // the undo pass takes the slice's swap path (move_last == move); a perceptron slice's Stabilities are a function of the
                // configuration, which a rejected move leaves as it was: they are updated once, below, for an accepted move
                if constexpr (!kWaveSlice<SLICE>) re_slice_update<SLICE>(v, xm);
                double zp = z;
                for (int y = jg; y < jg + M; ++y) {
                    if (y == move) continue;
                    const int sy = sbit(sp, (y - jg) * Nk + i);
                    const int k0 = cls[y], k1 = re_class(tab, M, L, munew - (2 * sy - 1), sy);
                    if (k0 == k1) continue;
                    const double f0 = re_class_f(ft, L, k0), f1 = re_class_f(ft, L, k1);
                    t_sub(T, k0 < L ? k0 : k0 - L + LM, f0);
                    t_add(T, k1 < L ? k1 : k1 - L + LM, f1);
                    zp += f1 - f0;
                    set_move(y, k0, k1);
                }
                {
                    const int k0 = cls[move], k1 = k0 >= L ? k0 - L : k0 + L;
                    const double f0 = re_class_f(ft, L, k0), f1 = re_class_f(ft, L, k1);
                    t_sub(T, k0 < L ? k0 : k0 - L + LM, f0);
                    t_add(T, k1 < L ? k1 : k1 - L + LM, f1);
                    zp += f1 - f0;
                    set_move(move, k0, k1);
                }
                const double cc = z / zp;
                z = zp;
                if (pass == 1) break;                                      // that was the undo
                if (accept_c(cc, -P.beta * dE1, q2, g)) { E += dE0 + dE1; accepted += 1; acc = true; break; }
            }
            if constexpr (kWaveSlice<SLICE>) { if (acc) re_slice_update<SLICE, LDS>(v, pv, xm, km, i); }
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
        const int nw = M * P.pc.PW;
        for (int i = (int)threadIdx.x; i < nw; i += (int)blockDim.x) { g_pv.pm[i] = pv.pm[i]; g_pv.mm[i] = pv.mm[i]; }
        for (int i = (int)threadIdx.x; i < 64 * nw; i += (int)blockDim.x) g_pv.ds[i] = pv.ds[i];
    }
    if constexpr (LDS && kCommSlice<SLICE>) {
        __syncthreads();
        const int nm = M * (int)comm_mk_row(P.cm.K2, P.cm.PW, comm_kind_of_slice(SLICE) == CK_QU), nd = M * (int)comm_ds_row(P.cm.K2, P.cm.PW, comm_kind_of_slice(SLICE) == CK_QU);
        for (int i = (int)threadIdx.x; i < nm; i += (int)blockDim.x) g_pv.mk[i] = pv.mk[i];
        for (int i = (int)threadIdx.x; i < nd; i += (int)blockDim.x) g_pv.ds[i] = pv.ds[i];
    }
    if constexpr (LDS && SLICE == RE_SPF) {
        if (P.spf_lds) spf_ens_detach(v, g_v, M);
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

// standardMC (src/RRRMC.jl:81-127): delta_energy = delta_energy(X0, C, j) + delta_energy_residual (RE.jl:312-315); the common SITE stream
// names ABI site j, rand() < exp(-β ΔE) on the ACCEPT_F64 stream.  E starts from E_cur (re_init_kernel, or the run a resumed call continues).
template <int SLICE>
__global__ __launch_bounds__(kRrrThreads) void re_standard_kernel(ReParams P)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= P.R) return;
    const int Nk = P.Nk, M = P.M;
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
        const int i = j / M, k = j - i * M, x = k * Nk + i;
        const int s = sbit(sp, x), sg = 2 * s - 1;
        const double dE = (double)sg * P.tab[(mu[i] - sg + M - 1) >> 1] + re_residual<SLICE>(v, pv, x, k, i);
        const double xx = -P.beta * dE;
        const bool acc = (xx >= 0.0) || (rand53(P.k0, P.k1, g, rep) < det_exp(xx));          // RRRMC.jl:39
        if (acc) {
            sflip(sp, x);
            mu[i] = (int8_t)(mu[i] - 2 * sg);
            re_slice_update<SLICE, false>(v, pv, x, k, i);
            E += dE;
            accepted += 1;
        }
    }
    P.E_cur[r] = E;
    P.stats[(size_t)r * 2] = accepted; P.stats[(size_t)r * 2 + 1] = 0;
}

// REenergies(X) (RE.jl:285-301): energy(X1[k], C1[k]) of every slice, one thread per (replica, slice).  Unlike the reference's (which calls
// energy and so resets the slice caches), this reads the configuration only: a hook that calls it does not change the run.
template <int SLICE>
__global__ __launch_bounds__(64) void re_energies_kernel(ReParams P)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= P.R * P.M) return;
    const int r = e / P.M, k = e - r * P.M;
    const RrrView v = re_view(P, P.sp + (size_t)r * P.W, r);
    P.Eslice[e] = re_slice_energy<SLICE>(P, v, k);
}

// debug mode (rrrmc_set_debug_checks): after a sampler call every replica's energy(X, C) is re-evaluated from its configuration and compared
// with the tracked E (|ΔE| <= 1e-10 max(1, |E|): the reference's check, RRRMC.jl:250, has an absolute 1e-10; relative once |E| > 1 is a deliberate departure — at N = 65 535 the
// energy reaches 10^4 and the rounding of a thousand E += ΔE alone can exceed an absolute 1e-10); μ, and after rrrMC every site's class and the set
// sizes, must equal what the configuration gives; GraphSKNormal slices: the cached fields within 1e-10 Nk of recomputed ones (sparse Float64
// slices: within 1e-10 K).
template <int SLICE>
__global__ __launch_bounds__(64) void re_check_kernel(ReParams P, int cache)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= P.R) return;
    const int Nk = P.Nk, M = P.M, L = P.L, N = P.N;
    const uint32_t* sp = P.sp + (size_t)r * P.W;
    const int8_t* mu = P.mu + (size_t)r * Nk;
    const RrrView v = re_view(P, P.sp + (size_t)r * P.W, r);
    bool bad = false;
    double E = 0.0;
    for (int i = 0; i < Nk; ++i) {
        int m = 0;
        for (int k = 0; k < M; ++k) m += 2 * sbit(sp, k * Nk + i) - 1;
        bad = bad || m != mu[i];
        E -= P.etab[(m + M) >> 1];
    }
    for (int k = 0; k < M; ++k) E += re_slice_energy<SLICE>(P, v, k);
    const double d = E - P.E_cur[r], tol = 1e-10 * (E < -1.0 ? -E : E > 1.0 ? E : 1.0);          // relative once |E| > 1, as le_check_kernel
    bad = bad || !(d <= tol && d >= -tol);
    if constexpr (SLICE == RE_SKN) {
        for (int k = 0; k < M; ++k)
            for (int i = 0; i < Nk; ++i) {
                const int si = sbit(sp, k * Nk + i);
                const double* Ji = P.Jd + (size_t)i * Nk;
                double lf = 0.0;
                for (int j = 0; j < Nk; ++j) lf += (double)(1 - 2 * (si ^ sbit(sp, k * Nk + j))) * Ji[j];
                const double dd = v.slf[((size_t)v.scur[k] * M + k) * Nk + i] - 2 * lf;
                bad = bad || !(dd <= 1e-10 * Nk && dd >= -1e-10 * Nk);
            }
    }
    if constexpr (SLICE == RE_SPF) bad = bad || spf_state_bad(P, v, sp, 0, M);
    if constexpr (kPercSlice<SLICE>) bad = bad || perc_state_bad<SLICE == RE_PLIN>(P.pc, perc_view(P.pc, r), sp, 0, Nk, N);
    if constexpr (kCommSlice<SLICE>) bad = bad || comm_state_bad<comm_kind_of_slice(SLICE)>(P.cm, comm_view<comm_kind_of_slice(SLICE)>(P.cm, r), sp, 0, Nk, N);
    if (cache) {
        int cnt[2 * (kReMmax / 2)];
        for (int k = 0; k < 2 * L; ++k) cnt[k] = 0;
        for (int j = 0; j < N; ++j) {
            const int i = j / M, k = j - i * M, s = sbit(sp, k * Nk + i);
            const int c = re_class(P.tab, M, L, mu[i] - (2 * s - 1), s);
            bad = bad || c != P.cls[(size_t)r * N + j] || P.sv[((size_t)r * 2 * L + c) * N + P.spos[(size_t)r * N + j]] != j;
            cnt[c] += 1;
        }
        for (int k = 0; k < 2 * L; ++k) bad = bad || cnt[k] != P.st[(size_t)r * 2 * L + k];
    }
    if (bad) { atomicAdd(&P.flag[0], 1); P.flag[1] = r; }
}

}  // namespace rrrmc
