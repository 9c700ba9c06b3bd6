// gfx950 kernels for GraphQuant over pattern-machine slices — GraphQPercStepT, GraphQPercLinearT, GraphQCommStepT, GraphQCommReLUT,
// GraphQCommQuT (src/QAliases.jl:85-181): M Suzuki-Trotter slices of one binary perceptron or committee machine, all on one pattern matrix, coupled along
// the Trotter axis by GraphQT{fourK} (src/graphs/QT.jl:42-122).
//
// Semantics (QT.jl).  Sites are GraphQuant's, x = k Nk + i (slice-major already: no working copy).  energy = energy(GraphQT) + Σ_k
// energy(X1[k], C1[k]) / M, added left to right, each slice divided by M (:185-199); delta_energy_residual = delta_energy(X1[k], C1[k], i) / M
// (:270-281) — for GraphPercLinear the slice's Float64 value 2n / √Nk is formed first and divided by M afterwards.  rrrMC(X::DoubleGraph)
// (src/RRRMC.jl:221-290) keeps its DeltaECache over GraphQT only (classes 0 / fourK, two neighbours): the kernels are rrr_kernels.hpp's
// rrr_quant_kernel / quant_standard_kernel with the slice policy below, so the Trotter part and the random streams are the other GraphQuants'.
//
// Slice state: per replica and slice the int16 stabilities and the P-bit membership masks of perc_kernels.hpp /
// comm_kernels.hpp, rows = M.  It is a pure function of the configuration: built by quant_pat_init_kernel (one workgroup per replica, masks by
// ballot), carried between resumed calls in device memory like the DeltaECache, and updated once per ACCEPTED move — the direct branch's
// flip-then-undo would restore it exactly (kOnAccept).  Builds: one thread per replica, or one wavefront per replica with or without the slice
// state staged in LDS (PatSlices below); integer arithmetic in the slice part, so all give the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#include "rrr_kernels.hpp"
#include "perc_kernels.hpp"
#include "comm_kernels.hpp"

namespace rrrmc {

enum QuantPat { QP_PSTEP = 3, QP_PLIN = 4, QP_CSTEP = 5, QP_CRELU = 6, QP_CQU = 9 };       // the slice kinds of the C ABI (RRRMC_RE_SLICE_*)
template <int KIND> constexpr bool qp_perc = KIND == QP_PSTEP || KIND == QP_PLIN;

struct QuantPatParams {
    PercParams pc;                                          // perceptron slices (rows = M), else unused
    CommParams cm;                                          // committee slices (rows = M), else unused
    int32_t* flag;                                          // debug mode: [2]
    double* Eslice;                                         // [R][M] quant_pat_energies_kernel
};

// The slice policy of rrr_quant_kernel / quant_standard_kernel for one replica.
//   WAVE = false: one thread per replica, the slice state in HBM/L2.
//   WAVE = true:  one wavefront per replica, all 64 lanes run the chain with identical values; the accepted-move update takes one pattern per
//     lane per 64-pattern word and rebuilds the mask words by ballot (perc_update / comm_update <.., true>).  STAGE = true keeps the
//     stabilities and masks of the replica's M slices in LDS behind the kernel's own arrays for the length of the call (attach / detach);
//     STAGE = false leaves them in HBM/L2 (a workgroup-scope barrier orders lane 0's mask stores before the other lanes' reads).
//   Integer arithmetic in the slice part: every build gives the same bits.
template <int KIND, bool WAVE = false, bool STAGE = false>
struct PatSlices {
    using Params = QuantPatParams;
    using View = std::conditional_t<qp_perc<KIND>, PercView, CommView>;
    static constexpr bool kOnAccept = true;
    static constexpr bool kWave = WAVE;
    View w, g;                                              // the state the chain works on, and its home in device memory
    int rows;
    __device__ __forceinline__ PatSlices(const Params& Q, int r)
    {
        if constexpr (qp_perc<KIND>) { w = perc_view(Q.pc, r); rows = Q.pc.rows; }
        else { w = comm_view<comm_kind_of_slice(KIND)>(Q.cm, r); rows = Q.cm.rows; }
        g = w;
    }
    // 64-bit words of masks and 16-bit stabilities of the replica's `rows` slices
    __device__ __forceinline__ int n_mask() const
    {
        if constexpr (qp_perc<KIND>) return 2 * rows * w.PW;
        else return rows * (int)comm_mk_row(w.K2, w.PW, KIND == QP_CQU);
    }
    __device__ __forceinline__ int n_ds() const
    {
        if constexpr (qp_perc<KIND>) return rows * 64 * w.PW;
        else return rows * (int)comm_ds_row(w.K2, w.PW, KIND == QP_CQU);
    }
    __device__ __forceinline__ void attach(uint32_t* lds)
    {
        if constexpr (WAVE && STAGE) {
            uint64_t* lm = reinterpret_cast<uint64_t*>((reinterpret_cast<uintptr_t>(lds) + 7) & ~(uintptr_t)7);
            int16_t* ld = reinterpret_cast<int16_t*>(lm + n_mask());
            const int tid = (int)threadIdx.x, nt = (int)blockDim.x, nm = n_mask(), nd = n_ds();
            if constexpr (qp_perc<KIND>) {
                for (int i = tid; i < nm / 2; i += nt) { lm[i] = g.pm[i]; lm[nm / 2 + i] = g.mm[i]; }
                w.pm = lm; w.mm = lm + nm / 2;
            } else {
                for (int i = tid; i < nm; i += nt) lm[i] = g.mk[i];
                w.mk = lm;
            }
            for (int i = tid; i < nd; i += nt) ld[i] = g.ds[i];
            w.ds = ld;
            __syncthreads();
        } else {
            (void)lds;
        }
    }
    __device__ __forceinline__ void detach()                // (after a barrier: the chain has finished)
    {
        if constexpr (WAVE && STAGE) {
            const int tid = (int)threadIdx.x, nt = (int)blockDim.x, nm = n_mask(), nd = n_ds();
            if constexpr (qp_perc<KIND>) {
                for (int i = tid; i < nm / 2; i += nt) { g.pm[i] = w.pm[i]; g.mm[i] = w.mm[i]; }
            } else {
                for (int i = tid; i < nm; i += nt) g.mk[i] = w.mk[i];
            }
            for (int i = tid; i < nd; i += nt) g.ds[i] = w.ds[i];
        }
    }
    __device__ __forceinline__ double residual(const RrrView& v, int move) const
    {
        const int k = slice_of(move, v.Nk, v.nk_magic, v.wide), i = move - k * v.Nk, s = sbit(v.sp, move);
        if constexpr (KIND == QP_PSTEP) return perc_residual<false>(w, k, i, s) / (double)v.M;
        else if constexpr (KIND == QP_PLIN) return perc_residual<true>(w, k, i, s) / (double)v.M;
        else return comm_residual<comm_kind_of_slice(KIND), WAVE>(w, k, i, s) / (double)v.M;
    }
    __device__ __forceinline__ void update(const RrrView& v, int move) const          // after the bit flip
    {
        const int k = slice_of(move, v.Nk, v.nk_magic, v.wide), i = move - k * v.Nk, s = sbit(v.sp, move);
        if constexpr (qp_perc<KIND>) perc_update<KIND == QP_PLIN, WAVE>(w, k, i, s);
        else comm_update<comm_kind_of_slice(KIND), WAVE>(w, k, i, s);
    }
};
// bytes of LDS attach() uses with STAGE (8 for the alignment of the mask words)
inline size_t quant_pat_stage_bytes(bool perc, int64_t M, int64_t K2, int64_t PW, bool qu) { return 8 + (perc ? perc_lds_bytes(M, PW) : comm_lds_bytes(M, K2, PW, qu)); }
// energy(X1[k], C1[k]) of the slice that starts at bit `off`, recomputed from the configuration
template <int KIND>
__device__ __forceinline__ double pat_row_energy(const QuantPatParams& Q, const uint32_t* sp, int off, int Nk, int Nbits)
{
    if constexpr (qp_perc<KIND>) return perc_row_energy<KIND == QP_PLIN>(Q.pc, sp, off, Nk, Nbits);
    else return comm_row_energy<comm_kind_of_slice(KIND)>(Q.cm, sp, off, Nbits);
}

// the two samplers over these slices, one thread per replica ...
template <int KIND> constexpr void (*rrr_quant_pat_kernel)(RrrParams, QuantPatParams) = rrr_quant_kernel<false, PatSlices<KIND>>;
template <int KIND> constexpr void (*quant_standard_pat_kernel)(RrrParams, QuantPatParams) = quant_standard_kernel<PatSlices<KIND>>;
// ... and one wavefront per replica: rrrMC is the LDS build of rrr_quant_kernel (spins, classes, positions, set sizes and the RRR draws of 64
// iterations in LDS) run wave-uniformly, with (STAGE) or without the slice state in LDS behind them
template <int KIND, bool STAGE> constexpr void (*rrr_quant_pat_wave_kernel)(RrrParams, QuantPatParams) = rrr_quant_kernel<true, PatSlices<KIND, true, STAGE>>;

// standardMC with one wavefront per replica: quant_standard_kernel's loop run wave-uniformly (every lane computes the same site, ΔE and
// acceptance), the replica's spins in LDS, the accepted-move update lane-parallel.  grid R, block 64, dynamic LDS = the spins (8-byte
// multiple) + quant_pat_stage_bytes with STAGE.
template <int KIND, bool STAGE>
__global__ __launch_bounds__(kRrrThreads) void quant_standard_pat_wave_kernel(RrrParams P, QuantPatParams Q)
{
    extern __shared__ uint32_t qsw_lds[];
    const int r = (int)blockIdx.x, tid = (int)threadIdx.x, nt = (int)blockDim.x;
    RrrView v = rrr_view(P, r);
    uint32_t* g_sp = v.sp;
    for (int i = tid; i < P.W; i += nt) qsw_lds[i] = g_sp[i];
    v.sp = qsw_lds;
    PatSlices<KIND, true, STAGE> sl(Q, r);
    sl.attach(qsw_lds + P.W);
    __syncthreads();
    const uint32_t rep = P.replica0 + (uint32_t)r;
    double E = P.E_cur[r];
    int64_t accepted = 0, ns = 0;
    long long next_sample = P.step;
    for (int64_t it = 1; it <= P.iters; ++it) {
        if (it == next_sample) { next_sample += P.step; P.Es[ns * P.R + r] = E; ns += 1; }
        const uint64_t g = P.g0 + (uint64_t)it;
        const int move = (int)site_of(P.k0, P.k1, g, (uint32_t)P.N);
        const double dE = (double)qt_delta(v, move) * P.fourK + sl.residual(v, move);
        const double x = -P.beta * dE;
        const bool acc = (x >= 0.0) || (rand53(P.k0, P.k1, g, rep) < det_exp(x));        // RRRMC.jl:39
        if (acc) { sflip(v.sp, move); sl.update(v, move); E += dE; accepted += 1; }
    }
    P.E_cur[r] = E;
    P.stats[(size_t)r * 2] = accepted; P.stats[(size_t)r * 2 + 1] = 0;
    __syncthreads();
    for (int i = tid; i < P.W; i += nt) g_sp[i] = qsw_lds[i];
    sl.detach();
}

// energy(X::GraphQuant, C) (QT.jl:185-199), the slices' Stabilities and the DeltaECache in site order (DeltaE.jl:74-103), one workgroup per
// replica: the Trotter sum and the classes as rrr_init_coop_kernel builds them, the slice rows by perc_init_rows / comm_init_rows.
template <int KIND>
__global__ __launch_bounds__(kInitThreads) void quant_pat_init_kernel(RrrParams P, QuantPatParams Q)
{
    __shared__ int s_cnt[4][kInitThreads];
    __shared__ int s_tot[4];
    __shared__ long long s_n0;
    extern __shared__ long long s_slice[];             // [M] integer slice energies
    const int r = (int)blockIdx.x, tid = (int)threadIdx.x;
    const RrrView v = rrr_view(P, r);
    const int N = P.N, Nk = P.Nk, M = P.M;
    if (tid == 0) s_n0 = 0;
    for (int k = tid; k < M; k += kInitThreads) s_slice[k] = 0;
    __syncthreads();
    {
        long long n0 = 0;
        for (int x = tid; x < N; x += kInitThreads) {
            const int i = x % Nk, k = x / Nk;
            const int prev = i + (k == 0 ? M - 1 : k - 1) * Nk;
            n0 -= 1 - 2 * (sbit(v.sp, x) ^ sbit(v.sp, prev));
        }
        atomicAdd(reinterpret_cast<unsigned long long*>(&s_n0), (unsigned long long)n0);
    }
    if constexpr (qp_perc<KIND>) perc_init_rows<KIND == QP_PLIN>(Q.pc, perc_view(Q.pc, r), v.sp, Nk, 32 * P.W, s_slice);
    else comm_init_rows<comm_kind_of_slice(KIND)>(Q.cm, comm_view<comm_kind_of_slice(KIND)>(Q.cm, r), v.sp, Nk, 32 * P.W, s_slice);
    // classes of this thread's block of spins, then the exclusive scan and the fills (as rrr_init_coop_kernel)
    const int per = (N + kInitThreads - 1) / kInitThreads, x0 = tid * per, x1 = x0 + per < N ? x0 + per : N;
    int cnt[4] = {0, 0, 0, 0};
    for (int x = x0; x < x1; ++x) {
        const int k = qt_class(v, x);
        v.cls[x] = (uint8_t)k;
        cnt[k] += 1;
    }
    for (int k = 0; k < 4; ++k) s_cnt[k][tid] = cnt[k];
    __syncthreads();
    if (tid < 4) {
        int run = 0;
        for (int t = 0; t < kInitThreads; ++t) { const int c = s_cnt[tid][t]; s_cnt[tid][t] = run; run += c; }
        s_tot[tid] = run;
    }
    __syncthreads();
    int off[4];
    for (int k = 0; k < 4; ++k) off[k] = s_cnt[k][tid];
    for (int x = x0; x < x1; ++x) {
        const int k = v.cls[x];
        idx_set(v.sv, (size_t)k * N + off[k], x, v.wide);
        idx_set(v.spos, x, off[k], v.wide);
        off[k] += 1;
    }
    if (tid == 0) {
        double E = (double)s_n0 * P.fourK / 4;
        for (int k = 0; k < M; ++k) {
            const double Ek = qp_perc<KIND> ? perc_energy_of<KIND == QP_PLIN>(s_slice[k], Q.pc.sN) : (double)s_slice[k];
            E += Ek / (double)M;
        }
        P.E_cur[r] = E;
        double z = 0.0;
        for (int k = 0; k < 4; ++k) {
            v.t[k] = s_tot[k];
            const double x = (double)s_tot[k] * class_f(k, P.ft1);
            z += x;
            P.T[(size_t)r * 4 + k] = x;
        }
        P.zz[r] = z;
        P.acc_rate[r] = 0.5;
        P.stats[(size_t)r * 2] = 0;
        P.stats[(size_t)r * 2 + 1] = 0;
    }
}

// debug mode (rrrmc_set_debug_checks): after a call, the Stabilities and masks of every slice and the tracked energy against what the
// configuration gives; one thread per replica.  The energy bound is relative: E carries one rounding per accepted move.
template <int KIND>
__global__ __launch_bounds__(64) void quant_pat_check_kernel(RrrParams P, QuantPatParams Q)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= P.R) return;
    const uint32_t* sp = P.spins + (size_t)r * P.W;
    const int Nk = P.Nk, M = P.M, Nbits = 32 * P.W;
    bool bad;
    if constexpr (qp_perc<KIND>) bad = perc_state_bad<KIND == QP_PLIN>(Q.pc, perc_view(Q.pc, r), sp, 0, Nk, Nbits);
    else bad = comm_state_bad<comm_kind_of_slice(KIND)>(Q.cm, comm_view<comm_kind_of_slice(KIND)>(Q.cm, r), sp, 0, Nk, Nbits);
    long long n0 = 0;
    for (int i = 0; i < Nk; ++i) {
        int sj = sbit(sp, i + (M - 1) * Nk);
        for (int k = 0; k < M; ++k) {
            const int sk = sbit(sp, i + k * Nk);
            n0 -= 1 - 2 * (sk ^ sj);
            sj = sk;
        }
    }
    double E = (double)n0 * P.fourK / 4;
    for (int k = 0; k < M; ++k) E += pat_row_energy<KIND>(Q, sp, k * Nk, Nk, Nbits) / (double)M;
    const double d = E - P.E_cur[r], tol = 1e-10 * (fabs(E) > 1.0 ? fabs(E) : 1.0);
    bad = bad || !(d <= tol && d >= -tol);
    if (bad) { atomicAdd(&Q.flag[0], 1); Q.flag[1] = r; }
}

// Renergies (QT.jl:201-211): energy(X1[k], C1[k]) of every slice — the training errors — recomputed from the configuration; one thread per
// (replica, slice).  Read-only: a run the context continues is not disturbed.
template <int KIND>
__global__ __launch_bounds__(64) void quant_pat_energies_kernel(QuantPatParams Q, const uint32_t* __restrict__ spins, int Nk, int M, int W, int R)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= R * M) return;
    const int r = t / M, k = t - r * M;
    Q.Eslice[t] = pat_row_energy<KIND>(Q, spins + (size_t)r * W, k * Nk, Nk, 32 * W);
}

}  // namespace rrrmc
