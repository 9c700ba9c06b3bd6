// gfx950 kernels for the two-layer binary committee machines (src/graphs/CommStep.jl, CommReLU.jl): N = K1 K2 binary synapses in K2
// hidden units of K1 synapses (unit u owns synapses u K1 .. (u + 1) K1 − 1), trained on P random patterns ξ.  Per pattern a, the unit
// stabilities Δ1[u][a] = K1 − 2 Σ_(i in u) (s_i ⊻ ξ[a,i]).
// GraphCommStep{Int} (K1, K2 odd): Δ2[a] = Σ_u sign(Δ1[u][a]), energy = #{Δ2 < 0} (CommStep.jl:107-141).
// GraphCommReLU{Int} (K1, K2 even): Δ2[a] = o_a Σ_u c_u max(Δ1[u][a], 0) with o_a = 2 y_a − 1 and c_u = +1 for 2 (u + 1) <= K2, −1 beyond;
// energy = #{Δ2 <= 0} (CommReLU.jl:111-147).
// GraphCommQu{Int} (K1, K2 even): the same with the unit term c_u Δ1[u][a]², Δ2[a] = o_a Σ_u c_u Δ1[u][a]² (CommQu.jl:115-152); its state
// and ΔE are described further down.
// All three are used as the slice graph of the Robust Ensemble and the Local Entropy ensemble (re_kernels.hpp, le_kernels.hpp:
// GraphComm{Step,ReLU,Qu}RE / GraphComm{Step,ReLU,Qu}LE), of GraphQuant (quant_pat_kernels.hpp) and, stand-alone, under standardMC.
//
// State.  Per chain (and per slice of an ensemble): Δ1 [K2][64 PW] and Δ2 [64 PW] as int16 (|Δ1| <= K1, |Δ2| <= N <= 32 767),
// and the reference's ArraySets p1[u], m1[u], p2, m2 as P-bit masks.  As for the perceptron (perc_kernels.hpp) member ORDER never reaches a
// result (delta_energy sums integers over members, CommStep.jl:212-242, CommReLU.jl:229-266) and membership is a function of the
// stabilities alone, which every branch of update_cache! keeps (CommStep.jl:143-197, CommReLU.jl:149-214):
//   step: p1[u] = {Δ1 = 1}, m1[u] = {Δ1 = −1}, p2 = {Δ2 = 1}, m2 = {Δ2 = −1};
//   ReLU: p1[u] = {Δ1 > 0}, m1[u] = {Δ1 = 0}, p2 = {Δ2 = 2}, m2 = {Δ2 = 0}.
// tests/test_comm_cpu.py checks the masks against literal ArraySets over a random walk.  The state is a pure function of the configuration,
// so the direct branch of rrrMC updates a slice only for an accepted move, as for perceptron slices.
//
// delta_energy of synapse i (unit u = i / K1, col = the pattern column of i ⊻ its spin bit):
//   step: popc(p2 & p1[u] & ~col) − popc(m2 & m1[u] & col);
//   ReLU: eq = the patterns with c_u = o_a (y for c_u = +1, ~y otherwise), A = p1[u], Z = m1[u]:
//         popc(p2 & eq & A & ~col) + popc(p2 & ~eq & (A|Z) & col) − popc(m2 & eq & (A|Z) & col) − popc(m2 & ~eq & A & ~col).
// update_cache! after the flip (new spin bit s): Δ1[u][a] += 2 − 4 col_a, Δ2 moves by the change of unit u's term, the masks of unit u and
// p2 / m2 are rebuilt from the new values; no other unit's row is touched.  WAVE = false: a loop of one thread; WAVE = true: the 64 lanes
// of a one-wavefront workgroup run the chain with identical values, lane l owns pattern 64 w + l, the mask words are ballots.  Integer
// arithmetic only: both builds give the same bits.
//
// GraphCommQu (CK_QU).  |Δ2| <= K2 K1² = N K1 passes int16, so its Δ2 row is int32: a chain's row is Δ1 [K2][64 PW] int16, then Δ2 [64 PW]
// int32 (comm_ds_row counts it as two int16 rows; 64 consecutive patterns are 128 resp. 256 contiguous bytes: no LDS bank conflict).  The
// reference's two heaps per pattern and its sets p2 / m2 (CommQu.jl:30-50, :221-255) only bound which patterns can change sign under one
// flip; the engine keeps two P-bit masks that are functions of Δ2 alone instead, wrong = {Δ2 <= 0} and near = {|Δ2| <= 4 (1 + K1)}:
//   flipping synapse i of unit u (x = ξ[a,i] ⊻ s_i before the flip) moves Δ1[u][a] by 4x − 2 and Δ2[a] by t_a = o_a c_u 4 (1 − (1 − 2x) Δ1[u][a])
//   (= o_a c_u (newΔ1² − oldΔ1²), CommQu.jl:174-176, :240, :246); |t_a| <= 4 (1 + K1), so a pattern outside `near` keeps its sign and
//   delta_energy = #{a in near : Δ2[a] + t_a <= 0} − popc(wrong & near).
// tests/test_comm_qu_cpu.py holds this formula to the literal reference (heaps, p2 / m2) over random walks.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rrr_kernels.hpp"    // sbit / sflip, kRrrThreads, site_of, rand53, det_exp
#include "perc_kernels.hpp"   // perc_row_word (a row's bits from any offset)

namespace rrrmc {

constexpr int kCommNmax = 32767;                            // synapses K1 K2 (int16 stabilities)
constexpr int kCommPmax = 4096;                             // patterns (64 mask words)
enum CommKind { CK_STEP = 0, CK_RELU = 1, CK_QU = 2 };      // GraphCommStep, GraphCommReLU, GraphCommQu
// the committee kind of a slice kind of the C ABI (RRRMC_RE_SLICE_COMM_STEP = 5, _COMM_RELU = 6, _COMM_QU = 9)
constexpr int comm_kind_of_slice(int slice) { return slice == 6 ? CK_RELU : slice == 9 ? CK_QU : CK_STEP; }

struct CommParams {
    const uint64_t* col;                                    // [Nk][PW]  one pattern column per synapse
    const uint32_t* row;                                    // [P][RW]   RW = 2 ceil(Nk / 64); bits beyond Nk are 0
    const uint64_t* lab;                                    // [2][PW]   ReLU, Qu: y, then ~y (bits beyond P are 0 in both); step: unused
    int16_t* ds;                                            // [R][rows][K2 + 1][64 PW]   Δ1 of the units, then Δ2 (entries a >= P stay 0)
                                                            //   Qu: [R][rows] { int16 [K2][64 PW], int32 [64 PW] }
    uint64_t* mk;                                           // [R][rows][2 K2 + 2][PW]    p1[K2], m1[K2], p2, m2;  Qu: [R][rows][2][PW] wrong, near
    int P, PW, RW, rows, K1, K2;
};

struct CommView {                                           // one chain's state (HBM/L2, or LDS in the WAVE build)
    const uint64_t* col; const uint64_t* lab;
    int16_t* ds; uint64_t* mk;
    int P, PW, K1, K2;
};

// one row's stabilities in int16 units and its 64-bit mask words
__host__ __device__ inline size_t comm_ds_row(int K2, int PW, bool qu) { return (size_t)(K2 + (qu ? 2 : 1)) * 64 * PW; }
__host__ __device__ inline size_t comm_mk_row(int K2, int PW, bool qu) { return qu ? (size_t)2 * PW : (size_t)(2 * K2 + 2) * PW; }
inline size_t comm_lds_bytes(int64_t rows, int64_t K2, int64_t PW, bool qu)
{
    return (size_t)rows * (comm_mk_row((int)K2, (int)PW, qu) * 8 + comm_ds_row((int)K2, (int)PW, qu) * 2);
}

template <int KIND>
__device__ __forceinline__ CommView comm_view(const CommParams& Q, int r)
{
    CommView v{};
    v.col = Q.col; v.lab = Q.lab; v.P = Q.P; v.PW = Q.PW; v.K1 = Q.K1; v.K2 = Q.K2;
    if (Q.ds) {
        v.ds = Q.ds + (size_t)r * Q.rows * comm_ds_row(Q.K2, Q.PW, KIND == CK_QU);
        v.mk = Q.mk + (size_t)r * Q.rows * comm_mk_row(Q.K2, Q.PW, KIND == CK_QU);
    }
    return v;
}

__device__ __forceinline__ int comm_c(int u, int K2) { return 2 * (u + 1) <= K2 ? 1 : -1; }          // CommReLU.jl:124
__device__ __forceinline__ int comm_sign(int d) { return (d > 0) - (d < 0); }
__device__ __forceinline__ int comm_label(const uint64_t* lab, int a) { return (int)((lab[a >> 6] >> (a & 63)) & 1ull); }
// unit u's term of Δ2 (before the label o_a)
template <int KIND> __device__ __forceinline__ int comm_term(int d1, int u, int K2)
{
    return KIND == CK_QU ? comm_c(u, K2) * d1 * d1 : KIND == CK_RELU ? comm_c(u, K2) * (d1 > 0 ? d1 : 0) : comm_sign(d1);
}
template <int KIND> constexpr bool kCommLabelled = KIND != CK_STEP;                                  // Δ2 carries the label o_a
template <int KIND> __device__ __forceinline__ bool comm_in_p1(int d) { return KIND == CK_RELU ? d > 0 : d == 1; }
template <int KIND> __device__ __forceinline__ bool comm_in_m1(int d) { return KIND == CK_RELU ? d == 0 : d == -1; }
template <int KIND> __device__ __forceinline__ bool comm_in_p2(int d) { return KIND == CK_RELU ? d == 2 : d == 1; }
template <int KIND> __device__ __forceinline__ bool comm_in_m2(int d) { return KIND == CK_RELU ? d == 0 : d == -1; }
template <int KIND> __device__ __forceinline__ bool comm_wrong(int d) { return KIND == CK_STEP ? d < 0 : d <= 0; }
// Qu: the patterns whose Δ2 one flip can carry across zero
__device__ __forceinline__ bool comm_qu_near(int d2, int K1) { return (d2 < 0 ? -d2 : d2) <= 4 * (1 + K1); }
// Qu: the Δ2 row of the row of stabilities that starts at ds
__device__ __forceinline__ int32_t* comm_qu_d2(int16_t* ds, int K2, int PW) { return reinterpret_cast<int32_t*>(ds + (size_t)K2 * 64 * PW); }
__device__ __forceinline__ const int32_t* comm_qu_d2(const int16_t* ds, int K2, int PW) { return reinterpret_cast<const int32_t*>(ds + (size_t)K2 * 64 * PW); }

// Δ1 of unit u of the configuration in the row that starts at bit `off` (CommStep.jl:120-122)
__device__ __forceinline__ int comm_unit_stability(const CommParams& Q, const uint32_t* sp, int off, int Nbits, int u, int a)
{
    const uint32_t* xa = Q.row + (size_t)a * Q.RW;
    const int K1 = Q.K1;
    int cnt = 0;
    for (int w = 0; 32 * w < K1; ++w)
        cnt += __popc(perc_row_word(sp, off + u * K1, w, K1, Nbits) ^ perc_row_word(xa, u * K1, w, K1, 32 * Q.RW));
    return K1 - 2 * cnt;
}
// Δ2 of pattern a (label included)
template <int KIND>
__device__ __forceinline__ int comm_output(const CommParams& Q, const uint32_t* sp, int off, int Nbits, int a)
{
    int t = 0;
    for (int u = 0; u < Q.K2; ++u) t += comm_term<KIND>(comm_unit_stability(Q, sp, off, Nbits, u, a), u, Q.K2);
    if constexpr (kCommLabelled<KIND>) t *= 2 * comm_label(Q.lab, a) - 1;
    return t;
}

// energy(X, C) of one row, sequential, from the configuration only
template <int KIND>
__device__ inline double comm_row_energy(const CommParams& Q, const uint32_t* sp, int off, int Nbits)
{
    long long n = 0;
    for (int a = 0; a < Q.P; ++a) n += comm_wrong<KIND>(comm_output<KIND>(Q, sp, off, Nbits, a)) ? 1 : 0;
    return (double)n;
}

// energy (CommStep.jl:107-141, CommReLU.jl:111-147) of every row of one chain by a whole workgroup (blockDim a multiple of 64): Δ1, Δ2 and
// the masks are written, the number of misclassified patterns of row k is added to s_n[k] (zeroed by the caller, who synchronises after)
template <int KIND>
__device__ inline void comm_init_rows(const CommParams& Q, const CommView& cv, const uint32_t* sp, int Nk, int Nbits, long long* s_n)
{
    const int Pp = 64 * Q.PW, tot = Q.rows * Pp, lane = (int)threadIdx.x & 63, K2 = Q.K2, PW = Q.PW;
    for (int idx = (int)threadIdx.x; idx < tot; idx += (int)blockDim.x) {          // a wavefront covers one mask word: uniform trip counts
        const int k = idx / Pp, a = idx - k * Pp;
        const bool in = a < Q.P;
        int16_t* ds = cv.ds + (size_t)k * comm_ds_row(K2, PW, KIND == CK_QU);
        uint64_t* mk = cv.mk + (size_t)k * comm_mk_row(K2, PW, KIND == CK_QU);
        int t = 0;
        for (int u = 0; u < K2; ++u) {
            const int d1 = in ? comm_unit_stability(Q, sp, k * Nk, Nbits, u, a) : 0;
            ds[(size_t)u * Pp + a] = (int16_t)d1;
            t += comm_term<KIND>(d1, u, K2);
            if constexpr (KIND != CK_QU) {
                const uint64_t p = __ballot(in && comm_in_p1<KIND>(d1)), m = __ballot(in && comm_in_m1<KIND>(d1));
                if (lane == 0) { mk[(size_t)u * PW + (a >> 6)] = p; mk[(size_t)(K2 + u) * PW + (a >> 6)] = m; }
            }
        }
        if constexpr (kCommLabelled<KIND>) t = in ? t * (2 * comm_label(Q.lab, a) - 1) : 0;
        if constexpr (KIND == CK_QU) {
            comm_qu_d2(ds, K2, PW)[a] = t;
            const uint64_t wr = __ballot(in && comm_wrong<KIND>(t)), nr = __ballot(in && comm_qu_near(t, Q.K1));
            if (lane == 0) { mk[a >> 6] = wr; mk[(size_t)PW + (a >> 6)] = nr; }
        } else {
            ds[(size_t)K2 * Pp + a] = (int16_t)t;
            const uint64_t p = __ballot(in && comm_in_p2<KIND>(t)), m = __ballot(in && comm_in_m2<KIND>(t));
            if (lane == 0) { mk[(size_t)2 * K2 * PW + (a >> 6)] = p; mk[(size_t)(2 * K2 + 1) * PW + (a >> 6)] = m; }
        }
        if (in && comm_wrong<KIND>(t)) atomicAdd(reinterpret_cast<unsigned long long*>(&s_n[k]), 1ull);
    }
}

// Qu: delta_energy (CommQu.jl:221-255, over every pattern that can change sign) of flipping synapse i of row k, whose spin bit is s.
// WAVE: called by all 64 lanes of a one-wavefront workgroup with identical arguments, lane l takes pattern 64 w + l of every word that
// has a near pattern; every lane returns the same count.
template <bool WAVE>
__device__ __forceinline__ int comm_qu_delta(const CommView& cv, int k, int i, int s)
{
    const int PW = cv.PW, K2 = cv.K2, u = i / cv.K1, Pp = 64 * PW;
    const int cu4 = 4 * comm_c(u, K2);
    const uint64_t* c = cv.col + (size_t)i * PW;
    const int16_t* ds = cv.ds + (size_t)k * comm_ds_row(K2, PW, true);
    const int16_t* d1 = ds + (size_t)u * Pp;
    const int32_t* d2 = comm_qu_d2(ds, K2, PW);
    const uint64_t* wrong = cv.mk + (size_t)k * comm_mk_row(K2, PW, true);
    const uint64_t* near = wrong + PW;
    const uint64_t sx = s ? ~0ull : 0ull;
    int d = 0;
    for (int w = 0; w < PW; ++w) {
        const uint64_t nr = near[w];
        if (!nr) continue;
        const uint64_t cw = c[w] ^ sx, yw = cv.lab[w];
        // Δ2 + o_a c_u 4 (1 − (1 − 2x) Δ1) <= 0 for the pattern at bit b of the word
        auto wrong_after = [&](int b) {
            const int a = 64 * w + b, x = (int)((cw >> b) & 1ull), o = 2 * (int)((yw >> b) & 1ull) - 1;
            return d2[a] + o * cu4 * (1 - (1 - 2 * x) * (int)d1[a]) <= 0;
        };
        int nw = 0;
        if constexpr (WAVE) {
            const int lane = (int)threadIdx.x;
            nw = __popcll(__ballot(((nr >> lane) & 1ull) && wrong_after(lane)));
        } else {
            for (uint64_t m = nr; m; m &= m - 1) nw += wrong_after(__ffsll((unsigned long long)m) - 1) ? 1 : 0;
        }
        d += nw - __popcll(wrong[w] & nr);
    }
    return d;
}

// delta_energy (CommStep.jl:212-242, CommReLU.jl:229-266, CommQu.jl:221-255) of flipping synapse i of row k, whose spin bit is s
// (WAVE matters to Qu only: the popcounts of the other two are the same in every lane)
template <int KIND, bool WAVE = false>
__device__ __forceinline__ double comm_residual(const CommView& cv, int k, int i, int s)
{
    if constexpr (KIND == CK_QU) return (double)comm_qu_delta<WAVE>(cv, k, i, s);
    constexpr bool RELU = KIND == CK_RELU;
    const int PW = cv.PW, K2 = cv.K2, u = i / cv.K1;
    const uint64_t* c = cv.col + (size_t)i * PW;
    const uint64_t* mk = cv.mk + (size_t)k * comm_mk_row(K2, PW, false);
    const uint64_t* p1 = mk + (size_t)u * PW;
    const uint64_t* m1 = mk + (size_t)(K2 + u) * PW;
    const uint64_t* p2 = mk + (size_t)2 * K2 * PW;
    const uint64_t* m2 = p2 + PW;
    const uint64_t sx = s ? ~0ull : 0ull;
    int d = 0;
    if constexpr (RELU) {
        const bool pos = comm_c(u, K2) > 0;
        const uint64_t* eq = cv.lab + (pos ? 0 : PW);
        const uint64_t* ne = cv.lab + (pos ? PW : 0);
        for (int w = 0; w < PW; ++w) {
            const uint64_t cw = c[w] ^ sx, A = p1[w], AZ = A | m1[w], P2 = p2[w], M2 = m2[w], E = eq[w], NE = ne[w];
            d += __popcll(P2 & E & A & ~cw) + __popcll(P2 & NE & AZ & cw) - __popcll(M2 & E & AZ & cw) - __popcll(M2 & NE & A & ~cw);
        }
    } else {
        for (int w = 0; w < PW; ++w) {
            const uint64_t cw = c[w] ^ sx;
            d += __popcll(p2[w] & p1[w] & ~cw) - __popcll(m2[w] & m1[w] & cw);
        }
    }
    return (double)d;
}

// Qu: update_cache! (CommQu.jl:154-219) of row k after synapse i was flipped to the spin bit s: Δ1[u], Δ2 and the two masks
template <bool WAVE>
__device__ __forceinline__ void comm_qu_update(const CommView& cv, int k, int i, int s)
{
    const int PW = cv.PW, K2 = cv.K2, K1 = cv.K1, u = i / K1, Pp = 64 * PW;
    const int cu = comm_c(u, K2);
    const uint64_t* c = cv.col + (size_t)i * PW;
    int16_t* ds = cv.ds + (size_t)k * comm_ds_row(K2, PW, true);
    int16_t* d1 = ds + (size_t)u * Pp;
    int32_t* d2 = comm_qu_d2(ds, K2, PW);
    uint64_t* wrong = cv.mk + (size_t)k * comm_mk_row(K2, PW, true);
    uint64_t* near = wrong + PW;
    const uint64_t sx = s ? ~0ull : 0ull;
    if constexpr (WAVE) {
        const int lane = (int)threadIdx.x;
        for (int w = 0; w < PW; ++w) {
            const uint64_t cw = c[w] ^ sx;
            const int a = 64 * w + lane;
            const bool in = a < cv.P;
            const int o1 = d1[a], n1 = in ? o1 + 2 - 4 * (int)((cw >> lane) & 1ull) : 0;
            int n2 = d2[a];
            if (in) n2 += (2 * comm_label(cv.lab, a) - 1) * cu * (n1 * n1 - o1 * o1);
            d1[a] = (int16_t)n1;
            d2[a] = n2;
            const uint64_t wr = __ballot(in && n2 <= 0), nr = __ballot(in && comm_qu_near(n2, K1));
            if (lane == 0) { wrong[w] = wr; near[w] = nr; }
        }
        __syncthreads();                                    // (one wavefront per workgroup) the masks are read by every lane
    } else {
        for (int w = 0; w < PW; ++w) {
            const uint64_t cw = c[w] ^ sx, yw = cv.lab[w];
            const int nb = cv.P - 64 * w < 64 ? cv.P - 64 * w : 64;
            uint64_t wr = 0, nr = 0;
            for (int b = 0; b < nb; ++b) {
                const int a = 64 * w + b;
                const int o1 = d1[a], n1 = o1 + 2 - 4 * (int)((cw >> b) & 1ull);
                const int n2 = d2[a] + (2 * (int)((yw >> b) & 1ull) - 1) * cu * (n1 * n1 - o1 * o1);
                d1[a] = (int16_t)n1;
                d2[a] = n2;
                wr |= (uint64_t)(n2 <= 0) << b;
                nr |= (uint64_t)comm_qu_near(n2, K1) << b;
            }
            wrong[w] = wr; near[w] = nr;
        }
    }
}

// update_cache! (CommStep.jl:143-197, CommReLU.jl:149-214, CommQu.jl:154-219) of row k after synapse i was flipped to the spin bit s
template <int KIND, bool WAVE>
__device__ __forceinline__ void comm_update(const CommView& cv, int k, int i, int s)
{
    if constexpr (KIND == CK_QU) { comm_qu_update<WAVE>(cv, k, i, s); return; }
    constexpr bool RELU = KIND == CK_RELU;
    const int PW = cv.PW, K2 = cv.K2, u = i / cv.K1, Pp = 64 * PW;
    const int cu = RELU ? comm_c(u, K2) : 1;
    const uint64_t* c = cv.col + (size_t)i * PW;
    int16_t* d1 = cv.ds + (size_t)k * comm_ds_row(K2, PW, false) + (size_t)u * Pp;
    int16_t* d2 = cv.ds + (size_t)k * comm_ds_row(K2, PW, false) + (size_t)K2 * Pp;
    uint64_t* mk = cv.mk + (size_t)k * comm_mk_row(K2, PW, false);
    uint64_t* p1 = mk + (size_t)u * PW;
    uint64_t* m1 = mk + (size_t)(K2 + u) * PW;
    uint64_t* p2 = mk + (size_t)2 * K2 * PW;
    uint64_t* m2 = p2 + PW;
    const uint64_t sx = s ? ~0ull : 0ull;
    if constexpr (WAVE) {
        const int lane = (int)threadIdx.x;
        for (int w = 0; w < PW; ++w) {
            const uint64_t cw = c[w] ^ sx;
            const int a = 64 * w + lane;
            const bool in = a < cv.P;
            const int o1 = d1[a], n1 = in ? o1 + 2 - 4 * (int)((cw >> lane) & 1ull) : 0;
            int n2 = d2[a];
            if constexpr (RELU) { if (in) n2 += (2 * comm_label(cv.lab, a) - 1) * cu * ((n1 > 0 ? n1 : 0) - (o1 > 0 ? o1 : 0)); }
            else n2 += comm_sign(n1) - comm_sign(o1);
            d1[a] = (int16_t)n1;
            d2[a] = (int16_t)n2;
            const uint64_t q1 = __ballot(in && comm_in_p1<KIND>(n1)), r1 = __ballot(in && comm_in_m1<KIND>(n1));
            const uint64_t q2 = __ballot(in && comm_in_p2<KIND>(n2)), r2 = __ballot(in && comm_in_m2<KIND>(n2));
            if (lane == 0) { p1[w] = q1; m1[w] = r1; p2[w] = q2; m2[w] = r2; }
        }
        __syncthreads();                                    // (one wavefront per workgroup) the masks are read by every lane
    } else {
        for (int w = 0; w < PW; ++w) {
            const uint64_t cw = c[w] ^ sx;
            const uint64_t yw = RELU ? cv.lab[w] : 0ull;
            const int nb = cv.P - 64 * w < 64 ? cv.P - 64 * w : 64;
            uint64_t q1 = 0, r1 = 0, q2 = 0, r2 = 0;
            for (int b = 0; b < nb; ++b) {
                const int a = 64 * w + b;
                const int o1 = d1[a], n1 = o1 + 2 - 4 * (int)((cw >> b) & 1ull);
                int n2 = d2[a];
                if constexpr (RELU) n2 += (2 * (int)((yw >> b) & 1ull) - 1) * cu * ((n1 > 0 ? n1 : 0) - (o1 > 0 ? o1 : 0));
                else n2 += comm_sign(n1) - comm_sign(o1);
                d1[a] = (int16_t)n1;
                d2[a] = (int16_t)n2;
                q1 |= (uint64_t)comm_in_p1<KIND>(n1) << b;
                r1 |= (uint64_t)comm_in_m1<KIND>(n1) << b;
                q2 |= (uint64_t)comm_in_p2<KIND>(n2) << b;
                r2 |= (uint64_t)comm_in_m2<KIND>(n2) << b;
            }
            p1[w] = q1; m1[w] = r1; p2[w] = q2; m2[w] = r2;
        }
    }
}

// debug checks: Δ1, Δ2 and the masks of rows row0 .. rows-1 equal what the configuration gives
template <int KIND>
__device__ inline bool comm_state_bad(const CommParams& Q, const CommView& cv, const uint32_t* sp, int row0, int Nk, int Nbits)
{
    const int K2 = Q.K2, PW = Q.PW, Pp = 64 * PW;
    auto bit = [](const uint64_t* m, int a) { return (int)((m[a >> 6] >> (a & 63)) & 1ull); };
    bool bad = false;
    for (int k = row0; k < Q.rows; ++k) {
        const int16_t* ds = cv.ds + (size_t)k * comm_ds_row(K2, PW, KIND == CK_QU);
        const uint64_t* mk = cv.mk + (size_t)k * comm_mk_row(K2, PW, KIND == CK_QU);
        for (int a = 0; a < Q.P; ++a) {
            int t = 0;
            for (int u = 0; u < K2; ++u) {
                const int d1 = comm_unit_stability(Q, sp, k * Nk, Nbits, u, a);
                t += comm_term<KIND>(d1, u, K2);
                bad = bad || d1 != ds[(size_t)u * Pp + a];
                if constexpr (KIND != CK_QU)
                    bad = bad || bit(mk + (size_t)u * PW, a) != (int)comm_in_p1<KIND>(d1) || bit(mk + (size_t)(K2 + u) * PW, a) != (int)comm_in_m1<KIND>(d1);
            }
            if constexpr (kCommLabelled<KIND>) t *= 2 * comm_label(Q.lab, a) - 1;
            if constexpr (KIND == CK_QU)
                bad = bad || t != comm_qu_d2(ds, K2, PW)[a] || bit(mk, a) != (int)comm_wrong<KIND>(t) || bit(mk + PW, a) != (int)comm_qu_near(t, Q.K1);
            else
                bad = bad || t != ds[(size_t)K2 * Pp + a] || bit(mk + (size_t)2 * K2 * PW, a) != (int)comm_in_p2<KIND>(t) ||
                      bit(mk + (size_t)(2 * K2 + 1) * PW, a) != (int)comm_in_m2<KIND>(t);
        }
    }
    return bad;
}

// ---- the stand-alone graphs: GraphCommStep / GraphCommReLU / GraphCommQu(K1, K2, P) under standardMC --------------------------------------
struct CommMcParams {
    CommParams cm;
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

constexpr int kCommInitThreads = 256;
// energy(X, C) and the Stabilities of every chain, one workgroup per chain
template <int KIND>
__global__ __launch_bounds__(kCommInitThreads) void comm_init_kernel(CommMcParams P)
{
    __shared__ long long s_n;
    const int r = (int)blockIdx.x;
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    comm_init_rows<KIND>(P.cm, comm_view<KIND>(P.cm, r), P.sp + (size_t)r * P.W, P.N, 32 * P.W, &s_n);
    __syncthreads();
    if (threadIdx.x == 0) {
        P.E_cur[r] = (double)s_n;
        P.stats[(size_t)r * 2] = 0; P.stats[(size_t)r * 2 + 1] = 0;
    }
}

// standardMC (src/RRRMC.jl:81-127), one thread per chain, on the streams of perc_standard_kernel: the common SITE stream names the
// synapse, rand() < exp(-β ΔE) on the ACCEPT_F64 stream.  E starts from E_cur (comm_init_kernel, or the run a resumed call continues).
template <int KIND>
__global__ __launch_bounds__(kRrrThreads) void comm_standard_kernel(CommMcParams P)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= P.R) return;
    uint32_t* sp = P.sp + (size_t)r * P.W;
    const CommView cv = comm_view<KIND>(P.cm, r);
    const uint32_t rep = P.replica0 + (uint32_t)r;
    double E = P.E_cur[r];
    int64_t accepted = 0, ns = 0;
    long long next_sample = P.samp0;
    for (int64_t it = 1; it <= P.iters; ++it) {
        if (it == next_sample) { next_sample += P.step; P.Es[ns * P.R + r] = E; ns += 1; }
        const uint64_t g = P.g0 + (uint64_t)it;
        const int i = (int)site_of(P.k0, P.k1, g, (uint32_t)P.N);
        const double dE = comm_residual<KIND>(cv, 0, i, sbit(sp, i));
        const double xx = -P.beta * dE;
        const bool acc = (xx >= 0.0) || (rand53(P.k0, P.k1, g, rep) < det_exp(xx));          // RRRMC.jl:39
        if (acc) {
            sflip(sp, i);
            comm_update<KIND, false>(cv, 0, i, sbit(sp, i));
            E += dE;
            accepted += 1;
        }
    }
    P.E_cur[r] = E;
    P.stats[(size_t)r * 2] = accepted; P.stats[(size_t)r * 2 + 1] = 0;
}

// debug mode (rrrmc_set_debug_checks): the tracked energy, Δ1, Δ2 and the masks against the configuration
template <int KIND>
__global__ __launch_bounds__(64) void comm_check_kernel(CommMcParams P)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= P.R) return;
    const uint32_t* sp = P.sp + (size_t)r * P.W;
    bool bad = comm_state_bad<KIND>(P.cm, comm_view<KIND>(P.cm, r), sp, 0, P.N, 32 * P.W);
    // |ΔE| <= 1e-10 max(1, |E|), as perc_check_kernel: a deliberate departure from the reference's absolute 1e-10 once |E| > 1 (the
    // Float64 energies of GraphCommReLU / GraphCommQu grow with K1 K2 and P; the step graph's integers stay exact)
    const double E = comm_row_energy<KIND>(P.cm, sp, 0, 32 * P.W);
    const double d = E - P.E_cur[r], tol = 1e-10 * (E < -1.0 ? -E : E > 1.0 ? E : 1.0);
    bad = bad || !(d <= tol && d >= -tol);
    if (bad) { atomicAdd(&P.flag[0], 1); P.flag[1] = r; }
}

}  // namespace rrrmc
