// Replica exchange between two contexts of one graph (rrrmc_exchange_async): ONE kernel decides and swaps.
//
// A workgroup serves one replica group of the native spin layout — the replicas that share a word — and one range of that group's
// words.  Its wavefronts derive the group's verdicts from the two energy arrays, one replica per lane (pt_core.hpp: the rule, the
// EXCHANGE stream), ballot them into the group's mask, and blend their words of the two buffers:
//     t = (a ^ b) & m;  a ^= t;  b ^= t
// Replica r occupies the same bits of the same words in both contexts' buffers, so the blend is the whole exchange.  A group whose mask
// is zero returns before it loads a word.  The workgroups of word range 0 also write the mask words and the two energies (the call's
// results).  Bits of replicas >= R are never set: the padding replicas of the last group come out as they went in.
//
// Layouts (layout_kernels.hpp: bit b of a word = replica group * W + b):
//   d_spins  [G][N]   uint32    W = 32: the group's mask word
//   pf_spins [pfW][N] uint64    W = 64: two consecutive mask words
//   sk_spins [G8][N]  uint8     W = 8:  one byte of a mask word
//   q_spins  [R][qW]  uint32    a row per replica: a group is 32 rows, a row is swapped whole or not at all
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pt_core.hpp"

namespace rrrmc {

constexpr int kPtThreads = 256;
constexpr int kPtWordsPerThread = 8;          // 16-byte accesses: two (uint32 x 4 twice), four (uint64 x 2), half of one (bytes x 16, one access)

struct PtParams {
    void* sa; void* sb;                       // the two native spin buffers
    const void* Ea; const void* Eb;           // energies of the live configurations: int32 level units (EINT) or Float64, [Rpad]
    uint32_t* mask32;                         // [ceil(Rpad / 32)] out: the verdicts
    double* Ea_out; double* Eb_out;           // [R] out: the energies the verdicts were taken from, in the model's units
    double beta_a, beta_b;
    long long lv_mul; double lv_div;          // EINT: units -> Float64
    uint64_t round;
    uint32_t k0, k1, replica0;
    int R;
    long long len;                            // words per group (N), or words per row (qW) in the row layout
};

// verdict of replica r (false beyond R); the word-range-0 workgroups also record the energies
template <bool EINT>
__device__ __forceinline__ bool pt_decide(const PtParams& P, int r, bool record)
{
    if (r >= P.R) return false;
    double ea, eb;
    if constexpr (EINT) {
        ea = pt_units_to_f64((long long)((const int32_t*)P.Ea)[r], P.lv_mul, P.lv_div);
        eb = pt_units_to_f64((long long)((const int32_t*)P.Eb)[r], P.lv_mul, P.lv_div);
    } else {
        ea = ((const double*)P.Ea)[r];
        eb = ((const double*)P.Eb)[r];
    }
    if (record) { P.Ea_out[r] = ea; P.Eb_out[r] = eb; }
    return pt_accept(P.beta_a, P.beta_b, ea, eb, pt_rand(P.k0, P.k1, P.round, P.replica0 + (uint32_t)r));
}

template <typename V>
__device__ __forceinline__ void pt_blend(V* __restrict__ a, V* __restrict__ b, V m)
{
    const V x = *a, y = *b;
    const V t = (x ^ y) & m;
    *a = x ^ t;
    *b = y ^ t;
}

// words [w0, w1) of two rows with one mask for all of them; 16-byte accesses over the aligned middle when both rows are congruent mod 16
template <typename WordT>
__device__ __forceinline__ void pt_blend_range(WordT* __restrict__ a, WordT* __restrict__ b, long long w0, long long w1, WordT m, int tid, int nth)
{
    constexpr int VW = 16 / (int)sizeof(WordT);
    typedef WordT VecT __attribute__((ext_vector_type(VW)));
    const uintptr_t pa = (uintptr_t)(a + w0), pb = (uintptr_t)(b + w0);
    if ((pa & 15u) != (pb & 15u)) {           // (never with the library's allocations: both buffers start 256-byte aligned)
        for (long long w = w0 + tid; w < w1; w += nth) pt_blend(a + w, b + w, m);
        return;
    }
    long long head = (long long)(((16u - (pa & 15u)) & 15u) / sizeof(WordT));
    if (head > w1 - w0) head = w1 - w0;
    const long long nvec = (w1 - w0 - head) / VW;
    const long long tail0 = w0 + head + nvec * VW;
    if (tid < head) pt_blend(a + w0 + tid, b + w0 + tid, m);
    VecT mv;
#pragma unroll
    for (int i = 0; i < VW; ++i) mv[i] = m;
    VecT* va = (VecT*)(a + w0 + head);
    VecT* vb = (VecT*)(b + w0 + head);
    for (long long v = tid; v < nvec; v += nth) pt_blend(va + v, vb + v, mv);
    if (tail0 + tid < w1) pt_blend(a + tail0 + tid, b + tail0 + tid, m);          // fewer than VW <= 16 words
}

// The replica-in-word layouts: grid (word ranges, groups).
template <typename WordT, bool EINT>
__global__ __launch_bounds__(kPtThreads) void pt_exchange_kernel(PtParams P)
{
    constexpr int W = (int)sizeof(WordT) * 8;                 // replicas per word: 32, 64, 8
    const int g = (int)blockIdx.y, tid = (int)threadIdx.x, lane = tid & 63;
    const bool first = blockIdx.x == 0;
    const bool v = pt_decide<EINT>(P, g * W + (lane & (W - 1)), first && tid < W);
    const unsigned long long bal = __ballot((int)v);          // lanes W .. 63 repeat lanes 0 .. W - 1
    const WordT m = (WordT)bal;
    if (first && tid == 0) {
        if constexpr (W == 64) { P.mask32[2 * g] = (uint32_t)bal; P.mask32[2 * g + 1] = (uint32_t)(bal >> 32); }
        else if constexpr (W == 32) P.mask32[g] = (uint32_t)bal;
        else ((uint8_t*)P.mask32)[g] = (uint8_t)bal;          // little endian: byte g of the mask = replicas 8 g .. 8 g + 7
    }
    if (m == (WordT)0) return;
    const long long per = (long long)kPtThreads * kPtWordsPerThread * (W == 8 ? 8 : 1);       // bytes: 64 per thread
    const long long w0 = (long long)blockIdx.x * per;
    long long w1 = w0 + per;
    if (w1 > P.len) w1 = P.len;
    WordT* a = (WordT*)P.sa + (size_t)g * (size_t)P.len;
    WordT* b = (WordT*)P.sb + (size_t)g * (size_t)P.len;
    pt_blend_range<WordT>(a, b, w0, w1, m, tid, kPtThreads);
}

// The row layout (q_spins[R][qW]): grid (word ranges of a row, groups of 32 rows); the accepted rows are swapped whole.
template <bool EINT>
__global__ __launch_bounds__(kPtThreads) void pt_exchange_rows_kernel(PtParams P)
{
    const int g = (int)blockIdx.y, tid = (int)threadIdx.x, lane = tid & 63;
    const bool first = blockIdx.x == 0;
    const bool v = pt_decide<EINT>(P, g * 32 + (lane & 31), first && tid < 32);
    uint32_t m = (uint32_t)__ballot((int)v);
    if (first && tid == 0) P.mask32[g] = m;
    const long long per = (long long)kPtThreads * kPtWordsPerThread;
    const long long w0 = (long long)blockIdx.x * per;
    long long w1 = w0 + per;
    if (w1 > P.len) w1 = P.len;
    while (m) {                                               // wave-uniform: every lane holds the same mask
        const int bit = __builtin_ctz(m);
        m &= m - 1u;
        const size_t row = (size_t)(g * 32 + bit) * (size_t)P.len;
        pt_blend_range<uint32_t>((uint32_t*)P.sa + row, (uint32_t*)P.sb + row, w0, w1, ~0u, tid, kPtThreads);
    }
}

}  // namespace rrrmc
