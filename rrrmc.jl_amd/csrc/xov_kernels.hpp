// Overlaps between DIFFERENT replicas of stored configurations: q(r1, r2) = N - 2 |a[r1] xor b[r2]|, a bit-matrix product
// over rows of ceil(N/64) BitVector chunks.  Every layout is first brought to that one row form (spins_pack_kernel, layout_kernels.hpp;
// the chunk layouts have it already), so there is one kernel, with two epilogues: the int32 matrix, or the histogram of Hamming distances.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "xov_core.hpp"

namespace rrrmc {

// grid (tiles of B, tiles of A, slot pairs), block 256 = 16 x 16 threads; thread (ty, tx) holds the 4 x 4 counts of the A rows
// {2ty, 2ty+1, 32+2ty, 33+2ty} against the B rows {2tx, 2tx+1, 32+2tx, 33+2tx} of the tile.
//   rows[s]   : [R][nch] chunks of the call's s-th distinct slot;  ia[p], ib[p] : the two slots of pair p
//   LDS image : word k of a slab, row r at s[k * kXovPitch + r] — the 16 lanes of a ds_read_b128 group read 256 contiguous bytes (two
//               rows each), so no two of them share a bank; the +2 words of pitch spread the staging writes (same row, 16 columns)
//   matrix    : q[(p * nA + i) * nB + j] for the rows a0 + i, b0 + j; rows beyond nA / nB are neither read nor written
//   histogram : (a0, b0) = (0, 0), nA = nB = R; bin d += 1 for every counted pair (xov_pair_counted) at Hamming distance d; lds_bins != 0:
//               (N + 1) 32-bit bins in dynamic LDS, flushed with one 64-bit atomic per non-zero bin, else one global atomic per pair
// The bits beyond N in a row's last chunk are masked off as the row is staged.
template <bool HIST>
__global__ __launch_bounds__(kXovThreads) void xov_tile_kernel(const unsigned long long* const* __restrict__ rows, const int32_t* __restrict__ ia,
                                                               const int32_t* __restrict__ ib, int N, int nch, int a0, int nA, int b0, int nB,
                                                               int32_t* __restrict__ q, unsigned long long* __restrict__ hist, int lds_bins)
{
    __shared__ __attribute__((aligned(16))) unsigned long long sA[kXovSlab * kXovPitch];
    __shared__ __attribute__((aligned(16))) unsigned long long sB[kXovSlab * kXovPitch];
    extern __shared__ uint32_t xov_bins[];
    const int p = (int)blockIdx.z, ti = (int)blockIdx.y, tj = (int)blockIdx.x;
    const bool same = ia[p] == ib[p];
    if (HIST && xov_tile_skipped(same, ti, tj)) return;          // uniform over the workgroup
    const unsigned long long* __restrict__ A = rows[ia[p]];
    const unsigned long long* __restrict__ B = rows[ib[p]];
    const int tid = (int)threadIdx.x, tx = tid & 15, ty = tid >> 4;
    if (HIST && lds_bins)
        for (int d = tid; d <= N; d += kXovThreads) xov_bins[d] = 0u;          // ordered before the epilogue by the slab barriers (nch >= 1)
    const unsigned long long tail = (N & 63) ? (~0ull >> (64 - (N & 63))) : ~0ull;
    uint32_t cnt[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) cnt[i][j] = 0u;

    for (int k0 = 0; k0 < nch; k0 += kXovSlab) {
        const int ks = nch - k0 < kXovSlab ? nch - k0 : kXovSlab;              // the last slab is shorter
        for (int e = tid; e < kXovTile * kXovSlab; e += kXovThreads) {
            const int row = e / kXovSlab, k = e % kXovSlab, c = k0 + k;
            const int ra = ti * kXovTile + row, rb = tj * kXovTile + row;
            unsigned long long va = 0ull, vb = 0ull;
            if (c < nch) {
                if (ra < nA) va = A[(size_t)(a0 + ra) * (size_t)nch + (size_t)c];
                if (rb < nB) vb = B[(size_t)(b0 + rb) * (size_t)nch + (size_t)c];
                if (c == nch - 1) { va &= tail; vb &= tail; }
            }
            sA[k * kXovPitch + row] = va;
            sB[k * kXovPitch + row] = vb;
        }
        __syncthreads();
        for (int k = 0; k < ks; ++k) {
            const ulonglong2 a01 = *reinterpret_cast<const ulonglong2*>(&sA[k * kXovPitch + 2 * ty]);
            const ulonglong2 a23 = *reinterpret_cast<const ulonglong2*>(&sA[k * kXovPitch + 32 + 2 * ty]);
            const ulonglong2 b01 = *reinterpret_cast<const ulonglong2*>(&sB[k * kXovPitch + 2 * tx]);
            const ulonglong2 b23 = *reinterpret_cast<const ulonglong2*>(&sB[k * kXovPitch + 32 + 2 * tx]);
            const unsigned long long a[4] = {a01.x, a01.y, a23.x, a23.y};
            const unsigned long long b[4] = {b01.x, b01.y, b23.x, b23.y};
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) cnt[i][j] += (uint32_t)__popcll(a[i] ^ b[j]);
        }
        __syncthreads();
    }

#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int ra = ti * kXovTile + (i >> 1) * 32 + 2 * ty + (i & 1);
        if (ra >= nA) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int rb = tj * kXovTile + (j >> 1) * 32 + 2 * tx + (j & 1);
            if (rb >= nB) continue;
            if (!HIST) {
                q[((size_t)p * (size_t)nA + (size_t)ra) * (size_t)nB + (size_t)rb] = N - 2 * (int32_t)cnt[i][j];
            } else if (xov_pair_counted(same, ra, rb)) {
                if (lds_bins) atomicAdd(&xov_bins[cnt[i][j]], 1u);
                else atomicAdd(&hist[cnt[i][j]], 1ull);
            }
        }
    }
    if (HIST && lds_bins) {
        __syncthreads();
        for (int d = tid; d <= N; d += kXovThreads) {
            const uint32_t v = xov_bins[d];
            if (v) atomicAdd(&hist[d], (unsigned long long)v);
        }
    }
}

}  // namespace rrrmc
