// The HIP-free planning core of the cross-replica overlaps (rrrmc_cross_overlaps / rrrmc_overlap_hist): the tile grid over
// (nA, nB) replica pairs, which tiles and pairs of a same-slot histogram count, the caps, the LDS-or-global histogram decision, and the
// batches of slot pairs whose distinct slots are packed together.  Compiles with hipcc (host and device) and with a plain C++ compiler
// (tests/xov_core_check.cpp runs it under the host sanitizers).
//
// q(r1, r2) = pm1dot(a[r1], b[r2]) = N - 2 |a[r1] xor b[r2]| over rows of ceil(N/64) BitVector chunks (scripts/scripts.jl:283-295).
#pragma once
#include <stdint.h>

#include <map>
#include <vector>

#if defined(__HIPCC__)
#define RRRMC_XOV_HD __host__ __device__
#else
#define RRRMC_XOV_HD
#endif

namespace rrrmc {

constexpr int kXovTile = 64;                                 // replicas per side of a workgroup's tile
constexpr int kXovSlab = 16;                                 // 64-bit words of every row staged in LDS at a time
constexpr int kXovPitch = kXovTile + 2;                      // words between two slab columns: 16-byte aligned, off the 256-byte bank row
constexpr int kXovThreads = 256;                             // 16 x 16 threads, a 4 x 4 register tile each
constexpr int kXovTileLdsBytes = 2 * kXovSlab * kXovPitch * 8;   // the A and the B image
constexpr int kXovLdsBudget = 64 * 1024;                     // what one workgroup asks for at most (tiles + histogram)
constexpr int64_t kXovMaxPairs = 65535;                      // slot pairs per call (grid z)
constexpr int64_t kXovMaxMatrix = 1ll << 26;                 // npairs * nA * nB results of a matrix call (256 MiB of int32)
constexpr int64_t kXovMaxTiles = 65535;                      // tiles along A (grid y)
constexpr int64_t kXovPackBytes = 256ll << 20;               // packed copies of a batch's distinct slots

RRRMC_XOV_HD inline int64_t xov_tiles(int64_t n) { return (n + kXovTile - 1) / kXovTile; }
// a histogram over (slot, slot) counts r1 < r2 only: a tile wholly below the diagonal has nothing to count
RRRMC_XOV_HD inline bool xov_tile_skipped(bool same_slot, int64_t ti, int64_t tj) { return same_slot && ti > tj; }
RRRMC_XOV_HD inline bool xov_pair_counted(bool same_slot, int64_t r1, int64_t r2) { return same_slot ? r1 < r2 : r1 != r2; }
inline int64_t xov_counted_pairs(bool same_slot, int64_t R) { return same_slot ? R * (R - 1) / 2 : R * (R - 1); }

// (N + 1) 32-bit bins beside the two tile images within the workgroup's LDS budget
inline bool xov_hist_fits_lds(int64_t N) { return (N + 1) * 4 <= (int64_t)(kXovLdsBudget - kXovTileLdsBytes); }
inline bool xov_hist_in_lds(int64_t N, bool force_global) { return !force_global && xov_hist_fits_lds(N); }

inline bool xov_pairs_ok(int64_t npairs) { return npairs >= 0 && npairs <= kXovMaxPairs; }
inline bool xov_rows_ok(int64_t r0, int64_t n, int64_t R) { return r0 >= 0 && n >= 1 && n <= R && r0 <= R - n; }
// npairs * nA * nB <= kXovMaxMatrix without forming a product that could overflow
inline bool xov_matrix_ok(int64_t npairs, int64_t nA, int64_t nB)
{
    if (npairs < 1 || nA < 1 || nB < 1) return npairs == 0;
    if (nA > kXovMaxMatrix || nB > kXovMaxMatrix) return false;
    const int64_t per = nA * nB;                             // <= 2^52
    return per <= kXovMaxMatrix && npairs <= kXovMaxMatrix / per;
}

// how many distinct slots one batch may hold: what fits the pack budget, at least the two a single pair can name
inline int64_t xov_max_distinct(int64_t R, int64_t nch, int64_t budget_bytes)
{
    const int64_t per = R * nch * 8;
    const int64_t n = per > 0 ? budget_bytes / per : 2;
    return n < 2 ? 2 : n;
}

// pairs p0 .. p1-1 of a call, the distinct slots they name in order of first appearance (-1, the live configuration, is a slot like any
// other) and each pair's indices into that list
struct XovBatch {
    int64_t p0 = 0, p1 = 0;
    std::vector<int32_t> slots;
    std::vector<int32_t> ia, ib;                             // [p1 - p0]
};

// the longest run of pairs from p0 on that names at most max_distinct (>= 2) slots
inline XovBatch xov_next_batch(const int32_t* slotA, const int32_t* slotB, int64_t p0, int64_t npairs, int64_t max_distinct)
{
    XovBatch b;
    b.p0 = b.p1 = p0;
    std::map<int32_t, int32_t> at;
    for (int64_t p = p0; p < npairs; ++p) {
        const int32_t sa = slotA[p], sb = slotB[p];
        const int64_t fresh = (at.count(sa) ? 0 : 1) + (sb != sa && !at.count(sb) ? 1 : 0);
        if ((int64_t)b.slots.size() + fresh > max_distinct) break;
        for (const int32_t s : {sa, sb})
            if (!at.count(s)) { at[s] = (int32_t)b.slots.size(); b.slots.push_back(s); }
        b.ia.push_back(at[sa]);
        b.ib.push_back(at[sb]);
        b.p1 = p + 1;
    }
    return b;
}

}  // namespace rrrmc
