// Stand-alone check of rrrmc.jl_amd/csrc/xov_core.hpp, the HIP-free planning core of the cross-replica overlaps, meant to be built with
// g++ -fsanitize=address,undefined (tests/test_xov_sanitize_cpu.py): the tile grid, the same-slot triangle, the batches of slot pairs
// with their distinct-slot lists, the caps and the histogram-form decision at their boundaries.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../rrrmc.jl_amd/csrc/xov_core.hpp"

using namespace rrrmc;

#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } \
    } while (0)

// the rows thread (ty, tx) of xov_tile_kernel owns inside a tile
static int tile_row(int t, int i) { return (i >> 1) * 32 + 2 * t + (i & 1); }

int main()
{
    // a thread's four rows, over the 16 threads of a side, are the 64 rows of the tile, each once; the LDS image is 16-byte aligned
    {
        std::vector<int> seen(kXovTile, 0);
        for (int t = 0; t < 16; ++t)
            for (int i = 0; i < 4; ++i) { CHECK(tile_row(t, i) >= 0 && tile_row(t, i) < kXovTile); ++seen[(size_t)tile_row(t, i)]; }
        for (int v : seen) CHECK(v == 1);
        CHECK(kXovThreads == 16 * 16 && kXovTile == 4 * 16 && (kXovPitch * 8) % 16 == 0 && kXovPitch >= kXovTile);
        CHECK(kXovTileLdsBytes == 2 * kXovSlab * kXovPitch * 8 && kXovTileLdsBytes < kXovLdsBudget);
    }
    // the tile grid covers every (i, j) of (nA, nB) exactly once
    const int64_t sizes[] = {1, 63, 64, 65, 200};
    for (int64_t nA : sizes)
        for (int64_t nB : sizes) {
            std::vector<int> hit((size_t)(nA * nB), 0);
            for (int64_t ti = 0; ti < xov_tiles(nA); ++ti)
                for (int64_t tj = 0; tj < xov_tiles(nB); ++tj)
                    for (int ty = 0; ty < 16; ++ty)
                        for (int tx = 0; tx < 16; ++tx)
                            for (int i = 0; i < 4; ++i)
                                for (int j = 0; j < 4; ++j) {
                                    const int64_t ra = ti * kXovTile + tile_row(ty, i), rb = tj * kXovTile + tile_row(tx, j);
                                    if (ra < nA && rb < nB) ++hit[(size_t)(ra * nB + rb)];
                                }
            for (int v : hit) CHECK(v == 1);
            CHECK(xov_tiles(nA) * kXovTile >= nA && (xov_tiles(nA) - 1) * kXovTile < nA);
        }
    // the same-slot triangle: skipped tiles hold no counted pair, and the others count exactly R (R - 1) / 2; two slots count R (R - 1)
    const int64_t Rs[] = {1, 2, 33, 70, 129};
    for (int64_t R : Rs) {
        int64_t same = 0, diff = 0;
        for (int64_t ti = 0; ti < xov_tiles(R); ++ti)
            for (int64_t tj = 0; tj < xov_tiles(R); ++tj)
                for (int64_t ra = ti * kXovTile; ra < (ti + 1) * kXovTile && ra < R; ++ra)
                    for (int64_t rb = tj * kXovTile; rb < (tj + 1) * kXovTile && rb < R; ++rb) {
                        if (xov_tile_skipped(true, ti, tj)) CHECK(!xov_pair_counted(true, ra, rb));
                        else same += xov_pair_counted(true, ra, rb);
                        CHECK(!xov_tile_skipped(false, ti, tj));
                        diff += xov_pair_counted(false, ra, rb);
                    }
        CHECK(same == R * (R - 1) / 2 && same == xov_counted_pairs(true, R));
        CHECK(diff == R * (R - 1) && diff == xov_counted_pairs(false, R));
    }
    // the distinct-slot list of a batch, with -1 and repeated slots
    {
        const std::vector<int32_t> a = {0, 2, -1, 2, 5, 0}, b = {1, 2, 0, -1, 5, 7};
        XovBatch bt = xov_next_batch(a.data(), b.data(), 0, (int64_t)a.size(), 100);
        CHECK(bt.p0 == 0 && bt.p1 == 6);
        CHECK((bt.slots == std::vector<int32_t>{0, 1, 2, -1, 5, 7}));
        CHECK((bt.ia == std::vector<int32_t>{0, 2, 3, 2, 4, 0}) && (bt.ib == std::vector<int32_t>{1, 2, 0, 3, 4, 5}));
        for (size_t p = 0; p < a.size(); ++p) CHECK(bt.slots[(size_t)bt.ia[p]] == a[p] && bt.slots[(size_t)bt.ib[p]] == b[p]);
        // small budgets: every pair lands in exactly one batch, in order, and no batch names more slots than allowed
        for (int64_t cap = 2; cap <= 7; ++cap) {
            int64_t p0 = 0, batches = 0;
            while (p0 < (int64_t)a.size()) {
                bt = xov_next_batch(a.data(), b.data(), p0, (int64_t)a.size(), cap);
                CHECK(bt.p0 == p0 && bt.p1 > p0 && (int64_t)bt.slots.size() <= cap);
                CHECK((int64_t)bt.ia.size() == bt.p1 - bt.p0 && bt.ib.size() == bt.ia.size());
                for (int64_t p = bt.p0; p < bt.p1; ++p) {
                    const int32_t ia = bt.ia[(size_t)(p - p0)], ib = bt.ib[(size_t)(p - p0)];
                    CHECK(ia >= 0 && ib >= 0 && (size_t)ia < bt.slots.size() && (size_t)ib < bt.slots.size());
                    CHECK(bt.slots[(size_t)ia] == a[(size_t)p] && bt.slots[(size_t)ib] == b[(size_t)p]);
                    CHECK((ia == ib) == (a[(size_t)p] == b[(size_t)p]));
                }
                for (size_t s = 0; s < bt.slots.size(); ++s)
                    for (size_t t = s + 1; t < bt.slots.size(); ++t) CHECK(bt.slots[s] != bt.slots[t]);
                p0 = bt.p1;
                ++batches;
            }
            CHECK(cap < 6 ? batches > 1 : batches == 1);
        }
        CHECK(xov_max_distinct(8192, 64, kXovPackBytes) == 64 && xov_max_distinct(8192, 64, 1) == 2 && xov_max_distinct(1, 1, 80) == 10);
    }
    // the caps, at their boundaries
    CHECK(xov_pairs_ok(0) && xov_pairs_ok(65535) && !xov_pairs_ok(65536) && !xov_pairs_ok(-1));
    CHECK(xov_matrix_ok(1, 8192, 8192) && !xov_matrix_ok(2, 8192, 8192) && xov_matrix_ok(65535, 32, 32) && !xov_matrix_ok(65535, 32, 33));
    CHECK(xov_matrix_ok(1, 1, kXovMaxMatrix) && !xov_matrix_ok(1, 1, kXovMaxMatrix + 1) && !xov_matrix_ok(1, kXovMaxMatrix + 1, 1));
    CHECK(!xov_matrix_ok(65535, INT64_MAX / 2, INT64_MAX / 2) && xov_matrix_ok(0, 5, 5) && !xov_matrix_ok(1, 0, 5));
    CHECK(xov_matrix_ok(13695, 70, 70) && !xov_matrix_ok(13696, 70, 70));          // 2^26 / 4900 = 13695.7
    CHECK(xov_rows_ok(0, 70, 70) && xov_rows_ok(69, 1, 70) && !xov_rows_ok(69, 2, 70) && !xov_rows_ok(-1, 1, 70) && !xov_rows_ok(0, 0, 70));
    CHECK(!xov_rows_ok(0, 71, 70) && !xov_rows_ok(INT64_MAX, 1, 70) && !xov_rows_ok(1, INT64_MAX, 70));
    // the histogram form: (N + 1) bins beside the tiles, or global atomics
    {
        const int64_t Nmax = (kXovLdsBudget - kXovTileLdsBytes) / 4 - 1;
        CHECK(xov_hist_fits_lds(Nmax) && !xov_hist_fits_lds(Nmax + 1) && xov_hist_fits_lds(4096) && xov_hist_fits_lds(1));
        CHECK(xov_hist_in_lds(Nmax, false) && !xov_hist_in_lds(Nmax + 1, false) && !xov_hist_in_lds(10, true));
        CHECK(kXovTileLdsBytes + 4 * (Nmax + 1) <= kXovLdsBudget && kXovTileLdsBytes + 4 * (Nmax + 2) > kXovLdsBudget);
    }
    std::printf("xov_core_check: all invariants hold\n");
    return 0;
}
