// HIP-free core of the Topological Local Entropy ensemble (src/graphs/TLE.jl): the constructor's checks of the neighbour lists ∂i
// (TLE.jl:33-46), the neighbour program of the inner graph GraphTLE{M,γT,λT} (TLE.jl:313-333), its level table allΔE (TLE.jl:335-347) and the
// class-code table the kernels look classes up in.  Plain C++: included by host_tle.hpp and tle_kernels.hpp, and compiled on its own with
// g++ -fsanitize=address,undefined by tests/tle_core_check.cpp.
//
// ∂i crosses the ABI as ordered 0-based lists in CSR form, rowptr[Nk + 1] and cols[rowptr[Nk]].  The messages carry the reference's 1-based
// numbers and its wording.
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <vector>

namespace rrrmc {

constexpr int kTleMmax = 31;                                // replicas M (M + 1 rows)
constexpr int64_t kTleNmax = 65535;                         // 16-bit set members and positions
constexpr int64_t kTleClassMax = 65535;                     // 2L: 16-bit class ids
constexpr uint32_t kTleNoCode = 0xFFFFFFFFu;                // code of a field pair that has no level
constexpr uint32_t kTleCodeUp = 0x40000000u;                // ΔE > 0
constexpr uint32_t kTleCodeZero = 0x80000000u;              // ΔE == 0: `up` follows the spin (DeltaE.jl:83)

// The checks of GraphTLE's constructor on the lists (TLE.jl:34-46), in its order: per list the range, no self-loop, no duplicate; then
// symmetry.  Returns 0, or 1 with the reference's message.  maxdeg = max |∂i|.
inline int tle_check_topology(int64_t Nk, const int32_t* rowptr, const int32_t* cols, int64_t* maxdeg, char* msg, size_t msg_len)
{
    if (Nk < 1) { snprintf(msg, msg_len, "Nk must be >= 1, given: %lld", (long long)Nk); return 1; }
    if (!rowptr) { snprintf(msg, msg_len, "rowptr is NULL"); return 1; }
    if (rowptr[0] != 0) { snprintf(msg, msg_len, "invalid neighb argument, rowptr[0] must be 0, given: %d", rowptr[0]); return 1; }
    for (int64_t i = 0; i < Nk; ++i)
        if (rowptr[i + 1] < rowptr[i]) { snprintf(msg, msg_len, "invalid neighb argument, rowptr decreases at %lld", (long long)(i + 1)); return 1; }
    if (rowptr[Nk] > 0 && !cols) { snprintf(msg, msg_len, "cols is NULL"); return 1; }
    int64_t md = 0;
    std::vector<int32_t> first((size_t)Nk, -1), stamp((size_t)Nk, -1);
    for (int64_t i = 0; i < Nk; ++i) {
        const int32_t* ni = cols + rowptr[i];
        const int64_t l = rowptr[i + 1] - rowptr[i];
        for (int64_t p = 0; p < l; ++p)
            if (ni[p] < 0 || ni[p] >= Nk) {
                snprintf(msg, msg_len, "invalid neighb[%lld] argument, all elements must be between 1 and %lld", (long long)(i + 1), (long long)Nk);
                return 1;
            }
        for (int64_t p = 0; p < l; ++p)
            if (ni[p] == i) { snprintf(msg, msg_len, "invalid neighb[%lld], contains itself", (long long)(i + 1)); return 1; }
        int64_t dup = -1;                                   // the smallest position that has a later equal: the pair the reference's loops meet first
        for (int64_t p = 0; p < l; ++p) {
            const size_t v = (size_t)ni[p];
            if (stamp[v] == (int32_t)i) { if (dup < 0 || first[v] < dup) dup = first[v]; }
            else { stamp[v] = (int32_t)i; first[v] = (int32_t)p; }
        }
        if (dup >= 0) { snprintf(msg, msg_len, "duplicated element %lld in neighb[%lld]", (long long)(dup + 1), (long long)(i + 1)); return 1; }
        md = l > md ? l : md;
    }
    std::vector<int32_t> sorted(cols, cols + rowptr[Nk]);
    for (int64_t i = 0; i < Nk; ++i) std::sort(sorted.begin() + rowptr[i], sorted.begin() + rowptr[i + 1]);
    for (int64_t i = 0; i < Nk; ++i)
        for (int64_t p = rowptr[i]; p < rowptr[i + 1]; ++p) {
            const int32_t i1 = cols[p];
            if (!std::binary_search(sorted.begin() + rowptr[i1], sorted.begin() + rowptr[i1 + 1], (int32_t)i)) {
                snprintf(msg, msg_len, "neighb is not symmetrical, %d ∈ ∂%lld but %lld ∉ ∂%d", i1 + 1, (long long)(i + 1), (long long)(i + 1), i1 + 1);
                return 1;
            }
        }
    if (maxdeg) *maxdeg = md;
    return 0;
}

// neighbors(X0, j) (TLE.jl:313-333), 0-based ABI sites j = i (M+1) + k.  A centre (k = 0): its M replicas ascending, then for each i1 ∈ ∂i in
// list order the whole slice interval of i1, centre first.  A replica (i, k): the centre, then for each i1 ∈ ∂i the centre of i1, then (i1, k).
inline int64_t tle_neighbor_count(int M, const int32_t* rowptr, int64_t j)
{
    const int64_t i = j / (M + 1), k = j % (M + 1), deg = rowptr[i + 1] - rowptr[i];
    return k == 0 ? M + (int64_t)(M + 1) * deg : 1 + 2 * deg;
}
// the q-th neighbour of site j = (i, k) whose list starts at ni
#if defined(__HIP_DEVICE_COMPILE__) || defined(__HIPCC__)
__host__ __device__
#endif
inline int tle_neighbor(int M, const int32_t* ni, int i, int k, int q)
{
    const int rows = M + 1;
    if (k == 0) {
        if (q < M) return i * rows + q + 1;
        const int p = q - M, n = p / rows;
        return ni[n] * rows + (p - n * rows);
    }
    if (q == 0) return i * rows;
    const int p = q - 1;
    return ni[p >> 1] * rows + ((p & 1) ? k : 0);
}

// length of ΔE1 of allΔE (TLE.jl:337-338)
inline int tle_len1(int64_t M) { return (int)(M % 2 == 0 ? M / 2 + 2 : (M + 1) / 2); }

// allΔE(GraphTLE{M,γT,λT}) = sort(unique(abs.(ΔE1 .+ ΔE2'))) (TLE.jl:335-347): ΔE1 the levels of GraphLE without the abs (M even: 4dγT for
// d = 0 .. M/2 with 2γT inserted second; M odd: 2(2d-1)γT), ΔE2 = 2dλT for d = -mn .. mn, mn = M max|∂i|.  Julia multiplies the integer
// factors first (4*d*γT = (4d) γT).
inline void tle_tables(int64_t M, double gT, double lT, int64_t maxdeg, std::vector<double>& out)
{
    std::vector<double> e1;
    if (M % 2 == 0) {
        for (int64_t d = 0; d <= M / 2; ++d) e1.push_back((double)(4 * d) * gT);
        e1.insert(e1.begin() + 1, 2 * gT);
    } else {
        for (int64_t d = 1; d <= (M + 1) / 2; ++d) e1.push_back((double)(2 * (2 * d - 1)) * gT);
    }
    const int64_t mn = M * maxdeg;
    out.clear();
    out.reserve(e1.size() * (size_t)(2 * mn + 1));
    for (int64_t d = -mn; d <= mn; ++d) {
        const double e2 = (double)(2 * d) * lT;
        for (double a : e1) out.push_back(fabs(a + e2));
    }
    std::sort(out.begin(), out.end());
    out.erase(std::unique(out.begin(), out.end()), out.end());
}

// findk(ΔElist, dE) (DeltaE.jl:26-60) as its generated code runs: 1-based, a binary search down to ranges of fewer than 10 entries, which are
// scanned in ascending order; 0 = not found
inline int tle_findk(const double* t, int imin, int imax, int i, double dE)
{
    if (imax - imin < 10) {
        for (int j = imin; j <= imax; ++j)
            if (dE == t[j - 1]) return j;
        return 0;
    }
    const double cE = t[i - 1];
    if (cE == dE) return i;
    if (cE < dE) return tle_findk(t, i + 1, imax, (i + 1 + imax) / 2, dE);
    return tle_findk(t, imin, i - 1, (imin + i - 1) / 2, dE);
}

// ΔE0 of a site whose two integer fields are lf1, lf2 (TLE.jl:301-311): 2γT lfields1 + 2λT lfields2 in that order
#if defined(__HIP_DEVICE_COMPILE__) || defined(__HIPCC__)
__host__ __device__
#endif
inline double tle_delta0(double g2, double l2, int lf1, int lf2) { return g2 * (double)lf1 + l2 * (double)lf2; }

// The class-code table, [2M + 1][2mn + 1] by (lfields1 + M, lfields2 + mn): the level a = findk(allΔE, |ΔE0|) - 1, kTleCodeUp when
// ΔE0 > 0, kTleCodeZero when ΔE0 == 0 (DeltaE.jl:80-86), kTleNoCode when findk finds no level.  Returns false when a pair the fields can
// take (a replica's lfields1 is ±1 with |lfields2| <= max|∂i|, a centre's has the parity of M) has none.
inline bool tle_codes(int64_t M, double gT, double lT, int64_t maxdeg, const std::vector<double>& dElist, std::vector<uint32_t>& code)
{
    const int64_t mn = M * maxdeg, nc = 2 * mn + 1;
    const int L = (int)dElist.size();
    const double g2 = 2 * gT, l2 = 2 * lT;
    code.assign((size_t)((2 * M + 1) * nc), kTleNoCode);
    for (int64_t lf1 = -M; lf1 <= M; ++lf1)
        for (int64_t lf2 = -mn; lf2 <= mn; ++lf2) {
            const double dE = tle_delta0(g2, l2, (int)lf1, (int)lf2);
            const int a = tle_findk(dElist.data(), 1, L, (1 + L) / 2, fabs(dE));
            const bool reach = ((lf1 == 1 || lf1 == -1) && lf2 >= -maxdeg && lf2 <= maxdeg) || ((lf1 - M) % 2 == 0);
            if (a == 0) {
                if (reach) return false;
                continue;
            }
            code[(size_t)((lf1 + M) * nc + (lf2 + mn))] = (uint32_t)(a - 1) | (dE > 0 ? kTleCodeUp : 0u) | (dE == 0 ? kTleCodeZero : 0u);
        }
    return true;
}

// class a + L up of a site with the given code and spin bit s (DeltaE.jl:80-86)
#if defined(__HIP_DEVICE_COMPILE__) || defined(__HIPCC__)
__host__ __device__
#endif
inline int tle_class_of(uint32_t c, int L, int s)
{
    const int up = (c & kTleCodeUp) != 0 || ((c & kTleCodeZero) != 0 && s == 1);
    return (int)(c & 0x3FFFFFFFu) + L * up;
}

}  // namespace rrrmc
