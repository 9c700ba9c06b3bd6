// gfx950 kernels for the Topological Local Entropy ensemble (src/graphs/TLE.jl): GraphTopologicalLocalEntropy{M,γT,λT,G} = the inner graph
// GraphTLE{M,γT,λT} plus a centre graph and M slice graphs of one graph G — GraphEmpty (Graph0TLE), binary GraphSK (GraphSKTLE), GraphSKNormal,
// GraphSAT (GraphSATTLE, src/TLEAliases.jl), GraphEANormal (GraphEATLE; its ∂i is uA[i], each lattice neighbour once).  Samplers: rrrMC(X::DoubleGraph) (src/RRRMC.jl:221-290) over the DeltaECache{Float64,L}
// (src/DeltaE.jl:63-295) and standardMC (src/RRRMC.jl:81-127); the observables are LE's kernel (TLEenergies / cenergy / distances read the
// slices only, TLE.jl:437-502).
//
// Layout.  Sites and the slice-major working copy are LE's (le_kernels.hpp): ABI site j = i (M+1) + k, k = 0 the centre; the
// kernels work on x = k Nk + i with M + 1 rows and the slice helpers of re_kernels.hpp run unchanged on it.
//
// GraphTLE keeps two integer caches (TLE.jl:79-142).  lfields1 is GraphLE's and is never stored: σc σ_(i,k) on a replica site, σc μ_i on a
// centre, from the spins and the stored μ_i.  lfields2 is the topological field over the slice graph's neighbourhoods ∂i:
//     replica (i,k):  σ_(i,k) σc_i Σ_{i2 ∈ ∂i} σc_i2 σ_(i2,k)          centre i:  Σ_k lfields2(i,k)
// (the centre's value, σc_i Σ_{i2} σc_i2 Σ_k σ_(i,k) σ_(i2,k), is that sum term by term).  It is stored by ABI site during rrrMC, since
// recomputing it costs |∂i| spin reads, and kept by the increments of update_cache! (TLE.jl:246-295), which are functions of the spins:
//     replica move (i,k), σx its new spin:  lfields2(i,k) changes sign, the centre i takes twice the new value; for i1 ∈ ∂i both (i1,k) and the
//         centre of i1 take + 2 σx σc_i σ_(i1,k) σc_i1
//     centre move i, σc its new spin:  the whole interval of i changes sign; for i1 ∈ ∂i, (i1,k) takes + 2 σ_(i,k) σc σ_(i1,k) σc_i1 and the
//         centre of i1 the sum of those over k.
// The move_last swap of an immediate undo restores the integers these increments restore (tests/tle_reference.py checks both against the
// definition).  A class is a look-up by (lfields1, lfields2) in the table the host fills with findk run literally (tle_core.hpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "le_kernels.hpp"
#include "tle_core.hpp"

namespace rrrmc {

// LeParams with L = the length of allΔE(GraphTLE), tab / ft of that length, and TLE's own state; LeParams::cls / ctab are not used
struct TleParams : LeParams {
    const int32_t* rowptr;                                  // [Nk + 1]  ∂i, CSR
    const int32_t* cols;                                    // [rowptr[Nk]]
    const uint32_t* code;                                   // [2 Mr + 1][2 mn + 1]  class codes by (lfields1 + Mr, lfields2 + mn)
    int32_t* lf2;                                           // [R][N]  lfields2 by ABI site (live during rrrMC runs)
    uint16_t* wcls;                                         // [R][N]  DeltaECache.pos (a + L up), by ABI site
    double l2;                                              // 2λT
    double lT;                                              // λT = λ / β
    int mn;                                                 // Mr max|∂i|
};

__device__ __forceinline__ int tle_sigma(const uint32_t* sp, int x) { return 2 * sbit(sp, x) - 1; }

// class of a site with fields (lf1, lf2) and spin bit s.  The fields are clamped to the table (|lfields1| <= M and |lfields2| <= M max|∂i|
// hold for every configuration) and a pair without a level (never one the fields take) reads as class 0, so that a class is always one of
// the 2L the arrays are sized for; the debug check reports either.
__device__ __forceinline__ int tle_class(const TleParams& P, int lf1, int lf2, int s)
{
    lf1 = lf1 < -P.Mr ? -P.Mr : lf1 > P.Mr ? P.Mr : lf1;
    lf2 = lf2 < -P.mn ? -P.mn : lf2 > P.mn ? P.mn : lf2;
    const uint32_t c = P.code[(size_t)(lf1 + P.Mr) * (size_t)(2 * P.mn + 1) + (size_t)(lf2 + P.mn)];
    return c == kTleNoCode ? 0 : tle_class_of(c, P.L, s);
}

// lfields2 of replica site (i, k) from the slice-major spins
__device__ inline int tle_lf2_replica(const TleParams& P, const uint32_t* sp, int i, int k)
{
    const int Nk = P.Nk;
    int sum = 0;
    for (int p = P.rowptr[i]; p < P.rowptr[i + 1]; ++p) {
        const int i2 = P.cols[p];
        sum += tle_sigma(sp, i2) * tle_sigma(sp, k * Nk + i2);
    }
    return tle_sigma(sp, k * Nk + i) * tle_sigma(sp, i) * sum;
}

// energy(X::GraphTopologicalLocalEntropy, C) (TLE.jl:413-435: energy(X0) = n γT + r λT, then the M slices in k order; the centre's own
// energy is not part of it), μ, lfields2, the slice caches and, with `cache`, the DeltaECache (DeltaE.jl:74-103: sites pushed in ABI order),
// one workgroup per replica.
template <int SLICE>
__global__ __launch_bounds__(kReInitThreads) void tle_init_kernel(TleParams P, int cache)
{
    __shared__ long long s_n[kLeMmax + 1];
    __shared__ double s_E[kLeMmax + 1];
    __shared__ long long s_n0, s_r0;
    const int r = (int)blockIdx.x, tid = (int)threadIdx.x;
    const int N = P.N, Nk = P.Nk, rows = P.M, L = P.L;
    uint32_t* sp = P.sp + (size_t)r * P.W;
    int8_t* mu = P.mu + (size_t)r * Nk;
    int32_t* lf2 = P.lf2 + (size_t)r * N;
    const RrrView v = re_view(P, sp, r);
    for (int k = tid; k < rows; k += kReInitThreads) s_n[k] = 0;
    if (tid == 0) { s_n0 = 0; s_r0 = 0; }
    __syncthreads();
    for (int i = tid; i < Nk; i += kReInitThreads) {
        int m = 0;
        for (int k = 1; k < rows; ++k) m += tle_sigma(sp, k * Nk + i);
        mu[i] = (int8_t)m;
        atomicAdd(reinterpret_cast<unsigned long long*>(&s_n0), (unsigned long long)(long long)(-tle_sigma(sp, i) * m));
    }
    // the slices, as le_init_kernel builds them
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
        spf_init_rows(P, v, sp, 1, rows, s_E);
    } else if constexpr (SLICE == RE_SAT) {
        sat_init_rows(P.sat, sp, Nk, 1, rows, s_n);
    }
    // lfields2: the replica sites from the definition, a centre as the sum of its replicas'; r = -Σ_i lfields2(centre i) / 2 (TLE.jl:109-134)
    for (int x = Nk + tid; x < N; x += kReInitThreads) {
        const int k = x / Nk, i = x - k * Nk;
        lf2[i * rows + k] = tle_lf2_replica(P, sp, i, k);
    }
    __syncthreads();
    for (int i = tid; i < Nk; i += kReInitThreads) {
        int c = 0;
        for (int k = 1; k < rows; ++k) c += lf2[i * rows + k];
        lf2[i * rows] = c;
        atomicAdd(reinterpret_cast<unsigned long long*>(&s_r0), (unsigned long long)(long long)(-c));
    }
    __syncthreads();
    if (cache) {
        // classes in parallel; the sets are then filled by one thread in ABI site order, as push! in site order leaves them (the class count
        // has no bound that a per-thread scan in LDS could rely on)
        uint16_t* cls = P.wcls + (size_t)r * N;
        int32_t* st = P.st + (size_t)r * 2 * L;
        for (int j = tid; j < N; j += kReInitThreads) {
            const int i = j / rows, k = j - i * rows, s = sbit(sp, k * Nk + i), sc = tle_sigma(sp, i);
            cls[j] = (uint16_t)tle_class(P, k == 0 ? sc * mu[i] : sc * (2 * s - 1), lf2[j], s);
        }
        for (int k = tid; k < 2 * L; k += kReInitThreads) st[k] = 0;
        __syncthreads();
    }
    if (tid == 0) {
        long long rr = s_r0;
        rr /= 2;
        double E = (double)s_n0 * P.gT + (double)rr * P.lT;
        for (int k = 1; k < rows; ++k) {
            if constexpr (SLICE == RE_SK) { long long n = s_n[k]; n /= 2; E += (double)n / P.sN; }
            else if constexpr (SLICE == RE_SKN || SLICE == RE_SPF) E += s_E[k];
            else if constexpr (SLICE == RE_SAT) E += (double)s_n[k];
            else E += 0.0;
        }
        P.E_cur[r] = E;
        if (cache) {
            const uint16_t* cls = P.wcls + (size_t)r * N;
            uint16_t* spos = P.spos + (size_t)r * N;
            uint16_t* sv = P.sv + (size_t)r * 2 * L * N;
            int32_t* st = P.st + (size_t)r * 2 * L;
            for (int j = 0; j < N; ++j) {
                const int c = cls[j], p = st[c];
                sv[(size_t)c * N + p] = (uint16_t)j;
                spos[j] = (uint16_t)p;
                st[c] = p + 1;
            }
            double z = 0.0;
            for (int k = 0; k < 2 * L; ++k) {
                const double x = (double)st[k] * re_class_f(P.ft, L, k);
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

constexpr int kTleWave = 64;

// bytes of LDS of tle_rrr_kernel: the RRR draws of 64 iterations, and in the LDS build the replica's hot state behind them
__host__ __device__ inline size_t tle_rrr_lds_bytes(bool lds, int64_t N, int64_t W, int64_t Nk, int64_t L2)
{
    size_t b = (size_t)kTleWave * 8 * 4;
    if (lds) b += (size_t)L2 * 8 + (size_t)N * 4 + (size_t)L2 * 4 + (size_t)W * 4 + 2 * (((size_t)N * 2 + 3) & ~(size_t)3) + (((size_t)Nk + 3) & ~(size_t)3);
    return b;
}

// rrrMC(X::DoubleGraph) (src/RRRMC.jl:221-290) on the ensemble: one wavefront per replica, its 64 lanes working for the one chain.  Every
// lane holds the chain's scalars (z, E, acc_rate, the move) with identical values; lane 0 alone writes the chain's memory.
//
// rand_move (DeltaE.jl:146-167): cT += T[k] over the 2L classes is a sequential Float64 sum whose rounding the chain depends on.  The lanes
// ballot 64 entries at a time and only the non-zero ones are added, in ascending k: cT starts at +0.0 and x + (±0.0) == x for every x that
// can arise (a sum that is -0.0 only meets +0.0 comparisons), so skipping exact zeros leaves every comparison r < cT as it was.  Small
// non-zero residues of emptied classes are added, as the reference adds them; the tail `r < cT || while T[k] == 0` is the last non-zero entry.
//
// Neighbours (apply_move! / compute_staged!, DeltaE.jl:202-295): the lanes take the move's neighbours 64 at a time in the order of
// neighbors(X0, move) (tle_neighbor), each computing its neighbour's new lfields2 and class — these depend on the spins and on that
// neighbour's own old field only, not on the other neighbours.  A ballot selects those whose class changes, and they are retired in lane
// order: T[k0] -= f0; T[k1] += f1; z' += f1 - f0 and the ArraySet delete! / push!, all order-dependent, run as the reference runs them.
// The staged path runs the same two phases without writing; when the move is accepted the committing pass repeats them (same values, same
// order: the T and z' it leaves are the staged ones).
template <bool LDS, int SLICE>
__global__ __launch_bounds__(kTleWave) void tle_rrr_kernel(TleParams P)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t tle_lds[];
    const int r = (int)blockIdx.x, lane = (int)threadIdx.x;
    const int N = P.N, Nk = P.Nk, Mr = P.Mr, rows = P.M, L = P.L, L2 = 2 * P.L;
    uint32_t* const g_sp = P.sp + (size_t)r * P.W;
    int8_t* const g_mu = P.mu + (size_t)r * Nk;
    int32_t* const g_lf2 = P.lf2 + (size_t)r * N;
    uint16_t* const g_cls = P.wcls + (size_t)r * N;
    uint16_t* const g_spos = P.spos + (size_t)r * N;
    int32_t* const g_t = P.st + (size_t)r * L2;
    double* const g_T = P.T + (size_t)r * L2;
    uint16_t* const sv = P.sv + (size_t)r * L2 * N;
    uint32_t* sp = g_sp; int8_t* mu = g_mu; int32_t* lf2 = g_lf2; uint16_t* cls = g_cls; uint16_t* spos = g_spos; int32_t* t = g_t; double* T = g_T;
    uint32_t* const l_rng = tle_lds;                                               // [64][8]
    if constexpr (LDS) {
        double* l_T = reinterpret_cast<double*>(l_rng + kTleWave * 8);             // [2L]
        int32_t* l_lf2 = reinterpret_cast<int32_t*>(l_T + L2);                     // [N]
        int32_t* l_t = l_lf2 + N;                                                  // [2L]
        uint32_t* l_sp = reinterpret_cast<uint32_t*>(l_t + L2);                    // [W]
        uint16_t* l_spos = reinterpret_cast<uint16_t*>(l_sp + P.W);                // [N]
        uint16_t* l_cls = reinterpret_cast<uint16_t*>(reinterpret_cast<char*>(l_spos) + ((2 * N + 3) & ~3));   // [N]
        int8_t* l_mu = reinterpret_cast<int8_t*>(reinterpret_cast<char*>(l_cls) + ((2 * N + 3) & ~3));         // [Nk]
        for (int i = lane; i < L2; i += kTleWave) { l_T[i] = g_T[i]; l_t[i] = g_t[i]; }
        for (int i = lane; i < N; i += kTleWave) { l_lf2[i] = g_lf2[i]; l_spos[i] = g_spos[i]; l_cls[i] = g_cls[i]; }
        for (int i = lane; i < P.W; i += kTleWave) l_sp[i] = g_sp[i];
        for (int i = lane; i < Nk; i += kTleWave) l_mu[i] = g_mu[i];
        __syncthreads();
        sp = l_sp; mu = l_mu; lf2 = l_lf2; cls = l_cls; spos = l_spos; t = l_t; T = l_T;
    }
    const RrrView g_v = re_view(P, sp, r);
    RrrView v = g_v;
    if constexpr (LDS && SLICE == RE_SPF) {                                        // the rows' LocalFields behind the chain's own arrays, as in re_rrr_kernel
        if (P.spf_lds) spf_ens_attach(v, reinterpret_cast<char*>(tle_lds) + ((tle_rrr_lds_bytes(true, N, P.W, Nk, L2) + 7) & ~(size_t)7), rows);
    }
    const auto pv = re_slice_view<SLICE>(P, r);
    const uint32_t rep = P.replica0 + (uint32_t)r;
    const double* tab = P.tab;
    const double* ft = P.ft;
    double z = P.zz[r], E = P.E_cur[r], acc_rate = P.acc_rate[r];
    int64_t accepted = P.stats[(size_t)r * 2], staged_its = P.stats[(size_t)r * 2 + 1];
    int64_t ns = 0;
    long long next_sample = P.samp0;

    // ArraySet delete! / push! (ArraySets.jl:56-76), lane 0
    auto set_move = [&](int j, int k0, int k1) {
        const int p = spos[j];
        if (t[k0] <= 0) return;                                                    // (never: j is a member of k0; keeps every index in bounds)
        const int last = sv[(size_t)k0 * N + t[k0] - 1];
        sv[(size_t)k0 * N + p] = (uint16_t)last;
        spos[last] = (uint16_t)p;
        t[k0] -= 1;
        sv[(size_t)k1 * N + t[k1]] = (uint16_t)j;
        spos[j] = (uint16_t)t[k1];
        t[k1] += 1;
        cls[j] = (uint16_t)k1;
    };
    auto accept_c = [&](double c, double x, const uint32_t* q2) {                  // accept(c, x), RRRMC.jl:40-44
        bool ok = (c >= 1 && x >= 0);
        if (!ok) {
            const double a = c * det_exp(x);
            ok = a >= 1;
            if (!ok) ok = (double)((((uint64_t)q2[0] << 32) | q2[1]) >> 11) * 0x1.0p-53 < a;
        }
        return ok;
    };
    // One pass over the move (i, km) and its neighbours for the configuration in which the move's spin is sm (±1) and μ_i is mui; the
    // other sites are read from sp.  commit: apply_move! — the spin is flipped, the caches and the sets are updated; otherwise
    // compute_staged! + compute_reverse_probabilities!, nothing is written.  Returns z'.
    auto pass = [&](bool commit, int move, int i, int km, int sm, int mui) -> double {
        const int xm = km * Nk + i;
        const int lf2m = lf2[move];                                                // the move's old field
        const int32_t* ni = P.cols + P.rowptr[i];
        const int deg = P.rowptr[i + 1] - P.rowptr[i];
        const int nn = km == 0 ? Mr + rows * deg : 1 + 2 * deg;
        const int sci = km == 0 ? sm : tle_sigma(sp, i);                           // the centre of i in that configuration
        if (commit && lane == 0) {
            sflip(sp, xm);                                                         // spinflip!(X, C, move)
            if (km != 0) { mu[i] = (int8_t)mui; re_slice_update<SLICE>(v, xm); }   // (an undo takes the slice's swap path)
            lf2[move] = -lf2m;
        }
        double zp = z;
        auto retire = [&](int y, int k0, int k1) {
            const double f0 = re_class_f(ft, L, k0), f1 = re_class_f(ft, L, k1);
            if (commit && lane == 0) {
                T[k0] -= f0;
                T[k1] += f1;
                set_move(y, k0, k1);
            }
            zp += f1 - f0;
        };
        for (int q0 = 0; q0 < nn; q0 += kTleWave) {
            const int q = q0 + lane;
            int y = 0, k0 = 0, k1 = 0;
            if (q < nn) {
                y = tle_neighbor(Mr, ni, i, km, q);
                const int iy = y / rows, ky = y - iy * rows;
                const int old = lf2[y];
                int lf1, lfn, sy;
                if (km == 0) {
                    if (q < Mr) {                                                  // replica (i, ky): both fields change sign
                        sy = sbit(sp, ky * Nk + i);
                        lf1 = sci * (2 * sy - 1);
                        lfn = -old;
                    } else if (ky == 0) {                                          // the centre of i1 = iy
                        const int sc1 = tle_sigma(sp, iy);
                        int sum = 0;
                        for (int k = 1; k < rows; ++k) sum += tle_sigma(sp, k * Nk + i) * tle_sigma(sp, k * Nk + iy);
                        sy = (sc1 + 1) >> 1;
                        lf1 = sc1 * mu[iy];
                        lfn = old + 2 * sci * sc1 * sum;
                    } else {                                                       // (i1, ky)
                        const int sc1 = tle_sigma(sp, iy);
                        sy = sbit(sp, ky * Nk + iy);
                        lf1 = sc1 * (2 * sy - 1);
                        lfn = old + 2 * tle_sigma(sp, ky * Nk + i) * sci * (2 * sy - 1) * sc1;
                    }
                } else {
                    if (q == 0) {                                                  // the centre of i: the sum of its replicas' fields
                        sy = (sci + 1) >> 1;
                        lf1 = sci * mui;
                        lfn = old - 2 * lf2m;
                    } else {
                        const int sc1 = tle_sigma(sp, iy);
                        const int s1 = tle_sigma(sp, km * Nk + iy);
                        const int sg = sm * sci * s1 * sc1;
                        lfn = old + 2 * sg;
                        if (ky == 0) { sy = (sc1 + 1) >> 1; lf1 = sc1 * mu[iy]; }  // the centre of i1
                        else { sy = (s1 + 1) >> 1; lf1 = sc1 * s1; }               // (i1, km)
                    }
                }
                k0 = cls[y];
                k1 = tle_class(P, lf1, lfn, sy);
                if (commit) lf2[y] = lfn;
            }
            unsigned long long m = __ballot(q < nn && k0 != k1);
            while (m) {
                const int b = __ffsll((long long)m) - 1;
                m &= m - 1;
                retire(__shfl(y, b), __shfl(k0, b), __shfl(k1, b));
            }
        }
        { const int k0 = cls[move]; retire(move, k0, k0 >= L ? k0 - L : k0 + L); }
        if (commit) __syncthreads();
        return zp;
    };

    for (int64_t base = 0; base < P.iters; base += kTleWave) {
        __syncthreads();
        {
            const uint64_t gl = P.g0 + (uint64_t)(base + 1 + (int64_t)lane);
            const Philox4 a = philox4x32_10((uint32_t)gl, (uint32_t)(gl >> 32), rep, TAG_RRR, P.k0, P.k1);
            const Philox4 b = philox4x32_10((uint32_t)gl, (uint32_t)(gl >> 32), rep, TAG_RRR | (1u << 8), P.k0, P.k1);
            uint32_t* q = l_rng + lane * 8;
            q[0] = a.w[0]; q[1] = a.w[1]; q[2] = a.w[2]; q[3] = a.w[3]; q[4] = b.w[0]; q[5] = b.w[1]; q[6] = b.w[2]; q[7] = b.w[3];
        }
        __syncthreads();
        const int64_t it_end = base + kTleWave < P.iters ? base + kTleWave : P.iters;
        for (int64_t it = base + 1; it <= it_end; ++it) {
            if (it == next_sample) { next_sample += P.step; if (lane == 0) P.Es[ns * P.R + r] = E; ns += 1; }
            const uint32_t* q = l_rng + (it - base - 1) * 8;
            const uint32_t* q2 = q + 4;
            // rand_move
            const double rr = (double)((((uint64_t)q[0] << 32) | q[1]) >> 11) * 0x1.0p-53 * z;
            int k = -1, knz = -1;
            double cT = 0.0;
            for (int c0 = 0; c0 < L2 && k < 0; c0 += kTleWave) {
                const int kk = c0 + lane;
                const double tv = kk < L2 ? T[kk] : 0.0;
                unsigned long long m = __ballot(tv != 0.0);
                while (m) {
                    const int b = __ffsll((long long)m) - 1;
                    m &= m - 1;
                    cT += T[c0 + b];
                    knz = c0 + b;
                    if (rr < cT) { k = knz; break; }
                }
            }
            if (k < 0) k = knz < 0 ? 0 : knz;                                      // r < cT failed: the last class with T != 0
            const double dE0 = k < L ? -tab[k] : tab[k - L];
            const uint64_t uu = ((uint64_t)q[2] << 32) | q[3];
            int move = sv[(size_t)k * N + (size_t)mulhi64(uu, (uint64_t)t[k])];
            move = move < N ? move : N - 1;                                        // (a class emptied down to a rounding residue holds no site)
            const int i = move / rows, km = move - i * rows, xm = km * Nk + i;
            // delta_energy_residual (TLE.jl:460-469): 0.0 for the centre, the replica slice's delta_energy
            const double dE1 = km == 0 ? 0.0 : re_residual<SLICE, false>(v, pv, xm, km, i);
            const int sm_new = -tle_sigma(sp, xm);
            const int mu_new = km == 0 ? mu[i] : mu[i] + 2 * sm_new;
            __syncthreads();                                                       // every lane has read the state the move starts from

            bool acc = false;
            if (acc_rate < P.staged_thr) {
                // staged branch: step_rrr (RRRMC.jl:131-138)
                staged_its += 1;
                const double zp = pass(false, move, i, km, sm_new, mu_new);
                const double c = z / zp;
                if (accept_c(c, -P.beta * dE1, q2)) {
                    z = pass(true, move, i, km, sm_new, mu_new);                   // apply_staged!
                    E += dE0 + dE1;
                    accepted += 1;
                    acc = true;
                }
            } else {
                // direct branch: apply_move! (DeltaE.jl:232-295), undone by a second apply_move! on rejection
                const double zp = pass(true, move, i, km, sm_new, mu_new);
                const double cc = z / zp;
                z = zp;
                if (accept_c(cc, -P.beta * dE1, q2)) { E += dE0 + dE1; accepted += 1; acc = true; }
                else z = pass(true, move, i, km, -sm_new, km == 0 ? mu_new : mu_new - 2 * sm_new);
            }
            acc_rate = acc_rate * (1 - P.lambda) + (acc ? 1.0 : 0.0) * P.lambda;          // RRRMC.jl:281
        }
    }
    __syncthreads();
    if (lane == 0) {
        P.zz[r] = z; P.E_cur[r] = E; P.acc_rate[r] = acc_rate;
        P.stats[(size_t)r * 2] = accepted; P.stats[(size_t)r * 2 + 1] = staged_its;
    }
    if constexpr (LDS && SLICE == RE_SPF) {
        if (P.spf_lds) spf_ens_detach(v, g_v, rows);
    }
    if constexpr (LDS) {
        for (int i = lane; i < L2; i += kTleWave) { g_T[i] = T[i]; g_t[i] = t[i]; }
        for (int i = lane; i < N; i += kTleWave) { g_lf2[i] = lf2[i]; g_spos[i] = spos[i]; g_cls[i] = cls[i]; }
        for (int i = lane; i < P.W; i += kTleWave) g_sp[i] = sp[i];
        for (int i = lane; i < Nk; i += kTleWave) g_mu[i] = mu[i];
    }
}

// ΔE0 of ABI site (i, k) from the spins and μ: standardMC keeps no lfields2 (|∂i| spin reads per attempt, M |∂i| for a centre)
__device__ inline double tle_delta0_site(const TleParams& P, const uint32_t* sp, const int8_t* mu, int i, int k)
{
    const int sc = tle_sigma(sp, i);
    int lf1, l2 = 0;
    if (k == 0) {
        lf1 = sc * mu[i];
        for (int kk = 1; kk < P.M; ++kk) l2 += tle_lf2_replica(P, sp, i, kk);
    } else {
        lf1 = sc * tle_sigma(sp, k * P.Nk + i);
        l2 = tle_lf2_replica(P, sp, i, k);
    }
    return tle_delta0(P.g2, P.l2, lf1, l2);
}

// standardMC (src/RRRMC.jl:81-127): delta_energy = ΔE0 + delta_energy_residual (TLE.jl:471-474); LE's streams (SITE names ABI site j,
// rand() < exp(-β ΔE) on ACCEPT_F64).  E starts from E_cur (tle_init_kernel, or the run a resumed call continues).
template <int SLICE>
__global__ __launch_bounds__(kRrrThreads) void tle_standard_kernel(TleParams P)
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
        const double dE = tle_delta0_site(P, sp, mu, i, k) + (k == 0 ? 0.0 : re_residual<SLICE>(v, pv, x, k, i));
        const double xx = -P.beta * dE;
        const bool acc = (xx >= 0.0) || (rand53(P.k0, P.k1, g, rep) < det_exp(xx));          // RRRMC.jl:39
        if (acc) {
            const int sg = tle_sigma(sp, x);
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

// debug mode (rrrmc_set_debug_checks): after a sampler call every replica's energy(X, C) is recomputed from its configuration and compared
// with the tracked E (LE's bound); μ, and after rrrMC every site's lfields2, class, membership and the set sizes must equal what the
// configuration gives (each site sits at its position inside its class's size, and the sizes add up to N: the sets are then exactly the
// classes); GraphSKNormal slices: the cached fields within 1e-10 Nk of recomputed ones.
template <int SLICE>
__global__ __launch_bounds__(64) void tle_check_kernel(TleParams P, int cache)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= P.R) return;
    const int Nk = P.Nk, rows = P.M, L = P.L, N = P.N;
    const uint32_t* sp = P.sp + (size_t)r * P.W;
    const int8_t* mu = P.mu + (size_t)r * Nk;
    const RrrView v = re_view(P, P.sp + (size_t)r * P.W, r);
    bool bad = false;
    long long n0 = 0, r0 = 0;
    for (int i = 0; i < Nk; ++i) {
        int m = 0, c = 0;
        for (int k = 1; k < rows; ++k) {
            m += tle_sigma(sp, k * Nk + i);
            const int f = tle_lf2_replica(P, sp, i, k);
            c += f;
            if (cache) bad = bad || f != P.lf2[(size_t)r * N + i * rows + k];
        }
        if (cache) bad = bad || c != P.lf2[(size_t)r * N + i * rows];
        bad = bad || m != mu[i];
        n0 -= tle_sigma(sp, i) * m;
        r0 -= c;
    }
    r0 /= 2;
    double E = (double)n0 * P.gT + (double)r0 * P.lT;
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
    if (cache) {
        long long tot = 0;
        for (int k = 0; k < 2 * L; ++k) { const int c = P.st[(size_t)r * 2 * L + k]; bad = bad || c < 0 || c > N; tot += c; }
        bad = bad || tot != N;
        for (int j = 0; j < N && !bad; ++j) {
            const int i = j / rows, k = j - i * rows, s = sbit(sp, k * Nk + i), sc = tle_sigma(sp, i);
            const int c = tle_class(P, k == 0 ? sc * mu[i] : sc * (2 * s - 1), P.lf2[(size_t)r * N + j], s);
            const int p = P.spos[(size_t)r * N + j];
            bad = bad || c != P.wcls[(size_t)r * N + j] || p >= P.st[(size_t)r * 2 * L + c] || P.sv[((size_t)r * 2 * L + c) * N + p] != j;
        }
    }
    if (bad) { atomicAdd(&P.flag[0], 1); P.flag[1] = r; }
}

}  // namespace rrrmc
