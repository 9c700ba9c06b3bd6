// gfx950 kernels for GraphMixed (src/graphs/Mixed.jl:15-61): two to seven graphs on one set of N spins,
//   energy(X, C)          = sum(energy(x, C) for x in graphs)            (:33-36)
//   delta_energy(X, C, i) = sum(delta_energy(x, C, i) for x in graphs)   (:38-40)
//   update_cache!(X, C, i) on every component                           (:42-47)
// Julia's sum over a generator folds from the left, ((d1 + d2) + d3) ..., so the order of the list is part of the model.  Every
// component is one of the slice kinds of re_kernels.hpp used as ONE slice (M = 1), in the buffers its kind has in ReParams; a context holds
// one upload of each storage group (mixed_models.hpp), so the kinds of a list share one RrrView and one view per pattern family.
//
// The list (MixedList: n, kind[7]) is a kernel argument, the same for every chain of a launch: the switch over kind[c] is wave-uniform and
// no kernel is instantiated per combination.  DESIGN §4v.
//
// Two forms of every device function.  WAVE = false: one thread runs the chain.  WAVE = true: the 64 lanes of a one-wavefront workgroup
// call it with identical arguments and get identical values; the pattern machines spread their patterns over the lanes
// (perc_update / comm_update / xentr_*<.., true>), the kinds whose update is written for one thread run it on lane 0.
//
// Included by af_kernels.hpp behind AfParams, which the kernels below take: the wrappers' af_init / af_standard / af_check with the mix in
// place of the one slice (the stand-alone GraphMixed runs as sub = 1, where the fields are never read), and mixed_wave_kernel, standardMC
// with one wavefront per chain.  rrrMC is af_rrr_kernel<RE_MIXED, LDS> (af_kernels.hpp) with the hooks of this file.
#pragma once

namespace rrrmc {

struct MixedViews { PercView pv; XentrView xv; CommView cv; SatTable sat; };

__device__ __forceinline__ MixedViews mixed_views(const ReParams& P, const MixedList& L, int r)
{
    MixedViews V{};
    V.sat = P.sat;
    for (int c = 0; c < L.n; ++c) {
        switch (L.kind[c]) {
            case RE_PSTEP: case RE_PLIN: V.pv = perc_view(P.pc, r); break;
            case RE_PXE: V.xv = xentr_view(P.pc, P.xe, r); break;
            case RE_CSTEP: V.cv = comm_view<CK_STEP>(P.cm, r); break;
            case RE_CRELU: V.cv = comm_view<CK_RELU>(P.cm, r); break;
            case RE_CQU: V.cv = comm_view<CK_QU>(P.cm, r); break;
            default: break;
        }
    }
    return V;
}

// delta_energy(graphs[c], C, i) at the current configuration
template <bool WAVE>
__device__ __forceinline__ double mixed_component_residual(int kind, const RrrView& v, const MixedViews& V, int i)
{
    switch (kind) {
        case RE_SK: return re_residual<RE_SK>(v, i, 0, i);
        case RE_SKN: return re_residual<RE_SKN>(v, i, 0, i);
        case RE_SPF: return re_residual<RE_SPF>(v, i, 0, i);
        case RE_PSTEP: return re_residual<RE_PSTEP, WAVE>(v, V.pv, i, 0, i);
        case RE_PLIN: return re_residual<RE_PLIN, WAVE>(v, V.pv, i, 0, i);
        case RE_PXE: return re_residual<RE_PXE, WAVE>(v, V.xv, i, 0, i);
        case RE_CSTEP: return re_residual<RE_CSTEP, WAVE>(v, V.cv, i, 0, i);
        case RE_CRELU: return re_residual<RE_CRELU, WAVE>(v, V.cv, i, 0, i);
        case RE_CQU: return re_residual<RE_CQU, WAVE>(v, V.cv, i, 0, i);
        case RE_SAT: return re_residual<RE_SAT, WAVE>(v, V.sat, i, 0, i);
        default: return 0.0;                                // GraphEmpty
    }
}
// delta_energy(X, C, i): the fold from the left over the list
template <bool WAVE>
__device__ __forceinline__ double mixed_residual(const MixedList& L, const RrrView& v, const MixedViews& V, int i)
{
    double d = mixed_component_residual<WAVE>(L.kind[0], v, V, i);
    for (int c = 1; c < L.n; ++c) d = d + mixed_component_residual<WAVE>(L.kind[c], v, V, i);
    return d;
}
// update_cache! of the components that keep an undo record and so follow every flip, the undo flip of a rejected rrrMC move included
// (GraphSKNormal's swap, the sparse Float64 graphs' record); called after the bit flip
template <bool WAVE>
__device__ __forceinline__ void mixed_update_follow(const MixedList& L, const RrrView& v, int i)
{
    for (int c = 0; c < L.n; ++c) {
        const int kind = L.kind[c];
        if (kind != RE_SKN && kind != RE_SPF) continue;
        if constexpr (WAVE) __syncthreads();
        if (!WAVE || threadIdx.x == 0) {
            if (kind == RE_SKN) skn_update(v, i);
            else spf_slice_update(v, i);
        }
        if constexpr (WAVE) __syncthreads();
    }
}
// update_cache! of the components whose state is a pure function of the configuration (the pattern machines): once per accepted move,
// after the bit flip.  Binary SK and K-SAT keep no state.
template <bool WAVE>
__device__ __forceinline__ void mixed_update_pure(const MixedList& L, const RrrView& v, const MixedViews& V, int i)
{
    for (int c = 0; c < L.n; ++c) {
        switch (L.kind[c]) {
            case RE_PSTEP: re_slice_update<RE_PSTEP, WAVE>(v, V.pv, i, 0, i); break;
            case RE_PLIN: re_slice_update<RE_PLIN, WAVE>(v, V.pv, i, 0, i); break;
            case RE_PXE: re_slice_update<RE_PXE, WAVE>(v, V.xv, i, 0, i); break;
            case RE_CSTEP: re_slice_update<RE_CSTEP, WAVE>(v, V.cv, i, 0, i); break;
            case RE_CRELU: re_slice_update<RE_CRELU, WAVE>(v, V.cv, i, 0, i); break;
            case RE_CQU: re_slice_update<RE_CQU, WAVE>(v, V.cv, i, 0, i); break;
            default: break;
        }
    }
}
// energy(graphs[c], C) from the configuration only, sequential
__device__ inline double mixed_component_energy(int kind, const ReParams& P, const RrrView& v)
{
    switch (kind) {
        case RE_SK: return re_slice_energy<RE_SK>(P, v, 0);
        case RE_SKN: return re_slice_energy<RE_SKN>(P, v, 0);
        case RE_SPF: return re_slice_energy<RE_SPF>(P, v, 0);
        case RE_PSTEP: return re_slice_energy<RE_PSTEP>(P, v, 0);
        case RE_PLIN: return re_slice_energy<RE_PLIN>(P, v, 0);
        case RE_PXE: return re_slice_energy<RE_PXE>(P, v, 0);
        case RE_CSTEP: return re_slice_energy<RE_CSTEP>(P, v, 0);
        case RE_CRELU: return re_slice_energy<RE_CRELU>(P, v, 0);
        case RE_CQU: return re_slice_energy<RE_CQU>(P, v, 0);
        case RE_SAT: return re_slice_energy<RE_SAT>(P, v, 0);
        default: return 0.0;
    }
}
// energy(X, C): the fold from the left
__device__ inline double mixed_energy(const MixedList& L, const ReParams& P, const RrrView& v)
{
    double E = mixed_component_energy(L.kind[0], P, v);
    for (int c = 1; c < L.n; ++c) E = E + mixed_component_energy(L.kind[c], P, v);
    return E;
}
// debug mode: every component's cache held as its own family's check holds it
__device__ inline bool mixed_state_bad(const MixedList& L, const ReParams& P, const RrrView& v, const uint32_t* sp, int r)
{
    const int N = P.N;
    bool bad = false;
    for (int c = 0; c < L.n; ++c) {
        switch (L.kind[c]) {
            case RE_SKN:
                for (int i = 0; i < N; ++i) {
                    const int si = sbit(sp, i);
                    const double* Ji = P.Jd + (size_t)i * N;
                    double lf = 0.0;
                    for (int j = 0; j < N; ++j) lf += (double)(1 - 2 * (si ^ sbit(sp, j))) * Ji[j];
                    const double dd = v.slf[(size_t)v.scur[0] * N + i] - 2 * lf;
                    bad = bad || !(dd <= 1e-10 * N && dd >= -1e-10 * N);
                }
                break;
            case RE_SPF: bad = bad || spf_state_bad(P, v, sp, 0, 1); break;
            case RE_PSTEP: bad = bad || perc_state_bad<false>(P.pc, perc_view(P.pc, r), sp, 0, N, N); break;
            case RE_PLIN: bad = bad || perc_state_bad<true>(P.pc, perc_view(P.pc, r), sp, 0, N, N); break;
            case RE_PXE: bad = bad || xentr_state_bad(P.pc, P.xe, P.pc.ds + (size_t)r * 64 * P.pc.PW, 1, sp, N); break;
            case RE_CSTEP: bad = bad || comm_state_bad<CK_STEP>(P.cm, comm_view<CK_STEP>(P.cm, r), sp, 0, N, N); break;
            case RE_CRELU: bad = bad || comm_state_bad<CK_RELU>(P.cm, comm_view<CK_RELU>(P.cm, r), sp, 0, N, N); break;
            case RE_CQU: bad = bad || comm_state_bad<CK_QU>(P.cm, comm_view<CK_QU>(P.cm, r), sp, 0, N, N); break;
            default: break;
        }
    }
    return bad;
}

// The start of a reference call (src/RRRMC.jl:95, :237-240): every component's cache, E = energy(X, C) with each component's energy made
// as its own family makes it (af_init_kernel, re_init_kernel) and, with `cache`, DeltaECacheCont(X0, C, β) as af_init_kernel builds it.
// One workgroup per chain.
__global__ __launch_bounds__(kAfInitThreads) void mixed_init_kernel(AfParams A, int cache)
{
    __shared__ long long s_n[kMixedMax];
    __shared__ double s_E[kMixedMax];
    __shared__ double s_t[kPercPmax];
    const ReParams& P = A.re;
    const MixedList& L = A.mx;
    const int r = (int)blockIdx.x, tid = (int)threadIdx.x;
    const int N = P.N;
    uint32_t* sp = P.sp + (size_t)r * P.W;
    const RrrView v = re_view(P, sp, r);
    if (tid < kMixedMax) { s_n[tid] = 0; s_E[tid] = 0.0; }
    __syncthreads();
    for (int c = 0; c < L.n; ++c) {
        switch (L.kind[c]) {
            case RE_SK:
                for (int x = tid; x < N; x += kAfInitThreads)
                    atomicAdd(reinterpret_cast<unsigned long long*>(&s_n[c]), (unsigned long long)(long long)(-(slice_delta(v, x) / 2)));
                break;
            case RE_SKN:                                    // SK.jl:212-237: lfields = 2 lf, lfields_last = 0, move_last = none
                for (int i = tid; i < N; i += kAfInitThreads) {
                    const double* Ji = P.Jd + (size_t)i * N;
                    const int si = sbit(sp, i);
                    double lf = 0.0;
                    for (int j = 0; j < N; ++j) lf += (double)(1 - 2 * (si ^ sbit(sp, j))) * Ji[j];
                    v.slf[i] = 2 * lf;
                    v.slf[(size_t)N + i] = lf;
                }
                __syncthreads();
                if (tid == 0) {
                    double n = 0.0;
                    for (int i = 0; i < N; ++i) n -= v.slf[(size_t)N + i];
                    n /= 2;
                    s_E[c] = n;
                    v.smv[0] = -1;
                    v.scur[0] = 0;
                }
                __syncthreads();
                for (int i = tid; i < N; i += kAfInitThreads) v.slf[(size_t)N + i] = 0.0;
                break;
            case RE_SPF: spf_init_rows(P, v, sp, 0, 1, s_E + c); break;
            case RE_PSTEP: perc_init_rows<false>(P.pc, perc_view(P.pc, r), sp, N, N, s_n + c); break;
            case RE_PLIN: perc_init_rows<true>(P.pc, perc_view(P.pc, r), sp, N, N, s_n + c); break;
            case RE_PXE: {
                const double Eg = xentr_init_chain(P.pc, P.xe, P.pc.ds + (size_t)r * 64 * P.pc.PW, 1, sp, N, s_t);
                if (tid == 0) s_E[c] = Eg;
                break;
            }
            case RE_CSTEP: comm_init_rows<CK_STEP>(P.cm, comm_view<CK_STEP>(P.cm, r), sp, N, N, s_n + c); break;
            case RE_CRELU: comm_init_rows<CK_RELU>(P.cm, comm_view<CK_RELU>(P.cm, r), sp, N, N, s_n + c); break;
            case RE_CQU: comm_init_rows<CK_QU>(P.cm, comm_view<CK_QU>(P.cm, r), sp, N, N, s_n + c); break;
            case RE_SAT: sat_init_rows(P.sat, sp, N, 0, 1, s_n + c); break;
            default: break;
        }
        __syncthreads();
    }
    if (cache) {
        double* dEs = A.dEs + (size_t)r * N;
        double* w = A.v + (size_t)r * A.N2;
        double* ps = A.ps + (size_t)r * A.N2;
        for (int i = tid; i < A.N2; i += kAfInitThreads) {
            double x = 0.0;
            if (i < N) {
                const double d = af_delta0(A.h, i, sbit(sp, i));
                dEs[i] = d;
                x = prior_of(P.beta * d);
            }
            w[i] = x;
        }
        __syncthreads();
        // refresh!: node (lev, k) = the sum of the elements of its left subtree, ascending, from 0.0
        const int levs = A.levs;
        for (int n = tid; n < A.N2 - 1; n += kAfInitThreads) {
            const int lev = 31 - __builtin_clz((unsigned)n + 1u), k = n + 1 - (1 << lev), half = 1 << (levs - 1 - lev), i0 = k << (levs - lev);
            double acc = 0.0;
            for (int e = 0; e < half; ++e) { const int i = i0 + e; if (i < N) acc += w[i]; }
            ps[n] = acc;
        }
        if (tid == 0) ps[A.N2 - 1] = 0.0;
    }
    if (tid == 0) {
        double E0 = 0.0;
        if (!A.sub)
            for (int i = 0; i < N; ++i) E0 += A.h[i] * (double)(2 * sbit(sp, i) - 1);          // AddFields.jl:33-43
        double Eg = 0.0;
        for (int c = 0; c < L.n; ++c) {
            const int kind = L.kind[c];
            double Ec;
            if (kind == RE_SK) Ec = af_g_energy<RE_SK>(P, s_n[c], 0.0);
            else if (kind == RE_PSTEP) Ec = af_g_energy<RE_PSTEP>(P, s_n[c], 0.0);
            else if (kind == RE_PLIN) Ec = af_g_energy<RE_PLIN>(P, s_n[c], 0.0);
            else if (kind == RE_CSTEP || kind == RE_CRELU || kind == RE_CQU || kind == RE_SAT) Ec = (double)s_n[c];
            else Ec = s_E[c];                               // GraphSKNormal, sparse Float64, GraphPercXEntr; 0 for GraphEmpty
            Eg = c == 0 ? Ec : Eg + Ec;
        }
        P.E_cur[r] = A.sub ? Eg : E0 + Eg;                  // AddFields.jl:81, :117
        if (cache) {
            const double* w = A.v + (size_t)r * A.N2;
            double z = 0.0;
            for (int i = 0; i < N; ++i) z += w[i];
            P.zz[r] = z;
            P.acc_rate[r] = 0.5;
            A.tref[r] = 0;
        }
        P.stats[(size_t)r * 2] = 0;
        P.stats[(size_t)r * 2 + 1] = 0;
    }
}

// standardMC (src/RRRMC.jl:81-127), one thread per chain: af_standard_kernel with the mix in place of the one slice
__global__ __launch_bounds__(kRrrThreads) void mixed_standard_kernel(AfParams A)
{
    const ReParams& P = A.re;
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= P.R) return;
    uint32_t* sp = P.sp + (size_t)r * P.W;
    const RrrView v = re_view(P, sp, r);
    const MixedViews V = mixed_views(P, A.mx, r);
    const uint32_t rep = P.replica0 + (uint32_t)r;
    double E = P.E_cur[r];
    int64_t accepted = 0, ns = 0;
    long long next_sample = P.samp0;
    for (int64_t it = 1; it <= P.iters; ++it) {
        if (it == next_sample) { next_sample += P.step; P.Es[ns * P.R + r] = E; ns += 1; }
        const uint64_t g = P.g0 + (uint64_t)it;
        const int i = (int)site_of(P.k0, P.k1, g, (uint32_t)P.N);
        const double dg = mixed_residual<false>(A.mx, v, V, i);
        const double dE = A.sub ? dg : af_delta0(A.h, i, sbit(sp, i)) + dg;
        const double xx = -P.beta * dE;
        const bool acc = (xx >= 0.0) || (rand53(P.k0, P.k1, g, rep) < det_exp(xx));          // RRRMC.jl:39
        if (acc) {
            sflip(sp, i);
            mixed_update_follow<false>(A.mx, v, i);
            mixed_update_pure<false>(A.mx, v, V, i);
            E += dE;
            accepted += 1;
        }
    }
    P.E_cur[r] = E;
    P.stats[(size_t)r * 2] = accepted; P.stats[(size_t)r * 2 + 1] = 0;
}

// the sum of an integer over the wavefront, in every lane
__device__ __forceinline__ int mixed_wave_sum(int x)
{
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) x += __shfl_xor(x, s, 64);
    return x;
}

// LDS of mixed_wave_kernel: the term buffer of a GraphPercXEntr component (16-byte aligned, first), then the spins
__host__ __device__ inline size_t mixed_wave_lds_bytes(int64_t W, int64_t xe_PW) { return (size_t)xe_PW * 64 * 8 + (size_t)W * 4; }

// standardMC, one wavefront (one workgroup of 64) per chain: the shape of sat_wave_kernel.  The spins live in LDS for the call; the 64
// lanes draw the sites and the uniforms of 64 iterations at once (the streams of the thread build: site_of, rand53); the chain then runs
// on wave-uniform values, E and the accepted count included, and lane 0 stores.  Per iteration the components are evaluated by the
// wavefront:
//   K-SAT           one occurrence per lane, ΔE by ballot, in passes of 64 (sat_wave_kernel's loop);
//   binary SK       one 32-bit word of row i of J per lane, popcounts summed over the wavefront (integers: any order);
//   the perceptrons, committee machines, GraphPercXEntr   their wavefront forms (one pattern per lane; GraphPercXEntr's terms are added
//                   in pattern order by every lane, from the term buffer in LDS);
//   GraphSKNormal   the field read; on acceptance skn_update's loop strided over the lanes.  It is element-wise (lf[j], ll[j] depend on
//                   entry j alone), so every entry gets skn_update's value, the move_last swap included;
//   sparse Float64  the field read; update_cache! (K <= 8 neighbours, the run of a repeated neighbour in order) on lane 0.
// The Float64 additions are the thread build's in the thread build's order: the two builds give the same bits.
__global__ __launch_bounds__(64) void mixed_wave_kernel(AfParams A, int xe_PW)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char mx_lds[];
    __shared__ int l_site[64];
    __shared__ double l_u[64];
    const ReParams& P = A.re;
    const MixedList& L = A.mx;
    const int r = (int)blockIdx.x, lane = (int)threadIdx.x;
    const int N = P.N, W = P.W;
    double* const l_term = reinterpret_cast<double*>(mx_lds);                      // [64 xe_PW]
    uint32_t* const l_sp = reinterpret_cast<uint32_t*>(l_term + (size_t)64 * xe_PW);       // [W]
    uint32_t* const g_sp = P.sp + (size_t)r * W;
    for (int w = lane; w < W; w += 64) l_sp[w] = g_sp[w];
    const RrrView v = re_view(P, l_sp, r);
    MixedViews V = mixed_views(P, L, r);
    V.xv.term = l_term;
    const SatLdsBits bits{l_sp};
    const uint32_t rep = P.replica0 + (uint32_t)r;
    double E = P.E_cur[r];
    int64_t accepted = 0, ns = 0;
    long long next_sample = P.samp0;
    for (int64_t base = 0; base < P.iters; base += 64) {
        __syncthreads();
        {
            const uint64_t gl = P.g0 + (uint64_t)(base + 1 + lane);
            l_site[lane] = (int)site_of(P.k0, P.k1, gl, (uint32_t)N);
            l_u[lane] = rand53(P.k0, P.k1, gl, rep);
        }
        __syncthreads();
        const int64_t it_end = base + 64 < P.iters ? base + 64 : P.iters;
        for (int64_t it = base + 1; it <= it_end; ++it) {
            if (it == next_sample) { next_sample += P.step; if (lane == 0) P.Es[ns * P.R + r] = E; ns += 1; }
            const int i = l_site[it - base - 1];
            const int si = sbit(l_sp, i);
            double dg = 0.0;
            for (int c = 0; c < L.n; ++c) {
                double dc;
                switch (L.kind[c]) {
                    case RE_SAT: {
                        const uint32_t e0 = P.sat.off[i], e1 = P.sat.off[i + 1];
                        int d = 0;
                        for (uint32_t eb = e0; eb < e1; eb += 64) {
                            const uint32_t e = eb + (uint32_t)lane;
                            int term = 0;
                            if (e < e1) { const SatEntry en = P.sat.ent[e]; term = sat_entry_term(en, si, bits); }
                            d += __popcll(__ballot(term > 0)) - __popcll(__ballot(term < 0));
                        }
                        dc = (double)d;
                        break;
                    }
                    case RE_SK: {                           // slice_delta with M = 1: the row's words over the lanes
                        const uint32_t* Ji = P.Jb + (size_t)i * P.Wk;
                        int sc = 0;
                        for (int w = lane; 32 * w < N; w += 64) {
                            uint32_t b = l_sp[w];
                            const int rem = N - 32 * w;
                            if (rem < 32) b &= (1u << rem) - 1u;
                            sc += __popc(b ^ Ji[w]);
                        }
                        sc = mixed_wave_sum(sc);
                        dc = (double)(2 * (2 * si - 1) * (N - 1 - 2 * (sc - si))) / P.sN;
                        break;
                    }
                    default: dc = mixed_component_residual<true>(L.kind[c], v, V, i); break;
                }
                dg = c == 0 ? dc : dg + dc;
            }
            const double dE = A.sub ? dg : af_delta0(A.h, i, si) + dg;
            const double xx = -P.beta * dE;
            const bool acc = (xx >= 0.0) || (l_u[it - base - 1] < det_exp(xx));                  // RRRMC.jl:39
            if (acc) {
                __syncthreads();                            // (one wavefront) every lane has read the bits of this iteration
                if (lane == 0) l_sp[i >> 5] ^= 1u << (i & 31);
                __syncthreads();
                for (int c = 0; c < L.n; ++c) {
                    if (L.kind[c] == RE_SKN) {              // skn_update (SK.jl:239-276), M = 1
                        const int cur = v.scur[0];
                        const bool swap = v.smv[0] == i;
                        double* lf = v.slf + (size_t)cur * N;
                        double* ll = v.slf + (size_t)(cur ^ 1) * N;
                        const double lfm = lf[i];
                        __syncthreads();                    // every lane has read scur, move_last and lf[i]
                        if (swap) {
                            if (lane == 0) v.scur[0] = (uint8_t)(cur ^ 1);
                        } else {
                            const double* Ji = P.Jd + (size_t)i * N;
                            const int snew = si ^ 1;
                            for (int j = lane; j < N; j += 64) {
                                if (j == i) continue;       // (J_ii = 0, and entry i is set below)
                                const double Jsij = (double)(1 - 2 * (snew ^ sbit(l_sp, j))) * Ji[j];
                                const double lfj = lf[j];
                                ll[j] = lfj;
                                lf[j] = lfj + 4 * Jsij;
                            }
                            if (lane == 0) { ll[i] = lfm; lf[i] = -lfm; v.smv[0] = i; }
                        }
                        __syncthreads();
                    } else if (L.kind[c] == RE_SPF) {
                        if (lane == 0) spf_slice_update(v, i);
                        __syncthreads();
                    }
                }
                mixed_update_pure<true>(L, v, V, i);
                E += dE;
                accepted += 1;
            }
        }
    }
    __syncthreads();
    for (int w = lane; w < W; w += 64) g_sp[w] = l_sp[w];
    if (lane == 0) {
        P.E_cur[r] = E;
        P.stats[(size_t)r * 2] = accepted; P.stats[(size_t)r * 2 + 1] = 0;
    }
}

// debug mode (rrrmc_set_debug_checks): af_check_kernel with the mix in place of the one slice — the tracked E within 1e-10 of a fresh
// energy(X, C), every component's own state check, and after rrrMC ΔEs and the weights equal to their definitions bit for bit
__global__ __launch_bounds__(64) void mixed_check_kernel(AfParams A, int cache)
{
    const ReParams& P = A.re;
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= P.R) return;
    const int N = P.N;
    const uint32_t* sp = P.sp + (size_t)r * P.W;
    const RrrView v = re_view(P, P.sp + (size_t)r * P.W, r);
    bool bad = false;
    double E0 = 0.0;
    if (!A.sub)
        for (int i = 0; i < N; ++i) E0 += A.h[i] * (double)(2 * sbit(sp, i) - 1);
    const double Eg = mixed_energy(A.mx, P, v);
    const double E = A.sub ? Eg : E0 + Eg;
    const double d = E - P.E_cur[r], tol = 1e-10 * (E < -1.0 ? -E : E > 1.0 ? E : 1.0);          // relative once |E| > 1, as af_check_kernel
    bad = bad || !(d <= tol && d >= -tol);
    bad = bad || mixed_state_bad(A.mx, P, v, sp, r);
    if (cache) {
        const double* dEs = A.dEs + (size_t)r * N;
        const double* w = A.v + (size_t)r * A.N2;
        for (int i = 0; i < N; ++i) {
            const double de = af_delta0(A.h, i, sbit(sp, i));
            bad = bad || !(dEs[i] == de) || !(w[i] == prior_of(P.beta * de));
        }
        for (int i = N; i < A.N2; ++i) bad = bad || !(w[i] == 0.0);
    }
    if (bad) { atomicAdd(&P.flag[0], 1); P.flag[1] = r; }
}

// rrrmc_mixed_energies: energy(graphs[c], C) of every component of every chain, one thread per (chain, component); reads the configuration only
__global__ __launch_bounds__(64) void mixed_energies_kernel(AfParams A, double* out)
{
    const ReParams& P = A.re;
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= P.R * A.mx.n) return;
    const int r = e / A.mx.n, c = e - r * A.mx.n;
    const RrrView v = re_view(P, P.sp + (size_t)r * P.W, r);
    out[e] = mixed_component_energy(A.mx.kind[c], P, v);
}

}  // namespace rrrmc
