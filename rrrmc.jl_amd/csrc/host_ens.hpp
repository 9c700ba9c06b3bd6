// Host code that the three ensembles share (GraphRobustEnsemble, GraphLocalEntropy, GraphTopologicalLocalEntropy): the slice dispatcher, context
// creation and the frame of a sampler call.  Included by rrrmc_hip.hip inside its anonymous namespace, after the context struct and the common
// helpers (fail, HIP_TRY, dev_alloc / dev_free, dbg_flag_ensure, smp_begin) and before host_re.hpp / host_le.hpp / host_tle.hpp, which keep what differs:
// their tables, *_params, *_run_init, the build choice and the launch.  Not a stand-alone translation unit.
//
// The model <-> (ensemble, slice kind) relation is the table of ens_models.hpp.  ens_slice(model) selects the kernels' SLICE template
// argument directly: enum ReSlice (re_kernels.hpp) and rrrmc_re_slice (the ABI) are the same numbers.
static_assert((int)RE_EMPTY == RRRMC_RE_SLICE_EMPTY && (int)RE_SK == RRRMC_RE_SLICE_SK && (int)RE_SKN == RRRMC_RE_SLICE_SKN, "ReSlice is rrrmc_re_slice");
static_assert((int)RE_PSTEP == RRRMC_RE_SLICE_PERC_STEP && (int)RE_PLIN == RRRMC_RE_SLICE_PERC_LINEAR, "ReSlice is rrrmc_re_slice");
static_assert((int)RE_CSTEP == RRRMC_RE_SLICE_COMM_STEP && (int)RE_CRELU == RRRMC_RE_SLICE_COMM_RELU && (int)RE_CQU == RRRMC_RE_SLICE_COMM_QU, "ReSlice is rrrmc_re_slice");
static_assert((int)RE_SAT == RRRMC_RE_SLICE_SAT && (int)RE_SPF == RRRMC_RE_SLICE_SPARSE_F64, "ReSlice is rrrmc_re_slice");

// with_slice(Set{}, slice, f) calls f(std::integral_constant<int, S>{}) for the S of the set that equals `slice`, so that a generic lambda can
// launch kernel<decltype(s)::value>; false when the set has no such S (the table makes that unreachable: callers fail with ens_bad_slice).
// A kernel template is built once per member of the set it is dispatched over: the TLE kernels over TleSlices, all others over AllSlices.
template <int... S> struct SliceSet {};
using AllSlices = SliceSet<RE_EMPTY, RE_SK, RE_SKN, RE_PSTEP, RE_PLIN, RE_CSTEP, RE_CRELU, RE_SAT, RE_CQU, RE_SPF>;
using TleSlices = SliceSet<RE_EMPTY, RE_SK, RE_SKN, RE_SAT, RE_SPF>;
template <int... S, typename F> bool with_slice(SliceSet<S...>, int slice, F&& f)
{
    return ((slice == S && (f(std::integral_constant<int, S>{}), true)) || ...);
}
int32_t ens_bad_slice(rrrmc_ctx* ctx) { return fail(ctx, RRRMC_ERR_STATE, "internal error: model %d has no kernels for slice kind %d", ctx->model, ens_slice(ctx->model)); }

inline bool is_re(const rrrmc_ctx* ctx) { return ens_family(ctx->model) == ENS_RE; }
inline bool is_le(const rrrmc_ctx* ctx) { return ens_family(ctx->model) == ENS_LE; }
inline bool is_tle(const rrrmc_ctx* ctx) { return ens_family(ctx->model) == ENS_TLE; }
inline int re_levels(int64_t M) { return (int)((M + 1) / 2); }          // allΔE(GraphRE): ceil(M / 2) values (RE.jl:208-213)
inline int le_levels(int64_t M) { return (int)(M % 2 == 0 ? M / 2 + 2 : (M + 1) / 2); }        // length of allΔE(GraphLE) (LE.jl:176-179)

inline const char* ens_graph_name(const rrrmc_ctx* ctx)
{
    return is_re(ctx) ? "GraphRobustEnsemble" : is_le(ctx) ? "GraphLocalEntropy" : "GraphTopologicalLocalEntropy";
}
// bklMC, wtmMC and extremal_opt on an ensemble
int32_t ens_not_wired(rrrmc_ctx* ctx, const char* sampler)
{
    return fail(ctx, RRRMC_ERR_UNSUPPORTED, "%s is not wired for the %s (rrrMC and standardMC are)", sampler, ens_graph_name(ctx));
}
// a call that needs the ensemble's parameters before rrrmc_*_set_params has given them (the samplers spell them in Greek, the energy call in Latin)
int32_t ens_needs_params(rrrmc_ctx* ctx, bool greek)
{
    const char *g = greek ? "γ" : "gamma", *l = greek ? "λ" : "lambda", *b = greek ? "β" : "beta";
    if (is_tle(ctx))
        return fail(ctx, RRRMC_ERR_STATE, "a %s needs its neighbour lists and (%s, %s, %s): call rrrmc_tle_set_topology and rrrmc_tle_set_params first", ens_graph_name(ctx), g, l, b);
    return fail(ctx, RRRMC_ERR_STATE, "a %s needs (%s, %s): call rrrmc_%s_set_params first", ens_graph_name(ctx), g, b, is_re(ctx) ? "re" : "le");
}

int32_t re_to_slices(rrrmc_ctx* ctx, const ReParams& P)
{
    hipLaunchKernelGGL(re_to_slices_kernel, dim3((unsigned)((P.W + 255) / 256), (unsigned)P.R), dim3(256), 0, ctx->stream, P);
    HIP_TRY(ctx, hipGetLastError());
    return RRRMC_OK;
}

// ---- the frame of a sampler call: rrrMC(X::DoubleGraph) (standard = false) or standardMC (standard = true) on an ensemble ----
struct EnsCall {
    SmpState S;
    int64_t nsamp;
    bool cont;          // the call continues the live run: no *_run_init
};
// the argument checks, the run's state, room for the samples, the events; ends with ev_begin on the stream.  ensemble = false: the caller is no
// ensemble (host_af.hpp) and has checked what its own graph needs
int32_t ens_call_begin(rrrmc_ctx* ctx, bool standard, double beta, int64_t iters, int64_t step, double staged_thr, double staged_thr_fact, EnsCall* C, bool ensemble = true)
{
    int32_t rc = RRRMC_OK;
    if (ensemble && !ctx->re_params_set) return ens_needs_params(ctx, true);
    if (iters < 0) return fail(ctx, RRRMC_ERR_INVALID_ARG, "iters must be >= 0, given %lld", (long long)iters);
    if (step < 1) return fail(ctx, RRRMC_ERR_INVALID_ARG, "step must be >= 1, given %lld", (long long)step);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    ctx->results_valid = false; ctx->last_call_wtm = false; ctx->last_call_eo = false;
    ctx->timing_valid = false;
    C->S = SmpState{};
    if (!standard) { rc = smp_begin(ctx, 1, beta, staged_thr, staged_thr_fact, 0.0, step, nullptr, &C->S); if (rc) return rc; }
    else C->S.samp0 = step;
    C->nsamp = standard ? iters / step : smp_nsamp(ctx, iters, step);
    const size_t es_need = (size_t)(C->nsamp > 0 ? C->nsamp : 1) * ctx->R;
    HIP_TRY(ctx, dev_grow(ctx, ctx->sk_Es, ctx->sk_Es_cap, es_need));
    while (ctx->ev_sweep.size() < 2) {
        hipEvent_t e;
        HIP_TRY(ctx, hipEventCreate(&e));
        ctx->ev_sweep.push_back(e);
    }
    HIP_TRY(ctx, hipEventRecord(ctx->ev_begin, ctx->stream));
    ctx->stats_stride = 2;
    C->cont = (standard && ctx->resume && ctx->std_cache_live) || C->S.resume;
    return RRRMC_OK;
}
// a continued call in place of *_run_init: the working copy gets the same bits the run left (nothing in between changed the configuration)
int32_t ens_call_resume(rrrmc_ctx* ctx, const ReParams& P, bool standard)
{
    const int32_t rc = re_to_slices(ctx, P);
    if (rc) return rc;
    if (!standard) HIP_TRY(ctx, hipMemsetAsync(ctx->q_stats, 0, sizeof(int64_t) * (size_t)ctx->R * 2, ctx->stream));
    return RRRMC_OK;
}
// the call's own fields of the kernel parameters
inline void ens_call_params(const rrrmc_ctx* ctx, const EnsCall& C, int64_t iters, int64_t step, double staged_thr, double staged_thr_fact, ReParams* P)
{
    P->staged_thr = staged_thr;
    P->lambda = staged_thr_fact / (double)ctx->N;              // RRRMC.jl:243
    P->g0 = ctx->it_done; P->iters = iters; P->step = step; P->samp0 = C.S.samp0;
}
// behind the sweep kernel: the spins back in ABI order, the family's debug check (debug_check() -> int32_t), the bookkeeping
template <typename Check> int32_t ens_call_end(rrrmc_ctx* ctx, const ReParams& P, const EnsCall& C, bool standard, int64_t iters, Check&& debug_check)
{
    hipStream_t st = ctx->stream;
    HIP_TRY(ctx, hipEventRecord(ctx->ev_sweep[1], st));
    hipLaunchKernelGGL(re_from_slices_kernel, dim3((unsigned)((P.W + 255) / 256), (unsigned)P.R), dim3(256), 0, st, P);
    HIP_TRY(ctx, hipGetLastError());
    if (ctx->debug_checks) { const int32_t rc = debug_check(); if (rc) return rc; }
    HIP_TRY(ctx, hipEventRecord(ctx->ev_end, st));
    ctx->sweep_launches = 1;
    ctx->nsamp = C.nsamp;
    ctx->it_done += (uint64_t)iters;
    if (!standard) smp_commit(ctx, 1, iters);
    ctx->results_valid = true;
    ctx->timing_valid = true;
    ctx->last_call_rrr = true;          // accepted / staged counts live in q_stats
    ctx->q_cache_valid = !standard;
    ctx->std_cache_live = standard;
    return RRRMC_OK;
}

// ---- context creation: a Robust Ensemble has M rows of Nk spins, a Local Entropy ensemble M + 1 (row 0 the centre); a TLE context starts
//      as a Local Entropy one (tle_ctx_create) ----
// the table width K of a sparse Float64 slice graph: given by rrrmc_ctx_create_re_f64 / _le_f64 / _tle_f64, not by the creators that carry no K
struct SliceK { bool given = false; int64_t K = 0; };
// the sparse Float64 slices of the call's parameters, and whether the LDS build with `base` bytes of its own can stage their state too
inline void ens_spf_params(const rrrmc_ctx* ctx, ReParams* P)
{
    P->A = ctx->d_A; P->Jf = ctx->q_Jf; P->K = (int)ctx->K; P->flf = ctx->q_flf; P->fundo = ctx->q_fundo; P->fml = ctx->q_fml;
}
inline size_t ens_spf_lds(const rrrmc_ctx* ctx, size_t base, int64_t rows, ReParams* P)
{
    const size_t tot = ((base + 7) & ~(size_t)7) + spf_ens_lds_bytes(rows, ctx->qNk, ctx->K);
    P->spf_lds = base <= (size_t)kLdsLimit && tot <= (size_t)kLdsLimit ? 1 : 0;          // else the slice state stays in global memory, as RE_SKN's does
    return P->spf_lds ? tot : base;
}
// `creator`: the ensemble whose exported creator was called, where it is not `family` (tle_ctx_create builds on a Local Entropy context)
int32_t ens_ctx_create(EnsFamily family, rrrmc_ctx** out, int64_t Nk, int64_t M, int32_t slice_kind, int64_t R, int32_t device, uint32_t replica0, SliceK k = {},
                       EnsFamily creator = ENS_NONE)
{
    const int64_t K = k.K;
    if (creator == ENS_NONE) creator = family;
    const bool re = family == ENS_RE;
    const char* name = re ? "Robust Ensemble" : "Local Entropy";
    const int Mmax = re ? kReMmax : kLeMmax;
    if (!out) return fail(nullptr, RRRMC_ERR_INVALID_ARG, "out is NULL");
    *out = nullptr;
    const bool perc = slice_kind == RRRMC_RE_SLICE_PERC_STEP || slice_kind == RRRMC_RE_SLICE_PERC_LINEAR;
    const bool comm = slice_kind == RRRMC_RE_SLICE_COMM_STEP || slice_kind == RRRMC_RE_SLICE_COMM_RELU || slice_kind == RRRMC_RE_SLICE_COMM_QU;
    if (ens_model(family, slice_kind) == kEnsNoModel)
        return fail(nullptr, RRRMC_ERR_INVALID_ARG, "slice_kind must be RRRMC_RE_SLICE_EMPTY, _SK, _SKN, _PERC_STEP, _PERC_LINEAR, _COMM_STEP, _COMM_RELU, _SAT or _COMM_QU, given: %d", slice_kind);
    const bool spf = slice_kind == RRRMC_RE_SLICE_SPARSE_F64;
    if (spf && !k.given)
        return fail(nullptr, RRRMC_ERR_INVALID_ARG, "slice_kind RRRMC_RE_SLICE_SPARSE_F64 needs the K of the slice graph: use rrrmc_ctx_create_%s_f64",
                    creator == ENS_RE ? "re" : creator == ENS_LE ? "le" : "tle");
    if (Nk < 1 || R < 1) return fail(nullptr, RRRMC_ERR_INVALID_ARG, "Nk and R must be >= 1");
    if (spf && K < 1) return fail(nullptr, RRRMC_ERR_INVALID_ARG, "Nk, K, R must be >= 1");
    if (spf && K > kContKmax) return fail(nullptr, RRRMC_ERR_UNSUPPORTED, "K=%lld: the Float64 sparse slice kernels cover K <= %d", (long long)K, kContKmax);
    if (perc) { const int32_t rcn = perc_check_n(Nk); if (rcn) return rcn; }
    if (comm) { const int32_t rcn = comm_check_nk(Nk, slice_kind != RRRMC_RE_SLICE_COMM_STEP); if (rcn) return rcn; }
    if (M <= 2) return fail(nullptr, RRRMC_ERR_INVALID_ARG, "M must be greater than 2, given: %lld", (long long)M);      // RE.jl:37, LE.jl:24
    if (M > Mmax) return fail(nullptr, RRRMC_ERR_UNSUPPORTED, "M = %lld: the %s kernels cover M <= %d", (long long)M, name, Mmax);
    const int64_t rows = re ? M : M + 1, N = Nk * rows, L = re ? re_levels(M) : le_levels(M);
    if (N > 65535)
        return fail(nullptr, RRRMC_ERR_UNSUPPORTED, "N = Nk*%s = %lld is beyond the %s kernels (16-bit set members: N <= 65535)", re ? "M" : "(M+1)", (long long)N, name);
    if (replica0 % 32) return fail(nullptr, RRRMC_ERR_INVALID_ARG, "replica0 must be a multiple of 32 (given %u)", replica0);
    rrrmc_ctx* ctx = nullptr;
    { const int32_t rcb = ctx_create_begin(&ctx, device, false); if (rcb) return rcb; }
    ctx->model = ens_model(family, slice_kind);
    ctx->N = N; ctx->K = spf ? K : 0; ctx->R = R; ctx->Rpad = R;
    ctx->qNk = Nk; ctx->qM = M; ctx->qW = 2 * ((N + 63) / 64); ctx->q_Wk = 2 * ((Nk + 63) / 64);
    ctx->replica0 = replica0;
    ctx->graph_set = slice_kind == RRRMC_RE_SLICE_EMPTY;          // Graph0RE / Graph0LE has no couplings to give
    // Robust Ensemble: host tables ΔElist [M], the μ-energies [M + 1]; device: the same, then ft [L].
    // Local Entropy: host tables allΔE [L], the class codes [2M + 1] apart in le_hcode; device: allΔE [L], ft [L], the codes.  re_hft stages ft [L].
    const int64_t ncode_d = re ? 0 : (2 * M + 1 + 7) / 8, ntab_h = re ? 2 * M + 1 : L, ntab_d = re ? 2 * M + 1 + L : 2 * L + ncode_d;
    ctx->re_htab.assign((size_t)ntab_h, 0.0);
    ctx->le_hcode.assign((size_t)(8 * ncode_d), 0xFF);
    ctx->re_hft.assign((size_t)L, 0.0);
    if (slice_kind == RRRMC_RE_SLICE_SKN) {
        CTX_CREATE_TRY(ctx, false, dev_alloc(ctx, ctx->sk_J, Nk * Nk));
        CTX_CREATE_TRY(ctx, false, dev_alloc(ctx, ctx->q_slf, (size_t)R * 2 * (size_t)rows * (size_t)Nk));
        CTX_CREATE_TRY(ctx, false, dev_alloc(ctx, ctx->q_smv, (size_t)R * (size_t)rows));
        CTX_CREATE_TRY(ctx, false, dev_alloc(ctx, ctx->q_scur, (size_t)R * (size_t)rows));
    } else if (slice_kind == RRRMC_RE_SLICE_SK) {
        CTX_CREATE_TRY(ctx, false, dev_alloc(ctx, ctx->q_Jb, Nk * ctx->q_Wk));
    } else if (spf) {
        // the shared graph, and per chain every row's LocalFields{Float64}: lfields, the K + 1 values of the undo record, move_last
        CTX_CREATE_TRY(ctx, false, dev_alloc(ctx, ctx->d_A, Nk * K));
        CTX_CREATE_TRY(ctx, false, dev_alloc(ctx, ctx->q_Jf, Nk * K));
        CTX_CREATE_TRY(ctx, false, dev_alloc(ctx, ctx->q_flf, (size_t)R * (size_t)rows * (size_t)Nk));
        CTX_CREATE_TRY(ctx, false, dev_alloc(ctx, ctx->q_fundo, (size_t)R * (size_t)rows * (size_t)(K + 1)));
        CTX_CREATE_TRY(ctx, false, dev_alloc(ctx, ctx->q_fml, (size_t)R * (size_t)rows));
        CTX_CREATE_TRY(ctx, false, hipMemset(ctx->q_flf, 0, sizeof(double) * (size_t)R * (size_t)rows * (size_t)Nk));          // (a centre row is never built)
    }
    CTX_CREATE_TRY(ctx, false, dev_alloc(ctx, ctx->re_tab, (size_t)ntab_d));
    CTX_CREATE_TRY(ctx, false, dev_alloc(ctx, ctx->q_spins, R * ctx->qW));
    CTX_CREATE_TRY(ctx, false, dev_alloc(ctx, ctx->re_sp, R * ctx->qW));
    CTX_CREATE_TRY(ctx, false, dev_alloc(ctx, ctx->re_mu, (size_t)R * Nk));
    CTX_CREATE_TRY(ctx, false, dev_alloc(ctx, ctx->q_cls, (size_t)R * N));
    CTX_CREATE_TRY(ctx, false, dev_alloc(ctx, ctx->q_sv, (size_t)R * 2 * L * N));
    CTX_CREATE_TRY(ctx, false, dev_alloc(ctx, ctx->q_spos, (size_t)R * N));
    CTX_CREATE_TRY(ctx, false, dev_alloc(ctx, ctx->q_st, R * 2 * L));
    CTX_CREATE_TRY(ctx, false, dev_alloc(ctx, ctx->q_T, R * 2 * L));
    CTX_CREATE_TRY(ctx, false, dev_alloc(ctx, ctx->q_z, R));
    CTX_CREATE_TRY(ctx, false, dev_alloc(ctx, ctx->q_accrate, R));
    CTX_CREATE_TRY(ctx, false, dev_alloc(ctx, ctx->q_stats, R * 2));
    CTX_CREATE_TRY(ctx, false, dev_alloc(ctx, ctx->sk_E, R));
    CTX_CREATE_TRY(ctx, false, dev_alloc(ctx, ctx->re_Eslice, R * rows));
    if (!re) CTX_CREATE_TRY(ctx, false, dev_alloc(ctx, ctx->le_dist, R * M * M));
    CTX_CREATE_TRY(ctx, false, hipMemset(ctx->q_spins, 0, sizeof(uint32_t) * R * ctx->qW));
    *out = ctx;
    return RRRMC_OK;
}
