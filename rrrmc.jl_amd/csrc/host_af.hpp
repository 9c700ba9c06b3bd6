// Host side of GraphAddFields / GraphAddSubFields (af_kernels.hpp): context creation, the fields, the kernel parameters, the start of a
// run, the debug check, the build choice and launch of a sampler call.  g is one slice of the ensembles' slice kinds (M = 1), so its
// uploads are the ensembles' (rrrmc_set_couplings_bits / _dense, rrrmc_set_patterns, rrrmc_set_comm_patterns, rrrmc_set_clauses) and the
// frame of a sampler call is theirs (host_ens.hpp).  The model <-> (wrapper, kind of g) relation is the table of af_models.hpp.
// Included by rrrmc_hip.hip inside its anonymous namespace, after host_ens.hpp; not a stand-alone translation unit.
// (a mixed context, host_mixed.hpp, is one of the family: the stand-alone GraphMixed runs as a GraphAddSubFields whose fields are never read)
// (so is a wrapper over a GraphPSpin3, host_pspin.hpp, whose model ids have a lookup of their own: af_slice_of / af_sub_of below)
inline bool is_af(const rrrmc_ctx* ctx) { return af_family(ctx->model) != AF_NONE || is_mixed(ctx) || pspin_af(ctx); }
// the kind of g and the wrapper of a context of the family that is no mix
inline int af_slice_of(const rrrmc_ctx* ctx) { return pspin_af(ctx) ? (int)RE_PSPIN3 : (int)af_slice(ctx->model); }
inline bool af_sub_of(const rrrmc_ctx* ctx) { return pspin_af(ctx) ? pspin_wrap(ctx->model) == 2 : af_family(ctx->model) == AF_ADDSUB; }
inline const char* af_graph_name(const rrrmc_ctx* ctx)
{
    if (is_mixed(ctx)) return mixed_wrap(ctx->model) == 0 ? "GraphMixed" : mixed_wrap(ctx->model) == 2 ? "GraphAddSubFields over a GraphMixed" : "GraphAddFields over a GraphMixed";
    return af_sub_of(ctx) ? "GraphAddSubFields" : "GraphAddFields";
}
int32_t mixed_run_init(rrrmc_ctx* ctx, double beta, bool cache);          // host_mixed.hpp
int32_t mixed_mc_async(rrrmc_ctx* ctx, bool standard, double beta, int64_t iters, int64_t step, double staged_thr, double staged_thr_fact);
// bklMC, wtmMC and extremal_opt on the family
int32_t af_not_wired(rrrmc_ctx* ctx, const char* sampler)
{
    return fail(ctx, RRRMC_ERR_UNSUPPORTED, "%s is not wired for %s (rrrMC and standardMC are)", sampler, af_graph_name(ctx));
}
int32_t af_needs_fields(rrrmc_ctx* ctx) { return fail(ctx, RRRMC_ERR_STATE, "a %s needs its fields: call rrrmc_af_set_fields first", af_graph_name(ctx)); }

// g is any ensemble slice kind, or GraphPercXEntr or GraphPSpin3 (which no ensemble takes): the wrappers' kernels are built over this set
using AfSlices = SliceSet<RE_EMPTY, RE_SK, RE_SKN, RE_PSTEP, RE_PLIN, RE_CSTEP, RE_CRELU, RE_SAT, RE_CQU, RE_PXE, RE_PSPIN3>;
static_assert((int)RE_PXE == RRRMC_RE_SLICE_PERC_XENTR, "ReSlice is rrrmc_re_slice");

constexpr int64_t kAfNmax = 65535;          // N of a wrapper over GraphEmpty / GraphSK / GraphSKNormal (the other kinds bring their own bound)

// every check of rrrmc_ctx_create_af, before any device query
int32_t af_check_create(rrrmc_ctx** out, int32_t slice_kind, int32_t sub, int64_t N, int64_t K2, int64_t R, uint32_t replica0)
{
    if (!out) return fail(nullptr, RRRMC_ERR_INVALID_ARG, "out is NULL");
    *out = nullptr;
    if (af_model(AF_ADD, slice_kind) == kAfNoModel)
        return fail(nullptr, RRRMC_ERR_INVALID_ARG, "GraphAddFields: slice_kind must be RRRMC_RE_SLICE_EMPTY, _SK, _SKN, _PERC_STEP, _PERC_LINEAR, _COMM_STEP, _COMM_RELU, _SAT, _COMM_QU or _PERC_XENTR, given: %d", slice_kind);
    if (sub != 0 && sub != 1) return fail(nullptr, RRRMC_ERR_INVALID_ARG, "sub must be 0 (GraphAddFields) or 1 (GraphAddSubFields), given: %d", sub);
    if (N < 1 || R < 1) return fail(nullptr, RRRMC_ERR_INVALID_ARG, "GraphAddFields: N and R must be >= 1");
    const bool perc = slice_kind == RRRMC_RE_SLICE_PERC_STEP || slice_kind == RRRMC_RE_SLICE_PERC_LINEAR || slice_kind == RRRMC_RE_SLICE_PERC_XENTR;
    const bool comm = slice_kind == RRRMC_RE_SLICE_COMM_STEP || slice_kind == RRRMC_RE_SLICE_COMM_RELU || slice_kind == RRRMC_RE_SLICE_COMM_QU;
    if (perc) { const int32_t rcn = perc_check_n(N); if (rcn) return rcn; }
    if (comm) {
        if (K2 < 1 || N % K2 != 0)
            return fail(nullptr, RRRMC_ERR_INVALID_ARG, "a committee machine takes N = K1*K2 with N %% K2 == 0, given N = %lld, K2 = %lld", (long long)N, (long long)K2);
        const int32_t rck = comm_check_k(nullptr, N / K2, K2, slice_kind != RRRMC_RE_SLICE_COMM_STEP);
        if (rck) return rck;
    }
    if (slice_kind == RRRMC_RE_SLICE_SAT && N > kSatNmax)
        return fail(nullptr, RRRMC_ERR_UNSUPPORTED, "N = %lld: the K-SAT kernels cover N <= %d (16-bit variable ids)", (long long)N, kSatNmax);
    if (N > kAfNmax) return fail(nullptr, RRRMC_ERR_UNSUPPORTED, "N = %lld: the GraphAddFields kernels cover N <= %lld", (long long)N, (long long)kAfNmax);
    if (replica0 % 32) return fail(nullptr, RRRMC_ERR_INVALID_ARG, "replica0 must be a multiple of 32 (given %u)", replica0);
    return RRRMC_OK;
}

int32_t af_ctx_create(rrrmc_ctx** out, int32_t slice_kind, int32_t sub, int64_t N, int64_t K2, int64_t R, int32_t device, uint32_t replica0)
{
    { const int32_t rcc = af_check_create(out, slice_kind, sub, N, K2, R, replica0); if (rcc) return rcc; }
    rrrmc_ctx* ctx = nullptr;
    { const int32_t rcb = ctx_create_begin(&ctx, device, false); if (rcb) return rcb; }
    ctx->model = af_model(sub ? AF_ADDSUB : AF_ADD, slice_kind);
    ctx->N = N; ctx->K = 0; ctx->R = R; ctx->Rpad = R;
    ctx->qNk = N; ctx->qM = 1; ctx->qW = 2 * ((N + 63) / 64); ctx->q_Wk = ctx->qW;
    ctx->replica0 = replica0;
    ctx->graph_set = slice_kind == RRRMC_RE_SLICE_EMPTY;          // GraphEmpty has nothing to upload
    if (slice_kind == RRRMC_RE_SLICE_COMM_STEP || slice_kind == RRRMC_RE_SLICE_COMM_RELU || slice_kind == RRRMC_RE_SLICE_COMM_QU) ctx->cm_K2 = K2;
    int levs = 0;
    while (((int64_t)1 << levs) < N) ++levs;                       // DynamicSamplers.jl:36
    ctx->af_levs = levs; ctx->af_N2 = (int64_t)1 << levs;
    if (slice_kind == RRRMC_RE_SLICE_SKN) {
        CTX_CREATE_TRY(ctx, false, dev_alloc(ctx, ctx->sk_J, N * N));
        CTX_CREATE_TRY(ctx, false, dev_alloc(ctx, ctx->q_slf, (size_t)R * 2 * (size_t)N));
        CTX_CREATE_TRY(ctx, false, dev_alloc(ctx, ctx->q_smv, (size_t)R));
        CTX_CREATE_TRY(ctx, false, dev_alloc(ctx, ctx->q_scur, (size_t)R));
    } else if (slice_kind == RRRMC_RE_SLICE_SK) {
        CTX_CREATE_TRY(ctx, false, dev_alloc(ctx, ctx->q_Jb, N * ctx->q_Wk));
    }
    CTX_CREATE_TRY(ctx, false, dev_alloc(ctx, ctx->q_spins, R * ctx->qW));
    CTX_CREATE_TRY(ctx, false, dev_alloc(ctx, ctx->q_z, R));
    CTX_CREATE_TRY(ctx, false, dev_alloc(ctx, ctx->q_accrate, R));
    CTX_CREATE_TRY(ctx, false, dev_alloc(ctx, ctx->q_stats, R * 2));
    CTX_CREATE_TRY(ctx, false, dev_alloc(ctx, ctx->sk_E, R));
    CTX_CREATE_TRY(ctx, false, dev_alloc(ctx, ctx->af_h, N));
    CTX_CREATE_TRY(ctx, false, dev_alloc(ctx, ctx->af_dEs, (size_t)R * (size_t)N));
    CTX_CREATE_TRY(ctx, false, dev_alloc(ctx, ctx->af_v, (size_t)R * (size_t)ctx->af_N2));
    CTX_CREATE_TRY(ctx, false, dev_alloc(ctx, ctx->af_ps, (size_t)R * (size_t)ctx->af_N2));
    CTX_CREATE_TRY(ctx, false, dev_alloc(ctx, ctx->af_tref, (size_t)R));
    CTX_CREATE_TRY(ctx, false, dev_alloc(ctx, ctx->af_status, 2));
    CTX_CREATE_TRY(ctx, false, hipMemset(ctx->q_spins, 0, sizeof(uint32_t) * R * ctx->qW));
    CTX_CREATE_TRY(ctx, false, hipMemset(ctx->af_status, 0, sizeof(int32_t) * 2));
    *out = ctx;
    return RRRMC_OK;
}

// rrrmc_af_set_fields on one device
int32_t af_set_fields(rrrmc_ctx* ctx, const double* h)
{
    if (!h) return fail(ctx, RRRMC_ERR_INVALID_ARG, "%s: h is NULL", af_graph_name(ctx));
    for (int64_t i = 0; i < ctx->N; ++i)
        if (!std::isfinite(h[i])) return fail(ctx, RRRMC_ERR_INVALID_ARG, "%s: the fields must be finite, found: h[%lld] = %g", af_graph_name(ctx), (long long)i, h[i]);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipMemcpy(ctx->af_h, h, sizeof(double) * (size_t)ctx->N, hipMemcpyHostToDevice));
    ctx->std_cache_live = false;
    ctx->q_cache_valid = false;
    ctx->af_fields_set = true;
    return RRRMC_OK;
}

AfParams af_params(rrrmc_ctx* ctx, double beta)
{
    AfParams A{};
    ReParams& P = A.re;
    const int slice = af_slice_of(ctx);
    if (slice == RE_SK) { P.Jb = ctx->q_Jb; P.Wk = (int)ctx->q_Wk; P.sN = std::sqrt((double)ctx->N); }
    if (slice == RE_SKN) { P.Jd = ctx->sk_J; P.slf = ctx->q_slf; P.smv = ctx->q_smv; P.scur = ctx->q_scur; }
    if (slice == RE_PSTEP || slice == RE_PLIN) P.pc = perc_params(ctx, 1);
    if (slice == RE_PXE) { P.pc = perc_params(ctx, 1); P.xe = xentr_params(ctx); }
    if (slice == RE_CSTEP || slice == RE_CRELU || slice == RE_CQU) P.cm = comm_params(ctx, 1);
    if (slice == RE_SAT) P.sat = sat_table(ctx);
    if (slice == RE_PSPIN3) P.ps3 = pspin_table(ctx);
    P.abi = ctx->q_spins; P.sp = ctx->q_spins;          // M = 1: the ABI site order is the slice's own
    P.zz = ctx->q_z; P.E_cur = ctx->sk_E; P.acc_rate = ctx->q_accrate; P.stats = ctx->q_stats; P.Es = ctx->sk_Es; P.flag = ctx->dbg_flag;
    P.beta = beta;
    P.k0 = (uint32_t)ctx->seed; P.k1 = (uint32_t)(ctx->seed >> 32); P.replica0 = ctx->replica0;
    P.Nk = (int)ctx->N; P.M = 1; P.L = 0; P.N = (int)ctx->N; P.W = (int)ctx->qW; P.R = (int)ctx->R;
    A.h = ctx->af_h; A.dEs = ctx->af_dEs; A.v = ctx->af_v; A.ps = ctx->af_ps; A.tref = ctx->af_tref; A.status = ctx->af_status;
    A.sub = af_sub_of(ctx) ? 1 : 0; A.levs = ctx->af_levs; A.N2 = (int)ctx->af_N2;
    return A;
}

// energy(X, C), g's cache and, for rrrMC, a fresh DeltaECacheCont over X0: the start of a reference call (src/RRRMC.jl:237-240)
int32_t af_run_init(rrrmc_ctx* ctx, double beta, bool cache)
{
    if (is_mixed(ctx)) return mixed_run_init(ctx, beta, cache);
    const AfParams A = af_params(ctx, beta);
    const dim3 grid((unsigned)ctx->R), blk(kAfInitThreads);
    if (!with_slice(AfSlices{}, af_slice_of(ctx), [&](auto s) { hipLaunchKernelGGL(af_init_kernel<decltype(s)::value>, grid, blk, 0, ctx->stream, A, cache ? 1 : 0); }))
        return ens_bad_slice(ctx);
    HIP_TRY(ctx, hipGetLastError());
    return RRRMC_OK;
}

// debug mode: the consistency check behind a sampler call (reported by the next sync, post_sync_checks)
int32_t af_debug_check(rrrmc_ctx* ctx, const AfParams& A0, bool cache)
{
    const int32_t rc = dbg_flag_ensure(ctx);
    if (rc) return rc;
    AfParams A = A0;
    A.re.flag = ctx->dbg_flag;
    const dim3 grid((unsigned)((ctx->R + 63) / 64)), blk(64);
    if (!with_slice(AfSlices{}, af_slice_of(ctx), [&](auto s) { hipLaunchKernelGGL(af_check_kernel<decltype(s)::value>, grid, blk, 0, ctx->stream, A, cache ? 1 : 0); }))
        return ens_bad_slice(ctx);
    HIP_TRY(ctx, hipGetLastError());
    return RRRMC_OK;
}

typedef void (*af_kernel_fn)(AfParams);
// nullptr: no such slice
af_kernel_fn af_rrr_fn(int slice, bool lds)
{
    af_kernel_fn fn = nullptr;
    with_slice(AfSlices{}, slice, [&](auto s) { fn = lds ? af_rrr_kernel<decltype(s)::value, true> : af_rrr_kernel<decltype(s)::value, false>; });
    return fn;
}

// rrrMC(X::DoubleGraph) (standard = false) or standardMC (standard = true) on a GraphAddFields / GraphAddSubFields
int32_t af_mc_async(rrrmc_ctx* ctx, bool standard, double beta, int64_t iters, int64_t step, double staged_thr, double staged_thr_fact)
{
    if (!ctx->af_fields_set) return af_needs_fields(ctx);
    if (is_mixed(ctx)) return mixed_mc_async(ctx, standard, beta, iters, step, staged_thr, staged_thr_fact);
    if (standard && std::isnan(beta)) return fail(ctx, RRRMC_ERR_INVALID_ARG, "beta is NaN");
    EnsCall C;
    int32_t rc = ens_call_begin(ctx, standard, beta, iters, step, staged_thr, staged_thr_fact, &C, false);
    if (rc) return rc;
    if (C.cont) { if (!standard) HIP_TRY(ctx, hipMemsetAsync(ctx->q_stats, 0, sizeof(int64_t) * (size_t)ctx->R * 2, ctx->stream)); }
    else { rc = af_run_init(ctx, beta, !standard); if (rc) return rc; }
    AfParams A = af_params(ctx, beta);
    ens_call_params(ctx, C, iters, step, staged_thr, staged_thr_fact, &A.re);
    const int slice = af_slice_of(ctx);
    hipStream_t st = ctx->stream;
    HIP_TRY(ctx, hipEventRecord(ctx->ev_sweep[0], st));
    if (standard) {
        const dim3 grid(rrr_blocks(ctx->R)), blk(rrr_tpb(ctx->R));
        if (!with_slice(AfSlices{}, slice, [&](auto s) { hipLaunchKernelGGL(af_standard_kernel<decltype(s)::value>, grid, blk, 0, st, A); })) return ens_bad_slice(ctx);
    } else {
        // the LDS build whenever the chain's state fits: a rule of fit, not a measured crossing (RRRMC_AF_NO_LDS=1 forces the global build:
        // the builds' parity test)
        size_t lds = (af_lds_bytes(ctx->N, ctx->af_N2, ctx->qW) + 7) & ~(size_t)7;
        if (slice == RE_SKN) lds += (size_t)16 * (size_t)ctx->N;
        if (slice == RE_PSTEP || slice == RE_PLIN) lds += perc_lds_bytes(1, A.re.pc.PW);
        if (A.re.cm.ds) lds += comm_lds_bytes(1, A.re.cm.K2, A.re.cm.PW, slice == RE_CQU);
        if (slice == RE_PXE) {          // Δs and the term buffer; the loss table joins them when everything still fits
            lds = (af_lds_bytes(ctx->N, ctx->af_N2, ctx->qW) + 15) & ~(size_t)15;
            A.xe_hs_lds = lds + xentr_lds_bytes(ctx->N, A.re.pc.PW, 0, true) <= (size_t)kLdsLimit ? 1 : 0;
            lds += xentr_lds_bytes(ctx->N, A.re.pc.PW, 0, A.xe_hs_lds != 0);
        }
        const char* no_lds = std::getenv("RRRMC_AF_NO_LDS");
        const bool use_lds = lds <= (size_t)kLdsLimit && !(no_lds && no_lds[0] == '1');
        if (slice == RE_PXE && !use_lds) {          // the global build keeps the term buffer in global memory
            const int64_t Pp = 64 * (int64_t)A.re.pc.PW;
            if (ctx->xe_term_P != ctx->pc_P) { dev_free(ctx, ctx->xe_term); ctx->xe_term_P = 0; }
            if (!ctx->xe_term) { HIP_TRY(ctx, dev_alloc(ctx, ctx->xe_term, (size_t)(ctx->R * Pp))); ctx->xe_term_P = ctx->pc_P; }
            A.re.xe.term = ctx->xe_term;
        }
        const af_kernel_fn fn = af_rrr_fn(slice, use_lds);
        if (!fn) return ens_bad_slice(ctx);
        if (use_lds) HIP_TRY(ctx, raise_lds_attr(reinterpret_cast<const void*>(fn), lds));
        hipLaunchKernelGGL(fn, dim3((unsigned)ctx->R), dim3(64), use_lds ? lds : 0, st, A);
        ctx->af_build = use_lds ? 1 : 2;
    }
    HIP_TRY(ctx, hipGetLastError());
    // behind the kernel: what ens_call_end does, without the copy back from a slice-major working set (there is none)
    HIP_TRY(ctx, hipEventRecord(ctx->ev_sweep[1], st));
    if (ctx->debug_checks) { rc = af_debug_check(ctx, A, !standard); if (rc) return rc; }
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
