// Host side of the Robust Ensemble (GraphRobustEnsemble over GraphEmpty / binary GraphSK / GraphSKNormal slices, re_kernels.hpp).
// Included by rrrmc_hip.hip inside its anonymous namespace, after the context struct and the common helpers
// (fail, HIP_TRY, free_dev, ensure_state, smp_begin); not a stand-alone translation unit.
inline bool is_re(const rrrmc_ctx* ctx) { return ctx->model == RRRMC_MODEL_RE_EMPTY || ctx->model == RRRMC_MODEL_RE_SK || ctx->model == RRRMC_MODEL_RE_SKN ||
                                                ctx->model == RRRMC_MODEL_RE_PERC_STEP || ctx->model == RRRMC_MODEL_RE_PERC_LINEAR ||
                                                ctx->model == RRRMC_MODEL_RE_COMM_STEP || ctx->model == RRRMC_MODEL_RE_COMM_RELU || ctx->model == RRRMC_MODEL_RE_SAT ||
                                                ctx->model == RRRMC_MODEL_RE_COMM_QU; }
inline int re_slice_of(const rrrmc_ctx* ctx) { return ctx->model == RRRMC_MODEL_RE_SK ? RE_SK : ctx->model == RRRMC_MODEL_RE_SKN ? RE_SKN :
                                                      ctx->model == RRRMC_MODEL_RE_PERC_STEP ? RE_PSTEP : ctx->model == RRRMC_MODEL_RE_PERC_LINEAR ? RE_PLIN :
                                                      ctx->model == RRRMC_MODEL_RE_COMM_STEP ? RE_CSTEP : ctx->model == RRRMC_MODEL_RE_COMM_RELU ? RE_CRELU : ctx->model == RRRMC_MODEL_RE_SAT ? RE_SAT :
                                                      ctx->model == RRRMC_MODEL_RE_COMM_QU ? RE_CQU : RE_EMPTY; }
inline int re_levels(int64_t M) { return (int)((M + 1) / 2); }          // allΔE(GraphRE): ceil(M / 2) values (RE.jl:208-213)

// logcoshratio and fk (RE.jl:18-26), ΔElist (RE.jl:53-56) and the μ-energy table log(2 cosh(γ μ)) / β (RE.jl:90-93), host libm
void re_tables(int64_t M, double gamma, double beta, double* dElist, double* e0)
{
    auto logcoshratio = [](double a, double b) {
        a = std::fabs(a);
        b = std::fabs(b);
        return a - b + (std::log1p(std::exp(-2 * a)) - std::log1p(std::exp(-2 * b)));
    };
    for (int64_t d = 0; d < M; ++d) {
        const int64_t mub = 2 * d - (M - 1);
        dElist[d] = logcoshratio(gamma * (double)(mub + 1), gamma * (double)(mub - 1)) / beta;
    }
    for (int64_t d = 0; d <= M; ++d) {
        const int64_t mu = 2 * d - M;
        e0[d] = std::log(2 * std::cosh(gamma * (double)mu)) / beta;
    }
}

ReParams re_params(rrrmc_ctx* ctx, double beta)
{
    ReParams P{};
    const int64_t M = ctx->qM;
    if (ctx->model == RRRMC_MODEL_RE_SK) { P.Jb = ctx->q_Jb; P.Wk = (int)ctx->q_Wk; P.sN = std::sqrt((double)ctx->qNk); }
    if (ctx->model == RRRMC_MODEL_RE_SKN) { P.Jd = ctx->sk_J; P.slf = ctx->q_slf; P.smv = ctx->q_smv; P.scur = ctx->q_scur; }
    if (re_slice_of(ctx) == RE_PSTEP || re_slice_of(ctx) == RE_PLIN) P.pc = perc_params(ctx, M);
    if (re_slice_of(ctx) == RE_CSTEP || re_slice_of(ctx) == RE_CRELU || re_slice_of(ctx) == RE_CQU) P.cm = comm_params(ctx, M);
    if (re_slice_of(ctx) == RE_SAT) P.sat = sat_table(ctx);
    P.tab = ctx->re_tab; P.etab = ctx->re_tab + M; P.ft = ctx->re_tab + 2 * M + 1;
    P.abi = ctx->q_spins; P.sp = ctx->re_sp; P.mu = ctx->re_mu; P.cls = ctx->q_cls; P.sv = ctx->q_sv; P.spos = ctx->q_spos; P.st = ctx->q_st;
    P.T = ctx->q_T; P.zz = ctx->q_z; P.E_cur = ctx->sk_E; P.acc_rate = ctx->q_accrate; P.stats = ctx->q_stats; P.Es = ctx->sk_Es;
    P.Eslice = ctx->re_Eslice; P.flag = ctx->dbg_flag;
    P.beta = beta;
    P.k0 = (uint32_t)ctx->seed; P.k1 = (uint32_t)(ctx->seed >> 32); P.replica0 = ctx->replica0;
    P.Nk = (int)ctx->qNk; P.M = (int)M; P.L = re_levels(M); P.N = (int)ctx->N; P.W = (int)ctx->qW; P.R = (int)ctx->R;
    return P;
}

int32_t re_to_slices(rrrmc_ctx* ctx, const ReParams& P)
{
    hipLaunchKernelGGL(re_to_slices_kernel, dim3((unsigned)((P.W + 255) / 256), (unsigned)P.R), dim3(256), 0, ctx->stream, P);
    HIP_TRY(ctx, hipGetLastError());
    return RRRMC_OK;
}

// energy(X, C) and, for rrrMC, a fresh DeltaECache: the start of a reference call (src/RRRMC.jl:95, :236-238).  The class weights need the
// sampler's β: ft is uploaded here (stream-ordered behind earlier launches that read the previous values).
int32_t re_run_init(rrrmc_ctx* ctx, double beta, bool cache)
{
    const int L = re_levels(ctx->qM);
    for (int a = 0; a < L; ++a) ctx->re_hft[(size_t)a] = host_det_exp(-beta * ctx->re_htab[(size_t)(a + ctx->qM / 2)]);      // DeltaE.jl:91
    HIP_TRY(ctx, hipMemcpyAsync(ctx->re_tab + 2 * ctx->qM + 1, ctx->re_hft.data(), sizeof(double) * (size_t)L, hipMemcpyHostToDevice, ctx->stream));
    const ReParams P = re_params(ctx, beta);
    int32_t rc = re_to_slices(ctx, P);
    if (rc) return rc;
    switch (re_slice_of(ctx)) {
        case RE_SK: hipLaunchKernelGGL(re_init_kernel<RE_SK>, dim3((unsigned)ctx->R), dim3(kReInitThreads), 0, ctx->stream, P, cache ? 1 : 0); break;
        case RE_SKN: hipLaunchKernelGGL(re_init_kernel<RE_SKN>, dim3((unsigned)ctx->R), dim3(kReInitThreads), 0, ctx->stream, P, cache ? 1 : 0); break;
        case RE_PSTEP: hipLaunchKernelGGL(re_init_kernel<RE_PSTEP>, dim3((unsigned)ctx->R), dim3(kReInitThreads), 0, ctx->stream, P, cache ? 1 : 0); break;
        case RE_PLIN: hipLaunchKernelGGL(re_init_kernel<RE_PLIN>, dim3((unsigned)ctx->R), dim3(kReInitThreads), 0, ctx->stream, P, cache ? 1 : 0); break;
        case RE_CSTEP: hipLaunchKernelGGL(re_init_kernel<RE_CSTEP>, dim3((unsigned)ctx->R), dim3(kReInitThreads), 0, ctx->stream, P, cache ? 1 : 0); break;
        case RE_CRELU: hipLaunchKernelGGL(re_init_kernel<RE_CRELU>, dim3((unsigned)ctx->R), dim3(kReInitThreads), 0, ctx->stream, P, cache ? 1 : 0); break;
        case RE_CQU: hipLaunchKernelGGL(re_init_kernel<RE_CQU>, dim3((unsigned)ctx->R), dim3(kReInitThreads), 0, ctx->stream, P, cache ? 1 : 0); break;
        case RE_SAT: hipLaunchKernelGGL(re_init_kernel<RE_SAT>, dim3((unsigned)ctx->R), dim3(kReInitThreads), 0, ctx->stream, P, cache ? 1 : 0); break;
        default: hipLaunchKernelGGL(re_init_kernel<RE_EMPTY>, dim3((unsigned)ctx->R), dim3(kReInitThreads), 0, ctx->stream, P, cache ? 1 : 0); break;
    }
    HIP_TRY(ctx, hipGetLastError());
    return RRRMC_OK;
}

typedef void (*re_kernel_fn)(ReParams);
template <bool LDS, int SLICE> re_kernel_fn re_rrr_for_L(int L)
{
    if (L <= 2) return re_rrr_kernel<LDS, 2, SLICE>;
    if (L <= 4) return re_rrr_kernel<LDS, 4, SLICE>;
    if (L <= 8) return re_rrr_kernel<LDS, 8, SLICE>;
    return re_rrr_kernel<LDS, 16, SLICE>;
}
re_kernel_fn re_rrr_fn(int slice, bool lds, int L)
{
    switch (slice) {
        case RE_SK: return lds ? re_rrr_for_L<true, RE_SK>(L) : re_rrr_for_L<false, RE_SK>(L);
        case RE_SKN: return lds ? re_rrr_for_L<true, RE_SKN>(L) : re_rrr_for_L<false, RE_SKN>(L);
        case RE_PSTEP: return lds ? re_rrr_for_L<true, RE_PSTEP>(L) : re_rrr_for_L<false, RE_PSTEP>(L);
        case RE_PLIN: return lds ? re_rrr_for_L<true, RE_PLIN>(L) : re_rrr_for_L<false, RE_PLIN>(L);
        case RE_CSTEP: return lds ? re_rrr_for_L<true, RE_CSTEP>(L) : re_rrr_for_L<false, RE_CSTEP>(L);
        case RE_CRELU: return lds ? re_rrr_for_L<true, RE_CRELU>(L) : re_rrr_for_L<false, RE_CRELU>(L);
        case RE_CQU: return lds ? re_rrr_for_L<true, RE_CQU>(L) : re_rrr_for_L<false, RE_CQU>(L);
        case RE_SAT: return lds ? re_rrr_for_L<true, RE_SAT>(L) : re_rrr_for_L<false, RE_SAT>(L);
        default: return lds ? re_rrr_for_L<true, RE_EMPTY>(L) : re_rrr_for_L<false, RE_EMPTY>(L);
    }
}

// debug mode: the consistency check behind a sampler call (reported by the next sync, post_sync_checks)
int32_t re_debug_check(rrrmc_ctx* ctx, const ReParams& P0, bool cache)
{
    if (!ctx->dbg_flag) { HIP_TRY(ctx, hipMalloc(&ctx->dbg_flag, sizeof(int32_t) * 2)); HIP_TRY(ctx, hipMemsetAsync(ctx->dbg_flag, 0, sizeof(int32_t) * 2, ctx->stream)); }
    ReParams P = P0;
    P.flag = ctx->dbg_flag;
    const dim3 grid((unsigned)((ctx->R + 63) / 64)), blk(64);
    switch (re_slice_of(ctx)) {
        case RE_SK: hipLaunchKernelGGL(re_check_kernel<RE_SK>, grid, blk, 0, ctx->stream, P, cache ? 1 : 0); break;
        case RE_SKN: hipLaunchKernelGGL(re_check_kernel<RE_SKN>, grid, blk, 0, ctx->stream, P, cache ? 1 : 0); break;
        case RE_PSTEP: hipLaunchKernelGGL(re_check_kernel<RE_PSTEP>, grid, blk, 0, ctx->stream, P, cache ? 1 : 0); break;
        case RE_PLIN: hipLaunchKernelGGL(re_check_kernel<RE_PLIN>, grid, blk, 0, ctx->stream, P, cache ? 1 : 0); break;
        case RE_CSTEP: hipLaunchKernelGGL(re_check_kernel<RE_CSTEP>, grid, blk, 0, ctx->stream, P, cache ? 1 : 0); break;
        case RE_CRELU: hipLaunchKernelGGL(re_check_kernel<RE_CRELU>, grid, blk, 0, ctx->stream, P, cache ? 1 : 0); break;
        case RE_CQU: hipLaunchKernelGGL(re_check_kernel<RE_CQU>, grid, blk, 0, ctx->stream, P, cache ? 1 : 0); break;
        case RE_SAT: hipLaunchKernelGGL(re_check_kernel<RE_SAT>, grid, blk, 0, ctx->stream, P, cache ? 1 : 0); break;
        default: hipLaunchKernelGGL(re_check_kernel<RE_EMPTY>, grid, blk, 0, ctx->stream, P, cache ? 1 : 0); break;
    }
    HIP_TRY(ctx, hipGetLastError());
    return RRRMC_OK;
}

// rrrMC(X::DoubleGraph) (standard = false) or standardMC (standard = true) on a GraphRobustEnsemble
int32_t re_mc_async(rrrmc_ctx* ctx, bool standard, double beta, int64_t iters, int64_t step, double staged_thr, double staged_thr_fact)
{
    int32_t rc = RRRMC_OK;
    if (!ctx->re_params_set) return fail(ctx, RRRMC_ERR_STATE, "a GraphRobustEnsemble needs (γ, β): call rrrmc_re_set_params first");
    if (iters < 0) return fail(ctx, RRRMC_ERR_INVALID_ARG, "iters must be >= 0, given %lld", (long long)iters);
    if (step < 1) return fail(ctx, RRRMC_ERR_INVALID_ARG, "step must be >= 1, given %lld", (long long)step);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    ctx->results_valid = false; ctx->last_call_wtm = false; ctx->last_call_eo = false;
    ctx->timing_valid = false;
    SmpState S{};
    if (!standard) { rc = smp_begin(ctx, 1, beta, staged_thr, staged_thr_fact, 0.0, step, nullptr, &S); if (rc) return rc; }
    else S.samp0 = step;
    const int64_t nsamp = standard ? iters / step : smp_nsamp(ctx, iters, step);
    const size_t es_need = (size_t)(nsamp > 0 ? nsamp : 1) * ctx->R;
    if (es_need > ctx->sk_Es_cap) {
        free_dev(ctx->sk_Es);
        ctx->sk_Es_cap = 0;
        HIP_TRY(ctx, hipMalloc(&ctx->sk_Es, sizeof(double) * es_need));
        ctx->sk_Es_cap = es_need;
    }
    while (ctx->ev_sweep.size() < 2) {
        hipEvent_t e;
        HIP_TRY(ctx, hipEventCreate(&e));
        ctx->ev_sweep.push_back(e);
    }
    hipStream_t st = ctx->stream;
    HIP_TRY(ctx, hipEventRecord(ctx->ev_begin, st));
    ctx->stats_stride = 2;
    const bool cont = (standard && ctx->resume && ctx->std_cache_live) || S.resume;
    if (!cont) { rc = re_run_init(ctx, beta, !standard); if (rc) return rc; }
    else {
        rc = re_to_slices(ctx, re_params(ctx, beta));          // (the same bits the run left: nothing in between changed the configuration)
        if (rc) return rc;
        if (!standard) HIP_TRY(ctx, hipMemsetAsync(ctx->q_stats, 0, sizeof(int64_t) * (size_t)ctx->R * 2, st));
    }
    ReParams P = re_params(ctx, beta);
    P.staged_thr = staged_thr;
    P.lambda = staged_thr_fact / (double)ctx->N;              // RRRMC.jl:243
    P.g0 = ctx->it_done; P.iters = iters; P.step = step; P.samp0 = S.samp0;
    const int slice = re_slice_of(ctx);
    HIP_TRY(ctx, hipEventRecord(ctx->ev_sweep[0], st));
    if (standard) {
        switch (slice) {
            case RE_SK: hipLaunchKernelGGL(re_standard_kernel<RE_SK>, dim3(rrr_blocks(ctx->R)), dim3(rrr_tpb(ctx->R)), 0, st, P); break;
            case RE_SKN: hipLaunchKernelGGL(re_standard_kernel<RE_SKN>, dim3(rrr_blocks(ctx->R)), dim3(rrr_tpb(ctx->R)), 0, st, P); break;
            case RE_PSTEP: hipLaunchKernelGGL(re_standard_kernel<RE_PSTEP>, dim3(rrr_blocks(ctx->R)), dim3(rrr_tpb(ctx->R)), 0, st, P); break;
            case RE_PLIN: hipLaunchKernelGGL(re_standard_kernel<RE_PLIN>, dim3(rrr_blocks(ctx->R)), dim3(rrr_tpb(ctx->R)), 0, st, P); break;
            case RE_CSTEP: hipLaunchKernelGGL(re_standard_kernel<RE_CSTEP>, dim3(rrr_blocks(ctx->R)), dim3(rrr_tpb(ctx->R)), 0, st, P); break;
            case RE_CRELU: hipLaunchKernelGGL(re_standard_kernel<RE_CRELU>, dim3(rrr_blocks(ctx->R)), dim3(rrr_tpb(ctx->R)), 0, st, P); break;
            case RE_CQU: hipLaunchKernelGGL(re_standard_kernel<RE_CQU>, dim3(rrr_blocks(ctx->R)), dim3(rrr_tpb(ctx->R)), 0, st, P); break;
            case RE_SAT: hipLaunchKernelGGL(re_standard_kernel<RE_SAT>, dim3(rrr_blocks(ctx->R)), dim3(rrr_tpb(ctx->R)), 0, st, P); break;
            default: hipLaunchKernelGGL(re_standard_kernel<RE_EMPTY>, dim3(rrr_blocks(ctx->R)), dim3(rrr_tpb(ctx->R)), 0, st, P); break;
        }
    } else {
        // up to 2048 replicas: one replica per workgroup with its hot state in LDS (GraphSKRE(1024, 5): 1.25x the thread build at 128 and at
        // 1024 replicas); beyond, one thread per replica fills the chip better (1.6x at 4096; profiles/r07/re_skre.md).  RRRMC_RE_NO_LDS=1
        // forces the thread build, RRRMC_RE_LDS=1 the LDS build (timing experiments, the builds' parity test)
        size_t lds = re_rrr_lds_bytes(ctx->N, ctx->qW, ctx->qNk);
        if (P.pc.ds) lds = ((lds + 7) & ~(size_t)7) + perc_lds_bytes(P.pc.rows, P.pc.PW);
        if (P.cm.ds) lds = ((lds + 7) & ~(size_t)7) + comm_lds_bytes(P.cm.rows, P.cm.K2, P.cm.PW, slice == RE_CQU);          // the slices' Stabilities
        const char* no_lds = std::getenv("RRRMC_RE_NO_LDS");
        const char* want_lds = std::getenv("RRRMC_RE_LDS");
        // perceptron slices: the LDS build at every replica count (its update_cache! is spread over the wavefront; the thread build's is a
        // loop of P uncoalesced 16-bit updates: 5.8x slower at 4096 replicas of GraphPercStepRE(1001, 400, 5), profiles/r08/perc.md)
        const bool use_lds = lds <= (size_t)kLdsLimit && !(no_lds && no_lds[0] == '1') && (ctx->R <= 2048 || P.pc.ds || P.cm.ds || (want_lds && want_lds[0] == '1'));
        const re_kernel_fn fn = re_rrr_fn(slice, use_lds, P.L);
        if (use_lds) {
            HIP_TRY(ctx, raise_lds_attr(reinterpret_cast<const void*>(fn), lds));
            hipLaunchKernelGGL(fn, dim3((unsigned)ctx->R), dim3(kRrrThreads), lds, st, P);
        } else {
            hipLaunchKernelGGL(fn, dim3(rrr_blocks(ctx->R)), dim3(rrr_tpb(ctx->R)), 0, st, P);
        }
    }
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipEventRecord(ctx->ev_sweep[1], st));
    hipLaunchKernelGGL(re_from_slices_kernel, dim3((unsigned)((P.W + 255) / 256), (unsigned)P.R), dim3(256), 0, st, P);
    HIP_TRY(ctx, hipGetLastError());
    if (ctx->debug_checks) { rc = re_debug_check(ctx, P, !standard); if (rc) return rc; }
    HIP_TRY(ctx, hipEventRecord(ctx->ev_end, st));
    ctx->sweep_launches = 1;
    ctx->nsamp = nsamp;
    ctx->it_done += (uint64_t)iters;
    if (!standard) smp_commit(ctx, 1, iters);
    ctx->results_valid = true;
    ctx->timing_valid = true;
    ctx->last_call_rrr = true;          // accepted / staged counts live in q_stats
    ctx->q_cache_valid = !standard;
    ctx->std_cache_live = standard;
    return RRRMC_OK;
}

int32_t re_ctx_create(rrrmc_ctx** out, int64_t Nk, int64_t M, int32_t slice_kind, int64_t R, int32_t device, uint32_t replica0)
{
    if (!out) return fail(nullptr, RRRMC_ERR_INVALID_ARG, "out is NULL");
    *out = nullptr;
    const bool perc = slice_kind == RRRMC_RE_SLICE_PERC_STEP || slice_kind == RRRMC_RE_SLICE_PERC_LINEAR;
    const bool comm = slice_kind == RRRMC_RE_SLICE_COMM_STEP || slice_kind == RRRMC_RE_SLICE_COMM_RELU || slice_kind == RRRMC_RE_SLICE_COMM_QU;
    if (slice_kind != RRRMC_RE_SLICE_EMPTY && slice_kind != RRRMC_RE_SLICE_SK && slice_kind != RRRMC_RE_SLICE_SKN && slice_kind != RRRMC_RE_SLICE_SAT && !perc && !comm)
        return fail(nullptr, RRRMC_ERR_INVALID_ARG, "slice_kind must be RRRMC_RE_SLICE_EMPTY, _SK, _SKN, _PERC_STEP, _PERC_LINEAR, _COMM_STEP, _COMM_RELU, _SAT or _COMM_QU, given: %d", slice_kind);
    if (Nk < 1 || R < 1) return fail(nullptr, RRRMC_ERR_INVALID_ARG, "Nk and R must be >= 1");
    if (perc) { const int32_t rcn = perc_check_n(Nk); if (rcn) return rcn; }
    if (comm) { const int32_t rcn = comm_check_nk(Nk, slice_kind != RRRMC_RE_SLICE_COMM_STEP); if (rcn) return rcn; }
    if (M <= 2) return fail(nullptr, RRRMC_ERR_INVALID_ARG, "M must be greater than 2, given: %lld", (long long)M);      // RE.jl:37
    if (M > kReMmax) return fail(nullptr, RRRMC_ERR_UNSUPPORTED, "M = %lld: the Robust Ensemble kernels cover M <= %d", (long long)M, kReMmax);
    if (Nk * M > 65535) return fail(nullptr, RRRMC_ERR_UNSUPPORTED, "N = Nk*M = %lld is beyond the Robust Ensemble kernels (16-bit set members: N <= 65535)", (long long)(Nk * M));
    if (replica0 % 32) return fail(nullptr, RRRMC_ERR_INVALID_ARG, "replica0 must be a multiple of 32 (given %u)", replica0);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(nullptr, RRRMC_ERR_HIP, "no HIP device is visible: this library has no CPU path");
    if (device < 0 || device >= ndev) return fail(nullptr, RRRMC_ERR_INVALID_ARG, "device %d out of range (0..%d)", device, ndev - 1);
    rrrmc_ctx* ctx = new (std::nothrow) rrrmc_ctx();
    if (!ctx) return fail(nullptr, RRRMC_ERR_NOMEM, "out of host memory");
    ctx->model = slice_kind == RRRMC_RE_SLICE_SK ? RRRMC_MODEL_RE_SK : slice_kind == RRRMC_RE_SLICE_SKN ? RRRMC_MODEL_RE_SKN :
                 slice_kind == RRRMC_RE_SLICE_PERC_STEP ? RRRMC_MODEL_RE_PERC_STEP : slice_kind == RRRMC_RE_SLICE_PERC_LINEAR ? RRRMC_MODEL_RE_PERC_LINEAR :
                 slice_kind == RRRMC_RE_SLICE_COMM_STEP ? RRRMC_MODEL_RE_COMM_STEP : slice_kind == RRRMC_RE_SLICE_COMM_RELU ? RRRMC_MODEL_RE_COMM_RELU :
                 slice_kind == RRRMC_RE_SLICE_SAT ? RRRMC_MODEL_RE_SAT : slice_kind == RRRMC_RE_SLICE_COMM_QU ? RRRMC_MODEL_RE_COMM_QU : RRRMC_MODEL_RE_EMPTY;
    ctx->N = Nk * M; ctx->K = 0; ctx->R = R; ctx->Rpad = R;
    ctx->qNk = Nk; ctx->qM = M; ctx->qW = 2 * ((Nk * M + 63) / 64); ctx->q_Wk = 2 * ((Nk + 63) / 64);
    ctx->device = device; ctx->replica0 = replica0;
    ctx->graph_set = slice_kind == RRRMC_RE_SLICE_EMPTY;          // Graph0RE has no couplings to give
    const int64_t N = ctx->N, L = re_levels(M);
    ctx->re_htab.assign((size_t)(2 * M + 1), 0.0);
    ctx->re_hft.assign((size_t)L, 0.0);
#define RE_TRY(expr)                                                                                             \
    do {                                                                                                         \
        hipError_t e_ = (expr);                                                                                  \
        if (e_ != hipSuccess) {                                                                                  \
            int32_t rc_ = fail(nullptr, RRRMC_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_));           \
            rrrmc_ctx_destroy(ctx);                                                                              \
            return rc_;                                                                                          \
        }                                                                                                        \
    } while (0)
    RE_TRY(hipSetDevice(device));
    RE_TRY(hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking));
    RE_TRY(hipEventCreate(&ctx->ev_begin));
    RE_TRY(hipEventCreate(&ctx->ev_end));
    if (slice_kind == RRRMC_RE_SLICE_SKN) {
        RE_TRY(hipMalloc(&ctx->sk_J, sizeof(double) * Nk * Nk));
        RE_TRY(hipMalloc(&ctx->q_slf, sizeof(double) * (size_t)R * 2 * (size_t)M * (size_t)Nk));
        RE_TRY(hipMalloc(&ctx->q_smv, sizeof(int32_t) * (size_t)R * (size_t)M));
        RE_TRY(hipMalloc(&ctx->q_scur, (size_t)R * (size_t)M));
    } else if (slice_kind == RRRMC_RE_SLICE_SK) {
        RE_TRY(hipMalloc(&ctx->q_Jb, sizeof(uint32_t) * Nk * ctx->q_Wk));
    }
    RE_TRY(hipMalloc(&ctx->re_tab, sizeof(double) * (size_t)(2 * M + 1 + L)));
    RE_TRY(hipMalloc(&ctx->q_spins, sizeof(uint32_t) * R * ctx->qW));
    RE_TRY(hipMalloc(&ctx->re_sp, sizeof(uint32_t) * R * ctx->qW));
    RE_TRY(hipMalloc(&ctx->re_mu, (size_t)R * Nk));
    RE_TRY(hipMalloc(&ctx->q_cls, (size_t)R * N));
    RE_TRY(hipMalloc(reinterpret_cast<void**>(&ctx->q_sv), sizeof(uint16_t) * (size_t)R * 2 * L * N));
    RE_TRY(hipMalloc(reinterpret_cast<void**>(&ctx->q_spos), sizeof(uint16_t) * (size_t)R * N));
    RE_TRY(hipMalloc(&ctx->q_st, sizeof(int32_t) * R * 2 * L));
    RE_TRY(hipMalloc(&ctx->q_T, sizeof(double) * R * 2 * L));
    RE_TRY(hipMalloc(&ctx->q_z, sizeof(double) * R));
    RE_TRY(hipMalloc(&ctx->q_accrate, sizeof(double) * R));
    RE_TRY(hipMalloc(&ctx->q_stats, sizeof(int64_t) * R * 2));
    RE_TRY(hipMalloc(&ctx->sk_E, sizeof(double) * R));
    RE_TRY(hipMalloc(&ctx->re_Eslice, sizeof(double) * R * M));
    RE_TRY(hipMemset(ctx->q_spins, 0, sizeof(uint32_t) * R * ctx->qW));
#undef RE_TRY
    *out = ctx;
    return RRRMC_OK;
}
