// Host side of the Robust Ensemble (GraphRobustEnsemble, re_kernels.hpp): its tables, kernel parameters, run start, debug check and the
// build choice and launch of a sampler call.  What it shares with the other two ensembles (the slice dispatcher, context creation, the
// frame of a sampler call) is in host_ens.hpp.  Included by rrrmc_hip.hip inside its anonymous namespace, after host_ens.hpp; not a
// stand-alone translation unit.

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
    const int slice = ens_slice(ctx->model);
    if (slice == RE_SK) { P.Jb = ctx->q_Jb; P.Wk = (int)ctx->q_Wk; P.sN = std::sqrt((double)ctx->qNk); }
    if (slice == RE_SKN) { P.Jd = ctx->sk_J; P.slf = ctx->q_slf; P.smv = ctx->q_smv; P.scur = ctx->q_scur; }
    if (slice == RE_PSTEP || slice == RE_PLIN) P.pc = perc_params(ctx, M);
    if (slice == RE_CSTEP || slice == RE_CRELU || slice == RE_CQU) P.cm = comm_params(ctx, M);
    if (slice == RE_SAT) P.sat = sat_table(ctx);
    if (slice == RE_SPF) ens_spf_params(ctx, &P);
    P.tab = ctx->re_tab; P.etab = ctx->re_tab + M; P.ft = ctx->re_tab + 2 * M + 1;
    P.abi = ctx->q_spins; P.sp = ctx->re_sp; P.mu = ctx->re_mu; P.cls = ctx->q_cls; P.sv = ctx->q_sv; P.spos = ctx->q_spos; P.st = ctx->q_st;
    P.T = ctx->q_T; P.zz = ctx->q_z; P.E_cur = ctx->sk_E; P.acc_rate = ctx->q_accrate; P.stats = ctx->q_stats; P.Es = ctx->sk_Es;
    P.Eslice = ctx->re_Eslice; P.flag = ctx->dbg_flag;
    P.beta = beta;
    P.k0 = (uint32_t)ctx->seed; P.k1 = (uint32_t)(ctx->seed >> 32); P.replica0 = ctx->replica0;
    P.Nk = (int)ctx->qNk; P.M = (int)M; P.L = re_levels(M); P.N = (int)ctx->N; P.W = (int)ctx->qW; P.R = (int)ctx->R;
    return P;
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
    const dim3 grid((unsigned)ctx->R), blk(kReInitThreads);
    if (!with_slice(AllSlices{}, ens_slice(ctx->model), [&](auto s) { hipLaunchKernelGGL(re_init_kernel<decltype(s)::value>, grid, blk, 0, ctx->stream, P, cache ? 1 : 0); }))
        return ens_bad_slice(ctx);
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
// nullptr: no such slice
re_kernel_fn re_rrr_fn(int slice, bool lds, int L)
{
    re_kernel_fn fn = nullptr;
    with_slice(AllSlices{}, slice, [&](auto s) { fn = lds ? re_rrr_for_L<true, decltype(s)::value>(L) : re_rrr_for_L<false, decltype(s)::value>(L); });
    return fn;
}

// debug mode: the consistency check behind a sampler call (reported by the next sync, post_sync_checks)
int32_t re_debug_check(rrrmc_ctx* ctx, const ReParams& P0, bool cache)
{
    const int32_t rc = dbg_flag_ensure(ctx);
    if (rc) return rc;
    ReParams P = P0;
    P.flag = ctx->dbg_flag;
    const dim3 grid((unsigned)((ctx->R + 63) / 64)), blk(64);
    if (!with_slice(AllSlices{}, ens_slice(ctx->model), [&](auto s) { hipLaunchKernelGGL(re_check_kernel<decltype(s)::value>, grid, blk, 0, ctx->stream, P, cache ? 1 : 0); }))
        return ens_bad_slice(ctx);
    HIP_TRY(ctx, hipGetLastError());
    return RRRMC_OK;
}

// rrrMC(X::DoubleGraph) (standard = false) or standardMC (standard = true) on a GraphRobustEnsemble
int32_t re_mc_async(rrrmc_ctx* ctx, bool standard, double beta, int64_t iters, int64_t step, double staged_thr, double staged_thr_fact)
{
    EnsCall C;
    int32_t rc = ens_call_begin(ctx, standard, beta, iters, step, staged_thr, staged_thr_fact, &C);
    if (rc) return rc;
    rc = C.cont ? ens_call_resume(ctx, re_params(ctx, beta), standard) : re_run_init(ctx, beta, !standard);
    if (rc) return rc;
    ReParams P = re_params(ctx, beta);
    ens_call_params(ctx, C, iters, step, staged_thr, staged_thr_fact, &P);
    const int slice = ens_slice(ctx->model);
    hipStream_t st = ctx->stream;
    HIP_TRY(ctx, hipEventRecord(ctx->ev_sweep[0], st));
    if (standard) {
        const dim3 grid(rrr_blocks(ctx->R)), blk(rrr_tpb(ctx->R));
        if (!with_slice(AllSlices{}, slice, [&](auto s) { hipLaunchKernelGGL(re_standard_kernel<decltype(s)::value>, grid, blk, 0, st, P); })) return ens_bad_slice(ctx);
    } else {
        // up to 2048 replicas: one replica per workgroup with its hot state in LDS (GraphSKRE(1024, 5): 1.25x the thread build at 128 and at
        // 1024 replicas); beyond, one thread per replica fills the chip better (1.6x at 4096; profiles/r07/re_skre.md).  RRRMC_RE_NO_LDS=1
        // forces the thread build, RRRMC_RE_LDS=1 the LDS build (timing experiments, the builds' parity test)
        size_t lds = re_rrr_lds_bytes(ctx->N, ctx->qW, ctx->qNk);
        if (P.pc.ds) lds = ((lds + 7) & ~(size_t)7) + perc_lds_bytes(P.pc.rows, P.pc.PW);
        if (P.cm.ds) lds = ((lds + 7) & ~(size_t)7) + comm_lds_bytes(P.cm.rows, P.cm.K2, P.cm.PW, slice == RE_CQU);          // the slices' Stabilities
        if (slice == RE_SPF) lds = ens_spf_lds(ctx, lds, ctx->qM, &P);          // the slices' LocalFields, when they fit too
        const char* no_lds = std::getenv("RRRMC_RE_NO_LDS");
        const char* want_lds = std::getenv("RRRMC_RE_LDS");
        // perceptron slices: the LDS build at every replica count (its update_cache! is spread over the wavefront; the thread build's is a
        // loop of P uncoalesced 16-bit updates: 5.8x slower at 4096 replicas of GraphPercStepRE(1001, 400, 5), profiles/r08/perc.md)
        const bool use_lds = lds <= (size_t)kLdsLimit && !(no_lds && no_lds[0] == '1') && (ctx->R <= 2048 || P.pc.ds || P.cm.ds || (want_lds && want_lds[0] == '1'));
        const re_kernel_fn fn = re_rrr_fn(slice, use_lds, P.L);
        if (!fn) return ens_bad_slice(ctx);
        if (use_lds) {
            HIP_TRY(ctx, raise_lds_attr(reinterpret_cast<const void*>(fn), lds));
            hipLaunchKernelGGL(fn, dim3((unsigned)ctx->R), dim3(kRrrThreads), lds, st, P);
        } else {
            hipLaunchKernelGGL(fn, dim3(rrr_blocks(ctx->R)), dim3(rrr_tpb(ctx->R)), 0, st, P);
        }
        ctx->ens_build = use_lds ? 1 : 2;
    }
    HIP_TRY(ctx, hipGetLastError());
    return ens_call_end(ctx, P, C, standard, iters, [&] { return re_debug_check(ctx, P, !standard); });
}
