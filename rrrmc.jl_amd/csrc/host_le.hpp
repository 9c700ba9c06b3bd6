// Host side of the Local Entropy ensemble (GraphLocalEntropy over GraphEmpty / binary GraphSK / GraphSKNormal slices, le_kernels.hpp).
// Included by rrrmc_hip.hip inside its anonymous namespace, after host_re.hpp; not a stand-alone translation unit.  The context reuses the
// Robust Ensemble's buffers (re_sp, re_mu, re_tab, re_Eslice and the q_* DeltaECache arrays) with M + 1 rows.
inline bool is_le(const rrrmc_ctx* ctx) { return ctx->model == RRRMC_MODEL_LE_EMPTY || ctx->model == RRRMC_MODEL_LE_SK || ctx->model == RRRMC_MODEL_LE_SKN ||
                                                ctx->model == RRRMC_MODEL_LE_PERC_STEP || ctx->model == RRRMC_MODEL_LE_PERC_LINEAR ||
                                                ctx->model == RRRMC_MODEL_LE_COMM_STEP || ctx->model == RRRMC_MODEL_LE_COMM_RELU || ctx->model == RRRMC_MODEL_LE_SAT ||
                                                ctx->model == RRRMC_MODEL_LE_COMM_QU; }
inline int le_slice_of(const rrrmc_ctx* ctx) { return ctx->model == RRRMC_MODEL_LE_SK || ctx->model == RRRMC_MODEL_TLE_SK ? RE_SK : ctx->model == RRRMC_MODEL_LE_SKN || ctx->model == RRRMC_MODEL_TLE_SKN ? RE_SKN :
                                                      ctx->model == RRRMC_MODEL_LE_PERC_STEP ? RE_PSTEP : ctx->model == RRRMC_MODEL_LE_PERC_LINEAR ? RE_PLIN :
                                                      ctx->model == RRRMC_MODEL_LE_COMM_STEP ? RE_CSTEP : ctx->model == RRRMC_MODEL_LE_COMM_RELU ? RE_CRELU : ctx->model == RRRMC_MODEL_LE_SAT || ctx->model == RRRMC_MODEL_TLE_SAT ? RE_SAT :
                                                      ctx->model == RRRMC_MODEL_LE_COMM_QU ? RE_CQU : RE_EMPTY; }
inline int le_levels(int64_t M) { return (int)(M % 2 == 0 ? M / 2 + 2 : (M + 1) / 2); }        // length of allΔE(GraphLE) (LE.jl:176-179)

// allΔE(GraphLE{M,γT}) (LE.jl:176-179): M even (0, 2|γT|, 4|γT|, 8|γT|, ..., 2M|γT|), M odd (2|γT|, 6|γT|, ..., 2M|γT|); Julia's integer
// factor times abs(γT)
void le_tables(int64_t M, double gT, double* dElist)
{
    const double ag = std::fabs(gT);
    if (M % 2 == 0) {
        dElist[0] = (double)0 * ag;
        dElist[1] = 2 * ag;
        for (int64_t d = 1; d <= M / 2; ++d) dElist[d + 1] = (double)(4 * d) * ag;
    } else {
        for (int64_t d = 1; d <= (M + 1) / 2; ++d) dElist[d - 1] = (double)(2 * (2 * d - 1)) * ag;
    }
}

// findk(ΔElist, dE) (DeltaE.jl:26-60) as its generated code runs: 1-based, a binary search down to ranges of fewer than 10 entries, which are
// scanned in ascending order; 0 = not found
int le_findk(const double* t, int imin, int imax, int i, double dE)
{
    if (imax - imin < 10) {
        for (int j = imin; j <= imax; ++j)
            if (dE == t[j - 1]) return j;
        return 0;
    }
    const double cE = t[i - 1];
    if (cE == dE) return i;
    if (cE < dE) return le_findk(t, i + 1, imax, (i + 1 + imax) / 2, dE);
    return le_findk(t, imin, i - 1, (imin + i - 1) / 2, dE);
}

// class codes of lfields = -M .. M: the level a = findk(ΔElist, 2γT lf) - 1, 0x40 when ΔE > 0, 0x80 when ΔE == 0 (DeltaE.jl:80-86).
// Values lfields never takes (the centre's has the parity of M, a replica's is ±1) may have no level: 0xFF.  Returns false when a value
// lfields does take has none (only for non-finite tables, which rrrmc_le_set_params refuses first).
bool le_codes(int64_t M, double gT, const double* dElist, uint8_t* code)
{
    const int L = le_levels(M);
    const double g2 = 2 * gT;
    for (int64_t lf = -M; lf <= M; ++lf) {
        const double dE = g2 * (double)lf;
        const int a = le_findk(dElist, 1, L, (1 + L) / 2, std::fabs(dE));
        const bool reach = lf == 1 || lf == -1 || ((lf - M) % 2 == 0);
        if (a == 0) {
            if (reach) return false;
            code[lf + M] = 0xFF;
            continue;
        }
        code[lf + M] = (uint8_t)((a - 1) | (dE > 0 ? 0x40 : 0) | (dE == 0 ? 0x80 : 0));
    }
    return true;
}

LeParams le_params(rrrmc_ctx* ctx, double beta)
{
    LeParams P{};
    const int64_t M = ctx->qM, L = le_levels(M);
    if (le_slice_of(ctx) == RE_SK) { P.Jb = ctx->q_Jb; P.Wk = (int)ctx->q_Wk; P.sN = std::sqrt((double)ctx->qNk); }
    if (le_slice_of(ctx) == RE_SKN) { P.Jd = ctx->sk_J; P.slf = ctx->q_slf; P.smv = ctx->q_smv; P.scur = ctx->q_scur; }
    if (le_slice_of(ctx) == RE_PSTEP || le_slice_of(ctx) == RE_PLIN) P.pc = perc_params(ctx, M + 1);
    if (le_slice_of(ctx) == RE_CSTEP || le_slice_of(ctx) == RE_CRELU || le_slice_of(ctx) == RE_CQU) P.cm = comm_params(ctx, M + 1);
    if (le_slice_of(ctx) == RE_SAT) P.sat = sat_table(ctx);
    P.tab = ctx->re_tab; P.etab = nullptr; P.ft = ctx->re_tab + L; P.ctab = reinterpret_cast<const uint8_t*>(ctx->re_tab + 2 * L);
    P.abi = ctx->q_spins; P.sp = ctx->re_sp; P.mu = ctx->re_mu; P.cls = ctx->q_cls; P.sv = ctx->q_sv; P.spos = ctx->q_spos; P.st = ctx->q_st;
    P.T = ctx->q_T; P.zz = ctx->q_z; P.E_cur = ctx->sk_E; P.acc_rate = ctx->q_accrate; P.stats = ctx->q_stats; P.Es = ctx->sk_Es;
    P.Eslice = ctx->re_Eslice; P.flag = ctx->dbg_flag; P.dist = ctx->le_dist;
    P.beta = beta;
    P.g2 = 2 * ctx->le_gT; P.gT = ctx->le_gT;
    P.k0 = (uint32_t)ctx->seed; P.k1 = (uint32_t)(ctx->seed >> 32); P.replica0 = ctx->replica0;
    P.Nk = (int)ctx->qNk; P.M = (int)(M + 1); P.Mr = (int)M; P.L = (int)L; P.N = (int)ctx->N; P.W = (int)ctx->qW; P.R = (int)ctx->R;
    return P;
}

// energy(X, C) and, for rrrMC, a fresh DeltaECache: the start of a reference call (src/RRRMC.jl:95, :236-238).  The class weights need the
// sampler's β: ft is uploaded here (stream-ordered behind earlier launches that read the previous values).
int32_t le_run_init(rrrmc_ctx* ctx, double beta, bool cache)
{
    const int L = le_levels(ctx->qM);
    for (int a = 0; a < L; ++a) ctx->re_hft[(size_t)a] = host_det_exp(-beta * ctx->re_htab[(size_t)a]);      // DeltaE.jl:91
    HIP_TRY(ctx, hipMemcpyAsync(ctx->re_tab + L, ctx->re_hft.data(), sizeof(double) * (size_t)L, hipMemcpyHostToDevice, ctx->stream));
    const LeParams P = le_params(ctx, beta);
    int32_t rc = re_to_slices(ctx, P);
    if (rc) return rc;
    switch (le_slice_of(ctx)) {
        case RE_SK: hipLaunchKernelGGL(le_init_kernel<RE_SK>, dim3((unsigned)ctx->R), dim3(kReInitThreads), 0, ctx->stream, P, cache ? 1 : 0); break;
        case RE_SKN: hipLaunchKernelGGL(le_init_kernel<RE_SKN>, dim3((unsigned)ctx->R), dim3(kReInitThreads), 0, ctx->stream, P, cache ? 1 : 0); break;
        case RE_PSTEP: hipLaunchKernelGGL(le_init_kernel<RE_PSTEP>, dim3((unsigned)ctx->R), dim3(kReInitThreads), 0, ctx->stream, P, cache ? 1 : 0); break;
        case RE_PLIN: hipLaunchKernelGGL(le_init_kernel<RE_PLIN>, dim3((unsigned)ctx->R), dim3(kReInitThreads), 0, ctx->stream, P, cache ? 1 : 0); break;
        case RE_CSTEP: hipLaunchKernelGGL(le_init_kernel<RE_CSTEP>, dim3((unsigned)ctx->R), dim3(kReInitThreads), 0, ctx->stream, P, cache ? 1 : 0); break;
        case RE_CRELU: hipLaunchKernelGGL(le_init_kernel<RE_CRELU>, dim3((unsigned)ctx->R), dim3(kReInitThreads), 0, ctx->stream, P, cache ? 1 : 0); break;
        case RE_CQU: hipLaunchKernelGGL(le_init_kernel<RE_CQU>, dim3((unsigned)ctx->R), dim3(kReInitThreads), 0, ctx->stream, P, cache ? 1 : 0); break;
        case RE_SAT: hipLaunchKernelGGL(le_init_kernel<RE_SAT>, dim3((unsigned)ctx->R), dim3(kReInitThreads), 0, ctx->stream, P, cache ? 1 : 0); break;
        default: hipLaunchKernelGGL(le_init_kernel<RE_EMPTY>, dim3((unsigned)ctx->R), dim3(kReInitThreads), 0, ctx->stream, P, cache ? 1 : 0); break;
    }
    HIP_TRY(ctx, hipGetLastError());
    return RRRMC_OK;
}

typedef void (*le_kernel_fn)(LeParams);
template <bool LDS, int SLICE> le_kernel_fn le_rrr_for_L(int L)
{
    if (L <= 2) return le_rrr_kernel<LDS, 2, SLICE>;
    if (L <= 4) return le_rrr_kernel<LDS, 4, SLICE>;
    if (L <= 8) return le_rrr_kernel<LDS, 8, SLICE>;
    return le_rrr_kernel<LDS, kLeLmax, SLICE>;
}
le_kernel_fn le_rrr_fn(int slice, bool lds, int L)
{
    switch (slice) {
        case RE_SK: return lds ? le_rrr_for_L<true, RE_SK>(L) : le_rrr_for_L<false, RE_SK>(L);
        case RE_SKN: return lds ? le_rrr_for_L<true, RE_SKN>(L) : le_rrr_for_L<false, RE_SKN>(L);
        case RE_PSTEP: return lds ? le_rrr_for_L<true, RE_PSTEP>(L) : le_rrr_for_L<false, RE_PSTEP>(L);
        case RE_PLIN: return lds ? le_rrr_for_L<true, RE_PLIN>(L) : le_rrr_for_L<false, RE_PLIN>(L);
        case RE_CSTEP: return lds ? le_rrr_for_L<true, RE_CSTEP>(L) : le_rrr_for_L<false, RE_CSTEP>(L);
        case RE_CRELU: return lds ? le_rrr_for_L<true, RE_CRELU>(L) : le_rrr_for_L<false, RE_CRELU>(L);
        case RE_CQU: return lds ? le_rrr_for_L<true, RE_CQU>(L) : le_rrr_for_L<false, RE_CQU>(L);
        case RE_SAT: return lds ? le_rrr_for_L<true, RE_SAT>(L) : le_rrr_for_L<false, RE_SAT>(L);
        default: return lds ? le_rrr_for_L<true, RE_EMPTY>(L) : le_rrr_for_L<false, RE_EMPTY>(L);
    }
}

// debug mode: the consistency check behind a sampler call (reported by the next sync, post_sync_checks)
int32_t le_debug_check(rrrmc_ctx* ctx, const LeParams& P0, bool cache)
{
    if (!ctx->dbg_flag) { HIP_TRY(ctx, hipMalloc(&ctx->dbg_flag, sizeof(int32_t) * 2)); HIP_TRY(ctx, hipMemsetAsync(ctx->dbg_flag, 0, sizeof(int32_t) * 2, ctx->stream)); }
    LeParams P = P0;
    P.flag = ctx->dbg_flag;
    const dim3 grid((unsigned)((ctx->R + 63) / 64)), blk(64);
    switch (le_slice_of(ctx)) {
        case RE_SK: hipLaunchKernelGGL(le_check_kernel<RE_SK>, grid, blk, 0, ctx->stream, P, cache ? 1 : 0); break;
        case RE_SKN: hipLaunchKernelGGL(le_check_kernel<RE_SKN>, grid, blk, 0, ctx->stream, P, cache ? 1 : 0); break;
        case RE_PSTEP: hipLaunchKernelGGL(le_check_kernel<RE_PSTEP>, grid, blk, 0, ctx->stream, P, cache ? 1 : 0); break;
        case RE_PLIN: hipLaunchKernelGGL(le_check_kernel<RE_PLIN>, grid, blk, 0, ctx->stream, P, cache ? 1 : 0); break;
        case RE_CSTEP: hipLaunchKernelGGL(le_check_kernel<RE_CSTEP>, grid, blk, 0, ctx->stream, P, cache ? 1 : 0); break;
        case RE_CRELU: hipLaunchKernelGGL(le_check_kernel<RE_CRELU>, grid, blk, 0, ctx->stream, P, cache ? 1 : 0); break;
        case RE_CQU: hipLaunchKernelGGL(le_check_kernel<RE_CQU>, grid, blk, 0, ctx->stream, P, cache ? 1 : 0); break;
        case RE_SAT: hipLaunchKernelGGL(le_check_kernel<RE_SAT>, grid, blk, 0, ctx->stream, P, cache ? 1 : 0); break;
        default: hipLaunchKernelGGL(le_check_kernel<RE_EMPTY>, grid, blk, 0, ctx->stream, P, cache ? 1 : 0); break;
    }
    HIP_TRY(ctx, hipGetLastError());
    return RRRMC_OK;
}

// rrrMC(X::DoubleGraph) (standard = false) or standardMC (standard = true) on a GraphLocalEntropy
int32_t le_mc_async(rrrmc_ctx* ctx, bool standard, double beta, int64_t iters, int64_t step, double staged_thr, double staged_thr_fact)
{
    int32_t rc = RRRMC_OK;
    if (!ctx->re_params_set) return fail(ctx, RRRMC_ERR_STATE, "a GraphLocalEntropy needs (γ, β): call rrrmc_le_set_params first");
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
    if (!cont) { rc = le_run_init(ctx, beta, !standard); if (rc) return rc; }
    else {
        rc = re_to_slices(ctx, le_params(ctx, beta));          // (the same bits the run left: nothing in between changed the configuration)
        if (rc) return rc;
        if (!standard) HIP_TRY(ctx, hipMemsetAsync(ctx->q_stats, 0, sizeof(int64_t) * (size_t)ctx->R * 2, st));
    }
    LeParams P = le_params(ctx, beta);
    P.staged_thr = staged_thr;
    P.lambda = staged_thr_fact / (double)ctx->N;              // RRRMC.jl:243
    P.g0 = ctx->it_done; P.iters = iters; P.step = step; P.samp0 = S.samp0;
    const int slice = le_slice_of(ctx);
    HIP_TRY(ctx, hipEventRecord(ctx->ev_sweep[0], st));
    if (standard) {
        switch (slice) {
            case RE_SK: hipLaunchKernelGGL(le_standard_kernel<RE_SK>, dim3(rrr_blocks(ctx->R)), dim3(rrr_tpb(ctx->R)), 0, st, P); break;
            case RE_SKN: hipLaunchKernelGGL(le_standard_kernel<RE_SKN>, dim3(rrr_blocks(ctx->R)), dim3(rrr_tpb(ctx->R)), 0, st, P); break;
            case RE_PSTEP: hipLaunchKernelGGL(le_standard_kernel<RE_PSTEP>, dim3(rrr_blocks(ctx->R)), dim3(rrr_tpb(ctx->R)), 0, st, P); break;
            case RE_PLIN: hipLaunchKernelGGL(le_standard_kernel<RE_PLIN>, dim3(rrr_blocks(ctx->R)), dim3(rrr_tpb(ctx->R)), 0, st, P); break;
            case RE_CSTEP: hipLaunchKernelGGL(le_standard_kernel<RE_CSTEP>, dim3(rrr_blocks(ctx->R)), dim3(rrr_tpb(ctx->R)), 0, st, P); break;
            case RE_CRELU: hipLaunchKernelGGL(le_standard_kernel<RE_CRELU>, dim3(rrr_blocks(ctx->R)), dim3(rrr_tpb(ctx->R)), 0, st, P); break;
            case RE_CQU: hipLaunchKernelGGL(le_standard_kernel<RE_CQU>, dim3(rrr_blocks(ctx->R)), dim3(rrr_tpb(ctx->R)), 0, st, P); break;
            case RE_SAT: hipLaunchKernelGGL(le_standard_kernel<RE_SAT>, dim3(rrr_blocks(ctx->R)), dim3(rrr_tpb(ctx->R)), 0, st, P); break;
            default: hipLaunchKernelGGL(le_standard_kernel<RE_EMPTY>, dim3(rrr_blocks(ctx->R)), dim3(rrr_tpb(ctx->R)), 0, st, P); break;
        }
    } else {
        // the build choice of re_mc_async (one replica per workgroup in LDS up to 2048 replicas, one thread per replica beyond);
        // RRRMC_LE_NO_LDS=1 forces the thread build, RRRMC_LE_LDS=1 the LDS build (timing experiments, the builds' parity test)
        size_t lds = le_rrr_lds_bytes(ctx->N, ctx->qW, ctx->qNk);
        if (P.pc.ds) lds = ((lds + 7) & ~(size_t)7) + perc_lds_bytes(P.pc.rows, P.pc.PW);
        if (P.cm.ds) lds = ((lds + 7) & ~(size_t)7) + comm_lds_bytes(P.cm.rows, P.cm.K2, P.cm.PW, slice == RE_CQU);          // the rows' Stabilities
        const char* no_lds = std::getenv("RRRMC_LE_NO_LDS");
        const char* want_lds = std::getenv("RRRMC_LE_LDS");
        // (perceptron slices: the LDS build at every replica count, as in re_mc_async)
        const bool use_lds = lds <= (size_t)kLdsLimit && !(no_lds && no_lds[0] == '1') && (ctx->R <= 2048 || P.pc.ds || P.cm.ds || (want_lds && want_lds[0] == '1'));
        const le_kernel_fn fn = le_rrr_fn(slice, use_lds, P.L);
        if (use_lds) {
            HIP_TRY(ctx, raise_lds_attr(reinterpret_cast<const void*>(fn), lds));
            hipLaunchKernelGGL(fn, dim3((unsigned)ctx->R), dim3(kRrrThreads), lds, st, P);
        } else {
            hipLaunchKernelGGL(fn, dim3(rrr_blocks(ctx->R)), dim3(rrr_tpb(ctx->R)), 0, st, P);
        }
    }
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipEventRecord(ctx->ev_sweep[1], st));
    hipLaunchKernelGGL(re_from_slices_kernel, dim3((unsigned)((P.W + 255) / 256), (unsigned)P.R), dim3(256), 0, st, static_cast<const ReParams&>(P));
    HIP_TRY(ctx, hipGetLastError());
    if (ctx->debug_checks) { rc = le_debug_check(ctx, P, !standard); if (rc) return rc; }
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

// LEenergies + cenergy (Eslice [R][M + 1]) and distances (le_dist [R][M][M]) of the current configuration, on the stream
int32_t le_observables(rrrmc_ctx* ctx)
{
    // read-only for a live run: the working copy is rewritten with the bits it already holds (every sampler call ends by writing it back)
    const LeParams P = le_params(ctx, 1.0);
    int32_t rc = re_to_slices(ctx, P);
    if (rc) return rc;
    const int64_t n = ctx->R * (ctx->qM + 1) + ctx->R * ctx->qM * ctx->qM;
    const dim3 grid((unsigned)((n + 63) / 64)), blk(64);
    switch (le_slice_of(ctx)) {
        case RE_SK: hipLaunchKernelGGL(le_obs_kernel<RE_SK>, grid, blk, 0, ctx->stream, P); break;
        case RE_SKN: hipLaunchKernelGGL(le_obs_kernel<RE_SKN>, grid, blk, 0, ctx->stream, P); break;
        case RE_PSTEP: hipLaunchKernelGGL(le_obs_kernel<RE_PSTEP>, grid, blk, 0, ctx->stream, P); break;
        case RE_PLIN: hipLaunchKernelGGL(le_obs_kernel<RE_PLIN>, grid, blk, 0, ctx->stream, P); break;
        case RE_CSTEP: hipLaunchKernelGGL(le_obs_kernel<RE_CSTEP>, grid, blk, 0, ctx->stream, P); break;
        case RE_CRELU: hipLaunchKernelGGL(le_obs_kernel<RE_CRELU>, grid, blk, 0, ctx->stream, P); break;
        case RE_CQU: hipLaunchKernelGGL(le_obs_kernel<RE_CQU>, grid, blk, 0, ctx->stream, P); break;
        case RE_SAT: hipLaunchKernelGGL(le_obs_kernel<RE_SAT>, grid, blk, 0, ctx->stream, P); break;
        default: hipLaunchKernelGGL(le_obs_kernel<RE_EMPTY>, grid, blk, 0, ctx->stream, P); break;
    }
    HIP_TRY(ctx, hipGetLastError());
    return RRRMC_OK;
}

int32_t le_ctx_create(rrrmc_ctx** out, int64_t Nk, int64_t M, int32_t slice_kind, int64_t R, int32_t device, uint32_t replica0)
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
    if (M <= 2) return fail(nullptr, RRRMC_ERR_INVALID_ARG, "M must be greater than 2, given: %lld", (long long)M);      // LE.jl:24
    if (M > kLeMmax) return fail(nullptr, RRRMC_ERR_UNSUPPORTED, "M = %lld: the Local Entropy kernels cover M <= %d", (long long)M, kLeMmax);
    if (Nk * (M + 1) > 65535)
        return fail(nullptr, RRRMC_ERR_UNSUPPORTED, "N = Nk*(M+1) = %lld is beyond the Local Entropy kernels (16-bit set members: N <= 65535)", (long long)(Nk * (M + 1)));
    if (replica0 % 32) return fail(nullptr, RRRMC_ERR_INVALID_ARG, "replica0 must be a multiple of 32 (given %u)", replica0);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(nullptr, RRRMC_ERR_HIP, "no HIP device is visible: this library has no CPU path");
    if (device < 0 || device >= ndev) return fail(nullptr, RRRMC_ERR_INVALID_ARG, "device %d out of range (0..%d)", device, ndev - 1);
    rrrmc_ctx* ctx = new (std::nothrow) rrrmc_ctx();
    if (!ctx) return fail(nullptr, RRRMC_ERR_NOMEM, "out of host memory");
    ctx->model = slice_kind == RRRMC_RE_SLICE_SK ? RRRMC_MODEL_LE_SK : slice_kind == RRRMC_RE_SLICE_SKN ? RRRMC_MODEL_LE_SKN :
                 slice_kind == RRRMC_RE_SLICE_PERC_STEP ? RRRMC_MODEL_LE_PERC_STEP : slice_kind == RRRMC_RE_SLICE_PERC_LINEAR ? RRRMC_MODEL_LE_PERC_LINEAR :
                 slice_kind == RRRMC_RE_SLICE_COMM_STEP ? RRRMC_MODEL_LE_COMM_STEP : slice_kind == RRRMC_RE_SLICE_COMM_RELU ? RRRMC_MODEL_LE_COMM_RELU :
                 slice_kind == RRRMC_RE_SLICE_SAT ? RRRMC_MODEL_LE_SAT : slice_kind == RRRMC_RE_SLICE_COMM_QU ? RRRMC_MODEL_LE_COMM_QU : RRRMC_MODEL_LE_EMPTY;
    const int64_t rows = M + 1, N = Nk * rows, L = le_levels(M);
    ctx->N = N; ctx->K = 0; ctx->R = R; ctx->Rpad = R;
    ctx->qNk = Nk; ctx->qM = M; ctx->qW = 2 * ((N + 63) / 64); ctx->q_Wk = 2 * ((Nk + 63) / 64);
    ctx->device = device; ctx->replica0 = replica0;
    ctx->graph_set = slice_kind == RRRMC_RE_SLICE_EMPTY;          // Graph0LE has no couplings to give
    // host tables: allΔE [L], then the class codes [2M + 1] (re_hft stages ft [L]); device: allΔE [L], ft [L], the codes
    const int64_t ncode_d = (2 * M + 1 + 7) / 8;
    ctx->re_htab.assign((size_t)L, 0.0);
    ctx->le_hcode.assign((size_t)(8 * ncode_d), 0xFF);
    ctx->re_hft.assign((size_t)L, 0.0);
#define LE_TRY(expr)                                                                                             \
    do {                                                                                                         \
        hipError_t e_ = (expr);                                                                                  \
        if (e_ != hipSuccess) {                                                                                  \
            int32_t rc_ = fail(nullptr, RRRMC_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_));           \
            rrrmc_ctx_destroy(ctx);                                                                              \
            return rc_;                                                                                          \
        }                                                                                                        \
    } while (0)
    LE_TRY(hipSetDevice(device));
    LE_TRY(hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking));
    LE_TRY(hipEventCreate(&ctx->ev_begin));
    LE_TRY(hipEventCreate(&ctx->ev_end));
    if (slice_kind == RRRMC_RE_SLICE_SKN) {
        LE_TRY(hipMalloc(&ctx->sk_J, sizeof(double) * Nk * Nk));
        LE_TRY(hipMalloc(&ctx->q_slf, sizeof(double) * (size_t)R * 2 * (size_t)rows * (size_t)Nk));
        LE_TRY(hipMalloc(&ctx->q_smv, sizeof(int32_t) * (size_t)R * (size_t)rows));
        LE_TRY(hipMalloc(&ctx->q_scur, (size_t)R * (size_t)rows));
    } else if (slice_kind == RRRMC_RE_SLICE_SK) {
        LE_TRY(hipMalloc(&ctx->q_Jb, sizeof(uint32_t) * Nk * ctx->q_Wk));
    }
    LE_TRY(hipMalloc(&ctx->re_tab, sizeof(double) * (size_t)(2 * L + ncode_d)));
    LE_TRY(hipMalloc(&ctx->q_spins, sizeof(uint32_t) * R * ctx->qW));
    LE_TRY(hipMalloc(&ctx->re_sp, sizeof(uint32_t) * R * ctx->qW));
    LE_TRY(hipMalloc(&ctx->re_mu, (size_t)R * Nk));
    LE_TRY(hipMalloc(&ctx->q_cls, (size_t)R * N));
    LE_TRY(hipMalloc(reinterpret_cast<void**>(&ctx->q_sv), sizeof(uint16_t) * (size_t)R * 2 * L * N));
    LE_TRY(hipMalloc(reinterpret_cast<void**>(&ctx->q_spos), sizeof(uint16_t) * (size_t)R * N));
    LE_TRY(hipMalloc(&ctx->q_st, sizeof(int32_t) * R * 2 * L));
    LE_TRY(hipMalloc(&ctx->q_T, sizeof(double) * R * 2 * L));
    LE_TRY(hipMalloc(&ctx->q_z, sizeof(double) * R));
    LE_TRY(hipMalloc(&ctx->q_accrate, sizeof(double) * R));
    LE_TRY(hipMalloc(&ctx->q_stats, sizeof(int64_t) * R * 2));
    LE_TRY(hipMalloc(&ctx->sk_E, sizeof(double) * R));
    LE_TRY(hipMalloc(&ctx->re_Eslice, sizeof(double) * R * rows));
    LE_TRY(hipMalloc(&ctx->le_dist, sizeof(int64_t) * R * M * M));
    LE_TRY(hipMemset(ctx->q_spins, 0, sizeof(uint32_t) * R * ctx->qW));
#undef LE_TRY
    *out = ctx;
    return RRRMC_OK;
}
