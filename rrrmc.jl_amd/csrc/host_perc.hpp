// Host side of the binary perceptron (perc_kernels.hpp): the stand-alone GraphPercStep / GraphPercLinear contexts under standardMC, and the
// pattern matrix and Stabilities that the Robust Ensemble and Local Entropy contexts with perceptron slices share with them.
// Included by rrrmc_hip.hip inside its anonymous namespace, before host_re.hpp; not a stand-alone translation unit.
inline bool is_perc(const rrrmc_ctx* ctx) { return ctx->model == RRRMC_MODEL_PERC_STEP || ctx->model == RRRMC_MODEL_PERC_LINEAR; }
inline bool perc_slices(const rrrmc_ctx* ctx)          // an ensemble over perceptron slices (ens_models.hpp), or a field wrapper over a perceptron (af_models.hpp)
{
    return model_slice(ctx->model) == RRRMC_RE_SLICE_PERC_STEP || model_slice(ctx->model) == RRRMC_RE_SLICE_PERC_LINEAR;
}

// GraphPercStep(ξ, ξv): isodd(N) || throw(ArgumentError) (PercStep.jl:57); the kernels' bound on N
int32_t perc_check_n(int64_t N)
{
    if (N % 2 == 0) return fail(nullptr, RRRMC_ERR_INVALID_ARG, "N must be odd, given: %lld", (long long)N);
    if (N > kPercNmax) return fail(nullptr, RRRMC_ERR_UNSUPPORTED, "N = %lld: the perceptron kernels cover N <= %d (16-bit stabilities)", (long long)N, kPercNmax);
    return RRRMC_OK;
}

PercParams perc_params(const rrrmc_ctx* ctx, int64_t rows)
{
    PercParams Q{};
    Q.col = ctx->pc_col; Q.row = ctx->pc_row; Q.ds = ctx->pc_ds; Q.pm = ctx->pc_pm; Q.mm = ctx->pc_mm;
    Q.P = (int)ctx->pc_P; Q.PW = (int)((ctx->pc_P + 63) / 64); Q.RW = (int)(2 * ((ctx->qNk + 63) / 64)); Q.rows = (int)rows;
    Q.sN = std::sqrt((double)ctx->qNk);
    return Q;
}

// rrrmc_set_patterns on one device: rows = chains' rows that carry Stabilities (1, M, or M + 1); chains = the chains Δs is sized for where
// that is not R (the tiles of xentr_kernels.hpp)
int32_t perc_set_patterns(rrrmc_ctx* ctx, const uint64_t* xi, int64_t P, int64_t rows, int64_t chains = 0)
{
    const int64_t Rc = chains ? chains : ctx->R;
    if (!xi) return fail(ctx, RRRMC_ERR_INVALID_ARG, "xi is NULL");
    if (P < 1) return fail(ctx, RRRMC_ERR_INVALID_ARG, "P must be >= 1, given: %lld", (long long)P);
    if (P > kPercPmax) return fail(ctx, RRRMC_ERR_UNSUPPORTED, "P = %lld: the perceptron kernels cover P <= %d", (long long)P, kPercPmax);
    const int64_t N = ctx->qNk, nch = (N + 63) / 64, PW = (P + 63) / 64;
    if (N % 64)
        for (int64_t a = 0; a < P; ++a)
            if (xi[a * nch + nch - 1] >> (N % 64)) return fail(ctx, RRRMC_ERR_INVALID_ARG, "pattern %lld: bits beyond N are set", (long long)a);
    std::vector<uint64_t> col((size_t)(N * PW), 0ull);          // the ξ representation of gen_ξ: one column per synapse
    for (int64_t a = 0; a < P; ++a)
        for (int64_t i = 0; i < N; ++i)
            col[(size_t)(i * PW + (a >> 6))] |= ((xi[a * nch + (i >> 6)] >> (i & 63)) & 1ull) << (a & 63);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (P != ctx->pc_P) {
        dev_free(ctx, ctx->pc_col); dev_free(ctx, ctx->pc_row); dev_free(ctx, ctx->pc_ds); dev_free(ctx, ctx->pc_pm); dev_free(ctx, ctx->pc_mm);
        ctx->pc_P = 0; ctx->graph_set = false;
        HIP_TRY(ctx, dev_alloc(ctx, ctx->pc_col, (size_t)(N * PW)));
        HIP_TRY(ctx, dev_alloc_bytes(ctx, ctx->pc_row, sizeof(uint64_t) * (size_t)(P * nch)));
        HIP_TRY(ctx, dev_alloc(ctx, ctx->pc_ds, (size_t)(Rc * rows * 64 * PW)));
        HIP_TRY(ctx, dev_alloc(ctx, ctx->pc_pm, (size_t)(Rc * rows * PW)));
        HIP_TRY(ctx, dev_alloc(ctx, ctx->pc_mm, (size_t)(Rc * rows * PW)));
        ctx->pc_P = P;
    }
    HIP_TRY(ctx, hipMemcpy(ctx->pc_col, col.data(), sizeof(uint64_t) * col.size(), hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemcpy(ctx->pc_row, xi, sizeof(uint64_t) * (size_t)(P * nch), hipMemcpyHostToDevice));     // chunk = two little-endian words
    ctx->std_cache_live = false;
    ctx->q_cache_valid = false;
    ctx->graph_set = true;
    return RRRMC_OK;
}

PercMcParams perc_mc_params(rrrmc_ctx* ctx, double beta)
{
    PercMcParams P{};
    P.pc = perc_params(ctx, 1);
    P.sp = ctx->q_spins; P.E_cur = ctx->sk_E; P.stats = ctx->q_stats; P.Es = ctx->sk_Es; P.flag = ctx->dbg_flag;
    P.beta = beta;
    P.k0 = (uint32_t)ctx->seed; P.k1 = (uint32_t)(ctx->seed >> 32); P.replica0 = ctx->replica0;
    P.N = (int)ctx->N; P.W = (int)ctx->qW; P.R = (int)ctx->R;
    return P;
}

// energy(X, C) into sk_E, and the Stabilities of every chain: the start of a reference call (src/RRRMC.jl:95)
int32_t perc_run_init(rrrmc_ctx* ctx)
{
    const PercMcParams P = perc_mc_params(ctx, 1.0);
    if (ctx->model == RRRMC_MODEL_PERC_LINEAR) hipLaunchKernelGGL(perc_init_kernel<true>, dim3((unsigned)ctx->R), dim3(kPercInitThreads), 0, ctx->stream, P);
    else hipLaunchKernelGGL(perc_init_kernel<false>, dim3((unsigned)ctx->R), dim3(kPercInitThreads), 0, ctx->stream, P);
    HIP_TRY(ctx, hipGetLastError());
    return RRRMC_OK;
}

// standardMC on a stand-alone GraphPercStep / GraphPercLinear
int32_t perc_mc_async(rrrmc_ctx* ctx, double beta, int64_t iters, int64_t step)
{
    if (iters < 0) return fail(ctx, RRRMC_ERR_INVALID_ARG, "iters must be >= 0, given %lld", (long long)iters);
    if (step < 1) return fail(ctx, RRRMC_ERR_INVALID_ARG, "step must be >= 1, given %lld", (long long)step);
    if (std::isnan(beta)) return fail(ctx, RRRMC_ERR_INVALID_ARG, "beta is NaN");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    ctx->results_valid = false; ctx->last_call_wtm = false; ctx->last_call_eo = false;
    ctx->timing_valid = false;
    const int64_t nsamp = iters / step;
    const size_t es_need = (size_t)(nsamp > 0 ? nsamp : 1) * ctx->R;
    HIP_TRY(ctx, dev_grow(ctx, ctx->sk_Es, ctx->sk_Es_cap, es_need));
    while (ctx->ev_sweep.size() < 2) {
        hipEvent_t e;
        HIP_TRY(ctx, hipEventCreate(&e));
        ctx->ev_sweep.push_back(e);
    }
    hipStream_t st = ctx->stream;
    HIP_TRY(ctx, hipEventRecord(ctx->ev_begin, st));
    ctx->stats_stride = 2;
    // a resumed call continues from the tracked energy and the live Stabilities (rrrmc_set_resume), as inside one reference call
    if (!(ctx->resume && ctx->std_cache_live)) { const int32_t rc = perc_run_init(ctx); if (rc) return rc; }
    PercMcParams P = perc_mc_params(ctx, beta);
    P.g0 = ctx->it_done; P.iters = iters; P.step = step; P.samp0 = step;
    const bool lin = ctx->model == RRRMC_MODEL_PERC_LINEAR;
    HIP_TRY(ctx, hipEventRecord(ctx->ev_sweep[0], st));
    if (lin) hipLaunchKernelGGL(perc_standard_kernel<true>, dim3(rrr_blocks(ctx->R)), dim3(rrr_tpb(ctx->R)), 0, st, P);
    else hipLaunchKernelGGL(perc_standard_kernel<false>, dim3(rrr_blocks(ctx->R)), dim3(rrr_tpb(ctx->R)), 0, st, P);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipEventRecord(ctx->ev_sweep[1], st));
    if (ctx->debug_checks) {
        if (!ctx->dbg_flag) { HIP_TRY(ctx, dev_alloc(ctx, ctx->dbg_flag, 2)); HIP_TRY(ctx, hipMemsetAsync(ctx->dbg_flag, 0, sizeof(int32_t) * 2, st)); }
        P.flag = ctx->dbg_flag;
        const dim3 grid((unsigned)((ctx->R + 63) / 64)), blk(64);
        if (lin) hipLaunchKernelGGL(perc_check_kernel<true>, grid, blk, 0, st, P);
        else hipLaunchKernelGGL(perc_check_kernel<false>, grid, blk, 0, st, P);
        HIP_TRY(ctx, hipGetLastError());
    }
    HIP_TRY(ctx, hipEventRecord(ctx->ev_end, st));
    ctx->sweep_launches = 1;
    ctx->nsamp = nsamp;
    ctx->it_done += (uint64_t)iters;
    ctx->results_valid = true;
    ctx->timing_valid = true;
    ctx->last_call_rrr = true;          // accepted counts live in q_stats
    ctx->std_cache_live = true;
    return RRRMC_OK;
}

int32_t perc_ctx_create(rrrmc_ctx** out, int64_t N, int32_t linear, int64_t R, int32_t device, uint32_t replica0)
{
    if (!out) return fail(nullptr, RRRMC_ERR_INVALID_ARG, "out is NULL");
    *out = nullptr;
    if (N < 1 || R < 1) return fail(nullptr, RRRMC_ERR_INVALID_ARG, "N and R must be >= 1");
    { const int32_t rcn = perc_check_n(N); if (rcn) return rcn; }
    if (replica0 % 32) return fail(nullptr, RRRMC_ERR_INVALID_ARG, "replica0 must be a multiple of 32 (given %u)", replica0);
    rrrmc_ctx* ctx = nullptr;
    { const int32_t rcb = ctx_create_begin(&ctx, device, false); if (rcb) return rcb; }
    ctx->model = linear ? RRRMC_MODEL_PERC_LINEAR : RRRMC_MODEL_PERC_STEP;
    ctx->N = N; ctx->K = 0; ctx->R = R; ctx->Rpad = R;
    ctx->qNk = N; ctx->qM = 1; ctx->qW = 2 * ((N + 63) / 64);
    ctx->replica0 = replica0;
    CTX_CREATE_TRY(ctx, false, dev_alloc(ctx, ctx->q_spins, R * ctx->qW));
    CTX_CREATE_TRY(ctx, false, dev_alloc(ctx, ctx->q_stats, R * 2));
    CTX_CREATE_TRY(ctx, false, dev_alloc(ctx, ctx->sk_E, R));
    CTX_CREATE_TRY(ctx, false, hipMemset(ctx->q_spins, 0, sizeof(uint32_t) * R * ctx->qW));
    *out = ctx;
    return RRRMC_OK;
}
