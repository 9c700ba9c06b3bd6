// Host side of the binary committee machines (comm_kernels.hpp): the stand-alone GraphCommStep / GraphCommReLU / GraphCommQu contexts under
// standardMC,
// and the pattern matrix, labels and Stabilities that the Robust Ensemble and Local Entropy contexts with committee slices share with them.
// Included by rrrmc_hip.hip inside its anonymous namespace, before host_re.hpp; not a stand-alone translation unit.
inline bool is_comm(const rrrmc_ctx* ctx) { return ctx->model == RRRMC_MODEL_COMM_STEP || ctx->model == RRRMC_MODEL_COMM_RELU || ctx->model == RRRMC_MODEL_COMM_QU; }
inline bool comm_slices(const rrrmc_ctx* ctx)          // an ensemble over committee machine slices (ens_models.hpp), or a field wrapper over a committee machine (af_models.hpp)
{
    const int32_t s = model_slice(ctx->model);
    return s == RRRMC_RE_SLICE_COMM_STEP || s == RRRMC_RE_SLICE_COMM_RELU || s == RRRMC_RE_SLICE_COMM_QU;
}
inline bool comm_relu(const rrrmc_ctx* ctx)
{
    return ctx->model == RRRMC_MODEL_COMM_RELU || model_slice(ctx->model) == RRRMC_RE_SLICE_COMM_RELU ||
           (ctx->model == RRRMC_MODEL_QUANT_RRG && ctx->q_pat == RRRMC_RE_SLICE_COMM_RELU) || mixed_has(ctx, RRRMC_RE_SLICE_COMM_RELU);
}
inline bool comm_qu(const rrrmc_ctx* ctx)
{
    return ctx->model == RRRMC_MODEL_COMM_QU || model_slice(ctx->model) == RRRMC_RE_SLICE_COMM_QU ||
           (ctx->model == RRRMC_MODEL_QUANT_RRG && ctx->q_pat == RRRMC_RE_SLICE_COMM_QU) || mixed_has(ctx, RRRMC_RE_SLICE_COMM_QU);
}
// GraphCommReLU and GraphCommQu: K1, K2 even, labelled patterns
inline bool comm_labelled(const rrrmc_ctx* ctx) { return comm_relu(ctx) || comm_qu(ctx); }
inline int comm_kind(const rrrmc_ctx* ctx) { return comm_qu(ctx) ? CK_QU : comm_relu(ctx) ? CK_RELU : CK_STEP; }

// GraphCommStep(K2, ξ, ξv): isodd(K1), isodd(K2) (CommStep.jl:65-66); GraphCommReLU, GraphCommQu (relu = true): iseven (CommReLU.jl:68-69,
// CommQu.jl:72-73)
int32_t comm_check_k(rrrmc_ctx* ctx, int64_t K1, int64_t K2, bool relu)
{
    if (K1 < 1 || K2 < 1) return fail(ctx, RRRMC_ERR_INVALID_ARG, "K1 and K2 must be >= 1, given: %lld, %lld", (long long)K1, (long long)K2);
    const char* par = relu ? "even" : "odd";
    if ((K1 % 2 == 0) == !relu) return fail(ctx, RRRMC_ERR_INVALID_ARG, "K1 must be %s, given: %lld", par, (long long)K1);
    if ((K2 % 2 == 0) == !relu) return fail(ctx, RRRMC_ERR_INVALID_ARG, "K2 must be %s, given: %lld", par, (long long)K2);
    if (K1 * K2 > kCommNmax)
        return fail(ctx, RRRMC_ERR_UNSUPPORTED, "N = K1*K2 = %lld: the committee machine kernels cover N <= %d (16-bit stabilities)", (long long)(K1 * K2), kCommNmax);
    return RRRMC_OK;
}
// what an ensemble context can check before K2 is known: N = K1 K2 is odd (step) or a multiple of 4 (relu = true: ReLU, Qu), and the
// kernels' bound
int32_t comm_check_nk(int64_t N, bool relu)
{
    if (!relu && N % 2 == 0) return fail(nullptr, RRRMC_ERR_INVALID_ARG, "N = K1*K2 with K1, K2 odd must be odd, given: %lld", (long long)N);
    if (relu && N % 4 != 0) return fail(nullptr, RRRMC_ERR_INVALID_ARG, "N = K1*K2 with K1, K2 even must be a multiple of 4, given: %lld", (long long)N);
    if (N > kCommNmax) return fail(nullptr, RRRMC_ERR_UNSUPPORTED, "N = %lld: the committee machine kernels cover N <= %d (16-bit stabilities)", (long long)N, kCommNmax);
    return RRRMC_OK;
}

CommParams comm_params(const rrrmc_ctx* ctx, int64_t rows)
{
    CommParams Q{};
    Q.col = ctx->cm_col; Q.row = ctx->cm_row; Q.lab = ctx->cm_lab; Q.ds = ctx->cm_ds; Q.mk = ctx->cm_mk;
    Q.P = (int)ctx->cm_P; Q.PW = (int)((ctx->cm_P + 63) / 64); Q.RW = (int)(2 * ((ctx->qNk + 63) / 64)); Q.rows = (int)rows;
    Q.K2 = (int)ctx->cm_K2; Q.K1 = ctx->cm_K2 ? (int)(ctx->qNk / ctx->cm_K2) : 0;
    return Q;
}

// rrrmc_set_comm_patterns on one device: rows = chains' rows that carry Stabilities (1, M, or M + 1)
int32_t comm_set_patterns(rrrmc_ctx* ctx, int64_t K2, const uint64_t* xi, const uint64_t* y, int64_t P, int64_t rows)
{
    const bool relu = comm_labelled(ctx), qu = comm_qu(ctx);
    const int64_t N = ctx->qNk;
    if (!xi) return fail(ctx, RRRMC_ERR_INVALID_ARG, "xi is NULL");
    if (relu && !y) return fail(ctx, RRRMC_ERR_INVALID_ARG, "a %s needs the labels y", qu ? "GraphCommQu" : "GraphCommReLU");
    if (!relu && y) return fail(ctx, RRRMC_ERR_INVALID_ARG, "a GraphCommStep has no labels: y must be NULL");
    if (K2 < 1 || N % K2 != 0) return fail(ctx, RRRMC_ERR_INVALID_ARG, "N = %lld is not a multiple of K2 = %lld", (long long)N, (long long)K2);
    if ((is_comm(ctx) || ctx->model == RRRMC_MODEL_QUANT_RRG || af_family(ctx->model) != AF_NONE || is_mixed(ctx)) && K2 != ctx->cm_K2)
        return fail(ctx, RRRMC_ERR_INVALID_ARG, "K2 = %lld, but the context was made with K2 = %lld", (long long)K2, (long long)ctx->cm_K2);
    { const int32_t rck = comm_check_k(ctx, N / K2, K2, relu); if (rck) return rck; }
    if (P < 1) return fail(ctx, RRRMC_ERR_INVALID_ARG, "P must be >= 1, given: %lld", (long long)P);
    if (P > kCommPmax) return fail(ctx, RRRMC_ERR_UNSUPPORTED, "P = %lld: the committee machine kernels cover P <= %d", (long long)P, kCommPmax);
    const int64_t nch = (N + 63) / 64, PW = (P + 63) / 64;
    if (N % 64)
        for (int64_t a = 0; a < P; ++a)
            if (xi[a * nch + nch - 1] >> (N % 64)) return fail(ctx, RRRMC_ERR_INVALID_ARG, "pattern %lld: bits beyond N are set", (long long)a);
    if (relu && P % 64 && (y[PW - 1] >> (P % 64))) return fail(ctx, RRRMC_ERR_INVALID_ARG, "y: bits beyond P are set");
    std::vector<uint64_t> col((size_t)(N * PW), 0ull);          // the ξ representation of gen_ξ: one column per synapse
    for (int64_t a = 0; a < P; ++a)
        for (int64_t i = 0; i < N; ++i)
            col[(size_t)(i * PW + (a >> 6))] |= ((xi[a * nch + (i >> 6)] >> (i & 63)) & 1ull) << (a & 63);
    std::vector<uint64_t> lab((size_t)(2 * PW), 0ull);          // y, then ~y; both 0 beyond P
    if (relu)
        for (int64_t w = 0; w < PW; ++w) {
            const uint64_t valid = P - 64 * w >= 64 ? ~0ull : (1ull << (P - 64 * w)) - 1ull;
            lab[(size_t)w] = y[w] & valid;
            lab[(size_t)(PW + w)] = ~y[w] & valid;
        }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (P != ctx->cm_P || K2 != ctx->cm_K2 || !ctx->cm_col) {
        dev_free(ctx, ctx->cm_col); dev_free(ctx, ctx->cm_row); dev_free(ctx, ctx->cm_lab); dev_free(ctx, ctx->cm_ds); dev_free(ctx, ctx->cm_mk);
        ctx->cm_P = 0; ctx->graph_set = false;
        HIP_TRY(ctx, dev_alloc(ctx, ctx->cm_col, (size_t)(N * PW)));
        HIP_TRY(ctx, dev_alloc_bytes(ctx, ctx->cm_row, sizeof(uint64_t) * (size_t)(P * nch)));
        HIP_TRY(ctx, dev_alloc(ctx, ctx->cm_lab, (size_t)(2 * PW)));
        HIP_TRY(ctx, dev_alloc(ctx, ctx->cm_ds, (size_t)ctx->R * (size_t)rows * comm_ds_row((int)K2, (int)PW, qu)));
        HIP_TRY(ctx, dev_alloc(ctx, ctx->cm_mk, (size_t)ctx->R * (size_t)rows * comm_mk_row((int)K2, (int)PW, qu)));
        ctx->cm_P = P; ctx->cm_K2 = K2;
    }
    HIP_TRY(ctx, hipMemcpy(ctx->cm_col, col.data(), sizeof(uint64_t) * col.size(), hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemcpy(ctx->cm_row, xi, sizeof(uint64_t) * (size_t)(P * nch), hipMemcpyHostToDevice));     // chunk = two little-endian words
    HIP_TRY(ctx, hipMemcpy(ctx->cm_lab, lab.data(), sizeof(uint64_t) * lab.size(), hipMemcpyHostToDevice));
    ctx->std_cache_live = false;
    ctx->q_cache_valid = false;
    ctx->graph_set = true;
    return RRRMC_OK;
}

CommMcParams comm_mc_params(rrrmc_ctx* ctx, double beta)
{
    CommMcParams P{};
    P.cm = comm_params(ctx, 1);
    P.sp = ctx->q_spins; P.E_cur = ctx->sk_E; P.stats = ctx->q_stats; P.Es = ctx->sk_Es; P.flag = ctx->dbg_flag;
    P.beta = beta;
    P.k0 = (uint32_t)ctx->seed; P.k1 = (uint32_t)(ctx->seed >> 32); P.replica0 = ctx->replica0;
    P.N = (int)ctx->N; P.W = (int)ctx->qW; P.R = (int)ctx->R;
    return P;
}

// energy(X, C) into sk_E, and the Stabilities of every chain: the start of a reference call (src/RRRMC.jl:95)
int32_t comm_run_init(rrrmc_ctx* ctx)
{
    const CommMcParams P = comm_mc_params(ctx, 1.0);
    switch (comm_kind(ctx)) {
        case CK_QU: hipLaunchKernelGGL(comm_init_kernel<CK_QU>, dim3((unsigned)ctx->R), dim3(kCommInitThreads), 0, ctx->stream, P); break;
        case CK_RELU: hipLaunchKernelGGL(comm_init_kernel<CK_RELU>, dim3((unsigned)ctx->R), dim3(kCommInitThreads), 0, ctx->stream, P); break;
        default: hipLaunchKernelGGL(comm_init_kernel<CK_STEP>, dim3((unsigned)ctx->R), dim3(kCommInitThreads), 0, ctx->stream, P); break;
    }
    HIP_TRY(ctx, hipGetLastError());
    return RRRMC_OK;
}

// standardMC on a stand-alone GraphCommStep / GraphCommReLU (perc_mc_async's sequence)
int32_t comm_mc_async(rrrmc_ctx* ctx, double beta, int64_t iters, int64_t step)
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
    if (!(ctx->resume && ctx->std_cache_live)) { const int32_t rc = comm_run_init(ctx); if (rc) return rc; }
    CommMcParams P = comm_mc_params(ctx, beta);
    P.g0 = ctx->it_done; P.iters = iters; P.step = step; P.samp0 = step;
    const int kind = comm_kind(ctx);
    HIP_TRY(ctx, hipEventRecord(ctx->ev_sweep[0], st));
    switch (kind) {
        case CK_QU: hipLaunchKernelGGL(comm_standard_kernel<CK_QU>, dim3(rrr_blocks(ctx->R)), dim3(rrr_tpb(ctx->R)), 0, st, P); break;
        case CK_RELU: hipLaunchKernelGGL(comm_standard_kernel<CK_RELU>, dim3(rrr_blocks(ctx->R)), dim3(rrr_tpb(ctx->R)), 0, st, P); break;
        default: hipLaunchKernelGGL(comm_standard_kernel<CK_STEP>, dim3(rrr_blocks(ctx->R)), dim3(rrr_tpb(ctx->R)), 0, st, P); break;
    }
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipEventRecord(ctx->ev_sweep[1], st));
    if (ctx->debug_checks) {
        if (!ctx->dbg_flag) { HIP_TRY(ctx, dev_alloc(ctx, ctx->dbg_flag, 2)); HIP_TRY(ctx, hipMemsetAsync(ctx->dbg_flag, 0, sizeof(int32_t) * 2, st)); }
        P.flag = ctx->dbg_flag;
        const dim3 grid((unsigned)((ctx->R + 63) / 64)), blk(64);
        switch (kind) {
            case CK_QU: hipLaunchKernelGGL(comm_check_kernel<CK_QU>, grid, blk, 0, st, P); break;
            case CK_RELU: hipLaunchKernelGGL(comm_check_kernel<CK_RELU>, grid, blk, 0, st, P); break;
            default: hipLaunchKernelGGL(comm_check_kernel<CK_STEP>, grid, blk, 0, st, P); break;
        }
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

// kind: CK_STEP, CK_RELU or CK_QU
int32_t comm_ctx_create(rrrmc_ctx** out, int64_t K1, int64_t K2, int kind, int64_t R, int32_t device, uint32_t replica0)
{
    if (!out) return fail(nullptr, RRRMC_ERR_INVALID_ARG, "out is NULL");
    *out = nullptr;
    if (R < 1) return fail(nullptr, RRRMC_ERR_INVALID_ARG, "R must be >= 1");
    { const int32_t rck = comm_check_k(nullptr, K1, K2, kind != CK_STEP); if (rck) return rck; }
    if (replica0 % 32) return fail(nullptr, RRRMC_ERR_INVALID_ARG, "replica0 must be a multiple of 32 (given %u)", replica0);
    rrrmc_ctx* ctx = nullptr;
    { const int32_t rcb = ctx_create_begin(&ctx, device, false); if (rcb) return rcb; }
    const int64_t N = K1 * K2;
    ctx->model = kind == CK_QU ? RRRMC_MODEL_COMM_QU : kind == CK_RELU ? RRRMC_MODEL_COMM_RELU : RRRMC_MODEL_COMM_STEP;
    ctx->N = N; ctx->K = 0; ctx->R = R; ctx->Rpad = R;
    ctx->qNk = N; ctx->qM = 1; ctx->qW = 2 * ((N + 63) / 64);
    ctx->cm_K2 = K2;
    ctx->replica0 = replica0;
    CTX_CREATE_TRY(ctx, false, dev_alloc(ctx, ctx->q_spins, R * ctx->qW));
    CTX_CREATE_TRY(ctx, false, dev_alloc(ctx, ctx->q_stats, R * 2));
    CTX_CREATE_TRY(ctx, false, dev_alloc(ctx, ctx->sk_E, R));
    CTX_CREATE_TRY(ctx, false, hipMemset(ctx->q_spins, 0, sizeof(uint32_t) * R * ctx->qW));
    *out = ctx;
    return RRRMC_OK;
}
