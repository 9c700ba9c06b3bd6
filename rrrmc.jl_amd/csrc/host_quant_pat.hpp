// Host side of GraphQuant over pattern-machine slices (quant_pat_kernels.hpp): GraphQPercStepT / GraphQPercLinearT / GraphQCommStepT /
// GraphQCommReLUT / GraphQCommQuT.  The context is a RRRMC_MODEL_QUANT_RRG context (quant_ctx_create) whose q_pat names the slice kind; patterns, labels and
// the slices' Stabilities live in the perceptron / committee buffers (host_perc.hpp, host_comm.hpp) with rows = M.
// Included by rrrmc_hip.hip inside its anonymous namespace, after host_comm.hpp; not a stand-alone translation unit.
inline bool quant_pat(const rrrmc_ctx* ctx) { return ctx->model == RRRMC_MODEL_QUANT_RRG && ctx->q_pat != 0; }
inline bool quant_pat_perc(const rrrmc_ctx* ctx) { return quant_pat(ctx) && (ctx->q_pat == RRRMC_RE_SLICE_PERC_STEP || ctx->q_pat == RRRMC_RE_SLICE_PERC_LINEAR); }
inline bool quant_pat_comm(const rrrmc_ctx* ctx) { return quant_pat(ctx) && (ctx->q_pat == RRRMC_RE_SLICE_COMM_STEP || ctx->q_pat == RRRMC_RE_SLICE_COMM_RELU || ctx->q_pat == RRRMC_RE_SLICE_COMM_QU); }

QuantPatParams quant_pat_params(const rrrmc_ctx* ctx)
{
    QuantPatParams Q{};
    if (quant_pat_perc(ctx)) Q.pc = perc_params(ctx, ctx->qM);
    else Q.cm = comm_params(ctx, ctx->qM);
    Q.flag = ctx->dbg_flag; Q.Eslice = ctx->re_Eslice;
    return Q;
}

// one launch of a kernel template over the five slice kinds
#define QUANT_PAT_LAUNCH(ctx, KERNEL, grid, block, lds, ...)                                                                        \
    do {                                                                                                                            \
        switch ((ctx)->q_pat) {                                                                                                     \
            case RRRMC_RE_SLICE_PERC_STEP: hipLaunchKernelGGL(KERNEL<QP_PSTEP>, grid, block, lds, (ctx)->stream, __VA_ARGS__); break;   \
            case RRRMC_RE_SLICE_PERC_LINEAR: hipLaunchKernelGGL(KERNEL<QP_PLIN>, grid, block, lds, (ctx)->stream, __VA_ARGS__); break;  \
            case RRRMC_RE_SLICE_COMM_STEP: hipLaunchKernelGGL(KERNEL<QP_CSTEP>, grid, block, lds, (ctx)->stream, __VA_ARGS__); break;   \
            case RRRMC_RE_SLICE_COMM_QU: hipLaunchKernelGGL(KERNEL<QP_CQU>, grid, block, lds, (ctx)->stream, __VA_ARGS__); break;       \
            default: hipLaunchKernelGGL(KERNEL<QP_CRELU>, grid, block, lds, (ctx)->stream, __VA_ARGS__); break;                         \
        }                                                                                                                           \
        HIP_TRY(ctx, hipGetLastError());                                                                                            \
    } while (0)

// energy(X, C) + gen_ΔEcache + the slices' Stabilities (quant_run_init's job for these slices)
int32_t quant_pat_run_init(rrrmc_ctx* ctx, const RrrParams& P)
{
    const size_t lds = (size_t)ctx->qM * sizeof(long long);
    if (lds > 32768) return fail(ctx, RRRMC_ERR_UNSUPPORTED, "M = %lld slices exceed the init kernel's LDS", (long long)ctx->qM);
    const QuantPatParams Q = quant_pat_params(ctx);
    QUANT_PAT_LAUNCH(ctx, quant_pat_init_kernel, dim3((unsigned)ctx->R), dim3(kInitThreads), lds, P, Q);
    return RRRMC_OK;
}

// The build a sampler call on this context runs, by the rule of the other GraphQuants (quant_mc_async): few replicas get one WAVEFRONT per
// replica — 2 with the slices' Stabilities staged in LDS when they fit the 160 KB next to the kernel's own arrays, 1 with them in HBM/L2 —,
// many (or RRRMC_QUANT_NO_WAVE=1) one thread per replica (0).  RRRMC_QUANT_WAVE_MAX_R moves the bound, RRRMC_QUANT_NO_LDS=1 forbids the staging.
// GraphCommQu slices: the bound is 16384, the last measured count at which the wave build the rule picks still wins both samplers.  On
// GraphQCommQuT(250, 4, 400, 5) the staged wave build runs rrrMC 3.8x faster than the thread build at 4096 replicas and 1.36x at 16 384; at
// 32 768 the two are level in rrrMC (standardMC: 1.9x still).  Nothing between 16 384 and 32 768 was measured (profiles/r13/comm_qu.md).
// *lds_out = the dynamic LDS of the wave builds.
int quant_pat_build(const rrrmc_ctx* ctx, bool standard, size_t* lds_out)
{
    const char* no_wave = std::getenv("RRRMC_QUANT_NO_WAVE");
    const char* no_lds = std::getenv("RRRMC_QUANT_NO_LDS");
    int64_t wave_max_R = ctx->q_pat == RRRMC_RE_SLICE_COMM_QU ? 16384 : 2048;
    if (const char* e = std::getenv("RRRMC_QUANT_WAVE_MAX_R")) wave_max_R = std::atoll(e);
    const int64_t PW = ((quant_pat_perc(ctx) ? ctx->pc_P : ctx->cm_P) + 63) / 64;
    const size_t base = standard ? sizeof(uint32_t) * (size_t)ctx->qW : rrr_quant_lds_bytes(ctx->N, ctx->qW, ctx->qNk, 0);
    const size_t stage = quant_pat_stage_bytes(quant_pat_perc(ctx), ctx->qM, ctx->cm_K2, PW, ctx->q_pat == RRRMC_RE_SLICE_COMM_QU);
    *lds_out = base;
    if ((no_wave && no_wave[0] == '1') || ctx->R > wave_max_R || base > (size_t)kLdsLimit) return 0;
    if ((no_lds && no_lds[0] == '1') || base + stage > (size_t)kLdsLimit) return 1;
    *lds_out = base + stage;
    return 2;
}

typedef void (*quant_pat_fn)(RrrParams, QuantPatParams);
template <int KIND> quant_pat_fn quant_pat_kernel_of(bool standard, int build)
{
    if (standard) return build == 2 ? quant_standard_pat_wave_kernel<KIND, true> : build == 1 ? quant_standard_pat_wave_kernel<KIND, false> : quant_standard_pat_kernel<KIND>;
    return build == 2 ? rrr_quant_pat_wave_kernel<KIND, true> : build == 1 ? rrr_quant_pat_wave_kernel<KIND, false> : rrr_quant_pat_kernel<KIND>;
}

// the sampler kernel of quant_mc_async
int32_t quant_pat_launch(rrrmc_ctx* ctx, bool standard, const RrrParams& P)
{
    const QuantPatParams Q = quant_pat_params(ctx);
    size_t lds = 0;
    const int build = quant_pat_build(ctx, standard, &lds);
    const quant_pat_fn fn = ctx->q_pat == RRRMC_RE_SLICE_PERC_STEP     ? quant_pat_kernel_of<QP_PSTEP>(standard, build)
                            : ctx->q_pat == RRRMC_RE_SLICE_PERC_LINEAR ? quant_pat_kernel_of<QP_PLIN>(standard, build)
                            : ctx->q_pat == RRRMC_RE_SLICE_COMM_STEP   ? quant_pat_kernel_of<QP_CSTEP>(standard, build)
                            : ctx->q_pat == RRRMC_RE_SLICE_COMM_QU     ? quant_pat_kernel_of<QP_CQU>(standard, build)
                                                                       : quant_pat_kernel_of<QP_CRELU>(standard, build);
    if (build == 0) {
        hipLaunchKernelGGL(fn, dim3(rrr_blocks(ctx->R)), dim3(rrr_tpb(ctx->R)), 0, ctx->stream, P, Q);
    } else {
        HIP_TRY(ctx, raise_lds_attr(reinterpret_cast<const void*>(fn), lds));
        hipLaunchKernelGGL(fn, dim3((unsigned)ctx->R), dim3(kRrrThreads), lds, ctx->stream, P, Q);
    }
    HIP_TRY(ctx, hipGetLastError());
    ctx->q_pat_build = build;
    return RRRMC_OK;
}

// debug mode: Stabilities, masks and E recomputed after the call (reported by the next sync, post_sync_checks)
int32_t quant_pat_check(rrrmc_ctx* ctx, const RrrParams& P)
{
    if (!ctx->dbg_flag) { HIP_TRY(ctx, dev_alloc(ctx, ctx->dbg_flag, 2)); HIP_TRY(ctx, hipMemsetAsync(ctx->dbg_flag, 0, sizeof(int32_t) * 2, ctx->stream)); }
    const QuantPatParams Q = quant_pat_params(ctx);
    QUANT_PAT_LAUNCH(ctx, quant_pat_check_kernel, dim3((unsigned)((ctx->R + 63) / 64)), dim3(64), 0, P, Q);
    return RRRMC_OK;
}

// energy(X1[k], C1[k]) of every slice of the live configuration into re_Eslice [R][M] (queued on the context's stream)
int32_t quant_pat_energies(rrrmc_ctx* ctx)
{
    if (!ctx->re_Eslice) HIP_TRY(ctx, dev_alloc(ctx, ctx->re_Eslice, (size_t)(ctx->R * ctx->qM)));
    const QuantPatParams Q = quant_pat_params(ctx);
    QUANT_PAT_LAUNCH(ctx, quant_pat_energies_kernel, dim3((unsigned)((ctx->R * ctx->qM + 63) / 64)), dim3(64), 0, Q, ctx->q_spins, (int)ctx->qNk, (int)ctx->qM, (int)ctx->qW, (int)ctx->R);
    return RRRMC_OK;
}

int32_t quant_ctx_create(rrrmc_ctx** out, int64_t Nk, int64_t K, int64_t M, int64_t R, int32_t device, uint32_t replica0, bool sk, bool skn, bool spf, int32_t pat);
int32_t quant_pat_ctx_create(rrrmc_ctx** out, int32_t slice_kind, int64_t Nk, int64_t K2, int64_t M, int64_t R, int32_t device, uint32_t replica0)
{
    if (!out) return fail(nullptr, RRRMC_ERR_INVALID_ARG, "out is NULL");
    *out = nullptr;
    if ((slice_kind < RRRMC_RE_SLICE_PERC_STEP || slice_kind > RRRMC_RE_SLICE_COMM_RELU) && slice_kind != RRRMC_RE_SLICE_COMM_QU)
        return fail(nullptr, RRRMC_ERR_INVALID_ARG, "slice_kind must be RRRMC_RE_SLICE_PERC_STEP / _PERC_LINEAR / _COMM_STEP / _COMM_RELU / _COMM_QU, given: %d", slice_kind);
    if (Nk < 1 || R < 1) return fail(nullptr, RRRMC_ERR_INVALID_ARG, "Nk and R must be >= 1");
    const bool comm = slice_kind >= RRRMC_RE_SLICE_COMM_STEP;
    if (comm) {
        if (K2 < 1 || Nk % K2 != 0) return fail(nullptr, RRRMC_ERR_INVALID_ARG, "Nk = %lld is not a multiple of K2 = %lld", (long long)Nk, (long long)K2);
        const int32_t rck = comm_check_k(nullptr, Nk / K2, K2, slice_kind != RRRMC_RE_SLICE_COMM_STEP);
        if (rck) return rck;
    } else {
        const int32_t rcn = perc_check_n(Nk);
        if (rcn) return rcn;
    }
    if (M <= 2) return fail(nullptr, RRRMC_ERR_INVALID_ARG, "M must be greater than 2, given: %lld", (long long)M);   // QT.jl:47
    if (Nk * M > 65535) return fail(nullptr, RRRMC_ERR_UNSUPPORTED, "N = Nk*M = %lld: GraphQuant over pattern machines covers N <= 65535", (long long)(Nk * M));
    const int32_t rc = quant_ctx_create(out, Nk, 0, M, R, device, replica0, false, false, false, slice_kind);
    if (rc) return rc;
    (*out)->cm_K2 = comm ? K2 : 0;
    return RRRMC_OK;
}
