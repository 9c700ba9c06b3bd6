// Host side of the cross-entropy perceptron (xentr_kernels.hpp): the stand-alone GraphPercXEntr contexts under standardMC, the loss table,
// step_energy, and what the field wrappers over it (host_af.hpp) share with them.  The patterns are the perceptrons' (perc_set_patterns).
// Included by rrrmc_hip.hip inside its anonymous namespace, after host_perc.hpp and before host_af.hpp; not a stand-alone translation unit.
inline bool is_xentr(const rrrmc_ctx* ctx) { return ctx->model == RRRMC_MODEL_PERC_XENTR; }
inline bool xentr_slices(const rrrmc_ctx* ctx) { return model_slice(ctx->model) == RRRMC_RE_SLICE_PERC_XENTR; }          // a field wrapper over it

XentrParams xentr_params(const rrrmc_ctx* ctx)
{
    XentrParams X{};
    X.Hs = ctx->xe_Hs; X.term = ctx->xe_term; X.hmax = ctx->xe_hmax; X.N = (int)ctx->qNk;
    return X;
}

// rrrmc_set_patterns on a stand-alone context: Δs in tiles of 64 chains
int32_t xentr_set_patterns(rrrmc_ctx* ctx, const uint64_t* xi, int64_t P)
{
    const int32_t rc = perc_set_patterns(ctx, xi, P, 1, 64 * ((ctx->R + 63) / 64));
    if (rc) return rc;
    ctx->graph_set = ctx->xe_table_set;
    return RRRMC_OK;
}

// rrrmc_set_loss_table on one device.  A non-finite entry is refused: the reference would carry Inf − Inf = NaN into accept
int32_t xentr_set_table(rrrmc_ctx* ctx, const double* Hs, int64_t n)
{
    if (!Hs) return fail(ctx, RRRMC_ERR_INVALID_ARG, "Hs is NULL");
    if (n != ctx->qNk + 1) return fail(ctx, RRRMC_ERR_INVALID_ARG, "the loss table has N + 1 = %lld entries (Δ = -N:2:N), given: %lld", (long long)(ctx->qNk + 1), (long long)n);
    double hmax = 0.0;
    for (int64_t k = 0; k < n; ++k) {
        if (!std::isfinite(Hs[k])) return fail(ctx, RRRMC_ERR_INVALID_ARG, "the loss table must be finite, found: Hs[%lld] = %g", (long long)k, Hs[k]);
        hmax = std::max(hmax, std::fabs(Hs[k]));
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (!ctx->xe_Hs) HIP_TRY(ctx, dev_alloc(ctx, ctx->xe_Hs, (size_t)n));
    HIP_TRY(ctx, hipMemcpy(ctx->xe_Hs, Hs, sizeof(double) * (size_t)n, hipMemcpyHostToDevice));
    ctx->xe_hmax = hmax;
    ctx->xe_table_set = true;
    ctx->std_cache_live = false;          // the tracked energy was the old table's: the next call starts from energy(X, C)
    ctx->q_cache_valid = false;
    ctx->graph_set = ctx->pc_P > 0;
    return RRRMC_OK;
}

XentrMcParams xentr_mc_params(rrrmc_ctx* ctx, double beta)
{
    XentrMcParams P{};
    P.pc = perc_params(ctx, 1);
    P.xe = xentr_params(ctx);
    P.sp = ctx->q_spins; P.E_cur = ctx->sk_E; P.stats = ctx->q_stats; P.Es = ctx->sk_Es; P.nacc = ctx->xe_nacc; P.flag = ctx->dbg_flag;
    P.beta = beta;
    P.k0 = (uint32_t)ctx->seed; P.k1 = (uint32_t)(ctx->seed >> 32); P.replica0 = ctx->replica0;
    P.N = (int)ctx->N; P.W = (int)ctx->qW; P.R = (int)ctx->R;
    return P;
}

// energy(X, C) into sk_E, and the stabilities of every chain: the start of a reference call (src/RRRMC.jl:95)
int32_t xentr_run_init(rrrmc_ctx* ctx)
{
    const XentrMcParams P = xentr_mc_params(ctx, 1.0);
    hipLaunchKernelGGL(xentr_init_kernel, dim3((unsigned)ctx->R), dim3(kXentrInitThreads), 0, ctx->stream, P);
    HIP_TRY(ctx, hipGetLastError());
    return RRRMC_OK;
}

// Which build runs R chains: the wavefront-per-chain kernel up to kXentrWaveMaxR chains, the thread-per-chain kernel beyond.  The bound is
// the largest measured chain count at which the wave build is ahead on GraphPercXEntr(1001, 400, λ): it leads at all four counts measured,
// 8 .. 32 768 (profiles/r17/perc_xentr.md), and the ratio shrinks with the count — no crossing was seen, so nothing beyond the last
// measured count is claimed for it.  RRRMC_XENTR_NO_WAVE=1 forces the thread build, RRRMC_XENTR_WAVE=1 the wave build (timing
// experiments, the builds' parity tests).
constexpr int64_t kXentrWaveMaxR = 32768;
inline bool xentr_use_wave(int64_t R)
{
    const char* no_wave = std::getenv("RRRMC_XENTR_NO_WAVE");
    const char* want_wave = std::getenv("RRRMC_XENTR_WAVE");
    return !(no_wave && no_wave[0] == '1') && (R <= kXentrWaveMaxR || (want_wave && want_wave[0] == '1'));
}
// The wave build stages the loss table in LDS only up to this many chains: the largest measured count at which staging is ahead (1.04 and 1.05
// times at 8 and at 512 chains of N = 1001; at 4096 and 32 768 the table's 8 KiB per wavefront cap the resident wavefronts and the global-memory
// table leads 1.17 and 1.27 times, profiles/r17/perc_xentr.md)
constexpr int64_t kXentrWaveTableLdsMaxR = 512;
inline bool xentr_no_lds() { const char* e = std::getenv("RRRMC_XENTR_NO_LDS"); return e && e[0] == '1'; }

// standardMC on a stand-alone GraphPercXEntr
int32_t xentr_mc_async(rrrmc_ctx* ctx, double beta, int64_t iters, int64_t step)
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
    // a resumed call continues from the tracked energy and the live stabilities (rrrmc_set_resume), as inside one reference call
    if (!(ctx->resume && ctx->std_cache_live)) { const int32_t rc = xentr_run_init(ctx); if (rc) return rc; }
    XentrMcParams P = xentr_mc_params(ctx, beta);
    P.g0 = ctx->it_done; P.iters = iters; P.step = step; P.samp0 = step;
    const bool wave = xentr_use_wave(ctx->R), no_lds = xentr_no_lds();
    const int64_t PW = P.pc.PW;
    HIP_TRY(ctx, hipEventRecord(ctx->ev_sweep[0], st));
    if (wave) {
        // the table joins Δs, the term buffer and the spins in LDS when all four fit and the chains are few enough for that to pay
        const bool hs = !no_lds && ctx->R <= kXentrWaveTableLdsMaxR && xentr_lds_bytes(ctx->N, PW, ctx->qW, true) <= (size_t)kLdsLimit;
        const size_t lds = xentr_lds_bytes(ctx->N, PW, ctx->qW, hs);
        void (*fn)(XentrMcParams) = hs ? xentr_wave_kernel<true> : xentr_wave_kernel<false>;
        HIP_TRY(ctx, raise_lds_attr(reinterpret_cast<const void*>(fn), lds));
        hipLaunchKernelGGL(fn, dim3((unsigned)ctx->R), dim3(64), lds, st, P);
    } else {
        const size_t lds = ((size_t)ctx->N + 1) * 8;
        const bool hs = !no_lds && lds <= (size_t)kLdsLimit;
        void (*fn)(XentrMcParams) = hs ? xentr_standard_kernel<true> : xentr_standard_kernel<false>;
        if (hs) HIP_TRY(ctx, raise_lds_attr(reinterpret_cast<const void*>(fn), lds));
        hipLaunchKernelGGL(fn, dim3(rrr_blocks(ctx->R)), dim3(rrr_tpb(ctx->R)), hs ? lds : 0, st, P);
    }
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipEventRecord(ctx->ev_sweep[1], st));
    if (ctx->debug_checks) {
        { const int32_t rcf = dbg_flag_ensure(ctx); if (rcf) return rcf; }
        P.flag = ctx->dbg_flag;
        hipLaunchKernelGGL(xentr_check_kernel, dim3((unsigned)((ctx->R + 63) / 64)), dim3(64), 0, st, P);
        HIP_TRY(ctx, hipGetLastError());
    }
    HIP_TRY(ctx, hipEventRecord(ctx->ev_end, st));
    ctx->xe_build = wave ? 2 : 1;
    ctx->sweep_launches = 1;
    ctx->nsamp = nsamp;
    ctx->it_done += (uint64_t)iters;
    ctx->results_valid = true;
    ctx->timing_valid = true;
    ctx->last_call_rrr = true;          // accepted counts live in q_stats
    ctx->std_cache_live = true;
    return RRRMC_OK;
}

// rrrmc_perc_step_energy on one device: the training error of every chain's live configuration
int32_t perc_step_energy(rrrmc_ctx* ctx, int64_t* out)
{
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int64_t* d_out = nullptr;
    HIP_TRY(ctx, dev_alloc(ctx, d_out, (size_t)ctx->R));
    hipLaunchKernelGGL(perc_step_energy_kernel, dim3((unsigned)ctx->R), dim3(64), 0, ctx->stream, perc_params(ctx, 1), ctx->q_spins, (int)ctx->qNk, (int)ctx->qW, d_out);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(out, d_out, sizeof(int64_t) * (size_t)ctx->R, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    dev_free(ctx, d_out);
    HIP_TRY(ctx, e);
    return RRRMC_OK;
}

int32_t xentr_ctx_create(rrrmc_ctx** out, int64_t N, int64_t R, int32_t device, uint32_t replica0)
{
    if (!out) return fail(nullptr, RRRMC_ERR_INVALID_ARG, "out is NULL");
    *out = nullptr;
    if (N < 1 || R < 1) return fail(nullptr, RRRMC_ERR_INVALID_ARG, "N and R must be >= 1");
    { const int32_t rcn = perc_check_n(N); if (rcn) return rcn; }
    if (replica0 % 32) return fail(nullptr, RRRMC_ERR_INVALID_ARG, "replica0 must be a multiple of 32 (given %u)", replica0);
    rrrmc_ctx* ctx = nullptr;
    { const int32_t rcb = ctx_create_begin(&ctx, device, false); if (rcb) return rcb; }
    ctx->model = RRRMC_MODEL_PERC_XENTR;
    ctx->N = N; ctx->K = 0; ctx->R = R; ctx->Rpad = R;
    ctx->qNk = N; ctx->qM = 1; ctx->qW = 2 * ((N + 63) / 64);
    ctx->replica0 = replica0;
    CTX_CREATE_TRY(ctx, false, dev_alloc(ctx, ctx->q_spins, R * ctx->qW));
    CTX_CREATE_TRY(ctx, false, dev_alloc(ctx, ctx->q_stats, R * 2));
    CTX_CREATE_TRY(ctx, false, dev_alloc(ctx, ctx->sk_E, R));
    CTX_CREATE_TRY(ctx, false, dev_alloc(ctx, ctx->xe_nacc, R));
    CTX_CREATE_TRY(ctx, false, hipMemset(ctx->q_spins, 0, sizeof(uint32_t) * R * ctx->qW));
    CTX_CREATE_TRY(ctx, false, hipMemset(ctx->xe_nacc, 0, sizeof(int64_t) * R));
    *out = ctx;
    return RRRMC_OK;
}
