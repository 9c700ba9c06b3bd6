// Host side of the regular 3-spin model (pspin_kernels.hpp): the generator of a partner table, the contexts of rrrmc_ctx_create_pspin3 —
// the stand-alone GraphPSpin3 under standardMC, and the two field wrappers over it, which run through host_af.hpp with RE_PSPIN3 as the
// kind of g — and the upload of a table.  The limits and the validation are pspin_core.hpp's.
// The first part is HIP-free (tests/pspin_core_check.cpp compiles it with RRRMC_PSPIN_HOST_CORE_ONLY); the rest is included by
// rrrmc_hip.hip inside its anonymous namespace, before host_af.hpp; not a stand-alone translation unit.
#ifndef RRRMC_PSPIN_HOST_CORE
#define RRRMC_PSPIN_HOST_CORE
constexpr uint32_t kTagPspin = 13;                          // the Philox stream of rrrmc_gen_pspin3
// GraphPSpin3's constructor (PSpin3.jl:32-43) on the PSPIN stream: layer k is a Fisher-Yates shuffle of 0 .. N-1 — for j = N-1 down to 1,
// swap(l[j], l[floor(u64 (j + 1) / 2^64)]) with draw k (N - 1) + (N - 1 - j) —, consecutive threes of it are the triples.  A [N][2K],
// 0-based.  The caller has checked (N, K) with pspin_check_size.
inline void pspin_generate(int64_t N, int64_t K, uint64_t seed, int32_t* A)
{
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    std::vector<int32_t> l((size_t)N);
    for (int64_t k = 0; k < K; ++k) {
        for (int64_t i = 0; i < N; ++i) l[(size_t)i] = (int32_t)i;
        for (int64_t j = N - 1; j >= 1; --j) {
            const uint64_t n = (uint64_t)(k * (N - 1) + (N - 1 - j));
            const int64_t q = (int64_t)rrrmc::mulhi64(rrrmc::stream_u64(k0, k1, kTagPspin, n), (uint64_t)(j + 1));
            const int32_t t = l[(size_t)j]; l[(size_t)j] = l[(size_t)q]; l[(size_t)q] = t;
        }
        for (int64_t i = 0; i + 2 < N; i += 3) {
            const int32_t v1 = l[(size_t)i], v2 = l[(size_t)i + 1], v3 = l[(size_t)i + 2];
            A[(int64_t)v1 * 2 * K + 2 * k] = v2; A[(int64_t)v1 * 2 * K + 2 * k + 1] = v3;
            A[(int64_t)v2 * 2 * K + 2 * k] = v1; A[(int64_t)v2 * 2 * K + 2 * k + 1] = v3;
            A[(int64_t)v3 * 2 * K + 2 * k] = v1; A[(int64_t)v3 * 2 * K + 2 * k + 1] = v2;
        }
    }
}
#endif  // RRRMC_PSPIN_HOST_CORE

#ifndef RRRMC_PSPIN_HOST_CORE_ONLY
static_assert(RRRMC_MODEL_PSPIN3 == kPspinModelBase && RRRMC_MODEL_PSPIN3_AF == kPspinModelBase + 1 && RRRMC_MODEL_PSPIN3_ASF == kPspinModelBase + 2,
              "pspin_core.hpp restates the model ids");
static_assert((int)RE_PSPIN3 == RRRMC_RE_SLICE_PSPIN3, "ReSlice is rrrmc_re_slice");
inline bool is_pspin(const rrrmc_ctx* ctx) { return pspin_wrap(ctx->model) == 0; }          // the stand-alone graph
inline bool pspin_af(const rrrmc_ctx* ctx) { return pspin_wrap(ctx->model) > 0; }           // a field wrapper over it (one of host_af.hpp's family)

inline PspinTable pspin_table(const rrrmc_ctx* ctx)
{
    PspinTable T{};
    T.A = ctx->ps_A; T.N = (int)ctx->N; T.K = (int)ctx->K;
    return T;
}

// the four samplers over a DeltaECache on the stand-alone graph
int32_t pspin_not_wired(rrrmc_ctx* ctx, const char* sampler)
{
    return fail(ctx, RRRMC_ERR_UNSUPPORTED, "%s is not wired for the stand-alone GraphPSpin3 (a DeltaECache over unique neighbourhoods of variable size): standardMC is, "
                                            "and rrrMC on GraphAddFields / GraphAddSubFields over it (rrrmc_ctx_create_pspin3 with wrap 1 or 2)", sampler);
}

// rrrmc_set_pspin3 on one device
int32_t pspin_set_table(rrrmc_ctx* ctx, const int32_t* A)
{
    if (!A) return fail(ctx, RRRMC_ERR_INVALID_ARG, "A is NULL");
    std::vector<uint16_t> tab((size_t)(ctx->N * 2 * ctx->K));
    char msg[256];
    const int rcv = pspin_validate(ctx->N, ctx->K, A, tab.data(), msg, sizeof msg);
    if (rcv) return fail(ctx, rcv == 3 ? RRRMC_ERR_UNSUPPORTED : RRRMC_ERR_INVALID_ARG, "%s", msg);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->graph_set = false;
    HIP_TRY(ctx, hipMemcpy(ctx->ps_A, tab.data(), sizeof(uint16_t) * tab.size(), hipMemcpyHostToDevice));
    ctx->std_cache_live = false;
    ctx->q_cache_valid = false;
    ctx->graph_set = true;
    return RRRMC_OK;
}

PspinMcParams pspin_mc_params(rrrmc_ctx* ctx, double beta)
{
    PspinMcParams P{};
    P.tab = pspin_table(ctx);
    P.sp = ctx->q_spins; P.spT = ctx->ps_spT; P.E_cur = ctx->sk_E; P.stats = ctx->q_stats; P.Es = ctx->sk_Es; P.flag = ctx->dbg_flag;
    P.beta = beta;
    P.k0 = (uint32_t)ctx->seed; P.k1 = (uint32_t)(ctx->seed >> 32); P.replica0 = ctx->replica0;
    P.N = (int)ctx->N; P.W = (int)ctx->qW; P.R = (int)ctx->R;
    return P;
}

// energy(X, C) into sk_E: the start of a reference call (src/RRRMC.jl:95)
int32_t pspin_run_init(rrrmc_ctx* ctx)
{
    const PspinMcParams P = pspin_mc_params(ctx, 1.0);
    hipLaunchKernelGGL(pspin_init_kernel, dim3((unsigned)((ctx->R + 63) / 64)), dim3(64), 0, ctx->stream, P);
    HIP_TRY(ctx, hipGetLastError());
    return RRRMC_OK;
}

// Which build runs R chains: the wavefront-per-chain kernel up to kPspinWaveMaxR chains, the thread-per-chain kernel beyond.  The bound
// is the largest measured chain count at which the wave build is ahead on both GraphPSpin3(3000, 3) and GraphPSpin3(3000, 8) at β = 1 —
// 1.87x and 2.66x at 16 384; at 32 768 the thread build leads by 1.12x at K = 3 and trails by 1.13x at K = 8, at 65 536 it leads by 1.78x
// and 1.45x (profiles/r20/pspin3.md).  RRRMC_PSPIN_NO_WAVE=1 forces the thread build, RRRMC_PSPIN_WAVE=1 the wave build (timing
// experiments, the builds' parity and Boltzmann tests).
constexpr int64_t kPspinWaveMaxR = 16384;
inline bool pspin_use_wave(int64_t R)
{
    const char* no_wave = std::getenv("RRRMC_PSPIN_NO_WAVE");
    const char* want_wave = std::getenv("RRRMC_PSPIN_WAVE");
    return !(no_wave && no_wave[0] == '1') && (R <= kPspinWaveMaxR || (want_wave && want_wave[0] == '1'));
}

// standardMC on a stand-alone GraphPSpin3
int32_t pspin_mc_async(rrrmc_ctx* ctx, double beta, int64_t iters, int64_t step)
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
    const bool wave = pspin_use_wave(ctx->R);
    if (!wave && !ctx->ps_spT) HIP_TRY(ctx, dev_alloc(ctx, ctx->ps_spT, (size_t)ctx->R * (size_t)ctx->qW));
    hipStream_t st = ctx->stream;
    HIP_TRY(ctx, hipEventRecord(ctx->ev_begin, st));
    ctx->stats_stride = 2;
    // a resumed call continues from the tracked energy (rrrmc_set_resume), as inside one reference call
    if (!(ctx->resume && ctx->std_cache_live)) { const int32_t rc = pspin_run_init(ctx); if (rc) return rc; }
    PspinMcParams P = pspin_mc_params(ctx, beta);
    P.g0 = ctx->it_done; P.iters = iters; P.step = step; P.samp0 = step;
    const unsigned tgrid = (unsigned)(((size_t)ctx->R * (size_t)ctx->qW + 255) / 256);
    // the sampler's events bracket the thread build's two transposes too: they are work only that build does, on every call
    HIP_TRY(ctx, hipEventRecord(ctx->ev_sweep[0], st));
    if (!wave) { hipLaunchKernelGGL(pspin_transpose_kernel, dim3(tgrid), dim3(256), 0, st, P, 0); HIP_TRY(ctx, hipGetLastError()); }
    if (wave) hipLaunchKernelGGL(pspin_wave_kernel, dim3((unsigned)ctx->R), dim3(64), 0, st, P);
    else hipLaunchKernelGGL(pspin_standard_kernel, dim3(rrr_blocks(ctx->R)), dim3(rrr_tpb(ctx->R)), 0, st, P);
    HIP_TRY(ctx, hipGetLastError());
    if (!wave) { hipLaunchKernelGGL(pspin_transpose_kernel, dim3(tgrid), dim3(256), 0, st, P, 1); HIP_TRY(ctx, hipGetLastError()); }
    HIP_TRY(ctx, hipEventRecord(ctx->ev_sweep[1], st));
    if (ctx->debug_checks) {
        const int32_t rcf = dbg_flag_ensure(ctx);
        if (rcf) return rcf;
        P.flag = ctx->dbg_flag;
        hipLaunchKernelGGL(pspin_check_kernel, dim3((unsigned)((ctx->R + 63) / 64)), dim3(64), 0, st, P);
        HIP_TRY(ctx, hipGetLastError());
    }
    HIP_TRY(ctx, hipEventRecord(ctx->ev_end, st));
    ctx->ps_build = wave ? 2 : 1;
    ctx->sweep_launches = 1;
    ctx->nsamp = nsamp;
    ctx->it_done += (uint64_t)iters;
    ctx->results_valid = true;
    ctx->timing_valid = true;
    ctx->last_call_rrr = true;          // accepted counts live in q_stats
    ctx->std_cache_live = true;
    return RRRMC_OK;
}

// every check of rrrmc_ctx_create_pspin3, before any device query
int32_t pspin_check_create(rrrmc_ctx** out, int64_t N, int64_t K, int32_t wrap, int64_t R, uint32_t replica0)
{
    if (!out) return fail(nullptr, RRRMC_ERR_INVALID_ARG, "out is NULL");
    *out = nullptr;
    if (wrap < 0 || wrap > 2)
        return fail(nullptr, RRRMC_ERR_INVALID_ARG, "wrap must be 0 (GraphPSpin3), 1 (GraphAddFields over it) or 2 (GraphAddSubFields over it), given: %d", wrap);
    if (R < 1) return fail(nullptr, RRRMC_ERR_INVALID_ARG, "GraphPSpin3: R must be >= 1");
    char msg[256];
    const int rcs = pspin_check_size(N, K, msg, sizeof msg);
    if (rcs) return fail(nullptr, rcs == 3 ? RRRMC_ERR_UNSUPPORTED : RRRMC_ERR_INVALID_ARG, "%s", msg);
    if (replica0 % 32) return fail(nullptr, RRRMC_ERR_INVALID_ARG, "replica0 must be a multiple of 32 (given %u)", replica0);
    return RRRMC_OK;
}

int32_t pspin_ctx_create(rrrmc_ctx** out, int64_t N, int64_t K, int32_t wrap, int64_t R, int32_t device, uint32_t replica0)
{
    { const int32_t rcc = pspin_check_create(out, N, K, wrap, R, replica0); if (rcc) return rcc; }
    rrrmc_ctx* ctx = nullptr;
    { const int32_t rcb = ctx_create_begin(&ctx, device, false); if (rcb) return rcb; }
    ctx->model = pspin_model(wrap);
    ctx->N = N; ctx->K = K; ctx->R = R; ctx->Rpad = R;
    ctx->qNk = N; ctx->qM = 1; ctx->qW = 2 * ((N + 63) / 64); ctx->q_Wk = ctx->qW;
    ctx->replica0 = replica0;
    CTX_CREATE_TRY(ctx, false, dev_alloc(ctx, ctx->ps_A, (size_t)(N * 2 * K)));
    CTX_CREATE_TRY(ctx, false, dev_alloc(ctx, ctx->q_spins, R * ctx->qW));
    CTX_CREATE_TRY(ctx, false, dev_alloc(ctx, ctx->q_stats, R * 2));
    CTX_CREATE_TRY(ctx, false, dev_alloc(ctx, ctx->sk_E, R));
    if (wrap != 0) {                                               // the wrappers' buffers, as af_ctx_create makes them
        int levs = 0;
        while (((int64_t)1 << levs) < N) ++levs;                   // DynamicSamplers.jl:36
        ctx->af_levs = levs; ctx->af_N2 = (int64_t)1 << levs;
        CTX_CREATE_TRY(ctx, false, dev_alloc(ctx, ctx->q_z, R));
        CTX_CREATE_TRY(ctx, false, dev_alloc(ctx, ctx->q_accrate, R));
        CTX_CREATE_TRY(ctx, false, dev_alloc(ctx, ctx->af_h, N));
        CTX_CREATE_TRY(ctx, false, dev_alloc(ctx, ctx->af_dEs, (size_t)R * (size_t)N));
        CTX_CREATE_TRY(ctx, false, dev_alloc(ctx, ctx->af_v, (size_t)R * (size_t)ctx->af_N2));
        CTX_CREATE_TRY(ctx, false, dev_alloc(ctx, ctx->af_ps, (size_t)R * (size_t)ctx->af_N2));
        CTX_CREATE_TRY(ctx, false, dev_alloc(ctx, ctx->af_tref, (size_t)R));
        CTX_CREATE_TRY(ctx, false, dev_alloc(ctx, ctx->af_status, 2));
        CTX_CREATE_TRY(ctx, false, hipMemset(ctx->af_status, 0, sizeof(int32_t) * 2));
    }
    CTX_CREATE_TRY(ctx, false, hipMemset(ctx->q_spins, 0, sizeof(uint32_t) * R * ctx->qW));
    *out = ctx;
    return RRRMC_OK;
}
#endif  // RRRMC_PSPIN_HOST_CORE_ONLY
