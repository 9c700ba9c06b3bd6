// Host side of random K-SAT (sat_kernels.hpp): the occurrence program built from a clause list, the stand-alone GraphSAT contexts under
// standardMC, and the clause upload that the Robust Ensemble and Local Entropy contexts with SAT slices share with them.
// The first part is HIP-free (tests/sat_core_check.cpp compiles it with RRRMC_SAT_HOST_CORE_ONLY); the rest is included by rrrmc_hip.hip
// inside its anonymous namespace, before host_re.hpp; not a stand-alone translation unit.
#ifndef RRRMC_SAT_HOST_CORE
#define RRRMC_SAT_HOST_CORE
// The occurrence program (sat_core.hpp) of clauses given as vars[Mc][Kmax] (0-based, ascending, -1 pads at the end) and lits[Mc][Kmax].
// Returns 0, or 1 (invalid argument) / 3 (beyond the kernels' limits) with a message.  max_conn = max |T[i]|.
inline int sat_build_program(int64_t N, int64_t Mc, int64_t Kmax, const int32_t* vars, const int8_t* lits, std::vector<uint32_t>& off,
                             std::vector<rrrmc::SatEntry>& ent, int64_t* max_conn, char* msg, size_t msg_len)
{
    using namespace rrrmc;
    if (N < 1 || Mc < 1 || Kmax < 1) { snprintf(msg, msg_len, "N, Mc and Kmax must be >= 1, given: %lld, %lld, %lld", (long long)N, (long long)Mc, (long long)Kmax); return 1; }
    if (N > kSatNmax) { snprintf(msg, msg_len, "N = %lld: the K-SAT kernels cover N <= %d (16-bit variable ids)", (long long)N, kSatNmax); return 3; }
    if (Mc > kSatMcMax) { snprintf(msg, msg_len, "Mc = %lld: the K-SAT kernels cover Mc <= 2^20 clauses", (long long)Mc); return 3; }
    std::vector<int> len((size_t)Mc, 0);
    std::vector<uint32_t> deg((size_t)N + 1, 0u);
    for (int64_t a = 0; a < Mc; ++a) {
        const int32_t* va = vars + a * Kmax;
        int64_t l = 0;
        while (l < Kmax && va[l] >= 0) ++l;
        for (int64_t k = l; k < Kmax; ++k)
            if (va[k] != -1) { snprintf(msg, msg_len, "clause %lld: entry %lld follows a pad", (long long)a, (long long)k); return 1; }
        if (l == 0) { snprintf(msg, msg_len, "clause %lld is empty", (long long)a); return 1; }
        for (int64_t k = 0; k < l; ++k) {
            if (va[k] >= N) { snprintf(msg, msg_len, "clause %lld: variable %d out of range (N = %lld)", (long long)a, va[k], (long long)N); return 1; }
            if (k && va[k] == va[k - 1]) { snprintf(msg, msg_len, "clause %lld: variable %d appears twice", (long long)a, va[k]); return 1; }
            if (k && va[k] < va[k - 1]) { snprintf(msg, msg_len, "clause %lld: the variables are not in ascending order", (long long)a); return 1; }
            if (lits[a * Kmax + k] < 0 || lits[a * Kmax + k] > 1) { snprintf(msg, msg_len, "clause %lld: literal bits must be 0 or 1", (long long)a); return 1; }
        }
        if (l > kSatLenMax) { snprintf(msg, msg_len, "clause %lld has %lld literals: the K-SAT kernels cover <= %d", (long long)a, (long long)l, kSatLenMax); return 3; }
        len[(size_t)a] = (int)l;
        for (int64_t k = 0; k < l; ++k) deg[(size_t)va[k]] += 1u;
    }
    uint32_t mc = 0;
    for (int64_t i = 0; i < N; ++i) mc = deg[(size_t)i] > mc ? deg[(size_t)i] : mc;
    if (mc > (uint32_t)kSatDegMax) { snprintf(msg, msg_len, "a variable appears in %u clauses: the K-SAT kernels cover <= %d", mc, kSatDegMax); return 3; }
    off.assign((size_t)N + 1, 0u);
    for (int64_t i = 0; i < N; ++i) off[(size_t)i + 1] = off[(size_t)i] + deg[(size_t)i];
    ent.assign((size_t)off[(size_t)N], SatEntry{});
    std::vector<uint32_t> cur(off.begin(), off.end() - 1);
    for (int64_t a = 0; a < Mc; ++a) {                       // clause order: T[i] as SAT.jl:92-97 builds it
        const int32_t* va = vars + a * Kmax;
        const int8_t* ja = lits + a * Kmax;
        const int l = len[(size_t)a];
        for (int k = 0; k < l; ++k) {
            SatEntry e{};
            unsigned h = (unsigned)(ja[k] & 1) | ((unsigned)(l - 1) << 1) | (k == 0 ? 1u << 11 : 0u);
            int q = 0;
            for (int k2 = 0; k2 < l; ++k2) {
                if (k2 == k) continue;
                sat_entry_set_half(e, 1 + q, (unsigned)va[k2]);
                h |= (unsigned)(ja[k2] & 1) << (4 + q);
                ++q;
            }
            sat_entry_set_half(e, 0, h);
            ent[(size_t)cur[(size_t)va[k]]++] = e;
        }
    }
    if (max_conn) *max_conn = (int64_t)mc;
    return 0;
}
#endif  // RRRMC_SAT_HOST_CORE

#ifndef RRRMC_SAT_HOST_CORE_ONLY
inline bool is_sat(const rrrmc_ctx* ctx) { return ctx->model == RRRMC_MODEL_SAT; }
inline bool sat_slices(const rrrmc_ctx* ctx) { return model_slice(ctx->model) == RRRMC_RE_SLICE_SAT; }          // an ensemble over K-SAT slices (ens_models.hpp), or a field wrapper over a GraphSAT (af_models.hpp)

inline SatTable sat_table(const rrrmc_ctx* ctx)
{
    SatTable T{};
    T.off = ctx->sat_off; T.ent = ctx->sat_ent; T.N = (int)ctx->qNk;
    return T;
}

// rrrmc_set_clauses on one device
int32_t sat_set_clauses(rrrmc_ctx* ctx, int64_t Mc, int64_t Kmax, const int32_t* vars, const int8_t* lits)
{
    if (!vars || !lits) return fail(ctx, RRRMC_ERR_INVALID_ARG, "vars or lits is NULL");
    std::vector<uint32_t> off;
    std::vector<SatEntry> ent;
    int64_t mc = 0;
    char msg[256];
    const int rcb = sat_build_program(ctx->qNk, Mc, Kmax, vars, lits, off, ent, &mc, msg, sizeof msg);
    if (rcb) return fail(ctx, rcb == 3 ? RRRMC_ERR_UNSUPPORTED : RRRMC_ERR_INVALID_ARG, "%s", msg);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    dev_free(ctx, ctx->sat_off); dev_free(ctx, ctx->sat_ent);
    ctx->graph_set = false;
    HIP_TRY(ctx, dev_alloc(ctx, ctx->sat_off, off.size()));
    HIP_TRY(ctx, dev_alloc(ctx, ctx->sat_ent, (ent.empty() ? 1 : ent.size())));
    HIP_TRY(ctx, hipMemcpy(ctx->sat_off, off.data(), sizeof(uint32_t) * off.size(), hipMemcpyHostToDevice));
    if (!ent.empty()) HIP_TRY(ctx, hipMemcpy(ctx->sat_ent, ent.data(), sizeof(SatEntry) * ent.size(), hipMemcpyHostToDevice));
    ctx->sat_Mc = Mc; ctx->sat_maxconn = mc;
    ctx->std_cache_live = false;
    ctx->q_cache_valid = false;
    ctx->graph_set = true;
    return RRRMC_OK;
}

SatMcParams sat_mc_params(rrrmc_ctx* ctx, double beta)
{
    SatMcParams P{};
    P.tab = sat_table(ctx);
    P.sp = ctx->q_spins; P.spT = ctx->sat_spT; P.E_cur = ctx->sk_E; P.stats = ctx->q_stats; P.Es = ctx->sk_Es; P.flag = ctx->dbg_flag;
    P.beta = beta;
    P.k0 = (uint32_t)ctx->seed; P.k1 = (uint32_t)(ctx->seed >> 32); P.replica0 = ctx->replica0;
    P.N = (int)ctx->N; P.W = (int)ctx->qW; P.R = (int)ctx->R;
    return P;
}

// energy(X, C) into sk_E: the start of a reference call (src/RRRMC.jl:95)
int32_t sat_run_init(rrrmc_ctx* ctx)
{
    const SatMcParams P = sat_mc_params(ctx, 1.0);
    hipLaunchKernelGGL(sat_init_kernel, dim3((unsigned)((ctx->R + 63) / 64)), dim3(64), 0, ctx->stream, P);
    HIP_TRY(ctx, hipGetLastError());
    return RRRMC_OK;
}

// Which build runs R replicas: the wavefront-per-replica kernel up to kSatWaveMaxR replicas, the thread-per-replica kernel beyond.  The
// bound is the largest measured replica count at which the wave build is ahead on GraphSAT(1000, 3, 4.2) — 1.54x at 16 384; at 32 768 the
// thread build leads by 1.21x (profiles/r12/sat.md) —, not the 2048 of the GraphQuant pattern builds this started from: a wavefront per
// replica keeps the chip full long before one thread per replica does.  RRRMC_SAT_NO_WAVE=1 forces the thread
// build, RRRMC_SAT_WAVE=1 the wave build (timing experiments, the builds' parity and Boltzmann tests).
constexpr int64_t kSatWaveMaxR = 16384;
inline bool sat_use_wave(int64_t R)
{
    const char* no_wave = std::getenv("RRRMC_SAT_NO_WAVE");
    const char* want_wave = std::getenv("RRRMC_SAT_WAVE");
    return !(no_wave && no_wave[0] == '1') && (R <= kSatWaveMaxR || (want_wave && want_wave[0] == '1'));
}

// standardMC on a stand-alone GraphSAT
int32_t sat_mc_async(rrrmc_ctx* ctx, double beta, int64_t iters, int64_t step)
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
    const bool wave = sat_use_wave(ctx->R);
    if (!wave && !ctx->sat_spT) HIP_TRY(ctx, dev_alloc(ctx, ctx->sat_spT, (size_t)ctx->R * (size_t)ctx->qW));
    hipStream_t st = ctx->stream;
    HIP_TRY(ctx, hipEventRecord(ctx->ev_begin, st));
    ctx->stats_stride = 2;
    // a resumed call continues from the tracked energy (rrrmc_set_resume), as inside one reference call
    if (!(ctx->resume && ctx->std_cache_live)) { const int32_t rc = sat_run_init(ctx); if (rc) return rc; }
    SatMcParams P = sat_mc_params(ctx, beta);
    P.g0 = ctx->it_done; P.iters = iters; P.step = step; P.samp0 = step;
    const unsigned tgrid = (unsigned)(((size_t)ctx->R * (size_t)ctx->qW + 255) / 256);
    // the sampler's events bracket the thread build's two transposes too: they are work only that build does, on every call
    HIP_TRY(ctx, hipEventRecord(ctx->ev_sweep[0], st));
    if (!wave) { hipLaunchKernelGGL(sat_transpose_kernel, dim3(tgrid), dim3(256), 0, st, P, 0); HIP_TRY(ctx, hipGetLastError()); }
    if (wave) hipLaunchKernelGGL(sat_wave_kernel, dim3((unsigned)ctx->R), dim3(64), 0, st, P);
    else hipLaunchKernelGGL(sat_standard_kernel, dim3(rrr_blocks(ctx->R)), dim3(rrr_tpb(ctx->R)), 0, st, P);
    HIP_TRY(ctx, hipGetLastError());
    if (!wave) { hipLaunchKernelGGL(sat_transpose_kernel, dim3(tgrid), dim3(256), 0, st, P, 1); HIP_TRY(ctx, hipGetLastError()); }
    HIP_TRY(ctx, hipEventRecord(ctx->ev_sweep[1], st));
    if (ctx->debug_checks) {
        if (!ctx->dbg_flag) { HIP_TRY(ctx, dev_alloc(ctx, ctx->dbg_flag, 2)); HIP_TRY(ctx, hipMemsetAsync(ctx->dbg_flag, 0, sizeof(int32_t) * 2, st)); }
        P.flag = ctx->dbg_flag;
        hipLaunchKernelGGL(sat_check_kernel, dim3((unsigned)((ctx->R + 63) / 64)), dim3(64), 0, st, P);
        HIP_TRY(ctx, hipGetLastError());
    }
    HIP_TRY(ctx, hipEventRecord(ctx->ev_end, st));
    ctx->sat_build = wave ? 2 : 1;
    ctx->sweep_launches = 1;
    ctx->nsamp = nsamp;
    ctx->it_done += (uint64_t)iters;
    ctx->results_valid = true;
    ctx->timing_valid = true;
    ctx->last_call_rrr = true;          // accepted counts live in q_stats
    ctx->std_cache_live = true;
    return RRRMC_OK;
}

int32_t sat_ctx_create(rrrmc_ctx** out, int64_t N, int64_t R, int32_t device, uint32_t replica0)
{
    if (!out) return fail(nullptr, RRRMC_ERR_INVALID_ARG, "out is NULL");
    *out = nullptr;
    if (N < 1 || R < 1) return fail(nullptr, RRRMC_ERR_INVALID_ARG, "N and R must be >= 1");
    if (N > kSatNmax) return fail(nullptr, RRRMC_ERR_UNSUPPORTED, "N = %lld: the K-SAT kernels cover N <= %d (16-bit variable ids)", (long long)N, kSatNmax);
    if (replica0 % 32) return fail(nullptr, RRRMC_ERR_INVALID_ARG, "replica0 must be a multiple of 32 (given %u)", replica0);
    rrrmc_ctx* ctx = nullptr;
    { const int32_t rcb = ctx_create_begin(&ctx, device, false); if (rcb) return rcb; }
    ctx->model = RRRMC_MODEL_SAT;
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
#endif  // RRRMC_SAT_HOST_CORE_ONLY
