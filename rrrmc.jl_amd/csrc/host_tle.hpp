// Host side of the Topological Local Entropy ensemble (GraphTopologicalLocalEntropy over GraphEmpty / binary GraphSK / GraphSKNormal /
// GraphSAT / sparse Float64 slices, tle_kernels.hpp).  Included by rrrmc_hip.hip inside its anonymous namespace, after host_le.hpp; not a stand-alone
// translation unit.  A TLE context is a Local Entropy context (the same spins, μ, slice state, scalars, observables) whose level tables and
// DeltaECache arrays are sized by rrrmc_tle_set_params — the number of levels depends on the topology and on (γT, λT) — and which adds the
// neighbour lists, the class-code table, lfields2 and 16-bit class ids.  What the three ensembles share is in host_ens.hpp; the TLE kernels
// are dispatched over TleSlices, the five slice kinds they are built for.

// Device-memory rule: the sets are dense, [2L][N] 16-bit members per replica, as in the other ensembles; a context whose sets would take
// more than kTleSetBytesMax in all is refused.
constexpr size_t kTleSetBytesMax = (size_t)16 << 30;

TleParams tle_params(rrrmc_ctx* ctx, double beta)
{
    TleParams P{};
    static_cast<LeParams&>(P) = le_params(ctx, beta);
    const int64_t L = ctx->tle_L;
    P.tab = ctx->re_tab; P.ft = ctx->re_tab + L; P.ctab = nullptr; P.cls = nullptr; P.L = (int)L;
    P.rowptr = ctx->tle_rowptr; P.cols = ctx->tle_cols; P.code = ctx->tle_code; P.lf2 = ctx->tle_lf2; P.wcls = ctx->tle_cls;
    P.l2 = 2 * ctx->tle_lT; P.lT = ctx->tle_lT; P.mn = (int)(ctx->qM * ctx->tle_maxdeg);
    return P;
}

// energy(X, C) and, for rrrMC, a fresh DeltaECache: the start of a reference call (src/RRRMC.jl:95, :236-238); ft needs the sampler's β
int32_t tle_run_init(rrrmc_ctx* ctx, double beta, bool cache)
{
    const int64_t L = ctx->tle_L;
    for (int64_t a = 0; a < L; ++a) ctx->re_hft[(size_t)a] = host_det_exp(-beta * ctx->re_htab[(size_t)a]);      // DeltaE.jl:91
    HIP_TRY(ctx, hipMemcpyAsync(ctx->re_tab + L, ctx->re_hft.data(), sizeof(double) * (size_t)L, hipMemcpyHostToDevice, ctx->stream));
    const TleParams P = tle_params(ctx, beta);
    int32_t rc = re_to_slices(ctx, P);
    if (rc) return rc;
    const dim3 grid((unsigned)ctx->R), blk(kReInitThreads);
    if (!with_slice(TleSlices{}, ens_slice(ctx->model), [&](auto s) { hipLaunchKernelGGL(tle_init_kernel<decltype(s)::value>, grid, blk, 0, ctx->stream, P, cache ? 1 : 0); }))
        return ens_bad_slice(ctx);
    HIP_TRY(ctx, hipGetLastError());
    return RRRMC_OK;
}

typedef void (*tle_kernel_fn)(TleParams);
// nullptr: no such slice
tle_kernel_fn tle_rrr_fn(int slice, bool lds)
{
    tle_kernel_fn fn = nullptr;
    with_slice(TleSlices{}, slice, [&](auto s) { fn = lds ? tle_rrr_kernel<true, decltype(s)::value> : tle_rrr_kernel<false, decltype(s)::value>; });
    return fn;
}

// debug mode: the consistency check behind a sampler call (reported by the next sync, post_sync_checks)
int32_t tle_debug_check(rrrmc_ctx* ctx, const TleParams& P0, bool cache)
{
    const int32_t rc = dbg_flag_ensure(ctx);
    if (rc) return rc;
    TleParams P = P0;
    P.flag = ctx->dbg_flag;
    const dim3 grid((unsigned)((ctx->R + 63) / 64)), blk(64);
    if (!with_slice(TleSlices{}, ens_slice(ctx->model), [&](auto s) { hipLaunchKernelGGL(tle_check_kernel<decltype(s)::value>, grid, blk, 0, ctx->stream, P, cache ? 1 : 0); }))
        return ens_bad_slice(ctx);
    HIP_TRY(ctx, hipGetLastError());
    return RRRMC_OK;
}

// rrrMC(X::DoubleGraph) (standard = false) or standardMC (standard = true) on a GraphTopologicalLocalEntropy
int32_t tle_mc_async(rrrmc_ctx* ctx, bool standard, double beta, int64_t iters, int64_t step, double staged_thr, double staged_thr_fact)
{
    EnsCall C;
    int32_t rc = ens_call_begin(ctx, standard, beta, iters, step, staged_thr, staged_thr_fact, &C);
    if (rc) return rc;
    rc = C.cont ? ens_call_resume(ctx, tle_params(ctx, beta), standard) : tle_run_init(ctx, beta, !standard);
    if (rc) return rc;
    TleParams P = tle_params(ctx, beta);
    ens_call_params(ctx, C, iters, step, staged_thr, staged_thr_fact, &P);
    hipStream_t st = ctx->stream;
    HIP_TRY(ctx, hipEventRecord(ctx->ev_sweep[0], st));
    if (standard) {
        const dim3 grid(rrr_blocks(ctx->R)), blk(rrr_tpb(ctx->R));
        if (!with_slice(TleSlices{}, ens_slice(ctx->model), [&](auto s) { hipLaunchKernelGGL(tle_standard_kernel<decltype(s)::value>, grid, blk, 0, st, P); })) return ens_bad_slice(ctx);
    } else {
        // The build: the replica's hot state in LDS (the sets stay in global memory) when it fits and all R wavefronts are resident at
        // once, else everything in global memory.  Measured (profiles/r14/tle.md): on GraphSATTLE(1000, 3, 4.2, 3) the LDS build is 1.13x
        // faster at 8 and 128 replicas and 1.28x slower at 2048; on GraphSKTLE(201, 3) the two tie at 8 and 128 and LDS is 1.55x slower at
        // 2048 — there its LDS footprint cuts the resident wavefronts per compute unit and the chains run in two rounds.
        // Both builds run the same code on the same values; RRRMC_TLE_NO_LDS=1 forces the second, RRRMC_TLE_LDS=1 the first when it fits
        // (the builds' parity test, timing experiments).
        const char* no_lds = std::getenv("RRRMC_TLE_NO_LDS");
        const char* want_lds = std::getenv("RRRMC_TLE_LDS");
        size_t state = tle_rrr_lds_bytes(true, ctx->N, ctx->qW, ctx->qNk, 2 * ctx->tle_L);
        if (ens_slice(ctx->model) == RE_SPF) state = ens_spf_lds(ctx, state, ctx->qM + 1, &P);          // with the rows' LocalFields, when they fit too
        int cus = 0;
        HIP_TRY(ctx, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device));
        const bool resident = state <= (size_t)kLdsLimit && (size_t)ctx->R <= (size_t)cus * ((size_t)kLdsLimit / state);
        const bool use_lds = state <= (size_t)kLdsLimit && !(no_lds && no_lds[0] == '1') && (resident || (want_lds && want_lds[0] == '1'));
        const size_t lds = use_lds ? state : tle_rrr_lds_bytes(false, ctx->N, ctx->qW, ctx->qNk, 2 * ctx->tle_L);
        const tle_kernel_fn fn = tle_rrr_fn(ens_slice(ctx->model), use_lds);
        if (!fn) return ens_bad_slice(ctx);
        HIP_TRY(ctx, raise_lds_attr(reinterpret_cast<const void*>(fn), lds));
        hipLaunchKernelGGL(fn, dim3((unsigned)ctx->R), dim3(kTleWave), lds, st, P);
        ctx->tle_build = use_lds ? 1 : 2;
    }
    HIP_TRY(ctx, hipGetLastError());
    return ens_call_end(ctx, P, C, standard, iters, [&] { return tle_debug_check(ctx, P, !standard); });
}

int32_t tle_ctx_create(rrrmc_ctx** out, int64_t Nk, int64_t M, int32_t slice_kind, int64_t R, int32_t device, uint32_t replica0, SliceK k = {})
{
    if (!out) return fail(nullptr, RRRMC_ERR_INVALID_ARG, "out is NULL");
    *out = nullptr;
    if (ens_model(ENS_LE, slice_kind) == kEnsNoModel)          // (the Local Entropy ensemble has every slice kind there is)
        return fail(nullptr, RRRMC_ERR_INVALID_ARG, "slice_kind must be one of rrrmc_re_slice, given: %d", slice_kind);
    // (the kernels cover sparse Float64 slices too; the text is kept as tests/golden/ens_refusals.json records it, byte for byte)
    if (ens_model(ENS_TLE, slice_kind) == kEnsNoModel)
        return fail(nullptr, RRRMC_ERR_UNSUPPORTED, "slice kind %d: the Topological Local Entropy kernels cover GraphEmpty, GraphSK, GraphSKNormal and GraphSAT slices", slice_kind);
    if (Nk < 1 || R < 1) return fail(nullptr, RRRMC_ERR_INVALID_ARG, "Nk and R must be >= 1");
    if (M <= 2) return fail(nullptr, RRRMC_ERR_INVALID_ARG, "M must be greater than 2, given: %lld", (long long)M);      // TLE.jl:29
    if (M > kTleMmax) return fail(nullptr, RRRMC_ERR_UNSUPPORTED, "M = %lld: the Topological Local Entropy kernels cover M <= %d", (long long)M, kTleMmax);
    if (Nk * (M + 1) > kTleNmax)
        return fail(nullptr, RRRMC_ERR_UNSUPPORTED, "N = Nk*(M+1) = %lld is beyond the Topological Local Entropy kernels (16-bit set members: N <= 65535)", (long long)(Nk * (M + 1)));
    const int32_t rc = ens_ctx_create(ENS_LE, out, Nk, M, slice_kind, R, device, replica0, k, ENS_TLE);
    if (rc) return rc;
    rrrmc_ctx* ctx = *out;
    ctx->model = ens_model(ENS_TLE, slice_kind);
    // the arrays sized by the level count come with rrrmc_tle_set_params
    dev_free(ctx, ctx->q_cls); dev_free(ctx, ctx->q_sv); dev_free(ctx, ctx->q_st); dev_free(ctx, ctx->q_T); dev_free(ctx, ctx->re_tab);
    ctx->re_htab.clear(); ctx->re_hft.clear(); ctx->le_hcode.clear();
    return RRRMC_OK;
}

int32_t tle_set_topology(rrrmc_ctx* ctx, const int32_t* rowptr, const int32_t* cols)
{
    int64_t md = 0;
    char msg[256];
    if (tle_check_topology(ctx->qNk, rowptr, cols, &md, msg, sizeof msg)) return fail(ctx, RRRMC_ERR_INVALID_ARG, "%s", msg);
    const int64_t Nk = ctx->qNk, nnz = rowptr[Nk];
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->re_params_set = false; ctx->tle_topology_set = false;
    ctx->std_cache_live = false; ctx->q_cache_valid = false;
    dev_free(ctx, ctx->tle_rowptr); dev_free(ctx, ctx->tle_cols);
    HIP_TRY(ctx, dev_alloc(ctx, ctx->tle_rowptr, (size_t)(Nk + 1)));
    HIP_TRY(ctx, dev_alloc(ctx, ctx->tle_cols, (size_t)(nnz > 0 ? nnz : 1)));
    HIP_TRY(ctx, hipMemcpy(ctx->tle_rowptr, rowptr, sizeof(int32_t) * (size_t)(Nk + 1), hipMemcpyHostToDevice));
    if (nnz > 0) HIP_TRY(ctx, hipMemcpy(ctx->tle_cols, cols, sizeof(int32_t) * (size_t)nnz, hipMemcpyHostToDevice));
    ctx->tle_maxdeg = md;
    ctx->tle_topology_set = true;
    return RRRMC_OK;
}

// the refusals of a level table, shared by rrrmc_tle_tables and rrrmc_tle_set_params
int32_t tle_host_tables(rrrmc_ctx* ctx, int64_t M, double gamma, double lambda, double beta, int64_t maxdeg, std::vector<double>& dElist)
{
    if (M <= 2) return fail(ctx, RRRMC_ERR_INVALID_ARG, "M must be greater than 2, given: %lld", (long long)M);
    if (M > kTleMmax) return fail(ctx, RRRMC_ERR_UNSUPPORTED, "M = %lld: the Topological Local Entropy ensemble covers M <= %d", (long long)M, kTleMmax);
    if (maxdeg < 0 || maxdeg > kTleNmax) return fail(ctx, RRRMC_ERR_INVALID_ARG, "maxdeg must be in 0 .. %lld, given: %lld", (long long)kTleNmax, (long long)maxdeg);
    const double gT = gamma / beta, lT = lambda / beta;         // TLE.jl:390-396
    const double top = 2 * (double)M * std::fabs(gT) + 2 * (double)(M * maxdeg) * std::fabs(lT);
    if (!std::isfinite(gT) || !std::isfinite(lT) || !std::isfinite(top))
        return fail(ctx, RRRMC_ERR_INVALID_ARG, "gamma / beta and lambda / beta must be finite (and the largest level too), given: %g, %g, %g", gamma, lambda, beta);
    if ((int64_t)tle_len1(M) * (2 * M * maxdeg + 1) > ((int64_t)1 << 26))
        return fail(ctx, RRRMC_ERR_UNSUPPORTED, "M = %lld, max|∂i| = %lld: the level table is beyond the Topological Local Entropy kernels (2L <= %lld)", (long long)M, (long long)maxdeg, (long long)kTleClassMax);
    tle_tables(M, gT, lT, maxdeg, dElist);
    return RRRMC_OK;
}

int32_t tle_set_params(rrrmc_ctx* ctx, double gamma, double lambda, double beta_graph)
{
    if (!ctx->tle_topology_set) return fail(ctx, RRRMC_ERR_STATE, "rrrmc_tle_set_params comes after rrrmc_tle_set_topology");
    const int64_t M = ctx->qM, N = ctx->N, R = ctx->R;
    std::vector<double> dE;
    const int32_t rc = tle_host_tables(ctx, M, gamma, lambda, beta_graph, ctx->tle_maxdeg, dE);
    if (rc) return rc;
    const int64_t L = (int64_t)dE.size();
    if (2 * L > kTleClassMax)
        return fail(ctx, RRRMC_ERR_UNSUPPORTED, "allΔE has L = %lld levels: the Topological Local Entropy kernels cover 2L <= %lld (16-bit class ids)", (long long)L, (long long)kTleClassMax);
    if ((size_t)R * (size_t)(2 * L) * (size_t)N * sizeof(uint16_t) > kTleSetBytesMax)
        return fail(ctx, RRRMC_ERR_UNSUPPORTED, "R = %lld replicas with 2L = %lld classes of N = %lld sites: the dense sets take more than the %zu GiB this build allows", (long long)R, (long long)(2 * L), (long long)N, kTleSetBytesMax >> 30);
    const double gT = gamma / beta_graph, lT = lambda / beta_graph;
    std::vector<uint32_t> code;
    if (!tle_codes(M, gT, lT, ctx->tle_maxdeg, dE, code))
        return fail(ctx, RRRMC_ERR_INVALID_ARG, "findk finds no level for a field pair of GraphTLE{%lld, %g, %g}", (long long)M, gT, lT);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->re_params_set = false;
    ctx->std_cache_live = false; ctx->q_cache_valid = false;
    dev_free(ctx, ctx->re_tab); dev_free(ctx, ctx->tle_code); dev_free(ctx, ctx->q_sv); dev_free(ctx, ctx->q_st); dev_free(ctx, ctx->q_T); dev_free(ctx, ctx->tle_cls); dev_free(ctx, ctx->tle_lf2);
    HIP_TRY(ctx, dev_alloc(ctx, ctx->re_tab, (size_t)(2 * L)));
    HIP_TRY(ctx, dev_alloc(ctx, ctx->tle_code, code.size()));
    HIP_TRY(ctx, dev_alloc(ctx, ctx->q_sv, (size_t)R * (size_t)(2 * L) * (size_t)N));
    HIP_TRY(ctx, dev_alloc(ctx, ctx->q_st, (size_t)R * (size_t)(2 * L)));
    HIP_TRY(ctx, dev_alloc(ctx, ctx->q_T, (size_t)R * (size_t)(2 * L)));
    HIP_TRY(ctx, dev_alloc(ctx, ctx->tle_cls, (size_t)R * (size_t)N));
    HIP_TRY(ctx, dev_alloc(ctx, ctx->tle_lf2, (size_t)R * (size_t)N));
    HIP_TRY(ctx, hipMemcpy(ctx->re_tab, dE.data(), sizeof(double) * (size_t)L, hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemcpy(ctx->tle_code, code.data(), sizeof(uint32_t) * code.size(), hipMemcpyHostToDevice));
    // (a set slot that no push! has written is never read as a site: zeroed all the same, so that nothing in the arrays is indeterminate)
    HIP_TRY(ctx, hipMemset(ctx->q_sv, 0, sizeof(uint16_t) * (size_t)R * (size_t)(2 * L) * (size_t)N));
    ctx->re_htab = dE;
    ctx->re_hft.assign((size_t)L, 0.0);
    ctx->tle_L = L; ctx->le_gT = gT; ctx->tle_lT = lT;
    ctx->re_params_set = true;
    return RRRMC_OK;
}
