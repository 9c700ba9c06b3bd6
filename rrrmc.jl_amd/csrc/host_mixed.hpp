// Host side of GraphMixed and the field wrappers over it (mixed_kernels.hpp): context creation, the kernel parameters, the start of a run,
// the debug check, the build choice and launch of a sampler call, the components' energies.  A mixed context is one of the wrappers'
// family (host_af.hpp: AfParams, af_set_fields, rrrmc_af_cache / _build, the frame of a sampler call of host_ens.hpp); every component is
// uploaded by its own kind's call into the buffers that kind has.  The component list and its checks are mixed_models.hpp's.
// Included by rrrmc_hip.hip inside its anonymous namespace, after host_af.hpp; not a stand-alone translation unit.
static_assert((int)RE_MIXED == RRRMC_RE_SLICE_MIXED, "ReSlice is rrrmc_re_slice");
static_assert(kMixedNmax == kAfNmax && kMixedPatNmax == kPercNmax && kMixedPatNmax == kCommNmax && kMixedKmax == kContKmax && kMixedNmax <= kSatNmax,
              "mixed_models.hpp restates the kernels' bounds");

// every check of rrrmc_ctx_create_mixed, before any device query
int32_t mixed_check(rrrmc_ctx** out, const int32_t* kinds, int32_t nkinds, int32_t wrap, int64_t N, int64_t K, int64_t K2, int64_t R, uint32_t replica0)
{
    if (!out) return fail(nullptr, RRRMC_ERR_INVALID_ARG, "out is NULL");
    *out = nullptr;
    char msg[320];
    const int32_t rc = mixed_check_create(kinds, nkinds, wrap, N, K, K2, R, replica0, msg, sizeof msg);
    if (rc) return fail(nullptr, rc, "%s", msg);
    return RRRMC_OK;
}

inline MixedList mixed_list_of(const int32_t* kinds, int32_t nkinds)
{
    MixedList L{};
    L.n = nkinds;
    for (int32_t c = 0; c < nkinds; ++c) L.kind[c] = kinds[c];
    return L;
}

int32_t mixed_ctx_create(rrrmc_ctx** out, const int32_t* kinds, int32_t nkinds, int32_t wrap, int64_t N, int64_t K, int64_t K2, int64_t R, int32_t device, uint32_t replica0)
{
    { const int32_t rcc = mixed_check(out, kinds, nkinds, wrap, N, K, K2, R, replica0); if (rcc) return rcc; }
    rrrmc_ctx* ctx = nullptr;
    { const int32_t rcb = ctx_create_begin(&ctx, device, false); if (rcb) return rcb; }
    ctx->model = mixed_model(wrap);
    ctx->mx = mixed_list_of(kinds, nkinds);
    ctx->mx_need = mixed_need_mask(ctx->mx);
    const bool spf = mixed_list_has(ctx->mx, RRRMC_RE_SLICE_SPARSE_F64);
    ctx->N = N; ctx->K = spf ? K : 0; ctx->R = R; ctx->Rpad = R;
    ctx->qNk = N; ctx->qM = 1; ctx->qW = 2 * ((N + 63) / 64); ctx->q_Wk = ctx->qW;
    ctx->replica0 = replica0;
    ctx->graph_set = ctx->mx_need == 0;                            // a mix of GraphEmptys has nothing to upload
    ctx->af_fields_set = wrap == 0;                                // the stand-alone mix has no fields: it runs as sub = 1, which never reads them
    if (mixed_list_has_group(ctx->mx, MG_COMM)) ctx->cm_K2 = K2;
    int levs = 0;
    while (((int64_t)1 << levs) < N) ++levs;                       // DynamicSamplers.jl:36
    ctx->af_levs = levs; ctx->af_N2 = (int64_t)1 << levs;
    if (mixed_list_has(ctx->mx, RRRMC_RE_SLICE_SKN)) {
        CTX_CREATE_TRY(ctx, false, dev_alloc(ctx, ctx->sk_J, N * N));
        CTX_CREATE_TRY(ctx, false, dev_alloc(ctx, ctx->q_slf, (size_t)R * 2 * (size_t)N));
        CTX_CREATE_TRY(ctx, false, dev_alloc(ctx, ctx->q_smv, (size_t)R));
        CTX_CREATE_TRY(ctx, false, dev_alloc(ctx, ctx->q_scur, (size_t)R));
    }
    if (mixed_list_has(ctx->mx, RRRMC_RE_SLICE_SK)) CTX_CREATE_TRY(ctx, false, dev_alloc(ctx, ctx->q_Jb, N * ctx->q_Wk));
    if (spf) {
        CTX_CREATE_TRY(ctx, false, dev_alloc(ctx, ctx->d_A, N * K));
        CTX_CREATE_TRY(ctx, false, dev_alloc(ctx, ctx->q_Jf, N * K));
        CTX_CREATE_TRY(ctx, false, dev_alloc(ctx, ctx->q_flf, (size_t)R * (size_t)N));
        CTX_CREATE_TRY(ctx, false, dev_alloc(ctx, ctx->q_fundo, (size_t)R * (size_t)(K + 1)));
        CTX_CREATE_TRY(ctx, false, dev_alloc(ctx, ctx->q_fml, (size_t)R));
    }
    CTX_CREATE_TRY(ctx, false, dev_alloc(ctx, ctx->q_spins, R * ctx->qW));
    CTX_CREATE_TRY(ctx, false, dev_alloc(ctx, ctx->q_z, R));
    CTX_CREATE_TRY(ctx, false, dev_alloc(ctx, ctx->q_accrate, R));
    CTX_CREATE_TRY(ctx, false, dev_alloc(ctx, ctx->q_stats, R * 2));
    CTX_CREATE_TRY(ctx, false, dev_alloc(ctx, ctx->sk_E, R));
    if (wrap != 0) {
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

// the same context over several devices: shards of whole 32-replica groups in global-id order, as rrrmc_ctx_create_multi makes them
int32_t mixed_ctx_create_multi(rrrmc_ctx** out, const int32_t* kinds, int32_t nkinds, int32_t wrap, int64_t N, int64_t K, int64_t K2, int64_t R,
                               const int32_t* device_ids, int32_t ndev, uint32_t replica0)
{
    { const int32_t rcc = mixed_check(out, kinds, nkinds, wrap, N, K, K2, R, replica0); if (rcc) return rcc; }
    if (!device_ids || ndev < 1) return fail(nullptr, RRRMC_ERR_INVALID_ARG, "device_ids must name at least one device (ndev = %d)", ndev);
    if (ndev > 64) return fail(nullptr, RRRMC_ERR_INVALID_ARG, "ndev = %d: at most 64 devices", ndev);
    rrrmc_ctx* ctx = new (std::nothrow) rrrmc_ctx();
    if (!ctx) return fail(nullptr, RRRMC_ERR_NOMEM, "out of host memory");
    ctx->model = mixed_model(wrap);
    ctx->mx = mixed_list_of(kinds, nkinds);
    ctx->mx_need = mixed_need_mask(ctx->mx);
    ctx->N = N; ctx->K = mixed_list_has(ctx->mx, RRRMC_RE_SLICE_SPARSE_F64) ? K : 0; ctx->R = R; ctx->replica0 = replica0; ctx->device = device_ids[0];
    ctx->qNk = N; ctx->qM = 1;
    if (mixed_list_has_group(ctx->mx, MG_COMM)) ctx->cm_K2 = K2;
    for (int32_t d = 0; d < ndev; ++d) {
        int64_t b0 = 0, b1 = 0;
        shard_bounds(R, ndev, d, &b0, &b1);
        if (b1 <= b0) continue;          // fewer groups than devices: this one stays idle
        rrrmc_ctx* c = nullptr;
        const int32_t rc = mixed_ctx_create(&c, kinds, nkinds, wrap, N, K, K2, b1 - b0, device_ids[d], replica0 + (uint32_t)b0);
        if (rc) {
            for (rrrmc_ctx* k : ctx->kids) rrrmc_ctx_destroy(k);
            delete ctx;
            return rc;                   // (the text of the failure is already in the creation-error slot)
        }
        ctx->kids.push_back(c);
        ctx->kid_r0.push_back(b0);
    }
    *out = ctx;
    return RRRMC_OK;
}

AfParams mixed_params(rrrmc_ctx* ctx, double beta)
{
    AfParams A{};
    ReParams& P = A.re;
    const MixedList& L = ctx->mx;
    A.mx = L;
    if (mixed_list_has(L, RE_SK)) { P.Jb = ctx->q_Jb; P.Wk = (int)ctx->q_Wk; P.sN = std::sqrt((double)ctx->N); }
    if (mixed_list_has(L, RE_SKN)) { P.Jd = ctx->sk_J; P.slf = ctx->q_slf; P.smv = ctx->q_smv; P.scur = ctx->q_scur; }
    if (mixed_list_has_group(L, MG_PERC)) P.pc = perc_params(ctx, 1);
    if (mixed_list_has(L, RE_PXE)) P.xe = xentr_params(ctx);
    if (mixed_list_has_group(L, MG_COMM)) P.cm = comm_params(ctx, 1);
    if (mixed_list_has(L, RE_SAT)) P.sat = sat_table(ctx);
    if (mixed_list_has(L, RE_SPF)) ens_spf_params(ctx, &P);
    P.abi = ctx->q_spins; P.sp = ctx->q_spins;          // M = 1: the ABI site order is every component's own
    P.zz = ctx->q_z; P.E_cur = ctx->sk_E; P.acc_rate = ctx->q_accrate; P.stats = ctx->q_stats; P.Es = ctx->sk_Es; P.flag = ctx->dbg_flag;
    P.beta = beta;
    P.k0 = (uint32_t)ctx->seed; P.k1 = (uint32_t)(ctx->seed >> 32); P.replica0 = ctx->replica0;
    P.Nk = (int)ctx->N; P.M = 1; P.L = 0; P.N = (int)ctx->N; P.W = (int)ctx->qW; P.R = (int)ctx->R;
    A.h = ctx->af_h; A.dEs = ctx->af_dEs; A.v = ctx->af_v; A.ps = ctx->af_ps; A.tref = ctx->af_tref; A.status = ctx->af_status;
    A.sub = mixed_wrap(ctx->model) == 1 ? 0 : 1; A.levs = ctx->af_levs; A.N2 = (int)ctx->af_N2;
    return A;
}

// energy(X, C), every component's cache and, for rrrMC, a fresh DeltaECacheCont over X0: the start of a reference call
int32_t mixed_run_init(rrrmc_ctx* ctx, double beta, bool cache)
{
    const AfParams A = mixed_params(ctx, beta);
    hipLaunchKernelGGL(mixed_init_kernel, dim3((unsigned)ctx->R), dim3(kAfInitThreads), 0, ctx->stream, A, cache ? 1 : 0);
    HIP_TRY(ctx, hipGetLastError());
    return RRRMC_OK;
}

// debug mode: the consistency check behind a sampler call (reported by the next sync, post_sync_checks)
int32_t mixed_debug_check(rrrmc_ctx* ctx, const AfParams& A0, bool cache)
{
    const int32_t rc = dbg_flag_ensure(ctx);
    if (rc) return rc;
    AfParams A = A0;
    A.re.flag = ctx->dbg_flag;
    hipLaunchKernelGGL(mixed_check_kernel, dim3((unsigned)((ctx->R + 63) / 64)), dim3(64), 0, ctx->stream, A, cache ? 1 : 0);
    HIP_TRY(ctx, hipGetLastError());
    return RRRMC_OK;
}

// Which standardMC build runs R chains: the wavefront-per-chain kernel up to kMixedWaveMaxR chains, the thread-per-chain kernel beyond.
// The bound is the largest measured chain count at which the wave build is ahead on GraphMixed(GraphSK(1001), GraphPercStep(1001, 400),
// GraphSAT(1001, 3, 4.2)): it leads at all four counts measured, 8 .. 16 384 (5.0, 6.5, 11.2 and 4.3 times; profiles/r19/mixed.md) — no
// crossing was seen, so nothing beyond the last measured count is claimed for it.  RRRMC_MIXED_NO_WAVE=1 forces the thread build,
// RRRMC_MIXED_WAVE=1 the wave build (timing experiments, the builds' parity tests).
constexpr int64_t kMixedWaveMaxR = 16384;
inline bool mixed_use_wave(int64_t R)
{
    const char* no_wave = std::getenv("RRRMC_MIXED_NO_WAVE");
    const char* want_wave = std::getenv("RRRMC_MIXED_WAVE");
    if (no_wave && no_wave[0] == '1') return false;
    if (want_wave && want_wave[0] == '1') return true;
    return R <= kMixedWaveMaxR;
}

// rrrMC(X::DoubleGraph) on a wrapper over the mix (standard = false), or standardMC on any of the three models (standard = true)
int32_t mixed_mc_async(rrrmc_ctx* ctx, bool standard, double beta, int64_t iters, int64_t step, double staged_thr, double staged_thr_fact)
{
    if (standard && std::isnan(beta)) return fail(ctx, RRRMC_ERR_INVALID_ARG, "beta is NaN");
    if (!standard && mixed_wrap(ctx->model) == 0)
        return fail(ctx, RRRMC_ERR_UNSUPPORTED, "rrrMC is not wired for the stand-alone GraphMixed (DeltaECacheCont over the union of the components' neighbourhoods): standardMC is, "
                                                "and rrrMC on GraphAddFields / GraphAddSubFields over it (rrrmc_ctx_create_mixed with wrap 1 or 2)");
    EnsCall C;
    int32_t rc = ens_call_begin(ctx, standard, beta, iters, step, staged_thr, staged_thr_fact, &C, false);
    if (rc) return rc;
    const bool pxe = mixed_list_has(ctx->mx, RE_PXE);
    const int64_t xe_PW = pxe ? (ctx->pc_P + 63) / 64 : 0;
    if (pxe && !standard) {          // the wavefront form of GraphPercXEntr's residual adds its terms from a buffer: global memory here
        if (ctx->xe_term_P != ctx->pc_P) { dev_free(ctx, ctx->xe_term); ctx->xe_term_P = 0; }
        if (!ctx->xe_term) { HIP_TRY(ctx, dev_alloc(ctx, ctx->xe_term, (size_t)(ctx->R * 64 * xe_PW))); ctx->xe_term_P = ctx->pc_P; }
    }
    if (C.cont) { if (!standard) HIP_TRY(ctx, hipMemsetAsync(ctx->q_stats, 0, sizeof(int64_t) * (size_t)ctx->R * 2, ctx->stream)); }
    else { rc = mixed_run_init(ctx, beta, !standard); if (rc) return rc; }
    AfParams A = mixed_params(ctx, beta);
    ens_call_params(ctx, C, iters, step, staged_thr, staged_thr_fact, &A.re);
    hipStream_t st = ctx->stream;
    HIP_TRY(ctx, hipEventRecord(ctx->ev_sweep[0], st));
    if (standard) {
        const size_t lds = mixed_wave_lds_bytes(ctx->qW, xe_PW);
        if (mixed_use_wave(ctx->R) && lds <= (size_t)kLdsLimit - 1024) {
            HIP_TRY(ctx, raise_lds_attr(reinterpret_cast<const void*>(mixed_wave_kernel), lds + 1024));
            hipLaunchKernelGGL(mixed_wave_kernel, dim3((unsigned)ctx->R), dim3(64), lds, st, A, (int)xe_PW);
            ctx->mx_build = 2;
        } else {
            hipLaunchKernelGGL(mixed_standard_kernel, dim3(rrr_blocks(ctx->R)), dim3(rrr_tpb(ctx->R)), 0, st, A);
            ctx->mx_build = 1;
        }
    } else {
        // the LDS build stages the sampler's tree, weights, ΔEs and the spins; the components' per-chain state stays in global memory
        // (RRRMC_AF_NO_LDS=1 forces the global build: the builds' parity test)
        const size_t lds = (af_lds_bytes(ctx->N, ctx->af_N2, ctx->qW) + 7) & ~(size_t)7;
        const char* no_lds = std::getenv("RRRMC_AF_NO_LDS");
        const bool use_lds = lds <= (size_t)kLdsLimit && !(no_lds && no_lds[0] == '1');
        const af_kernel_fn fn = use_lds ? af_rrr_kernel<RE_MIXED, true> : af_rrr_kernel<RE_MIXED, false>;
        if (use_lds) HIP_TRY(ctx, raise_lds_attr(reinterpret_cast<const void*>(fn), lds));
        hipLaunchKernelGGL(fn, dim3((unsigned)ctx->R), dim3(64), use_lds ? lds : 0, st, A);
        ctx->af_build = use_lds ? 1 : 2;
    }
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipEventRecord(ctx->ev_sweep[1], st));
    if (ctx->debug_checks) { rc = mixed_debug_check(ctx, A, !standard); if (rc) return rc; }
    HIP_TRY(ctx, hipEventRecord(ctx->ev_end, st));
    ctx->sweep_launches = 1;
    ctx->nsamp = C.nsamp;
    ctx->it_done += (uint64_t)iters;
    if (!standard) smp_commit(ctx, 1, iters);
    ctx->results_valid = true;
    ctx->timing_valid = true;
    ctx->last_call_rrr = true;          // accepted / staged counts live in q_stats
    ctx->q_cache_valid = !standard;
    ctx->std_cache_live = standard;
    return RRRMC_OK;
}

// rrrmc_mixed_energies on one device
int32_t mixed_energies(rrrmc_ctx* ctx, double* E_out)
{
    const size_t n = (size_t)ctx->R * (size_t)ctx->mx.n;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    double* d_out = nullptr;
    HIP_TRY(ctx, dev_alloc(ctx, d_out, n));
    const AfParams A = mixed_params(ctx, 1.0);
    hipLaunchKernelGGL(mixed_energies_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, ctx->stream, A, d_out);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(E_out, d_out, sizeof(double) * n, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    dev_free(ctx, d_out);
    HIP_TRY(ctx, e);
    return RRRMC_OK;
}
