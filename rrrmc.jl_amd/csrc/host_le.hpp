// Host side of the Local Entropy ensemble (GraphLocalEntropy, le_kernels.hpp): its tables and class codes, kernel parameters, run start,
// debug check, observables and the build choice and launch of a sampler call.  What it shares with the other two ensembles is in
// host_ens.hpp.  Included by rrrmc_hip.hip inside its anonymous namespace, after host_re.hpp; not a stand-alone translation unit.  The
// context reuses the Robust Ensemble's buffers (re_sp, re_mu, re_tab, re_Eslice and the q_* DeltaECache arrays) with M + 1 rows.

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
    const int slice = ens_slice(ctx->model);
    if (slice == RE_SK) { P.Jb = ctx->q_Jb; P.Wk = (int)ctx->q_Wk; P.sN = std::sqrt((double)ctx->qNk); }
    if (slice == RE_SKN) { P.Jd = ctx->sk_J; P.slf = ctx->q_slf; P.smv = ctx->q_smv; P.scur = ctx->q_scur; }
    if (slice == RE_PSTEP || slice == RE_PLIN) P.pc = perc_params(ctx, M + 1);
    if (slice == RE_CSTEP || slice == RE_CRELU || slice == RE_CQU) P.cm = comm_params(ctx, M + 1);
    if (slice == RE_SAT) P.sat = sat_table(ctx);
    if (slice == RE_SPF) ens_spf_params(ctx, &P);
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
    const dim3 grid((unsigned)ctx->R), blk(kReInitThreads);
    if (!with_slice(AllSlices{}, ens_slice(ctx->model), [&](auto s) { hipLaunchKernelGGL(le_init_kernel<decltype(s)::value>, grid, blk, 0, ctx->stream, P, cache ? 1 : 0); }))
        return ens_bad_slice(ctx);
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
// nullptr: no such slice
le_kernel_fn le_rrr_fn(int slice, bool lds, int L)
{
    le_kernel_fn fn = nullptr;
    with_slice(AllSlices{}, slice, [&](auto s) { fn = lds ? le_rrr_for_L<true, decltype(s)::value>(L) : le_rrr_for_L<false, decltype(s)::value>(L); });
    return fn;
}

// debug mode: the consistency check behind a sampler call (reported by the next sync, post_sync_checks)
int32_t le_debug_check(rrrmc_ctx* ctx, const LeParams& P0, bool cache)
{
    const int32_t rc = dbg_flag_ensure(ctx);
    if (rc) return rc;
    LeParams P = P0;
    P.flag = ctx->dbg_flag;
    const dim3 grid((unsigned)((ctx->R + 63) / 64)), blk(64);
    if (!with_slice(AllSlices{}, ens_slice(ctx->model), [&](auto s) { hipLaunchKernelGGL(le_check_kernel<decltype(s)::value>, grid, blk, 0, ctx->stream, P, cache ? 1 : 0); }))
        return ens_bad_slice(ctx);
    HIP_TRY(ctx, hipGetLastError());
    return RRRMC_OK;
}

// rrrMC(X::DoubleGraph) (standard = false) or standardMC (standard = true) on a GraphLocalEntropy
int32_t le_mc_async(rrrmc_ctx* ctx, bool standard, double beta, int64_t iters, int64_t step, double staged_thr, double staged_thr_fact)
{
    EnsCall C;
    int32_t rc = ens_call_begin(ctx, standard, beta, iters, step, staged_thr, staged_thr_fact, &C);
    if (rc) return rc;
    rc = C.cont ? ens_call_resume(ctx, le_params(ctx, beta), standard) : le_run_init(ctx, beta, !standard);
    if (rc) return rc;
    LeParams P = le_params(ctx, beta);
    ens_call_params(ctx, C, iters, step, staged_thr, staged_thr_fact, &P);
    const int slice = ens_slice(ctx->model);
    hipStream_t st = ctx->stream;
    HIP_TRY(ctx, hipEventRecord(ctx->ev_sweep[0], st));
    if (standard) {
        const dim3 grid(rrr_blocks(ctx->R)), blk(rrr_tpb(ctx->R));
        if (!with_slice(AllSlices{}, slice, [&](auto s) { hipLaunchKernelGGL(le_standard_kernel<decltype(s)::value>, grid, blk, 0, st, P); })) return ens_bad_slice(ctx);
    } else {
        // the build choice of re_mc_async (one replica per workgroup in LDS up to 2048 replicas, one thread per replica beyond);
        // RRRMC_LE_NO_LDS=1 forces the thread build, RRRMC_LE_LDS=1 the LDS build (timing experiments, the builds' parity test)
        size_t lds = le_rrr_lds_bytes(ctx->N, ctx->qW, ctx->qNk);
        if (P.pc.ds) lds = ((lds + 7) & ~(size_t)7) + perc_lds_bytes(P.pc.rows, P.pc.PW);
        if (P.cm.ds) lds = ((lds + 7) & ~(size_t)7) + comm_lds_bytes(P.cm.rows, P.cm.K2, P.cm.PW, slice == RE_CQU);          // the rows' Stabilities
        if (slice == RE_SPF) lds = ens_spf_lds(ctx, lds, ctx->qM + 1, &P);          // the rows' LocalFields, when they fit too
        const char* no_lds = std::getenv("RRRMC_LE_NO_LDS");
        const char* want_lds = std::getenv("RRRMC_LE_LDS");
        // (perceptron slices: the LDS build at every replica count, as in re_mc_async)
        const bool use_lds = lds <= (size_t)kLdsLimit && !(no_lds && no_lds[0] == '1') && (ctx->R <= 2048 || P.pc.ds || P.cm.ds || (want_lds && want_lds[0] == '1'));
        const le_kernel_fn fn = le_rrr_fn(slice, use_lds, P.L);
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
    return ens_call_end(ctx, P, C, standard, iters, [&] { return le_debug_check(ctx, P, !standard); });
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
    if (!with_slice(AllSlices{}, ens_slice(ctx->model), [&](auto s) { hipLaunchKernelGGL(le_obs_kernel<decltype(s)::value>, grid, blk, 0, ctx->stream, P); }))
        return ens_bad_slice(ctx);
    HIP_TRY(ctx, hipGetLastError());
    return RRRMC_OK;
}
