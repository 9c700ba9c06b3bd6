// Host side of rrrmc_exchange_async / rrrmc_exchange_results: the refusals, the energies of the two live configurations, the
// ordering between the two contexts' streams, the one launch of pt_kernels.hpp, and what an exchange invalidates.  Included by
// rrrmc_hip.hip behind native_spins and the models' energy passes.
#pragma once

namespace {

inline bool pt_model_ok(int32_t model)
{
    return model == RRRMC_MODEL_SPARSE_PM1 || model == RRRMC_MODEL_SPARSE_LEVELS || model == RRRMC_MODEL_SPARSE_F64 ||
           model == RRRMC_MODEL_SK_NORMAL || model == RRRMC_MODEL_SK_BINARY;
}

// a refused model by the name its users know
const char* pt_model_name(const rrrmc_ctx* c)
{
    if (c->model == RRRMC_MODEL_QUANT_RRG) return "GraphQuant";
    if (c->model == RRRMC_MODEL_SPARSE_DISCRETIZED) return "GraphRRGNormalDiscretized / GraphEANormalDiscretized";
    if (is_mixed(c)) return "GraphMixed";
    if (is_tle(c)) return "GraphTopologicalLocalEntropy";
    if (is_le(c)) return "GraphLocalEntropy";
    if (is_re(c)) return "GraphRobustEnsemble";
    if (is_af(c)) return "GraphAddFields / GraphAddSubFields";
    if (is_xentr(c)) return "GraphPercXEntr";
    if (is_perc(c)) return "GraphPercStep / GraphPercLinear";
    if (is_comm(c)) return "GraphCommStep / GraphCommReLU / GraphCommQu";
    if (is_sat(c)) return "GraphSAT";
    if (is_pspin(c)) return "GraphPSpin3";
    return "this model";
}

// an exchange has rewritten the spins: the state rrrmc_set_spins leaves (no live run, stale caches, no tracked energy); the last call's
// samples stay (they belong to the temperature, not to the walker), and so does it_done
inline void pt_invalidate(rrrmc_ctx* c)
{
    smp_drop(c);
    c->std_cache_live = false;
    c->pf_lf_live = false;
    c->pt_E_live = false;
    c->pt_swapped = true;
}

// the energies of c's live configuration, on c's stream: the exact tracked energy of an integer model when a standardMC call left it and
// nothing has touched the spins since, otherwise energy(X, C) by the model's own energy pass.  *E: the array ([Rpad] int32 or Float64)
int32_t pt_energies(rrrmc_ctx* c, const void** E)
{
    HIP_TRY(c, hipSetDevice(c->device));
    if (sparse_int_model(c)) {
        *E = c->d_E;
        if (c->pt_E_live && c->results_valid && !c->colored_call) return RRRMC_OK;
        smp_drop(c);                                          // as rrrmc_energy does
        return c->model == RRRMC_MODEL_SPARSE_LEVELS ? lev_standard_mc_async(c, 0.0, 0, 1, true) : run_energy_bs(c, nullptr);
    }
    *E = c->sk_E;
    smp_drop(c);                                              // as rrrmc_energy_f64 does
    return c->model == RRRMC_MODEL_SPARSE_F64 ? spf_run_energy(c) : sk_run_energy(c);
}

// what must hold of one (single-device) pair before anything is queued; errors go to `top` (the caller's first handle)
int32_t pt_check_pair(rrrmc_ctx* top, rrrmc_ctx* a, rrrmc_ctx* b)
{
    for (rrrmc_ctx* c : {a, b})
        if (!c->graph_set || !c->spins_set)
            return fail(top, RRRMC_ERR_STATE, "rrrmc_exchange_async: %s of the two contexts has no %s", c == a ? "the first" : "the second", c->graph_set ? "configuration" : "graph");
    if (a->model != b->model || a->N != b->N || a->K != b->K || a->R != b->R || a->replica0 != b->replica0)
        return fail(top, RRRMC_ERR_STATE, "rrrmc_exchange_async: the two contexts differ (model %d / %d, N %lld / %lld, K %lld / %lld, R %lld / %lld, replica0 %u / %u): "
                    "an exchange is between two contexts of one graph", a->model, b->model, (long long)a->N, (long long)b->N, (long long)a->K, (long long)b->K,
                    (long long)a->R, (long long)b->R, a->replica0, b->replica0);
    if (a->device != b->device)
        return fail(top, RRRMC_ERR_UNSUPPORTED, "rrrmc_exchange_async: the two contexts are on different devices (%d and %d)", a->device, b->device);
    // one workgroup row per replica group (grid y)
    const int64_t groups = a->model == RRRMC_MODEL_SPARSE_F64 ? a->pfW : a->model == RRRMC_MODEL_SK_NORMAL || a->model == RRRMC_MODEL_SK_BINARY ? a->G8 : a->G;
    if (groups > 65535 || a->R > INT32_MAX / 2)
        return fail(top, RRRMC_ERR_UNSUPPORTED, "rrrmc_exchange_async covers at most 65535 replica groups per context (or shard), given %lld", (long long)groups);
    return RRRMC_OK;
}

// one single-device pair: everything is queued, nothing waits (the first exchange of a context allocates its result buffers and events)
int32_t pt_exchange_pair(rrrmc_ctx* a, rrrmc_ctx* b, double beta_a, double beta_b, uint64_t seed, uint64_t round)
{
    HIP_TRY(a, hipSetDevice(a->device));
    const size_t nw = (size_t)pt_mask_words(a->Rpad);
    // each resource on its own: a first call that failed half way leaves the rest to the next one
    if (!a->pt_mask) {
        HIP_TRY(a, dev_alloc(a, a->pt_mask, nw));
        HIP_TRY(a, hipMemsetAsync(a->pt_mask, 0, sizeof(uint32_t) * nw, a->stream));     // (the byte layout's last word is written in part only)
    }
    if (!a->pt_E) HIP_TRY(a, dev_alloc(a, a->pt_E, 2 * (size_t)a->Rpad));
    for (int i = 0; i < 2; ++i)
        if (!a->pt_ev[i]) HIP_TRY(a, hipEventCreateWithFlags(&a->pt_ev[i], hipEventDisableTiming));
    a->pt_valid = false;
    // the two energy passes run side by side on their own streams, behind everything queued there
    const void* Ea = nullptr; const void* Eb = nullptr;
    { const int32_t rc = pt_energies(b, &Eb); if (rc) { a->err = b->err; return rc; } }
    { const int32_t rc = pt_energies(a, &Ea); if (rc) return rc; }
    // b's stream -> a's: the launch below runs behind everything queued on either stream
    HIP_TRY(a, hipEventRecord(a->pt_ev[0], b->stream));
    HIP_TRY(a, hipStreamWaitEvent(a->stream, a->pt_ev[0], 0));
    PtParams P{};
    P.sa = const_cast<void*>(native_spins(a)); P.sb = const_cast<void*>(native_spins(b));
    P.Ea = Ea; P.Eb = Eb;
    P.mask32 = a->pt_mask; P.Ea_out = a->pt_E; P.Eb_out = a->pt_E + a->Rpad;
    P.beta_a = beta_a; P.beta_b = beta_b;
    P.lv_mul = a->model == RRRMC_MODEL_SPARSE_LEVELS ? a->lv_mul : 1; P.lv_div = a->model == RRRMC_MODEL_SPARSE_LEVELS ? a->lv_div : 1.0;
    P.round = round; P.k0 = (uint32_t)seed; P.k1 = (uint32_t)(seed >> 32); P.replica0 = a->replica0;
    P.R = (int)a->R;
    const dim3 block(kPtThreads);
    const long long per = (long long)kPtThreads * kPtWordsPerThread;
    auto ranges = [](long long len, long long p) { return (unsigned)((len + p - 1) / p); };
    if (a->model == RRRMC_MODEL_SPARSE_LEVELS) {
        P.len = a->qW;
        hipLaunchKernelGGL(pt_exchange_rows_kernel<true>, dim3(ranges(P.len, per), (unsigned)a->G), block, 0, a->stream, P);
    } else if (a->model == RRRMC_MODEL_SPARSE_PM1) {
        P.len = a->N;
        hipLaunchKernelGGL((pt_exchange_kernel<uint32_t, true>), dim3(ranges(P.len, per), (unsigned)a->G), block, 0, a->stream, P);
    } else if (a->model == RRRMC_MODEL_SPARSE_F64) {
        P.len = a->N;
        hipLaunchKernelGGL((pt_exchange_kernel<unsigned long long, false>), dim3(ranges(P.len, per), (unsigned)a->pfW), block, 0, a->stream, P);
    } else {
        P.len = a->N;
        hipLaunchKernelGGL((pt_exchange_kernel<uint8_t, false>), dim3(ranges(P.len, 8 * per), (unsigned)a->G8), block, 0, a->stream, P);
    }
    HIP_TRY(a, hipGetLastError());
    pt_invalidate(a);                                         // the swap is queued: from here on the spins are new (until here the two
    pt_invalidate(b);                                         // contexts are in the state their energy calls leave)
    // a's stream -> b's: whatever is queued on b from here on runs behind the swap
    HIP_TRY(a, hipEventRecord(a->pt_ev[1], a->stream));
    HIP_TRY(a, hipStreamWaitEvent(b->stream, a->pt_ev[1], 0));
    a->pt_valid = true;
    return RRRMC_OK;
}

int32_t pt_exchange(rrrmc_ctx* a, rrrmc_ctx* b, double beta_a, double beta_b, uint64_t seed, uint64_t round)
{
    if (!a) return RRRMC_ERR_INVALID_ARG;
    if (!b) return fail(a, RRRMC_ERR_INVALID_ARG, "rrrmc_exchange_async: the second context is NULL");
    if (a == b) return fail(a, RRRMC_ERR_INVALID_ARG, "rrrmc_exchange_async: the two contexts are the same one");
    if (!std::isfinite(beta_a) || !std::isfinite(beta_b))
        return fail(a, RRRMC_ERR_INVALID_ARG, "rrrmc_exchange_async: beta_a = %g, beta_b = %g must be finite (an infinite difference makes x = NaN at equal energies)", beta_a, beta_b);
    for (rrrmc_ctx* c : {a, b})
        if (is_multi(c) && c->multi_poisoned)
            return fail(a, RRRMC_ERR_STATE, "an earlier call failed on some devices of a multi-device context only: its shards are at different positions; destroy it");
    if (!pt_model_ok(a->model))
        return fail(a, RRRMC_ERR_UNSUPPORTED, "rrrmc_exchange_async is not wired for %s (model %d): it covers RRRMC_MODEL_SPARSE_PM1, SPARSE_LEVELS, SPARSE_F64, SK_NORMAL and SK_BINARY",
                    pt_model_name(a), a->model);
    if (is_multi(a) != is_multi(b))
        return fail(a, RRRMC_ERR_UNSUPPORTED, "rrrmc_exchange_async: a multi-device context exchanges with one over the same device list only");
    if (!is_multi(a)) {
        const int32_t rc = pt_check_pair(a, a, b);
        return rc ? rc : pt_exchange_pair(a, b, beta_a, beta_b, seed, round);
    }
    if (a->model != b->model || a->N != b->N || a->K != b->K || a->R != b->R || a->replica0 != b->replica0)
        return fail(a, RRRMC_ERR_STATE, "rrrmc_exchange_async: the two contexts differ (model %d / %d, N %lld / %lld, K %lld / %lld, R %lld / %lld): an exchange is between two contexts of one graph",
                    a->model, b->model, (long long)a->N, (long long)b->N, (long long)a->K, (long long)b->K, (long long)a->R, (long long)b->R);
    bool same = a->kids.size() == b->kids.size();
    for (size_t d = 0; same && d < a->kids.size(); ++d) same = a->kids[d]->device == b->kids[d]->device && a->kid_r0[d] == b->kid_r0[d] && a->kids[d]->R == b->kids[d]->R;
    if (!same) return fail(a, RRRMC_ERR_UNSUPPORTED, "rrrmc_exchange_async: the two multi-device contexts are over different device lists");
    for (size_t d = 0; d < a->kids.size(); ++d) {             // every shard is checked before any is queued
        const int32_t rc = pt_check_pair(a, a->kids[d], b->kids[d]);
        if (rc) return rc;
    }
    for (size_t d = 0; d < a->kids.size(); ++d) {
        const int32_t rc = pt_exchange_pair(a->kids[d], b->kids[d], beta_a, beta_b, seed, round);
        if (rc) {
            a->err = "device " + std::to_string(a->kids[d]->device) + " (replicas from " + std::to_string(a->kid_r0[d]) + "): " + a->kids[d]->err;
            if (d > 0) a->multi_poisoned = b->multi_poisoned = true;
            return rc;
        }
    }
    return RRRMC_OK;
}

int32_t pt_results_one(rrrmc_ctx* a, uint8_t* swapped_out, int64_t* nswapped_out, double* Ea_out, double* Eb_out)
{
    if (!a->pt_valid) return fail(a, RRRMC_ERR_STATE, "no rrrmc_exchange_async has been made with this context as its first argument");
    HIP_TRY(a, hipSetDevice(a->device));
    HIP_TRY(a, hipStreamSynchronize(a->stream));
    { const int32_t rcp = post_sync_checks(a); if (rcp) return rcp; }
    std::vector<uint32_t> m((size_t)pt_mask_words(a->Rpad));
    HIP_TRY(a, hipMemcpy(m.data(), a->pt_mask, sizeof(uint32_t) * m.size(), hipMemcpyDeviceToHost));
    int64_t n = 0;
    for (int64_t r = 0; r < a->R; ++r) {
        const bool s = pt_mask_get(m.data(), r);
        if (swapped_out) swapped_out[r] = s ? 1 : 0;
        n += s ? 1 : 0;
    }
    if (nswapped_out) *nswapped_out = n;
    if (Ea_out) HIP_TRY(a, hipMemcpy(Ea_out, a->pt_E, sizeof(double) * (size_t)a->R, hipMemcpyDeviceToHost));
    if (Eb_out) HIP_TRY(a, hipMemcpy(Eb_out, a->pt_E + a->Rpad, sizeof(double) * (size_t)a->R, hipMemcpyDeviceToHost));
    return RRRMC_OK;
}

int32_t pt_results(rrrmc_ctx* a, uint8_t* swapped_out, int64_t* nswapped_out, double* Ea_out, double* Eb_out)
{
    if (!a) return RRRMC_ERR_INVALID_ARG;
    if (!is_multi(a)) return pt_results_one(a, swapped_out, nswapped_out, Ea_out, Eb_out);
    std::vector<int64_t> cnt(a->kids.size(), 0);
    const int32_t rc = multi_each(a, [&](rrrmc_ctx* c, int64_t r0, int64_t) -> int32_t {
        size_t d = 0;
        while (a->kids[d] != c) ++d;
        return pt_results_one(c, at_row(swapped_out, r0), &cnt[d], at_row(Ea_out, r0), at_row(Eb_out, r0));
    }, true);
    if (rc) return rc;
    if (nswapped_out) { *nswapped_out = 0; for (int64_t n : cnt) *nswapped_out += n; }
    return RRRMC_OK;
}

}  // namespace
