// Host side of rrrmc_cross_overlaps / rrrmc_overlap_hist: argument checks, the batches of slot pairs (xov_core.hpp), one
// packed copy per distinct slot per batch, the launches of xov_tile_kernel.  Included by rrrmc_hip.hip behind native_spins / spins_to_chunks.
#pragma once

namespace {

// the native buffer a slot names on a single-device context; nullptr: out of range or empty
const void* xov_slot_native(const rrrmc_ctx* c, int32_t sl)
{
    if (sl == -1) return native_spins(c);                    // the live configuration
    if (sl < 0 || sl >= c->snap_slots || !c->snap_valid[(size_t)sl]) return nullptr;
    return c->snap + native_spin_bytes(c) * (size_t)sl;
}

// One call of either kind.  hist: a0 = b0 = 0 and nA = nB = R.  On a multi-device context the packed rows of every distinct slot are
// gathered from the shards through the host onto the first shard's device, and the kernel runs there over all R replicas.
int32_t xov_call(rrrmc_ctx* ctx, bool hist, int64_t npairs, const int32_t* slotA, const int32_t* slotB, int64_t a0, int64_t nA, int64_t b0,
                 int64_t nB, int32_t* q_out, int64_t* hist_out)
{
    if (!ctx) return RRRMC_ERR_INVALID_ARG;
    const bool multi = is_multi(ctx);
    if (multi && ctx->multi_poisoned)
        return fail(ctx, RRRMC_ERR_STATE, "an earlier call failed on some devices of this multi-device context only: its shards are at different positions; destroy it");
    rrrmc_ctx* ex = multi ? ctx->kids[0] : ctx;               // where the kernel runs
    const size_t nkids = multi ? ctx->kids.size() : 1;
    for (size_t d = 0; d < nkids; ++d) {
        rrrmc_ctx* k = multi ? ctx->kids[d] : ctx;
        const int32_t rc = ensure_state(k, true);
        if (rc) { if (multi) ctx->err = k->err; return rc; }
    }
    const int64_t R = ctx->R, N = ctx->N, nch = (N + 63) / 64;
    if (npairs < 0) return fail(ctx, RRRMC_ERR_INVALID_ARG, "npairs must be >= 0, given %lld", (long long)npairs);
    if (npairs == 0) return RRRMC_OK;
    if (!slotA || !slotB || !(hist ? (const void*)hist_out : (const void*)q_out))
        return fail(ctx, RRRMC_ERR_INVALID_ARG, "slotA, slotB, %s must not be NULL", hist ? "hist_out" : "q_out");
    if (!xov_pairs_ok(npairs)) return fail(ctx, RRRMC_ERR_INVALID_ARG, "at most %lld slot pairs per call, given %lld", (long long)kXovMaxPairs, (long long)npairs);
    if (hist) { a0 = b0 = 0; nA = nB = R; }
    if (!xov_rows_ok(a0, nA, R)) return fail(ctx, RRRMC_ERR_INVALID_ARG, "rows of A: a0 = %lld, nA = %lld are outside 0 <= a0, nA >= 1, a0 + nA <= R = %lld", (long long)a0, (long long)nA, (long long)R);
    if (!xov_rows_ok(b0, nB, R)) return fail(ctx, RRRMC_ERR_INVALID_ARG, "rows of B: b0 = %lld, nB = %lld are outside 0 <= b0, nB >= 1, b0 + nB <= R = %lld", (long long)b0, (long long)nB, (long long)R);
    if (!hist && !xov_matrix_ok(npairs, nA, nB))
        return fail(ctx, RRRMC_ERR_INVALID_ARG, "npairs * nA * nB = %lld * %lld * %lld exceeds the cap of %lld results per call", (long long)npairs, (long long)nA, (long long)nB, (long long)kXovMaxMatrix);
    for (int64_t p = 0; p < npairs; ++p)
        for (int side = 0; side < 2; ++side) {
            const int32_t sl = side ? slotB[p] : slotA[p];
            if (!xov_slot_native(ex, sl)) return fail(ctx, RRRMC_ERR_INVALID_ARG, "pair %lld: snapshot slot %d is out of range or empty", (long long)p, sl);
        }
    if (xov_tiles(nA) > kXovMaxTiles || N > INT32_MAX / 2 || R > INT32_MAX / 2)
        return fail(ctx, RRRMC_ERR_UNSUPPORTED, "cross overlaps cover at most %lld rows of A per call", (long long)(kXovMaxTiles * kXovTile));

    const bool direct = !multi && chunk_layout(ctx);         // the native buffer is [R][nch] chunks already
    const char* no_lds = std::getenv("RRRMC_XOV_NO_LDS_HIST");             // tests: one global atomic per counted pair
    const bool lds_bins = hist && xov_hist_in_lds(N, no_lds && no_lds[0] == '1');
    int64_t budget = kXovPackBytes;
    if (const char* e = std::getenv("RRRMC_XOV_PACK_BYTES"); e && std::atoll(e) > 0) budget = std::atoll(e);      // tests: small batches
    const int64_t max_distinct = direct ? 2 * npairs : xov_max_distinct(R, nch, budget);
    const size_t slot_words = (size_t)R * (size_t)nch;

    HIP_TRY(ctx, hipSetDevice(ex->device));
    if (hist) {
        HIP_TRY(ctx, hipStreamSynchronize(ex->stream));
        if (dev_grow(ex, ex->xov_hist, ex->xov_hist_cap, (size_t)N + 1) != hipSuccess) return fail(ctx, RRRMC_ERR_NOMEM, "cannot allocate the overlap histogram");
        HIP_TRY(ctx, hipMemsetAsync(ex->xov_hist, 0, sizeof(unsigned long long) * ((size_t)N + 1), ex->stream));
    }
    std::vector<uint64_t> gathered;                           // multi-device: one slot's rows of every shard
    for (int64_t p0 = 0; p0 < npairs;) {
        const XovBatch bt = xov_next_batch(slotA, slotB, p0, npairs, max_distinct);
        const size_t nd = bt.slots.size(), np = (size_t)(bt.p1 - bt.p0);
        p0 = bt.p1;
        HIP_TRY(ctx, hipSetDevice(ex->device));
        HIP_TRY(ctx, hipStreamSynchronize(ex->stream));      // the buffers below may move
        if (!direct && dev_grow(ex, ex->xov_pk, ex->xov_pk_cap, nd * slot_words) != hipSuccess)
            return fail(ctx, RRRMC_ERR_NOMEM, "cannot allocate %zu bytes for the packed rows of %zu slots", 8 * nd * slot_words, nd);
        const size_t tab_bytes = sizeof(void*) * nd + sizeof(int32_t) * 2 * np;
        if (dev_grow_bytes(ex, ex->xov_tab, ex->xov_tab_cap, tab_bytes) != hipSuccess) return fail(ctx, RRRMC_ERR_NOMEM, "cannot allocate the slot-pair table");
        if (!hist && dev_grow(ex, ex->xov_q, ex->xov_q_cap, np * (size_t)nA * (size_t)nB) != hipSuccess)
            return fail(ctx, RRRMC_ERR_NOMEM, "cannot allocate %zu bytes for the overlap matrices", 4 * np * (size_t)nA * (size_t)nB);
        // one packed copy per distinct slot of the batch
        std::vector<uint8_t> tab(tab_bytes);
        for (size_t s = 0; s < nd; ++s) {
            const void* rowp = nullptr;
            if (direct) {
                rowp = xov_slot_native(ctx, bt.slots[s]);
            } else if (!multi) {
                const int32_t rc = pack_native(ctx, xov_slot_native(ctx, bt.slots[s]), ex->xov_pk + s * slot_words);
                if (rc) return rc;
                rowp = ex->xov_pk + s * slot_words;
            } else {
                gathered.resize(slot_words);
                for (size_t d = 0; d < nkids; ++d) {
                    rrrmc_ctx* k = ctx->kids[d];
                    const int32_t rc = spins_to_chunks(k, xov_slot_native(k, bt.slots[s]), gathered.data() + (size_t)ctx->kid_r0[d] * (size_t)nch);
                    if (rc) { ctx->err = k->err; return rc; }
                }
                HIP_TRY(ctx, hipSetDevice(ex->device));
                HIP_TRY(ctx, hipMemcpy(ex->xov_pk + s * slot_words, gathered.data(), 8 * slot_words, hipMemcpyHostToDevice));
                rowp = ex->xov_pk + s * slot_words;
            }
            std::memcpy(tab.data() + sizeof(void*) * s, &rowp, sizeof(void*));
        }
        std::memcpy(tab.data() + sizeof(void*) * nd, bt.ia.data(), sizeof(int32_t) * np);
        std::memcpy(tab.data() + sizeof(void*) * nd + sizeof(int32_t) * np, bt.ib.data(), sizeof(int32_t) * np);
        HIP_TRY(ctx, hipMemcpyAsync(ex->xov_tab, tab.data(), tab_bytes, hipMemcpyHostToDevice, ex->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ex->stream));      // tab is pageable host memory
        const unsigned long long* const* d_rows = (const unsigned long long* const*)ex->xov_tab;
        const int32_t* d_ia = (const int32_t*)(ex->xov_tab + sizeof(void*) * nd);
        const int32_t* d_ib = d_ia + np;
        const dim3 grid((unsigned)xov_tiles(nB), (unsigned)xov_tiles(nA), (unsigned)np);
        if (hist)
            hipLaunchKernelGGL(xov_tile_kernel<true>, grid, dim3(kXovThreads), lds_bins ? sizeof(uint32_t) * ((size_t)N + 1) : 0, ex->stream, d_rows, d_ia, d_ib,
                               (int)N, (int)nch, 0, (int)R, 0, (int)R, (int32_t*)nullptr, ex->xov_hist, lds_bins ? 1 : 0);
        else
            hipLaunchKernelGGL(xov_tile_kernel<false>, grid, dim3(kXovThreads), 0, ex->stream, d_rows, d_ia, d_ib,
                               (int)N, (int)nch, (int)a0, (int)nA, (int)b0, (int)nB, ex->xov_q, (unsigned long long*)nullptr, 0);
        HIP_TRY(ctx, hipGetLastError());
        if (!hist) {
            HIP_TRY(ctx, hipMemcpyAsync(q_out + (size_t)bt.p0 * (size_t)nA * (size_t)nB, ex->xov_q, sizeof(int32_t) * np * (size_t)nA * (size_t)nB,
                                        hipMemcpyDeviceToHost, ex->stream));
            HIP_TRY(ctx, hipStreamSynchronize(ex->stream));
        }
    }
    if (hist) {
        static_assert(sizeof(unsigned long long) == sizeof(int64_t), "the histogram bins are read back as int64");
        HIP_TRY(ctx, hipMemcpyAsync(hist_out, ex->xov_hist, sizeof(int64_t) * ((size_t)N + 1), hipMemcpyDeviceToHost, ex->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ex->stream));
    }
    return RRRMC_OK;
}

}  // namespace
