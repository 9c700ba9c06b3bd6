// GraphMixed (src/graphs/Mixed.jl) on the ABI (include/rrrmc_hip.h): the component list of a mixed graph, the storage group of every kind,
// the three models (the stand-alone mix and the two field wrappers over it) and every check rrrmc_ctx_create_mixed makes before it touches
// a device.  Plain C++: included by rrrmc_hip.hip ahead of the host headers, by the kernels (MixedList is a kernel argument), and compiled
// on its own with g++ -fsanitize=address,undefined by tests/mixed_models_check.cpp.
#pragma once
#include <stdint.h>
#include <stdio.h>

#include "../../include/rrrmc_hip.h"

namespace rrrmc {

constexpr int kMixedMin = 2, kMixedMax = 7;                 // components of one mix (Mixed.jl:22 asks for at least 2)
constexpr int64_t kMixedNmax = 65535;                       // the wrappers' bound (16-bit site ids in the sampler's tree walk)
constexpr int64_t kMixedPatNmax = 32767;                    // perceptrons and committee machines: 16-bit stabilities (kPercNmax, kCommNmax)
constexpr int64_t kMixedKmax = 8;                           // sparse Float64 components (kContKmax)

// the list as the kernels take it: the same for every chain of a launch, so a switch over kind[c] is wave-uniform
struct MixedList { int32_t n; int32_t kind[kMixedMax]; };

// A context holds one upload of each storage group, so a mix takes at most one component from each; GraphEmpty stores nothing
enum MixedGroup { MG_EMPTY = -1, MG_SK = 0, MG_SKN = 1, MG_PERC = 2, MG_COMM = 3, MG_SAT = 4, MG_SPF = 5, MG_BAD = -2 };
constexpr int kMixedGroups = 6;
constexpr int kMixedTableBit = 6;                           // beside the groups' bits: GraphPercXEntr's loss table, a second upload of MG_PERC

struct MixedKind { int32_t kind; MixedGroup group; };
constexpr MixedKind kMixedKinds[] = {
    {RRRMC_RE_SLICE_EMPTY, MG_EMPTY},
    {RRRMC_RE_SLICE_SK, MG_SK},
    {RRRMC_RE_SLICE_SKN, MG_SKN},
    {RRRMC_RE_SLICE_PERC_STEP, MG_PERC}, {RRRMC_RE_SLICE_PERC_LINEAR, MG_PERC}, {RRRMC_RE_SLICE_PERC_XENTR, MG_PERC},
    {RRRMC_RE_SLICE_COMM_STEP, MG_COMM}, {RRRMC_RE_SLICE_COMM_RELU, MG_COMM}, {RRRMC_RE_SLICE_COMM_QU, MG_COMM},
    {RRRMC_RE_SLICE_SAT, MG_SAT},
    {RRRMC_RE_SLICE_SPARSE_F64, MG_SPF},
};
// the storage group of a component kind; MG_BAD for anything that is no component kind (RRRMC_RE_SLICE_MIXED among them: no nesting)
constexpr MixedGroup mixed_group(int32_t kind)
{
    for (const MixedKind& e : kMixedKinds)
        if (e.kind == kind) return e.group;
    return MG_BAD;
}
// the kinds of a group, as the refusal of a duplicate names them
constexpr const char* mixed_group_name(int group)
{
    return group == MG_SK ? "{SK}" : group == MG_SKN ? "{SKN}" : group == MG_PERC ? "{PERC_STEP, PERC_LINEAR, PERC_XENTR}"
           : group == MG_COMM ? "{COMM_STEP, COMM_RELU, COMM_QU}" : group == MG_SAT ? "{SAT}" : group == MG_SPF ? "{SPARSE_F64}" : "{}";
}
// the upload call that fills a group (bit kMixedTableBit: the loss table)
constexpr const char* mixed_upload_name(int bit)
{
    return bit == MG_SK ? "rrrmc_set_couplings_bits" : bit == MG_SKN ? "rrrmc_set_couplings_dense" : bit == MG_PERC ? "rrrmc_set_patterns"
           : bit == MG_COMM ? "rrrmc_set_comm_patterns" : bit == MG_SAT ? "rrrmc_set_clauses" : bit == MG_SPF ? "rrrmc_set_graph_f64"
           : bit == kMixedTableBit ? "rrrmc_set_loss_table" : "nothing";
}

// wrap: 0 GraphMixed itself, 1 GraphAddFields(h, mixed), 2 GraphAddSubFields(h, mixed); -1 for every other model
constexpr int32_t mixed_wrap(int32_t model)
{
    return model == RRRMC_MODEL_MIXED ? 0 : model == RRRMC_MODEL_MIXED_AF ? 1 : model == RRRMC_MODEL_MIXED_ASF ? 2 : -1;
}
constexpr int32_t mixed_model(int32_t wrap)
{
    return wrap == 0 ? RRRMC_MODEL_MIXED : wrap == 1 ? RRRMC_MODEL_MIXED_AF : wrap == 2 ? RRRMC_MODEL_MIXED_ASF : 0;
}
constexpr bool mixed_list_has(const MixedList& L, int32_t kind)
{
    for (int c = 0; c < L.n; ++c)
        if (L.kind[c] == kind) return true;
    return false;
}
constexpr bool mixed_list_has_group(const MixedList& L, int group)
{
    for (int c = 0; c < L.n; ++c)
        if (mixed_group(L.kind[c]) == group) return true;
    return false;
}
// the uploads a list waits for, one bit per group and kMixedTableBit
constexpr uint32_t mixed_need_mask(const MixedList& L)
{
    uint32_t m = 0;
    for (int c = 0; c < L.n; ++c) {
        const int g = mixed_group(L.kind[c]);
        if (g >= 0) m |= 1u << g;
        if (L.kind[c] == RRRMC_RE_SLICE_PERC_XENTR) m |= 1u << kMixedTableBit;
    }
    return m;
}

// Every check of rrrmc_ctx_create_mixed that needs no device.  0: fine; RRRMC_ERR_INVALID_ARG / RRRMC_ERR_UNSUPPORTED with the text in msg.
inline int32_t mixed_check_create(const int32_t* kinds, int32_t nkinds, int32_t wrap, int64_t N, int64_t K, int64_t K2, int64_t R, uint32_t replica0,
                                  char* msg, size_t len)
{
    auto bad = [&](int32_t code) { return code; };
    if (!kinds) { snprintf(msg, len, "GraphMixed: kinds is NULL"); return bad(RRRMC_ERR_INVALID_ARG); }
    if (nkinds < kMixedMin) { snprintf(msg, len, "GraphMixed: at least 2 base graphs needed, given: %d", nkinds); return bad(RRRMC_ERR_INVALID_ARG); }
    if (nkinds > kMixedMax) { snprintf(msg, len, "GraphMixed: %d components: the mixed kernels cover <= %d", nkinds, kMixedMax); return bad(RRRMC_ERR_UNSUPPORTED); }
    if (wrap < 0 || wrap > 2) { snprintf(msg, len, "wrap must be 0 (GraphMixed), 1 (GraphAddFields) or 2 (GraphAddSubFields), given: %d", wrap); return bad(RRRMC_ERR_INVALID_ARG); }
    if (N < 1 || R < 1) { snprintf(msg, len, "GraphMixed: N and R must be >= 1"); return bad(RRRMC_ERR_INVALID_ARG); }
    uint32_t seen = 0;
    for (int32_t c = 0; c < nkinds; ++c) {
        const int g = mixed_group(kinds[c]);
        if (kinds[c] == RRRMC_RE_SLICE_MIXED) { snprintf(msg, len, "GraphMixed: component %d is a GraphMixed: a mix does not nest", c); return bad(RRRMC_ERR_INVALID_ARG); }
        if (g == MG_BAD) { snprintf(msg, len, "GraphMixed: component %d: %d is no component kind (RRRMC_RE_SLICE_*)", c, kinds[c]); return bad(RRRMC_ERR_INVALID_ARG); }
        if (g == MG_EMPTY) continue;
        if (seen & (1u << g)) {
            snprintf(msg, len, "GraphMixed: component %d is a second graph of the storage group %s: a context holds one upload of each group", c, mixed_group_name(g));
            return bad(RRRMC_ERR_UNSUPPORTED);
        }
        seen |= 1u << g;
    }
    for (int32_t c = 0; c < nkinds; ++c) {
        const int g = mixed_group(kinds[c]);
        if (g == MG_PERC) {
            if (N % 2 == 0) { snprintf(msg, len, "component %d (a perceptron): N must be odd, given: %lld", c, (long long)N); return bad(RRRMC_ERR_INVALID_ARG); }
            if (N > kMixedPatNmax) { snprintf(msg, len, "component %d: N = %lld: the perceptron kernels cover N <= %lld (16-bit stabilities)", c, (long long)N, (long long)kMixedPatNmax); return bad(RRRMC_ERR_UNSUPPORTED); }
        }
        if (g == MG_COMM) {
            const bool even = kinds[c] != RRRMC_RE_SLICE_COMM_STEP;
            const char* par = even ? "even" : "odd";
            if (K2 < 1 || N % K2 != 0) {
                snprintf(msg, len, "component %d (a committee machine) takes N = K1*K2 with N %% K2 == 0, given N = %lld, K2 = %lld", c, (long long)N, (long long)K2);
                return bad(RRRMC_ERR_INVALID_ARG);
            }
            const int64_t K1 = N / K2;
            if ((K1 % 2 == 0) != even) { snprintf(msg, len, "component %d (a committee machine): K1 must be %s, given: %lld", c, par, (long long)K1); return bad(RRRMC_ERR_INVALID_ARG); }
            if ((K2 % 2 == 0) != even) { snprintf(msg, len, "component %d (a committee machine): K2 must be %s, given: %lld", c, par, (long long)K2); return bad(RRRMC_ERR_INVALID_ARG); }
            if (N > kMixedPatNmax) { snprintf(msg, len, "component %d: N = K1*K2 = %lld: the committee machine kernels cover N <= %lld (16-bit stabilities)", c, (long long)N, (long long)kMixedPatNmax); return bad(RRRMC_ERR_UNSUPPORTED); }
        }
        if (g == MG_SPF) {
            if (K < 1) { snprintf(msg, len, "component %d (a sparse Float64 graph): K must be >= 1, given: %lld", c, (long long)K); return bad(RRRMC_ERR_INVALID_ARG); }
            if (K > kMixedKmax) { snprintf(msg, len, "component %d: K = %lld: the Float64 sparse slice kernels cover K <= %lld", c, (long long)K, (long long)kMixedKmax); return bad(RRRMC_ERR_UNSUPPORTED); }
        }
    }
    if (N > kMixedNmax) { snprintf(msg, len, "N = %lld: the GraphMixed kernels cover N <= %lld", (long long)N, (long long)kMixedNmax); return bad(RRRMC_ERR_UNSUPPORTED); }
    if (replica0 % 32) { snprintf(msg, len, "replica0 must be a multiple of 32 (given %u)", replica0); return bad(RRRMC_ERR_INVALID_ARG); }
    return RRRMC_OK;
}

}  // namespace rrrmc
