// The GraphAddFields / GraphAddSubFields models of the ABI (include/rrrmc_hip.h): which wrapper a model id names and what kind of graph g
// it wraps.  One table, read in both directions, beside the ensembles' (ens_models.hpp), which it leaves alone.  Plain C++: included by
// rrrmc_hip.hip ahead of the host headers, and compiled on its own with g++ -fsanitize=address,undefined by tests/af_models_check.cpp.
#pragma once
#include <stdint.h>

#include "../../include/rrrmc_hip.h"
#include "ens_models.hpp"

namespace rrrmc {

enum AfFamily { AF_NONE = 0, AF_ADD = 1, AF_ADDSUB = 2 };      // GraphAddFields, GraphAddSubFields
constexpr int32_t kAfNoModel = 0;                           // no rrrmc_model is 0
constexpr int32_t kAfNoSlice = -1;                          // no rrrmc_re_slice is negative

struct AfModel { int32_t model; AfFamily family; int32_t slice; };
constexpr AfModel kAfModels[] = {
    {RRRMC_MODEL_AF_EMPTY, AF_ADD, RRRMC_RE_SLICE_EMPTY},
    {RRRMC_MODEL_AF_SK, AF_ADD, RRRMC_RE_SLICE_SK},
    {RRRMC_MODEL_AF_SKN, AF_ADD, RRRMC_RE_SLICE_SKN},
    {RRRMC_MODEL_AF_PERC_STEP, AF_ADD, RRRMC_RE_SLICE_PERC_STEP},
    {RRRMC_MODEL_AF_PERC_LINEAR, AF_ADD, RRRMC_RE_SLICE_PERC_LINEAR},
    {RRRMC_MODEL_AF_COMM_STEP, AF_ADD, RRRMC_RE_SLICE_COMM_STEP},
    {RRRMC_MODEL_AF_COMM_RELU, AF_ADD, RRRMC_RE_SLICE_COMM_RELU},
    {RRRMC_MODEL_AF_SAT, AF_ADD, RRRMC_RE_SLICE_SAT},
    {RRRMC_MODEL_AF_COMM_QU, AF_ADD, RRRMC_RE_SLICE_COMM_QU},
    {RRRMC_MODEL_ASF_EMPTY, AF_ADDSUB, RRRMC_RE_SLICE_EMPTY},
    {RRRMC_MODEL_ASF_SK, AF_ADDSUB, RRRMC_RE_SLICE_SK},
    {RRRMC_MODEL_ASF_SKN, AF_ADDSUB, RRRMC_RE_SLICE_SKN},
    {RRRMC_MODEL_ASF_PERC_STEP, AF_ADDSUB, RRRMC_RE_SLICE_PERC_STEP},
    {RRRMC_MODEL_ASF_PERC_LINEAR, AF_ADDSUB, RRRMC_RE_SLICE_PERC_LINEAR},
    {RRRMC_MODEL_ASF_COMM_STEP, AF_ADDSUB, RRRMC_RE_SLICE_COMM_STEP},
    {RRRMC_MODEL_ASF_COMM_RELU, AF_ADDSUB, RRRMC_RE_SLICE_COMM_RELU},
    {RRRMC_MODEL_ASF_SAT, AF_ADDSUB, RRRMC_RE_SLICE_SAT},
    {RRRMC_MODEL_ASF_COMM_QU, AF_ADDSUB, RRRMC_RE_SLICE_COMM_QU},
    {RRRMC_MODEL_XENTR_AF, AF_ADD, RRRMC_RE_SLICE_PERC_XENTR},
    {RRRMC_MODEL_XENTR_ASF, AF_ADDSUB, RRRMC_RE_SLICE_PERC_XENTR},
};

// the wrapper of a model id; AF_NONE for every other model
constexpr AfFamily af_family(int32_t model)
{
    for (const AfModel& e : kAfModels)
        if (e.model == model) return e.family;
    return AF_NONE;
}
// the kind of g (rrrmc_re_slice) of a wrapper model; kAfNoSlice for every other model
constexpr int32_t af_slice(int32_t model)
{
    for (const AfModel& e : kAfModels)
        if (e.model == model) return e.slice;
    return kAfNoSlice;
}
// the model of (wrapper, kind of g); kAfNoModel where there is none
constexpr int32_t af_model(int32_t family, int32_t slice_kind)
{
    for (const AfModel& e : kAfModels)
        if (e.family == family && e.slice == slice_kind) return e.model;
    return kAfNoModel;
}
// the slice kind of any model that is made of slices of one graph: an ensemble's, or the g of a wrapper; -1 for every other model
constexpr int32_t model_slice(int32_t model)
{
    return ens_slice(model) != kEnsNoSlice ? ens_slice(model) : af_slice(model);
}

}  // namespace rrrmc
