// The ensemble models of the ABI (include/rrrmc_hip.h): which of the three ensembles a model id belongs to and what its slices are.
// One table, read in both directions.  Plain C++: included by rrrmc_hip.hip ahead of the host headers, and compiled on its own with
// g++ -fsanitize=address,undefined by tests/ens_models_check.cpp.
//
// A new slice kind is a row per ensemble here, an entry of AllSlices (host_ens.hpp) and the kernels' `if constexpr` branches.
#pragma once
#include <stdint.h>

#include "../../include/rrrmc_hip.h"

namespace rrrmc {

enum EnsFamily { ENS_NONE = 0, ENS_RE = 1, ENS_LE = 2, ENS_TLE = 3 };      // GraphRobustEnsemble, GraphLocalEntropy, GraphTopologicalLocalEntropy
constexpr int32_t kEnsNoModel = 0;                          // no rrrmc_model is 0
constexpr int32_t kEnsNoSlice = -1;                         // no rrrmc_re_slice is negative

struct EnsModel { int32_t model; EnsFamily family; int32_t slice; };
constexpr EnsModel kEnsModels[] = {
    {RRRMC_MODEL_RE_EMPTY, ENS_RE, RRRMC_RE_SLICE_EMPTY},
    {RRRMC_MODEL_RE_SK, ENS_RE, RRRMC_RE_SLICE_SK},
    {RRRMC_MODEL_RE_SKN, ENS_RE, RRRMC_RE_SLICE_SKN},
    {RRRMC_MODEL_RE_PERC_STEP, ENS_RE, RRRMC_RE_SLICE_PERC_STEP},
    {RRRMC_MODEL_RE_PERC_LINEAR, ENS_RE, RRRMC_RE_SLICE_PERC_LINEAR},
    {RRRMC_MODEL_RE_COMM_STEP, ENS_RE, RRRMC_RE_SLICE_COMM_STEP},
    {RRRMC_MODEL_RE_COMM_RELU, ENS_RE, RRRMC_RE_SLICE_COMM_RELU},
    {RRRMC_MODEL_RE_SAT, ENS_RE, RRRMC_RE_SLICE_SAT},
    {RRRMC_MODEL_RE_COMM_QU, ENS_RE, RRRMC_RE_SLICE_COMM_QU},
    {RRRMC_MODEL_LE_EMPTY, ENS_LE, RRRMC_RE_SLICE_EMPTY},
    {RRRMC_MODEL_LE_SK, ENS_LE, RRRMC_RE_SLICE_SK},
    {RRRMC_MODEL_LE_SKN, ENS_LE, RRRMC_RE_SLICE_SKN},
    {RRRMC_MODEL_LE_PERC_STEP, ENS_LE, RRRMC_RE_SLICE_PERC_STEP},
    {RRRMC_MODEL_LE_PERC_LINEAR, ENS_LE, RRRMC_RE_SLICE_PERC_LINEAR},
    {RRRMC_MODEL_LE_COMM_STEP, ENS_LE, RRRMC_RE_SLICE_COMM_STEP},
    {RRRMC_MODEL_LE_COMM_RELU, ENS_LE, RRRMC_RE_SLICE_COMM_RELU},
    {RRRMC_MODEL_LE_SAT, ENS_LE, RRRMC_RE_SLICE_SAT},
    {RRRMC_MODEL_LE_COMM_QU, ENS_LE, RRRMC_RE_SLICE_COMM_QU},
    {RRRMC_MODEL_TLE_EMPTY, ENS_TLE, RRRMC_RE_SLICE_EMPTY},          // (the TLE kernels cover these four slice kinds and the sparse Float64 one below)
    {RRRMC_MODEL_TLE_SK, ENS_TLE, RRRMC_RE_SLICE_SK},
    {RRRMC_MODEL_TLE_SKN, ENS_TLE, RRRMC_RE_SLICE_SKN},
    {RRRMC_MODEL_TLE_SAT, ENS_TLE, RRRMC_RE_SLICE_SAT},
    {RRRMC_MODEL_RE_SPARSE_F64, ENS_RE, RRRMC_RE_SLICE_SPARSE_F64},          // sparse Float64 slices (GraphEARE, GraphEALE, GraphEATLE)
    {RRRMC_MODEL_LE_SPARSE_F64, ENS_LE, RRRMC_RE_SLICE_SPARSE_F64},
    {RRRMC_MODEL_TLE_SPARSE_F64, ENS_TLE, RRRMC_RE_SLICE_SPARSE_F64},
};

// the ensemble of a model id; ENS_NONE for every model that is not an ensemble
constexpr EnsFamily ens_family(int32_t model)
{
    for (const EnsModel& e : kEnsModels)
        if (e.model == model) return e.family;
    return ENS_NONE;
}
// the slice kind (rrrmc_re_slice) of an ensemble model; kEnsNoSlice for every other model
constexpr int32_t ens_slice(int32_t model)
{
    for (const EnsModel& e : kEnsModels)
        if (e.model == model) return e.slice;
    return kEnsNoSlice;
}
// the model of (ensemble, slice kind); kEnsNoModel where there is none
constexpr int32_t ens_model(int32_t family, int32_t slice_kind)
{
    for (const EnsModel& e : kEnsModels)
        if (e.family == family && e.slice == slice_kind) return e.model;
    return kEnsNoModel;
}

}  // namespace rrrmc
