// Prints what rrrmc.jl_amd/csrc/ens_models.hpp says about the ensemble models over sparse Float64 slices and about their surroundings, for
// tests/test_sparse_ens_models_cpu.py:
//   "M <model id> <family> <slice kind>" for every model id 48 .. 101, then
//   "P <family> <slice kind> <model id>" for every family 0 .. 3 and slice kind 11 .. 13.
// Plain C++ (no HIP); built with g++ -fsanitize=address,undefined.
#include <stdio.h>

#include "../include/rrrmc_hip.h"
#include "../rrrmc.jl_amd/csrc/ens_models.hpp"

int main()
{
    using namespace rrrmc;
    static_assert(RRRMC_RE_SLICE_SPARSE_F64 == 12, "the ABI number of the slice kind");
    static_assert(RRRMC_MODEL_RE_SPARSE_F64 == 67 && RRRMC_MODEL_LE_SPARSE_F64 == 68 && RRRMC_MODEL_TLE_SPARSE_F64 == 69, "the ABI numbers of the models");
    static_assert(ens_family(RRRMC_MODEL_TLE_SPARSE_F64) == ENS_TLE && ens_slice(RRRMC_MODEL_RE_SPARSE_F64) == RRRMC_RE_SLICE_SPARSE_F64, "the lookups are constexpr");
    for (int model = 48; model <= 101; ++model) printf("M %d %d %d\n", model, (int)ens_family(model), (int)ens_slice(model));
    for (int family = 0; family <= 3; ++family)
        for (int slice = 11; slice <= 13; ++slice) printf("P %d %d %d\n", family, slice, (int)ens_model(family, slice));
    return 0;
}
