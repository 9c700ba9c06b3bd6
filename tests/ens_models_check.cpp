// Prints the ensemble-model table of rrrmc.jl_amd/csrc/ens_models.hpp in both directions, for tests/test_ens_models_cpu.py:
//   "M <model id> <family> <slice kind>" for every model id 0 .. 47, then
//   "P <family> <slice kind> <model id>" for every family 0 .. 3 and slice kind -1 .. 10.
// Plain C++ (no HIP); built with g++ -fsanitize=address,undefined.
#include <stdio.h>

#include "../include/rrrmc_hip.h"
#include "../rrrmc.jl_amd/csrc/ens_models.hpp"

int main()
{
    using namespace rrrmc;
    static_assert(ens_family(RRRMC_MODEL_TLE_SAT) == ENS_TLE && ens_slice(RRRMC_MODEL_LE_COMM_QU) == RRRMC_RE_SLICE_COMM_QU, "the lookups are constexpr");
    static_assert(ens_model(ENS_TLE, RRRMC_RE_SLICE_PERC_STEP) == kEnsNoModel && ens_family(RRRMC_MODEL_QUANT_RRG) == ENS_NONE, "the lookups are constexpr");
    for (int model = 0; model <= 47; ++model) printf("M %d %d %d\n", model, (int)ens_family(model), (int)ens_slice(model));
    for (int family = 0; family <= 3; ++family)
        for (int slice = -1; slice <= 10; ++slice) printf("P %d %d %d\n", family, slice, (int)ens_model(family, slice));
    return 0;
}
