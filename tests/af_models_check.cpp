// Prints the GraphAddFields / GraphAddSubFields model table of rrrmc.jl_amd/csrc/af_models.hpp in both directions, for
// tests/test_add_fields_cpu.py:
//   "M <model id> <wrapper> <kind of g> <model_slice>" for every model id 0 .. 99, then
//   "P <wrapper> <kind of g> <model id>" for every wrapper 0 .. 2 and kind -1 .. 10.
// Plain C++ (no HIP); built with g++ -fsanitize=address,undefined.
#include <stdio.h>

#include "../include/rrrmc_hip.h"
#include "../rrrmc.jl_amd/csrc/af_models.hpp"

int main()
{
    using namespace rrrmc;
    static_assert(af_family(RRRMC_MODEL_ASF_SAT) == AF_ADDSUB && af_slice(RRRMC_MODEL_AF_COMM_QU) == RRRMC_RE_SLICE_COMM_QU, "the lookups are constexpr");
    static_assert(af_model(AF_ADD, 7) == kAfNoModel && af_family(RRRMC_MODEL_RE_SAT) == AF_NONE && af_family(99) == AF_NONE, "the lookups are constexpr");
    static_assert(model_slice(RRRMC_MODEL_LE_SK) == RRRMC_RE_SLICE_SK && model_slice(RRRMC_MODEL_AF_SKN) == RRRMC_RE_SLICE_SKN && model_slice(RRRMC_MODEL_SAT) == -1, "ensembles and wrappers");
    for (int model = 0; model <= 99; ++model) printf("M %d %d %d %d\n", model, (int)af_family(model), (int)af_slice(model), (int)model_slice(model));
    for (int family = 0; family <= 2; ++family)
        for (int slice = -1; slice <= 10; ++slice) printf("P %d %d %d\n", family, slice, (int)af_model(family, slice));
    return 0;
}
