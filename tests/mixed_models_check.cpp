// Prints what rrrmc.jl_amd/csrc/mixed_models.hpp decides, for tests/test_mixed_cpu.py:
//   "G <kind> <group>"            the storage group of every kind -2 .. 15 (-1 GraphEmpty, -2 no component kind);
//   "W <model id> <wrap>"         the wrap of every model id 0 .. 110, and "V <wrap> <model id>" the other way for wrap -1 .. 3;
//   "N <mask>"                    the uploads a list of all six groups plus GraphPercXEntr waits for;
//   "C <case> <code> <message>"   every create-time check, one case per line (code 0: accepted).
// Plain C++ (no HIP); built with g++ -fsanitize=address,undefined.
#include <stdio.h>

#include <initializer_list>
#include <vector>

#include "../include/rrrmc_hip.h"
#include "../rrrmc.jl_amd/csrc/mixed_models.hpp"

using namespace rrrmc;

static void check(const char* name, std::initializer_list<int32_t> kinds, int32_t wrap, int64_t N, int64_t K, int64_t K2, int64_t R, uint32_t replica0)
{
    std::vector<int32_t> k(kinds);                          // (heap storage: a read past the list is the sanitizer's to find)
    char msg[320] = "";
    const int32_t rc = mixed_check_create(k.data(), (int32_t)k.size(), wrap, N, K, K2, R, replica0, msg, sizeof msg);
    printf("C %s %d %s\n", name, rc, msg);
}

int main()
{
    static_assert(mixed_group(RRRMC_RE_SLICE_PERC_XENTR) == MG_PERC && mixed_group(RRRMC_RE_SLICE_MIXED) == MG_BAD && mixed_group(7) == MG_BAD, "the lookups are constexpr");
    static_assert(mixed_wrap(RRRMC_MODEL_MIXED_ASF) == 2 && mixed_wrap(RRRMC_MODEL_XENTR_ASF) == -1 && mixed_model(1) == RRRMC_MODEL_MIXED_AF, "the lookups are constexpr");
    for (int kind = -2; kind <= 15; ++kind) printf("G %d %d\n", kind, (int)mixed_group(kind));
    for (int model = 0; model <= 110; ++model) printf("W %d %d\n", model, (int)mixed_wrap(model));
    for (int wrap = -1; wrap <= 3; ++wrap) printf("V %d %d\n", wrap, (int)mixed_model(wrap));
    {
        MixedList L{};
        for (int32_t k : {1, 2, 11, 5, 8, 12, 0}) L.kind[L.n++] = k;
        printf("N %u\n", mixed_need_mask(L));
        printf("H %d %d %d %d\n", (int)mixed_list_has(L, 11), (int)mixed_list_has(L, 3), (int)mixed_list_has_group(L, MG_PERC), (int)mixed_list_has_group(L, MG_SAT));
    }
    const int E = 0, SK = 1, SKN = 2, PS = 3, PL = 4, CS = 5, CR = 6, SAT = 8, CQ = 9, PX = 11, SPF = 12, MIX = 13;
    check("ok_all_groups", {SK, SKN, PS, CS, SAT, SPF}, 0, 15, 4, 3, 33, 0);
    check("ok_seven_with_empties", {E, SK, E, SKN, E, SAT, E}, 2, 8, 0, 0, 1, 32);
    check("ok_relu_even", {SPF, CR, SK, E}, 1, 8, 6, 2, 1, 0);
    check("ok_xentr", {PX, SK}, 0, 33, 0, 0, 1, 0);
    check("ok_qu", {CQ, SAT}, 0, 16, 0, 4, 1, 0);
    check("ok_n_max", {SK, SAT}, 0, 65535, 0, 0, 1, 0);
    check("one_component", {SK}, 0, 15, 0, 0, 1, 0);
    check("eight_components", {E, E, E, E, E, E, E, SK}, 0, 15, 0, 0, 1, 0);
    check("bad_wrap", {SK, SAT}, 3, 15, 0, 0, 1, 0);
    check("zero_n", {SK, SAT}, 0, 0, 0, 0, 1, 0);
    check("zero_r", {SK, SAT}, 0, 15, 0, 0, 0, 0);
    check("kind_7", {SK, 7}, 0, 15, 0, 0, 1, 0);
    check("kind_10", {10, SK}, 0, 15, 0, 0, 1, 0);
    check("kind_negative", {SK, -1}, 0, 15, 0, 0, 1, 0);
    check("nested", {SK, MIX}, 0, 15, 0, 0, 1, 0);
    check("dup_sk", {SK, SAT, SK}, 0, 15, 0, 0, 1, 0);
    check("dup_skn", {SKN, SKN}, 0, 15, 0, 0, 1, 0);
    check("dup_perc", {PS, PL}, 0, 15, 0, 0, 1, 0);
    check("dup_perc_xentr", {PX, E, PS}, 0, 15, 0, 0, 1, 0);
    check("dup_comm", {CS, CQ}, 0, 15, 0, 3, 1, 0);
    check("dup_sat", {SAT, SK, SAT}, 0, 15, 0, 0, 1, 0);
    check("dup_spf", {SPF, SPF}, 0, 15, 3, 0, 1, 0);
    check("perc_even_n", {SK, PS}, 0, 16, 0, 0, 1, 0);
    check("perc_even_n_next_to_relu", {PL, CR}, 0, 8, 0, 2, 1, 0);
    check("relu_odd_n_next_to_perc", {PL, CR}, 0, 15, 0, 3, 1, 0);
    check("perc_n_max", {SK, PX}, 0, 32769, 0, 0, 1, 0);
    check("comm_k2_zero", {CS, SK}, 0, 15, 0, 0, 1, 0);
    check("comm_not_multiple", {CS, SK}, 0, 15, 0, 4, 1, 0);
    check("comm_step_even_k2", {CS, SK}, 0, 12, 0, 4, 1, 0);
    check("comm_relu_odd_k1", {CR, SK}, 0, 12, 0, 4, 1, 0);
    check("comm_n_max", {CQ, SK}, 0, 32768, 0, 4, 1, 0);
    check("spf_k0", {SPF, SK}, 0, 15, 0, 0, 1, 0);
    check("spf_k9", {SPF, SK}, 0, 15, 9, 0, 1, 0);
    check("k_ignored_without_spf", {SKN, SK}, 0, 15, 9, 7, 1, 0);
    check("n_max", {SK, SAT}, 0, 65536, 0, 0, 1, 0);
    check("replica0", {SK, SAT}, 0, 15, 0, 0, 1, 16);
    {
        char msg[64];
        printf("C null_kinds %d\n", mixed_check_create(nullptr, 2, 0, 15, 0, 0, 1, 0, msg, sizeof msg));
    }
    return 0;
}
