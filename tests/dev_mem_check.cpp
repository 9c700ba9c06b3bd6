// Stand-alone check of rrrmc.jl_amd/csrc/dev_mem.hpp (the registry of a context's device allocations), built by tests/test_dev_mem_cpu.py with
// g++ and the address / undefined-behaviour sanitizers: the raw hooks are malloc / free with a count of the live blocks, so a block that is
// never freed, or freed twice, fails the run (the sanitizer's leak and double-free reports) as well as the counts below.
// Prints "ok <scenario>" per scenario; the first failed expectation ends the program with status 1.
#include <cstdio>
#include <cstdlib>
#include <cstdint>
#include <set>
#include <vector>

typedef int dev_err_t;
#include "../rrrmc.jl_amd/csrc/dev_mem.hpp"

static std::set<void*> g_live;          // blocks the hooks have handed out and not taken back
static size_t g_allocs = 0, g_frees = 0, g_last_bytes = 0;
static bool g_fail_next = false;        // the next allocation fails (once)

#define EXPECT(cond)                                                                       \
    do {                                                                                   \
        if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } \
    } while (0)

dev_err_t dev_raw_alloc(void** p, size_t bytes)
{
    if (g_fail_next) { g_fail_next = false; return 2; }          // (p is left as it was, as hipMalloc leaves it)
    *p = std::malloc(bytes ? bytes : 1);
    EXPECT(*p != nullptr);
    g_live.insert(*p);
    ++g_allocs;
    g_last_bytes = bytes;
    return 0;
}
void dev_raw_free(void* p)
{
    EXPECT(g_live.erase(p) == 1);          // freed once, and only what a hook handed out
    ++g_frees;
    std::free(p);
}

struct Ctx {
    DevMem mem;
    double* a = nullptr;
    int32_t* b = nullptr;
    uint16_t* wide = nullptr;               // element width chosen at run time: the byte-sized form
    uint32_t* pair[2] = {nullptr, nullptr};
    std::vector<uint32_t*> list;
    double* es = nullptr;
    size_t es_cap = 0;
    unsigned long long* io = nullptr;
    size_t io_cap = 0;                      // bytes
};

static void alloc_then_free()
{
    Ctx c;
    EXPECT(dev_alloc(&c, c.a, 10) == 0 && c.a && g_last_bytes == 10 * sizeof(double));
    EXPECT(dev_alloc_bytes(&c, c.wide, 12) == 0 && c.wide && g_last_bytes == 12);
    EXPECT(g_live.size() == 2 && c.mem.blocks.size() == 2);
    c.a[9] = 1.0;                                                  // (the sanitizer checks the size)
    dev_free(&c, c.a);
    EXPECT(c.a == nullptr && g_live.size() == 1 && c.mem.blocks.size() == 1);
    dev_free(&c, c.wide);
    EXPECT(c.wide == nullptr && g_live.empty() && c.mem.blocks.empty());
    std::puts("ok alloc_then_free");
}

static void failing_alloc()
{
    Ctx c;
    EXPECT(dev_alloc(&c, c.a, 4) == 0);
    int32_t stale = 0;
    c.b = &stale;                                                  // whatever the field held is not kept on failure
    g_fail_next = true;
    EXPECT(dev_alloc(&c, c.b, 4) == 2);
    EXPECT(c.b == nullptr && c.mem.blocks.size() == 1 && c.mem.blocks[0] == c.a && g_live.size() == 1);
    dev_free_all(&c);
    EXPECT(g_live.empty());
    std::puts("ok failing_alloc");
}

static void grow()
{
    Ctx c;
    const size_t a0 = g_allocs, f0 = g_frees;
    EXPECT(dev_grow(&c, c.es, c.es_cap, 8) == 0 && c.es && c.es_cap == 8 && g_last_bytes == 8 * sizeof(double));
    double* first = c.es;
    EXPECT(dev_grow(&c, c.es, c.es_cap, 8) == 0 && dev_grow(&c, c.es, c.es_cap, 3) == 0 && dev_grow(&c, c.es, c.es_cap, 0) == 0);
    EXPECT(c.es == first && c.es_cap == 8 && g_allocs == a0 + 1 && g_frees == f0);          // need <= cap: nothing allocated
    EXPECT(dev_grow(&c, c.es, c.es_cap, 64) == 0);
    EXPECT(c.es && c.es_cap == 64 && g_live.size() == 1 && c.mem.blocks.size() == 1 && g_allocs == a0 + 2 && g_frees == f0 + 1);
    c.es[63] = 1.0;
    EXPECT(dev_grow_bytes(&c, c.io, c.io_cap, 100) == 0 && c.io_cap == 100 && g_last_bytes == 100);          // a cap in bytes
    EXPECT(dev_grow_bytes(&c, c.io, c.io_cap, 100) == 0 && g_allocs == a0 + 3);
    dev_free_all(&c);
    EXPECT(g_live.empty());
    std::puts("ok grow");
}

static void grow_that_fails()
{
    Ctx c;
    EXPECT(dev_grow(&c, c.es, c.es_cap, 8) == 0);
    const size_t f0 = g_frees;
    g_fail_next = true;
    EXPECT(dev_grow(&c, c.es, c.es_cap, 16) == 2);
    EXPECT(c.es == nullptr && c.es_cap == 0 && g_frees == f0 + 1 && g_live.empty() && c.mem.blocks.empty());          // the old block freed, once
    EXPECT(dev_grow(&c, c.es, c.es_cap, 16) == 0 && c.es && c.es_cap == 16);                                          // and the next call starts over
    dev_free_all(&c);
    EXPECT(g_live.empty());
    std::puts("ok grow_that_fails");
}

static void pointers_in_a_vector_that_moves()
{
    Ctx c;
    for (int i = 0; i < 3; ++i) { c.list.push_back(nullptr); EXPECT(dev_alloc(&c, c.list[(size_t)i], 4) == 0); }
    uint32_t* const* before = c.list.data();
    c.list.reserve(c.list.capacity() * 8 + 64);                    // the fields move: the registry holds values, not their addresses
    EXPECT(c.list.data() != before);
    for (int i = 3; i < 40; ++i) { c.list.push_back(nullptr); EXPECT(dev_alloc(&c, c.list[(size_t)i], 4) == 0); }
    EXPECT(g_live.size() == 40);
    const size_t f0 = g_frees;
    for (size_t i = 0; i < 20; ++i) dev_free(&c, c.list[i]);
    EXPECT(g_frees == f0 + 20 && g_live.size() == 20 && c.mem.blocks.size() == 20);
    dev_free_all(&c);                                              // the other twenty
    EXPECT(g_frees == f0 + 40 && g_live.empty());
    std::puts("ok pointers_in_a_vector_that_moves");
}

static void free_all_after_a_mix()
{
    Ctx c;
    EXPECT(dev_alloc(&c, c.a, 5) == 0 && dev_alloc(&c, c.b, 5) == 0 && dev_alloc_bytes(&c, c.wide, 20) == 0);
    for (int i = 0; i < 2; ++i) EXPECT(dev_alloc(&c, c.pair[i], 7) == 0);
    c.list.resize(2, nullptr);
    for (uint32_t*& l : c.list) EXPECT(dev_alloc(&c, l, 3) == 0);
    EXPECT(dev_grow(&c, c.es, c.es_cap, 4) == 0 && dev_grow(&c, c.es, c.es_cap, 9) == 0);
    g_fail_next = true;
    EXPECT(dev_grow_bytes(&c, c.io, c.io_cap, 32) == 2);
    dev_free(&c, c.b);
    EXPECT(dev_alloc(&c, c.b, 6) == 0);                            // a field allocated again after its free
    EXPECT(g_live.size() == 8 && c.mem.blocks.size() == 8);
    dev_free_all(&c);
    EXPECT(g_live.empty() && c.mem.blocks.empty());
    const size_t f0 = g_frees;
    dev_free_all(&c);                                              // a second time: nothing is registered, nothing is freed
    EXPECT(g_frees == f0);
    // the fields still hold the freed values; freeing through them is harmless too and nulls them
    dev_free(&c, c.a); dev_free(&c, c.pair[1]); dev_free(&c, c.list[0]);
    EXPECT(g_frees == f0 && c.a == nullptr && c.pair[1] == nullptr && c.list[0] == nullptr);
    std::puts("ok free_all_after_a_mix");
}

static void free_of_null_and_of_a_stranger()
{
    Ctx c, other;
    EXPECT(dev_alloc(&c, c.a, 2) == 0 && dev_alloc(&other, other.a, 2) == 0);
    const size_t f0 = g_frees;
    dev_free(&c, c.b);                                             // null
    EXPECT(c.b == nullptr && g_frees == f0);
    int32_t on_the_stack = 0;
    int32_t* stranger = &on_the_stack;
    dev_free(&c, stranger);                                        // not the registry's: not freed
    double* others = other.a;
    dev_free(&c, others);                                          // another context's block: not freed here
    EXPECT(g_frees == f0 && g_live.size() == 2 && c.mem.blocks.size() == 1 && other.mem.blocks.size() == 1);
    dev_free_all(&c);
    dev_free_all(&other);
    EXPECT(g_live.empty());
    std::puts("ok free_of_null_and_of_a_stranger");
}

int main()
{
    alloc_then_free();
    failing_alloc();
    grow();
    grow_that_fails();
    pointers_in_a_vector_that_moves();
    free_all_after_a_mix();
    free_of_null_and_of_a_stranger();
    EXPECT(g_live.empty() && g_allocs == g_frees);
    std::puts("ok all");
    return 0;
}
