// Device memory a context owns: one registry per context, so that destroying the context frees whatever it allocated without naming a buffer.
//
// The fields of the context stay raw pointers (kernels and parameter structs take them as they are); the registry keeps the pointer VALUES
// of the live allocations, not the addresses of the fields, so a pointer may live in an array or in a std::vector that moves.
// Nothing here knows HIP: the includer declares `dev_err_t` (zero is success) before this header and defines the two raw hooks below
// (rrrmc_hip.hip: hipMalloc / hipFree; tests/dev_mem_check.cpp: malloc / free with a count of the live blocks).
// `Ctx` is any type with a member `DevMem mem`.
#pragma once

#include <cstddef>
#include <vector>

dev_err_t dev_raw_alloc(void** p, size_t bytes);
void dev_raw_free(void* p);

struct DevMem { std::vector<void*> blocks; };

// p = a new block of `bytes` bytes, owned by ctx; p == nullptr and nothing registered when the allocation fails.  The byte-sized form is for
// buffers whose element width is chosen at run time.
template <typename Ctx, typename T> dev_err_t dev_alloc_bytes(Ctx* ctx, T*& p, size_t bytes)
{
    p = nullptr;
    std::vector<void*>& b = ctx->mem.blocks;
    b.push_back(nullptr);          // the registry's room first: once the block exists, recording it cannot fail
    const dev_err_t e = dev_raw_alloc(&b.back(), bytes);
    if (e != dev_err_t(0)) { b.pop_back(); return e; }
    p = static_cast<T*>(b.back());
    return e;
}
template <typename Ctx, typename T> dev_err_t dev_alloc(Ctx* ctx, T*& p, size_t count) { return dev_alloc_bytes(ctx, p, sizeof(T) * count); }

// frees p if ctx owns it, and nulls it; a null pointer, or one the registry does not hold, is not freed
template <typename Ctx, typename T> void dev_free(Ctx* ctx, T*& p)
{
    std::vector<void*>& b = ctx->mem.blocks;
    for (size_t i = b.size(); p && i-- > 0;)
        if (b[i] == static_cast<void*>(p)) { dev_raw_free(b[i]); b[i] = b.back(); b.pop_back(); break; }
    p = nullptr;
}

// grow on demand: p holds at least `need` elements (dev_grow) or bytes (dev_grow_bytes) afterwards; `cap` is what it holds.  The old contents
// are not kept.  A failed allocation leaves p == nullptr and cap == 0.
template <typename Ctx, typename T> dev_err_t dev_grow_bytes(Ctx* ctx, T*& p, size_t& cap, size_t need, size_t unit = 1)
{
    if (need <= cap) return dev_err_t(0);
    dev_free(ctx, p);
    cap = 0;
    const dev_err_t e = dev_alloc_bytes(ctx, p, unit * need);
    if (e == dev_err_t(0)) cap = need;
    return e;
}
template <typename Ctx, typename T> dev_err_t dev_grow(Ctx* ctx, T*& p, size_t& cap, size_t need) { return dev_grow_bytes(ctx, p, cap, need, sizeof(T)); }

// everything ctx still owns (the fields that pointed there are the caller's to forget: the context is being destroyed)
template <typename Ctx> void dev_free_all(Ctx* ctx)
{
    for (void* q : ctx->mem.blocks) dev_raw_free(q);
    ctx->mem.blocks.clear();
}
