// mcl_buffers.h -- device and pinned buffers that own their memory.  Every buffer of the library is one of these: the engine's
// (struct mcl_engine), the clustering's, the communicator's, the group's and the side calls'.  This is the one file of csrc/
// that allocates or frees device or pinned memory.  Host code only.
#pragma once
#include "../../include/mcl_hip_engine.h"

#include <hip/hip_runtime.h>

#include <cstddef>
#include <string>

struct mcl_engine;
namespace mcl_host {
int fail(mcl_engine *h, int code, const std::string &msg);     // mcl_engine.hip: the engine's error text (h may be null)
}

// `cap` elements at `p`, freed with the buffer.  reserve: room for `want` elements -- nothing when they are there, else the old
// memory is dropped and new asked for (the contents are not kept).  A failure is the engine's error and leaves p null, cap 0.
// drop + reserve: memory of exactly that size.  Moving (a container of buffers) leaves the source empty.
template <class T, class Mem>
struct Buf {
    T *p = nullptr;
    size_t cap = 0;
    Buf() = default;
    Buf(const Buf &) = delete;
    Buf &operator=(const Buf &) = delete;
    Buf(Buf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    Buf &operator=(Buf &&o) noexcept
    {
        if (this != &o) { drop(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; }
        return *this;
    }
    ~Buf() { drop(); }
    void drop()
    {
        if (p) Mem::release(p);
        p = nullptr;
        cap = 0;
    }
    // bytes: the caller's count of what was ever asked of the device (never reduced by a free)
    int reserve(mcl_engine *h, size_t want, size_t *bytes = nullptr)
    {
        if (want <= cap) return MCL_OK;
        drop();
        const int rc = Mem::alloc(h, (void **)&p, want * sizeof(T));
        if (rc) { p = nullptr; return rc; }
        cap = want;
        if (bytes) *bytes += want * sizeof(T);
        return MCL_OK;
    }
    operator T *() const { return p; }
    T *operator->() const { return p; }
};
struct DeviceMem {
    static int alloc(mcl_engine *h, void **p, size_t n)
    {
        const hipError_t e = hipMalloc(p, n);
        return e == hipSuccess ? MCL_OK : mcl_host::fail(h, MCL_ERR_HIP, std::string("hipMalloc(p, n): ") + hipGetErrorString(e));
    }
    static void release(void *p) { (void)hipFree(p); }
};
struct PinnedMem {
    static int alloc(mcl_engine *h, void **p, size_t n)
    {
        const hipError_t e = hipHostMalloc(p, n);
        return e == hipSuccess ? MCL_OK : mcl_host::fail(h, MCL_ERR_HIP, std::string("hipHostMalloc(p, n): ") + hipGetErrorString(e));
    }
    static void release(void *p) { (void)hipHostFree(p); }
};
template <class T> using DevBuf = Buf<T, DeviceMem>;
template <class T> using HostBuf = Buf<T, PinnedMem>;       // pinned staging: not counted in any byte counter
