// dev_buf.h — the buffer cache's interface (gpb_pool.hip) and the one type that owns a device buffer taken from it.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

namespace gpb {

// cache of freed device buffers: every pointer from pool_malloc goes back through pool_free — which DevBuf sees to
hipError_t pool_malloc(void** p, size_t bytes);
void pool_free(void* p);
void pool_trim();

// `cap` elements of T at `p`, or nothing.  Reads like the T* it replaces (kernel arguments, pointer arithmetic, null tests,
// copies); release() hands the buffer back to the cache, so whoever calls it — or lets the destructor — has made sure that
// no stream still uses the buffer (ctx_replace / ctx_grow of gpb_internal.h for the buffers of a context).
template <typename T>
struct DevBuf {
    T* p = nullptr;
    int64_t cap = 0;            // elements

    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }

    operator T*() const { return p; }
    T* get() const { return p; }
    void release() {
        pool_free(p);
        p = nullptr;
        cap = 0;
    }
    // a fresh buffer of n (at least one) elements, contents undefined; a failure leaves the buffer empty
    hipError_t alloc(int64_t n) {
        release();
        if (n < 1) n = 1;
        const hipError_t e = pool_malloc(reinterpret_cast<void**>(&p), sizeof(T) * (size_t)n);
        if (e != hipSuccess) p = nullptr;
        else cap = n;
        return e;
    }
};

}  // namespace gpb
