// lo_buf.h — the one owner of device, pinned and pinned-mapped memory in the library.
//
// Buf<T, Alloc, Free> holds a pointer and its capacity (in elements; bytes for T = void) together.  reserve() only
// grows, frees the old block before it allocates the new one (peak memory as a hand-written grow), keeps no contents,
// and leaves the buffer empty -- null, capacity 0 -- when the allocation fails.  It adds no synchronisation: a caller
// that grows a buffer the device may still read waits for that work first, as before.  Alloc / Free are template
// parameters only so that a host-only test can count and fail allocations (LO_BUF_NO_HIP: no HIP runtime).
#pragma once
#include <atomic>
#include <cstddef>
#include <type_traits>

namespace lo {

// bytes currently held through Buf, process-wide (lo_debug_live_bytes)
inline std::atomic<long long> g_buf_live_bytes{0};

template <class T, auto Alloc, auto Free>
class Buf {
    static constexpr size_t kElem = sizeof(std::conditional_t<std::is_void_v<T>, char, T>);
    T* p_ = nullptr;
    size_t cap_ = 0;

public:
    using err_t = decltype(Alloc(static_cast<void**>(nullptr), size_t(0)));   // value-initialised = success
    Buf() = default;
    Buf(const Buf&) = delete;
    Buf& operator=(const Buf&) = delete;
    Buf(Buf&& o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
    Buf& operator=(Buf&& o) noexcept {
        if (this != &o) {
            reset();
            p_ = o.p_; cap_ = o.cap_;
            o.p_ = nullptr; o.cap_ = 0;
        }
        return *this;
    }
    ~Buf() { reset(); }

    err_t reserve(size_t count) {
        if (count <= cap_) return err_t{};
        reset();
        void* q = nullptr;
        const err_t e = Alloc(&q, count * kElem);
        if (e != err_t{}) return e;
        p_ = static_cast<T*>(q);
        cap_ = count;
        g_buf_live_bytes.fetch_add(static_cast<long long>(count * kElem), std::memory_order_relaxed);
        return e;
    }
    void reset() {
        if (p_) {
            Free(p_);
            g_buf_live_bytes.fetch_sub(static_cast<long long>(cap_ * kElem), std::memory_order_relaxed);
        }
        p_ = nullptr;
        cap_ = 0;
    }
    T* get() const { return p_; }
    size_t capacity() const { return cap_; }
    operator T*() const { return p_; }
    T* operator->() const { return p_; }
};

}  // namespace lo

#ifndef LO_BUF_NO_HIP
#include <hip/hip_runtime.h>

#include <string>

namespace lo {
inline hipError_t buf_alloc_device(void** p, size_t bytes) { return hipMalloc(p, bytes); }
inline hipError_t buf_alloc_pinned(void** p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
inline hipError_t buf_alloc_mapped(void** p, size_t bytes) {
    return hipHostMalloc(p, bytes, hipHostMallocMapped | hipHostMallocCoherent);
}
inline void buf_free_device(void* p) { (void)hipFree(p); }
inline void buf_free_host(void* p) { (void)hipHostFree(p); }

template <class T> using DevBuf = Buf<T, buf_alloc_device, buf_free_device>;
template <class T> using PinnedBuf = Buf<T, buf_alloc_pinned, buf_free_host>;
template <class T> using MappedBuf = Buf<T, buf_alloc_mapped, buf_free_host>;
}  // namespace lo

// A failed HIP call ends the enclosing function with LO_ERR_HIP; h is any handle with a std::string err.
#define LO_HIP(h, call)                                                                    \
    do {                                                                                   \
        hipError_t e_ = (call);                                                            \
        if (e_ != hipSuccess) {                                                            \
            (h)->err = std::string(#call) + ": " + hipGetErrorString(e_);                 \
            return LO_ERR_HIP;                                                             \
        }                                                                                  \
    } while (0)
#endif
