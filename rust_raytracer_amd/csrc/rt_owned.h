// rt_owned.h — host only: the owners of everything the library allocates through HIP (device buffers, pinned host buffers,
// events, streams), and how a HIP failure reaches the error channel (rt_error.h).  This is the one file that calls the HIP
// allocation and creation functions; every struct that holds a device resource holds one of these, so a destructor releases
// it and no release list has to remember it.  The owners do not switch devices: whoever destroys them on another device
// than the current one calls hipSetDevice first (~RtScene, ~RtAccum).
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>
#include <string>
#include <utility>

#include "../../include/rt_mi355.h"
#include "rt_error.h"

namespace rt {

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return rt::set_err(RT_E_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_));    \
    } while (0)

// What is alive (rt_debug_live_resources): device buffers, their bytes, pinned buffers, events + streams.
enum { LIVE_BUFFERS = 0, LIVE_BYTES = 1, LIVE_PINNED = 2, LIVE_HANDLES = 3 };
inline std::atomic<uint64_t> g_live[4];

// Every allocation of the library.  nomem != NULL: hipErrorOutOfMemory becomes RT_E_NOMEM with that message and the (not
// sticky) error is cleared, for callers that retry with less; any other failure is RT_E_DEVICE.
inline int owned_alloc(void** p, size_t bytes, bool pinned, const char* nomem) {
    const hipError_t e = pinned ? hipHostMalloc(p, bytes) : hipMalloc(p, bytes);
    if (e == hipErrorOutOfMemory && nomem) {
        (void)hipGetLastError();
        return set_err(RT_E_NOMEM, nomem);
    }
    if (e != hipSuccess) return set_err(RT_E_DEVICE, std::string(pinned ? "hipHostMalloc: " : "hipMalloc: ") + hipGetErrorString(e));
    g_live[pinned ? LIVE_PINNED : LIVE_BUFFERS]++;
    if (!pinned) g_live[LIVE_BYTES] += bytes;
    return RT_OK;
}

// A grow-only buffer of T in device memory (PINNED: in pinned host memory).  Converts to T* wherever a pointer is read;
// kernel launches take get().
template <typename T, bool PINNED = false>
class DevBuf {
    T* p_ = nullptr;
    size_t bytes_ = 0;

  public:
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p_(std::exchange(o.p_, nullptr)), bytes_(std::exchange(o.bytes_, 0)) {}
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) {
            reset();
            p_ = std::exchange(o.p_, nullptr);
            bytes_ = std::exchange(o.bytes_, 0);
        }
        return *this;
    }
    ~DevBuf() { reset(); }
    void reset() {
        if (!p_) return;
        (void)(PINNED ? hipHostFree(p_) : hipFree(p_));
        g_live[PINNED ? LIVE_PINNED : LIVE_BUFFERS]--;
        if (!PINNED) g_live[LIVE_BYTES] -= bytes_;
        p_ = nullptr;
        bytes_ = 0;
    }
    // At least `need` bytes afterwards, contents not kept.  The old memory is released and the pair cleared BEFORE the new
    // allocation, so a failure leaves (NULL, 0) behind and never a size without its memory.
    int reserve(size_t need, const char* nomem = nullptr) {
        if (bytes_ >= need) return RT_OK;
        reset();
        if (int st = owned_alloc(reinterpret_cast<void**>(&p_), need, PINNED, nomem)) {
            p_ = nullptr;
            return st;
        }
        bytes_ = need;
        return RT_OK;
    }
    T* get() const { return p_; }
    operator T*() const { return p_; }
    T* operator->() const { return p_; }
    size_t bytes() const { return bytes_; }
};
template <typename T> using PinnedBuf = DevBuf<T, true>;

// An event or a stream: created on first use by Event::ensure / Stream::create, destroyed with its owner.
template <typename H, hipError_t (*DESTROY)(H)>
class Handle {
  protected:
    H h_ = nullptr;
    int created(hipError_t e, const char* what) {
        if (e != hipSuccess) {
            h_ = nullptr;
            return set_err(RT_E_DEVICE, std::string(what) + ": " + hipGetErrorString(e));
        }
        g_live[LIVE_HANDLES]++;
        return RT_OK;
    }

  public:
    Handle() = default;
    Handle(Handle&& o) noexcept : h_(std::exchange(o.h_, nullptr)) {}
    Handle& operator=(Handle&& o) noexcept {
        std::swap(h_, o.h_);
        return *this;
    }
    ~Handle() {
        if (!h_) return;
        (void)DESTROY(h_);
        g_live[LIVE_HANDLES]--;
    }
    operator H() const { return h_; }
};
struct Event : Handle<hipEvent_t, hipEventDestroy> {
    int ensure() { return h_ ? RT_OK : created(hipEventCreate(&h_), "hipEventCreate"); }
};
struct Stream : Handle<hipStream_t, hipStreamDestroy> {
    int create_non_blocking() { return h_ ? RT_OK : created(hipStreamCreateWithFlags(&h_, hipStreamNonBlocking), "hipStreamCreateWithFlags"); }
};

}  // namespace rt
