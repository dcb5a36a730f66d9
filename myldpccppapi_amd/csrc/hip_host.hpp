/*
 * hip_host.hpp -- the host scaffolding every translation unit of libldpc_hip.so shares: the setter of the calling
 * thread's ldpc_last_error() message (and its two accessors), the one HIP error macro, the owners of the HIP resources
 * (DevBuf: device memory, HostBuf: pinned host memory, Event, Stream), and the small helpers of the handle-less stage
 * entry points (device selection, argument checks, grid sizing, the host-buffer loop).
 */
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <initializer_list>
#include <string>
#include <vector>

#include "../../include/ldpc_hip.h"

namespace ldpc {

/* stores the formatted message for ldpc_last_error() and returns `code` (ldpc_hip.hip) */
int set_error(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
/* the calling thread's message, and putting a saved one back: a worker thread's text crosses to the thread that waited
 * for it, and a call's first error survives its clean-up (ldpc_hip.hip) */
std::string last_error_text();
void restore_error(const std::string &text);

#define LDPC_HIP_TRY(expr)                                                                             \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess)                                                                          \
            return ldpc::set_error(LDPC_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                                   __FILE__, __LINE__);                                                \
    } while (0)

/* device memory with an owner: freed when the owner goes, on every path */
template <typename T> struct DevBuf {
    T *p = nullptr;
    size_t n = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept
    {
        if (this != &o) { release(); p = o.p; n = o.n; o.p = nullptr; o.n = 0; }
        return *this;
    }
    hipError_t alloc(size_t count)
    {
        release();
        n = count;
        if (!count) return hipSuccess;
        return hipMalloc((void **)&p, count * sizeof(T));
    }
    hipError_t upload(const std::vector<T> &h)
    {
        hipError_t e = alloc(h.size());
        if (e != hipSuccess || h.empty()) return e;
        return hipMemcpy(p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice);
    }
    /* made by the first caller that needs it: nothing happens when it is there already */
    hipError_t ensure(size_t count) { return p ? hipSuccess : alloc(count); }
    void release()
    {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
    ~DevBuf() { release(); }
};

/* pinned host memory with an owner */
template <typename T> struct HostBuf {
    T *p = nullptr;
    size_t n = 0;
    HostBuf() = default;
    HostBuf(const HostBuf &) = delete;
    HostBuf &operator=(const HostBuf &) = delete;
    HostBuf(HostBuf &&o) noexcept : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }
    HostBuf &operator=(HostBuf &&o) noexcept
    {
        if (this != &o) { release(); p = o.p; n = o.n; o.p = nullptr; o.n = 0; }
        return *this;
    }
    hipError_t alloc(size_t count)
    {
        release();
        if (!count) return hipSuccess;
        const hipError_t e = hipHostMalloc((void **)&p, count * sizeof(T), hipHostMallocDefault);
        if (e != hipSuccess) p = nullptr;
        else n = count;
        return e;
    }
    hipError_t ensure(size_t count) { return p ? hipSuccess : alloc(count); }
    void release()
    {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        n = 0;
    }
    ~HostBuf() { release(); }
};

/* an event with an owner; create(false): hipEventDisableTiming (an ordering mark only) */
struct Event {
    hipEvent_t e = nullptr;
    Event() = default;
    Event(const Event &) = delete;
    Event &operator=(const Event &) = delete;
    Event(Event &&o) noexcept : e(o.e) { o.e = nullptr; }
    Event &operator=(Event &&o) noexcept
    {
        if (this != &o) { release(); e = o.e; o.e = nullptr; }
        return *this;
    }
    hipError_t create(bool timed = true)
    {
        release();
        const hipError_t r = timed ? hipEventCreate(&e) : hipEventCreateWithFlags(&e, hipEventDisableTiming);
        if (r != hipSuccess) e = nullptr;
        return r;
    }
    hipError_t ensure(bool timed = true) { return e ? hipSuccess : create(timed); }
    void release()
    {
        if (e) (void)hipEventDestroy(e);
        e = nullptr;
    }
    ~Event() { release(); }
};

/* a non-blocking stream with an owner.  The destructor does not wait: whoever owns memory or events used on the stream
 * drains it first (decoder.hpp: ~ldpc_decoder) */
struct Stream {
    hipStream_t s = nullptr;
    Stream() = default;
    Stream(const Stream &) = delete;
    Stream &operator=(const Stream &) = delete;
    Stream(Stream &&o) noexcept : s(o.s) { o.s = nullptr; }
    Stream &operator=(Stream &&o) noexcept
    {
        if (this != &o) { release(); s = o.s; o.s = nullptr; }
        return *this;
    }
    hipError_t create()
    {
        release();
        const hipError_t r = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
        if (r != hipSuccess) s = nullptr;
        return r;
    }
    hipError_t ensure() { return s ? hipSuccess : create(); }
    void release()
    {
        if (s) (void)hipStreamDestroy(s);
        s = nullptr;
    }
    ~Stream() { release(); }
};

/* makes `device` current after checking that it exists; `what` names the stage in "... has no CPU fallback" */
inline int use_device(int32_t device, const char *what)
{
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
        return set_error(LDPC_ERR_HIP, "no usable HIP device (%s has no CPU fallback)", what);
    if (device < 0 || device >= count) return set_error(LDPC_ERR_ARG, "device %d of %d", device, count);
    LDPC_HIP_TRY(hipSetDevice(device));
    return LDPC_OK;
}

inline bool ranges_overlap(const void *p, int64_t p_bytes, const void *q, int64_t q_bytes)
{
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return a < b + (uintptr_t)q_bytes && b < a + (uintptr_t)p_bytes;
}

inline int known_code_format(int32_t f, const char *what)
{
    if (f != LDPC_CODE_PACKED && f != LDPC_CODE_BITS) return set_error(LDPC_ERR_ARG, "unknown %s %d", what, f);
    return LDPC_OK;
}

/* grid.y of the stage kernels: they stride over the frames, so that a lane's index arithmetic serves many frames and
 * the grid is a few rounds of resident workgroups instead of one small workgroup per frame and tile */
const int64_t kFrameTargetBlocks = 16384;    /* 8 resident workgroups of 256 on each of 256 CUs, eight rounds */
inline unsigned frame_grid(int64_t frames, unsigned grid_x)
{
    return (unsigned)std::min<int64_t>(std::min<int64_t>(frames, 65535), std::max<int64_t>(1, kFrameTargetBlocks / grid_x));
}

/* The host-buffer form of a handle-less stage: the frames pass through device scratch in chunks of at most
 * kHostChunkBytes per array; per chunk the `in` arrays are copied up, launch(frames_in_chunk, first_frame, dev) runs on
 * the null stream and the `out` arrays are copied back, all in the order of `arrays`.  dev[i] belongs to the i-th array
 * and is null where that array's host pointer is (array absent).  At most four arrays. */
const int64_t kHostChunkBytes = (int64_t)64 << 20;
struct HostArray {
    void *host;
    int64_t row;        /* bytes per frame */
    bool in, out;
};
template <typename Launch> int host_chunks(int64_t frames, std::initializer_list<HostArray> arrays, Launch launch)
{
    int64_t widest = 1;
    for (const HostArray &a : arrays) widest = std::max(widest, a.row);
    const int64_t chunk = std::min<int64_t>(frames, std::max<int64_t>(1, kHostChunkBytes / widest));
    DevBuf<uint8_t> buf[4];
    void *dev[4] = {nullptr, nullptr, nullptr, nullptr};
    int i = 0;
    for (const HostArray &a : arrays) {
        if (a.host) {
            LDPC_HIP_TRY(buf[i].alloc((size_t)(chunk * a.row)));
            dev[i] = buf[i].p;
        }
        ++i;
    }
    for (int64_t f0 = 0; f0 < frames; f0 += chunk) {
        const int64_t n = std::min(chunk, frames - f0);
        i = 0;
        for (const HostArray &a : arrays) {
            if (a.host && a.in)
                LDPC_HIP_TRY(hipMemcpy(dev[i], (const uint8_t *)a.host + f0 * a.row, (size_t)(n * a.row), hipMemcpyHostToDevice));
            ++i;
        }
        if (int rc = launch(n, f0, dev)) return rc;
        i = 0;
        for (const HostArray &a : arrays) {
            if (a.host && a.out)
                LDPC_HIP_TRY(hipMemcpy((uint8_t *)a.host + f0 * a.row, dev[i], (size_t)(n * a.row), hipMemcpyDeviceToHost));
            ++i;
        }
    }
    return LDPC_OK;
}

}  // namespace ldpc
