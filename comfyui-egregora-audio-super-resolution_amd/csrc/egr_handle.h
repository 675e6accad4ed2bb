// What the model handles that live inside the library (DfnCore, Dac) share around a call: the kept workspace, the device checks and the
// stage copy-out and the pinned staging of per-row tables (TableStage); and the move-only owners of device resources (DevBuf, EventPair, Stream) that the FlashSR handle and the Fat-Llama plan
// hold as members.  WPE (caller-owned workspace) has a lifetime of its own.
#pragma once
#include "egr_common.h"

#include <string.h>

#include <initializer_list>
#include <map>
#include <mutex>

namespace egr {

#define EGR_TRY(x) do { int rc__ = (x); if (rc__ != EGR_OK) return rc__; } while (0)

// Selects `device` for a scope (create, upload, destroy) and makes the previous device current again; ok: both calls succeeded.
struct DeviceScope {
    int prev = 0;
    bool ok;
    explicit DeviceScope(int device) { ok = hipGetDevice(&prev) == hipSuccess && hipSetDevice(device) == hipSuccess; }
    ~DeviceScope() { (void)hipSetDevice(prev); }
    DeviceScope(const DeviceScope&) = delete;
    DeviceScope& operator=(const DeviceScope&) = delete;
};

// A call works on the handle's device: the caller makes it current.
inline int check_current_device(const char* who, int device) {
    int cur = -1;
    EGR_HIP(hipGetDevice(&cur));
    EGR_CHECK(cur == device, EGR_ERR_ARG, "%s: handle belongs to device %d, current device is %d", who, device, cur);
    return EGR_OK;
}

// The workspace a handle keeps between calls: grow-only, stream-ordered (nothing synchronises).
struct Workspace {
    void* p = nullptr;
    size_t bytes = 0;
    int grow(size_t need, hipStream_t st) {
        if (need <= bytes) return EGR_OK;
        if (p) EGR_HIP(hipFreeAsync(p, st));
        p = nullptr;
        bytes = 0;
        EGR_HIP(hipMallocAsync(&p, need, st));
        bytes = need;
        return EGR_OK;
    }
    // at destroy, on the handle's device: hipMallocAsync memory is returned stream-ordered, then waited for (not a pipeline call)
    void release() {
        if (!p) return;
        (void)hipFreeAsync(p, nullptr);
        (void)hipDeviceSynchronize();
        p = nullptr;
        bytes = 0;
    }
};

// Pinned host memory a tracks call copies its tables from, so that the copy is asynchronous, and the event behind the last such copy:
// the next call waits for that copy alone (not for the stream's other work) before it overwrites the memory.
struct TableStage {
    void* p = nullptr;
    size_t bytes = 0;
    hipEvent_t copied = nullptr;
    int reserve(size_t need) {
        if (!copied) EGR_HIP(hipEventCreateWithFlags(&copied, hipEventDisableTiming));
        else EGR_HIP(hipEventSynchronize(copied));
        if (need <= bytes) return EGR_OK;
        if (p) EGR_HIP(hipHostFree(p));
        p = nullptr;
        bytes = 0;
        EGR_HIP(hipHostMalloc(&p, need, hipHostMallocDefault));
        bytes = need;
        return EGR_OK;
    }
    // the copy of the first `n` staged bytes to dst (device) on st, and the event behind it
    int upload(void* dst, size_t n, hipStream_t st) {
        EGR_HIP(hipMemcpyAsync(dst, p, n, hipMemcpyHostToDevice, st));
        EGR_HIP(hipEventRecord(copied, st));
        return EGR_OK;
    }
    void release() {
        if (copied) { (void)hipEventSynchronize(copied); (void)hipEventDestroy(copied); }
        if (p) (void)hipHostFree(p);
        p = nullptr; bytes = 0; copied = nullptr;
    }
};

// Tables of a call that has no handle to keep a stage in (the eval and null-test calls of egr_glue.hip, egr_nullmany_delays,
// egr_wpemany_dereverb): the spans go, back to back, through the current device's stage of one registry and up to dst in one
// asynchronous copy.  One registry for all of them: a call waits (in reserve) for the previous table copy on its device, whichever
// family made it -- a few kilobytes, the same wait each family made on its own previous copy when it had a stage to itself.
// The stage is the CURRENT device's (hipGetDevice), the one the call launches on: egr_nullmany_delays, which used to take its plan's
// device, runs on that device like every other call of a plan.
struct TableSpan {
    const void* p;
    size_t bytes;
};
inline int upload_table(std::initializer_list<TableSpan> spans, void* dst, hipStream_t st) {
    static std::mutex mu;
    static std::map<int, TableStage> stages;      // device -> pinned staging (under mu)
    int dev = 0;
    EGR_HIP(hipGetDevice(&dev));
    size_t bytes = 0;
    for (const TableSpan& s : spans) bytes += s.bytes;
    std::lock_guard<std::mutex> lk(mu);
    TableStage& stage = stages[dev];
    EGR_TRY(stage.reserve(bytes));
    char* h = (char*)stage.p;
    for (const TableSpan& s : spans) { memcpy(h, s.p, s.bytes); h += s.bytes; }
    return stage.upload(dst, bytes, st);
}

// a hipMalloc'ed buffer and its hipFree (move-only); whoever must wait for the device before a free does so before reset()
struct DevBuf {
    void* p = nullptr;
    DevBuf() {}
    DevBuf(DevBuf&& o) noexcept : p(o.p) { o.p = nullptr; }
    DevBuf& operator=(DevBuf&& o) noexcept { if (this != &o) { reset(); p = o.p; o.p = nullptr; } return *this; }
    ~DevBuf() { reset(); }
    bool alloc(size_t bytes) { reset(); if (hipMalloc(&p, bytes) != hipSuccess) p = nullptr; return p != nullptr; }
    void reset() { if (p) hipFree(p); p = nullptr; }
    void* release() { void* q = p; p = nullptr; return q; }
    template <class T> T* as() const { return (T*)p; }
};

// the two events around a timed launch, or a fork / join pair (move-only; empty until create())
struct EventPair {
    hipEvent_t a = nullptr, b = nullptr;
    EventPair() {}
    EventPair(EventPair&& o) noexcept : a(o.a), b(o.b) { o.a = o.b = nullptr; }
    EventPair& operator=(EventPair&& o) noexcept { if (this != &o) { reset(); a = o.a; b = o.b; o.a = o.b = nullptr; } return *this; }
    ~EventPair() { reset(); }
    hipError_t create(unsigned flags = hipEventDefault) {
        const hipError_t e = hipEventCreateWithFlags(&a, flags);
        return e != hipSuccess ? e : hipEventCreateWithFlags(&b, flags);
    }
    void reset() { if (a) hipEventDestroy(a); if (b) hipEventDestroy(b); a = b = nullptr; }
};

// a non-blocking stream the holder created (destroyed with it), or one handed in by the caller (left alone)
struct Stream {
    hipStream_t s = nullptr;
    bool owned = false;
    Stream() {}
    Stream(const Stream&) = delete;
    Stream& operator=(const Stream&) = delete;
    ~Stream() { reset(); }
    hipError_t create() { reset(); const hipError_t e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking); owned = e == hipSuccess; return e; }
    void borrow(hipStream_t theirs) { reset(); s = theirs; }
    void reset() { if (s && owned) hipStreamDestroy(s); s = nullptr; owned = false; }
};

// The stage read of the C ABI: *count = n always; a null dst only asks for it; else n floats of src go to dst (device to device, on `stream`).
inline int stage_copy_out(const char* who, const float* src, int64_t n, float* dst, int64_t capacity, int64_t* count, void* stream) {
    *count = n;
    if (!dst) return EGR_OK;
    EGR_CHECK(capacity >= n, EGR_ERR_ARG, "%s: %lld floats do not fit a capacity of %lld", who, (long long)n, (long long)capacity);
    EGR_HIP(hipMemcpyAsync(dst, src, sizeof(float) * (size_t)n, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return EGR_OK;
}

}  // namespace egr
