// swf_stage.h — the host-memory path of the stand-alone batch operators, once.  Host only.
//
// An operator called with host memory allocates device buffers, copies in, launches, copies out, synchronises and frees.  HostStage
// owns the buffers and the error handling of that path; the entry point is straight-line code around it:
//
//     <host arrays that the copies read or write>       rel, the h_* staging vectors, code
//     HostStage S("swf_xxx_batch", st);
//     A.in = S.up(in, n);  A.out = S.out<double>(n);    allocate (at least 8 bytes), remember, enqueue the copy in
//     if (S.failed()) return S.rc();                    (1) no kernel runs on null pointers
//     launch;  S.check(hipGetLastError(), ...)          or the operator's swf_internal_*_launch
//     S.down(out, A.out, n);  S.sync();
//     if (S.failed()) return S.rc();                    (2)
//
// Failure is sticky: after the first failing HIP call every later call does nothing and up / out return nullptr.  The first failure
// sets the library's error text once, "<entry point>: <HIP call>: <hipGetErrorString>"; rc() is SWF_E_NODEVICE from then on.
//
// Lifetime rule.  The copies are asynchronous, so every host array that one of them reads or writes is declared BEFORE the HostStage
// and therefore outlives it.  The destructor waits for the stream (result ignored) if anything was enqueued and not synchronised
// since, then frees: no way out of the entry point, an early return included, leaves a copy in flight on a dead array.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <string>
#include <vector>
#include "../../include/swf_solver.h"

void swf_internal_set_error(const std::string& m);

class HostStage {
public:
    HostStage(const char* entry, hipStream_t st) : entry_(entry), st_(st) {}
    HostStage(const HostStage&) = delete;
    HostStage& operator=(const HostStage&) = delete;
    ~HostStage() {
        if (pending_) (void)hipStreamSynchronize(st_);
        for (void* p : bufs_) (void)hipFree(p);
    }

    bool failed() const { return failed_; }
    int rc() const { return failed_ ? SWF_E_NODEVICE : SWF_OK; }

    // the result of a HIP call the entry point makes itself (hipGetLastError() after its launch); false once anything has failed
    bool check(hipError_t e, const char* call) {
        if (!failed_ && e != hipSuccess) {
            failed_ = true;
            swf_internal_set_error(std::string(entry_) + ": " + call + ": " + hipGetErrorString(e));
        }
        return !failed_;
    }

    // a device buffer of max(n, n_min) elements, of 8 bytes at least: an empty array still gets an address
    template <class T> T* out(size_t n, size_t n_min = 0) {
        void* d = nullptr;
        if (failed_ || !check(hipMalloc(&d, std::max<size_t>(std::max(n, n_min) * sizeof(T), 8)), "hipMalloc")) return nullptr;
        bufs_.push_back(d);
        return (T*)d;
    }
    // a device buffer of max(n, n_min) elements holding src[0 .. n); nothing is copied from a null src
    template <class T> T* up(const T* src, size_t n, size_t n_min = 0) {
        T* d = out<T>(n, n_min);
        put(d, src, n);
        return d;
    }
    // host to device into memory of a buffer of this stage
    template <class T> void put(T* d, const T* src, size_t n) { copy(d, src, n * sizeof(T), hipMemcpyHostToDevice); }
    // device to host; nothing for a null dst (an output the caller did not ask for)
    template <class T> void down(T* dst, const T* d, size_t n) { copy(dst, d, n * sizeof(T), hipMemcpyDeviceToHost); }
    void sync() {
        if (failed_) return;
        pending_ = false;
        check(hipStreamSynchronize(st_), "hipStreamSynchronize");
    }

private:
    void copy(void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
        if (failed_ || !dst || !src || !bytes) return;
        pending_ = true;
        check(hipMemcpyAsync(dst, src, bytes, kind, st_), "hipMemcpyAsync");
    }
    const char* entry_;
    hipStream_t st_;
    std::vector<void*> bufs_;
    bool failed_ = false, pending_ = false;
};
