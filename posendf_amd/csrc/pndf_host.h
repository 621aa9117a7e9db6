// Host-side helpers shared by the C-ABI translation units.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/posendf_amd.h"
#include "pndf_error.h"

// Every entry point runs on the device that owns its buffers and leaves the caller's current device as it found it
// (torch keeps a per-thread current device; an engine for cuda:1 must not change what torch.cuda.current_device() says).
struct DeviceGuard {
    int prev = -1;
    bool ok = true;
    explicit DeviceGuard(int device) {
        if (device < 0) return;                   // unknown: stay on the current device
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != device) ok = (hipSetDevice(device) == hipSuccess);
        else prev = -1;                           // nothing to restore
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;
};

// device that owns a device pointer (-1 if the runtime does not know it): the stateless helpers have no handle
inline int pndf_pointer_device(const void* p) {
    hipPointerAttribute_t attr;
    if (!p || hipPointerGetAttributes(&attr, p) != hipSuccess) {
        (void)hipGetLastError();
        return -1;
    }
    return attr.device;
}

// A failed HIP call ends the entry point with PNDF_ERR_HIP and the call's own text on the handle `h` (pndf_error.h)
#define HIP_TRY(h, expr)                                                                          \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess)                                                                     \
            return pndf_fail(h, PNDF_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

// after the launches of an entry point: PNDF_OK, or PNDF_ERR_HIP with "<what>: <the runtime's text>" on the handle
template <class H>
PNDF_LOCAL inline int pndf_check_launch(H* h, const char* what) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return pndf_fail(h, PNDF_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
    return PNDF_OK;
}

// do two buffers of `floats` floats each share memory?  (a null one shares none)
PNDF_LOCAL inline bool overlaps(const float* a, const float* b, int64_t floats) {
    return a && b && (uintptr_t)a < (uintptr_t)(b + floats) && (uintptr_t)b < (uintptr_t)(a + floats);
}

// The caller's workspace of `have` units ("floats", "bytes") against the `need` that `asks` (the unit's own query) returns:
// PNDF_OK, or PNDF_ERR_BAD_ARG with the text on the handle
template <class H>
PNDF_LOCAL inline int pndf_check_workspace(H* h, const void* workspace, int64_t have, int64_t need, const char* unit, const char* asks) {
    if (!workspace) return pndf_fail(h, PNDF_ERR_BAD_ARG, "null workspace");
    if (((uintptr_t)workspace & 15) != 0) return pndf_fail(h, PNDF_ERR_BAD_ARG, "workspace must be 16-byte aligned");
    if (have < need)
        return pndf_fail(h, PNDF_ERR_BAD_ARG, "workspace of " + std::to_string(have) + " " + unit + ", " + asks + " asks for " + std::to_string(need));
    return PNDF_OK;
}

// Is `device` a gfx950 device, and what are its properties?  `who` ("the engine", "training", ...) names the caller in the text.
// PNDF_ANY_DEVICE asks only whether the runtime sees a device at all (the pose index learns its device from a pointer afterwards).
// Every refusal clears the runtime's sticky error.  `verbose`: pndf_create's wording, which names the failed call and the
// architecture it found.
constexpr int PNDF_ANY_DEVICE = -0x7fffffff - 1;
struct PNDF_LOCAL PndfDeviceCheck {
    int code = PNDF_OK;
    std::string text;
    hipDeviceProp_t prop;
};
PNDF_LOCAL inline PndfDeviceCheck pndf_check_gfx950(int device, const char* who, bool verbose = false) {
    PndfDeviceCheck r;
    auto refuse = [&r](int code, const std::string& text) -> PndfDeviceCheck& {
        (void)hipGetLastError();
        r.code = code;
        r.text = text;
        return r;
    };
    const bool any = device == PNDF_ANY_DEVICE;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1 || (!any && (device < 0 || device >= ndev)))
        return refuse(PNDF_ERR_NO_DEVICE, "no HIP device " + (any ? std::string() : std::to_string(device) + " ") + "(" + who + " has no CPU fallback)");
    if (any) return r;
    const hipError_t e = hipGetDeviceProperties(&r.prop, device);
    if (e != hipSuccess && verbose) return refuse(PNDF_ERR_HIP, std::string("hipGetDeviceProperties(&prop, device): ") + hipGetErrorString(e));
    if (e != hipSuccess || std::string(r.prop.gcnArchName).rfind("gfx950", 0) != 0)
        return refuse(PNDF_ERR_NO_DEVICE, (verbose ? std::string("device is ") + r.prop.gcnArchName + ", " : std::string()) + "kernels are built for gfx950 only");
    return r;
}

// Launches of one handle that share a scratch buffer: a launch on another stream than the previous one first waits (on the
// device) for that one's completion event.  wait() goes before the launch, record() after it; a capturing stream is left alone
// (a captured graph replays in the order it was captured).
struct PNDF_LOCAL PndfScratchOrder {
    hipEvent_t done = nullptr;
    void* last_stream = nullptr;
    bool pending = false, capturing = false;
    hipError_t create() { return hipEventCreateWithFlags(&done, hipEventDisableTiming); }
    void destroy() {
        if (done) (void)hipEventDestroy(done);
        done = nullptr;
    }
    hipError_t wait(void* stream) {
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        (void)hipStreamIsCapturing((hipStream_t)stream, &cap);
        capturing = cap != hipStreamCaptureStatusNone;
        if (pending && last_stream != stream && !capturing) return hipStreamWaitEvent((hipStream_t)stream, done, 0);
        return hipSuccess;
    }
    hipError_t record(void* stream) {
        if (capturing) return hipSuccess;
        const hipError_t e = hipEventRecord(done, (hipStream_t)stream);
        if (e == hipSuccess) {
            last_stream = stream;
            pending = true;
        }
        return e;
    }
};

// roctx ranges around the C-ABI compute entry points: `rocprofv3 --marker-trace` then shows
// pndf_forward / pndf_forward_grad / pndf_project / pndf_lbs_terms_grad ... as named host ranges next to the kernels they
// launch.  The library does NOT link against the profiler: the marker library is picked up when the process already has it
// loaded (rocprofv3 preloads it) or when PNDF_ROCTX=1 asks for it; otherwise a range is two null checks.
#include <dlfcn.h>
#include <stdlib.h>
struct PndfRoctx {
    int (*push)(const char*) = nullptr;
    int (*pop)() = nullptr;
    PndfRoctx() {
        const char* env = getenv("PNDF_ROCTX");
        if (env && env[0] == '0') return;
        const bool force = env && env[0] == '1';
        const char* libs[] = {"librocprofiler-sdk-roctx.so.1", "librocprofiler-sdk-roctx.so", "libroctx64.so.4", "libroctx64.so"};
        for (const char* name : libs) {
            void* lib = dlopen(name, RTLD_NOW | RTLD_NOLOAD);
            if (!lib && force) lib = dlopen(name, RTLD_NOW);
            if (!lib) continue;
            push = (int (*)(const char*))dlsym(lib, "roctxRangePushA");
            pop = (int (*)())dlsym(lib, "roctxRangePop");
            if (push && pop) return;
            push = nullptr;
            pop = nullptr;
        }
    }
};
inline PndfRoctx& pndf_roctx() {
    static PndfRoctx r;
    return r;
}
struct PndfRange {
    bool on;
    explicit PndfRange(const char* name) : on(pndf_roctx().push != nullptr) {
        if (on) pndf_roctx().push(name);
    }
    ~PndfRange() {
        if (on) pndf_roctx().pop();
    }
    PndfRange(const PndfRange&) = delete;
    PndfRange& operator=(const PndfRange&) = delete;
};
