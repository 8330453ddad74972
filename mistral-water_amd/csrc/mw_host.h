// mw_host.h -- host-side helpers every part of the library shares (device build only): the error channel behind mw_last_error(), the
// typed hipMalloc, its scoped form and the one list of transform sizes.  Everything here has internal linkage: nothing joins the library's exported symbols.
#pragma once
#include <hip/hip_runtime.h>

#include <mutex>
#include <string>

#include "../../include/mistral_water.h"

// ------------------------------------------------------------------------------------------------
// error plumbing
// ------------------------------------------------------------------------------------------------
static thread_local std::string g_err;
static mw_status fail(mw_status s, const std::string& m) {
    g_err = m;
    return s;
}
static mw_status fail(mw_status s, const char* who, const std::string& m) { return fail(s, std::string(who) + ": " + m); }
#define HIP_TRY(expr)                                                                                   \
    do {                                                                                                \
        hipError_t e_ = (expr);                                                                         \
        if (e_ != hipSuccess)                                                                           \
            return fail(MW_EDEVICE, std::string(#expr) + ": " + hipGetErrorString(e_));                 \
    } while (0)

template <typename T>
static mw_status dmalloc(T** p, size_t count) {
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(p), count * sizeof(T)));
    return MW_OK;
}
// a device allocation of one call (the test hooks): freed on every way out of its scope
namespace {
template <typename T>
struct DevTmp {
    T* p = nullptr;
    DevTmp() = default;
    DevTmp(const DevTmp&) = delete;
    ~DevTmp() { hipFree(p); }
    hipError_t alloc(size_t count) { return hipMalloc(reinterpret_cast<void**>(&p), count * sizeof(T)); }
};
}  // namespace

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) once per (kernel, device), safe from any number of host threads
namespace mw {
struct AttrOnce {
    std::once_flag once[64];
    hipError_t res[64];
    hipError_t set(const void* fn, int bytes) {
        int dev = 0;
        hipError_t e = hipGetDevice(&dev);
        if (e != hipSuccess) return e;
        const int d = dev & 63;
        std::call_once(once[d], [&] { res[d] = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes); });
        return res[d];
    }
};
}  // namespace mw

// The transform sizes the library has kernels for, named once.  The statement(s) after DEFAULT run with NN a constant expression equal
// to N_; any other N_ runs DEFAULT (the caller's own message and status).
#define MW_FOR_SIZE(N_, DEFAULT, ...)                                 \
    switch (N_) {                                                     \
        case 64: { constexpr int NN = 64; __VA_ARGS__; } break;       \
        case 128: { constexpr int NN = 128; __VA_ARGS__; } break;     \
        case 256: { constexpr int NN = 256; __VA_ARGS__; } break;     \
        case 512: { constexpr int NN = 512; __VA_ARGS__; } break;     \
        case 1024: { constexpr int NN = 1024; __VA_ARGS__; } break;   \
        case 2048: { constexpr int NN = 2048; __VA_ARGS__; } break;   \
        case 4096: { constexpr int NN = 4096; __VA_ARGS__; } break;   \
        default: DEFAULT;                                             \
    }
