// abi_error.h -- the error plumbing of every library of the project, defined once: a thread-local message (what <prefix>_last_error()
// returns), set_error / hip_fail that write it, and the early-return macros of the entry points.  It knows no public header: the including
// library passes its own namespace and its own EINVAL / EHIP status values, and names the macros with its own prefix, one line each:
//
//     namespace miocc {
//     ABI_ERROR_STATE(static, MI_OCC_EHIP)
//     #define OCC_CHECK_ARG(cond, ...) ABI_CHECK_ARG(::miocc, MI_OCC_EINVAL, cond, __VA_ARGS__)
//     #define OCC_HIP(call) ABI_HIP(::miocc, call, #call)
//     #define OCC_LAUNCH_CHECK(name) ABI_LAUNCH_CHECK(::miocc, name)
//
// Each library keeps a buffer of its own.  A one-file library passes `static`: the buffer and both functions have internal linkage and the
// library exports nothing but the names of its header.  libmi_nerf.so passes nothing: api.hip holds the one buffer, and its other
// translation units reach set_error / hip_fail through the declarations in common.h.
//
// Being the one header every library includes, it also holds the two size helpers of every host side: align256 and blocks_for.
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stddef.h>
#include <stdio.h>

// a region of a scratch or workspace starts on a 256-byte boundary
static inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }
// blocks of `per_block` items that cover n
static inline unsigned blocks_for(long long n, int per_block) { return (unsigned)((n + per_block - 1) / per_block); }

#define ABI_ERROR_STATE(linkage, ehip)                                                \
    static thread_local char g_err[768] = "";                                         \
    linkage void set_error(const char* fmt, ...) {                                    \
        va_list ap;                                                                   \
        va_start(ap, fmt);                                                            \
        vsnprintf(g_err, sizeof(g_err), fmt, ap);                                     \
        va_end(ap);                                                                   \
    }                                                                                 \
    linkage int hip_fail(hipError_t e, const char* what) {                            \
        set_error("HIP error %d (%s) in %s", (int)e, hipGetErrorString(e), what);     \
        return ehip;                                                                  \
    }

// a failed call into libmi_nerf.so from a library that links against it (after ABI_ERROR_STATE; the library's header includes mi_nerf.h):
// its status becomes ours (EINVAL stays EINVAL), its text is carried over
#define ABI_NERF_FAIL(einval, ehip)                                                   \
    static int nerf_fail(int rc, const char* what) {                                  \
        set_error("%s failed (status %d): %s", what, rc, mi_nerf_last_error());       \
        return rc == MI_NERF_EINVAL ? einval : ehip;                                  \
    }

#define ABI_CHECK_ARG(ns, einval, cond, ...) \
    do {                                     \
        if (!(cond)) {                       \
            ns::set_error(__VA_ARGS__);      \
            return einval;                   \
        }                                    \
    } while (0)

// `text` is #call, taken by the one-line alias: there the call is still spelled as the source spells it
#define ABI_HIP(ns, call, text)                               \
    do {                                                      \
        hipError_t e__ = (call);                              \
        if (e__ != hipSuccess) return ns::hip_fail(e__, text); \
    } while (0)

#define ABI_LAUNCH_CHECK(ns, name)                                       \
    do {                                                                 \
        hipError_t e__ = hipGetLastError();                              \
        if (e__ != hipSuccess) return ns::hip_fail(e__, "launch " name); \
    } while (0)

#define ABI_NERF(ns, call, text)                                  \
    do {                                                          \
        int rc__ = (call);                                        \
        if (rc__ != MI_NERF_OK) return ns::nerf_fail(rc__, text); \
    } while (0)
