// s360_launch.h — host-side rules every entry point of the library shares: the check after a launch, the bound on a grid,
// pointer alignment, the pointer rule of an entry's inputs and outputs, the workspace-size protocol of include/s360.h and the
// check of a "high" call's scratch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/s360.h"

#define S360_BLOCK 256  // threads of a workgroup of every 1-D launch

#ifdef S360_DEBUG_LAUNCH  /* compile-time diagnostic (-DS360_DEBUG_LAUNCH): no environment reads in the host path */
#define S360_LAUNCH_DIAG(e, file, line) fprintf(stderr, "s360: %s at %s:%d\n", hipGetErrorString(e), file, line)
#else
#define S360_LAUNCH_DIAG(e, file, line) ((void)(file), (void)(line))
#endif

// S360_OK, or S360_E_LAUNCH when a launch since the last check failed: `return s360_launch_status();` ends an entry point.
// The default arguments are the caller's file and line, for the diagnostic.
static inline int s360_launch_status(const char* file = __builtin_FILE(), int line = __builtin_LINE()) {
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return S360_OK;
    S360_LAUNCH_DIAG(e, file, line);
    return S360_E_LAUNCH;
}

// between two launches: leaves the entry point with S360_E_LAUNCH when the launch failed
#define S360_CHECK_LAUNCH()                                           \
    do {                                                              \
        if (s360_launch_status() != S360_OK) return S360_E_LAUNCH;    \
    } while (0)

// A grid holds at most 2^31 work-items: `blocks` workgroups of S360_BLOCK threads fit.
static inline bool s360_grid_fits(long long blocks) { return blocks <= 0x7fffffffLL / S360_BLOCK; }

// p is a multiple of a (a power of two)
static inline bool s360_aligned(const void* p, size_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

// The pointer rule of include/s360.h for one entry point: `in` is what the call reads, `out` what it writes, the caller's
// scratch among them.  Every pointer is non-null and 16-byte aligned, no output is an input and no two outputs are the same.
template <size_t NI, size_t NO>
static inline bool s360_pointers_ok(const void* const (&in)[NI], const void* const (&out)[NO]) {
    for (const void* p : in)
        if (!p || !s360_aligned(p, 16)) return false;
    for (size_t i = 0; i < NO; ++i) {
        if (!out[i] || !s360_aligned(out[i], 16)) return false;
        for (const void* p : in)
            if (p == out[i]) return false;
        for (size_t j = i + 1; j < NO; ++j)
            if (out[j] == out[i]) return false;
    }
    return true;
}

// The workspace-size protocol of include/s360.h.  workspace == NULL is the size query: *bytes = need, S360_OK.  Otherwise
// args_ok (the entry point's own pointer checks) and the alignment of the workspace come first, S360_E_BADARG, then the size,
// S360_E_WORKSPACE.  S360_WS_READY: go on and launch.
enum { S360_WS_READY = 1 };
static inline int s360_workspace(const void* workspace, size_t* bytes, size_t need, size_t align, bool args_ok) {
    if (!workspace) {
        *bytes = need;
        return S360_OK;
    }
    if (!args_ok || !s360_aligned(workspace, align)) return S360_E_BADARG;
    return *bytes < need ? S360_E_WORKSPACE : S360_WS_READY;
}

// The caller's scratch of a "high" call (its size comes from the operator's *_scratch_bytes): S360_E_BADARG for a null or
// misaligned one, then S360_E_WORKSPACE for a short one, S360_OK otherwise.
static inline int s360_scratch(const void* scratch, size_t bytes, size_t need) {
    if (!scratch || !s360_aligned(scratch, 16)) return S360_E_BADARG;
    return bytes < need ? S360_E_WORKSPACE : S360_OK;
}
