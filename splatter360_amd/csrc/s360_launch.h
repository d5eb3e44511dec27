// s360_launch.h — host-side rules every entry point of the library shares: the check after a launch, the bound on a grid,
// pointer alignment, the pointer rule of an entry's inputs and outputs and the workspace-size protocol of include/s360.h.
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
// scratch among them, `opt` the outputs the caller may leave out (a null one is skipped, any other is an output like those of
// `out`).  Every pointer is non-null and a multiple of `align` (16 bytes unless the operator's kernels ask for less), no output
// is an input and no two outputs are the same; inputs may be one another.
template <size_t NI, size_t NO, size_t NP>
static inline bool s360_pointers_ok(const void* const (&in)[NI], const void* const (&out)[NO], const void* const (&opt)[NP],
                                    size_t align = 16) {
    for (const void* p : in)
        if (!p || !s360_aligned(p, align)) return false;
    const void* w[NO + NP];
    size_t n = 0;
    for (const void* p : out) {
        if (!p) return false;
        w[n++] = p;
    }
    for (const void* p : opt)
        if (p) w[n++] = p;
    for (size_t i = 0; i < n; ++i) {
        if (!s360_aligned(w[i], align)) return false;
        for (const void* p : in)
            if (p == w[i]) return false;
        for (size_t j = i + 1; j < n; ++j)
            if (w[j] == w[i]) return false;
    }
    return true;
}
template <size_t NI, size_t NO>
static inline bool s360_pointers_ok(const void* const (&in)[NI], const void* const (&out)[NO]) {
    const void* const none[] = {nullptr};
    return s360_pointers_ok(in, out, none);
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
