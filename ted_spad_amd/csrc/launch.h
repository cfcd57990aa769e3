// Host-side launch helpers shared by every .hip file of libtedspad_hip.so (included from common.h; not part of the public ABI).
#pragma once

namespace tedspad {

// Kernels that use more than the default 64 KB of dynamic LDS need the limit raised once per kernel (and per thread: the flag is thread_local so that no launch
// path takes a lock). KFN is the kernel instantiation itself, so every kernel owns its flag and no launcher indexes a flag array by hand. Steady state: one flag test.
template <auto KFN>
inline int32_t raise_lds(const char *who) {
    static thread_local bool raised = false;
    if (raised) return TEDSPAD_OK;
    if (hipFuncSetAttribute((const void *)KFN, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess) {
        set_error("%s: cannot raise the dynamic LDS limit", who);
        return TEDSPAD_ELAUNCH;
    }
    raised = true;
    return TEDSPAD_OK;
}

// The same, the launch and its check, so that a kernel with a large LDS image is named once. `who` is the entry point a failure to raise the limit is reported
// under, `what` the name check_launch reports a failed launch under (some launchers add their form: "tedspad_conv_fwd(flat halo)").
template <auto KFN, typename... Args>
inline int32_t launch_lds(const char *who, const char *what, dim3 grid, dim3 block, size_t lds, hipStream_t s, const Args &...args) {
    const int32_t rc = raise_lds<KFN>(who);
    if (rc != TEDSPAD_OK) return rc;
    hipLaunchKernelGGL(KFN, grid, block, lds, s, args...);
    return check_launch(what);
}

template <auto KFN, typename... Args>
inline int32_t launch_lds(const char *who, dim3 grid, dim3 block, size_t lds, hipStream_t s, const Args &...args) {
    return launch_lds<KFN>(who, who, grid, block, lds, s, args...);
}

// workgroups of 256 threads for `items` work items, at most 16 per CU: the kernels grid-stride the rest
inline int grid_for(long items) {
    long g = (items + 255) / 256;
    if (g > 256 * 16) g = 256 * 16;
    return g < 1 ? 1 : (int)g;
}

}  // namespace tedspad

// Expands the statement(s) once with T = F16 and once with T = BF16 and runs the one `dtype` (already validated: TEDSPAD_F16 or TEDSPAD_BF16) selects, so that an
// argument list is written once for both storage types.
#define TS_WITH_T(dtype, ...)                  \
    do {                                       \
        if ((dtype) == TEDSPAD_F16) {          \
            using T = tedspad::F16;            \
            __VA_ARGS__;                       \
        } else {                               \
            using T = tedspad::BF16;           \
            __VA_ARGS__;                       \
        }                                      \
    } while (0)

// One kernel launch through it. KERN names T and stands in parentheses where it holds a comma: TS_LAUNCH_T(dtype, (foo_kernel<T, 4>), grid, block, lds, stream, args...)
#define TS_LAUNCH_T(dtype, KERN, grid, block, lds, stream, ...) TS_WITH_T(dtype, hipLaunchKernelGGL(KERN, grid, block, lds, stream, __VA_ARGS__))
