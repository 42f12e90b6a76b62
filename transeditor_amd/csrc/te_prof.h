// Phase-profiler plumbing of the kernel files, written once.  A profiled file (conv.hip, wgrad.hip, wino6.hip, s2s6.hip, t2s6.hip,
// wgrad6.hip) turns its own -D name into TE_PROF - and conv.hip the name of its second instrument, the whole-block timeline, into
// TE_PROF2 - in front of this include.  (The -D names are spelled in the files that own them only: tools/exp_build.py rebuilds the
// sources whose text, headers included, mentions a flag.)
// In the product build (neither defined) every macro below expands to nothing: a profiling line in a kernel body is one macro call and
// the kernel's machine code does not know it is there.  Profiling builds are experiments (tools/*_phase_prof.py, tools/conv_timeline.py,
// tools/wgrad6_check.py prof); they compute the same results, slower.
//     PROF_BUFFER(name, n)   __device__ unsigned long long te_<name>_prof_buf[n]
//     PROF_READBACK(name)    extern "C" int te_debug_<name>_prof(void* host_dst, int64_t bytes)      PROF_CLEAR(name): ..._prof_clear()
//     PROF_T(v)              time stamp v (shader cycles); PROF2_T(v): the 100 MHz s_memrealtime counter
//     PROF_ACC(acc, a, b)    acc += b - a                   PROF_LAP(acc): acc += now - tlast, tlast = now
//     PROF_ONLY(...)         tokens that exist in TE_PROF builds only; PROF2_ONLY: TE_PROF2 builds; PROF_ANY: either
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#ifdef TE_PROF
#define PROF_ONLY(...) __VA_ARGS__
#else
#define PROF_ONLY(...)
#endif
#ifdef TE_PROF2
#define PROF2_ONLY(...) __VA_ARGS__
#else
#define PROF2_ONLY(...)
#endif
#if defined(TE_PROF) || defined(TE_PROF2)
#define PROF_ANY(...) __VA_ARGS__
#else
#define PROF_ANY(...)
#endif

#define PROF_T(v) PROF_ONLY(const unsigned long long v = __builtin_readcyclecounter())
#define PROF2_T(v) PROF2_ONLY(const unsigned long long v = __builtin_amdgcn_s_memrealtime())
#define PROF_ACC(acc, a, b) PROF_ONLY(acc += (b) - (a))
#define PROF_LAP(acc) PROF_ONLY({ const unsigned long long t_ = __builtin_readcyclecounter(); acc += t_ - tlast; tlast = t_; })

#define PROF_BUFFER(name, n) PROF_ANY(__device__ unsigned long long te_##name##_prof_buf[n];)
#define PROF_READBACK(name) PROF_ANY(extern "C" int te_debug_##name##_prof(void* host_dst, int64_t bytes) { \
    return (int)hipMemcpyFromSymbol(host_dst, HIP_SYMBOL(te_##name##_prof_buf), (size_t)bytes, 0, hipMemcpyDeviceToHost); })
#define PROF_CLEAR(name) PROF_ANY(extern "C" int te_debug_##name##_prof_clear() { \
    void* dptr = nullptr; \
    if (hipGetSymbolAddress(&dptr, HIP_SYMBOL(te_##name##_prof_buf)) != hipSuccess) return -1; \
    return (int)hipMemset(dptr, 0, sizeof(te_##name##_prof_buf)); })
