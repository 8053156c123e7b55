// ccunion.hpp — union-find rooted at the smallest index, shared by the connected-component kernels (maskcc.hip, stereofilter.hip).  A parent never exceeds its child, so
// a root IS its set's smallest index; values only decrease, so every loop ends and no workgroup waits for another.
#pragma once
#include "common.hpp"

// ---- union-find in LDS (workgroup scope) -------------------------------------------------------------
__device__ __forceinline__ int cc_lfind(int* par, int i)
{
    for (;;) { const int p = __hip_atomic_load(par + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); if (p == i) return i; i = p; }
}
__device__ __forceinline__ void cc_lunion(int* par, int a, int b)
{
    for (;;) {
        a = cc_lfind(par, a); b = cc_lfind(par, b);
        if (a == b) return;
        if (a < b) { const int s = a; a = b; b = s; }              // a > b: a's root goes under the smaller index
        const int old = __hip_atomic_fetch_min(par + a, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (old == a) return;
        a = old;                                                    // somebody moved a meanwhile: go on from where it points
    }
}
// ---- union-find in global memory, every access an agent-scope atomic ---------------------------------
__device__ __forceinline__ int cc_gfind(int32_t* par, int i)
{
    for (;;) { const int p = __hip_atomic_load(par + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); if (p == i) return i; i = p; }
}
__device__ __forceinline__ void cc_gunion(int32_t* par, int a, int b)
{
    for (;;) {
        a = cc_gfind(par, a); b = cc_gfind(par, b);
        if (a == b) return;
        if (a < b) { const int s = a; a = b; b = s; }
        const int old = __hip_atomic_fetch_min(par + a, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old == a) return;
        a = old;
    }
}
