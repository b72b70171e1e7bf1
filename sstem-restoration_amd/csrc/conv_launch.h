// Host-side helpers shared by the convolution launchers (conv_kernels.hip, conv_bf16_kernels.hip, conv_split_kernels.hip,
// conv_split_wgrad.hip, convt_kernels.hip): the two plan rules every kernel family uses, one launch path, and the step from runtime
// flags to template arguments.  Everything here has internal linkage or is a template.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include <type_traits>

namespace sstem {

// K slices for small grids.  A workgroup owns one pixel tile x one block of output channels and walks all of K; while the grid is
// below `target` workgroups K is cut into 2, 4 or 8 slices of whole input-channel chunks, at least `min_chunks` chunks each (the
// double-buffered pipelines want two).  A pure function of the problem size: launcher and workspace query see the same number.
// SSTEM_CONV_KSPLIT=0: never (read here and nowhere else).
inline int conv_ksplit(int64_t wgs, int nchunks, int target, int min_chunks)
{
    static const bool off = [] { const char* e = getenv("SSTEM_CONV_KSPLIT"); return e && atoi(e) == 0; }();
    int ks = 1;
    if (!off)
        while (wgs * ks < target && ks < 8 && nchunks % (ks * 2) == 0 && nchunks / (ks * 2) >= min_chunks) ks *= 2;
    return ks;
}

// Partial slabs of a weight gradient: enough of them to bring `blocks` (co, ci) blocks to about `target` workgroups, but at least
// `min_tiles` of the `ntiles` pixel tiles per workgroup (the partial-slab traffic stays below the useful work), and at least one.
inline int wgrad_slabs(int target, int64_t blocks, int64_t ntiles, int min_tiles)
{
    int64_t k = (target + blocks - 1) / blocks;
    if (k > ntiles / min_tiles) k = ntiles / min_tiles;
    if (k < 1) k = 1;
    return (int)k;
}

// workgroups of `threads` for the grid-stride kernels over n elements: at most 8192, at least one
inline int grid_1d(int64_t n, int threads)
{
    int64_t g = (n + threads - 1) / threads;
    if (g > 256 * 32) g = 256 * 32;
    if (g < 1) g = 1;
    return (int)g;
}

// One launch of one kernel instance.  The instance is the template argument itself, not its type: two instances with the same
// signature share a type and would share the flag below.  Dynamic LDS above the 64 KB default needs
// hipFuncAttributeMaxDynamicSharedMemorySize raised, once per instance and device: devices 0-63 remember the largest size they were
// given, any other device sets the attribute at every launch.  The arguments go to the kernel as written (no default arguments
// through a function pointer: name every one).
template <auto Kernel, class... Args>
inline hipError_t launch_kernel(dim3 grid, dim3 block, size_t lds_bytes, hipStream_t s, Args... args)
{
    if (lds_bytes > 0) {
        static int raised[64] = {};
        int dev = 0;
        hipError_t e = hipGetDevice(&dev);
        if (e != hipSuccess) return e;
        const bool cached = dev >= 0 && dev < 64;
        if (!cached || raised[dev] < (int)lds_bytes) {
            e = hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
            if (e != hipSuccess) return e;
            if (cached) raised[dev] = (int)lds_bytes;
        }
    }
    Kernel<<<grid, block, lds_bytes, s>>>(args...);
    return hipGetLastError();
}

// Runtime flags to compile-time constants: with_flags(f, a, b, ...) calls f(A, B, ...) where each argument is std::true_type or
// std::false_type after the flag's value.  f is a generic lambda; it cuts the combinations that have no kernel instance with
// `if constexpr` BEFORE it names the kernel, so nothing is instantiated for them.
template <class F>
inline hipError_t with_flags(F&& f) { return f(); }
template <class F, class... Rest>
inline hipError_t with_flags(F&& f, bool flag, Rest... rest)
{
    auto bound = [&](auto c) { return with_flags([&](auto... cs) { return f(c, cs...); }, rest...); };
    return flag ? bound(std::true_type{}) : bound(std::false_type{});
}

}  // namespace sstem
