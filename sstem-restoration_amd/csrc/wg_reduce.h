// Deterministic sums over a whole launch: every workgroup leaves its partial sums in global memory and the LAST workgroup to arrive
// adds them in a fixed order -- no float atomics, the same bits every run, nothing to clear between calls or graph replays.
// This header is the only place the protocol lives (bn_channel_barrier of norm_kernels.hip is a different thing: a spin barrier between
// resident workgroups).  Device-only; workgroups of 256 threads = four waves of 64.
//
// The helpers own the protocol, the kernel owns the ORDER in which the last workgroup reads the partials: the order is part of the result.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sstem {

// relaxed, agent scope: a partial or a counter another workgroup of this launch reads or has written
template <class T>
__device__ __forceinline__ T agent_load(const T* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

template <class T>
__device__ __forceinline__ void agent_store(T* p, T v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

template <class T>
__device__ __forceinline__ T wave_sum(T v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

// red[wave][q]: one slot per wave and quantity; lane 0 of a wave holds the wave's result
template <class T, int N>
__device__ __forceinline__ void wave_slot(T (*red)[N], int q, T v) { if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][q] = v; }

// the fixed tree over the four slots of quantity q (after a __syncthreads() behind the slot writes)
template <class T, int N>
__device__ __forceinline__ T block_tree(T (*red)[N], int q) { return (red[0][q] + red[1][q]) + (red[2][q] + red[3][q]); }

// N sums over the workgroup: wave sums (the N ladders side by side, so their shuffles overlap), slots, barrier.
// block_tree(red, q) then gives sum q to any thread.
template <int N, class T>
__device__ __forceinline__ void block_sum(const T (&v)[N], T (*red)[N])
{
    T s[N];
#pragma unroll
    for (int q = 0; q < N; ++q) s[q] = v[q];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int q = 0; q < N; ++q) s[q] += __shfl_down(s[q], o, 64);
    }
#pragma unroll
    for (int q = 0; q < N; ++q) wave_slot(red, q, s[q]);
    __syncthreads();
}

// Arrival of a workgroup at a launch-wide counter (zero before the launch's first arrival); true, for every thread of the workgroup,
// in the one workgroup that arrives last.  Call it from all 256 threads, once per kernel (the flag is not guarded against a second use).
// The ordering contract:
//   before: THREAD 0 has written everything the last workgroup is to read from this one, with agent_store.  The add releases what
//           thread 0 stored before it, at agent scope; stores of other threads are not covered.
//   after : in the last workgroup every thread has passed an agent-scope acquire, and may read every workgroup's partials with
//           agent_load, in whatever fixed order the kernel chooses.
//   reset : the last workgroup calls release_counter (one thread, after the workgroup's use of the count), so the next launch on the
//           stream finds zero; nobody else writes the counter.
__device__ __forceinline__ bool arrive_last(unsigned* counter)
{
    __shared__ int last;
    if (threadIdx.x == 0) {
        const unsigned prev = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        last = prev == gridDim.x - 1;
    }
    __syncthreads();
    if (!last) return false;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    return true;
}

__device__ __forceinline__ void release_counter(unsigned* counter) { agent_store(counter, 0u); }

// The last workgroup's second stage where all 256 threads add all partials: partials[N * i + q] of workgroup i, thread t takes
// i = t, t + 256, ... in index order, then block_sum; block_tree(red, q) holds total q.  The leading barrier lets red be the array the
// first stage went through.
template <int N, class T>
__device__ __forceinline__ void block_total(const T* partials, int64_t count, T (*red)[N])
{
    T t[N] = {};
    for (int64_t i = threadIdx.x; i < count; i += 256) {
#pragma unroll
        for (int q = 0; q < N; ++q) t[q] += agent_load(partials + N * i + q);
    }
    __syncthreads();
    block_sum(t, red);
}

}  // namespace sstem
