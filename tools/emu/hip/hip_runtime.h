// hip/hip_runtime.h -- HOST stand-in used ONLY by tools/emu (a debugging build of the kernel sources for the CPU).
// It lets csrc/race_kernel_reg.hip.h compile with g++ so that a kernel edit can be checked against the oracle in
// seconds before it is sent to a GPU.  Execution model: the threads of ONE block run one after another, phase by
// phase (tools/emu/emu_kernel.cpp); __syncthreads() is a no-op and LDS is a plain array.  Nothing under monte_carlo_gp_amd/
// includes or links this: the product has no CPU path.
//
// EMU_BLOCK_THREADS (tools/emu/emu_champ.cpp only): a block is blockDim.x HOST THREADS that run at the same time.
// threadIdx and blockIdx are thread-local, __syncthreads() is a real barrier over the block (emu_block_barrier, defined
// by the driver), atomicAdd is atomic, a __shared__ array is one static object that all threads of the block see, and the
// dynamic LDS is the buffer emu_dynamic_lds points to.
// Without the macro everything below is as it always was.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

#define __global__
#define __device__
#define __host__
#define __forceinline__ inline __attribute__((always_inline))
#define __launch_bounds__(...)
#ifdef EMU_BLOCK_THREADS
#define __shared__ static
#define HIP_DYNAMIC_SHARED(type, var) type *var = reinterpret_cast<type *>(emu_dynamic_lds);
extern void *emu_dynamic_lds;            // the running launch's dynamic LDS: a buffer of exactly the launch's bytes
#else
#define __shared__
#define HIP_DYNAMIC_SHARED(type, var) extern __shared__ type var[];
#endif
#define __align__(x)
#ifndef __restrict__
#define __restrict__ __restrict
#endif

struct emu_dim3 {
    unsigned x, y, z;
};
#ifdef EMU_BLOCK_THREADS
extern thread_local emu_dim3 threadIdx, blockIdx;
extern emu_dim3 blockDim, gridDim;
void emu_block_barrier();
#else
extern emu_dim3 threadIdx, blockIdx, blockDim, gridDim;
#endif

struct float4 {
    float x, y, z, w;
};

#ifdef EMU_BLOCK_THREADS
inline void __syncthreads() { emu_block_barrier(); }
#else
inline void __syncthreads() {}
#endif
inline int __popc(unsigned v) { return __builtin_popcount(v); }
inline int __ffs(int v) { return __builtin_ffs(v); }
inline int __clz(int v) { return v == 0 ? 32 : __builtin_clz((unsigned)v); }
inline int __clzll(long long v) { return v == 0 ? 64 : __builtin_clzll((unsigned long long)v); }
inline double __hiloint2double(int hi, int lo)
{
    const uint64_t u = ((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo;
    double d;
    std::memcpy(&d, &u, 8);
    return d;
}
inline unsigned long long __umul64hi(unsigned long long a, unsigned long long b)
{
    return (unsigned long long)(((unsigned __int128)a * (unsigned __int128)b) >> 64);
}
inline int __double2loint(double x)
{
    uint64_t u;
    std::memcpy(&u, &x, 8);
    return (int)(uint32_t)u;
}
inline int __double2hiint(double x)
{
    uint64_t u;
    std::memcpy(&u, &x, 8);
    return (int)(uint32_t)(u >> 32);
}
inline uint32_t __float_as_uint(float f)
{
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}
inline float __uint_as_float(uint32_t u)
{
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}
template <typename T>
inline T atomicAdd(T *p, T v)
{
#ifdef EMU_BLOCK_THREADS
    return __atomic_fetch_add(p, v, __ATOMIC_RELAXED);
#else
    const T old = *p;
    *p = old + v;
    return old;
#endif
}
// Cross-lane operations have no meaning in a block of one thread.  They are declared so that headers whose GPU-only
// kernels use them (trace_count_positions: __shfl_down; the matchups kernel: __ballot; stints_count: __ballot, __shfl)
// compile here; the host builds never call those kernels, and a call ends the process rather than return a made-up value.
template <typename T>
inline T __shfl_down(T, int, int = 64)
{
    __builtin_trap();
}
template <typename T>
inline T __shfl(T, int, int = 64)
{
    __builtin_trap();
}
inline unsigned long long __ballot(int) { __builtin_trap(); }
inline int __popcll(unsigned long long v) { return __builtin_popcountll(v); }
inline int __ffsll(unsigned long long v) { return __builtin_ffsll((long long)v); }
