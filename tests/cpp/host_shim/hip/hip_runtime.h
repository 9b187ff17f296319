// host_shim/hip/hip_runtime.h -- NOT the HIP runtime: the few names a kernel's text needs to compile for the HOST, so that
// tests/cpp/emulate_hoisted.cpp can run it on CPU threads under AddressSanitizer.
// One workgroup = one std::thread per lane, __syncthreads = a std::barrier; threadIdx / blockIdx / blockDim are thread-local.  Put this directory in
// front of the include path of a plain clang++ (never hipcc).
#pragma once
#include <barrier>
#include <cstddef>
#include <cstdint>
#define __device__
#define __host__
#define __global__
#define __forceinline__ inline
#define __launch_bounds__(x)
#define __shared__
#define __align__(x) __attribute__((aligned(x)))
struct dim3
{
    unsigned x = 1, y = 1, z = 1;
    dim3() = default;
    dim3(unsigned a, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {}
};
extern thread_local dim3 threadIdx, blockIdx, blockDim, gridDim;
extern std::barrier<>* g_block_barrier; // of the workgroup that is running
inline void __syncthreads() { g_block_barrier->arrive_and_wait(); }
inline unsigned __umulhi(unsigned a, unsigned b) { return static_cast<unsigned>((static_cast<unsigned long long>(a) * b) >> 32); }
inline unsigned long long __umul64hi(unsigned long long a, unsigned long long b)
{
    return static_cast<unsigned long long>((static_cast<unsigned __int128>(a) * b) >> 64);
}
// what gpuntt/common/common.cuh names
typedef struct ihipStream_t* hipStream_t;
typedef int hipError_t;
constexpr hipError_t hipSuccess = 0;
inline const char* hipGetErrorString(hipError_t) { return "host shim"; }
inline hipError_t hipGetLastError() { return hipSuccess; }
