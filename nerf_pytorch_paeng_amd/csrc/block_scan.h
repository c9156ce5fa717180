// block_scan.h -- the deterministic sums over a workgroup that the libraries beside libmi_nerf.so share at compile time: the exclusive
// prefix sum of an array in three launches (mesh.hip on uint32, occ.hip on the packed 64-bit counts, vox.hip's chunk counts), and the fp64
// block sum of frames.hip and iqa.hip.  Everything is a __device__ __forceinline__ template: the __global__ kernels stay in their
// libraries under their own names (profiles and tools find them by name), each a few lines that call a body below, and no library gains
// a symbol.  No atomic; wave64; the order of every addition is fixed.
//
//     reduce   grid = ceil(n / SCAN_TILE) blocks of 256    bsum[b] = sum of block b's SCAN_TILE elements
//     sums     ONE block of 1024                           bsum -> its exclusive prefix sums in place; returns the grand total
//     apply    grid as reduce                              data -> its exclusive prefix sums in place
#pragma once
#include <hip/hip_runtime.h>

namespace miblock {

constexpr int SCAN_TILE = 1024;                          // elements of one block of reduce / apply: 256 threads x 4

// exclusive scan of one value per thread over a block of NT threads; *total = the block's sum.  lds: NT / 64 + 1 words.
template <int NT, typename T>
__device__ __forceinline__ T block_exclusive_scan(T v, T* total, T* lds) {
    constexpr int NW = NT / 64;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    T x = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T t = __shfl_up(x, d, 64);
        if (lane >= d) x += t;
    }
    if (lane == 63) lds[wave] = x;
    __syncthreads();
    if (threadIdx.x == 0) {
        T run = 0;
        for (int w = 0; w < NW; ++w) {
            const T s = lds[w];
            lds[w] = run;
            run += s;
        }
        lds[NW] = run;
    }
    __syncthreads();
    const T r = x - v + lds[wave];
    *total = lds[NW];
    __syncthreads();                                                     // lds is reused by the caller's next round
    return r;
}

template <typename T>
__device__ __forceinline__ void scan_reduce(const T* data, long long n, T* bsum) {
    __shared__ T lds[4];
    const long long base = (long long)blockIdx.x * SCAN_TILE + threadIdx.x * 4;
    T s = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (base + k < n) s += data[base + k];
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) bsum[blockIdx.x] = (lds[0] + lds[1]) + (lds[2] + lds[3]);
}

// one block of 1024 threads, in rounds of 1024 block sums with a carry.  The grand total is returned in every thread; the caller's
// thread 0 writes it in the form its library publishes.
template <typename T>
__device__ __forceinline__ T scan_sums(T* bsum, int nb) {
    __shared__ T lds[1024 / 64 + 1];
    T carry = 0;
    for (int c = 0; c < nb; c += 1024) {
        const int i = c + (int)threadIdx.x;
        const T v = i < nb ? bsum[i] : (T)0;
        T sum;
        const T ex = block_exclusive_scan<1024>(v, &sum, lds);
        if (i < nb) bsum[i] = carry + ex;
        carry += sum;
    }
    return carry;
}

template <typename T>
__device__ __forceinline__ void scan_apply(T* data, long long n, const T* bsum) {
    __shared__ T lds[256 / 64 + 1];
    const long long base = (long long)blockIdx.x * SCAN_TILE + threadIdx.x * 4;
    T v[4], s = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        v[k] = base + k < n ? data[base + k] : (T)0;
        s += v[k];
    }
    T sum;
    T run = bsum[blockIdx.x] + block_exclusive_scan<256>(s, &sum, lds);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (base + k < n) data[base + k] = run;
        run += v[k];
    }
}

// deterministic sum of one fp64 value per thread over the block's blockDim.x / 64 waves (sh: that many words); valid on thread 0
__device__ __forceinline__ double block_sum(double v, double* sh) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
    if (threadIdx.x == 0)
        for (int i = 0; i < (int)(blockDim.x >> 6); ++i) s += sh[i];
    return s;
}

}  // namespace miblock
