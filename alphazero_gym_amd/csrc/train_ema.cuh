// train_ema.cuh -- the exponential moving average of the trainer's parameters (include/azgym_train_ema.h): one streaming kernel over
// the n_nets * P floats, launched by dispatch_train.hip behind an optimiser step's backward launch.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#define TR_EMA_THREADS 256
#define TR_EMA_MAX_BLOCKS 2048   // 8 workgroups per CU of 256 CUs; the rest is a grid stride

// ema[i] += om[i / P] * (params[i] - ema[i]) for i < N = n_nets * P, each operation rounded by itself (the build's -ffp-contract=off).
// [n_nets][P] is one contiguous array.  n4 groups of four floats go through 16-byte loads and stores (the host passes n4 = N / 4 when
// both bases are 16-byte aligned and P >= 4, else 0); P need not be a multiple of 4, so a group may straddle two nets -- never three --
// and takes its second net's factor from the element on where the first net ends.  A thread divides once, for its first group; from
// then on the group's net and its offset in the net advance by the grid stride's quotient and remainder.  Elements 4 * n4 .. N - 1
// are the scalar tail (at most three of them on the aligned path).  No LDS, no atomics.
__global__ __launch_bounds__(TR_EMA_THREADS) void train_ema_kernel(const float* __restrict__ params, float* __restrict__ ema,
                                                                   const float* __restrict__ om, unsigned P, size_t n4, size_t N) {
    const size_t tid = (size_t)blockIdx.x * TR_EMA_THREADS + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * TR_EMA_THREADS;
    if (tid < n4) {
        const size_t e0 = 4 * tid, es = 4 * stride;
        size_t k = e0 / P;
        unsigned r = (unsigned)(e0 - k * P);          // the group's first element is element r of net k
        const size_t dk = es / P;
        const unsigned dr = (unsigned)(es - dk * P);
        const float4* __restrict__ p4 = reinterpret_cast<const float4*>(params);
        float4* __restrict__ m4 = reinterpret_cast<float4*>(ema);
        for (size_t g = tid; g < n4; g += stride) {
            const float4 p = p4[g];
            float4 m = m4[g];
            const unsigned left = P - r;              // elements of net k from the group's first on (>= 1)
            const float o0 = om[k];
            const float o1 = left < 4 ? om[k + 1] : o0;   // (left < 4: the group's last element lies in net k + 1 < n_nets)
            m.x = m.x + o0 * (p.x - m.x);
            m.y = m.y + (left > 1 ? o0 : o1) * (p.y - m.y);
            m.z = m.z + (left > 2 ? o0 : o1) * (p.z - m.z);
            m.w = m.w + (left > 3 ? o0 : o1) * (p.w - m.w);
            m4[g] = m;
            k += dk;
            r += dr;                                  // (r, dr < P < 2^31)
            if (r >= P) { r -= P; ++k; }
        }
    }
    for (size_t i = 4 * n4 + tid; i < N; i += stride) {
        const float m = ema[i];
        ema[i] = m + om[i / P] * (params[i] - m);
    }
}
