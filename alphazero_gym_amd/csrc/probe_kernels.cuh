// probe_kernels.cuh -- the math / MFMA self tests and microbenchmark probes behind azg_math_selftest (engine_selftest.hip).
#pragma once
#include "records.h"
#include "env.cuh"
#include "tree.cuh"
#include "mlp.cuh"

// fn_ids 13 / 14: act4<false> (mlp.cuh: the device-only ELU / ReLU of the register-resident kernels) on in[i], placed in component
// i & 3 of the vector; the other three components hold fixed bystanders (a positive, a negative, a clamped one and a zero).
// fn_id 15: tree_div over operand pairs: in[2j] is the numerator and in[2j + 1] the divisor (a positive count) of pair j, and both
// out[2j] and out[2j + 1] receive the quotient (n must be even; a numerator without a divisor yields 0).
__device__ __forceinline__ double act4_probe(int act, float x, int comp) {
    f32x4 v = {3.0f, -0.5f, -100.0f, 0.0f};
    if (comp == 0) v.x = x; else if (comp == 1) v.y = x; else if (comp == 2) v.z = x; else v.w = x;
    const f32x4 r = act4<false>(act, v);
    return (double)(comp == 0 ? r.x : comp == 1 ? r.y : comp == 2 ? r.z : r.w);
}

__global__ void math_selftest_kernel(int fn_id, const double* in, double* out, size_t n) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double x = in[i], s, c;
    switch (fn_id) {
        case 0: out[i] = (double)azg_expf((float)x); break;
        case 1: out[i] = (double)azg_expm1f((float)x); break;
        case 2: out[i] = (double)azg_tanhf((float)x); break;
        case 3: out[i] = (double)azg_logf((float)x); break;
        case 4: out[i] = (double)azg_cos2pif((float)x); break;
        case 5: azg_sincos(x, &s, &c); out[i] = s; break;
        case 6: azg_sincos(x, &s, &c); out[i] = c; break;
        case 7: out[i] = azg_pymod(x, 2.0 * 3.141592653589793, 0.15915494309189535); break;
        case 8: out[i] = (double)azg_normal(34u, (uint32_t)x, 0u, (uint32_t)(x * 7.0)); break;
        case 9: out[i] = (double)((float)x / 3.0f); break;
        case 10: out[i] = (double)__builtin_sqrtf((float)x); break;
        case 11: out[i] = x / 3.0; break;
        case 12: out[i] = __builtin_sqrt(x); break;
        case 13: out[i] = act4_probe(AZG_ACT_ELU, (float)x, (int)(i & 3)); break;
        case 14: out[i] = act4_probe(AZG_ACT_RELU, (float)x, (int)(i & 3)); break;
        case 15: out[i] = (i | 1) < n ? tree_div(in[i & ~(size_t)1], in[i | 1]) : 0.0; break;
        default: out[i] = 0.0;
    }
}

// fn_id 100: one 16x16x4 MFMA chain over n/… ; in = [a0..a(K-1), b0..b(K-1), c], out[0] = D[0][0]; probes the accumulation order
__global__ void mfma_probe_kernel(const double* in, double* out, int K) {
    int lane = threadIdx.x;
    f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
    float c = (float)in[2 * K];
    acc.x = acc.y = acc.z = acc.w = c;
    for (int s = 0; s < K / 4; ++s) {
        int k = 4 * s + (lane >> 4);
        float a = (float)in[k];
        float b = (float)in[K + k];
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0);
    }
    if (lane == 0) out[0] = (double)acc.x;
}

// fn_id 101: matrix-pipe rate probe (diagnostic): every wave issues iters x 16 register-only fp32 MFMAs (4 independent chains);
// out[0..1] of wave 0: shader-clock cycles (s_memtime) and constant 100 MHz ticks (s_memrealtime) across the loop.
__global__ __launch_bounds__(256) void mfma_rate_kernel(double* out, int iters) {
    f32x4 acc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    float a = 1.0f + 1e-7f * threadIdx.x, b = 1.0f - 1e-7f * threadIdx.x;
    const unsigned long long t0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
#pragma unroll 1
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc[i], 0, 0, 0);
    }
    const unsigned long long t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
    float sum = acc[0].x + acc[1].y + acc[2].z + acc[3].w;
    if (blockIdx.x == 0 && threadIdx.x == 0) { out[0] = (double)(t1 - t0); out[1] = (double)(r1 - r0); }
    if (sum == 123.456f) out[2] = sum;   // keeps the chains alive
}

// fn_id 102: latency probe (diagnostic): one wave, dependent chains of N operations each; out[i] = shader cycles per operation.
//   0 v_fma_f64   1 v_fma_f32   2 v_mul_f64 + v_add_f64   3 float64 division (tree_div)   4 IEEE float64 division
//   5 LDS round trip (ds_read_b32, dependent address)   6 LDS 16-byte round trip   7 DPP move (dependent)   8 ds_bpermute
//   9 global load round trip (dependent address, L2-resident)   10 azg_sincos   11 v_mfma_f32_16x16x4 dependent chain
__global__ __launch_bounds__(64) void latency_probe_kernel(double* out, int* chase, int n) {
    __shared__ int s_chase[1024];
    __shared__ f32x4 s_wide[256];
    const int lane = threadIdx.x;
    for (int i = lane; i < 1024; i += 64) s_chase[i] = (i * 17 + 5) & 1023;
    for (int i = lane; i < 256; i += 64) s_wide[i] = f32x4{(float)((i * 7 + 3) & 255), 0.0f, 0.0f, 0.0f};
    __syncthreads();
    unsigned long long t0, t1;
    double res[12];
#define PROBE(idx, init, body, sink)                                              \
    {                                                                             \
        init;                                                                     \
        __builtin_amdgcn_s_waitcnt(0);                                            \
        t0 = __builtin_amdgcn_s_memtime();                                        \
        __builtin_amdgcn_sched_barrier(0);                                        \
        _Pragma("unroll 1") for (int it = 0; it < n; it += 8) { body; body; body; body; body; body; body; body; }   \
        sink;                                                                     \
        __builtin_amdgcn_sched_barrier(0);                                        \
        t1 = __builtin_amdgcn_s_memtime();                                        \
        res[idx] = (double)(t1 - t0) / n;                                         \
    }
    double xd = 1.0 + 1e-9 * lane, ad = 0.999999, bd = 1e-7, accd = 0.0;
    float xf = 1.0f + 1e-6f * lane;
    PROBE(0, , xd = __builtin_fma(xd, ad, bd), accd += xd)
    PROBE(1, , xf = __builtin_fmaf(xf, 0.99999f, 1e-6f), accd += xf)
    PROBE(2, , xd = xd * ad + bd, accd += xd)
    PROBE(3, , xd = tree_div(xd + 2.0, 1.5), accd += xd)
    PROBE(4, , xd = (xd + 2.0) / 1.5, accd += xd)
    int p = lane;
    PROBE(5, , p = s_chase[p], accd += p)
    int pw = lane;
    PROBE(6, , pw = (int)s_wide[pw & 255].x, accd += pw)
    int dv = lane;
    PROBE(7, , dv = __builtin_amdgcn_update_dpp(0, dv, 0x121, 0xf, 0xf, false) + 1, accd += dv)
    int bv = lane;
    PROBE(8, , bv = __builtin_amdgcn_ds_bpermute(((bv + 1) & 63) << 2, bv), accd += bv)
    int g = lane;
    PROBE(9, , g = chase[g], accd += g)
    double sn = 0.1 * lane, cs = 0.0;
    PROBE(10, , azg_sincos(sn + 0.5, &sn, &cs), accd += sn + cs)
    f32x4 ma = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    PROBE(11, , ma = __builtin_amdgcn_mfma_f32_16x16x4f32(xf, 1.0f, ma, 0, 0, 0), accd += ma.x)
#undef PROBE
    if (lane == 0) for (int i = 0; i < 12; ++i) out[i] = res[i];
    if (accd == 1.2345) out[12] = accd;
}
