/*
 * azg_math.h -- bit-reproducible elementary functions + Philox for the azgym MCTS engine.
 *
 * Every function here is built ONLY from IEEE-754 correctly rounded primitives
 * (+, -, *, /, sqrt, fma) and integer/bit operations, written out in one fixed
 * evaluation order.  Compiled with -ffp-contract=off on both sides, the host
 * (gcc) and the gfx950 device (hipcc) therefore produce bit-identical results,
 * which is what lets tests/ compare the HIP search against the CPU oracle
 * bit-for-bit (visit counts, Q, W, actions) instead of within a tolerance.
 *
 * What each function stands in for in the reference (file:line under /root/reference):
 *   azg_expf / azg_expm1f / azg_tanhf  torch ELU, exp(log_std), softmax, tanh squash
 *                                      (alphazero/network/policies.py:101-120, 456-462;
 *                                       alphazero/network/distributions.py:63)
 *   azg_sincos, azg_pymod              numpy float64 sin/cos/% inside gym's classic-control
 *                                      dynamics (call sites alphazero/search/mcts.py:449, 686)
 *   azg_philox4x32, azg_normal         the engine's own counter-based RNG (the reference draws from
 *                                      torch/python global generators: policies.py:497, helpers.py:51)
 * Accuracy against the exact value on each function's documented domain: at most 2 ulp -- azg_expf 0.9, azg_expm1f 1.6, azg_cos2pif
 * 1.9 ulp of float32, azg_sincos 1.2 ulp of float64 -- except azg_logf, 2.9 ulp (x near 1.13, where the result is small), and azg_tanhf,
 * 2.4 ulp (|x| near 0.016); azg_pymod is exact.  At the functions' own thresholds (-87 / 88, 9, sqrt 2), +-0, subnormal inputs and
 * the ends of the domains: at most 1.3 ulp.  Measured (tests/math_accuracy_scan.py, profiles/math_edge_accuracy.txt) and checked in tests/test_math_env_abi.py
 * (test_math_accuracy_against_libm; test_math_edges_against_mpmath, against mpmath at 100 digits); device against host, bit for bit,
 * on the same inputs: tests/test_hip_parity.py (test_device_math_is_bit_identical_to_host).
 * Agreement with torch/numpy is therefore far inside the 1e-5 parity tolerance.
 */
#ifndef AZG_MATH_H
#define AZG_MATH_H

#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define AZG_HD __host__ __device__ __forceinline__
#define AZG_UNROLL _Pragma("unroll")   /* (small fixed-size arrays must stay in registers on the device) */
#else
#define AZG_HD static inline
#define AZG_UNROLL
#endif

#define AZG_FMAF(a, b, c) __builtin_fmaf((a), (b), (c))
#define AZG_FMA(a, b, c) __builtin_fma((a), (b), (c))

AZG_HD uint32_t azg_f2u(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
AZG_HD float azg_u2f(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
AZG_HD uint64_t azg_d2u(double f) { uint64_t u; memcpy(&u, &f, 8); return u; }
AZG_HD double azg_u2d(uint64_t u) { double f; memcpy(&f, &u, 8); return f; }

/* ---------------------------------------------------------------- float32 */

/* e^x, x finite.  Returns 0 below -87, clamps above 88. */
AZG_HD float azg_expf(float x) {
    if (x < -87.0f) return 0.0f;
    if (x > 88.0f) x = 88.0f;
    const float magic = 12582912.0f; /* 1.5 * 2^23: round-to-nearest-even of small floats */
    float kf = AZG_FMAF(x, 1.44269504088896341f, magic);
    kf = kf - magic;
    float r = AZG_FMAF(-kf, 0.693145751953125f, x);       /* ln2 hi (12 bits) */
    r = AZG_FMAF(-kf, 1.42860682030941723212e-6f, r);      /* ln2 lo */
    float p = 1.98412698412698413e-4f;                     /* 1/5040 */
    p = AZG_FMAF(p, r, 1.38888888888888894e-3f);           /* 1/720 */
    p = AZG_FMAF(p, r, 8.33333333333333322e-3f);           /* 1/120 */
    p = AZG_FMAF(p, r, 4.16666666666666644e-2f);           /* 1/24 */
    p = AZG_FMAF(p, r, 1.66666666666666657e-1f);           /* 1/6 */
    p = AZG_FMAF(p, r, 0.5f);
    p = AZG_FMAF(p, r, 1.0f);
    p = AZG_FMAF(p, r, 1.0f);
    int k = (int)kf;
    return p * azg_u2f((uint32_t)(k + 127) << 23);
}

/* e^x - 1, branch-free: x = k ln2 + r, result = 2^k * expm1(r) + (2^k - 1) */
AZG_HD float azg_expm1f(float x) {
    float xc = x < -87.0f ? -87.0f : (x > 88.0f ? 88.0f : x);
    const float magic = 12582912.0f;
    float kf = AZG_FMAF(xc, 1.44269504088896341f, magic);
    kf = kf - magic;
    float r = AZG_FMAF(-kf, 0.693145751953125f, xc);
    r = AZG_FMAF(-kf, 1.42860682030941723212e-6f, r);
    float p = 1.98412698412698413e-4f;                     /* 1/5040 */
    p = AZG_FMAF(p, r, 1.38888888888888894e-3f);
    p = AZG_FMAF(p, r, 8.33333333333333322e-3f);
    p = AZG_FMAF(p, r, 4.16666666666666644e-2f);
    p = AZG_FMAF(p, r, 1.66666666666666657e-1f);
    p = AZG_FMAF(p, r, 0.5f);
    float em1 = AZG_FMAF(p * r, r, r);
    int k = (int)kf;
    float sc = azg_u2f((uint32_t)(k + 127) << 23);
    return AZG_FMAF(sc, em1, sc - 1.0f);
}

/* tanh(z) = sign(z) * em1/(em1+2), em1 = e^{2|z|}-1 */
AZG_HD float azg_tanhf(float z) {
    float az = z < 0.0f ? -z : z;
    float t;
    if (az > 9.0f) {
        t = 1.0f;
    } else {
        float em1 = azg_expm1f(az + az);
        t = em1 / (em1 + 2.0f);
    }
    return z < 0.0f ? -t : t;
}

/* trunk activations with torch's default parameters (alphazero/network/utils.py:5-14): 0 relu, 1 elu (alpha 1), 2 leakyrelu
 * (slope 0.01), 3 relu6, 4 silu/swish x*sigmoid(x), 5 hardswish x*relu6(x+3)/6 */
AZG_HD float azg_activation(int act, float x) {
    float pos = x > 0.0f ? x : 0.0f;
    float neg = x > 0.0f ? 0.0f : x;
    switch (act) {
        case 1: return pos + azg_expm1f(neg);
        case 2: return pos + 0.01f * neg;
        case 3: return pos < 6.0f ? pos : 6.0f;
        case 4: return x / (1.0f + azg_expf(-x));
        case 5: { float t = x + 3.0f; t = t > 0.0f ? t : 0.0f; t = t < 6.0f ? t : 6.0f; return (x * t) / 6.0f; }
        default: return pos;
    }
}

/* ln(x) for x in (0, +inf) normal floats */
AZG_HD float azg_logf(float x) {
    uint32_t ix = azg_f2u(x);
    int e = (int)(ix >> 23) - 127;
    float m = azg_u2f((ix & 0x007fffffu) | 0x3f800000u);  /* [1,2) */
    if (m > 1.41421356237309515f) { m = m * 0.5f; e += 1; }
    float s = (m - 1.0f) / (m + 1.0f);
    float z = s * s;
    float p = 1.11111111111111105e-1f;                     /* 1/9 */
    p = AZG_FMAF(p, z, 1.42857142857142849e-1f);           /* 1/7 */
    p = AZG_FMAF(p, z, 0.2f);
    p = AZG_FMAF(p, z, 3.33333333333333315e-1f);
    p = AZG_FMAF(p, z, 1.0f);
    float lm = (s + s) * p;
    return AZG_FMAF((float)e, 0.693147180559945286f, lm);
}

/* cos(2*pi*u), u in [0,1) */
AZG_HD float azg_cos2pif(float u) {
    const float magic = 12582912.0f;
    float t = u * 4.0f;
    float qf = (t + magic) - magic;
    float f = t - qf;                                      /* [-0.5, 0.5], exact */
    float x = f * 1.57079632679489656f;
    float z = x * x;
    float sp = 2.75573192239858925e-6f;                    /* sin: x + x^3 * (...) */
    sp = AZG_FMAF(sp, z, -1.98412698412698413e-4f);
    sp = AZG_FMAF(sp, z, 8.33333333333333322e-3f);
    sp = AZG_FMAF(sp, z, -1.66666666666666657e-1f);
    float sn = AZG_FMAF(sp * z, x, x);
    float cp = 2.48015873015873016e-5f;                    /* cos: 1 - z/2 + ... */
    cp = AZG_FMAF(cp, z, -1.38888888888888894e-3f);
    cp = AZG_FMAF(cp, z, 4.16666666666666644e-2f);
    cp = AZG_FMAF(cp, z, -0.5f);
    float cs = AZG_FMAF(cp, z, 1.0f);
    int q = ((int)qf) & 3;
    return q == 0 ? cs : (q == 1 ? -sn : (q == 2 ? -cs : sn));
}

/* ---------------------------------------------------------------- float64 */

/* sin and cos of x, |x| < ~1e5 */
AZG_HD void azg_sincos(double x, double* sn, double* cs) {
    const double magic = 6755399441055744.0; /* 1.5 * 2^52 */
    double nf = AZG_FMA(x, 6.36619772367581382433e-01, magic);
    nf = nf - magic;
    double r = AZG_FMA(-nf, 1.57079632679489655800e+00, x);
    r = AZG_FMA(-nf, 6.12323399573676603587e-17, r);
    r = AZG_FMA(-nf, -1.49738490485919833842e-33, r);
    double z = r * r;
    /* fdlibm minimax kernels on [-pi/4, pi/4] */
    double ps = 1.58969099521155010221e-10;
    ps = AZG_FMA(ps, z, -2.50507602534068634195e-08);
    ps = AZG_FMA(ps, z, 2.75573137070700676789e-06);
    ps = AZG_FMA(ps, z, -1.98412698298579493134e-04);
    ps = AZG_FMA(ps, z, 8.33333333332248946124e-03);
    ps = AZG_FMA(ps, z, -1.66666666666666324348e-01);
    double s = AZG_FMA(ps * z, r, r);
    double pc = -1.13596475577881948265e-11;
    pc = AZG_FMA(pc, z, 2.08757232129817482790e-09);
    pc = AZG_FMA(pc, z, -2.75573143513906633035e-07);
    pc = AZG_FMA(pc, z, 2.48015872894767294178e-05);
    pc = AZG_FMA(pc, z, -1.38888888888741095749e-03);
    pc = AZG_FMA(pc, z, 4.16666666666666019037e-02);
    double hz = 0.5 * z;
    double w = 1.0 - hz;
    double c = w + (((1.0 - w) - hz) + (z * z) * pc);
    int q = ((int)nf) & 3;   /* |x| < 1e5: the quadrant count fits 32 bits */
    *sn = q == 0 ? s : (q == 1 ? c : (q == 2 ? -s : -c));
    *cs = q == 0 ? c : (q == 1 ? -s : (q == 2 ? -c : s));
}

/* Python/NumPy float `x % y` for y > 0 and |x/y| < 2^20: exact, result in [0, y).  inv_y = 1/y (any rounding): the
 * quotient estimate trunc(x * inv_y) may be off by one, which the sign of the first remainder reveals; the second fma
 * then computes x - q*y for the true floor quotient, which is exactly representable (the fmod property). */
AZG_HD double azg_pymod(double x, double y, double inv_y) {
    double qt = __builtin_trunc(x * inv_y);
    double r0 = AZG_FMA(-qt, y, x);
    double adj = r0 < 0.0 ? -1.0 : (r0 >= y ? 1.0 : 0.0);
    qt = qt + adj;
    double r = AZG_FMA(-qt, y, x);
    if (r < 0.0) r = r + y;   /* x < 0 with trunc instead of floor: one more period (exact: both terms are multiples of ulp) */
    return r;
}

/* ---------------------------------------------------------------- RNG */

typedef struct { uint32_t v[4]; } azg_u32x4;

AZG_HD void azg_mulhilo(uint32_t a, uint32_t b, uint32_t* hi, uint32_t* lo) {
    uint64_t p = (uint64_t)a * (uint64_t)b;
    *hi = (uint32_t)(p >> 32);
    *lo = (uint32_t)p;
}

/* Philox4x32-10 (Salmon et al., SC'11) */
AZG_HD azg_u32x4 azg_philox4x32(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
    for (int i = 0; i < 10; ++i) {
        uint32_t hi0, lo0, hi1, lo1;
        azg_mulhilo(0xD2511F53u, c0, &hi0, &lo0);
        azg_mulhilo(0xCD9E8D57u, c2, &hi1, &lo1);
        uint32_t n0 = hi1 ^ c1 ^ k0;
        uint32_t n1 = lo1;
        uint32_t n2 = hi0 ^ c3 ^ k1;
        uint32_t n3 = lo0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    azg_u32x4 r;
    r.v[0] = c0; r.v[1] = c1; r.v[2] = c2; r.v[3] = c3;
    return r;
}

/* gym Acrobot-v1 ("book" dynamics, torque noise 0; all link masses / lengths / inertias 1, centres of mass at 0.5, g = 9.8):
 * the derivative of (theta1, theta2, dtheta1, dtheta2) under torque a, with the constants multiplied out in gym's own order of
 * operations where a factor is not exactly 1 (alphazero_gym_amd/envs.py AcrobotEnv._dsdt is the definition; this is its mirror). */
AZG_HD void azg_acrobot_dsdt(const double* s, double a, double* ds) {
    const double pi = 3.141592653589793, g = 9.8;
    const double theta1 = s[0], theta2 = s[1], dtheta1 = s[2], dtheta2 = s[3];
    double sn2, cs2, sn, c12, c1;
    azg_sincos(theta2, &sn2, &cs2);
    azg_sincos((theta1 + theta2) - pi / 2.0, &sn, &c12);
    azg_sincos(theta1 - pi / 2.0, &sn, &c1);
    const double d1 = ((0.25 + (1.25 + cs2)) + 1.0) + 1.0;     /* m1 lc1^2 + m2 (l1^2 + lc2^2 + 2 l1 lc2 cos theta2) + I1 + I2 */
    const double d2 = (0.25 + 0.5 * cs2) + 1.0;                /* m2 (lc2^2 + l1 lc2 cos theta2) + I2 */
    const double phi2 = (0.5 * g) * c12;                       /* m2 lc2 g cos(theta1 + theta2 - pi / 2) */
    const double phi1 = ((-(0.5 * (dtheta2 * dtheta2)) * sn2 - ((1.0 * dtheta2) * dtheta1) * sn2) + (1.5 * g) * c1) + phi2;
    const double ddtheta2 = ((((a + (d2 / d1) * phi1) - (0.5 * (dtheta1 * dtheta1)) * sn2) - phi2)) / ((0.25 + 1.0) - (d2 * d2) / d1);
    const double ddtheta1 = -((d2 * ddtheta2 + phi1)) / d1;
    ds[0] = dtheta1; ds[1] = dtheta2; ds[2] = ddtheta1; ds[3] = ddtheta2;
}

/* AcrobotEnv.step: one classical Runge-Kutta step of dt = 0.2 (gym's rk4), angles wrapped into [-pi, pi], velocities bounded to
 * +-4 pi / +-9 pi; terminal when the tip is above the line (-cos theta1 - cos(theta1 + theta2) > 1); reward -1, 0 on the terminal step. */
AZG_HD void azg_acrobot_step(const double* s, int action, double* o, double* reward, int* done) {
    const double pi = 3.141592653589793, dt = 0.2, dt2 = 0.1;
    const double a = (double)(action - 1);
    double k1[4], k2[4], k3[4], k4[4], y[4];
    azg_acrobot_dsdt(s, a, k1);
    AZG_UNROLL for (int i = 0; i < 4; ++i) y[i] = s[i] + dt2 * k1[i];
    azg_acrobot_dsdt(y, a, k2);
    AZG_UNROLL for (int i = 0; i < 4; ++i) y[i] = s[i] + dt2 * k2[i];
    azg_acrobot_dsdt(y, a, k3);
    AZG_UNROLL for (int i = 0; i < 4; ++i) y[i] = s[i] + dt * k3[i];
    azg_acrobot_dsdt(y, a, k4);
    AZG_UNROLL for (int i = 0; i < 4; ++i) o[i] = s[i] + (dt / 6.0) * (((k1[i] + 2.0 * k2[i]) + 2.0 * k3[i]) + k4[i]);
    AZG_UNROLL for (int i = 0; i < 2; ++i) {   /* wrap(x, -pi, pi) */
        double x = o[i];
        for (int it = 0; it < 64 && x > pi; ++it) x = x - 2.0 * pi;
        for (int it = 0; it < 64 && x < -pi; ++it) x = x + 2.0 * pi;
        o[i] = x;
    }
    const double m1 = 4.0 * pi, m2 = 9.0 * pi;
    o[2] = o[2] < -m1 ? -m1 : (o[2] > m1 ? m1 : o[2]);
    o[3] = o[3] < -m2 ? -m2 : (o[3] > m2 ? m2 : o[3]);
    double sn, c0, c01;
    azg_sincos(o[0], &sn, &c0);
    azg_sincos(o[1] + o[0], &sn, &c01);
    const int d = (-c0 - c01) > 1.0;
    *done = d;
    *reward = d ? 0.0 : -1.0;
}
AZG_HD int azg_acrobot_terminal(const double* s) {
    double sn, c0, c01;
    azg_sincos(s[0], &sn, &c0);
    azg_sincos(s[1] + s[0], &sn, &c01);
    return (-c0 - c01) > 1.0;
}
AZG_HD void azg_acrobot_obs(const double* s, float* obs) {
    double sn, cs;
    azg_sincos(s[0], &sn, &cs);
    obs[0] = (float)cs; obs[1] = (float)sn;
    azg_sincos(s[1], &sn, &cs);
    obs[2] = (float)cs; obs[3] = (float)sn;
    obs[4] = (float)s[2]; obs[5] = (float)s[3];
}

/* uniform in (0,1) with 24 bits: (x>>8 + 0.5) * 2^-24 */
AZG_HD float azg_u01(uint32_t x) {
    return AZG_FMAF((float)(x >> 8), 5.9604644775390625e-08f, 2.98023223876953125e-08f);
}

#define AZG_STREAM_PW 0u      /* progressive-widening action noise, N(0,1) */
#define AZG_STREAM_EPS 1u     /* epsilon-greedy: v[0] -> u, v[1] -> random child */
#define AZG_STREAM_ROOT 2u    /* synthetic root states (bench / self-play resets): counter (tree, episode, 0, stream) */
#define AZG_STREAM_TIE 4u     /* AZG_TIE_RANDOM: v[0] picks among tied children: counter (tree, search, node_n << 16 ^ node record, stream) */
#define AZG_STREAM_ACT 3u     /* self-play: final action sampled from the visit counts: counter (tree, step, 0, stream) */
#define AZG_STREAM_SAMPLE 5u  /* prioritised row draws (azgym_priority.h): v[0], v[1] -> 64 bits: counter (net's first tree, sample index, draw, stream) */
#define AZG_STREAM_SLOT 6u    /* prioritised slot draws: v[0], v[1] -> 64 bits: counter (tree, sample index, 0, stream) */

/* fixed-seed reset state of game `tree`, episode `episode` (Pendulum theta~U(-pi,pi), theta_dot~U(-1,1);
 * CartPole ~U(-0.05,0.05)^4; MountainCar position~U(-0.6,-0.4), velocity 0: the envs' own reset laws).
 * kind: AZG_RESET_PENDULUM / AZG_RESET_CARTPOLE / AZG_RESET_MOUNTAINCAR (azg_reset_kind(env_id)) */
#define AZG_RESET_PENDULUM 0
#define AZG_RESET_CARTPOLE 1
#define AZG_RESET_MOUNTAINCAR 2
#define AZG_RESET_ACROBOT 3   /* all four state variables ~ U(-0.1, 0.1) */
/* (both MountainCar envs start at position U(-0.6, -0.4) with velocity 0) */
AZG_HD int azg_reset_kind(int env_id) {
    return env_id == 0 ? AZG_RESET_CARTPOLE : ((env_id == 3 || env_id == 4) ? AZG_RESET_MOUNTAINCAR : (env_id == 5 ? AZG_RESET_ACROBOT : AZG_RESET_PENDULUM));
}
AZG_HD void azg_reset_state(uint64_t seed, uint32_t tree, uint32_t episode, int kind, double* s);

/* the engine's draw #`draw` of stream `stream` for (global tree id, search index) */
AZG_HD azg_u32x4 azg_draw(uint64_t seed, uint32_t tree, uint32_t search, uint32_t draw, uint32_t stream) {
    return azg_philox4x32(tree, search, draw, stream, (uint32_t)seed, (uint32_t)(seed >> 32));
}

AZG_HD void azg_reset_state(uint64_t seed, uint32_t tree, uint32_t episode, int kind, double* s) {
    const double pi = 3.141592653589793;
    azg_u32x4 b = azg_draw(seed, tree, episode, 0u, AZG_STREAM_ROOT);
    double u[4];
    for (int k = 0; k < 4; ++k) u[k] = ((double)b.v[k] + 0.5) * (1.0 / 4294967296.0);
    if (kind == AZG_RESET_CARTPOLE) {
        for (int k = 0; k < 4; ++k) s[k] = -0.05 + 0.1 * u[k];
    } else if (kind == AZG_RESET_ACROBOT) {
        for (int k = 0; k < 4; ++k) s[k] = -0.1 + 0.2 * u[k];
    } else if (kind == AZG_RESET_MOUNTAINCAR) {
        s[0] = -0.6 + 0.2 * u[0];
        s[1] = 0.0;
    } else {
        s[0] = -pi + 2.0 * pi * u[0];
        s[1] = -1.0 + 2.0 * u[1];
    }
}

/* standard normal (Box-Muller, cosine branch) */
AZG_HD float azg_normal(uint64_t seed, uint32_t tree, uint32_t search, uint32_t draw) {
    azg_u32x4 b = azg_draw(seed, tree, search, draw, AZG_STREAM_PW);
    float u1 = azg_u01(b.v[0]);
    float u2 = azg_u01(b.v[1]);
    float r = __builtin_sqrtf(-2.0f * azg_logf(u1));
    return r * azg_cos2pif(u2);
}

#endif /* AZG_MATH_H */
