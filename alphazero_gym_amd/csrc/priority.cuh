// priority.cuh -- prioritised sampling from the device replay ring (include/azgym_priority.h states the rule; compiled in one translation
// unit: engine_selfplay.hip).  The draws' kernels: the priority q of every stored row; the prefix sums of a net's q in two levels (each
// segment of PR_SEG rows scanned by one workgroup, then the segment totals scanned by one wave per net); the row draws, each a binary
// search over the segment totals and then within one segment; the slot draws, one thread per game column.  Every sum is an integer add
// of uint64 values whose total stays below 2^63, so the sums are exact whatever the order and nothing here is atomic.  The
// importance-sampling weights' kernels: a net's least q in the same two levels, then the weight of every stored row.  The priorities
// fed back from the trainer's value errors (at the end): a net's largest seen error in those two levels, then q of every stored row.
// The rules are device functions (priority_q, priority_trained_q, prio_scan_totals, prio_min_net, prio_draw_row, priority_is_weight):
// priority_online.cuh's fused kernels call them too.
#pragma once
#include "../../include/azg_math.h"
#include "../../include/azgym_priority.h"

typedef unsigned long long pr_u64;
#define PR_THREADS 256
#define PR_SEG 256   // rows per scan segment: one per thread of a workgroup

// ------------------------------------------------------------------------------------------------ priorities

// d -> q.  The sum, the product and the functions' own steps are rounded one by one: no contraction into a fused multiply-add.
__host__ __device__ __forceinline__ pr_u64 priority_q(float d, float alpha, float eps) {
#pragma clang fp contract(off)
    float p = 1.0f;
    if (alpha != 0.0f) {
        const float s = d + eps;
        const float m = alpha * azg_logf(s);
        p = azg_expf(m);
    }
    if (!(p >= 9.5367431640625e-07f)) return 1ull;   // below 2^-20, or NaN
    if (p >= 1048576.0f) return 1ull << 40;
    return (pr_u64)((double)p * 1048576.0);
}

// One thread per stored row, thread slot * B + tree: consecutive lanes are consecutive trees of one slot, so every load of the
// [slot][tree] arrays is coalesced (the V_target column is a strided load of one float per row).
struct Priorities {
    long long rows_n;         // stored rows: size_steps * n_trees
    int source;               // AZG_PRIO_*
    int row_len, vcol;        // a row's length and its V_target column
    float alpha, eps;
    const double* value;      // AZG_PRIO_VALUE_GAP: the kept float64 values [capacity_steps][B]
    const float* rows;        // ... and the replay ring [capacity_steps][B][row_len]
    const float* given;       // AZG_PRIO_GIVEN: the caller's d, uploaded [size_steps][B]
    pr_u64* q;                // [capacity_steps][B]
};
__global__ __launch_bounds__(PR_THREADS) void priorities_kernel(Priorities pr) {
    const long long idx = (long long)blockIdx.x * PR_THREADS + threadIdx.x;
    if (idx >= pr.rows_n) return;
    float d;
    if (pr.source == AZG_PRIO_GIVEN) {
        d = pr.given[idx];
    } else {
        const double z = (double)pr.rows[(size_t)idx * pr.row_len + pr.vcol];
        d = (float)fabs(pr.value[idx] - z);
    }
    pr.q[idx] = priority_q(d, pr.alpha, pr.eps);
}

// ------------------------------------------------------------------------------------------------ prefix sums

// Inclusive scan over the 64 lanes of a wave
__device__ __forceinline__ pr_u64 wave_scan_u64(pr_u64 v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const pr_u64 up = __shfl_up(v, o, 64);
        if (lane >= o) v += up;
    }
    return v;
}

// Net k's rows in its own numbering: row i = slot * T + j is element slot * B + k * T + j of a [slot][tree] array; N = size * T rows,
// nseg = ceil(N / PR_SEG) segments.  Net k's block of the scratch starts at k * N (within, at k * nseg (seg)): the nets' blocks tile
// [0, size * B) and [0, n_nets * nseg).
struct PrioScan {
    int B, T;
    int N, nseg;
    const pr_u64* q;     // [capacity_steps][B]
    pr_u64* within;      // [n_nets][N]: the inclusive prefix sum of a row's q within its segment
    pr_u64* seg;         // [n_nets][nseg]: a segment's total, then (prio_scan_totals_kernel) the inclusive prefix sum of the totals
};
__device__ __forceinline__ size_t prio_elem(const PrioScan& ps, int k, int i) {
    const int slot = i / ps.T;
    return (size_t)slot * ps.B + (size_t)k * ps.T + (i - slot * ps.T);
}

// grid (nseg, n_nets): one workgroup scans one segment
__global__ __launch_bounds__(PR_THREADS) void prio_scan_segments_kernel(PrioScan ps) {
    __shared__ pr_u64 wave_tot[PR_THREADS / 64];
    const int k = blockIdx.y, seg = blockIdx.x;
    const int i = seg * PR_SEG + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    pr_u64 v = i < ps.N ? ps.q[prio_elem(ps, k, i)] : 0ull;
    v = wave_scan_u64(v, lane);
    if (lane == 63) wave_tot[wave] = v;
    __syncthreads();
    pr_u64 before = 0ull;
#pragma unroll
    for (int w = 0; w < PR_THREADS / 64; ++w)
        if (w < wave) before += wave_tot[w];
    v += before;
    if (i < ps.N) ps.within[(size_t)k * ps.N + i] = v;
    if (threadIdx.x == PR_THREADS - 1) ps.seg[(size_t)k * ps.nseg + seg] = v;   // (rows past N add 0: the last thread holds the total)
}

// grid (n_nets), one wave: lane l folds the run of segments [l * per, l * per + per), the lanes' sums are scanned, then every lane
// writes its run's inclusive prefix sums
__device__ __forceinline__ void prio_scan_totals(const PrioScan& ps, int k, int lane) {
    pr_u64* seg = ps.seg + (size_t)k * ps.nseg;
    const int per = (ps.nseg + 63) / 64;
    const int lo = lane * per < ps.nseg ? lane * per : ps.nseg;
    const int hi = lo + per < ps.nseg ? lo + per : ps.nseg;
    pr_u64 sum = 0ull;
    for (int s = lo; s < hi; ++s) sum += seg[s];
    pr_u64 acc = wave_scan_u64(sum, lane) - sum;   // the segments before this lane's run
    for (int s = lo; s < hi; ++s) { acc += seg[s]; seg[s] = acc; }
}
__global__ __launch_bounds__(64) void prio_scan_totals_kernel(PrioScan ps) { prio_scan_totals(ps, blockIdx.x, threadIdx.x); }

// ------------------------------------------------------------------------------------------------ draws

// the 64 bits of a draw times the total, high half: uniform over [0, total)
__device__ __forceinline__ pr_u64 prio_target(const azg_u32x4& w, pr_u64 total) {
    const pr_u64 x = (pr_u64)w.v[0] << 32 | (pr_u64)w.v[1];
    return __umul64hi(x, total);
}
// the least index in [0, n) with c[index] > target; c is non-decreasing and c[n - 1] > target
__device__ __forceinline__ int prio_upper(const pr_u64* c, int n, pr_u64 target) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (c[mid] > target) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// Draw d of net k under sample_index (ps after both scans): the row number in the net's own numbering
__device__ __forceinline__ int prio_draw_row(const PrioScan& ps, int k, unsigned long long seed, unsigned tree_base, unsigned sample_index,
                                             int d) {
    const pr_u64* seg = ps.seg + (size_t)k * ps.nseg;
    const pr_u64* within = ps.within + (size_t)k * ps.N;
    const azg_u32x4 w = azg_draw(seed, tree_base + (unsigned)(k * ps.T), sample_index, (unsigned)d, AZG_STREAM_SAMPLE);
    const pr_u64 target = prio_target(w, seg[ps.nseg - 1]);
    const int s = prio_upper(seg, ps.nseg, target);
    const pr_u64 rest = target - (s ? seg[s - 1] : 0ull);
    const int first = s * PR_SEG;
    const int len = ps.N - first < PR_SEG ? ps.N - first : PR_SEG;
    return first + prio_upper(within + first, len, rest);
}

// grid (ceil(n_order / PR_THREADS), n_nets): one thread per draw
struct PrioRows {
    PrioScan ps;              // (after both scan kernels)
    int n_order;
    unsigned sample_index, tree_base;
    unsigned long long seed;
    int* order;               // [n_nets][n_order]
};
__global__ __launch_bounds__(PR_THREADS) void prio_draw_rows_kernel(PrioRows dr) {
    const int k = blockIdx.y;
    const int d = blockIdx.x * PR_THREADS + threadIdx.x;
    if (d >= dr.n_order) return;
    dr.order[(size_t)k * dr.n_order + d] = prio_draw_row(dr.ps, k, dr.seed, dr.tree_base, dr.sample_index, d);
}

// One thread per game column, walking its stored slots twice (the total, then the running sum); consecutive lanes are consecutive
// trees, so every load is coalesced.
struct PrioSlots {
    int B, size;
    unsigned sample_index, tree_base;
    unsigned long long seed;
    const pr_u64* q;          // [capacity_steps][B]
    int* slots;               // [B]
};
__global__ __launch_bounds__(PR_THREADS) void prio_draw_slots_kernel(PrioSlots dr) {
    const int t = blockIdx.x * PR_THREADS + threadIdx.x;
    if (t >= dr.B) return;
    pr_u64 total = 0ull;
    for (int s = 0; s < dr.size; ++s) total += dr.q[(size_t)s * dr.B + t];
    const azg_u32x4 w = azg_draw(dr.seed, dr.tree_base + (unsigned)t, dr.sample_index, 0u, AZG_STREAM_SLOT);
    const pr_u64 target = prio_target(w, total);
    pr_u64 run = 0ull;
    int s = 0;
    for (; s < dr.size - 1; ++s) {   // (total > target: the last slot is the answer if none before it was)
        run += dr.q[(size_t)s * dr.B + t];
        if (run > target) break;
    }
    dr.slots[t] = s;
}

// ------------------------------------------------------------------------------------------------ importance-sampling weights

// q, the least q of the row's net, beta -> w = (q_min / q)^beta.  Every step is rounded on its own, as in priority_q.
__host__ __device__ __forceinline__ float priority_is_weight(pr_u64 q, pr_u64 q_min, float beta) {
#pragma clang fp contract(off)
    if (beta == 0.0f || q == q_min) return 1.0f;
    const float r = (float)((double)q_min / (double)q);   // both at most 2^40: exact conversions, one rounded division
    const float m = beta * azg_logf(r);
    return azg_expf(m);
}

// The least q of every net, in the scan's two levels and over the scan's segments (PrioScan's numbering of a net's rows).
struct PrioMin {
    int B, T;
    int N, nseg;
    const pr_u64* q;     // [capacity_steps][B]
    pr_u64* seg_min;     // [n_nets][nseg]: a segment's least q
    pr_u64* net_min;     // [n_nets]
};
__device__ __forceinline__ pr_u64 wave_min_u64(pr_u64 v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const pr_u64 other = __shfl_xor(v, o, 64);
        v = other < v ? other : v;
    }
    return v;
}

// grid (nseg, n_nets): one workgroup folds one segment (a row past N counts as the largest uint64; a segment has at least one row)
__global__ __launch_bounds__(PR_THREADS) void prio_min_segments_kernel(PrioMin pm) {
    __shared__ pr_u64 wave_least[PR_THREADS / 64];
    const int k = blockIdx.y, seg = blockIdx.x;
    const int i = seg * PR_SEG + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    pr_u64 v = ~0ull;
    if (i < pm.N) {
        const int slot = i / pm.T;
        v = pm.q[(size_t)slot * pm.B + (size_t)k * pm.T + (i - slot * pm.T)];
    }
    v = wave_min_u64(v);
    if (lane == 0) wave_least[wave] = v;
    __syncthreads();
    if (threadIdx.x != 0) return;
#pragma unroll
    for (int w = 1; w < PR_THREADS / 64; ++w) v = wave_least[w] < v ? wave_least[w] : v;
    pm.seg_min[(size_t)k * pm.nseg + seg] = v;
}

// grid (n_nets), one wave: lane l folds segments l, l + 64, ...; then the wave's least
__device__ __forceinline__ pr_u64 prio_min_net(const pr_u64* seg, int nseg, int lane) {
    pr_u64 v = ~0ull;
    for (int s = lane; s < nseg; s += 64) v = seg[s] < v ? seg[s] : v;
    return wave_min_u64(v);
}
__global__ __launch_bounds__(64) void prio_min_nets_kernel(PrioMin pm) {
    const pr_u64 v = prio_min_net(pm.seg_min + (size_t)blockIdx.x * pm.nseg, pm.nseg, threadIdx.x);
    if (threadIdx.x == 0) pm.net_min[blockIdx.x] = v;
}

// One thread per stored row, thread slot * B + tree, like priorities_kernel: q and w are coalesced, the net's minimum is one of a few
// addresses per wave.
struct IsWeights {
    long long rows_n;         // stored rows: size_steps * n_trees
    int B, T;
    float beta;
    const pr_u64* q;          // [capacity_steps][B]
    const pr_u64* net_min;    // [n_nets] (after both minimum kernels)
    float* w;                 // [capacity_steps][B]
};
__global__ __launch_bounds__(PR_THREADS) void is_weights_kernel(IsWeights iw) {
    const long long idx = (long long)blockIdx.x * PR_THREADS + threadIdx.x;
    if (idx >= iw.rows_n) return;
    const int tree = (int)(idx % iw.B);
    iw.w[idx] = priority_is_weight(iw.q[idx], iw.net_min[tree / iw.T], iw.beta);
}

// ------------------------------------------------------------------------------------------------ priorities from the trainer's errors

#define PR_ERR_UNSEEN (-1.0f)           // the sentinel of an entry never trained on since it was stored ...
#define PR_ERR_UNSEEN_BITS 0xBF800000   // ... and its bit pattern, for the 32-bit fills

// The largest seen error of every net, in the minimum's two levels and over the same segments.  Only entries >= 0 count (the sentinel
// and NaN do not): non-negative floats order like their bit patterns read as int32 (-0.0f counts as +0.0f), and -1 stands for "none",
// so this is an integer maximum, exact in any order.
struct PrioErrMax {
    int B, T;
    int N, nseg;
    const float* err;    // [capacity_steps][B]
    int* seg_max;        // [n_nets][nseg]: the bits of a segment's largest seen error, or -1
    int* net_max;        // [n_nets]
};
__device__ __forceinline__ int wave_max_i32(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int other = __shfl_xor(v, o, 64);
        v = other > v ? other : v;
    }
    return v;
}

// grid (nseg, n_nets): one workgroup folds one segment (a row past N counts as none)
__global__ __launch_bounds__(PR_THREADS) void prio_errmax_segments_kernel(PrioErrMax pm) {
    __shared__ int wave_most[PR_THREADS / 64];
    const int k = blockIdx.y, seg = blockIdx.x;
    const int i = seg * PR_SEG + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int v = -1;
    if (i < pm.N) {
        const int slot = i / pm.T;
        const float x = pm.err[(size_t)slot * pm.B + (size_t)k * pm.T + (i - slot * pm.T)];
        if (x >= 0.0f) v = __float_as_int(fabsf(x));
    }
    v = wave_max_i32(v);
    if (lane == 0) wave_most[wave] = v;
    __syncthreads();
    if (threadIdx.x != 0) return;
#pragma unroll
    for (int w = 1; w < PR_THREADS / 64; ++w) v = wave_most[w] > v ? wave_most[w] : v;
    pm.seg_max[(size_t)k * pm.nseg + seg] = v;
}

// grid (n_nets), one wave: lane l folds segments l, l + 64, ...; then the wave's largest
__global__ __launch_bounds__(64) void prio_errmax_nets_kernel(PrioErrMax pm) {
    const int* seg = pm.seg_max + (size_t)blockIdx.x * pm.nseg;
    int v = -1;
    for (int s = threadIdx.x; s < pm.nseg; s += 64) v = seg[s] > v ? seg[s] : v;
    v = wave_max_i32(v);
    if (threadIdx.x == 0) pm.net_max[blockIdx.x] = v;
}

// One thread per stored row, thread slot * B + tree, like priorities_kernel.  A seen entry (anything but the sentinel, NaN included) is
// the row's d; an unseen one takes the largest seen error of its net (1.0f if the net has none), the value gap, or a constant.
// q is priority_q's, except that a d that is NaN or +inf is decided here.
struct PrioritiesTrained {
    long long rows_n;         // stored rows: size_steps * n_trees
    int unseen;               // AZG_UNSEEN_*
    int row_len, vcol;        // a row's length and its V_target column
    int B, T;
    float alpha, eps, unseen_d;
    const float* err;         // [capacity_steps][B]
    const int* net_max;       // AZG_UNSEEN_MAX: [n_nets] (after both maximum kernels)
    const double* value;      // AZG_UNSEEN_VALUE_GAP: the kept float64 values [capacity_steps][B]
    const float* rows;        // ... and the replay ring [capacity_steps][B][row_len]
    pr_u64* q;                // [capacity_steps][B]
};
// q of the stored row at element idx = slot * B + tree
__device__ __forceinline__ pr_u64 priority_trained_q(const PrioritiesTrained& pr, long long idx) {
    float d = pr.err[idx];
    if (d == PR_ERR_UNSEEN) {
        if (pr.unseen == AZG_UNSEEN_MAX) {
            const int m = pr.net_max[(int)(idx % pr.B) / pr.T];
            d = m < 0 ? 1.0f : __int_as_float(m);
        } else if (pr.unseen == AZG_UNSEEN_VALUE_GAP) {
            const double z = (double)pr.rows[(size_t)idx * pr.row_len + pr.vcol];
            d = (float)fabs(pr.value[idx] - z);
        } else {
            d = pr.unseen_d;
        }
    }
    // (a NaN or +inf d lies outside azg_logf's domain, which reads its argument's bits: p is taken as NaN / +inf by the header's rule)
    pr_u64 q;
    if (pr.alpha != 0.0f && !(d < __builtin_inff())) q = d != d ? 1ull : 1ull << 40;
    else q = priority_q(d, pr.alpha, pr.eps);
    return q;
}
__global__ __launch_bounds__(PR_THREADS) void priorities_trained_kernel(PrioritiesTrained pr) {
    const long long idx = (long long)blockIdx.x * PR_THREADS + threadIdx.x;
    if (idx >= pr.rows_n) return;
    pr.q[idx] = priority_trained_q(pr, idx);
}
