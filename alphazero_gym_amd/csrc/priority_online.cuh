// priority_online.cuh -- the refresh in front of every minibatch of an online epoch (include/azgym_train_online.h; compiled in one
// translation unit, engine_selfplay.hip, after priority.cuh whose device functions state every rule used here).  Three launches
// stand for azg_selfplay_priorities_trained's q kernel, azg_selfplay_sample_rows' three, azg_selfplay_is_weights' three and the
// epoch's gather: q + segment scan + segment minimum in one pass over err; the segment totals' scan + the net's minimum; and draw +
// weight + gather, one wave per drawn row.  Under AZG_UNSEEN_MAX the two error-maximum launches of priority.cuh stay in front: 5
// launches per minibatch before the step's own, 3 under the other modes.  Integer sums and minima only, nothing atomic; the LDS is
// the scan's few words.
#pragma once
#include "gather_row.cuh"
#include "priority.cuh"

// grid (nseg, n_nets): one workgroup per scan segment, thread i of net k at element prio_elem(ps, k, i).  Writes q of its row, the
// row's inclusive prefix sum within the segment (prio_scan_segments_kernel's `within` and `seg`) and the segment's least q
// (prio_min_segments_kernel's seg_min).  A row past N adds 0 and counts as the largest uint64.
struct OnlineRefresh {
    PrioritiesTrained pr;    // (rows_n is not read: the grid is the scan's)
    PrioScan ps;             // ps.q == pr.q, written here
    pr_u64* seg_min;         // [n_nets][nseg]
};
__global__ __launch_bounds__(PR_THREADS) void online_refresh_segments_kernel(OnlineRefresh on) {
    __shared__ pr_u64 wave_tot[PR_THREADS / 64];
    __shared__ pr_u64 wave_least[PR_THREADS / 64];
    const PrioScan& ps = on.ps;
    const int k = blockIdx.y, seg = blockIdx.x;
    const int i = seg * PR_SEG + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    pr_u64 v = 0ull, least = ~0ull;
    if (i < ps.N) {
        const size_t at = prio_elem(ps, k, i);
        v = least = priority_trained_q(on.pr, (long long)at);
        on.pr.q[at] = v;
    }
    v = wave_scan_u64(v, lane);
    least = wave_min_u64(least);
    if (lane == 63) wave_tot[wave] = v;
    if (lane == 0) wave_least[wave] = least;
    __syncthreads();
    pr_u64 before = 0ull;
#pragma unroll
    for (int w = 0; w < PR_THREADS / 64; ++w)
        if (w < wave) before += wave_tot[w];
    v += before;
    if (i < ps.N) ps.within[(size_t)k * ps.N + i] = v;
    if (threadIdx.x != PR_THREADS - 1) return;
    ps.seg[(size_t)k * ps.nseg + seg] = v;   // (rows past N add 0: the last thread holds the total)
#pragma unroll
    for (int w = 0; w < PR_THREADS / 64 - 1; ++w) least = wave_least[w] < least ? wave_least[w] : least;
    on.seg_min[(size_t)k * ps.nseg + seg] = least;
}

// grid (n_nets), one wave: prio_scan_totals_kernel's scan of the net's segment totals and prio_min_nets_kernel's fold of its segment
// minima
__global__ __launch_bounds__(64) void online_refresh_nets_kernel(PrioScan ps, const pr_u64* seg_min, pr_u64* net_min) {
    const int k = blockIdx.x, lane = threadIdx.x;
    prio_scan_totals(ps, k, lane);
    const pr_u64 v = prio_min_net(seg_min + (size_t)k * ps.nseg, ps.nseg, lane);
    if (lane == 0) net_min[k] = v;
}

// grid (ceil(n_rows / 4), n_nets), train_gather_errors_kernel's: one wave per drawn row.  Draw b of net k under sample_index is made
// with wave-uniform operands (both binary searches run on the scalar unit), the row's weight comes from its q and the net's minimum
// (no other row's weight is computed), and the row is copied into the minibatch's staging arrays with its weight and its element
// index; the row number goes to the log.
struct OnlineDraw {
    PrioScan ps;             // (after online_refresh_nets_kernel)
    GatherRow g;
    unsigned sample_index, tree_base;
    unsigned long long seed;
    float beta;
    int n_rows;              // rows per net of the minibatch
    const pr_u64* net_min;   // [n_nets]
    const float* rows;       // the replay ring [capacity_steps][B][row_len]
    float *obs, *actions, *counts, *values, *wout;   // the staging arrays, [n_nets][n_rows][.]
    long long* at_out;       // [n_nets][n_rows]
    int* drawn;              // this minibatch's block of the log, [n_nets][n_rows]
};
__global__ __launch_bounds__(PR_THREADS) void online_draw_gather_kernel(OnlineDraw od) {
    const int net = blockIdx.y, lane = threadIdx.x & 63;
    const int b = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (PR_THREADS / 64) + (threadIdx.x >> 6)));
    if (b >= od.n_rows) return;
    const int i = __builtin_amdgcn_readfirstlane(prio_draw_row(od.ps, net, od.seed, od.tree_base, od.sample_index, b));
    const size_t at = prio_elem(od.ps, net, i);
    const size_t out = (size_t)net * od.n_rows + b;
    gather_row(od.g, od.rows + at * od.g.row_len, out, lane, od.obs, od.actions, od.counts, od.values);
    if (lane != 0) return;
    od.wout[out] = priority_is_weight(od.ps.q[at], od.net_min[net], od.beta);
    od.at_out[out] = (long long)at;
    od.drawn[out] = i;
}
