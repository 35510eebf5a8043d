// gather_row.cuh -- one replay row into a minibatch's staging arrays: what the trainer's gather kernels (train.cuh) and the online
// epoch's draw (priority_online.cuh) do with the row they have picked.
#pragma once

// floats of a replay row: obs[state_dim] | actions[A] | counts[A] | Q[A] | V
struct GatherRow {
    int row_len, state_dim, A;
};

// One wave copies the row at src to place `out` of obs [.][state_dim], actions and counts [.][A] and values [.]: lane c takes floats c,
// c + 64, ... of the row, so a row is read as coalesced segments; the Q columns are skipped.
__device__ __forceinline__ void gather_row(const GatherRow& g, const float* src, size_t out, int lane, float* obs, float* actions,
                                           float* counts, float* values) {
    const int a0 = g.state_dim, c0 = a0 + g.A, q0 = c0 + g.A, v0 = g.row_len - 1;
    for (int c = lane; c < g.row_len; c += 64) {
        if (c >= q0 && c < v0) continue;
        const float x = src[c];
        if (c < a0) obs[out * g.state_dim + c] = x;
        else if (c < c0) actions[out * g.A + (c - a0)] = x;
        else if (c < q0) counts[out * g.A + (c - c0)] = x;
        else values[out] = x;
    }
}
