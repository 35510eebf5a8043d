// replay_ring.h -- the device replay ring of self-play as the host keeps it (engine_selfplay.hip): ReplayBuffer's books in steps, the
// game settings a step hands to the kernels, the games' counters, the rows and the three optional columns beside them, in one
// lifetime of device memory that a begin ends.  One member of azg_engine.
#pragma once
#include <cstdint>
#include <vector>

#include "hip_host.h"

// One net's rule of the lambda-return targets (azgym_lambda.h) as lambda_targets_kernel reads it: what the host resolved of the net's
// azg_return_rule -- n_step clamped to the ring's size, om = 1.0 - lambda in float64, gamma the search's where the flag asks for it
struct __attribute__((aligned(16))) ReturnRuleRec {
    int n_step, pad;
    double lambda, om, gamma;
};
static_assert(sizeof(ReturnRuleRec) == 32, "ReturnRuleRec must be 32 bytes");

// Everything a begin starts over: value-initialised as a whole (ReplayRing::restart), so no member can outlive the memory it points into
struct ReplayRingState {
    int on = 0;                      // azg_selfplay_begin has been called
    int B = 0, cap = 0, steps = 0, insert = 0, row = 0, mode = 0;   // games (rows per step: n_trees); capacity, ReplayBuffer.size and
    long long total = 0;                                            // .insert_index in steps; row length; AZG_RING_*; steps since the begin
    int max_len = 0, det = 0, fs = 0;   // azg_selfplay_config's game settings, as a step hands them to SelfPlay and its ActRule
    double agent_eps = 0.0;
    double* ctab = nullptr;          // (c / m)^temperature (act_rule_ctab; NULL: the rule needs none)
    uint32_t step_idx = 0;
    int* t = nullptr; int* episode = nullptr; int* fcnt = nullptr; double* ret = nullptr; double* fsum = nullptr;   // per game [B]
    float* rows = nullptr;           // [cap][B][row]
    // The optional columns (azg_selfplay_keep_*).  on 0: not kept; a column switched off keeps its allocation until the next begin.
    struct States {                  // the stored steps' env states d [cap][B][S_env], and what a reanalysis searches from: staging
        int on = 0;                  // roots [B][S_env], zero carried counts [B] and the device copy of its slots [B]
        double* d = nullptr; double* roots = nullptr; int* carry = nullptr; int* slots = nullptr;
        std::vector<int32_t> h_slots;   // host side of slots (outlives the asynchronous copy)
    } states;
    struct Transitions {             // the stored steps' reward, float64 value target, action and end kind, each [cap][B]
        int on = 0;
        double* reward = nullptr; double* value = nullptr; float* action = nullptr; int* end = nullptr;
    } tr;
    struct ValueRefresh {            // (azgym_refresh.h) the slot list of the last azg_selfplay_refresh_values call: d [cap] on the
        int* d = nullptr;            // device (grow-only within a begin) and its host side, which the call's asynchronous copy reads
        size_t cap = 0;              // (ReplayRing::slots_copied tells when it may be rewritten)
        std::vector<int32_t> h;
    } refresh;
    struct ReturnRules {             // (azgym_lambda.h) the rule table of the last lambda-target call: d [n] on the device, allocated by
        ReturnRuleRec* d = nullptr;  // the first call, and its host side, which the call's asynchronous copy reads (ReplayRing::
        int n = 0;                   // rules_copied tells when it may be rewritten)
        std::vector<ReturnRuleRec> h;
    } rules;
    struct Priorities {              // (azgym_priority.h) a priority q per stored row [cap][B], the upload of a caller's d [cap][B], the
        int on = 0;                  // draws' prefix sums (within a segment [cap][B], segment totals [segs]) and the drawn slots [B]
        unsigned long long* q = nullptr; unsigned long long* within = nullptr; unsigned long long* seg = nullptr;
        float* given = nullptr; int* slots = nullptr;
        size_t segs = 0;
        std::vector<float> h_given;  // host side of given (outlives the asynchronous copy)
        long long gen = -1;          // rows_gen when azg_selfplay_priorities last ran (-1: not since the begin or the switch-on)
        // azg_selfplay_is_weights, allocated by its first call: the weight of every stored row [cap][B] and the minima of q (one per scan
        // segment [segs], then one per net [B]); w_gen: rows_gen when the weights were last computed from the priorities that stand (-1:
        // never, or azg_selfplay_priorities has run since)
        float* w = nullptr; unsigned long long* w_min = nullptr;
        long long w_gen = -1;
        // azg_selfplay_keep_errors: the trainer's value error of every stored row [cap][B] (-1.0f: not trained on since it was stored),
        // the bits of the largest seen error per scan segment [segs] and per net [B], and the host side of an upload
        int err_on = 0;
        float* err = nullptr; int* err_max = nullptr;
        std::vector<float> h_err;
    } prio;
};

struct ReplayRing : ReplayRingState {
    DeviceAllocs mem;                // every device pointer of the state
    long long rows_gen = 0;          // counts the changes of the set of stored rows: a step, a clear, a begin (never reset)
    // recorded behind every copy of rules.h to the device (created by the first one): a later call waits for it before it rewrites
    // rules.h, so the staging outlives the copy that reads it
    hipEvent_t rules_copied = nullptr;
    hipEvent_t slots_copied = nullptr;   // the same for refresh.h (azg_selfplay_refresh_values)
    ReplayRing() = default;
    ReplayRing(const ReplayRing&) = delete;
    ReplayRing& operator=(const ReplayRing&) = delete;
    ~ReplayRing() {
        if (rules_copied) (void)hipEventDestroy(rules_copied);
        if (slots_copied) (void)hipEventDestroy(slots_copied);
    }
    // a begin: the memory goes, and every member of the state with it (the engine's stream is idle)
    void restart() { mem.clear(); static_cast<ReplayRingState&>(*this) = {}; rows_gen += 1; }
    // ReplayBuffer.store (buffers.py:75-82): the slot this step's block of B rows goes to
    int store_slot() {
        if (steps < cap) return steps++;
        const int slot = insert;
        insert = (insert + 1) % steps;
        return slot;
    }
    void stepped() { total += 1; step_idx += 1; rows_gen += 1; }   // the step's kernel has been launched
    void clear_rows() { steps = 0; insert = 0; rows_gen += 1; }   // ReplayBuffer.clear (buffers.py:56-60)
    size_t stored_rows() const { return (size_t)steps * B; }
};
