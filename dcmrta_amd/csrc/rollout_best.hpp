// rollout_best.hpp -- the best-keeping form of the persistent rollout (dcm_set_best_log: while set, every env keeps the best episode it
// has finished since dcm_reset -- by the pair (finished tasks, reward) -- with its summary row, its ordinal and its complete route and
// arrival log, on the device, across episodes and launches).
// Included by dcmrta_env.hip inside its anonymous namespace, after rollout_fast.hpp, in the translation unit of this form only
// (-DDCM_TU_B, or a one-unit developer build).
//
// The form is the existing kernel texts compiled once more:
//   k_bs_rollout_fast    from k_rollout_fast.inc    one-chunk layouts
//   k_bs_rollout_random  from k_rollout_random.inc  every other launch
// with the epsilon-greedy form's arguments plus the best log.  All three entry points run it while both logs are set:
// dcm_rollout_explore as it runs k_ex_*, dcm_rollout_policy / dcm_rollout_random with explore_q32 = 0 and `policy` any of the three,
// which are the decisions and the budget rule of k_lg_*.  The new work is keep_best below, called where a text sees a freshly
// finished episode and in front of the restart that empties the rollout log; the decision loop is the epsilon-greedy form's.
// No renewing form (the best of different instances means nothing: the host refuses the launch while a stride is set), no
// wave-priority (PRIO) instantiation, no form of k_rollout_fast_mc / k_rollout_fast_g (plan::form_rollout_kind).
#pragma once

// Keep the episode that env e has just finished if it beats the kept one: more finished tasks (summary column 1), or as many and a
// larger reward (column 0); strict and exact in fp64, so a tie keeps the earlier episode and a second look at the same episode
// changes nothing.  Wave-uniform branch; on an improvement the wave copies the summary row, the ordinal (Hdr::episodes before
// terminal()'s increment: the k of the return log), every agent's length (may exceed cap) and the entries [0, min(len, cap)) of every
// agent row a < A_, lanes striding one row at a time.
// REGS: the lengths are the fast form's FastLog registers (`lens`: lane a holds agent a's); else they are read from the log.
// The rows were stored by other lanes of this wave and the summary row by lane 0: a wave's vector memory operations are performed in
// order, so the wavefront fence (the compiler's order) is all the copy needs.
// Out of line, like the terminal metrics it follows: once per episode, and the kernels keep the registers and the schedule of their
// twins.  (Arguments of a device function arrive in vector registers: the wave-uniform ones are made scalar again first.)
template <class T>
__device__ __forceinline__ T* uni_ptr(T* p) { return (T*)uni((uint64_t)p); }
template <bool REGS>
__device__ __noinline__ void keep_best(BestLog best, RouteLog lg, int e, int BA, int A_, const double* row, int32_t lens) {
    const int lane = threadIdx.x;
    e = uni(e); BA = uni(BA); A_ = uni(A_);
    const int cap = uni(lg.cap);
    const size_t r0 = (size_t)e * BA;                                             // the env's first agent row
    const int16_t* const src_task = uni_ptr(lg.task) + r0 * cap;
    const double* const src_arrival = uni_ptr(lg.arrival) + r0 * cap;
    const int32_t* const src_len = uni_ptr(lg.len) + r0;
    int16_t* const dst_task = uni_ptr(best.task) + r0 * cap;
    double* const dst_arrival = uni_ptr(best.arrival) + r0 * cap;
    int32_t* const dst_len = uni_ptr(best.len) + r0;
    double* const kept_row = uni_ptr(best.summary) + (size_t)e * 8;
    int32_t* const kept_ord = uni_ptr(best.episode) + e;
    row = uni_ptr(row);
    WSYNC();
    // lane c (mod 8) holds column c of the episode's row and of the kept one
    const int c = lane & 7;
    const double cand = row[c], kept = kept_row[c];
    const int32_t kept_ep = uni(lane < 8 ? *kept_ord : 0);
    const double cn = rl(cand, 1), cr = rl(cand, 0), kn = rl(kept, 1), kr = rl(kept, 0);
    if (!(kept_ep == -1 || cn > kn || (cn == kn && cr > kr))) return;
    if (lane < 8) kept_row[lane] = cand;
    if (lane == 0) *kept_ord = (int32_t)(((const Hdr*)smem)->episodes - 1u);
#pragma nounroll
    for (int a = 0; a < A_; a++) {
        int n;
        if constexpr (REGS) n = rli(lens, a); else n = uni(src_len[a]);
        const int m = n < cap ? n : cap;
        const size_t o = (size_t)a * cap;
        for (int i = lane; i < m; i += WAVE) {
            dst_task[o + i] = src_task[o + i];
            dst_arrival[o + i] = src_arrival[o + i];
        }
        if (lane == 0) dst_len[a] = n;
    }
}

#define DCM_BEST 1
#define DCM_RENEW 0
#include "k_rollout_random.inc"
#include "k_rollout_fast.inc"
#undef DCM_RENEW
#undef DCM_BEST
