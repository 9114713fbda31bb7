// best_reduce.hpp -- the cross-env reduction of the best log (dcm_reduce_best): every group of `group` consecutive envs gives its
// winner -- the env whose kept episode is the best of the group -- with the winner's summary row, ordinal, lengths and routes in
// compact [G, ...] buffers, G = ceil(B / group).  N instances x K envs each in one handle: group = K, N plans out, and only those
// leave the device.
// Included by dcmrta_env.hip inside its anonymous namespace, next to instgen.hpp's utility kernels; launched by the host API only, so
// the device-only translation units (-DDCM_TU_*) do not emit it.
//
// Order of two envs of a group (the order of keep_best in rollout_best.hpp, completed by the env index): more finished tasks
// (best_summary column 1); then the larger reward (column 0); then the LOWER env index.  Compared as the fp64 values they are: 0.0 and
// -0.0 tie.  An env that keeps no episode (best_episode == -1) is no candidate.  The index is part of the key in every combining
// step, so the order is total over the candidates, every combining step is associative and commutative, and the winner is the first
// candidate a sequential scan in env order under keep_best's strict replace rule would keep -- whatever the shape of the tree.
// NaN: the best log's contract is that a kept row holds the eight values of a finished episode, none of them NaN (only rows of envs
// that keep nothing are NaN, and those are no candidates).  No order is defined for a NaN key.
#pragma once

struct BestKey {
    double n, r;   // finished tasks, reward
    int b;         // env index; BEST_NONE: no candidate
};
constexpr int BEST_NONE = 0x7FFFFFFF;
constexpr int BEST_REDUCE_MAX_WAVES = 16;   // a block of at most 1024 threads
#define BEST_NAN __longlong_as_double(0x7FF8000000000000ll)   // the summary row of a group without a candidate: the quiet NaN of numpy / torch

// does x come before y?
__device__ __forceinline__ bool best_before(BestKey x, BestKey y) {
    if (x.b == BEST_NONE) return false;
    if (y.b == BEST_NONE) return true;
    return x.n > y.n || (x.n == y.n && (x.r > y.r || (x.r == y.r && x.b < y.b)));
}
// (selected field by field: a select between two structs would be one between their addresses, i.e. a stack object)
__device__ __forceinline__ BestKey best_of(BestKey x, BestKey y) {
    const bool take = best_before(y, x);
    return BestKey{take ? y.n : x.n, take ? y.r : x.r, take ? y.b : x.b};
}
// butterfly over the lanes l ^ 1, l ^ 2, ... l ^ (W / 2): every lane of an aligned run of W lanes ends with the run's first key
template <int W>
__device__ __forceinline__ BestKey best_butterfly(BestKey k) {
#pragma unroll
    for (int s = W / 2; s >= 1; s >>= 1) {
        BestKey o;
        o.n = __shfl_xor(k.n, s); o.r = __shfl_xor(k.r, s); o.b = __shfl_xor(k.b, s);
        k = best_of(k, o);
    }
    return k;
}

// grid = G workgroups, block = min(1024, group rounded up to a multiple of 64) threads (the host's choice: a multiple of 64, <= 1024).
// win_summary / win_episode may be null on their own; win_len / win_task / win_arrival are null together.  A: the batch dimension of
// the best log's rows, cap: their entries per agent.  Writes the win_* buffers only, with plain stores.
__global__ __launch_bounds__(1024) void k_reduce_best(int B, int group, int A, int cap, const int16_t* __restrict__ best_task,
                                                      const double* __restrict__ best_arrival, const int32_t* __restrict__ best_len,
                                                      const double* __restrict__ best_summary, const int32_t* __restrict__ best_episode,
                                                      int32_t* __restrict__ win_env, double* __restrict__ win_summary,
                                                      int32_t* __restrict__ win_episode, int32_t* __restrict__ win_len,
                                                      int16_t* __restrict__ win_task, double* __restrict__ win_arrival) {
    __shared__ double s_n[BEST_REDUCE_MAX_WAVES], s_r[BEST_REDUCE_MAX_WAVES];
    __shared__ int s_b[BEST_REDUCE_MAX_WAVES];
    const int g = blockIdx.x, tid = threadIdx.x, lane = tid & (WAVE - 1);
    const int wave = uni(tid / WAVE), n_waves = (int)(blockDim.x / WAVE);
    // ---- phase 1: the group's first key.  (lo + group in 64 bits: it may pass 2^31 where the last group is short)
    const int64_t lo = (int64_t)g * group;
    const int hi = (int)(lo + group < (int64_t)B ? lo + group : (int64_t)B);
    BestKey k{0.0, 0.0, BEST_NONE};
    for (int b = (int)lo + tid; b < hi; b += (int)blockDim.x) {                  // ascending b: a later env must beat, not tie
        if (best_episode[b] == -1) continue;
        const BestKey c{best_summary[(size_t)b * 8 + 1], best_summary[(size_t)b * 8], b};
        k = best_of(k, c);
    }
    k = best_butterfly<WAVE>(k);
    if (lane == 0) { s_n[wave] = k.n; s_r[wave] = k.r; s_b[wave] = k.b; }
    __syncthreads();
    // every wave combines the waves' keys itself (lane l takes wave l mod 16's): the winner is block-uniform without a second barrier
    const int src = lane & (BEST_REDUCE_MAX_WAVES - 1);
    BestKey f{0.0, 0.0, BEST_NONE};
    if (src < n_waves) f = BestKey{s_n[src], s_r[src], s_b[src]};
    f = best_butterfly<BEST_REDUCE_MAX_WAVES>(f);
    const int fb = uni(f.b);
    const bool any = fb != BEST_NONE;
    const int w = any ? fb : -1;                                                 // scalar from here on
    // ---- phase 2: the winner's rows
    if (tid < 8 && win_summary) win_summary[(size_t)g * 8 + tid] = any ? best_summary[(size_t)w * 8 + tid] : BEST_NAN;
    if (tid == 0) {
        win_env[g] = w;
        if (win_episode) win_episode[g] = any ? best_episode[w] : -1;
    }
    if (!win_len) return;
    const int32_t* const src_len = best_len + (size_t)(any ? w : 0) * A;        // (never read when !any)
    const int16_t* const src_task = best_task + (size_t)(any ? w : 0) * A * cap;
    const double* const src_arrival = best_arrival + (size_t)(any ? w : 0) * A * cap;
    for (int a = tid; a < A; a += (int)blockDim.x) win_len[(size_t)g * A + a] = any ? src_len[a] : 0;
    // element width: A * cap * 2 bytes per env is no multiple of 16 for odd A * cap, and the kernel moves A * cap * 10 bytes per GROUP
    const int n_entries = A * cap;
    int16_t* const dst_task = win_task + (size_t)g * n_entries;
    double* const dst_arrival = win_arrival + (size_t)g * n_entries;
    for (int i = tid; i < n_entries; i += (int)blockDim.x) {
        const int a = i / cap, j = i - a * cap;
        int16_t t = -2;                                                          // the buffers' initial fill behind the prefix
        double at = 0.0;
        if (any && j < src_len[a]) { t = src_task[i]; at = src_arrival[i]; }     // j < cap already: entries [0, min(len, cap))
        dst_task[i] = t;
        dst_arrival[i] = at;
    }
}
