// instgen.hpp -- problem instances made on the device: TaskEnv(agents_range, tasks_range, max_coalition_size, seed=s).generate_env
// (env/task_env.py:57-71) for a whole batch, one wavefront per env, from nothing but the seeds.  The stream is the one of
// np.random.default_rng(s), restated in np_stream.hpp; included by dcmrta_env.hip.
//
// Draw order of generate_env: the number of tasks when tasks_range has lo < hi (:59), the number of agents likewise (:63), depot
// random((1,2)) :67, cost random((A,1)) :68 (never used, but it advances the stream), task xy random((T,2)) :69 row-major,
// requirements integers(1, max_coalition_size + 1, T) :71; durations are the constant max_duration :70.
//
// The sizes come first and every later position depends on them, so the wave draws them in step (every lane the same, the values are
// wave-uniform).  After that a lane takes its own draws by jump-ahead: lane l starts l + 1 steps ahead of the stream's state, which
// is draw l, and strides by 64.  A double is one 64-bit draw.  A bounded integer takes a 32-bit HALF of one -- low half first, the high half is kept for the
// next integer, and doubles do not touch that buffer: when exactly one size was drawn the first requirement takes the half the
// size left behind -- and Lemire's method rejects a word now and then (at most 15 in 2^32 at max_coalition_size <= 16), which shifts
// every later position.  wave_bounded therefore takes 128 words at a time on the assumption that none is rejected, and when one
// is, the whole wave falls back to the sequential routine of np_stream.hpp from the start of that block on.
//
// Instance renewal (dcm_set_instance_renewal): the kernels that restart episodes -- the renewing forms (k_rn_*: see k_step.inc) of k_step, k_step_fast and
// the four persistent rollout kernels -- call wave_renew_instance right before reset_state, so that every episode runs on a fresh
// instance the way every reference Worker builds a fresh TaskEnv (worker.py:32).  The size-renewing forms (k_rs_*) of the
// instantiations that read per-env sizes call wave_renew_instance_sized instead: the env's sizes are drawn anew as well.
#pragma once   // (inside dcmrta_env.hip's unnamed namespace, in front of its kernels: np_stream.hpp is included at the top of that file)

// n doubles of Generator.random from the wave-uniform stream p: put(j, value) is called by the lane that owns draw j.
// lane_j = nps::jump_coeffs(lane + 1).  p is left behind the last of them.
template <class F>
__device__ __forceinline__ void wave_doubles(nps::Pcg& p, const nps::Jump& lane_j, int n, int lane, F&& put) {
    constexpr nps::Jump j64 = nps::jump_coeffs(WAVE);
    const nps::u128 a64 = j64.A, g64 = j64.G * p.inc;
    nps::u128 s = nps::jump(p.state, p.inc, lane_j);
    for (int j = lane; j < n; j += WAVE) {
        put(j, nps::to_double(nps::output(s)));
        s = a64 * s + g64;
    }
    p.state = nps::jump(p.state, p.inc, nps::jump_coeffs((uint64_t)n));
}

// n values of Generator.integers(0, rng + 1) (0 <= rng <= 2^32 - 2) from the wave-uniform stream p: put(i, value) is called by one
// lane per i.  p is left behind the last of them, half-word buffer included.
// A block is 128 words = the buffered half, if any, + up to 64 fresh draws; lane l always holds draw l of the block.  Only a full block
// (w == 128) is followed by another one, and a full block takes 64 draws whether or not a half was buffered (with one, the high half
// of lane 63 stays buffered for the next block).  A short block (draws < 64) can therefore only be the last one: the lanes' own
// `s = a64 * s + g64` at the end of the body, which assumes that 64 draws were taken, is then never read again.
template <class F>
__device__ __forceinline__ void wave_bounded(nps::Pcg& p, const nps::Jump& lane_j, uint32_t rng, int n, int lane, F&& put) {
    if (rng == 0) {                                                  // integers(lo, lo + 1): nothing is drawn
        for (int i = lane; i < n; i += WAVE) put(i, 0u);
        return;
    }
    constexpr nps::Jump j64 = nps::jump_coeffs(WAVE);
    const nps::u128 a64 = j64.A, g64 = j64.G * p.inc;
    const uint32_t threshold = nps::lemire_threshold(rng);
    nps::u128 s = nps::jump(p.state, p.inc, lane_j);
    int base = 0;
    for (; base < n; base += 2 * WAVE) {
        // lane l holds 64-bit draw l of this block; words of the block in stream order: [the buffered half,] lo(0), hi(0), lo(1), ...
        const uint64_t r = nps::output(s);
        const uint32_t lo = (uint32_t)r, hi = (uint32_t)(r >> 32);
        const uint32_t hi_below = (uint32_t)__shfl_up((int)hi, 1);
        const bool has = p.has_uint32 != 0;
        const uint32_t u0 = has ? (lane == 0 ? p.uinteger : hi_below) : lo, u1 = has ? lo : hi;
        uint32_t v0, v1;
        const bool ok0 = nps::lemire_accepts(u0, rng, threshold, v0), ok1 = nps::lemire_accepts(u1, rng, threshold, v1);
        const int i0 = base + 2 * lane, i1 = i0 + 1;
        if (__any((i0 < n && !ok0) || (i1 < n && !ok1))) break;      // a rejected word: every later position shifts
        if (i0 < n) put(i0, v0);
        if (i1 < n) put(i1, v1);
        // the stream behind the w words this block took
        const int w = (n - base < 2 * WAVE) ? n - base : 2 * WAVE;
        const int fresh = has ? w - 1 : w, draws = (fresh + 1) >> 1;
        p.has_uint32 = (uint32_t)(fresh & 1);
        if (fresh & 1) p.uinteger = rl(hi, uni(draws - 1));
        p.state = draws == WAVE ? a64 * p.state + g64 : nps::jump(p.state, p.inc, nps::jump_coeffs((uint64_t)draws));
        s = a64 * s + g64;
    }
    for (int i = base; i < n; i++) {                                 // the fall-back: in step, the routine numpy itself runs
        const uint32_t v = nps::bounded(p, rng);
        if (lane == (i & (WAVE - 1))) put(i, v);
    }
}

// generate_env for one env by one wave, written where k_load_instances puts it: the instance sections tx / ty / tdur, the
// requirement in tinfo, the depot and the initial fields of the header.  The pointers may be into a record in HBM or its LDS image.
// Rows beyond the env's own sizes are not touched.  (eA, eT) = the sizes it drew, wave-uniform.
// INSTANCE_ONLY: of the header only the depot is written -- the form for a LIVE header (wave_renew_instance), whose flags, episode
// count, decision counter and seed must survive.
template <bool INSTANCE_ONLY = false>
__device__ __forceinline__ void wave_generate_instance(uint64_t seed, const GenArgs& g, const nps::Jump& lane_j, int lane, Hdr* h,
                                                       double* tx, double* ty, double* td, uint32_t* ti, int& eA, int& eT) {
    nps::Pcg p = nps::pcg_seed(seed);
    eT = uni(g.t_lo + (int32_t)nps::bounded(p, (uint32_t)(g.t_hi - g.t_lo)));
    eA = uni(g.a_lo + (int32_t)nps::bounded(p, (uint32_t)(g.a_hi - g.a_lo)));
    const int nA = eA;
    wave_doubles(p, lane_j, 2 + eA + 2 * eT, lane, [&](int j, double v) {
        if (j == 0) h->depot_x = v;
        else if (j == 1) h->depot_y = v;
        else if (j >= 2 + nA) { const int k = j - 2 - nA; (k & 1 ? ty : tx)[k >> 1] = v; }
    });
    const double dur = g.max_duration;
    wave_bounded(p, lane_j, (uint32_t)(g.max_coalition_size - 1), eT, lane, [&](int t, uint32_t v) { ti[t] = 1u + v; td[t] = dur; });
    if constexpr (!INSTANCE_ONLY) {
        if (lane == 0) {
            h->flags = DCM_FLAG_DONE; h->episodes = 0; h->d = 0; h->seed = 0;
            h->groups = 0; h->reserved = 0; h->max_arrival = 0.0;
        }
    }
}

// Instance renewal at an episode restart: env e's instance n + 1 (n = Hdr::reserved of the live header, the env's instance index)
// replaces instance n, and the index moves on.  S.base is the kernel's LDS image with the live header, rec the env's HBM record.
// The image does not always hold the instance -- the exact multi-chunk shapes keep task x / y in the XY registers, the
// register-resident kernels hold x / y / duration per lane -- and a write-back of the mutable part alone must leave the record with
// the new instance.  So the instance goes straight into the record's instance sections and requirement words, the depot and the
// index into the live header, and then the wave reloads what the kernel keeps: the instance part of the image (requirement words,
// durations, x / y where the image has them) and xy.  The caller runs reset_state next -- it expands the requirement words and reads
// the depot -- and then reloads its own per-lane constants (load_consts).
// The wave re-reads its own global stores, made by other lanes than those that read: the loads are agent-scope (past the CU's vector
// L1, whose lines may date from the record copy at the head of the launch) and follow a release fence that waits for the stores,
// the order step_fast.hpp keeps for its abandonment rows.
// (renew_draw + renew_reload below are this body in two halves, for the size-renewing forms: a change here -- the release fence, the
//  agent-scope loads, their order -- has to be made there as well, by hand.)
template <class SimT>
__device__ __forceinline__ void wave_renew_instance(const SimT& S, unsigned char* rec, const Renew& rn, int e, int lane,
                                                    typename SimT::XY& xy) {
    const Lay L = S.L();
    Hdr* const live = (Hdr*)S.base;
    const uint32_t n = uni(live->reserved) + 1u;
    const uint64_t seed = uni(rn.seeds[e]) + (uint64_t)n * rn.stride;
    const nps::Jump lane_j = nps::jump_coeffs((uint64_t)lane + 1);
    unsigned long long* const gx = (unsigned long long*)(rec + L.tx());
    unsigned long long* const gy = (unsigned long long*)(rec + L.ty());
    unsigned long long* const gd = (unsigned long long*)(rec + L.tdur());
    uint32_t* const gi = (uint32_t*)(rec + L.tinfo());
    int eA, eT;                                                      // (the batch is uniform: the handle's dims)
    wave_generate_instance<true>(seed, rn.g, lane_j, lane, live, (double*)gx, (double*)gy, (double*)gd, gi, eA, eT);
    if (lane == 0) live->reserved = n;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    auto gload = [](const unsigned long long* q) {
        return __longlong_as_double((long long)__hip_atomic_load(q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    };
    S.for_tasks(lane, [&](int t) {
        S.tinfo()[t] = __hip_atomic_load(gi + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        S.tdur()[t] = gload(gd + t);
        if constexpr (!SimT::IRB) { S.tx()[t] = gload(gx + t); S.ty()[t] = gload(gy + t); }
    });
    if constexpr (SimT::IRB) {
#pragma unroll
        for (int c = 0; c < SimT::NTC; c++) {
            const int t = c * WAVE + lane < S.T() ? c * WAVE + lane : 0;
            xy.x[c] = gload(gx + t);
            xy.y[c] = gload(gy + t);
        }
    }
    WSYNC();
}

// The same out of line, for the persistent rollout kernels: it runs once per episode, and inlined its 128-bit multiplies cost their
// decision loops up to nineteen VGPRs (k_rn_rollout_random<20,50, runtime sizes>: 129, three waves per SIMD instead of four; the
// register-resident kernels spilled).  The lockstep kernels inline it: a callee's registers count as the caller's, and the general
// k_step, which runs seven waves per SIMD on 68 VGPRs, would run five.
template <class SimT>
__device__ __noinline__ void wave_renew_instance_call(const SimT& S, unsigned char* rec, const Renew& rn, int e, int lane,
                                                      typename SimT::XY& xy) {
    wave_renew_instance(S, rec, rn, e, lane, xy);
}

// The same in two halves, for the form that also renews the sizes and changes them in between: renew_draw makes the instance,
// renew_reload brings it into what the kernel keeps.  (wave_renew_instance above keeps its one-piece text: the k_rn_* forms must
// compile to what they compiled to before the size-renewing forms existed, and they do not when it is rebuilt from these two.)
template <class SimT>
__device__ __forceinline__ void renew_draw(const SimT& S, unsigned char* rec, const Renew& rn, int e, int lane, int& eA, int& eT) {
    const Lay L = S.L();
    Hdr* const live = (Hdr*)S.base;
    const uint32_t n = uni(live->reserved) + 1u;
    const uint64_t seed = uni(rn.seeds[e]) + (uint64_t)n * rn.stride;
    const nps::Jump lane_j = nps::jump_coeffs((uint64_t)lane + 1);
    wave_generate_instance<true>(seed, rn.g, lane_j, lane, live, (double*)(rec + L.tx()), (double*)(rec + L.ty()), (double*)(rec + L.tdur()),
                                 (uint32_t*)(rec + L.tinfo()), eA, eT);
    if (lane == 0) live->reserved = n;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
}
template <class SimT>
__device__ __forceinline__ void renew_reload(const SimT& S, unsigned char* rec, int lane, typename SimT::XY& xy) {
    const Lay L = S.L();
    const unsigned long long* const gx = (const unsigned long long*)(rec + L.tx());
    const unsigned long long* const gy = (const unsigned long long*)(rec + L.ty());
    const unsigned long long* const gd = (const unsigned long long*)(rec + L.tdur());
    const uint32_t* const gi = (const uint32_t*)(rec + L.tinfo());
    auto gload = [](const unsigned long long* q) {
        return __longlong_as_double((long long)__hip_atomic_load(q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    };
    S.for_tasks(lane, [&](int t) {
        S.tinfo()[t] = __hip_atomic_load(gi + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        S.tdur()[t] = gload(gd + t);
        if constexpr (!SimT::IRB) { S.tx()[t] = gload(gx + t); S.ty()[t] = gload(gy + t); }
    });
    if constexpr (SimT::IRB) {
#pragma unroll
        for (int c = 0; c < SimT::NTC; c++) {
            const int t = c * WAVE + lane < S.T() ? c * WAVE + lane : 0;
            xy.x[c] = gload(gx + t);
            xy.y[c] = gload(gy + t);
        }
    }
    WSYNC();
}
// Size renewal (DCM_PARAM_RENEW_SIZES, a ragged generated batch): the size-renewing kernel forms (k_rs_*: see k_step.inc).  rn.g
// carries the real ranges, so the draw gives the env's next sizes with its next instance -- eT first, then eA, then the instance,
// what k_generate_instances does for that seed -- and the env becomes an (eA, eT) env: lane 0 writes the sizes to the handle's
// size table (sizes[2e], sizes[2e + 1]: where every getter, dcm_observe and the next launch read them), and the instance is
// reloaded under the new sizes.  Returns them packed, eA | eT << 16 (wave-uniform; by value, so that the out-of-line form does
// not force the caller's simulator into memory): the CALLER puts them into every copy of the simulator it holds (Sim::rA / rT,
// the copy inside Fast / FastG) and re-derives what it derived from the old ones -- lane ownership (Fast::init), observation row
// pointers, the padding rows (write_pad_obs) -- before reset_state.
// The abandonment count table: its spill check and clear (Sim::clear_spilled_counts) run here, FIRST, with the finished
// episode's sizes -- reset_state, which runs under the new ones, would miss agents beyond the new A and would not clear the old
// a * T + t layout in full.  reset_state's own check then sees stale counters of the agents both episodes have and at most clears
// an already clean table again.
template <class SimT>
__device__ __forceinline__ uint32_t wave_renew_instance_sized(const SimT& S, unsigned char* rec, const Renew& rn, int32_t* sizes, int e,
                                                              int lane, typename SimT::XY& xy) {
    static_assert(!SimT::EXACT, "size renewal needs an instantiation that reads per-env sizes");
    S.clear_spilled_counts(lane);
    int eA, eT;
    renew_draw(S, rec, rn, e, lane, eA, eT);
    if (lane == 0) { sizes[2 * e] = eA; sizes[2 * e + 1] = eT; }
    SimT N = S;
    N.rA = eA; N.rT = eT;
    renew_reload(N, rec, lane, xy);
    return (uint32_t)eA | ((uint32_t)eT << 16);
}
template <class SimT>
__device__ __noinline__ uint32_t wave_renew_instance_sized_call(const SimT& S, unsigned char* rec, const Renew& rn, int32_t* sizes, int e,
                                                                int lane, typename SimT::XY& xy) {
    return wave_renew_instance_sized(S, rec, rn, sizes, e, lane, xy);
}
// ... and the caller's part for a plain simulator: S takes the sizes (wave-uniform, in SGPRs)
template <class SimT>
__device__ __forceinline__ void take_sizes(SimT& S, uint32_t packed) {
    packed = uni(packed);
    S.rA = (int)(packed & 0xFFFFu); S.rT = (int)(packed >> 16);
}

#if !defined(DCM_TU_G) && !defined(DCM_TU_P) && !defined(DCM_TU_L) && !defined(DCM_TU_E) && !defined(DCM_TU_B)   // (the units of k_rollout_fast_g, of the greedy-policy, the logging, the epsilon-greedy and the best-keeping forms need the routines above only)

// dcm_generate_instances: sizes = the handle's per-env sizes [B][2] on a ragged batch, else nullptr
__global__ __launch_bounds__(WAVE) void k_generate_instances(int PA, int PT, int PC, unsigned char* state, const uint64_t* seeds, GenArgs g,
                                                            int32_t* sizes) {
    const int e = blockIdx.x, lane = threadIdx.x;
    const Lay L{PA, PT, PC};
    unsigned char* rec = state + (size_t)e * L.rec_bytes();
    const nps::Jump lane_j = nps::jump_coeffs((uint64_t)lane + 1);
    int eA, eT;
    wave_generate_instance(seeds[e], g, lane_j, lane, (Hdr*)rec, (double*)(rec + L.tx()), (double*)(rec + L.ty()),
                           (double*)(rec + L.tdur()), (uint32_t*)(rec + L.tinfo()), eA, eT);
    if (sizes && lane == 0) { sizes[2 * e] = eA; sizes[2 * e + 1] = eT; }
}

// dcm_get_instances: the instance every record holds, in the batch shapes of dcm_load_instances; rows beyond an env's own sizes
// read xy 0, req 1, dur 0 (the padding of instances.generate_batch_ranges)
__global__ __launch_bounds__(WAVE) void k_get_instances(int A, int T, int PA, int PT, int PC, const unsigned char* state, const int32_t* sizes,
                                                       double* depot, double* task_xy, int32_t* req, double* dur, int32_t* n_agents,
                                                       int32_t* n_tasks) {
    const int e = blockIdx.x, lane = threadIdx.x;
    int eA, eT;
    env_dims<0, 0, false>(sizes, e, A, T, eA, eT);
    const Lay L{PA, PT, PC};
    const unsigned char* rec = state + (size_t)e * L.rec_bytes();
    const double *tx = (const double*)(rec + L.tx()), *ty = (const double*)(rec + L.ty()), *td = (const double*)(rec + L.tdur());
    const uint32_t* ti = (const uint32_t*)(rec + L.tinfo());
    for (int t = lane; t < T; t += WAVE) {
        const size_t o = (size_t)e * T + t;
        const bool in = t < eT;
        if (task_xy) { task_xy[2 * o] = in ? tx[t] : 0.0; task_xy[2 * o + 1] = in ? ty[t] : 0.0; }
        if (req) req[o] = in ? (int32_t)(ti[t] & 0xFFu) : 1;
        if (dur) dur[o] = in ? td[t] : 0.0;
    }
    if (lane == 0) {
        const Hdr* h = (const Hdr*)rec;
        if (depot) { depot[2 * (size_t)e] = h->depot_x; depot[2 * (size_t)e + 1] = h->depot_y; }
        if (n_agents) n_agents[e] = eA;
        if (n_tasks) n_tasks[e] = eT;
    }
}

// dcm_instance_index: Hdr::reserved of every env (layout dims: only the record pitch matters)
__global__ __launch_bounds__(WAVE) void k_instance_index(int PA, int PT, int PC, const unsigned char* state, int B, uint32_t* index_out) {
    const int e = blockIdx.x * WAVE + threadIdx.x;
    if (e >= B) return;
    const Lay L{PA, PT, PC};
    index_out[e] = ((const Hdr*)(state + (size_t)e * L.rec_bytes()))->reserved;
}

// dcm_generator_draws: per seed the first n_doubles of Generator.random, then n_ints of Generator.integers(0, rng + 1), through the
// routines the instance kernel uses
__global__ __launch_bounds__(WAVE) void k_generator_draws(const uint64_t* seeds, int n_doubles, uint32_t rng, int n_ints, double* doubles_out,
                                                         uint32_t* ints_out) {
    const int e = blockIdx.x, lane = threadIdx.x;
    const nps::Jump lane_j = nps::jump_coeffs((uint64_t)lane + 1);
    nps::Pcg p = nps::pcg_seed(seeds[e]);
    wave_doubles(p, lane_j, n_doubles, lane, [&](int j, double v) { doubles_out[(size_t)e * n_doubles + j] = v; });
    wave_bounded(p, lane_j, rng, n_ints, lane, [&](int i, uint32_t v) { ints_out[(size_t)e * n_ints + i] = v; });
}
#endif   // DCM_TU_G, DCM_TU_P, DCM_TU_L, DCM_TU_E, DCM_TU_B
