// rollout_fast.hpp -- the persistent rollout kernel of the ONE-CHUNK layouts (A <= 64, T <= 63: one lane per agent and per task):
// lane-owned state lives in REGISTERS for the whole fast path, LDS is only the cross-lane exchange.
// Included by dcmrta_env.hip inside its anonymous namespace, after Sim<>.
//
// Why: k_rollout_random keeps the record in LDS and re-reads every field in every phase of a decision -- ~60 LDS instructions in
// ~12 DEPENDENT round trips, each phase fenced from the next, and (round-3 profile) 0.39 of the wave time parked on s_waitcnt,
// 347 scalar + 89 branch instructions per decision, most of them the compiler's exec-mask bookkeeping around guarded lane loops
// and error returns.  With four waves per SIMD (4096 envs on 1024 SIMDs) the kernel is bound by ONE wave's critical path, so the
// cure is fewer dependent steps, not more parallelism:
//   * lane a owns agent a (x, y, arrival, next_decision, travel_dist, route[-1], flags), lane t owns task t (status word,
//     time_start, time_finish, ordered member ids, and the read-only x, y, duration); lane 63 owns the depot as a pseudo-task
//     (its observation row 0 and mask byte 0 leave in the same store instructions as the task rows);
//   * wave-uniform reads of a chosen lane's state (the leader's position, the chosen task's status word / ids / position) are
//     v_readlane -- no LDS round trip; per-lane reads of own state cost nothing;
//   * LDS carries only what another lane must read by INDEX: the member arrival slots f64[M][T] (written by the joining agents'
//     lanes, read by the task's lane), and the status words and the two time arrays (written through by the task lanes, gathered
//     by the agents' lanes in agent_update);
//   * member removal needs no scatter from a task's lane to its members: the task's lane compacts its own slots and publishes a
//     `gone` agent bitmask, and a wave-uniform pass over the dropping tasks lets each agent's lane take its own abandonment
//     (v_readlane of the mask) -- the agents' counters and flags never leave their registers;
//   * the lane code is select-based (no per-lane branches except the member-removal compaction), error returns do not exist on
//     this path (the device policy only takes valid actions on a validated instance), the observation pointers are a template
//     parameter, and every loop / branch condition is wave-uniform in SGPRs.
// Everything that happens once per episode or less -- reset, the terminal metrics, events at which nobody can decide, the first
// event of an episode -- runs the verified Sim<> code on the LDS image: the fast path flushes its registers, calls it, reloads.
//
// Round 6 (profiles/r06_budget.md): the kernel is bound by the length of ONE wave's instruction stream (a lone wave needs 0.78 ms of
// the 1.24 ms a 4096-env launch takes), so the stream itself was cut: the choice-protocol keys of 64 decisions are computed one per
// lane; decide() has no exit in its middle (an exit there keeps a second copy of all 15 lane-owned fields alive: 15 v_mov per
// decision); task_update touches the latest arrival / time_start only when a coalition is complete / a task becomes feasible.
//
// Reference restated: worker.py:45-87 (loop), env/task_env.py:161-342 (the functions named at each block below).
#pragma once
#include <type_traits>

// The rollout log of the logging kernel forms (dcm_set_rollout_log; k_lg_rollout_fast / k_lgrn_rollout_fast): the env's rows of
// route_task / route_arrival as wave-uniform bases, and agent a's running length in lane a's register.  Only Fast<>::apply<true> touches
// it, which only those forms instantiate.
struct FastLog {
    int16_t* task;    // the env's [A][cap] block
    double* arrival;
    int32_t cap;
    int32_t len;      // lane-owned: entries appended to this lane's agent in the env's current episode (may exceed cap)
};

// The second keys of the persistent kernels' decisions live one per lane beside the first ones (k_rollout_fast.inc: kv2, ki).  Only a
// decision with follower draws needs its own, so apply() fetches it (two v_readlane) inside that branch and not at the loop's top.
struct Key2 {
    uint64_t kv2;     // lane-owned: the second key of the decision whose first key this lane holds
    int ki;           // wave-uniform: the lane of the current decision
};

// TRK (lockstep kernel): the fast path records which task sections of the record it has changed (Sim::DIRTY_* bits), so that
// the write-back can skip the others
template <int CA, int CT, bool RS, bool OBS, bool TRK = false>
struct Fast {
    using SimT = Sim<CA, CT, RS, false>;
    using AMask = typename SimT::AMask;
    static_assert(CA >= 1 && CA <= 64 && CT >= 1 && CT <= 64, "one lane per agent / task; lane 63 is the depot's (the host dispatches T <= 63 only)");
    static constexpr int DL = 63;                     // depot lane
    static constexpr Lay L{CA, CT};

    SimT S;
    uint4* rtab;                                       // the removal path's compaction table (removal_table.hpp): 32 x 16 bytes of LDS
    mutable uint32_t dirty = 0;                        // TRK only
    mutable uint64_t achg = ~0ull;                     // TRK only: the agents whose fields the step has changed (set by flush)
    mutable uint64_t dt_join = 0, dt_times = 0;        // TRK only: the tasks whose ids / arrival rows (a join) and time_start / time_finish
                                                       // (became feasible) the fast path has changed: the write-back sends their 64-byte
                                                       // pieces of those sections instead of the sections
    mutable uint64_t unsettled = ~0ull;                // 0: the last task_update call left every task at a fixed point for its `now` ("calm");
                                                       // a mask tested where it is used, not a bool (common.hpp, the rule of the uniform conditions)
    FPH_MEMBERS;
    uint64_t am, tm;                                   // lanes that own an agent / a task (wave-uniform masks)
    // per-lane constants
    bool inA, inT, isD;
    int la, lt;                                        // clamped own agent / task index (0 for the lanes that own none)

    struct R {
        double ax, ay, arr, nd, td;                    // agent: location, arrival_time[-1], next_decision, travel_dist
        int32_t cur; uint32_t ai;                      //        route[-1], ainfo word
        double cts, cdur;                              //        time_start / duration of route[-1] as of the last agent_update
        uint32_t ti; double ts, tf; uint64_t ids;      // task:  tinfo word, time_start, time_finish, ordered member ids
        uint64_t lm; uint32_t nab;                     //        the listed members as an agent bitmask; len(abandoned_agent)
        double tx, ty, dur;                            //        instance (depot lane: depot x, y, 0)
        uint16_t* ab;                                  // agent: its row of the abandonment log (HBM side table)
    };

    __device__ __forceinline__ void init(int lane) {
        const int A_ = S.A(), T_ = S.T();
        am = A_ >= 64 ? ~0ull : ((1ull << A_) - 1ull);
        tm = (1ull << T_) - 1ull;
        // (a constant mask that is ANDed more than once is an SGPR pair: folded as a literal, `ballot & tm` is s_and_b32 of the high
        //  half and a copy of the low one)
        asm("" : "+s"(tm));
        inA = lane < A_; inT = lane < T_; isD = lane == DL;
        la = inA ? lane : 0; lt = inT ? lane : 0;
    }
    // Once per kernel, behind init: lanes 0..31 write one entry each of the compaction table (computed, not loaded).  A leaver's
    // arrival goes to "slot 5" of its task, which is the task's own word of the id section behind the five arrival rows: the fast
    // path keeps the ids in r.ids and nobody reads that word before flush() has rewritten it.
    static_assert(M == RT_SLOTS && L.mids() == L.marr() + 8u * RT_SLOTS * CT && L.mids() + 8u * CT <= L.tinfo(),
                  "slot 5 of task t is the id word of task t");
    __device__ __forceinline__ void build_removal_table(int lane) const {
        const RemovalEntry e = removal_entry((uint32_t)lane & (RT_ENTRIES - 1u), 8u * CT);
        if (lane < (int)RT_ENTRIES) rtab[lane] = make_uint4(e.perm, e.off01, e.off23, e.off4_left);
        WSYNC();
    }

    // ------------------------------------------------------------------------------ registers <-> LDS image
    __device__ __forceinline__ void load_consts(R& r) const {
        r.tx = isD ? ((const Hdr*)S.base)->depot_x : S.tx()[lt];
        r.ty = isD ? ((const Hdr*)S.base)->depot_y : S.ty()[lt];
        r.dur = isD ? 0.0 : S.tdur()[lt];
        r.ab = S.ablog() + la * AB_CAP;
    }
    __device__ __forceinline__ void reload(R& r) const {
        unsettled = ~0ull;                             // nothing is known about the general code's last call
        r.ax = S.ax()[la]; r.ay = S.ay()[la]; r.arr = S.arr()[la]; r.nd = S.nd()[la]; r.td = S.tdist()[la];
        r.cur = S.cur()[la]; r.ai = S.ainfo()[la];
        const int K = r.cur < 0 ? 0 : r.cur;
        r.cts = S.ts()[K]; r.cdur = S.tdur()[K];
        r.ti = S.tinfo()[lt]; r.ts = S.ts()[lt]; r.tf = S.tf()[lt]; r.ids = S.mids()[lt]; r.nab = S.tnab()[lt];
        r.lm = 0ull;
        const int n = (r.ti >> 16) & 0xFF;
#pragma unroll
        for (int j = 0; j < M; j++) r.lm |= (j < n) ? (1ull << ((r.ids >> (8 * j)) & 0xFF)) : 0ull;
    }
    // what the fast path keeps in registers only (everything else is written through when it changes)
    __device__ __forceinline__ void flush(const R& r) const {
        if constexpr (TRK) { if (gridDim.x >= 8192u) {
            // which agents differ from the image the record was loaded into (bit patterns: next_decision may be NaN)?  The
            // write-back sends only their 16-byte pieces of the agent arrays -- for grids that fill the machine several times over,
            // where HBM traffic is what the launch costs (a single round of workgroups is latency-bound: the compare would only add
            // to the chain, 15.4 vs 15.2 us at 4096 envs).
            auto ne = [](double a, double b) { return __double_as_longlong(a) != __double_as_longlong(b); };
            const int ch_ = (int)ne(r.ax, S.ax()[la]) | (int)ne(r.ay, S.ay()[la]) | (int)ne(r.arr, S.arr()[la]) | (int)ne(r.nd, S.nd()[la]) |
                            (int)ne(r.td, S.tdist()[la]) | (int)(r.cur != S.cur()[la]) | (int)(r.ai != S.ainfo()[la]);
            achg = __ballot(ch_ != 0) & am;
        } }
        if (inA) {
            S.ax()[la] = r.ax; S.ay()[la] = r.ay; S.arr()[la] = r.arr; S.nd()[la] = r.nd; S.tdist()[la] = r.td;
            S.cur()[la] = r.cur; S.ainfo()[la] = r.ai;
        }
        if (inT) { S.mids()[lt] = r.ids; S.tnab()[lt] = r.nab; }
        WSYNC();
    }

    // ------------------------------------------------------------------------------ task_update, env/task_env.py:245-281
    // One lane per task, inputs from the lane's registers + the member arrival slots in LDS.  Returns with tinfo / time_start /
    // time_finish written through for agent_update's gather.
    // (site: which call this is -- path counters of the developer builds only)
    __device__ __forceinline__ void task_update(R& r, double now, double mwt, int lane, int site = 0) const {
        uint32_t info = r.ti;
        const bool feas0 = info & T_FEAS;
        const int req = info & 0xFF, n = (info >> 16) & 0xFF;                    // :250
        double av[M];
#pragma unroll
        for (int j = 0; j < M; j++) av[j] = S.marr()[j * CT + lt];               // :251 (unused slots hold NaN)
        const double tfin = r.tf, dur = r.dur;
        const int status = req - n;                                              // :252
        // The latest arrival only matters for a task whose coalition is complete (status <= 0 :254): the spread test, time_start and
        // the spread rule's threshold (:255-265).  Such a task exists at the one call after the completing join (or while a stale
        // status lingers, Q3); every other call -- wave-uniform test -- skips the four v_max_f64 and the tests that need them.
        static_assert(M == 5, "nanmin5 / nanmax5");
        const double mn = nanmin5(av[0], av[1], av[2], av[3], av[4]);
        const bool le0 = status <= 0;                                            // :254
        // The predicates live as wave-uniform masks (common.hpp, lane_of): every ballot is one direct compare, the combinations are
        // scalar.  The lanes that own no task hold a copy of task 0's words (lt is clamped): whatever decides anything passes through
        // tm -- `open` -- exactly where inT stood.
        const uint64_t nfm = __ballot((info & T_FEAS) == 0u);                    // !feas0
        const uint64_t open = nfm & tm;                                          // the tasks without a feasible assignment
        const uint64_t le0m = __ballot(status <= 0);
        double mx = 0.0, thr = 0.0;
        uint64_t okm = 0ull, sdrop = 0ull;
        if (open & le0m) {
            mx = nanmax5(av[0], av[1], av[2], av[3], av[4]);
            okm = le0m & __ballot(mx - mn <= mwt);                               // :255
            thr = mx - mwt;                                                      // :262
            sdrop = open & le0m & ~okm & __ballot(mn <= thr);                    // the spread rule's leavers (none without such a task)
        }
        const bool ok = lane_of(okm);
        // does any member leave?  (see Sim::task_update: decided on the earliest arrival alone)
        const uint64_t wdrop = open & ~le0m & __ballot(now - mn >= mwt);         // the waiting rule's
        const uint64_t dmask = sdrop | wdrop;
        const bool becomes = lane_of(nfm & okm);                                 // :256-258
        // time_start / time_finish change -- and are written through for agent_update's gather -- only when a task becomes feasible
        // (:256-257): wave-uniform test
        const uint64_t bec = open & okm;
        double nts = r.ts, ntf = tfin;
        if (bec) { nts = becomes ? mx : nts; ntf = becomes ? mx + dur : ntf; }
        int nn = n;
        if (dmask) {
            CNT(6 + site);
            FPM(20);
            // Members leave (:262-265 spread branch, :268-271 waiting branch with its remove-while-iterating skip, Q1).  The
            // task's lane compacts its own slots; the agents' lanes then take their abandonment from the task's `gone` mask --
            // no scatter through LDS: an agent's counters live in its own lane.
            uint64_t gone = 0ull;
            // (which of the two removal rules is in play is wave-uniform almost always -- the spread rule fires ~3 times per
            //  episode -- so the per-slot tests of the other one are skipped by a scalar branch)
            const bool any_spread = sdrop != 0ull, any_wait = wdrop != 0ull;
            uint32_t spread = 0, q1 = 0;
            if (any_spread) {
#pragma unroll
                for (int j = 0; j < M; j++) spread |= (av[j] <= thr) ? (1u << j) : 0u;       // :262-265
            }
            if (any_wait) {
                bool prev = false;
#pragma unroll
                for (int j = 0; j < M; j++) {
                    const bool e = !prev && (now - av[j] >= mwt);                // :269, skipping the element after a removal (Q1)
                    q1 |= e ? (1u << j) : 0u;
                    prev = e;
                }
            }
            if (lane_of(dmask)) {
                const uint32_t drop = le0 ? spread : q1;                         // only listed slots can be set: unused ones hold NaN
                const uint32_t keep = ((1u << n) - 1u) & ~drop;
                // Compact the survivors in order, without a branch and without per-slot arithmetic: where every slot goes, the new
                // id word and the new length are functions of `keep` alone and come from the workgroup's 32-entry table
                // (removal_table.hpp) in one 128-bit LDS read, issued ahead of the writes that vacate the slots, which hide its
                // latency.  Then all five arrivals are written: a survivor to its rank among the survivors (a target never lies
                // above its source, and the values are in registers anyway), a leaver to "slot 5", the task's own word of the id
                // section, which is stale on the fast path and rewritten by flush().  One v_perm_b32 makes the id word (at least
                // one listed member leaves, so at most four survive: the low word).  The 512 bytes of the table are the former
                // per-lane dummy slots of the leavers' writes: the launch's LDS is unchanged.  Measured (profiles/HISTORY.md, last
                // section): the removal region of k_rollout_fast<20,50> 116 -> 78 static VALU (the per-slot rank / target / id /
                // select arithmetic was ~70 of them, now five SDWA adds, a permute and the `gone` shifts), 285.0 -> 264.0 VALU per
                // decision, product line +4.0 %.  (Writing each slot straight to its final place -- survivors to their rank,
                // leavers as NaN behind them: five writes instead of ten -- was tried in round 6 with computed targets: +20 VALU
                // for the target and value selects, not faster.)
                const uint4 e = rtab[keep];
                const uint32_t idl = (uint32_t)r.ids, idh = (uint32_t)(r.ids >> 32);
                using gone_t = typename std::conditional<(CA <= 32), uint32_t, uint64_t>::type;   // agent ids below 32: one word
                gone_t g = 0;
                double* const row0 = S.marr() + lt;
#pragma unroll
                for (int j = 0; j < M; j++) row0[j * CT] = __builtin_nan("");
                const uint32_t off[M] = {e.y & 0xFFFFu, e.y >> 16, e.z & 0xFFFFu, e.z >> 16, e.w & 0xFFFFu};
#pragma unroll
                for (int j = 0; j < M; j++) {
                    const uint32_t id = (j < 4 ? (idl >> (8 * j)) : idh) & 0xFFu;
                    g |= (gone_t)((drop >> j) & 1u) << id;
                    *(double*)((unsigned char*)row0 + off[j]) = av[j];
                }
                gone = (uint64_t)g;
                r.ids = (uint64_t)__builtin_amdgcn_perm(idh, idl, e.x);
                r.lm &= ~gone;
                nn = (int)(e.w >> 16);
                r.nab += (uint32_t)(n - nn);                                     // abandoned_agent.append :265/:271
            }
            if constexpr (TRK) dirty |= SimT::DIRTY_ALL & ~SimT::DIRTY_TIMES;   // slots compacted: every arrival row, ids, counts
            uint64_t todo = dmask;
            do {
                CNT(7);
                const int t = __ffsll((unsigned long long)todo) - 1;
                todo &= todo - 1ull;
                const uint64_t g = rl(gone, t);
                // the dropped agents whose log still has room: the count (bits 16-31 of ainfo) below AB_CAP, one compare of the word
                const uint64_t room = g & __ballot(r.ai < ((uint32_t)AB_CAP << 16));
                const uint32_t nth_ = r.ai >> 16;
                // (Both side tables live in HBM.  The LDS image keeps generic pointers to them, so the compiler emitted FLAT
                //  instructions, which count on lgkmcnt as well as vmcnt: the next lgkmcnt(0) also waited for this store.  With
                //  the cast to the global address space they are global_store_short / global_atomic_add.)
                // The store is the one arm under the lanes' own predicate; an agent past AB_CAP abandonments in one episode is the rare
                // case and sits behind ONE wave-uniform test (as an if / else per lane the two arms cost every trip two exec saves, an
                // exec flip, two branches and the load of the count table's pointer).
                if (lane_of(room)) ((__attribute__((address_space(1))) uint16_t*)r.ab)[nth_] = (uint16_t)t;
                const uint64_t over = g & ~room;
                if (over) {
                    if (lane_of(over)) {
                        const uint32_t ci = (uint32_t)(la * S.T() + t);
                        __hip_atomic_fetch_add((__attribute__((address_space(1))) uint32_t*)S.abcnt() + (ci >> 1), 1u << (16 * (ci & 1)),
                                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    }
                }
                if (lane_of(g)) {                                                // this lane's agent was dropped by task t
                    r.ai += 1u << 16;
                    if (r.cur == t) r.ai &= ~A_MEMBER;                           // no longer `agent in current_task['members']` :230
                }
            } while (todo);
            FPM(21);
        }
        const uint32_t info_i = ((info | (ok ? T_FEAS : 0u)) & (T_FEAS | T_FIN | 0xFFu)) | ((uint32_t)(status & 0xFF) << 8) | ((uint32_t)nn << 16);
        const uint32_t info_f = info | ((now >= tfin) ? T_FIN : 0u);             // :273-274
        info = feas0 ? info_f : info_i;
        r.ti = info;
        // (The guard stays.  Tried: the lanes that own no task write through a pointer of their own to a dead word, task 0's id word --
        //  the loop 4 instructions shorter, but the pointer is a second address register beside 4 * lt, which reload() keeps: 108 VGPRs
        //  for 106.  And time_start / time_finish below leave in ONE ds_write2_b64 off ONE address register, 8 CT bytes apart, while
        //  the id section is 8 CT bytes long: no two dead words lie that far apart.  profiles/HISTORY.md, last section.)
        if (inT) S.tinfo()[lt] = info;
        uint64_t over_already = 0ull;                                            // the tasks that became feasible and are over at `now`
        if (bec) {
            r.ts = nts; r.tf = ntf;
            if (inT) { S.ts()[lt] = nts; S.tf()[lt] = ntf; }
            if constexpr (TRK) { dirty |= SimT::DIRTY_TIMES; dt_times |= bec; }
            over_already = bec & __ballot(now >= ntf);
        }
        const bool all_feasible = (__ballot((info & T_FEAS) == 0u) & tm) == 0ull;
        // (see Sim::task_update: a call can only change a task again at the same `now` if this one removed members or made a task
        //  feasible that is already over)
        // (one test of one mask, selected into a 0/1 word where it is formed: a bool here is a lane mask from call to call)
        unsettled = dmask | over_already;
        WSYNC();
        if (all_feasible) {                                                      // depot :277-280
            CNT(16);
            if ((r.ai & A_INDEPOT) && now >= r.arr) r.ai |= A_RETURNED;
        }
    }

    // ------------------------------------------------------------------------------ agent_update, env/task_env.py:207-243
    __device__ __forceinline__ void agent_update(R& r, double now, double mwt) const {
        const int c = r.cur;
        const int K = c < 0 ? 0 : c;
        const uint32_t gi = S.tinfo()[K];                                        // :228
        const double gts = S.ts()[K], gtf = S.tf()[K], gdur = S.tdur()[K];
        const bool member = (gi & T_FEAS) && (r.ai & A_MEMBER);                  // :229-230
        const double ndv = (c == -1) ? __builtin_nan("") : (member ? gtf : r.arr + mwt);   // :226,:231,:235,:238
        const uint32_t as = member ? ((r.ai & A_ASSIGNED) | ((now >= gts) ? A_ASSIGNED : 0u)) : 0u;   // :232-240
        r.nd = (c != -2) ? ndv : r.nd;                                           // :209
        r.ai = (c >= 0) ? ((r.ai & ~A_ASSIGNED) | as) : r.ai;                    // depot leaves `assigned` untouched (Q6)
        r.cts = gts; r.cdur = gdur;
    }

    // ------------------------------------------------------------------------------ observation, worker.py:57-68
    // env/task_env.py:165-200 relative to the leader; rows straight into the policy's input tensors.  Returns the ballot of the
    // unmasked tasks (the random policy picks from it).
    __device__ __forceinline__ uint64_t observe(const R& r, double now, int leader, float* __restrict__ agrow, float* __restrict__ tkrow,
                                                uint8_t* __restrict__ mkp) const {
        const double lx = rl(r.ax, leader), ly = rl(r.ay, leader);
        if constexpr (OBS) {
            const bool on = r.cur >= 0;                                          // :168
            const double x = r.arr - now, w = now - r.arr, rem = r.cts + r.cdur - now;
            const double travel = (on && x > 0.) ? x : 0.;                       // :169
            const double waiting = (on && now <= r.cts && w > 0.) ? w : 0.;      // :170
            const double remaining = (on && now >= r.cts && rem > 0.) ? rem : 0.;   // :171
            const float f0 = (float)travel, f1 = (float)remaining, f2 = (float)waiting;
            const float f3 = (float)(lx - r.ax), f4 = (float)(ly - r.ay), f5 = (r.ai & A_ASSIGNED) ? 1.f : 0.f;
            if (inA) { agrow[0] = f0; agrow[1] = f1; agrow[2] = f2; agrow[3] = f3; agrow[4] = f4; agrow[5] = f5; }   // :176-177
        }
        const uint32_t info = isD ? 0u : r.ti;
        const int status = (int)(int8_t)((info >> 8) & 0xFF);
        const uint64_t bm = __ballot((info & T_FEAS) == 0u) & __ballot(status > 0) & tm;   // unfinished :199
        if constexpr (OBS) {
            // :193 per task; the depot's byte is False iff every task is masked (worker.py:58-61): the depot lane's bit of bm is
            // never set (T <= 63), it stands in for `every task is masked`
            const bool zero = lane_of(bm | (bm == 0ull ? 1ull << DL : 0ull));
            const uint8_t mv = zero ? 0 : 1;
            const float g0 = (float)status, g1 = (float)(info & 0xFF), g2 = (float)r.dur;
            const float g3 = (float)(r.tx - lx), g4 = (float)(r.ty - ly);        // :185-188
            if (inT || isD) { *mkp = mv; tkrow[0] = g0; tkrow[1] = g1; tkrow[2] = g2; tkrow[3] = g3; tkrow[4] = g4; }
        }
        return bm;
    }

    // ------------------------------------------------------------------------------ one decision
    // worker.py:54-76: leader, observation, uniform-random valid action, TaskEnv.step + agent_step (env/task_env.py:300-342),
    // task_update, agent_update.  Returns the number of agents of the group that have not acted yet.
    // worker.py:54 -- the deciding agent of the current group (protocol slot 0); -1: the group is empty (unreachable)
    __device__ __forceinline__ int pick_leader(const R& r, const HdrRegs& h, uint64_t k1, uint64_t& gm) const {
        gm = __ballot((int)((r.ai >> 8) & 0xFFu) == h.cur_group) & am;
        const int glen = __popcll(gm);
        if (glen == 0) return -1;
        return nth(gm, below((uint32_t)(k1 >> 32), glen));
    }
    // The same for the decisions of the persistent kernels, which have no exit in their middle (see decide): an empty group flags the
    // env DCM_FLAG_BAD_LEADER | DCM_FLAG_DONE and goes on with leader 0 and group mask 1.  The group's length is a number on the
    // scalar unit and the fix-up is arithmetic on it (common.hpp, the rule of the uniform conditions) -- `bad` is all ones iff the
    // length is 0, its low bit is the mask's bit 0 and the length 1 (nth(1, 0) = 0 is the leader by itself), its flag bits the flags:
    // no compare, no select, no lane mask.  (The opaque copy keeps the compiler from turning `bad` back into `glen == 0`, which it
    // holds as a lane mask across the observation to the place where the flags are merged.)
    __device__ __forceinline__ int pick_leader_flagged(const R& r, HdrRegs& h, uint64_t k1, uint64_t& gm) const {
        const uint64_t g = __ballot((int)((r.ai >> 8) & 0xFFu) == h.cur_group) & am;
        int glen = __popcll(g);
        asm("" : "+s"(glen));
        const uint32_t bad = (uint32_t)((glen - 1) >> 31);
        gm = g | (uint64_t)(bad & 1u);
        h.flags |= bad & (uint32_t)(DCM_FLAG_BAD_LEADER | DCM_FLAG_DONE);
        return nth(gm, below((uint32_t)(k1 >> 32), glen + (int)(bad & 1u)));
    }
    // k2p: where the decision's second key mix64(k1 + GAMMA) (the first two follower draws) is, if the caller has it, else nullptr
    // nvp: receives the number of unmasked tasks the decision saw (the launch's wave-priority estimate of the work left)
    __device__ __forceinline__ int decide(R& r, HdrRegs& h, const KP& P, int lane, uint64_t k1, float* agrow, float* tkrow, uint8_t* mkp,
                                          const Key2* k2p = nullptr, int* nvp = nullptr) const {
        uint64_t gm;
        // (no early return: an exit from the middle of a decision would keep the whole register set of the agent / task state alive
        //  in a second copy -- 15 v_mov per decision at the loop latch.  An empty group is unreachable; if it ever happened the env
        //  is flagged and stops at the loop's ordinary exit test, its state no longer meaningful.)
        const int leader = pick_leader_flagged(r, h, k1, gm);
        FPH(0);
        const uint64_t bm = observe(r, h.now, leader, agrow, tkrow, mkp);
        FPH(1);
        // uniform-random valid action (protocol slot 1)
        int nv = __popcll(bm);
        asm("" : "+s"(nv));                                                      // (tested as a number: not as observe()'s `bm == 0`, kept as a lane mask)
        if (nvp) *nvp = nv;
        // (the draw is made whether or not there is a task to draw -- nth() of an empty mask is harmless -- and the depot selected behind
        //  it: as `nv ? draw : 0` the draw sits in a branch of its own, whose condition waits as a lane mask across the task rows' stores)
        const int drawn = nth(bm, below((uint32_t)k1, nv)) + 1;
        const int action = nv ? drawn : 0;
        FPH(2);
        return apply(r, h, P, lane, k1, gm, leader, action, k2p);
    }
    // The same decision under a greedy device policy (dcm_rollout_policy, the k_hp_* kernel forms; `policy` wave-uniform): a
    // function of the ballot observe() returns, protocol slot 1 is not consumed.  FIRST: the lowest unmasked task.  NEAREST: every
    // task lane computes its own fp64 distance from the leader (dist2, agent first -- the routine agent_step travels by); the argmin
    // is the NaN-ignoring wave minimum of the ROUNDED distances (masked lanes hold NaN) and a ballot of the lanes equal to it, whose
    // lowest bit is the lowest task index: strict < in the oracle's policy_pick.  No unmasked task: the depot.
    __device__ __forceinline__ int decide_policy(R& r, HdrRegs& h, const KP& P, int lane, uint64_t k1, float* agrow, float* tkrow, uint8_t* mkp,
                                                 const Key2* k2p, int policy) const {
        uint64_t gm;
        const int leader = pick_leader_flagged(r, h, k1, gm);
        FPH(0);
        const uint64_t bm = observe(r, h.now, leader, agrow, tkrow, mkp);
        FPH(1);
        uint64_t pick = bm;
        if (policy == DCM_POLICY_NEAREST) {
            const double lx = rl(r.ax, leader), ly = rl(r.ay, leader);
            const double dd = dist2_inrange(lx, ly, r.tx, r.ty);
            const bool open = lane_of(bm);
            const double m = wave_nanmin_n<CT>(open ? dd : __builtin_nan(""));
            pick = bm & __ballot(dd == m);
        }
        const int action = __ffsll((unsigned long long)pick);                    // lowest set bit + 1 = the action; 0 = depot
        FPH(2);
        return apply(r, h, P, lane, k1, gm, leader, action, k2p);
    }
    // The same decision with the rollout log set (the k_lg_* kernel forms; `policy` wave-uniform, any of the three): the action is chosen
    // first -- decide()'s draw or decide_policy()'s pick -- and ONE apply follows, the logging one (a branch between decide and
    // decide_policy would inline apply twice into the loop).
    __device__ __forceinline__ int decide_logged(R& r, HdrRegs& h, const KP& P, int lane, uint64_t k1, float* agrow, float* tkrow, uint8_t* mkp,
                                                 const Key2* k2p, int policy, FastLog& lg) const {
        uint64_t gm;
        const int leader = pick_leader_flagged(r, h, k1, gm);
        FPH(0);
        const uint64_t bm = observe(r, h.now, leader, agrow, tkrow, mkp);
        FPH(1);
        // Both candidates are made -- the greedy pick behind its one wave-uniform branch (NEAREST), the random draw unconditionally as in
        // decide() -- and one scalar select on `policy` takes the action: as if / else arms the policy tests meet again as lane masks
        // where the arms join.
        int nv = __popcll(bm);
        asm("" : "+s"(nv));
        const int drawn = nth(bm, below((uint32_t)k1, nv)) + 1;
        uint64_t pick = bm;
        if (policy == DCM_POLICY_NEAREST) {
            const double lx = rl(r.ax, leader), ly = rl(r.ay, leader);
            const double dd = dist2_inrange(lx, ly, r.tx, r.ty);
            const bool open = lane_of(bm);
            const double m = wave_nanmin_n<CT>(open ? dd : __builtin_nan(""));
            pick = bm & __ballot(dd == m);
        }
        const int greedy = __ffsll((unsigned long long)pick);
        int pol = policy;
        asm("" : "+s"(pol));
        const int action = pol == DCM_POLICY_RANDOM ? (nv ? drawn : 0) : greedy;
        FPH(2);
        return apply<true>(r, h, P, lane, k1, gm, leader, action, k2p, &lg);
    }
    // TaskEnv.step :326-342 with the leader's (valid: unmasked task or depot) action, then task_update / agent_update
    // LOG (the k_lg_* kernel forms alone): every member lane appends (task id, arrival) to its agent's row of the rollout log
    template <bool LOG = false>
    __device__ __forceinline__ int apply(R& r, const HdrRegs& h, const KP& P, int lane, uint64_t k1, uint64_t gm, int leader, int action,
                                         const Key2* k2p = nullptr, FastLog* lg = nullptr) const {
        const double now = h.now;
        uint64_t rest = gm & ~(1ull << leader);                                  // :328
        int rlen = __popcll(gm) - 1;
        uint64_t mm = 1ull << leader, mlist = (uint64_t)(uint32_t)leader;
        int nm = 1;
        int mypos = 0;                                                           // this lane's position in the step's member list
        // `action - 1` pinned to the scalar unit: left alone the compiler fuses it with `action != 0` into ONE VALU subtract-with-borrow
        // (r.cur wants the difference in a VGPR) and fetches every uniform use of the target lane back by v_readfirstlane
        action = uni(action);                                                    // (the lockstep kernel's comes from a vector load; free here)
        int task = action - 1;                                                   // route[-1] of the members (-1: the depot)
        asm("" : "+s"(task));
        int act_ = action;                                                       // (an opaque copy for the `action != 0` tests)
        asm("" : "+s"(act_));
        // a task, not the depot?  A number on the scalar unit, compared where it is used: every test takes a fresh opaque copy, or the
        // compiler forms `act_ != 0` once and carries it from block to block as a lane mask (common.hpp, the rule of the uniform conditions)
        auto go = [&]() __attribute__((always_inline)) { int c = act_; asm("" : "+s"(c)); return c != 0; };
        static_assert(DL == 63, "task & DL");
        const int tl = task & DL;                                                // lane that owns the target: the task's, or (-1 & 63) the depot's
        // the target's status word, read ONCE for the vacancy and for the join below (nothing writes r.ti between the two; the depot
        // lane's word is read too and not used)
        const uint32_t tiw = (uint32_t)__builtin_amdgcn_readlane((int)r.ti, tl);
        if (!go()) {                                                               // vacancy = len(group) :327 (Q9)
            CNT(2);
            mm |= rest; nm += rlen; rlen = 0;
        } else if (rlen != 0) {
            const int vacancy = (int)(int8_t)((tiw >> 8) & 0xFF);                  // :327 (may be stale)
            const int nf = (vacancy > 1) ? ((vacancy - 1 < rlen) ? vacancy - 1 : rlen) : 0;   // :330-331
            uint64_t kk = k1;
            auto draw = [&](uint32_t rr) {
                CNT(1);
                FPM(22);
                const int f = nth(rest, below(rr, rlen));
                rest &= ~(1ull << f); rlen--;                                    // :332-333
                mm |= 1ull << f;
                mlist |= (uint64_t)(uint32_t)f << (8 * nm);
                // lane f takes its list position
                mypos = lane == f ? nm : mypos;
                nm++;
                FPM(23);
            };
            // :331 choice without replacement, two draws per trip: one key serves the draw from its high word and, if there is one,
            // the draw from its low word
            for (int j = 0; j < nf; j += 2) {
                kk = (j == 0 && k2p) ? rl(k2p->kv2, k2p->ki) : mix64(kk + GAMMA);
                draw((uint32_t)(kk >> 32));
                if (j + 1 < nf) draw((uint32_t)kk);
            }
        }
        FPH(3);
        const double tx_ = rl(r.tx, tl), ty_ = rl(r.ty, tl);
        // agent_step :300-324 on ALL lanes (fp64 VALU work with fewer than 16 active lanes is 4x slower on gfx950; the asm
        // statement keeps the compiler from sinking the chain into the members-only block below)
        double d = dist2_inrange(r.ax, r.ay, tx_, ty_);                          // (a handle with a smaller square never gets here: plan.hpp)
        double arrv = now + over_velocity(d);                                    // :315,:318
        asm volatile("" : "+v"(d), "+v"(arrv));
        FPH(4);
        const bool mem = lane_of(mm);
        uint64_t ids = 0ull; uint32_t kinfo = 0; int n = 0;
        int slot = 0;
        if (go()) {
            // :321-322 members.append unless already listed (Q4: a re-joining agent keeps its slot, its arrival is overwritten)
            kinfo = tiw;
            ids = rl(r.ids, tl);
            n = (kinfo >> 16) & 0xFF;
            slot = n + mypos;
            if constexpr (TRK) {
                dirty |= SimT::DIRTY_IDS | ((rl(r.lm, tl) & mm) ? SimT::DIRTY_ROWS : ((((1u << nm) - 1u) << (n + 1)) & SimT::DIRTY_ROWS));   // ids + the arrival rows written
                dt_join |= 1ull << tl;
            }
            if (rl(r.lm, tl) & mm) {
                CNT(3);
                // rare (Q4): walk the members in order as the reference does; every member's lane learns its own slot
                for (int j = 0; j < nm; j++) {
                    const int m = (int)((mlist >> (8 * j)) & 0xFF);
                    const uint64_t x = ids ^ (0x0101010101010101ull * (uint64_t)(uint32_t)m);
                    uint64_t z = (x - 0x0101010101010101ull) & ~x & 0x8080808080808080ull;
                    z &= (n >= 8) ? ~0ull : ((1ull << (8 * n)) - 1ull);
                    int pos;
                    if (z) pos = (__ffsll((unsigned long long)z) - 1) >> 3;
                    else { pos = n++; ids |= (uint64_t)(uint32_t)m << (8 * pos); }
                    if (lane == m) slot = pos;
                }
            } else {
                ids |= mlist << (8 * n);                                         // bytes above n are always zero
                n += nm;
            }
        }
        if (mem) {
            r.td += d;                                                           // :317
            r.arr = arrv;
            r.ax = tx_; r.ay = ty_;                                              // :320
            r.cur = task;                                                        // :314
            r.ai = (r.ai & ~(A_GRP | A_MEMBER)) | (go() ? A_MEMBER : A_INDEPOT);
            if constexpr (LOG) {
                // route.append / arrival_time += (:314,:318): one 16-bit and one 64-bit store behind the env's wave-uniform bases, at
                // the lane's 32-bit entry index; the length never leaves the lane's register
                const uint32_t o = (uint32_t)(la * lg->cap + lg->len);
                if (lg->len < lg->cap) {
                    *(int16_t*)((unsigned char*)lg->task + (o << 1)) = (int16_t)task;
                    *(double*)((unsigned char*)lg->arrival + (o << 3)) = arrv;
                }
                lg->len++;
            }
        }
        // (the members' arrival slots, under a mask of its own: as a uniform `if (go)` inside the members' block the compiler inverts
        //  the condition through a 0/1 VGPR)
        if (lane_of(go() ? mm : 0ull)) S.marr()[slot * CT + tl] = arrv;
        // A QUIET join: the task still lacks members after it (status = requirement - len(members) > 0) and the previous
        // task_update call -- at this same `now` -- left every task at a fixed point.  task_update (:245-281) then changes
        // nothing but this task's status: not enough members -> not feasible (:254); the joining members have not waited
        // (arrival >= now, :269); everybody else was evaluated at this `now` by the previous call.  The pass over the tasks is
        // skipped and the task's lane takes the new status itself.
        const int status_k = (int)(kinfo & 0xFFu) - n;
        // (the depot has status_k = 0; the target's lane is `task`, which is -1, no lane, for the depot: neither needs `go`)
        const uint64_t loud = status_k > 0 ? unsettled : ~0ull;                  // 0: quiet
        auto quiet = [&]() __attribute__((always_inline)) { uint64_t c = loud; asm("" : "+s"(c)); return c == 0ull; };
        if (lane == task) {
            r.ids = ids; r.lm |= mm;
            r.ti = quiet() ? ((kinfo & (T_FEAS | T_FIN | 0xFFu)) | ((uint32_t)(status_k & 0xFF) << 8) | ((uint32_t)n << 16))
                         : ((kinfo & ~0x00FF0000u) | ((uint32_t)n << 16));
            if (quiet()) S.tinfo()[lt] = r.ti;                                     // (written through like task_update does)
        }
        WSYNC();
        FPH(5);
        if (!quiet()) { CNT(5); task_update(r, now, P.mwt, lane); } else CNT(4);         // worker.py:74
        FPH(6);
        agent_update(r, now, P.mwt);                                                 // worker.py:76
        FPH(7);
        return rlen;
    }

    // ------------------------------------------------------------------------------ next event (common case)
    // Boxes D + A of the loop when somebody can decide and MAX_TIME has not passed: next_decision (env/task_env.py:283-289),
    // get_unique_group (:291-298), task_update, agent_update (worker.py:49-51).  Returns false -- with nothing changed -- when the
    // event needs the general code (nobody can decide: check_finished :366-373; or the loop test of worker.py:45 ends the episode).
    __device__ __forceinline__ bool next_event(R& r, HdrRegs& h, const KP& P, int lane) const {
        FPH(8);
        if (h.now >= P.max_time) return false;
        const double ndv = inA ? r.nd : __builtin_nan("");
        const double tmin = wave_nanmin_n<CA>(ndv);                              // :287
        if (!(tmin == tmin)) return false;
        CNT(10);
        h.now = tmin;                                                            // worker.py:49
        const bool dec = (ndv == tmin);                                          // :288 exact ==
        const uint64_t dm = __ballot(dec);
        const int first = __ffsll((unsigned long long)dm) - 1;
        uint64_t apart = 0ull;                                                   // the deciders that are not on the first one's point
        if (dm & (dm - 1ull)) {                                                  // more than one decider: all on one point?
            CNT(12);
            const double x0 = rl(r.ax, first), y0 = rl(r.ay, first);
            apart = dm & (__ballot(r.ax != x0) | __ballot(r.ay != y0));          // (!= is true on NaN, like !(a == x && b == y))
        }
        asm("" : "+s"(apart));                                                   // (ONE test of the mask, here: or the lone decider's path carries a lane mask to it)
        if (apart == 0ull) {
            r.ai = (r.ai & ~A_GRP) | (dec ? (1u << 8) : 0u);
            h.n_groups = 1;
        } else {
            CNT(13);
            // groups in ascending (x, then y) order == rows of np.unique(axis=0) :293
            bool todo = dec;
            uint32_t gid = 0;
            int g = 0;
            for (;;) {
                CNT(14);
                const double mxv = wave_nanmin_n<CA>(todo ? r.ax : __builtin_nan(""));
                if (!(mxv == mxv)) break;
                const double myv = wave_nanmin_n<CA>((todo && r.ax == mxv) ? r.ay : __builtin_nan(""));
                g++;
                if (todo && r.ax == mxv && r.ay == myv) { gid = (uint32_t)g; todo = false; }
            }
            r.ai = (r.ai & ~A_GRP) | (gid << 8);
            h.n_groups = g;
        }
        FPH(9);
        task_update(r, tmin, P.mwt, lane, 11);                                       // worker.py:50
        FPH(10);
        agent_update(r, tmin, P.mwt);                                                // worker.py:51
        FPH(11);
        h.empty_passes = 0;
        h.cur_group = 1;
        return true;
    }
};

// dynamic LDS of a k_rollout_fast launch: what the general code uses (the record image, + the scratch when it sits in LDS), then
// the removal path's compaction table (DUMMY_SLOT_BYTES: the bytes the leavers' dummy slots used to take)
template <int CA, int CT, bool RS>
constexpr uint32_t rollout_fast_lds_bytes(Lay L) {
    using SimT = Sim<CA, CT, RS, false>;
    return (SimT::SCR_IN_LDS ? L.lds_bytes() : SimT::lds_image_bytes(L)) + DUMMY_SLOT_BYTES;
}

// Same contract as k_rollout_random (see there); OBS: all three observation buffers given / none of them.
// PRIO: wave priorities, longest remaining work first (see the main loop) -- the host picks it for launches that fill the machine alone
// k_rollout_fast and its renewing form k_rn_rollout_fast: see k_rollout_fast.inc
#define DCM_RENEW 0
#include "k_rollout_fast.inc"
#undef DCM_RENEW
#define DCM_RENEW 1
#include "k_rollout_fast.inc"
#undef DCM_RENEW
#define DCM_RENEW 2   // the size-renewing form (k_rs_*): runtime-size instantiations only
#include "k_rollout_fast.inc"
#undef DCM_RENEW
