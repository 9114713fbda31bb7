/*
 * dcmrta_env.h -- C ABI of the MI355X-native batched coalition-formation + routing env.
 *
 * The reference (marmotlab/DCMRTA) has no FFI on this path: its boundary is duck-typed
 * Python (env/task_env.py class TaskEnv, driven by worker.py:41-112).  This header is
 * the boundary a maintainer binds instead (ctypes stub in INTEGRATION.md).  Each entry
 * point cites the reference interface it replaces.
 *
 * Conventions
 *  - plain C symbols, every call returns 0 on success or a negative dcm_status;
 *    dcm_last_error() returns a thread-local message for the last failure.
 *  - every array argument is a caller-owned DEVICE pointer (tensor.data_ptr()) unless it
 *    is marked "host"; the library never frees or retains it past the call.
 *  - every call takes the hipStream_t to enqueue on (torch.cuda.current_stream().cuda_stream,
 *    passed as void*) and is asynchronous with respect to the host.
 *  - a handle is bound to one device and is not thread-safe (one host thread per GPU,
 *    like one env per Ray actor in runner.py:74).  Calls that launch work must be made with
 *    that device current (hipSetDevice / torch.cuda.device): otherwise they fail with
 *    DCM_ERR_STATE instead of launching on the wrong GPU.
 *  - there is NO CPU implementation behind this ABI: without a HIP device dcm_create fails.
 *
 * One "env step" = one leader decision in one env = one TaskEnv.step call
 * (env/task_env.py:326) plus the task_update/agent_update and observation/mask
 * construction the worker wraps around it (worker.py:57-84).
 */
#ifndef DCMRTA_ENV_H
#define DCMRTA_ENV_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DCM_ABI_VERSION 5 /* v3: dcm_build_id, dcm_set_visibility, dcm_load_instances validates req on the device; v4: dcm_set_replay_placement; v5: DCM_PARAM_WIDE_MEMBERS; still v5, additions only: dcm_generate_instances, dcm_get_instances, dcm_generator_draws, dcm_set_instance_renewal, dcm_instance_index, DCM_PARAM_RENEW_SIZES, dcm_set_rollout_log, dcm_set_best_log, dcm_reduce_best, dcm_fork_envs, dcm_rollout_lookahead, dcm_rollout_lookahead_width, dcm_kernel_name, dcm_rollout_individual */

typedef struct dcm_env dcm_env; /* opaque */

typedef enum {
    DCM_OK = 0,
    DCM_ERR_INVALID = -1, /* bad argument */
    DCM_ERR_HIP = -2,     /* HIP runtime error (message has hipGetErrorString) */
    DCM_ERR_NO_DEVICE = -3,
    DCM_ERR_STATE = -4    /* call not valid in the handle's current state */
} dcm_status;

/* limits of this build */
#define DCM_MAX_AGENTS 128
#define DCM_MAX_TASKS 1023
#define DCM_MAX_MEMBERS 5 /* COALITION_SIZE, parameters.py:17: members <= requirement <= 5 */
#define DCM_MAX_MEMBERS_WIDE 16 /* member slots per task of a DCM_PARAM_WIDE_MEMBERS handle */
#define DCM_FOLLOWER_COLS 4

/* per-env flag bits reported by dcm_env_status */
#define DCM_FLAG_DONE 1u       /* episode over (terminal box of worker.py:87) */
#define DCM_FLAG_FINISHED 2u   /* env.finished is True (env/task_env.py:366-373) */
#define DCM_FLAG_TRUNCATED 4u  /* zero-decider guard fired (the reference would spin) */
#define DCM_FLAG_BAD_ACTION 8u /* action outside [0, T]; with DCM_PARAM_STRICT_MASK also a task the mask forbids */
#define DCM_FLAG_OVERFLOW 16u  /* a task would exceed DCM_MAX_MEMBERS members / injected follower count too large */
#define DCM_FLAG_BAD_LEADER 32u /* injected leader/follower not in the current group */
#define DCM_FLAG_WAIT_ORDER 128u /* informational, does not freeze the env: a per-(agent, task) abandonment counter saturated \
                                  * (65535; RL mode) or, in route replay, an agent was moved to abandoned_agent lists more than 16 \
                                  * times: that agent's sum_waiting_time then adds the excess max_waiting_time terms last instead \
                                  * of in task order (env/task_env.py:363-364), i.e. it may differ in the last bits */
#define DCM_FLAG_BAD_INSTANCE 256u /* dcm_load_instances found a requirement outside 1..DCM_MAX_MEMBERS (checked on the device): \
                                    * the env never starts (DONE from dcm_reset on) until a valid instance is loaded */
#define DCM_FLAG_TYPE_ERROR 64u /* route replay: the reference raises TypeError here (env/task_env.py:220, pre_set_route None) */

/* dcm_params.flags: individual selection (Worker.run_test_IS, worker.py:159-198, skips get_unique_group) -- all agents
 * deciding at an event form ONE group and act one by one in ascending id, each alone: unless a leader / follower count is
 * injected, dcm_observe / dcm_step take the lowest pending id as the deciding agent and no followers.
 * Honoured by dcm_reset / dcm_observe / dcm_step, and by dcm_rollout_individual, the persistent launch of this protocol, which
 * needs the flag; dcm_rollout_random / _policy / _explore / _lookahead* group by location on every handle. */
#define DCM_PARAM_NO_GROUPING 1u
/* dcm_params.flags: auto-reset for the lockstep API -- when a dcm_step ends an env's episode (terminal box of worker.py:87,
 * results written to its dcm_summary row), the same call restarts the env from the instance its record holds -- or, with
 * dcm_set_instance_renewal, from the env's next instance, drawn right there -- (reset + clear_decisions
 * + the first event, exactly what dcm_rollout_random does between its episodes: the decision counter keeps running) and the
 * fused observation is the first decision of the new episode; the env stays active.  dcm_env_episodes counts the finished
 * episodes.  This is SURVEY.md §8(d)'s "consecutive episodes, auto-reset to the same instance" for a policy in the loop: the
 * batch stays full instead of waiting for its longest episode.  Envs frozen by an error flag are not restarted, nor envs
 * that have finished dcm_params.auto_reset_episodes episodes (when that is non-zero).
 * The summary row of an episode that ended in an eager dcm_step may be computed LAZILY (the wave that ends an episode is the slowest
 * of its launch: it parks the final record and the reward + metrics are computed from it later, in batches): dcm_summary -- like
 * every entry point that reads or writes summary rows -- completes the waiting rows first, on the stream it is given, so callers
 * see no difference; the return log (dcm_set_return_log) and dcm_env_episodes are always up to date.  A dcm_step issued under
 * stream capture computes its terminal metrics inline and refuses (DCM_ERR_STATE) to be captured while rows of earlier eager steps
 * are still waiting: call dcm_summary or dcm_reset before the capture.  After a capture every step of the handle, eager or replayed,
 * computes its metrics inline. */
#define DCM_PARAM_AUTO_RESET 2u
/* dcm_params.flags: refuse host-supplied actions on masked tasks.  By default dcm_step simulates ANY action in [0, T] the way
 * TaskEnv.step does (env/task_env.py:326-342 never looks at the mask; worker.py:140's argmax can return a masked index): on a
 * task that is feasible or has status <= 0 the leader goes alone, the task may list more agents than it requires, and time
 * can even step backwards when an agent joins a task that is already over -- all of it restated.  The one limit is the
 * member-slot capacity: a task that would list more than DCM_MAX_MEMBERS agents freezes the env with DCM_FLAG_OVERFLOW.  With
 * this flag such an action freezes the env with DCM_FLAG_BAD_ACTION instead (the policy contract gives masked actions
 * probability 0, attention.py:74-76: a runner can use it to catch a policy that does not). */
#define DCM_PARAM_STRICT_MASK 4u
/* dcm_params.flags: DCM_MAX_MEMBERS_WIDE (16) member slots per task instead of DCM_MAX_MEMBERS (5).  The reference's member lists
 * are unbounded (env/task_env.py:321-322): a policy that ignores the mask (worker.py:140) can send more agents to a task than it
 * requires, and generate_env takes any max_coalition_size (:71).  A wide handle simulates both up to sixteen listed members per
 * task (requirements 1..16 are accepted by dcm_load_instances; a seventeenth member freezes the env with DCM_FLAG_OVERFLOW); its
 * records are 96 * T bytes larger, every shape runs the runtime-size kernels, dcm_get_members returns ids_out[B][T][16], and route
 * replay (which has its own member_cap) is not available on it.  Injected follower lists still hold at most DCM_FOLLOWER_COLS. */
#define DCM_PARAM_WIDE_MEMBERS 8u
/* dcm_params.flags: size renewal.  With this flag dcm_set_instance_renewal also accepts a RAGGED batch made by
 * dcm_generate_instances (a range with lo < hi: the reference's own training configuration, AGENTS_RANGE = (10, 20), TASKS_RANGE =
 * (20, 50), parameters.py:15-16): an env that restarts an episode inside a kernel then draws its next instance WITH its next sizes --
 * TaskEnv(agents_range, tasks_range, ..., seed = inst_seeds[e] + (n + 1) * stride), the number of tasks first, then the number of
 * agents, then the instance (env/task_env.py:58-71) -- and carries on as an env of those sizes.  The handle's per-env sizes then
 * change inside launches: dcm_get_instances returns the sizes of the instance an env holds now, observation rows beyond them are
 * padding, getters follow them, and they are part of a snapshot (see dcm_state_bytes).  Episode ends of such launches compute their
 * summary rows inline (no lazy rows, see DCM_PARAM_AUTO_RESET).  Without the flag, and on every other batch of a flagged handle,
 * nothing changes: a uniform generated batch renews exactly as on an unflagged handle, a ragged batch from
 * dcm_load_instances_ragged is still refused. */
#define DCM_PARAM_RENEW_SIZES 16u

typedef struct {
    int32_t n_envs;             /* B */
    int32_t n_agents;           /* A, identical for every env of the batch (driver.py:114-117) */
    int32_t n_tasks;            /* T */
    int32_t device;             /* HIP device ordinal */
    double max_waiting_time;    /* env/task_env.py:30 (10) */
    double max_time;            /* MAX_TIME, parameters.py:18 (100) */
    uint32_t flags;             /* DCM_PARAM_* bits */
    uint32_t auto_reset_episodes; /* with DCM_PARAM_AUTO_RESET: an env stops restarting once it has finished this many
                                   * episodes since dcm_reset (0 = it restarts forever) */
} dcm_params;

const char *dcm_last_error(void);
int dcm_abi_version(void);
/* 16 hex digits: sha256 over the kernel sources and compile flags this library was built from.  profiles/counters.json
 * stores it with every rocprof counter set, so bench.py can tell when the counters describe another binary. */
const char *dcm_build_id(void);

/* TaskEnv.__init__ (env/task_env.py:9-34): allocate SoA state for B envs of (A,T). */
int dcm_create(const dcm_params *params, dcm_env **out);
int dcm_destroy(dcm_env *env);

/* generate_env outputs (env/task_env.py:57-114) handed over as arrays:
 * depot[B,2] f64, task_xy[B,T,2] f64, req[B,T] i32 in 1..DCM_MAX_MEMBERS, dur[B,T] f64.
 * req is validated on the device: an env with a requirement outside the range gets DCM_FLAG_BAD_INSTANCE and stays frozen. */
int dcm_load_instances(dcm_env *env, const double *depot, const double *task_xy, const int32_t *req,
                       const double *dur, void *stream);
/* Distances in range.  The register-resident kernels of the one-chunk shapes (k_rollout_fast and its forms, k_step_fast) take the
 * square root of a squared distance without the scaling that arguments below 2^-767 need.  Instances made by dcm_generate_instances
 * never hold such a distance (coordinates are multiples of 2^-53).  For loaded instances dcm_load_instances /
 * dcm_load_instances_ragged (and dcm_restore_state, whose records may hold any instances) check every env on the device -- the
 * squared distance fma(dy, dy, dx * dx) between any two of the env's T + 1 points, depot included, must be 0 or >= 2^-767 -- and
 * read one word back, so these calls wait for the stream.  A handle that holds an env with a smaller non-zero squared distance
 * (two points some 1e-116 apart) runs the general code: k_rollout_random and k_step, same results, slower.  Inside a stream
 * capture the word cannot be read: the handle then runs the general code until its instances are next loaded outside one.
 * dcm_kernel_name tells which it is. */

/* The kernel a plain launch of the handle takes as things stand: entry 0 = dcm_rollout_random with all three observation buffers or
 * none ("k_rollout_fast", "k_rollout_fast_mc", "k_rollout_fast_g", "k_rollout_random"), entry 1 = dcm_step without leader / follower
 * overrides and without a route log ("k_step_fast", "k_step").  The base name: the renewing, logging and policy forms share it.
 * NULL (and dcm_last_error) for a null handle or another entry.  Host-side. */
#define DCM_KERNEL_ROLLOUT 0
#define DCM_KERNEL_STEP 1
const char *dcm_kernel_name(dcm_env *env, int32_t entry);

/* Ragged batch: TaskEnv(agents_range=(lo,hi), tasks_range=(lo,hi)) draws its own sizes per env
 * (env/task_env.py:58-65), which is what Runner.testing(seed) does with the default ranges
 * (runner.py:45-49, parameters.py:15-16).  Env e has n_agents[e] <= A agents and n_tasks[e] <= T tasks
 * and behaves exactly like an (n_agents[e], n_tasks[e]) env; the device arrays keep the batch shapes
 * of dcm_load_instances (rows beyond an env's own sizes are ignored).  Every output keeps the batch
 * shapes too: observation rows beyond an env's sizes are padding in the policy's convention --
 * all features -1 (attention.py:10-18, worker.py:253-257) and mask True (worker.py:258-261); getter
 * rows beyond the sizes read as 0 (next_decision NaN, current -2).  n_agents / n_tasks are HOST
 * arrays of B int32 (validated here).  dcm_load_instances switches back to a uniform batch.
 * Route replay (dcm_execute_routes) needs a uniform batch. */
int dcm_load_instances_ragged(dcm_env *env, const double *depot, const double *task_xy, const int32_t *req,
                              const double *dur, const int32_t *n_agents, const int32_t *n_tasks, void *stream);

/* TaskEnv(agents_range, tasks_range, max_coalition_size=.., max_duration=.., seed=inst_seeds[e]) for every env, made on the device
 * (env/task_env.py:21-22,57-71): replaces the host generator plus dcm_load_instances / dcm_load_instances_ragged, and nothing but
 * inst_seeds[B] u64 comes from the caller.  The instances are bit-equal to the reference's: np.random.default_rng(seed) is restated
 * in csrc/np_stream.hpp, the draw order of generate_env in csrc/instgen.hpp.  A range with lo == hi is an int (or a tuple that
 * draws nothing); lo < hi draws the env's own size from the stream first, tasks before agents (:58-65).
 * Needs 1 <= agents_lo <= agents_hi <= A, 1 <= tasks_lo <= tasks_hi <= T and 1 <= max_coalition_size <= the member slots of the
 * handle (DCM_MAX_MEMBERS, or DCM_MAX_MEMBERS_WIDE with DCM_PARAM_WIDE_MEMBERS), max_duration >= 0: otherwise DCM_ERR_INVALID, and
 * nothing is launched or changed.  When both ranges are the handle's dims the batch is uniform, exactly as after
 * dcm_load_instances; otherwise it is ragged as after dcm_load_instances_ragged, with the per-env sizes written on the device
 * (dcm_get_instances returns them).  dcm_reset must follow, as after dcm_load_instances. */
int dcm_generate_instances(dcm_env *env, const uint64_t *inst_seeds, int32_t agents_lo, int32_t agents_hi, int32_t tasks_lo,
                           int32_t tasks_hi, int32_t max_coalition_size, double max_duration, void *stream);

/* The instances the handle holds, however they got there, in the batch shapes of dcm_load_instances (any pointer may be NULL):
 * depot[B,2] f64, task_xy[B,T,2] f64, req[B,T] i32, dur[B,T] f64, n_agents[B] / n_tasks[B] i32 (the batch dims on a uniform
 * batch).  Rows beyond an env's own sizes read xy 0, req 1, dur 0. */
int dcm_get_instances(dcm_env *env, double *depot, double *task_xy, int32_t *req, double *dur, int32_t *n_agents,
                      int32_t *n_tasks, void *stream);

/* A fresh instance at every episode restart, drawn on the device: the reference never plays an instance twice, every Worker builds a
 * new TaskEnv(..., seed=...) (worker.py:32).  dcm_generate_instances keeps a device copy of inst_seeds[B] and its scalar arguments in
 * the handle and sets every env's INSTANCE INDEX to 0.  With stride != 0, whenever env e restarts an episode inside a kernel -- the
 * auto-reset of dcm_step (DCM_PARAM_AUTO_RESET), the restart between or before episodes of dcm_rollout_random -- it first replaces
 * its instance by the one of seed inst_seeds[e] + (n + 1) * stride (mod 2^64), n its index so far, and its index becomes n + 1; then
 * reset + clear_decisions and the first event as always.  With stride = B and seeds base + 0..B-1, episode k of env e plays instance
 * base + k * B + e.  stride == 0 (the default) turns renewal off: behaviour is then exactly that of a handle that never set it.
 * Valid only while the handle's instances came from dcm_generate_instances and the batch is uniform; otherwise DCM_ERR_STATE, and
 * nothing changes.  A ragged batch (a range with lo < hi) is refused, because an env's sizes would change inside a launch -- unless
 * the handle was created with DCM_PARAM_RENEW_SIZES: a ragged batch made by dcm_generate_instances is then accepted, and a
 * restarting env draws its next sizes with its next instance (see the flag; its sizes in the handle's table move with it, and an
 * env that does not renew -- below -- keeps the sizes of the episode it finished).  A ragged batch from dcm_load_instances_ragged
 * is refused with or without the flag.  dcm_load_instances[_ragged] and a new dcm_generate_instances turn renewal off.
 * What does not renew: dcm_reset restarts the instance the record holds and leaves the index alone; an env that stops at an episode
 * boundary -- the last of a call's `episodes`, a spent decision budget, the auto_reset_episodes limit, an error flag -- keeps the
 * finished episode's instance and results until a later call restarts it, so every getter stays valid for that episode.  The
 * index lives in the env's record: dcm_clone_state / dcm_restore_state carry it with the instance, and dcm_state_bytes is unchanged
 * (on a DCM_PARAM_RENEW_SIZES handle with a ragged batch the per-env sizes are carried as well: see dcm_state_bytes).
 * The seeds, the generator's arguments and the stride are the handle's and are not part of a snapshot: dcm_restore_state leaves them
 * and the setting as they are, so restore only snapshots of the instances the handle's last dcm_generate_instances made (or of
 * their renewals) while a stride is set -- a snapshot from before that call, or of loaded instances, would renew from seeds that are
 * not its own; turn renewal off first.
 * dcm_get_instances returns the instance a record holds now.  Host-side setter; takes effect at the next launch (a captured graph
 * keeps the setting it was captured with). */
int dcm_set_instance_renewal(dcm_env *env, uint64_t stride);
/* index_out[B] u32: every env's instance index n (0 after dcm_generate_instances / dcm_load_instances; see above). */
int dcm_instance_index(dcm_env *env, uint32_t *index_out, void *stream);

/* Known-answer entry point of the instance generator's random stream (no handle, like dcm_distance): for each of the n seeds
 * (u64[n]) the first n_doubles values of np.random.default_rng(seed).random(), then n_ints values of .integers(0, bound),
 * 1 <= bound <= 2^32 - 1, through the device routines dcm_generate_instances uses: doubles_out f64[n, n_doubles],
 * ints_out u32[n, n_ints]. */
int dcm_generator_draws(const uint64_t *seeds, int64_t n, int32_t n_doubles, uint32_t bound, int32_t n_ints,
                        double *doubles_out, uint32_t *ints_out, void *stream);

/* reset + clear_decisions (env/task_env.py:116-140) for every env, then advance each env to its
 * first decision point (event t=0, one group of all agents; worker.py:45-51).
 * seeds[B] u64: per-env seed of the choice protocol; the decision counter restarts at 0. */
int dcm_reset(dcm_env *env, const uint64_t *seeds, void *stream);

/* What worker.py:54-68 builds before calling the policy, for all envs at once:
 *   agents_out[B,A,6] f32   get_current_agent_status  (env/task_env.py:165-180)
 *   tasks_out[B,T+1,5] f32  get_current_task_status   (env/task_env.py:182-190)
 *   mask_out[B,T+1] u8      get_unfinished_task_mask + depot bit (:192-200, worker.py:57-61); 1 = forbidden
 *   leader_out[B] i32       the deciding agent (worker.py:54), -1 for finished envs
 *   active_out[B] u8        0 once the env's episode is over
 * leader_in (nullable, [B] i32, -1 = draw): inject the leader instead of drawing it.
 * Pure function of the state: calling it twice returns the same tensors. */
int dcm_observe(dcm_env *env, float *agents_out, float *tasks_out, uint8_t *mask_out, int32_t *leader_out,
                uint8_t *active_out, const int32_t *leader_in, void *stream);

/* TaskEnv.step (env/task_env.py:326-342) for the current leader of every active env, followed by
 * task_update/agent_update (worker.py:74-76) and the advance to the next decision point:
 * next leader in the group -> next group -> check_finished (worker.py:85) -> next event
 * (worker.py:45-51) -> terminal (worker.py:87, metrics :103-108).
 *   actions[B] i32: 0 = depot, k = task k-1.
 *   leader_in / nfol_in / followers_in[B,DCM_FOLLOWER_COLS] (all nullable): injected choices;
 *   nfol_in[b] < 0 means "draw followers from the protocol"; nfol_in[b] >= 0 is honoured for the depot action too (the
 *   leader returns with exactly those followers -- agent_step(agent, 0) of individual selection -- instead of the whole group).
 * If agents_out..active_out are non-NULL the observation of the NEW decision point is written
 * in the same launch (fused observe; leader drawn from the protocol). */
int dcm_step(dcm_env *env, const int32_t *actions, const int32_t *leader_in, const int32_t *nfol_in,
             const int16_t *followers_in, float *agents_out, float *tasks_out, uint8_t *mask_out,
             int32_t *leader_out, uint8_t *active_out, void *stream);

/* Optional route history = agent['route'] / agent['arrival_time'] of the reference (env/task_env.py:95-96,314,318), the
 * input of generate_traj / generate_route (env/task_env.py:375-418, worker.py:244-251).  When set, every agent_step
 * executed by dcm_step appends (task id, -1 = depot; arrival time) to the agent's log:
 * route_task[B,A,cap] i16, route_arrival[B,A,cap] f64, route_len[B,A] i32 -- caller-owned device memory that must
 * outlive its use; all NULL disables.  dcm_reset zeroes route_len; entries beyond cap are counted but not stored.
 * (The persistent launches, dcm_rollout_random / dcm_rollout_policy, never write this log: they have their own, dcm_set_rollout_log.) */
int dcm_set_route_log(dcm_env *env, int16_t *route_task, double *route_arrival, int32_t *route_len, int32_t cap);

/* The same history for the persistent launches: the routes of the episodes dcm_rollout_random / dcm_rollout_policy play.  Layout and
 * argument check of dcm_set_route_log: route_task[B,A,cap] i16 (-1 = depot), route_arrival[B,A,cap] f64, route_len[B,A] i32 --
 * caller-owned device memory that must outlive its use; all NULL disables.  A is the batch's agent dimension, also on a ragged batch,
 * where an env writes the rows a < its own A.  In addition n_agents x cap x 8 bytes must stay below 4 GiB (DCM_ERR_INVALID otherwise).
 *   What is logged: while set, every agent_step that dcm_rollout_random / dcm_rollout_policy execute appends (task id, arrival time)
 *     to the acting agent's row -- the leader, its followers, and the whole group on a depot action.
 *   Which episode: the log is that of the env's CURRENT episode.  The kernel zeroes the env's route_len row when it restarts an
 *     episode (after the instance renewal, if there is one); dcm_reset zeroes all rows.
 *   After a call the log holds the last episode the env played: complete if the env is DONE -- also for an env that stopped at an
 *     episode boundary with its budget spent, which keeps the finished episode's log.  If the decision budget stopped the env in the
 *     middle of an episode the log holds the prefix played so far, and a later persistent launch carries on appending from the
 *     stored lengths.
 *   Overflow: entries beyond cap are counted in route_len but not stored; only [0, min(len, cap)) of a row is defined.
 *   Independence: dcm_step never writes this log, and the persistent launches still never write the dcm_set_route_log one; an
 *     episode played partly by dcm_step is logged only for the part the persistent launches played.  The log is not part of
 *     dcm_clone_state / dcm_restore_state.
 *   Refusal: a launch that would take the size-renewing form (DCM_PARAM_RENEW_SIZES handle, ragged generated batch, stride set) while
 *     the log is set returns DCM_ERR_STATE under every policy, nothing changes, and the message names the log.
 *   Invariant: a launch with the log set returns exactly what the same launch returns without it -- steps_out, records, summaries,
 *     the return log, the per-decision observation stores, the instance index, every policy's budget rule.  (It runs other kernels:
 *     the logging forms of the one-chunk register-resident kernel and of the general one, under all three policies.)
 * Host-side setter. */
int dcm_set_rollout_log(dcm_env *env, int16_t *route_task, double *route_arrival, int32_t *route_len, int32_t cap);

/* The best episode of every env, kept on the device: with dcm_set_rollout_log set as well, the persistent launches (dcm_rollout_random,
 * dcm_rollout_policy, dcm_rollout_explore) keep for every env the best episode it has finished since dcm_reset -- across the
 * episodes of a launch and across launches -- so that ONE launch of B envs x E episodes yields B x E samples and B plans.
 * best_task[B,A,cap] i16, best_arrival[B,A,cap] f64, best_len[B,A] i32, best_summary[B,8] f64, best_episode[B] i32: caller-owned
 * device memory that must outlive its use; A and cap are those of the rollout log that is set when a launch runs.  All NULL
 * disables; some NULL and some not is DCM_ERR_INVALID.
 *   Candidates: an episode that reaches its end inside one of the three entry points without an error flag -- also one that began in
 *     an earlier launch or under dcm_step.  An episode the decision budget stops in mid-flight is no candidate until a later launch
 *     ends it; episodes that dcm_step ends never are.
 *   Order: a candidate replaces the kept episode if the env keeps none (best_episode == -1), if its n_finished (summary column 1) is
 *     larger, or if n_finished is equal and its reward (column 0) is larger.  Strict and exact in fp64: on a tie the earliest stays.
 *   On replacement best_summary[b] becomes the episode's eight dcm_summary values, best_episode[b] its ordinal since dcm_reset (the
 *     k of dcm_set_return_log), best_len[b, a] the rollout log's length (it may exceed cap), and best_task / best_arrival the rollout
 *     log's entries [0, min(len, cap)) of every agent row a < the env's own A.  Nothing is defined behind that prefix or in rows
 *     beyond the env's A.
 *   dcm_reset sets every best_episode to -1, every best_summary row to NaN and every best_len to 0.
 *   Invariant: a launch with the best log set returns exactly what the same launch returns with only the rollout log set -- steps,
 *     records, summaries, the return log, the rollout log (still the last episode), observation stores, status, episode counts.  (It
 *     runs another kernel form, k_bs_*.)
 *   Refusals, nothing launched and nothing changed: a launch while the best log is set and the rollout log is not, DCM_ERR_STATE; a
 *     launch while a renewal stride is set (dcm_set_instance_renewal), DCM_ERR_STATE -- the best of different instances means nothing:
 *     clear the stride or the best log.  Every refusal the entry point makes anyway stays as it is.
 * Host-side setter; not part of dcm_clone_state / dcm_restore_state. */
int dcm_set_best_log(dcm_env *env, int16_t *best_task, double *best_arrival, int32_t *best_len, double *best_summary,
                     int32_t *best_episode);

/* The best log reduced over groups of envs, on the device: envs [g * group, (g + 1) * group) are one group (K samples of one
 * instance, say), G = ceil(B / group) groups, the last one possibly short.  One kernel launch finds every group's winner and gathers
 * the winner's rows of the best log into compact caller-owned device buffers, so that N instances x K samples in ONE handle give N
 * plans and only those have to leave the device:
 *   win_env[G] i32          the winner's env index, -1 for a group in which no env keeps an episode
 *   win_summary[G,8] f64    its best_summary row (NaN for such a group); may be NULL
 *   win_episode[G] i32      its best_episode (-1); may be NULL
 *   win_len[G,A] i32        its best_len row (0)
 *   win_task[G,A,cap] i16, win_arrival[G,A,cap] f64   entries [0, min(len, cap)) of each of its agent rows, and behind them the fill
 *                           the logs start from, -2 / 0.0 (all fill): every element is written
 * A and cap are those of the logs that are set.  win_len, win_task and win_arrival may be NULL together (summaries only).
 *   Order: an env is a candidate iff best_episode != -1.  The winner has the most finished tasks (best_summary column 1), among those
 *     the largest reward (column 0), among those the LOWEST env index -- exact in fp64, 0.0 and -0.0 tie: it is the env a sequential
 *     scan of the group in env order would keep under dcm_set_best_log's strict replace rule.  Kept rows hold no NaN by that log's
 *     contract; no order is defined for one.
 *   Refusals, nothing launched: the best log not set, DCM_ERR_STATE (call dcm_set_best_log first); the three route arrays given while
 *     the rollout log, whose cap the rows have, is not set, DCM_ERR_STATE; group < 1, win_env NULL, or some but not all of win_len /
 *     win_task / win_arrival, DCM_ERR_INVALID.
 * Stream-ordered behind the launches that wrote the best log; no host synchronisation, legal under stream capture.  It reads the
 * best log and writes the win_* buffers, nothing else: no handle state changes, and a launch after it returns what it would have. */
int dcm_reduce_best(dcm_env *env, int32_t group, int32_t *win_env, double *win_summary, int32_t *win_episode,
                    int32_t *win_len, int16_t *win_task, double *win_arrival, void *stream);

/* Optional history of route replay: what execute_by_route leaves for generate_traj / plot_animation (env/task_env.py:375-418,
 * 589-590) -- agent['route'] / ['arrival_time'], task['members'] and task['feasible_assignment'].  When set, dcm_execute_routes
 * restarts the log of every env and each agent_step it runs (forced depot visits of :573-584 included) appends (task id, -1 =
 * depot; arrival time) to the agent's log: route_task[B,A,cap] i16, route_arrival[B,A,cap] f64, route_len[B,A] i32 (the layout of
 * dcm_set_route_log; entries beyond cap are counted but not stored; per env the lengths sum to steps_out).  After the episode
 * member_ids[B,T,member_cols] i16 holds every task's final member list in list order, -1 padded, and feasible[B,T] u8 its
 * feasible_assignment (at the cut-off t = 200 or on a TRUNCATED env a task can be feasible and not finished).  dcm_execute_routes
 * fails with DCM_ERR_INVALID, before it launches anything, when member_cols is smaller than the member_cap of dcm_load_routes.
 * Caller-owned device memory that must outlive its use; all NULL disables; member_ids and feasible may be NULL on their own.
 * The contents are defined for envs that end FINISHED, at the cut-off or TRUNCATED; for envs flagged TYPE_ERROR, BAD_ACTION or
 * OVERFLOW they are unspecified.  Independent of dcm_set_route_log, which dcm_step alone writes.  Host-side setter. */
int dcm_set_replay_log(dcm_env *env, int16_t *route_task, double *route_arrival, int32_t *route_len, int32_t cap,
                       int16_t *member_ids, int32_t member_cols, uint8_t *feasible);

/* Optional log of EVERY episode's return (reward = -makespan, env/task_env.py:424; what worker.py:87 reads per episode):
 * returns[B,cap] f64, caller-owned device memory that must outlive its use; NULL / 0 disables.  The k-th episode an env
 * finishes since dcm_reset (dcm_rollout_random, dcm_step) writes returns[b, k mod cap] -- a ring, so a caller that plays
 * `cap` episodes per call finds all of them after the call (dcm_summary keeps only the last one).  Host-side setter. */
int dcm_set_return_log(dcm_env *env, double *returns, int32_t cap);

/* Config-2 hot path: every env plays `episodes` complete episodes under the uniform-random valid
 * policy inside ONE persistent launch (worker.py:45-87 with the action drawn from slot 1 of the
 * protocol); the observation tensors + mask are produced at every decision exactly as dcm_observe
 * does and written to agents_out/tasks_out/mask_out (nullable: skip the stores).  Envs restart
 * from the instance their record holds between episodes -- or, with dcm_set_instance_renewal, from their next instance, drawn at
 * the restart --; the decision counter keeps running.  An env that is in the middle of an
 * episode when the call starts first plays that episode to its end (it counts as one of the `episodes`).
 * Decision budget: max_decisions_in[B] i64 (nullable device array) or, when NULL, the scalar max_decisions -- an env
 * takes at most that many decisions in this call (< 0 = unlimited).  When the budget runs out the env stays at the
 * decision point it has reached with nothing of the pending decision applied (dcm_observe gives its observation;
 * dcm_step / a further dcm_rollout_random carry on from there with identical results), and agents_out / tasks_out /
 * mask_out hold what the kernel stored for the LAST DECISION TAKEN -- which is how the parity tests compare the
 * persistent kernel's own per-decision stores with the oracle at arbitrary decision indices.
 * Handover: the env's record in HBM is the one place where the entry points meet.  After a budget stop or a dcm_step ANY of them
 * carries on with identical results -- dcm_step with or without injected choices, dcm_rollout_random / dcm_rollout_policy /
 * dcm_rollout_explore with all, some or none of the observation buffers, with the rollout log, the best log or a renewal stride set,
 * cleared or set since the last call -- whichever kernel each of them takes for the handle's shape, and in any order; an env of a
 * DCM_PARAM_AUTO_RESET handle that a persistent launch left DONE is restarted by the next persistent launch that gives it a budget,
 * not by dcm_step.  The rollout log is appended by the persistent launches only, each from the lengths the last one stored
 * (dcm_set_rollout_log).  tests/test_gpu_relay.py hands one episode across every ordered pair of kernel families a shape has.
 * steps_out[B] i64: decisions taken by each env in this call. */
int dcm_rollout_random(dcm_env *env, int32_t episodes, int64_t max_decisions, const int64_t *max_decisions_in,
                       float *agents_out, float *tasks_out, uint8_t *mask_out, int64_t *steps_out, void *stream);

/* The same persistent launch under a device policy.  Every argument other than `policy` means what it means in dcm_rollout_random:
 * the decision budget and the stop at a decision point with nothing applied, the per-decision observation stores, the restart
 * between episodes (with dcm_set_instance_renewal: on the env's next instance), the return log and the summary rows.
 *   DCM_POLICY_RANDOM   dcm_rollout_random itself: the same kernels, the same launch, the same results.
 *   DCM_POLICY_FIRST    the lowest unmasked task.
 *   DCM_POLICY_NEAREST  the unmasked task with the smallest fp64 Euclidean distance (env/task_env.py:161-163) from the deciding
 *                       agent's position; a tie goes to the lowest task index (the rounded distances are compared, strict <).
 * Both greedy policies take the depot (0) when no task is unmasked, like the random one.  Choice protocol: the leader (slot 0) and
 * the followers (slots 2+j) are drawn as always, slot 1 is simply not consumed, the decision counter advances as before.
 * An unknown policy: DCM_ERR_INVALID, nothing is launched.  A greedy policy while a ragged batch renews its SIZES
 * (DCM_PARAM_RENEW_SIZES handle, ragged generated batch, stride set): DCM_ERR_STATE, nothing changes -- ragged batches without
 * renewal, and uniform batches with it, work.
 * On a handle with max_waiting_time <= 0 a greedy policy does not end its episodes in general -- a member that has waited 0 is dropped
 * at once (env/task_env.py:269), decides again at the same time and takes the same task again, in the reference as here -- so such
 * a launch must be bounded: max_decisions >= 0 or max_decisions_in given, else DCM_ERR_INVALID; a negative entry of max_decisions_in counts as 0
 * there (the env takes no decision in the launch). */
#define DCM_POLICY_RANDOM 0
#define DCM_POLICY_FIRST 1
#define DCM_POLICY_NEAREST 2
int dcm_rollout_policy(dcm_env *env, int32_t policy, int32_t episodes, int64_t max_decisions,
                       const int64_t *max_decisions_in, float *agents_out, float *tasks_out,
                       uint8_t *mask_out, int64_t *steps_out, void *stream);

/* The same persistent launch under an EPSILON-GREEDY policy: the sampling baseline (play a stochastic heuristic many times -- one
 * instance replicated over the envs under different seeds -- and keep the best episode).  Every argument other than explore_q32
 * means what it means in the greedy launch above; `policy` is the BASE policy, DCM_POLICY_FIRST or DCM_POLICY_NEAREST.
 * Choice protocol (bit-exact everywhere): with key_1 = mix64(seed_e + GAMMA (d + 1)) of decision d, the decision's explore word is
 *     mix64(key_1 XOR 0xD6E8FEB86659FD93) >> 32        (32 bits)
 * and the decision EXPLORES iff explore word < explore_q32, a value in [0, 2^32] (epsilon = explore_q32 / 2^32).  An exploring
 * decision takes exactly the random policy's action (protocol slot 1 over the unmasked tasks); every other decision takes the base
 * policy's pick and does not consume slot 1.  The leader (slot 0), the followers (slots 2+j), the decision counter and the depot
 * action when no task is unmasked are as always.  So explore_q32 = 0 is the greedy policy and explore_q32 = 2^32 the random one,
 * bit for bit -- through this entry point's own kernels: there is no host-side shortcut for either value.
 * The rollout log may be set (the best env's log is the plan) or not (return sampling on large batches).
 * Refusals, nothing launched and nothing changed: a base policy other than FIRST / NEAREST (DCM_POLICY_RANDOM included) or
 * explore_q32 > 2^32: DCM_ERR_INVALID.  A launch that would renew a ragged batch's SIZES: DCM_ERR_STATE.  On a handle with
 * max_waiting_time <= 0 the base policy's rule holds: a decision budget must be given, else DCM_ERR_INVALID, and a negative entry
 * of max_decisions_in counts as 0. */
int dcm_rollout_explore(dcm_env *env, int32_t policy, uint64_t explore_q32, int32_t episodes, int64_t max_decisions,
                        const int64_t *max_decisions_in, float *agents_out, float *tasks_out, uint8_t *mask_out,
                        int64_t *steps_out, void *stream);

/* The same persistent launch under INDIVIDUAL SELECTION, the reference's second evaluation protocol (Worker.run_test_IS,
 * worker.py:159-198): the deciders of an event are not grouped by location; they act one by one in ascending id, each alone through
 * agent_step, task_update and agent_update behind each, and the depot action moves the deciding agent only.  A DECISION under this
 * form is one agent's agent_step: steps_out, max_decisions, max_decisions_in and the decision counter of the choice protocol count
 * those, and the observation buffers hold what the last deciding agent saw.
 * `policy` is any of DCM_POLICY_RANDOM, DCM_POLICY_FIRST, DCM_POLICY_NEAREST; explore_q32 in [0, 2^32] makes FIRST / NEAREST
 * epsilon-greedy by dcm_rollout_explore's rule (explore word of key_1 below explore_q32: the random policy's action, protocol slot 1)
 * and must be 0 with DCM_POLICY_RANDOM, which takes slot 1 at every decision.  Slot 0 (the leader draw) and the follower slots are
 * never consumed.  episodes, the budgets, the rollout log (set or not), the return log, the abandonment log, instance renewal with a
 * uniform stride and ragged batches work as in dcm_rollout_explore.  One kernel text serves every shape (k_is_rollout_random /
 * k_isrn_rollout_random): there is no register-resident form.
 * The handle must have been created with DCM_PARAM_NO_GROUPING: dcm_reset and dcm_step form the one-group event and take the lowest
 * pending id only under it, so a launch stopped by its budget in the middle of an event is carried on by dcm_step (or by another
 * launch) and the other way round.  The other dcm_rollout_* entry points keep grouping by location on such a handle.
 * Refusals, nothing launched and nothing changed.  DCM_ERR_INVALID: an unknown policy; explore_q32 > 2^32; explore_q32 != 0 with
 * DCM_POLICY_RANDOM; episodes < 1; FIRST / NEAREST on a handle with max_waiting_time <= 0 without a decision budget (a negative
 * entry of max_decisions_in counts as 0 there).  DCM_ERR_STATE: a handle without DCM_PARAM_NO_GROUPING; no dcm_reset yet; the best
 * log is set (there is no best-keeping form); a launch that would renew a ragged batch's SIZES. */
int dcm_rollout_individual(dcm_env *env, int32_t policy, uint64_t explore_q32, int32_t episodes, int64_t max_decisions,
                           const int64_t *max_decisions_in, float *agents_out, float *tasks_out, uint8_t *mask_out,
                           int64_t *steps_out, void *stream);

/* The same persistent launch with every decision chosen by ONE-STEP LOOKAHEAD over a base policy: the rollout algorithm, on the device.
 * Every argument other than base_policy means what it means in dcm_rollout_policy; base_policy is any of DCM_POLICY_RANDOM,
 * DCM_POLICY_FIRST, DCM_POLICY_NEAREST.
 * The rule: an env in front of decision d, with leader and mask drawn as always, values every action a the mask allows by
 *     v(a) = (finished tasks, reward)   -- entries 1 and 0 of the summary row
 * of the episode in which decision d takes a -- with this leader and the followers of protocol slots 2+j of decision d -- and the
 * base policy takes every later decision d+1, d+2, ... (same seed, running counter) until the episode ends.  Decision d then takes the
 * action with the largest v: finished tasks first, then reward, a tie to the lowest index; the depot when no task is unmasked.  The
 * choice protocol is a pure function of (seed, decision counter, slot), so the values are exact and the episode never ends below the
 * base policy's from the same state.
 * One wave owns one env and values its own actions one after the other between two snapshots of the env; masked actions cost
 * nothing, no second handle exists and nothing returns to the host.  The inner episodes leave NOTHING behind: the decision counter,
 * the episode count, the flags, the summary row, the return log, the rollout log, the abandonment log and its overflow counts,
 * steps_out and the observation buffers are what a launch leaves that only ever took the chosen actions.  steps_out, the decision
 * budget and the decision counter count the chosen (outer) decisions only; agents_out / tasks_out / mask_out hold the outer
 * decisions' rows; the rollout log (dcm_set_rollout_log, set or not) is appended by the outer decisions only and holds the plan.
 * episodes, budgets and the stop at a decision point, the restart between episodes, dcm_set_instance_renewal on a uniform generated
 * batch, ragged batches and DCM_PARAM_WIDE_MEMBERS handles work as in dcm_rollout_policy.  An inner episode that ends under the
 * zero-decider guard or at max_time is valued by (finished tasks, -now) like any other -- its summary row's entries.
 * The snapshots live in a device buffer the handle owns: per env its share of the dcm_clone_state blob (record + 64 B + 32 n_agents
 * + the overflow count table).  It is allocated by the FIRST call on a handle, not by dcm_create, so the first call cannot be
 * captured into a HIP graph (DCM_ERR_STATE under stream capture); later calls can.  Cost: about (unmasked actions) x (decisions
 * left in the episode) base-policy decisions per outer decision, serial in one wave: a 20A/50T launch takes some hundred milliseconds
 * whatever the batch size up to a full machine (DESIGN.md 6 has the measured times against the host-driven fan-out).
 * Refusals, before anything is launched or changed, every message names dcm_rollout_lookahead.  DCM_ERR_INVALID: a base policy
 * outside the three; episodes < 1; a handle with max_waiting_time <= 0 -- also with a decision budget, which bounds the outer
 * decisions only while every inner episode must end by itself.  DCM_ERR_STATE: no dcm_reset yet; the best log set (there is no
 * best-keeping lookahead form); a launch that would renew a ragged batch's SIZES. */
int dcm_rollout_lookahead(dcm_env *env, int32_t base_policy, int32_t episodes, int64_t max_decisions,
                          const int64_t *max_decisions_in, float *agents_out, float *tasks_out, uint8_t *mask_out,
                          int64_t *steps_out, void *stream);

/* dcm_rollout_lookahead with a CANDIDATE LIST: a decision values only the `width` nearest unmasked tasks, and the launch reports what
 * its inner episodes cost.  dcm_rollout_lookahead is this call with width = 0 and inner_out = NULL; every argument they share means
 * the same, and everything said there about what a launch leaves behind holds here.
 * The rule, for decision d of an env with n unmasked tasks and width = W >= 0:
 *   n == 0: the depot.  n == 1: that task.  Neither costs a snapshot or an inner episode.
 *   W == 0 or W >= n: dcm_rollout_lookahead's rule -- every unmasked action is valued, in ascending order, and the launch leaves byte
 *     for byte what that entry leaves.
 *   W == 1: DCM_POLICY_NEAREST's pick itself, whatever the base policy; no snapshot, no inner episode.
 *   otherwise: the candidates are the W unmasked tasks DCM_POLICY_NEAREST would pick one after the other if each pick were masked for
 *     the next one -- the W smallest by (distance from the leader, task index), compared lexicographically: the ROUNDED fp64 distances
 *     (dist2, agent first), so two tasks at an equal distance rank by the lower index, also across the cut between the W-th and the
 *     (W+1)-th.  The ranking is always NEAREST's; it does not depend on base_policy.  Each candidate is valued as in
 *     dcm_rollout_lookahead: decision d takes it with the leader and followers the real step draws and base_policy plays to the end;
 *     the largest (finished tasks, reward) wins, exact in fp64, and a tie of both goes to the LOWEST ACTION INDEX, whatever order the
 *     candidates were valued in.
 * inner_out[n_envs] (device, int64; may be NULL): the number of base-policy decisions the env took INSIDE inner episodes during this
 * launch, over all its outer decisions and episodes: every decision of an inner episode but its first, which is decision d itself.
 * An env that valued nothing (budget 0, width 1, never two unmasked tasks) gets 0.  Written once per launch like steps_out, which
 * still counts the outer decisions only.  The candidate list is never stored (n_tasks goes up to 1023): the env is back bit for bit
 * after every inner episode, so the next candidate is found again from the last one's (distance, index).
 * Cost: about min(W, unmasked actions) x (decisions left in the episode) base-policy decisions per outer decision; inner_out is that
 * number as played (DESIGN.md 6 has measured times beside it).
 * Refusals, before anything is launched or written (steps_out and inner_out included), every message names
 * dcm_rollout_lookahead_width: those of dcm_rollout_lookahead with the same status, and DCM_ERR_INVALID for width < 0. */
int dcm_rollout_lookahead_width(dcm_env *env, int32_t base_policy, int32_t width, int32_t episodes, int64_t max_decisions,
                                const int64_t *max_decisions_in, float *agents_out, float *tasks_out, uint8_t *mask_out,
                                int64_t *steps_out, int64_t *inner_out, void *stream);

/* Terminal results of the last finished episode (worker.py:87,103-108):
 * out[B,8] f64 = reward(-makespan), n_finished_tasks, success_rate, makespan, time_cost,
 *                waiting_time, travel_dist, efficiency. Rows of envs not yet done are NaN.
 * For an env that stops with an error flag (DCM_FLAG_BAD_*, DCM_FLAG_OVERFLOW) inside a multi-episode rollout call without a decision
 * budget, the row is that of some earlier finished episode of the call (or what it held before), not necessarily the latest: such a
 * call computes the metrics of the episode it ends with, and of every episode while a budget is set. */
int dcm_summary(dcm_env *env, double *out, void *stream);

/* Per-env flags (DCM_FLAG_*), decision counters and current time. Any pointer may be NULL. */
int dcm_env_status(dcm_env *env, uint32_t *flags_out, int64_t *decisions_out, double *now_out, void *stream);

/* episodes_out[B] i32: episodes finished by each env since dcm_reset (dcm_step with DCM_PARAM_AUTO_RESET, dcm_rollout_random). */
int dcm_env_episodes(dcm_env *env, int32_t *episodes_out, void *stream);

/* Per-task / per-agent state for parity tests and the per-env facade (any pointer may be NULL):
 * tasks: finished,feasible u8[B,T]; time_start,time_finish,sum_waiting_time f64[B,T]; status,n_members,n_abandoned i32[B,T]
 * agents: sum_waiting_time,travel_dist,next_decision,arrival f64[B,A]; x,y f64[B,A]; returned,assigned u8[B,A];
 *         current i32[B,A] (route[-1]: -2 none, -1 depot, k task); pending_group i32[B,A] (0 = not deciding in this
 *         event, g >= 1 = index of its group in get_unique_group order, env/task_env.py:291-298) */
int dcm_get_tasks(dcm_env *env, uint8_t *finished, uint8_t *feasible, double *time_start, double *time_finish,
                  double *sum_wait, int32_t *status, int32_t *n_members, int32_t *n_abandoned, void *stream);
int dcm_get_agents(dcm_env *env, double *sum_wait, double *travel_dist, double *next_decision, double *arrival,
                   double *x, double *y, uint8_t *returned, uint8_t *assigned, int32_t *current,
                   int32_t *pending_group, void *stream);

/* task['members'] (env/task_env.py:80) of every task in list order: ids_out int16[B,T,DCM_MAX_MEMBERS], -1 padded
 * (what generate_traj :390,:400 and the plotting code test membership against). */
int dcm_get_members(dcm_env *env, int16_t *ids_out, void *stream);

/* task['abandoned_agent'] (env/task_env.py:89) of every task as counts: counts_out uint16[B,A,T], [b,a,t] = number of times
 * task t has moved agent a to its abandoned_agent list in the current episode (calculate_waiting_time :358-364 only uses
 * membership and multiplicity; the order of the appends is not kept). */
int dcm_get_abandoned(dcm_env *env, uint16_t *counts_out, void *stream);

/* copy.deepcopy(env) (worker.py:33): snapshot / restore of the mutable SoA state.
 * dcm_state_bytes gives the buffer size (device memory) needed for all B envs.
 * Size renewal: while a DCM_PARAM_RENEW_SIZES handle holds a ragged batch, its per-env sizes change with the instances, so they
 * are part of the snapshot -- 8 * B more bytes at its end -- and dcm_restore_state brings them back with the records; dcm_state_bytes
 * reports the larger size.  Ask again after the batch changes between uniform and ragged, and restore a snapshot only into the
 * kind of batch it was taken from.  Handles without the flag are unchanged: their sizes never change after the load. */
int dcm_state_bytes(dcm_env *env, size_t *bytes_out);
int dcm_clone_state(dcm_env *env, void *dst, void *stream);
int dcm_restore_state(dcm_env *env, const void *src, void *stream);

/* Per-env copy between handles, on the device: for every env b of dst, s = src_index[b] (i32[B_dst], device):
 *   s == -1   env b is left alone.
 *   otherwise env b of dst BECOMES env s of src: the whole record -- header, mutable part and instance part, so the current time, the
 *             decision counter, the episode count and the instance index come with it --, the dcm_summary row, the abandonment log
 *             and its overflow counts.  Per env it is what dcm_clone_state / dcm_restore_state move for the whole batch, without the
 *             two extra copies, between handles of any two batch sizes: B envs fan out to B x K branches in one launch.
 *   seeds_in  u64[B_dst], device, or NULL.  Given, the choice-protocol seed in the header of every env that was copied becomes
 *             seeds_in[b]; the decision counter is not touched.  NULL: the copy keeps the source's seed and, the protocol being a pure
 *             function of (seed, decision counter, slot), behaves exactly as the source would have under any later sequence of calls
 *             -- each handle under its own parameters (max_waiting_time, max_time).
 *   ok_out    u8[B_dst], device, or NULL: 1 for every env that was copied or left alone, 0 for one that was refused (below).
 * dst may be src.  In place the call is race-free by contract and by check: a source must be its own source,
 * src_index[src_index[b]] == src_index[b], which the kernel tests with one more 4-byte load.  An env whose index breaks that rule, or
 * -- in place or not -- lies outside [-1, B_src), is left untouched and gets ok_out[b] = 0; every other env gets 1, s == b in place
 * included, where only the seed may change.  Between two handles the rule does not apply (nothing is read from dst).
 * All writes are plain stores, there is no host synchronisation, and the call is legal under stream capture.
 *   Refusals on the host, nothing launched and nothing changed, every message names dcm_fork_envs.  DCM_ERR_INVALID: n_agents,
 *     n_tasks or DCM_PARAM_WIDE_MEMBERS differ between the handles (the record layouts must be identical); the handles are on different
 *     devices; src_index NULL.  DCM_ERR_STATE: either handle has not been loaded and reset (also dst, although the call would fill
 *     it: a kernel is never pointed at a record nobody wrote); either handle holds a ragged batch (the per-env sizes have a host copy
 *     that a device-side map cannot keep in step); either handle has a renewal stride set; the current device is not the handles'.
 *   Host bookkeeping on success: deferred terminal metrics of both handles are computed first (a parked snapshot must not land on a
 *     copied summary row later); dst drops the restart image of its lockstep kernel (it belongs to the old instances; DCM_PARAM_AUTO_RESET
 *     restarts then recompute the first event, with the same results); dst no longer counts as made by dcm_generate_instances (its
 *     records no longer match its inst_seeds), so dcm_set_instance_renewal(dst, stride != 0) is refused until it is generated again.
 *   NOT copied: the caller-owned logs -- the buffers of dcm_set_route_log, dcm_set_rollout_log, dcm_set_best_log and
 *     dcm_set_return_log are not touched and stay dst's own lineage.  The episode count IS copied, so later return-log slots and
 *     best_episode ordinals of dst continue from the source's count; a caller who wants a source's log rows in the copy gathers them
 *     in their own memory.  Neither are the handle's parameters, seeds of dcm_generate_instances, routes or visibility schedule. */
int dcm_fork_envs(dcm_env *dst, dcm_env *src, const int32_t *src_index, const uint64_t *seeds_in, uint8_t *ok_out,
                  void *stream);

/* calculate_eulidean_distance (env/task_env.py:161-163) and travel time (:315) on the device, for the
 * known-answer test of the fp64 sqrt/divide path: dist_out[n], time_out[n] (nullable). */
int dcm_distance(const double *ax, const double *ay, const double *bx, const double *by, double *dist_out,
                 double *time_out, int64_t n, void *stream);

/* pre_set_route (env/task_env.py:595-599) for every agent of every env:
 * routes[B,A,route_cap] i32 actions in visiting order (0 = depot, k = task k-1; what baselines/CTAS-D.py:41-45 passes),
 * route_len[B,A] i32 (-1 = pre_set_route stays None, 0 = empty list).  member_cap (1..32) sizes the per-task member
 * slots of replay mode, where a task may collect more agents than it requires. Arrays are copied. */
int dcm_load_routes(dcm_env *env, const int32_t *routes, const int32_t *route_len, int32_t route_cap,
                    int32_t member_cap, void *stream);

/* The dynamic-arrival schedule of execute_by_route's reactive mode.  The reference hard-codes it:
 *   visible_length = int(np.clip(current_time // 10 * 20 + 20, 20, 100))     env/task_env.py:567
 *   depot re-arm time (next_action - 1) // 20 * 10                           env/task_env.py:221
 * i.e. 20 tasks at t = 0, 20 more every 10 time units, never more than 100 -- tasks 101.. of a larger instance never appear.
 * Here the four constants are handle parameters (initial, batch, period, cap; defaults 20, 20, 10, 100 = the reference):
 *   visible_length = int(clip(now // period * batch + initial, initial, cap)),  re-arm (next - 1) // batch * period.
 * Needs initial >= 0, batch >= 1, period >= 1, cap >= initial.  Host-side setter; takes effect at the next dcm_execute_routes. */
int dcm_set_visibility(dcm_env *env, int32_t initial, int32_t batch, int32_t period, int32_t cap);

/* Which replay kernel dcm_execute_routes runs and where it keeps its state.
 * 0 = auto (default): the register-resident kernel whenever the shape allows it -- at most 128 agents, member_cap <= 8, and at
 *     most 128 LIVE tasks, i.e. tasks that can ever get a member: all of them without dynamic arrivals, tasks 1..cap with them
 *     (an agent is never sent to a task that is not visible yet, env/task_env.py:578-584, and visible <= cap, :567).  BASELINE
 *     config 5 (100A/500T at the reference's cap of 100) and every 20A/50T-class replay qualify.  Otherwise the general kernel,
 *     with its "replay scratch" (member arrival times, time_finish, wake-up times, travel distance, latest arrival; allocated by
 *     dcm_load_routes: 8 T (member_cap + 1) + 16 A + 4 T bytes per env) in LDS when the batch has at most four envs per CU --
 *     every env is resident at once anyway and one wave's latency is what counts -- else in HBM.
 * 1 / 2: always the general kernel, replay scratch in LDS / in HBM (for tests and measurements).
 * Results do not depend on it. */
int dcm_set_replay_placement(dcm_env *env, int32_t placement);

/* execute_by_route (env/task_env.py:562-593; max_waiting_time 100, cut-off 200) followed by get_episode_reward
 * (:420-425), whole episode in one launch.  reactive != 0 enables dynamic task visibility (:566-567,:578-584 and the
 * depot branch of agent_update :213-224).  Results: dcm_summary rows + the optional arrays
 * steps_out i64[B] (agent_step calls), flags_out u32[B] (DCM_FLAG_*), finished u8[B,T], time_start/time_finish/
 * task_wait f64[B,T], n_members i32[B,T], agent_wait/travel_dist f64[B,A], returned u8[B,A]. */
int dcm_execute_routes(dcm_env *env, int32_t reactive, int64_t *steps_out, uint32_t *flags_out, uint8_t *finished,
                       double *time_start, double *time_finish, double *task_wait, int32_t *n_members,
                       double *agent_wait, double *travel_dist, uint8_t *returned, void *stream);

/* bytes of canonical state per env: S = 64 + 48*A + 96*T.  (Handles with A <= 20 and T <= 50 keep their
 * records in the fixed Lay{20,50} layout -- 5824 B per env -- so that every shape of the reference's training range runs
 * the same constant-offset kernels; dcm_state_bytes reports what is really allocated.) */
int dcm_record_bytes(dcm_env *env, size_t *bytes_out);

#ifdef __cplusplus
}
#endif
#endif /* DCMRTA_ENV_H */
