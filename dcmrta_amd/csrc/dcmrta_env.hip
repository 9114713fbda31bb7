// dcmrta_env.hip -- MI355X (gfx950) batched coalition-formation + routing environment.
//
// One wavefront (64 lanes) per env instance, one env per 64-thread workgroup.  The env's
// canonical record (S = 64 + 48*A + 96*T bytes, SURVEY.md §8d / DESIGN.md §3) is copied
// HBM -> LDS with 16-byte-per-lane coalesced loads, every phase of the reference state
// machine then runs wave-parallel on the LDS copy (lanes stride over tasks for
// task_update / mask / task observation and over agents for agent_update / agent
// observation / next_decision; wave-wide reductions use ballots and DPP row shifts),
// and the mutable part of the record is copied back.  The persistent rollout kernel keeps
// the record in LDS for whole episodes.  All times and positions are fp64 with the
// reference's operation order (compile with -ffp-contract=off); observations are rounded to
// fp32 exactly where the reference casts (worker.py:62,64).  No MFMA: the path is
// elementwise/reduction work, not a dense contraction.
//
// The simulator is a template over the batch shape (A agents, T tasks): the BASELINE shapes
// (20/50, 50/200, 100/500) are compiled with constant LDS offsets and fully unrolled
// lane-chunk loops, any other shape runs the <0,0> instantiation with runtime sizes.
// Wave-uniform state (header, choice-protocol keys, group bitmasks) lives in SGPRs.
//
// Reference restated: env/task_env.py (TaskEnv) and worker.py:41-112 (the rollout loop).
// Every device function cites the lines it follows.
#include <array>
#include <cstdlib>
#include <mutex>
#include <tuple>
#include <type_traits>

#include "common.hpp"
#include "np_stream.hpp"

using namespace dcm;

// Translation units (Makefile).  The library is built from this file eight times; every unit but the main one holds device code and
// its launchers only, and the main unit reaches them through the dcm::launch_rollout_* functions declared below.
//   unit    macro          holds                                                          options
//   env     -DDCM_SPLIT_G  the host API and every kernel that is not in a unit below      SPLIT SCHED
//   env_g   -DDCM_TU_G     k_rollout_fast_g and its forms (rollout_fast_g.hpp)            SCHED
//   env_p   -DDCM_TU_P     the greedy forms k_hp_* / k_hprn_* (rollout_policy.hpp)        SPLIT SCHED
//   env_l   -DDCM_TU_L     the logging forms k_lg_* / k_lgrn_* (rollout_log.hpp)          SPLIT SCHED
//   env_e   -DDCM_TU_E     the epsilon-greedy forms k_ex_* / k_exrn_* (rollout_explore.hpp)  SPLIT SCHED
//   env_b   -DDCM_TU_B     the best-keeping form k_bs_* (rollout_best.hpp)                 SPLIT SCHED
//   env_a   -DDCM_TU_A     the lookahead form k_la_* / k_larn_* (rollout_lookahead.hpp)    SPLIT SCHED
//   env_i   -DDCM_TU_I     the individual-selection form k_is_* / k_isrn_* (rollout_individual.hpp)  SPLIT SCHED
// SPLIT (-mllvm -phi-elim-split-all-critical-edges=1) costs k_rollout_fast_g 4 % (8.19 -> 8.53 ms per 4096 x 70A/130T launch) while it
// buys the one-chunk and the 50A/200T kernel 2.1 % / 1.3 %: hence env_g.  The form units exist so that every kernel that was there
// before them compiles from the text, and to the code, it had without them.  With none of the macros (the developer tools'
// one-command builds) everything is in one unit.
#if defined(DCM_TU_G) || defined(DCM_TU_P) || defined(DCM_TU_L) || defined(DCM_TU_E) || defined(DCM_TU_B) || defined(DCM_TU_A) || \
    defined(DCM_TU_I)
#define DCM_DEVICE_ONLY_TU 1
#elif !defined(DCM_SPLIT_G)
#define DCM_ONE_UNIT 1
#endif
#if defined(DCM_TU_G) || defined(DCM_ONE_UNIT)
#define DCM_HAVE_FAST_G 1     // this unit holds k_rollout_fast_g and its launcher
#endif
#if defined(DCM_TU_P) || defined(DCM_ONE_UNIT)
#define DCM_HAVE_POLICY 1     // ... the greedy-policy forms and their launcher
#endif
#if defined(DCM_TU_L) || defined(DCM_ONE_UNIT)
#define DCM_HAVE_LOG 1        // ... the logging forms and their launcher
#endif
#if defined(DCM_TU_E) || defined(DCM_ONE_UNIT)
#define DCM_HAVE_EXPLORE 1    // ... the epsilon-greedy forms and their launcher
#endif
#if defined(DCM_TU_B) || defined(DCM_ONE_UNIT)
#define DCM_HAVE_BEST 1       // ... the best-keeping form and its launcher
#endif
#if defined(DCM_TU_A) || defined(DCM_ONE_UNIT)
#define DCM_HAVE_LOOKAHEAD 1  // ... the lookahead form and its launcher
#endif
#if defined(DCM_TU_I) || defined(DCM_ONE_UNIT)
#define DCM_HAVE_INDIVIDUAL 1 // ... the individual-selection form and its launcher
#endif
namespace dcm {
#if !defined(DCM_DEVICE_ONLY_TU)
thread_local char g_err[512] = "";
int fail(int code, const char* fmt, const char* a, const char* b) {
    snprintf(g_err, sizeof(g_err), fmt, a, b);
    return code;
}
#endif
// The arguments of every persistent rollout kernel (k_rollout_random, k_rollout_fast, k_rollout_fast_mc, k_rollout_fast_g), in
// their order
struct RolloutArgs {
    int A, T, PA, PT;
    KP kp;
    unsigned char* state;
    int episodes;
    float* agents_out; float* tasks_out; uint8_t* mask_out;
    int64_t* steps_out; double* summary; uint16_t* ablog;
    int32_t* sizes;      // the handle's size table: a size-renewing form (k_rs_*) writes it, every other form takes it const
    int64_t budget_all; const int64_t* budget_in;
    unsigned char* gscr; double* retlog; int retcap;
    auto kernel_args() const {
        return std::make_tuple(A, T, PA, PT, kp, state, episodes, agents_out, tasks_out, mask_out, steps_out, summary, ablog, sizes, budget_all,
                               budget_in, gscr, retlog, retcap);
    }
    Renew rn;            // last argument of the renewing forms (k_rn_*, k_rs_*)
    plan::RenewForm form;  // which form the launch takes (plan::renew_form)
    int policy = DCM_POLICY_RANDOM;   // last argument of the greedy-policy forms (k_hp_*, k_hprn_*)
    RouteLog lg{nullptr, nullptr, nullptr, 0};   // last argument of the logging forms (k_lg_*, k_lgrn_*), behind `policy`
    uint64_t explore_q32 = 0;          // the epsilon-greedy forms (k_ex_*, k_exrn_*): between `policy` and the log
    BestLog best{nullptr, nullptr, nullptr, nullptr, nullptr};   // the best-keeping form (k_bs_*): behind the epsilon-greedy forms' arguments
    unsigned char* snap = nullptr;     // the lookahead form (k_la_*, k_larn_*): the handle's snapshot buffer, behind `policy` and the log
    int width = 0;                     // ... then the number of nearest actions a decision values (0: every unmasked one)
    int64_t* inner_out = nullptr;      // ... and, per env, the decisions of the inner episodes (null: not wanted)
};
// k_rollout_fast_g<NAC, NTC, OBS> / k_rn_rollout_fast_g / k_rs_rollout_fast_g (rollout_fast_g.hpp, its own translation unit)
void launch_rollout_fast_g(int nac, int ntc, bool obs, unsigned grid, Lay L, hipStream_t stream, const RolloutArgs& a);
// The greedy, logging and epsilon-greedy forms of k_rollout_fast / k_rollout_random (k_form.inc), each set in a translation unit of its
// own.  fast: plan::form_rollout_kind said Fast; a.form: Plain or Instance; a.policy: DCM_POLICY_FIRST or DCM_POLICY_NEAREST, in the
// logging forms any of the three; a.lg: the handle's rollout log, which the epsilon-greedy forms also take unset; a.explore_q32 <= 2^32.
// The best-keeping form (k_bs_*) takes the epsilon-greedy forms' arguments and a.best; it has no renewing kernels (-1 for a.form other
// than Plain: the host has refused that launch).
// Return 0, or -1 when `kind` has no one-chunk kernel (the caller asked plan::form_rollout_kind, so it has).
// allow_lds_*: the form's share of dcm_create's dynamic-LDS limit (see there).
using FormLauncher = int(plan::SimKind kind, bool fast, bool obs, unsigned grid, Lay L, hipStream_t stream, const RolloutArgs& a);
// The lookahead form (k_la_* / k_larn_*) takes a.policy (any of the three), a.lg (set or not), a.snap, a.width and a.inner_out; it
// exists for the general kernel text alone: `fast` and `obs` are ignored.
FormLauncher launch_rollout_policy, launch_rollout_log, launch_rollout_explore, launch_rollout_best, launch_rollout_lookahead;
// The individual-selection form (k_is_* / k_isrn_*) takes the epsilon-greedy forms' arguments, a.policy being any of the three; like the
// lookahead form it exists for the general kernel text alone.
FormLauncher launch_rollout_individual;
void allow_lds_policy(int lds);
void allow_lds_log(int lds);
void allow_lds_explore(int lds);
void allow_lds_best(int lds);
void allow_lds_lookahead(int lds);
void allow_lds_individual(int lds);
}  // namespace dcm

namespace {

// Optional per-phase cycle accounting of the rollout kernel (tools/phase_profile.py builds a separate
// libdcmrta_prof.so with -DDCM_PROFILE_PHASES; the product build compiles these macros to nothing).
#ifdef DCM_PROFILE_PHASES
__device__ unsigned long long g_phase_cycles[16];
// k_step (lockstep kernel): per-env rows (no contended atomics: one wave owns its row).  Row e = 32 words: [0..7] phase cycles
// summed over the launches, [8..15] their maxima over the launches, [16..27] the inner marks of apply_and_advance summed,
// [28] launches in which the env was active  (tools/phase_profile.py lockstep)
#define DCM_STEP_PROF_ENVS 65536
__device__ unsigned long long g_step_rows[DCM_STEP_PROF_ENVS * 32];
#define PHK_DECL unsigned long long phk_t = __builtin_readcyclecounter(); const unsigned long long phk_start = phk_t; \
                 unsigned long long* const phk_row = g_step_rows + (size_t)(blockIdx.x % DCM_STEP_PROF_ENVS) * 32
#define PHK_ADD(i, v) do { if (lane == 0) { phk_row[i] += (v); if (phk_row[8 + (i)] < (v)) phk_row[8 + (i)] = (v); } } while (0)
#define PHK_MARK(i) do { const unsigned long long t_ = __builtin_readcyclecounter(); PHK_ADD(i, t_ - phk_t); phk_t = t_; } while (0)
#define PHK_TOTAL(i) do { const unsigned long long t_ = __builtin_readcyclecounter(); PHK_ADD(i, t_ - phk_start); \
                          if (lane == 0) phk_row[28] += 1; } while (0)
#define PHK_INNER() do { if (lane == 0) for (int i_ = 0; i_ < 12; i_++) phk_row[16 + i_] += ph_acc[i_]; } while (0)
#define PH_DECL unsigned long long ph_t0 = __builtin_readcyclecounter(), ph_acc[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}
#define PH_MARK(i) do { unsigned long long t_ = __builtin_readcyclecounter(); ph_acc[i] += t_ - ph_t0; ph_t0 = t_; } while (0)
#define PH_FLUSH(lane) do { if ((lane) == 0) for (int i_ = 0; i_ < 12; i_++) atomicAdd(&g_phase_cycles[i_], ph_acc[i_]); } while (0)
#define PH_ARGS , unsigned long long& ph_t0, unsigned long long (&ph_acc)[12]
#define PH_PASS , ph_t0, ph_acc
// the register-resident persistent kernel (rollout_fast.hpp): its own marks, kept in the Fast<> object (tools/phase_fast.py)
__device__ unsigned long long g_fast_cycles[16];
#define FPH_MEMBERS mutable unsigned long long fph_t = 0, fph_acc[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}
#define FPH_START(f) ((f).fph_t = __builtin_readcyclecounter())
#define FPH(i) do { const unsigned long long t_ = __builtin_readcyclecounter(); this->fph_acc[i] += t_ - this->fph_t; this->fph_t = t_; } while (0)
#define FPHK(f, i) do { const unsigned long long t_ = __builtin_readcyclecounter(); (f).fph_acc[i] += t_ - (f).fph_t; (f).fph_t = t_; } while (0)
#define FPH_FLUSH(f, lane) do { if ((lane) == 0) for (int i_ = 0; i_ < 16; i_++) atomicAdd(&g_fast_cycles[i_], (f).fph_acc[i_]); } while (0)
#elif defined(DCM_PHASE_MARKS)
// tools/loop_insts.py --phases: the same marks as assembler comments, to attribute the decision loop's instructions to phases
#define FPH_MEMBERS
#define FPH_START(f)
#define FPH(i) asm volatile("; FPHMARK " #i)
#define FPHK(f, i) asm volatile("; FPHMARK " #i)
#define FPH_FLUSH(f, lane)
#define FPM(i) asm volatile("; FPHMARK " #i)     // sub-phase brackets (20/21 member removal, 22/23 one follower draw): marks mode only
#else
#define FPH_MEMBERS
#define FPH_START(f)
#define FPH(i)
#define FPHK(f, i)
#define FPH_FLUSH(f, lane)
#endif
#ifndef FPM
#define FPM(i)
#endif
#ifndef DCM_PROFILE_PHASES
#define PHK_DECL
#define PHK_MARK(i)
#define PHK_TOTAL(i)
#define PHK_INNER()
#define PH_DECL
#define PH_MARK(i)
#define PH_FLUSH(lane)
#define PH_ARGS
#define PH_PASS
#endif

// Optional dynamic path counts of the register-resident rollout kernel (tools/path_counts.py builds a separate library with
// -DDCM_COUNT_PATHS; behind profiles/r06_budget.md).  The product build compiles CNT() to nothing.
#ifdef DCM_COUNT_PATHS
__device__ unsigned long long g_path_counts[32];
#define CNT(i) do { if (threadIdx.x == 0) atomicAdd(&g_path_counts[i], 1ull); } while (0)
#else
#define CNT(i)
#endif

// ================================================================================== the simulator
// Three kinds of instantiation:
//   <CA, CT, false>  exact shape: sizes, record layout and lane-chunk trip counts are compile-time constants
//   <CA, CT, true>   runtime sizes (uniform or per-env) inside the CONSTANT record layout Lay{CA,CT}: every shape with
//                    A <= CA and T <= CT -- the reference's whole training range for <20,50> (parameters.py:15-16,
//                    driver.py:114-115 draws a new shape every round) -- keeps constant LDS offsets and unrolled lane-chunk
//                    loops; only the loop guards read the sizes
//   <0, 0, false>    anything else: runtime sizes and a runtime layout Lay{pA,pT}
// MG (exact multi-chunk shapes, persistent kernel only): the member arrival times f64[M][T] -- 43 % of a 50A/200T LDS image -- are
// not copied into LDS at all: the kernel works on the marr section of the env's own HBM record (one wave owns the record; a
// wave's global accesses are issued and served in order, so it sees its own stores, and the section is read only at the head of
// task_update's chain and by the terminal metrics).  The sections behind it move up by MSH bytes in the LDS image.
// MC: member slots per task (5; 16 = DCM_MAX_MEMBERS_WIDE, two id words, on a DCM_PARAM_WIDE_MEMBERS handle, which always runs the
// <0,0> instantiation).
template <int CA, int CT, bool RS, bool MG = false, int MC = M>
struct Sim {
    static_assert(MC == M || (MC == MW && CA == 0 && !MG), "wide member slots: runtime-size instantiation only");
    static constexpr int IW = (MC + 7) / 8;               // 64-bit id words per task
    using Ids = IdW<IW>;
    static constexpr int NAW = CA ? (CA + 63) / 64 : AW_MAX;  // agent chunks == words of an agent bitmask
    static constexpr int NTC = CT ? (CT + 63) / 64 : 0;       // task lane chunks (0 = runtime)
    static constexpr bool EXACT = (CA != 0) && !RS;
    // <CA, CT, true> with more than one task chunk (<128,256,true>): the template only BOUNDS the sizes -- agent-mask words and
    // lane-chunk trip counts are constants, loops unrolled -- while the record keeps the batch's own layout Lay{pA,pT} (a
    // Lay{128,256} image would be 30 KB per env whatever the batch needs); every mid-size shape shares this one instantiation
    static constexpr bool RL = RS && (CT > WAVE);
    int rA, rT;           // this env's own sizes (ignored by the exact instantiation)
    int pA, pT;           // record layout dims (read by the <0,0> instantiation only)
    unsigned char* base;  // record base (LDS in the env kernels)
    unsigned char* scr;   // terminal-metrics scratch (LDS behind the record, or this env's slice of the HBM scratch)
    double* gm = nullptr; // MG: the marr section of this env's HBM record
    static constexpr uint32_t MSH = MG ? 8u * (uint32_t)MC * (uint32_t)CT : 0u;   // = Lay::mids() - Lay::marr()
    // Exact multi-chunk shapes (50A/200T, 100A/500T): the task coordinates -- read-only instance data that only the task's own
    // lane and, for the chosen task, the whole wave ever read -- live in two registers per lane chunk (struct XY, owned by the
    // kernel and handed to observe / apply_and_advance) instead of 16 bytes per task of LDS.  The LDS image of a 50A/200T env
    // shrinks from 21.7 to 18.5 KB = 8 instead of 7 resident workgroups per CU: config 4 launch 9.63 -> 9.08 ms (-5.8 %),
    // k_step<50,200> at 16 384 envs -4 %.  (For the one-chunk layouts the same change was measured SLOWER: their kernels are
    // limited by registers, not LDS.)
    static constexpr bool IRB = (CT > WAVE) && !RS;
    static_assert(!MG || ((CT > WAVE) && !RS), "MG needs an exact multi-chunk shape");
    struct XY { double x[IRB ? NTC : 1], y[IRB ? NTC : 1]; };
    // the persistent kernel of the one-chunk shapes keeps the scratch in LDS (9.5 KB per env at 20A/50T with the per-agent term
    // lists, + 512 B for the removal path (Fast<>: its table): sixteen workgroups fill the CU's 160 KB exactly and all 4096 envs of the BASELINE batch are
    // resident); every other kernel trades it for more resident workgroups
    static constexpr bool SCR_IN_LDS = (CA != 0 && !RL && Lay{CA, CT}.lds_bytes() <= 10240);   // 16 workgroups per CU still fit

    __device__ __forceinline__ int A() const { return EXACT ? CA : rA; }
    __device__ __forceinline__ int T() const { return EXACT ? CT : rT; }
    __device__ __forceinline__ Lay L() const { return Lay{(CA && !RL) ? CA : pA, (CT && !RL) ? CT : pT, MC}; }
    __device__ __forceinline__ int PT() const { return (CT && !RL) ? CT : pT; }     // pitch of the [M][T] member-arrival slots
    // batch dims (shapes of the output arrays) given the kernel's (A,T) arguments
    __device__ __forceinline__ static int BA(int A) { return EXACT ? CA : A; }
    __device__ __forceinline__ static int BT(int T) { return EXACT ? CT : T; }
    // lane-chunk loops over tasks / agents: constant trip count (fully unrolled, guard per chunk) unless the layout is runtime
    __device__ __forceinline__ int tchunks() const { return CT ? NTC : (rT + WAVE - 1) / WAVE; }
    __device__ __forceinline__ int achunks() const { return CA ? NAW : (rA + WAVE - 1) / WAVE; }
    template <class F>
    __device__ __forceinline__ void for_tasks(int lane, F&& f) const {        // f(t) for t = lane, lane + 64, ... < T
        if constexpr (RS) {
#pragma unroll
            for (int c = 0; c < NTC; c++) { const int t = c * WAVE + lane; if (t < rT) f(t); }
        } else {
            for (int t = lane; t < T(); t += WAVE) f(t);
        }
    }
    template <class F>
    __device__ __forceinline__ void for_agents(int lane, F&& f) const {
        if constexpr (RS) {
#pragma unroll
            for (int c = 0; c < NAW; c++) { const int a = c * WAVE + lane; if (a < rA) f(a); }
        } else {
            for (int a = lane; a < A(); a += WAVE) f(a);
        }
    }
    __device__ __forceinline__ double* ax() const { return (double*)(base + L().ax()); }
    __device__ __forceinline__ double* ay() const { return (double*)(base + L().ay()); }
    __device__ __forceinline__ double* arr() const { return (double*)(base + L().arr()); }
    __device__ __forceinline__ double* nd() const { return (double*)(base + L().nd()); }
    __device__ __forceinline__ double* tdist() const { return (double*)(base + L().tdist()); }
    __device__ __forceinline__ int32_t* cur() const { return (int32_t*)(base + L().cur()); }
    __device__ __forceinline__ uint32_t* ainfo() const { return (uint32_t*)(base + L().ainfo()); }
    __device__ __forceinline__ double* ts() const { return (double*)(base + L().ts()); }
    __device__ __forceinline__ double* tf() const { return (double*)(base + L().tf()); }
    __device__ __forceinline__ double* marr() const { if constexpr (MG) return gm; else return (double*)(base + L().marr()); }
    __device__ __forceinline__ uint64_t* mids() const { return (uint64_t*)(base + L().mids() - MSH); }   // u64[IW][PT], word-major
    __device__ __forceinline__ Ids load_ids(int t) const { Ids x;
#pragma unroll
        for (int i = 0; i < IW; i++) x.w[i] = mids()[i * PT() + t];
        return x; }
    __device__ __forceinline__ void store_ids(int t, const Ids& x) const {
#pragma unroll
        for (int i = 0; i < IW; i++) mids()[i * PT() + t] = x.w[i]; }
    __device__ __forceinline__ uint32_t* tinfo() const { return (uint32_t*)(base + L().tinfo() - MSH); }
    __device__ __forceinline__ uint32_t* tnab() const { return (uint32_t*)(base + L().tnab() - MSH); }
    __device__ __forceinline__ double* tx() const { return (double*)(base + L().tx()); }
    __device__ __forceinline__ double* ty() const { return (double*)(base + L().ty()); }
    __device__ __forceinline__ double* tdur() const { return (double*)(base + (IRB ? L().tx() : L().tdur()) - MSH); }   // IRB image: no x / y sections
    __device__ __forceinline__ uint32_t aux_off() const { return (IRB ? L().tx() + 8u * (uint32_t)PT() : L().aux()) - MSH; }
    // (+ 4 T bytes of wake-up times, see task_update, for the layouts with more than one lane chunk of tasks)
    static __host__ __device__ constexpr uint32_t lds_image_bytes(Lay l) {
        return (IRB ? l.tx() + 8u * (uint32_t)l.T + 48u : l.lds_rec()) - MSH + ((CT == 0 || CT > WAVE) ? align16(4u * (uint32_t)l.T) : 0u);
    }
    // coordinates of task k (wave-uniform k): lane k & 63 of chunk k >> 6 holds them, or the LDS image does
    __device__ __forceinline__ void task_xy(int k, const XY& xy, double& x, double& y) const {
        if constexpr (IRB) {
            const int kc = k >> 6, kl = k & 63;
            x = 0.; y = 0.;
#pragma unroll
            for (int c = 0; c < NTC; c++) if (c == kc) {
                x = rl(xy.x[c], kl);
                y = rl(xy.y[c], kl);
            }
        } else { x = tx()[k]; y = ty()[k]; }
    }
    __device__ __forceinline__ double* tw() const { return (double*)(scr + L().s_tw()); }
    __device__ __forceinline__ double* aw() const { return (double*)(scr + L().s_aw()); }
    __device__ __forceinline__ uint16_t* absort() const { return (uint16_t*)(scr + L().s_absort()); }
    __device__ __forceinline__ double* terms() const { return (double*)(scr + L().s_terms()); }
    __device__ __forceinline__ unsigned long long* amask() const { return (unsigned long long*)(scr + L().s_amask()); }
    // this env's rows of the abandonment side table (pointer stashed in LDS by the kernel prologue: no SGPRs held)
    __device__ __forceinline__ uint16_t* ablog() const { return *(uint16_t* const*)(base + aux_off()); }
    __device__ __forceinline__ uint8_t* abcnt() const { return *(uint8_t* const*)(base + aux_off() + 16); }
    // (pitch_A / pitch_T = sizes the side tables are laid out for = the batch maximum; equal A() / T() unless the batch is
    //  ragged.  One workgroup per env: gridDim.x is the batch size, the count tables follow the logs of all envs.)
    __device__ __forceinline__ void set_ablog(uint16_t* table, int env_index, int pitch_A, int pitch_T, int lane) const {
        if (lane == 0) {
            *(uint16_t**)(base + aux_off()) = table + (size_t)env_index * pitch_A * AB_CAP;
            *(uint8_t**)(base + aux_off() + 16) = (uint8_t*)(table + (size_t)gridDim.x * pitch_A * AB_CAP) +
                                                  (size_t)env_index * abcnt_pitch(pitch_A, pitch_T);
        }
    }

    // record HBM -> LDS (base): every load in flight before the first LDS write when the layout is a compile-time constant
    // ALL = false: the plain chunk-by-chunk loop (4 VGPRs).  The persistent kernel copies its record once per launch of
    // hundreds of decisions, so the copy's latency is irrelevant there, while the 32 transient VGPRs of the all-in-flight copy
    // pushed k_rollout_random<64,64,runtime sizes> from 128 to 132 VGPRs = 3 instead of 4 waves per SIMD = two rounds of
    // workgroups for a 4096-env batch (5.7e8 instead of 8.1e8 steps/s at 21A/51T).
    template <bool NT = true, bool ALL = true>
    __device__ __forceinline__ void load_record(const unsigned char* rec, int lane, XY& xy) const {
        if constexpr (IRB) {
            constexpr Lay l{CA, CT};
#pragma unroll
            for (int c = 0; c < NTC; c++) {
                const int t = c * WAVE + lane < CT ? c * WAVE + lane : 0;
                xy.x[c] = ((const double*)(rec + l.tx()))[t];
                xy.y[c] = ((const double*)(rec + l.ty()))[t];
            }
            if constexpr (MG) {        // ... and the member arrival times stay where they are
                static_assert(l.marr() % 16 == 0 && l.mids() % 16 == 0 && MSH % 16 == 0, "16-byte copies");
                copy16_in(base, rec, l.marr(), lane);
                copy16_in(base + l.mids() - MSH, rec + l.mids(), l.mut_bytes() - l.mids(), lane);
                copy16_in(base + l.tx() - MSH, rec + l.tdur(), align16(8 * CT), lane);
            } else if constexpr (ALL) {       // mutable part, then the durations right behind it (the x / y sections are skipped)
                copy16_in_all<l.mut_bytes(), NT>(base, rec, lane);
                copy16_in_all<align16(8 * CT), NT>(base + l.tx(), rec + l.tdur(), lane);
            } else {
                copy16_in(base, rec, l.mut_bytes(), lane);
                copy16_in(base + l.tx(), rec + l.tdur(), align16(8 * CT), lane);
            }
        } else if constexpr (CA != 0 && !RL && ALL) copy16_in_all<Lay{CA, CT}.rec_bytes(), NT>(base, rec, lane);
        else copy16_in(base, rec, L().rec_bytes(), lane);
    }

    // mutable part of the LDS image -> HBM record
    __device__ __forceinline__ void store_record(unsigned char* rec, int lane) const {
        const Lay l = L();
        if constexpr (MG) {
            copy16(rec, base, l.marr(), lane);
            copy16(rec + l.mids(), base + l.mids() - MSH, l.mut_bytes() - l.mids(), lane);
        } else copy16(rec, base, l.mut_bytes(), lane);
    }
    // ... and back: the mutable part of a record image `img` that store_record wrote -> the LDS image (the lookahead form's restore;
    // the instance part of the LDS image stays).  MG: the member arrival times are not in LDS, see snapshot_marr / restore_marr.
    __device__ __forceinline__ void load_mutable(const unsigned char* img, int lane) const {
        const Lay l = L();
        if constexpr (MG) {
            copy16_in(base, img, l.marr(), lane);
            copy16_in(base + l.mids() - MSH, img + l.mids(), l.mut_bytes() - l.mids(), lane);
        } else copy16_in(base, img, l.mut_bytes(), lane);
    }
    // MG: the member arrival times live in the env's HBM record (gm): HBM -> HBM between the record and a record image
    __device__ __forceinline__ void snapshot_marr(unsigned char* img, int lane) const {
        if constexpr (MG) copy16_in(img + L().marr(), (const unsigned char*)gm, MSH, lane);
    }
    __device__ __forceinline__ void restore_marr(const unsigned char* img, int lane) const {
        if constexpr (MG) copy16_in((unsigned char*)gm, img + L().marr(), MSH, lane);
    }

    // optional return log (dcm_set_return_log): this env's ring of `cap` episode returns; pointer kept in the LDS image
    __device__ __forceinline__ void set_retlog(double* log, int cap, int env_index, int lane) const {
        if (lane == 0) {
            *(double**)(base + aux_off() + 32) = log ? log + (size_t)env_index * cap : nullptr;
            *(int32_t*)(base + aux_off() + 40) = cap;
        }
    }

    struct AMask { uint64_t w[NAW]; };
    __device__ __forceinline__ static int am_count(const AMask& m) { int n = 0;
#pragma unroll
        for (int i = 0; i < NAW; i++) n += __popcll(m.w[i]);
        return n; }
    __device__ __forceinline__ static bool am_test(const AMask& m, int a) {
        bool r = false;
#pragma unroll
        for (int i = 0; i < NAW; i++) if (i == (a >> 6)) r = (m.w[i] >> (a & 63)) & 1ull;
        return r; }
    __device__ __forceinline__ static void am_clear(AMask& m, int a) {
#pragma unroll
        for (int i = 0; i < NAW; i++) if (i == (a >> 6)) m.w[i] &= ~(1ull << (a & 63)); }
    __device__ __forceinline__ static void am_set(AMask& m, int a) {
#pragma unroll
        for (int i = 0; i < NAW; i++) if (i == (a >> 6)) m.w[i] |= (1ull << (a & 63)); }
    __device__ __forceinline__ static int am_nth(const AMask& m, int idx, int lane) {
        if constexpr (NAW == 1) return nth(m.w[0], idx);
        int b = 0, res = -1;
#pragma unroll
        for (int i = 0; i < NAW; i++) {
            const int c = __popcll(m.w[i]);
            const int p = nth(m.w[i], idx - b);
            if (res < 0 && idx - b >= 0 && idx - b < c) res = i * 64 + p;
            b += c;
        }
        return res; }
    // agents whose pending group id equals g
    __device__ __forceinline__ AMask group_mask(int g, int lane) const {
        AMask m;
#pragma unroll
        for (int i = 0; i < NAW; i++) {
            const int a = i * 64 + lane;
            const uint32_t ai = ainfo()[a < A() ? a : 0];
            m.w[i] = __ballot((a < A()) && (int)((ai >> 8) & 0xFFu) == g);
        }
        return m; }

    // ------------------------------------------------------------------------------ task_update
    // env/task_env.py:245-281.  Lanes stride over tasks; each lane holds its task's <=M ordered member
    // arrivals in registers.  status = requirements - len(members) is the coalition capability-vs-
    // requirement reduction.  Straight-line predicated code; the member-removal compaction is the only
    // (rare) divergent branch.
    //
    // Incremental mode (shapes with more than one lane pass over the tasks, persistent kernel only): `only` names the task
    // the deciding agents have just joined (-2: they went to the depot, -1: every task).  At an unchanged `now` a second
    // call can only change a task whose member list was touched or that became feasible in the previous call (a
    // Q1-skipped member, the stale status after the spread branch, `finished` of a freshly feasible task :273), so when
    // the call only revisits the 64-task lane chunks the previous call touched (bitmask in inc_state()[1]) plus the chunk
    // of `only`; every other task is at a fixed point of task_update.  inc_state()[0] carries the number of infeasible
    // tasks for np.all(feasible) :279.
    // only == -3: the call of a NEW event (advance(): `now` has moved, no agent_step in between).  With the time alone a task that
    // was at a fixed point changes in two ways only: a feasible one finishes (now >= time_finish :273), or the earliest member of
    // an infeasible one has waited max_waiting_time (now - arrival >= mwt :269; also a member the rounding of that expression
    // left listed when its agent moved on).  Every visit of a task therefore leaves the time of its next possible change --
    // time_finish, or min(arrival) + mwt, +inf if neither applies, -inf if the visit itself removed members -- rounded DOWN to
    // fp32 (a margin of 1e-7 relative, far above the rounding of the two fp64 expressions) in wake()[t], an LDS-only array behind
    // the record image; the call of a new event compares `now` with it and visits the lane chunks with a due task plus those the
    // previous call touched, instead of all of them (one or two of the four at 50A/200T).  tools/inc_selfcheck.py dry-runs
    // every skipped task.
    static constexpr bool INC = (CT == 0 || CT > WAVE);
    __device__ __forceinline__ int32_t* inc_state() const { return (int32_t*)(base + aux_off() + 8); }
    __device__ __forceinline__ float* wake() const { return (float*)(base + aux_off() + 48); }    // f32[PT], INC kernels only
    // k_step only: which task sections this call has written (bit 0 time_start / time_finish, bits 1..MC member-arrival row j,
    // bit 20 member ids, bit 21 abandonment counts), so that the write-back can skip the rest (DIRTY_ALL after a reset)
    static_assert(MC + 1 < 20, "dirty mask: bits 1..MC are the arrival rows, 20 / 21 the ids / abandonment counts");
    static constexpr uint32_t DIRTY_TIMES = 1u, DIRTY_ROWS = ((1u << MC) - 1u) << 1, DIRTY_IDS = 1u << 20, DIRTY_NAB = 1u << 21,
                              DIRTY_ALL = DIRTY_TIMES | DIRTY_ROWS | DIRTY_IDS | DIRTY_NAB;
    static constexpr uint32_t DIRTY_TASK_SHIFT = 22;   // bits 22..31: the joined task (T <= 1023), valid while IDS is set and NAB is not
    static_assert(DCM_MAX_TASKS < (1 << (32 - 22)), "the joined task must fit the dirty word");
    __device__ __forceinline__ uint32_t* dirty() const { return (uint32_t*)(base + aux_off() + 24); }
    // second tracking word (lockstep kernels): bits 24..31 = how many tasks became feasible in this step, bits 0..23 = the sum of
    // their ids -- i.e. THE task when the count is 1 (the common case), so that the write-back can send its 64-byte pieces of
    // time_start / time_finish instead of the two sections
    __device__ __forceinline__ uint32_t* dirty2() const { return (uint32_t*)(base + aux_off() + 28); }
    __device__ __forceinline__ void task_update(const HdrRegs& h, const KP& P, int lane, int only = -1, bool track = false) const {
        const double now = h.now, mwt = P.mwt;
        const int T_ = T(), PT_ = PT();
        bool allf = true, touched = false;
        auto one = [&](int t) {
            uint32_t info = tinfo()[t];
            const bool feas0 = info & T_FEAS;
            const int req = info & 0xFF;
            const int n = (info >> 16) & 0xFF;                               // :250
            // Unused slots (j >= n) hold NaN in LDS (reset / compaction keep that invariant): v_max/v_min ignore
            // them and every comparison against them is false, so no per-slot validity predicate is needed.
            double av[MC];
#pragma unroll
            for (int j = 0; j < MC; j++) av[j] = marr()[j * PT_ + t];        // :251
            const double tfin = tf()[t], dur = tdur()[t];
            const int status = req - n;                                      // :252
            double mx = av[0], mn = av[0];
#pragma unroll
            for (int j = 1; j < MC; j++) { mx = nanmax2(mx, av[j]); mn = nanmin2(mn, av[j]); }
            const bool le0 = status <= 0;                                    // :254
            const bool ok = le0 && (mx - mn <= mwt);                         // :255
            const double thr = mx - mwt;                                     // :262
            // Does any member leave?  Spread branch (:262): some av[j] <= thr  <=>  mn <= thr.  Waiting branch (:269): some
            // now - av[j] >= mwt  <=>  now - mn >= mwt (fp subtraction and comparison are monotone in av[j]; the first
            // expired member is never skipped by Q1).  NaN (no members) makes both false.  The per-slot masks are only
            // built inside this rare divergent branch.
            const bool any_drop = !feas0 && (le0 ? (!ok && mn <= thr) : (now - mn >= mwt));
            if (!feas0) {
                if (ok) { ts()[t] = mx; tf()[t] = mx + dur; info |= T_FEAS; if (track) { atomicOr(dirty(), DIRTY_TIMES); atomicAdd(dirty2(), (1u << 24) | (uint32_t)t); } }  // :256-258
                int nn = n;
                if (any_drop) {  // rare: compact the surviving members in order
                    uint32_t spread = 0, q1 = 0;
                    bool prev = false;
#pragma unroll
                    for (int j = 0; j < MC; j++) {
                        spread |= (av[j] <= thr) ? (1u << j) : 0u;           // :262-265
                        // :268-271 iterates task['members'] while removing from it: after a removal the element
                        // that slides into the freed slot is skipped by the list iterator (quirk Q1).
                        const bool e = !prev && (now - av[j] >= mwt);        // :269
                        q1 |= e ? (1u << j) : 0u;
                        prev = e;
                    }
                    const uint32_t drop = le0 ? spread : q1;
                    const Ids ids = load_ids(t);
                    Ids nids{};
                    int k = 0;
#pragma unroll
                    for (int j = 0; j < MC; j++) if (j < n) {
                        const uint32_t id = ids.byte(j);
                        if (drop & (1u << j)) {
                            // abandoned_agent.append(member) :265/:271; the agent stops being listed at `t`
                            const uint32_t nth = atomicAdd(&ainfo()[id], 1u << 16) >> 16;
                            if (nth < (uint32_t)AB_CAP) ablog()[id * AB_CAP + nth] = (uint16_t)t;
                            else { const uint32_t ci = (uint32_t)(id * T_ + t); atomicAdd((uint32_t*)abcnt() + (ci >> 1), 1u << (16 * (ci & 1))); }
                            if (cur()[id] == t) atomicAnd(&ainfo()[id], ~A_MEMBER);
                        } else {
                            nids.put(k, id);
                            marr()[k * PT_ + t] = av[j];
                            k++;
                        }
                    }
                    for (int j = k; j < n; j++) marr()[j * PT_ + t] = __builtin_nan("");  // vacated slots
                    store_ids(t, nids);
                    tnab()[t] += (uint32_t)(n - k);
                    nn = k;
                    if (track) atomicOr(dirty(), DIRTY_ALL & ~DIRTY_TIMES);   // slots compacted: every arrival row, ids, counts
                }
                info = (info & (T_FEAS | T_FIN | 0xFFu)) | ((uint32_t)(status & 0xFF) << 8) | ((uint32_t)nn << 16);
            } else {
                info |= (now >= tfin) ? T_FIN : 0u;                          // :273-274
            }
            tinfo()[t] = info;
            if constexpr (INC) {
                // when can the time alone change this task next?  (mn: the earliest listed arrival; NaN without members)
                double w = (info & T_FEAS) ? ((info & T_FIN) ? __builtin_inf() : (feas0 ? tfin : mx + dur)) : mn + mwt;
                w = (w == w) ? w : __builtin_inf();
                wake()[t] = any_drop ? -__builtin_inff() : __double2float_rd(w);
            }
            allf = allf && (info & T_FEAS);
            // a freshly feasible task only changes again at this `now` if it is already over (finished is evaluated one
            // call later, :273): now >= time_finish needs zero duration and every member already there
            touched = touched || any_drop || (!feas0 && ok && now >= mx + dur);
        };
        bool all_feasible;
        if constexpr (!INC) {
            for_tasks(lane, one);
            all_feasible = __all(allf);
        } else {
            // st[0] = number of infeasible tasks, st[1] = lane-chunk bitmask of the tasks the previous call touched
            int32_t* st = inc_state();
            const uint32_t nchunk = (uint32_t)(T_ + WAVE - 1) / WAVE, all = nchunk >= 32 ? ~0u : ((1u << nchunk) - 1u);
            uint32_t todo = all;
            if (only == -3 && T_ > WAVE) {
                uint32_t cand = 0;
                for (uint32_t ch = 0; ch < nchunk; ch++) {
                    const int t = (int)(ch * WAVE) + lane;
                    cand |= __ballot(t < T_ && now >= (double)wake()[t < T_ ? t : 0]) ? (1u << ch) : 0u;
                }
                todo = ((uint32_t)uni(st[1]) | cand) & all;
            } else if (only != -1 && only != -3 && T_ > WAVE) {
                todo = ((uint32_t)uni(st[1]) | (only >= 0 ? (1u << (only >> 6)) : 0u)) & all;
            }
            const bool full = todo == all;
            int n_infeas = full ? 0 : uni(st[0]);
            uint32_t dirty = 0;
#ifdef DCM_INC_DEBUG   // developer self-check of the chunk skipping (tools/inc_selfcheck.py); never in the product build
#include "../../tools/inc_selfcheck.inc"
#endif
            for (uint32_t c = 0; c < nchunk; c++) {                            // uniform trip count and branch: ballots inside
                if (!((todo >> c) & 1u)) continue;
                const int t = (int)(c * WAVE) + lane;
                allf = true; touched = false;
                bool was_infeasible = false;
                if (t < T_) { was_infeasible = !(tinfo()[t] & T_FEAS); one(t); }
                if (full) n_infeas += __popcll(__ballot(!allf));
                else n_infeas -= __popcll(__ballot(was_infeasible && allf));    // became feasible in this call
                if (__any(touched)) dirty |= 1u << c;
            }
            if (lane == 0) { st[0] = n_infeas; st[1] = (int32_t)dirty; }
            all_feasible = n_infeas == 0;
        }
        WSYNC();
        // depot :277-280 (np.all(feasible) is wave-uniform and false until the last task is feasible: nothing to scan before)
        if (all_feasible) {
            for_agents(lane, [&](int a) {
                const uint32_t ai = ainfo()[a];
                if ((ai & A_INDEPOT) && now >= arr()[a]) ainfo()[a] = ai | A_RETURNED;
            });
        }
    }

    // ------------------------------------------------------------------------------ agent_update
    // env/task_env.py:207-243 (non-reactive branch :226).  `agent in current_task['members']` (:230) is the
    // cached A_MEMBER bit (set by agent_step, cleared when task_update drops the agent from that task).
    __device__ __forceinline__ void agent_update(const HdrRegs& h, const KP& P, int lane) const {
        const double now = h.now;
        for_agents(lane, [&](int a) {
            const int c = cur()[a];
            const int K = c < 0 ? 0 : c;
            const uint32_t info = tinfo()[K];                                 // :228
            const double tfK = tf()[K], tsK = ts()[K], av = arr()[a];
            uint32_t ai = ainfo()[a];
            const bool member = (info & T_FEAS) && (ai & A_MEMBER);          // :229-230
            const double ndv = (c == -1) ? __builtin_nan("") : (member ? tfK : av + P.mwt);  // :226,:231,:235,:238
            const uint32_t as = member ? ((ai & A_ASSIGNED) | ((now >= tsK) ? A_ASSIGNED : 0u)) : 0u;  // :232-240
            if (c != -2) {                                                   // :209
                nd()[a] = ndv;
                if (c >= 0) ainfo()[a] = (ai & ~A_ASSIGNED) | as;            // depot leaves `assigned` untouched (Q6)
            }
        });
    }

    // ------------------------------------------------------------------------------ terminal
    // calculate_waiting_time (env/task_env.py:344-364) into LDS scratch tw[T], aw[A].
    // Returns true when a per-(agent, task) abandonment counter saturated (DCM_FLAG_WAIT_ORDER; the only inexact case).
    //
    // The per-task sums are one lane pass.  The per-agent sums (:358-364) must be accumulated in the reference's order -- tasks
    // ascending; for each task first the member term, then +max_waiting_time once per entry of the agent in that task's
    // abandoned_agent list -- a serial fp64 chain per agent.  The walking code does that literally: per agent a bitmask of the
    // tasks that list it, the agent looked up in each of them (status word, id word, arrival slot, the task's latest arrival: a
    // dependent chain of LDS round trips per task), merged with its abandonment entries sorted in place.
    // When the scratch is in LDS (the one-chunk kernels) everything but the additions is taken out of the serial part: a second
    // lane pass over the TASKS writes every member's term to its place in the agent's list (place = the number of lower tasks that
    // list the agent) together with the number of the agent's abandonment entries that belong to lower tasks (its row of the side
    // table is requested from HBM before the first pass), and the agent lane reads its list front to back and adds.  Measured on
    // the wave that ends a 20A/50T episode (s_memrealtime marks): 10.0 -> 6.4 us for the whole terminal call -- and that wave is
    // the slowest wave of a lockstep launch.  An agent listed by more than list_cap tasks or with more than eight abandonments
    // takes the walking code.
    __device__ bool compute_waits(double now, double mwt, int lane) const {
        const int T_ = T(), A_ = A(), PT_ = PT();
        const int TW = (int)L().twords();
        const int LC = (int)L().list_cap();
        // (compiled only into the simulators whose scratch can be in LDS: the code's mere presence in the out-of-line function costs the
        //  general k_step of the mid-size class 2 us per launch -- registers it clobbers are registers the caller cannot keep live)
        const bool gather = SCR_IN_LDS && uni((uint32_t)in_lds(scr)) != 0u && A_ <= WAVE && LC >= 1 && LC <= 16;
#ifdef DCM_PROFILE_PHASES
        const unsigned long long pt0 = __builtin_readcyclecounter();
#endif
        uint4 row{0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};       // this lane's agent: its first eight abandonment entries
        if (gather && lane < A_) {
            // (agent-scope loads, past the CU's vector L1: the row was written by this wave's own removal path, possibly after an
            //  earlier terminal call of the same launch had read -- and cached -- the line; the same rule as replay_fast.hpp's gload)
            const unsigned long long* q = (const unsigned long long*)(ablog() + lane * AB_CAP);
            const unsigned long long lo = __hip_atomic_load(q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const unsigned long long hi = __hip_atomic_load(q + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            row = uint4{(uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32)};
        }
        for (int i = lane; i < A_ * TW; i += WAVE) amask()[i] = 0ull;         // per agent: bitmask of the tasks listing it
        WSYNC();
        for_tasks(lane, [&](int t) {
            const uint32_t info = tinfo()[t];
            const int n = (info >> 16) & 0xFF;
            const double ab = (double)tnab()[t] * mwt;
            // all M member slots are read back to back (unused ones hold NaN, which v_max_f64 ignores) instead of walking
            // the n valid ones with one LDS round trip each
            double av[MC];
#pragma unroll
            for (int j = 0; j < MC; j++) av[j] = marr()[j * PT_ + t];
            double mx = av[0];
#pragma unroll
            for (int j = 1; j < MC; j++) mx = nanmax2(mx, av[j]);            // np.max(arrival) :350
            mx = n ? mx : 0.;
            const bool feas = info & T_FEAS;
            double s = 0., term[MC];
#pragma unroll
            for (int j = 0; j < MC; j++) { term[j] = feas ? mx - av[j] : now - av[j]; s = (j < n) ? s + term[j] : s; }   // :351 / :354
            if constexpr (MC >= 8) {   // np.sum of eight or more terms is numpy's unrolled pairwise block, not a running sum
                if (n >= 8) {
                    double r8[8];
#pragma unroll
                    for (int j = 0; j < 8; j++) r8[j] = term[j];
                    if constexpr (MC >= 16) { if (n >= 16) {
#pragma unroll
                        for (int j = 0; j < 8; j++) r8[j] += term[8 + j]; } }
                    s = ((r8[0] + r8[1]) + (r8[2] + r8[3])) + ((r8[4] + r8[5]) + (r8[6] + r8[7]));
                    const int nb = n - (n % 8);
#pragma unroll
                    for (int j = 8; j < MC; j++) s = (j >= nb && j < n) ? s + term[j] : s;
                }
            }
            tw()[t] = s + ab;                                                // :351-357
            if (!gather) terms()[t] = mx;                                    // np.max(arrival), reused per agent by the walking code
            const Ids ids = load_ids(t);
            for (int j = 0; j < n; j++)                                      // transpose members -> per-agent task set
                atomicOr(&amask()[(int)ids.byte(j) * TW + (t >> 6)], 1ull << (t & 63));
        });
        uint32_t nab0 = 0;                                                   // this lane's agent: its number of abandonments
        if (gather && lane < A_) {
            // the agent's entries where the task lanes of the second pass find them; entries it does not have become 0xFFFF
            nab0 = ainfo()[lane] >> 16;
            auto pad = [&](uint32_t v, uint32_t k) { return (k < nab0 ? (v & 0xFFFFu) : 0xFFFFu) | (k + 1u < nab0 ? (v & 0xFFFF0000u) : 0xFFFF0000u); };
            *(uint4*)(absort() + lane * AB_CAP) = uint4{pad(row.x, 0u), pad(row.y, 2u), pad(row.z, 4u), pad(row.w, 6u)};
        }
        WSYNC();
        // the member term of agent a in task tm (:360 / :362), looked up
        auto member_term = [&](int a, int tm) {
            const uint32_t info = tinfo()[tm];
            const int n = (info >> 16) & 0xFF;
            const int pos = load_ids(tm).find((uint32_t)a, n);
            const double mine = marr()[pos * PT_ + tm];
            double mx;                                                       // np.max(arrival) :350
            if (gather) {                                                    // (the lists occupy the scratch the first pass would keep it in)
                mx = marr()[tm];
                for (int j = 1; j < MC; j++) mx = nanmax2(mx, marr()[j * PT_ + tm]);
            } else mx = terms()[tm];
            const double wv = now - mine;
            return (info & T_FEAS) ? (mx - mine) : ((wv > 0.) ? wv : 0.);
        };
        bool walk = lane < A_;                                               // this lane's agent still needs the walking code
        if (gather) {
            // (LDS-typed pointers: this function is out of line and sees `base` / `scr` as generic pointers -- flat instructions,
            //  64-bit addresses; here both are known to be LDS)
            typedef __attribute__((address_space(3))) unsigned char* lds_p;
            const lds_p lscr = (lds_p)scr, limg = (lds_p)base;
            auto* const l_amask = (__attribute__((address_space(3))) unsigned long long*)(lscr + L().s_amask());
            auto* const l_terms = (__attribute__((address_space(3))) double*)(lscr + L().s_terms());
            const lds_p l_rows = lscr + L().s_absort();                      // per agent 32 B: eight entries, sixteen count bytes
            auto* const l_marr = (__attribute__((address_space(3))) const double*)(limg + L().marr() - MSH);
            auto* const l_tinfo = (__attribute__((address_space(3))) const uint32_t*)(limg + L().tinfo() - MSH);
            // every member's term to its place in the agent's list, and with it the number of the agent's abandonment entries that
            // belong to lower tasks (the +max_waiting_time additions that precede the term)
            for_tasks(lane, [&](int t) {
                const uint32_t info = l_tinfo[t];
                const int n = (info >> 16) & 0xFF;
                const bool feas = info & T_FEAS;
                double av[MC];
#pragma unroll
                for (int j = 0; j < MC; j++) av[j] = l_marr[j * PT_ + t];
                double mx = av[0];
#pragma unroll
                for (int j = 1; j < MC; j++) mx = nanmax2(mx, av[j]);
                const Ids ids = load_ids(t);
                const int w = t >> 6;
                const uint64_t below = (1ull << (t & 63)) - 1ull;
                const uint32_t tt = (uint32_t)t;
#pragma unroll
                for (int j = 0; j < MC; j++) {
                    if (j < n) {
                        const int a = (int)ids.byte(j);
                        int place = __popcll(l_amask[a * TW + w] & below);
                        for (int w2 = 0; w2 < w; w2++) place += __popcll(l_amask[a * TW + w2]);
                        auto* const ev = (const __attribute__((address_space(3))) uint32_t*)(l_rows + a * (2 * AB_CAP));   // (0xFFFF: no entry)
                        const uint32_t e0 = ev[0], e1 = ev[1], e2 = ev[2], e3 = ev[3];
                        const uint32_t before = (uint32_t)((e0 & 0xFFFFu) < tt) + (uint32_t)((e0 >> 16) < tt) + (uint32_t)((e1 & 0xFFFFu) < tt) +
                                                (uint32_t)((e1 >> 16) < tt) + (uint32_t)((e2 & 0xFFFFu) < tt) + (uint32_t)((e2 >> 16) < tt) +
                                                (uint32_t)((e3 & 0xFFFFu) < tt) + (uint32_t)((e3 >> 16) < tt);
                        const double wv = now - av[j];
                        if (place < LC) {
                            l_terms[a * LC + place] = feas ? (mx - av[j]) : ((wv > 0.) ? wv : 0.);
                            (l_rows + a * (2 * AB_CAP) + 16)[place] = (unsigned char)before;
                        }
                    }
                }
            });
            WSYNC();
            if (lane < A_) {
                const int a = lane;
                int cnt = 0;
                for (int w = 0; w < TW; w++) cnt += __popcll(l_amask[a * TW + w]);
                if (cnt <= LC && nab0 <= 8u) {
                    walk = false;
                    // the list front to back (four terms requested at a time): before each term the entries of lower tasks that
                    // have not been added yet (:363-364), then the term (:360 / :362); the remaining entries at the end
                    auto* const bv = (const __attribute__((address_space(3))) uint32_t*)(l_rows + a * (2 * AB_CAP) + 16);
                    const uint32_t bw[4] = {bv[0], bv[1], bv[2], bv[3]};
                    auto* const mine = l_terms + a * LC;
                    double s = 0.;
                    int done = 0;
#pragma unroll
                    for (int c = 0; c < 4; c++) {
                        if (4 * c < cnt) {
                            double v[4];
#pragma unroll
                            for (int k = 0; k < 4; k++) v[k] = mine[(4 * c + k < cnt) ? 4 * c + k : 0];
#pragma unroll
                            for (int k = 0; k < 4; k++) {
                                if (4 * c + k < cnt) {
                                    const int before = (int)((bw[c] >> (8 * k)) & 0xFFu);
                                    for (; done < before; done++) s += mwt;
                                    s += v[k];
                                }
                            }
                        }
                    }
                    for (; done < (int)nab0; done++) s += mwt;
                    aw()[a] = s;
                }
            }
        }
#ifdef DCM_PROFILE_PHASES
        const unsigned long long pt1 = __builtin_readcyclecounter();
        if (lane == 0) atomicAdd(&g_phase_cycles[12], pt1 - pt0);
#endif
        bool over = false;
        if (!gather || __any(walk)) {
            // the walking code.  The abandonment entries come from the log (event order), sorted here by task id; entries beyond
            // AB_CAP per episode (never seen) are in the dense count table.
            {   // bring this env's rows of the side table (A x 32 B, contiguous) into LDS with one coalesced pass
                const uint4* src = (const uint4*)ablog();
                uint4* dst = (uint4*)absort();
                for (int i = lane; i < A_ * AB_CAP * 2 / 16; i += WAVE) dst[i] = src[i];
            }
            WSYNC();
            for (int a = lane; a < A_; a += WAVE) {
                if (gather && !walk) continue;
                const uint32_t nab = ainfo()[a] >> 16;
                const int nl = nab < (uint32_t)AB_CAP ? (int)nab : AB_CAP;
                uint16_t* my = absort() + a * AB_CAP;
                for (int i = 1; i < nl; i++) {                               // in-place insertion sort by task id
                    const uint16_t v = my[i];
                    int j = i;
                    while (j > 0 && my[j - 1] > v) { my[j] = my[j - 1]; j--; }
                    my[j] = v;
                }
                double s = 0.;
                if (nab <= (uint32_t)AB_CAP) {
                    // merge, in ascending task id, the tasks that list the agent (member term) with its abandonment entries
                    int p = 0;
                    for (int w = 0; w < TW; w++) {
                        uint64_t m = amask()[a * TW + w];
                        const int wend = (w + 1) * 64;
                        for (;;) {
                            const int tm = m ? (w * 64 + __ffsll((unsigned long long)m) - 1) : wend;
                            if (p < nl && (int)my[p] < tm) { s += mwt; p++; continue; }   // :363-364 of an earlier task
                            if (!m) break;
                            m &= m - 1;
                            s += member_term(a, tm);
                        }
                    }
                } else {
                    // the log overflowed: this agent from the dense count table, tasks ascending, member term first and then
                    // one +max_waiting_time per abandonment by that task (:358-364), exact for any number of abandonments
                    const uint16_t* cnt16 = (const uint16_t*)abcnt() + a * T_;   // abandonments beyond the first AB_CAP (those are in `my`, sorted)
                    int q = 0;
                    for (int t = 0; t < T_; t++) {
                        if ((amask()[a * TW + (t >> 6)] >> (t & 63)) & 1ull) s += member_term(a, t);
                        int c = cnt16[t];
                        over = over || c == 65535;                            // saturated counter: the only inexact case left
                        while (q < nl && my[q] == (uint16_t)t) { c++; q++; }
                        for (int k = 0; k < c; k++) s += mwt;
                    }
                }
                aw()[a] = s;
            }
        }
#ifdef DCM_PROFILE_PHASES
        if (lane == 0) atomicAdd(&g_phase_cycles[13], __builtin_readcyclecounter() - pt1);
#endif
        WSYNC();
        return __any(over);
    }

    // get_episode_reward + perf metrics (env/task_env.py:420-425, worker.py:87,103-108) -> row[8]
    // (header fields are passed by value: a by-reference Hdr would force the caller's header into scratch memory)
    // (called out of line through a by-VALUE copy of the simulator: a noinline member function would take `this`, which
    //  forces the Sim object -- and with it 64 bytes of scratch memory per lane and two scratch stores in every kernel
    //  prologue -- into memory)
    __device__ __noinline__ static bool terminal_metrics(Sim S, double now, double mwt, int lane, double* __restrict__ row) {
        return S.terminal_metrics_body(now, mwt, lane, row);
    }
    __device__ __forceinline__ bool terminal_metrics_body(double now, double mwt, int lane, double* __restrict__ row) const {
        WSYNC();
        const bool over = compute_waits(now, mwt, lane);
        const int T_ = T(), A_ = A();
        int nfin = 0;
        for (int t0 = 0; t0 < T_; t0 += WAVE) {
            const int t = t0 + lane;
            nfin += __popcll(__ballot(t < T_ && (tinfo()[t < T_ ? t : 0] & T_FIN)));
        }
        // :422 check_finished() once more can only re-assign the same `now`
#ifdef DCM_PROFILE_PHASES
        const unsigned long long pt2 = __builtin_readcyclecounter();
#endif
        const double Td = (double)T_, Ad = (double)A_;
        // (numpy's pairwise sum is a single block up to 128 elements: always for agents, A <= DCM_MAX_AGENTS = 128, and for
        //  tasks whenever the layout bounds T by 128)
        double m2, m3, m4, m5;
        if constexpr (CT != 0 && CT <= 128) {
            // the four sums at once, eight lanes each: lane j of a group owns numpy's accumulator r[j] (np.add.reduce's
            // unrolled block loop), the three xor-exchanges form ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)) -- fp addition is
            // commutative, so every lane of the group ends with the same bits -- and the tail elements are added last
            const int g = (lane >> 3) & 3, j = lane & 7;
            const double* arr4 = g == 0 ? ts() : g == 1 ? aw() : g == 2 ? tdist() : tw();
            const int n = (g == 0 || g == 3) ? T_ : A_;
            double r;
            if (n < 8) {
                r = 0.;
                for (int i = 0; i < n; i++) r += arr4[i];
            } else {
                const int nb = n - (n % 8);
                r = arr4[j];
                for (int i = 8 + j; i < nb; i += 8) r += arr4[i];
                r += __shfl_xor(r, 1);
                r += __shfl_xor(r, 2);
                r += __shfl_xor(r, 4);
                for (int i = nb; i < n; i++) r += arr4[i];
            }
            m2 = rl(r, 0) / Td;                        // np.nanmean(time_start)      worker.py:105
            m3 = rl(r, 8) / Ad;                        // np.mean(agent sum_waiting)  :106
            m4 = rl(r, 16);                            // np.sum(travel_dist)         :107
            m5 = rl(r, 24) / Td;                       // np.mean(task sum_waiting)   :108
        } else {
            m2 = psum<4>(ts(), T_) / Td;
            m3 = psum_block(aw(), A_) / Ad;
            m4 = psum_block(tdist(), A_);
            m5 = psum<4>(tw(), T_) / Td;
        }
#ifdef DCM_PROFILE_PHASES
        if (lane == 0) atomicAdd(&g_phase_cycles[14], __builtin_readcyclecounter() - pt2);
#endif
        if (lane == 0 && row) {
            row[0] = -now;                             // reward, env/task_env.py:424
            row[1] = (double)nfin;
            row[2] = (double)nfin / Td;                // success_rate :103
            row[3] = now;                              // makespan :104
            row[4] = m2; row[5] = m3; row[6] = m4; row[7] = m5;
        }
        return over;
    }
    __device__ __forceinline__ void terminal(HdrRegs& h, const KP& P, int lane, double* __restrict__ row) const {
#ifdef DCM_PROFILE_PHASES
        const unsigned long long pt = __builtin_readcyclecounter();
#endif
        // (the out-of-line call returns in a VGPR: without the readfirstlane the compiler treats h.flags -- and with it every loop
        //  the flags control -- as divergent, and turns the kernels' scalar branches into exec-mask bookkeeping)
        const bool over = uni((uint32_t)terminal_metrics(*this, h.now, P.mwt, lane, row)) != 0u;
#ifdef DCM_PROFILE_PHASES
        if (lane == 0) atomicAdd(&g_phase_cycles[15], __builtin_readcyclecounter() - pt);
#endif
        h.flags |= DCM_FLAG_DONE | (over ? DCM_FLAG_WAIT_ORDER : 0u);
        if (lane == 0) {                              // cold header fields stay in the LDS record
            const uint32_t n = ((Hdr*)base)->episodes;
            ((Hdr*)base)->episodes = n + 1;
            double* ring = *(double* const*)(base + aux_off() + 32);          // dcm_set_return_log
            if (ring) ring[n % (uint32_t)*(const int32_t*)(base + aux_off() + 40)] = -h.now;   // reward, env/task_env.py:424
        }
        h.cur_group = 0;
    }

    // The end of an INNER episode of the lookahead form (k_la_*): the episode is over and nothing else happens -- no metrics, no
    // summary row, no episode count, no return log.  Its value is read off the state: (finished tasks, -now), which is what
    // terminal_metrics would have put into entries 1 and 0 of the row.
    __device__ __forceinline__ void terminal_inner(HdrRegs& h) const {
        h.flags |= DCM_FLAG_DONE;
        h.cur_group = 0;
    }

    // What terminal() does without the metrics (k_step_fast with a snapshot buffer, see dcm_env::side): the caller parks the record,
    // k_terminal_flush computes reward + metrics from it later.  The informational WAIT_ORDER flag is not kept: the env restarts
    // in this very launch, which clears the flags anyway.
    static constexpr uint32_t FLAG_DEFERRED = 1u << 30;      // internal, never stored in a record
    __device__ __forceinline__ void terminal_deferred(HdrRegs& h, int lane) const {
        h.flags |= DCM_FLAG_DONE | FLAG_DEFERRED;
        if (lane == 0) {
            const uint32_t n = ((Hdr*)base)->episodes;
            ((Hdr*)base)->episodes = n + 1;
            double* ring = *(double* const*)(base + aux_off() + 32);          // dcm_set_return_log
            if (ring) ring[n % (uint32_t)*(const int32_t*)(base + aux_off() + 40)] = -h.now;   // reward, env/task_env.py:424
        }
        h.cur_group = 0;
    }

    // ------------------------------------------------------------------------------ event loop
    // Boxes D + A of SURVEY.md Appendix B: check_finished (worker.py:85, env/task_env.py:366-373), loop test
    // (worker.py:45), next_decision (:283-289), get_unique_group (:291-298), task_update, agent_update
    // (worker.py:50-51).  Returns at the next decision point or after terminal().
    // no_grouping: every deciding agent forms ONE group (individual selection, worker.py:159-198 iterates the deciders without
    // get_unique_group); lockstep API only.
    // INNER: an inner episode of the lookahead form, which ends in terminal_inner.
    template <bool INNER = false>
    __device__ __forceinline__ void advance(HdrRegs& h, const KP& P, int lane, double* __restrict__ row PH_ARGS,
                                            bool no_grouping = false, bool track = false, bool defer = false) const {
        const int A_ = A();
        for (;;) {
            WSYNC();
            // ---- D: check_finished.  np.nanmin over next_decision (:287)
            double ndv[NAW];
            double lmin = __builtin_nan("");
#pragma unroll
            for (int i = 0; i < NAW; i++) {
                const int a = i * 64 + lane;
                ndv[i] = (a < A_) ? nd()[a] : __builtin_nan("");
                lmin = nanmin2(lmin, ndv[i]);
            }
            const double tmin = wave_nanmin(lmin);
            const bool any = (tmin == tmin);
            bool finished = false;
            if (!any) {                                                       // :368 nobody can decide any more
                double maxarr = 0.0;
                bool allret = true;
                for_agents(lane, [&](int a) {
                    const double av = (cur()[a] != -2) ? arr()[a] : 0.0;     // max(arrival_time) or 0 :286
                    maxarr = av > maxarr ? av : maxarr;
                    allret = allret && (ainfo()[a] & A_RETURNED);
                });
                // max over the WHOLE arrival lists (:286): the agents' last arrivals, and -- for lists that a masked action made
                // non-monotone -- the running maximum of the episode kept in the header
                const double hmax = uni(((const Hdr*)base)->max_arrival);
                const double lmax = wave_nanmax(maxarr);
                h.now = lmax > hmax ? lmax : hmax;                            // :369
                bool allfin = true;
                for_tasks(lane, [&](int t) { allfin = allfin && (tinfo()[t] & T_FIN); });
                finished = __all(allret) && __all(allfin);                   // :370
            }
            if (finished) h.flags |= DCM_FLAG_FINISHED;
            if (finished || h.now >= P.max_time) {                           // worker.py:45
                if constexpr (INNER) terminal_inner(h);
                else if (defer) terminal_deferred(h, lane); else terminal(h, P, lane, row);
                return;
            }
            // ---- A: new event
            h.n_groups = 0;
            if (any) {
                h.now = tmin;                                                 // worker.py:49
                bool dec[NAW];
                uint64_t dm[NAW];
#pragma unroll
                for (int i = 0; i < NAW; i++) { dec[i] = (ndv[i] == tmin); dm[i] = __ballot(dec[i]); }  // :288 exact ==
                int first = -1;
#pragma unroll
                for (int i = NAW - 1; i >= 0; i--) if (dm[i]) first = i * 64 + __ffsll((unsigned long long)dm[i]) - 1;
                // fast paths: a single deciding agent, or every deciding agent on the same point -> one group
                int ndec = 0;
#pragma unroll
                for (int i = 0; i < NAW; i++) ndec += __popcll(dm[i]);
                bool same = true;
                double px[NAW], py[NAW];
                if (ndec > 1 && !no_grouping)
                {
                    const double x0 = ax()[first], y0 = ay()[first];
#pragma unroll
                    for (int i = 0; i < NAW; i++) {
                        const int a = i * 64 + lane;
                        px[i] = ax()[a < A_ ? a : 0]; py[i] = ay()[a < A_ ? a : 0];
                        same = same && (!dec[i] || (px[i] == x0 && py[i] == y0));
                    }
                    same = __all(same);
                }
                if (no_grouping || same) {
#pragma unroll
                    for (int i = 0; i < NAW; i++) {
                        const int a = i * 64 + lane;
                        if (a < A_) ainfo()[a] = (ainfo()[a] & ~A_GRP) | (dec[i] ? (1u << 8) : 0u);
                    }
                    h.n_groups = 1;
                } else {
                    // general: groups in ascending (x, then y) order == rows of np.unique(axis=0) :293
                    bool todo[NAW];
                    uint32_t gid[NAW];
#pragma unroll
                    for (int i = 0; i < NAW; i++) { todo[i] = dec[i]; gid[i] = 0; }
                    int g = 0;
                    for (;;) {
                        double lx = __builtin_nan("");
#pragma unroll
                        for (int i = 0; i < NAW; i++) lx = nanmin2(lx, todo[i] ? px[i] : __builtin_nan(""));
                        const double mxv = wave_nanmin(lx);
                        if (!(mxv == mxv)) break;
                        double ly = __builtin_nan("");
#pragma unroll
                        for (int i = 0; i < NAW; i++) ly = nanmin2(ly, (todo[i] && px[i] == mxv) ? py[i] : __builtin_nan(""));
                        const double myv = wave_nanmin(ly);
                        g++;
#pragma unroll
                        for (int i = 0; i < NAW; i++) if (todo[i] && px[i] == mxv && py[i] == myv) { gid[i] = (uint32_t)g; todo[i] = false; }
                    }
#pragma unroll
                    for (int i = 0; i < NAW; i++) {
                        const int a = i * 64 + lane;
                        if (a < A_) ainfo()[a] = (ainfo()[a] & ~A_GRP) | (gid[i] << 8);
                    }
                    h.n_groups = g;
                }
            }
            WSYNC();
            PH_MARK(6);
            task_update(h, P, lane, -3, track);                               // worker.py:50
            WSYNC();
            PH_MARK(7);
            agent_update(h, P, lane);                                         // worker.py:51
            PH_MARK(8);
            if (!any) {
                if (++h.empty_passes > 4) {
                    h.flags |= DCM_FLAG_TRUNCATED;
                    if constexpr (INNER) terminal_inner(h);
                    else if (defer) terminal_deferred(h, lane); else terminal(h, P, lane, row);
                    return;
                }
                continue;
            }
            h.empty_passes = 0;
            h.cur_group = 1;
            WSYNC();
            return;
        }
    }

    // The count table (HBM, 2*A*T bytes, indexed a * T + t with the env's own T) only holds the abandonments beyond the log's 16 per
    // agent, so it needs clearing only after an episode in which some agent overflowed its log.  Judged by, and sized for, the sizes
    // the simulator has NOW: a kernel form that changes an env's sizes at a restart (wave_renew_instance_sized) calls this with the
    // finished episode's sizes still in place -- before they change -- so that every agent of that episode is looked at and its
    // whole table is cleared; the table is then all zero whenever an episode starts, whatever sizes it starts with.
    __device__ __forceinline__ void clear_spilled_counts(int lane) const {
        bool spilled = false;
        for_agents(lane, [&](int a) { spilled = spilled || (ainfo()[a] >> 16) > (uint32_t)AB_CAP; });
        if (__any(spilled)) {
            uint4* c = (uint4*)abcnt();
            const int n16 = (int)(abcnt_pitch(A(), T()) / 16);
            for (int i = lane; i < n16; i += WAVE) c[i] = uint4{0u, 0u, 0u, 0u};
        }
    }

    // reset + clear_decisions (env/task_env.py:116-140); keeps seed, d, episodes
    __device__ __forceinline__ void reset_state(HdrRegs& h, int lane) const {
        const int PT_ = PT();
        if constexpr (INC) { if (lane == 0) inc_state()[1] = -1; }   // incremental task_update: the next call visits every task
        for_tasks(lane, [&](int t) {
            const uint32_t req = tinfo()[t] & 0xFF;
            tinfo()[t] = req | (req << 8);       // status = requirements :131, members [], not feasible/finished
            tnab()[t] = 0;
            store_ids(t, Ids{});
            ts()[t] = 0.0; tf()[t] = 0.0;
#pragma unroll
            for (int j = 0; j < MC; j++) marr()[j * PT_ + t] = __builtin_nan("");  // empty member slots
        });
        clear_spilled_counts(lane);              // abandoned_agent = [] :131
        for_agents(lane, [&](int a) {
            ax()[a] = ((const Hdr*)base)->depot_x; ay()[a] = ((const Hdr*)base)->depot_y;      // :134
            arr()[a] = 0.0; nd()[a] = 0.0; tdist()[a] = 0.0;  // :135
            cur()[a] = -2; ainfo()[a] = 0;
        });
        h.now = 0.0; h.flags = 0; h.cur_group = 0; h.n_groups = 0; h.empty_passes = 0;  // :139-140
        if (lane == 0) ((Hdr*)base)->max_arrival = 0.0;
    }

    // ------------------------------------------------------------------------------ decisions
    // worker.py:54 -- the deciding agent of the current group (protocol slot 0), or the injected one
    // (Keeping the group bitmask in SGPRs from one decision to the next was measured SLOWER: +12 % launch time from
    // the extra SGPR pressure / spills, so it is recomputed with one LDS read + ballot per decision.)
    // lowest: individual selection (DCM_PARAM_NO_GROUPING) -- the deciders act one by one in ascending id, `for agent_id in
    // decision_agents` of worker.py:170, so the next one is simply the lowest pending id (no draw)
    __device__ __forceinline__ int pick_leader(HdrRegs& h, int lane, int leader_in, uint64_t k1, AMask& gm, bool lowest = false) const {
        gm = group_mask(h.cur_group, lane);
        const int glen = am_count(gm);
        if (glen == 0) { h.flags |= DCM_FLAG_BAD_LEADER | DCM_FLAG_DONE; return -1; }  // unreachable: groups are never empty
        if (leader_in >= 0) {
            if (leader_in >= A() || !am_test(gm, leader_in)) { h.flags |= DCM_FLAG_BAD_LEADER | DCM_FLAG_DONE; return -1; }
            return leader_in;
        }
        if (lowest) return am_nth(gm, 0, lane);
        return am_nth(gm, below((uint32_t)(k1 >> 32), glen), lane);
    }

    // worker.py:57-68: mask + both observation tensors relative to `leader`, straight into the policy's input
    // tensors (fp32 casts of worker.py:62,64).
    __device__ __forceinline__ void observe(const HdrRegs& h, int lane, int leader, float* __restrict__ ag,
                                            float* __restrict__ tk, uint8_t* __restrict__ mask, const XY& xy) const {
        const double now = h.now;
        const double lx = ax()[leader], ly = ay()[leader];
        // get_current_agent_status, env/task_env.py:165-180
        if (ag) {
            for_agents(lane, [&](int a) {
                const int c = cur()[a];
                const int K = c < 0 ? 0 : c;
                const double av = arr()[a], tsK = ts()[K], durK = tdur()[K];
                const bool on = c >= 0;                                       // :168
                const double x = av - now, w = now - av, r = tsK + durK - now;
                const double travel = (on && x > 0.) ? x : 0.;                // :169
                const double waiting = (on && now <= tsK && w > 0.) ? w : 0.; // :170
                const double remaining = (on && now >= tsK && r > 0.) ? r : 0.;  // :171
                float* row = ag + 6 * a;                                      // :176-177
                row[0] = (float)travel; row[1] = (float)remaining; row[2] = (float)waiting;
                row[3] = (float)(lx - ax()[a]); row[4] = (float)(ly - ay()[a]);
                row[5] = (ainfo()[a] & A_ASSIGNED) ? 1.f : 0.f;
            });
        }
        // get_current_task_status :182-190 and get_unfinished_task_mask :192-200
        bool allmasked = true;
        for_tasks(lane, [&](int t) {
            const uint32_t info = tinfo()[t];
            const int status = (int)(int8_t)((info >> 8) & 0xFF);
            const bool unfinished = !(info & T_FEAS) && status > 0;           // :199
            allmasked = allmasked && !unfinished;
            if (mask) mask[t + 1] = unfinished ? 0 : 1;                       // :193
            if (tk) {
                float* row = tk + 5 * (t + 1);                                // :185-186
                row[0] = (float)status; row[1] = (float)(info & 0xFF); row[2] = (float)tdur()[t];
                if constexpr (IRB) {
                    double x = 0., y = 0.;
#pragma unroll
                    for (int c = 0; c < NTC; c++) if (c == (t >> 6)) { x = xy.x[c]; y = xy.y[c]; }   // (t = chunk * 64 + lane)
                    row[3] = (float)(x - lx); row[4] = (float)(y - ly);
                } else { row[3] = (float)(tx()[t] - lx); row[4] = (float)(ty()[t] - ly); }
            }
        });
        allmasked = __all(allmasked);
        // (fp64 subtract / convert on all lanes, store by one: single-lane fp64 VALU work is 4x slower on gfx950)
        const float dxf = (float)(((const Hdr*)base)->depot_x - lx), dyf = (float)(((const Hdr*)base)->depot_y - ly);
        if (lane == 0) {
            if (mask) mask[0] = allmasked ? 0 : 1;                            // worker.py:58-61
            if (tk) { tk[0] = 0.f; tk[1] = 0.f; tk[2] = 0.f; tk[3] = dxf; tk[4] = dyf; }  // :188
        }
    }

    // uniform-random valid action (protocol slot 1): valid = ascending unmasked action ids
    __device__ __forceinline__ int pick_random_action(int lane, uint64_t k1) const {
        const int T_ = T();
        if constexpr (CT != 0 && CT <= 64) {
            const uint32_t info = tinfo()[lane < T_ ? lane : 0];
            const uint64_t bm = __ballot((lane < T_) && !(info & T_FEAS) && ((int)(int8_t)((info >> 8) & 0xFF) > 0));
            const int nv = __popcll(bm);
            if (nv == 0) return 0;  // only the depot is unmasked
            return nth(bm, below((uint32_t)k1, nv)) + 1;
        } else {
            int nv = 0;
            for (int t0 = 0; t0 < T_; t0 += WAVE) {
                const int t = t0 + lane;
                const uint32_t info = tinfo()[t < T_ ? t : 0];
                nv += __popcll(__ballot((t < T_) && !(info & T_FEAS) && ((int)(int8_t)((info >> 8) & 0xFF) > 0)));
            }
            if (nv == 0) return 0;
            int idx = below((uint32_t)k1, nv);
            int action = 0;
            for (int t0 = 0; t0 < T_; t0 += WAVE) {
                const int t = t0 + lane;
                const uint32_t info = tinfo()[t < T_ ? t : 0];
                const uint64_t bm = __ballot((t < T_) && !(info & T_FEAS) && ((int)(int8_t)((info >> 8) & 0xFF) > 0));
                const int c = __popcll(bm);
                const int p = nth(bm, idx);
                if (action == 0 && idx >= 0 && idx < c) action = t0 + p + 1;
                idx -= c;
            }
            return action;
        }
    }

    // The greedy device policies (dcm_rollout_policy; policy_pick of the oracle): functions of the same unmasked tasks, no draw
    // (protocol slot 1 is not consumed).  FIRST: the lowest unmasked task.  NEAREST: the unmasked task with the smallest fp64
    // distance from the leader -- dist2, agent first, the ROUNDED distances compared (two different squares can round to one root)
    // with strict <, so a tie goes to the lowest index.  Lane l walks tasks l, l + 64, ... in ascending order and keeps its first
    // minimum; the wave minimum of the distances, then the wave minimum of the indices of the lanes that hold it, is the lowest
    // index overall.  No unmasked task: the depot (0).  Instantiated by the k_hp_* kernel forms only.
    __device__ __forceinline__ int pick_policy_action(int lane, int leader, int policy, const XY& xy) const {
        const int T_ = T();
        const double lx = ax()[leader], ly = ay()[leader];
        const bool nearest = policy == DCM_POLICY_NEAREST;   // wave-uniform
        double bd = __builtin_nan("");
        int bt = 0x7FFFFFFF;
        auto visit = [&](int t, int c) {                      // t = c * 64 + lane; every lane calls (ballot-free, but keeps fp64 work on all lanes)
            const bool in = t < T_;
            const int ts_ = in ? t : 0;
            const uint32_t info = tinfo()[ts_];
            const bool open = in && !(info & T_FEAS) && ((int)(int8_t)((info >> 8) & 0xFF) > 0);
            double dd = 0.0;
            if (nearest) {
                double x, y;
                if constexpr (IRB) {
                    x = 0.; y = 0.;
#pragma unroll
                    for (int k = 0; k < NTC; k++) if (k == c) { x = xy.x[k]; y = xy.y[k]; }
                } else { x = tx()[ts_]; y = ty()[ts_]; }
                dd = dist2(lx, ly, x, y);
            }
            const bool better = open && (bt == 0x7FFFFFFF || dd < bd);
            bd = better ? dd : bd;
            bt = better ? t : bt;
        };
        if constexpr (CT != 0) {
#pragma unroll
            for (int c = 0; c < NTC; c++) visit(c * WAVE + lane, c);
        } else {
            for (int t0 = 0, c = 0; t0 < T_; t0 += WAVE, c++) visit(t0 + lane, c);
        }
        const bool have = bt != 0x7FFFFFFF;
        if (__ballot(have) == 0ull) return 0;                // only the depot is unmasked
        bool cand = have;
        if (nearest) {
            const double m = wave_nanmin(have ? bd : __builtin_nan(""));
            cand = have && bd == m;
        }
        if constexpr (CT != 0 && CT <= 64) {
            return __ffsll((unsigned long long)__ballot(cand));          // one chunk: lane = task, action = task + 1
        } else {
            const double mt = wave_nanmin(cand ? (double)bt : __builtin_nan(""));   // (indices below 2^10: exact in fp64)
            return (mt == mt) ? (int)mt + 1 : 0;
        }
    }

    // NEAREST's next pick behind a cursor (the width-limited lookahead form's candidate list, rollout_lookahead.hpp): the unmasked task
    // with the smallest (rounded fp64 distance from the leader, index) among those with d > pd || (d == pd && t > pt) -- what
    // pick_policy_action(NEAREST) would return if every task up to the cursor, in that order, were masked.  (pd, pt) wave-uniform;
    // (-1, -1) is in front of every task.  The same walk and reduction: lane l keeps its first minimum BEHIND THE CURSOR (a lane that
    // owns two tasks at one distance moves on from the first to the second), the wave minimum of the distances, then the lowest
    // index among the lanes that hold it.  Returns the task (wave-uniform, its distance in `dist`), or -1 when no unmasked task lies
    // behind the cursor.  Instantiated by the lookahead form only.
    __device__ __forceinline__ int next_nearest_task(int lane, int leader, double pd, int pt, const XY& xy, double& dist) const {
        const int T_ = T();
        const double lx = ax()[leader], ly = ay()[leader];
        double bd = __builtin_nan("");
        int bt = 0x7FFFFFFF;
        auto visit = [&](int t, int c) {                      // t = c * 64 + lane; every lane calls (keeps the fp64 work on all lanes)
            const bool in = t < T_;
            const int ts_ = in ? t : 0;
            const uint32_t info = tinfo()[ts_];
            const bool open = in && !(info & T_FEAS) && ((int)(int8_t)((info >> 8) & 0xFF) > 0);
            double x, y;
            if constexpr (IRB) {
                x = 0.; y = 0.;
#pragma unroll
                for (int k = 0; k < NTC; k++) if (k == c) { x = xy.x[k]; y = xy.y[k]; }
            } else { x = tx()[ts_]; y = ty()[ts_]; }
            const double dd = dist2(lx, ly, x, y);
            const bool behind = dd > pd || (dd == pd && t > pt);
            const bool better = open && behind && (bt == 0x7FFFFFFF || dd < bd);
            bd = better ? dd : bd;
            bt = better ? t : bt;
        };
        if constexpr (CT != 0) {
#pragma unroll
            for (int c = 0; c < NTC; c++) visit(c * WAVE + lane, c);
        } else {
            for (int t0 = 0, c = 0; t0 < T_; t0 += WAVE, c++) visit(t0 + lane, c);
        }
        const bool have = bt != 0x7FFFFFFF;
        if (__ballot(have) == 0ull) return -1;
        const double m = wave_nanmin(have ? bd : __builtin_nan(""));
        const bool cand = have && bd == m;
        dist = m;
        if constexpr (CT != 0 && CT <= 64) {
            return __ffsll((unsigned long long)__ballot(cand)) - 1;      // one chunk: lane = task
        } else {
            return (int)wave_nanmin(cand ? (double)bt : __builtin_nan(""));   // (indices below 2^10: exact in fp64)
        }
    }

    // TaskEnv.step (env/task_env.py:326-342) + agent_step (:300-324) for leader + followers, then
    // task_update / agent_update (worker.py:74-76) and the move to the next decision point.
    // DEV: the action comes from the device's own valid-action policy on a validated instance (persistent kernel): the error
    // exits below cannot be taken and are compiled out -- each `return` in the middle of the step costs the structured control
    // flow of the whole function scalar bookkeeping at every decision.
    // INNER: advance<INNER>, see there.
    template <bool DEV = false, bool INNER = false>
    __device__ __forceinline__ void apply_and_advance(HdrRegs& h, const KP& P, int lane, int leader, const AMask& gm0,
                                                      int action, uint64_t k1, int nfol_in,
                                                      const int16_t* __restrict__ fol_in, double* __restrict__ row PH_ARGS,
                                                      RouteLog log = RouteLog{nullptr, nullptr, nullptr, 0}, int log_row = 0,
                                                      bool no_grouping = false, int host_actions = 0,
                                                      bool incremental = false, bool track = false, const XY* xyp = nullptr) const {
        // host_actions: 0 = the action comes from the device's own valid-action policy (persistent kernel); 1 = from the host
        // (lockstep API): ANY action in [0, T] is simulated as TaskEnv.step would (env/task_env.py:326-342 has no mask check) --
        // on a masked task (feasible, or status <= 0 incl. the stale status of quirk Q3, :192-200) vacancy <= 0 sends the
        // leader alone (:330-336), the task may then list more members than it requires, and an agent released before it
        // arrives makes its arrival list non-monotone, which is why the header keeps the episode's running maximum; 2 = from
        // the host with DCM_PARAM_STRICT_MASK: such an action freezes the env instead (DCM_FLAG_BAD_ACTION).
        const int A_ = A(), T_ = T();
        if constexpr (!DEV) { if (action < 0 || action > T_) { h.flags |= DCM_FLAG_BAD_ACTION | DCM_FLAG_DONE; return; } }
        if (!DEV && host_actions == 2 && action > 0) {
            const uint32_t ik = uni(tinfo()[action - 1]);
            if ((ik & T_FEAS) || (int)(int8_t)((ik >> 8) & 0xFF) <= 0) { h.flags |= DCM_FLAG_BAD_ACTION | DCM_FLAG_DONE; return; }
        }
        AMask rest = gm0;
        am_clear(rest, leader);                                               // :328 group.remove(leader)
        int rlen = am_count(rest);
        AMask mm;                                                             // members of this step
#pragma unroll
        for (int i = 0; i < NAW; i++) mm.w[i] = 0;
        am_set(mm, leader);
        Ids mlist{};                                                          // ordered member ids of this step, byte j (task actions only)
        mlist.put(0, (uint32_t)leader);
        int nm = 1;
        double tx_, ty_;
        if (action == 0 && nfol_in < 0 && !no_grouping) {   // (individual selection: agent_step(agent, 0) moves that agent only)
            // vacancy = len(group) (:327): every co-located agent returns with the leader (Q9); the draw
            // order of the followers cannot change any state, so no draws are spent.
#pragma unroll
            for (int i = 0; i < NAW; i++) mm.w[i] |= rest.w[i];
            nm += rlen; rlen = 0;
            tx_ = ((const Hdr*)base)->depot_x; ty_ = ((const Hdr*)base)->depot_y;
        } else {
            const int k = action - 1;
            int nf;
            if (nfol_in >= 0) nf = nfol_in;                                   // injected (also for the depot: individual selection)
            else if (rlen == 0 || no_grouping) nf = 0;                        // nobody left to follow / individual selection: agent_step alone (worker.py:186)
            else {
                const int vacancy = (int)(int8_t)((uni(tinfo()[k]) >> 8) & 0xFF);  // :327 task status (may be stale)
                nf = (vacancy > 1) ? ((vacancy - 1 < rlen) ? vacancy - 1 : rlen) : 0;  // :330-331
            }
            if constexpr (!DEV) {
                if (nf > MC - 1 || nf > rlen || (nfol_in >= 0 && nf > DCM_FOLLOWER_COLS)) { h.flags |= DCM_FLAG_OVERFLOW | DCM_FLAG_DONE; return; }
            }
            uint64_t kk = k1;
            for (int j = 0; j < nf; j++) {                                    // :331 choice without replacement
                int f;
                if (nfol_in >= 0) {
                    f = fol_in[j];
                    if (f < 0 || f >= A_ || !am_test(rest, f)) { h.flags |= DCM_FLAG_BAD_LEADER | DCM_FLAG_DONE; return; }
                } else {
                    if ((j & 1) == 0) kk = mix64(kk + GAMMA);                 // key_{2+j/2}
                    const uint32_t r = (j & 1) ? (uint32_t)kk : (uint32_t)(kk >> 32);
                    f = am_nth(rest, below(r, rlen), lane);
                }
                am_clear(rest, f); rlen--;                                    // :332-333
                am_set(mm, f);
                mlist.put(nm, (uint32_t)f);
                nm++;
            }
            if (action == 0) { tx_ = ((const Hdr*)base)->depot_x; ty_ = ((const Hdr*)base)->depot_y; }
            else task_xy(k, *xyp, tx_, ty_);
        }
        PH_MARK(11);
        // agent_step for every member (:300-324); independent per agent.  The fp64 arithmetic (distance, sqrt, division) runs
        // on ALL lanes with a clamped agent index and only the stores are predicated on membership: gfx950 executes an fp64
        // VALU instruction with fewer than 16 active lanes 4x slower (17 instead of 4.2 clocks, profiles/r03_calib), and a
        // step moves 1..5 agents.
        double arrv[NAW];
#pragma unroll
        for (int i = 0; i < NAW; i++) {
            const int a = i * 64 + lane;
            const int ac = a < A_ ? a : 0;
            const double d = dist2(ax()[ac], ay()[ac], tx_, ty_);
            const double travel_time = over_velocity(d);                              // :315 velocity 0.2 (:99)
            const double td = tdist()[ac] + d;                                        // :317
            arrv[i] = h.now + travel_time;                                            // :318
            if (a < A_ && ((mm.w[i] >> lane) & 1ull)) {
                tdist()[a] = td;
                arr()[a] = arrv[i];
                ax()[a] = tx_; ay()[a] = ty_;                                 // :320
                cur()[a] = action - 1;                                        // :314 route.append
                uint32_t ai = ainfo()[a] & ~(A_GRP | A_MEMBER);               // leaves the pending group
                ai |= (action == 0) ? A_INDEPOT : A_MEMBER;                   // :321-322 listed in the target's members
                ainfo()[a] = ai;
                if (log.len) {                                                // route.append / arrival_time += (:314,:318)
                    const size_t o = (size_t)log_row + a;                     // log_row = env index x agents per env
                    const int c = log.len[o];
                    if (c < log.cap) { log.task[o * log.cap + c] = (int16_t)(action - 1); log.arrival[o * log.cap + c] = arrv[i]; }
                    log.len[o] = c + 1;
                }
            }
        }
        if (host_actions) {
            // running maximum of every arrival appended in this episode (see Hdr::max_arrival)
            double m = __builtin_nan("");
#pragma unroll
            for (int i = 0; i < NAW; i++) m = nanmax2(m, ((mm.w[i] >> lane) & 1ull) ? arrv[i] : __builtin_nan(""));
            const double wm = wave_nanmax(m);
            if (lane == 0) { Hdr* q = (Hdr*)base; if (wm > q->max_arrival) q->max_arrival = wm; }
        }
        if (action > 0) {
            // :321-322 members.append unless already listed; a re-joining agent keeps its slot but
            // get_arrival_time (:202-205) now returns the new, later arrival (Q4).  Wave-uniform loop over the
            // 1..5 members in order; "already listed" is a SWAR byte search in the packed ordered id word.
            const int k = action - 1;
            const uint32_t info = uni(tinfo()[k]);
            Ids ids = load_ids(k);
#pragma unroll
            for (int i = 0; i < IW; i++) ids.w[i] = uni(ids.w[i]);
            int n = (info >> 16) & 0xFF;
            for (int j = 0; j < nm; j++) {
                const int m = (int)mlist.byte(j);
                int pos = ids.find((uint32_t)m, n);
                if (pos < 0) {
                    if constexpr (!DEV) { if (n >= MC) { h.flags |= DCM_FLAG_OVERFLOW | DCM_FLAG_DONE; return; } }
                    pos = n++;
                    ids.put(pos, (uint32_t)m);                                // bytes above n are always zero
                }
                // the arrival was computed by agent m's own lane above: that lane stores it (no readlane round trip through
                // the scalar unit, and the store does not wait for the sqrt chain of the other members)
#pragma unroll
                for (int i = 0; i < NAW; i++) if (i * WAVE + lane == m) marr()[pos * PT() + k] = arrv[i];
                // (bits 22..31 of the dirty word: the task that was joined -- one per step -- so that the write-back can send its
                //  64-byte pieces of the arrival rows / member ids instead of the sections)
                if (track && lane == 0) *dirty() = (*dirty() & ((1u << DIRTY_TASK_SHIFT) - 1u)) | (2u << pos) | DIRTY_IDS | ((uint32_t)k << DIRTY_TASK_SHIFT);
            }
            if (lane == 0) { store_ids(k, ids); tinfo()[k] = (info & ~0x00FF0000u) | ((uint32_t)n << 16); }
        }
        h.d += 1;
        WSYNC();
        PH_MARK(3);
        task_update(h, P, lane, incremental ? (action > 0 ? action - 1 : -2) : -1, track);   // worker.py:74
        WSYNC();
        PH_MARK(4);
        agent_update(h, P, lane);                                             // worker.py:76
        WSYNC();
        PH_MARK(5);
        if (rlen > 0) return;                                                 // worker.py:53 same group, next leader
        if (h.cur_group < h.n_groups) { h.cur_group++; return; }              // worker.py:52 next group
        advance<INNER>(h, P, lane, row PH_PASS, no_grouping, track);          // worker.py:85 -> :45
        PH_MARK(9);
    }

    __device__ __forceinline__ void write_inactive_obs(int lane, float* ag, float* tk, uint8_t* mask) const {
        if (ag) for (int i = lane; i < 6 * A(); i += WAVE) ag[i] = 0.f;
        if (tk) for (int i = lane; i < 5 * (T() + 1); i += WAVE) tk[i] = 0.f;
        if (mask) for (int i = lane; i <= T(); i += WAVE) mask[i] = (i == 0) ? 0 : 1;
    }
    // Ragged batch: rows beyond this env's own A / T+1 are padding in the convention the policy already understands --
    // every feature -1 (attention.py:10-18 get_attn_pad_mask, worker.py:253-261 zero_padding) and mask True (true_padding).
    __device__ __forceinline__ void write_pad_obs(int lane, int pitch_A, int pitch_T, float* ag, float* tk, uint8_t* mask) const {
        if (ag) for (int i = 6 * A() + lane; i < 6 * pitch_A; i += WAVE) ag[i] = -1.f;
        if (tk) for (int i = 5 * (T() + 1) + lane; i < 5 * (pitch_T + 1); i += WAVE) tk[i] = -1.f;
        if (mask) for (int i = T() + 1 + lane; i <= pitch_T; i += WAVE) mask[i] = 1;
    }
};

// Three levels of dims.  (A,T) = batch dims: the shapes of every input / output array and the default env sizes.
// (eA,eT) = this env's own sizes: (A,T) for a uniform batch, sizes[e] for a ragged one (dcm_load_instances_ragged).
// (PA,PT) = layout dims of the record (Lay{PA,PT}, the same for every env of the handle, >= the batch dims): the
// template constants, or the kernel arguments for the <0,0> instantiation.  Only the entries below an env's own sizes
// are ever touched, so the simulator code is the same for all three kinds of instantiation (see Sim).
template <int CA, int CT, bool RS>
__device__ __forceinline__ void env_dims(const int32_t* sizes, int e, int A, int T, int& eA, int& eT) {
    eA = A; eT = T;
    if constexpr (RS || CA == 0) {
        if (sizes) { eA = uni(sizes[2 * e]); eT = uni(sizes[2 * e + 1]); }
    }
}

// ---------------------------------------------------------------------------------- kernels
// XCD-aware env placement of the one-workgroup-per-env kernels.  Workgroups are dealt round-robin over the 8 XCDs (each with its own
// L2 and its own path to memory): workgroup b runs env  xcd(b) * ceil(B/8) + b/8,  i.e. every XCD owns a CONTIGUOUS block of envs.
//  * persistent kernel: the observation rows an XCD rewrites at every decision are one dense region of its L2 instead of every
//    eighth 480 / 1020-byte row, which aliased in the L2 sets and sent ~10 % of the per-decision stores to HBM (243 MB per
//    4096-env launch; 55 MB = the compulsory traffic with this map, profiles/r03_xcd_map);
//  * lockstep kernel: with e = blockIdx.x all XCDs stream through the SAME neighbourhood of the state array at any moment; with
//    contiguous blocks they work in eight separate regions: 147-170 -> 136 us at 65 536 envs (0.80 of the HBM peak).
__device__ __forceinline__ int env_of_workgroup() {
    const int nb = gridDim.x, q = nb >> 3, r = nb & 7, x = blockIdx.x & 7, i = blockIdx.x >> 3;
    return x * q + (x < r ? x : r) + i;
}

#include "instgen.hpp"
#ifndef DCM_DEVICE_ONLY_TU   // k_reduce_best: the host API's unit only (the form units hold their forms and nothing else)
#include "best_reduce.hpp"
#endif
#ifndef DCM_DEVICE_ONLY_TU   // k_fork_envs: likewise
#include "fork_envs.hpp"
#endif

__global__ __launch_bounds__(WAVE) void k_load_instances(int A, int T, int PA, int PT, int PC, unsigned char* state, const double* depot,
                                                        const double* task_xy, const int32_t* req, const double* dur,
                                                        const int32_t* sizes) {
    const int e = blockIdx.x, lane = threadIdx.x;
    int eA, eT;
    env_dims<0, 0, false>(sizes, e, A, T, eA, eT);
    const Lay L{PA, PT, PC};                                   // input arrays are pitched by the batch dims (A,T)
    unsigned char* rec = state + (size_t)e * L.rec_bytes();
    double *tx = (double*)(rec + L.tx()), *ty = (double*)(rec + L.ty()), *td = (double*)(rec + L.tdur());
    uint32_t* ti = (uint32_t*)(rec + L.tinfo());
    bool bad = false;
    for (int t = lane; t < eT; t += WAVE) {
        tx[t] = task_xy[((size_t)e * T + t) * 2];
        ty[t] = task_xy[((size_t)e * T + t) * 2 + 1];
        td[t] = dur[(size_t)e * T + t];
        // requirements outside 1..(member slots of the handle) do not fit the member slots (the reference takes any max_coalition_size,
        // env/task_env.py:71): the env is marked and stays frozen instead of simulating something else
        const int32_t r = req[(size_t)e * T + t];
        bad = bad || r < 1 || r > PC;
        ti[t] = (uint32_t)(r < 1 ? 1 : r > PC ? PC : r);
    }
    bad = __any(bad);
    if (lane == 0) {
        Hdr* h = (Hdr*)rec;
        h->depot_x = depot[2 * (size_t)e]; h->depot_y = depot[2 * (size_t)e + 1];
        h->flags = DCM_FLAG_DONE | (bad ? DCM_FLAG_BAD_INSTANCE : 0u); h->episodes = 0; h->d = 0; h->seed = 0;
        h->groups = 0; h->reserved = 0; h->max_arrival = 0.0;
    }
}

#ifndef DCM_DEVICE_ONLY_TU   // the host API's unit only
// The load-time check behind plan::Shape::inrange: does any env hold two of its T_e + 1 points (the depot, then its tasks) whose squared
// distance -- formed as dist2 forms it; the square of a negated difference is the same number -- lies strictly between 0 and
// DIST2_INRANGE_MIN?  Such a square is the only argument on which dist2_inrange differs from dist2 (NaN and inf pass through both
// alike).  Sets *bad; one wave per env over the i < j pairs of its own record.
__global__ __launch_bounds__(WAVE) void k_points_inrange(int A, int T, int PA, int PT, int PC, const unsigned char* state, const int32_t* sizes,
                                                        uint32_t* bad) {
    const int e = blockIdx.x, lane = threadIdx.x;
    int eA, eT;
    env_dims<0, 0, false>(sizes, e, A, T, eA, eT);
    const Lay L{PA, PT, PC};
    const unsigned char* rec = state + (size_t)e * L.rec_bytes();
    const double *tx = (const double*)(rec + L.tx()), *ty = (const double*)(rec + L.ty());
    const Hdr* h = (const Hdr*)rec;
    bool out = false;
    for (int j = lane; j < eT; j += WAVE) {                  // point j + 1 = task j against the depot and the tasks below it
        const double bx = tx[j], by = ty[j];
        for (int i = -1; i < j; i++) {
            const double dx = (i < 0 ? h->depot_x : tx[i]) - bx, dy = (i < 0 ? h->depot_y : ty[i]) - by;
            const double q = __builtin_fma(dy, dy, dx * dx);
            out = out || (q > 0.0 && q < DIST2_INRANGE_MIN);
        }
    }
    if (__any(out) && lane == 0) atomicOr(bad, 1u);
}
#endif

// dynamic LDS of a k_reset / k_observe / k_step launch: the record image (MC moves no section of it)
template <int CA, int CT, bool RS>
constexpr uint32_t env_kernel_lds_bytes(Lay L) { return Sim<CA, CT, RS>::lds_image_bytes(L); }

template <int CA, int CT, bool RS, int MC = M>
__global__ __launch_bounds__(WAVE) void k_reset(int A, int T, int PA, int PT, KP P, unsigned char* state, const uint64_t* seeds,
                                               double* summary, uint16_t* ablog, uint32_t mode, const int32_t* sizes,
                                               unsigned char* gscr) {
    const int e = env_of_workgroup(), lane = threadIdx.x;
    int eA, eT;
    env_dims<CA, CT, RS>(sizes, e, A, T, eA, eT);
    Sim<CA, CT, RS, false, MC> S{eA, eT, PA, PT, smem, nullptr};
    const Lay L = S.L();
    S.scr = gscr + (size_t)e * L.scratch_bytes();
    unsigned char* rec = state + (size_t)e * L.rec_bytes();
    typename Sim<CA, CT, RS, false, MC>::XY xy;
    S.load_record(rec, lane, xy);
    WSYNC();
    S.set_ablog(ablog, e, S.BA(A), S.BT(T), lane);
    S.set_retlog(nullptr, 0, e, lane);
    HdrRegs h = load_hdr(smem);
    h.seed = seeds[e]; h.d = 0;
    if (lane == 0) ((Hdr*)smem)->episodes = 0;
    const bool bad_instance = h.flags & DCM_FLAG_BAD_INSTANCE;                // set by dcm_load_instances, survives resets
    S.reset_state(h, lane);
    if (lane < 8) summary[(size_t)e * 8 + lane] = __builtin_nan("");
    PH_DECL;
    if (bad_instance) h.flags = DCM_FLAG_DONE | DCM_FLAG_BAD_INSTANCE;
    else S.advance(h, P, lane, summary + (size_t)e * 8 PH_PASS, (mode & DCM_PARAM_NO_GROUPING) != 0);
    WSYNC();
    store_hdr(h, lane);
    WSYNC();
    copy16(rec, smem, L.mut_bytes(), lane);
}

template <int CA, int CT, bool RS, int MC = M>
__global__ __launch_bounds__(WAVE) void k_observe(int A, int T, int PA, int PT, unsigned char* state, float* agents_out, float* tasks_out,
                                                 uint8_t* mask_out, int32_t* leader_out, uint8_t* active_out,
                                                 const int32_t* leader_in, const int32_t* sizes, uint32_t mode) {
    const int e = env_of_workgroup(), lane = threadIdx.x;
    int eA, eT;
    env_dims<CA, CT, RS>(sizes, e, A, T, eA, eT);
    using SimT = Sim<CA, CT, RS, false, MC>;
    SimT S{eA, eT, PA, PT, smem, nullptr};   // (observe never reaches the terminal metrics: no scratch)
    const Lay L = S.L();
    const int BA = S.BA(A), BT = S.BT(T);
    unsigned char* rec = state + (size_t)e * L.rec_bytes();
    typename SimT::XY xy;
    S.load_record(rec, lane, xy);
    WSYNC();
    HdrRegs h = load_hdr(smem);
    float* ag = agents_out ? agents_out + (size_t)e * 6 * BA : nullptr;
    float* tk = tasks_out ? tasks_out + (size_t)e * 5 * (BT + 1) : nullptr;
    uint8_t* mk = mask_out ? mask_out + (size_t)e * (BT + 1) : nullptr;
    int leader = -1;
    const uint32_t flags0 = h.flags;
    if (!(h.flags & DCM_FLAG_DONE)) {
        typename SimT::AMask gm;
        leader = S.pick_leader(h, lane, leader_in ? leader_in[e] : -1, key1(h.seed, h.d), gm, (mode & DCM_PARAM_NO_GROUPING) != 0);
    }
    if (leader >= 0) S.observe(h, lane, leader, ag, tk, mk, xy);
    else S.write_inactive_obs(lane, ag, tk, mk);
    if constexpr (RS || CA == 0) S.write_pad_obs(lane, BA, BT, ag, tk, mk);
    if (lane == 0) {
        if (leader_out) leader_out[e] = leader;
        if (active_out) active_out[e] = leader >= 0 ? 1 : 0;
        if (h.flags != flags0) ((Hdr*)rec)->flags = h.flags;  // injected-leader error freezes the env
    }
}

// k_step, its renewing form k_rn_step and its size-renewing form k_rs_step: see k_step.inc
#define DCM_RENEW 0
#include "k_step.inc"
#undef DCM_RENEW
#define DCM_RENEW 1
#include "k_step.inc"
#undef DCM_RENEW
#define DCM_RENEW 2   // the size-renewing form (k_rs_*): runtime-size instantiations only
#include "k_step.inc"
#undef DCM_RENEW

// ================================================================================== the persistent rollout kernels' budget and error stop
// Shared by k_rollout_random below and the register-resident k_rollout_fast, k_rollout_fast_mc and k_rollout_fast_g.

// errors that end an env's rollout at the next episode boundary (instead of the restart of a finished episode)
constexpr uint32_t ROLLOUT_ERR = DCM_FLAG_BAD_ACTION | DCM_FLAG_OVERFLOW | DCM_FLAG_BAD_LEADER | DCM_FLAG_BAD_INSTANCE;

// budget (per env: budget_in[e] if given, else budget_all; < 0 = unlimited): an env takes at most that many decisions in
// this launch; when the budget runs out the env stays at the decision point it has reached (a later call -- dcm_rollout_random,
// dcm_observe or dcm_step -- carries on from it) and the observation buffers hold what the last decision TAKEN saw.
// Returns the decisions left in this launch: a 32-bit countdown is the only loop-carried counter (steps = budget - left afterwards).
constexpr int NO_BUDGET = 0x7FFFFFFF;
__device__ __forceinline__ int rollout_budget(int e, int64_t budget_all, const int64_t* budget_in) {
    const int64_t bud = budget_in ? budget_in[e] : budget_all;
    return uni((int)((bud < 0 || bud >= NO_BUDGET) ? NO_BUDGET : bud));
}

// The budget of a greedy launch.  With max_waiting_time <= 0 a greedy episode does not end in general (plan::policy_needs_budget), so
// there "no limit" (a negative entry of max_decisions_in; the host refuses a negative scalar) counts as 0: the env takes no decision
// in this launch instead of spinning at a constant clock.  (Only the general form runs on such a handle.)
__device__ __forceinline__ int rollout_budget_policy(int e, int64_t budget_all, const int64_t* budget_in, const KP& P) {
    const int64_t bud = budget_in ? budget_in[e] : budget_all;
    const int left = rollout_budget(e, budget_all, budget_in);
    return uni((!(P.mwt > 0.0) && bud < 0) ? 0 : left);
}

// dynamic LDS of a k_rollout_random launch: the record image, or record + scratch for the layouts that keep the scratch in LDS
template <int CA, int CT, bool RS>
constexpr uint32_t rollout_random_lds_bytes(Lay L) {
    using SimT = Sim<CA, CT, RS, (CT > WAVE) && !RS>;
    return SimT::SCR_IN_LDS ? L.lds_bytes() : SimT::lds_image_bytes(L);
}

// Config-2 hot path: whole episodes in one persistent launch, record resident in LDS.  Budget: see rollout_budget.
// __launch_bounds__(64, 3): at least three waves per SIMD.  The one-chunk shapes need 111 VGPRs anyway (four waves per SIMD); the
// 50A/200T instantiation wants 176 -- two waves per SIMD although its LDS image (10.9 KB with the member arrival times left in
// the HBM record) would let twelve workgroups share a CU -- and with 168 (five spilled) it runs three: 8.65 -> 6.90 ms per
// 8192-env launch.  Four (128 VGPRs, 47 spilled) measured slower again (7.15 ms).
// k_rollout_random, its renewing form k_rn_rollout_random and its size-renewing form k_rs_rollout_random: see k_rollout_random.inc
#define DCM_RENEW 0
#include "k_rollout_random.inc"
#undef DCM_RENEW
#define DCM_RENEW 1
#include "k_rollout_random.inc"
#undef DCM_RENEW
#define DCM_RENEW 2   // the size-renewing form (k_rs_*): runtime-size instantiations only
#include "k_rollout_random.inc"
#undef DCM_RENEW

#include "rollout_fast.hpp"
#include "step_fast.hpp"
#include "rollout_fast_mc.hpp"
#ifdef DCM_HAVE_FAST_G
#include "rollout_fast_g.hpp"
#endif
#ifdef DCM_HAVE_POLICY
#include "rollout_policy.hpp"
#endif
#ifdef DCM_HAVE_LOG
#include "rollout_log.hpp"
#endif
#ifdef DCM_HAVE_EXPLORE
#include "rollout_explore.hpp"
#endif
#ifdef DCM_HAVE_BEST
#include "rollout_best.hpp"
#endif
#ifdef DCM_HAVE_LOOKAHEAD
#include "rollout_lookahead.hpp"
#endif
#ifdef DCM_HAVE_INDIVIDUAL
#include "rollout_individual.hpp"
#endif

__global__ __launch_bounds__(WAVE) void k_env_status(int PA, int PT, int PC, const unsigned char* state, int B, uint32_t* flags_out,
                                                    int64_t* dec_out, double* now_out, int32_t* episodes_out) {
    const int e = blockIdx.x * WAVE + threadIdx.x;
    if (e >= B) return;
    const Hdr* h = (const Hdr*)(state + (size_t)e * Lay{PA, PT, PC}.rec_bytes());
    if (episodes_out) episodes_out[e] = (int32_t)h->episodes;
    if (flags_out) flags_out[e] = h->flags;
    if (dec_out) dec_out[e] = (int64_t)h->d;
    if (now_out) now_out[e] = h->now;
}

template <int MC>
__global__ __launch_bounds__(WAVE) void k_get_tasks(int A, int T, int PA, int PT, KP P, unsigned char* state, uint8_t* finished,
                                                   uint8_t* feasible, double* time_start, double* time_finish,
                                                   double* sum_wait, int32_t* status, int32_t* n_members,
                                                   int32_t* n_abandoned, uint16_t* ablog, const int32_t* sizes,
                                                   unsigned char* gscr) {
    const int e = blockIdx.x, lane = threadIdx.x;
    int eA, eT;
    env_dims<0, 0, false>(sizes, e, A, T, eA, eT);
    Sim<0, 0, false, false, MC> S{eA, eT, PA, PT, smem, nullptr};
    const Lay L = S.L();
    S.scr = gscr + (size_t)e * L.scratch_bytes();
    copy16_in(smem, state + (size_t)e * L.rec_bytes(), L.rec_bytes(), lane);
    S.set_ablog(ablog, e, A, T, lane);
    WSYNC();
    HdrRegs h = load_hdr(smem);
    if (sum_wait) S.compute_waits(h.now, P.mwt, lane);
    for (int t = lane; t < T; t += WAVE) {                                  // rows t >= T_e of a ragged batch read as 0
        const size_t o = (size_t)e * T + t;
        const bool in = t < eT;
        const uint32_t info = in ? S.tinfo()[t] : 0u;
        if (finished) finished[o] = (info & T_FIN) ? 1 : 0;
        if (feasible) feasible[o] = (info & T_FEAS) ? 1 : 0;
        if (time_start) time_start[o] = in ? S.ts()[t] : 0.0;
        if (time_finish) time_finish[o] = in ? S.tf()[t] : 0.0;
        if (sum_wait) sum_wait[o] = in ? S.tw()[t] : 0.0;
        if (status) status[o] = (int)(int8_t)((info >> 8) & 0xFF);
        if (n_members) n_members[o] = (info >> 16) & 0xFF;
        if (n_abandoned) n_abandoned[o] = in ? (int32_t)S.tnab()[t] : 0;
    }
}

template <int MC>
__global__ __launch_bounds__(WAVE) void k_get_agents(int A, int T, int PA, int PT, KP P, unsigned char* state, double* sum_wait,
                                                    double* travel_dist, double* next_decision, double* arrival,
                                                    double* x, double* y, uint8_t* returned, uint8_t* assigned,
                                                    int32_t* current, int32_t* pending, uint16_t* ablog,
                                                    const int32_t* sizes, unsigned char* gscr) {
    const int e = blockIdx.x, lane = threadIdx.x;
    int eA, eT;
    env_dims<0, 0, false>(sizes, e, A, T, eA, eT);
    Sim<0, 0, false, false, MC> S{eA, eT, PA, PT, smem, nullptr};
    const Lay L = S.L();
    S.scr = gscr + (size_t)e * L.scratch_bytes();
    copy16_in(smem, state + (size_t)e * L.rec_bytes(), L.rec_bytes(), lane);
    S.set_ablog(ablog, e, A, T, lane);
    WSYNC();
    HdrRegs h = load_hdr(smem);
    if (sum_wait) S.compute_waits(h.now, P.mwt, lane);
    for (int a = lane; a < A; a += WAVE) {                                  // rows a >= A_e of a ragged batch: 0 / NaN timer
        const size_t o = (size_t)e * A + a;
        const bool in = a < eA;
        const uint32_t ai = in ? S.ainfo()[a] : 0u;
        if (sum_wait) sum_wait[o] = in ? S.aw()[a] : 0.0;
        if (travel_dist) travel_dist[o] = in ? S.tdist()[a] : 0.0;
        if (next_decision) next_decision[o] = in ? S.nd()[a] : __builtin_nan("");
        if (arrival) arrival[o] = in ? S.arr()[a] : 0.0;
        if (x) x[o] = in ? S.ax()[a] : 0.0;
        if (y) y[o] = in ? S.ay()[a] : 0.0;
        if (returned) returned[o] = (ai & A_RETURNED) ? 1 : 0;
        if (assigned) assigned[o] = (ai & A_ASSIGNED) ? 1 : 0;
        if (current) current[o] = in ? S.cur()[a] : -2;
        if (pending) pending[o] = (int32_t)((ai >> 8) & 0xFFu);
    }
}

// task['members'] of every task, in list order (env/task_env.py:80): ids_out[B][T][member slots of the handle], -1 padded
__global__ void k_get_members(int T, int PA, int PT, int PC, const unsigned char* state, int B, int16_t* ids_out, const int32_t* sizes) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)B * T) return;
    const int e = (int)(i / T), t = (int)(i % T);
    const int eT = sizes ? sizes[2 * e + 1] : T;
    const Lay L{PA, PT, PC};
    const unsigned char* rec = state + (size_t)e * L.rec_bytes();
    uint64_t ids[2] = {0, 0};
    int n = 0;
    if (t < eT) {
        for (uint32_t w = 0; w < L.idw(); w++) ids[w] = ((const uint64_t*)(rec + L.mids()))[w * PT + t];
        n = (int)((((const uint32_t*)(rec + L.tinfo()))[t] >> 16) & 0xFF);
    }
    for (int j = 0; j < PC; j++) ids_out[i * PC + j] = (j < n) ? (int16_t)((ids[j >> 3] >> (8 * (j & 7))) & 0xFF) : (int16_t)-1;
}

// task['abandoned_agent'] (env/task_env.py:89) as a dense count table: out[B][A][T] = number of times task t moved agent a to
// its abandoned_agent list in the current episode = entries of the agent's abandonment log + the overflow count table
__global__ __launch_bounds__(WAVE) void k_get_abandoned(int A, int T, int PA, int PT, int PC, const unsigned char* state,
                                                       const uint16_t* ablog, uint16_t* out, const int32_t* sizes) {
    const int e = blockIdx.x, lane = threadIdx.x, B = gridDim.x;
    int eA, eT;
    env_dims<0, 0, false>(sizes, e, A, T, eA, eT);
    const Lay L{PA, PT, PC};
    const uint32_t* ainfo = (const uint32_t*)(state + (size_t)e * L.rec_bytes() + L.ainfo());
    const uint16_t* log_e = ablog + (size_t)e * A * AB_CAP;
    const uint16_t* cnt_e = (const uint16_t*)((const uint8_t*)(ablog + (size_t)B * A * AB_CAP) + (size_t)e * abcnt_pitch(A, T));
    uint16_t* o = out + (size_t)e * A * T;
    for (int i = lane; i < A * T; i += WAVE) o[i] = 0;
    __syncthreads();
    for (int a = lane; a < eA; a += WAVE) {                                 // one lane per agent: no two lanes share a row
        const uint32_t nab = ainfo[a] >> 16;
        const int nl = nab < (uint32_t)AB_CAP ? (int)nab : AB_CAP;
        for (int i = 0; i < nl; i++) o[a * T + log_e[a * AB_CAP + i]] += 1;
        if (nab > (uint32_t)AB_CAP)
            for (int t = 0; t < eT; t++) o[a * T + t] += cnt_e[a * eT + t];
    }
}

__global__ void k_distance(const double* ax, const double* ay, const double* bx, const double* by, double* dist_out,
                           double* time_out, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double d = dist2(ax[i], ay[i], bx[i], by[i]);
    if (dist_out) dist_out[i] = d;
    if (time_out) time_out[i] = over_velocity(d);
}

// ---------------------------------------------------------------------------------- host side
// Which Sim<> instantiation and which kernels serve a handle is decided in plan.hpp; here its answers become template arguments.
// The instantiations by their plan::SimKind: the single list
#define FOR_EACH_INSTANCE(X) X(S20x50, 20, 50, false) X(S20x50_RS, 20, 50, true) X(S64x64_RS, 64, 64, true) X(S50x200, 50, 200, false) \
    X(S100x500, 100, 500, false) X(S128x256_RS, 128, 256, true) X(Runtime, 0, 0, false) X(RuntimeWide, 0, 0, false, MW)
// One of them as a type, with the two facts that decide which kernels exist for it
template <int CA_, int CT_, bool RS_, int MC_ = M>
struct SimTag {
    static constexpr int CA = CA_, CT = CT_, MC = MC_;
    static constexpr bool RS = RS_;
    // a one-chunk layout: the only ones that have the register-resident kernels of rollout_fast.hpp / step_fast.hpp
    static constexpr bool one_chunk = CA != 0 && CA <= WAVE && CT <= WAVE;
    // reads per-env sizes, i.e. what plan::sim_kind gives a ragged batch: the only ones the size-renewing forms (k_rs_*) exist for
    static constexpr bool reads_sizes = RS || CA == 0;
};
#define SIM_ARGS(S) S::CA, S::CT, S::RS
// The one dispatch: f(SimTag<...>{}) for the instantiation of `kind`; f returns 0, or -1 where it has no kernel for that one (a site
// that serves a subset says so with `if constexpr` on the tag: a kernel that is named is compiled).  for_each_sim: f for every one.
template <class F>
int with_sim(plan::SimKind kind, F&& f) {
    switch (kind) {
#define SIM_CASE(KIND, ...) case plan::SimKind::KIND: return f(SimTag<__VA_ARGS__>{});
    FOR_EACH_INSTANCE(SIM_CASE)
#undef SIM_CASE
    }
    return -1;
}
template <class F>
void for_each_sim(F&& f) {
#define SIM_EACH(KIND, ...) f(SimTag<__VA_ARGS__>{});
    FOR_EACH_INSTANCE(SIM_EACH)
#undef SIM_EACH
}
// ... and a runtime flag as a type (std::true_type first)
template <class F>
auto with_bool(bool b, F&& f) { return b ? f(std::true_type{}) : f(std::false_type{}); }
// kernel arguments every env kernel starts with: batch dims, layout dims
#define DIMS(env) (env)->A, (env)->T, (env)->L.A, (env)->L.T

// what plan.hpp reads of a handle
plan::Shape shape_of(const dcm_env* env) { return {env->A, env->T, env->sizes != nullptr, env->L.C > M, env->kp.mwt > 0.0, env->inrange}; }
plan::SimKind sim_of(const dcm_env* env) { return plan::sim_kind(shape_of(env)); }

// dcm_create / dcm_destroy run on the handle's device but leave the caller's current device as they found it
struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int dev) { if (hipGetDevice(&prev) != hipSuccess) prev = -1; if (prev != dev) (void)hipSetDevice(dev); else prev = -1; }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};

// Launch a kernel, one workgroup of one wave per env: `args` (a tuple: RolloutArgs::kernel_args, or what dcm_step packs), then `tail`.
// Each argument converts to the parameter it is passed to, so the handle's size table arrives const everywhere but in a k_rs_* form.
template <class K, class... Args, class... Tail>
void launch(K kernel, unsigned grid, unsigned lds_bytes, hipStream_t stream, const std::tuple<Args...>& args, const Tail&... tail) {
    std::apply([&](const Args&... a) { hipLaunchKernelGGL(kernel, dim3(grid), dim3(WAVE), lds_bytes, stream, a..., tail...); }, args);
}
template <class... K>
void allow_lds(int bytes, K... kernels) { ((void)hipFuncSetAttribute((const void*)kernels, hipFuncAttributeMaxDynamicSharedMemorySize, bytes), ...); }

// A kernel family: the forms of one kernel text (k_form.inc) under one name each; <V...> are the kernel's template arguments, the
// same in every form.  DCM_FAMILY(base) is the family of a text compiled with DCM_RENEW 0 / 1 / 2.  (Return types written out:
// the kernel is then instantiated when the function that names the accessor is, in the order of the names, like one named directly.)
#define DCM_FORM(NAME, KERNEL) template <auto... V> static decltype(&KERNEL<V...>) NAME() { return KERNEL<V...>; }
#define DCM_FORMS(PLAIN, RENEWING) DCM_FORM(plain, PLAIN) DCM_FORM(renewing, RENEWING)
#define DCM_FAMILY(base) struct base##_family { DCM_FORMS(k_##base, k_rn_##base) DCM_FORM(size_renewing, k_rs_##base) };
DCM_FAMILY(step)
DCM_FAMILY(step_fast)
DCM_FAMILY(rollout_random)
DCM_FAMILY(rollout_fast)
struct rollout_fast_mc_family { DCM_FORMS(k_rollout_fast_mc, k_rn_rollout_fast_mc) };   // (exact shape, never ragged: no size-renewing form)
#ifdef DCM_HAVE_FAST_G
DCM_FAMILY(rollout_fast_g)
#endif
#undef DCM_FAMILY

// Launch the member <V...> of a family in the form plan::renew_form chose, the one place that knows the rule: k_rs_* for Sizes, k_rn_*
// for Instance, k_* otherwise, `rn` behind the common arguments of the renewing two, then the `tail` of a greedy, logging or epsilon-
// greedy family.  HAS_RS: the member has a size-renewing form (SimTag::reads_sizes; all of k_rollout_fast_g); -1 for Sizes without.
// (Kernels are instantiated in the order they are named and a unit's assembly lists them in that order: keep rs, rn, plain.)
template <class Fam, bool HAS_RS, auto... V, class Args, class... Tail>
int launch_family(plan::RenewForm form, unsigned grid, unsigned lds_bytes, hipStream_t stream, const Args& args, const Renew& rn,
                  const Tail&... tail) {
    if (form == plan::RenewForm::Sizes) {
        if constexpr (HAS_RS) launch(Fam::template size_renewing<V...>(), grid, lds_bytes, stream, args, rn, tail...);
        else return -1;
    } else if (form == plan::RenewForm::Instance) launch(Fam::template renewing<V...>(), grid, lds_bytes, stream, args, rn, tail...);
    else launch(Fam::template plain<V...>(), grid, lds_bytes, stream, args, tail...);
    return 0;
}

// dcm::launch_rollout_<form> and dcm::allow_lds_<form> for a form F (DCM_FORM_LAUNCHERS), which names its two families and its tail
template <class F>
int launch_rollout_form(plan::SimKind kind, bool fast, bool obs, unsigned grid, Lay L, hipStream_t stream, const RolloutArgs& a) {
    if (fast)
        return with_sim(kind, [&](auto s) {
            using S = decltype(s);
            if constexpr (S::one_chunk)
                return with_bool(obs, [&](auto obs_c) {
                    return F::template go<typename F::fast, SIM_ARGS(S), decltype(obs_c)::value>(grid, rollout_fast_lds_bytes<SIM_ARGS(S)>(L), stream, a);
                });
            else return -1;
        });
    return with_sim(kind, [&](auto s) {
        using S = decltype(s);
        return F::template go<typename F::general, SIM_ARGS(S), S::MC>(grid, rollout_random_lds_bytes<SIM_ARGS(S)>(L), stream, a);
    });
}
template <class F>
void allow_lds_form(int lds) {
    for_each_sim([&](auto s) {
        using S = decltype(s);
        if constexpr (F::has_renewing)
            allow_lds(lds, F::general::template plain<SIM_ARGS(S), S::MC>(), F::general::template renewing<SIM_ARGS(S), S::MC>());
        else allow_lds(lds, F::general::template plain<SIM_ARGS(S), S::MC>());
    });
    for_each_sim([&](auto s) {
        using S = decltype(s);
        if constexpr (S::one_chunk && F::has_renewing)
            allow_lds(lds, F::fast::template plain<SIM_ARGS(S), true>(), F::fast::template plain<SIM_ARGS(S), false>(),
                      F::fast::template renewing<SIM_ARGS(S), true>(), F::fast::template renewing<SIM_ARGS(S), false>());
        else if constexpr (S::one_chunk)
            allow_lds(lds, F::fast::template plain<SIM_ARGS(S), true>(), F::fast::template plain<SIM_ARGS(S), false>());
    });
}
}  // namespace

// One form: its name, the prefix of its plain and of its renewing kernels, and the arguments it appends behind retcap (behind a.rn in
// the renewing ones).  The form has no size-renewing kernels and no wave-priority (PRIO) instantiation.
// DCM_PLAIN_FORM_LAUNCHERS: a form without renewing kernels either (HAS_RN false: its `renewing` accessors are never named, and a
// launch in another form than Plain returns -1).
#define DCM_FORM_LAUNCHERS(FORM, plain, renewing, ...) DCM_FORM_LAUNCHERS_(FORM, true, plain, renewing, __VA_ARGS__)
#define DCM_PLAIN_FORM_LAUNCHERS(FORM, plain, ...) DCM_FORM_LAUNCHERS_(FORM, false, plain, plain, __VA_ARGS__)
#define DCM_FORM_LAUNCHERS_(FORM, HAS_RN, P_, R_, ...)                                                                              \
    namespace {                                                                                                                      \
    struct FORM##_form {                                                                                                             \
        static constexpr bool has_renewing = HAS_RN;                                                                                 \
        struct fast { DCM_FORMS(P_##rollout_fast, R_##rollout_fast) };                                                               \
        struct general { DCM_FORMS(P_##rollout_random, R_##rollout_random) };                                                        \
        template <class Fam, auto... V>                                                                                              \
        static int go(unsigned grid, unsigned lds_bytes, hipStream_t stream, const RolloutArgs& a) {                                 \
            if constexpr (HAS_RN)                                                                                                    \
                return launch_family<Fam, false, V...>(a.form, grid, lds_bytes, stream, a.kernel_args(), a.rn, __VA_ARGS__);         \
            else {                                                                                                                   \
                if (a.form != plan::RenewForm::Plain) return -1;                                                                     \
                launch(Fam::template plain<V...>(), grid, lds_bytes, stream, a.kernel_args(), __VA_ARGS__);                          \
                return 0;                                                                                                            \
            }                                                                                                                        \
        }                                                                                                                            \
    };                                                                                                                               \
    }                                                                                                                                \
    int dcm::launch_rollout_##FORM(plan::SimKind kind, bool fast, bool obs, unsigned grid, Lay L, hipStream_t stream, const RolloutArgs& a) { \
        return launch_rollout_form<FORM##_form>(kind, fast, obs, grid, L, stream, a);                                                \
    }                                                                                                                                \
    void dcm::allow_lds_##FORM(int lds) { allow_lds_form<FORM##_form>(lds); }
// Each pair inside its unit's guard: a device-only unit learns from here which kernels to instantiate
#ifdef DCM_HAVE_POLICY
DCM_FORM_LAUNCHERS(policy, k_hp_, k_hprn_, a.policy)
#endif
#ifdef DCM_HAVE_LOG
DCM_FORM_LAUNCHERS(log, k_lg_, k_lgrn_, a.policy, a.lg)
#endif
#ifdef DCM_HAVE_EXPLORE
DCM_FORM_LAUNCHERS(explore, k_ex_, k_exrn_, a.policy, a.explore_q32, a.lg)
#endif
#ifdef DCM_HAVE_BEST
DCM_PLAIN_FORM_LAUNCHERS(best, k_bs_, a.policy, a.explore_q32, a.lg, a.best)
#endif
#undef DCM_FORM_LAUNCHERS_
#undef DCM_PLAIN_FORM_LAUNCHERS
#undef DCM_FORM_LAUNCHERS
// The lookahead form has the general family alone (no k_la_rollout_fast): written out instead of a third shape of the macro above
#ifdef DCM_HAVE_LOOKAHEAD
namespace {
struct lookahead_general { DCM_FORMS(k_la_rollout_random, k_larn_rollout_random) };
}
int dcm::launch_rollout_lookahead(plan::SimKind kind, bool, bool, unsigned grid, Lay L, hipStream_t stream, const RolloutArgs& a) {
    return with_sim(kind, [&](auto s) {
        using S = decltype(s);
        return launch_family<lookahead_general, false, SIM_ARGS(S), S::MC>(a.form, grid, rollout_random_lds_bytes<SIM_ARGS(S)>(L), stream,
                                                                           a.kernel_args(), a.rn, a.policy, a.lg, a.snap, a.width,
                                                                           a.inner_out);
    });
}
void dcm::allow_lds_lookahead(int lds) {
    for_each_sim([&](auto s) {
        using S = decltype(s);
        allow_lds(lds, lookahead_general::plain<SIM_ARGS(S), S::MC>(), lookahead_general::renewing<SIM_ARGS(S), S::MC>());
    });
}
#endif
// The individual-selection form likewise: the general family alone (no k_is_rollout_fast)
#ifdef DCM_HAVE_INDIVIDUAL
namespace {
struct individual_general { DCM_FORMS(k_is_rollout_random, k_isrn_rollout_random) };
}
int dcm::launch_rollout_individual(plan::SimKind kind, bool, bool, unsigned grid, Lay L, hipStream_t stream, const RolloutArgs& a) {
    return with_sim(kind, [&](auto s) {
        using S = decltype(s);
        return launch_family<individual_general, false, SIM_ARGS(S), S::MC>(a.form, grid, rollout_random_lds_bytes<SIM_ARGS(S)>(L), stream,
                                                                            a.kernel_args(), a.rn, a.policy, a.explore_q32, a.lg);
    });
}
void dcm::allow_lds_individual(int lds) {
    for_each_sim([&](auto s) {
        using S = decltype(s);
        allow_lds(lds, individual_general::plain<SIM_ARGS(S), S::MC>(), individual_general::renewing<SIM_ARGS(S), S::MC>());
    });
}
#endif
#undef DCM_FORMS
#undef DCM_FORM

#ifdef DCM_HAVE_FAST_G
void dcm::launch_rollout_fast_g(int nac, int ntc, bool obs, unsigned grid, Lay L, hipStream_t stream, const RolloutArgs& a) {
    with_bool(obs, [&](auto obs_c) {
        with_bool(nac > 1, [&](auto two_c) {
            auto go = [&](auto ntc_c) {
                launch_family<rollout_fast_g_family, true, decltype(two_c)::value ? 2 : 1, decltype(ntc_c)::value, decltype(obs_c)::value>(
                    a.form, grid, rollout_fast_g_lds_bytes(L), stream, a.kernel_args(), a.rn);
            };
            if (ntc > 3) go(std::integral_constant<int, 4>{});
            else if (ntc > 2) go(std::integral_constant<int, 3>{});
            else go(std::integral_constant<int, 2>{});
        });
    });
}
#endif

#ifndef DCM_DEVICE_ONLY_TU   // (tools/loop_insts.py compiles single kernel instantiations of this file without the host API)
namespace {
constexpr uint32_t CU_LDS_BYTES = 160u * 1024u;
// the end of a launch: rc = -1 from with_sim / launch_family says that plan.hpp sent it to a kernel that does not exist
int launched(int rc) {
    if (rc != 0) return fail(DCM_ERR_STATE, "internal error: no such kernel for the handle's layout and renewal form");
    LAUNCH_OK();
    return DCM_OK;
}

// The most dynamic LDS any kernel of this file asks for on a layout: the general image with the wake-up times of the multi-chunk
// layouts, or record + scratch where the persistent kernels keep the scratch in LDS (Sim::SCR_IN_LDS); then the dummy slots
int largest_lds_request(Lay L) {
    uint32_t lds = Sim<0, 0, false>::lds_image_bytes(L);
    if (L.lds_bytes() <= 10240) lds = L.lds_bytes();
    if (lds + DUMMY_SLOT_BYTES <= CU_LDS_BYTES) lds += DUMMY_SLOT_BYTES;
    return (int)lds;
}
// ADVICE.md item 2 is to be fixed here: an error from hipStreamIsCapturing counts as "capturing"
bool stream_capturing(void* stream) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    return hipStreamIsCapturing((hipStream_t)stream, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone;
}

// the last argument of the renewing kernel forms (k_rn_*, k_rs_*), which are launched while the stride is not 0; on a ragged batch
// (k_rs_*) env->gen holds the real ranges
Renew renew_args(const dcm_env* env) { return Renew{env->inst_seeds, env->renew_stride, env->gen}; }
bool renew_sizes_opted_in(const dcm_env* env) { return (env->p.flags & DCM_PARAM_RENEW_SIZES) != 0; }
// The form the handle's next launch of a restarting kernel takes (plan::renew_form); changes nothing
plan::RenewForm launch_form(const dcm_env* env) {
    return plan::renew_form(shape_of(env), env->renew_stride != 0, renew_sizes_opted_in(env));
}
// ... and what the host has to note when that launch is really about to be made.  While the stride is set it is a renewing one: it
// may replace instances, so the restart image of k_step_fast (dcm_env::init, the records as dcm_reset saw them) is no longer theirs
// -- also after the stride is cleared.  Captured, the launch replaces instances at every replay, unseen by the host: the handle then
// counts as captured, which keeps dcm_step from using an image for good.  Called behind every check that can still refuse the call.
plan::RenewForm renewing_launch(dcm_env* env, void* stream) {
    const plan::RenewForm form = launch_form(env);
    if (form == plan::RenewForm::Plain) return form;
    env->init_valid = false;
    if (stream_capturing(stream)) env->captured = true;
    return form;
}
// the handle's instances no longer come from dcm_generate_instances, or come from a new call of it: renewal is off
void renewal_off(dcm_env* env, bool generated) { env->generated = generated; env->renew_stride = 0; }

// plan::Shape::inrange of the records as they stand, for instances that were not made on the device: one small kernel over the
// records and one word read back, so the call waits for the stream -- where instances are loaded or a state is restored, never at a
// launch.  Only a handle whose shape could take the Fast<> kernels at all is looked at.  Under stream capture nothing can be read
// back: the handle then takes the general kernels until its instances are next loaded, generated or restored.
int check_points_inrange(dcm_env* env, void* stream) {
    env->inrange = true;
    if (!plan::one_chunk_ok(shape_of(env))) return DCM_OK;
    env->inrange = false;
    if (stream_capturing(stream)) return DCM_OK;
    if (!env->inrange_bad) HIP_TRY(hipMalloc((void**)&env->inrange_bad, sizeof(uint32_t)));
    HIP_TRY(hipMemsetAsync(env->inrange_bad, 0, sizeof(uint32_t), (hipStream_t)stream));
    hipLaunchKernelGGL(k_points_inrange, GRID(env), 0, (hipStream_t)stream, DIMS(env), env->L.C, (const unsigned char*)env->state,
                       (const int32_t*)env->sizes, env->inrange_bad);
    LAUNCH_OK();
    uint32_t bad = 1;
    HIP_TRY(hipMemcpyAsync(&bad, env->inrange_bad, sizeof(uint32_t), hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    env->inrange = bad == 0;
    return DCM_OK;
}

// the common tail of dcm_load_instances / dcm_load_instances_ragged (env->sizes: the per-env sizes of a ragged batch, or nullptr)
int launch_load(dcm_env* env, const double* depot, const double* task_xy, const int32_t* req, const double* dur, void* stream) {
    hipLaunchKernelGGL(k_load_instances, GRID(env), 0, (hipStream_t)stream, DIMS(env), env->L.C, env->state, depot, task_xy,
                       req, dur, (const int32_t*)env->sizes);
    LAUNCH_OK();
    env->loaded = true;
    env->reset_done = false;
    renewal_off(env, false);
    return check_points_inrange(env, stream);
}

// dcm_env_status / dcm_env_episodes: header fields of every env (layout dims: only the record pitch matters)
int launch_env_status(dcm_env* env, uint32_t* flags_out, int64_t* decisions_out, double* now_out, int32_t* episodes_out, void* stream) {
    const int B = env->p.n_envs;
    hipLaunchKernelGGL(k_env_status, dim3((B + WAVE - 1) / WAVE), dim3(WAVE), 0, (hipStream_t)stream, env->L.A, env->L.T, env->L.C,
                       env->state, B, flags_out, decisions_out, now_out, episodes_out);
    LAUNCH_OK();
    return DCM_OK;
}

// the blob of dcm_state_bytes / dcm_clone_state / dcm_restore_state: these sections of the handle, in this order
// (the last one only where the per-env sizes can change after the load: a ragged batch on a DCM_PARAM_RENEW_SIZES handle; else empty)
struct Section { void* ptr; size_t bytes; };
std::array<Section, 4> state_sections(const dcm_env* env) {
    const size_t B = (size_t)env->p.n_envs;
    const bool with_sizes = env->sizes && renew_sizes_opted_in(env);
    return {{{env->state, B * env->L.rec_bytes()}, {env->summary, B * 8 * sizeof(double)},
             {env->ablog, side_bytes(env->p.n_envs, env->A, env->T)}, {env->sizes, with_sizes ? B * 2 * sizeof(int32_t) : 0}}};
}

// the arguments every persistent rollout kernel starts with, from the handle and the call
dcm::RolloutArgs rollout_args(const dcm_env* env, plan::RenewForm form, int32_t episodes, int64_t max_decisions, const int64_t* max_decisions_in,
                              float* agents_out, float* tasks_out, uint8_t* mask_out, int64_t* steps_out) {
    return {DIMS(env), env->kp, env->state, (int)episodes, agents_out, tasks_out, mask_out, steps_out, env->summary,
            env->ablog, env->sizes, max_decisions, max_decisions_in, env->gscratch, env->retlog,
            (int)env->retcap, renew_args(env), form};
}

// A greedy, logging or epsilon-greedy form to the host: its launcher, and what `fn` says when a size-renewing launch asks for it
// (keeps_best: the best-keeping form, which rollout_form also refuses without the rollout log and while any renewal stride is set)
// (lookahead: the lookahead form, which has no one-chunk kernels -- every shape takes the general text -- and whose snapshot buffer
//  rollout_form allocates at the first launch)
// (general_only: the lookahead and the individual-selection form, which have no one-chunk kernels -- every shape takes the general text)
struct RolloutForm { dcm::FormLauncher* launch; const char* no_sizes_form; bool keeps_best = false; bool lookahead = false; bool general_only = lookahead; };
const RolloutForm FORM_POLICY{dcm::launch_rollout_policy,
    "%s: no greedy policy while a ragged batch renews its sizes (DCM_PARAM_RENEW_SIZES with a stride set): "
    "clear the stride with dcm_set_instance_renewal(env, 0), or use DCM_POLICY_RANDOM"};
const RolloutForm FORM_LOG{dcm::launch_rollout_log,
    "%s: no rollout log while a ragged batch renews its sizes (DCM_PARAM_RENEW_SIZES with a stride set): "
    "clear the stride with dcm_set_instance_renewal(env, 0), or clear the log with dcm_set_rollout_log(env, NULL, NULL, NULL, 0)"};
const RolloutForm FORM_EXPLORE{dcm::launch_rollout_explore,
    "%s: no epsilon-greedy policy while a ragged batch renews its sizes (DCM_PARAM_RENEW_SIZES with a stride "
    "set): clear the stride with dcm_set_instance_renewal(env, 0), or use dcm_rollout_random"};
const RolloutForm FORM_BEST{dcm::launch_rollout_best,
    "%s: no best log while instances are renewed (the best episode of different instances means nothing): clear the stride with "
    "dcm_set_instance_renewal(env, 0), or clear the best log with dcm_set_best_log(env, NULL, NULL, NULL, NULL, NULL)", true};
const RolloutForm FORM_LOOKAHEAD{dcm::launch_rollout_lookahead,
    "%s: no lookahead while a ragged batch renews its sizes (DCM_PARAM_RENEW_SIZES with a stride set): clear the stride with "
    "dcm_set_instance_renewal(env, 0)", false, true};
const RolloutForm FORM_INDIVIDUAL{dcm::launch_rollout_individual,
    "%s: no individual-selection launch while a ragged batch renews its sizes (DCM_PARAM_RENEW_SIZES with a stride set): clear the "
    "stride with dcm_set_instance_renewal(env, 0)", false, false, true};
// the form an entry point takes: the best-keeping one while dcm_set_best_log is set, else its own
const RolloutForm& form_of(const dcm_env* env, const RolloutForm& own) { return env->best_log.episode ? FORM_BEST : own; }

// The common tail of the entry points that launch such a form: dcm_rollout_policy, dcm_rollout_explore, and dcm_rollout_random /
// dcm_rollout_policy while the rollout log is set (FORM_LOG, under any of the three policies).  The caller `fn` has validated its
// arguments.  explore_q32: 0 and 2^32 run the same kernels as every other value, no shortcut to the greedy / random forms.
// While dcm_set_best_log is set every one of them comes here with FORM_BEST (form_of), which needs the rollout log and no stride.
int rollout_form(dcm_env* env, const char* fn, const RolloutForm& form, int32_t policy, uint64_t explore_q32, int32_t episodes,
                 int64_t max_decisions, const int64_t* max_decisions_in, float* agents_out, float* tasks_out, uint8_t* mask_out,
                 int64_t* steps_out, void* stream, int32_t width = 0, int64_t* inner_out = nullptr) {
    if (form.keeps_best) {
        if (!env->rollout_log.len)
            return fail(DCM_ERR_STATE, "%s: the best log is set and the rollout log is not: the kept episode is copied from it; call "
                                       "dcm_set_rollout_log first, or clear the best log with dcm_set_best_log(env, NULL, NULL, NULL, NULL, NULL)", fn);
        if (env->renew_stride != 0) return fail(DCM_ERR_STATE, form.no_sizes_form, fn);
    }
    if (!plan::form_ok(launch_form(env))) return fail(DCM_ERR_STATE, form.no_sizes_form, fn);
    if (form.lookahead && !env->la_snap) {
        // per env one env's share of the dcm_clone_state blob: record, 64 B, abandonment rows, overflow counts.  Allocated here, at
        // the first lookahead launch, behind every refusal: hipMalloc is not allowed while the stream is capturing
        if (stream_capturing(stream))
            return fail(DCM_ERR_STATE, "%s: the first call on a handle allocates the snapshot buffer and cannot be captured into a graph: "
                                       "call it once outside the capture", fn);
        const size_t pitch = (size_t)env->L.rec_bytes() + 64u + 2u * AB_CAP * (size_t)env->A + abcnt_pitch(env->A, env->T);
        if (hipMalloc((void**)&env->la_snap, (size_t)env->p.n_envs * pitch) != hipSuccess) {
            (void)hipGetLastError();
            env->la_snap = nullptr;
            return fail(DCM_ERR_HIP, "%s: hipMalloc of the snapshot buffer failed", fn);
        }
    }
    DCM_TRY(dcm::flush_pending(env, stream));
    dcm::RolloutArgs ra = rollout_args(env, renewing_launch(env, stream), episodes, max_decisions, max_decisions_in, agents_out, tasks_out,
                                       mask_out, steps_out);
    ra.policy = policy;
    ra.explore_q32 = explore_q32;
    ra.lg = env->rollout_log;          // (the epsilon-greedy forms take it set or not: one set of forms)
    ra.best = env->best_log;
    ra.snap = env->la_snap;
    ra.width = width;                  // (the lookahead form alone: dcm_rollout_lookahead_width)
    ra.inner_out = inner_out;
    const bool all_obs = agents_out && tasks_out && mask_out, no_obs = !agents_out && !tasks_out && !mask_out;
    const plan::Shape shape = shape_of(env);
    const bool fast = !form.general_only && plan::form_rollout_kind(shape, all_obs || no_obs) == plan::Rollout::Fast;
    return launched(form.launch(plan::sim_kind(shape), fast, all_obs, (unsigned)env->p.n_envs, env->L, (hipStream_t)stream, ra));
}

// plan::policy_needs_budget: `fn` refuses an unlimited greedy launch there
int need_budget(const dcm_env* env, const char* fn, int64_t max_decisions, const int64_t* max_decisions_in) {
    if (plan::policy_needs_budget(shape_of(env)) && !max_decisions_in && max_decisions < 0)
        return fail(DCM_ERR_INVALID, "%s: with max_waiting_time <= 0 a greedy policy does not end its episodes (a dropped member takes "
                                     "the same task again at the same time): give a decision budget", fn);
    return DCM_OK;
}

// dcm_rollout_lookahead (width 0, no inner_out) and dcm_rollout_lookahead_width: one set of refusals, each message under the name `fn`
int rollout_lookahead(dcm_env* env, const char* fn, int32_t base_policy, int32_t width, int32_t episodes, int64_t max_decisions,
                      const int64_t* max_decisions_in, float* agents_out, float* tasks_out, uint8_t* mask_out, int64_t* steps_out,
                      int64_t* inner_out, void* stream) {
    CHECK_ENV(env);
    if (base_policy != DCM_POLICY_RANDOM && base_policy != DCM_POLICY_FIRST && base_policy != DCM_POLICY_NEAREST)
        return fail(DCM_ERR_INVALID, "%s: unknown base policy (DCM_POLICY_RANDOM, DCM_POLICY_FIRST, DCM_POLICY_NEAREST)", fn);
    if (width < 0) return fail(DCM_ERR_INVALID, "%s: width must be >= 0 (0: every unmasked action is valued)", fn);
    if (episodes < 1) return fail(DCM_ERR_INVALID, "%s: episodes must be >= 1", fn);
    // every inner episode must end by itself; a decision budget bounds the outer decisions only
    if (!(env->kp.mwt > 0.0))
        return fail(DCM_ERR_INVALID, "%s: the handle has max_waiting_time <= 0, where a base policy does not end its episodes "
                                     "(a dropped member takes the same task again at the same time): an action has no episode to be valued by, "
                                     "with or without a decision budget", fn);
    if (!env->reset_done) return fail(DCM_ERR_STATE, "%s: call dcm_reset first", fn);
    if (env->best_log.episode)
        return fail(DCM_ERR_STATE, "%s: the best log is set and there is no best-keeping lookahead form: clear it with "
                                   "dcm_set_best_log(env, NULL, NULL, NULL, NULL, NULL)", fn);
    return rollout_form(env, fn, FORM_LOOKAHEAD, base_policy, 0, episodes, max_decisions, max_decisions_in, agents_out, tasks_out, mask_out,
                        steps_out, stream, width, inner_out);
}
}  // namespace

extern "C" {

const char* dcm_last_error(void) { return dcm::g_err; }
int dcm_abi_version(void) { return DCM_ABI_VERSION; }
#ifndef DCM_BUILD_ID
#define DCM_BUILD_ID "unknown"
#endif
const char* dcm_build_id(void) { return DCM_BUILD_ID; }
// plan.hpp's answer for the handle as it stands, by the kernel's base name
const char* dcm_kernel_name(dcm_env* env, int32_t entry) {
    if (!env) { (void)dcm::fail(DCM_ERR_INVALID, "null env handle"); return nullptr; }
    const plan::Shape shape = shape_of(env);
    if (entry == DCM_KERNEL_STEP) return plan::one_chunk_ok(shape) ? "k_step_fast" : "k_step";
    if (entry != DCM_KERNEL_ROLLOUT) { (void)dcm::fail(DCM_ERR_INVALID, "dcm_kernel_name: unknown entry"); return nullptr; }
    switch (plan::rollout_kind(shape, true)) {
    case plan::Rollout::Fast: return "k_rollout_fast";
    case plan::Rollout::FastMc: return "k_rollout_fast_mc";
    case plan::Rollout::FastG: return "k_rollout_fast_g";
    default: return "k_rollout_random";
    }
}
#ifdef DCM_COUNT_PATHS
// developer build only (tools/path_counts.py): read and clear the dynamic path counts of the register-resident rollout kernel
int dcm_debug_path_counts(unsigned long long* out32) {
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpyFromSymbol(out32, HIP_SYMBOL(g_path_counts), 32 * sizeof(unsigned long long)));
    static const unsigned long long zero[32] = {};
    HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_path_counts), zero, sizeof(zero)));
    return 0;
}
#endif

int dcm_create(const dcm_params* params, dcm_env** out) {
    if (!params || !out) return fail(DCM_ERR_INVALID, "dcm_create: null argument");
    *out = nullptr;
    if (params->n_envs < 1 || params->n_agents < 1 || params->n_agents > DCM_MAX_AGENTS || params->n_tasks < 1 ||
        params->n_tasks > DCM_MAX_TASKS)
        return fail(DCM_ERR_INVALID, "dcm_create: need 1<=A<=128, 1<=T<=1023, B>=1");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
        return fail(DCM_ERR_NO_DEVICE, "dcm_create: no HIP device (this library has no CPU path)");
    if (params->device < 0 || params->device >= ndev) return fail(DCM_ERR_INVALID, "dcm_create: bad device ordinal");
    DeviceGuard guard(params->device);
    dcm_env* h = new (std::nothrow) dcm_env();
    if (!h) return fail(DCM_ERR_INVALID, "dcm_create: out of host memory");
    h->p = *params;
    h->A = params->n_agents; h->T = params->n_tasks;
    const plan::LayDims ld = plan::layout_dims(h->A, h->T, (params->flags & DCM_PARAM_WIDE_MEMBERS) != 0);
    h->L = Lay{ld.A, ld.T, ld.C};
    h->kp.mwt = params->max_waiting_time;
    h->kp.max_time = params->max_time;
    // (from here on dcm_destroy frees whatever the partly built handle holds)
    if (Sim<0, 0, false>::lds_image_bytes(h->L) > CU_LDS_BYTES) { dcm_destroy(h); return fail(DCM_ERR_INVALID, "dcm_create: env record does not fit the 160 KiB LDS"); }
    const size_t B = (size_t)params->n_envs, bytes = B * h->L.rec_bytes(), side = side_bytes(params->n_envs, h->A, h->T);
    hipError_t e = hipMalloc((void**)&h->state, bytes);
    if (e == hipSuccess) e = hipMalloc((void**)&h->summary, B * 8 * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void**)&h->ablog, side);
    if (e == hipSuccess) e = hipMalloc((void**)&h->gscratch, B * h->L.scratch_bytes());
    if (e != hipSuccess) { dcm_destroy(h); return fail(DCM_ERR_HIP, "dcm_create: hipMalloc failed: %s", hipGetErrorString(e)); }
    e = hipMemset(h->state, 0, bytes);
    if (e == hipSuccess) e = hipMemset(h->ablog, 0, side);
    if (e != hipSuccess) { dcm_destroy(h); return fail(DCM_ERR_HIP, "hipMemset: %s", hipGetErrorString(e)); }
    *out = h;
    // kernels that keep the record in LDS may need more than the default 64 KiB of dynamic LDS.  The limit is a
    // per-function, per-device attribute shared by every handle of the process, so it only ever grows: a later, smaller
    // env must not lower it under an earlier handle's launches.
    static int lds_limit[64] = {0};
    static std::mutex lds_mutex;                 // handles are created from several host threads (one actor thread per GPU)
    std::lock_guard<std::mutex> lds_guard(lds_mutex);
    const int dev_slot = params->device & 63;
    const int lds = largest_lds_request(h->L);
    // (only when the limit really grows: the attribute calls of one host thread must not keep landing in another thread's
    //  stream capture -- actors create handles for new batch shapes while others capture)
    if (lds <= lds_limit[dev_slot]) return DCM_OK;
    lds_limit[dev_slot] = lds;
    // every kernel that takes the record into LDS, from the tables the launches use (in the order the main unit's assembly has them)
    for_each_sim([&](auto s) {
        using S = decltype(s);
        allow_lds(lds, k_reset<SIM_ARGS(S), S::MC>, k_observe<SIM_ARGS(S), S::MC>);
        allow_lds(lds, step_family::plain<SIM_ARGS(S), S::MC>(), rollout_random_family::plain<SIM_ARGS(S), S::MC>(),
                  step_family::renewing<SIM_ARGS(S), S::MC>(), rollout_random_family::renewing<SIM_ARGS(S), S::MC>());
    });
    for_each_sim([&](auto s) {
        using S = decltype(s);
        if constexpr (S::reads_sizes)
            allow_lds(lds, step_family::size_renewing<SIM_ARGS(S), S::MC>(), rollout_random_family::size_renewing<SIM_ARGS(S), S::MC>());
    });
    using fast = rollout_fast_family;                    // <..., OBS, PRIO>: both OBS, without and with wave priorities
    for_each_sim([&](auto s) {
        using S = decltype(s);
        if constexpr (S::one_chunk) {
            allow_lds(lds, fast::plain<SIM_ARGS(S), true>(), fast::plain<SIM_ARGS(S), false>(), fast::plain<SIM_ARGS(S), true, true>(),
                      fast::plain<SIM_ARGS(S), false, true>(), step_fast_family::plain<SIM_ARGS(S)>());
            allow_lds(lds, fast::renewing<SIM_ARGS(S), true>(), fast::renewing<SIM_ARGS(S), false>(), fast::renewing<SIM_ARGS(S), true, true>(),
                      fast::renewing<SIM_ARGS(S), false, true>(), step_fast_family::renewing<SIM_ARGS(S)>());
        }
    });
    for_each_sim([&](auto s) {
        using S = decltype(s);
        if constexpr (S::one_chunk && S::reads_sizes)
            allow_lds(lds, fast::size_renewing<SIM_ARGS(S), true>(), fast::size_renewing<SIM_ARGS(S), false>(),
                      fast::size_renewing<SIM_ARGS(S), true, true>(), fast::size_renewing<SIM_ARGS(S), false, true>(),
                      step_fast_family::size_renewing<SIM_ARGS(S)>());
    });
    using mc = rollout_fast_mc_family;
    allow_lds(lds, mc::plain<50, 200, true>(), mc::plain<50, 200, false>(), mc::renewing<50, 200, true>(), mc::renewing<50, 200, false>());
    dcm::allow_lds_policy(lds);
    dcm::allow_lds_log(lds);
    dcm::allow_lds_explore(lds);
    dcm::allow_lds_best(lds);
    dcm::allow_lds_lookahead(lds);
    dcm::allow_lds_individual(lds);
    allow_lds(lds, k_get_tasks<M>, k_get_agents<M>, k_get_tasks<MW>, k_get_agents<MW>);
    return DCM_OK;
}

int dcm_destroy(dcm_env* env) {
    if (!env) return DCM_OK;
    DeviceGuard guard(env->p.device);
    void* const owned[] = {env->state, env->summary, env->ablog, env->gscratch, env->routes, env->route_len,
                           env->rmarr, env->sizes, env->side, env->pendq, env->init, env->inst_seeds, env->la_snap, env->inrange_bad};
    for (void* p : owned)
        if (p) (void)hipFree(p);
    delete env;
    return DCM_OK;
}

int dcm_load_instances(dcm_env* env, const double* depot, const double* task_xy, const int32_t* req, const double* dur,
                       void* stream) {
    CHECK_ENV(env);
    if (!depot || !task_xy || !req || !dur) return fail(DCM_ERR_INVALID, "dcm_load_instances: null array");
    DCM_TRY(dcm::drop_pending(env, stream));
    if (env->sizes) { HIP_TRY(hipFree(env->sizes)); env->sizes = nullptr; }   // back to a uniform batch (hipFree synchronises)
    return launch_load(env, depot, task_xy, req, dur, stream);
}

int dcm_load_instances_ragged(dcm_env* env, const double* depot, const double* task_xy, const int32_t* req,
                              const double* dur, const int32_t* n_agents_host, const int32_t* n_tasks_host, void* stream) {
    CHECK_ENV(env);
    DCM_TRY(dcm::drop_pending(env, stream));
    if (!depot || !task_xy || !req || !dur || !n_agents_host || !n_tasks_host)
        return fail(DCM_ERR_INVALID, "dcm_load_instances_ragged: null array");
    const int B = env->p.n_envs;
    env->sizes_host.resize((size_t)2 * B);
    for (int e = 0; e < B; e++) {
        const int a = n_agents_host[e], t = n_tasks_host[e];
        if (a < 1 || a > env->A || t < 1 || t > env->T)
            return fail(DCM_ERR_INVALID, "dcm_load_instances_ragged: need 1 <= n_agents[e] <= A and 1 <= n_tasks[e] <= T");
        env->sizes_host[2 * (size_t)e] = a; env->sizes_host[2 * (size_t)e + 1] = t;
    }
    if (!env->sizes) HIP_TRY(hipMalloc((void**)&env->sizes, (size_t)2 * B * sizeof(int32_t)));
    HIP_TRY(hipMemcpyAsync(env->sizes, env->sizes_host.data(), (size_t)2 * B * sizeof(int32_t), hipMemcpyHostToDevice,
                           (hipStream_t)stream));
    return launch_load(env, depot, task_xy, req, dur, stream);
}

// TaskEnv(agents_range, tasks_range, max_coalition_size, max_duration, seed=inst_seeds[e]) for every env, made on the device
int dcm_generate_instances(dcm_env* env, const uint64_t* inst_seeds, int32_t agents_lo, int32_t agents_hi, int32_t tasks_lo,
                           int32_t tasks_hi, int32_t max_coalition_size, double max_duration, void* stream) {
    CHECK_ENV(env);
    if (!inst_seeds) return fail(DCM_ERR_INVALID, "dcm_generate_instances: null seeds");
    if (agents_lo < 1 || agents_lo > agents_hi || agents_hi > env->A || tasks_lo < 1 || tasks_lo > tasks_hi || tasks_hi > env->T)
        return fail(DCM_ERR_INVALID, "dcm_generate_instances: need 1 <= agents_lo <= agents_hi <= A and 1 <= tasks_lo <= tasks_hi <= T");
    if (max_coalition_size < 1 || max_coalition_size > env->L.C)
        return fail(DCM_ERR_INVALID, "dcm_generate_instances: need 1 <= max_coalition_size <= the member slots of the handle");
    if (!(max_duration >= 0.0)) return fail(DCM_ERR_INVALID, "dcm_generate_instances: need max_duration >= 0");
    DCM_TRY(dcm::drop_pending(env, stream));
    // renewal is off before the sizes or the kept seeds change: a failure below cannot leave it on with seeds that are not the records'
    renewal_off(env, false);
    const bool uniform = agents_lo == env->A && tasks_lo == env->T;    // (lo <= hi <= the dim: both ranges zero-width at the dims)
    if (uniform && env->sizes) { HIP_TRY(hipFree(env->sizes)); env->sizes = nullptr; }
    if (!uniform && !env->sizes) HIP_TRY(hipMalloc((void**)&env->sizes, (size_t)2 * env->p.n_envs * sizeof(int32_t)));
    // the handle keeps the seeds and the scalar arguments: what a renewal draws the env's later instances from
    const size_t seed_bytes = (size_t)env->p.n_envs * sizeof(uint64_t);
    if (!env->inst_seeds) HIP_TRY(hipMalloc((void**)&env->inst_seeds, seed_bytes));
    HIP_TRY(hipMemcpyAsync(env->inst_seeds, inst_seeds, seed_bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    const GenArgs g{agents_lo, agents_hi, tasks_lo, tasks_hi, max_coalition_size, max_duration};
    hipLaunchKernelGGL(k_generate_instances, GRID(env), 0, (hipStream_t)stream, env->L.A, env->L.T, env->L.C, env->state, inst_seeds, g,
                       env->sizes);
    LAUNCH_OK();
    env->loaded = true;
    env->reset_done = false;
    env->gen = g;
    env->inrange = true;              // coordinates are multiples of 2^-53 (plan::Shape::inrange), renewed instances included
    renewal_off(env, true);
    return DCM_OK;
}

int dcm_get_instances(dcm_env* env, double* depot, double* task_xy, int32_t* req, double* dur, int32_t* n_agents, int32_t* n_tasks,
                      void* stream) {
    CHECK_ENV(env);
    if (!env->loaded) return fail(DCM_ERR_STATE, "dcm_get_instances: no instances loaded");
    hipLaunchKernelGGL(k_get_instances, GRID(env), 0, (hipStream_t)stream, DIMS(env), env->L.C, (const unsigned char*)env->state,
                       (const int32_t*)env->sizes, depot, task_xy, req, dur, n_agents, n_tasks);
    LAUNCH_OK();
    return DCM_OK;
}

int dcm_set_instance_renewal(dcm_env* env, uint64_t stride) {
    CHECK_HANDLE(env);
    const bool generated = env->loaded && env->generated;
    if (stride != 0 && !plan::renewal_ok(shape_of(env), generated) && !plan::renewal_sizes_ok(shape_of(env), generated, renew_sizes_opted_in(env)))
        return fail(DCM_ERR_STATE, "dcm_set_instance_renewal: needs a batch made by dcm_generate_instances, uniform unless the handle has DCM_PARAM_RENEW_SIZES");
    env->renew_stride = stride;
    return DCM_OK;
}

int dcm_instance_index(dcm_env* env, uint32_t* index_out, void* stream) {
    CHECK_ENV(env);
    if (!index_out) return fail(DCM_ERR_INVALID, "dcm_instance_index: null index_out");
    if (!env->loaded) return fail(DCM_ERR_STATE, "dcm_instance_index: no instances loaded");
    const int B = env->p.n_envs;
    hipLaunchKernelGGL(k_instance_index, dim3((B + WAVE - 1) / WAVE), dim3(WAVE), 0, (hipStream_t)stream, env->L.A, env->L.T, env->L.C,
                       (const unsigned char*)env->state, B, index_out);
    LAUNCH_OK();
    return DCM_OK;
}

int dcm_generator_draws(const uint64_t* seeds, int64_t n, int32_t n_doubles, uint32_t bound, int32_t n_ints, double* doubles_out,
                        uint32_t* ints_out, void* stream) {
    if (!seeds || n < 0 || n > INT32_MAX || n_doubles < 0 || n_ints < 0 || bound < 1 || (n_doubles > 0 && !doubles_out) ||
        (n_ints > 0 && !ints_out))
        return fail(DCM_ERR_INVALID, "dcm_generator_draws: bad argument");
    if (n == 0) return DCM_OK;
    hipLaunchKernelGGL(k_generator_draws, dim3((unsigned)n), dim3(WAVE), 0, (hipStream_t)stream, seeds, n_doubles, bound - 1u, n_ints,
                       doubles_out, ints_out);
    LAUNCH_OK();
    return DCM_OK;
}

}  // extern "C"

namespace dcm {
int flush_pending(dcm_env* env, void* stream) {
    if (!env->maybe_pending) return DCM_OK;
    const auto args = std::make_tuple(DIMS(env), env->kp, env->side, env->side_pitch, env->pendq, env->summary, env->sizes, env->gscratch);
    const int rc = with_sim(sim_of(env), [&](auto s) {
        using S = decltype(s);
        if constexpr (S::one_chunk) {
            launch(k_terminal_flush<SIM_ARGS(S)>, (unsigned)env->p.n_envs, step_fast_lds_bytes<SIM_ARGS(S)>(env->L), (hipStream_t)stream, args);
            return 0;
        } else return -1;
    });
    DCM_TRY(launched(rc));
    env->maybe_pending = false;
    env->steps_since_flush = 0;
    return DCM_OK;
}
int drop_pending(dcm_env* env, void* stream) {
    if (!env->maybe_pending) return DCM_OK;
    HIP_TRY(hipMemsetAsync(env->pendq, 0, (size_t)env->p.n_envs * sizeof(uint32_t), (hipStream_t)stream));
    env->maybe_pending = false;
    env->steps_since_flush = 0;
    return DCM_OK;
}
}  // namespace dcm

extern "C" {

int dcm_reset(dcm_env* env, const uint64_t* seeds, void* stream) {
    CHECK_ENV(env);
    DCM_TRY(dcm::drop_pending(env, stream));
    if (!env->loaded) return fail(DCM_ERR_STATE, "dcm_reset: call dcm_load_instances first");
    if (!seeds) return fail(DCM_ERR_INVALID, "dcm_reset: null seeds");
    const auto args = std::make_tuple(DIMS(env), env->kp, env->state, seeds, env->summary, env->ablog, env->p.flags, env->sizes, env->gscratch);
    DCM_TRY(launched(with_sim(sim_of(env), [&](auto s) {
        using S = decltype(s);
        launch(k_reset<SIM_ARGS(S), S::MC>, (unsigned)env->p.n_envs, env_kernel_lds_bytes<SIM_ARGS(S)>(env->L), (hipStream_t)stream, args);
        return 0;
    })));
    if (env->log.len)
        HIP_TRY(hipMemsetAsync(env->log.len, 0, (size_t)env->p.n_envs * env->A * sizeof(int32_t), (hipStream_t)stream));
    if (env->rollout_log.len)
        HIP_TRY(hipMemsetAsync(env->rollout_log.len, 0, (size_t)env->p.n_envs * env->A * sizeof(int32_t), (hipStream_t)stream));
    if (env->best_log.episode) {       // no episode kept: ordinal -1, a NaN summary row (all bits set), lengths 0
        const size_t B = (size_t)env->p.n_envs;
        HIP_TRY(hipMemsetAsync(env->best_log.episode, 0xFF, B * sizeof(int32_t), (hipStream_t)stream));
        HIP_TRY(hipMemsetAsync(env->best_log.summary, 0xFF, B * 8 * sizeof(double), (hipStream_t)stream));
        HIP_TRY(hipMemsetAsync(env->best_log.len, 0, B * env->A * sizeof(int32_t), (hipStream_t)stream));
    }
    env->reset_done = true;
    // the restart image of the register-resident lockstep kernel (dcm_env::init, read by k_step_fast only): what this reset produced
    env->init_valid = false;
    // (max_time <= 0: the first event already ends the episode -- summary row, episode count, return log -- which a copied image cannot redo)
    if ((env->p.flags & DCM_PARAM_AUTO_RESET) && plan::one_chunk_ok(shape_of(env)) && !env->init_failed && env->kp.max_time > 0.0 &&
        !stream_capturing(stream)) {
        const size_t sb = (size_t)env->p.n_envs * env->L.rec_bytes();
        if (!env->init && hipMalloc((void**)&env->init, sb) != hipSuccess) {
            (void)hipGetLastError();                                         // out of memory: the kernel restarts the long way
            env->init = nullptr;
            env->init_failed = true;
        }
        if (env->init) {
            HIP_TRY(hipMemcpyAsync(env->init, env->state, sb, hipMemcpyDeviceToDevice, (hipStream_t)stream));
            env->init_valid = true;
        }
    }
    return DCM_OK;
}

int dcm_set_route_log(dcm_env* env, int16_t* route_task, double* route_arrival, int32_t* route_len, int32_t cap) {
    CHECK_HANDLE(env);
    return make_route_log("dcm_set_route_log", route_task, route_arrival, route_len, cap, &env->log);
}

int dcm_set_return_log(dcm_env* env, double* returns, int32_t cap) {
    CHECK_HANDLE(env);
    if ((returns == nullptr) != (cap == 0) || cap < 0)
        return fail(DCM_ERR_INVALID, "dcm_set_return_log: give a buffer and cap >= 1, or NULL and 0");
    env->retlog = returns; env->retcap = cap;
    return DCM_OK;
}

int dcm_observe(dcm_env* env, float* agents_out, float* tasks_out, uint8_t* mask_out, int32_t* leader_out,
                uint8_t* active_out, const int32_t* leader_in, void* stream) {
    CHECK_ENV(env);
    if (!env->reset_done) return fail(DCM_ERR_STATE, "dcm_observe: call dcm_reset first");
    const auto args = std::make_tuple(DIMS(env), env->state, agents_out, tasks_out, mask_out, leader_out, active_out, leader_in, env->sizes,
                                      env->p.flags);
    return launched(with_sim(sim_of(env), [&](auto s) {
        using S = decltype(s);
        launch(k_observe<SIM_ARGS(S), S::MC>, (unsigned)env->p.n_envs, env_kernel_lds_bytes<SIM_ARGS(S)>(env->L), (hipStream_t)stream, args);
        return 0;
    }));
}

int dcm_step(dcm_env* env, const int32_t* actions, const int32_t* leader_in, const int32_t* nfol_in,
             const int16_t* followers_in, float* agents_out, float* tasks_out, uint8_t* mask_out, int32_t* leader_out,
             uint8_t* active_out, void* stream) {
    CHECK_ENV(env);
    if (!env->reset_done) return fail(DCM_ERR_STATE, "dcm_step: call dcm_reset first");
    if (!actions) return fail(DCM_ERR_INVALID, "dcm_step: null actions");
    if ((nfol_in == nullptr) != (followers_in == nullptr))
        return fail(DCM_ERR_INVALID, "dcm_step: nfol_in and followers_in must be given together");
    // The plain call shape on a one-chunk layout: the register-resident step (step_fast.hpp); same contract, same results.
    if (plan::one_chunk_ok(shape_of(env)) && !leader_in && !nfol_in && !env->log.len && agents_out && tasks_out &&
        mask_out && leader_out && active_out && !(env->p.flags & DCM_PARAM_NO_GROUPING)) {
        // Deferred terminal metrics (dcm_env::side) for auto-resetting handles: not under stream capture -- the periodic flush is a
        // host-side decision and the buffers are allocated on first use -- where episode ends keep computing their metrics inline.
        uint32_t* pendq = nullptr;
        const plan::RenewForm form = launch_form(env);
        const bool renew = form != plan::RenewForm::Plain;
        if (env->p.flags & DCM_PARAM_AUTO_RESET) {
            if (stream_capturing(stream)) {
                if (env->maybe_pending)
                    return fail(DCM_ERR_STATE, "dcm_step under stream capture: deferred episode summaries are waiting; call dcm_summary (or dcm_reset) before the capture");
                env->captured = true;      // a replay of this graph writes summary rows unseen by the host: no snapshots on this handle any more
            } else if (plan::defer_terminal(env->captured, form)) {
                if (!env->side && !env->side_failed) {
                    const uint32_t pitch = dcm::align16(env->L.rec_bytes() + (uint32_t)env->L.A * dcm::AB_CAP * (uint32_t)sizeof(uint16_t));
                    const size_t qn = (size_t)env->p.n_envs;
                    if (hipMalloc((void**)&env->side, (size_t)env->p.n_envs * pitch) != hipSuccess ||
                        hipMalloc((void**)&env->pendq, qn * sizeof(uint32_t)) != hipSuccess ||
                        hipMemset(env->pendq, 0, qn * sizeof(uint32_t)) != hipSuccess) {
                        (void)hipGetLastError();                         // out of memory: keep the inline terminal metrics
                        if (env->side) { (void)hipFree(env->side); env->side = nullptr; }
                        if (env->pendq) { (void)hipFree(env->pendq); env->pendq = nullptr; }
                        env->side_failed = true;
                    } else env->side_pitch = pitch;
                }
                pendq = env->pendq;
            }
        }
        // (a size-renewing launch defers nothing, plan::defer_terminal: rows still waiting from earlier eager launches are computed
        //  first, while the size table still holds their episodes' sizes; under capture none can be waiting, see above)
        if (form == plan::RenewForm::Sizes && !stream_capturing(stream)) DCM_TRY(dcm::flush_pending(env, stream));
        (void)renewing_launch(env, stream);
        const unsigned char* const image = plan::step_restart_image(env->init_valid, pendq != nullptr, renew) ? env->init : nullptr;
        const auto args = std::make_tuple(DIMS(env), env->kp, env->state, actions, agents_out, tasks_out, mask_out, leader_out, active_out,
                                          env->summary, env->ablog, env->p.flags, env->sizes, env->gscratch, env->p.auto_reset_episodes,
                                          env->retlog, (int)env->retcap, env->side, env->side_pitch, pendq, image);
        const int rc = with_sim(sim_of(env), [&](auto s) {
            using S = decltype(s);
            if constexpr (S::one_chunk)
                return launch_family<step_fast_family, S::reads_sizes, SIM_ARGS(S)>(form, (unsigned)env->p.n_envs, step_fast_lds_bytes<SIM_ARGS(S)>(env->L),
                                                                                    (hipStream_t)stream, args, renew_args(env));
            else return -1;
        });
        DCM_TRY(launched(rc));
        if (pendq) {
            env->maybe_pending = true;
            if (++env->steps_since_flush >= dcm_env::FLUSH_EVERY) return dcm::flush_pending(env, stream);
        }
        return DCM_OK;
    }
    DCM_TRY(dcm::flush_pending(env, stream));    // (the general kernel writes summary rows itself)
    const plan::RenewForm form = renewing_launch(env, stream);
    const auto args = std::make_tuple(DIMS(env), env->kp, env->state, actions, leader_in, nfol_in, followers_in, agents_out, tasks_out, mask_out,
                                      leader_out, active_out, env->summary, env->log, env->ablog, env->p.flags, env->sizes, env->gscratch,
                                      env->p.auto_reset_episodes, env->retlog, (int)env->retcap);
    const int rc = with_sim(sim_of(env), [&](auto s) {
        using S = decltype(s);
        return launch_family<step_family, S::reads_sizes, SIM_ARGS(S), S::MC>(form, (unsigned)env->p.n_envs, env_kernel_lds_bytes<SIM_ARGS(S)>(env->L),
                                                                              (hipStream_t)stream, args, renew_args(env));
    });
    return launched(rc);
}

int dcm_set_rollout_log(dcm_env* env, int16_t* route_task, double* route_arrival, int32_t* route_len, int32_t cap) {
    CHECK_HANDLE(env);
    // (the register-resident logging forms address an env's [A][cap] block of route_arrival by a 32-bit byte offset)
    if (cap > 0 && (uint64_t)env->A * (uint64_t)cap * sizeof(double) > 0xFFFFFFFFull)
        return fail(DCM_ERR_INVALID, "dcm_set_rollout_log: cap too large (n_agents x cap x 8 bytes must stay below 4 GiB per env)");
    return make_route_log("dcm_set_rollout_log", route_task, route_arrival, route_len, cap, &env->rollout_log);
}

int dcm_set_best_log(dcm_env* env, int16_t* best_task, double* best_arrival, int32_t* best_len, double* best_summary,
                     int32_t* best_episode) {
    CHECK_HANDLE(env);
    const bool off = !best_task && !best_arrival && !best_len && !best_summary && !best_episode;
    if (!off && (!best_task || !best_arrival || !best_len || !best_summary || !best_episode))
        return fail(DCM_ERR_INVALID, "dcm_set_best_log: give all five arrays, or all NULL");
    env->best_log = dcm::BestLog{best_task, best_arrival, best_len, best_summary, best_episode};
    return DCM_OK;
}

int dcm_reduce_best(dcm_env* env, int32_t group, int32_t* win_env, double* win_summary, int32_t* win_episode, int32_t* win_len,
                    int16_t* win_task, double* win_arrival, void* stream) {
    CHECK_ENV(env);
    if (!env->best_log.episode)
        return fail(DCM_ERR_STATE, "dcm_reduce_best: the best log is not set: call dcm_set_best_log (and play some episodes) first");
    if (group < 1) return fail(DCM_ERR_INVALID, "dcm_reduce_best: group must be >= 1");
    if (!win_env) return fail(DCM_ERR_INVALID, "dcm_reduce_best: null win_env");
    const bool routes = win_len && win_task && win_arrival;
    if (!routes && (win_len || win_task || win_arrival))
        return fail(DCM_ERR_INVALID, "dcm_reduce_best: give win_len, win_task and win_arrival together, or all three NULL");
    // the best log's rows have the cap of the rollout log they are copied from
    if (routes && !env->rollout_log.len)
        return fail(DCM_ERR_STATE, "dcm_reduce_best: the rollout log is not set, so the best log's rows have no cap: call dcm_set_rollout_log "
                                   "first, or pass win_len, win_task and win_arrival as NULL");
    const int B = env->p.n_envs;
    const unsigned G = (unsigned)(((int64_t)B + group - 1) / group);
    const int64_t threads = ((int64_t)group + WAVE - 1) / WAVE * WAVE;
    const dcm::BestLog& bl = env->best_log;
    hipLaunchKernelGGL(k_reduce_best, dim3(G), dim3((unsigned)(threads < 1024 ? threads : 1024)), 0, (hipStream_t)stream, B, (int)group, env->A,
                       (int)env->rollout_log.cap, (const int16_t*)bl.task, (const double*)bl.arrival, (const int32_t*)bl.len,
                       (const double*)bl.summary, (const int32_t*)bl.episode, win_env, win_summary, win_episode, win_len, win_task, win_arrival);
    LAUNCH_OK();
    return DCM_OK;
}

int dcm_fork_envs(dcm_env* dst, dcm_env* src, const int32_t* src_index, const uint64_t* seeds_in, uint8_t* ok_out, void* stream) {
    if (!dst || !src) return fail(DCM_ERR_INVALID, "dcm_fork_envs: null env handle");
    if (dst->p.device != src->p.device) return fail(DCM_ERR_INVALID, "dcm_fork_envs: the two handles are on different devices");
    int cur = -1;
    if (hipGetDevice(&cur) != hipSuccess || cur != dst->p.device)
        return fail(DCM_ERR_STATE, "dcm_fork_envs: the current HIP device is not the device the handles were created on");
    // one record layout: the dims and the member slots decide every offset in a record and the pitch of the side rows
    if (dst->A != src->A || dst->T != src->T || (dst->p.flags & DCM_PARAM_WIDE_MEMBERS) != (src->p.flags & DCM_PARAM_WIDE_MEMBERS))
        return fail(DCM_ERR_INVALID, "dcm_fork_envs: n_agents, n_tasks and DCM_PARAM_WIDE_MEMBERS must be the same on both handles (one record layout)");
    if (!src_index) return fail(DCM_ERR_INVALID, "dcm_fork_envs: null src_index");
    for (const dcm_env* e : {dst, src}) {
        const char* which = e == dst ? "dst" : "src";
        // (dst too, although the call would fill it: no kernel is ever pointed at a record nobody wrote, and src_index may hold -1)
        if (!e->loaded || !e->reset_done)
            return fail(DCM_ERR_STATE, "dcm_fork_envs: %s has not been loaded and reset: call dcm_load_instances / dcm_generate_instances and dcm_reset first", which);
        if (e->sizes)
            return fail(DCM_ERR_STATE, "dcm_fork_envs: %s holds a ragged batch: the per-env sizes have a host copy that a device-side map cannot keep in step", which);
        if (e->renew_stride != 0)
            return fail(DCM_ERR_STATE, "dcm_fork_envs: %s has a renewal stride set: clear it with dcm_set_instance_renewal(env, 0) first", which);
    }
    // a deferred terminal snapshot must not land on a copied summary row later (nor a source row be read before it is computed)
    DCM_TRY(dcm::flush_pending(src, stream));
    if (dst != src) DCM_TRY(dcm::flush_pending(dst, stream));
    const Lay& L = dst->L;
    const uint32_t log_bytes = (uint32_t)dst->A * AB_CAP * sizeof(uint16_t), cnt_bytes = (uint32_t)abcnt_pitch(dst->A, dst->T);
    // (the count tables follow the logs of ALL of a handle's envs: the two handles' tables start at different offsets)
    unsigned char* const cnt_dst = (unsigned char*)dst->ablog + (size_t)dst->p.n_envs * log_bytes;
    const unsigned char* const cnt_src = (const unsigned char*)src->ablog + (size_t)src->p.n_envs * log_bytes;
    hipLaunchKernelGGL(k_fork_envs, GRID(dst), 0, (hipStream_t)stream, src->p.n_envs, dst == src, L.rec_bytes() / 16, log_bytes / 16, cnt_bytes / 16,
                       dst->state, (const unsigned char*)src->state, dst->summary, (const double*)src->summary, (unsigned char*)dst->ablog,
                       (const unsigned char*)src->ablog, cnt_dst, cnt_src, src_index, seeds_in, ok_out);
    LAUNCH_OK();
    dst->init_valid = false;          // the restart image of k_step_fast belongs to the old instances
    renewal_off(dst, false);          // the records no longer match dst's inst_seeds: not a generated batch any more
    dst->inrange = dst->inrange && src->inrange;   // dst now holds instances of both (src_index -1 keeps its own)
    return DCM_OK;
}

int dcm_rollout_random(dcm_env* env, int32_t episodes, int64_t max_decisions, const int64_t* max_decisions_in,
                       float* agents_out, float* tasks_out, uint8_t* mask_out, int64_t* steps_out, void* stream) {
    CHECK_ENV(env);
    if (!env->reset_done) return fail(DCM_ERR_STATE, "dcm_rollout_random: call dcm_reset first");
    if (episodes < 1) return fail(DCM_ERR_INVALID, "dcm_rollout_random: episodes must be >= 1");
    if (env->rollout_log.len || env->best_log.episode)
        return rollout_form(env, "dcm_rollout_random", form_of(env, FORM_LOG), DCM_POLICY_RANDOM, 0, episodes, max_decisions, max_decisions_in, agents_out,
                            tasks_out, mask_out, steps_out, stream);
    DCM_TRY(dcm::flush_pending(env, stream));
    // the renewing (k_rn_*) or size-renewing (k_rs_*) form of whichever kernel serves the handle, while a stride is set (dcm_set_instance_renewal)
    const plan::RenewForm form = renewing_launch(env, stream);
    const dcm::RolloutArgs ra = rollout_args(env, form, episodes, max_decisions, max_decisions_in, agents_out, tasks_out, mask_out, steps_out);
    const auto args = ra.kernel_args();
    const unsigned grid = (unsigned)env->p.n_envs;
    const hipStream_t hs = (hipStream_t)stream;
    // The register-resident kernels have the same contract and the same results as the general one (tests/test_gpu_rollout.py runs both)
    const bool all_obs = agents_out && tasks_out && mask_out, no_obs = !agents_out && !tasks_out && !mask_out;
    int rc = 0;
    switch (plan::rollout_kind(shape_of(env), all_obs || no_obs)) {
    case plan::Rollout::Fast: {
        // wave priorities (k_rollout_fast, PRIO) for a launch that fills the machine by itself: 16 workgroups x 256 CUs
        const bool prio = env->p.n_envs >= 4096;
        rc = with_sim(sim_of(env), [&](auto s) {
            using S = decltype(s);
            if constexpr (S::one_chunk)
                return with_bool(prio, [&](auto prio_c) {
                    return with_bool(all_obs, [&](auto obs_c) {
                        return launch_family<rollout_fast_family, S::reads_sizes, SIM_ARGS(S), decltype(obs_c)::value, decltype(prio_c)::value>(
                            form, grid, rollout_fast_lds_bytes<SIM_ARGS(S)>(env->L), hs, args, ra.rn);
                    });
                });
            else return -1;
        });
        break;
    }
    case plan::Rollout::FastMc:
        rc = with_bool(all_obs, [&](auto obs_c) {
            constexpr bool OBS = decltype(obs_c)::value;
            return launch_family<rollout_fast_mc_family, false, 50, 200, OBS>(form, grid, FastM<50, 200, OBS>::LDS_BYTES, hs, args, ra.rn);
        });
        break;
    case plan::Rollout::FastG:
        dcm::launch_rollout_fast_g(plan::fast_g_agent_chunks(env->A), plan::fast_g_task_chunks(env->T), all_obs, grid, env->L, hs, ra);
        break;
    case plan::Rollout::General:
        rc = with_sim(sim_of(env), [&](auto s) {
            using S = decltype(s);
            return launch_family<rollout_random_family, S::reads_sizes, SIM_ARGS(S), S::MC>(form, grid, rollout_random_lds_bytes<SIM_ARGS(S)>(env->L),
                                                                                            hs, args, ra.rn);
        });
        break;
    }
    return launched(rc);
}

int dcm_rollout_policy(dcm_env* env, int32_t policy, int32_t episodes, int64_t max_decisions, const int64_t* max_decisions_in,
                       float* agents_out, float* tasks_out, uint8_t* mask_out, int64_t* steps_out, void* stream) {
    if (policy == DCM_POLICY_RANDOM)
        return dcm_rollout_random(env, episodes, max_decisions, max_decisions_in, agents_out, tasks_out, mask_out, steps_out, stream);
    CHECK_ENV(env);
    if (policy != DCM_POLICY_FIRST && policy != DCM_POLICY_NEAREST)
        return fail(DCM_ERR_INVALID, "dcm_rollout_policy: unknown policy (DCM_POLICY_RANDOM, DCM_POLICY_FIRST, DCM_POLICY_NEAREST)");
    if (!env->reset_done) return fail(DCM_ERR_STATE, "dcm_rollout_policy: call dcm_reset first");
    if (episodes < 1) return fail(DCM_ERR_INVALID, "dcm_rollout_policy: episodes must be >= 1");
    DCM_TRY(need_budget(env, "dcm_rollout_policy", max_decisions, max_decisions_in));
    return rollout_form(env, "dcm_rollout_policy", form_of(env, env->rollout_log.len ? FORM_LOG : FORM_POLICY), policy, 0, episodes, max_decisions,
                        max_decisions_in, agents_out, tasks_out, mask_out, steps_out, stream);
}

int dcm_rollout_explore(dcm_env* env, int32_t policy, uint64_t explore_q32, int32_t episodes, int64_t max_decisions,
                        const int64_t* max_decisions_in, float* agents_out, float* tasks_out, uint8_t* mask_out, int64_t* steps_out,
                        void* stream) {
    CHECK_ENV(env);
    if (policy != DCM_POLICY_FIRST && policy != DCM_POLICY_NEAREST)
        return fail(DCM_ERR_INVALID, "dcm_rollout_explore: the base policy must be DCM_POLICY_FIRST or DCM_POLICY_NEAREST");
    if (explore_q32 > (1ull << 32)) return fail(DCM_ERR_INVALID, "dcm_rollout_explore: explore_q32 must be <= 2^32");
    if (!env->reset_done) return fail(DCM_ERR_STATE, "dcm_rollout_explore: call dcm_reset first");
    if (episodes < 1) return fail(DCM_ERR_INVALID, "dcm_rollout_explore: episodes must be >= 1");
    DCM_TRY(need_budget(env, "dcm_rollout_explore", max_decisions, max_decisions_in));
    return rollout_form(env, "dcm_rollout_explore", form_of(env, FORM_EXPLORE), policy, explore_q32, episodes, max_decisions, max_decisions_in, agents_out,
                        tasks_out, mask_out, steps_out, stream);
}

int dcm_rollout_individual(dcm_env* env, int32_t policy, uint64_t explore_q32, int32_t episodes, int64_t max_decisions,
                           const int64_t* max_decisions_in, float* agents_out, float* tasks_out, uint8_t* mask_out, int64_t* steps_out,
                           void* stream) {
    CHECK_ENV(env);
    if (policy != DCM_POLICY_RANDOM && policy != DCM_POLICY_FIRST && policy != DCM_POLICY_NEAREST)
        return fail(DCM_ERR_INVALID, "dcm_rollout_individual: unknown policy (DCM_POLICY_RANDOM, DCM_POLICY_FIRST, DCM_POLICY_NEAREST)");
    if (explore_q32 > (1ull << 32)) return fail(DCM_ERR_INVALID, "dcm_rollout_individual: explore_q32 must be <= 2^32");
    if (policy == DCM_POLICY_RANDOM && explore_q32 != 0)
        return fail(DCM_ERR_INVALID, "dcm_rollout_individual: explore_q32 needs a greedy base policy (DCM_POLICY_RANDOM explores at every "
                                     "decision already): give 0");
    if (episodes < 1) return fail(DCM_ERR_INVALID, "dcm_rollout_individual: episodes must be >= 1");
    if (policy != DCM_POLICY_RANDOM) DCM_TRY(need_budget(env, "dcm_rollout_individual", max_decisions, max_decisions_in));
    // dcm_reset and dcm_step form the one-group event and take the lowest pending id only under the flag: a budget-stopped launch must
    // be continuable by dcm_step and the other way round
    if (!(env->p.flags & DCM_PARAM_NO_GROUPING))
        return fail(DCM_ERR_STATE, "dcm_rollout_individual: the handle was not created with DCM_PARAM_NO_GROUPING (dcm_reset and dcm_step "
                                   "group its deciders by location)");
    if (!env->reset_done) return fail(DCM_ERR_STATE, "dcm_rollout_individual: call dcm_reset first");
    if (env->best_log.episode)
        return fail(DCM_ERR_STATE, "dcm_rollout_individual: the best log is set and there is no best-keeping individual-selection form: "
                                   "clear it with dcm_set_best_log(env, NULL, NULL, NULL, NULL, NULL)");
    return rollout_form(env, "dcm_rollout_individual", FORM_INDIVIDUAL, policy, explore_q32, episodes, max_decisions, max_decisions_in,
                        agents_out, tasks_out, mask_out, steps_out, stream);
}

int dcm_rollout_lookahead(dcm_env* env, int32_t base_policy, int32_t episodes, int64_t max_decisions, const int64_t* max_decisions_in,
                          float* agents_out, float* tasks_out, uint8_t* mask_out, int64_t* steps_out, void* stream) {
    return rollout_lookahead(env, "dcm_rollout_lookahead", base_policy, 0, episodes, max_decisions, max_decisions_in, agents_out, tasks_out,
                             mask_out, steps_out, nullptr, stream);
}

int dcm_rollout_lookahead_width(dcm_env* env, int32_t base_policy, int32_t width, int32_t episodes, int64_t max_decisions,
                                const int64_t* max_decisions_in, float* agents_out, float* tasks_out, uint8_t* mask_out,
                                int64_t* steps_out, int64_t* inner_out, void* stream) {
    return rollout_lookahead(env, "dcm_rollout_lookahead_width", base_policy, width, episodes, max_decisions, max_decisions_in, agents_out,
                             tasks_out, mask_out, steps_out, inner_out, stream);
}

int dcm_summary(dcm_env* env, double* out, void* stream) {
    CHECK_ENV(env);
    if (!out) return fail(DCM_ERR_INVALID, "dcm_summary: null out");
    DCM_TRY(dcm::flush_pending(env, stream));
    HIP_TRY(hipMemcpyAsync(out, env->summary, (size_t)env->p.n_envs * 8 * sizeof(double), hipMemcpyDeviceToDevice,
                           (hipStream_t)stream));
    return DCM_OK;
}

int dcm_env_status(dcm_env* env, uint32_t* flags_out, int64_t* decisions_out, double* now_out, void* stream) {
    CHECK_ENV(env);
    return launch_env_status(env, flags_out, decisions_out, now_out, nullptr, stream);
}

int dcm_env_episodes(dcm_env* env, int32_t* episodes_out, void* stream) {
    CHECK_ENV(env);
    if (!episodes_out) return fail(DCM_ERR_INVALID, "dcm_env_episodes: null episodes_out");
    return launch_env_status(env, nullptr, nullptr, nullptr, episodes_out, stream);
}

int dcm_get_tasks(dcm_env* env, uint8_t* finished, uint8_t* feasible, double* time_start, double* time_finish,
                  double* sum_wait, int32_t* status, int32_t* n_members, int32_t* n_abandoned, void* stream) {
    CHECK_ENV(env);
#define GETT(MCV) hipLaunchKernelGGL(k_get_tasks<MCV>, GRID(env), env->L.lds_rec(), (hipStream_t)stream, DIMS(env), env->kp, \
                       env->state, finished, feasible, time_start, time_finish, sum_wait, status, n_members, n_abandoned, \
                       env->ablog, (const int32_t*)env->sizes, env->gscratch)
    if (env->L.C > M) { GETT(MW); } else { GETT(M); }
#undef GETT
    LAUNCH_OK();
    return DCM_OK;
}

int dcm_get_agents(dcm_env* env, double* sum_wait, double* travel_dist, double* next_decision, double* arrival, double* x,
                   double* y, uint8_t* returned, uint8_t* assigned, int32_t* current, int32_t* pending_group,
                   void* stream) {
    CHECK_ENV(env);
#define GETA(MCV) hipLaunchKernelGGL(k_get_agents<MCV>, GRID(env), env->L.lds_rec(), (hipStream_t)stream, DIMS(env), env->kp, \
                       env->state, sum_wait, travel_dist, next_decision, arrival, x, y, returned, assigned, current, \
                       pending_group, env->ablog, (const int32_t*)env->sizes, env->gscratch)
    if (env->L.C > M) { GETA(MW); } else { GETA(M); }
#undef GETA
    LAUNCH_OK();
    return DCM_OK;
}

int dcm_get_members(dcm_env* env, int16_t* ids_out, void* stream) {
    CHECK_ENV(env);
    if (!ids_out) return fail(DCM_ERR_INVALID, "dcm_get_members: null ids_out");
    const int64_t n = (int64_t)env->p.n_envs * env->T;
    hipLaunchKernelGGL(k_get_members, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, env->T, env->L.A, env->L.T, env->L.C,
                       env->state, env->p.n_envs, ids_out, (const int32_t*)env->sizes);
    LAUNCH_OK();
    return DCM_OK;
}

int dcm_get_abandoned(dcm_env* env, uint16_t* counts_out, void* stream) {
    CHECK_ENV(env);
    if (!counts_out) return fail(DCM_ERR_INVALID, "dcm_get_abandoned: null counts_out");
    hipLaunchKernelGGL(k_get_abandoned, GRID(env), 0, (hipStream_t)stream, DIMS(env), env->L.C, env->state, env->ablog, counts_out,
                       (const int32_t*)env->sizes);
    LAUNCH_OK();
    return DCM_OK;
}

int dcm_state_bytes(dcm_env* env, size_t* bytes_out) {
    CHECK_HANDLE(env);
    if (!bytes_out) return fail(DCM_ERR_INVALID, "null bytes_out");
    *bytes_out = 0;
    for (const Section& s : state_sections(env)) *bytes_out += s.bytes;
    return DCM_OK;
}

int dcm_clone_state(dcm_env* env, void* dst, void* stream) {
    CHECK_ENV(env);
    if (!dst) return fail(DCM_ERR_INVALID, "dcm_clone_state: null dst");
    DCM_TRY(dcm::flush_pending(env, stream));
    unsigned char* out = (unsigned char*)dst;
    for (const Section& s : state_sections(env)) {
        if (s.bytes == 0) continue;
        HIP_TRY(hipMemcpyAsync(out, s.ptr, s.bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
        out += s.bytes;
    }
    return DCM_OK;
}

int dcm_restore_state(dcm_env* env, const void* src, void* stream) {
    CHECK_ENV(env);
    if (!src) return fail(DCM_ERR_INVALID, "dcm_restore_state: null src");
    DCM_TRY(dcm::drop_pending(env, stream));
    const unsigned char* in = (const unsigned char*)src;
    for (const Section& s : state_sections(env)) {
        if (s.bytes == 0) continue;
        HIP_TRY(hipMemcpyAsync(s.ptr, in, s.bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
        in += s.bytes;
    }
    env->loaded = true;
    env->reset_done = true;
    env->init_valid = false;          // (the restored records may belong to other instances)
    return check_points_inrange(env, stream);
}

int dcm_distance(const double* ax, const double* ay, const double* bx, const double* by, double* dist_out, double* time_out,
                 int64_t n, void* stream) {
    if (!ax || !ay || !bx || !by || n < 0) return fail(DCM_ERR_INVALID, "dcm_distance: bad argument");
    if (n == 0) return DCM_OK;
    hipLaunchKernelGGL(k_distance, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, ax, ay, bx, by,
                       dist_out, time_out, n);
    LAUNCH_OK();
    return DCM_OK;
}

#ifdef DCM_PROFILE_PHASES
int dcm_prof_read_fast(unsigned long long* out16, int reset) {
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_fast_cycles), sizeof(unsigned long long) * 16));
    if (reset) { unsigned long long z[16] = {0}; HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_fast_cycles), z, sizeof(z))); }
    return 0;
}
int dcm_prof_read(unsigned long long* out16, int reset) {
    HIP_TRY(hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_phase_cycles), sizeof(unsigned long long) * 16));
    if (reset) { unsigned long long z[16] = {0}; HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_phase_cycles), z, sizeof(z))); }
    return DCM_OK;
}
int dcm_prof_read_step(unsigned long long* out, int n_envs, int reset) {   // out[n_envs][32]
    if (n_envs > DCM_STEP_PROF_ENVS) n_envs = DCM_STEP_PROF_ENVS;
    HIP_TRY(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_step_rows), sizeof(unsigned long long) * 32 * (size_t)n_envs));
    if (reset) { void* p = nullptr; HIP_TRY(hipGetSymbolAddress(&p, HIP_SYMBOL(g_step_rows))); HIP_TRY(hipMemset(p, 0, sizeof(unsigned long long) * 32 * (size_t)DCM_STEP_PROF_ENVS)); }
    return DCM_OK;
}
#endif

int dcm_record_bytes(dcm_env* env, size_t* bytes_out) {
    CHECK_HANDLE(env);
    if (!bytes_out) return fail(DCM_ERR_INVALID, "null bytes_out");
    *bytes_out = env->L.rec_bytes();
    return DCM_OK;
}

}  // extern "C"
#endif  // DCM_DEVICE_ONLY_TU
