"""BatchedTaskEnv -- host-side face of the HIP env (B independent TaskEnv instances on one GPU).

Mirrors what worker.py:41-112 does around one reference TaskEnv, for a whole batch:

    env = BatchedTaskEnv(B, A, T, device="cuda:0")
    env.load_instances(depot, task_xy, req, dur)        # generate_env outputs  (env/task_env.py:57-114)
    obs = env.reset(seeds)                              # reset+clear_decisions (:116-140) -> first decision
    while obs.active.any():
        logp = policy(obs.tasks, obs.agents, obs.mask)  # attention.py:288-297 input contract
        obs = env.step(actions)                         # TaskEnv.step :326-342 + worker.py:74-85
    env.summary()                                       # reward + perf metrics, worker.py:87,103-108

torch is used for device memory and streams only; all simulation work happens in
libdcmrta_hip.so (hand-written gfx950 kernels) through the C ABI of include/dcmrta_env.h.
"""
import ctypes as C
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from ._lib import DcmError, DcmParams, check
from .choice import explore_q32 as _choice_explore_q32

SUMMARY_COLUMNS = ("reward", "n_finished", "success_rate", "makespan", "time_cost", "waiting_time", "travel_dist",
                   "efficiency")


@dataclass
class Observation:
    """Inputs of the attention policy for every env (SURVEY §8b policy contract)."""
    agents: torch.Tensor  # f32[B,A,6]
    tasks: torch.Tensor   # f32[B,T+1,5]
    mask: torch.Tensor    # bool[B,T+1], True = forbidden
    leader: torch.Tensor  # i32[B], -1 when the env's episode is over
    active: torch.Tensor  # bool[B]


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


# hipStream_t of torch's current stream on a device as a plain int (the raw accessor skips the Stream object)
_RAW_STREAM = getattr(torch._C, "_cuda_getCurrentRawStream", None) or (lambda i: torch.cuda.current_stream(i).cuda_stream)


class BatchedTaskEnv:
    def __init__(self, n_envs, n_agents, n_tasks, device="cuda:0", max_waiting_time=10.0, max_time=100.0,
                 individual_selection=False, auto_reset=False, auto_reset_episodes=0, strict_mask=False, member_cap=5,
                 renew_sizes=False):
        self._h = None
        self._lib = _lib.load()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise DcmError("BatchedTaskEnv runs on a HIP device only (device='cuda:N'); there is no CPU path")
        if not torch.cuda.is_available():
            raise DcmError("no HIP device visible to torch; BatchedTaskEnv has no CPU fallback")
        self.B, self.A, self.T = int(n_envs), int(n_agents), int(n_tasks)
        self.max_waiting_time, self.max_time = float(max_waiting_time), float(max_time)
        idx = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self.device = torch.device("cuda", idx)
        # individual_selection: Worker.run_test_IS (worker.py:159-198) -- deciders are not grouped by location
        # auto_reset: step() restarts an env from its instance in the call that ends its episode (DCM_PARAM_AUTO_RESET): the
        # batch stays full; summary() holds each env's last finished episode, episodes() counts them
        # strict_mask: freeze an env whose host-supplied action is on a masked task (DCM_PARAM_STRICT_MASK) instead of
        # simulating it like the reference's TaskEnv.step does
        # member_cap: member slots per task -- 5 (COALITION_SIZE, parameters.py:17) or, for a mask-ignoring policy (worker.py:140) or
        # max_coalition_size > 5 (env/task_env.py:71), 16 (DCM_PARAM_WIDE_MEMBERS: larger records, runtime-size kernels, no replay)
        # renew_sizes: set_instance_renewal also takes a ragged batch made by generate_instances (DCM_PARAM_RENEW_SIZES): an env that
        # restarts an episode then draws its next sizes with its next instance, as every reference Worker's TaskEnv does with tuple
        # ranges (env/task_env.py:58-65); nothing else changes
        if not 1 <= int(member_cap) <= _lib.MAX_MEMBERS_WIDE:
            raise DcmError(f"member_cap must be in 1..{_lib.MAX_MEMBERS_WIDE}")
        self.member_cap = _lib.MAX_MEMBERS if int(member_cap) <= _lib.MAX_MEMBERS else _lib.MAX_MEMBERS_WIDE
        flags = (1 if individual_selection else 0) | (2 if auto_reset else 0) | (4 if strict_mask else 0) | \
                (_lib.PARAM_WIDE_MEMBERS if self.member_cap > _lib.MAX_MEMBERS else 0) | (_lib.PARAM_RENEW_SIZES if renew_sizes else 0)
        self.renew_sizes = bool(renew_sizes)
        self.individual_selection, self.auto_reset, self.strict_mask = bool(individual_selection), bool(auto_reset), bool(strict_mask)
        # auto_reset_episodes: an env stops restarting after that many finished episodes (0 = never)
        p = DcmParams(self.B, self.A, self.T, idx, self.max_waiting_time, self.max_time, flags, int(auto_reset_episodes))
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            check(self._lib.dcm_create(C.byref(p), C.byref(h)))
        self._h = h
        B, A, T = self.B, self.A, self.T
        dev = self.device
        self._agents = torch.empty((B, A, 6), dtype=torch.float32, device=dev)
        self._tasks = torch.empty((B, T + 1, 5), dtype=torch.float32, device=dev)
        self._mask = torch.empty((B, T + 1), dtype=torch.uint8, device=dev)
        self._leader = torch.empty((B,), dtype=torch.int32, device=dev)
        self._active = torch.empty((B,), dtype=torch.uint8, device=dev)
        self._instances = None
        # host copies of a ragged batch's per-env sizes, taken when the batch is loaded or generated.  Under size renewal
        # (renew_sizes=True, set_instance_renewal on a ragged batch) the device changes an env's sizes at its restarts: these two
        # then still describe instance 0, and instances() returns the sizes of the instance each env holds now
        self.n_agents = self.n_tasks = None
        # the lockstep hot path (step() once per decision of a policy in the loop): everything that does not change between calls is
        # bound once -- the output pointers as plain ints, the Observation over the static buffers, the entry point
        self._out_ptrs = tuple(int(t.data_ptr()) for t in (self._agents, self._tasks, self._mask, self._leader, self._active))
        self._obs_static = Observation(self._agents, self._tasks, self._mask.view(torch.bool), self._leader, self._active.view(torch.bool))
        self._dcm_step = self._lib.dcm_step
        self._dev_index = idx
        # bumped whenever something a captured HIP graph of dcm_step has baked in changes (raggedness of the batch: the
        # per-env sizes pointer and the kernel instantiation; the route-log pointers): GraphedRollout re-captures
        self.graph_epoch = 0

    # ------------------------------------------------------------------ lifecycle
    def close(self):
        if getattr(self, "_h", None):
            self._lib.dcm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _dev(self, x, dtype):
        if isinstance(x, torch.Tensor):
            return x.to(device=self.device, dtype=dtype).contiguous()
        return torch.as_tensor(np.ascontiguousarray(x), dtype=dtype).to(self.device)

    # ------------------------------------------------------------------ instances / reset
    def load_instances(self, depot, task_xy, req, dur, n_agents=None, n_tasks=None):
        """depot[B,2] f64, task_xy[B,T,2] f64, req[B,T] int in 1..member_cap, dur[B,T] f64 (numpy or torch).

        n_agents[B] / n_tasks[B] (host ints, 1..A / 1..T) make the batch ragged: env e is an (n_agents[e], n_tasks[e])
        env (TaskEnv with tuple ranges, env/task_env.py:58-65), rows beyond its sizes in the arrays are ignored and its
        observation rows beyond them are padding (-1 features, mask True: attention.py:10-18, worker.py:253-261)."""
        B, T = self.B, self.T
        if (n_agents is None) != (n_tasks is None):
            raise DcmError("give both n_agents and n_tasks, or neither")
        req_np = (req.cpu().numpy() if isinstance(req, torch.Tensor) else np.asarray(req)).copy()
        if req_np.shape != (B, T):
            raise DcmError(f"req must be int[{B},{T}]")
        if n_tasks is not None:
            nt = np.ascontiguousarray(n_tasks, dtype=np.int32)
            na = np.ascontiguousarray(n_agents, dtype=np.int32)
            if nt.shape != (B,) or na.shape != (B,):
                raise DcmError(f"n_agents / n_tasks must be int[{B}]")
            req_np[np.arange(T)[None, :] >= nt[:, None]] = 1      # ignored rows: anything valid
        if req_np.min() < 1 or req_np.max() > self.member_cap:
            raise DcmError(f"req must be int[{B},{T}] with values in 1..{self.member_cap} (member_cap of this env)")
        d = self._dev(depot, torch.float64)
        xy = self._dev(task_xy, torch.float64)
        rq = self._dev(req, torch.int32)
        du = self._dev(dur, torch.float64)
        if d.shape != (B, 2) or xy.shape != (B, T, 2) or du.shape != (B, T):
            raise DcmError("instance arrays have the wrong shape")
        if (n_tasks is None) != (self.n_tasks is None):
            self.graph_epoch += 1
        kernels = self._kernel_names()
        with torch.cuda.device(self.device):
            if n_tasks is None:
                check(self._lib.dcm_load_instances(self._h, _ptr(d), _ptr(xy), _ptr(rq), _ptr(du), self._stream()))
                self.n_agents = self.n_tasks = None
            else:
                check(self._lib.dcm_load_instances_ragged(self._h, _ptr(d), _ptr(xy), _ptr(rq), _ptr(du),
                                                          na.ctypes.data_as(C.c_void_p), nt.ctypes.data_as(C.c_void_p),
                                                          self._stream()))
                self.n_agents, self.n_tasks = na.copy(), nt.copy()
        self._instances = (d, xy, rq, du)  # keep alive until the kernel ran
        self._kernels_since(kernels)
        return self

    # ------------------------------------------------------------------ which kernels (dcm_kernel_name)
    def kernel_name(self, entry="rollout"):
        """The kernel a plain launch takes as things stand: entry "rollout" = rollout_random with all observation buffers or none,
        "step" = step() without overrides.  A loaded batch in which two points of an env are closer than some 1e-116 without
        coinciding runs the general kernels ("k_rollout_random", "k_step") instead of the register-resident ones: same results."""
        which = {"rollout": _lib.KERNEL_ROLLOUT, "step": _lib.KERNEL_STEP}.get(entry)
        if which is None:
            raise DcmError('kernel_name: entry is "rollout" or "step"')
        name = self._lib.dcm_kernel_name(self._h, which)
        if name is None:
            check(-1)
        return name.decode()

    def _kernel_names(self):
        return self.kernel_name("rollout"), self.kernel_name("step")

    def _kernels_since(self, before):
        # a captured dcm_step has its kernel baked in: new instances that change the family end the graphs' epoch
        if self._kernel_names() != before:
            self.graph_epoch += 1

    @staticmethod
    def _range(r, dim):
        return (dim, dim) if r is None else (int(r[0]), int(r[1])) if isinstance(r, (tuple, list)) else (int(r), int(r))

    def generate_instances(self, seeds, agents_range=None, tasks_range=None, max_coalition_size=5, max_duration=5.0):
        """Make the batch on the device: env b = TaskEnv(agents_range, tasks_range, max_coalition_size=.., max_duration=..,
        seed=seeds[b]) of the reference (env/task_env.py:9-24,57-71), bit-equal to instances.generate_batch /
        generate_batch_ranges followed by load_instances, with nothing but the seeds crossing to the device.

        seeds: an int `first` (seeds first .. first + B - 1), a numpy array or a torch uint64 / int64 tensor of B seeds.
        A range is an int or (lo, hi); None = the env's own dim.  When both ranges are the env's dims the batch is uniform, otherwise
        ragged with the drawn sizes in self.n_agents / self.n_tasks (one read-back of 2 B ints).  A zero-width tuple at the dim, such as
        (20, 20) on a 20-agent env, counts as the dim: the batch is uniform and the shape-specialised kernels run, where
        load_instances(**generate_batch_ranges(...)) of the same ranges makes a ragged batch of equal sizes -- same results, other kernels."""
        B = self.B
        if isinstance(seeds, (int, np.integer)):
            seeds = np.uint64(int(seeds)) + np.arange(B, dtype=np.uint64)
        if isinstance(seeds, torch.Tensor):
            if seeds.dtype not in (torch.int64, torch.uint64):
                raise DcmError("seeds must be a uint64 / int64 tensor")
            s = seeds.to(self.device).contiguous()
        else:
            s = torch.from_numpy(np.ascontiguousarray(seeds, dtype=np.uint64).view(np.int64)).to(self.device)
        if s.numel() != B:
            raise DcmError("seeds must have one entry per env")
        (a_lo, a_hi), (t_lo, t_hi) = self._range(agents_range, self.A), self._range(tasks_range, self.T)
        # the library's own rule (dcm_generate_instances), from lo alone: it rejects lo > hi and hi > dim before anything changes, so
        # lo == dim leaves hi == dim, and where it rejects, check() raises before `ragged` is used
        ragged = not (a_lo == self.A and t_lo == self.T)
        kernels = self._kernel_names()
        with torch.cuda.device(self.device):
            check(self._lib.dcm_generate_instances(self._h, _ptr(s), a_lo, a_hi, t_lo, t_hi, int(max_coalition_size),
                                                   float(max_duration), self._stream()))
            if ragged != (self.n_tasks is not None):
                self.graph_epoch += 1
            if ragged:
                sizes = torch.empty((2, B), dtype=torch.int32, device=self.device)
                check(self._lib.dcm_get_instances(self._h, None, None, None, None, _ptr(sizes[0]), _ptr(sizes[1]), self._stream()))
                sizes = sizes.cpu().numpy()
                self.n_agents, self.n_tasks = sizes[0].copy(), sizes[1].copy()
            else:
                self.n_agents = self.n_tasks = None
        self._instances = (s,)  # keep alive until the kernel ran
        self._kernels_since(kernels)
        return self

    def set_instance_renewal(self, stride):
        """A fresh instance at every episode restart (dcm_set_instance_renewal): with stride != 0 an env that restarts an episode
        inside step() (auto_reset) or rollout() / rollout_random() first replaces its instance by the one of seed seeds[b] + (n + 1) * stride
        (mod 2**64; seeds = what generate_instances was given, n = instance_index()[b]) -- instances.renewal_seeds -- the way every
        reference Worker builds a new TaskEnv (worker.py:32).  With stride = B and seeds base + arange(B), episode k of env b plays
        instance base + k * B + b.  0 turns it off.  Needs a batch made by generate_instances (DcmError otherwise): a uniform one,
        or, on an env created with renew_sizes=True, a ragged one -- the restarting env then draws its next sizes as well (the number of
        tasks, then the number of agents, then the instance, as generate_instances does for that seed), self.n_agents / self.n_tasks
        keep describing instance 0 and instances() returns the current sizes.  A ragged batch from load_instances is always refused.
        load_instances and a new generate_instances turn it off; reset() does not renew, nor does an env that stops at an episode
        boundary: it keeps the finished episode's instance, sizes and results."""
        check(self._lib.dcm_set_instance_renewal(self._h, int(stride) % (1 << 64)))
        self.graph_epoch += 1          # a captured dcm_step has the kernel form and its arguments baked in
        return self

    def instance_index(self):
        """uint32-valued int64[B] device tensor: how many times each env's instance has been renewed since generate_instances."""
        out = torch.empty((self.B,), dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            check(self._lib.dcm_instance_index(self._h, _ptr(out), self._stream()))
        return out.to(torch.int64) & 0xFFFFFFFF

    def instances(self):
        """The instances the env holds, however they got there, as device tensors in the keyword format of load_instances:
        depot[B,2], task_xy[B,T,2], req[B,T], dur[B,T], n_agents[B], n_tasks[B] (rows beyond an env's own sizes: xy 0, req 1, dur 0, the
        padding of instances.generate_batch_ranges; n_agents / n_tasks are None on a uniform batch, and under size renewal they are
        the sizes of the instance each env holds NOW)."""
        B, T, dev = self.B, self.T, self.device
        o = dict(depot=torch.empty((B, 2), dtype=torch.float64, device=dev), task_xy=torch.empty((B, T, 2), dtype=torch.float64, device=dev),
                 req=torch.empty((B, T), dtype=torch.int32, device=dev), dur=torch.empty((B, T), dtype=torch.float64, device=dev),
                 n_agents=torch.empty((B,), dtype=torch.int32, device=dev), n_tasks=torch.empty((B,), dtype=torch.int32, device=dev))
        with torch.cuda.device(dev):
            check(self._lib.dcm_get_instances(self._h, *[_ptr(v) for v in o.values()], self._stream()))
        if self.n_tasks is None:
            o["n_agents"] = o["n_tasks"] = None
        return o

    def reset(self, seeds, observe=True):
        """seeds: uint64[B] per-env choice-protocol seeds (numpy/torch) or an int base seed."""
        if isinstance(seeds, (int, np.integer)):
            from .choice import env_seeds
            seeds = env_seeds(int(seeds), 0, self.B)
        if isinstance(seeds, torch.Tensor):
            s = seeds.to(self.device).contiguous()
        else:
            s = torch.from_numpy(np.ascontiguousarray(seeds, dtype=np.uint64).view(np.int64)).to(self.device)
        if s.numel() != self.B:
            raise DcmError("seeds must have one entry per env")
        with torch.cuda.device(self.device):
            check(self._lib.dcm_reset(self._h, _ptr(s), self._stream()))
        self._seeds = s
        return self.observe() if observe else None

    # ------------------------------------------------------------------ observe / step
    def _obs(self):
        return self._obs_static

    def observe(self, leader=None):
        li = None if leader is None else self._dev(leader, torch.int32)
        with torch.cuda.device(self.device):
            check(self._lib.dcm_observe(self._h, _ptr(self._agents), _ptr(self._tasks), _ptr(self._mask),
                                        _ptr(self._leader), _ptr(self._active), _ptr(li), self._stream()))
        return self._obs()

    def step(self, actions, leader=None, n_followers=None, followers=None, observe=True):
        """actions int32[B] (0 = depot, k = task k-1).  Optional injected choices for parity replays:
        leader int32[B] (-1 = draw), n_followers int32[B] (-1 = draw), followers int16[B,4]."""
        if (leader is None and n_followers is None and followers is None and observe and type(actions) is torch.Tensor
                and actions.dtype is torch.int32 and actions.is_cuda and actions.is_contiguous()
                and actions.device.index == self._dev_index and actions.numel() == self.B and torch.cuda.current_device() == self._dev_index):
            # the plain call of a policy in the loop (worker.py:73-76): no conversions, no device switch, no per-call allocation
            rc = self._dcm_step(self._h, actions.data_ptr(), None, None, None, *self._out_ptrs, _RAW_STREAM(self._dev_index))
            if rc != 0:
                check(rc)
            return self._obs_static
        a = self._dev(actions, torch.int32)
        li = None if leader is None else self._dev(leader, torch.int32)
        nf = None if n_followers is None else self._dev(n_followers, torch.int32)
        fo = None if followers is None else self._dev(followers, torch.int16)
        if fo is not None and tuple(fo.shape) != (self.B, _lib.FOLLOWER_COLS):
            raise DcmError("followers must be int16[B,4]")
        o = (self._agents, self._tasks, self._mask, self._leader, self._active) if observe else (None,) * 5
        with torch.cuda.device(self.device):
            check(self._lib.dcm_step(self._h, _ptr(a), _ptr(li), _ptr(nf), _ptr(fo), *[_ptr(x) for x in o],
                                     self._stream()))
        return self._obs() if observe else None

    def rollout_random(self, episodes=1, write_obs=True, max_decisions=-1):
        """Config-2 hot path: `episodes` full random-policy episodes per env in one persistent launch: rollout("random", ...),
        which see for max_decisions and the returned steps."""
        return self.rollout("random", episodes, write_obs, max_decisions)

    POLICIES = {"random": _lib.POLICY_RANDOM, "first": _lib.POLICY_FIRST, "nearest": _lib.POLICY_NEAREST}

    def rollout(self, policy="random", episodes=1, write_obs=True, max_decisions=-1, *, explore=None, explore_q32=None, lookahead=False,
                width=0, return_inner=False, individual=False):
        """`episodes` full episodes per env in one persistent launch under a device policy (dcm_rollout_policy): "random" (uniform
        over the unmasked tasks: the config-2 hot path), "first" (the lowest unmasked task) or "nearest" (the unmasked task closest
        to the deciding agent, ties to the lowest index).
        max_decisions: int (all envs) or int64[B] (numpy/torch) -- decision budget of this call (< 0 = unlimited); an env that
        runs out of budget stays at its pending decision, the obs buffers (obs()) hold what its last decision TAKEN saw.
        explore (a float epsilon in [0, 1]) or explore_q32 (an int in [0, 2^32]; choice.explore_q32(epsilon)): epsilon-greedy over
        "first" / "nearest" (dcm_rollout_explore) -- a decision takes the random policy's action with probability epsilon, decided by
        the choice protocol's explore word (choice.explores), and the base policy's pick otherwise.  Give at most one of the two;
        with neither the call is the plain one.
        lookahead=True: every decision is chosen by one-step lookahead over the base `policy` (any of the three), on the device and
        inside the same persistent launch (dcm_rollout_lookahead): the env's wave values each unmasked action by the episode in which
        the leader takes it now and `policy` plays every later decision, and takes the action with the largest (finished tasks,
        reward), ties to the lowest index -- Lookahead.values() + best_actions() of lookahead.py, bit for bit, with no branch handle
        and no host round trip.  episodes, max_decisions (outer decisions only), the rollout log, the return log, instance renewal
        and ragged batches work as in every other call; the handle needs max_waiting_time > 0 and no best log, and explore /
        explore_q32 cannot be combined with it.
        width (with lookahead=True; dcm_rollout_lookahead_width): a decision values only the `width` unmasked tasks nearest to the
        leader -- "nearest"'s own order, ties to the lowest index, whatever the base policy -- instead of all of them; 0 (the default)
        values all, 1 is "nearest" itself.  The best (finished tasks, reward) wins, a tie to the lowest action index.
        return_inner=True (with lookahead=True): also return inner int64[B], the base-policy decisions each env took inside inner
        episodes during this call -- what the launch cost beside its outer decisions.
        individual=True (dcm_rollout_individual; a handle created with individual_selection=True): the launch plays the reference's
        individual-selection protocol, Worker.run_test_IS -- the deciders of an event act one by one in ascending id, each alone, no
        followers, and the depot action moves that agent only.  A decision is then one agent's step: steps, max_decisions and the
        decision counter count those.  Any of the three policies; explore / explore_q32 as above; not with lookahead / width /
        return_inner or the best log.  A launch stopped by its budget is carried on by step() and the other way round.
        Returns steps int64[B] (device tensor), or (steps, inner) with return_inner=True."""
        if policy not in self.POLICIES:
            raise DcmError("policy must be one of %s" % ", ".join(repr(p) for p in self.POLICIES))
        if individual:
            if lookahead:
                raise DcmError("individual=True has no lookahead form: give lookahead=False")
            if width != 0 or return_inner:
                raise DcmError("width / return_inner belong to the lookahead form, which individual=True does not have")
            if not self.individual_selection:
                raise DcmError("individual=True needs a handle created with individual_selection=True (reset() and step() group the "
                               "deciders by location otherwise)")
        if lookahead and (explore is not None or explore_q32 is not None):
            raise DcmError("lookahead=True takes the base policy's own decisions inside its rollouts: it cannot be combined with explore / explore_q32")
        if isinstance(width, (bool, np.bool_)) or not isinstance(width, (int, np.integer)) or width < 0:
            raise DcmError("width must be an integer >= 0 (0: every unmasked action is valued)")
        if not lookahead and (width != 0 or return_inner):
            raise DcmError("width / return_inner belong to the lookahead form: give lookahead=True")
        q32 = None
        if explore is not None or explore_q32 is not None:
            if explore is not None and explore_q32 is not None:
                raise DcmError("give explore (epsilon) or explore_q32, not both")
            if policy == "random":
                raise DcmError("explore needs a greedy base policy: 'first' or 'nearest' ('random' explores at every decision already)")
            if explore is not None:
                try:
                    q32 = _choice_explore_q32(explore)
                except ValueError as e:
                    raise DcmError(str(e))
            else:
                q32 = int(explore_q32)
                if not 0 <= q32 <= 1 << 32:
                    raise DcmError("explore_q32 must lie in [0, 2^32]")
        steps = torch.empty((self.B,), dtype=torch.int64, device=self.device)
        o = (self._agents, self._tasks, self._mask) if write_obs else (None, None, None)
        per_env = None
        if not isinstance(max_decisions, (int, np.integer)):
            per_env = self._dev(max_decisions, torch.int64)
            if per_env.numel() != self.B:
                raise DcmError("max_decisions must be an int or int64[B]")
            max_decisions = -1
        inner = torch.empty((self.B,), dtype=torch.int64, device=self.device) if return_inner else None
        with torch.cuda.device(self.device):
            if lookahead and (width != 0 or return_inner):
                check(self._lib.dcm_rollout_lookahead_width(self._h, self.POLICIES[policy], int(width), int(episodes), int(max_decisions),
                                                            _ptr(per_env), *[_ptr(x) for x in o], _ptr(steps), _ptr(inner), self._stream()))
                if return_inner:
                    return steps, inner
            elif lookahead:
                check(self._lib.dcm_rollout_lookahead(self._h, self.POLICIES[policy], int(episodes), int(max_decisions), _ptr(per_env),
                                                      *[_ptr(x) for x in o], _ptr(steps), self._stream()))
            elif individual:
                check(self._lib.dcm_rollout_individual(self._h, self.POLICIES[policy], 0 if q32 is None else q32, int(episodes),
                                                       int(max_decisions), _ptr(per_env), *[_ptr(x) for x in o], _ptr(steps),
                                                       self._stream()))
            elif q32 is None:
                check(self._lib.dcm_rollout_policy(self._h, self.POLICIES[policy], int(episodes), int(max_decisions), _ptr(per_env),
                                                   *[_ptr(x) for x in o], _ptr(steps), self._stream()))
            else:
                check(self._lib.dcm_rollout_explore(self._h, self.POLICIES[policy], q32, int(episodes), int(max_decisions), _ptr(per_env),
                                                    *[_ptr(x) for x in o], _ptr(steps), self._stream()))
        return steps

    def obs(self):
        """The env's static observation buffers (written by the last observe / step / rollout / rollout_random call)."""
        return self._obs()

    # ------------------------------------------------------------------ results
    def summary(self):
        """f64[B,8]: reward, n_finished, success_rate, makespan, time_cost, waiting_time, travel_dist, efficiency."""
        out = torch.empty((self.B, 8), dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            check(self._lib.dcm_summary(self._h, _ptr(out), self._stream()))
        return out

    def status(self):
        flags = torch.empty((self.B,), dtype=torch.int32, device=self.device)
        dec = torch.empty((self.B,), dtype=torch.int64, device=self.device)
        now = torch.empty((self.B,), dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            check(self._lib.dcm_env_status(self._h, _ptr(flags), _ptr(dec), _ptr(now), self._stream()))
        return dict(flags=flags, decisions=dec, now=now)

    def episodes(self):
        """int32[B]: episodes finished by each env since reset()."""
        out = torch.empty((self.B,), dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            check(self._lib.dcm_env_episodes(self._h, _ptr(out), self._stream()))
        return out

    def tasks_state(self):
        B, T, dev = self.B, self.T, self.device
        u8 = lambda: torch.empty((B, T), dtype=torch.uint8, device=dev)
        f8 = lambda: torch.empty((B, T), dtype=torch.float64, device=dev)
        i4 = lambda: torch.empty((B, T), dtype=torch.int32, device=dev)
        o = dict(finished=u8(), feasible=u8(), time_start=f8(), time_finish=f8(), sum_waiting_time=f8(), status=i4(),
                 n_members=i4(), n_abandoned=i4())
        with torch.cuda.device(dev):
            check(self._lib.dcm_get_tasks(self._h, *[_ptr(v) for v in o.values()], self._stream()))
        return o

    def agents_state(self):
        B, A, dev = self.B, self.A, self.device
        f8 = lambda: torch.empty((B, A), dtype=torch.float64, device=dev)
        u8 = lambda: torch.empty((B, A), dtype=torch.uint8, device=dev)
        o = dict(sum_waiting_time=f8(), travel_dist=f8(), next_decision=f8(), arrival=f8(), x=f8(), y=f8(),
                 returned=u8(), assigned=u8(), current=torch.empty((B, A), dtype=torch.int32, device=dev),
                 pending_group=torch.empty((B, A), dtype=torch.int32, device=dev))
        with torch.cuda.device(dev):
            check(self._lib.dcm_get_agents(self._h, *[_ptr(v) for v in o.values()], self._stream()))
        return o

    def task_members(self):
        """int16[B,T,member_cap]: task['members'] of every task in list order, -1 padded (env/task_env.py:80)."""
        out = torch.empty((self.B, self.T, self.member_cap), dtype=torch.int16, device=self.device)
        with torch.cuda.device(self.device):
            check(self._lib.dcm_get_members(self._h, _ptr(out), self._stream()))
        return out

    def abandoned_counts(self):
        """int16[B,A,T]: how often task t has moved agent a to its abandoned_agent list this episode (env/task_env.py:89)."""
        out = torch.empty((self.B, self.A, self.T), dtype=torch.int16, device=self.device)
        with torch.cuda.device(self.device):
            check(self._lib.dcm_get_abandoned(self._h, _ptr(out), self._stream()))
        return out

    def enable_return_log(self, cap):
        """Keep every episode's return: f64[B, cap] ring, the k-th episode an env finishes since reset() lands in column
        k mod cap (dcm_set_return_log).  summary() keeps only the last episode; with cap = episodes per rollout_random call
        all of a call's episode returns are here afterwards.  cap = 0 disables."""
        self._retlog = torch.full((self.B, int(cap)), float("nan"), dtype=torch.float64, device=self.device) if cap else None
        check(self._lib.dcm_set_return_log(self._h, _ptr(self._retlog), int(cap)))
        self.graph_epoch += 1
        return self._retlog

    # ------------------------------------------------------------------ route history (agent['route'], agent['arrival_time'])
    def enable_route_log(self, cap=64):
        """Record every agent_step of the lockstep API (reset / step): route_task[B,A,cap] (-1 = depot), route_arrival, route_len."""
        B, A, dev = self.B, self.A, self.device
        self._route = (torch.full((B, A, cap), -2, dtype=torch.int16, device=dev),
                       torch.zeros((B, A, cap), dtype=torch.float64, device=dev),
                       torch.zeros((B, A), dtype=torch.int32, device=dev))
        check(self._lib.dcm_set_route_log(self._h, *[_ptr(x) for x in self._route], int(cap)))
        self.graph_epoch += 1
        return self

    def routes(self):
        """(task[B,A,cap], arrival[B,A,cap], length[B,A]) recorded since the last reset."""
        return self._route

    def enable_rollout_log(self, cap=64):
        """Record every agent_step of the persistent launches (rollout / rollout_random, any policy; dcm_set_rollout_log) in buffers of
        enable_route_log's layout.  They hold the LAST episode each env played: an env zeroes its lengths when it restarts an episode,
        reset() zeroes all; after a budget stop in mid-episode they hold the prefix played and the next rollout() carries on.
        step() never writes them, and rollout() never writes the enable_route_log ones.  cap = 0 / None disables."""
        B, A, dev = self.B, self.A, self.device
        if not cap:
            check(self._lib.dcm_set_rollout_log(self._h, None, None, None, 0))
            self._rollout_route = None
        else:
            bufs = (torch.full((B, A, cap), -2, dtype=torch.int16, device=dev),
                    torch.zeros((B, A, cap), dtype=torch.float64, device=dev),
                    torch.zeros((B, A), dtype=torch.int32, device=dev))
            check(self._lib.dcm_set_rollout_log(self._h, *[_ptr(x) for x in bufs], int(cap)))
            self._rollout_route = bufs
        self.graph_epoch += 1
        if getattr(self, "_best", None) is not None:                        # the best log has the rollout log's cap: it follows
            self.enable_best_log(bool(cap))
        return self

    def rollout_routes(self):
        """(task[B,A,cap], arrival[B,A,cap], length[B,A]) of enable_rollout_log: the last episode each env played in rollout()."""
        r = getattr(self, "_rollout_route", None)
        if r is None:
            raise DcmError("the rollout log is off: call enable_rollout_log(cap) first")
        return r

    def rollout_plan(self, b=None):
        """The logged routes as the nested lists load_routes takes -- plan[b][a] = [action, ...] with 0 = depot, k = task k-1 -- for
        every env, or for env b alone (plan[a]).  On a ragged batch the agents beyond an env's own size have empty lists.
        ValueError, like route_lists, when a route is longer than the log's cap."""
        from .trajectory import route_lists
        task, arrival, length = (x.cpu().numpy() for x in self.rollout_routes())
        one = lambda e: [[t + 1 for t in r] for r, _ in route_lists(task[e], arrival[e], length[e], "enable_rollout_log(cap)")]
        return one(b) if b is not None else [one(e) for e in range(self.B)]

    def enable_best_log(self, on=True):
        """Keep every env's best episode on the device (dcm_set_best_log): while on, rollout() under any policy keeps for each env the
        best episode it has finished since reset() -- by the pair (finished tasks, reward); on a tie the earliest -- with its summary
        row, its ordinal and its complete routes, across the episodes of a call and across calls: one call of B envs x E episodes
        gives B x E samples and B plans (best_summary / best_episode / best_routes / best_plan).  Needs enable_rollout_log, whose cap
        the buffers take (calling it again re-allocates them); reset() forgets the kept episodes.  rollout() refuses while instances
        are renewed.  enable_best_log(False) disables."""
        if not on:
            if getattr(self, "_best", None) is not None:
                check(self._lib.dcm_set_best_log(self._h, None, None, None, None, None))
                self.graph_epoch += 1
            self._best = None
            return self
        r = getattr(self, "_rollout_route", None)
        if r is None:
            raise DcmError("the best log copies the kept episode from the rollout log: call enable_rollout_log(cap) first")
        B, A, dev, cap = self.B, self.A, self.device, r[0].shape[2]
        bufs = (torch.full((B, A, cap), -2, dtype=torch.int16, device=dev),
                torch.zeros((B, A, cap), dtype=torch.float64, device=dev),
                torch.zeros((B, A), dtype=torch.int32, device=dev),
                torch.full((B, 8), float("nan"), dtype=torch.float64, device=dev),
                torch.full((B,), -1, dtype=torch.int32, device=dev))
        check(self._lib.dcm_set_best_log(self._h, *[_ptr(x) for x in bufs]))
        self._best = bufs
        self.graph_epoch += 1
        return self

    def _best_log(self):
        r = getattr(self, "_best", None)
        if r is None:
            raise DcmError("the best log is off: call enable_best_log() first")
        return r

    def best_routes(self):
        """(task[B,A,cap], arrival[B,A,cap], length[B,A]) of enable_best_log: each env's kept episode, in rollout_routes' layout.  Only
        [0, min(length, cap)) of a row is defined, and nothing for an env that keeps no episode (best_episode -1)."""
        return self._best_log()[:3]

    def best_summary(self):
        """f64[B,8]: the summary row of each env's kept episode (summary's columns); NaN rows where none is kept."""
        return self._best_log()[3]

    def best_episode(self):
        """int32[B]: the ordinal since reset() of each env's kept episode (its column of the return log), -1 = none kept."""
        return self._best_log()[4]

    def best_plan(self, b=None):
        """rollout_plan over the kept episodes: plan[b][a] = [action, ...] with 0 = depot, k = task k-1, for every env or for env b
        alone.  ValueError, like route_lists, when a kept route is longer than the log's cap."""
        from .trajectory import route_lists
        task, arrival, length = (x.cpu().numpy() for x in self.best_routes())
        one = lambda e: [[t + 1 for t in r] for r, _ in route_lists(task[e], arrival[e], length[e], "enable_rollout_log(cap)")]
        return one(b) if b is not None else [one(e) for e in range(self.B)]

    def reduce_best(self, group=None, routes=True):
        """The best log reduced over groups of envs on the device (dcm_reduce_best): envs [g * group, (g + 1) * group) are group g
        (group=None: all B envs, one group; the last group may be short), and each group's winner is the env with the most finished
        tasks, then the largest reward, then the lowest index.  Returns a dict of device tensors allocated by this call -- env[G]
        (int32, -1 = no env of the group keeps an episode), summary[G,8], episode[G] and, with routes, len[G,A], task[G,A,cap],
        arrival[G,A,cap]: the winner's rows of best_summary / best_episode / best_routes, the route rows filled with -2 / 0.0 behind
        [0, min(len, cap)).  N instances x K envs each in one handle: reduce_best(group=K) gives the N plans (group_plan) and only
        those leave the device.  Stream-ordered, no synchronisation; changes nothing in the handle."""
        if group is not None and int(group) < 1:
            raise ValueError("reduce_best: group must be >= 1")
        best = self._best_log()
        group = self.B if group is None else int(group)
        G, A, dev, cap = -(-self.B // group), self.A, self.device, best[0].shape[2]
        red = dict(env=torch.full((G,), -1, dtype=torch.int32, device=dev),
                   summary=torch.full((G, 8), float("nan"), dtype=torch.float64, device=dev),
                   episode=torch.full((G,), -1, dtype=torch.int32, device=dev))
        if routes:
            red.update(len=torch.zeros((G, A), dtype=torch.int32, device=dev),
                       task=torch.full((G, A, cap), -2, dtype=torch.int16, device=dev),
                       arrival=torch.zeros((G, A, cap), dtype=torch.float64, device=dev))
        with torch.cuda.device(self.device):
            check(self._lib.dcm_reduce_best(self._h, group, _ptr(red["env"]), _ptr(red["summary"]), _ptr(red["episode"]),
                                            _ptr(red.get("len")), _ptr(red.get("task")), _ptr(red.get("arrival")), self._stream()))
        return red

    @staticmethod
    def group_plan(red, g):
        """best_plan's nested lists for the winner of group g of a reduce_best() result (with routes): plan[a] = [action, ...] with
        0 = depot, k = task k-1; empty lists for a group without a winner.  ValueError, like route_lists, when a kept route is longer
        than the log's cap."""
        from .trajectory import route_lists
        task, arrival, length = (red[k][g].cpu().numpy() for k in ("task", "arrival", "len"))
        return [[t + 1 for t in r] for r, _ in route_lists(task, arrival, length, "enable_rollout_log(cap)")]

    # ------------------------------------------------------------------ route replay (env/task_env.py:562-599)
    def load_routes(self, routes, member_cap=8):
        """routes[b][a] = list of actions (0 = depot, k = task k-1) or None (pre_set_route stays None)."""
        B, A = self.B, self.A
        cap = max([len(r) for env in routes for r in env if r is not None] + [1])
        arr = np.zeros((B, A, cap), np.int32)
        ln = np.full((B, A), -1, np.int32)
        for b in range(B):
            for a in range(A):
                r = routes[b][a] if a < len(routes[b]) else None
                if r is not None:
                    ln[b, a] = len(r)
                    arr[b, a, :len(r)] = r
        return self.load_route_arrays(arr, ln, member_cap)

    def load_route_arrays(self, routes, route_len, member_cap=8):
        """routes int32[B,A,cap] (actions, 0-padded), route_len int32[B,A] (-1 = pre_set_route stays None): dcm_load_routes."""
        routes, route_len = np.ascontiguousarray(routes, np.int32), np.ascontiguousarray(route_len, np.int32)
        if routes.ndim != 3 or routes.shape[:2] != (self.B, self.A) or route_len.shape != (self.B, self.A):
            raise DcmError(f"routes must be int32[{self.B},{self.A},cap] and route_len int32[{self.B},{self.A}]")
        d_arr, d_ln = self._dev(routes, torch.int32), self._dev(route_len, torch.int32)
        with torch.cuda.device(self.device):
            check(self._lib.dcm_load_routes(self._h, _ptr(d_arr), _ptr(d_ln), int(routes.shape[2]), int(member_cap), self._stream()))
            torch.cuda.current_stream(self.device).synchronize()
        self._replay_member_cap = int(member_cap)
        rlog = getattr(self, "_rlog", None)
        if rlog is not None and rlog["members"].shape[2] != self._replay_member_cap:
            self.enable_replay_log(rlog["route"].shape[2])                   # member_cols follows the routes' member_cap
        return self

    def enable_replay_log(self, cap=64):
        """Record what execute_routes leaves for generate_traj (dcm_set_replay_log): every agent_step's (task id, -1 = depot;
        arrival) in route[B,A,cap] / arrival[B,A,cap] / route_len[B,A] (agent['route'] / ['arrival_time']), and after the replay
        members[B,T,member_cols] (task['members'], -1 padded) and feasible[B,T] (task['feasible_assignment']).  member_cols = the
        member_cap of the last load_routes (re-allocated there when it changes).  cap = 0 disables."""
        B, A, T, dev = self.B, self.A, self.T, self.device
        if not cap:
            check(self._lib.dcm_set_replay_log(self._h, None, None, None, 0, None, 0, None))
            self._rlog = None
            return self
        mc = getattr(self, "_replay_member_cap", 8)
        self._rlog = dict(route=torch.full((B, A, cap), -2, dtype=torch.int16, device=dev),
                          arrival=torch.zeros((B, A, cap), dtype=torch.float64, device=dev),
                          route_len=torch.zeros((B, A), dtype=torch.int32, device=dev),
                          members=torch.full((B, T, mc), -1, dtype=torch.int16, device=dev),
                          feasible=torch.zeros((B, T), dtype=torch.uint8, device=dev))
        r = self._rlog
        check(self._lib.dcm_set_replay_log(self._h, _ptr(r["route"]), _ptr(r["arrival"]), _ptr(r["route_len"]), int(cap),
                                           _ptr(r["members"]), mc, _ptr(r["feasible"])))
        return self

    def set_visibility(self, initial=20, batch=20, period=10, cap=100):
        """Dynamic-arrival schedule of the reactive replay: visible = clip(now // period * batch + initial, initial, cap)
        (env/task_env.py:567; re-arm (next - 1) // batch * period, :221).  Defaults = the reference's hard-coded constants."""
        check(self._lib.dcm_set_visibility(self._h, int(initial), int(batch), int(period), int(cap)))
        return self

    def set_replay_placement(self, placement="auto"):
        """Which replay kernel execute_routes runs: "auto" = the register-resident one whenever the shape allows it (<= 128 agents,
        <= 128 live tasks, member_cap <= 8), else the general one with its replay scratch in LDS for batches of at most four envs
        per CU and in HBM otherwise; "lds" / "hbm" = always the general kernel with its scratch there (dcm_set_replay_placement).
        Results do not depend on it."""
        check(self._lib.dcm_set_replay_placement(self._h, {"auto": 0, "lds": 1, "hbm": 2}[placement]))
        return self

    def execute_routes(self, reactive=False, fields=None):
        """execute_by_route + get_episode_reward for every env; returns a dict of device tensors.
        fields: which of the optional per-task / per-agent arrays to produce (default: all; () = steps, flags, summary only).
        With the replay log on (enable_replay_log) the dict also holds its buffers -- route, arrival, route_len, members,
        feasible -- which the next execute_routes overwrites."""
        B, A, T, dev = self.B, self.A, self.T, self.device
        spec = dict(finished=((B, T), torch.uint8), time_start=((B, T), torch.float64), time_finish=((B, T), torch.float64),
                    task_wait=((B, T), torch.float64), n_members=((B, T), torch.int32), agent_wait=((B, A), torch.float64),
                    travel_dist=((B, A), torch.float64), returned=((B, A), torch.uint8))
        o = dict(steps=torch.empty((B,), dtype=torch.int64, device=dev), flags=torch.empty((B,), dtype=torch.int32, device=dev))
        for k, (shape, dt) in spec.items():
            o[k] = torch.empty(shape, dtype=dt, device=dev) if fields is None or k in fields else None
        with torch.cuda.device(dev):
            check(self._lib.dcm_execute_routes(self._h, int(bool(reactive)), *[_ptr(v) for v in o.values()], self._stream()))
        o = {k: v for k, v in o.items() if v is not None}
        o["summary"] = self.summary()
        if getattr(self, "_rlog", None) is not None:
            o.update(self._rlog)
        return o

    # ------------------------------------------------------------------ snapshot (copy.deepcopy(env), worker.py:33)
    def clone_state(self):
        n = C.c_size_t()
        check(self._lib.dcm_state_bytes(self._h, C.byref(n)))
        buf = torch.empty((n.value,), dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            check(self._lib.dcm_clone_state(self._h, _ptr(buf), self._stream()))
        return buf

    def restore_state(self, buf):
        # dcm_restore_state takes no length, and the blob of a renew_sizes handle is 8 * B bytes longer while its batch is ragged: a
        # snapshot taken from the other kind of batch would be read past its end
        n = C.c_size_t()
        check(self._lib.dcm_state_bytes(self._h, C.byref(n)))
        if buf.numel() * buf.element_size() != n.value:
            raise DcmError(f"restore_state: the snapshot holds {buf.numel() * buf.element_size()} bytes, this env's state is {n.value} "
                           "(taken from another env, or before the batch changed between uniform and ragged)")
        kernels = self._kernel_names()
        with torch.cuda.device(self.device):
            check(self._lib.dcm_restore_state(self._h, _ptr(buf), self._stream()))
        self._kernels_since(kernels)

    # ------------------------------------------------------------------ per-env copy (dcm_fork_envs)
    def fork_from(self, src, index, seeds=None, check=False):
        """Env b of this handle becomes env index[b] of `src` (dcm_fork_envs): the record with its instance, clock, decision counter
        and episode count, the summary row and the abandonment tables.  index: int32[B] (numpy/torch), -1 = leave env b alone.
        seeds: uint64[B] -- the copied envs draw from seeds[b] from here on; None -- a copy keeps its source's seed and plays exactly what
        the source would.  src may be this handle: a source must then be its own source (index[index[b]] == index[b]).  Envs whose index
        breaks that rule or lies outside [-1, src.B) are left untouched; check=True reads the device's verdict back and raises
        DcmError for them (otherwise the call does not synchronise).  Both handles need the same n_agents, n_tasks and member_cap, a
        uniform batch that has been loaded and reset, and no renewal stride.  The logs (enable_route_log / enable_rollout_log /
        enable_best_log / enable_return_log) are not copied: they stay this handle's.  Returns self."""
        if not isinstance(src, BatchedTaskEnv):
            raise DcmError("fork_from: src must be a BatchedTaskEnv")
        if (src.A, src.T, src.member_cap) != (self.A, self.T, self.member_cap):
            raise DcmError(f"fork_from: src is a {src.A}A/{src.T}T env with member_cap {src.member_cap}, this one {self.A}A/{self.T}T "
                           f"with {self.member_cap}: the record layouts must be identical")
        n = index.numel() if isinstance(index, torch.Tensor) else np.asarray(index).size
        if n != self.B:
            raise DcmError(f"fork_from: index must be int32[{self.B}], one entry per env of this handle")
        if seeds is not None:
            if isinstance(seeds, torch.Tensor):
                if seeds.dtype not in (torch.int64, torch.uint64):
                    raise DcmError("fork_from: seeds must be a uint64 / int64 tensor")
                ns = seeds.numel()
            else:
                seeds = np.ascontiguousarray(seeds, dtype=np.uint64)
                ns = seeds.size
            if ns != self.B:
                raise DcmError(f"fork_from: seeds must be uint64[{self.B}], one entry per env of this handle")
        if src.device != self.device:
            raise DcmError("fork_from: the two handles are on different devices")
        if src._h is None or self._h is None:
            raise DcmError("fork_from: a handle is closed")
        idx = self._dev(index, torch.int32).reshape(-1)
        s = None
        if seeds is not None:
            s = seeds.to(self.device).contiguous() if isinstance(seeds, torch.Tensor) else torch.from_numpy(seeds.view(np.int64)).to(self.device)
        ok = torch.empty((self.B,), dtype=torch.uint8, device=self.device) if check else None
        kernels = self._kernel_names()
        with torch.cuda.device(self.device):
            _lib.check(self._lib.dcm_fork_envs(self._h, src._h, _ptr(idx), _ptr(s), _ptr(ok), self._stream()))
        self._kernels_since(kernels)
        self._fork_args = (idx, s)      # keep alive until the kernel ran
        if check:
            bad = torch.nonzero(ok == 0).flatten().cpu().numpy()
            if len(bad):
                raise DcmError(f"fork_from: {len(bad)} env(s) were refused and left untouched (first: env {int(bad[0])}, index "
                               f"{int(idx[int(bad[0])])}): the index is outside [-1, {src.B}) or, in place, its source is not its own source")
        return self

    def record_bytes(self):
        n = C.c_size_t()
        check(self._lib.dcm_record_bytes(self._h, C.byref(n)))
        return n.value


group_plan = BatchedTaskEnv.group_plan    # needs the reduced buffers only, no handle


def device_distance(a_xy, b_xy, device="cuda:0"):
    """calculate_eulidean_distance + travel time on the device (known-answer test helper)."""
    lib = _lib.load()
    dev = torch.device(device)
    a = torch.as_tensor(np.ascontiguousarray(a_xy), dtype=torch.float64).to(dev)
    b = torch.as_tensor(np.ascontiguousarray(b_xy), dtype=torch.float64).to(dev)
    ax, ay, bx, by = a[:, 0].contiguous(), a[:, 1].contiguous(), b[:, 0].contiguous(), b[:, 1].contiguous()
    d = torch.empty_like(ax)
    t = torch.empty_like(ax)
    with torch.cuda.device(dev):
        check(lib.dcm_distance(_ptr(ax), _ptr(ay), _ptr(bx), _ptr(by), _ptr(d), _ptr(t), ax.numel(),
                               C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    return d.cpu().numpy(), t.cpu().numpy()


def device_generator_draws(seeds, n_doubles, bound, n_ints, device="cuda:0"):
    """Per seed the first n_doubles of np.random.default_rng(seed).random(), then n_ints of .integers(0, bound), from the device
    routines generate_instances uses (known-answer test helper): (f64[n, n_doubles], u32[n, n_ints]) as numpy arrays."""
    lib = _lib.load()
    dev = torch.device(device)
    s = torch.from_numpy(np.ascontiguousarray(seeds, dtype=np.uint64).view(np.int64)).to(dev)
    d = torch.empty((s.numel(), int(n_doubles)), dtype=torch.float64, device=dev)
    i = torch.empty((s.numel(), int(n_ints)), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        check(lib.dcm_generator_draws(_ptr(s), s.numel(), int(n_doubles), int(bound), int(n_ints), _ptr(d), _ptr(i),
                                      C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    return d.cpu().numpy(), i.cpu().numpy().view(np.uint32)
