"""One-step lookahead over a base heuristic, on the device: value every action of every env by a rollout, and plan with the values.

    env = BatchedTaskEnv(B, A, T).load_instances(...).enable_route_log(cap)
    env.reset(seeds, observe=False)
    la = Lookahead(env, policy="nearest")
    reward, finished = la.values()          # f64[B, T+1], i32[B, T+1]: the episode's result if the leader takes action a now and
                                            # `nearest` plays on; NaN / -1 where the mask forbids a (or the env's episode is over)
    la.plan()                               # the rollout algorithm: step the env by its best action until every episode is over

values() forks every env of `env` into T + 1 envs of a branch handle (BatchedTaskEnv.fork_from: dcm_fork_envs, the copies keep their
source's seed and decision counter, so each plays exactly what the source would), steps branch a of an env with action a, and plays
all branches to the end of their episodes in one persistent launch of the base policy.  Nothing of `env` changes.  The choice
protocol is a pure function of (seed, decision counter, slot), so the values are exact, not estimates: the column of the action the
base policy itself picks is the result of the base policy's own episode, and plan(), which always takes the action with the largest
(finished tasks, reward), never ends below the base policy started from the same state.
All T + 1 actions get a branch, the masked ones too (they run the env's lowest unmasked action and their values are dropped):
compacting the branches to the unmasked actions would make the fan-out data dependent.
The same decisions without a branch handle and without the host: BatchedTaskEnv.rollout(policy, lookahead=True), the device form, in
which every env's wave values its own actions one after the other inside one persistent launch."""
import torch

from ._lib import DcmError
from .batched_env import BatchedTaskEnv


class Lookahead:
    def __init__(self, env, policy="nearest"):
        if not isinstance(env, BatchedTaskEnv):
            raise DcmError("Lookahead: env must be a BatchedTaskEnv")
        if policy not in BatchedTaskEnv.POLICIES:
            raise DcmError("Lookahead: policy must be one of %s" % ", ".join(repr(p) for p in BatchedTaskEnv.POLICIES))
        if not env.max_waiting_time > 0.0:
            raise DcmError("Lookahead: the env has max_waiting_time <= 0, where a greedy policy does not end its episodes without a "
                           "decision budget: there is no episode result to value an action by")
        if env.auto_reset:
            raise DcmError("Lookahead: the env restarts its episodes by itself (auto_reset=True): an action is valued by ONE episode's "
                           "result and plan() ends when every episode is over")
        if env.n_tasks is not None:
            raise DcmError("Lookahead: the env holds a ragged batch, which fork_from cannot copy")
        self.env, self.policy = env, policy
        B, T1, dev = env.B, env.T + 1, env.device
        self.launches = 0                  # values() calls so far: each is one fork, one step and one persistent launch of B (T + 1) envs
        self.decisions = torch.zeros((), dtype=torch.int64, device=dev)        # ... and the decisions the branches have played in them
        # the branch handle: the env's dims, flags and parameters, B (T + 1) envs, no logs.  Loaded and reset once, with anything,
        # so that it may be forked into; every values() call replaces all of its envs
        self.branch = BatchedTaskEnv(B * T1, env.A, env.T, device=dev, max_waiting_time=env.max_waiting_time, max_time=env.max_time,
                                     individual_selection=env.individual_selection, strict_mask=env.strict_mask, member_cap=env.member_cap)
        self.branch.generate_instances(0)
        self.branch.reset(0, observe=False)
        i = torch.arange(B * T1, dtype=torch.int64, device=dev)
        self._source = (i // T1).to(torch.int32)             # branch i is a copy of env i // (T + 1) ...
        self._action = i % T1                                # ... that takes action i % (T + 1)
        self._row = i

    def close(self):
        self.branch.close()

    def values(self):
        """reward f64[B, T+1], finished i32[B, T+1] (device tensors): for every env, which must sit at a decision point, and every
        action a the leader may take, the reward and the number of finished tasks of the episode in which the leader takes a now and
        the base policy plays every later decision.  NaN / -1 where the mask forbids a, and in the whole row of an env whose episode is
        over.  No synchronisation; the env itself is not changed in any way."""
        env, br = self.env, self.branch
        B, T1 = env.B, env.T + 1
        br.fork_from(env, self._source)
        obs = br.observe()
        forbidden = obs.mask[self._row, self._action]
        valid = obs.active & ~forbidden
        self.active = obs.active.view(B, T1)[:, 0].clone()                        # bool[B]: the envs whose episode is not over
        lowest = (~obs.mask).to(torch.uint8).argmax(dim=1)                       # the lowest unmasked action (0 where there is none)
        actions = torch.where(forbidden, lowest, self._action).to(torch.int32)
        stepped = obs.active.sum()
        obs = br.step(actions)
        # a branch that is DONE -- its source was, or the step ended its episode -- gets no budget: a persistent launch restarts a DONE env
        # that has one.  (-1 = unlimited for the active ones)
        budget = -obs.active.to(torch.int64)
        self.decisions += stepped + br.rollout(self.policy, episodes=1, write_obs=False, max_decisions=budget).sum()
        sm = br.summary()
        nan = torch.full((), float("nan"), dtype=torch.float64, device=env.device)
        reward = torch.where(valid, sm[:, 0], nan).view(B, T1)
        finished = torch.where(valid, sm[:, 1].to(torch.int32), torch.full((), -1, dtype=torch.int32, device=env.device)).view(B, T1)
        self.launches += 1
        return reward, finished

    @staticmethod
    def best_actions(reward, finished):
        """int32[B]: per env the action with the largest (finished, reward) pair of a values() result, ties to the lowest index; 0 for
        an env without a valid action."""
        T1 = reward.shape[1]
        cand = (finished == finished.max(dim=1, keepdim=True).values) & (finished >= 0)
        r = torch.where(cand, reward, torch.full_like(reward, float("-inf")))
        best = cand & (r == r.max(dim=1, keepdim=True).values)
        col = torch.arange(T1, device=reward.device).expand_as(reward)
        first = torch.where(best, col, torch.full_like(col, T1)).min(dim=1).values
        return torch.where(first < T1, first, torch.zeros_like(first)).to(torch.int32)

    def plan(self):
        """The rollout algorithm: until every env's episode is over, take values() and step the env with each env's best action
        (best_actions).  The env's route log (enable_route_log) then holds the plan and summary() its result, which is never below the
        base policy's from the state the env was in.  One host synchronisation per decision (the loop's end test).  Returns the number
        of values() calls made."""
        n = 0
        while True:
            reward, finished = self.values()
            n += 1
            if not bool(self.active.any()):
                return n
            self.env.step(self.best_actions(reward, finished), observe=False)
