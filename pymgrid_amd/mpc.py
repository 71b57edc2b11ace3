"""Planning by simulation ("shooting" model-predictive control) over ``PerGridWindowEnv.lookahead``.

The reference's ``ModelPredictiveControl`` (algos/mpc/mpc.py) chooses the next control by solving a cvxpy program over the forecast
horizon; that solver is not rebuilt here.  What it stands for -- the next control out of the microgrid simulated forward over the
horizon -- is: ``lookahead`` simulates C candidate plans per grid from the current state in one launch and commits none of them,
``lookahead_host`` states the rule of its results in torch, and ``ShootingMPC`` is the receding-horizon loop over it.
"""
import torch


def lookahead_host(reward, done, gamma=1.0):
    """The rule of ``mgx_lookahead`` (include/mgx.h) in torch, on any device, operation by operation, from what C roll-outs of H
    steps returned: ``reward`` float64 ``[C, H, N]`` (candidate c's per-step rewards), ``done`` bool or uint8 ``[H, N]`` (the
    grids' done flags over those steps: they depend on the grid alone).  Per grid and candidate ``ret = ret + w * r; w = w * gamma``
    in step order, up to and including the first step with ``done`` set and no further.  Returns ``ret`` ``[C, N]``, ``steps`` int32
    ``[N]`` (the steps counted), ``last`` int64 ``[N]`` (the index of the last counted step: where ``end_soc`` is read off a SoC
    trace), ``best`` int32 ``[N]`` (candidate 0, replaced by every later one whose return is GREATER: the first maximum) and
    ``best_ret`` ``[N]``."""
    if reward.dim() != 3 or done.dim() != 2 or tuple(done.shape) != (reward.shape[1], reward.shape[2]):
        raise ValueError(f"reward must be [C, H, N] and done [H, N], not {list(reward.shape)} and {list(done.shape)}")
    if reward.dtype != torch.float64:
        raise ValueError("reward must be float64")
    gamma = float(gamma)
    if not 0.0 <= gamma <= 1.0:
        raise ValueError(f"gamma = {gamma} is outside [0, 1]")
    C, H, N = reward.shape
    dev = reward.device
    ret = torch.zeros((C, N), dtype=torch.float64, device=dev)
    w = torch.ones((), dtype=torch.float64, device=dev)
    alive = torch.ones(N, dtype=torch.bool, device=dev)            # the grid's episode has not ended before step k
    steps = torch.zeros(N, dtype=torch.int32, device=dev)
    for k in range(H):
        ret = torch.where(alive, ret + w * reward[:, k], ret)
        w = w * gamma
        steps = steps + alive.to(torch.int32)
        alive = alive & (done[k] == 0)
    best = torch.zeros(N, dtype=torch.int32, device=dev)
    best_ret = ret[0].clone()
    for c in range(1, C):
        better = ret[c] > best_ret
        best = torch.where(better, torch.full_like(best, c), best)
        best_ret = torch.where(better, ret[c], best_ret)
    return {"ret": ret, "steps": steps, "last": steps.to(torch.int64) - 1, "best": best, "best_ret": best_ret}


def _generator(seed, counter):
    """The host generator of the random plans of step counter ``counter``: a function of ``(seed, counter)`` alone, the same draws
    whatever device the plans go to."""
    g = torch.Generator(device="cpu")
    g.manual_seed((int(seed) * 1000003 + int(counter)) & (2 ** 63 - 1))
    return g


def shooting_candidates(n_lists, horizon, n_random=0, seed=0, counter=0, device=None):
    """``ShootingMPC``'s default discrete candidate set: uint8 ``[n_lists + n_random, horizon]`` -- one CONSTANT plan per priority
    list (row j holds id j at every step), then ``n_random`` id sequences uniform over the lists, a function of ``(seed, counter)``
    alone."""
    n, H, R = int(n_lists), int(horizon), int(n_random)
    if not 1 <= n <= 256 or H < 1 or R < 0:
        raise ValueError("need 1 <= n_lists <= 256, horizon >= 1, n_random >= 0")
    const = torch.arange(n, dtype=torch.int64).view(n, 1).expand(n, H)
    rnd = torch.randint(0, n, (R, H), generator=_generator(seed, counter), dtype=torch.int64)
    return torch.cat([const, rnd]).to(torch.uint8).to(device or "cpu").contiguous()


class ShootingMPC:
    """Receding-horizon control by enumeration / random shooting over ``env.lookahead`` (``env``: a ``PerGridWindowEnv`` that offers
    it).  Every step: one lookahead of the candidate plans over ``horizon`` steps, the pick of the best plan per grid, its first
    action executed with ``env.step``.

    ``candidates=None`` -- the default set.  Discrete env: one CONSTANT plan per priority list (list j at every step: the rule-based
    controllers, so with ``n_random=0`` the controller picks per grid and step the list whose H-step return is best) followed by
    ``n_random`` id sequences (``shooting_candidates``); continuous env: ``n_random`` plans uniform in [0, 1]^A (normalised controls).  The random plans are
    shared by all grids and redrawn every step from a ``torch.Generator`` seeded with ``(seed, env.env.current_step)``, so a run is
    reproducible however it is cut into calls.  ``candidates=``: a tensor of plans as ``lookahead`` takes them, or a callable
    ``(env) -> plans`` evaluated every step -- how a CEM or warm-started loop plugs in."""

    def __init__(self, env, horizon, candidates=None, n_random=0, seed=0, gamma=1.0):
        from .envs import DiscreteBatchedMicrogridEnv
        from .hetero import PerGridWindowEnv
        if not isinstance(env, PerGridWindowEnv):
            raise TypeError("env must be a PerGridWindowEnv (auto_reset=True): ShootingMPC plans over its lookahead")
        why = env._lookahead_refusal()
        if why is not None:
            raise ValueError(f"ShootingMPC is not offered with {why}")
        self.env = env
        self.discrete = isinstance(env.env, DiscreteBatchedMicrogridEnv)
        self.horizon = int(horizon)
        self.n_random = int(n_random)
        self.seed = int(seed)
        self.gamma = float(gamma)
        if self.horizon < 1 or self.n_random < 0:
            raise ValueError("horizon must be positive and n_random non-negative")
        self.candidates = candidates
        if candidates is None and not self.discrete and self.n_random < 1:
            raise ValueError("a continuous env has no default plans without n_random >= 1 (or pass candidates=)")
        e = env.env.engine
        self._dev = e.device
        if self.discrete:
            self._constant = shooting_candidates(int(env.env.action_space.n), self.horizon, device=self._dev)
        self.last = None                   # what the latest lookahead returned

    def default_candidates(self, counter=None):
        """The default plans at step counter ``counter`` (default: the env's): ``shooting_candidates`` of the env's priority lists,
        or, for a continuous env, ``n_random`` uniform plans ``[n_random, H, A]`` in the env's ``action_dtype``."""
        counter = int(self.env.env.current_step if counter is None else counter)
        if self.discrete:
            if self.n_random == 0:
                return self._constant
            return shooting_candidates(self._constant.shape[0], self.horizon, self.n_random, self.seed, counter, self._dev)
        e = self.env.env.engine
        u = torch.rand((self.n_random, self.horizon, e.action_dim), generator=_generator(self.seed, counter), dtype=torch.float64)
        return u.to(device=self._dev, dtype=e.action_dtype)

    def plans(self):
        """The candidate plans of the coming step."""
        c = self.candidates
        if c is None:
            return self.default_candidates()
        return c(self.env) if callable(c) else c

    def act(self):
        """One lookahead and pick at the env's current state: ``first_action`` of the best plan per grid, as ``env.step`` takes it
        (int32 ids ``[N]``, or controls ``[N, A]``).  ``self.last`` keeps the lookahead's results (``ret``, ``steps``, ``best``,
        ``best_ret``, ``first_action``)."""
        self.last = self.env.lookahead(self.plans(), gamma=self.gamma)
        a = self.last["first_action"]
        return a.to(torch.int32) if self.discrete else a

    def run(self, n_steps, reward=True, done=False):
        """The receding-horizon loop for ``n_steps`` steps from where the env stands (``env.reset()`` first): one lookahead, one
        pick, one ``env.step`` per step.  Returns the stacked ``reward`` / ``done`` ``[n_steps, N]`` asked for and the per-grid
        episode statistics by the names of ``RuleBasedControl.run_episodes`` (``episode_return_sum``, ``episode_return_last``,
        ``episodes``, ``return_running``), accumulated in ``env.episode_stats`` by the rule of ``mgx_episode_stats`` and carried on
        into a later call."""
        env = self.env
        if env.starts is None:
            raise RuntimeError("run() before env.reset()")
        e = env.env.engine
        if env.episode_stats is None:
            env.episode_stats = {name: torch.zeros(e.N, dtype=dtype, device=e.device) for name, dtype in e.EPISODE_STATS}
        st = env.episode_stats
        rows = {"reward": [], "done": []}
        for _ in range(int(n_steps)):
            _, r, d, _ = env.step(self.act())
            # mgx_episode_stats' rule, stated on the host (single steps carry no statistics of their own)
            run = st["ret_running"] + r
            st["ret_last"].copy_(torch.where(d, run, st["ret_last"]))
            st["ret_sum"].copy_(torch.where(d, st["ret_sum"] + run, st["ret_sum"]))
            st["episodes"].add_(d.to(torch.int32))
            st["ret_running"].copy_(torch.where(d, torch.zeros_like(run), run))
            if reward:
                rows["reward"].append(r.clone())
            if done:
                rows["done"].append(d.clone())
        res = {name: torch.stack(v) if v else torch.empty((0, e.N), dtype=torch.float64 if name == "reward" else torch.bool, device=e.device)
               for name, v in rows.items() if (reward if name == "reward" else done)}
        res.update(episode_return_sum=st["ret_sum"], episode_return_last=st["ret_last"], episodes=st["episodes"],
                   return_running=st["ret_running"])
        return res
