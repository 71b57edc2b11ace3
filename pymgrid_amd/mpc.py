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


class _RecedingHorizon:
    """The loop the planners share: ``act()`` (the planner's own: the next action out of a lookahead at the env's current state),
    then ``env.step`` -- with the per-grid episode statistics.  A subclass sets ``self.env`` (a ``PerGridWindowEnv``)."""

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


class ShootingMPC(_RecedingHorizon):
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


CEM_KEY_TAG = 0xCE3F0000    # fourth Philox counter word of the draw cem_key takes its 64 bits from


def cem_key(seed, counter, iteration):
    """The key of CEM iteration ``iteration`` at step counter ``counter`` under ``seed``: 64 bits out of
    ``philox_words(seed, counter, iteration, CEM_KEY_TAG)`` -- integer arithmetic on the host, the same key on every machine and
    whatever device the env lies on, so a run is reproducible however it is cut into calls."""
    from .policy import philox_words
    r = philox_words(int(seed), int(counter), int(iteration), CEM_KEY_TAG, device="cpu")
    return int(r[0]) | (int(r[1]) << 32)


class CEMPlanner(_RecedingHorizon):
    """Receding-horizon control by the cross-entropy method on a continuous ``PerGridWindowEnv``: every grid keeps a Gaussian over
    its next ``horizon`` normalised controls (``mean`` / ``sigma`` float64 ``[H, N, A]``).  ``act()`` runs ``n_iters`` rounds of
    ``env.lookahead_gaussian`` (``n_candidates`` plans per grid drawn inside the launch; candidate 0 is the mean itself) and
    ``env.cem_refit`` (mean and deviation of the ``n_elite`` best, mixed in with weight ``alpha``, sigma floored at ``sigma_min``)
    under ``key = cem_key(seed, env.env.current_step, it)``, then one last lookahead under iteration number ``n_iters`` whose
    ``first_action`` it returns; ``self.last`` keeps that lookahead's results (so ``last["best_ret"] >= last["ret"][0]``, the
    refitted mean's return).  No plan tensor ``[C, H, N, A]`` exists at any point.

    ``warm_start=True``: the next ``act()`` starts from the refitted mean shifted by one step (its last row repeated) with sigma
    back at ``init_sigma`` -- one ``env.step`` is assumed between two calls; grids whose episode restarted in between (the counter
    value their episode started at has changed) start from ``init_mean``.  ``warm_start=False``: every ``act()`` starts from ``init_mean`` / ``init_sigma``.  Both are numbers or tensors
    that broadcast against ``[H, N, A]``."""

    def __init__(self, env, horizon, n_candidates=64, n_elite=8, n_iters=3, seed=0, gamma=1.0, init_mean=0.5, init_sigma=0.3,
                 sigma_min=0.01, alpha=1.0, warm_start=True):
        from .envs import DiscreteBatchedMicrogridEnv
        from .hetero import PerGridWindowEnv
        if not isinstance(env, PerGridWindowEnv):
            raise TypeError("env must be a PerGridWindowEnv (auto_reset=True): CEMPlanner plans over its lookahead_gaussian")
        why = env._lookahead_refusal()
        if why is None and isinstance(env.env, DiscreteBatchedMicrogridEnv):
            why = "discrete=True: the candidates are drawn round a mean of continuous controls"
        if why is not None:
            raise ValueError(f"CEMPlanner is not offered with {why}")
        self.env = env
        self.horizon, self.n_candidates, self.n_elite, self.n_iters = int(horizon), int(n_candidates), int(n_elite), int(n_iters)
        self.seed, self.gamma, self.alpha, self.sigma_min = int(seed), float(gamma), float(alpha), float(sigma_min)
        self.warm_start = bool(warm_start)
        if self.horizon < 1 or self.n_candidates < 1 or self.n_iters < 0:
            raise ValueError("horizon and n_candidates must be positive and n_iters non-negative")
        if not 1 <= self.n_elite <= min(self.n_candidates, 32):
            raise ValueError(f"n_elite = {n_elite} is outside [1, min(n_candidates, 32)]")
        if not 0.0 <= self.alpha <= 1.0 or not self.sigma_min >= 0.0:
            raise ValueError("alpha lies in [0, 1] and sigma_min is non-negative")
        e = env.env.engine
        shape = (self.horizon, e.N, e.action_dim)
        self._init = tuple(torch.as_tensor(v, dtype=torch.float64, device=e.device).expand(shape) for v in (init_mean, init_sigma))
        self.mean = self.sigma = None      # [H, N, A]: the distribution the latest act() left
        self._epoch = None                 # the counter value every grid's episode had started at, at the latest act()
        self.last = None                   # what the latest (final) lookahead returned

    def _start(self):
        """``mean`` / ``sigma`` as the coming ``act()`` starts from them."""
        epoch = self.env.env.engine._window_t0       # (in-place episodes: the step kernels keep it current)
        if self.mean is None or not self.warm_start:
            self.mean = self._init[0].clone()
        else:
            went_on = (epoch == self._epoch).view(1, -1, 1)
            self.mean = torch.where(went_on, torch.cat([self.mean[1:], self.mean[-1:]]), self._init[0]).contiguous()
        self.sigma = self._init[1].clone()
        self._epoch = epoch.clone()

    def act(self):
        """The next controls ``[N, A]`` (as ``env.step`` takes them) out of ``n_iters`` rounds of lookahead and refit and a last
        lookahead at the env's current state; nothing of the env moves."""
        env, C_ = self.env, self.n_candidates
        t = env.env.current_step
        self._start()
        for it in range(self.n_iters):
            key = cem_key(self.seed, t, it)
            out = env.lookahead_gaussian(self.mean, self.sigma, C_, key, gamma=self.gamma, pick=False)
            env.cem_refit(out["ret"], out["steps"], self.mean, self.sigma, key, self.n_elite, alpha=self.alpha,
                          sigma_min=self.sigma_min, best_plan=False, out={"mean": self.mean, "sigma": self.sigma})
        self.last = env.lookahead_gaussian(self.mean, self.sigma, C_, cem_key(self.seed, t, self.n_iters), gamma=self.gamma)
        return self.last["first_action"]
