"""Any of the ten module layouts the fused kernels are compiled for (template parameter F: bit 0 genset, bit 1 battery, bit 2 grid,
bit 3 grid before battery), carved out of ONE generated ``genset+battery+grid`` batch: the columns of the absent modules are
dropped, everything else -- series, parameters, initial state -- is cloned, so the ten batches differ in their module set alone.

The second half builds the inputs of the GENERAL path (several modules of a kind per grid) from parameter dicts
(``MicrogridBatch.from_grids`` on the device, ``oracle.OracleMultiMicrogrid`` on the CPU) and collects what the oracle returns into
arrays, so that a test compares whole columns: ``general_grids`` / ``general_controls`` / ``drawn_lists``, ``OracleGrids``,
``addend_counts``, ``log_columns``, ``episodes_vs_oracle``.

The third part is the reference side of the single-step family (tests/test_single_step_matrix.py): ``single_params`` turns the
columns of a carved batch into the dicts ``oracle.OracleMicrogrid`` takes, ``OracleSingles`` steps one such microgrid per grid."""
import dataclasses

import numpy as np

F_GENSET, F_BATTERY, F_GRID, F_GRID_FIRST = 1, 2, 4, 8
LAYOUTS = (0, 1, 2, 3, 4, 5, 6, 7, 14, 15)
FACTOR_GRID_COLUMNS = ("base_co2", "co2_profile", "tariff", "outage_bits")


def flags_of(layout):
    """The kernels' F of a BatchLayout (one module of every present kind)."""
    return (F_GENSET * layout.has_genset) | (F_BATTERY * layout.has_battery) | (F_GRID * layout.has_grid) \
        | (F_GRID_FIRST * layout.grid_before_battery)


def belongs_to(name):
    """The module kind a column belongs to: "genset" / "battery" / "grid", or None (load, renewable, unbalanced energy)."""
    if name.startswith("gen_"):
        return "genset"
    if name.startswith("bat_") or name in ("charge", "soc"):
        return "battery"
    if name.startswith("grid_") or name in FACTOR_GRID_COLUMNS:
        return "grid"
    return None


def carve(full, flags):
    """A MicrogridBatch of layout ``flags`` with clones of the columns of ``full`` (a ``generate(arch="genset+battery+grid")``
    batch, materialised or factorised) that the layout keeps."""
    from pymgrid_amd import MicrogridBatch
    if flags not in LAYOUTS:
        raise ValueError(f"layout {flags} is not one of {LAYOUTS}")
    L = full.layout
    if not (L.has_genset and L.has_battery and L.has_grid) or L.multi or L.grid_before_battery:
        raise ValueError("carve() starts from a genset+battery+grid batch with one module of every kind")
    has = {"genset": bool(flags & F_GENSET), "battery": bool(flags & F_BATTERY), "grid": bool(flags & F_GRID)}
    layout = dataclasses.replace(L, n_genset=int(has["genset"]), n_battery=int(has["battery"]), n_grid=int(has["grid"]),
                                 grid_before_battery=bool(flags & F_GRID_FIRST))
    cols = {name: t.clone() for name, t in full.cols.items() if has.get(belongs_to(name), True)}
    sub = MicrogridBatch(layout, cols, forecast_noise=full.forecast_noise)
    assert flags_of(sub.layout) == flags, (flags, sub.layout)
    return sub


def walked(cols, rows):
    """The columns of a batch (``numpy_columns()``) with the [K, N] series every grid walked in place of the [T, N] ones: ``rows``
    int [K, N], grid i's series row at step k, restarts included."""
    K = rows.shape[0]
    assert rows.min() >= 0 and rows.max() < cols["layout"]["T"]
    out = dict(cols)
    out["layout"] = dict(cols["layout"], T=K, final_step=K)
    out["load_ts"] = np.ascontiguousarray(np.take_along_axis(cols["load_ts"], rows, 0))
    out["pv_ts"] = np.ascontiguousarray(np.take_along_axis(cols["pv_ts"], rows, 0))
    if cols.get("grid_ts") is not None:
        out["grid_ts"] = np.ascontiguousarray(np.take_along_axis(cols["grid_ts"], rows[:, None, :].repeat(4, 1), 0))
    return out


def replay(oracle, cols, trace, normalized=True, label=""):
    """The fused launches of ``trace`` against the CPU oracle: the series every grid walked (its row at every step, restarts
    included) out of ``cols``, the materialised columns of the batch before the first launch, replayed from row 0 -- a restart
    keeps the module state and moves only the counter, so one batch run covers the restarts.  Rewards and the state after the last
    launch must equal the fused ones on every grid: the oracle may leave none out.  ``trace``: ``launches`` (per launch ``rows``
    [K, N], ``controls`` ids [K, N] or controls [K, N, A], ``reward`` [K, N]), ``state`` (the state columns after the last launch)
    and, for ids, ``table`` (the priority lists)."""
    st = {k: cols[k].copy() for k in ("charge", "soc", "gen_status") if k in cols}
    rows = np.concatenate([ln["rows"].cpu().numpy() for ln in trace["launches"]]).astype(np.int64)
    controls = np.concatenate([ln["controls"].double().cpu().numpy() if ln["controls"].is_floating_point() else ln["controls"].cpu().numpy()
                               for ln in trace["launches"]])
    reward = np.concatenate([ln["reward"].cpu().numpy() for ln in trace["launches"]])
    K, n = rows.shape
    assert len(np.unique(rows[0])) > 10 and (np.diff(rows, axis=0) != 1).any()         # own rows, and restarts among them
    series = walked(cols, rows)
    failed = np.zeros(n, dtype=np.uint8)
    if trace.get("table") is not None:
        ref = oracle.rollout_batch(series, st, 0, K, controls, trace["table"], nthreads=8, failed=failed)
    else:
        ref = oracle.run_batch(series, st, 0, K, controls, normalized=normalized, nthreads=8, failed=failed)
    assert int(failed.sum()) == 0, f"{label}: the oracle left out {int(failed.sum())} of {n} grids"
    assert np.array_equal(reward, ref), label
    for name, want in st.items():
        got = trace["state"][name].cpu().numpy()
        assert np.array_equal(got.view(np.uint32) if name == "gen_status" else got, want), (label, name)


# ---- the general path: grids with several modules of a kind, built from parameter dicts ------------------------------------------
PLAIN, STRESSED, MIRRORED = 0, 1, 2


def random_multi_grid(rs, T, n_gen, n_bat, n_grid, n_load, n_pv, horizon=0, grid_first=False):
    """The parameter dict of one microgrid with the given numbers of modules: every instance its own parameters, every grid
    instance its own ``grid_ts`` (outages among its rows), gensets with timers 0..2 and both initial states."""
    g = dict(load_ts=80 * rs.rand(T, n_load) + 5, pv_ts=60 * rs.rand(T, n_pv) * (rs.rand(T, n_pv) > 0.3), horizon=horizon,
             final_step=T, initial_step=0, unbalanced=dict(loss_load_cost=10.0, overgeneration_cost=1.0 + rs.rand()),
             controllable_order=["genset", "grid", "battery"] if grid_first else ["genset", "battery", "grid"])
    if n_gen:
        g["genset"] = [dict(running_min_production=float(rs.choice([0.0, 5.0, 12.0])), running_max_production=40.0 + 40 * rs.rand(),
                            genset_cost=0.3 + 0.3 * rs.rand(), co2_per_unit=2.0, cost_per_unit_co2=0.1,
                            start_up_time=int(rs.randint(0, 3)), wind_down_time=int(rs.randint(0, 3)),
                            init_start_up=bool(rs.randint(0, 2))) for _ in range(n_gen)]
    if n_bat:
        g["battery"] = [dict(min_capacity=10.0, max_capacity=60.0 + 80 * rs.rand(), max_charge=20.0 + 10 * rs.rand(),
                             max_discharge=25.0, efficiency=float(rs.choice([0.9, 0.95, 1.0])), battery_cost_cycle=0.02 * rs.rand(),
                             init_soc=0.3 + 0.6 * rs.rand()) for _ in range(n_bat)]
    if n_grid:
        g["grid"] = [dict(max_import=30.0 + 40 * rs.rand(), max_export=20.0 + 30 * rs.rand(), cost_per_unit_co2=0.1)
                     for _ in range(n_grid)]
        g["grid_ts"] = [np.stack([0.1 + rs.rand(T), 0.5 * rs.rand(T), 0.3 * rs.rand(T), (rs.rand(T) > 0.2).astype(float)], axis=1)
                        for _ in range(n_grid)]
    return g


def populations(N, mirrored=False):
    """[N] PLAIN / STRESSED / MIRRORED: the first half of the grids is the stressed population (loads x 4, batteries and grids asked
    to discharge and import: long ``provided`` lists that end in loss load); with ``mirrored`` the last quarter is its mirror image
    (pvs x 4, batteries and grids asked to charge and export: long ``absorbed`` lists that end in overgeneration)."""
    pop = np.full(N, PLAIN)
    pop[:N // 2] = STRESSED
    if mirrored:
        pop[N - N // 4:] = MIRRORED
    return pop


def general_grids(flags, counts, N, T, seed, horizon=0, mirrored=False):
    """N parameter dicts of layout ``flags`` (one of LAYOUTS; ``controllable_order`` follows bit 3) with ``counts`` = (n_genset,
    n_battery, n_grid, n_load, n_pv) modules, for ``MicrogridBatch.from_grids`` and ``oracle.OracleMultiMicrogrid``."""
    ng, nb, nr, nl, npv = counts
    if flags not in LAYOUTS or (ng > 0, nb > 0, nr > 0) != (bool(flags & F_GENSET), bool(flags & F_BATTERY), bool(flags & F_GRID)):
        raise ValueError(f"the counts {counts} are not a mix of layout {flags}")
    if min(nl, npv) < 1 or max(counts) < 2:
        raise ValueError(f"{counts}: the general path takes at least one load and pv, and several modules of some kind")
    rs = np.random.RandomState(seed)
    grids = [random_multi_grid(rs, T, ng, nb, nr, nl, npv, horizon, bool(flags & F_GRID_FIRST)) for _ in range(N)]
    for g, p in zip(grids, populations(N, mirrored)):
        if p == STRESSED:
            g["load_ts"] = g["load_ts"] * 4
        elif p == MIRRORED:
            g["pv_ts"] = g["pv_ts"] * 4
    return grids


def general_controls(rs, K, N, counts, mirrored=False):
    """Normalised controls [K, N, A]: U[0, 1), the battery and grid columns of the stressed population from the upper half (they
    discharge and import), of the mirrored one from the lower half."""
    ng, nb, nr = counts[:3]
    a = rs.rand(K, N, 2 * ng + nb + nr)
    pop = populations(N, mirrored)
    a[:, pop == STRESSED, 2 * ng:] = 0.5 + 0.5 * a[:, pop == STRESSED, 2 * ng:]
    a[:, pop == MIRRORED, 2 * ng:] = 0.5 * a[:, pop == MIRRORED, 2 * ng:]
    return a


def raw_controls(a, counts):
    """Unnormalised controls out of normalised ones: genset goals 0 / 1, genset requests in [0, 60), battery and grid requests in
    [-42, 78) (the stressed population's above 18)."""
    ng = counts[0]
    raw = (a * 2 - 0.7) * 60
    raw[..., 0:2 * ng:2] = np.round(a[..., 0:2 * ng:2])
    raw[..., 1:2 * ng:2] = a[..., 1:2 * ng:2] * 60
    return raw


def instances_differ(grids):
    """True where, in every grid, any two instances of a kind differ in a parameter (and any two grid instances in their series)."""
    for g in grids:
        for kind in ("genset", "battery", "grid"):
            inst = g.get(kind, [])
            for i in range(len(inst)):
                for j in range(i):
                    if inst[i] == inst[j] or (kind == "grid" and np.array_equal(g["grid_ts"][i], g["grid_ts"][j])):
                        return False
        for name in ("load_ts", "pv_ts"):
            ts = g[name]
            if any(np.array_equal(ts[:, i], ts[:, j]) for i in range(ts.shape[1]) for j in range(i)):
                return False
    return True


def drawn_lists(rs, counts, n_lists=24):
    """int32 [n_lists, width, 3] priority lists over module instances, drawn by hand (the reference's enumeration is factorial in the
    elements): every module somewhere, genset goals 0 / 1, a module named twice (the second is skipped, priority_list.py:82-88),
    padding and an element the layout does not have in between; one list in five stops short of the last modules."""
    ng, nb, nr = counts[:3]
    mods = [(0, j) for j in range(ng)] + [(1, j) for j in range(nb)] + [(2, j) for j in range(nr)]
    rows = []
    for _ in range(n_lists):
        els = [(k, j, int(rs.randint(0, 2)) if k == 0 else 0) for k, j in (mods[q] for q in rs.permutation(len(mods)))]
        els.insert(int(rs.randint(0, len(els) + 1)), (-1, -1, -1))
        els.insert(int(rs.randint(0, len(els) + 1)), (int(rs.randint(0, 3)), 5, 0))
        els.insert(int(rs.randint(1, len(els) + 1)), els[0])
        rows.append(els[: len(mods) + 3] if rs.rand() < 0.8 else els[: max(1, len(mods) - 1)])
    width = max(len(r) for r in rows)
    tab = -np.ones((len(rows), width, 3), dtype=np.int32)
    for q, r in enumerate(rows):
        tab[q, :len(r)] = r
    return tab


def own_elements(table, counts):
    """The lists of ``table`` [n_lists, width, 3] as the oracle takes them: padding and elements naming a module the layout does not
    have are left out, as the device skips them."""
    n = counts[:3]
    return [[(int(k), int(j), int(a)) for k, j, a in pl if 0 <= k <= 2 and 0 <= j < n[k]] for pl in table]


def status_words(cur, goal, up, down):
    """The device's packed genset status (uint32) of the oracle's four counters."""
    return (np.asarray(cur).astype(np.uint32) | (np.asarray(goal).astype(np.uint32) << 8) | (np.asarray(up).astype(np.uint32) << 16)
            | (np.asarray(down).astype(np.uint32) << 24))


class OracleGrids:
    """``oracle.OracleMultiMicrogrid`` of every grid of a batch, stepped together; what the oracle returns is collected into arrays
    (a record array of ``MStepOut`` per step, observation rows, state columns) so that a test compares column by column.  An
    exception of the oracle (the reference's AssertionError, an unbalanced step) is not caught: no grid may be left out."""

    def __init__(self, oracle, grids):
        self.oms = [oracle.OracleMultiMicrogrid(g) for g in grids]
        self.dtype = np.dtype(oracle.MStepOut)
        self.N = len(grids)

    def reset(self, rows):
        """Moves every grid's counter (``rows``: one row, or [N]) and keeps the module state, as Microgrid.reset does -> obs [N, D]."""
        rows = np.broadcast_to(np.asarray(rows), (self.N,))
        return np.stack([om.reset(int(t)) for om, t in zip(self.oms, rows)])

    def set_rows(self, rows, only=None):
        """Moves the counter of every grid (``only``: of the grids of a mask [N]) to ``rows`` [N]."""
        for j in (range(self.N) if only is None else np.flatnonzero(only)):
            self.oms[j].s.t = int(rows[j])

    def rows(self):
        return np.array([om.s.t for om in self.oms])

    def observe(self):
        return np.stack([om.observe() for om in self.oms])

    def step(self, controls, normalized=True):
        """One ``run`` of every grid (controls [N, A]) -> MStepOut records [N]."""
        rec = np.empty(self.N, dtype=self.dtype)
        for j, om in enumerate(self.oms):
            rec[j] = np.frombuffer(om.run(controls[j], normalized), dtype=self.dtype, count=1)[0]
        return rec

    def run(self, controls, normalized=True, observe=False):
        """K steps (controls [K, N, A]) -> records [K, N] (and the observation rows [K, N, D] behind every step)."""
        recs, obs = [], []
        for a in controls:
            recs.append(self.step(a, normalized))
            if observe:
                obs.append(self.observe())
        return (np.stack(recs), np.stack(obs)) if observe else np.stack(recs)

    def expand(self, plists):
        """``populate_action`` of every grid's list (``plists``: N lists of (kind, instance, action)) -> raw controls [N, A]."""
        return np.stack([om.populate_action(pl) for om, pl in zip(self.oms, plists)])

    def state(self):
        """The state columns as the batch holds them: charge / soc [n_battery, N], gen_status uint32 [n_genset, N]."""
        c = self.oms[0].counts
        out = {}
        if c["battery"]:
            out["charge"] = np.array([[om.s.battery[q].charge for om in self.oms] for q in range(c["battery"])])
            out["soc"] = np.array([[om.s.battery[q].soc for om in self.oms] for q in range(c["battery"])])
        if c["genset"]:
            st = [[(om.s.genset[q].gen_cur, om.s.genset[q].gen_goal, om.s.genset[q].gen_up, om.s.genset[q].gen_down)
                   for om in self.oms] for q in range(c["genset"])]
            out["gen_status"] = status_words(*np.moveaxis(np.array(st), -1, 0))
        return out


def log_columns(rec, names):
    """name -> the oracle's column [..., N] of the device's log (``engine.log_names``: ``name`` / ``name[j]``) out of MStepOut
    records; ``genset_status`` is the packed word as the log holds it (a double); ``violations`` is not the oracle's (None).  The
    vectorised twin of ``OracleMultiMicrogrid.log_row`` (tests/test_layouts.py holds the two against each other)."""
    out = {}
    flat = "common" not in rec.dtype.names                    # StepOut records of OracleSingles: one module of a kind, one record
    common = rec if flat else rec["common"]
    part = (lambda kind, j: rec) if flat else (lambda kind, j: rec[kind][..., j])
    for n in names:
        base, j = (n[:n.index("[")], int(n[n.index("[") + 1:-1])) if n.endswith("]") else (n, 0)
        assert not (flat and j), n
        if base == "genset_status":
            g = part("genset", j)
            out[n] = status_words(g["gen_cur"], g["gen_goal"], g["gen_up"], g["gen_down"]).astype(np.float64)
        elif base.startswith("genset_"):
            out[n] = part("genset", j)[base]
        elif base in ("discharge_amount", "charge_amount", "battery_reward", "soc_pre", "charge_pre"):
            out[n] = part("battery", j)[base]
        elif base.startswith("grid_"):
            out[n] = part("grid", j)[base]
        else:
            out[n] = common[base] if base in common.dtype.names else None
    return out


def assert_log_equals(log, rec, names, label=""):
    """A device log [..., L, N] (host array) against the oracle's records [..., N], column by column, bit for bit."""
    columns = log_columns(rec, names)
    assert len(columns) == len(names) == log.shape[-2]
    assert [n for n, want in columns.items() if want is None] == ["violations"], "a log column the oracle side does not know"
    for c, (n, want) in enumerate(columns.items()):
        if want is not None:
            assert np.array_equal(log[..., c, :], want), (label, n)


def requests(grids, controls, normalized):
    """(battery requests [..., N, n_battery], grid requests [..., N, n_grid]) in energy units, as ``battery_step`` / ``grid_step`` of
    oracle/mgx_oracle.c denormalise a control (low + (high - low) * v, a zero spread taken as 1), in their order of operations."""
    nb, nr = len(grids[0].get("battery", [])), len(grids[0].get("grid", []))
    ng = len(grids[0].get("genset", []))
    bat, grd = controls[..., 2 * ng:2 * ng + nb], controls[..., 2 * ng + nb:]
    if not normalized:
        return bat, grd

    def denormalise(lo, hi, v):
        spread = hi - lo
        return lo + np.where(spread == 0.0, 1.0, spread) * v
    par = lambda kind, key: np.array([[q[key] for q in g.get(kind, [])] for g in grids], dtype=np.float64).reshape(len(grids), -1)  # noqa: E731
    if nb:
        bat = denormalise(-par("battery", "max_discharge") / par("battery", "efficiency"),
                          par("battery", "max_charge") * par("battery", "efficiency"), bat)
    if nr:
        grd = denormalise(-1 * par("grid", "max_export"), par("grid", "max_import"), grd)
    return bat, grd


def addend_counts(grids, rec, controls, normalized):
    """(addends of ``provided``, addends of ``absorbed``) [..., N] of the oracle steps ``rec`` (MStepOut records) taken under
    ``controls`` [..., N, A]: by the rule of ``mstep_append`` in oracle/mgx_oracle.c a module appends ONE addend, a zero included, to
    the list of the side it acted on -- a genset and a pv to ``provided``, a load to ``absorbed``, a battery and a grid by the SIGN OF
    THE REQUEST (below zero: ``absorbed``; zero and above: ``provided``), not by the amount that went through (an empty battery asked
    to discharge appends 0.0 to ``provided``) -- and the unbalanced-energy module closes the step on ``absorbed`` (overgeneration:
    the balance after the controllable modules is positive) or on ``provided`` (loss load).  The records hold the amounts, not the
    requests, so the sign is taken from the controls; where an amount is not zero it must agree, which is asserted."""
    g0 = grids[0]
    ng, nb, nr = len(g0.get("genset", [])), len(g0.get("battery", [])), len(g0.get("grid", []))
    nl, npv = g0["load_ts"].shape[1], g0["pv_ts"].shape[1]
    bat, grd = requests(grids, controls, normalized)
    bat_source, grid_source = ~(bat < 0), ~(grd < 0)
    assert not (rec["battery"]["charge_amount"][..., :nb] != 0)[bat_source].any()
    assert not (rec["battery"]["discharge_amount"][..., :nb] != 0)[~bat_source].any()
    assert not (rec["grid"]["grid_export"][..., :nr] != 0)[grid_source].any()
    assert not (rec["grid"]["grid_import"][..., :nr] != 0)[~grid_source].any()
    over = rec["common"]["overgeneration"] > 0
    assert not (over & (rec["common"]["loss_load"] != 0)).any()
    provided = ng + npv + bat_source.sum(-1) + grid_source.sum(-1) + ~over
    absorbed = nl + (~bat_source).sum(-1) + (~grid_source).sum(-1) + over
    return provided, absorbed


class EpisodeReplay:
    """The steps of ``env``, a PerGridWindowEnv(auto_reset=True), replayed on the CPU oracle ``og`` (an ``OracleGrids`` or
    ``OracleSingles`` over the env's batch) with the rows every grid walked, taken from what the env reports (``starts``, ``lengths``,
    ``current_steps``): a restart moves the counter and keeps the module state.  ``begin(obs)`` takes the rows of the env's reset,
    ``oracle_step(a)`` steps the oracle under the ids / controls ``a`` and returns the tensor the env takes, ``after(k, ...)`` holds what
    the env's step returned against it: rewards, done flags (an episode is over when its length is used up), observation rows (of a
    restarted grid: the first row of its new episode; ``final``: ``info["final_observation"]`` of the finished grids, the oracle's rows
    behind the step, before the restart moves the counter; float32 rows: the oracle's rounded), ``finish()`` the state of every module
    instance -- the oracle's, bit for bit, on every grid.  The steps of a fleet's buckets interleave: one replay per bucket."""

    def __init__(self, env, og, label="", final=False):
        import torch
        self.env, self.og, self.label, self.final = env, og, label, final
        self.discrete = hasattr(env.env, "actions_list")
        self.rounded = (lambda rows: rows.astype(np.float32)) if env.env.engine.obs_dtype == torch.float32 else (lambda rows: rows)
        self.restarts = np.zeros(og.N, dtype=np.int64)

    def lengths_now(self):
        env = self.env
        return np.full(self.og.N, env.length) if env.lengths is None else env.lengths.cpu().numpy().astype(np.int64)

    def begin(self, obs):
        env = self.env
        self.rows, self.left = env.env.current_steps.cpu().numpy(), self.lengths_now()
        assert np.array_equal(self.rows, env.starts.cpu().numpy()), self.label
        assert np.array_equal(obs.cpu().numpy(), self.rounded(self.og.reset(self.rows))), (self.label, "first rows")

    def oracle_step(self, a):
        import torch
        env, og = self.env, self.og
        if self.discrete:
            lists = env.env.actions_list
            single = isinstance(og, OracleSingles)                # its lists hold (module, action) elements
            plists = [lists[i] if env.env._instances or single else [(m, 0, act) for m, act in lists[i]] for i in a]
            self.want = og.step(og.expand(plists), False)
            return torch.as_tensor(a, dtype=torch.int32, device=env.full.device)
        self.want = og.step(a, True)
        return torch.as_tensor(a, dtype=env.env.engine.action_dtype, device=env.full.device)

    def after(self, k, obs, reward, done, info):
        env, og, label = self.env, self.og, self.label
        done = done.cpu().numpy().astype(bool)
        assert np.array_equal(reward.cpu().numpy(), common(self.want)["reward"]), (label, k)
        left = self.left - 1
        assert np.array_equal(done, left == 0), (label, k)
        if self.final:
            assert np.array_equal(info["final_observation"].cpu().numpy()[done], self.rounded(og.observe())[done]), (label, k, "final rows")
        after = env.env.current_steps.cpu().numpy()
        assert np.array_equal(after[~done], self.rows[~done] + 1) and np.array_equal(after[done], env.starts.cpu().numpy()[done]), (label, k)
        self.rows, self.left = after, np.where(done, self.lengths_now(), left)
        self.restarts += done
        og.set_rows(after, only=done)                             # a restart moves the counter; every other grid's is the oracle's own
        assert np.array_equal(og.rows(), after), (label, k)
        assert np.array_equal(obs.cpu().numpy(), self.rounded(og.observe())), (label, k, "rows")

    def finish(self):
        for name, want in self.og.state().items():
            got = self.env.env.batch.cols[name].cpu().numpy().reshape(want.shape)
            assert np.array_equal(got.view(np.uint32) if name == "gen_status" else got, want), (self.label, name)
        return self.restarts


def episodes_vs_oracle(oracle, env, grids, K, draw, first=None, label="", final=False):
    """K steps of ``env``, a PerGridWindowEnv(auto_reset=True) over ``MicrogridBatch.from_grids(grids)`` (continuous or discrete; not
    yet reset), replayed on the CPU oracle (``EpisodeReplay``): rewards, done flags, observation rows and the final state of every
    module instance must be the oracle's, bit for bit, on every grid.  ``grids``: the parameter dicts (the multi-instance oracle), or
    the oracle side itself (an ``OracleSingles`` over the env's batch); ``draw(k)``: ids [N] of the env's ``actions_list`` or
    normalised controls [N, A] of step k (host arrays); ``first``: the (starts, lengths) of the first episodes, else the env draws
    them; ``final``: the env reports ``info["final_observation"]``.  Returns the restarts per grid."""
    og = grids if isinstance(grids, (OracleGrids, OracleSingles)) else OracleGrids(oracle, grids)
    replay = EpisodeReplay(env, og, label, final)
    replay.begin(env.reset(*first) if first is not None else env.reset())
    for k in range(K):
        replay.after(k, *env.step(replay.oracle_step(draw(k))))
    return replay.finish()


# ---- the single-step family: one module of every kind, an OracleMicrogrid per grid ------------------------------------------------
KIND_NAMES = ("genset", "battery", "grid")                   # module ids of a priority-list element (pymgrid_amd.priority_list)


def common(rec):
    """The whole-microgrid fields (reward, done, the balance) of step records: MStepOut's ``common``, or the StepOut itself."""
    return rec["common"] if "common" in rec.dtype.names else rec


def single_params(cols):
    """``MicrogridBatch.numpy_columns()`` of a batch with one module of every kind (a ``carve()``) -> the N parameter dicts
    ``oracle.OracleMicrogrid`` takes: the series, every parameter, the battery's ``charge`` / ``soc`` and the genset's four status
    counters as the batch holds them now, ``controllable_order`` (grid first: layouts 14 / 15), ``horizon`` and ``final_step``."""
    lay = cols["layout"]
    N, grid_first = lay["N"], bool(lay.get("grid_before_battery", 0))
    assert cols["load_ts"].shape == cols["pv_ts"].shape == (lay["T"], N), "one load and one pv per grid"
    out = []
    for j in range(N):
        f = lambda name: float(cols[name][j])                # noqa: E731
        p = dict(load_ts=np.ascontiguousarray(cols["load_ts"][:, j]), pv_ts=np.ascontiguousarray(cols["pv_ts"][:, j]),
                 horizon=int(lay["horizon"]), initial_step=0, final_step=int(lay["final_step"]),
                 unbalanced=dict(loss_load_cost=f("loss_load_cost"), overgeneration_cost=f("overgeneration_cost")),
                 controllable_order=["genset", "grid", "battery"] if grid_first else ["genset", "battery", "grid"])
        if lay["has_battery"]:
            p["battery"] = dict(min_capacity=f("bat_min_capacity"), max_capacity=f("bat_max_capacity"), max_charge=f("bat_max_charge"),
                                max_discharge=f("bat_max_discharge"), efficiency=f("bat_efficiency"),
                                battery_cost_cycle=f("bat_cost_cycle"), charge=f("charge"), soc=f("soc"))
        if lay["has_genset"]:
            times, word = int(cols["gen_times"][j]), int(cols["gen_status"][j])
            p["genset"] = dict(running_min_production=f("gen_running_min"), running_max_production=f("gen_running_max"),
                               genset_cost=f("gen_cost"), co2_per_unit=f("gen_co2_per_unit"), cost_per_unit_co2=f("gen_cost_per_unit_co2"),
                               start_up_time=times & 0xff, wind_down_time=(times >> 16) & 0xff, allow_abortion=not (times >> 8) & 1,
                               status=[word & 0xff, (word >> 8) & 0xff, (word >> 16) & 0xff, (word >> 24) & 0xff])
        if lay["has_grid"]:
            p["grid"] = dict(max_import=f("grid_max_import"), max_export=f("grid_max_export"), cost_per_unit_co2=f("grid_cost_per_unit_co2"))
            p["grid_ts"] = np.ascontiguousarray(cols["grid_ts"][:, :, j])
        out.append(p)
    return out


class OracleSingles:
    """``oracle.OracleMicrogrid`` of EVERY grid of a batch with one module of every kind (``numpy_columns()`` through
    ``single_params``), stepped together with the oracle's own surface -- ``run``, ``observe``, ``reset``, ``populate_action`` -- and
    collected into arrays: StepOut records, observation rows, state columns.  The twin of ``OracleGrids``; an exception of the oracle
    (the reference's AssertionError, an unbalanced step, an assert of ``_populate_action``) is not caught: no grid may be left out."""

    def __init__(self, oracle, cols):
        lay = cols["layout"]
        self.has = (bool(lay["has_genset"]), bool(lay["has_battery"]), bool(lay["has_grid"]))
        self.oms = [oracle.OracleMicrogrid(p) for p in single_params(cols)]
        self.dtype = np.dtype(oracle.StepOut)
        self.N = len(self.oms)
        self.action_dim = 2 * self.has[0] + self.has[1] + self.has[2]

    def reset(self, rows):
        """Moves every grid's counter (``rows``: one row, or [N]) and keeps the module state -> obs [N, D]."""
        rows = np.broadcast_to(np.asarray(rows), (self.N,))
        return np.stack([om.reset(int(t)) for om, t in zip(self.oms, rows)])

    def set_rows(self, rows, only=None):
        for j in (range(self.N) if only is None else np.flatnonzero(only)):
            self.oms[j].s.t = int(rows[j])

    def rows(self):
        return np.array([om.s.t for om in self.oms])

    def observe(self):
        return np.stack([om.observe() for om in self.oms])

    def _control(self, a):
        """A control row (genset goal, genset energy, battery, grid: the ones the layout has) as ``run`` takes it."""
        d, c = {}, 0
        if self.has[0]:
            d["genset"] = (a[0], a[1]); c = 2
        if self.has[1]:
            d["battery"] = a[c]; c += 1
        if self.has[2]:
            d["grid"] = a[c]
        return d

    def step(self, controls, normalized=True):
        """One ``run`` of every grid (controls [N, A]) -> StepOut records [N]."""
        rec = np.empty(self.N, dtype=self.dtype)
        for j, om in enumerate(self.oms):
            rec[j] = np.frombuffer(om.run(self._control(controls[j]), normalized), dtype=self.dtype, count=1)[0]
        return rec

    def run(self, controls, normalized=True, observe=False):
        """K steps (controls [K, N, A]) -> records [K, N] (and the observation rows [K, N, D] behind every step)."""
        recs, obs = [], []
        for a in controls:
            recs.append(self.step(a, normalized))
            if observe:
                obs.append(self.observe())
        return (np.stack(recs), np.stack(obs)) if observe else np.stack(recs)

    def expand(self, plists):
        """``populate_action`` of every grid's list (``plists``: N lists of (module id, action)) -> raw controls [N, A]."""
        out = np.zeros((self.N, self.action_dim))
        for j, (om, pl) in enumerate(zip(self.oms, plists)):
            d = om.populate_action([(KIND_NAMES[m], act) for m, act in pl])
            out[j] = list(d.get("genset", [])) + [d[k] for k in ("battery", "grid") if k in d]
        return out

    def state(self):
        """The state columns as the batch holds them: charge / soc [N], gen_status uint32 [N]."""
        out = {}
        if self.has[1]:
            out["charge"] = np.array([om.s.charge for om in self.oms])
            out["soc"] = np.array([om.s.soc for om in self.oms])
        if self.has[0]:
            out["gen_status"] = status_words(*np.array([om.status for om in self.oms]).T)
        return out
