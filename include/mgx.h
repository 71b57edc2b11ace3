/*
 * mgx.h -- C ABI of the MI355X-native batched microgrid-step engine (libmgx.so).
 *
 * The reference (Total-RD/pymgrid v1.2.2) is pure Python and has NO FFI: its boundary for this hot path is
 * the Gym surface  DiscreteMicrogridEnv.step / BaseMicrogridEnv.step / reset
 * (src/pymgrid/envs/discrete/discrete.py:109-143, src/pymgrid/envs/base/base.py:165-209) over
 * Microgrid.run / Microgrid.reset (src/pymgrid/microgrid/microgrid.py:227-325, :205-219).
 * This header is what a binding for that path would bind (INTEGRATION.md shows the ctypes stub): every
 * entry point below names the reference interface it replaces.  Plain C types only -- no torch, no HIP
 * types in the signatures (a stream is passed as void*, it is a hipStream_t).
 *
 * Conventions
 *  - N microgrids ("grids") advance in lock-step; all share the step counter t, the series length T and
 *    the episode window [initial_step, final_step) -- unless the episode was started with mgx_reset_windows, which
 *    gives every grid its own start row and episode length (its own trajectory) behind the shared counter.
 *  - Every pointer in mgx_columns and every data argument is a DEVICE pointer owned by the caller
 *    (e.g. torch tensors); the library allocates only a small scratch buffer in mgx_create.
 *  - All arithmetic is IEEE fp64, unfused (no FMA contraction), in the reference's operation order.
 *  - Zero signs: every output equals the reference's VALUE bit for bit, except that a result that is zero may carry the other
 *    sign (+0.0 vs -0.0).  The reference produces -0.0 in places (-1.0 * get_cost(0.0); a flex source asked for `-difference`
 *    with difference == 0.0, microgrid.py:300-314), its min / max return the first argument on ties where v_min_f64 /
 *    v_max_f64 order -0 < +0; no operation of the path divides by such a zero or takes its sign, so the difference cannot
 *    propagate into a non-zero value.  Parity tests compare with `==` (profiles/r03/zero_signs.txt has the census).
 *  - Calls are asynchronous on the given stream and must be issued from one host thread per handle.
 *  - Return value: MGX_OK or an error code; mgx_last_error() gives a thread-local message.
 *
 * Column layouts (struct-of-arrays, grid index fastest):
 *    parameter / state columns   [N]
 *    load_ts, pv_ts              [T, N]     sign as the reference STORES it: load <= 0, pv >= 0
 *                                           (base_timeseries_module.py:68-79); with several load / renewable
 *                                           modules per grid: [T, n_load, N] / [T, n_pv, N], bounds [n, N]
 *    grid_ts                     [T, 4, N]  components import_price, export_price, co2_per_kwh, grid_status
 *                                           (grid_module.py:70)
 *    actions                     [N, A]     A = 2*has_genset + has_battery + has_grid, order
 *                                           genset(goal_status, energy), battery, grid = the reference's
 *                                           controllable sweep order (module_container.py:355-413)
 *    obs                         [N, D]     D = mgx_obs_dim(); order load(1+H), pv(1+H), genset(4), battery(2),
 *                                           grid(4*(1+H), component-minor) -- or, with mgx_layout.flat_order = MGX_FLAT_GYM,
 *                                           battery, genset, grid, load, pv
 *    log                         [L, N]     L = mgx_log_dim(); names from mgx_log_name()
 */
#ifndef MGX_H
#define MGX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MGX_ABI_VERSION 9    /* frozen: struct layouts and the meaning of every v9 entry point do not change any more */
#define MGX_ABI_MINOR 3      /* additions only: 1 = mgx_abi_minor, mgx_set_tunable / mgx_get_tunable, mgx_set_launch_threads,
                              * mgx_action_bounds; 2 = mgx_step_lists; 3 = MGX_TUNE_FLEET_EPISODES */

enum mgx_status {
    MGX_OK = 0,
    MGX_ERR_INVALID = 1,      /* bad argument / inconsistent layout */
    MGX_ERR_UNSUPPORTED = 2,  /* valid in the reference, not offered on device */
    MGX_ERR_RANGE = 3,        /* step counter would leave the time series (IndexError in the reference) */
    MGX_ERR_DEVICE = 4        /* HIP runtime error (message holds hipGetErrorString) */
};

/* element type of the observation rows (mgx_set_obs_format) */
enum mgx_obs_format { MGX_OBS_F64 = 0, MGX_OBS_F32 = 1 };
/* element type of the continuous `actions` of mgx_step / mgx_step_k (mgx_set_action_format) */
enum mgx_action_format { MGX_ACT_F64 = 0, MGX_ACT_F32 = 1 };
/* what the `obs` argument of mgx_step / mgx_step_discrete / mgx_observe / mgx_reset receives (mgx_set_obs_mode) */
enum mgx_obs_rows { MGX_OBS_ROWS_FULL = 0, MGX_OBS_ROWS_STATE_ONLY = 1, MGX_OBS_ROWS_STATE_COMPACT = 2 };
/* what the `done` argument of the fused calls (mgx_step_k, mgx_rollout_discrete) receives (mgx_set_done_format) */
enum mgx_done_format { MGX_DONE_U8 = 0, MGX_DONE_BITS = 1 };

/* Reward shaping functions of the reference (microgrid/reward_shaping/): what step() RETURNS as reward.
 * The log's "reward" column always keeps the unshaped sum (the balance log's `reward` vs `shaped_reward`). */
enum mgx_reward_shaper {
    MGX_SHAPER_NONE = 0,
    MGX_SHAPER_PV_CURTAILMENT = 1,     /* PVCurtailmentShaper:    -curtailment                       */
    MGX_SHAPER_BATTERY_DISCHARGE = 2   /* BatteryDischargeShaper: (discharge - loss_load) / load     */
};

/* Bits of a violations mask (mgx_check_step, mgx_check_discrete, the `violations` outputs of mgx_expand_discrete /
 * mgx_expand_lists, the last log column).  Bits 0-2: requests the reference refuses only with raise_errors=True
 * (base_module.py:79-93,213-224,265-270).  Bits 3-8: states in which the reference ALWAYS gives up with an AssertionError /
 * TypeError -- the device goes on with the clipped value (unspecified there); the mask is how a caller finds out. */
enum mgx_violation_bit {
    MGX_V_GENSET_RANGE = 1,        /* genset request outside [min_production, max_production] */
    MGX_V_BATTERY_LIMIT = 2,       /* battery request above max_production / max_consumption */
    MGX_V_GRID_LIMIT = 4,          /* grid request above max import / export */
    MGX_V_GENSET_GOAL = 8,         /* genset goal_status outside [0, 1] (`assert`, genset_module.py:146-147) */
    MGX_V_GENSET_NEGATIVE = 16,    /* negative genset energy: a pure source asked to absorb */
    MGX_V_NEGATIVE_LIMIT = 32,     /* a battery / grid acting at a NEGATIVE limit: asked to absorb while its max_consumption is
                                    * negative -- `assert absorbed_energy >= 0` (base_module.py:272), a lossy battery whose charge
                                    * was rounded one ulp above max_capacity -- or to produce (even 0.0) while its max_production
                                    * is negative -- `assert internal_energy_change <= 0` (battery_module.py:114), a battery
                                    * below min_capacity */
    MGX_V_EXPAND_CONSUME = 64,     /* discrete expansion: `assert module_max_consumption >= 0` (priority_list.py:124), the same
                                    * battery state met by _consume_in_module with load left to absorb */
    MGX_V_EXPAND_PRODUCE = 128,    /* discrete expansion: `assert module_production >= 0` (priority_list.py:154): a module whose
                                    * max_production is negative (a battery below min_capacity) is asked to produce */
    MGX_V_EXPAND_SIGN = 256        /* discrete expansion: `assert total_load >= 0 and renewable >= 0` / `assert remaining_load
                                    * <= 0.0` (priority_list.py:73,121): series of the wrong sign, NaN */
};
/* The expansion bits are exclusive: the reference stops at the first assert that fails on its way down the priority list,
 * and the mask names that one. */

typedef struct mgx_handle mgx_handle;
typedef void *mgx_stream;     /* hipStream_t */

/* Static shape of the batch.  Replaces the module list handed to Microgrid.__init__ (microgrid.py:100-128). */
typedef struct mgx_layout {
    int32_t struct_size;      /* = sizeof(mgx_layout), ABI guard */
    int32_t n_grids;          /* N */
    int32_t n_steps;          /* T, rows of every time series */
    int32_t horizon;          /* forecast_horizon H of the (oracle) forecaster, 0 = no forecast */
    int32_t initial_step;     /* base_module.py:40 */
    int32_t final_step;       /* resolved as base_timeseries_module.py:317-330 does: <=0 means T */
    int32_t has_genset;       /* 0/1 GensetModule  */
    int32_t has_battery;      /* 0/1 BatteryModule */
    int32_t has_grid;         /* 0/1 GridModule    */
    int32_t n_load;           /* LoadModule count      (1 on the fast path; 0..16 via the general kernels) */
    int32_t n_pv;             /* RenewableModule count (1 on the fast path; 0..16 via the general kernels) */
    int32_t grid_before_battery;   /* 0/1: the GridModule precedes the BatteryModule in the microgrid's module list and is
                                    * therefore stepped / summed first (module_container.py:355-413; the controllable
                                    * sweep is pure sources, then sources-and-sinks in list order).  Changes the last
                                    * bit of the balance sums, not the action / log / observation column order. */
    /* Module multiplicities (the container holds a LIST of modules per name, module_container.py:355-413, and
     * Microgrid.run sweeps every list in order, microgrid.py:262-275): 0 = "as has_*" (0 or 1).  With n > 1 every
     * column of that module kind is [n, N] (instance-major), grid_ts is [T, n_grid, 4, N], grid_lo / grid_hi
     * [n_grid, 4, N]; actions are (goal, energy) per genset, then the batteries, then the grids; the log carries one
     * block per instance; observations one group of state columns / one grid window per instance.  Such layouts run on
     * the general kernels (as do n_load / n_pv != 1): single steps, K-step launches (mgx_step_k, mgx_rollout_lists),
     * observations, priority lists (mgx_expand_lists). */
    int32_t n_genset, n_battery, n_grid;      /* <= MGX_MAX_INSTANCES */
    /* Order of the module blocks inside a flat observation row (envs/base/base.py:128-163,211-223: the reference flattens
     * a gym.spaces.Dict built from a plain dict, and gym sorts the keys of such a Dict):
     *   MGX_FLAT_MODULE (0)  load, pv, genset, battery, grid   (this library's native order)
     *   MGX_FLAT_GYM    (1)  battery, genset, grid, load, pv   (alphabetical by module name: what a policy trained against the
     *                        reference with gym <= 0.26 / gymnasium sees)
     * Only the column BASES of the blocks move (every kernel writes a block at its base): no cost.  One module of every kind
     * per grid only. */
    int32_t flat_order;
} mgx_layout;

enum mgx_flat_order { MGX_FLAT_MODULE = 0, MGX_FLAT_GYM = 1 };

#define MGX_MAX_INSTANCES 8

/* Device columns.  Pointers for absent modules may be NULL. */
/* Batch-UNIFORM parameter columns (mgx_columns.uniform_mask): bit b set = the parameter column b below holds ONE value that
 * every grid shares (the pointer addresses a single element; kernels index it with 0).  MicrogridGenerator gives every microgrid
 * the same battery efficiency / cycle cost, genset cost / co2 figures, unbalanced-energy costs and -- unless drawn -- genset
 * timers (convert/get_module.py:39-97, MicrogridGenerator.py:472): 60 of the 108 parameter bytes a single step reads per grid.
 * Values are the same, the loads become same-address (broadcast) loads out of the caches.  One module of every kind only. */
enum mgx_uniform_bit {
    MGX_U_BAT_MIN_CAPACITY = 0, MGX_U_BAT_MAX_CAPACITY, MGX_U_BAT_MAX_CHARGE, MGX_U_BAT_MAX_DISCHARGE, MGX_U_BAT_EFFICIENCY,
    MGX_U_BAT_COST_CYCLE, MGX_U_GEN_RUNNING_MIN, MGX_U_GEN_RUNNING_MAX, MGX_U_GEN_COST, MGX_U_GEN_CO2_PER_UNIT,
    MGX_U_GEN_COST_PER_UNIT_CO2, MGX_U_GEN_TIMES, MGX_U_GRID_MAX_IMPORT, MGX_U_GRID_MAX_EXPORT, MGX_U_GRID_COST_PER_UNIT_CO2,
    MGX_U_LOSS_LOAD_COST, MGX_U_OVERGENERATION_COST
};

typedef struct mgx_columns {
    int32_t struct_size;      /* = sizeof(mgx_columns) */
    uint32_t uniform_mask;    /* bits of enum mgx_uniform_bit; 0 = every column is [N] */
    /* BatteryModule parameters (battery_module.py:66-93) */
    const double *bat_min_capacity, *bat_max_capacity, *bat_max_charge, *bat_max_discharge;
    const double *bat_efficiency, *bat_cost_cycle;
    /* GensetModule parameters (genset_module.py:61-98) */
    const double *gen_running_min, *gen_running_max, *gen_cost, *gen_co2_per_unit, *gen_cost_per_unit_co2;
    const uint32_t *gen_times;            /* start_up_time | (!allow_abortion) << 8 | wind_down_time << 16 (times <= 255) */
    /* GridModule parameters (grid_module.py:72-101) */
    const double *grid_max_import, *grid_max_export, *grid_cost_per_unit_co2;
    /* UnbalancedEnergyModule parameters (unbalanced_energy_module.py:11-26) */
    const double *loss_load_cost, *overgeneration_cost;
    /* time series */
    const double *load_ts, *pv_ts, *grid_ts;
    /* observation bounds (needed only when observations are requested):
     * base_timeseries_module.py:81-88 (load/pv: min(ts.min(),0), max(ts.max(),0)), grid_module.py:125-132 */
    const double *load_lo, *load_hi, *pv_lo, *pv_hi;      /* [N] */
    const double *grid_lo, *grid_hi;                      /* [4, N] */
    /* GaussianNoiseForecaster (forecast/forecaster.py:220-275): per-grid noise standard deviation of each module's
     * forecast, already scaled by |mean(series)| when relative_noise is set; NULL = OracleForecaster */
    const double *load_noise_std, *pv_noise_std, *grid_noise_std;   /* [N] */
    /* dynamic state, read and written by every step */
    double *charge, *soc;                 /* BatteryModule._current_charge / _soc */
    uint32_t *gen_status;                 /* current | goal<<8 | steps_until_up<<16 | steps_until_down<<24 */
    /* FACTORISED series (optional; base_load != NULL switches it on).  Every series MicrogridGenerator builds is one of a
     * few base profiles times a per-grid scalar (MicrogridGenerator.py:137-147 _scale_ts: ts * (size / ts.max()); :205-212
     * co2 profile verbatim; :253-285 import tariff by hour of day; :321-340 weak-grid outages), so a generated batch is
     * fully described by the base tables + a profile id and a ratio per grid.  In this mode load_ts / pv_ts / grid_ts may be
     * NULL and the kernels FORM the series values as they go, with the same single multiply the generator performs:
     *     load[t, i] = -|base_load[t, load_profile[i]] * load_ratio[i]|     (sign as stored, base_timeseries_module.py:68-79)
     *     pv[t, i]   =  |base_pv[t, pv_profile[i]] * pv_ratio[i]|
     *     grid[t, :, i] = (tariff price of hour t % 24 under pattern tariff[i] (1 or 2), 0, base_co2[t, co2_profile[i]],
     *                      1 - bit t of grid i's outage words)
     * -- bit-identical to the arrays mgx_synthesize_series writes.  The [T, N] series (16 of the 57 B a fused env-step of a
     * Template-4 grid streams; 14 GB per 100 000 grid-years) then never exist; the base tables (<= 560 KB each) stay in
     * the caches.  Base tables are [n_steps, MGX_PROFILE_PITCH] doubles (one 64-byte row per step, unused columns
     * arbitrary), profile ids < MGX_PROFILE_PITCH and tariff in {0, 1, 2} -- a PRECONDITION the library cannot check (device
     * pointers): an id beyond the pitch reads a neighbouring row / table.  outage_bits: [ceil(n_steps / 64), N] words, bit (t & 63) of word
     * t >> 6 set = grid_status 0 at row t; NULL = no outages.  Offered with one module of every kind per grid (the general
     * kernels read materialised series only). */
    const double *base_load, *base_pv, *base_co2;
    const uint8_t *load_profile, *pv_profile, *co2_profile, *tariff;      /* [N] */
    const double *load_ratio, *pv_ratio;                                   /* [N] */
    const uint64_t *outage_bits;
} mgx_columns;

#define MGX_PROFILE_PITCH 8

/* ---- lifetime ------------------------------------------------------------------------------------- */
int mgx_abi_version(void);
int mgx_abi_minor(void);

/* Process-wide launch-shape knobs.  The library reads nothing from the environment: this is the only way to change what the
 * measurements behind DESIGN.md chose, and a consumer can read back what a process runs with.  They change HOW a call is
 * launched (never a value it computes) and take effect for the calls / handles that follow. */
enum mgx_tunable {
    MGX_TUNE_WIN_THREADS = 0,      /* threads of a ring-refill workgroup: 0 = automatic, 256 / 512 / 1024 */
    MGX_TUNE_WIN_GROUP = 1,        /* grids per refill workgroup: 0 = automatic (16 / 32), else a power of two <= 64 */
    MGX_TUNE_WIN_PAIRS = 2,        /* column-major refill stores carry a pair of adjacent grids per lane: -1 = automatic, 0, 1 */
    MGX_TUNE_WIN_MIN_LDS = 3,      /* LDS bytes a refill ahead of the counter asks for at least (occupancy cap): -1 = automatic */
    MGX_TUNE_PREFETCH_POOL = 4,    /* 1: one prefetch stream per device shared by all handles (default 0: one per handle) */
    MGX_TUNE_MULTI_GENERIC = 5,    /* 1: handles CREATED afterwards run every general layout on the run-time-count kernels */
    MGX_TUNE_MULTI_SMALL_OWN = 6,  /* 0: mgx_step_k of small general layouts through the shared kernel (default 1: its own) */
    MGX_TUNE_GRID_MAJOR_COPY = 7,  /* 0: mgx_reset_episodes on [T, N] series gathers rows instead of making its grid-major copy */
    MGX_TUNE_FLEET_BYVALUE = 8,    /* 0: mgx_fleet_step launches the pointer form of the fleet kernel (default 1: by value) */
    MGX_TUNE_LAUNCH_THREADS = 9,   /* mode (0 / 1 / 2) handles created afterwards start with: mgx_set_launch_threads (default 1) */
    MGX_TUNE_MULTI_STATIC = 10,    /* 0: mgx_step_k of small general layouts never takes a compile-time-count specialisation (A/B, tests) */
    MGX_TUNE_FLEET_EPISODES = 11,  /* 0: mgx_fleet_step steps in-place-episode items beside its launches (default 1: one launch for them) */
    MGX_TUNE_STEP_K_HOT = 12,      /* 0: mgx_step_k never takes step_k_hot_kernel, the kernel of its own the lock-step reward + SoC launch on
                                    * factorised series without a GridModule has (default 1; same values either way: A/B, tests) */
    MGX_TUNE_COUNT_ = 13
};
int mgx_set_tunable(int32_t id, int64_t value);                                /* MGX_ERR_INVALID: unknown id / value out of range */
int mgx_get_tunable(int32_t id, int64_t *value, int64_t *default_value);       /* either pointer may be NULL */
/* thread-local text of the last error returned on this thread ("" if none) */
const char *mgx_last_error(void);

/* Microgrid.__init__ (microgrid.py:100-128): bind a layout + columns.  The step counter starts at
 * layout->initial_step. */
int mgx_create(const mgx_layout *layout, const mgx_columns *columns, mgx_handle **out);
void mgx_destroy(mgx_handle *h);

/* ---- shape queries -------------------------------------------------------------------------------- */
int32_t mgx_action_dim(const mgx_handle *h);
int32_t mgx_obs_dim(const mgx_handle *h);
int32_t mgx_log_dim(const mgx_handle *h);
const char *mgx_log_name(const mgx_handle *h, int32_t column);   /* NULL if out of range */
int32_t mgx_current_step(const mgx_handle *h);                   /* BaseMicrogridModule.current_step */

/* Keep the step counter in DEVICE memory (enable != 0) so that a sequence of mgx_step / mgx_step_discrete / mgx_step_k /
 * mgx_rollout_discrete / mgx_observe calls can be captured in a hipGraph (stream capture) and replayed: kernels read
 * the counter, the last workgroup of every stepping kernel to finish advances it.  While enabled, launch-time range checks are
 * replaced by an in-kernel clamp + sticky overrun flag (reported as MGX_ERR_RANGE when the mode is switched off), and
 * mgx_current_step() performs a blocking device read (after synchronising the stream of the last call that moved the
 * counter).  Disabling copies the counter back to the host. */
int mgx_use_device_counter(mgx_handle *h, int enable, mgx_stream stream);

/* ---- the hot path --------------------------------------------------------------------------------- */
/* Microgrid.reset (microgrid.py:205-219) -> BaseMicrogridModule.reset (base_module.py:65-77): the step counter
 * returns to initial_step (or to `initial_step` if >= 0: the trajectory_func hook, microgrid.py:221-225);
 * battery charge and genset status are NOT touched (the reference does not restore them).
 * obs [N, D] may be NULL. */
int mgx_reset(mgx_handle *h, int32_t initial_step, void *obs, mgx_stream stream);

/* Episode window [initial_step, final_step) for the next reset -- what a trajectory_func returns
 * (microgrid.py:221-225, microgrid/trajectory/ classes; validated like _check_trajectory_func, microgrid.py:181-203:
 * inside the window given at create, initial < final).  Does not move the step counter; call mgx_reset next. */
int mgx_set_window(mgx_handle *h, int32_t initial_step, int32_t final_step);

/* Per-grid episodes.  In the reference every Microgrid owns its step counter and draws its own trajectory at reset
 * (Microgrid.reset -> _set_trajectory, microgrid.py:205-225; BaseMicrogridModule.reset, base_module.py:65-77,292-296;
 * FixedLengthStochasticTrajectory / StochasticTrajectory, microgrid/trajectory/stochastic.py:9-30).  Batched form:
 * grid i starts at series row start[i] and its episode lasts length[i] steps (NULL: max_length for every grid), i.e.
 * it reports done from counter value length[i] - 1 on (base_timeseries_module.py:124-125 with its own final_step =
 * start[i] + length[i]).  A HIP kernel gathers rows [start[i], start[i] + max_length + horizon] of every grid's series
 * into the caller's window buffers load_w / pv_w [R, N], grid_w [R, 4, N] (R = max_length + horizon + 1; rows beyond
 * the end of a series hold the forecaster's padding value (lo + hi) / 2, forecaster.py:95,120-137), and the handle then
 * steps over those buffers from counter 0: mgx_current_step() = steps since the reset, grid i's own current_step =
 * start[i] + mgx_current_step().  start / length are DEVICE arrays [N]; a start outside the window given at create is
 * clamped into it and a length is cut at the env's final step (the reference raises ValueError in
 * _check_trajectory_func, microgrid.py:181-203: validate on the host if the arrays come from outside).  final_rel [N]
 * (device, int32; required with `length`) receives the episode lengths actually used and must stay alive until the
 * next reset.  Observation bounds stay those of the full series.  Stepping past the longest episode (counter >= max_length)
 * is MGX_ERR_RANGE, like stepping past the end of a series.  mgx_reset() returns to the full series.
 * Layouts with several modules of a kind per grid (series [T, n, N]): load_w [R, n_load, N], pv_w [R, n_pv, N], grid_w
 * [R, n_grid, 4, N]; rings (mgx_observe_windows[_ahead]) work over them as over the full series.
 * MGX_ERR_UNSUPPORTED in device-counter mode, while stepping in shards, with column-major ring blocks. */
int mgx_reset_windows(mgx_handle *h, const int32_t *start, const int32_t *length, int32_t max_length,
                      double *load_w, double *pv_w, double *grid_w, int32_t *final_rel, void *obs, mgx_stream stream);

/* Rolling per-grid windows: N reference microgrids reset one by one, each when ITS episode ends (what a vectorised
 * Gym env does with auto-reset; microgrid.py:205-225 per microgrid, at different times).  As mgx_reset_windows, but the
 * window buffers [ring_rows, N] ([ring_rows, 4, N]) are rings addressed by (step counter & (ring_rows - 1)):
 * ring_rows a power of two >= max_length + horizon + 1.  The shared counter restarts at 0 and never ends; final_abs [N]
 * (device, required) receives the counter value at which each grid's episode has run its length, done_i =
 * counter >= final_abs[i] - 1.  Single steps only (mgx_step, mgx_step_discrete, mgx_step_many, mgx_observe,
 * mgx_observe_windows[_ahead] + mgx_patch_windows, ...); fused launches, shards and the device counter are refused in this
 * mode.  mgx_reset / mgx_reset_windows
 * leave it. */
int mgx_reset_windows_rolling(mgx_handle *h, const int32_t *start, const int32_t *length, int32_t max_length,
                              int32_t ring_rows, double *load_w, double *pv_w, double *grid_w, int32_t *final_abs, void *obs,
                              mgx_stream stream);
/* Restart the grids with mask[i] != 0 at the current counter value: their rows start[i] .. of the full series are
 * gathered into the rings from the current row on, final_abs[i] = counter + length[i] (length NULL: max_length).  Dynamic
 * state is untouched, as in Microgrid.reset.  mask / start / length: device arrays [N]. */
int mgx_reset_grids(mgx_handle *h, const uint8_t *mask, const int32_t *start, const int32_t *length, mgx_stream stream);
/* The same with the new episodes DRAWN ON DEVICE, one draw per restarted grid as its own trajectory_func would make it:
 * fixed_length > 0 = FixedLengthStochasticTrajectory(fixed_length) (start = randint(initial, final - length)),
 * fixed_length == 0 = StochasticTrajectory (start = randint(initial, final - 2), final = randint(start, final));
 * microgrid/trajectory/stochastic.py:9-30.  Uniforms: Philox4x32-10 of (seed; grid, 2 * counter [+ 1]) -- reproducible and
 * independent of how often or in which order grids restart.  start_io / length_io / t0_io (device [N], each may be NULL)
 * receive, for the restarted grids only, the drawn start row, the episode length and the counter value of the restart.
 * Both restart calls also serve in-place episodes (mgx_reset_episodes below): no rows are gathered then. */
int mgx_reset_grids_random(mgx_handle *h, const uint8_t *mask, uint64_t seed, int32_t fixed_length, int32_t *start_io,
                           int32_t *length_io, int32_t *t0_io, mgx_stream stream);

/* Rolling per-grid episodes IN PLACE.  Same model as mgx_reset_windows_rolling (one shared counter that restarts at 0 and
 * never ends, every grid with its own episode: microgrid.py:205-225 per microgrid), but nothing is copied: grid i simply reads
 * row counter + row_off[i] of its own series and reports done_i = counter >= final_abs[i] - 1.  With factorised series
 * (mgx_columns.base_load ...) the rows come out of small cached base tables; for [T, N] arrays the handle makes a grid-major
 * copy per call ([N, T, 2 or 6]: as much device memory again; a grid's own row is then one 16- or 48-byte read) -- if that
 * allocation is refused the lanes gather out of the [T, N] arrays instead (same values, slower).  row_off / final_abs: caller-owned
 * DEVICE arrays [N] that the handle keeps reading AND writing until the next mgx_reset*; start / length as for
 * mgx_reset_windows (length NULL: max_length).  (Re)starts -- mgx_reset_grids, mgx_reset_grids_random -- then rewrite two
 * words per grid instead of gathering rows.  Observation windows reach beyond an episode's end into the grid's series and
 * beyond the series' end into the forecaster's padding, exactly as in lock-step.  Single steps only (as for rolling windows);
 * observation rings work as they do there (mgx_observe_windows[_ahead] + mgx_patch_windows for the grids that restarted).
 * A grid whose episode is over and that has not been restarted (auto-reset off, or a late mgx_reset_grids) keeps stepping on
 * its own series; the shared counter has no end in this mode, so nothing refuses the step that would leave the series:
 * from row n_steps on such a grid re-reads its LAST row (the step stays defined and finite; its observation windows show the
 * forecaster's padding, as they do at the end of a series in lock-step).
 * Layouts with several modules of a kind (ABI minor 1): single steps of the general kernels, every grid reading its own rows of the
 * [T, n, N] series (a per-lane gather; no grid-major copy), restarts and mgx_set_auto_reset as above; observation rows per step
 * only (MGX_OBS_ROWS_FULL: the ring patches are single-instance) and no mgx_set_final_obs. */
int mgx_reset_episodes(mgx_handle *h, const int32_t *start, const int32_t *length, int32_t max_length, int32_t *row_off,
                       int32_t *final_abs, void *obs, mgx_stream stream);
/* Auto-reset inside the step (in-place episodes only): every single step restarts the grids whose episode it ends -- the
 * draw mgx_reset_grids_random(mask = done, seed, fixed_length) would make at the counter value after the step, made by the
 * step kernel itself -- so that the step's `obs` is, for those grids, the first observation of their new episode (what a
 * vectorised Gym env with auto-reset returns) and no further launch is needed.  start_io / length_io / t0_io as for
 * mgx_reset_grids_random (device [N], each may be NULL; kept until the mode is switched off or the next mgx_reset*).
 * Steps that restart so: mgx_step, mgx_step_discrete and, on layouts with several modules of a kind,
 * mgx_step_lists (discrete steps over priority lists of module instances: in ONE launch where the layout holds at most two
 * modules of a kind, in its two launches otherwise -- the restart then happens in the second).
 * enable = 0 switches it off. */
int mgx_set_auto_reset(mgx_handle *h, int32_t enable, uint64_t seed, int32_t fixed_length, int32_t *start_io, int32_t *length_io,
                       int32_t *t0_io);
/* Where the observation BEFORE a restart goes ("final_observation" of a vectorised Gym env): device [N, D] rows in the handle's
 * observation format.  Rows written per step (no ring): the following single steps write every grid's pre-restart row (grids
 * that do not restart get the same row as `obs`).  Prefetched rings (MGX_OBS_ROWS_STATE_ONLY): mgx_patch_windows saves the
 * row of block first_block of every MASKED grid here before it rewrites it; the other rows are left as they are.
 * NULL (default) = off.  In-place episodes only. */
int mgx_set_final_obs(mgx_handle *h, void *final_obs);

/* Microgrid.reward_shaping_func (microgrid.py:105,130): one of enum mgx_reward_shaper. */
int mgx_set_reward_shaper(mgx_handle *h, int32_t shaper);

/* GaussianNoiseForecaster switches: Philox seed of the forecast noise and `increase_uncertainty`
 * (std_j = std * (1 + log(1 + j)) for forecast_j, forecaster.py:243-249).  Noise is drawn per (grid, module
 * component, step, horizon index); statistical -- not bit -- parity with the reference's np.random.normal.
 * With several modules of a kind the *_noise_std columns are [n, N]: one std per module instance, independent streams. */
int mgx_set_forecast_noise(mgx_handle *h, uint64_t seed, int increase_uncertainty);

/* Element type of every `obs` argument below: MGX_OBS_F64 (default; the reference's float64 arrays) or MGX_OBS_F32
 * = the same value rounded to nearest float on the way out (what an RL policy consumes after gym's / torch's cast,
 * envs/base/base.py:211-223: half the bytes of the largest output of the step).  The pointers are `void *` for that
 * reason: [N, D] doubles or [N, D] floats. */
int mgx_set_obs_format(mgx_handle *h, int32_t format);

/* Element type of the continuous controls passed to mgx_step / mgx_step_k: MGX_ACT_F64 (default) or MGX_ACT_F32 -- a
 * policy network emits floats; they are widened to double exactly and every operation after that is the float64 one
 * (= the reference fed `actions.astype(float64)`).  Halves the action stream of the fused kernel (24 -> 12 of 57 B). */
int mgx_set_action_format(mgx_handle *h, int32_t format);

/* Window prefetch.  The time-series windows of an observation (load / pv / grid: current value + forecast, the bulk of
 * the row; base_timeseries_module.py:103-140, forecaster.py:120-149) depend on the series only, never on the actions, and
 * consecutive steps share all but one of their rows.  mgx_observe_windows writes the observation rows of the NEXT K
 * steps -- ring [K, N, D], block k = the row the reference returns at step counter t + k -- reading and normalising
 * every series value once instead of 1 + horizon times.  Block 0 is complete (state columns of the current state); in
 * blocks 1..K-1 the genset / battery state columns are zero: with mgx_set_obs_mode(MGX_OBS_ROWS_STATE_ONLY) the `obs`
 * argument of mgx_step / mgx_step_discrete (pass ring + k*N*D for the step that reaches counter t + k) receives just
 * those columns.  Values are identical to mgx_observe's.  MGX_ERR_UNSUPPORTED with forecast noise (it depends on the
 * (step, horizon index) pair).  Microgrids with several modules of a kind (module_container.py:355-413) are served by the
 * general form of the same kernel -- a window per load / renewable / grid module instance, 4 state columns per genset and
 * 2 per battery -- for lock-step episodes, row- or column-major blocks (tests/test_multi_windows.py: rows == the per-step rows). */
int mgx_observe_windows(mgx_handle *h, int32_t K, void *ring, mgx_stream stream);
/* Rows between consecutive blocks of the rings handed to mgx_observe_windows / mgx_observe_windows_ahead / mgx_fleet_step
 * refills (default: N, i.e. a dense [K, N, D] ring).  With N not a multiple of 16 the blocks of a dense ring are not
 * 128-byte aligned and every 1-KB wave store of the refill begins and ends in a partial line; a ring [K, P, D] with
 * P = N rounded up to 16 rows, block k = the first N rows of ring[k], avoids that. */
int mgx_set_ring_pitch(mgx_handle *h, int32_t rows);
/* Layout of a ring BLOCK.  MGX_RING_ROWS (default): [P, D] row-major -- a grid's observation is D consecutive values, the
 * reference's flat vector (envs/base/base.py:211-223).  MGX_RING_COLUMNS: [D, P] -- value (grid i, column c) at c * P + i, P = the
 * ring pitch (mgx_set_ring_pitch; a multiple of 32: whole 128-byte lines per 32 float / 16 double grids): the SAME [N, D] matrix read with strides (1, P), which is what a policy's
 * first matrix product takes either way.  Why: in a row-major block the step's state columns are 48 bytes at a 8 D-byte stride --
 * 100 000 scattered partial lines per step, 3.5-4 us of a 24-us config-5 fleet step (profiles/r04/exp_fleet_state_patch_cost.txt) --
 * in a column-major block they are six coalesced runs of 8 N bytes.  Applies to mgx_observe_windows[_ahead], the fleets' refills and
 * the state-only `obs` target of the steps (pass the block's base).  A ring written AHEAD of the counter does not touch the state
 * columns of a column-major block at all (they are lines of their own; the step that reaches the block writes them), where a
 * row-major one receives zeros.  Layouts with several modules of a kind per grid included (their 4 n_genset + 2 n_battery state
 * columns).  Lock-step episodes only (mgx_patch_windows and the in-place / rolling modes keep row-major rings). */
enum mgx_ring_layout { MGX_RING_ROWS = 0, MGX_RING_COLUMNS = 1 };
int mgx_set_ring_layout(mgx_handle *h, int32_t layout);
/* Rolling windows with prefetched rings: after mgx_reset_grids* has replaced the series rows of the grids with mask[i] != 0,
 * recompute the window columns of THEIR rows in blocks first_block .. K-1 of `ring` (block first_block = the row of
 * counter value current + ahead).  State columns are left as they are.  A ring written AHEAD of the counter
 * (mgx_observe_windows_ahead) may have read a restarting grid's rows before or while they were replaced: once it is complete
 * (mgx_prefetch_wait), patch into it every grid that restarted since it was launched (first_block = 0 at the moment the
 * counter reaches its block 0).  `restarted` (device [N], may be NULL, must not be `mask`): restarted[i] = 1 for every masked
 * grid -- the accumulator of that later patch. */
int mgx_patch_windows(mgx_handle *h, const uint8_t *mask, int32_t K, void *ring, int32_t first_block, int32_t ahead,
                      uint8_t *restarted, mgx_stream stream);
/* MGX_OBS_ROWS_STATE_COMPACT: `obs` receives ONLY the genset / battery state columns, as a dense [N, S] array,
 * S = 4 * has_genset + 2 * has_battery (the zero-copy observation contract: the window columns are views of the normalised
 * series written once by mgx_normalise_series). */
int mgx_set_obs_mode(mgx_handle *h, int32_t mode);

/* `done` of the fused calls.  MGX_DONE_U8 (default): one byte per grid and step, [K, N].  MGX_DONE_BITS: a bit set per step,
 * [K, W] uint16 words with W = ceil(N / 16), bit (i & 15) of word i >> 4 = done of grid i (little-endian: the row is a
 * ceil(N / 16) * 2-byte bit array) -- 1/8 byte instead of 1 byte per env-step, written by one lane in 16.
 * In lock-step (no per-grid episode ends) `done` is the same for every grid, done(k) = (t0 + k >= final_step - 1)
 * (base_timeseries_module.py:124-125): pass done = NULL and derive it from mgx_current_step / the window. */
int mgx_set_done_format(mgx_handle *h, int32_t format);

/* The zero-copy observation contract for a forecast horizon H > 0.  With the oracle forecaster the window columns of the
 * observation at step t are  norm[t .. t + H]  of a series normalised ONCE ((v - lo) / spread, space.py:207-218; rows past
 * the end of the series = the padding value (lo + hi) / 2, forecaster.py:95,120-137; the forecast clip, forecaster.py:139-149,
 * is the identity because lo / hi bound the series).  mgx_normalise_series writes that normalised copy GRID-major:
 *     load_n, pv_n  [N, R]      R = n_steps + horizon + 1 (the observation after the last step, counter = n_steps, is all padding)
 *     grid_n        [N, R, 4]   (component-minor: the reference's window order falls out of a flat slice)
 * as float64 or float32 (the handle's obs format) so that the window of grid i at step t is the contiguous slice
 * load_n[i, t : t + 1 + H] -- a strided VIEW, no bytes moved per step.  The contract needs every bound column to bound its
 * series (else the reference's forecast clip is not the identity and the views differ from its observations).  That is checked
 * ON DEVICE, asynchronously: the call itself returns MGX_OK; `clipped` (device int32[1], zeroed by the caller) is incremented per
 * offending value and must be read after the stream has synchronised -- a non-zero count means the views are NOT the
 * reference's observations (pymgrid_amd refuses such a batch).  Passing NULL skips the check: only for series known to lie
 * inside their bounds (e.g. bounds computed from the series, base_timeseries_module.py:81-88).  grid_n may be NULL without a
 * GridModule. */
int mgx_normalise_series(mgx_handle *h, void *load_n, void *pv_n, void *grid_n, int32_t *clipped, mgx_stream stream);

/* The same prefetch AHEAD of the counter, overlapped with the steps: block k of `ring` = the window columns of counter
 * value t + ahead + k (ahead >= 1; the state columns of every block are zero and are filled in by the steps that reach
 * them).  The kernel runs on the handle's own prefetch stream, behind everything queued on `stream` so far (the readers
 * of the ring's previous contents); mgx_prefetch_wait(h, s) makes stream s wait for the last prefetch.  Typical use:
 * three rings of K blocks -- while the steps walk ring r, ring r + 1 is being written and ring r - 1 is still readable by
 * the policy (pymgrid_amd/envs.py).  The series rows do not depend on the state, so the overlap needs no other ordering.
 * MGX_ERR_UNSUPPORTED in device-counter mode. */
int mgx_observe_windows_ahead(mgx_handle *h, int32_t ahead, int32_t K, void *ring, mgx_stream stream);
int mgx_prefetch_wait(mgx_handle *h, mgx_stream stream);

/* Normalised observation of the current state (BaseMicrogridModule.to_normalized(state), base_module.py:157;
 * forecast window + end-of-series padding forecaster.py:120-149,215-217). */
int mgx_observe(mgx_handle *h, void *obs, mgx_stream stream);

/* ONE Microgrid.run(control, normalized) for all N grids (microgrid.py:227-325), as BaseMicrogridEnv.step
 * returns it (base.py:169-209): reward [N], done [N] (0/1), optional post-step obs [N, D] and log [L, N].
 * The step counter advances by one.  MGX_ERR_RANGE if the counter is already outside the series. */
int mgx_step(mgx_handle *h, const void *actions, int normalized,
             double *reward, uint8_t *done, void *obs, double *log, mgx_stream stream);

/* K consecutive Microgrid.run calls in ONE launch: parameters and state stay in registers, actions
 * [K, N, A] are streamed.  Outputs (each may be NULL): reward [K, N], done [K, N], soc_trace [K, N],
 * status_trace [K, N] (post-step packed genset status), ret_acc [N] (+= sum of the K rewards per grid),
 * log [K, L, N].  Replaces the user loop `for a in actions: env.step(a)` (README.md:109-111). */
int mgx_step_k(mgx_handle *h, const void *actions, int32_t K, int normalized,
               double *reward, uint8_t *done, double *soc_trace, uint32_t *status_trace,
               double *ret_acc, double *log, mgx_stream stream);

/* DiscreteMicrogridEnv._get_action -> PriorityListAlgo._populate_action (discrete.py:82-88,
 * priority_list.py:69-167): expand one priority-list id per grid into an UNNORMALISED control [N, A]
 * (feed it to mgx_step(..., normalized=0)).  `table` is a HOST array [n_actions, 3, 2] of
 * (module, action) pairs, module 0 genset / 1 battery / 2 grid, -1 = padding; n_actions <= 12.
 * violations [N] uint32 (device, may be NULL) receives, per grid, the assert the reference's _populate_action would have
 * failed in this state (MGX_V_EXPAND_*; 0 = none): there the reference raises AssertionError and returns no control. */
int mgx_expand_discrete(mgx_handle *h, const int32_t *action_id, const int32_t *table, int32_t n_actions,
                        double *control, uint32_t *violations, mgx_stream stream);

/* The same for priority lists over module INSTANCES (microgrids with several gensets / batteries / grids:
 * get_priority_lists enumerates (module name, module number, action) elements, priority_list.py:15-67, and there can
 * be hundreds of lists): `lists` is a DEVICE array int32 [n_lists, list_len, 3] of (kind, instance, action), kind
 * 0 genset / 1 battery / 2 grid, kind -1 = padding.  Works for every layout. */
int mgx_expand_lists(mgx_handle *h, const int32_t *action_id, const int32_t *lists, int32_t n_lists, int32_t list_len,
                     double *control, uint32_t *violations /* as in mgx_expand_discrete; may be NULL */, mgx_stream stream);

/* K fused discrete steps with priority lists over module instances: the general-path counterpart of
 * mgx_rollout_discrete (`for a in ids: env.step(a)`, discrete.py:109-143, or RuleBasedControl.run with one fixed list
 * per grid, rbc.py:64-93).  action_id int32 [K, N] (per_step != 0) or [N]; lists as in mgx_expand_lists; outputs as in
 * mgx_step_k (soc_trace / status_trace report battery 0 / genset 0).  Works for every layout. */
int mgx_rollout_lists(mgx_handle *h, const int32_t *action_id, int per_step, const int32_t *lists, int32_t n_lists,
                      int32_t list_len, int32_t K, double *reward, uint8_t *done, double *soc_trace,
                      uint32_t *status_trace, double *ret_acc, double *log, mgx_stream stream);

/* DiscreteMicrogridEnv.step (discrete.py:109-143) in ONE launch: mgx_expand_discrete + mgx_step(normalized=0) with the
 * control kept in registers.  control [N, A] (optional, may be NULL) receives the expanded control; the other
 * outputs are those of mgx_step. */
int mgx_step_discrete(mgx_handle *h, const int32_t *action_id, const int32_t *table, int32_t n_actions, double *control,
                      double *reward, uint8_t *done, void *obs, double *log, mgx_stream stream);

/* (minor 2) DiscreteMicrogridEnv.step (discrete.py:109-143) for priority lists over module INSTANCES: mgx_expand_lists +
 * mgx_step(normalized=0).  ONE launch -- the list walked and the control kept in registers -- where the layout holds at most two
 * modules of a kind and steps in lock-step, per-grid windows or in-place episodes (mgx_reset_episodes, restarts of
 * mgx_set_auto_reset included); two launches through `control` otherwise.  control [N, A]: optional
 * where one launch is taken (it receives the expanded control when given), REQUIRED (the buffer between the two launches) for any
 * other layout -- MGX_ERR_INVALID without it.  lists as in mgx_expand_lists; the other outputs are those of mgx_step. */
int mgx_step_lists(mgx_handle *h, const int32_t *action_id, const int32_t *lists, int32_t n_lists, int32_t list_len,
                   double *control, double *reward, uint8_t *done, void *obs, double *log, mgx_stream stream);

/* K fused DiscreteMicrogridEnv steps with the control expanded ON DEVICE: action_id holds priority-list ids as
 * bytes, either [K, N] (per_step != 0: `for a in ids: env.step(a)`, discrete.py:109-143) or [N] (per_step == 0: one
 * fixed list per grid for the whole call = RuleBasedControl.run, algos/rbc/rbc.py:64-93).  `table` as in
 * mgx_expand_discrete; outputs as in mgx_step_k.  No action stream is read at all. */
int mgx_rollout_discrete(mgx_handle *h, const uint8_t *action_id, int per_step, const int32_t *table,
                         int32_t n_actions, int32_t K, double *reward, uint8_t *done, double *soc_trace,
                         uint32_t *status_trace, double *ret_acc, double *log, mgx_stream stream);

/* Per-grid episode statistics of mgx_rollout_episodes (device arrays, each may be NULL).  They are read, updated and written
 * back, so they carry from one call to the next; the caller zeroes them when it resets.  Per step of grid i, in step order and
 * in plain fp64 (a host loop over the per-step rewards reproduces them bit for bit):
 *     ret_running[i] += reward
 *     if this step is the last one of the grid's episode (counter == ep_final[i] - 1):
 *         ret_last[i] = ret_running[i];  ret_sum[i] += ret_running[i];  episodes[i] += 1;  ret_running[i] = 0
 * A grid that is not restarted (mgx_set_auto_reset off) walks on with done = 1; it is counted once, when it crosses its end. */
typedef struct mgx_episode_stats {
    double *ret_running;   /* [N] return of the episode in progress */
    double *ret_sum;       /* [N] sum of the returns of the episodes finished so far, added in the order they finish */
    double *ret_last;      /* [N] return of the most recently finished episode */
    int32_t *episodes;     /* [N] number of episodes finished */
} mgx_episode_stats;

/* The fused discrete roll-out over per-grid IN-PLACE episodes (mgx_reset_episodes): K steps in one launch, every grid reading the
 * rows of its own episode and -- with mgx_set_auto_reset -- restarting inside the launch whenever a step ends its episode, with
 * the draw, the offsets and the start / length / t0 arrays exactly as K calls of mgx_step_discrete would leave them.  action_id /
 * per_step / table as in mgx_rollout_discrete; reward / done (bytes) / soc_trace / status_trace [K, N] and `stats` (the struct
 * pointer too) may be NULL.  No observations and no balance log are written.  The counter moves by K.
 * MGX_ERR_INVALID: the handle does not step in-place episodes.  MGX_ERR_UNSUPPORTED: several modules of a kind, shards, device-counter
 * mode, `done` as bit sets, mgx_set_final_obs set.  Nothing is launched when the call is refused.
 * An ADDITION to ABI 9 that leaves MGX_ABI_MINOR at 3: consumers find it by name (dlsym); mgx_step_k, mgx_rollout_discrete and
 * mgx_rollout_lists keep refusing handles in this mode. */
int mgx_rollout_episodes(mgx_handle *h, const uint8_t *action_id, int per_step, const int32_t *table, int32_t n_actions,
                         int32_t K, double *reward, uint8_t *done, double *soc_trace, uint32_t *status_trace,
                         const mgx_episode_stats *stats, mgx_stream stream);

/* The fused CONTINUOUS K-step over per-grid IN-PLACE episodes (mgx_reset_episodes): K consecutive Microgrid.run(control, normalized)
 * steps (microgrid.py:227-325) in one launch, every grid on the rows of its own FixedLengthStochasticTrajectory /
 * StochasticTrajectory episode (trajectory/stochastic.py) and -- with mgx_set_auto_reset -- restarting inside the launch whenever a
 * step ends its episode, with the draw, the offsets and the start / length / t0 arrays exactly as K calls of mgx_step would leave
 * them.  actions [K, N, A] in the handle's action format (mgx_set_action_format; may be NULL for a layout without a controllable
 * module, A = 0): row k belongs to step k of the call, whatever episode a grid is in.  `normalized` and the reward shaper as in
 * mgx_step.  reward / done (bytes) / soc_trace / status_trace [K, N] and `stats` (the struct pointer too; the statistics of
 * mgx_rollout_episodes, by the same rule) may be NULL.  No observations and no balance log are written.  The counter moves by K.
 * MGX_ERR_INVALID: NULL handle / actions, K <= 0, the handle does not step in-place episodes (lock-step: mgx_step_k).
 * MGX_ERR_UNSUPPORTED: several modules of a kind, shards, device-counter mode, `done` as bit sets with done != NULL,
 * mgx_set_final_obs set.  MGX_ERR_RANGE: the counter would leave its range.  Nothing is launched when the call is refused.
 * An ADDITION to ABI 9 that leaves MGX_ABI_MINOR at 3: consumers find it by name (dlsym); mgx_step_k keeps refusing handles in
 * this mode. */
int mgx_step_k_episodes(mgx_handle *h, const void *actions, int32_t K, int normalized, double *reward, uint8_t *done,
                        double *soc_trace, uint32_t *status_trace, const mgx_episode_stats *stats, mgx_stream stream);

/* The observation rows of a fused launch over in-place episodes (mgx_rollout_episodes_rows, mgx_step_k_episodes_rows): whole
 * H = 0 rows [K, N, D] in the handle's observation format (mgx_set_obs_format), D = mgx_obs_dim.  Each pointer may be NULL.
 *     obs[k, i, :]        the observation step k returned for grid i: the post-step state over the series row the grid stands on
 *                         after the step -- the first row of its new episode where the step restarted it (what `obs` of K calls
 *                         of mgx_step holds, one after the other)
 *     final_obs[k, i, :]  written ONLY where step k restarted grid i (mgx_set_auto_reset on, done[k, i] set): the row before the
 *                         restart, what mgx_set_final_obs receives from a single step.  Every other entry keeps the caller's bytes. */
typedef struct mgx_episode_rows {
    int32_t struct_size;   /* = sizeof(mgx_episode_rows) */
    int32_t reserved;
    void *obs;             /* [K, N, D] in the handle's observation format, or NULL */
    void *final_obs;       /* [K, N, D], written only where a grid restarts at step k, or NULL */
} mgx_episode_rows;

/* mgx_rollout_episodes + the observation every step returned (MicrogridEnv.step's observation, envs/base/base.py:169-209) and the
 * last observation of every episode that ends inside the launch, before the restart replaces it with the reset observation
 * (Microgrid.reset, microgrid.py:205-225): one launch of a kernel of its own (rollout_episodes_rows_kernel).  Every argument but
 * `rows` as in mgx_rollout_episodes, everything that call leaves (state, counter, episode arrays, statistics, the [K, N] outputs)
 * is left bit for bit the same; a row equals the row of the single step bit for bit.  rows == NULL, or both of its pointers NULL:
 * the call IS mgx_rollout_episodes (forwarded; the rows kernel is not launched).
 * MGX_ERR_INVALID: NULL handle, rows->struct_size != sizeof(mgx_episode_rows), and what mgx_rollout_episodes refuses so.
 * MGX_ERR_UNSUPPORTED: a forecast horizon (H != 0), an observation mode other than whole rows (mgx_set_obs_mode), mgx_set_final_obs
 * set (its per-step [N, D] buffer has no meaning across K steps), and what mgx_rollout_episodes refuses so.  MGX_ERR_RANGE as
 * mgx_rollout_episodes.  Nothing is launched when the call is refused.
 * An ADDITION to ABI 9 that leaves MGX_ABI_MINOR at 3: consumers find it by name (dlsym). */
int mgx_rollout_episodes_rows(mgx_handle *h, const uint8_t *action_id, int per_step, const int32_t *table, int32_t n_actions,
                              int32_t K, double *reward, uint8_t *done, double *soc_trace, uint32_t *status_trace,
                              const mgx_episode_stats *stats, const mgx_episode_rows *rows, mgx_stream stream);

/* mgx_step_k_episodes + the observation every step returned (MicrogridEnv.step's observation, envs/base/base.py:169-209) and the
 * last observation of every episode that ends inside the launch (before Microgrid.reset, microgrid.py:205-225, replaces it): one
 * launch of step_k_episodes_rows_kernel.  Every argument but `rows` as in mgx_step_k_episodes; forwarding, results and refusals
 * by the rules of mgx_rollout_episodes_rows, with mgx_step_k_episodes in the place of mgx_rollout_episodes.
 * An ADDITION to ABI 9 that leaves MGX_ABI_MINOR at 3: consumers find it by name (dlsym). */
int mgx_step_k_episodes_rows(mgx_handle *h, const void *actions, int32_t K, int normalized, double *reward, uint8_t *done,
                             double *soc_trace, uint32_t *status_trace, const mgx_episode_stats *stats,
                             const mgx_episode_rows *rows, mgx_stream stream);

/* CLOSED-LOOP fused launches over in-place episodes: the control of every step is chosen inside the launch, by a policy applied to
 * the observation the grid's last step (or reset) returned -- the loop `a = policy(obs); obs, r, done, _ = env.step(a)` K times in
 * one launch.
 *
 * The policy is a small float64 network of plain IEEE operations (separate multiplies and adds, fixed order), so that a host loop
 * over the returned observations reproduces every decision bit for bit.  x[0 .. n_in) is the grid's H = 0 observation row AS THE
 * HANDLE'S OBSERVATION FORMAT HOLDS IT (mgx_set_obs_format float32: the float value widened back to double).
 *     hidden layer (n_hidden > 0):  hid[u] = b1[u]; for j = 0 .. n_in - 1 in order: hid[u] = hid[u] + w1[u, j] * x[j];
 *                                   then hid[u] = hid[u] > 0 ? hid[u] : 0.0 (NaN and -0.0 become +0.0)
 *     output layer:                 y[o] = b2[o]; for j in order: y[o] = y[o] + w2[o, j] * v[j], v = hid (n_hidden > 0) or x
 *     discrete head (mgx_rollout_policy_episodes):  best = -inf, id = 0; for o = 0 .. n_out - 1: if y[o] > best: best = y[o], id = o
 *                                   -- ties go to the lowest index, a NaN never wins, all-NaN is id 0
 *     continuous head (mgx_step_k_policy_episodes): u[o] = !(y[o] > 0) ? 0.0 : (y[o] > 1 ? 1.0 : y[o]) -- normalised controls in
 *                                   the order of the action columns (mgx_step with normalized = 1)
 * n_policies >= 1 parameter sets are stacked along a leading axis; policy_index[i] names the set of grid i (NULL: set 0 for every
 * grid; an index outside [0, n_policies): set 0).  All arrays are float64 device arrays, C order. */
#define MGX_POLICY_MAX_HIDDEN 64        /* n_hidden of a policy, at most */
#define MGX_POLICY_LDS_BYTES 32768      /* the staged parameter sets of a launch, at most.  A launch stages
                                         *     n_policies * 8 * even(m + (n_hidden ? n_hidden * (n_in + 1 + m) : n_in * m)) bytes,
                                         * m = n_out (the discrete call: n_out rounded up to a multiple of 4), even(v) = v rounded
                                         * up to an even number */
typedef struct mgx_policy {
    int32_t struct_size;         /* = sizeof(mgx_policy) */
    int32_t n_policies;          /* P >= 1 */
    int32_t n_in;                /* = mgx_obs_dim of the handle (an H = 0 row: at most 12) */
    int32_t n_hidden;            /* 0: a linear policy on x; at most MGX_POLICY_MAX_HIDDEN */
    int32_t n_out;               /* discrete: the table's n_actions (at most 12); continuous: mgx_action_dim (at most 4) */
    int32_t reserved;
    const double *w1;            /* [P, n_hidden, n_in]; not read when n_hidden = 0 */
    const double *b1;            /* [P, n_hidden]; not read when n_hidden = 0 */
    const double *w2;            /* [P, n_out, n_hidden ? n_hidden : n_in] */
    const double *b2;            /* [P, n_out] */
    const int32_t *policy_index; /* [N], or NULL */
} mgx_policy;

/* K discrete steps in one launch of rollout_policy_episodes_kernel, the priority-list id of step k being the discrete head of
 * `policy` on the row the grid stands on before the step (after a restart inside the launch: the first row of the new episode).
 * Everything else is what K calls of mgx_step_discrete with those ids leave: state, counter, the episode arrays, the draws of
 * mgx_set_auto_reset, the statistics by the rule of mgx_episode_stats, rows->obs / rows->final_obs by the rule of mgx_episode_rows
 * (rows may be NULL).  action_id_out: uint8 [K, N], the ids taken, or NULL.  `table`, `n_actions` as in mgx_rollout_episodes.
 * Refused -- nothing is launched -- as mgx_rollout_episodes_rows refuses, with the same codes; a forecast horizon, a state-only
 * observation mode and a set mgx_set_final_obs whether or not `rows` is given (the policy reads whole H = 0 rows).  On top:
 * MGX_ERR_INVALID: NULL policy / table, policy->struct_size != sizeof(mgx_policy), n_policies < 1, n_in != mgx_obs_dim,
 * n_out != n_actions, n_hidden < 0, NULL weights.  MGX_ERR_UNSUPPORTED: n_hidden > MGX_POLICY_MAX_HIDDEN, parameter sets beyond
 * MGX_POLICY_LDS_BYTES (the message names the size).
 * An ADDITION to ABI 9 that leaves MGX_ABI_MINOR at 3: consumers find it by name (dlsym). */
int mgx_rollout_policy_episodes(mgx_handle *h, const mgx_policy *policy, const int32_t *table, int32_t n_actions, int32_t K,
                                double *reward, uint8_t *done, double *soc_trace, uint32_t *status_trace, uint8_t *action_id_out,
                                const mgx_episode_stats *stats, const mgx_episode_rows *rows, mgx_stream stream);

/* The continuous twin (step_k_policy_episodes_kernel): the controls of step k are the continuous head of `policy`, stepped as
 * mgx_step(..., normalized = 1) steps them.  actions_out: double [K, N, A], the controls taken, or NULL.  Refusals as above with
 * mgx_step_k_episodes_rows in the place of mgx_rollout_episodes_rows and n_out != mgx_action_dim; MGX_ERR_UNSUPPORTED also on a
 * handle whose action format is float32 (mgx_set_action_format): the controls are formed and written as doubles.
 * An ADDITION to ABI 9 that leaves MGX_ABI_MINOR at 3: consumers find it by name (dlsym). */
int mgx_step_k_policy_episodes(mgx_handle *h, const mgx_policy *policy, int32_t K, double *reward, uint8_t *done,
                               double *soc_trace, uint32_t *status_trace, double *actions_out, const mgx_episode_stats *stats,
                               const mgx_episode_rows *rows, mgx_stream stream);

/* EXPLORATION inside the closed-loop launches: epsilon-greedy on the discrete head, additive noise on the continuous head, drawn
 * on the device from a counter-based generator -- a draw is a function of (seed, grid, step counter, number) alone, so a host loop
 * reproduces it bit for bit and it does not depend on how a roll-out is cut into launches.  THE RULE (stated here once):
 *
 * Draw of grid i at step counter t, number j:  t is the handle's shared counter BEFORE the step (mgx_current_step; step k of a
 * launch: its value at the call + k), i the grid index the restart draws of mgx_set_auto_reset use.
 *     r[0 .. 3] = Philox4x32-10(counter words (lo32(i), hi32(i), (uint32)t, 0xE9100000u + j); key (lo32(seed), hi32(seed)))
 * (the fourth counter word of the series and episode draws is 0x5eed: an exploration seed equal to the auto-reset seed still has a
 * stream of its own).  U(a, b) = (double)(((uint64)a << 21) ^ (b >> 11)) * 2^-53, in [0, 1): the 53-bit value of every other
 * uniform draw here.
 *
 * Discrete head: ONE draw, j = 0.  u1 = U(r[0], r[1]), u2 = U(r[2], r[3]); e = scale ? epsilon * scale[i] : epsilon;
 *     if u1 < e:  id = min((int)floor(u2 * (double)n_out), n_out - 1)     (n_out: policy->n_out, the table's rows)
 *     else:       id = the greedy head of mgx_policy, unchanged
 * Continuous head: one draw per action column o, j = o.  S = the integer sum of the twelve 10-bit fields at bits [0, 10), [10, 20),
 * [20, 30) of each of the four words; z = ((double)S - 6138.0) * (1.0 / 1024.0) -- the classical twelve-uniform normal quantised
 * at 2^-10: mean 0, standard deviation 0.9999995, support [-6138 / 1024, 6138 / 1024] (within +-6); s = scale ? sigma[o] * scale[i] : sigma[o];
 *     v = y[o] + s * z    (a separate multiply and add);   u[o] = !(v > 0) ? 0.0 : (v > 1 ? 1.0 : v)
 * With epsilon == 0, or every sigma == 0, the results are those of the calls without exploration, bit for bit. */
typedef struct mgx_exploration {
    int32_t struct_size;      /* = sizeof(mgx_exploration) */
    int32_t reserved;
    uint64_t seed;            /* Philox key */
    double epsilon;           /* discrete head, in [0, 1] */
    double sigma[4];          /* continuous head, one per action column, >= 0; entries beyond mgx_action_dim not read */
    const double *scale;      /* device [N] or NULL (= 1.0 for every grid): multiplies epsilon and every sigma of grid i */
} mgx_exploration;

/* mgx_rollout_policy_episodes with the discrete head exploring by the rule of mgx_exploration: one launch of
 * rollout_policy_head_episodes_kernel (exploring head).  action_id_out receives the ids taken, explored ones included.  explore == NULL: the call
 * IS mgx_rollout_policy_episodes (forwarded).  Every other argument, result and refusal as there; on top MGX_ERR_INVALID for
 * explore->struct_size != sizeof(mgx_exploration), an epsilon outside [0, 1] or NaN, a negative or NaN sigma[o] for
 * o < mgx_action_dim (both calls check the whole struct, whichever head they run).
 * An ADDITION to ABI 9 that leaves MGX_ABI_MINOR at 3: consumers find it by name (dlsym). */
int mgx_rollout_policy_explore_episodes(mgx_handle *h, const mgx_policy *policy, const mgx_exploration *explore, const int32_t *table,
                                        int32_t n_actions, int32_t K, double *reward, uint8_t *done, double *soc_trace,
                                        uint32_t *status_trace, uint8_t *action_id_out, const mgx_episode_stats *stats,
                                        const mgx_episode_rows *rows, mgx_stream stream);

/* The continuous twin (step_k_policy_head_episodes_kernel, exploring head): mgx_step_k_policy_episodes with the noise of mgx_exploration on
 * every control before its clip.  actions_out receives the controls taken.  explore == NULL: the call IS
 * mgx_step_k_policy_episodes.  On top of its refusals MGX_ERR_INVALID as mgx_rollout_policy_explore_episodes refuses a mgx_exploration.
 * An ADDITION to ABI 9 that leaves MGX_ABI_MINOR at 3: consumers find it by name (dlsym). */
int mgx_step_k_policy_explore_episodes(mgx_handle *h, const mgx_policy *policy, const mgx_exploration *explore, int32_t K,
                                       double *reward, uint8_t *done, double *soc_trace, uint32_t *status_trace, double *actions_out,
                                       const mgx_episode_stats *stats, const mgx_episode_rows *rows, mgx_stream stream);

/* SAMPLING inside the closed-loop discrete launch: the id of every step is drawn from the policy's own categorical distribution,
 * softmax(y / tau), and the launch returns the probability of the id taken -- what the on-policy methods (REINFORCE, A2C, PPO)
 * need; the caller takes the logarithm.  exp is PART OF THE RULE, a fixed sequence of plain IEEE fp64 operations, not a call into
 * a math library: host and device evaluate the same operations, so fused == stepped stays bit for bit.  THE RULE (stated here once):
 *
 * E(d), for -708 <= d <= 0   (every multiply and add separate):
 *     k = floor(d * 1.4426950408889634 + 0.5)
 *     r = (d - k * 6.93147180369123816490e-01) - k * 1.90821492927058770002e-10
 *     p = c[13];  for n = 12 .. 0:  p = p * r + c[n]        c[n]: the double nearest 1/n! --
 *         c[0 .. 13] = 1.0, 1.0, 0.5, 0.16666666666666666, 0.041666666666666664, 0.008333333333333333, 0.001388888888888889,
 *                      0.0001984126984126984, 2.48015873015873e-05, 2.7557319223985893e-06, 2.755731922398589e-07,
 *                      2.505210838544172e-08, 2.08767569878681e-09, 1.6059043836821613e-10
 *     E = p * 2^k       (2^k built from its bits, (uint64)(k + 1023) << 52: a normal number, since k >= -1021)
 * E stays below 1 ulp of exp(d), is monotone, never exceeds 1.0 and E(+-0.0) == 1.0.
 *
 * Sampling head of grid i at step counter t (i, t, the draw and U(a, b) as mgx_exploration states them), on y[0 .. n_out) of mgx_policy:
 *     best, g = the greedy head of mgx_policy, unchanged (strict >, from -inf, the lowest index wins, a NaN never wins)
 *     tau  = scale ? temperature * scale[i] : temperature
 *     if !(tau > 0):  id = g, prob = 1.0, and no draw is made      (temperature 0 or scale[i] == 0: the greedy launch, bit for bit)
 *     beta = 1.0 / tau
 *     for o = 0 .. n_out - 1:  d = (y[o] - best) * beta;  e[o] = (o == g) ? 1.0 : (d >= -708.0 ? E(d) : 0.0)
 *         (a NaN d gives 0; e[g] is 1.0 by definition, so S >= 1 whatever the logits hold)
 *     S = 0.0;  for o in order:  S = S + e[o]
 *     r[0 .. 3] = the draw of (seed, i, t) with number j = 1  (0xE9100000u + 1; the epsilon-greedy draw is j = 0)
 *     u = U(r[0], r[1]);  v = u * S
 *     c = 0.0;  id = g;  for o in order:  c = c + e[o];  the FIRST o with v < c becomes id
 *         (an id with e[o] == 0 can never be taken; if rounding leaves none, id stays g)
 *     prob = e[id] / S
 * At the corners: best = +-inf or all-NaN logits leave e[g] = 1.0 as the only weight (every other d is NaN or -inf), so id = g and
 * prob = 1.0 / S = 1.0; ties at the maximum share the mass, because E(+-0.0) == 1.0. */
typedef struct mgx_sampling {
    int32_t struct_size;      /* = sizeof(mgx_sampling) */
    int32_t reserved;
    uint64_t seed;            /* Philox key */
    double temperature;       /* tau >= 0, finite; 0: the greedy head */
    const double *scale;      /* device [N] or NULL (= 1.0 for every grid): multiplies the temperature of grid i */
} mgx_sampling;

/* mgx_rollout_policy_episodes with the discrete head sampling by the rule of mgx_sampling: one launch of
 * rollout_policy_head_episodes_kernel (sampling head).  action_id_out receives the ids taken; prob_out: double [K, N], the probability of the id
 * taken at every step, or NULL.  Every other argument, result and refusal as mgx_rollout_policy_episodes; on top MGX_ERR_INVALID for
 * a NULL sampling, sampling->struct_size != sizeof(mgx_sampling), a negative, infinite or NaN temperature.
 * An ADDITION to ABI 9 that leaves MGX_ABI_MINOR at 3: consumers find it by name (dlsym). */
int mgx_rollout_policy_sample_episodes(mgx_handle *h, const mgx_policy *policy, const mgx_sampling *sampling, const int32_t *table,
                                       int32_t n_actions, int32_t K, double *reward, uint8_t *done, double *soc_trace,
                                       uint32_t *status_trace, uint8_t *action_id_out, double *prob_out,
                                       const mgx_episode_stats *stats, const mgx_episode_rows *rows, mgx_stream stream);

/* A CRITIC beside the actor of the sampling launch: a value head on the trunk of a mgx_policy -- what A2C and PPO need of a
 * collector on top of the ids and their probabilities.  THE RULE (stated here once), with n_mid = n_hidden ? n_hidden : n_in of
 * the policy it goes with, v the policy's hidden vector after its ReLU (n_hidden > 0) or x (n_hidden = 0), ps the grid's
 * parameter set by mgx_policy's own rule (policy_index, an index outside [0, n_policies): set 0):
 *     V(x) = b[ps];  for j = 0 .. n_mid - 1 in order:  V = V + w[ps, j] * v[j]          (multiply and add separate)
 * x is the H = 0 observation row as the handle's observation format holds it (a float32 row widened back): V is exactly one more
 * output row of the same network. */
typedef struct mgx_critic {
    int32_t struct_size;      /* = sizeof(mgx_critic) */
    int32_t reserved;
    const double *w;          /* device [P, n_mid] */
    const double *b;          /* device [P] */
} mgx_critic;

/* mgx_rollout_policy_sample_episodes with a critic: one launch of rollout_policy_head_episodes_kernel (sampling head with a critic).  Each of the three
 * outputs may be NULL:
 *   value_out        double [K, N]: V of the row the id of step k was chosen on (the row the policy reads at step k; after a
 *                    restart inside the launch the first row of the new episode)
 *   final_value_out  double [K, N]: V of the row mgx_episode_rows.final_obs[k, i, :] holds, written ONLY where step k restarted
 *                    grid i -- every other entry keeps the caller's bytes (final_obs's rule), whether or not rows->final_obs is
 *                    given.  Episodes end by their length, a time limit: the target at `done` bootstraps from this value
 *   last_value_out   double [N]: V of the row the last step returned (obs[K - 1, i, :]), the bootstrap of a roll-out cut here
 * Everything else the call leaves -- state, counter, episode arrays, draws, statistics, ids, probabilities, traces, rows -- is bit
 * for bit what mgx_rollout_policy_sample_episodes leaves with the same policy and sampling: the critic changes no decision, and
 * temperature == 0 stays the greedy head.  Refusals as the sampling call's; on top MGX_ERR_INVALID for a NULL critic,
 * critic->struct_size != sizeof(mgx_critic), a NULL w or b, and MGX_ERR_UNSUPPORTED where the staged sets pass
 * MGX_POLICY_LDS_BYTES: the critic adds 1 + n_mid doubles to a set, the launch stages
 *     n_policies * 8 * even(m + 1 + (n_hidden ? n_hidden * (n_in + 2 + m) : n_in * (m + 1))) bytes,   m = n_out rounded up to a
 * multiple of 4 (MGX_POLICY_LDS_BYTES states the formula without a critic).  Nothing is launched when the call is refused.
 * An ADDITION to ABI 9 that leaves MGX_ABI_MINOR at 3: consumers find it by name (dlsym). */
int mgx_rollout_policy_critic_episodes(mgx_handle *h, const mgx_policy *policy, const mgx_sampling *sampling, const mgx_critic *critic,
                                       const int32_t *table, int32_t n_actions, int32_t K, double *reward, uint8_t *done,
                                       double *soc_trace, uint32_t *status_trace, uint8_t *action_id_out, double *prob_out,
                                       double *value_out, double *final_value_out, double *last_value_out,
                                       const mgx_episode_stats *stats, const mgx_episode_rows *rows, mgx_stream stream);

/* Generalised advantage estimation over the [K, N] outputs of such a launch, handle-free on the current device (as
 * mgx_generate_columns): one launch of gae_kernel, one lane per grid walking k backwards.  reward, value, advantage, returns:
 * double [K, N]; done: uint8 [K, N] in the byte form the launches write; final_value: double [K, N] or NULL (read only where done);
 * last_value: double [N]; returns may be NULL.  THE RULE (stated here once; multiply and add separate):
 *     c = gamma * lambda                       (one multiply, done once on the host)
 *     per grid i:  next = last_value[i];  carry = 0.0
 *     for k = K - 1 down to 0:
 *         d     = done[k, i] != 0
 *         nv    = d ? (final_value ? final_value[k, i] : 0.0) : next
 *         delta = (reward[k, i] + gamma * nv) - value[k, i]
 *         A     = d ? delta : delta + c * carry        (a select: a NaN carry does not cross an episode boundary)
 *         advantage[k, i] = A;  returns[k, i] = A + value[k, i]
 *         carry = A;  next = value[k, i]
 * MGX_ERR_INVALID: N <= 0, K <= 0, a NULL reward / done / value / last_value / advantage, gamma or lambda outside [0, 1] or NaN.
 * Outputs must not overlap inputs (not checked).  An ADDITION to ABI 9 that leaves MGX_ABI_MINOR at 3. */
int mgx_gae(int64_t N, int32_t K, const double *reward, const uint8_t *done, const double *value, const double *final_value,
            const double *last_value, double gamma, double lambda, double *advantage, double *returns, mgx_stream stream);

/* THE GRADIENT of the PPO-clip / A2C loss with respect to the parameters of a discrete mgx_policy and the mgx_critic on its trunk,
 * from what the sampling launch returned (rows, ids, probabilities) and mgx_gae made of it (advantages, returns); handle-free on the
 * current device (as mgx_gae).  The forward pass is the launch's own sequence of operations, so on an un-updated policy the
 * probability ratio is exactly 1.0.  K * N samples s = (k, i); x = x[k, i, :] (float64, or float32 widened to double as mgx_policy
 * widens a float32 row).  mask: uint8 [K, N] or NULL; a sample with mask 0 contributes nothing (a minibatch, an excluded sample);
 * M is the number of live samples, counted on the device as an integer.  THE RULE (stated here once; every multiply and add
 * separate, sums in index order):
 *     forward:    y[0 .. n_out), V by mgx_policy and mgx_critic; h[u] the hidden vector after its ReLU (n_hidden = 0: h = x)
 *                 best, g, tau = scale ? temperature * scale[i] : temperature, beta, e[o], S exactly as mgx_sampling states them;
 *                 d[o] = (y[o] - best) * beta, d[g] = 0.0 (as e[g] is 1.0 by definition)
 *                 pi[o] = e[o] / S;  a = action_id[s];  rho = pi[a] / old_prob[s]
 *                 where !(tau > 0) (the greedy head): rho = 1.0 / old_prob[s], and the policy and entropy terms of the sample --
 *                 c, dy, its policy loss, entropy and clipped flag -- are zero; the value term stays
 *     surrogate:  A = advantage[s];  active = !((A > 0 && rho > hi) || (A < 0 && rho < lo)),  hi = 1.0 + clip_eps, lo = 1.0 - clip_eps
 *                 (formed once on the host; clip_eps = +inf never gates: A2C, the unclipped surrogate)
 *                 c = active ? -(A * rho) : 0.0;   the sample's policy loss: active ? c : -(A * (A > 0 ? hi : lo))
 *     entropy:    lnS = L(S), the L of mgx_gaussian;  logpi[o] = d[o] - lnS
 *                 Hs = 0.0; for o in order, where e[o] > 0:  Hs = Hs + pi[o] * logpi[o];   H = -Hs
 *     logits:     dy[o] = beta * (c * ((o == a ? 1.0 : 0.0) - pi[o]) + ent_coef * t[o]),  t[o] = e[o] > 0 ? pi[o] * (logpi[o] + H) : 0.0
 *     value:      diff = V - returns[s];  dv = vf_coef * diff;  the sample's value loss: 0.5 * (diff * diff)    (no critic: dv = 0)
 *     trunk:      per hidden unit u:  q = 0.0; for o in order: q = q + w2[o, u] * dy[o];  with a critic: q = q + cw[u] * dv;
 *                 dh[u] = h[u] > 0 ? q : 0.0
 *     per-sample terms:  dy[o] * h[u] -> g_w2[o, u];  dy[o] -> g_b2[o];  dv * h[u] -> g_cw[u];  dv -> g_cb;
 *                        dh[u] * x[j] -> g_w1[u, j];  dh[u] -> g_b1[u]         (n_hidden = 0: x in the place of h, no g_w1 / g_b1)
 *     result:     every output = (1.0 / M) * (the sum of its term over the live samples);  M = 0 gives zeros
 *     stats[0 .. 3] = the means over the live samples of policy loss, value loss, entropy H and the clipped flag (!active)
 *     ratio_out[s] = rho on the live samples; masked samples keep the caller's bytes
 * The loss these are the gradient of: mean(policy loss) + vf_coef * mean(value loss) - ent_coef * mean(H).
 * THE SUMS over the samples go through the matrix cores (v_mfma_f64_16x16x4_f64, four samples per instruction) and then over waves
 * and workgroups in a fixed order: the result is the same from run to run, but the ORDER of the sum is the kernel's, and how the
 * fp64 MFMA rounds its inner sum of four products is not documented -- so a sum over many samples is within the any-order bound
 * (M + 2) * 2^-53 * sum_s |term_s| / M of the exact one, not bit for bit a host loop's.  One live sample is exact: a product added
 * to zeros.  How the MFMA treats subnormal products is not known either: keep the terms normal numbers.  No atomics are used. */
struct mgx_policy_grad {
    int32_t struct_size;      /* = sizeof(struct mgx_policy_grad) */
    int32_t x_f32;            /* 0: x is float64; 1: float32 */
    const void    *x;         /* [K, N, n_in]: the row decision (k, i) was taken on */
    const uint8_t *action_id; /* [K, N] */
    const double  *old_prob;  /* [K, N] */
    const double  *advantage; /* [K, N] */
    const double  *returns;   /* [K, N]; NULL without a critic */
    const uint8_t *mask;      /* [K, N] or NULL */
    double clip_eps;          /* >= 0; +inf: no clipping */
    double vf_coef, ent_coef;
    double *g_w1, *g_b1;      /* [n_hidden, n_in], [n_hidden]; each output may be NULL */
    double *g_w2, *g_b2;      /* [n_out, n_mid], [n_out] */
    double *g_cw, *g_cb;      /* [n_mid], [1]; NULL without a critic */
    double *stats;            /* [4] */
    double *ratio_out;        /* [K, N] */
    void   *workspace;        /* the per-workgroup partials: mgx_policy_grad_workspace bytes, at least; 8-byte aligned */
    int64_t workspace_bytes;
};                            /* (a struct tag without a typedef: the call below bears the same name) */

/* The bytes of workspace a call with these shapes needs.  Refusals as mgx_policy_grad refuses N, K and the policy; NULL bytes. */
int mgx_policy_grad_workspace(int64_t N, int32_t K, const mgx_policy *policy, int64_t *bytes);

/* Two launches: policy_grad_kernel (a lane per sample, a wave 64 grids and a chunk of k) and policy_grad_finish_kernel (the
 * partials in a fixed order, times 1 / M, into the caller's arrays).  Of `sampling` only temperature and scale are read: no draw is
 * made.  critic may be NULL: no value term, and returns, g_cw and g_cb must then be NULL.  Nothing is launched when the call is refused:
 * MGX_ERR_INVALID: a NULL pg / policy / sampling / x / action_id / old_prob / advantage, a wrong struct_size (pg, policy, sampling,
 * critic), N or K below 1, n_in or n_out outside 1 .. 12, NULL weights, a negative, infinite or NaN temperature, a negative or NaN
 * clip_eps, a NaN coefficient, x_f32 other than 0 or 1, returns, g_cw or g_cb without a critic, NULL returns with one, a NULL or too
 * small workspace.  MGX_ERR_UNSUPPORTED: n_policies > 1 or a policy_index (the gradient of a population is not offered),
 * n_hidden > MGX_POLICY_MAX_HIDDEN.  An ADDITION to ABI 9 that leaves MGX_ABI_MINOR at 3: found by name (dlsym). */
int mgx_policy_grad(int64_t N, int32_t K, const mgx_policy *policy, const mgx_critic *critic, const mgx_sampling *sampling,
                    const struct mgx_policy_grad *pg, mgx_stream stream);

/* A GAUSSIAN policy head inside the closed-loop continuous launch: every control is drawn from N(y[o], s[o]^2) -- a true normal
 * draw, not the lattice of mgx_exploration -- and the launch returns the pre-clip action and its exact log-density, what the
 * on-policy methods need on the continuous head.  As exp in mgx_sampling, log, sine and cosine are PART OF THE RULE: fixed sequences
 * of plain IEEE fp64 operations (every multiply and add separate), no call into a math library, so fused == stepped stays bit for
 * bit.  The division is the correctly rounded IEEE one on both sides.  The SQUARE ROOT is a fixed sequence too, S below: with the
 * library roots the device/host parity test passed on L and on the quarter turn and failed on the pair.  THE RULE (stated here once):
 *
 * L(a), for a positive NORMAL double a (within 4 ulp of log(a); L(1.0) == 0.0 exactly):
 *     e = the unbiased exponent of a, m = its mantissa as a double in [1, 2)     (both out of the bits of a)
 *     if m > 1.4142135623730951:  m = m * 0.5,  e = e + 1
 *     t = (m - 1.0) / (m + 1.0);  w = t * t
 *     p = c[10];  for n = 9 .. 0:  p = p * w + c[n]        c[n]: the double nearest 2 / (2n + 1) --
 *         c[0 .. 10] = 2.0, 0.6666666666666666, 0.4, 0.2857142857142857, 0.2222222222222222, 0.18181818181818182,
 *                      0.15384615384615385, 0.13333333333333333, 0.11764705882352941, 0.10526315789473684, 0.09523809523809523
 *     L = e * 6.93147180369123816490e-01 + (e * 1.90821492927058770002e-10 + t * p)      (e as a double; the ln 2 constants of E)
 *
 * Quarter turn: (sin, cos) of the angle f * pi / 2, for f an exact multiple of 2^-52 in [0, 1) (within 2^-51 of sin and cos):
 *     hi = f > 0.5;  g = hi ? 1.0 - f : f        (exact)
 *     x = g * 1.5707963267948966;  w = x * x
 *     q = a[6];  for n = 5 .. 0:  q = q * w + a[n];   s = x * (q * w + 1.0)       a[n]: the double nearest (-1)^(n+1) / (2n + 3)! --
 *         a[0 .. 6] = -0.16666666666666666, 0.008333333333333333, -0.0001984126984126984, 2.7557319223985893e-06,
 *                     -2.505210838544172e-08, 1.6059043836821613e-10, -7.647163731819816e-13
 *     c = b[7];  for n = 6 .. 0:  c = c * w + b[n];   c = c * w + 1.0             b[n]: the double nearest (-1)^(n+1) / (2n + 2)! --
 *         b[0 .. 7] = -0.5, 0.041666666666666664, -0.001388888888888889, 2.48015873015873e-05, -2.755731922398589e-07,
 *                     2.08767569878681e-09, -1.1470745597729725e-11, 4.779477332387385e-14
 *     (sin, cos) = hi ? (c, s) : (s, c)
 *
 * S(v), for a finite double v (within 1 ulp of sqrt(v) for v > 0; multiplies and adds only):
 *     if !(v > 0):  S = 0.0                       (v = -2.0 * L(1.0) is -0.0)
 *     y = the double whose bits are 0x5FE6EB50C7B537A9 - (bits(v) >> 1)          (1 / sqrt(v) within 3.5 %)
 *     h = 0.5 * v;  four times:  y = y * (1.5 - (h * y) * y)
 *     r = v * y;  S = r + (0.5 * y) * (v - r * r)
 *
 * Normal pair number p of grid i at step counter t (i, t, the draw and U(a, b) as mgx_exploration states them): ONE draw,
 * r[0 .. 3] = the draw of (seed, i, t) with number j = 8 + p (numbers 0 .. 3 are the exploring head's, 1 the softmax head's):
 *     u1 = 1.0 - U(r[0], r[1])                   (exact, in (0, 1])
 *     R  = S(-2.0 * L(u1))                       (at most 8.58)
 *     a64 = (uint64)r[2] << 32 | r[3];  q = a64 >> 62;  f = (double)((a64 >> 10) & (2^52 - 1)) * 2^-52
 *     (s, c) = the quarter turn of f, turned by the quadrant:
 *         q = 0: (sn, cs) = (s, c);   q = 1: (c, -s);   q = 2: (-s, -c);   q = 3: (-c, s)
 *     z[2p] = R * cs;  z[2p + 1] = R * sn
 * Pair 0 serves action columns 0 and 1, pair 1 columns 2 and 3; a pair whose second column does not exist (mgx_action_dim 1 or 3)
 * drops its sine.
 *
 * Head of grid i, on y[0 .. n_out) of mgx_policy:
 *     s[o] = scale ? sigma[o] * scale[i] : sigma[o];   column o is LIVE if s[o] > 0   (false for a NaN)
 *     raw[o] = live ? y[o] + s[o] * z[o] : y[o]        (a separate multiply and add)
 *     u[o] = !(raw[o] > 0) ? 0.0 : (raw[o] > 1 ? 1.0 : raw[o])                         (the clip of mgx_policy, unchanged)
 * The draw of a pair without a live column is not made.  With every sigma == 0 (or scale[i] == 0) the controls are those of
 * mgx_step_k_policy_episodes, bit for bit.  A scale[i] must leave a live s[o] a normal finite number: L reads exponent and mantissa.
 *
 * Log-probability, of the PRE-CLIP action raw (as PPO implementations take it where the environment clips):
 *     C = 0.0;  for each live o in order:  C = C + (L(s[o]) + 0.9189385332046727)      (log(2 pi) / 2; once per grid and launch)
 *     Q = 0.0;  for each live o in order:  Q = Q + z[o] * z[o]
 *     logp = (-0.5 * Q) - C
 * NaN logits give raw = NaN, the control 0.0 and a finite logp (it depends on z and s alone). */
typedef struct mgx_gaussian {
    int32_t struct_size;      /* = sizeof(mgx_gaussian) */
    int32_t reserved;
    uint64_t seed;            /* Philox key */
    double sigma[4];          /* one per action column: 0 (the column stays greedy) or a positive, finite, normal number */
    const double *scale;      /* device [N] or NULL (= 1.0 for every grid): multiplies every sigma of grid i */
} mgx_gaussian;

/* mgx_step_k_policy_episodes with the Gaussian head of mgx_gaussian, and with `critic` the value head of mgx_critic: one launch of
 * step_k_policy_head_episodes_kernel (Gaussian head).  actions_out: double [K, N, A], the clipped controls taken; raw_actions_out: double
 * [K, N, A], the pre-clip actions raw; logp_out: double [K, N], their log-probability; each may be NULL.  critic == NULL: no values
 * -- value_out, final_value_out and last_value_out must then be NULL.  With a critic the three follow
 * mgx_rollout_policy_critic_episodes word for word (each may be NULL; untouched entries of final_value_out keep the caller's
 * bytes), and every other result is bit for bit what the call without a critic leaves.  Refusals as
 * mgx_step_k_policy_explore_episodes; on top MGX_ERR_INVALID for a NULL gaussian, gaussian->struct_size != sizeof(mgx_gaussian), a
 * sigma[o] (all four are checked) that is negative, NaN, infinite or positive and subnormal, a value output given without a
 * critic, and a mgx_critic as mgx_rollout_policy_critic_episodes refuses it; MGX_ERR_UNSUPPORTED where the staged sets -- with a
 * critic n_policies * 8 * even(m + 1 + (n_hidden ? n_hidden * (n_in + 2 + m) : n_in * (m + 1))) bytes, m = n_out -- pass
 * MGX_POLICY_LDS_BYTES.  What needs no handle (the structs, the value outputs) is checked first.  Nothing is launched when the call
 * is refused.  An ADDITION to ABI 9 that leaves MGX_ABI_MINOR at 3: consumers find it by name (dlsym). */
int mgx_step_k_policy_gaussian_episodes(mgx_handle *h, const mgx_policy *policy, const mgx_gaussian *gaussian,
                                        const mgx_critic *critic, int32_t K, double *reward, uint8_t *done, double *soc_trace,
                                        uint32_t *status_trace, double *actions_out, double *raw_actions_out, double *logp_out,
                                        double *value_out, double *final_value_out, double *last_value_out,
                                        const mgx_episode_stats *stats, const mgx_episode_rows *rows, mgx_stream stream);

/* THE GRADIENT of the same loss for the GAUSSIAN head of the continuous policy (mgx_gaussian, stated above): with respect to the
 * parameters of a continuous mgx_policy, the mgx_critic on its trunk and log sigma, from what mgx_step_k_policy_gaussian_episodes
 * returned (rows, the pre-clip actions raw, their log-density) and mgx_gae made of it; handle-free on the current device.  Samples,
 * x, mask and M as in mgx_policy_grad.  THE RULE (stated here once; every multiply and add separate, sums in index order; L of
 * mgx_gaussian, E of mgx_sampling; A = n_out = the action dim, 1 .. 4):
 *     forward:    y[0 .. A), V, h[u] by mgx_policy / mgx_critic on x = x[k, i, :]
 *                 s[o] = scale ? sigma[o] * scale[i] : sigma[o];  column o is LIVE iff s[o] > 0           (mgx_gaussian)
 *                 C = mgx_gaussian's log-probability constant: the sum over the live o of L(s[o]) + 0.9189385332046727
 *     density:    zeta[o] = (raw[k, i, o] - y[o]) / s[o]  on the live o     (a subtraction, then the IEEE division)
 *                 Q = 0.0;  for each live o in order:  Q = Q + zeta[o] * zeta[o];     logp = (-0.5 * Q) - C
 *                 D = logp - old_logp[s]
 *                 rho = D <= 0 ? E(D < -708 ? -708 : D) : 1.0 / E(-D < -708 ? -708 : -D);   a NaN D: rho = NaN by a select (E sees 0.0)
 *     surrogate:  A_s = advantage[s], hi, lo, active, c and the sample's policy loss: word for word mgx_policy_grad
 *     entropy:    H = 0.0;  for each live o in order:  H = H + (L(s[o]) + 1.4189385332046727)     (a constant of the grid: once per lane)
 *     means:      dy[o]  = live ? c * (zeta[o] / s[o]) : 0.0
 *     log sigma:  dls[o] = live ? (c * (zeta[o] * zeta[o] - 1.0)) - ent_coef : 0.0        -> g_log_sigma[o]
 *     value, trunk, per-sample terms, result = (1.0 / M) * the sum over the live samples: word for word mgx_policy_grad, n_out = A
 *     a grid without a live column (every sigma 0, or scale[i] == 0): its policy loss, entropy, clipped flag, kl and dy are zero, the
 *                 value term stays; rho is still the formula's (logp = -0.0)
 *     stats[0 .. 5) = the means over the live samples of policy loss, value loss, H, the clipped flag (!active) and
 *                 kl = (rho - 1.0) - D       (the usual early-stopping estimate of the divergence from the collecting policy)
 *     ratio_out[s] = rho on the live samples; masked samples keep the caller's bytes
 * These are the gradient of mean(policy loss) + vf_coef * mean(value loss) - ent_coef * mean(H).  g_log_sigma[o] is the gradient
 * with respect to log sigma[o]: the entropy of a Gaussian whose sigma does not depend on the state does not depend on the mean, so
 * ent_coef appears there alone.  Sigma stays a host value of mgx_gaussian: who learns it keeps log sigma, steps it with g_log_sigma
 * and hands the next launch exp(log sigma) -- four numbers cross to the host per iteration.
 * THE RATIO of an un-updated policy is NOT exactly 1.0, unlike mgx_policy_grad's: raw = y + s * z is rounded, so (raw - y) / s is not
 * z bit for bit.  With u = 2^-53, delta[o] = u * (4 |zeta[o]| + 2 |raw[o]| / s[o]) and
 * B = sum over the live o of |zeta[o]| * delta[o] + 5 u Q + 2 u |logp|, it stays within |rho - 1| <= 1.01 * B + 8 u.
 * The sums over the samples, their order and what is unknown about the MFMA: as mgx_policy_grad states them. */
struct mgx_policy_grad_gaussian {
    int32_t struct_size;      /* = sizeof(struct mgx_policy_grad_gaussian) */
    int32_t x_f32;            /* 0: x is float64; 1: float32 */
    const void    *x;         /* [K, N, n_in]: the row decision (k, i) was taken on */
    const double  *raw_action;/* [K, N, n_out]: raw_actions_out of the launch */
    const double  *old_logp;  /* [K, N]: logp_out of the launch */
    const double  *advantage; /* [K, N] */
    const double  *returns;   /* [K, N]; NULL without a critic */
    const uint8_t *mask;      /* [K, N] or NULL */
    double clip_eps;          /* >= 0; +inf: no clipping */
    double vf_coef, ent_coef;
    double *g_w1, *g_b1;      /* [n_hidden, n_in], [n_hidden]; each output may be NULL */
    double *g_w2, *g_b2;      /* [n_out, n_mid], [n_out] */
    double *g_cw, *g_cb;      /* [n_mid], [1]; NULL without a critic */
    double *g_log_sigma;      /* [4]; entries o >= n_out and those of a dead column are 0.0 */
    double *stats;            /* [5] */
    double *ratio_out;        /* [K, N] */
    void   *workspace;        /* mgx_policy_grad_workspace bytes, at least (it serves both calls); 8-byte aligned */
    int64_t workspace_bytes;
};

/* Two launches: policy_grad_kernel with the Gaussian head and policy_grad_finish_kernel.  Of `gaussian` only sigma[0 .. n_out) and
 * scale are read (all four sigma are checked): no draw is made.  critic may be NULL as in mgx_policy_grad.  Nothing is launched when
 * the call is refused: everything mgx_policy_grad refuses, with gaussian / raw_action / old_logp in the place of sampling / action_id
 * / old_prob; MGX_ERR_INVALID on top for gaussian->struct_size != sizeof(mgx_gaussian), a sigma[o] that is negative, NaN, infinite
 * or positive and subnormal, and n_out outside 1 .. 4.  An ADDITION to ABI 9 that leaves MGX_ABI_MINOR at 3: found by name (dlsym). */
int mgx_policy_grad_gaussian(int64_t N, int32_t K, const mgx_policy *policy, const mgx_critic *critic, const mgx_gaussian *gaussian,
                             const struct mgx_policy_grad_gaussian *pg, mgx_stream stream);

/* WHAT-IF roll-outs of candidate plans ("shooting" model-predictive control): what would grid i earn over the next H steps under
 * plan c, without taking those steps.  It stands in for the horizon loop of ModelPredictiveControl (algos/mpc/mpc.py: the cost of
 * running the microgrid over the forecast horizon, on the series a forecaster="oracle" shows) with the simulator in the place of the
 * cvxpy program: every candidate is H steps of Microgrid.run (microgrid.py:227-325) on a COPY of the grid's state.  The launch
 * reads the handle of in-place episodes (mgx_reset_episodes) as mgx_rollout_episodes / mgx_step_k_episodes do -- state, parameters,
 * the rows of the grid's own running episode from the handle's current counter value t0 on, the reward shaper -- and writes
 * NOTHING back: no state, no counter move, no episode arrays, no statistics, no done flags, no rows.  THE RULE (stated here once;
 * plain fp64 in step order, multiply and add separate):
 *     per grid i and candidate c:  w = 1.0;  ret = 0.0
 *     for k = 0 .. H - 1:
 *         r   = the reward step k of plan c returns (what mgx_step_discrete / mgx_step return for it, shaper included)
 *         ret = ret + w * r;   w = w * gamma
 *         if t0 + k >= ep_final[i] - 1: stop        (the step that ends the episode is counted, nothing after it)
 * Nothing beyond the end of the RUNNING episode is simulated, with or without mgx_set_auto_reset: where a restart would land is a
 * draw that belongs to another episode.  The stop depends on the grid alone: steps[i] = min(H, ep_final[i] - t0), at least 1.
 *     ret[c, i]       the discounted return above
 *     steps[i]        the steps counted
 *     end_soc[c, i]   the state of charge after the last counted step (what soc_trace of the roll-out holds there)
 *     best[i]         the smallest c whose ret[c, i] no other exceeds: c = 0, then every later c replaces it where ret[c, i] is
 *                     GREATER (ties go to the first maximum)
 *     best_ret[i]     ret[best[i], i]
 *     first_action    step 0 of plan best[i], in the form the plans have: the id byte, or the A controls
 * best / best_ret / first_action / steps come from a second, small launch that is skipped when all four are NULL. */
typedef struct mgx_lookahead {
    int32_t struct_size;   /* = sizeof(mgx_lookahead) */
    int32_t C, H;          /* candidates per grid, horizon; both >= 1 */
    int32_t per_grid;      /* 0: plans shared by all grids; 1: a plan per grid */
    double  gamma;         /* in [0, 1] */
    double  *ret;          /* [C, N], required */
    int32_t *steps;        /* [N] or NULL */
    double  *end_soc;      /* [C, N] or NULL: the value soc_trace would hold at the last counted step */
    int32_t *best;         /* [N] or NULL */
    double  *best_ret;     /* [N] or NULL */
    void    *first_action; /* discrete: uint8 [N]; continuous: [N, A] in the action format; or NULL */
} mgx_lookahead;

/* Discrete plans: priority-list ids as bytes, [C, H] (la->per_grid == 0) or [C, H, N]; `table` / n_actions as in
 * mgx_rollout_discrete, ids outside the table select list 0.  One launch of lookahead_episodes_kernel (+ the pick).
 * MGX_ERR_INVALID: a NULL la / ret / handle / plans / table, la->struct_size != sizeof(mgx_lookahead), C or H below 1, gamma outside
 * [0, 1] or NaN, end_soc on a layout without a battery, a handle that does not step in-place episodes.  MGX_ERR_UNSUPPORTED: what
 * mgx_rollout_episodes refuses so (several modules of a kind, shards, device-counter mode) and a handle with
 * mgx_set_forecast_noise set -- the lookahead reads the series rows themselves, which is what the oracle forecaster shows.
 * MGX_ERR_RANGE: the counter stands outside its range.  mgx_set_final_obs, a forecast horizon in the observation and `done` as bit
 * sets change nothing (neither rows nor done flags are written).  What needs no handle (la and its fields) is checked first.
 * Nothing is launched when the call is refused.  An ADDITION to ABI 9 that leaves MGX_ABI_MINOR at 3: found by name (dlsym). */
int mgx_lookahead_episodes(mgx_handle *h, const uint8_t *plans, const int32_t *table, int32_t n_actions,
                           const mgx_lookahead *la, mgx_stream stream);

/* Continuous plans: controls [C, H, A] (la->per_grid == 0) or [C, H, N, A] in the handle's action format
 * (mgx_set_action_format); `normalized` as in mgx_step.  One launch of lookahead_step_k_episodes_kernel (+ the pick).  Refusals as
 * mgx_lookahead_episodes (there is no table), with mgx_step_k_episodes in the place of mgx_rollout_episodes. */
int mgx_lookahead_step_k_episodes(mgx_handle *h, const void *plans, int normalized,
                                  const mgx_lookahead *la, mgx_stream stream);

/* CROSS-ENTROPY METHOD (CEM) planning: the candidates of a what-if launch DRAWN INSIDE IT round a per-grid mean, and the refit of
 * that mean and deviation on the best few on the device.  The plan tensor [C, H, N, A] never exists: a candidate control is a
 * function of (key, grid, candidate, plan step, column) formed in registers, and the refit regenerates the elites' controls from
 * the same draws.  mean, sigma: double [H, N, A] (device), NORMALISED controls.  THE RULE (stated here once):
 *
 * Normal pair p of grid i, candidate c, plan step k (k: the index into the plan, not the step counter): Philox4x32-10 with the
 * counter words (lo32(i), (uint32)c, (uint32)k, 0xCE300000 + p) and the key (lo32(key), hi32(key)); its four words r[0 .. 3] give
 * (z[2p], z[2p + 1]) exactly as the normal pair of mgx_gaussian forms its pair out of r[0 .. 3].  Pair 0 serves columns 0 and 1,
 * pair 1 columns 2 and 3.
 *
 * Candidate value x[c, k, i, o]:
 *     c == 0:  v = mean[k, i, o]                                    (candidate 0 is the mean plan itself: no draw)
 *     c >= 1:  s = sigma[k, i, o];  v = s > 0 ? mean[k, i, o] + s * z[o] : mean[k, i, o]      (a separate multiply and add)
 *     x = !(v > 0) ? 0.0 : (v > 1 ? 1.0 : v)                        (the clip of mgx_policy)
 *     action format F32 (mgx_set_action_format; mgx_cem_refit.round_f32):  x = (double)(float)x -- what a float32 plan would hold
 * A pair is drawn only where one of its columns is live (s > 0: false for a negative or NaN sigma, which are not scanned for). */
typedef struct mgx_cem {
    int32_t struct_size;      /* = sizeof(mgx_cem) */
    int32_t reserved;
    uint64_t key;             /* Philox key */
    const double *mean;       /* device [H, N, A] */
    const double *sigma;      /* device [H, N, A] */
} mgx_cem;

/* mgx_lookahead_step_k_episodes with plans[c, k, i, :] replaced by x[c, k, i, :] above (normalised controls: there is no
 * `normalized`): one launch of lookahead_gaussian_episodes_kernel (+ the pick, which regenerates step 0 of candidate best[i] as
 * first_action, in the action format).  The return rule, the stop at the episode's end and every output are those of mgx_lookahead,
 * word for word; la->per_grid must be 1.  Refusals: those of mgx_lookahead_step_k_episodes; on top MGX_ERR_INVALID for a NULL cem,
 * cem->struct_size != sizeof(mgx_cem), a NULL mean or sigma, la->per_grid != 1 and a layout without a control.  (The draw holds 32 bits of i; a handle
 * holds fewer grids than that, mgx_cem_refit refuses more.)  Nothing is launched when the call is refused.  An ADDITION to ABI 9 that
 * leaves MGX_ABI_MINOR at 3: found by name (dlsym). */
int mgx_lookahead_gaussian_episodes(mgx_handle *h, const mgx_cem *cem, const mgx_lookahead *la, mgx_stream stream);

/* The refit of (mean, sigma) on the n_elite best of the C candidates of such a launch.  THE RULE (stated here once; plain fp64,
 * every multiply and add separate, sums in the order e = 0 .. n_elite - 1, S the square root of mgx_gaussian):
 *     elite[e, i]: for e = 0 .. n_elite - 1 the first maximum of ret[:, i] among the candidates not yet taken -- start at the lowest
 *         such c, a later c replaces it where its return is GREATER (so elite[0] is best of mgx_lookahead and ties go to the lower c)
 *     n = steps ? steps[i] : H.   Rows k < n, per column o, x_e = x[elite[e, i], k, i, o]:
 *         m = (x_0 + x_1 + ...) / n_elite;   d = S(((x_0 - m)^2 + (x_1 - m)^2 + ...) / n_elite)
 *         mean_out = alpha * m + (1.0 - alpha) * mean;   sg = alpha * d + (1.0 - alpha) * sigma
 *         sigma_out = sg > sigma_min ? sg : sigma_min
 *     Rows k >= n (nothing of them was simulated): mean_out = mean, sigma_out = sigma.
 *     best_plan[k, i, :] = x[elite[0, i], k, i, :] for every k, float32 where round_f32 (which also rounds every x above).
 * Two launches: cem_elite_kernel (a lane per grid), cem_refit_kernel (a lane per (grid, k)).  mean_out / sigma_out may be
 * cem->mean / cem->sigma: a lane reads only the entries it writes. */
struct mgx_cem_refit {
    int32_t struct_size;      /* = sizeof(mgx_cem_refit) */
    int32_t C, H;             /* candidates, horizon of the launch whose returns these are; both >= 1 */
    int32_t n_elite;          /* in [1, min(C, 32)] */
    int32_t round_f32;        /* the action format of that launch: 0 F64, 1 F32 */
    double  alpha;            /* in [0, 1]: the weight of the new estimate */
    double  sigma_min;        /* >= 0: the floor of sigma_out on the refitted rows */
    const double  *ret;       /* [C, N] */
    const int32_t *steps;     /* [N] or NULL (= H for every grid) */
    int32_t *elite;           /* [n_elite, N], required */
    double  *mean_out;        /* [H, N, A] */
    double  *sigma_out;       /* [H, N, A] */
    void    *best_plan;       /* [H, N, A] float64, or float32 where round_f32; or NULL */
};                            /* (a struct tag without a typedef: the call below bears the same name) */

/* Handle-free on the current device (as mgx_gae); N grids of A action columns.  MGX_ERR_INVALID: a NULL cem / refit / mean / sigma /
 * ret / elite / mean_out / sigma_out, a wrong struct_size, N, C or H below 1, n_elite outside [1, min(C, 32)], A outside 1 .. 4,
 * alpha outside [0, 1] or NaN, sigma_min negative or NaN.  MGX_ERR_UNSUPPORTED: N > 2^32.  An ADDITION to ABI 9 that leaves
 * MGX_ABI_MINOR at 3. */
int mgx_cem_refit(int64_t N, int32_t A, const mgx_cem *cem, const struct mgx_cem_refit *refit, mgx_stream stream);

/* raise_errors=True(BaseMicrogridModule.__init__, base_module.py:40; as_source / as_sink, :213-224,265-270; _raise_error,
 * :79-93): the reference refuses a request a module cannot meet with a ValueError instead of clipping it.  mgx_step always
 * clips; mgx_check_step is its DRY RUN -- the same arithmetic on a register copy of the state, nothing stored, the counter
 * untouched -- and writes per grid the mask of requests the reference would refuse: bit 0 genset request outside
 * [min, max] production, bit 1 battery request above max_production / max_consumption, bit 2 grid request above its
 * limit, bit 3 genset goal outside [0, 1], bit 4 negative genset energy, bit 5 a battery / grid acting at a negative
 * limit (enum mgx_violation_bit).  A caller that wants raise_errors semantics
 * checks first and steps only when every mask is 0 (the reference has by then already stepped the modules that come
 * before the refusing one in its sweep; here nothing is applied).  violations [N] uint32 (device). */
int mgx_check_step(mgx_handle *h, const void *actions, int normalized, uint32_t *violations, mgx_stream stream);
/* The dry run of mgx_step_discrete: DiscreteMicrogridEnv.step asserts its way through _populate_action
 * (priority_list.py:73,121,124,135,154) and through the step (base_module.py:272) whatever raise_errors says.  violations [N]
 * receives the expansion's assert bit where the reference would have raised inside _populate_action (MGX_V_EXPAND_*: it never
 * steps then), else the mask mgx_check_step would give for the expanded control.  Nothing is stored, the counter does not
 * move.  One module of every kind per grid (layouts with several: mgx_expand_lists with `violations`, then mgx_check_step). */
int mgx_check_discrete(mgx_handle *h, const int32_t *action_id, const int32_t *table, int32_t n_actions, uint32_t *violations,
                       mgx_stream stream);

/* K consecutive mgx_step calls issued by ONE call: the Gym cadence (`for a in actions: env.step(a)`, one kernel launch
 * per env-step, envs/base/base.py:169-209) without a host round trip per step -- from Python a per-step call costs
 * more than the 5 us the kernel takes at N = 100 000.  actions [K, N, A]; reward [K, N]; done [K, N], obs [K, N, D]
 * (block k = the observation after step k) and log [K, L, N] may be NULL. */
int mgx_step_many(mgx_handle *h, const void *actions, int32_t K, int normalized,
                  double *reward, uint8_t *done, void *obs, double *log, mgx_stream stream);

/* The Gym step with NO per-step bookkeeping on the caller's side (`while not done: obs, r, done, info = env.step(a)`,
 * README.md:109-111, envs/discrete/discrete.py:109-143, envs/base/base.py:169-209).  A single-step kernel takes ~5 us at
 * N = 100 000, so whatever the host does between two launches -- choosing the output buffers, walking the observation rings,
 * issuing the next ring's prefetch -- is part of the env-step's time when it is done in an interpreter.  mgx_env_bind hands the
 * handle everything that rotates, once; mgx_env_step / mgx_env_step_discrete then take the controls and a stream and do the rest:
 *   outputs   step j (counted from the bind / the last mgx_env_seek) writes reward / done / log -- and, without rings, the
 *             observation row -- into slots[j % n_slots]: n_slots rotating buffer sets, each valid until the step n_slots later;
 *   rings     ring_K > 0 (the handle in MGX_OBS_ROWS_STATE_ONLY mode): three rings of ring_K row blocks written ahead by
 *             mgx_observe_windows[_ahead].  The env stands on block `ring_pos` of ring `ring_idx`; a step adds its state columns to
 *             the NEXT block (the observation it returns), moves there, and when that enters the following ring it first waits for
 *             that ring's prefetch (mgx_prefetch_wait) and afterwards starts the prefetch of the ring behind it
 *             (mgx_observe_windows_ahead(ahead = ring_K)): exactly the sequence pymgrid_amd/envs.py used to issue call by call.
 * Values are those of mgx_step / mgx_step_discrete, bit for bit (tests/test_env_step.py).  mgx_env_seek tells the handle where
 * the caller stands after anything that moved the rings or the slot outside these calls (mgx_reset + mgx_observe_windows: block 0
 * of ring 0); mgx_env_position reports where the LAST step's outputs are.  Slot and ring pointers are caller-owned device memory. */
typedef struct mgx_env_slot {
    double *reward;               /* [N] */
    uint8_t *done;                /* [N] or NULL (lock-step: derive it from the counter) */
    void *obs;                    /* [N, D] row target of the step (NULL with rings, or when no observation is wanted) */
    double *log;                  /* [L, N] or NULL */
} mgx_env_slot;
#define MGX_ENV_MAX_SLOTS 128
typedef struct mgx_env_plan {
    int32_t struct_size;          /* = sizeof(mgx_env_plan) */
    int32_t n_slots;              /* 1 .. MGX_ENV_MAX_SLOTS */
    const mgx_env_slot *slots;    /* host array [n_slots]; copied */
    int32_t ring_K;               /* 0: no rings */
    int32_t n_actions;            /* discrete: rows of `table` (0: continuous steps only) */
    void *rings[3];               /* ring r = [ring_K] blocks, the handle's ring pitch / layout (mgx_set_ring_pitch / _layout) */
    const int32_t *table;         /* host [n_actions, 3, 2] (mgx_expand_discrete); copied */
} mgx_env_plan;
int mgx_env_bind(mgx_handle *h, const mgx_env_plan *plan);           /* plan == NULL: unbind */
int mgx_env_seek(mgx_handle *h, int32_t next_slot, int32_t ring_idx, int32_t ring_pos);
int mgx_env_position(const mgx_handle *h, int32_t *last_slot, int32_t *ring_idx, int32_t *ring_pos);   /* each may be NULL */
int mgx_env_step(mgx_handle *h, const void *actions, int normalized, mgx_stream stream);
int mgx_env_step_discrete(mgx_handle *h, const int32_t *action_id, mgx_stream stream);

/* BaseMicrogridModule.sample_action(strict_bound=True) (modules/base/base_module.py:326-356, Microgrid.sample_action
 * microgrid.py:337-362): lo / hi [N, A] (device) receive, per action column, the NORMALISED interval a draw must come from to
 * respect the module's instantaneous limits at the current state and row: battery and grid columns
 * [normalize(-max_consumption), normalize(max_production)] (a NaN bound is 0, as there); genset columns [0, 1] (the reference
 * itself raises on a genset with strict_bound: the Python mirror refuses such layouts).  A strict sample is
 * lo + u * (hi - lo), u ~ U[0, 1).  Nothing is stepped. */
int mgx_action_bounds(mgx_handle *h, double *lo, double *hi, mgx_stream stream);

/* Shards.  Grids never interact (no cross-grid term anywhere in Microgrid.run), so the launch sequence of one range of
 * grids owes nothing to another's.  mgx_set_shards(h, S > 1) splits every stepping call (mgx_step, mgx_step_many,
 * mgx_step_k, mgx_step_discrete, mgx_expand_discrete, mgx_rollout_discrete) into S launches over contiguous grid ranges,
 * each on its own internal HIP stream, and the ranges are NOT joined between calls: while one range is in the ramp-up or
 * the tail of a launch another is in full flight (measured: 66-68 instead of 74-76 us per 64-step round of 100 000
 * grids with S = 2).  In this mode the `stream` argument of those calls is ignored; ordering
 * against other streams is explicit:
 *   mgx_fork(h, s)  the shard streams wait for everything queued on s so far  (inputs produced on s are then safe)
 *   mgx_join(h, s)  s waits for everything issued to the shard streams so far (outputs are then safe to read on s)
 * Every other entry point still runs on the stream it is given: bracket it with mgx_join / mgx_fork.  Buffers handed to
 * a stepping call must stay alive until the next mgx_join.  mgx_shard_stream returns the hipStream_t of a shard (for
 * timing events), NULL when shards are off.  Not offered in device-counter mode.  The shard streams are a per-device pool
 * shared by all handles of the process (the runtime multiplexes streams onto a few hardware queues: private pairs per handle
 * ended up on one queue): handles that step in shards at the same time are ordered per stream -- work of two handles on
 * shard j runs in issue order, and mgx_destroy / mgx_set_shards of one handle synchronise pooled streams that other handles
 * may still be using (a wait, never a loss).  The pool is created under a lock: handles may live on different host threads
 * (one thread per handle). */
int mgx_set_shards(mgx_handle *h, int32_t n_shards);
/* Single-step calls in shards (mgx_step, mgx_step_many, mgx_step_discrete, mgx_env_step*): one host thread issues a launch every
 * 3.4-4.3 us, so S launches per env-step from the calling thread make the Gym cadence S times slower than no shards at all.
 * Launch threads: shard j >= 1 is issued by a resident host thread of the library (one per device and shard, shared by all
 * handles, asleep when idle) while the caller issues shard 0.  mode 0: never; 1 (default): inside mgx_step_many, where every
 * thread gets its shard's K launches in one piece; 2: also for every single-step call (one hand-over per call).  A call still
 * returns only when every shard's launches have been issued, and values do not depend on the mode.  Fused calls (mgx_step_k,
 * rollouts) are always issued by the caller.
 * MEASURED (profiles/r06/exp_two_chains.txt, chain_trace_summary.txt; N = 100 000): two chains from two threads run 6.1 us per
 * env-step against 4.8 us for ONE chain from one thread (7.9 us for two chains from one thread): inside one process two threads
 * issue at 6 us per launch each, and a 50 000-grid launch lasts as long as a 100 000-grid one (4.2-4.8 us: the step is a latency
 * chain, not a transfer), so the second chain cannot pay whatever the host does.  Kept because it halves the cost of shards for
 * single steps; not a way below the one-chain cadence. */
int mgx_set_launch_threads(mgx_handle *h, int32_t mode);
int mgx_fork(mgx_handle *h, mgx_stream stream);
int mgx_join(mgx_handle *h, mgx_stream stream);
void *mgx_shard_stream(mgx_handle *h, int32_t shard);

/* Heterogeneous fleets (a population of microgrids with different module sets: one handle per layout).  One call steps
 * every batch of the fleet once -- `for m in microgrids: m.run(control)` over the whole population -- and, for the
 * batches whose observation ring is used up, issues the window prefetch of the next refill_K steps
 * (mgx_observe_windows) behind the steps; no host work between the launches.  An item is a continuous step
 * (actions; `normalized` applies) or, when action_id != NULL, a discrete one (mgx_step_discrete with table / n_actions).
 * All items are validated before the first launch. */
typedef struct mgx_fleet_item {
    int32_t struct_size;          /* = sizeof(mgx_fleet_item) */
    int32_t n_actions;            /* discrete: rows of `table` */
    mgx_handle *handle;
    const void *actions;          /* [N, A] continuous control, or NULL */
    const int32_t *action_id;     /* [N] priority-list ids (device), or NULL */
    const int32_t *table;         /* host [n_actions, 3, 2], discrete only */
    double *reward;               /* [N] */
    uint8_t *done;                /* [N] or NULL */
    void *obs;                    /* [N, D] (or the state-only target inside a ring block) or NULL */
    double *log;                  /* [L, N] or NULL */
    void *refill_ring;            /* [refill_K, N, D] or NULL: window prefetch issued with this step.  Block k = the window columns of
                                   * counter value (counter after this step) + refill_ahead + k.
                                   *   refill_chunks == 0: the whole batch -- mgx_observe_windows (refill_ahead == 0, after the step)
                                   *     or mgx_observe_windows_ahead (refill_ahead >= 1, on the handle's prefetch stream);
                                   *   refill_chunks >= 1 (refill_ahead >= 1): only chunk refill_chunk of refill_chunks of the
                                   *     batch's 16-grid groups, on `stream`, as extra workgroups of the step's own launch: a ring
                                   *     spread over the K - 1 steps before it is needed moves at a constant rate instead of
                                   *     one burst per K steps (state columns zero, as in mgx_observe_windows_ahead). */
    int32_t refill_K;
    int32_t refill_ahead;
    int32_t refill_chunk;
    int32_t refill_chunks;
    int32_t wait_prefetch;        /* != 0: mgx_prefetch_wait(handle, stream) before the step (its obs target lies in a ring that
                                   * mgx_observe_windows_ahead wrote) */
    int32_t reserved;
} mgx_fleet_item;
int mgx_fleet_step(const mgx_fleet_item *items, int32_t n_items, int normalized, mgx_stream stream);
/* Launch rule of mgx_fleet_step.  Lock-step items with one module of every kind (and those with at most two modules of a kind,
 * continuous controls and no forecast noise) share one launch of the fleet kernel per MGX_FLEET_MAX = 5 items.  Items whose handle
 * steps in-place per-grid episodes (mgx_reset_episodes; mgx_set_auto_reset / mgx_set_final_obs as for mgx_step) with one module of
 * every kind, no shards, no device counter, and rows written by the step itself -- no rows, whole H = 0 rows, or the state columns of
 * a ring block (MGX_OBS_ROWS_STATE_ONLY) -- share a launch of the fleet kernel's episode form per 5 items: each grid reads its own
 * rows, writes the row before its restart and restarts itself, as mgx_step / mgx_step_discrete do for one handle, with the same
 * values bit for bit.  MGX_TUNE_FLEET_EPISODES = 0 steps them beside instead.  Every other item is stepped beside the shared
 * launches through the single-handle path (several modules of a kind in episodes, rolling window buffers, rows with a horizon
 * written behind the step, shards, device counters).  The caller's per-handle work after a step (ring patches of the restarted
 * grids, mgx_patch_windows; restarts drawn on the host, mgx_reset_grids) follows the call on the same stream. */
/* The bound form of a fleet's Gym step: every handle carries an env plan (mgx_env_bind: rotating reward / done / row / log slots,
 * three observation rings) and the call is mgx_fleet_step over the items those plans produce -- handle j steps with actions[j]
 * (continuous controls [N, A], or int32 priority-list ids [N] where the plan holds a table) into its next slot and ring block,
 * waits for its prefetched ring when it enters it and has the ring after that one written ahead -- one launch for the steps of
 * all layouts, one C call per fleet step, no per-step bookkeeping on the host (`for env in envs: env.step(a)` of N reference
 * microgrids of different module sets; envs/base/base.py:169-209).  Afterwards every handle's slot and ring position have moved
 * as by mgx_env_step (mgx_env_position).  Nothing moves when the call fails validation.  n_handles <= 64. */
int mgx_fleet_env_step(mgx_handle *const *handles, const void *const *actions, int32_t n_handles, int normalized, mgx_stream stream);

/* MicrogridGenerator's time series on device (MicrogridGenerator.py): load / pv = base profile x size / max(profile)
 * (_scale_ts, :137-147; stored with the modules' sign, base_timeseries_module.py:68-79), import price = tariff pattern
 * 1 / 2 by hour of day (_get_electricity_tariff, :253-285), export price 0, co2 = base co2 profile (:205-212), grid
 * status = 1 except weak-grid outages (_generate_weak_grid_profile, :321-340: a uniform draw per row below
 * outage_per_day / 24 starts an outage whose back-fill covers the duration - 1 rows before it, never row 0; T + 1
 * draws).  Uniforms come from Philox4x32-10(seed; global grid index, row), so rank r of W writes exactly columns
 * [grid_index0, grid_index0 + n_grids) of the same global batch.  Everything is a device pointer; grid_ts (and the
 * arrays only it needs) may be NULL.  No handle: this runs before mgx_create. */
typedef struct mgx_synth {
    int32_t struct_size;          /* = sizeof(mgx_synth) */
    int32_t n_grids, n_steps;
    int32_t n_load_profiles, n_pv_profiles, n_co2_profiles;
    const double *base_load, *base_pv, *base_co2;          /* [T, n_*_profiles], values as in the reference's csv files */
    const int32_t *load_profile, *pv_profile, *co2_profile; /* [N] column of the base arrays */
    const double *load_ratio, *pv_ratio;                    /* [N] size / max(profile) */
    const int32_t *tariff;                                  /* [N] 1 or 2 */
    const int32_t *weak;                                    /* [N] 0 / 1 (rand_weak_grid, :535) */
    const double *outage_per_day;                           /* [N] randn * 3/4 + 0.25 (:291) */
    const int32_t *outage_duration;                         /* [N] randint(1, 8) (:292) */
    uint64_t seed;
    int64_t grid_index0;                                    /* global index of grid 0 ... */
    const int64_t *grid_index;                              /* ... or [N] global indices (a scattered selection); NULL: grid_index0 + i */
    double *load_ts, *pv_ts;                                /* out [T, N]; both NULL: only the outage words are produced */
    double *grid_ts;                                        /* out [T, 4, N] or NULL */
    uint64_t *outage_bits;                                  /* out [ceil(T / 64), N] or NULL: the factorised form of grid_status
                                                             * (mgx_columns.outage_bits), same draws as grid_ts[:, 3] */
} mgx_synth;
int mgx_synthesize_series(const mgx_synth *args, mgx_stream stream);

/* MicrogridGenerator's per-microgrid DRAWS and SIZING on device (MicrogridGenerator.py:346-386 _size_mg / _size_genset /
 * _size_battery, :417-441 _bin_genset_grid / _size_load, :230-243 _get_battery, :288-292 _get_grid, :535-538; module parameters
 * as convert/get_module.py:39-97 derives them): one lane per grid draws the grid's scalars and sizes its modules.  Every
 * output is a device array [n_grids] (NULL = not wanted); nothing of size N ever exists on the host, and rank r of W produces
 * exactly the grids [grid_index0, grid_index0 + n_grids) of the same global batch.
 *   draws   counter-based: U[0, 1) = Philox4x32-10(seed ^ 0x9E3779B97F4A7C15; global grid index, quantity id) -- the reference
 *           consumes numpy's global stream one microgrid at a time, which no batch can reproduce; what is reproduced is every
 *           RULE applied to the draws.  randint(lo, hi) = lo + floor(u (hi - lo)); a standard normal = the sum of 12 uniforms
 *           minus 6 (Irwin-Hall: additions only, so host and device agree bit for bit without sharing a libm).
 *   rules   size_load ~ randint(100, 100001), load / pv file ~ randint(0, n_profiles), pv penetration ~ randint(30, 151),
 *           battery hours ~ randint(3, 6); load_ratio = size_load / max(load profile) (_scale_ts, :137-147); pv size = peak of the
 *           scaled load x penetration / 100, pv_ratio = pv size / max(pv profile); battery capacity = ceil(hours x mean of the
 *           scaled load) -- the mean summed in numpy's pairwise order over the n_steps products, divided by n_steps -- power =
 *           ceil(capacity / 4), min capacity = 0.2 capacity, soc0 = min(max(normal, 0.2), 1), charge = soc0 x capacity; genset
 *           rating = ceil(peak / 0.9), running min / max = 0.05 / 0.9 of it; grid power = floor(2 peak); weak ~ randint(0, 2),
 *           tariff ~ randint(1, 3), outages per day = normal x 3 / 4 + 0.25, outage duration ~ randint(1, 8), co2 file ~
 *           randint(0, n_co2_profiles); genset timers ~ randint(0, 4) when mixed_timers else 0; architecture by
 *           _bin_genset_grid's uniform (< 0.33 genset only, < 0.66 grid only, else both; a weak grid forces a genset).
 * base_load: the load table; *_max / *_min: per-profile extrema (host: a few numbers).  Observation bounds come out as the
 * modules compute them from the series they hold (base_timeseries_module.py:81-88). */
typedef struct mgx_gen {
    int32_t struct_size;          /* = sizeof(mgx_gen) */
    int32_t n_grids, n_steps;
    int32_t n_load_profiles, n_pv_profiles, n_co2_profiles;
    int32_t mixed_timers;
    int32_t n_mean_rows;          /* rows of base_load the sizing rules see: the WHOLE profile (8 760), whatever n_steps is */
    uint64_t seed;
    int64_t grid_index0;
    const int64_t *grid_index;    /* [N] global indices (a scattered selection) or NULL: grid_index0 + i */
    const double *base_load;      /* [n_mean_rows, n_load_profiles] (the mean of the scaled load) */
    const double *load_max, *pv_max;                      /* [n_*_profiles]: max over the whole profile (the sizing rules) */
    const double *load_bound_max, *pv_bound_max;          /* [n_*_profiles]: max over the n_steps rows a module holds (its bounds) */
    const double *co2_min, *co2_max;                      /* [n_co2_profiles], over the n_steps rows */
    double tariff_min[3], tariff_max[3];                  /* by pattern (0 unused) */
    /* outputs, each [N] or NULL */
    uint8_t *arch;                /* 0 genset+battery, 1 battery+grid, 2 genset+battery+grid */
    uint8_t *load_profile, *pv_profile, *co2_profile, *tariff;
    int32_t *weak, *outage_duration;
    double *outage_per_day;
    double *load_ratio, *pv_ratio;
    double *load_lo, *load_hi, *pv_lo, *pv_hi;
    double *grid_lo, *grid_hi;    /* [4, N]; the status rows (component 3) come out as 1 ("never out"): the caller lowers them where
                                   * the outage words it synthesises say otherwise */
    double *bat_min_capacity, *bat_max_capacity, *bat_max_charge, *bat_max_discharge, *charge, *soc;
    double *gen_running_min, *gen_running_max;
    uint32_t *gen_times, *gen_status;
    double *grid_max_import, *grid_max_export;
    /* the raw draws, for whoever wants to re-apply the rules: [N] each or NULL */
    double *d_bin_rand, *d_soc0_normal, *d_outage_normal;
    int32_t *d_size_load, *d_pv_pen, *d_bat_hours, *d_su, *d_wd;
} mgx_gen;
int mgx_generate_columns(const mgx_gen *args, mgx_stream stream);

/* Column sums over the grids, sums[m] = sum_i values[m*N + i] (deterministic two-stage wavefront-shuffle +
 * LDS reduction; the "metrics" vector that is all-reduced across GPUs).  M <= 64. */
int mgx_metrics(mgx_handle *h, const double *values, int32_t M, double *sums, mgx_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* MGX_H */
