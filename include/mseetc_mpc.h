/*
 * mseetc_mpc.h -- C ABI of the device-resident shrinking-horizon loop (BASELINE config 4).
 *
 * The reference has no MPC loop: its mechanism for a re-solve from the current position is Track.updateLimits(positionStart)
 * (track.py:420-450) + a new casadiSolver on the cropped track + solve(T, initialTime, initialVelocity) (ocp.py:310), always from a
 * cold start (ocp.py:325-339).  mseetc/mpc.py: shrinkingHorizon does that for a batch of scenarios with one launch per re-solve and the
 * bookkeeping on the host; this entry point runs the same loop with the bookkeeping on the device: the sequence of grids does not depend
 * on the solutions, so all problem records are uploaded once, and per re-solve the measured state (time and speed at node `stride` of the
 * previous solution, perturbed by the caller's noise draws), the scenario records, the failure handling (minimum running time from the
 * time-optimal twin, arrival time moved there, repeated solve) and the log are small kernels between the solver's launches on one stream.
 * Nothing is waited for and nothing crosses PCIe between the first launch and the end of the loop.
 */
#ifndef MSEETC_MPC_H
#define MSEETC_MPC_H

#include "mseetc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct msd_mpc *msd_mpc_handle;

/* one record of the log per re-solve and scenario */
enum { MSD_MPC_T0 = 0,        /* measured time the re-solve starts from */
       MSD_MPC_V0,            /* measured speed (before the clipping of ocp.py:343) */
       MSD_MPC_T,             /* arrival time of the re-solve (moved where the measured state no longer allowed the one asked for) */
       MSD_MPC_STATUS, MSD_MPC_ITERS, MSD_MPC_OBJ,      /* MSD_ST_STATUS / _ITERS / _OBJ of the re-solve's last launch for the scenario */
       MSD_MPC_RELAXED,       /* > 0: the arrival time was moved in this re-solve -- 1 on the verdict of a converged time-optimal twin, 2 on that of a twin that ended next to its optimum without converging */
       MSD_MPC_COUNT };

typedef struct {
    int num_resolves;                      /* K: re-solve k runs on problems[k] */
    int stride;                            /* intervals the train advances between two re-solves (problems[k + 1] has `stride` intervals fewer) */
    const msd_problem_desc *problems;      /* [K] the energy problems on the cropped tracks (casadiSolver on Track.updateLimits(positionStart)) */
    const msd_problem_desc *twins;         /* [K] their time-optimal twins (ocp.py:146-150), or NULL: a failed re-solve is left as it is */
    const double *vlim_first;              /* [K] speed limit at the first node of grid k [m/s] (clipping of the initial speed, ocp.py:343) */
    const double *length;                  /* [K] length of grid k [m] */
    const unsigned char *tail;             /* [K] 1: grid k is grid k - 1 without its first `stride` intervals (the previous solutions are a
                                            * warm start for it on the device: msd_solve_batch_shifted); tail[0] is ignored */
    double vmin, vmax_train;               /* minimumVelocity; maximum speed of the train (loose running time of the twin) */
    double terminal_velocity;              /* clipped by the caller to [vmin, speed limit at the last node] (ocp.py:344) */
    int warm_start;                        /* 1: shifted primal-dual warm starts where tail[k]; 0: every re-solve from the problem's own starting point */
    double warm_mu, warm_push;             /* barrier parameter and interior push of a warm start (msd_solve_batch_shifted) */
    double noise;                          /* relative measurement noise: t <- max(t (1 + noise n1), 0), v <- v (1 + noise n2) */
    int relax_infeasible;                  /* 1: a re-solve that fails although ... see late_margin */
    double late_margin;                    /* a failed re-solve whose minimum running time tmin (twin) exceeds T - t0 is repeated with T = t0 + tmin (1 + m),
                                            * m = late_margin, then 4 m, then 16 m */
} msd_mpc_plan;

/*
 * Build the loop for one device handle pair: `h` is configured for problems[0] (its stream runs the loop), `twin` for twins[0] (may be NULL with
 * plan->twins).  Uploads every problem record; the descriptions may be freed afterwards.
 */
int msd_mpc_create(msd_handle h, msd_handle twin, const msd_mpc_plan *plan, msd_mpc_handle *out);
int msd_mpc_destroy(msd_mpc_handle m);

/*
 * Run the loop for nscen scenarios: arrival times T[nscen], common initial time and speed, draws n1/n2 [K - 1][nscen] (standard normal; the
 * state after re-solve k is perturbed with row k).  Host outputs (each may be NULL): log[K][nscen][MSD_MPC_COUNT]; z_log = the solutions of
 * every re-solve back to back ([nscen][nz_k] for k = 0 .. K - 1, nz_k = msd_mpc_nz(m, k)); loop_ms = device time of the whole loop (events around
 * it), solve_ms = sum of the solver's launches alone is not separable without waiting and is not reported.
 */
int msd_mpc_run(msd_mpc_handle m, int nscen, const double *T, double initial_time, double initial_velocity, const double *n1, const double *n2,
                double *log, double *z_log, float *loop_ms);
int msd_mpc_nz(msd_mpc_handle m, int k);

/*
 * Speed restrictions inside the loop: restrictions per scenario that become known while the train is under way (a temporary speed restriction announced at
 * re-solve k, a signal aspect, engineering works) -- msd_problem_speed_restrictions (mseetc_hip.h) for the loop, on the loop's own grids.
 *
 * A record is (begin [m], end [m], velocity [m/s], first_resolve).  Positions are route coordinates: 0 is the first node of the grid of re-solve 0.
 * first_resolve is the (integer-valued) index of the re-solve from which the restriction is known; 0: from the start.  Re-solve k starts at origin[k], the route
 * coordinate of the first node of grid k.  A record counts for its scenario in re-solve k if first_resolve <= k and, with begin_k = begin - origin[k] and
 * end_k = end - origin[k] (one rounded subtraction each), it restricts at least one interval of grid k under the rule of mseetc_hip.h
 * (pos[i] < end_k && pos[i+1] > begin_k, pos the node positions of grid k).  A restriction that lies wholly behind the train by then is ignored; that is no error.
 * The row of limits of scenario s in re-solve k is the row of mseetc_hip.h on grid k from (begin_k, end_k, velocity) of the records that count; the measured speed
 * is clipped to min(vlim_first[k], velocity of the records that restrict interval 0), the terminal speed to min(terminal_velocity, velocity of the records that
 * restrict the last interval) -- per scenario, on the device.  These are the rules of mseetc/ocp.py: _scenarios and restrictedLimits under restrictions, bit for
 * bit (mseetc/mpc.py: DeviceLoop.restrictedLimits is the host statement).
 *
 *   origin  [K]                                               non-decreasing, origin[0] = 0
 *   count   [nscen]                                           records of scenario s, 0 ... max_per_scenario
 *   records [nscen][max_per_scenario][MSD_MPC_RS_COUNT]       host; entries behind a scenario's count are ignored
 *
 * The records are state of the loop: every msd_mpc_run with exactly nscen scenarios runs under them until they are cleared with nscen = 0 (the other arguments may
 * be NULL then); a run with another nscen returns MSD_E_INVALID and enqueues nothing.  The call waits for the loop's stream and uploads records and counts once;
 * per re-solve one kernel in front of the scenario records builds the [nscen][N_k+1] rows and the two speed caps, and every launch of the re-solve -- the main one,
 * the time-optimal twin's, the repeated solves of moved arrival times -- runs under the rows.  Nothing is waited for and nothing crosses PCIe inside the loop.
 * Without records the loop launches exactly what it launched before this entry point existed.
 *
 * MSD_E_INVALID (text in msd_last_error(); the records the loop held stay as they were): a null pointer; max_per_scenario outside 1 ... MSD_RS_MAX; a count outside
 * 0 ... max_per_scenario; a record that is not finite; end <= begin; velocity <= 0 or velocity^2 <= vmin^2; a first_resolve that is not an integer in 0 ... K-1;
 * a record that restricts no interval of grid 0; an origin that is not non-decreasing from 0; an nscen other than that of the rolling stock the loop holds
 * (msd_mpc_rolling_stock).
 * Not built: a restriction that is lifted again, end points as grid nodes, a limit equal to the minimum speed.
 */
#define MSD_MPC_RS_COUNT 4      /* begin [m], end [m], velocity [m/s], first_resolve */
int msd_mpc_speed_restrictions(msd_mpc_handle m, const double *origin, int nscen, int max_per_scenario, const int *count, const double *records);

/*
 * Measurement aid: the rows of re-solve k under the loop's records, built by the kernel the loop launches, rows[nscen][N_k+1] (host).  Waits for the loop's stream.
 * MSD_E_INVALID when the loop holds no records or k is outside 0 ... K-1.  (tests/test_mpc_speed_restrictions_gpu.py: bit for bit the host statement)
 */
int msd_mpc_limit_rows(msd_mpc_handle m, int k, double *rows);

/*
 * Rolling stock inside the loop: a train of its own per scenario for the controller (config 3: msd_solve_batch_ex for the loop) and a plant per scenario -- the
 * train that actually runs, which need not be the controller's model.
 *
 * model [nscen][MSD_OV_COUNT]: the override rows of msd_solve_batch_ex (mseetc_hip.h), with its checks.  Row s goes into the main launch and the repeated solves
 * of every re-solve of scenario s; the time-optimal twin runs under the same row with MSD_OV_OBJ_DEN replaced by the objective scaling of the twin of that
 * re-solve (a constant of the twin's problem, length / maximum speed of grid k, not a function of the mass), rewritten on the device per re-solve.  NULL: the
 * problems' own train.
 *
 * plant [nscen][MSD_MPC_PL_COUNT]: without it the state the next re-solve starts from is read from node `stride` of the plan, which makes the plan its own plant.
 * With it one kernel per advance integrates the plant from the re-solve's own initial state (t0 and the clipped v0^2 of its scenario record) over the first
 * `stride` intervals of grid k under the planned forces w_i = (Fel_i + Fpb_i) force_scale of the re-solve's solution: per interval the explicit Runge-Kutta map of
 * the solver (4th order, plant_steps steps per interval, time integrated with the same stages: num_approx_steps = 0) with the plant's specific Davis
 * coefficients and the problem's own g, rho and track resistance -- whatever shooting integrator or loss model the problems have.  The noise is applied to that
 * state as it is to the plan's.  After an interval, !(b+ >= vmin^2) or a non-finite running time marks the scenario stalled: it keeps its last measurement from
 * then on (like a scenario whose re-solve failed) and MSD_MPC_PS_STALLED is 1 in this and every later record.  NULL: the plan is the plant.
 *
 * The records are state of the loop exactly like the speed restrictions: uploaded once; every msd_mpc_run with exactly nscen scenarios runs under them;
 * nscen = 0 clears them (the other arguments are ignored); a run with another count returns MSD_E_INVALID and enqueues nothing; refused records leave the previous
 * ones in place.  Restrictions and rolling stock compose; where the loop holds both their counts must agree (the later call is refused otherwise).  Nothing is
 * waited for and nothing crosses PCIe inside the loop.  With neither array the loop launches exactly what it launched before this entry point existed.
 *
 * MSD_E_INVALID: nscen < 0; both arrays NULL with nscen > 0; a model row msd_solve_batch_ex refuses; a plant row that is not finite, has a negative Davis
 * coefficient or force_scale <= 0; plant_steps outside 1 ... 64 (with a plant); a count other than that of the speed restrictions the loop holds.
 * Not built: a plant rho, adhesion or force limits of its own; disturbance estimation.  (The energy the closed loop really spends: msd_mpc_energy.)
 */
enum { MSD_MPC_PL_SR0 = 0, MSD_MPC_PL_SR1, MSD_MPC_PL_SR2,   /* specific Davis coefficients of the plant (per kg of ITS mass*rho) */
       MSD_MPC_PL_FORCE_SCALE,                               /* (mass*rho of the scenario's model) / (mass*rho of the plant): commanded newtons -> plant's specific force */
       MSD_MPC_PL_COUNT };
int msd_mpc_rolling_stock(msd_mpc_handle m, int nscen, const double *model, const double *plant, int plant_steps);

/*
 * The plant's state behind every advance of the last run, before the noise: states[K-1][nscen][MSD_MPC_PS_COUNT] (host), record k for the advance behind re-solve
 * k.  MSD_MPC_PS_T [s] and MSD_MPC_PS_V [m/s]: the state at node `stride` of grid k; for a scenario that stalls in this advance the last state in front of the
 * interval that stalled it; for a scenario that was not advanced (its re-solve failed, or it stalled earlier) the measurement it keeps.
 * MSD_E_INVALID: the loop holds no plant, or has not run under it yet.
 */
enum { MSD_MPC_PS_T = 0, MSD_MPC_PS_V, MSD_MPC_PS_STALLED, MSD_MPC_PS_COUNT };
int msd_mpc_plant_states(msd_mpc_handle m, double *states);

/*
 * The energy account of the closed loop: what the train really spent, leg by leg, kept on the device while the loop runs (the reference's accounting,
 * utils.py:243-257 and :291, Energy [kWh] = (1e-6/3.6) ds F + losses; mseetc/mpc.py: plantEnergy is the host statement the kernel is held to).
 *
 * A leg is what is driven behind a re-solve: the first `stride` intervals of its plan behind re-solve k < K-1 (record k), and behind the last re-solve the whole
 * remaining plan, N_{K-1} intervals (record K-1, the final leg: no noise, nothing is measured any more).  Forces in newtons are the plan's specific forces times
 * the total mass of the scenario's MODEL: total_mass = mass rho of the problems' train, or MSD_OV_TOTAL_MASS of the scenario's model row where the loop holds one
 * and it is non-zero -- the plant's traction equipment receives the commanded newtons whatever the plant weighs.
 * Speed trajectory.  With a plant (msd_mpc_rolling_stock) it is the plant's: one kernel per advance does state and account together, and time, speed, plant
 * states and stall flags come out bit for bit as without the account; a stall ends the leg in front of the interval that stalled it, and what was spent up to
 * there counts.  Without a plant the plan is the plant: an account kernel runs next to the advance, every interval restarts from the plan's own b_i and is
 * integrated with the model's Davis coefficients (what the reference's post-processing does per interval), and the state at the end is the plan's node, read.
 * Per interval, summed over the intervals completed:  traction = ds max(F_el, 0), regenerated = ds min(F_el, 0), pnBrake = ds F_pn, and losses --
 *   eta given ([nscen][2]: etaTraction, etaRgBrake of the PLANT, which need not be the model's) or loss_kind 1: ds (ct max(F, 0) + cr max(-F, 0)), ct = (1 - eta_t)/eta_t,
 *     cr = 1 - eta_r (closed form: the speed cancels, train.py:199-212);
 *   loss_kind 2 without eta: the integral of L(F_el, v)/v over the interval as a third component of the Runge-Kutta steps of the trajectory (`steps` per interval),
 *     k_E(x) = ds L(F, sqrt(x))/sqrt(x) at the four stage values of b, L the loop's own copy of the loss table with the scenario's total mass;
 *   loss_kind 0 without eta: 0.
 * A scenario that is not advanced (its re-solve failed, or it stalled in an earlier leg) has a zero record with 0 intervals.
 *
 * The account is state of the loop exactly like restrictions and rolling stock: every msd_mpc_run with exactly nscen scenarios keeps it; nscen = 0 clears it
 * (the other arguments are ignored); a run with another count returns MSD_E_INVALID and enqueues nothing; a refused call leaves the previous state in place; the
 * count must agree with those of the restrictions and the rolling stock the loop holds (the later call is refused otherwise).  steps: the plant's plant_steps where
 * the loop holds a plant (it must equal it, at the call and at the run), 1 ... 64 otherwise.  Without the account the loop launches exactly what it launched
 * before this entry point existed.  Nothing is waited for and nothing crosses PCIe inside the loop.
 *
 * MSD_E_INVALID: a null handle; nscen < 0; total_mass not finite or <= 0; an efficiency outside (0, 1]; steps out of range or other than the plant's; a count other
 * than that of the restrictions or rolling stock the loop holds; records asked for before a run under the account.
 */
enum { MSD_MPC_EN_TRACTION = 0, MSD_MPC_EN_REGENERATED, MSD_MPC_EN_PNBRAKE, MSD_MPC_EN_LOSSES,   /* kWh */
       MSD_MPC_EN_T, MSD_MPC_EN_V,          /* state at the end of the leg, before the noise */
       MSD_MPC_EN_INTERVALS,                /* intervals completed in this leg */
       MSD_MPC_EN_COUNT };
int msd_mpc_energy(msd_mpc_handle m, int nscen, double total_mass, const double *eta /* [nscen][2] or NULL */, int steps);

/* The account of every leg of the last run: records[K][nscen][MSD_MPC_EN_COUNT] (host); record K-1 is the final leg, whose MSD_MPC_EN_T / _V are the arrival:
 * the plant's with a plant, the plan's t_N and sqrt(b_N) without one.  MSD_E_INVALID: the loop keeps no account, or has not run under it yet. */
int msd_mpc_energy_records(msd_mpc_handle m, double *records /* [K][nscen][MSD_MPC_EN_COUNT], host */);

#ifdef __cplusplus
}
#endif
#endif
