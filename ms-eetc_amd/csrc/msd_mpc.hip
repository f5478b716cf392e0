/*
 * msd_mpc.hip -- the shrinking-horizon loop of BASELINE config 4 with its bookkeeping on the device (include/mseetc_mpc.h).
 *
 * Reference mechanism: Track.updateLimits(positionStart) (track.py:420-450) + casadiSolver on the cropped track + solve(T, initialTime,
 * initialVelocity) (ocp.py:310); mseetc/mpc.py: shrinkingHorizon is the host-side statement of the loop this file runs without the host.
 * One stream (the energy problem's handle), per re-solve:  scenario records from the measured state -> solve (first pass + follow-up kernel,
 * warm-started from the previous solutions and multipliers where the new grid is a tail of the old one; one attempt per scenario when the loop
 * relaxes infeasible arrival times: WarmStart::one_attempt) -> failed scenarios collected in a list -> their minimum running times from the
 * time-optimal twin (complete kernel launched on the list) -> arrival times of the late ones moved, list re-solved (up to three times with
 * growing margins; what the twin does not declare late is on the first of these lists too, arrival time unchanged, and gets both attempts
 * there) -> log -> measured state for the next re-solve.  Every launch is unconditional; the
 * kernels launched on an empty list return at once.
 * Under speed restrictions (msd_mpc_speed_restrictions) one more kernel in front of the scenario records builds the re-solve's rows of limits and the caps of the
 * end speeds from the records known by then; every launch of the re-solve, the twin's included, runs under the rows.
 * Under rolling stock of their own (msd_mpc_rolling_stock) every launch of a re-solve takes the scenarios' override rows (the twin's with its own objective
 * scaling, written per re-solve by mpc_twin_scaling), and with a plant mpc_plant stands where mpc_advance stood: the measured state comes from the plant
 * integrated under the planned forces, not from the plan.
 * Under the energy account (msd_mpc_energy) mpc_energy keeps the kWh of every leg: with a plant it stands where mpc_plant stood (state and account in one
 * launch), without one it runs next to mpc_advance; behind the last re-solve's log it runs once more over the whole last plan.
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "msd_handle.hpp"
#include "../../include/mseetc_mpc.h"

using msd_host::fail;

namespace {

constexpr int HDR = msd::FOLLOW_HDR;
constexpr int RING = 64;

__global__ void mpc_begin(int B, const double *T_in, double t0, double v0, double *T, double *tnow, double *vnow, int *flag)
{
    const int s = blockIdx.x*blockDim.x + threadIdx.x;
    if (s >= B) return;
    T[s] = T_in[s]; tnow[s] = t0; vnow[s] = v0; flag[s] = 0;
}

/* scenario records (t0, T, v0^2, vN^2) with the clipping of ocp.py:343-344 (mseetc/ocp.py: _scenarios), log of the measured state */
__device__ __forceinline__ void scen_record(int s, const double *T, const double *tnow, const double *vnow, double vmin, double vlim0, double vNsq, double *scen, double *log)
{
    const double v0 = fmin(fmax(vnow[s], vmin), vlim0);
    double *q = scen + (size_t)MSD_SC_COUNT*s;
    q[MSD_SC_T0] = tnow[s]; q[MSD_SC_TEND] = T[s]; q[MSD_SC_V0SQ] = v0*v0; q[MSD_SC_VNSQ] = vNsq;
    double *l = log + (size_t)MSD_MPC_COUNT*s;
    l[MSD_MPC_T0] = tnow[s]; l[MSD_MPC_V0] = vnow[s]; l[MSD_MPC_RELAXED] = 0.0;
}

__global__ void mpc_scen(int B, const double *T, const double *tnow, const double *vnow, double vmin, double vlim0, double vNsq, double *scen, double *log)
{
    const int s = blockIdx.x*blockDim.x + threadIdx.x;
    if (s >= B) return;
    scen_record(s, T, tnow, vnow, vmin, vlim0, vNsq, scen, log);
}

/* ... under speed restrictions (msd_mpc_speed_restrictions): the end speeds clipped per scenario to the caps mpc_limit_rows wrote, caps[2 s] for the measured speed
 * (the restricted limit of the first interval), caps[2 s + 1] for the terminal speed (that of the last interval) */
__global__ void mpc_scen_caps(int B, const double *T, const double *tnow, const double *vnow, double vmin, const double *caps, double *scen, double *log)
{
    const int s = blockIdx.x*blockDim.x + threadIdx.x;
    if (s >= B) return;
    const double vN = caps[2*s + 1];
    scen_record(s, T, tnow, vnow, vmin, caps[2*s], __dmul_rn(vN, vN), scen, log);
}

/*
 * Rows of speed limits of re-solve k and the two speed caps per scenario from the loop's restriction records (the rule of include/mseetc_mpc.h: limit_rows_kernel of
 * msd_api.hip on grid k, for the records known by re-solve k, moved into the coordinates of the grid by one rounded subtraction each).  The geometry is that
 * kernel's: one workgroup per scenario, threads strided over the nodes; the scenario's records are the same for every thread (scalar loads), the row is stored
 * coalesced.  v*v is one rounded product, the host rule's (mseetc/ocp.py: restrictedLimits).  A record that lies behind the train restricts no interval.
 *   records [nscen][max_per][MSD_MPC_RS_COUNT], count [nscen], bmax / pos [N+1] of grid k, rows [nscen][N+1], caps [nscen][2]
 */
__global__ void __launch_bounds__(256) mpc_limit_rows(int N, int max_per, int k, double origin, const double *bmax, const double *pos, const double *records, const int *count,
                                                      double vlim0, double vN, double *rows, double *caps)
{
    const int s = blockIdx.x;
    const int n = count[s];
    const double *rec = records + (size_t)MSD_MPC_RS_COUNT*max_per*s;
    double *row = rows + (size_t)(N + 1)*s;
    for (int i = threadIdx.x; i <= N; i += blockDim.x) {
        double b = bmax[i];
        if (i >= 1 && i < N) {
            const double p0 = pos[i - 1], p1 = pos[i], p2 = pos[i + 1];
            for (int j = 0; j < n; j++) {
                const double *r = rec + MSD_MPC_RS_COUNT*j;
                if (r[3] > (double)k) continue;      /* (not announced yet) */
                const double begin = __dsub_rn(r[0], origin), end = __dsub_rn(r[1], origin), v = r[2];
                /* interval i-1 or interval i is restricted */
                if ((p0 < end && p1 > begin) || (p1 < end && p2 > begin)) b = fmin(b, __dmul_rn(v, v));
            }
        }
        row[i] = b;
    }
    if (threadIdx.x == 0) {
        double first = vlim0, last = vN;
        const double a0 = pos[0], a1 = pos[1], z0 = pos[N - 1], z1 = pos[N];
        for (int j = 0; j < n; j++) {
            const double *r = rec + MSD_MPC_RS_COUNT*j;
            if (r[3] > (double)k) continue;
            const double begin = __dsub_rn(r[0], origin), end = __dsub_rn(r[1], origin), v = r[2];
            if (a0 < end && a1 > begin) first = fmin(first, v);
            if (z0 < end && z1 > begin) last = fmin(last, v);
        }
        caps[2*s] = first; caps[2*s + 1] = last;
    }
}

/* failed re-solves: into the list of the twin's launch, with a running time the twin can certainly meet (mseetc/ocp.py: minimumTime) */
__global__ void mpc_collect(int B, const double *stats, const double *scen, double loose, int *flag, int *list, double *scen_tw)
{
    const int s = blockIdx.x*blockDim.x + threadIdx.x;
    if (s >= B) return;
    const bool bad = stats[(size_t)MSD_ST_COUNT*s + MSD_ST_STATUS] < 0;
    flag[s] = bad ? 1 : 0;
    if (!bad) return;
    const double *q = scen + (size_t)MSD_SC_COUNT*s;
    double *w = scen_tw + (size_t)MSD_SC_COUNT*s;
    w[MSD_SC_T0] = q[MSD_SC_T0]; w[MSD_SC_TEND] = __dadd_rn(q[MSD_SC_T0], fmax(loose, __dmul_rn(3.0, q[MSD_SC_TEND] - q[MSD_SC_T0])));
    w[MSD_SC_V0SQ] = q[MSD_SC_V0SQ]; w[MSD_SC_VNSQ] = q[MSD_SC_VNSQ];
    const int k = atomicAdd(list, 1);
    list[HDR + 2*k] = s; list[HDR + 2*k + 1] = -1;
}

/*
 * attempt 0: a failed scenario whose minimum running time (twin) exceeds what its arrival time leaves is late: the arrival time moves to
 * t0 + tmin (1 + margin) and the scenario is solved again; the others keep their failure.  attempt > 0: a moved scenario that still fails
 * gets the next margin.  (mseetc/mpc.py: shrinkingHorizon, relaxInfeasible)
 */
__global__ void mpc_relax(int B, int attempt, const double *stats, const double *z_tw, int nz_tw, const double *st_tw, double *T, const double *tnow, double *tm,
                          int *flag, int *list, double *scen, double margin, double *log)
{
    const int s = blockIdx.x*blockDim.x + threadIdx.x;
    if (s >= B) return;
    bool again = false;
    if (attempt == 0) {
        if (flag[s] != 1) return;
        /* usable: the twin converged -- or it ended without converging on a feasible point NEXT TO its optimum: far down the central path (mu <= 1e-5) or
         * with an optimality error of 1e-4 (its primal point settles long before its multipliers do where both brakes share an active acceleration bound).
         * Round 6: feasibility alone is not enough.  The twin is given three times the running time asked for and its profile start uses that
         * time up, so a twin that breaks down EARLY sits on a feasible point whose time says nothing about the minimum: the scenario was declared late and
         * its arrival time moved by up to a factor of three although it may be feasible.  Such a scenario now keeps its arrival time and is solved again
         * with both attempts (flag 3).  The log tells the two kinds of verdict apart: 1 converged twin, 2 twin next to its optimum
         * (mseetc/ocp.py: minimumTime restates the rule) */
        const double *stw = st_tw + (size_t)MSD_ST_COUNT*s;
        const double viol = stw[MSD_ST_CONSTR_VIOL];
        const bool conv = stw[MSD_ST_STATUS] >= 0;
        const bool ok = conv || (isfinite(viol) && viol <= 1e-6 && (stw[MSD_ST_MU] <= 1e-5 || stw[MSD_ST_KKT] <= 1e-4));
        const double tmin = z_tw[(size_t)nz_tw*s + nz_tw - 2] - tnow[s];
        if (ok && tmin > T[s] - tnow[s]) { tm[s] = tmin; flag[s] = 2; again = true; log[(size_t)MSD_MPC_COUNT*s + MSD_MPC_RELAXED] = conv ? 1.0 : 2.0; }
        else {
            /* not late: the breakdown was the solver's.  The main launch makes one attempt per scenario (a late scenario would spend its second one, from
             * the other starting point, on a problem without a solution -- nine of 512 per re-solve, a third of the loop's time in round 4); the ones
             * the twin clears get both here, from the problem's own starting point, with their arrival time unchanged */
            flag[s] = 3;
            const int k = atomicAdd(list, 1);
            list[HDR + 2*k] = s; list[HDR + 2*k + 1] = -1;
            return;
        }
    } else {
        if (flag[s] != 2) return;
        if (stats[(size_t)MSD_ST_COUNT*s + MSD_ST_STATUS] < 0) again = true; else flag[s] = 0;
    }
    if (!again) return;
    T[s] = __dadd_rn(tnow[s], __dmul_rn(tm[s], 1 + margin));      /* (no contraction: the host loop's arithmetic, bit for bit) */
    scen[(size_t)MSD_SC_COUNT*s + MSD_SC_TEND] = T[s];
    const int k = atomicAdd(list, 1);
    list[HDR + 2*k] = s; list[HDR + 2*k + 1] = -1;
}

__global__ void mpc_log(int B, const double *stats, const double *T, double *log)
{
    const int s = blockIdx.x*blockDim.x + threadIdx.x;
    if (s >= B) return;
    const double *st = stats + (size_t)MSD_ST_COUNT*s;
    double *l = log + (size_t)MSD_MPC_COUNT*s;
    l[MSD_MPC_T] = T[s]; l[MSD_MPC_STATUS] = st[MSD_ST_STATUS]; l[MSD_MPC_ITERS] = st[MSD_ST_ITERS]; l[MSD_MPC_OBJ] = st[MSD_ST_OBJ];
}

/* the train advances `stride` intervals: time and speed at that node of the solution, perturbed; a failed scenario keeps its last measurement */
__global__ void mpc_advance(int B, const double *z, int nz, const double *stats, int off_t, int off_b, double noise, const double *n1, const double *n2,
                            double *tnow, double *vnow)
{
    const int s = blockIdx.x*blockDim.x + threadIdx.x;
    if (s >= B) return;
    if (stats[(size_t)MSD_ST_COUNT*s + MSD_ST_STATUS] < 0) return;
    const double t = z[(size_t)nz*s + off_t], v = sqrt(z[(size_t)nz*s + off_b]);
    tnow[s] = fmax(__dmul_rn(t, __dadd_rn(1.0, __dmul_rn(noise, n1[s]))), 0.0);      /* (no contraction: the host loop's arithmetic, bit for bit) */
    vnow[s] = __dmul_rn(v, __dadd_rn(1.0, __dmul_rn(noise, n2[s])));
}

/* the twin's rows of rolling stock: the model rows with MSD_OV_OBJ_DEN = the objective scaling of the twin of this re-solve (ocp.py:282: a constant of the twin's
 * problem, not a function of the mass -- mseetc/ocp.py: minimumTime does the same per call) */
__global__ void mpc_twin_scaling(int B, double obj_den, double *ovr_tw)
{
    const int s = blockIdx.x*blockDim.x + threadIdx.x;
    if (s >= B) return;
    ovr_tw[(size_t)MSD_OV_COUNT*s + MSD_OV_OBJ_DEN] = obj_den;
}

/*
 * The plant advances `stride` intervals (msd_mpc_rolling_stock; mseetc/mpc.py: plantAdvance is the host statement): from the re-solve's own initial state (its
 * scenario record) under the planned forces of its solution, interval by interval through the solver's explicit Runge-Kutta map with the plant's Davis
 * coefficients, `steps` steps per interval, the time integrated with the same stages.  One lane per scenario.  P: the re-solve's problem record (by value; its
 * profile pointers are read for the first `stride` intervals, stride < N).  The noise is mpc_advance's.  A scenario that stalls, has stalled or whose re-solve
 * failed keeps its last measurement.
 *   plant [B][MSD_MPC_PL_COUNT], stalled [B], ps [B][MSD_MPC_PS_COUNT] (the record of this advance)
 */
__global__ void mpc_plant(msd::DevProb P, int B, int stride, int steps, const double *z, int nz, const double *stats, const double *scen, const double *plant, double noise,
                          const double *n1, const double *n2, double *tnow, double *vnow, int *stalled, double *ps)
{
    const int s = blockIdx.x*blockDim.x + threadIdx.x;
    if (s >= B) return;
    double *rec = ps + (size_t)MSD_MPC_PS_COUNT*s;
    if (stalled[s] || stats[(size_t)MSD_ST_COUNT*s + MSD_ST_STATUS] < 0) {
        rec[MSD_MPC_PS_T] = tnow[s]; rec[MSD_MPC_PS_V] = vnow[s]; rec[MSD_MPC_PS_STALLED] = stalled[s] ? 1.0 : 0.0;
        return;
    }
    const double *pr = plant + (size_t)MSD_MPC_PL_COUNT*s;
    msd::DevProb Pp = P;
    Pp.sr0 = pr[MSD_MPC_PL_SR0]; Pp.sr1 = pr[MSD_MPC_PL_SR1]; Pp.sr2 = pr[MSD_MPC_PL_SR2];
    Pp.numSteps = steps; Pp.numApprox = 0;
    const double scale = pr[MSD_MPC_PL_FORCE_SCALE];
    const int stp = 4 + P.withPn;
    const double *zs = z + (size_t)nz*s;
    double t = scen[(size_t)MSD_SC_COUNT*s + MSD_SC_T0], b = scen[(size_t)MSD_SC_COUNT*s + MSD_SC_V0SQ];
    bool stall = false;
    for (int i = 0; i < stride; i++) {
        const double w = (zs[stp*i] + (P.withPn ? zs[stp*i + 1] : 0.0))*scale;
        double tau, bp;
        msd::interval_map<double>(Pp, b, w, msd::track_resistance(Pp, P.grad[i], P.curv[i]), P.ds[i], tau, bp);
        if (!(bp >= P.vminSq) || !isfinite(tau)) { stall = true; break; }      /* (a NaN fails the comparison) */
        t += tau; b = bp;
    }
    const double v = sqrt(b);
    rec[MSD_MPC_PS_T] = t; rec[MSD_MPC_PS_V] = v; rec[MSD_MPC_PS_STALLED] = stall ? 1.0 : 0.0;
    if (stall) { stalled[s] = 1; return; }
    tnow[s] = fmax(__dmul_rn(t, __dadd_rn(1.0, __dmul_rn(noise, n1[s]))), 0.0);      /* (mpc_advance's arithmetic) */
    vnow[s] = __dmul_rn(v, __dadd_rn(1.0, __dmul_rn(noise, n2[s])));
}

/* the loss integral of one interval [Nm]: d(E)/d(sigma) = ds L(F, sqrt(b))/sqrt(b) as a third component of the Runge-Kutta steps of interval_map's joint branch
 * (numSteps steps, the same stage values of b), L [W] = the specific losses of the table times the scenario's total mass.  With a plant the b trajectory of an
 * interval is therefore integrated twice: here for the stages of E, and by interval_map for the state, whose bits must be mpc_plant's.  The stage arithmetic below
 * restates that branch of interval_map (msd_kernel.hpp: numApprox == 0); should it change there, it changes here -- the statement (mseetc/mpc.py: _plantEnergy)
 * integrates b, t and E jointly, and tests/test_mpc_energy_gpu.py holds the table losses to it at rounding level */
__device__ __forceinline__ double loss_integral(const msd::DevProb &Pp, const msd::DynLoss &D, double b, double w, double f, double G, double ds)
{
    const bool traction = f >= 0;
    const auto ke = [&](double x) { const double v = sqrt(x); return ds*(msd::spec_losses(D, traction, f, v).v*D.M)/v; };
    const double h = 1.0/Pp.numSteps;
    double E = 0;
    for (int s = 0; s < Pp.numSteps; s++) {
        const double k1b = msd::ode_b(Pp, b, w, G, ds), k1e = ke(b);
        const double b2 = b + k1b*(0.5*h);
        const double k2b = msd::ode_b(Pp, b2, w, G, ds), k2e = ke(b2);
        const double b3 = b + k2b*(0.5*h);
        const double k3b = msd::ode_b(Pp, b3, w, G, ds), k3e = ke(b3);
        const double b4 = b + k3b*h;
        const double k4b = msd::ode_b(Pp, b4, w, G, ds), k4e = ke(b4);
        b = b + ((k1b + k2b*2.0) + (k3b*2.0 + k4b))*(h/6);
        E = E + ((k1e + k2e*2.0) + (k3e*2.0 + k4e))*(h/6);
    }
    return E;
}

/*
 * The energy account of one leg (msd_mpc_energy; mseetc/mpc.py: plantEnergy is the host statement): the first n intervals of the re-solve's solutions, one lane per
 * scenario.  plant != null: the trajectory is the plant's, integrated exactly as mpc_plant integrates it -- and with `advance` this kernel stands where mpc_plant
 * stood: it writes the record of the advance, the stall flag and the measured state as well (bit for bit mpc_plant's).  plant == null: the plan is the plant, every
 * interval restarts from the plan's own b_i under the model's Davis coefficients (the scenario's row of `ovr`, or the problem's), the state at the end is the
 * plan's node n.  advance == 0 (the final leg, n = N; any leg without a plant): nothing but the account is written.
 *   coef [B][2] (ct, cr of the plants' own efficiencies) or null: the problem's loss model; en [B][MSD_MPC_EN_COUNT] (the record of this leg)
 */
__global__ void mpc_energy(msd::DevProb P, int B, int n, int steps, const double *z, int nz, const double *stats, const double *scen, const double *ovr, const double *plant,
                           const double *coef, double total_mass, int advance, double noise, const double *n1, const double *n2, double *tnow, double *vnow, int *stalled,
                           double *ps, double *en)
{
    const int s = blockIdx.x*blockDim.x + threadIdx.x;
    if (s >= B) return;
    double *e = en + (size_t)MSD_MPC_EN_COUNT*s;
    double *rec = advance ? ps + (size_t)MSD_MPC_PS_COUNT*s : nullptr;
    const bool was = plant && stalled[s];
    if (was || stats[(size_t)MSD_ST_COUNT*s + MSD_ST_STATUS] < 0) {
        if (advance) { rec[MSD_MPC_PS_T] = tnow[s]; rec[MSD_MPC_PS_V] = vnow[s]; rec[MSD_MPC_PS_STALLED] = was ? 1.0 : 0.0; }
        for (int j = 0; j < MSD_MPC_EN_COUNT; j++) e[j] = 0.0;      /* (not advanced: a zero record with 0 intervals) */
        return;
    }
    const double *row = ovr ? ovr + (size_t)MSD_OV_COUNT*s : nullptr;
    const double M = (row && row[MSD_OV_TOTAL_MASS] != 0) ? row[MSD_OV_TOTAL_MASS] : total_mass;
    msd::DevProb Pp = P;
    double scale = 1.0;
    if (plant) {
        const double *pr = plant + (size_t)MSD_MPC_PL_COUNT*s;
        Pp.sr0 = pr[MSD_MPC_PL_SR0]; Pp.sr1 = pr[MSD_MPC_PL_SR1]; Pp.sr2 = pr[MSD_MPC_PL_SR2];
        scale = pr[MSD_MPC_PL_FORCE_SCALE];
    } else if (row) { Pp.sr0 = row[MSD_OV_SR0]; Pp.sr1 = row[MSD_OV_SR1]; Pp.sr2 = row[MSD_OV_SR2]; }
    Pp.numSteps = steps; Pp.numApprox = 0;
    const int kind = coef ? 1 : P.lossKind;
    const double ct = coef ? coef[2*s] : P.ct, cr = coef ? coef[2*s + 1] : P.cr;
    const int stp = 4 + P.withPn;
    const double *zs = z + (size_t)nz*s;
    double t = scen[(size_t)MSD_SC_COUNT*s + MSD_SC_T0], b = scen[(size_t)MSD_SC_COUNT*s + MSD_SC_V0SQ];
    double tr = 0, rg = 0, pb = 0, ls = 0;
    bool stall = false;
    int done = 0;
    for (int i = 0; i < n; i++) {
        const double fel = zs[stp*i], fpb = P.withPn ? zs[stp*i + 1] : 0.0;
        const double F = fel*M, ds = P.ds[i];
        double E = 0;
        if (plant || kind == 2) {
            const double w = (fel + fpb)*scale, G = msd::track_resistance(Pp, P.grad[i], P.curv[i]);
            const double b0 = plant ? b : zs[stp*i + stp - 1];
            if (kind == 2) { const msd::DynLoss D(P.loss, P.lossCoef, M); E = loss_integral(Pp, D, b0, w, fel, G, ds); }
            if (plant) {
                double tau, bp;
                msd::interval_map<double>(Pp, b, w, G, ds, tau, bp);
                if (!(bp >= P.vminSq) || !isfinite(tau)) { stall = true; break; }      /* (mpc_plant's rule) */
                t += tau; b = bp;
            }
        }
        if (kind == 1) E = ds*(ct*fmax(F, 0.0) + cr*fmax(-F, 0.0));
        tr += ds*fmax(F, 0.0); rg += ds*fmin(F, 0.0); pb += ds*(fpb*M); ls += E;
        done++;
    }
    if (!plant) { const int node = stp*n + (n < P.N ? stp - 2 : 0); t = zs[node]; b = zs[node + 1]; }
    const double v = sqrt(b), kwh = 1e-6/3.6;
    e[MSD_MPC_EN_TRACTION] = tr*kwh; e[MSD_MPC_EN_REGENERATED] = rg*kwh; e[MSD_MPC_EN_PNBRAKE] = pb*kwh; e[MSD_MPC_EN_LOSSES] = ls*kwh;
    e[MSD_MPC_EN_T] = t; e[MSD_MPC_EN_V] = v; e[MSD_MPC_EN_INTERVALS] = (double)done;
    if (!advance) return;
    rec[MSD_MPC_PS_T] = t; rec[MSD_MPC_PS_V] = v; rec[MSD_MPC_PS_STALLED] = stall ? 1.0 : 0.0;
    if (stall) { stalled[s] = 1; return; }
    tnow[s] = fmax(__dmul_rn(t, __dadd_rn(1.0, __dmul_rn(noise, n1[s]))), 0.0);      /* (mpc_advance's arithmetic) */
    vnow[s] = __dmul_rn(v, __dadd_rn(1.0, __dmul_rn(noise, n2[s])));
}

}  // namespace

struct msd_mpc {
    msd_problem *h = nullptr, *twin = nullptr;
    int K = 0, stride = 0;
    std::vector<msd_host::Plan> pl, tw;
    std::vector<double> vlim0, length;
    std::vector<unsigned char> tail;
    double vmin = 1, vmax = 1, vN = 1, wmu = 0, wpush = 0, noise = 0, margin = 0;
    int warm = 0, relax = 0;
    double *d_prof = nullptr, *d_work = nullptr;
    double *d_tables = nullptr;       /* the loop's own copies of the loss table and the collocation tables of its problems and of their twins: the handles may be
                                       * reconfigured (which frees and regrows theirs) while the loop exists */
    int *d_ints = nullptr;            /* queue ring | follow | follow (twin) | list A | list B | flags */
    int *d_queue = nullptr, *d_follow = nullptr, *d_follow_tw = nullptr, *d_listA = nullptr, *d_listB = nullptr, *d_flag = nullptr;
    int queue_slot = 0;
    double *d_buf = nullptr;          /* every per-scenario array of a run, carved below */
    double *d_Tin = nullptr, *d_T = nullptr, *d_tnow = nullptr, *d_vnow = nullptr, *d_tm = nullptr, *d_scen = nullptr, *d_scen_tw = nullptr, *d_z[2] = {nullptr, nullptr},
           *d_st[2] = {nullptr, nullptr}, *d_dual[2] = {nullptr, nullptr}, *d_ztw = nullptr, *d_sttw = nullptr, *d_log = nullptr, *d_n1 = nullptr, *d_n2 = nullptr;
    double *d_zlog = nullptr; size_t cap_zlog = 0;
    int cap = 0;
    int nz_max = 0, nz_tw_max = 0, nodes_max = 0;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    /* speed restrictions (msd_mpc_speed_restrictions): the records as uploaded (counts behind them), the rows and caps of the re-solve under way; rs_nscen scenarios
     * have records (0: none) and only a run of exactly that many is accepted */
    double *d_rs = nullptr, *d_rows = nullptr, *d_caps = nullptr;
    size_t cap_rs = 0, cap_rows = 0;      /* bytes of d_rs, scenarios of d_rows / d_caps */
    int rs_nscen = 0, rs_max = 0;
    std::vector<double> origin;           /* [K] route coordinate of the first node of grid k */
    double last0 = 0;                     /* position of the last node of grid 0 (the checks of the records) */
    /* rolling stock (msd_mpc_rolling_stock), one buffer: model rows | the twin's copy of them | plant rows | plant states [K-1][nscen] | stalled flags (ints);
     * ro_nscen scenarios have records (0: none) and only a run of exactly that many is accepted */
    double *d_ro = nullptr, *d_ovr = nullptr, *d_ovr_tw = nullptr, *d_plant = nullptr, *d_ps = nullptr;
    int *d_stalled = nullptr;
    int cap_ro = 0;                       /* scenarios of d_ro */
    int ro_nscen = 0, plant_steps = 0;
    bool ro_model = false, ro_plant = false;
    int ps_nscen = 0;                     /* scenarios of the plant states the last run left (0: none) */
    /* energy account (msd_mpc_energy), one buffer: ct, cr of the plants' own efficiencies [nscen][2] | records [K][nscen][MSD_MPC_EN_COUNT]; en_nscen scenarios are
     * accounted for (0: no account) and only a run of exactly that many is accepted */
    double *d_en = nullptr, *d_en_rec = nullptr;
    int cap_en = 0;                       /* scenarios of d_en */
    int en_nscen = 0, en_steps = 0;
    bool en_eta = false;
    double en_mass = 0;
    int en_run = 0;                       /* scenarios of the records the last run left (0: none) */
};

/* the rows and caps of re-solve k under the loop's records, on `st` */
static void launch_rows(msd_mpc *m, int k, hipStream_t st)
{
    const msd_host::Plan &pl = m->pl[k];
    const int N = pl.P.N;
    const size_t rec_doubles = (size_t)MSD_MPC_RS_COUNT*m->rs_max*m->rs_nscen;
    hipLaunchKernelGGL(mpc_limit_rows, dim3(m->rs_nscen), dim3(N + 1 < 256 ? 64*((N + 64)/64) : 256), 0, st, N, m->rs_max, k, m->origin[k], pl.P.bmax, pl.P.pos,
                       (const double *)m->d_rs, (const int *)(m->d_rs + rec_doubles), m->vlim0[k], m->vN, m->d_rows, m->d_caps);
}

extern "C" {

int msd_mpc_destroy(msd_mpc_handle m)
{
    if (!m) return MSD_OK;
    if (m->h) { hipSetDevice(m->h->device); hipStreamSynchronize(m->h->stream); m->h->attached_loops--; }
    if (m->twin) m->twin->attached_loops--;
    hipFree(m->d_prof); hipFree(m->d_work); hipFree(m->d_tables); hipFree(m->d_ints); hipFree(m->d_buf); hipFree(m->d_zlog);
    hipFree(m->d_rs); hipFree(m->d_rows); hipFree(m->d_ro); hipFree(m->d_en);
    if (m->e0) hipEventDestroy(m->e0);
    if (m->e1) hipEventDestroy(m->e1);
    delete m;
    return MSD_OK;
}

int msd_mpc_create(msd_handle h, msd_handle twin, const msd_mpc_plan *plan, msd_mpc_handle *out)
{
    if (!h || !plan || !out || plan->num_resolves < 1 || plan->stride < 1 || !plan->problems || !plan->vlim_first || !plan->length || !plan->tail)
        return fail(MSD_E_INVALID, "bad argument");
    if ((plan->twins != nullptr) != (twin != nullptr)) return fail(MSD_E_INVALID, "the time-optimal twins need a handle of their own (and only they)");
    if (plan->relax_infeasible && !plan->twins) return fail(MSD_E_INVALID, "relax_infeasible needs the time-optimal twins");
    if (twin && twin->device != h->device) return fail(MSD_E_INVALID, "both handles must live on one device");
    if (plan->warm_start && (!(plan->warm_mu > 0) || !(plan->warm_mu <= 1e3) || !(plan->warm_push > 0) || !(plan->warm_push <= 0.5)))
        return fail(MSD_E_INVALID, "warm start needs 0 < mu_init <= 1e3 and 0 < bound_push <= 0.5");
    HIP_TRY(hipSetDevice(h->device));
    msd_mpc *m = new msd_mpc();
    m->h = h; m->twin = twin; m->K = plan->num_resolves; m->stride = plan->stride;
    h->attached_loops++;      /* (the loop runs on the handle's stream: msd_problem_destroy refuses while a loop is attached) */
    if (twin) twin->attached_loops++;
    m->vmin = plan->vmin; m->vmax = plan->vmax_train; m->vN = plan->terminal_velocity; m->warm = plan->warm_start; m->wmu = plan->warm_mu; m->wpush = plan->warm_push;
    m->noise = plan->noise; m->relax = plan->relax_infeasible; m->margin = plan->late_margin;
    m->pl.resize(m->K); m->tw.resize(twin ? m->K : 0);
    m->vlim0.assign(plan->vlim_first, plan->vlim_first + m->K); m->length.assign(plan->length, plan->length + m->K); m->tail.assign(plan->tail, plan->tail + m->K);
    size_t prof = 0, work = 0;
    int rc = MSD_OK;
    for (int k = 0; k < m->K && rc == MSD_OK; k++) {
        const msd_problem_desc *d = plan->problems + k;
        rc = msd_host::check_desc(d);
        if (rc == MSD_OK && k > 0 && d->num_intervals != plan->problems[k - 1].num_intervals - m->stride) rc = fail(MSD_E_INVALID, "problem k + 1 must have `stride` intervals fewer than problem k");
        if (rc == MSD_OK && k > 0 && (d->loss_kind != plan->problems[0].loss_kind || d->integrator != plan->problems[0].integrator || d->loss_table_len != plan->problems[0].loss_table_len
                                       || (d->integrator == MSD_INTEGRATOR_COLLOCATION && d->coll_degree != plan->problems[0].coll_degree)))
            rc = fail(MSD_E_INVALID, "the problems of a loop share their loss model and integrator");
        if (rc == MSD_OK) rc = msd_host::make_plan(h->device, d, &m->pl[k]);
        if (rc == MSD_OK && twin) {
            const msd_problem_desc *t = plan->twins + k;
            rc = msd_host::check_desc(t);
            if (rc == MSD_OK && t->num_intervals != d->num_intervals) rc = fail(MSD_E_INVALID, "a twin shares the grid of its problem");
            if (rc == MSD_OK && k > 0 && (t->loss_kind != plan->twins[0].loss_kind || t->integrator != plan->twins[0].integrator)) rc = fail(MSD_E_INVALID, "the twins of a loop share their loss model and integrator");
            if (rc == MSD_OK) rc = msd_host::make_plan(h->device, t, &m->tw[k]);
        }
        if (rc != MSD_OK) break;
        prof += msd_host::profile_doubles(d->num_intervals);
        work = std::max(work, std::max(m->pl[k].work_area(), twin ? m->tw[k].work_area() : (size_t)0));
        m->nz_max = std::max(m->nz_max, m->pl[k].nz); m->nodes_max = std::max(m->nodes_max, d->num_intervals + 1);
        if (twin) m->nz_tw_max = std::max(m->nz_tw_max, m->tw[k].nz);
    }
    if (rc != MSD_OK) { msd_mpc_destroy(m); return rc; }
    /* every profile in one buffer: ds | grad | curv | bmax | pos per re-solve (the twin shares the grid of its problem) */
    std::vector<double> stage(prof);
    if (hipMalloc((void **)&m->d_prof, sizeof(double)*prof) != hipSuccess || hipMalloc((void **)&m->d_work, sizeof(double)*work) != hipSuccess
        || hipEventCreate(&m->e0) != hipSuccess || hipEventCreate(&m->e1) != hipSuccess) { msd_mpc_destroy(m); return fail(MSD_E_HIP, "device allocation failed"); }
    size_t off = 0;
    for (int k = 0; k < m->K; k++) {
        const msd_problem_desc *d = plan->problems + k;
        msd_host::pack_profile(d, stage.data() + off);
        if (k == 0) m->last0 = stage[off + msd_host::profile_doubles(d->num_intervals) - 1];
        msd_host::point_profile(m->pl[k].P, m->d_prof + off);
        if (twin) msd_host::point_profile(m->tw[k].P, m->d_prof + off);
        off += msd_host::profile_doubles(d->num_intervals);
    }
    if (hipMemcpy(m->d_prof, stage.data(), sizeof(double)*prof, hipMemcpyHostToDevice) != hipSuccess) { msd_mpc_destroy(m); return fail(MSD_E_HIP, "profile upload failed"); }
    {
        /* loss table and collocation tables: the loop's own copies, from the first problem's (and the first twin's) description -- the problems of a
         * loop share them (checked above).  Rounds 3-4 pointed at the handles' buffers, which msd_problem_reconfigure frees and regrows */
        const msd_problem_desc *d0 = plan->problems, *t0 = twin ? plan->twins : nullptr;
        auto loss_len = [](const msd_problem_desc *d) { return (d && d->loss_kind == 2) ? (size_t)d->loss_table_len : (size_t)0; };
        auto coll_len = [](const msd_problem_desc *d) { return (d && d->integrator == MSD_INTEGRATOR_COLLOCATION) ? (size_t)(d->coll_degree + 1)*(d->coll_degree + 2) : (size_t)0; };
        const size_t n[4] = {loss_len(d0), coll_len(d0), loss_len(t0), coll_len(t0)};
        const double *src[4] = {d0->loss_table, d0->coll_tables, t0 ? t0->loss_table : nullptr, t0 ? t0->coll_tables : nullptr};
        const size_t total = n[0] + n[1] + n[2] + n[3];
        const double *dev[4] = {nullptr, nullptr, nullptr, nullptr};
        if (total) {
            if (hipMalloc((void **)&m->d_tables, sizeof(double)*total) != hipSuccess) { msd_mpc_destroy(m); return fail(MSD_E_HIP, "device allocation failed"); }
            size_t o = 0;
            for (int a = 0; a < 4; a++) {
                if (!n[a]) continue;
                if (hipMemcpy(m->d_tables + o, src[a], sizeof(double)*n[a], hipMemcpyHostToDevice) != hipSuccess) { msd_mpc_destroy(m); return fail(MSD_E_HIP, "table upload failed"); }
                dev[a] = m->d_tables + o; o += n[a];
            }
        }
        for (int k = 0; k < m->K; k++) {
            m->pl[k].P.loss = dev[0]; m->pl[k].P.coll = dev[1];
            if (twin) { m->tw[k].P.loss = dev[2]; m->tw[k].P.coll = dev[3]; }
        }
    }
    *out = m;
    return MSD_OK;
}

int msd_mpc_nz(msd_mpc_handle m, int k) { return (m && k >= 0 && k < m->K) ? m->pl[k].nz : 0; }

static int grow(msd_mpc *m, int B, bool want_z)
{
    if (B > m->cap) {
        hipFree(m->d_buf); hipFree(m->d_ints); m->d_buf = nullptr; m->d_ints = nullptr; m->cap = 0;
        const size_t b = (size_t)B;
        const size_t dual = (size_t)MSD_DUAL_STRIDE*m->nodes_max*b;
        const size_t doubles = 5*b /* Tin T tnow vnow tm */ + 2*MSD_SC_COUNT*b + 2*(size_t)m->nz_max*b + 2*MSD_ST_COUNT*b + 2*dual + (size_t)std::max(m->nz_tw_max, 1)*b + MSD_ST_COUNT*b
                               + (size_t)MSD_MPC_COUNT*m->K*b + 2*(size_t)m->K*b;
        HIP_TRY(hipMalloc((void **)&m->d_buf, sizeof(double)*doubles));
        double *p = m->d_buf;
        m->d_Tin = p; p += b; m->d_T = p; p += b; m->d_tnow = p; p += b; m->d_vnow = p; p += b; m->d_tm = p; p += b;
        m->d_scen = p; p += MSD_SC_COUNT*b; m->d_scen_tw = p; p += MSD_SC_COUNT*b;
        for (int i = 0; i < 2; i++) { m->d_z[i] = p; p += (size_t)m->nz_max*b; }
        for (int i = 0; i < 2; i++) { m->d_st[i] = p; p += MSD_ST_COUNT*b; }
        for (int i = 0; i < 2; i++) { m->d_dual[i] = p; p += dual; }
        m->d_ztw = p; p += (size_t)std::max(m->nz_tw_max, 1)*b; m->d_sttw = p; p += MSD_ST_COUNT*b;
        m->d_log = p; p += (size_t)MSD_MPC_COUNT*m->K*b; m->d_n1 = p; p += (size_t)m->K*b; m->d_n2 = p; p += (size_t)m->K*b;
        const size_t list = HDR + 2*b;
        const size_t ints = RING + 4*list + b;
        HIP_TRY(hipMalloc((void **)&m->d_ints, sizeof(int)*ints));
        HIP_TRY(hipMemset(m->d_ints, 0, sizeof(int)*ints));
        int *q = m->d_ints;
        m->d_queue = q; q += RING; m->d_follow = q; q += list; m->d_follow_tw = q; q += list; m->d_listA = q; q += list; m->d_listB = q; q += list; m->d_flag = q;
        m->cap = B;
    }
    if (want_z) {
        size_t need = 0;
        for (int k = 0; k < m->K; k++) need += (size_t)m->pl[k].nz*B;
        if (need > m->cap_zlog) {
            hipFree(m->d_zlog); m->d_zlog = nullptr; m->cap_zlog = 0;
            HIP_TRY(hipMalloc((void **)&m->d_zlog, sizeof(double)*need));
            m->cap_zlog = need;
        }
    }
    return MSD_OK;
}

int msd_mpc_run(msd_mpc_handle m, int nscen, const double *T, double initial_time, double initial_velocity, const double *n1, const double *n2,
                double *log, double *z_log, float *loop_ms)
{
    if (!m || nscen < 1 || !T || (m->K > 1 && m->noise != 0 && (!n1 || !n2))) return fail(MSD_E_INVALID, "bad argument");
    if (!(initial_time >= 0)) return fail(MSD_E_INVALID, "Initial time must be a positive number!");
    const bool rs = m->rs_nscen != 0;
    if (rs && nscen != m->rs_nscen)
        return fail(MSD_E_INVALID, "the loop holds the speed restrictions of " + std::to_string(m->rs_nscen) + " scenarios, the run has " + std::to_string(nscen)
                                   + " (msd_mpc_speed_restrictions with nscen = 0 clears them)");
    const bool ro = m->ro_nscen != 0;
    if (ro && nscen != m->ro_nscen)
        return fail(MSD_E_INVALID, "the loop holds the rolling stock of " + std::to_string(m->ro_nscen) + " scenarios, the run has " + std::to_string(nscen)
                                   + " (msd_mpc_rolling_stock with nscen = 0 clears it)");
    const double *ovr = (ro && m->ro_model) ? m->d_ovr : nullptr;      /* (every launch: the lists carry original scenario indices, so row s stays with scenario s) */
    const bool plant = ro && m->ro_plant;
    const bool account = m->en_nscen != 0;
    if (account && nscen != m->en_nscen)
        return fail(MSD_E_INVALID, "the loop keeps the energy account of " + std::to_string(m->en_nscen) + " scenarios, the run has " + std::to_string(nscen)
                                   + " (msd_mpc_energy with nscen = 0 clears it)");
    if (account && plant && m->en_steps != m->plant_steps)
        return fail(MSD_E_INVALID, "the energy account takes " + std::to_string(m->en_steps) + " steps per interval, the plant " + std::to_string(m->plant_steps));
    for (int s = 0; s < nscen; s++) if (!(T[s] > 0)) return fail(MSD_E_INVALID, "Terminal time must be a strictly positive number!");
    msd_problem *h = m->h;
    if (h->begun) return fail(MSD_E_INVALID, "a batch begun with msd_solve_batch_begin has not been waited for (MSD_WAIT_ALL)");
    HIP_TRY(hipSetDevice(h->device));
    const int B = nscen, K = m->K;
    int rc = grow(m, B, z_log != nullptr);
    if (rc != MSD_OK) return rc;
    hipStream_t st = h->stream;
    HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(hipMemcpyAsync(m->d_Tin, T, sizeof(double)*B, hipMemcpyHostToDevice, st));
    if (K > 1 && n1 && n2) {
        HIP_TRY(hipMemcpyAsync(m->d_n1, n1, sizeof(double)*(size_t)(K - 1)*B, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(m->d_n2, n2, sizeof(double)*(size_t)(K - 1)*B, hipMemcpyHostToDevice, st));
    } else if (K > 1) {
        HIP_TRY(hipMemsetAsync(m->d_n1, 0, sizeof(double)*(size_t)(K - 1)*B, st));
        HIP_TRY(hipMemsetAsync(m->d_n2, 0, sizeof(double)*(size_t)(K - 1)*B, st));
    }
    if (plant) {
        m->ps_nscen = 0;
        HIP_TRY(hipMemsetAsync(m->d_stalled, 0, sizeof(int)*(size_t)B, st));
        HIP_TRY(hipMemsetAsync(m->d_ps, 0, sizeof(double)*(size_t)MSD_MPC_PS_COUNT*std::max(K - 1, 1)*B, st));      /* (a record no advance writes reads as zeros) */
    }
    if (account) {
        m->en_run = 0;
        HIP_TRY(hipMemsetAsync(m->d_en_rec, 0, sizeof(double)*(size_t)MSD_MPC_EN_COUNT*K*B, st));      /* (a record no leg writes reads as zeros) */
    }
    const dim3 tb(256), gb((B + 255)/256);
    auto queue = [&]() { int *q = m->d_queue + m->queue_slot; m->queue_slot = (m->queue_slot + 1) % RING; return q; };
    HIP_TRY(hipEventRecord(m->e0, st));
    hipLaunchKernelGGL(mpc_begin, gb, tb, 0, st, B, m->d_Tin, initial_time, initial_velocity, m->d_T, m->d_tnow, m->d_vnow, m->d_flag);
    int cur = 0;
    size_t zoff = 0;
    for (int k = 0; k < K; k++) {
        const msd_host::Plan &pl = m->pl[k];
        const int N = pl.P.N, stp = 4 + pl.P.withPn;
        double *logk = m->d_log + (size_t)MSD_MPC_COUNT*B*k;
        if (rs) {
            /* the rows of this grid and the caps of the end speeds from the records known by now, then the scenario records under the caps */
            launch_rows(m, k, st);
            hipLaunchKernelGGL(mpc_scen_caps, gb, tb, 0, st, B, m->d_T, m->d_tnow, m->d_vnow, m->vmin, m->d_caps, m->d_scen, logk);
        } else
            hipLaunchKernelGGL(mpc_scen, gb, tb, 0, st, B, m->d_T, m->d_tnow, m->d_vnow, m->vmin, m->vlim0[k], m->vN*m->vN, m->d_scen, logk);
        msd_host::WarmStart ws;
        ws.d_limits = rs ? m->d_rows : nullptr;      /* (every launch of the re-solve: the lists carry original scenario indices, so row s stays with scenario s) */
        const int prev = 1 - cur;
        if (m->warm && k > 0 && m->tail[k]) {
            /* the new grid is the tail of the old one: primal point and multipliers of the previous solutions, `stride` intervals down the horizon */
            const msd_host::Plan &pp = m->pl[k - 1];
            ws.d_guess = m->d_z[prev] + (size_t)stp*m->stride; ws.stride = pp.nz; ws.d_status = m->d_st[prev]; ws.mu = m->wmu; ws.push = m->wpush;
            ws.d_dual_in = m->d_dual[prev]; ws.dual_stride = (long long)MSD_DUAL_STRIDE*(pp.P.N + 1); ws.dual_shift = m->stride;
        }
        ws.d_dual_out = m->warm ? m->d_dual[cur] : nullptr;
        ws.one_attempt = m->relax;      /* (mpc_relax: what the twin does not declare late is solved again with both attempts) */
        ws.use_soc = true;              /* (second-order corrections are the rule in these re-solves: the first-pass kernel that has them, msd_kernel.hpp: SOCK) */
        rc = msd_host::launch_plan(pl, st, m->d_work, m->d_follow, queue(), B, m->d_scen, ovr, m->d_z[cur], nullptr, m->d_st[cur], nullptr, 0, ws);
        if (rc != MSD_OK) { hipStreamSynchronize(st); return rc; }      /* (nothing of a loop that failed half-way stays queued on the handle's stream) */
        if (m->relax) {
            const msd_host::Plan &tw = m->tw[k];
            hipLaunchKernelGGL(mpc_collect, gb, tb, 0, st, B, m->d_st[cur], m->d_scen, 3*m->length[k]/m->vmax, m->d_flag, m->d_listA, m->d_scen_tw);
            msd_host::WarmStart wtw;
            wtw.d_limits = ws.d_limits;
            if (ovr) hipLaunchKernelGGL(mpc_twin_scaling, gb, tb, 0, st, B, tw.P.objDen, m->d_ovr_tw);
            rc = msd_host::launch_plan(tw, st, m->d_work, m->d_follow_tw, queue(), B, m->d_scen_tw, ovr ? m->d_ovr_tw : nullptr, m->d_ztw, nullptr, m->d_sttw, nullptr, 0, wtw, m->d_listA);
            if (rc != MSD_OK) { hipStreamSynchronize(st); return rc; }
            double margin = m->margin;
            for (int a = 0; a < 3; a++, margin *= 4) {
                hipLaunchKernelGGL(mpc_relax, gb, tb, 0, st, B, a, m->d_st[cur], m->d_ztw, tw.nz, m->d_sttw, m->d_T, m->d_tnow, m->d_tm, m->d_flag, m->d_listB, m->d_scen, margin, logk);
                msd_host::WarmStart cold;
                cold.d_dual_out = ws.d_dual_out;
                cold.use_soc = true;
                cold.d_limits = ws.d_limits;
                rc = msd_host::launch_plan(pl, st, m->d_work, m->d_follow, queue(), B, m->d_scen, ovr, m->d_z[cur], nullptr, m->d_st[cur], nullptr, 0, cold, m->d_listB);
                if (rc != MSD_OK) { hipStreamSynchronize(st); return rc; }
            }
        }
        hipLaunchKernelGGL(mpc_log, gb, tb, 0, st, B, m->d_st[cur], m->d_T, logk);
        if (z_log) {
            HIP_TRY(hipMemcpyAsync(m->d_zlog + zoff, m->d_z[cur], sizeof(double)*(size_t)pl.nz*B, hipMemcpyDeviceToDevice, st));
            zoff += (size_t)pl.nz*B;
        }
        const bool leg = k + 1 < K && N - m->stride >= 1;
        if (account) {
            /* the account of the leg behind this re-solve: with a plant the kernel stands where mpc_plant stands and advances the state too; without one it runs
             * next to mpc_advance; behind the last re-solve the whole plan, and nothing but the account is written */
            const int adv = (leg && plant) ? 1 : 0;
            const size_t row = leg ? (size_t)B*k : 0;      /* (the final leg has no noise: the pointers are not read) */
            hipLaunchKernelGGL(mpc_energy, gb, tb, 0, st, pl.P, B, leg ? m->stride : N, m->en_steps, m->d_z[cur], pl.nz, m->d_st[cur], m->d_scen, ovr,
                               plant ? (const double *)m->d_plant : nullptr, m->en_eta ? (const double *)m->d_en : nullptr, m->en_mass, adv, m->noise, m->d_n1 + row, m->d_n2 + row,
                               m->d_tnow, m->d_vnow, plant ? m->d_stalled : nullptr, adv ? m->d_ps + (size_t)MSD_MPC_PS_COUNT*B*k : nullptr,
                               m->d_en_rec + (size_t)MSD_MPC_EN_COUNT*B*k);
        }
        if (leg && plant && !account)
            hipLaunchKernelGGL(mpc_plant, gb, tb, 0, st, pl.P, B, m->stride, m->plant_steps, m->d_z[cur], pl.nz, m->d_st[cur], m->d_scen, m->d_plant, m->noise,
                               m->d_n1 + (size_t)B*k, m->d_n2 + (size_t)B*k, m->d_tnow, m->d_vnow, m->d_stalled, m->d_ps + (size_t)MSD_MPC_PS_COUNT*B*k);
        else if (leg && !plant)
            hipLaunchKernelGGL(mpc_advance, gb, tb, 0, st, B, m->d_z[cur], pl.nz, m->d_st[cur], stp*m->stride + 2 + pl.P.withPn, stp*m->stride + 3 + pl.P.withPn, m->noise,
                               m->d_n1 + (size_t)B*k, m->d_n2 + (size_t)B*k, m->d_tnow, m->d_vnow);
        cur = prev;
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(m->e1, st));
    if (log) HIP_TRY(hipMemcpyAsync(log, m->d_log, sizeof(double)*(size_t)MSD_MPC_COUNT*K*B, hipMemcpyDeviceToHost, st));
    if (z_log) HIP_TRY(hipMemcpyAsync(z_log, m->d_zlog, sizeof(double)*zoff, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (loop_ms) HIP_TRY(hipEventElapsedTime(loop_ms, m->e0, m->e1));
    if (plant) m->ps_nscen = B;
    if (account) m->en_run = B;
    return MSD_OK;
}

int msd_mpc_energy(msd_mpc_handle m, int nscen, double total_mass, const double *eta, int steps)
{
    if (!m) return fail(MSD_E_INVALID, "null handle");
    if (nscen == 0) { m->en_nscen = 0; m->en_run = 0; return MSD_OK; }      /* (the buffer stays; no run is in flight) */
    if (nscen < 0) return fail(MSD_E_INVALID, "msd_mpc_energy: bad argument");
    if (m->rs_nscen && nscen != m->rs_nscen)
        return fail(MSD_E_INVALID, "the loop holds the speed restrictions of " + std::to_string(m->rs_nscen) + " scenarios: an energy account of " + std::to_string(nscen) + " does not compose with them");
    if (m->ro_nscen && nscen != m->ro_nscen)
        return fail(MSD_E_INVALID, "the loop holds the rolling stock of " + std::to_string(m->ro_nscen) + " scenarios: an energy account of " + std::to_string(nscen) + " does not compose with it");
    if (!std::isfinite(total_mass) || !(total_mass > 0)) return fail(MSD_E_INVALID, "msd_mpc_energy: total_mass must be positive");
    if (m->ro_nscen && m->ro_plant) {
        if (steps != m->plant_steps) return fail(MSD_E_INVALID, "msd_mpc_energy: steps must be the plant's plant_steps (" + std::to_string(m->plant_steps) + ")");
    } else if (steps < 1 || steps > 64) return fail(MSD_E_INVALID, "msd_mpc_energy: steps must be 1 ... 64");
    const size_t b = (size_t)nscen;
    std::vector<double> coef;
    if (eta) {
        coef.resize(2*b);
        for (size_t s = 0; s < b; s++) {
            const double et = eta[2*s], er = eta[2*s + 1];
            if (!(et > 0) || !(et <= 1) || !(er > 0) || !(er <= 1)) return fail(MSD_E_INVALID, "efficiencies of scenario " + std::to_string(s) + " are not in (0, 1]");
            coef[2*s] = (1 - et)/et; coef[2*s + 1] = 1 - er;      /* train.py:199-212 */
        }
    }
    msd_problem *h = m->h;
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    m->en_nscen = 0; m->en_run = 0;      /* (until the upload has ended) */
    if (nscen > m->cap_en) {
        hipFree(m->d_en); m->d_en = nullptr; m->cap_en = 0;
        HIP_TRY(hipMalloc((void **)&m->d_en, sizeof(double)*(2*b + (size_t)MSD_MPC_EN_COUNT*m->K*b)));
        m->cap_en = nscen;
    }
    m->d_en_rec = m->d_en + 2*b;
    if (eta) HIP_TRY(hipMemcpy(m->d_en, coef.data(), sizeof(double)*2*b, hipMemcpyHostToDevice));
    m->en_eta = eta != nullptr; m->en_mass = total_mass; m->en_steps = steps;
    m->en_nscen = nscen;
    return MSD_OK;
}

int msd_mpc_energy_records(msd_mpc_handle m, double *records)
{
    if (!m || !records) return fail(MSD_E_INVALID, "bad argument");
    if (!m->en_nscen) return fail(MSD_E_INVALID, "the loop keeps no energy account (msd_mpc_energy)");
    if (!m->en_run) return fail(MSD_E_INVALID, "msd_mpc_energy_records: the loop has not run under its account yet");
    msd_problem *h = m->h;
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipMemcpyAsync(records, m->d_en_rec, sizeof(double)*(size_t)MSD_MPC_EN_COUNT*m->K*m->en_run, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return MSD_OK;
}

int msd_mpc_rolling_stock(msd_mpc_handle m, int nscen, const double *model, const double *plant, int plant_steps)
{
    if (!m) return fail(MSD_E_INVALID, "null handle");
    if (nscen == 0) { m->ro_nscen = 0; m->ro_model = m->ro_plant = false; m->ps_nscen = 0; return MSD_OK; }      /* (the buffer stays; no run is in flight) */
    if (nscen < 0 || (!model && !plant)) return fail(MSD_E_INVALID, "msd_mpc_rolling_stock: bad argument");
    if (m->rs_nscen && nscen != m->rs_nscen)
        return fail(MSD_E_INVALID, "the loop holds the speed restrictions of " + std::to_string(m->rs_nscen) + " scenarios: rolling stock of " + std::to_string(nscen) + " does not compose with them");
    if (m->en_nscen && nscen != m->en_nscen)
        return fail(MSD_E_INVALID, "the loop keeps the energy account of " + std::to_string(m->en_nscen) + " scenarios: rolling stock of " + std::to_string(nscen) + " does not compose with it");
    if (model) {
        bool fused = false;      /* (any kernel of the loop that has the row structure compiled in) */
        for (int k = 0; k < m->K; k++) fused = fused || m->pl[k].fused_family || (m->twin && m->tw[k].fused_family);
        const int rc = msd_host::check_overrides(fused, nscen, model);
        if (rc != MSD_OK) return rc;
    }
    if (plant) {
        if (plant_steps < 1 || plant_steps > 64) return fail(MSD_E_INVALID, "msd_mpc_rolling_stock: plant_steps must be 1 ... 64");
        for (int s = 0; s < nscen; s++) {
            const double *r = plant + (size_t)MSD_MPC_PL_COUNT*s;
            for (int j = 0; j < MSD_MPC_PL_COUNT; j++) if (!std::isfinite(r[j])) return fail(MSD_E_INVALID, "plant of scenario " + std::to_string(s) + " is not finite");
            if (r[MSD_MPC_PL_SR0] < 0 || r[MSD_MPC_PL_SR1] < 0 || r[MSD_MPC_PL_SR2] < 0) return fail(MSD_E_INVALID, "plant of scenario " + std::to_string(s) + " has a negative Davis coefficient");
            if (!(r[MSD_MPC_PL_FORCE_SCALE] > 0)) return fail(MSD_E_INVALID, "plant of scenario " + std::to_string(s) + ": force_scale must be positive");
        }
    }
    msd_problem *h = m->h;
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    m->ro_nscen = 0; m->ro_model = m->ro_plant = false; m->ps_nscen = 0;      /* (until the upload has ended) */
    const size_t b = (size_t)nscen, states = (size_t)MSD_MPC_PS_COUNT*std::max(m->K - 1, 1)*b;
    if (nscen > m->cap_ro) {
        hipFree(m->d_ro); m->d_ro = nullptr; m->cap_ro = 0;
        HIP_TRY(hipMalloc((void **)&m->d_ro, sizeof(double)*(2*MSD_OV_COUNT*b + MSD_MPC_PL_COUNT*b + states + b)));      /* (the flags: ints in the room of b doubles) */
        m->cap_ro = nscen;
    }
    m->d_ovr = m->d_ro; m->d_ovr_tw = m->d_ovr + MSD_OV_COUNT*b; m->d_plant = m->d_ovr_tw + MSD_OV_COUNT*b; m->d_ps = m->d_plant + MSD_MPC_PL_COUNT*b;
    m->d_stalled = (int *)(m->d_ps + states);
    if (model) {
        HIP_TRY(hipMemcpy(m->d_ovr, model, sizeof(double)*MSD_OV_COUNT*b, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(m->d_ovr_tw, model, sizeof(double)*MSD_OV_COUNT*b, hipMemcpyHostToDevice));      /* (mpc_twin_scaling rewrites one column per re-solve) */
    }
    if (plant) HIP_TRY(hipMemcpy(m->d_plant, plant, sizeof(double)*MSD_MPC_PL_COUNT*b, hipMemcpyHostToDevice));
    m->ro_model = model != nullptr; m->ro_plant = plant != nullptr; m->plant_steps = plant ? plant_steps : 0;
    m->ro_nscen = nscen;
    return MSD_OK;
}

int msd_mpc_plant_states(msd_mpc_handle m, double *states)
{
    if (!m || !states) return fail(MSD_E_INVALID, "bad argument");
    if (!m->ro_nscen || !m->ro_plant) return fail(MSD_E_INVALID, "the loop holds no plant (msd_mpc_rolling_stock)");
    if (!m->ps_nscen) return fail(MSD_E_INVALID, "msd_mpc_plant_states: the loop has not run under its plant yet");
    if (m->K < 2) return MSD_OK;
    msd_problem *h = m->h;
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipMemcpyAsync(states, m->d_ps, sizeof(double)*(size_t)MSD_MPC_PS_COUNT*(m->K - 1)*m->ps_nscen, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return MSD_OK;
}

int msd_mpc_speed_restrictions(msd_mpc_handle m, const double *origin, int nscen, int max_per_scenario, const int *count, const double *records)
{
    if (!m) return fail(MSD_E_INVALID, "null handle");
    if (nscen == 0) { m->rs_nscen = 0; return MSD_OK; }      /* (the buffers stay; no run is in flight: msd_mpc_run waits for its own end) */
    if (nscen < 0 || !origin || !count || !records) return fail(MSD_E_INVALID, "msd_mpc_speed_restrictions: bad argument");
    if (m->ro_nscen && nscen != m->ro_nscen)
        return fail(MSD_E_INVALID, "the loop holds the rolling stock of " + std::to_string(m->ro_nscen) + " scenarios: speed restrictions of " + std::to_string(nscen) + " do not compose with it");
    if (m->en_nscen && nscen != m->en_nscen)
        return fail(MSD_E_INVALID, "the loop keeps the energy account of " + std::to_string(m->en_nscen) + " scenarios: speed restrictions of " + std::to_string(nscen) + " do not compose with it");
    if (max_per_scenario < 1 || max_per_scenario > MSD_RS_MAX)
        return fail(MSD_E_INVALID, "msd_mpc_speed_restrictions: max_per_scenario must be 1 ... " + std::to_string(MSD_RS_MAX));
    const int K = m->K;
    for (int k = 0; k < K; k++)
        if (!std::isfinite(origin[k]) || (k == 0 ? origin[0] != 0 : origin[k] < origin[k - 1]))
            return fail(MSD_E_INVALID, "msd_mpc_speed_restrictions: origin must be non-decreasing from 0");
    const double vminSq = m->pl[0].P.vminSq;
    for (int s = 0; s < nscen; s++) {
        const auto bad = [&](int j, const char *what) {
            return fail(MSD_E_INVALID, "speed restriction " + std::to_string(j) + " of scenario " + std::to_string(s) + " " + what);
        };
        if (count[s] < 0 || count[s] > max_per_scenario) return fail(MSD_E_INVALID, "scenario " + std::to_string(s) + ": the number of speed restrictions must be 0 ... max_per_scenario");
        for (int j = 0; j < count[s]; j++) {
            const double *r = records + (size_t)MSD_MPC_RS_COUNT*((size_t)max_per_scenario*s + j);
            const double begin = r[0], end = r[1], v = r[2], first = r[3];
            if (!std::isfinite(begin) || !std::isfinite(end) || !std::isfinite(v) || !std::isfinite(first)) return bad(j, "is not finite");
            if (!(end > begin)) return bad(j, "ends at or before its beginning");
            if (!(v > 0) || !(v*v > vminSq)) return bad(j, "is not above the minimum speed (a limit equal to it fixes adjacent nodes: not supported)");
            if (first != std::floor(first) || first < 0 || first > K - 1) return bad(j, "is not known from a re-solve 0 ... K-1 (first_resolve)");
            /* some interval of grid 0 is restricted  <=>  the restriction overlaps (pos[0], pos[N]) = (0, last0): the nodes are increasing */
            if (!(end > 0 && begin < m->last0)) return bad(j, "restricts no interval of the grid of re-solve 0");
        }
    }
    msd_problem *h = m->h;
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    m->rs_nscen = 0;      /* (until the upload has ended: a HIP failure below leaves the loop without records, not with half of them) */
    const size_t rec_doubles = (size_t)MSD_MPC_RS_COUNT*max_per_scenario*nscen;
    const size_t rec_bytes = sizeof(double)*rec_doubles + sizeof(int)*(size_t)nscen;      /* records, then the counts */
    if (rec_bytes > m->cap_rs) {
        hipFree(m->d_rs); m->d_rs = nullptr; m->cap_rs = 0;
        HIP_TRY(hipMalloc((void **)&m->d_rs, rec_bytes));
        m->cap_rs = rec_bytes;
    }
    if ((size_t)nscen > m->cap_rows) {
        /* the rows of one re-solve at a time, for the longest grid, and the two caps per scenario behind them */
        hipFree(m->d_rows); m->d_rows = nullptr; m->d_caps = nullptr; m->cap_rows = 0;
        HIP_TRY(hipMalloc((void **)&m->d_rows, sizeof(double)*((size_t)m->nodes_max + 2)*nscen));
        m->cap_rows = nscen;
    }
    m->d_caps = m->d_rows + (size_t)m->nodes_max*m->cap_rows;
    HIP_TRY(hipMemcpy(m->d_rs, records, sizeof(double)*rec_doubles, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(m->d_rs + rec_doubles, count, sizeof(int)*(size_t)nscen, hipMemcpyHostToDevice));
    m->origin.assign(origin, origin + K);
    m->rs_nscen = nscen; m->rs_max = max_per_scenario;
    return MSD_OK;
}

int msd_mpc_limit_rows(msd_mpc_handle m, int k, double *rows)
{
    if (!m || !rows) return fail(MSD_E_INVALID, "bad argument");
    if (!m->rs_nscen) return fail(MSD_E_INVALID, "the loop holds no speed restrictions (msd_mpc_speed_restrictions)");
    if (k < 0 || k >= m->K) return fail(MSD_E_INVALID, "msd_mpc_limit_rows: re-solve outside 0 ... K-1");
    msd_problem *h = m->h;
    HIP_TRY(hipSetDevice(h->device));
    launch_rows(m, k, h->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(rows, m->d_rows, sizeof(double)*(size_t)(m->pl[k].P.N + 1)*m->rs_nscen, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return MSD_OK;
}

}  // extern "C"
