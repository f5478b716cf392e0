/*
 * msd_select.hpp -- which kernels solve a problem description: the kernel family and structure of a description, its problem record, and the one
 * ladder from (family, horizon, structure) to a Geometry of kernel ids.  Host only and data only: no device call, no function pointer.  The library
 * (msd_api.hip: select_plan) and the host emulation of the kernels (tests/hip_emu/emu_driver.cpp) both pick through it; neither kernel unit includes it,
 * so an edit of the ladder recompiles no kernel.
 *
 * To add a family or a horizon range: one rung here, one MSD_KERNEL entry in the unit that is to hold the instantiation.
 */
#pragma once

#include <cmath>

#include "msd_geometry.hpp"

namespace msd_host {

using msd::Geometry;
using msd::KernelId;

/* the transcription a description asks for: which kernel family solves it */
enum Family { STATIC, DYNAMIC, INTLOSS, INTLOSS_TABLE, GENERAL, GENERAL_DYNAMIC, GENERAL_INTLOSS };
inline Family family_of(const msd_problem_desc *d)
{
    const bool dyn = d->loss_kind == 2, gen = d->integrator != 0, intloss = d->integrate_losses != 0 && d->energy_optimal != 0;
    if (dyn && intloss) return INTLOSS_TABLE;      /* the loss table integrated over the running time (msd_lossint_table.hpp: DYN = LOSS_INTEGRATED_TABLE) */
    if (gen) return dyn ? GENERAL_DYNAMIC : intloss ? GENERAL_INTLOSS : GENERAL;
    return intloss ? INTLOSS : dyn ? DYNAMIC : STATIC;
}
/* the structure of the reference's rolling stock, where the description has it: msd::FULL_BOTH / FULL_RG / FULL_TIME_BOTH / FULL_TIME_RG, or 0 */
inline int structure_of(const msd_problem_desc *d)
{
    /* power rows (finite by construction: ocp.py:186-187) and finite acceleration bounds (ocp.py:113-114) */
    if (d->has_power_rows == 0 || !std::isfinite(d->acc_min) || !std::isfinite(d->acc_max) || !std::isfinite(d->pw_upper) || !std::isfinite(d->pw_lower)) return 0;
    /* energy objective: both brakes, or the regenerative brake alone (forceMinPn = 0: the reference's scripts) */
    if (d->energy_optimal != 0) {
        /* The fused passes of these kernels take "variable k is free" from the structure (msd_kernel.hpp: Solver::on).  A description that fixes a variable
         * the structure has free -- no force range, a pneumatic brake without force -- is not of the structure: the general kernels solve it.  Where only a
         * scenario or an override does that, the kernel hands the scenario over (reason 0); so it does for an interior speed limit equal to the minimum speed,
         * which is a matter of the profile and not looked for here (the recorded plan table, tests/golden, describes its plans on such a profile) */
        if (d->f_min == d->f_max || (d->with_pn_brake != 0 && d->f_min_pn == 0.0)) return 0;
        return d->with_pn_brake != 0 ? msd::FULL_BOTH : msd::FULL_RG;
    }
    /* the time-optimal problem on the same rolling stock (energyOptimal = False: minimumTime, the twins of msd_mpc.hip): no loss rows */
    return d->with_pn_brake != 0 ? msd::FULL_TIME_BOTH : msd::FULL_TIME_RG;
}
/* loss transcription (solve_kernel's DYN) and shooting integrators (GEN) of a family's kernels */
inline int dyn_of(Family f) { return (f == DYNAMIC || f == GENERAL_DYNAMIC) ? msd::LOSS_TABLE : (f == INTLOSS || f == GENERAL_INTLOSS) ? msd::LOSS_INTEGRATED : f == INTLOSS_TABLE ? msd::LOSS_INTEGRATED_TABLE : msd::LOSS_STATIC; }
inline bool gen_of(Family f) { return f == GENERAL || f == GENERAL_DYNAMIC || f == GENERAL_INTLOSS; }

/* the problem record of a description.  Every pointer is null: the owner of the profile buffers fills ds ... pos, loss and coll, a launch the rest */
inline void fill_problem(msd::DevProb &P, const msd_problem_desc *d)
{
    P.N = d->num_intervals; P.withPn = d->with_pn_brake != 0; P.hasPower = d->has_power_rows != 0; P.energyOpt = d->energy_optimal != 0;
    P.numSteps = d->num_steps; P.numApprox = d->num_approx_steps; P.lossKind = d->loss_kind; P.maxIter = d->max_iterations;
    P.sr0 = d->sr0; P.sr1 = d->sr1; P.sr2 = d->sr2; P.g = d->g; P.rho = d->rho; P.fmax = d->f_max; P.fmin = d->f_min; P.fminPn = d->f_min_pn;
    P.pwU = d->pw_upper; P.pwL = d->pw_lower; P.accMin = d->acc_min; P.accMax = d->acc_max; P.ct = d->loss_ct; P.cr = d->loss_cr;
    P.vminSq = d->vmin_sq; P.objDen = d->obj_den; P.tol = d->tol;
    P.guess = nullptr; P.guessStride = 0; P.guessStatus = nullptr; P.warmMu = 0; P.warmPush = 0; P.start = d->start_kind; P.lossMass = 0; P.queue = nullptr; P.follow = nullptr; P.list = nullptr; P.socSeen = nullptr; P.done = nullptr; P.statsHost = nullptr; P.budget = 0; P.dualOut = nullptr; P.dualIn = nullptr; P.dualInStride = 0; P.dualShift = 0;
    P.ds = P.grad = P.curv = P.bmax = P.pos = nullptr;
    P.limits = nullptr;
    P.loss = nullptr; P.lossCoef = nullptr;
    P.integ = d->integrator; P.collD = d->coll_degree; P.newtonIters = d->newton_iterations; P.intAtol = d->int_abstol; P.intRtol = d->int_reltol;
    P.coll = nullptr;
    P.resto = d->no_restoration ? 0 : 1;
    P.oneAttempt = 0;
    P.wdTrigger = d->watchdog_trigger == 0 ? 10 : d->watchdog_trigger;      /* IPOPT's default */
    if (d->integrator == MSD_INTEGRATOR_ADAPTIVE) P.numApprox = 0;      /* train.py:314 */
}

/*
 * Which first pass of a split launch runs: the default instantiation, or its twin (msd::Geometry::early).  The default first passes of the fused family hold
 * one integrator -- one RK4 step and one trapezoid per interval (numSteps = 1, numApprox = 1: msd_kernel.hpp, Solver::FIXED_INTEG) -- and no early results; the
 * twin holds the early results and chooses the integrator at run time.  So the twin runs for a begun batch or an iteration budget (`early`), and on the fused
 * family for every other integrator shape.  Elsewhere a kernel is its own twin; so is, for the integrator, a first pass with the second-order correction inside
 * (SOCK), which chooses at run time too: the launch code asks this rule for the kernels without it only.  A default kernel that meets another integrator all the same hands every
 * scenario to the follow-up kernel (reason 0), which is what a launch falls back on where the build holds no twin and the results are not early ones.
 */
inline bool compiled_integrator(int num_steps, int num_approx) { return num_steps == 1 && num_approx == 1; }
inline bool first_pass_twin(bool fused_family, bool early, int num_steps, int num_approx)
{
    return early || (fused_family && !compiled_integrator(num_steps, num_approx));
}

/* tuning switches of the ladder, set through msd_tuning() of include/mseetc_aux.h (A/B runs, one GPU test): the library reads no environment variable.
 * no_full: the kernels without the structure of the NLP compiled in; two_nodes_per_lane: the 64 x 2 geometry for 65 ... 128 nodes of the loss-table,
 * shooting-integrator and integrateLosses families (default there: 128 x 1) */
struct Tuning {
    bool no_full = false, two_nodes_per_lane = false;
    int NT = 0, SPT = 0;      /* not 0: every rung offers this geometry instead of its own, whatever the horizon (the emulation's EMU_GEOMETRY=NTxSPT; msd_tuning("geometry", 16 NT + SPT)) */
};

/* does this build hold the kernel?  Answered by whoever links the instantiations: msd_api.hip (find_kernel over the kernel units), the emulation over its
 * own units.  A rung whose kernel the build does not hold is skipped -- the tuning builds (tools/build_hot.py -DMSD_HOT_ONLY_64X2, tools/build_variant.py:
 * MSD_MINIMAL_GEOMETRIES) and the emulation compile fewer kernels, and take the next rung */
bool has_kernel(const KernelId &id);

/* dynamic LDS of kernel `k` launched as part of `g` for N intervals */
inline size_t lds_bytes(const Geometry &g, const KernelId &k, int N)
{
    return sizeof(double)*(size_t)(k.STREAM ? msd::lds_doubles_stream() : msd::lds_doubles(N, k.NT*k.SPT, k.DYN != msd::LOSS_STATIC, g.xch, g.red) + msd::coop_doubles(k.NT, k.GEN) + g.extra);
}

/*
 * The LDS-resident kernels of a family for N intervals (first: none).  Three kinds of rung:
 *   - first-pass kernels (PART = 1: the general iteration without the restoration phase and the watchdog procedure) without a follow-up kernel of
 *     their own: the streamed kernel of the family follows up (msd_api.hip: select_plan);
 *   - the same with the structure of the reference's rolling stock compiled in (FULL), where the description has it and such kernels exist;
 *   - the fused kernels of the static loss model on that rolling stock: split solves with their own follow-up kernels.
 */
inline Geometry resident(Family family, int N, int structure, const Tuning &t)
{
    using namespace msd;
    const int nodes = N + 1, DYN = dyn_of(family);
    const bool GEN = gen_of(family), two = t.two_nodes_per_lane;
    Geometry g;
    int FULL = t.no_full ? 0 : structure;      /* (msd_tuning("no_full", 1): the general kernels, A/B runs) */
    /* a first-pass kernel of up to `top` nodes */
    const auto rung = [&](int top, int NT, int SPT, int WPS = 1) {
        if (t.NT) { NT = t.NT; SPT = t.SPT; top = NT*SPT; }
        const KernelId id{NT, SPT, WPS, DYN, false, GEN, FULL, 1};
        if (nodes > top || !has_kernel(id)) return false;
        g.first = id;
        return true;
    };
    /* a split solve of the fused family: first pass (the fused iteration alone: XCH_FAST exchange arrays, no reduction scratch for a single wave; the units
     * assert Solver::FAST of these kernels), the same behind the least-squares multiplier estimate, follow-up kernel (general iteration, restoration phase,
     * second attempt), and the first pass with the second-order correction inside where the build has one (both brakes, up to 103 intervals) */
    const auto fused = [&](int NT, int SPT, bool slds = false) {
        if (t.NT) { NT = t.NT; SPT = t.SPT; }
        const KernelId id{NT, SPT, 1, LOSS_STATIC, false, false, FULL, 1, slds};
        const int red = NT == 64 ? 0 : RED_DOUBLES;
        if (nodes > NT*SPT || sizeof(double)*(size_t)lds_doubles(N, NT*SPT, false, XCH_FAST, red) > 160*1024 || !has_kernel(id)) return false;
        Geometry s;
        s.first = s.lsq = s.follow = s.soc = id;
        s.lsq.PART = 3;
        s.follow.PART = 2; s.follow.SLDS = false;
        /* Horizons of up to 63 intervals where the build has no 64 x 1 follow-up kernel (both brakes; the one-brake family has its own, msd_kernels_rg2.hip): the
         * two-nodes-per-lane kernel follows up the one-node-per-lane first pass, its second node slots idle */
        if (NT == 64 && SPT == 1 && !has_kernel(s.follow)) s.follow.SPT = 2;
        if (!has_kernel(s.follow)) return false;
        if (!has_kernel(s.lsq)) s.lsq = KernelId{};      /* (then the follow-up kernel takes the launches that need the estimate: msd_api.hip: launch_plan) */
        s.soc.SOCK = true;
        if (!has_kernel(s.soc)) s.soc = KernelId{};
        s.xch = XCH_FAST; s.red = red; s.extra = slds ? STATIC_FIELDS*NT*SPT : 0;
        g = s;
        return true;
    };

    if (family == STATIC && full_energy(FULL)) {
        if (fused(64, 1)) return g;
        /* SLDS: the node constants in LDS where they do not cost the fourth resident workgroup of a compute unit (msd_kernel.hpp: STATIC_FIELDS) */
        if (MSD_STATIC_LDS && nodes > 64 && sizeof(double)*(size_t)(lds_doubles(N, 128, false, XCH_FAST, 0) + STATIC_FIELDS*128) <= 40*1024 && fused(64, 2, true)) return g;
        if (fused(64, 2)) return g;      /* the benchmark geometry */
        /* ... and longer horizons while the five additional exchange arrays still fit the LDS of a compute unit next to the stage blocks */
        if (fused(128, 2) || fused(192, 2) || fused(256, 2)) return g;
    }
    /* the time-optimal problem on the reference's rolling stock (msd_kernels_time.hip, msd_kernels_time2.hip) */
    if (family == STATIC && full_time(FULL) && (rung(64, 64, 1) || rung(128, 64, 2) || rung(256, 128, 2))) return g;
    /* the loss-table family with the structure of the energy problem (msd_kernels_dynamic2.hip, msd_kernels_dynamic3.hip; round 6: 438 k -> 508 k solves/s on
     * the figure-5 batch at N = 100).  65 ... 128 nodes have the one-node-per-lane kernel only */
    if (family == DYNAMIC && full_energy(FULL) && (rung(64, 64, 1) || (nodes > 64 && !(nodes <= 128 && two) && (rung(128, 128, 1) || rung(256, 128, 2) || rung(384, 192, 2))))) return g;
    /*
     * integrateLosses and the collocation / adaptive shooting integrators with both brakes (msd_kernels_full2.hip).  65 ... 128 nodes: two waves per scenario
     * with one node per lane and the whole register file of a SIMD each.  The jets through the Newton solve of a collocation step, through the adaptive steps,
     * or through the integrated loss distance are the bulk of an iteration here, and a lane that carries two nodes runs them one after the other with twice
     * the state to keep (1 400 ... 1 600 spilled registers at 64 x 2 against 250 ... 400 at 128 x 1): measured on the config-1 batch 346k against 284k
     * solves/s (integrateLosses), 186k against 166k (Radau, two points), 133k against 124k (adaptive at CVODES' tolerances); profiles/r03.
     */
    if ((family == INTLOSS || family == GENERAL) && FULL == FULL_BOTH && (rung(64, 64, 1) || (two && rung(128, 64, 2)) || rung(128, 128, 1))) return g;

    FULL = 0;
    /* families with ladders of their own: integrateLosses with a loss table (one node per lane: the jets of the two loss integrals are the bulk of an iteration,
     * msd_kernels_intloss_table.hip); the shooting integrators with the loss table or with integrateLosses (msd_kernels_compose.hip) */
    if (family == INTLOSS_TABLE) { (void)(rung(64, 64, 1) || rung(128, 128, 1)); return g; }
    if (family == GENERAL_DYNAMIC) { (void)(rung(64, 64, 1) || rung(128, 128, 1) || rung(256, 128, 2)); return g; }
    if (family == GENERAL_INTLOSS) { (void)(rung(64, 64, 1) || rung(128, 128, 1) || rung(256, 256, 1)); return g; }
    if (rung(64, 64, 1)) return g;
    /* the loss-table family on 65 ... 128 nodes: two waves with one node per lane and the whole register file of a SIMD each (round 6: 341 k against 289 k solves/s
     * on the figure-5 batch at N = 100, 307 k against 219 k at N = 120 -- the jets through the table are the bulk of its iteration;
     * msd_tuning("two_nodes_per_lane", 1): the one-wave geometry) */
    if (DYN == LOSS_TABLE && nodes > 64 && !two && rung(128, 128, 1)) return g;
    if (rung(128, 64, 2)) return g;      /* one wave per scenario, one wave per SIMD */
    if (rung(256, 128, 2) || rung(384, 192, 2) || rung(512, 256, 2)) return g;
    /* N = 512 ... 575 with static loss rows: three waves with three nodes per lane and the whole register file of a SIMD each -- the stage blocks and
     * six exchange arrays of 576 slots still fit the LDS of a compute unit.  (Round 3 ran these horizons on five waves of two nodes per lane with
     * half a register file each: 2 253 spilled registers, 25 ms per 1024 solves at N = 560 against 6.2 ms at N = 511.) */
    if (DYN == LOSS_STATIC && !GEN && rung(576, 192, 3)) return g;
    (void)rung(640, 320, 2, 2);
    return g;
}

/*
 * The streamed kernels of a family (first: none): horizons whose stage blocks do not fit the LDS of a compute unit -- node fields, stage blocks and
 * exchange arrays live in device memory, a lane's nodes are worked off one after the other.  512 threads (two waves per SIMD, 256 registers each) with the
 * stage-parallel KKT solve and as few nodes per lane as the horizon allows (N = 1000: two; 38 -> 11 ms per solve against round 2's 1024 x 5 with serial
 * sweeps).  A streamed solve is a split launch too (round 5): the first pass (PART = 1) and the follow-up kernel of the same geometry with the restoration
 * phase and the watchdog procedure (PART = 2), which also follows up the LDS-resident first-pass kernels of its family.  The static loss model goes up to
 * 5119 intervals, the other families to 1023.  The first pass has the structure of the energy problem compiled in where the build holds that kernel
 * (msd_kernels_stream5.hip, msd_kernels_stream6.hip; round 6: N = 700 / 1000 with the figure-10 train 9.7 / 11.5 -> 8.2 / 9.8 ms per solve); the follow-up
 * kernel is the family's general one either way.
 */
inline Geometry streamed(Family family, int N, int structure, const Tuning &t)
{
    const int nodes = N + 1;
    const int SPT = nodes <= 1024 ? 2 : family != STATIC ? 0 : nodes <= 2048 ? 4 : nodes <= 3072 ? 6 : nodes <= 5120 ? 10 : 0;
    Geometry g;
    if (!SPT) return g;
    g.stream = true;
    g.first = g.follow = KernelId{512, SPT, 2, dyn_of(family), true, gen_of(family), 0, 1};
    g.follow.PART = 2;
    KernelId structured = g.first;
    structured.FULL = structure;
    if (family == STATIC && msd::full_energy(structure) && !t.no_full && has_kernel(structured)) g.first = structured;
    if (!has_kernel(g.first)) g.first = KernelId{};      /* (each of the two on its own: the follow-up kernel also serves the LDS-resident first passes) */
    if (!has_kernel(g.follow)) g.follow = KernelId{};
    return g;
}

}  // namespace msd_host
