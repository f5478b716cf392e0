/*
 * TEST-ONLY: the launch of the fused family like msd_api.hip: launch_plan does it since round 11 -- the first pass is the default kernel or its twin by the rule
 * of msd_select.hpp (first_pass_twin).  A driver of its own next to emu_driver.cpp (which knows no twins), for tests/test_fused_first_pass_emulation.py; built
 * with UNITS="emu_driver emu_k_full emu_k_full_early emu_k_first_pass" of build.sh into an object folder of its own.  The other families' lookups, which
 * emu_driver.cpp refers to, are empty here: this library holds the fused family only.
 */
#include "emu_common.h"

EmuFn emu_kernels_full(const msd::KernelId &id);
EmuFn emu_kernels_full_early(const msd::KernelId &id);
#define EMU_NO_UNIT(unit) EmuFn emu_kernels_##unit(const msd::KernelId &) { return nullptr; }
EMU_NO_UNIT(static) EMU_NO_UNIT(dynamic) EMU_NO_UNIT(general) EMU_NO_UNIT(intloss) EMU_NO_UNIT(intloss_table) EMU_NO_UNIT(stream)

static EmuFn find(msd::KernelId id)
{
    if (!id) return nullptr;
    id.WPS = 1;
    if (const EmuFn fn = emu_kernels_full(id)) return fn;
    return emu_kernels_full_early(id);
}

/*
 * One launch.  flags: bit 0 the default kernel whatever the integrator (its guard), bit 1 no follow-up kernel.  info[0] = 1: the first pass was the twin;
 * info[1] PART of the first pass, info[2] NT, info[3] SPT, info[4] FULL; info[5] PART of the follow-up kernel that ran (0: none); info[8 + k]: scenarios handed
 * over for reason k (msd::FOLLOW_WHY).  dual_in / dual_out: the multipliers of a primal-dual warm start (with guess) and for the next one, or null.
 * Returns -3 where the problem is not of the fused family or the library holds no kernel for it.
 */
extern "C" int emu_first_pass_solve(const msd_problem_desc *d, int nscen, const double *scen, const double *guess, const double *dual_in, double *dual_out, double mu0, double push,
                                    double *z, double *lam, double *stats, int flags, int *info)
{
    using namespace msd_host;
    msd::DevProb P;
    fill_problem(P, d);
    P.guess = guess; P.guessStride = (4 + d->with_pn_brake)*d->num_intervals + 2; P.warmMu = mu0; P.warmPush = push;
    P.dualOut = dual_out; P.dualIn = guess ? dual_in : nullptr; P.dualInStride = 0;
    std::vector<double> pos(d->num_intervals + 1, 0.0);
    for (int i = 0; i < d->num_intervals; i++) pos[i + 1] = pos[i] + d->ds[i];
    P.pos = pos.data(); P.ds = d->ds; P.grad = d->grad; P.curv = d->curv; P.bmax = d->bmax; P.loss = d->loss_table; P.coll = d->coll_tables;
    std::vector<double> hist(64, 0.0);
    EmuArgs a = {P, nscen, scen, nullptr, z, lam, stats, hist.data(), 8};
    const int N = d->num_intervals;
    const msd::Geometry g = resident(family_of(d), N, structure_of(d), Tuning());
    if (!g.first || g.xch != msd::XCH_FAST || !g.follow) return -3;
    const bool plain = P.guess ? P.dualIn != nullptr : P.start == MSD_START_PROFILE;
    msd::KernelId first = plain ? g.first : g.lsq;
    if (!first) return -3;
    const bool twin = first_pass_twin(true, false, P.numSteps, P.numApprox) && !(flags & 1) && find(g.early(first));
    if (twin) first = g.early(first);
    const EmuFn run_first = find(first), run_follow = (flags & 2) ? nullptr : find(g.follow);
    if (!run_first || (!(flags & 2) && !run_follow)) return -3;
    std::vector<int> list(msd::FOLLOW_HDR + 2*(size_t)nscen, 0);
    a.P.follow = list.data();
    run_first(a, g);
    for (int k = 0; k < 16; k++) info[k] = 0;
    info[0] = twin; info[1] = first.PART; info[2] = first.NT; info[3] = first.SPT; info[4] = first.FULL;
    for (int k = 0; k < 8; k++) info[8 + k] = list[msd::FOLLOW_WHY + k];
    if (!run_follow) return 0;
    a.P.list = list.data(); a.P.follow = nullptr;
    run_follow(a, g);
    info[5] = g.follow.PART;
    return 0;
}
