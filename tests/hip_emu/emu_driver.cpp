/*
 * TEST-ONLY driver: runs msd::solve_kernel<NT> from ms-eetc_amd/csrc/msd_kernel.hpp on host threads
 * (see hip/hip_runtime.h in this directory).  Build: tests/hip_emu/build.sh.  Used by
 * tests/test_kernel_emulation.py to compare the kernel's logic with the oracle without a GPU.
 */
#include "emu_common.h"

thread_local emu_dim3 threadIdx, blockIdx, blockDim, gridDim;
thread_local emu_block *emu_blk;

#define EMU_UNITS(X) X(static) X(full) X(dynamic) X(general) X(intloss) X(intloss_table) X(stream)
#define X(unit) EmuFn emu_kernels_##unit(const msd::KernelId &id);
EMU_UNITS(X)
#undef X

static bool env_set(const char *name) { const char *v = getenv(name); return v && *v == '1'; }

/* the emulation's instantiation for a kernel id of the ladder.  The streamed kernels are a stand-in geometry the emulation can afford, 128 x 5 in place
 * of 512 x SPT (up to 639 intervals); waves per SIMD mean nothing on the host: every instantiation is compiled with WPS = 1 */
static msd::KernelId stand_in(msd::KernelId id)
{
    if (id.STREAM) { id.NT = 128; id.SPT = 5; }
    if (id) id.WPS = 1;
    return id;
}
static EmuFn emu_find(const msd::KernelId &ladder_id)
{
    const msd::KernelId id = stand_in(ladder_id);
    if (!id) return nullptr;
#define X(unit) if (const EmuFn fn = emu_kernels_##unit(id)) return fn;
    EMU_UNITS(X)
#undef X
    return nullptr;
}

/* what the ladder of msd_select.hpp asks: a rung whose kernel the emulation does not compile is skipped.  EMU_SOCK=1, for a launch that starts without the
 * least-squares estimate: a first pass also counts when only its twin with the second-order correction inside the fused iteration is compiled (msd_kernels_full4.hip:
 * what msd_api.hip launches for the re-solves of the shrinking-horizon loop and for a handle whose launches have handed corrections over) -- the twin then runs */
static bool g_sock = false;
bool msd_host::has_kernel(const msd::KernelId &id)
{
    msd::KernelId soc = id;
    soc.SOCK = true;
    return emu_find(id) || (g_sock && id.PART == 1 && emu_find(soc));
}

/* the kernels the last emu_solve_batch* call ran, as the template arguments of solve_kernel in the ladder's terms (before stand_in):
 * "first=NT,SPT,WPS,DYN,STREAM,GEN,FULL,PART,SLDS,SOCK follow=..." (NT = 0: none ran) */
static char g_last[256];
extern "C" const char *emu_last_kernels(void) { return g_last; }
static int put_id(char *p, const char *name, const msd::KernelId &k)
{
    return sprintf(p, "%s=%d,%d,%d,%d,%d,%d,%d,%d,%d,%d ", name, k.NT, k.SPT, k.WPS, k.DYN, (int)k.STREAM, (int)k.GEN, k.FULL, k.PART, (int)k.SLDS, (int)k.SOCK);
}

/* primal-dual warm starts in the emulation: buffers for the next emu_solve_batch* call (dual_in already points at the first node used) */
static const double *g_dual_in = nullptr;
static double *g_dual_out = nullptr;
static long long g_dual_stride = 0;
extern "C" void emu_set_duals(const double *dual_in, long long stride, double *dual_out) { g_dual_in = dual_in; g_dual_stride = stride; g_dual_out = dual_out; }

extern "C" int emu_solve_batch_warm(const msd_problem_desc *d, int nscen, const double *scen, const double *ovr, const double *guess, double mu0, double push,
                                   double *z, double *lam, double *stats, double *hist, int cap)
{
    using namespace msd_host;
    /* the problem record like the library fills it (msd_select.hpp), the profile pointers straight from the description */
    msd::DevProb P;
    fill_problem(P, d);
    P.guess = guess; P.guessStride = (4 + d->with_pn_brake)*d->num_intervals + 2; P.warmMu = mu0; P.warmPush = push;
    P.dualOut = g_dual_out; P.dualIn = guess ? g_dual_in : nullptr; P.dualInStride = g_dual_stride;
    std::vector<double> pos(d->num_intervals + 1, 0.0);
    for (int i = 0; i < d->num_intervals; i++) pos[i + 1] = pos[i] + d->ds[i];
    P.pos = pos.data(); P.ds = d->ds; P.grad = d->grad; P.curv = d->curv; P.bmax = d->bmax; P.loss = d->loss_table; P.coll = d->coll_tables;
    EmuArgs a = {P, nscen, scen, ovr, z, lam, stats, hist, cap};
    g_last[0] = 0;

    /* the kernels like the library picks them (msd_api.hip: select_plan): the same family, structure and ladder; EMU_NO_FULL=1 is msd_tuning("no_full", 1).
     * EMU_GEOMETRY=stream: the long-horizon kernels (stage blocks in memory) whatever the horizon */
    const Family family = family_of(d);
    const int structure = structure_of(d), N = d->num_intervals;
    Tuning tuning;
    tuning.no_full = env_set("EMU_NO_FULL");
    const char *force = getenv("EMU_GEOMETRY");      /* "NTxSPT": that geometry whatever the horizon (Tuning::NT, SPT) */
    const bool force_stream = force && !strcmp(force, "stream");
    if (force && !force_stream) sscanf(force, "%dx%d", &tuning.NT, &tuning.SPT);
    /* (msd_api.hip: launch_plan) every scenario can start without the least-squares multiplier estimate: profile start, primal-dual warm start */
    const bool plain = P.guess ? P.dualIn != nullptr : P.start == MSD_START_PROFILE;
    g_sock = plain && env_set("EMU_SOCK");
    msd::Geometry g = force_stream ? streamed(family, N, structure, tuning) : resident(family, N, structure, tuning);
    if (!g.first || N + 1 > stand_in(g.first).NT*stand_in(g.first).SPT) return -3;
    const bool fused = g.xch == msd::XCH_FAST;
    if (!g.follow) g.follow = streamed(family, N, structure, tuning).follow;      /* a first-pass kernel: the streamed kernel of the family follows up */

    /* the launch like launch_plan does it.  The first pass of a fused family -- EMU_SOCK=1: the one with the second-order correction inside -- where the
     * launch is plain, the one behind the estimate otherwise (none: the follow-up kernel takes the whole batch); then the follow-up kernel over the
     * list the first pass left.  EMU_MONOLITHIC=1: the kernel of a fused family with everything in it (PART = 0) instead; EMU_NO_FOLLOW=1: the first pass
     * alone (a test that a scenario needs no follow-up kernel) */
    msd::KernelId first = (!fused || plain) ? ((g_sock && emu_find(g.soc)) ? g.soc : g.first) : g.lsq ? g.lsq : g.follow, follow = g.follow;
    if (env_set("EMU_MONOLITHIC") && fused) { first = g.first; first.PART = 0; first.SLDS = false; }
    if (first.PART == 0 || first.PART == 2 || env_set("EMU_NO_FOLLOW")) follow = msd::KernelId{};
    const EmuFn run_first = emu_find(first), run_follow = emu_find(follow);
    if (!run_first || (follow && !run_follow)) return -3;
    put_id(g_last + put_id(g_last, "first", first), "follow", follow);
    std::vector<int> list(msd::FOLLOW_HDR + 2*(size_t)nscen, 0);
    if (follow || first.PART == 1 || first.PART == 3) a.P.follow = list.data();
    run_first(a, g);
    if (!run_follow) return 0;
    a.P.list = list.data(); a.P.follow = nullptr;
    run_follow(a, g);
    return 0;
}
extern "C" int emu_solve_batch_ex(const msd_problem_desc *d, int nscen, const double *scen, const double *ovr, double *z, double *lam, double *stats, double *hist, int cap)
{
    return emu_solve_batch_warm(d, nscen, scen, ovr, nullptr, 0.0, 0.0, z, lam, stats, hist, cap);
}
extern "C" int emu_solve_batch(const msd_problem_desc *d, int nscen, const double *scen, double *z, double *lam, double *stats, double *hist, int cap)
{
    return emu_solve_batch_ex(d, nscen, scen, nullptr, z, lam, stats, hist, cap);
}
