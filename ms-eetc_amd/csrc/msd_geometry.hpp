/*
 * msd_geometry.hpp -- which solve kernel (KernelId: data, no device, no function pointer) and the launch geometry built from such ids (Geometry).
 * The ladder that picks a Geometry by family and horizon is msd_select.hpp (host only); the instantiations live in the translation units
 * msd_kernels_*.hip -- split so that they compile in parallel --, each of which exports one lookup from KernelId to the kernels it holds.
 */
#pragma once

#include "msd_kernel.hpp"

namespace msd {

using KernelFn = void (*)(DevProb, int, const double *, const double *, double *, double *, double *, double *, int, double *);

/* the template arguments of solve_kernel (same order, same defaults); NT == 0: no kernel */
struct KernelId {
    int NT = 0, SPT = 0, WPS = 1, DYN = LOSS_STATIC;
    bool STREAM = false, GEN = false;
    int FULL = 0, PART = 0;
    bool SLDS = false, SOCK = false, EARLY = false;
    explicit operator bool() const { return NT != 0; }
};
inline bool operator==(const KernelId &a, const KernelId &b)
{
    return a.NT == b.NT && a.SPT == b.SPT && a.WPS == b.WPS && a.DYN == b.DYN && a.STREAM == b.STREAM && a.GEN == b.GEN && a.FULL == b.FULL && a.PART == b.PART
           && a.SLDS == b.SLDS && a.SOCK == b.SOCK && a.EARLY == b.EARLY;
}

/* one entry of a unit's lookup `KernelFn kernels_<unit>(const KernelId &id)`: the instantiation with these template arguments lives in this unit */
#define MSD_KERNEL(...) if (id == KernelId{__VA_ARGS__}) return solve_kernel<__VA_ARGS__>;
/* ... its twin with the early results inside (solve_kernel_early: the id with EARLY set) */
#define MSD_KERNEL_EARLY(...) if (KernelId twin_{__VA_ARGS__}; (twin_.EARLY = true, id == twin_)) return solve_kernel_early<__VA_ARGS__>;
/* ... and an instantiation the unit compiles that no rung of the ladder picks (it was instantiated when the ladder was a template over the loss model): kept, so that
 * the unit's code object stays what it was; the host side drops it */
#define MSD_KERNEL_UNUSED(...) if (false) return solve_kernel<__VA_ARGS__>;

/* the kernels of one solve: NT threads per workgroup, SPT shooting nodes per thread (NT*SPT >= N + 1) -- those of `first` */
struct Geometry {
    KernelId first;                      /* complete kernel, or the first pass of a split solve (solve_kernel's PART = 1) */
    KernelId follow;                     /* the follow-up kernel of a split solve (PART = 2), with its own NT and SPT: it restarts a scenario from its starting point, so nothing ties its geometry to the first pass's */
    KernelId lsq;                        /* first pass with the least-squares multiplier estimate in front (PART = 3): launches from the reference's starting point or a primal-only warm start */
    KernelId soc;                        /* `first` with the second-order correction inside the fused iteration (SOCK: msd_kernels_full4.hip), same launch */
    /* the twins of first / lsq / soc that hold the early results (solve_kernel: EARLY), same launch: the fused family's first passes have them;
     * everywhere else the kernel itself tests for them at run time and is its own twin */
    KernelId early(const KernelId &k) const { KernelId e = k; if (k && xch == XCH_FAST && (k.PART == 1 || k.PART == 3)) e.EARLY = true; return e; }
    bool stream = false;                 /* stage blocks in device memory (long horizons) */
    int xch = XCH_GENERAL;               /* exchange arrays in LDS and cross-wave reduction scratch (lds_doubles) */
    int red = RED_DOUBLES;
    int extra = 0;                       /* doubles of LDS behind the layout of lds_doubles (the SLDS instantiations' node constants) */
};

}  // namespace msd
