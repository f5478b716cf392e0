/* TEST-ONLY: host emulation, the twins of kernel family "full" (msd::solve_kernel_early: the early results inside and the integrator chosen at run time).
 * Not a unit of the default build: tests/test_fused_first_pass_emulation.py builds it, with emu_k_first_pass.cpp, through UNITS of build.sh */
#include "emu_common.h"

/* run_blocks of emu_common.h for msd::solve_kernel_early (same launch, same LDS as the default kernel) */
template <int NT, int SPT, int WPS, int DYN, bool STREAM = false, bool GEN = false, int FULL = 0, int PART = 0, bool SLDS = false, bool SOCK = false>
static void run_blocks_early(const EmuArgs &a, const msd::Geometry &g)
{
    const msd::DevProb &P = a.P;
    const int nscen = a.nscen;
    for (int b = 0; b < nscen; b++) {
        emu_block blk;
        blk.nthreads = NT;
        pthread_barrier_init(&blk.bar, nullptr, NT);
        std::vector<double> shfl(NT), xch((size_t)NT*EMU_XCH), lds(msd_host::lds_bytes(g, msd::KernelId{NT, SPT, WPS, DYN, STREAM, GEN, FULL, PART, SLDS, SOCK}, P.N)/sizeof(double));
        blk.shfl = shfl.data(); blk.xch = xch.data(); blk.lds = lds.data();
        std::vector<double> work(msd::work_doubles(NT*SPT)*(size_t)nscen);
        std::vector<std::thread> th;
        for (int t = 0; t < NT; t++)
            th.emplace_back([&, t]() {
                threadIdx = {(unsigned)t, 0, 0}; blockIdx = {(unsigned)b, 0, 0}; blockDim = {(unsigned)NT, 1, 1}; gridDim = {(unsigned)nscen, 1, 1};
                emu_blk = &blk;
                msd::solve_kernel_early<NT, SPT, 1, DYN, STREAM, GEN, FULL, PART, SLDS, SOCK>(P, nscen, a.scen, a.ovr, a.z, a.lam, a.stats, a.hist, a.cap, work.data());
            });
        for (auto &t : th) t.join();
        pthread_barrier_destroy(&blk.bar);
    }
}
#define EMU_KERNEL_EARLY(...) if (msd::KernelId twin_{__VA_ARGS__}; (twin_.EARLY = true, id == twin_)) return run_blocks_early<__VA_ARGS__>;

EmuFn emu_kernels_full_early(const msd::KernelId &id)
{
    EMU_KERNEL_EARLY(64, 1, 1, msd::LOSS_STATIC, false, false, msd::FULL_RG, 1)
    EMU_KERNEL_EARLY(64, 1, 1, msd::LOSS_STATIC, false, false, msd::FULL_RG, 3)
    EMU_KERNEL_EARLY(64, 2, 1, msd::LOSS_STATIC, false, false, msd::FULL_RG, 1)
    EMU_KERNEL_EARLY(64, 1, 1, msd::LOSS_STATIC, false, false, msd::FULL_BOTH, 1)
    EMU_KERNEL_EARLY(64, 1, 1, msd::LOSS_STATIC, false, false, msd::FULL_BOTH, 3)
    EMU_KERNEL_EARLY(64, 2, 1, msd::LOSS_STATIC, false, false, msd::FULL_BOTH, 1)
    EMU_KERNEL_EARLY(64, 2, 1, msd::LOSS_STATIC, false, false, msd::FULL_BOTH, 3)
    return nullptr;
}
