/*
 * TEST-ONLY: shared part of the host emulation (see emu_driver.cpp).  run_blocks<...> runs one instantiation of msd::solve_kernel on host
 * threads; the instantiations are spread over one translation unit per kernel family (emu_k_*.cpp) so that they compile in parallel --
 * an AddressSanitizer build of a single unit took twenty minutes.
 */
#pragma once
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "../../ms-eetc_amd/csrc/msd_kernel.hpp"

/* MemorySanitizer build (tests/hip_emu/build_msan.sh, emu_msan_main.cpp): LDS and work area of an emulated workgroup start as uninitialised memory, so a
 * read of shared memory before its first write is reported where it decides something -- with the origin of the value -- instead of showing as a NaN */
#if defined(__has_feature)
#if __has_feature(memory_sanitizer)
#include <sanitizer/msan_interface.h>
#define EMU_POISON_SHARED(p, n) __msan_poison((p), (n))
#endif
#endif
#ifndef EMU_POISON_SHARED
#define EMU_POISON_SHARED(p, n) ((void)0)
#endif


#include "../../ms-eetc_amd/csrc/msd_select.hpp"

struct EmuArgs { msd::DevProb P; int nscen; const double *scen, *ovr; double *z, *lam, *stats, *hist; int cap; };

/* one instantiation of the kernel (template arguments: solve_kernel's; the emulation compiles every one with WPS = 1) launched as part of the picked
 * geometry `g`, which says how the LDS is laid out -- exactly the LDS the library's launch allocates (msd_select.hpp: lds_bytes) */
template <int NT, int SPT, int WPS, int DYN, bool STREAM = false, bool GEN = false, int FULL = 0, int PART = 0, bool SLDS = false, bool SOCK = false>
void run_blocks(const EmuArgs &a, const msd::Geometry &g)
{
    const msd::DevProb &P = a.P;
    const int nscen = a.nscen;
    for (int b = 0; b < nscen; b++) {
        emu_block blk;
        blk.nthreads = NT;
        pthread_barrier_init(&blk.bar, nullptr, NT);
        std::vector<double> shfl(NT), xch((size_t)NT*EMU_XCH), lds(msd_host::lds_bytes(g, msd::KernelId{NT, SPT, WPS, DYN, STREAM, GEN, FULL, PART, SLDS, SOCK}, P.N)/sizeof(double));
        /* EMU_POISON=1 (environment): LDS and work area start as NaN instead of zero -- a read of shared memory before its first write, which on the
         * device sees whatever the kernel before left there, then shows in the results */
        const char *poison = getenv("EMU_POISON");
        if (poison && *poison == '1') std::fill(lds.begin(), lds.end(), std::nan(""));
        EMU_POISON_SHARED(lds.data(), 8*lds.size());
        blk.shfl = shfl.data(); blk.xch = xch.data(); blk.lds = lds.data();
        std::vector<double> work((STREAM ? msd::stream_doubles(P.N, NT*SPT, DYN != 0) : msd::work_doubles(NT*SPT))*(size_t)nscen);
        if (poison && *poison == '1') std::fill(work.begin(), work.end(), std::nan(""));
        EMU_POISON_SHARED(work.data(), 8*work.size());
        std::vector<std::thread> th;
        for (int t = 0; t < NT; t++)
            th.emplace_back([&, t]() {
                threadIdx = {(unsigned)t, 0, 0}; blockIdx = {(unsigned)b, 0, 0}; blockDim = {(unsigned)NT, 1, 1}; gridDim = {(unsigned)nscen, 1, 1};
                emu_blk = &blk;
                msd::solve_kernel<NT, SPT, 1, DYN, STREAM, GEN, FULL, PART, SLDS, SOCK>(P, nscen, a.scen, a.ovr, a.z, a.lam, a.stats, a.hist, a.cap, work.data());
            });
        for (auto &t : th) t.join();
        pthread_barrier_destroy(&blk.bar);
    }
}

/* the lookups of the units (emu_k_<unit>.cpp: emu_kernels_<unit>), like those of the library's kernel units: nullptr when the unit does not hold the kernel.
 * The streamed kernels are a stand-in geometry the emulation can afford, 128 x 5 (emu_driver.cpp: stand_in) */
using EmuFn = void (*)(const EmuArgs &a, const msd::Geometry &g);
#define EMU_KERNEL(...) if (id == msd::KernelId{__VA_ARGS__}) return run_blocks<__VA_ARGS__>;
