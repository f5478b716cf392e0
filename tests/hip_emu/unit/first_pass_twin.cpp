/* TEST-ONLY: the rule of msd_select.hpp that picks the first pass of a launch, printed for the argument tuples on the command line:
 *   first_pass_twin <fused_family> <early> <numSteps> <numApprox> [...]  ->  one 0 / 1 per tuple */
#include "../emu_common.h"

thread_local emu_dim3 threadIdx, blockIdx, blockDim, gridDim;
thread_local emu_block *emu_blk;
bool msd_host::has_kernel(const msd::KernelId &) { return false; }

int main(int argc, char **argv)
{
    for (int k = 1; k + 3 < argc; k += 4)
        printf("%d\n", msd_host::first_pass_twin(atoi(argv[k]) != 0, atoi(argv[k + 1]) != 0, atoi(argv[k + 2]), atoi(argv[k + 3])) ? 1 : 0);
    return 0;
}
