/*
 * mseetc_aux.h -- measurement aids of the C ABI (no counterpart in the reference: its only timing is IPOPT's t_wall_total, ocp.py:362).
 */
#ifndef MSEETC_AUX_H
#define MSEETC_AUX_H

#include "mseetc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * With `on`, every launch of the handle records HIP events around its first kernel alone (the first pass of a split solve, or the one kernel of
 * the others); msd_problem_first_pass_ms waits for the stream and returns the mean duration over the last launches (at most 64) -- the
 * dominant kernel's own time, next to the time of whole launches that msd_timer_begin / msd_timer_end bracket (bench.py: roofline).
 */
int msd_problem_time_first_pass(msd_handle h, int on);
int msd_problem_first_pass_ms(msd_handle h, float *mean_ms, int *launches);

/*
 * Page-locked host memory for the result arrays of msd_solve_batch: copies from the device into it run at the link's rate and need no staging
 * (into pageable memory they are staged and page-faulted: 34 MB of results per 8192 scenarios at N = 100 cost 2.8 ms instead of 0.7 ms).
 * mseetc/_device.py hands such arrays out as numpy arrays and reuses a buffer once nobody holds its array any more.
 */
int msd_host_alloc(unsigned long long bytes, void **ptr);
int msd_host_free(void *ptr);

/*
 * With `on`, a host-buffer call (msd_solve_batch, _ex, _warm, _multi) whose z_out -- and lam_out, if given -- lie in page-locked memory the device can
 * address (msd_host_alloc, hipHostMalloc, hipHostRegister) has the kernels store the results there themselves: every scenario's z* crosses the link when
 * that scenario is done, spread over the launch, and no copy waits behind the last one (config 1 on MI355X: 0.99 x the device-resident rate instead of
 * 0.89 x; same bits).  Arrays in pageable memory are served by copies as before.  The handle then keeps no device copy of such a solve:
 * msd_solve_batch_shifted right after it fails with MSD_E_INVALID -- a loop of shifted re-solves leaves the switch off (mseetc/mpc.py does); a handle with
 * msd_problem_keep_duals on is such a loop's and is served by copies whatever the switch says.  Default: off.
 * (The reference hands back host arrays, ocp.py:359-380: this is the boundary's own cost)
 */
int msd_problem_direct_results(msd_handle h, int on);

/*
 * Tuning switches of the kernel pickers for the problems created afterwards (process-wide; A/B measurements and one GPU test -- the library itself reads no
 * environment variable).  "no_full" != 0: the kernels without the structure of the NLP compiled in; "two_nodes_per_lane" != 0: the 64 x 2 geometry for
 * horizons of 64 ... 127 intervals of the shooting-integrator and integrateLosses families (default 128 x 1); "geometry" = 16 NT + SPT: every rung of the
 * ladder offers NT threads with SPT nodes each instead of its own geometry, whatever the horizon (0: off; a GPU test runs short horizons on the 64 x 2
 * kernels with it).  Unknown name: MSD_E_INVALID.
 */
int msd_tuning(const char *name, int value);

/*
 * The launch plan the library selects for a description, as one line of text in buf (len bytes): family, structure, NT SPT lds_bytes stream fused_family
 * work_doubles nz nl, NT2 SPT2 lds_bytes2 and the symbol names of the first-pass kernel, the least-squares first pass, the follow-up kernel and the candidate
 * with the second-order correction inside ("-": none; whether the candidate is taken depends on the device's occupancy).  Makes no device call.  A
 * description msd_problem_create would reject gets the same code and msd_last_error() here (tests/test_abi.py pins the table).
 */
int msd_plan_describe(const msd_problem_desc *desc, char *buf, int len);

/*
 * The symbol name of the first kernel of the handle's last launch, in buf (len bytes; "-": the handle has launched nothing yet): the first pass of a split
 * solve, or the one kernel of the others.  The first passes of the fused family exist twice -- the default kernels, and twins with the early results inside
 * that a begun batch (msd_solve_batch_begin) or an iteration budget (msd_problem_iteration_budget) launches; the tests see here which one ran.
 */
int msd_problem_last_first_pass(msd_handle h, char *buf, int len);

/*
 * The rows of speed limits the handle holds (msd_problem_speed_restrictions), as limit_rows_kernel built them: rows[nscen][N+1] (host), nscen of the call that set
 * them.  Waits for the handle's stream.  MSD_E_INVALID when the handle holds none.  (tests/test_speed_restrictions_gpu.py: bit for bit the host statement of the
 * rule, casadiSolver.restrictedLimits)
 */
int msd_problem_limit_rows(msd_handle h, double *rows);

/*
 * Test hook: the reciprocal and the square root / reciprocal square root of the fused interior-point iteration (csrc/msd_fastmath.hpp: v_rcp_f64 /
 * v_rsq_f64 refined without the compiler's range scaling) evaluated on n operands, so that the GPU tests can bound their error against the IEEE
 * operations (tests/test_gpu_parity.py::test_fast_reciprocal_and_square_root: <= 1 ulp on normal operands).  Errors: msd_interval_last_error().
 */
int msd_fastmath_probe(int device, int n, const double *x, double *rcp_out, double *sqrt_out, double *rsqrt_out);

/*
 * Test hook: the reduction over a workgroup that every solver kernel uses (csrc/msd_kernel.hpp: block_reduce<K>), run once by one workgroup of
 * `nthreads` threads (64, 128 or 256) on K values per thread (K = 1, 2, 4, 5, 6 or 8); op 0: sum, 1: maximum, 2: minimum.  Thread t brings
 * in[k*nthreads + t], k < K; out[k*nthreads + t] is what it holds afterwards (tests/test_wave_reduce_gpu.py: in every thread bit for bit the balanced
 * tree over aligned blocks of lanes, the waves' totals folded in their order).  Anything else: MSD_E_INVALID.  Errors: msd_interval_last_error().
 */
int msd_reduce_probe(int device, int nthreads, int K, int op, const double *in, double *out);

#ifdef __cplusplus
}
#endif
#endif
