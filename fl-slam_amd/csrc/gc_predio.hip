// gc_predio.hip — the front half of a GC_LIDAR_GIVEN scan after the predict launch: one workgroup of
// 256 per local hypothesis runs what workgroups [0, n_io) of k_bins_io run on the bins path (the
// predict's L_pred half, then the IMU/odom branch: the same routines on the same operands, so their
// outputs are the bins path's bits), then forms the linearisation pose the map branch's
// visual_pose_evidence takes (z_lin_pose, backend/pipeline.py:751-755). There are no bin tasks.
#include <hip/hip_runtime.h>
#include <algorithm>
#include "gc_internal.h"
#include "gc_pipe.h"
#include "gc_wgla.h"
#include "gc_opsdev.h"
#include "gc_iobranch_wg.h"

namespace gc {

// the tail's LDS (doubles), carved from the start of the branch's dead scratch: M | Mp | Cl |
// projection scratch 2 N2 + 4 n | b n | x n | red 16 | cert 8
constexpr int kLinLdsDoubles = 5 * kIoN2 + 4 * kDZ + 2 * kDZ + 16 + 8;
constexpr int kPredIoLdsDoubles =
    std::max(std::max(kLpredLdsDoubles, kIoLdsDoubles), kLinLdsDoubles);

__global__ void __launch_bounds__(256) k_pred_io(PipeDev P, ScanArgs S, const double* __restrict__ odom, int io_on) {
  extern __shared__ double lds[];
  constexpr int n = kDZ, N2 = kIoN2;
  const int hl = blockIdx.x, t = threadIdx.x;
  lpred_wg(P, S, hl, lds);
  if (io_on) io_branch_wg(P, S, odom, hl, lds);
  // L_pred / h_pred (pred_mode 0) and L_io / h_io were written by this workgroup: visible to all of it
  // after the barrier, and the branch's LDS is dead
  __syncthreads();
  // nothing after this point reads the scan slot, and no later launch of a GC_LIDAR_GIVEN scan does:
  // the last workgroup to arrive publishes the scan's ticket (the slot may be restaged). The counter is
  // the bins launch's task counter, which the predict launch re-arms every scan and this mode leaves
  // unused. No workgroup waits on another.
  if (t == 0 && S.done_word) {
    const unsigned prev = __hip_atomic_fetch_add(P.task_ctr, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    if (prev == gridDim.x - 1)
      __hip_atomic_store(S.done_word, S.ticket, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  // z_lin_pose (pipeline.py:751-755): L_f = PSD(L_pred + L_io), z = (L_f + ε_l I)⁻¹ (h_pred + h_io), by the
  // certified projection with its lifted factor and the lifted solve, as k_evidence does for L_post
  double* M = lds;
  double* Mp = M + N2;
  double* Cl = Mp + N2;
  double* Sx = Cl + N2;  // 2 N2 + 4 n
  double* b = Sx + 2 * N2 + 4 * n;
  double* x = b + n;
  double* red = x + n;   // 16
  double* c6 = red + 16;  // 8
  for (int i = t; i < N2; i += kWG) M[i] = P.Lpred[(int64_t)hl * N2 + i] + P.io_L[(int64_t)hl * N2 + i];
  if (t < n) b[t] = P.hpred[(int64_t)hl * n + t] + P.io_h[(int64_t)hl * n + t];
  __syncthreads();
  wg_psd_fast_lifted_chol(M, Mp, P.eps_psd, P.eps_lift, n, Sx, Cl, red, c6);
  __syncthreads();
  wg_chol_solve(Cl, b, x, n);
  if (t < 6) P.lin_pose[(int64_t)hl * 6 + t] = x[t];
}

hipError_t launch_pred_io(const PipeDev& P, const ScanArgs& S, const double* d_odom, bool io, hipStream_t st) {
  const size_t sh = sizeof(double) * (size_t)kPredIoLdsDoubles;
  if (sh > 65536)
    if (hipError_t e = ensure_dyn_lds((const void*)k_pred_io, sh)) return e;
  hipLaunchKernelGGL(k_pred_io, dim3(P.Hl), dim3(256), sh, st, P, S, d_odom, io ? 1 : 0);
  return hipGetLastError();
}

}  // namespace gc
