// gc_blocksum.h — the xor-tree family of fixed-order sums (device code only).
//
// The library has two families of reproducible workgroup sums, and they give DIFFERENT BITS for the
// same inputs, because they add in different trees. Neither can stand in for the other.
//
//  gc_wgla.h     wave_sum / wg_sum / wg_sum_n: DPP quad and mirror steps inside each 16-lane row, the
//                four row totals by readlane as (r0 + r1) + (r2 + r3), the four waves as
//                (w0 + w1) + (w2 + w3). Used by gc_points.hip, gc_bins.hip, gc_binstask.h, gc_evidence.hip, gc_ops.hip, gc_opsdev.h,
//                gc_belief.hip, gc_budget.h and gc_iofactors.h.
//  this header   an xor butterfly inside the wave (__shfl_xor, off = 32..1: each step adds to a lane's
//                partial the partial of lane ^ off, which covers a disjoint set of lanes; a + b = b + a,
//                so both partners, and in the end all lanes, hold the same bits), then the waves in wave
//                order, then the workgroups by sum_partials. Used by gc_assoc.hip, gc_vpe.hip,
//                gc_surfel.hip, gc_camsplat.hip and, for the wave step alone, gc_depthsurfel.hip (one wave
//                per cell) and gc_mapops.hip (whose block_partials adds its four waves pairwise and says why).
//
// The run-to-run bit identity of these operators, and a batch row being equal to the single call, rest
// on the order written here: lane-local sums in index order first (the caller's loop), no floating-point
// atomics anywhere. tests/test_gpu_ops_parent_bits.py pins the bits.
//
// Every function that takes LDS must be called by all threads of the workgroup, in workgroup-uniform
// control flow (it has barriers). group_sum_xor has none: the lanes of a group must be active together.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gc {

// Sum of x over the aligned group of WIDTH lanes the lane belongs to (64: the wave), on every lane of
// the group: the butterfly off = WIDTH/2 .. 1.
template <int WIDTH, typename T>
__device__ __forceinline__ T group_sum_xor(T x) {
  static_assert(WIDTH >= 2 && WIDTH <= 64 && (WIDTH & (WIDTH - 1)) == 0, "a power of two inside the wave");
#pragma unroll
  for (int off = WIDTH / 2; off >= 1; off >>= 1) x += __shfl_xor(x, off, 64);
  return x;
}

// The two halves of block_sum, for a kernel that wants each total on one thread only (thread q stores
// total q: k_vpe_collapse, k_sf_center) and would otherwise hold all NV totals in registers on every
// thread. block_sum_stage: the wave butterflies, lane 0 of each wave writes red, a barrier.
// block_sum_total: value q's waves in wave order from wave 0's value. Such a caller places no trailing
// barrier and must not reuse red before one.
template <int NV>
__device__ __forceinline__ void block_sum_stage(const double (&v)[NV], double* red) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  // every butterfly before the one branch that writes: a write under `if (lane == 0)` after each value
  // keeps the NV independent shuffle chains from overlapping (profiles/r12/ops_parent_vs_current.json)
  double x[NV];
#pragma unroll
  for (int q = 0; q < NV; ++q) x[q] = group_sum_xor<64>(v[q]);
  if (lane == 0) {
#pragma unroll
    for (int q = 0; q < NV; ++q) red[wv * NV + q] = x[q];
  }
  __syncthreads();
}
template <int NV, int WAVES>
__device__ __forceinline__ double block_sum_total(const double* red, int q) {
  double x = red[q];
  for (int w = 1; w < WAVES; ++w) x += red[w * NV + q];
  return x;
}

// NV sums over a workgroup of WAVES waves; the totals replace v on every thread.
// red: WAVES * NV doubles of LDS, not live on entry. Lane 0 of each wave writes its wave's totals, a
// barrier, then every thread adds the waves' values in wave order STARTING FROM WAVE 0's VALUE, and a
// trailing barrier, so red may be reused as soon as the call returns.
//
// Starting from wave 0's value and starting from 0.0 differ on one input only: a wave-0 total of -0.0
// with every other wave total a zero too (0.0 + -0.0 is +0.0). The callers that used to start from 0.0
// (gc_assoc.hip, gc_vpe.hip, gc_surfel.hip) build every per-thread value by `+=` from +0.0, and in
// round-to-nearest x + y is -0.0 only for x = y = -0.0, so neither a lane's value nor a butterfly's
// result can be -0.0 there and both forms give the same bits. (A contracted multiply-add whose exact
// result underflows could round to -0.0; that needs every contribution of a total to underflow, and the
// only difference then is the sign of a zero.)
template <int NV, int WAVES>
__device__ __forceinline__ void block_sum(double (&v)[NV], double* red) {
  block_sum_stage<NV>(v, red);
#pragma unroll
  for (int q = 0; q < NV; ++q) v[q] = block_sum_total<NV, WAVES>(red, q);
  __syncthreads();
}

// The second pass: the totals of NV <= COLS values over G per-workgroup partials (partial[b * NV + q]) by
// one workgroup of T threads, in an order that depends on G alone. Thread (c = tid / COLS, q = tid % COLS)
// adds value q of the workgroups c, c + T/COLS, ... (T/COLS independent chains keep the loads in
// flight); threads < NV then add the chains in the order c = 0, 1, ... from 0.0. stage: T doubles of
// LDS, tot: NV doubles of LDS, neither live on entry; tot holds the totals for every thread on return.
template <int COLS, int T>
__device__ __forceinline__ void sum_partials(int G, const double* __restrict__ partial, int NV, double* stage,
                                             double* tot) {
  static_assert(T % COLS == 0, "whole chains");
  const int q = threadIdx.x % COLS, c = threadIdx.x / COLS;
  double t = 0.0;
  if (q < NV) {
#pragma unroll 4
    for (int b = c; b < G; b += T / COLS) t += partial[(int64_t)b * NV + q];
  }
  stage[threadIdx.x] = t;
  __syncthreads();
  if ((int)threadIdx.x < NV) {
    double x = 0.0;
    for (int cc = 0; cc < T / COLS; ++cc) x += stage[cc * COLS + threadIdx.x];
    tot[threadIdx.x] = x;
  }
  __syncthreads();
}

}  // namespace gc
