// gc_bins.hip — the bins kernels that read the table exp (gfx950), and the exp table they share.
//
//  a5 BinSoftAssign         archive/legacy_operators/binning.py:56-131
//  a1 -> a4 -> a5 -> a6 fused: the grid form (gc_scan_bins_fused) and the batched pipeline's persistent
//  form with the IMU/odom branch's workgroups in the same launch (scan_bins_pipeline); the task body is
//  gc_binstask.h, the task tiers gc_binplan.h, the a6 contract kernel and the finalizes gc_moments.hip.
//  domain_projection_psd_core for any d (gc_domain_projection_psd_batch): kept beside k_bins_io, see there.
//
// Layout / mapping: a wave processes 4 points per step; its 64 lanes
// are 4 point-groups x 16 bin-lanes, bin-lane l owns bins {l, l+16, l+32, ...}. Per-point
// softmax sums are 16-lane DPP sums (butterflies; in the fused kernel a reduce-scatter over two steps
// at a time); per-bin moment accumulators live in VGPRs for the whole chunk and are reduced across
// groups/waves once, in a fixed order, into one partial record per (hypothesis, chunk). A finalize kernel sums the records in chunk order, so every
// result is bit-reproducible run to run (no float atomics anywhere).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <type_traits>
#include "gc_internal.h"
#include "gc_binsdev.h"
#include "gc_binstask.h"
#include "gc_binplan.h"
#include "gc_iobranch_wg.h"

namespace gc {

// The table formed once per context on the device (gc_ctx_create -> init_exp_table) by the same
// exp_table2_init the workgroups used to run themselves: a workgroup now copies 16 KB from L2 instead
// of evaluating 2048 exp2 (~2 us at the start of every bins launch), the same bits.
__device__ __attribute__((aligned(16))) double g_exp_tab2[kExpTab2];
__global__ void __launch_bounds__(256) k_exp_table_init() { exp_table2_init(g_exp_tab2); }
GC_DEV void exp_table2_load(double* T) {
  typedef double dvec2 __attribute__((ext_vector_type(2)));
  for (int j = threadIdx.x; j < kExpTab2 / 2; j += blockDim.x)
    reinterpret_cast<dvec2*>(T)[j] = reinterpret_cast<const dvec2*>(g_exp_tab2)[j];
}
hipError_t init_exp_table(hipStream_t st) {
  hipLaunchKernelGGL(k_exp_table_init, dim3(1), dim3(256), 0, st);
  return hipGetLastError();
}

// Un-fused similarity: the bin-index integer contract (argmax of exactly this f64 expression).
GC_DEV double sim_nofma(double d0, double d1, double d2, double b0, double b1, double b2) {
#pragma clang fp contract(off)
  double s = d0 * b0 + d1 * b1;
  s = s + d2 * b2;
  return s;
}

// ============================================================================ a5 soft assign
// grid (chunks, H), chunk = iters*256 points; each wave owns 64 points per iteration with
// lane = point: the 16*BPL similarities, exps and the softmax sum of a point stay in one lane
// (no cross-lane reductions) and the bin directions are wave-uniform LDS reads.
// The bin index is a running argmax in bin order (lowest index on ties).
// FULL (B == 16 BPL <= 48): the normalised rows leave through a wave-private LDS slab one half-wave at a
// time: 32 rows of B doubles (row stride B + 2: the 8 lanes of a ds_write_b128 group hit disjoint
// banks) go out as the contiguous 32·B·8-byte block they form in HBM, 16 B per lane, 1 KiB per store
// instruction. Ragged B and B = 64: the rows are transposed one 16-bin block at a time (row stride 18) and leave
// as 128-B row segments, 8 B per lane.
// One 16-bin block of a wave's 64 normalised rows, from the LDS transpose slab (row stride 18) to
// HBM as 128-B row segments: 16 B per lane (FULL, B == 16 BPL) or 8 B per lane (ragged B).
template <int BPL, bool FULL>
GC_DEV void sa_store_block(const double* S, double* Rh, int64_t wbase, int64_t n, int B, int blk, int lane) {
  typedef double dvec2 __attribute__((ext_vector_type(2)));
  constexpr int NB = 16 * BPL, RS = 18;
  if constexpr (FULL) {
    // lane writes pieces (point 8m + lane/8, bins 16 blk + 2 (lane%8) +{0,1}); B == NB
    const int i0 = lane >> 3, q = lane & 7;
    double* rowp = Rh + (wbase + i0) * NB + 16 * blk + 2 * q;
    const int64_t lim = n - wbase - i0;
#pragma unroll
    for (int m = 0; m < 8; ++m) {
      const dvec2 v = *reinterpret_cast<const dvec2*>(&S[(i0 + 8 * m) * RS + 2 * q]);
      if (8 * m < lim) *reinterpret_cast<dvec2*>(rowp + 8 * m * NB) = v;
    }
  } else {
#pragma unroll
    for (int m = 0; m < 16; ++m) {
      const int e = lane + 64 * m, i = e >> 4, k = e & 15;
      const double v = S[i * RS + k];
      if (wbase + i < n && 16 * blk + k < B) Rh[(wbase + i) * B + 16 * blk + k] = v;
    }
  }
}
// 2 waves per SIMD: the 48 similarities / exps of a lane's point stay in registers with no spill
// (at 3, the 168-VGPR budget spilled ~12-27 VGPRs per point to scratch: 0.6 GB of extra HBM reads and
// 0.9 GB of extra writes per C3 launch, tools/probe/probe_sa3.hip; 1.74 -> 1.32 ms)
constexpr int kSaOcc = 2;
// the responsibility rows leave by non-temporal stores: plain stores and an inline-asm sc1 write-through were
// tried, sc1 taking the kernel 1.39 -> 1.33 ms (the soft-assign / moment pair's roofline fraction 0.673 ->
// 0.676) but writing wrong values on a ragged tail (profiles/r05/ab_soft_assign_store_and_moment_order.txt)
// dynamic LDS of a soft-assign workgroup (doubles): exp table | bins (x, y, z rows of 64) | reduction |
// 4 wave slabs (FULL: 32 rows of 16 BPL + 2; ragged: 64 rows of 18)
__host__ __device__ constexpr bool sa_linear(int BPL, bool full) { return full && BPL <= 3; }  // B = 64: 16-bin blocks (register budget)
__host__ __device__ constexpr int sa_slab_doubles(int BPL, bool full) { return sa_linear(BPL, full) ? 32 * (16 * BPL + 2) : 64 * 18; }
__host__ __device__ constexpr int sa_lds_doubles(int BPL, bool full) { return kExpTab2 + 192 + 8 + 4 * sa_slab_doubles(BPL, full); }
template <int BPL, bool FULL>
__global__ void __launch_bounds__(256, kSaOcc) k_soft_assign(int64_t n, int B, int iters, const double* __restrict__ dirs,
                                                     const double* __restrict__ bins, double inv_tau,
                                                     double* resp, int32_t* bin_idx, double* partial) {
  constexpr int NB = 16 * BPL;
  constexpr int RS = 18;       // ragged slab row stride
  constexpr int RS2 = NB + 2;  // FULL slab row stride
  typedef double dvec2 __attribute__((ext_vector_type(2)));
  extern __shared__ __attribute__((aligned(16))) double sa_lds[];
  double* Tx = sa_lds;
  double* red = Tx + kExpTab2 + 192;  // (192 doubles after the table unused: the bins are scalar loads)
  exp_table2_load(Tx);
  __syncthreads();
  const int h = blockIdx.y;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  double* Rh = resp + (int64_t)h * n * B;
  const double* Dh = dirs + (int64_t)h * n * 3;
  double* S = red + 8 + wv * sa_slab_doubles(BPL, FULL);
  const double Beps = (double)B * 1e-12;
  // Σ log Z is kept as a product of mantissas and a sum of exponents (frexp), one log at the end
  double zm = 1.0, entq = 0.0, mxr = 0.0;
  int ze = 0;
  // iteration it of workgroup b covers points [(it G + b) 256, +256) (G = gridDim.x): the
  // workgroups in flight write one contiguous window of the responsibility matrix instead of G
  // chunks spread over the whole hypothesis (DRAM page locality of the 6.4 GB write stream)
  const int64_t G256 = (int64_t)gridDim.x * 256;
  const int64_t chunk0 = (int64_t)blockIdx.x * 256;
  // directions of the wave's next 64 points: 192 contiguous doubles, three fully coalesced 512-B
  // loads (8 B per lane, any alignment), handed to lane = point through the LDS slab
  const int64_t nd = 3 * n;
  double nd0, nd1, nd2;
#define GC_LOAD_DIRS(WB)                                             \
  {                                                                  \
    const int64_t e0_ = 3 * (WB) + lane;                             \
    nd0 = Dh[e0_ < nd ? e0_ : nd - 1];                               \
    nd1 = Dh[e0_ + 64 < nd ? e0_ + 64 : nd - 1];                     \
    nd2 = Dh[e0_ + 128 < nd ? e0_ + 128 : nd - 1];                   \
  }
  GC_LOAD_DIRS(chunk0 + wv * 64)
  for (int it = 0; it < iters; ++it) {
    const int64_t wbase = chunk0 + (int64_t)it * G256 + wv * 64;
    if (wbase >= n) break;  // wave-uniform
    S[lane] = nd0; S[64 + lane] = nd1; S[128 + lane] = nd2;
    lds_wave_sync();
    const double d0 = S[3 * lane], d1 = S[3 * lane + 1], d2 = S[3 * lane + 2];
    lds_wave_sync();
    GC_LOAD_DIRS(wbase + G256)
    const int64_t pt = wbase + lane;
    const bool valid = pt < n;
    // pass 1: the exact un-fused similarities (kept in ex[]), their row maximum and the integer bin
    // index; pass 2 exponentiates x = (S - S_max)/τ in place, the reference's jax.nn.softmax shift
    // (binning.py:68-69): any τ > 0 and any direction norm. The bin directions are wave-uniform LDS
    // reads (broadcast, no bank conflicts).
    double ex[NB];
    double best = -1e308;
    int bidx = 0;
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      // bin directions as wave-uniform scalar loads (SGPR operands; the LDS pipe keeps the exp table
      // and the row transposes)
      const double bx = FULL || j < B ? bins[3 * j] : 0.0, by = FULL || j < B ? bins[3 * j + 1] : 0.0,
                   bz = FULL || j < B ? bins[3 * j + 2] : 0.0;
      ex[j] = sim_nofma(d0, d1, d2, bx, by, bz);
      if ((FULL || j < B) && ex[j] > best) { best = ex[j]; bidx = j; }
    }
    // exponent in units of ln2/2048 (the 2048-entry table exp, exp2s_n): y = S ysc - S_max ysc by one
    // fma (the maximal bin gets y = the rounding error of S_max ysc, |y| < 1e-11, e = 1 within an ulp);
    // arguments below e^-700 are clamped there (R <= 1e-304 / Z instead of an underflow to 0)
    const double ysc = inv_tau * kTab2OverLn2;
    const double nbs = -(best * ysc);
    double Z = 0.0, sl = 0.0;
#pragma unroll
    for (int j0 = 0; j0 < NB; j0 += 8) {
      double y[8];
#pragma unroll
      for (int jj = 0; jj < 8; ++jj) {
        const int j = j0 + jj;
        y[jj] = (FULL || j < B) ? fmax(fma(ex[j], ysc, nbs), -700.0 * kTab2OverLn2) : 0.0;
      }
      double e8[8];
      exp2s_n<8>(y, Tx, e8);
#pragma unroll
      for (int jj = 0; jj < 8; ++jj) {
        const int j = j0 + jj;
        ex[j] = (FULL || j < B) ? e8[jj] : 0.0;
        Z += ex[j];
        sl = fma(ex[j], y[jj], sl);
      }
      asm volatile("" : "+v"(Z), "+v"(sl));  // accumulate now: the y of a group die here
    }
    sl *= kExp2C1;  // Σ e x in nats
    // the maximal bin has e = 1 (within an ulp): Z >= 1 and max_b R = 1/Z
    const double rZ = recip(Z);
    if (valid) {
      // entropy of the point: log Z - S/Z - B ε   (-Σ R log(R+ε) up to ≤ B·ε)
      int e;
      zm *= frexp(Z, &e);
      ze += e;
      entq += fma(sl, rZ, Beps);
      mxr = fmax(mxr, rZ);
      if (bin_idx) bin_idx[(int64_t)h * n + pt] = bidx;
    }
    if constexpr (sa_linear(BPL, FULL)) {
#pragma unroll
      for (int j = 0; j < NB; ++j) ex[j] *= rZ;
#pragma unroll
      for (int hf = 0; hf < 2; ++hf) {
        if ((lane >> 5) == hf) {
          const int i = lane & 31;
#pragma unroll
          for (int q = 0; q < NB / 2; ++q)
            *reinterpret_cast<dvec2*>(&S[i * RS2 + 2 * q]) = dvec2{ex[2 * q], ex[2 * q + 1]};
        }
        lds_wave_sync();
        // the half's 32 rows are one contiguous block of 32 NB doubles in HBM: 1 KiB per instruction
        const int64_t pbase = wbase + 32 * hf;
        double* dst = Rh + pbase * NB;
        const auto put = [&](int o, const dvec2& v) {
          __builtin_nontemporal_store(v, reinterpret_cast<dvec2*>(dst + o));
        };
        if (pbase + 32 <= n) {  // wave-uniform: the whole block is in range (every block but the tail's)
#pragma unroll
          for (int m = 0; m < NB / 4; ++m) {
            const int o = m * 128 + 2 * lane;
            const int row = o / NB, col = o - row * NB;
            put(o, *reinterpret_cast<const dvec2*>(&S[row * RS2 + col]));
          }
        } else {
          const int64_t lim = (n - pbase) * NB;  // doubles of the block that belong to points < n
#pragma unroll
          for (int m = 0; m < NB / 4; ++m) {
            const int o = m * 128 + 2 * lane;
            const int row = o / NB, col = o - row * NB;
            const dvec2 v = *reinterpret_cast<const dvec2*>(&S[row * RS2 + col]);
            if (o < lim) put(o, v);
          }
        }
        lds_wave_sync();
      }
    } else {
#pragma unroll
      for (int blk = 0; blk < BPL; ++blk) {
#pragma unroll
        for (int q = 0; q < 8; ++q)
          *reinterpret_cast<dvec2*>(&S[lane * RS + 2 * q]) =
              dvec2{ex[16 * blk + 2 * q] * rZ, ex[16 * blk + 2 * q + 1] * rZ};
        lds_wave_sync();
        sa_store_block<BPL, FULL>(S, Rh, wbase, n, B, blk, lane);
        lds_wave_sync();
      }
    }
    int e;
    zm = frexp(zm, &e);  // renormalise once per 64 points: |log2 zm| stays below ~64
    ze += e;
  }
  const double logacc = log(zm) + (double)ze * 0.69314718055994530942;
#undef GC_LOAD_DIRS
  const double es = wg_sum(logacc - entq, red);
  const double ms = wg_max(mxr, red);
  if (threadIdx.x == 0) {
    partial[((int64_t)h * gridDim.x + blockIdx.x) * 2] = es;
    partial[((int64_t)h * gridDim.x + blockIdx.x) * 2 + 1] = ms;
  }
}

__global__ void k_soft_assign_finalize(const double* __restrict__ partial, int64_t cols, int H,
                                       int64_t n, double* cert) {
  const int h = blockIdx.x * blockDim.x + threadIdx.x;
  if (h >= H) return;
  double e = 0.0, m = 0.0;
  for (int64_t c = 0; c < cols; ++c) {
    e += partial[((int64_t)h * cols + c) * 2];
    m = fmax(m, partial[((int64_t)h * cols + c) * 2 + 1]);
  }
  cert[2 * h] = e / ((double)n + 1e-12);
  cert[2 * h + 1] = m;
}

// Persistent form with the IMU/odom branch (the batched pipeline): workgroups [0, n_io) each run
// one hypothesis of the branch (io_branch_wg, independent of the bins); the rest stay resident and
// pull (hypothesis, chunk) tasks from a monotone counter until the H·chunks tasks are taken, so
// the branch's workgroups are dispatched first and the bin tasks balance over whatever CU slots
// remain — no stream fork / join and no partial last round of workgroups. Every task writes its
// own record, so the result does not depend on which workgroup ran it (bit-reproducible for a fixed
// device and shard size: the chunk geometry follows the CU count and H_l). ctr[0] is the task
// counter; the predict launch that precedes every k_bins_io on the stream zeroes it, so a launch
// never depends on how the previous one ended. No workgroup waits on another.
template <int BPL, bool FULL, bool AHEAD>
__global__ void __launch_bounds__(256, kFusedOcc) k_bins_io(FusedArgs A, PipeDev P, ScanArgs S,
                                                             const double* __restrict__ odom, int n_io, int io_on,
                                                             int H, int64_t chunks, unsigned* ctr) {
  extern __shared__ double lds[];
  unsigned& task_s = *reinterpret_cast<unsigned*>(lds + fused_lds_doubles(A.B));  // the launch's extra double
#ifdef GC_BINS_TIMING
  const double bt0 = GC_BT_NOW();
  double bt1 = bt0;
  int bt_n = 0;
#endif
  if ((int)blockIdx.x < n_io) {
    lpred_wg(P, S, blockIdx.x, lds);  // the predict's L_pred half (pred_mode 0), then the IMU/odom branch
    if (io_on) io_branch_wg(P, S, odom, blockIdx.x, lds);
#ifdef GC_BINS_TIMING
    if (threadIdx.x == 0 && blockIdx.x < 8192) {
      double* g = g_bins_trace + 4 * blockIdx.x;
      g[0] = bt0; g[1] = bt0; g[2] = GC_BT_NOW(); g[3] = -1.0;
    }
#endif
    return;
  }
  bins_prologue(A, lds);
#ifdef GC_BINS_TIMING
  bt1 = GC_BT_NOW();
#endif
  const int RL = A.B * NF_BASE + REC_EXTRA;
  const unsigned T = (unsigned)(H * chunks);
  // the next task's ticket is taken inside the current task before its epilogue, so the atomic's
  // round trip overlaps the epilogue (bins_task ends with a barrier: task_s is read by all before it
  // is rewritten). Taken at the start of the task instead, a ticket was held for the whole task: at
  // the end of the launch a workgroup pairing a long task with another on its CU (each then runs at
  // half speed) started its reserved one ~180 us late (GC_BINS_TIMING task traces)
  if (threadIdx.x == 0) task_s = atomicAdd(ctr, 1u);
  __syncthreads();
  TaskAhead ahead;
  ahead.valid = false;
  ahead.ok = false;
  ahead.t = task_s;
  int64_t n_sel, stride;  // the a1 selection, shared by every task of the launch
  selection_of(A, &n_sel, &stride);
  // uniform values in scalar registers: held in VGPRs they were spilled, and each task's reload waited
  // (in-order vmcnt) on the previous epilogue's look-ahead loads
  if constexpr (AHEAD) {
    n_sel = uniform_i64(n_sel);
    stride = uniform_i64(stride);
  }
  // Late-ticket instantiation (long tasks): the full feature set where the hypothesis's direction scatter
  // is read (bin_scatter_full: global hypothesis 0, the bin map's), the lean set for every other task. The
  // full-set tasks hold the first tickets (TaskOrder): a puller runs them in a loop of their own, then the
  // lean-set ones. The look-ahead instantiation (short tasks) runs the full set for every task, in one
  // loop and the flat ticket order: its tasks' outputs are pinned bit for bit to recorded arrays
  // (tests/test_gpu_bins_zbatch.py), which the lean set's two features moved to the matrix core would not
  // keep, and two variants in that kernel spilled in its task loops (profiles/r08/bins_variants_isa.txt).
  // The finalize writes 0.0 into a lean-set hypothesis's scatter columns from either record layout
  // (the launch's lean_records flag), so what a caller reads does not depend on the instantiation.
  const int nf = AHEAD ? 0 : bin_scatter_full_count(P);
  const TaskOrder ord{(unsigned)(nf * chunks), nf, H - nf};
  const auto pull = [&](auto lean_tag, const unsigned Tend) {
    constexpr bool LEAN = decltype(lean_tag)::value;
    for (;;) {
      // uniform: the task's record pointer lives in scalar registers (held in a VGPR it was spilled and
      // its reload waited on the look-ahead loads issued before it)
      const unsigned t = __builtin_amdgcn_readfirstlane(ahead.t);
      if (t >= Tend) break;
      int h;
      int64_t c;
      task_of(ord, t, &h, &c);
#ifdef GC_BINS_TIMING
      const double tt0 = GC_BT_NOW();
#endif
      double* rec = A.partials + ((int64_t)h * chunks + c) * RL;
      if constexpr (AHEAD) {
        bins_task<BPL, FULL, true, LEAN>(A, h, c, lds, rec, ctr, &task_s, &ahead, T, ord, nullptr, (int)t, n_sel, stride);
      } else {
        unsigned next = 0;
        bins_task<BPL, FULL, true, LEAN, LEAN>(A, h, c, lds, rec, ctr, &task_s, &ahead, T, ord, &next, (int)t, n_sel, stride);
        if (threadIdx.x == 0) task_s = next;
        __syncthreads();
        ahead.t = task_s;
      }
#ifdef GC_BINS_TIMING
      ++bt_n;
      if (threadIdx.x == 0 && t < 16384) {
        unsigned xcc = 0;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        double* g = g_task_trace + 4 * t;
        g[0] = tt0; g[1] = GC_BT_NOW(); g[2] = (double)blockIdx.x; g[3] = (double)(xcc & 0xf);
      }
#endif
    }
  };
  if constexpr (AHEAD) {
    pull(std::false_type{}, T);
  } else {
    pull(std::false_type{}, ord.Tf);
    pull(std::true_type{}, T);
  }
#ifdef GC_BINS_TIMING
  if (threadIdx.x == 0 && blockIdx.x < 8192) {
    double* g = g_bins_trace + 4 * blockIdx.x;
    g[0] = bt0; g[1] = bt1; g[2] = GC_BT_NOW(); g[3] = (double)bt_n;
  }
#endif
}

// Grid form (the gc_scan_bins_fused entry): grid (chunks, H), one task per workgroup.
template <int BPL, bool FULL>
__global__ void __launch_bounds__(256, kFusedOcc) k_bins_fused(FusedArgs A) {
  extern __shared__ double lds[];
  bins_prologue(A, lds);
  const int RL = A.B * NF_BASE + REC_EXTRA;
  int64_t n_sel, stride;
  selection_of(A, &n_sel, &stride);
  bins_task<BPL, FULL, false>(A, blockIdx.y, blockIdx.x, lds,
                              A.partials + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * RL, nullptr, nullptr,
                              nullptr, 0u, TaskOrder{0u, 0, 1}, nullptr, -1, n_sel, stride);
}

// ================================================================ PSD projection, any d
// The per-operator gc_domain_projection_psd_batch. Its kernels stay in this translation unit: they call
// wg_psd_project / wg_jacobi_eigh with a run-time size, as k_bins_io's lpred_wg does with kDZ, and with
// them in another unit the compiler specialises those functions for the one size left before it inlines
// them, which changes k_bins_io's instructions (and those of the unit that receives them;
// profiles/r15/isa_identity.txt).
__global__ void k_psd3(int batch, const double* __restrict__ M, double eps, double* Mo, double* cert) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= batch) return;
  double A[9], P[9], c[6];
  for (int k = 0; k < 9; ++k) A[k] = M[9 * i + k];
  psd_project3(A, eps, P, c);
  for (int k = 0; k < 9; ++k) Mo[9 * i + k] = P[k];
  for (int k = 0; k < 6; ++k) cert[6 * i + k] = c[k];
}

__global__ void __launch_bounds__(256) k_psd_wg(int d, const double* __restrict__ M, double eps,
                                                double* Mo, double* cert) {
  __shared__ double Ml[kDZ * kDZ], Mp[kDZ * kDZ], scr[2 * kDZ * kDZ + 4 * kDZ], red[4], c6[6];
  const int i = blockIdx.x;
  for (int k = threadIdx.x; k < d * d; k += kWG) Ml[k] = M[(int64_t)i * d * d + k];
  __syncthreads();
  wg_psd_project(Ml, Mp, eps, d, scr, red, c6);
  for (int k = threadIdx.x; k < d * d; k += kWG) Mo[(int64_t)i * d * d + k] = Mp[k];
  if (threadIdx.x < 6) cert[6 * i + threadIdx.x] = c6[threadIdx.x];
}

// domain_projection_psd_core (primitives.py:80-123) for any d (the per-operator drop-in; the
// pipeline uses the fixed-size forms above). An odd d is padded to even dp with a zero row and
// column: every Jacobi rotation touching the pad has a_pq = 0, so it is the identity, the pad stays
// decoupled with eigenvalue 0, contributes nothing to the d x d reconstruction (V[i][pad] = 0) and
// is left out of the certificate. Workspace: 3 dp² + 4 dp + 8 doubles of LDS (dp <= 64) or of
// global scratch (the same code on global pointers; __syncthreads orders the workgroup's accesses).
__host__ __device__ inline int psd_ws_len(int dp) { return 3 * dp * dp + 4 * dp + 8; }
__global__ void __launch_bounds__(256) k_psd_any(int d, const double* __restrict__ M, double eps, double* Mo,
                                                 double* cert, double* gws) {
  extern __shared__ double lds_psd[];
  const int dp = d + (d & 1);
  const int64_t i = blockIdx.x;
  double* A = gws ? gws + i * psd_ws_len(dp) : lds_psd;
  double* V = A + dp * dp;
  double* Ms = V + dp * dp;
  double* w = Ms + dp * dp;
  double* cs = w + dp;
  double* red = cs + 3 * dp;
  const double* Mi = M + i * d * d;
  double symloc = 0.0;
  for (int idx = threadIdx.x; idx < dp * dp; idx += kWG) {
    const int r = idx / dp, c = idx % dp;
    double sv = 0.0;
    if (r < d && c < d) {
      sv = 0.5 * (Mi[r * d + c] + Mi[c * d + r]);
      const double dd = sv - Mi[r * d + c];
      symloc += dd * dd;
    }
    A[idx] = sv;
    Ms[idx] = sv;
  }
  __syncthreads();
  const double symd = wg_sum(symloc, red);
  wg_jacobi_eigh(A, V, w, dp, cs, red);
  double mnl = 1e308, mxl = -1e308, nnl = 0.0;
  for (int k = threadIdx.x; k < dp; k += kWG) {
    const double wc = fmax(w[k], eps);
    w[k] = wc;
    if (k < d) {
      mnl = fmin(mnl, wc); mxl = fmax(mxl, wc); nnl += (wc < 10.0 * eps) ? 1.0 : 0.0;
    }
  }
  const double mn = -wg_max(-mnl, red);
  const double mx = wg_max(mxl, red);
  const double nn = wg_sum(nnl, red);
  double projloc = 0.0;
  for (int idx = threadIdx.x; idx < d * d; idx += kWG) {
    const int r = idx / d, c = idx % d;
    double v = 0.0;
    for (int k = 0; k < dp; ++k) v += V[r * dp + k] * w[k] * V[c * dp + k];
    const double dd = v - Ms[r * dp + c];
    projloc += dd * dd;
    Mo[i * d * d + idx] = v;
  }
  const double proj = wg_sum(projloc, red);
  if (threadIdx.x == 0) {
    double* c6 = cert + 6 * i;
    c6[0] = sqrt(proj); c6[1] = sqrt(symd); c6[2] = mn; c6[3] = mx; c6[4] = mx / mn; c6[5] = nn;
  }
}

}  // namespace gc

using namespace gc;

static int pick_iters(int64_t n, int H, int max_iters = 8, int64_t min_wgs = 2048) {
  // Aim for >= ~4 workgroups per CU-slot while keeping partial records small. The fused kernel
  // takes 16 (its per-workgroup prologue, the 16 KB exp table and the bin directions, and the
  // partial-record epilogue amortise over twice the points: 1.667 -> 1.604 ms/scan, 32 no better)
  // and halves only below 1024 workgroups (a 32-hypothesis shard: 8 iterations, 0.404 -> 0.395
  // ms/scan against 4).
  int iters = max_iters;
  while (iters > 1 && ((n + iters * 256 - 1) / (iters * 256)) * (int64_t)H < min_wgs) iters >>= 1;
  return iters;
}

extern "C" {

int32_t gc_bin_soft_assign(gc_ctx* ctx, int32_t H, int64_t n, int32_t B, const double* d_dirs,
                           const double* d_bins, double tau, double* d_resp_out, int32_t* d_bin_index_out,
                           double* d_cert_out) {
  GC_CHECK_ARG(nullptr, ctx != nullptr, "ctx is NULL");
  GC_CHECK_ARG(ctx, H > 0 && n > 0, "H and n must be positive");
  GC_CHECK_ARG(ctx, B >= 1 && B <= 64, "B must be in [1, 64]");
  GC_CHECK_ARG(ctx, tau > 0.0, "tau must be positive");
  GC_CHECK_ARG(ctx, d_dirs && d_bins && d_resp_out && d_cert_out, "NULL buffer");
  constexpr int kSaIters = 8;
  int iters = kSaIters;
  while (iters > 1 && ((n + iters * 256 - 1) / (iters * 256)) * (int64_t)H < 4096) iters >>= 1;
  const int64_t blocks = (n + iters * 256 - 1) / (iters * 256);
  void* scr;
  if (int rc = gc::scratch(ctx, sizeof(double) * 2 * blocks * H, &scr)) return rc;
  const double inv_tau = 1.0 / tau;
  dim3 grid((unsigned)blocks, H);
  const bool full = (B % 16) == 0 && ((uintptr_t)d_resp_out & 15) == 0;
  if (int32_t rc = dispatch_bpl(B, full, [&](auto bp, auto full_tag) -> int32_t {
        constexpr int BP = decltype(bp)::value;
        constexpr bool FULL = decltype(full_tag)::value;
        const size_t sh = sizeof(double) * (size_t)sa_lds_doubles(BP, FULL);
        GC_HIP(ctx, gc::ensure_dyn_lds((const void*)k_soft_assign<BP, FULL>, sh));
        hipLaunchKernelGGL((k_soft_assign<BP, FULL>), grid, dim3(256), sh, ctx->stream, n, B, iters, d_dirs, d_bins,
                           inv_tau, d_resp_out, d_bin_index_out, (double*)scr);
        return GC_OK;
      }))
    return rc;
  GC_LAUNCH_CHECK(ctx);
  hipLaunchKernelGGL(k_soft_assign_finalize, dim3((H + 63) / 64), dim3(64), 0, ctx->stream, (const double*)scr,
                     blocks, H, n, d_cert_out);
  GC_LAUNCH_CHECK(ctx);
  return GC_OK;
}

int32_t gc_scan_bins_fused(gc_ctx* ctx, int32_t H, int64_t n_in, int64_t n_cap, int32_t B,
                           const double* d_points_raw, const double* d_t_raw, const double* d_w_raw,
                           const double* d_budget_scalars, double t0, double t1, const double* d_xi,
                           const double* d_bins, double tau, const double* h_origin3, double eps_psd,
                           double eps_mass, double* d_stats_out, double* d_cert_out, int32_t iters) {
  GC_CHECK_ARG(nullptr, ctx != nullptr, "ctx is NULL");
  GC_CHECK_ARG(ctx, H > 0 && n_in > 0 && n_cap > 0, "H, n_in, n_cap must be positive");
  GC_CHECK_ARG(ctx, B >= 1 && B <= 64, "B must be in [1, 64]");
  // the table exp's exponent splice holds for arguments down to -2/τ (in units of ln 2 / 2048 that
  // is 2^-1022): below the floor the smallest responsibilities would wrap instead of underflowing
  GC_CHECK_ARG(ctx, tau >= GC_FUSED_TAU_MIN, "tau must be >= GC_FUSED_TAU_MIN (3e-3) for the fused kernel");
  GC_CHECK_ARG(ctx, iters >= 0 && iters <= 64, "iters must be in [0, 64] (0 = by grid size)");
  GC_CHECK_ARG(ctx, d_points_raw && d_t_raw && d_w_raw && d_budget_scalars && d_xi && d_bins && h_origin3 &&
                        d_stats_out && d_cert_out, "NULL buffer");
  (void)n_in;
  if (iters == 0) iters = pick_iters(n_cap, H, 16, 1024);
  const int64_t chunks = (n_cap + iters * 256 - 1) / (iters * 256);
  const int NF = NF_BASE;
  const int RL = B * NF + REC_EXTRA;
  void* scr;
  if (int rc = gc::scratch(ctx, sizeof(double) * RL * chunks * H, &scr)) return rc;
  const size_t sh = sizeof(double) * fused_lds_doubles(B);
  dim3 grid((unsigned)chunks, H);
  const FusedArgs FA{n_cap, B, iters, d_points_raw, d_t_raw, d_w_raw, d_budget_scalars, t0, t1, d_xi, d_bins,
                     1.0 / tau, h_origin3[0], h_origin3[1], h_origin3[2], (double*)scr, nullptr, chunks, iters,
                     0, iters};
  if (int32_t rc = dispatch_bpl(B, B == 16 * bpl_for(B), [&](auto bp, auto full_tag) -> int32_t {
        constexpr int BP = decltype(bp)::value;
        constexpr bool FULL = decltype(full_tag)::value;
        GC_HIP(ctx, gc::ensure_dyn_lds((const void*)k_bins_fused<BP, FULL>, sh));
        if (int rc_ = gc::ensure_no_static_lds(ctx, (const void*)k_bins_fused<BP, FULL>)) return rc_;
        hipLaunchKernelGGL((k_bins_fused<BP, FULL>), grid, dim3(256), sh, ctx->stream, FA);
        return GC_OK;
      }))
    return rc;
  GC_LAUNCH_CHECK(ctx);
  return gc::launch_bins_finalize(ctx, H, B, NF, chunks, (const double*)scr, eps_psd, eps_mass, d_stats_out,
                                  d_cert_out);
}

int32_t gc_bins_task_plan(int32_t H_geom, int64_t n_cap, int32_t cu_count, int64_t* out8) {
  GC_CHECK_ARG(nullptr, H_geom >= 1 && n_cap >= 1 && cu_count >= 1, "H_geom, n_cap and cu_count must be positive");
  GC_CHECK_ARG(nullptr, out8 != nullptr, "out8 is NULL");
  const BinsPlan pl = plan_bins_tasks(H_geom, n_cap, cu_count);
  const int64_t v[8] = {pl.iters, pl.iters_short, pl.iters_tiny, pl.k1, pl.k2, pl.chunks, pl.ahead ? 1 : 0, pl.pullers};
  std::copy(v, v + 8, out8);
  return GC_OK;
}

}  // extern "C"

namespace gc {
// The batched pipeline's a1 -> a6 bins for its Hl local hypotheses, with the IMU/odom branch's
// workgroups in the same launch when io (k_bins_io), then the chunk-order finalize.
int32_t scan_bins_pipeline(gc_ctx* ctx, const PipeDev& P, const ScanArgs& S, const double* d_odom, bool io,
                           const double* d_pts, const double* d_t, const double* d_w, int64_t n_in,
                           int64_t* done_word, int64_t ticket, BinsFold* fold) {
  (void)n_in;
  if (ctx->cu_count == 0) {
    int cus = 0;
    GC_HIP(ctx, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device));
    ctx->cu_count = cus > 0 ? cus : 1;
  }
  const int H = P.Hl, B = P.B;
  // the chunk tiers and the kernel form (gc_binplan.h)
  const BinsPlan pl = plan_bins_tasks(P.geom_H > 0 ? P.geom_H : H, P.n_cap, ctx->cu_count);
  const int64_t chunks = pl.chunks;
  GC_CHECK_ARG(ctx, (int64_t)H * chunks < (int64_t)0xFFFFFFFF, "too many bin tasks");
  const int NF = NF_BASE;
  const int RL = B * NF + REC_EXTRA;
  void* scr;
  if (int rc = gc::scratch(ctx, sizeof(double) * RL * chunks * H, &scr)) return rc;
  const FusedArgs FA{P.n_cap, B, pl.iters, d_pts, d_t, d_w, P.budget, S.t0, S.t1, P.xi, P.bins, 1.0 / P.tau,
                     P.o0, P.o1, P.o2, (double*)scr, P.w_win, pl.k1, pl.iters_short, pl.k2, pl.iters_tiny};
  // one auxiliary workgroup per hypothesis first: the predict's L_pred half (lpred_wg), then, when io,
  // the IMU/odom branch
  const int n_io = H, io_on = io ? 1 : 0;
  // + 1: the pullers' task slot after the fused layout (no static LDS in k_bins_io: the dynamic block
  // starts at LDS address 0, so the exp table's addresses need no base add, exp2s_shift_tab_n)
  const size_t sh = sizeof(double) * (std::max<size_t>(std::max<size_t>(fused_lds_doubles(B), (size_t)kLpredLdsDoubles),
                                                       io ? (size_t)kIoLdsDoubles : 0) + 1);
  const dim3 grid((unsigned)(n_io + pl.pullers));
  const bool ahead = pl.ahead;
  if (int32_t rc = dispatch_bpl(B, B == 16 * bpl_for(B), [&](auto bp, auto full_tag) -> int32_t {
        return dispatch_bool(ahead, [&](auto ahead_tag) -> int32_t {
          constexpr int BP = decltype(bp)::value;
          constexpr bool FULL = decltype(full_tag)::value, AH = decltype(ahead_tag)::value;
          GC_HIP(ctx, gc::ensure_dyn_lds((const void*)k_bins_io<BP, FULL, AH>, sh));
          if (int rc_ = gc::ensure_no_static_lds(ctx, (const void*)k_bins_io<BP, FULL, AH>)) return rc_;
          hipLaunchKernelGGL((k_bins_io<BP, FULL, AH>), grid, dim3(256), sh, ctx->stream, FA, P, S, d_odom, n_io,
                             io_on, H, chunks, P.task_ctr);
          return GC_OK;
        });
      }))
    return rc;
  GC_LAUNCH_CHECK(ctx);
  if (fold && chunks <= kFoldChunks && fold_record_fits(B)) {  // k_evidence reduces the records (gc_evidence.hip)
    fold->part = (const double*)scr;
    fold->chunks = chunks;
    fold->lean_records = !ahead;
    return GC_OK;
  }
  if (fold) fold->part = nullptr;
  return launch_bins_finalize_split(ctx, H, B, NF, chunks, (const double*)scr, P.eps_psd, P.eps_mass, P.stats,
                                    P.bincert, P.binaux, done_word, ticket, bin_scatter_full_count(P), ahead ? 0 : 1);
}
}  // namespace gc

extern "C" {

#ifdef GC_BINS_TIMING
// dev: the last k_bins_io launch's per-workgroup trace (4 doubles each) into h_out
int32_t gc_dev_bins_trace(double* h_out, int64_t n_wg) {
  if (n_wg < 0 || n_wg > 8192) return GC_ERR_RUNTIME;
  return hipMemcpyFromSymbol(h_out, HIP_SYMBOL(gc::g_bins_trace), sizeof(double) * 4 * n_wg) == hipSuccess
             ? GC_OK : GC_ERR_RUNTIME;
}
int32_t gc_dev_task_wv_trace(double* h_out, int64_t n_tasks) {
  if (n_tasks < 0 || n_tasks > 16384) return GC_ERR_RUNTIME;
  return hipMemcpyFromSymbol(h_out, HIP_SYMBOL(gc::g_task_wv), sizeof(double) * 4 * n_tasks) == hipSuccess
             ? GC_OK : GC_ERR_RUNTIME;
}
int32_t gc_dev_task_ep_trace(double* h_out, int64_t n_tasks) {
  if (n_tasks < 0 || n_tasks > 16384) return GC_ERR_RUNTIME;
  return hipMemcpyFromSymbol(h_out, HIP_SYMBOL(gc::g_task_ep), sizeof(double) * 2 * n_tasks) == hipSuccess
             ? GC_OK : GC_ERR_RUNTIME;
}
int32_t gc_dev_task_trace(double* h_out, int64_t n_tasks) {
  if (n_tasks < 0 || n_tasks > 16384) return GC_ERR_RUNTIME;
  return hipMemcpyFromSymbol(h_out, HIP_SYMBOL(gc::g_task_trace), sizeof(double) * 4 * n_tasks) == hipSuccess
             ? GC_OK : GC_ERR_RUNTIME;
}
#endif

int32_t gc_domain_projection_psd_batch(gc_ctx* ctx, int32_t batch, int32_t d, const double* d_M, double eps_psd,
                                       double* d_M_out, double* d_cert_out) {
  GC_CHECK_ARG(nullptr, ctx != nullptr, "ctx is NULL");
  GC_CHECK_ARG(ctx, batch >= 0 && d_M && d_M_out && d_cert_out, "bad arguments");
  GC_CHECK_ARG(ctx, d >= 1 && d <= 512, "d must be in [1, 512]");
  if (batch == 0) return GC_OK;
  if (d == 3) {
    hipLaunchKernelGGL(k_psd3, dim3((batch + 63) / 64), dim3(64), 0, ctx->stream, batch, d_M, eps_psd, d_M_out,
                       d_cert_out);
  } else if (d <= kDZ && d % 2 == 0) {
    hipLaunchKernelGGL(k_psd_wg, dim3(batch), dim3(256), 0, ctx->stream, d, d_M, eps_psd, d_M_out, d_cert_out);
  } else {
    const int dp = d + (d & 1);
    const size_t ws = sizeof(double) * (size_t)psd_ws_len(dp);
    if (dp <= 64) {
      GC_HIP(ctx, gc::ensure_dyn_lds((const void*)k_psd_any, ws));
      hipLaunchKernelGGL(k_psd_any, dim3(batch), dim3(256), ws, ctx->stream, d, d_M, eps_psd, d_M_out, d_cert_out,
                         (double*)nullptr);
    } else {
      void* scr;
      if (int rc = gc::scratch(ctx, ws * (size_t)batch, &scr)) return rc;
      hipLaunchKernelGGL(k_psd_any, dim3(batch), dim3(256), 0, ctx->stream, d, d_M, eps_psd, d_M_out, d_cert_out,
                         (double*)scr);
    }
  }
  GC_LAUNCH_CHECK(ctx);
  return GC_OK;
}

}  // extern "C"
