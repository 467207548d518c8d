// gc_binstask.h — one (hypothesis, chunk) task of the fused a1 -> a4 -> a5 -> a6 bins kernels (k_bins_fused,
// k_bins_io in gc_bins.hip): the partial-record writer, the launch arguments and LDS layout, the workgroup
// prologue, the chunk tiers, the look-ahead operands, the ticket order and the task body with its
// GC_BINS_TIMING hooks.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <type_traits>
#include "gc_binsdev.h"
#include "gc_wgla.h"
#include "gc_binfin.h"

namespace gc {

// a workgroup's copy of the exp table into its LDS. The library is built without relocatable device code,
// so the table is visible only in the translation unit that defines it: that unit (gc_bins.hip) defines
// this function, and every kernel that runs bins_prologue lives there.
GC_DEV void exp_table2_load(double* T);

// MFMA epilogue: reduce per-lane tiles over the 4 waves (LDS, fixed order) into one partial
// record. Lane (g, l) holds D_j[row g + 4r][col l] = Σ R[·][16j + g + 4r] F[·][l] for the 16
// MFMA features, and per-group partial sums accx[j][t] (bin 16j + l, feature 16 + t).
// DF = 9: feature 9 (Σ R w d_z²) is not accumulated; the MFMA columns hold features 0..8, 10..16 and
// the VALU ones 17.. . It is recovered from the trace of the direction scatter, Σ R w |d|² = N − ε_d
// with ε_d = Σ R w (1 − |d|²) ≤ 2·1e-12 / range of N (|d| = |r| / (|r| + 1e-12)): d_z² = N − d_x² − d_y²,
// an absolute error ~1e-12 N in that one scatter entry; N, the resultant and κ stay exact sums.
struct NoHook {
  GC_DEV void operator()() const {}
};
GC_DEV int64_t uniform_i64(int64_t v) {
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v);
  const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)((uint64_t)v >> 32));
  return (int64_t)(((uint64_t)hi << 32) | lo);
}
// pre() runs before the barrier, mid() after it (the persistent bins form's next-task broadcast). Each wave
// stages its tiles, its two VALU features and its three certificate partials in its OWN slab (WS doubles
// from lds + wv WS: no other wave reads it during a task, so no barrier is needed before the writes),
// and computes its log-product and wave sums before the barrier: every latency-bound step of the
// epilogue runs before mid() issues the next task's loads (a later wait on scratch or on the staged
// values would otherwise wait for those loads' HBM round trip as well). One barrier, the 4-wave sum in
// a fixed order, and the caller's closing barrier.
// NC: the MFMA columns the record keeps (columns NC.. of the tiles are dropped; the lean feature set's 13).
template <int BPL, int NX, int DF = -1, bool FULL = false, int WS = 0, int NC = 16, typename Pre = NoHook,
          typename Mid = NoHook>
GC_DEV void write_partial_record_mfma(const v4d (&acc4)[BPL], double (&accx)[BPL][NX > 0 ? NX : 1], double ent, double mxr,
                                      double sumw, double npts, int B_, double* lds, double* rec,
                                      const Pre& pre = Pre(), const Mid& mid = Mid()) {
  const int B = FULL ? 16 * BPL : B_;  // FULL: a compile-time bin count (immediate LDS offsets, no bounds branches)
  constexpr int ND = DF >= 0 ? 1 : 0;
  constexpr int NF = ND + NC + NX;
  static_assert(NC == 16 || (DF < 0 && NX == 0), "dropped columns: the lean set, every feature on the matrix core");
  static_assert(WS >= 16 * BPL * NF + 3, "a wave's slab holds its record tiles");
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, g = lane >> 4, bl = lane & 15;
  const int fcol = (DF >= 0 && bl >= DF) ? bl + 1 : bl;  // the feature of MFMA column bl
#pragma unroll
  for (int j = 0; j < BPL; ++j)
#pragma unroll
    for (int t = 0; t < NX; ++t) {
      // the column's sum over the wave's four 16-lane rows; gfx950's v_permlane16/32_swap in place of the two
      // shuffles buys nothing (profiles/r06/ab_bins_epilogue.txt)
      double v = accx[j][t];
      v += __shfl_xor(v, 16, 64);
      v += __shfl_xor(v, 32, 64);
      accx[j][t] = v;
    }
  const double e = wave_sum(ent), m = wave_max(mxr), s = wave_sum(sumw);
  double* W = lds + wv * WS;
#pragma unroll
  for (int j = 0; j < BPL; ++j) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int b = 16 * j + g + 4 * r;
      if (b < B && (NC == 16 || bl < NC)) W[b * NF + fcol] = acc4[j][r];
    }
    const int b = 16 * j + bl;
    if (g == 0 && b < B)
#pragma unroll
      for (int t = 0; t < NX; ++t) W[b * NF + ND + NC + t] = accx[j][t];
  }
  if (lane == 0) {
    W[B * NF + 0] = e;
    W[B * NF + 1] = m;
    W[B * NF + 2] = s;
  }
  pre();
  __syncthreads();
  mid();
  int tid = threadIdx.x;
  asm volatile("" : "+v"(tid));  // the per-lane addresses formed here, not hoisted out of the task loop and spilled
  const auto sum4 = [&](int e) { return (lds[e] + lds[WS + e]) + (lds[2 * WS + e] + lds[3 * WS + e]); };
  if constexpr (FULL) {
    // a compile-time entry count: every lane's entries summed with their LDS reads issued together (one
    // LDS round trip instead of one per entry), then stored; the complement entry's three sums are
    // selected, not branched to
    constexpr int NE = 16 * BPL * NF, NI = (NE + kWG - 1) / kWG;
    double v[NI];
#pragma unroll
    for (int k = 0; k < NI; ++k) {
      const int i = min(tid + k * kWG, NE - 1);
      if constexpr (DF >= 0) {
        const bool df = i % NF == DF;
        const int i0 = i - (df ? DF : 0);  // N
        const double a = sum4(i0), b = sum4(df ? i0 + 4 : i0), c = sum4(df ? i0 + 7 : i0);
        v[k] = df ? (a - b) - c : a;  // N − xx − yy
      } else {
        v[k] = sum4(i);
      }
    }
    // the scheduler otherwise pairs each two reads with a wait for them: every read first
    __builtin_amdgcn_sched_group_barrier(0x100, (DF >= 0 ? 12 : 4) * NI, 0);
#pragma unroll
    for (int k = 0; k < NI; ++k)
      if (k < NI - 1 || tid + k * kWG < NE) rec[tid + k * kWG] = v[k];
  } else {
    for (int i = tid; i < B * NF; i += kWG) {
      if (DF >= 0 && i % NF == DF) rec[i] = (sum4(i - DF) - sum4(i - DF + 4)) - sum4(i - DF + 7);  // N − xx − yy
      else rec[i] = sum4(i);
    }
  }
  if (threadIdx.x == 0) {
    const double* ex = lds + B * NF;
    double x[4][3];
#pragma unroll
    for (int w = 0; w < 4; ++w)
#pragma unroll
      for (int k = 0; k < 3; ++k) x[w][k] = ex[w * WS + k];
    __builtin_amdgcn_sched_group_barrier(0x100, 12, 0);
    rec[B * NF + 0] = (x[0][0] + x[1][0]) + (x[2][0] + x[3][0]);
    rec[B * NF + 1] = fmax(fmax(x[0][1], x[1][1]), fmax(x[2][1], x[3][1]));
    rec[B * NF + 2] = (x[0][2] + x[1][2]) + (x[2][2] + x[3][2]);
    rec[B * NF + 3] = npts;
  }
}

// =========================================================== fused a1 -> a4 -> a5 -> a6
// grid (chunks, H). Budget selection + deskew + directions + features in phase A (lane =
// point), soft assignment in phase B (lanes = 4 point-groups x 16 bin-lanes, 4 points per
// step). The moment sums are a GEMM, Mom[b][k] = Σ_p R[p][b] F[p][k]: the step's (16 bins x 4
// points) responsibility tile of bin block j is exactly the A operand of
// v_mfma_f64_16x16x4_f64 as the lanes already hold it, and F[p][k] for 4 points x 16 features
// is one LDS read per lane (B operand). The matrix core accumulates features 0..15 while the
// VALU does the exp/softmax; features 16..18 stay on the VALU. Responsibilities never leave
// registers.
// feature slab row stride: the B-operand read F[l][4s + g] of the 32 lanes of a ds_read_b64
// group lands on 32 distinct bank pairs (4 l + 2 g + 8 s mod 64)
constexpr int kFusedFS = 66;
constexpr int kFusedOcc = 2;   // waves per SIMD the register budget is sized for (3 spills: §5 of DESIGN.md)
constexpr int kFusedUnr = 8;   // softmax steps unrolled per block (Π Z renormalised after each block: exact)
constexpr int kFusedNacc = 2;  // MFMA accumulator sets (even / odd steps)
// Per-launch constants of the fused kernel and its LDS tables (exp table, scaled bins), set up once
// per workgroup by bins_prologue; a workgroup then runs one (grid form) or many (persistent form)
// (hypothesis, chunk) tasks with bins_task.
struct FusedArgs {
  int64_t n_cap;
  int B, iters;
  const double *pts_raw, *t_raw, *w_raw, *bscal;
  double t0, t1;
  const double *xi, *bins;
  double inv_tau, o0, o1, o2;
  double* partials;      // (H, chunks, RL) records
  const double* w_win;   // (n_cap) selected w x time window (the pipeline's predict), or NULL: per task
  // three chunk tiers: chunks [0, k1) hold iters x 256 points, the next k2 iters_s x 256, the rest
  // iters_t x 256 (the persistent form ends on ever shorter tasks, so the pullers finish together);
  // grid form: k1 = chunks
  int64_t k1;
  int iters_s;
  int64_t k2;
  int iters_t;
};
constexpr int kFusedNS = NF_BASE + 4;  // feature slab rows: 19 features + d(3) + valid flag
// the exp table's offset in a fused workgroup's dynamic LDS (doubles), after the 4 wave slabs. A point-major
// softmax (a quad of lanes per point, the responsibilities through a per-wave LDS slab into the matrix-core
// layout) measured neutral at H = 256 and 10 % slower at H = 32 (profiles/r06/ab_bins_point_major.txt).
__host__ __device__ constexpr int fused_tab_offset() { return 4 * kFusedFS * kFusedNS; }
// dynamic LDS of a fused workgroup (doubles): 4 wave slabs | exp table | scaled bins | epilogue reduction
// (aliases the slabs)
__host__ __device__ inline size_t fused_lds_doubles(int B) {
  const size_t a = (size_t)fused_tab_offset() + kExpTab2 + 192, b = 4 * (size_t)B * NF_BASE + 12;
  return a > b ? a : b;
}

GC_DEV void bins_prologue(const FusedArgs& A, double* lds) {
  double* Tx = lds + fused_tab_offset();
  exp_table2_load(Tx);
  double* Lb = Tx + kExpTab2;  // bin directions pre-scaled by 2048/(τ ln2) (x, y, z rows of 64)
  const double ysc = A.inv_tau * kTab2OverLn2;
  if (threadIdx.x < 64) {
    const int b = threadIdx.x;
    Lb[b] = b < A.B ? A.bins[3 * b] * ysc : 0.0;
    Lb[64 + b] = b < A.B ? A.bins[3 * b + 1] * ysc : 0.0;
    Lb[128 + b] = b < A.B ? A.bins[3 * b + 2] * ysc : 0.0;
  }
  __syncthreads();
}

// the first point index of chunk c (the tiers of FusedArgs) and its iteration count
GC_DEV int64_t chunk_first(const FusedArgs& A, int64_t c, int* iters_out) {
  const bool big = c < A.k1, mid = !big && c < A.k1 + A.k2;
  *iters_out = big ? A.iters : (mid ? A.iters_s : A.iters_t);
  return big ? c * A.iters * 256
             : (mid ? (A.k1 * A.iters + (c - A.k1) * A.iters_s) * 256
                    : (A.k1 * A.iters + A.k2 * A.iters_s + (c - A.k1 - A.k2) * A.iters_t) * 256);
}
// A task's operands that its first iteration waits for: the hypothesis's twist and the lane's raw point
// of iteration 0. The persistent form loads the next task's during the current task's epilogue
// (TaskAhead::valid), so the HBM round trip overlaps the record's reduction instead of opening the task.
struct TaskAhead {
  double xr[6];
  double np[3], ntt, nww;
  unsigned t;   // the next task's ticket (all lanes), read back from the workgroup's task slot
  bool valid;
  bool ok;      // the lane's point is selected (np / ntt / nww are then the point's; zeroed at use otherwise)
};
// n_sel / stride: the a1 selection's count and stride (budget scalars), read once per launch. The raw point
// is loaded unconditionally from a clamped index, its validity applied where the next task uses it: no
// branch merge right behind the loads, so the epilogue issuing them never waits for their HBM round trip.
template <bool PRE>
GC_DEV void task_operands(const FusedArgs& A, int h, int64_t c, int64_t n_sel, int64_t stride, TaskAhead& ta) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int it_unused;
  const int64_t chunk0 = chunk_first(A, c, &it_unused);
#pragma unroll
  for (int k = 0; k < 6; ++k) ta.xr[k] = A.xi[6 * h + k];
  const int64_t j = chunk0 + wv * 64 + lane;
  const bool ok = j < A.n_cap && j < n_sel;
  const int64_t jc = ok ? j : 0, i = jc * stride;
  ta.np[0] = A.pts_raw[3 * i]; ta.np[1] = A.pts_raw[3 * i + 1]; ta.np[2] = A.pts_raw[3 * i + 2];
  ta.ntt = A.t_raw[i];
  ta.nww = PRE ? A.w_win[jc] : A.w_raw[i];
  ta.ok = ok;
  ta.valid = true;
}
// The persistent form's ticket order: tickets [0, Tf) are the tasks of the launch's nf full-set
// hypotheses (local 0 .. nf - 1), the rest those of its nl lean-set ones (local nf .. nf + nl - 1), each
// range chunk-major (the workgroups in flight share a chunk's raw points across hypotheses in L2).
// Every puller runs its full-set tasks in one loop and its lean-set tasks in the next (k_bins_io), so
// the two variants never meet inside one loop.
struct TaskOrder {
  unsigned Tf;
  int nf, nl;
};
GC_DEV void task_of(const TaskOrder& O, unsigned t, int* h, int64_t* c) {
  const bool f = t < O.Tf;
  const unsigned u = f ? t : t - O.Tf, n = (unsigned)(f ? O.nf : O.nl);
  *c = (int64_t)(u / n);
  *h = (int)(u % n) + (f ? 0 : O.nf);
}
// the budget scalars a launch's tasks share (read once per workgroup)
GC_DEV void selection_of(const FusedArgs& A, int64_t* n_sel, int64_t* stride) {
  *n_sel = (int64_t)A.bscal[5];
  *stride = (int64_t)A.bscal[6];
}

#ifdef GC_BINS_TIMING
// dev instrumentation: per workgroup of the last k_bins_io launch [start, prologue end, end, tasks] in
// device real-time ticks (100 MHz, one clock for every XCD); tasks = -1 for a branch workgroup
__device__ double g_bins_trace[4 * 8192];
__device__ double g_task_trace[4 * 16384];  // per task [start, end, puller, XCD id]
__device__ double g_task_ep[2 * 16384];  // per task [end of its first iteration, start of its epilogue] (wave 0)
__device__ double g_task_wv[4 * 16384];  // per task and wave: the end of its iterations
#define GC_BT_NOW() ((double)__builtin_amdgcn_s_memrealtime())
#endif
// One task: hypothesis h, chunk c (its points: the tiers of FusedArgs) of the budgeted scan,
// its partial record written to rec. Ends with the workgroup synchronised (LDS free for the next task).
// Persistent form (ctr, task_slot, ahead non-null): the next task's ticket is taken by thread 0 at the
// start of the task's last iteration, broadcast through task_slot at the epilogue's first barrier, and
// the next task's operands are loaded into ahead during the rest of the epilogue (T tasks in the
// order ord, task_of).
// n_sel, stride: the launch's selection (selection_of), always given by the caller. The non-look-ahead
// persistent form measured better with it left in vector registers than moved to scalar ones (H = 256
// 1.1568 against 1.1592 ms; profiles/r06/ab_bins_epilogue.txt).
// LEAN: the lean feature set (NF_LEAN, gc_binfin.h), all on the matrix core: no direction scatter, no
// VALU moment feature, no trace complement; the record's first B * NF_LEAN + REC_EXTRA doubles. Only the
// late-ticket instantiation of k_bins_io runs it (see there).
// ENTM (with LEAN): the entropy partial Σ R x of a chunk without padding points on the three free MFMA
// columns instead of 3 v_fmac_f64 per step. Long tasks only (the late-ticket instantiation): H = 256
// 1.0621 -> 1.0504 ms per step, but the epilogue's per-bin dot made H = 32's short tasks 0.6 % slower
// (profiles/r08/ab_bins_lean.txt).
template <int BPL, bool FULL, bool PRE, bool LEAN = false, bool ENTM = false>
GC_DEV void bins_task(const FusedArgs& A, int h, int64_t c, double* lds, double* rec, unsigned* ctr,
                      unsigned* task_slot, TaskAhead* ahead, unsigned T, const TaskOrder& ord, unsigned* late_next, int bt_task,
                      int64_t n_sel, int64_t stride) {
  (void)bt_task;
  // softmax steps per 16-lane sum and reciprocal (group16_sum2). B = 16 (one bin per lane, every lane full)
  // keeps the per-step sum: its lane partial is a bare product t p, which the compiler fuses into the
  // butterfly's first add (Z starts as fma(t, p, partner)); the batched first round adds a selected value,
  // which would round the product first: other bits
  constexpr int ZB = FULL && BPL == 1 ? 1 : 2;
  static_assert(kFusedUnr % ZB == 0, "the unrolled block holds whole batches");
  static_assert(LEAN || !ENTM, "the entropy columns are the lean set's free ones");
  constexpr int NF = LEAN ? NF_LEAN : NF_BASE;
  // features 0..8 and 10..16 on the matrix core, 17..18 on the VALU; feature 9 (w d_z²) is the trace
  // complement N − w d_x² − w d_y² (write_partial_record_mfma<.., 9>): one VALU feature fewer per step.
  // LEAN: the 13 features on MFMA columns 0..12 in the base order; columns 13..15 read the slab's next
  // rows (the unweighted direction: finite values, 16 distinct bank groups) and are dropped
  constexpr int DF = LEAN ? -1 : 9;
  constexpr int NX = LEAN ? 0 : NF - 16 - 1;
  constexpr int NC = LEAN ? NF_LEAN : 16;
  constexpr int NS = kFusedNS;  // the slab stride of either set (a lean slab uses its first NF_LEAN + 4 rows)
  const int64_t n_cap = A.n_cap;
  const int B = A.B;
  int iters;
  const int64_t chunk0 = chunk_first(A, c, &iters);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int g = lane >> 4, bl = lane & 15;
  const int fcol = LEAN ? bl : (bl >= DF ? bl + 1 : bl);  // the slab row of this lane's MFMA column
  double* F = lds + wv * (NS * kFusedFS);
  const double o[3] = {A.o0, A.o1, A.o2};
  // the twist and iteration 0's raw point: loaded by the previous task's epilogue (persistent form), or
  // here
  TaskAhead ta_local;
  TaskAhead& ta = ahead ? *ahead : ta_local;
  if (!ahead || !ahead->valid) task_operands<PRE>(A, h, c, n_sel, stride, ta);
  double xr[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) xr[k] = ta.xr[k];
  const double* __restrict__ pts_raw = A.pts_raw;
  const double* __restrict__ t_raw = A.t_raw;
  const double* __restrict__ w_raw = A.w_raw;
  const double t0 = A.t0, t1 = A.t1;
  const double scale = A.bscal[2];
  const double denom = fmax(t1 - t0, 1e-12);
  const double inv_denom = 1.0 / denom;
  const double inv_sig = 1.0 / fmax(0.1 * denom, 1e-6);
  double* Tx = lds + 4 * kFusedFS * NS;
  double* Lb = Tx + kExpTab2;
  const double ysc = A.inv_tau * kTab2OverLn2;
  constexpr int NACC = kFusedNacc;
  v4d acc4[NACC][BPL];  // NACC = 2: even / odd steps, 2*BPL independent MFMA accumulation chains
  double accx[BPL][NX > 0 ? NX : 1];
#pragma unroll
  for (int j = 0; j < BPL; ++j) {
    acc4[0][j] = v4d{0.0, 0.0, 0.0, 0.0};
    acc4[NACC - 1][j] = v4d{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int t = 0; t < NX; ++t) accx[j][t] = 0.0;
  }
  double sumw = 0.0, entq = 0.0, mxr = 0.0;
  // Π Z of the lane's point group over the whole chunk as mantissa x 2^zex: renormalised every 8
  // points (Z >= e^{(S_max - 1)/τ} per point, so 8 factors stay normal for every τ the exp table
  // admits unless a direction lies almost opposite every bin), one log at the end
  double zst = 1.0;
  int zex = 0;
  // S <= 1 for unit vectors: the exp argument y - ymax = (S·ysc - ymax) <= 0 with an integer ymax
  // >= ysc (the shift cancels in R and is added back to the entropy below)
  const double ymax = ceil(ysc);
  const double Mp = kRoundMagic - ymax;  // the shift rides in the rounding constant (exp2s_shift_n)
  // raw point of the next iteration, loaded one iteration ahead (its HBM latency hides behind
  // this iteration's soft assignment)
  double np[3] = {0.0, 0.0, 0.0}, ntt = 0.0, nww = 0.0;
  auto fetch = [&](int it2) {
    const int64_t j = chunk0 + (int64_t)it2 * 256 + wv * 64 + lane;
    np[0] = 0.0; np[1] = 0.0; np[2] = 0.0; ntt = 0.0; nww = 0.0;
    if (j < n_cap && j < n_sel) {
      const int64_t i = j * stride;
      np[0] = pts_raw[3 * i]; np[1] = pts_raw[3 * i + 1]; np[2] = pts_raw[3 * i + 2];
      ntt = t_raw[i];
      nww = PRE ? A.w_win[j] : w_raw[i];  // PRE: the window is already applied (once per scan)
    }
  };
  {
    const bool ok = ta.ok;  // applied here, a task after the loads were issued
    np[0] = ok ? ta.np[0] : 0.0; np[1] = ok ? ta.np[1] : 0.0; np[2] = ok ? ta.np[2] : 0.0;
    ntt = ok ? ta.ntt : 0.0; nww = ok ? ta.nww : 0.0;
  }
  unsigned next = 0;
  // A chunk without padding points (all of it below n_cap: every chunk but the last) runs with
  // the valid flag folded to 1.0 — the masking multiplies vanish (x·1 = x, fma(Z−1, 1, 1) = Z
  // exactly), bit-identical to the masked form
  auto run_iters = [&](auto pad_tag) {
    constexpr bool PAD = decltype(pad_tag)::value;
    // ENTM without padding points: Σ_p R_pb x_pb is left to the matrix core. x_pb = L_b · d_p, and the free
    // columns 13..15 accumulate Σ_p R_pb d_p from the slab's direction rows (the epilogue's 3-term dot per
    // bin below). The padded form keeps the VALU sum: its padding points' directions are not zero.
    constexpr bool kEntMfma = ENTM && !PAD;
    for (int it = 0; it < iters; ++it) {
      const int64_t wbase = chunk0 + (int64_t)it * 256 + wv * 64;
      // the next task's ticket, a whole iteration before the epilogue that broadcasts it (its round trip
      // is long done by then; the ticket is held one iteration, not the whole task)
      if (ctr && !late_next && it == iters - 1 && threadIdx.x == 0) next = atomicAdd(ctr, 1u);
      {  // phase A
        const int64_t j = wbase + lane;
        const bool inr = j < n_cap;
        double p[3] = {np[0], np[1], np[2]};
        const double tt = ntt, ww = nww * scale;
        if (it + 1 < iters) fetch(it + 1);
        double q[3], d[3], f[NF_BASE];
        const double al = (tt - t0) * inv_denom;
        {  // six series terms when every lane of the wave has θ² <= kDeskewShortTs (wave-uniform branch)
          const double ph[3] = {al * xr[3], al * xr[4], al * xr[5]};
          if (__all(dot3(ph, ph) <= kDeskewShortTs)) deskew_point_cross<true>(p, al, xr, q);
          else deskew_point_cross<false>(p, al, xr, q);
        }
        const double wd = inr ? (PRE ? ww : ww * window_weight2(tt, t0, t1, inv_sig, Tx)) : 0.0;
        direction_fast(q, o, 1e-12, d);
        point_features_w(q, d, wd, f);
        sumw += wd;
        if constexpr (LEAN) {
  #pragma unroll
          for (int k = 0; k < NF; ++k) F[k * kFusedFS + lane] = f[k < 4 ? k : k + 6];  // w, w d | w p, w p pᵀ
        } else {
  #pragma unroll
        for (int k = 0; k < NF; ++k)
          if (k != DF) F[k * kFusedFS + lane] = f[k];
        }
        F[(NF + 0) * kFusedFS + lane] = d[0];
        F[(NF + 1) * kFusedFS + lane] = d[1];
        F[(NF + 2) * kFusedFS + lane] = d[2];
        F[(NF + 3) * kFusedFS + lane] = inr ? 1.0 : 0.0;
      }
      lds_wave_sync();
      for (int s8 = 0; s8 < 16; s8 += kFusedUnr) {
        // Per step (B = 16): logits, exps, the 16-lane sum Z and 1/Z, responsibilities, moments. Kept as
        // its own block beside the batched form below: the block's schedule follows the order of the source,
        // and the same statements arranged as a batch of one ran 1 % slower at H = 32
        // (profiles/r07/ab_bins_zbatch.txt)
        if constexpr (ZB == 1) {
  #pragma unroll
      for (int s = s8; s < s8 + kFusedUnr; ++s) {
        const int pl = s * 4 + g;
        const double d0 = F[(NF + 0) * kFusedFS + pl], d1 = F[(NF + 1) * kFusedFS + pl], d2 = F[(NF + 2) * kFusedFS + pl];
        const double vf = PAD ? F[(NF + 3) * kFusedFS + pl] : 1.0;  // 1 for a point of the chunk, 0 for padding
        const double fb = F[fcol * kFusedFS + pl];  // MFMA B operand: feature fcol of point 4s + g
        double e[BPL], x[BPL], ex[BPL];
  #pragma unroll
        for (int j = 0; j < BPL; ++j) {
          const int b = bl + 16 * j;  // Lb is zero past B: y = -ymax stays in range, then masked
          x[j] = fma(d0, Lb[b], fma(d1, Lb[64 + b], d2 * Lb[128 + b]));
        }
        exp2s_shift_tab_n<BPL, 8u * 4u * kFusedFS * kFusedNS>(x, Mp, ex);  // Tx at that absolute address
  #pragma unroll
        for (int j = 0; j < BPL; ++j) e[j] = (FULL || bl + 16 * j < B) ? ex[j] : 0.0;
        double zl = e[0];
  #pragma unroll
        for (int j = 1; j < BPL; ++j) zl += e[j];
        const double Z = group16_sum(zl);
        const double rZ = recip1(Z);
        double r[BPL];
  #pragma unroll
        for (int j = 0; j < BPL; ++j) r[j] = e[j] * rZ;
        double rm = r[0];  // max responsibility: max(e) rZ == max(e rZ) exactly (monotone rounding)
  #pragma unroll
        for (int j = 1; j < BPL; ++j) rm = fmax(rm, r[j]);
        // padding points (vf = 0) add nothing: S/Z scaled by 0, r >= 0 scaled to 0 under the max,
        // and log Z replaced by log 1
        if constexpr (!kEntMfma)
  #pragma unroll
        for (int j = 0; j < BPL; ++j)  // lane partials of Σ R·x (in y units), summed over lanes at the end
          entq = fma(r[j] * vf, x[j], entq);
        mxr = fmax(mxr, rm * vf);
        zst *= PAD ? fma(Z - 1.0, vf, 1.0) : Z;  // Π Z of the group's points (<= 48^8 per renormalisation)
  #pragma unroll
        for (int j = 0; j < BPL; ++j)
          acc4[s % NACC][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(r[j], fb, acc4[s % NACC][j], 0, 0, 0);
  #pragma unroll
        for (int t = 0; t < NX; ++t) {
          const double fk = F[(17 + t) * kFusedFS + pl];
  #pragma unroll
          for (int j = 0; j < BPL; ++j) accx[j][t] = fma(r[j], fk, accx[j][t]);
        }
      }
        } else {
        // Two steps at a time: their logits, exps and in-lane sums, then the 16-lane sums and one reciprocal
        // (group16_sum2), then each step's responsibilities and moments in step order and with the per-step
        // form's expressions
  #pragma unroll
      for (int sb = s8; sb < s8 + kFusedUnr; sb += ZB) {
        double e[ZB][BPL], x[ZB][BPL], zl[ZB], Z[ZB], rZ[ZB];
  #pragma unroll
        for (int u = 0; u < ZB; ++u) {
          const int pl = (sb + u) * 4 + g;
          const double d0 = F[(NF + 0) * kFusedFS + pl], d1 = F[(NF + 1) * kFusedFS + pl], d2 = F[(NF + 2) * kFusedFS + pl];
          double et[BPL], ep[BPL];
  #pragma unroll
          for (int j = 0; j < BPL; ++j) {
            const int b = bl + 16 * j;
            x[u][j] = fma(d0, Lb[b], fma(d1, Lb[64 + b], d2 * Lb[128 + b]));
          }
          exp2s_shift_tab_tp_n<BPL, 8u * 4u * kFusedFS * kFusedNS>(x[u], Mp, et, ep);
  #pragma unroll
          for (int j = 0; j < BPL; ++j) e[u][j] = (FULL || bl + 16 * j < B) ? et[j] * ep[j] : 0.0;
          // the in-lane sum. With every bin lane full each e is a bare product t p, and in the per-step
          // form the compiler's contraction fuses products of e0 + e1 + .. into the adds: e1 + t0 p0
          // unrounded, then + t_j p_j unrounded for j >= 2, in every step of every instantiation. Which
          // products fuse follows the surrounding code (left to the compiler here, it changed from step
          // to step), so it is written out: Z keeps the per-step form's bits. The masked form adds
          // selected values, which never fuse.
          if constexpr (FULL && BPL > 1) {
            zl[u] = fma(et[0], ep[0], e[u][1]);
  #pragma unroll
            for (int j = 2; j < BPL; ++j) zl[u] = fma(et[j], ep[j], zl[u]);
          } else {
            zl[u] = e[u][0];
  #pragma unroll
            for (int j = 1; j < BPL; ++j) zl[u] += e[u][j];
          }
        }
        group16_sum2(zl, lane, Z, rZ);
  #pragma unroll
        for (int u = 0; u < ZB; ++u) {
          const int s = sb + u;
          const int pl = s * 4 + g;
          const double vf = PAD ? F[(NF + 3) * kFusedFS + pl] : 1.0;
          const double fb = F[fcol * kFusedFS + pl];
          double r[BPL];
  #pragma unroll
          for (int j = 0; j < BPL; ++j) r[j] = e[u][j] * rZ[u];
          double rm = r[0];
  #pragma unroll
          for (int j = 1; j < BPL; ++j) rm = fmax(rm, r[j]);
          if constexpr (!kEntMfma)
  #pragma unroll
          for (int j = 0; j < BPL; ++j) entq = fma(r[j] * vf, x[u][j], entq);
          mxr = fmax(mxr, rm * vf);
          zst *= PAD ? fma(Z[u] - 1.0, vf, 1.0) : Z[u];
  #pragma unroll
          for (int j = 0; j < BPL; ++j)
            acc4[s % NACC][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(r[j], fb, acc4[s % NACC][j], 0, 0, 0);
  #pragma unroll
          for (int t = 0; t < NX; ++t) {
            const double fk = F[(17 + t) * kFusedFS + pl];
  #pragma unroll
            for (int j = 0; j < BPL; ++j) accx[j][t] = fma(r[j], fk, accx[j][t]);
          }
        }
      }
        }
        int e8;
        zst = frexp(zst, &e8);
        zex += e8;
      }
      lds_wave_sync();
#ifdef GC_BINS_TIMING
      if (it == 0 && threadIdx.x == 0 && bt_task >= 0 && bt_task < 16384) g_task_ep[2 * bt_task] = GC_BT_NOW();
#endif
    }
  };
  if (chunk0 + (int64_t)iters * 256 <= n_cap) run_iters(std::false_type{});
  else run_iters(std::true_type{});
#ifdef GC_BINS_TIMING
  if (threadIdx.x == 0 && bt_task >= 0 && bt_task < 16384) g_task_ep[2 * bt_task + 1] = GC_BT_NOW();
  if ((threadIdx.x & 63) == 0 && bt_task >= 0 && bt_task < 16384) g_task_wv[4 * bt_task + (threadIdx.x >> 6)] = GC_BT_NOW();
#endif
  // entropy sum over the chunk's valid points: Σ log Z - Σ S/Z - B ε
  int64_t npts = n_cap - chunk0;
  npts = npts < 0 ? 0 : (npts > (int64_t)iters * 256 ? (int64_t)iters * 256 : npts);
  // the 16 lanes of a point group hold the same product: only bin-lane 0 of each group contributes
  // its log. Σ log Z' (shifted by ymax) - Σ R y + ymax per valid point - B ε per point (lane 0 of
  // each wave)
  const double logacc = log_pos(zst) + (double)zex * 0.69314718055994530942;
#pragma unroll
  for (int j = 0; j < BPL; ++j)
    if (NACC == 2) acc4[0][j] += acc4[NACC - 1][j];
  if constexpr (ENTM) {
    // Σ_p R_pb x_pb of a chunk without padding points (kEntMfma): lane (g, 13 + k) holds Σ_p R_pb d_pk of
    // bins b = 16 j + g + 4 r; Lb is zero past B
    if (chunk0 + (int64_t)iters * 256 <= n_cap && bl >= NF)
#pragma unroll
      for (int j = 0; j < BPL; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) entq = fma(acc4[0][j][r], Lb[(bl - NF) * 64 + 16 * j + g + 4 * r], entq);
  }
  const double ent = (bl == 0 ? logacc : 0.0) - entq * kExp2C1 +
                     ((lane == 0) ? ent_shift(A.inv_tau, B) * (double)npts : 0.0);
  if (ahead) ahead->valid = false;
  // without the look-ahead (late_next): the ticket taken here, its round trip overlapping the epilogue,
  // and broadcast by the caller after it
  if (ctr && late_next && threadIdx.x == 0) *late_next = atomicAdd(ctr, 1u);
  const auto pre = [&]() {  // before the epilogue's first barrier: the ticket into the task slot
    if (ctr && !late_next && threadIdx.x == 0) *task_slot = next;
  };
  const auto mid = [&]() {  // after it: every lane reads the ticket and loads the next task's operands
    if (!ctr || late_next) return;
    const unsigned tn = *task_slot;
    ahead->t = tn;
    if (tn < T) {
      int hn;
      int64_t cn;
      task_of(ord, tn, &hn, &cn);
      task_operands<PRE>(A, hn, cn, n_sel, stride, *ahead);
    }
  };
  write_partial_record_mfma<BPL, NX, DF, FULL, NS * kFusedFS, NC>(acc4[0], accx, ent, mxr, sumw, (double)npts, B, lds, rec, pre, mid);
  __syncthreads();  // the epilogue's LDS reads are done before the next task writes the slabs
}

}  // namespace gc
