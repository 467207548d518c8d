// gc_binplan.h — the task plan of the persistent bins launch (scan_bins_pipeline, gc_bins.hip): how the
// 256-point units of a budgeted scan are cut into long, short and tiny chunks, and which k_bins_io form runs
// them. Pure host arithmetic: it fixes the order of summation (a hypothesis's records are summed in chunk
// order, which is why PipeDev::geom_H exists) and is exposed as gc_bins_task_plan.
#pragma once
#include <stdint.h>
#include <algorithm>

namespace gc {
// The task tiers of scan_bins_pipeline: long chunks for the bulk, then short ones, then tiny ones.
// >= 2 long tasks per puller: with the late ticket and the tiny tier the tail no longer needs a third,
// and fewer, longer tasks amortise each task's set-up and record epilogue: H = 32 4 -> 8 iterations,
// 92 -> 62 chunks, 0.2892 -> 0.2800 ms/scan (3 tasks: 0.2892, 1: 0.2848; profiles/r04/ab_bins_tail.txt);
// H >= 64 keep 16
constexpr int kBinsMinTasks = 2;
// short tasks of half a long one, at least 2 iterations: H = 256 8-iteration short tasks (interleaved
// A/B on one box, 1.2499/1.2463 ms/scan with 4 -> 1.2377/1.2391 with 8); H = 32 (4-iteration long
// tasks) 2, which stays best there (0.3013/0.3004/0.3003 ms against 0.305-0.313 for 8-iteration long
// tasks with 2- or 4-iteration short ones and for 4-iteration tasks only; tools/ab32.sh)
constexpr int kShortDiv = 2;
// a third tier of tiny tasks (a quarter of a short one) at the very end, about one per puller: with
// the next ticket taken before each task's epilogue (k_bins_io) the pullers' end spread fell from
// 57 to ~24 us at H = 256 (GC_BINS_TIMING traces); interleaved A/B against the two tiers and the
// ticket taken at the task start, 1.1999 -> 1.1950 ms at H = 256, 0.2930 -> 0.2903 at H = 32
// (profiles/r04/ab_bins_tail.txt; 2 tiny tasks per puller, or an eighth or a half of a short task,
// no better)
constexpr int kTinyDiv = 4, kTinyPerPuller = 1;
// the short tier's work: one long task per puller when every puller has at least 4 long tasks (H = 256),
// three quarters of one with fewer 32-iteration tasks (H = 128: 0.6497 -> 0.6459 ms/scan), half of one when
// the long tasks are shorter (H = 32's 8 iterations, H = 64's 16): with few long tasks per puller the
// epilogues of the many short tasks cost more than the finer tail gains (H = 32 0.2586 -> 0.2548 ms/scan;
// H = 256 1.1624 against 1.1656 with half, 1.1648 with three quarters; profiles/r05/ab_bins_short_share.txt)
constexpr double kShortShare = 0.5, kShortShare32 = 0.75;

// chunks [0, k1) hold iters x 256 points, the next k2 iters_short x 256, the rest iters_tiny x 256 (FusedArgs)
struct BinsPlan {
  int pullers;  // resident bin workgroups of the launch
  int iters, iters_short, iters_tiny;
  int64_t k1, k2, chunks;
  bool ahead;  // the look-ahead instantiation of k_bins_io (short tasks) rather than the late-ticket one
};

// H_geom: the hypotheses the chunk geometry is sized for (PipeDev::geom_H, or the launch's own count)
inline BinsPlan plan_bins_tasks(int H_geom, int64_t n_cap, int cu_count) {
  const int Hg = H_geom;
  const int pullers = 2 * cu_count;  // 2 resident bin workgroups per CU (VGPR-bound)
  // the largest iteration count that still gives every puller >= 4 tasks (tail <= 1/4 task)
  // Two tiers of chunks, taken in order: long tasks (iters x 256 points, the prologue / epilogue
  // amortised) for the bulk, then short ones (2 x 256) that hold one long task of work per puller,
  // so the pullers run out of work together instead of one long task apart (A/B on one box against
  // half a long task: 1.2998/1.2984/1.2981 vs 1.3004/1.2997/1.2990 ms at H = 256, 0.342 vs 0.345 at 32)
  // (P.geom_H > 0: sized as for a shard of that many hypotheses, the summation order then being the
  // same for every shard size)
  const int64_t U = (n_cap + 255) / 256;  // 256-point units per hypothesis
  // at most 32 iterations (8192 points) per long task: H = 256 1.1935 -> 1.1803 ms, H = 128 0.6706 ->
  // 0.6658 against 16; 64: 1.1872 (profiles/r04/ab_bins_tail.txt)
  int iters = 32;
  while (iters > 2 && (int64_t)Hg * U < kBinsMinTasks * (int64_t)pullers * iters) iters >>= 1;
  const int kItersShort = std::max(2, iters / kShortDiv);
  const int kItersTiny = std::max(1, kItersShort / kTinyDiv);
  int64_t Ut = ((int64_t)pullers * kItersTiny * kTinyPerPuller + Hg - 1) / Hg;
  Ut = std::min<int64_t>((Ut + kItersTiny - 1) / kItersTiny * kItersTiny, U);
  const bool many_long = (int64_t)Hg * U >= 4 * (int64_t)pullers * iters;
  const double short_share = many_long ? 1.0 : (iters >= 32 ? kShortShare32 : kShortShare);
  int64_t Us = std::max<int64_t>(iters, (int64_t)(short_share * (double)pullers * iters + Hg - 1) / Hg);
  Us = std::min(Us, U - Ut);
  const int64_t k1 = (U - Ut - Us) / iters;  // long chunks; the short and tiny tiers take the rest
  const int64_t k2 = (U - Ut - k1 * iters) / kItersShort;
  Ut = U - k1 * iters - k2 * kItersShort;
  const int64_t chunks = k1 + k2 + (Ut + kItersTiny - 1) / kItersTiny;
  // the look-ahead instantiation (the next task's operands loaded during the current task's epilogue,
  // the ticket taken one iteration earlier) for short tasks: H = 32's 8-iteration tasks 0.2597 ->
  // 0.2582 ms; H = 256's 32-iteration tasks keep the late ticket (holding it an iteration longer cost
  // as much as the hidden loads gained, 1.1699 -> 1.1709; profiles/r05/ab_bins_ahead.txt). One
  // instantiation per form: both paths in one kernel raised its spills and cost H = 32 10 us.
  const bool ahead = iters < 32;
  return BinsPlan{pullers, iters, kItersShort, kItersTiny, k1, k2, chunks, ahead};
}
}  // namespace gc
