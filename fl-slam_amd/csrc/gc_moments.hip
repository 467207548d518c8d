// gc_moments.hip — the a6 contract kernel and the bin finalizes (gfx950).
//
//  a6 ScanBinMomentMatch    archive/legacy_operators/binning.py:139-324, kappa.py:130-169
//
// k_moment_partials streams the responsibilities a5 wrote (gc_bins.hip) and sums the per-bin moments on
// the matrix core into one partial record per (hypothesis, chunk); k_bins_finalize and
// k_bins_finalize_split sum the records in chunk order (those of the fused bins kernels as well) and
// finish each bin (gc_binfin.h).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include "gc_internal.h"
#include "gc_binsdev.h"
#include "gc_wgla.h"
#include "gc_binfin.h"

namespace gc {

constexpr int NF_COV = 9;     // full 3x3 point covariance x w
// the moment kernel reads the responsibility stream exactly once: non-temporal loads for the 8-B
// per-lane tiles (A/B on one box, C3 contract launch: 1.548 -> 1.49 ms; the paired 16-B loads of bins
// 0-31 stay temporal: non-temporal there too measured 1.52, profiles/r02/ab_contract_pair_nt.txt)
#define GC_RESP_LOAD(ptr) __builtin_nontemporal_load(ptr)

// ===================================================================== a6 moment partials
// Contract variant: responsibilities streamed from HBM. grid (chunks, H), 4 waves per workgroup,
// each wave owns `groups` consecutive 32-point groups of the chunk. The moment sums
// Mom[b][k] = Σ_p R[p][b] F[p][k] run on the matrix core: per 4-point step s, bin tile j
// (16 bins) x feature tile t (16 features) is one v_mfma_f64_16x16x4_f64 with
// A[bin][point] = R (lane (g, l): point 4s + g, bin 16j + l) and B[point][feature] = F
// (lane (g, l): point 4s + g, feature 16t + l). The A operand is loaded from HBM straight into
// its lane (8 B per lane: four full 128-B row segments per load), a whole 32-point group ahead
// of its use (register double buffer, ~12 KiB of responsibilities in flight per wave); no LDS
// round trip. Features are computed lane = point for the next group and handed over through a
// wave-private LDS slab (feature-major, stride 34: the B-operand reads are bank-conflict free).
// The 4 waves are reduced in a fixed order into one record per chunk.
constexpr int kMomFS = 34;
// PAIR (B >= 32, 16-B aligned rows): bins 0..31 arrive as one 16-B load per lane (bins 2l, 2l+1 of its
// point: four 256-B row segments per load instead of two loads of four 128-B segments); tile 0 holds
// the even bins, tile 1 the odd ones (row i of tile j < 2 is bin 2i + j), tiles >= 2 bins 16j + l.
template <int BPL, bool COV, bool LAM, bool PAIR>
__global__ void __launch_bounds__(256, 2) k_moment_partials(int64_t n, int B, int groups,
                                                           const double* __restrict__ pts,
                                                           const double* __restrict__ covs,
                                                           const double* __restrict__ w,
                                                           const double* __restrict__ resp,
                                                           const double* __restrict__ lam, double o0,
                                                           double o1, double o2, double* partials) {
  constexpr int NF = COV ? NF_BASE + NF_COV : NF_BASE;
  constexpr int NT = (NF + 15) / 16;  // feature tiles (zero-padded to 16 NT)
  extern __shared__ double lds[];
  // workgroups run the (hypothesis, chunk) grid from its end: the soft-assign before this kernel wrote
  // the responsibilities in ascending block order, so the last-written (still in the Infinity Cache /
  // L2) are read first (records, and so the sums, are the same in either order; the forward order measured
  // the same, profiles/r05/ab_soft_assign_store_and_moment_order.txt)
  const int bx = (int)(gridDim.x - 1 - blockIdx.x);
  const int h = (int)(gridDim.y - 1 - blockIdx.y);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, g = lane >> 4, bl = lane & 15;
  double* F = lds + wv * (16 * NT * kMomFS);
  const double o[3] = {o0, o1, o2};
  const double* Rh = resp + (int64_t)h * n * B;
  const int64_t wbeg = ((int64_t)bx * 4 + wv) * groups * 32;
  int64_t wend = wbeg + (int64_t)groups * 32;
  wend = wend < n ? wend : n;
  const int ng = wbeg < n ? (int)((wend - wbeg + 31) / 32) : 0;
  v4d acc[BPL][NT];
#pragma unroll
  for (int j = 0; j < BPL; ++j)
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[j][t] = v4d{0.0, 0.0, 0.0, 0.0};
  // this lane's responsibility column offsets (bins 16 j + l), clamped into the row
  int cb[BPL];
  bool cv[BPL];
#pragma unroll
  for (int j = 0; j < BPL; ++j) {
    cv[j] = bl + 16 * j < B;
    cb[j] = cv[j] ? bl + 16 * j : 0;
  }
  double Ra[8][BPL], Rb[8][BPL];  // group c (A operands of its 8 steps) and group c + 1
#define GC_LOAD_R(RR, BASE)                                                     \
  {                                                                             \
    _Pragma("unroll") for (int s_ = 0; s_ < 8; ++s_) {                          \
      int64_t p_ = (BASE) + 4 * s_ + g;                                         \
      p_ = p_ < wend ? p_ : wend - 1; /* prefetch past the range re-reads a line */ \
      const double* row_ = Rh + p_ * B;                                         \
      if constexpr (PAIR) {                                                     \
        typedef double dv2_ __attribute__((ext_vector_type(2)));                \
        const dv2_ v_ = *reinterpret_cast<const dv2_*>(row_ + 2 * bl);         \
        RR[s_][0] = v_.x;                                                       \
        RR[s_][1] = v_.y;                                                       \
      }                                                                         \
      _Pragma("unroll") for (int j_ = PAIR ? 2 : 0; j_ < BPL; ++j_) RR[s_][j_] = GC_RESP_LOAD(row_ + cb[j_]); \
    }                                                                           \
  }
  // raw inputs of one 32-point group (point = lane & 31), loaded by every lane into registers and
  // consumed branch-free a group later (no load is sunk into a lane-conditional block)
  double rp[3], rc[9], rw, rl;
  bool rok;
#define GC_LOAD_RAW(BASE)                                                       \
  {                                                                             \
    const int64_t pt_ = (BASE) + (lane & 31);                                   \
    rok = pt_ < wend;                                                           \
    const int64_t row_ = (int64_t)h * n + (rok ? pt_ : wend - 1);               \
    rw = w[row_];                                                               \
    if constexpr (LAM) rl = lam[row_];                                          \
    rp[0] = pts[3 * row_]; rp[1] = pts[3 * row_ + 1]; rp[2] = pts[3 * row_ + 2]; \
    if constexpr (COV) {                                                        \
      _Pragma("unroll") for (int k_ = 0; k_ < 9; ++k_) rc[k_] = covs[9 * row_ + k_]; \
    }                                                                           \
  }
  // lanes 0..31 write features 0..15 of their point, lanes 32..63 features 16..31
  // (pp[11 12 22], cov x w, zero padding)
#define GC_FEATURES()                                                           \
  {                                                                             \
    lds_wave_sync(); /* the previous group's B-operand reads are done */        \
    double wl_ = LAM ? rw * rl : rw;                                            \
    wl_ = rok ? wl_ : 0.0;                                                      \
    double d_[3], f_[NF_BASE];                                                  \
    direction(rp, o, 1e-12, d_);                                                \
    point_features(rp, d_, wl_, f_);                                            \
    const bool lo_ = lane < 32;                                                 \
    double* Fl_ = F + (lo_ ? 0 : 16 * kMomFS) + (lane & 31);                    \
    _Pragma("unroll") for (int k_ = 0; k_ < 16; ++k_) {                         \
      const int kk_ = 16 + k_;                                                  \
      double hi_ = 0.0;                                                         \
      if (kk_ < NF_BASE) hi_ = f_[kk_ < NF_BASE ? kk_ : 0];                      \
      else if (COV && kk_ < NF) hi_ = wl_ * rc[kk_ - NF_BASE < 9 ? kk_ - NF_BASE : 0]; \
      Fl_[k_ * kMomFS] = lo_ ? f_[k_] : hi_;                                    \
    }                                                                           \
    lds_wave_sync();                                                            \
  }
#define GC_CONSUME(RR)                                                          \
  {                                                                             \
    _Pragma("unroll") for (int s_ = 0; s_ < 8; ++s_) {                          \
      double fb_[NT];                                                           \
      _Pragma("unroll") for (int t_ = 0; t_ < NT; ++t_) fb_[t_] = F[(16 * t_ + bl) * kMomFS + 4 * s_ + g]; \
      _Pragma("unroll") for (int j_ = 0; j_ < BPL; ++j_) {                      \
        const double ra_ = cv[j_] ? RR[s_][j_] : 0.0;                           \
        _Pragma("unroll") for (int t_ = 0; t_ < NT; ++t_)                       \
          acc[j_][t_] = __builtin_amdgcn_mfma_f64_16x16x4f64(ra_, fb_[t_], acc[j_][t_], 0, 0, 0);         \
      }                                                                         \
    }                                                                           \
  }
  if (ng > 0) {
    // loads past the wave's range are issued unconditionally (clamped rows, zero weights) so the
    // body is straight-line and every wait is a counted vmcnt, not a drain
    GC_LOAD_RAW(wbeg)
    __builtin_amdgcn_sched_barrier(0);
    GC_LOAD_R(Ra, wbeg)
    __builtin_amdgcn_sched_barrier(0);
    for (int c = 0; c < ng; c += 2) {
      GC_FEATURES()
      const int64_t b1 = wbeg + 32 * (int64_t)(c + 1);
      GC_LOAD_RAW(b1)  // raw first: the next features wait for these, not for the R stream
      __builtin_amdgcn_sched_barrier(0);
      GC_LOAD_R(Rb, b1)
      __builtin_amdgcn_sched_barrier(0);  // keep the prefetch ahead of the consumption
      GC_CONSUME(Ra)
      __builtin_amdgcn_sched_barrier(0);
      GC_FEATURES()
      const int64_t b2 = wbeg + 32 * (int64_t)(c + 2);
      GC_LOAD_RAW(b2)
      __builtin_amdgcn_sched_barrier(0);
      GC_LOAD_R(Ra, b2)
      __builtin_amdgcn_sched_barrier(0);
      GC_CONSUME(Rb)
      __builtin_amdgcn_sched_barrier(0);
    }
  }
#undef GC_LOAD_R
#undef GC_LOAD_RAW
#undef GC_FEATURES
#undef GC_CONSUME
  // epilogue: the 4 waves in a fixed order (LDS reused)
  __syncthreads();
  double* red = lds;  // [4][B][NF]
#pragma unroll
  for (int j = 0; j < BPL; ++j)
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int b = (PAIR && j < 2) ? 2 * (g + 4 * r) + j : 16 * j + g + 4 * r, k = 16 * t + bl;  // D[row g + 4r][col l]
        if (b < B && k < NF) red[(wv * B + b) * NF + k] = acc[j][t][r];
      }
  __syncthreads();
  int64_t npts = n - (int64_t)bx * 4 * groups * 32;
  npts = npts < 0 ? 0 : (npts > (int64_t)4 * groups * 32 ? (int64_t)4 * groups * 32 : npts);
  const int RL = B * NF + REC_EXTRA;
  double* rec = partials + ((int64_t)h * gridDim.x + bx) * RL;
  for (int i = threadIdx.x; i < B * NF; i += kWG)
    rec[i] = (red[i] + red[B * NF + i]) + (red[2 * B * NF + i] + red[3 * B * NF + i]);
  if (threadIdx.x < REC_EXTRA) rec[B * NF + threadIdx.x] = threadIdx.x == 3 ? (double)npts : 0.0;
}

// ================================================================ finalize (a6 + certs)
// One workgroup per hypothesis: chunk records summed in order, per-bin moments -> p̄, Σ_p
// (PSD-projected), κ; cert reductions in a fixed order.
// one hypothesis h (the whole workgroup); sm: B*NF + REC_EXTRA + 8 doubles
// One hypothesis h on a 1024-thread workgroup (kFinWG): the entry sums with 4x the loads in flight of
// a 256-thread one (the reduction is L2-latency-bound at small H), then per-bin moments -> p̄, Σ_p
// (PSD-projected), κ on lanes b < B of wave 0 (B <= 64) and the cert reductions on that wave.
// sm: B*NF + REC_EXTRA doubles.
constexpr int kFinWG = 1024;
GC_DEV void finalize_hyp(int h, int B, int NF, int64_t chunks, const double* __restrict__ partials, double eps_psd,
                         double eps_mass, double* stats, double* cert, double* sm) {
  const int RL = B * NF + REC_EXTRA;
  const double* P = partials + (int64_t)h * chunks * RL;
  const int imax = B * NF + 1;  // the max-responsibility entry reduces by fmax
  if (RL <= kFinWG) finalize_reduce<1, 32>(P, RL, RL, imax, chunks, sm);
  else finalize_reduce<2, 16>(P, RL, RL, imax, chunks, sm);
  __syncthreads();
  double Nl = 0.0, N2l = 0.0, psdl = 0.0, epsl = 0.0, sfl = 0.0;
  if ((int)threadIdx.x < B) {
    const int b = threadIdx.x;
    const double N = sm[b * NF];
    finalize_bin(sm + b * NF, NF, eps_psd, eps_mass, stats + ((int64_t)h * B + b) * GC_BIN_STATS, &psdl, &epsl);
    Nl = N; N2l = N * N; sfl = N / (N + eps_mass);
  }
  if (threadIdx.x >= 64) return;  // every bin lives on wave 0 (B <= 64)
  const double Nt = wave_sum(Nl);
  const double N2 = wave_sum(N2l);
  const double psd = wave_sum(psdl);
  const double mer = wave_max(epsl);
  const double sf = wave_sum(sfl);
  if (threadIdx.x == 0) {
    const double* ex = sm + B * NF;
    double* c = cert + (int64_t)h * GC_BIN_CERT;
    c[0] = Nt * Nt / (N2 + eps_mass);
    c[1] = sf / (double)B;
    c[2] = psd;
    c[3] = mer;
    c[4] = ex[0] / (ex[3] + eps_mass);
    c[5] = ex[1];
    c[6] = ex[2];
    c[7] = psd + mer;
  }
}
__global__ void __launch_bounds__(kFinWG) k_bins_finalize(int B, int NF, int64_t chunks,
                                                       const double* __restrict__ partials,
                                                       double eps_psd, double eps_mass,
                                                       double* stats, double* cert) {
  extern __shared__ double sm[];  // B*NF + 8 + 4
  finalize_hyp(blockIdx.x, B, NF, chunks, partials, eps_psd, eps_mass, stats, cert, sm);
}

// The batched pipeline's finalize, split over bins: grid (S, H), workgroup s of hypothesis h owns
// bins [s kFinBins, (s+1) kFinBins) (and, the last one, the record's extra entries). One lane per
// record entry sums the chunk records in chunk order (finalize_reduce's order and batching, so
// every sum is bit-identical to k_bins_finalize's), then one lane per bin runs finalize_bin. At
// small H this spreads a hypothesis's ~0.6 MB of records over S CUs instead of one (k_bins_finalize
// is bound by one CU's load rate there). The cross-bin certificate reductions need every bin: the
// per-bin projection delta and mass-epsilon ratio go to aux (H, B, 2) and k_evidence reduces them
// (finalize_cert), in k_bins_finalize's wave_sum order.
constexpr int kFinBins = 6;
constexpr int kFinKU = 16;  // chunk records in flight per lane in the split finalize (one L2 round trip per batch)
constexpr int kFinSplitWG = 128;
static_assert(kFinBins * NF_BASE + REC_EXTRA <= kFinSplitWG, "one lane per record entry");
__global__ void __launch_bounds__(kFinSplitWG) k_bins_finalize_split(int B, int NF, int64_t chunks,
                                                                     const double* __restrict__ partials,
                                                                     double eps_psd, double eps_mass, double* stats,
                                                                     double* cert, double* aux, int64_t* done_word,
                                                                     int64_t ticket, int n_full, int lean_records) {
  __shared__ double sm[kFinBins * NF_BASE + REC_EXTRA];
  // the bins launch before this one on the stream has completed, its reads of the scan slot
  // included: publish the scan's ticket to the host-coherent word the pipeline's staging checks.
  // Relaxed at system scope: one write-through store, no L2 writeback (nothing written before it
  // has to be visible to the host).
  if (done_word && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0)
    __hip_atomic_store(done_word, ticket, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  const int h = blockIdx.y, s = blockIdx.x;
  const int RL = B * NF + REC_EXTRA;  // the record slot of either feature set
  // hypotheses [0, n_full) keep their direction scatter (bin_scatter_full_count); the others' is written
  // as 0.0, and with lean_records their records hold the lean set at the head of their slots (k_bins_io)
  const bool zero_scatter = h >= n_full, lean = zero_scatter && lean_records;
  if (lean) NF = NF_LEAN;
  const int b0 = s * kFinBins, nb = min(kFinBins, B - b0);
  const bool last = s == (int)gridDim.x - 1;
  const int ne = nb * NF + (last ? REC_EXTRA : 0);
  const int e0 = b0 * NF, imax = B * NF + 1;
  const double* P = partials + (int64_t)h * chunks * RL;
  const int t = threadIdx.x;
  if (t < ne) {
    const int e = e0 + t;
    constexpr int KU = kFinKU;
    double v = 0.0;
    for (int64_t c = 0; c < chunks; c += KU) {
      double x[KU];
#pragma unroll
      for (int u = 0; u < KU; ++u) x[u] = c + u < chunks ? P[(c + u) * RL + e] : 0.0;
#pragma unroll
      for (int u = 0; u < KU; ++u) v = e == imax ? fmax(v, x[u]) : v + x[u];
    }
    sm[t] = v;
  }
  __syncthreads();
  if (t < nb) {
    double* ax = aux + ((int64_t)h * B + b0 + t) * 2;
    finalize_bin(sm + t * NF, NF, eps_psd, eps_mass, stats + ((int64_t)h * B + b0 + t) * GC_BIN_STATS, ax, ax + 1,
                 zero_scatter);
  } else if (last && t == 64) {
    const double* ex = sm + nb * NF;
    double* c = cert + (int64_t)h * GC_BIN_CERT;
    c[4] = ex[0] / (ex[3] + eps_mass);
    c[5] = ex[1];
    c[6] = ex[2];
  }
}

int32_t launch_bins_finalize(gc_ctx* ctx, int H, int B, int NF, int64_t chunks, const double* partials,
                             double eps_psd, double eps_mass, double* stats, double* cert) {
  const size_t sh = sizeof(double) * (B * NF + REC_EXTRA);
  hipLaunchKernelGGL(k_bins_finalize, dim3(H), dim3(kFinWG), sh, ctx->stream, B, NF, chunks, partials, eps_psd,
                     eps_mass, stats, cert);
  GC_LAUNCH_CHECK(ctx);
  return GC_OK;
}

int32_t launch_bins_finalize_split(gc_ctx* ctx, int H, int B, int NF, int64_t chunks, const double* partials,
                                   double eps_psd, double eps_mass, double* stats, double* cert, double* aux,
                                   int64_t* done_word, int64_t ticket, int n_full, int lean_records) {
  const dim3 fgrid((unsigned)((B + kFinBins - 1) / kFinBins), (unsigned)H);
  hipLaunchKernelGGL(k_bins_finalize_split, fgrid, dim3(kFinSplitWG), 0, ctx->stream, B, NF, chunks, partials,
                     eps_psd, eps_mass, stats, cert, aux, done_word, ticket, n_full, lean_records);
  GC_LAUNCH_CHECK(ctx);
  return GC_OK;
}

}  // namespace gc

using namespace gc;

extern "C" {

int32_t gc_scan_bin_moment_match(gc_ctx* ctx, int32_t H, int64_t n, int32_t B, const double* d_points,
                                 const double* d_covs, const double* d_w, const double* d_resp,
                                 const double* d_lambda, const double* h_origin3, double eps_psd, double eps_mass,
                                 double* d_stats_out, double* d_cert_out) {
  GC_CHECK_ARG(nullptr, ctx != nullptr, "ctx is NULL");
  GC_CHECK_ARG(ctx, H > 0 && n > 0, "H and n must be positive");
  GC_CHECK_ARG(ctx, B >= 1 && B <= 64, "B must be in [1, 64]");
  GC_CHECK_ARG(ctx, d_points && d_w && d_resp && d_stats_out && d_cert_out, "NULL buffer");
  double o[3] = {0.0, 0.0, 0.0};
  if (h_origin3) { o[0] = h_origin3[0]; o[1] = h_origin3[1]; o[2] = h_origin3[2]; }
  // chunk = 4 waves x groups x 32 points; aim for >= ~8 workgroups per CU over the grid
  int groups = 16;
  while (groups > 1 && ((n + 128 * groups - 1) / (128 * groups)) * (int64_t)H < 4096) groups >>= 1;
  const int64_t chunks = (n + 128 * groups - 1) / (128 * groups);
  const bool cov = d_covs != nullptr;
  const int NF = cov ? NF_BASE + NF_COV : NF_BASE;
  const int RL = B * NF + REC_EXTRA;
  void* scr;
  if (int rc = gc::scratch(ctx, sizeof(double) * RL * chunks * H, &scr)) return rc;
  dim3 grid((unsigned)chunks, H);
  const int NT = (NF + 15) / 16;
  const size_t sh = sizeof(double) * std::max<size_t>((size_t)4 * 16 * NT * kMomFS, (size_t)4 * B * NF);
  const bool pair = B >= 32 && ((uintptr_t)d_resp & 15) == 0;
  // PAIR only ever with BPL >= 2 (B >= 32)
  dispatch_bpl(B, cov, [&](auto bp, auto cov_tag) {
    dispatch_bool(d_lambda != nullptr, [&](auto lam_tag) {
      dispatch_bool(pair, [&](auto pair_tag) {
        constexpr int BP = decltype(bp)::value;
        constexpr bool CV = decltype(cov_tag)::value, LM = decltype(lam_tag)::value;
        constexpr bool PR = decltype(pair_tag)::value && BP >= 2;
        hipLaunchKernelGGL((k_moment_partials<BP, CV, LM, PR>), grid, dim3(256), sh, ctx->stream, n, B, groups,
                           d_points, d_covs, d_w, d_resp, d_lambda, o[0], o[1], o[2], (double*)scr);
      });
    });
  });
  GC_LAUNCH_CHECK(ctx);
  return gc::launch_bins_finalize(ctx, H, B, NF, chunks, (const double*)scr, eps_psd, eps_mass, d_stats_out,
                                  d_cert_out);
}

}  // extern "C"
