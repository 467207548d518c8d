// gc_mapops.hip — PrimitiveMap maintenance on the device.
//
//  primitive_map_forget                 backend/structures/primitive_map.py:1314-1390
//  primitive_map_recency_inflate        :1400-1490
//  primitive_map_cull                   :1175-1305
//  primitive_map_insert_masked          :807-982 (+ _select_lowest_mass_slots_fixed :325-353)
//  primitive_map_merge_reduce           :1809-2030 (+ _merge_reduce_jax :1501-1807)
//
// One reference tile = the slot range [s0, s0 + n) of the flat device map (gc_map.hip). The
// per-slot work is one thread per slot (HBM-bound streaming of the 176 B core record). Sums are
// per-block partials in slot order reduced by one thread in block order (deterministic; the
// integer counts are exact). Orderings that the reference defines by a stable sort (eviction
// slots, merge candidates) use a stable radix sort on the same key, so ties resolve by index
// exactly as jax.lax.sort / jnp.argsort do. The greedy disjoint-pair selection of merge-reduce is
// inherently sequential and runs on one lane over the sorted candidates, stopping at the first
// distance >= threshold.
//
// There is one kernel family, over a span of tiles with the tile in blockIdx.y (Tiles). A per-tile entry
// launches it on a span of one tile, waits for its counts and decides on the host what runs next.
// gc_primitive_map_maintain (backend/pipeline.py:1412-1447) launches it over all active tiles with no host
// wait: the entries' host decisions are per-tile predicates in device memory, one segmented sort per phase.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <vector>
#include "gc_blocksum.h"
#include "gc_internal.h"
#include "gc_math.h"
#include "gc_mapslot.h"
#include "gc_mapupdate.h"
#include "gc_sort.h"

namespace gc {
namespace {

constexpr int kPartBlocks = 240;  // grid of the reduction passes (<= one wave of workgroups)
constexpr int64_t kMaintainGroupTiles = GC_MAP_MAINTAIN_GROUP_TILES;

struct Tile {
  gc_primitive_map m;
  int64_t s0, n;
};

// What the maintenance kernels run over: tiles of n slots, tile a (blockIdx.y, or the a-th of a group)
// starting at slot s0 + dense[a] * n. A per-tile entry passes its own range as a span of one tile
// (dense = NULL, any s0); the passes over the active tiles pass s0 = 0 and the dense tile list. What the
// per-tile entries decide on the host, those passes read from the device statistics (kStats doubles per
// active tile).
constexpr int kStats = GC_MAP_MAINTAIN_STATS_TILE;
static_assert(kStats == 8, "the statistics row is written by index below");

struct Tiles {
  gc_primitive_map m;
  int64_t s0, n;
  const int32_t* dense;
};
GC_DEV Tile tile_of(const Tiles& S, int64_t a) {
  return Tile{S.m, S.s0 + (S.dense ? (int64_t)S.dense[a] * S.n : 0), S.n};
}
// whether tile a's merge runs; NULL: the caller has decided on the host that it does
GC_DEV bool merge_runs(const double* __restrict__ stats, int64_t a) {
  return !stats || stats[kStats * a + 7] == (double)GC_MAP_MAINTAIN_MERGE_RAN;
}

// Fixed-order block sum of NV per-thread values into part[blockIdx.x * NV + v]. The wave step is the
// butterfly of gc_blocksum.h; the four waves are added pairwise, (w0 + w1) + (w2 + w3), not in
// block_sum's sequential wave order: the maintenance operators have always summed so, and another
// association changes their bits.
template <int NV>
GC_DEV void block_partials(double (&v)[NV], double* part) {
  __shared__ double red[NV][4];
#pragma unroll
  for (int q = 0; q < NV; ++q) {
    const double x = group_sum_xor<64>(v[q]);
    if ((threadIdx.x & 63) == 0) red[q][threadIdx.x >> 6] = x;
  }
  __syncthreads();
  if ((int)threadIdx.x < NV)
    part[blockIdx.x * NV + threadIdx.x] =
        (red[threadIdx.x][0] + red[threadIdx.x][1]) + (red[threadIdx.x][2] + red[threadIdx.x][3]);
}

// the blocks' partials of tile blockIdx.x added in block order by one thread per value: out[a * NV + v]
template <int NV>
__global__ void k_sum_parts(const double* __restrict__ part, int blocks, double* out) {
  if ((int)threadIdx.x >= NV) return;
  const double* p = part + (size_t)blockIdx.x * blocks * NV;
  double s = 0.0;
  for (int b = 0; b < blocks; ++b) s += p[b * NV + threadIdx.x];
  out[blockIdx.x * NV + threadIdx.x] = s;
}

__global__ void k_forget(Tile T, double gamma) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s < T.n) mW(T.m, T.s0 + s) = gamma * mW(T.m, T.s0 + s);
}

GC_DEV double recency_decay(int64_t seq, int64_t last, double lam) {
  const int64_t dt = seq - last > 0 ? seq - last : 0;
  return exp(-lam * (double)dt);
}

// the thread's slots of the tile (block blockIdx.x of gridDim.x, in slot order): Λ, θ *= decay, and its
// terms of [n_valid, Σ(1 - decay), Σ(1/decay - 1)] over valid slots
GC_DEV void recency_slots(const Tile& T, int64_t seq, double lam, double min_scale, double (&acc)[3]) {
  for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < T.n; s += (int64_t)gridDim.x * blockDim.x) {
    const int64_t g = T.s0 + s;
    const bool valid = mValid(T.m, g) != 0;
    double decay = fmin(fmax(recency_decay(seq, mSup(T.m, g), lam), min_scale), 1.0);
    if (!valid) decay = 1.0;
    double* L = mLam(T.m, g);
#pragma unroll
    for (int q = 0; q < 9; ++q) L[q] = L[q] * decay;
#pragma unroll
    for (int q = 0; q < 3; ++q) mTh(T.m, g)[q] = mTh(T.m, g)[q] * decay;
    if (valid) {
      acc[0] += 1.0;
      acc[1] += 1.0 - decay;
      acc[2] += 1.0 / decay - 1.0;
    }
  }
}

// the tile in blockIdx.y; its partials [n_valid, Σ(1 - decay), Σ(1/decay - 1)] over valid slots at
// part + a * gridDim.x * 3
__global__ void __launch_bounds__(256) k_recency(Tiles S, int64_t seq, double lam, double min_scale, double* part) {
  double acc[3] = {0.0, 0.0, 0.0};
  recency_slots(tile_of(S, blockIdx.y), seq, lam, min_scale, acc);
  block_partials<3>(acc, part + (size_t)blockIdx.y * gridDim.x * 3);
}

// one slot's terms of [n_valid, n_below, mass_below, Σ w (all slots)]; returns whether the slot is culled at thr
GC_DEV bool cull_count_slot(const Tile& T, int64_t s, double thr, double (&acc)[4]) {
  const int64_t g = T.s0 + s;
  const double w = mW(T.m, g);
  const bool valid = mValid(T.m, g) != 0;
  const bool below = valid && w < thr;
  acc[0] += valid ? 1.0 : 0.0;
  acc[1] += below ? 1.0 : 0.0;
  acc[2] += w * (below ? 1.0 : 0.0);
  acc[3] += w;
  return below;
}

// The count of the tile in blockIdx.y at its threshold thr_a[a] (NULL: thr0): partials [n_valid, n_below,
// mass_below, Σ w (all slots)] at part + a * gridDim.x * 4. CULL: the slot is also culled in the same visit,
// FORGET: and forgotten (w *= gamma), which no other slot's result depends on. Without FORGET no weight is
// stored.
template <bool CULL, bool FORGET>
__global__ void __launch_bounds__(256) k_cull(Tiles S, double thr0, const double* __restrict__ thr_a, double gamma,
                                              double* part) {
  const Tile T = tile_of(S, blockIdx.y);
  const double thr = thr_a ? thr_a[blockIdx.y] : thr0;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < T.n; s += (int64_t)gridDim.x * blockDim.x) {
    const bool below = cull_count_slot(T, s, thr, acc);
    if (CULL && below) mValid(T.m, T.s0 + s) = 0;
    if (FORGET) mW(T.m, T.s0 + s) = gamma * mW(T.m, T.s0 + s);
  }
  block_partials<4>(acc, part + (size_t)blockIdx.y * gridDim.x * 4);
}

// keys[a * n + s] = w · valid of slot s of the tile in blockIdx.y
__global__ void k_cull_keys(Tiles S, double* keys) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S.n) return;
  const Tile T = tile_of(S, blockIdx.y);
  keys[(int64_t)blockIdx.y * S.n + s] = mW(T.m, T.s0 + s) * (mValid(T.m, T.s0 + s) ? 1.0 : 0.0);
}

__global__ void __launch_bounds__(256) k_count_valid(Tiles S, double* part) {
  const Tile T = tile_of(S, blockIdx.y);
  double acc[1] = {0.0};
  for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < T.n; s += (int64_t)gridDim.x * blockDim.x)
    acc[0] += mValid(T.m, T.s0 + s) ? 1.0 : 0.0;
  block_partials<1>(acc, part + (size_t)blockIdx.y * gridDim.x);
}

// eviction key (_select_lowest_mass_slots_fixed): retention w·exp(-λ dt) on valid slots, -inf on
// empty ones (selected first)
__global__ void k_insert_keys(Tile T, int64_t seq, double lam, double* keys, int32_t* vals) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= T.n) return;
  const int64_t g = T.s0 + s;
  const double ret = mW(T.m, g) * recency_decay(seq, mSup(T.m, g), lam);
  keys[s] = mValid(T.m, g) ? ret : -INFINITY;
  vals[s] = (int32_t)s;
}

// One workgroup: blocked exclusive prefix of the proposal mask (new ids), then each thread
// writes its proposals into their eviction slots.
__global__ void __launch_bounds__(256) k_insert_apply(Tile T, gc_insert_batch B, const int32_t* __restrict__ order,
                                                      double ts, int64_t seq, int64_t next_id0,
                                                      const int64_t* __restrict__ id_offset, int32_t* slots_out,
                                                      int64_t* ids_out, double* n_ins_out) {
  __shared__ int64_t scan[256];
  // ids run on from next_id0, plus a count still on the device (gc_primitive_map_update: the
  // proposals inserted into earlier tiles of the same call)
  const int64_t next_id = next_id0 + (id_offset ? *id_offset : 0);
  const int t = threadIdx.x;
  const int64_t per = (B.K + 255) / 256;
  const int64_t k0 = t * per, k1 = k0 + per < B.K ? k0 + per : B.K;
  int64_t cnt = 0;
  for (int64_t k = k0; k < k1; ++k) cnt += B.valid_mask[k] ? 1 : 0;
  scan[t] = cnt;
  __syncthreads();
  for (int off = 1; off < 256; off <<= 1) {  // inclusive Hillis-Steele over the 256 chunk counts
    const int64_t v = t >= off ? scan[t - off] : 0;
    __syncthreads();
    scan[t] += v;
    __syncthreads();
  }
  int64_t run = scan[t] - cnt;
  const int L = T.m.n_lobes;
  const bool color = T.m.cam_mass != nullptr;
  for (int64_t k = k0; k < k1; ++k) {
    const int32_t slot = order[k];
    const bool ins = B.valid_mask[k] != 0;
    if (slots_out) slots_out[k] = slot;
    if (ids_out) ids_out[k] = ins ? next_id + run : -1;
    if (!ins) continue;
    const int64_t g = T.s0 + slot;
    for (int q = 0; q < 9; ++q) mLam(T.m, g)[q] = B.Lambdas[9 * k + q];
    for (int q = 0; q < 3; ++q) mTh(T.m, g)[q] = B.thetas[3 * k + q];
    for (int q = 0; q < 3 * L; ++q) mEta(T.m, g)[q] = B.etas[(int64_t)3 * L * k + q];
    const double w = B.weights[k];
    mW(T.m, g) = w;
    mTs(T.m, g) = ts;
    if (T.m.created_timestamps) mCreated(T.m, g) = ts;
    mSup(T.m, g) = seq;
    mUpd(T.m, g) = seq;
    if (T.m.primitive_ids) mPid(T.m, g) = next_id + run;
    mValid(T.m, g) = 1;
    if (color) {
      const int src = B.sources ? B.sources[k] : 1;
      const double cam = w * (src == 0 ? 1.0 : 0.0), lid = w * (src == 1 ? 1.0 : 0.0);
      mCam(T.m, g) = cam;
      mLid(T.m, g) = lid;
      mDen(T.m, g) = cam;
      for (int q = 0; q < 3; ++q) {
        const double c = B.colors ? B.colors[3 * k + q] : 0.0;
        const double rgb = cam > 0.0 ? clampd(c, 0.0, 1.0) : 0.5;
        mAcc(T.m, g)[q] = c * cam;
        mRgb(T.m, g)[q] = rgb;
        if (T.m.colors) mCol(T.m, g)[q] = rgb;
      }
    }
    ++run;
  }
  if (t == 255) *n_ins_out = (double)scan[255];
}

// ---- merge-reduce
// μ = solve(Λ + εI, θ), Σ = inv(Λ + εI), det Σ (primitive_map.py:1908-1911)
GC_DEV void merge_prep_slot(const Tile& T, int64_t s, double eps_lift, double* mu, double* Sig, double* dets) {
  const int64_t g = T.s0 + s;
  double Lr[9];
  lifted3(mLam(T.m, g), eps_lift, Lr);
  solve3(Lr, mTh(T.m, g), mu + 3 * s);
  inv3(Lr, Sig + 9 * s);
  dets[s] = det3(Sig + 9 * s);
}

// The merge kernels run on the tiles a0 .. a0 + g - 1 of the span, the tile of the group in blockIdx.y (one
// workgroup per tile for the select); mu / Sig / dets / used hold n slots per tile of the group, keys / vals
// P pairs, sel max_pairs pairs, n_sel one count per tile of the span.
__global__ void k_merge_prep(Tiles S, int64_t a0, const double* __restrict__ stats, double eps_lift, double* mu,
                             double* Sig, double* dets) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, la = blockIdx.y;
  if (s >= S.n || !merge_runs(stats, a0 + la)) return;
  merge_prep_slot(tile_of(S, a0 + la), s, eps_lift, mu + 3 * la * S.n, Sig + 9 * la * S.n, dets + la * S.n);
}

// pair p of jnp.triu_indices(n, k=1) (row-major, i < j)
GC_DEV void triu_pair(int64_t n, int64_t p, int64_t* i, int64_t* j) {
  const double b = 2.0 * (double)n - 1.0;
  int64_t r = (int64_t)floor((b - sqrt(b * b - 8.0 * (double)p)) * 0.5);
  if (r < 0) r = 0;
  auto off = [n](int64_t x) { return x * (2 * n - x - 1) / 2; };
  while (r > 0 && off(r) > p) --r;
  while (off(r + 1) <= p) ++r;
  *i = r;
  *j = p - off(r) + r + 1;
}

// Bhattacharyya distance of pair p (primitive_map.py:1921-1930), +inf unless both slots are valid
GC_DEV double merge_pair_dist(const Tile& T, int64_t p, const double* __restrict__ mu, const double* __restrict__ Sig,
                              const double* __restrict__ dets, double eps_lift) {
  int64_t i, j;
  triu_pair(T.n, p, &i, &j);
  double S[9], Sr[9], Si[9];
  for (int q = 0; q < 9; ++q) S[q] = 0.5 * (Sig[9 * i + q] + Sig[9 * j + q]);
  const double detS = det3(S);
  for (int q = 0; q < 9; ++q) Sr[q] = S[q] + ((q % 4 == 0) ? eps_lift : 0.0);
  inv3(Sr, Si);
  const double dm[3] = {mu[3 * i] - mu[3 * j], mu[3 * i + 1] - mu[3 * j + 1], mu[3 * i + 2] - mu[3 * j + 2]};
  double rv[3];
  mat3_tvec(Si, dm, rv);  // dmuᵀ S⁻¹
  const double quad = 0.125 * dot3(rv, dm);
  const double logt = 0.5 * log(detS / sqrt(dets[i] * dets[j] + 1e-24));
  const bool pv = mValid(T.m, T.s0 + i) && mValid(T.m, T.s0 + j);
  return pv ? quad + logt : INFINITY;
}

__global__ void k_merge_dist(Tiles S, int64_t a0, int64_t P, const double* __restrict__ stats,
                             const double* __restrict__ mu, const double* __restrict__ Sig,
                             const double* __restrict__ dets, double eps_lift, double* keys, uint32_t* vals) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, la = blockIdx.y;
  if (p >= P) return;
  const int64_t x = la * P + p;
  vals[x] = (uint32_t)p;
  keys[x] = merge_runs(stats, a0 + la) ? merge_pair_dist(tile_of(S, a0 + la), p, mu + 3 * la * S.n,
                                                         Sig + 9 * la * S.n, dets + la * S.n, eps_lift)
                                       : INFINITY;
}

// greedy disjoint selection over the sorted candidates (_merge_reduce_jax select_body), one lane
GC_DEV int merge_select_walk(int64_t n, int64_t P, const double* __restrict__ keys, const uint32_t* __restrict__ vals,
                             double thr, int max_pairs, uint8_t* used, int32_t* sel) {
  int ns = 0;
  for (int64_t k = 0; k < P && ns < max_pairs; ++k) {
    const double d = keys[k];
    if (d == INFINITY) break;   // the tail: +inf (invalid pairs), then NaN
    if (!isfinite(d)) continue;  // -inf / NaN: never selectable (jnp.isfinite)
    if (!(d < thr)) break;       // ascending: nothing later qualifies
    int64_t i, j;
    triu_pair(n, vals[k], &i, &j);
    if (used[i] || used[j]) continue;
    used[i] = 1;
    used[j] = 1;
    sel[2 * ns] = (int32_t)i;
    sel[2 * ns + 1] = (int32_t)j;
    ++ns;
  }
  return ns;
}

__global__ void k_merge_select(int64_t n, int64_t a0, int64_t P, const double* __restrict__ stats,
                               const double* __restrict__ keys, const uint32_t* __restrict__ vals, double thr,
                               int max_pairs, uint8_t* used, int32_t* sel, int32_t* n_sel) {
  const int64_t la = blockIdx.x;
  if (threadIdx.x != 0 || !merge_runs(stats, a0 + la)) return;
  n_sel[a0 + la] = merge_select_walk(n, P, keys + la * P, vals + la * P, thr, max_pairs, used + la * n,
                                     sel + la * 2 * max_pairs);
}

// moment-matched merge of the pair (i, j) into slot i (_merge_reduce_jax merge_body)
GC_DEV void merge_apply_pair(const Tile& T, const double* __restrict__ mu, const double* __restrict__ Sig, int64_t i,
                             int64_t j, double eps_psd) {
  const int64_t gi = T.s0 + i, gj = T.s0 + j;
  const double w1 = mW(T.m, gi), w2 = mW(T.m, gj), ws = w1 + w2;
  if (!(ws > 0.0)) return;
  const double* m1 = mu + 3 * i;
  const double* m2 = mu + 3 * j;
  double mm[3], d1[3], d2[3], Sm[9], Lm[9], th[3];
  for (int q = 0; q < 3; ++q) mm[q] = (w1 * m1[q] + w2 * m2[q]) / ws;
  for (int q = 0; q < 3; ++q) { d1[q] = m1[q] - mm[q]; d2[q] = m2[q] - mm[q]; }
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) {
      const int q = 3 * r + c;
      Sm[q] = (w1 * (Sig[9 * i + q] + d1[r] * d1[c]) + w2 * (Sig[9 * j + q] + d2[r] * d2[c])) / ws +
              (r == c ? eps_psd : 0.0);
    }
  inv3(Sm, Lm);
  mat3_vec(Lm, mm, th);
  for (int q = 0; q < 9; ++q) mLam(T.m, gi)[q] = Lm[q];
  for (int q = 0; q < 3; ++q) mTh(T.m, gi)[q] = th[q];
  const int L = T.m.n_lobes;
  double* ei = mEta(T.m, gi);
  const double* ej = mEta(T.m, gj);
  for (int q = 0; q < 3 * L; ++q) ei[q] = (w1 * ei[q] + w2 * ej[q]) / ws;
  mW(T.m, gi) = ws;
  if (T.m.cam_mass) {
    const double cm = mCam(T.m, gi) + mCam(T.m, gj);
    const double den = mDen(T.m, gi) + mDen(T.m, gj);
    mCam(T.m, gi) = cm;
    mLid(T.m, gi) = mLid(T.m, gi) + mLid(T.m, gj);
    mDen(T.m, gi) = den;
    double acc[3];
    for (int q = 0; q < 3; ++q) mAcc(T.m, gi)[q] = acc[q] = mAcc(T.m, gi)[q] + mAcc(T.m, gj)[q];
    slot_colour(T.m, gi, cm, acc, den, eps_psd);
  }
  mTs(T.m, gi) = fmax(mTs(T.m, gi), mTs(T.m, gj));
  if (T.m.created_timestamps) mCreated(T.m, gi) = fmin(mCreated(T.m, gi), mCreated(T.m, gj));
  const int64_t ls = mSup(T.m, gj), lu = mUpd(T.m, gj);
  if (ls > mSup(T.m, gi)) mSup(T.m, gi) = ls;
  if (lu > mUpd(T.m, gi)) mUpd(T.m, gi) = lu;
  mW(T.m, gj) = 0.0;
  mValid(T.m, gj) = 0;
}

// each selected (disjoint) pair of the tile
__global__ void k_merge_apply(Tiles S, int64_t a0, const double* __restrict__ mu, const double* __restrict__ Sig,
                              const int32_t* __restrict__ sel, const int32_t* __restrict__ n_sel, double eps_psd,
                              int max_pairs) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t la = blockIdx.y;
  if (k >= max_pairs || k >= n_sel[a0 + la]) return;
  const int32_t* sl = sel + la * 2 * max_pairs;
  merge_apply_pair(tile_of(S, a0 + la), mu + 3 * la * S.n, Sig + 9 * la * S.n, sl[2 * k], sl[2 * k + 1], eps_psd);
}

// ---- the per-tile decisions of gc_primitive_map_maintain, one thread per active tile
// primitive_map.py:1222-1229 per tile: sums = the count at thr0, keys = the tile's w·valid descending
__global__ void k_tiles_cull_thr(int n_active, int64_t n, const double* __restrict__ sums,
                                 const double* __restrict__ keys, double thr0, int64_t max_primitives, double* thr_a) {
  const int a = blockIdx.x * blockDim.x + threadIdx.x;
  if (a >= n_active) return;
  const double* c = sums + 4 * a;
  const bool top = c[0] - c[1] > (double)max_primitives && max_primitives < n;
  thr_a[a] = top ? keys[(int64_t)a * n + max_primitives] : thr0;
}

// the cull's statistics and the merge's no-op tests (primitive_map.py:1879-1890), the valid count after the cull
__global__ void k_tiles_cull_stats(int n_active, int64_t n, const double* __restrict__ sums,
                                const double* __restrict__ thr_a, double thr0, int max_pairs, int capped,
                                double* stats) {
  const int a = blockIdx.x * blockDim.x + threadIdx.x;
  if (a >= n_active) return;
  const double* c = sums + 4 * a;
  double* st = stats + kStats * a;
  const double after = c[0] - c[1];
  st[0] = c[0];
  st[1] = c[1];
  st[2] = c[1] > 0.0 ? c[2] : 0.0;
  st[3] = c[3];
  st[4] = thr_a ? thr_a[a] : thr0;
  st[5] = 0.0;
  st[6] = after;
  st[7] = (n < 2 || after < 2.0 || max_pairs <= 0) ? (double)GC_MAP_MAINTAIN_MERGE_NOOP
          : capped                                  ? (double)GC_MAP_MAINTAIN_MERGE_CAPPED
                                                    : (double)GC_MAP_MAINTAIN_MERGE_RAN;
}

__global__ void k_tiles_merge_stats(int n_active, const double* __restrict__ part, int blocks,
                                 const int32_t* __restrict__ n_sel, double* stats) {
  const int a = blockIdx.x * blockDim.x + threadIdx.x;
  if (a >= n_active) return;
  double s = 0.0;
  for (int b = 0; b < blocks; ++b) s += part[(size_t)a * blocks + b];
  stats[kStats * a + 5] = (double)n_sel[a];
  stats[kStats * a + 6] = s;
}

unsigned blocks_for(int64_t n) { return (unsigned)((n + 255) / 256); }
unsigned part_blocks(int64_t n) {
  const int64_t b = (n + 255) / 256;
  return (unsigned)(b < kPartBlocks ? (b > 0 ? b : 1) : kPartBlocks);
}

// reduction pass over n_tiles tiles of n slots: launch(grid) writes part_blocks(n) x NV partials per tile into
// part, then the fixed-order finish into out[a * NV + v] (device)
template <int NV, typename Launch>
int reduce_into(gc_ctx* ctx, int64_t n, int64_t n_tiles, double* part, double* out, Launch launch) {
  const unsigned nb = part_blocks(n);
  launch(dim3(nb, (unsigned)n_tiles));
  GC_LAUNCH_CHECK(ctx);
  hipLaunchKernelGGL(k_sum_parts<NV>, dim3((unsigned)n_tiles), dim3(64), 0, ctx->stream, (const double*)part, (int)nb,
                     out);
  GC_LAUNCH_CHECK(ctx);
  return GC_OK;
}

// radix_sort_pairs on the context's stream, a failure reported as the context's error
int sort_pairs(gc_ctx* ctx, const double* keys_in, double* keys_out, const uint32_t* vals_in, uint32_t* vals_out,
               int64_t n_seg, int64_t len, bool descending, void* tmp) {
  if (gc::radix_sort_pairs(ctx->stream, keys_in, keys_out, vals_in, vals_out, n_seg, len, descending, tmp) !=
      hipSuccess) {
    gc::set_error(ctx, "radix sort failed");
    return GC_ERR_RUNTIME;
  }
  return GC_OK;
}

// scratch of a merge over a group of G tiles of n slots (P pairs each); n_sel is the caller's
struct MergeScratch {
  double *mu, *Sig, *dets, *keys_in, *keys;
  uint32_t *vals_in, *vals;
  uint8_t* used;
  int32_t* sel;
  void* tmp;
};
MergeScratch merge_layout(Carver& c, int64_t G, int64_t n, int64_t P, int max_pairs) {
  MergeScratch s;
  s.mu = c.take<double>(3 * (size_t)(G * n));
  s.Sig = c.take<double>(9 * (size_t)(G * n));
  s.dets = c.take<double>((size_t)(G * n));
  s.keys_in = c.take<double>((size_t)(G * P));
  s.keys = c.take<double>((size_t)(G * P));
  s.vals_in = c.take<uint32_t>((size_t)(G * P));
  s.vals = c.take<uint32_t>((size_t)(G * P));
  s.used = c.take<uint8_t>((size_t)(G * n));
  s.sel = c.take<int32_t>(2 * (size_t)G * (size_t)std::max(max_pairs, 1));
  s.tmp = c.take<char>(P > 0 ? gc::sort_temp_bytes(G, P, true) : 0);
  return s;
}

// The merge-reduce of the g tiles a0 .. a0 + g - 1 of the span (n >= 2 slots each, max_pairs >= 1), no host
// wait: distances, one segmented sort, the greedy selection and the merges; n_sel[a] = the pairs merged in
// tile a (written only where the merge runs, merge_runs).
int merge_group(gc_ctx* ctx, const Tiles& S, int64_t a0, int64_t g, const double* d_stats, const MergeScratch& s,
                double merge_thr, int max_pairs, double eps_psd, double eps_lift, int32_t* n_sel) {
  const int64_t P = S.n * (S.n - 1) / 2;
  GC_HIP(ctx, hipMemsetAsync(s.used, 0, (size_t)(g * S.n), ctx->stream));
  hipLaunchKernelGGL(k_merge_prep, dim3(blocks_for(S.n), (unsigned)g), dim3(256), 0, ctx->stream, S, a0, d_stats,
                     eps_lift, s.mu, s.Sig, s.dets);
  GC_LAUNCH_CHECK(ctx);
  hipLaunchKernelGGL(k_merge_dist, dim3(blocks_for(P), (unsigned)g), dim3(256), 0, ctx->stream, S, a0, P, d_stats,
                     (const double*)s.mu, (const double*)s.Sig, (const double*)s.dets, eps_lift, s.keys_in, s.vals_in);
  GC_LAUNCH_CHECK(ctx);
  if (int rc = sort_pairs(ctx, s.keys_in, s.keys, s.vals_in, s.vals, g, P, false, s.tmp)) return rc;
  hipLaunchKernelGGL(k_merge_select, dim3((unsigned)g), dim3(64), 0, ctx->stream, S.n, a0, P, d_stats,
                     (const double*)s.keys, (const uint32_t*)s.vals, merge_thr, max_pairs, s.used, s.sel, n_sel);
  GC_LAUNCH_CHECK(ctx);
  hipLaunchKernelGGL(k_merge_apply, dim3((unsigned)((max_pairs + 255) / 256), (unsigned)g), dim3(256), 0, ctx->stream,
                     S, a0, (const double*)s.mu, (const double*)s.Sig, (const int32_t*)s.sel, (const int32_t*)n_sel,
                     eps_psd, max_pairs);
  GC_LAUNCH_CHECK(ctx);
  return GC_OK;
}

int download(gc_ctx* ctx, void* h, const void* d, size_t bytes) {
  GC_HIP(ctx, hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, ctx->stream));
  if (int rc_w = gc::wait_stream(ctx, ctx->stream, "a result download")) return rc_w;
  return GC_OK;
}

// scratch of insert_launch on a tile of n_slots: the reduction partials with the two results behind them
// (part + kPartBlocks), the retention keys and slot numbers before and after the sort, and the sort's own
struct InsertScratch {
  double *part, *keys_in, *keys;
  int32_t *vals_in, *vals;
  void* tmp;
};
InsertScratch insert_layout(Carver& c, int64_t n_slots) {
  InsertScratch s;
  s.part = c.take<double>(kPartBlocks + 16);
  s.keys_in = c.take<double>(n_slots);
  s.keys = c.take<double>(n_slots);
  s.vals_in = c.take<int32_t>(n_slots);
  s.vals = c.take<int32_t>(n_slots);
  s.tmp = c.take<char>(gc::sort_temp_bytes(1, n_slots, true));
  return s;
}

// the checks of a pass over a list of tiles (gc_primitive_map_maintain, gc_primitive_map_recency_inflate_tiles),
// after check_tile: m_tile divides the map, the host list holds n_active distinct dense tiles of the map
int check_active_tiles(gc_ctx* ctx, const gc_primitive_map* map, int64_t m_tile, int32_t n_active,
                       const int32_t* d_active_dense, const int32_t* h_active_dense) {
  GC_CHECK_ARG(ctx, m_tile > 0 && map->m_slots % m_tile == 0, "m_tile must be > 0 and divide the map's slots");
  GC_CHECK_ARG(ctx, n_active >= 0 && n_active <= 65535, "n_active must be in [0, 65535]");
  if (n_active == 0) return GC_OK;
  GC_CHECK_ARG(ctx, d_active_dense && h_active_dense, "NULL argument");
  const int64_t n_tiles = map->m_slots / m_tile;
  GC_CHECK_ARG(ctx, n_active <= n_tiles, "more active tiles than the map holds");
  std::vector<uint8_t> seen((size_t)n_tiles, 0);
  for (int a = 0; a < n_active; ++a) {
    const int64_t d = h_active_dense[a];
    GC_CHECK_ARG(ctx, d >= 0 && d < n_tiles, "active dense tile outside the map");
    GC_CHECK_ARG(ctx, !seen[(size_t)d], "duplicate active tile");
    seen[(size_t)d] = 1;
  }
  return GC_OK;
}

}  // namespace

int check_map_core(gc_ctx* ctx, const gc_primitive_map* map, int64_t max_slots, bool need_valid) {
  GC_CHECK_ARG(ctx, map->m_slots > 0 && map->m_slots < max_slots, "m_slots out of range");
  GC_CHECK_ARG(ctx, map->n_lobes >= 1 && map->n_lobes <= kMapMaxLobes, "n_lobes must be in [1, 8]");
  {
    const char* lay_ = gc::map_layout_error(*map);
    GC_CHECK_ARG(ctx, lay_ == nullptr, lay_ ? lay_ : "");
  }
  GC_CHECK_ARG(ctx, map->Lambdas && map->thetas && map->etas && map->weights && map->timestamps &&
                        map->last_supported_scan_seq && map->last_update_scan_seq,
               "NULL map field");
  GC_CHECK_ARG(ctx, !need_valid || map->valid_mask, "valid_mask is required");
  return GC_OK;
}

int check_map(gc_ctx* ctx, const gc_primitive_map* map, int64_t max_slots, bool need_valid) {
  if (int rc = check_map_core(ctx, map, max_slots, need_valid)) return rc;
  const bool color = map->cam_mass != nullptr;
  GC_CHECK_ARG(ctx, !color || (map->lidar_mass && map->rgb_cam_accum && map->rgb_cam_denom && map->rgb),
               "colour fields must be all set or all NULL");
  return GC_OK;
}

int check_tile(gc_ctx* ctx, const gc_primitive_map* map, int64_t slot0, int64_t n_slots, bool need_valid) {
  GC_CHECK_ARG(nullptr, ctx != nullptr, "ctx is NULL");
  if (int rc_j = gc::join_side(ctx)) return rc_j;  // a pipeline's in-scan update may still write the map
  GC_CHECK_ARG(ctx, map != nullptr, "NULL map");
  GC_CHECK_ARG(ctx, map->m_slots > 0 && slot0 >= 0 && n_slots >= 0 && slot0 + n_slots <= map->m_slots,
               "tile range outside the map");
  return check_map(ctx, map, INT64_MAX, need_valid);
}

size_t insert_scratch_bytes(int64_t n_slots) {
  Carver c;
  insert_layout(c, n_slots);
  return c.bytes;
}

// The launches of gc_primitive_map_insert_masked on validated arguments (no host wait): scr holds
// insert_scratch_bytes(n_slots); d_out2 (device) = [valid count of the tile after, n_inserted].
// d_id_offset (device, or NULL) is added to next_global_id.
int insert_launch(gc_ctx* ctx, const gc_primitive_map* map, int64_t slot0, int64_t n_slots,
                  const gc_insert_batch* batch, double timestamp, int64_t scan_seq, double recency_decay_lambda,
                  int64_t next_global_id, const int64_t* d_id_offset, int32_t* d_target_slots_out,
                  int64_t* d_new_ids_out, void* scr, double* d_out2) {
  Carver carve{(char*)scr};
  const InsertScratch s = insert_layout(carve, n_slots);
  const Tile T{*map, slot0, n_slots};
  hipLaunchKernelGGL(k_insert_keys, dim3(blocks_for(n_slots)), dim3(256), 0, ctx->stream, T, scan_seq,
                     recency_decay_lambda, s.keys_in, s.vals_in);
  GC_LAUNCH_CHECK(ctx);
  if (int rc = sort_pairs(ctx, s.keys_in, s.keys, (const uint32_t*)s.vals_in, (uint32_t*)s.vals, 1, n_slots, false,
                          s.tmp))
    return rc;
  hipLaunchKernelGGL(k_insert_apply, dim3(1), dim3(256), 0, ctx->stream, T, *batch, (const int32_t*)s.vals, timestamp,
                     scan_seq, next_global_id, d_id_offset, d_target_slots_out, d_new_ids_out, d_out2 + 1);
  GC_LAUNCH_CHECK(ctx);
  return reduce_into<1>(ctx, n_slots, 1, s.part, d_out2, [&](dim3 grid) {
    hipLaunchKernelGGL(k_count_valid, grid, dim3(256), 0, ctx->stream, Tiles{*map, slot0, n_slots, nullptr}, s.part);
  });
}
}  // namespace gc

using namespace gc;

extern "C" {

int32_t gc_primitive_map_forget(gc_ctx* ctx, const gc_primitive_map* map, int64_t slot0, int64_t n_slots,
                                double gamma) {
  if (int rc = check_tile(ctx, map, slot0, n_slots, false)) return rc;
  if (n_slots == 0) return GC_OK;
  hipLaunchKernelGGL(k_forget, dim3(blocks_for(n_slots)), dim3(256), 0, ctx->stream, Tile{*map, slot0, n_slots},
                     gamma);
  GC_LAUNCH_CHECK(ctx);
  return GC_OK;
}

int32_t gc_primitive_map_recency_inflate(gc_ctx* ctx, const gc_primitive_map* map, int64_t slot0, int64_t n_slots,
                                         int64_t scan_seq, double decay_lambda, double min_scale,
                                         double* h_stats3) {
  if (int rc = check_tile(ctx, map, slot0, n_slots, true)) return rc;
  if (h_stats3) h_stats3[0] = h_stats3[1] = h_stats3[2] = 0.0;
  if (n_slots == 0) return GC_OK;
  double *part, *out;
  if (int rc = gc::carve_scratch(ctx, [&](gc::Carver& c) {
        part = c.take<double>(3 * kPartBlocks);
        out = c.take<double>(3);
      }))
    return rc;
  const Tiles S{*map, slot0, n_slots, nullptr};
  if (int rc = reduce_into<3>(ctx, n_slots, 1, part, out, [&](dim3 grid) {
        hipLaunchKernelGGL(k_recency, grid, dim3(256), 0, ctx->stream, S, scan_seq, decay_lambda, min_scale, part);
      }))
    return rc;
  return h_stats3 ? download(ctx, h_stats3, out, 3 * sizeof(double)) : GC_OK;
}

int32_t gc_primitive_map_recency_inflate_tiles(gc_ctx* ctx, const gc_primitive_map* map, int64_t m_tile,
                                               int32_t n_active, const int32_t* d_active_dense,
                                               const int32_t* h_active_dense, int64_t scan_seq, double decay_lambda,
                                               double min_scale, double* d_stats) {
  if (int rc = check_tile(ctx, map, 0, 0, true)) return rc;  // joins the side stream first
  if (int rc = check_active_tiles(ctx, map, m_tile, n_active, d_active_dense, h_active_dense)) return rc;
  if (n_active == 0) return GC_OK;
  GC_CHECK_ARG(ctx, d_stats != nullptr, "d_stats is NULL");
  double* part;
  if (int rc = gc::carve_scratch(
          ctx, [&](gc::Carver& c) { part = c.take<double>(3 * (size_t)part_blocks(m_tile) * n_active); }))
    return rc;
  const Tiles S{*map, 0, m_tile, d_active_dense};
  return reduce_into<3>(ctx, m_tile, n_active, part, d_stats, [&](dim3 grid) {
    hipLaunchKernelGGL(k_recency, grid, dim3(256), 0, ctx->stream, S, scan_seq, decay_lambda, min_scale, part);
  });
}

int32_t gc_test_radix_sort(gc_ctx* ctx, const double* d_keys_in, const uint32_t* d_vals_in, int64_t n_seg, int64_t L,
                           int32_t descending, double* d_keys_out, uint32_t* d_vals_out) {
  GC_CHECK_ARG(nullptr, ctx != nullptr, "ctx is NULL");
  GC_CHECK_ARG(ctx, n_seg >= 0 && L >= 0 && n_seg * L < ((int64_t)1 << 32), "n_seg * L must be in [0, 2^32)");
  GC_CHECK_ARG(ctx, n_seg * L == 0 || (d_keys_in && d_keys_out), "NULL key buffer");
  GC_CHECK_ARG(ctx, !d_vals_in || d_vals_out, "NULL value output");
  if (n_seg * L == 0) return GC_OK;
  void* scr;
  if (int rc = gc::scratch(ctx, gc::sort_temp_bytes(n_seg, L, d_vals_in != nullptr), &scr)) return rc;
  GC_HIP(ctx, gc::radix_sort_pairs(ctx->stream, d_keys_in, d_keys_out, d_vals_in, d_vals_out, n_seg, L, descending != 0,
                                   scr));
  return GC_OK;
}

int32_t gc_primitive_map_cull(gc_ctx* ctx, const gc_primitive_map* map, int64_t slot0, int64_t n_slots,
                              double weight_threshold, int64_t max_primitives, double* h_out4) {
  if (int rc = check_tile(ctx, map, slot0, n_slots, true)) return rc;
  GC_CHECK_ARG(ctx, h_out4 != nullptr, "h_out4 is NULL");
  for (int q = 0; q < 4; ++q) h_out4[q] = 0.0;
  if (n_slots == 0) return GC_OK;
  double *part, *out, *keys_in, *keys;
  void* tmp;
  if (int rc = gc::carve_scratch(ctx, [&](gc::Carver& c) {
        part = c.take<double>(4 * kPartBlocks);
        out = c.take<double>(4);
        keys_in = c.take<double>(n_slots);
        keys = c.take<double>(n_slots);
        tmp = c.take<char>(gc::sort_temp_bytes(1, n_slots, false));
      }))
    return rc;
  const Tiles S{*map, slot0, n_slots, nullptr};
  const double* no_thr = nullptr;
  auto count = [&](double thr, double* h4) -> int {
    if (int rc = reduce_into<4>(ctx, n_slots, 1, part, out, [&](dim3 grid) {
          hipLaunchKernelGGL((k_cull<false, false>), grid, dim3(256), 0, ctx->stream, S, thr, no_thr, 1.0, part);
        }))
      return rc;
    return download(ctx, h4, out, 4 * sizeof(double));
  };
  double c[4];
  if (int rc = count(weight_threshold, c)) return rc;
  const double n_valid = c[0];
  double thr = weight_threshold;
  // primitive_map.py:1222-1229: keep the top max_primitives by weight
  if (max_primitives >= 0 && n_valid - c[1] > (double)max_primitives && max_primitives < n_slots) {
    hipLaunchKernelGGL(k_cull_keys, dim3(blocks_for(n_slots), 1), dim3(256), 0, ctx->stream, S, keys_in);
    GC_LAUNCH_CHECK(ctx);
    if (int rc = sort_pairs(ctx, keys_in, keys, nullptr, nullptr, 1, n_slots, true, tmp)) return rc;
    if (int rc = download(ctx, &thr, keys + max_primitives, sizeof(double))) return rc;
    if (int rc = count(thr, c)) return rc;
  }
  if (c[1] > 0.0) {  // the cull alone (the forgetting is gc_primitive_map_forget's); its recount in part is not read
    hipLaunchKernelGGL((k_cull<true, false>), dim3(part_blocks(n_slots), 1), dim3(256), 0, ctx->stream, S, thr, no_thr,
                       1.0, part);
    GC_LAUNCH_CHECK(ctx);
  }
  h_out4[0] = c[1];
  h_out4[1] = c[1] > 0.0 ? c[2] : 0.0;
  h_out4[2] = c[3];
  h_out4[3] = n_valid;
  return GC_OK;
}

int32_t gc_primitive_map_insert_masked(gc_ctx* ctx, const gc_primitive_map* map, int64_t slot0, int64_t n_slots,
                                       const gc_insert_batch* batch, double timestamp, int64_t scan_seq,
                                       double recency_decay_lambda, int64_t next_global_id,
                                       int32_t* d_target_slots_out, int64_t* d_new_ids_out, int64_t* h_out2) {
  if (int rc = check_tile(ctx, map, slot0, n_slots, true)) return rc;
  GC_CHECK_ARG(ctx, batch && h_out2, "NULL batch or h_out2");
  GC_CHECK_ARG(ctx, batch->K >= 1 && batch->K <= n_slots, "K must be in [1, n_slots]");
  GC_CHECK_ARG(ctx, n_slots < (int64_t)INT32_MAX, "tile too large");
  GC_CHECK_ARG(ctx, batch->Lambdas && batch->thetas && batch->etas && batch->weights && batch->valid_mask,
               "NULL proposal field");
  void* scr;
  if (int rc = gc::scratch(ctx, gc::insert_scratch_bytes(n_slots), &scr)) return rc;
  gc::Carver carve{(char*)scr};
  double* out = insert_layout(carve, n_slots).part + kPartBlocks;  // [count_after, n_inserted]
  if (int rc = gc::insert_launch(ctx, map, slot0, n_slots, batch, timestamp, scan_seq, recency_decay_lambda,
                                 next_global_id, nullptr, d_target_slots_out, d_new_ids_out, scr, out))
    return rc;
  double counts[2];
  if (int rc = download(ctx, counts, out, sizeof(counts))) return rc;
  h_out2[0] = (int64_t)counts[1];
  h_out2[1] = (int64_t)counts[0];
  return GC_OK;
}

int32_t gc_primitive_map_merge_reduce(gc_ctx* ctx, const gc_primitive_map* map, int64_t slot0, int64_t n_slots,
                                      double merge_threshold, int32_t max_pairs, double eps_psd, double eps_lift,
                                      int64_t* h_out2) {
  if (int rc = check_tile(ctx, map, slot0, n_slots, true)) return rc;
  GC_CHECK_ARG(ctx, h_out2 != nullptr, "h_out2 is NULL");
  GC_CHECK_ARG(ctx, n_slots <= 65536, "merge-reduce tile larger than 65536 slots");
  h_out2[0] = 0;
  h_out2[1] = 0;
  const Tiles S{*map, slot0, n_slots, nullptr};
  const int64_t P = n_slots * (n_slots - 1) / 2;
  double *part, *out;
  int32_t* n_sel;
  MergeScratch mg;
  if (int rc = gc::carve_scratch(ctx, [&](gc::Carver& c) {
        part = c.take<double>(kPartBlocks);
        out = c.take<double>(1);
        n_sel = c.take<int32_t>(1);
        mg = merge_layout(c, 1, n_slots, P, max_pairs);
      }))
    return rc;
  auto count_valid = [&](double* h) -> int {
    if (int rc = reduce_into<1>(ctx, n_slots, 1, part, out, [&](dim3 grid) {
          hipLaunchKernelGGL(k_count_valid, grid, dim3(256), 0, ctx->stream, S, part);
        }))
      return rc;
    return download(ctx, h, out, sizeof(double));
  };
  double nv = 0.0;
  if (n_slots > 0)
    if (int rc = count_valid(&nv)) return rc;
  h_out2[1] = (int64_t)nv;
  if (n_slots < 2 || nv < 2.0 || max_pairs <= 0) return GC_OK;  // primitive_map.py:1879-1880
  // decided here on the host: no statistics row, the merge runs
  if (int rc = merge_group(ctx, S, 0, 1, nullptr, mg, merge_threshold, (int)max_pairs, eps_psd, eps_lift, n_sel))
    return rc;
  int32_t ns = 0;
  if (int rc = download(ctx, &ns, n_sel, sizeof(ns))) return rc;
  if (int rc = count_valid(&nv)) return rc;
  h_out2[0] = ns;
  h_out2[1] = (int64_t)nv;
  return GC_OK;
}

int32_t gc_primitive_map_maintain(gc_ctx* ctx, const gc_primitive_map* map, int64_t m_tile, int32_t n_active,
                                  const int32_t* d_active_dense, const int32_t* h_active_dense,
                                  const gc_map_maintain_cfg* cfg, int64_t max_primitives, int32_t max_pairs,
                                  int64_t max_tile_size, int64_t max_sort_keys, double* d_stats) {
  if (int rc = check_tile(ctx, map, 0, 0, true)) return rc;  // joins the side stream first
  if (int rc = check_active_tiles(ctx, map, m_tile, n_active, d_active_dense, h_active_dense)) return rc;
  if (n_active == 0) return GC_OK;
  GC_CHECK_ARG(ctx, cfg && d_stats, "NULL argument");
  GC_CHECK_ARG(ctx, max_sort_keys >= 0, "max_sort_keys must be >= 0");
  const double thr0 = cfg->primitive_cull_weight_threshold, gamma = cfg->primitive_forgetting_factor,
               merge_thr = cfg->primitive_merge_threshold, eps_psd = cfg->eps_psd, eps_lift = cfg->eps_lift;
  const bool top = max_primitives >= 0;
  const int64_t slots = (int64_t)n_active * m_tile;
  GC_CHECK_ARG(ctx, !top || slots < ((int64_t)1 << 32), "max_primitives: the active tiles must hold < 2^32 slots");
  // host-known: whether the merge launches at all, and its groups
  const bool capped = max_tile_size > 0 && m_tile > max_tile_size;
  const bool merge = !(m_tile < 2 || max_pairs <= 0) && !capped;
  GC_CHECK_ARG(ctx, !merge || m_tile <= 65536, "merge-reduce tile larger than 65536 slots");
  const int64_t P = m_tile * (m_tile - 1) / 2;
  int64_t G = 1;
  if (merge) {
    const int64_t budget = std::min<int64_t>(max_sort_keys > 0 ? max_sort_keys : GC_MAP_MAINTAIN_SORT_KEYS,
                                             ((int64_t)1 << 32) - 1);
    G = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(budget / P, kMaintainGroupTiles), n_active));
  }
  // one scratch for the whole call, sized before the first launch (growing it waits for the stream): the
  // partials, sums and thresholds, then the cull's sort and the merge's group, used one after the other
  struct CullSort {
    double *keys_in, *keys;
    void* tmp;
  } cs{};
  MergeScratch mg{};
  auto cull_layout = [&](gc::Carver& c) {
    cs.keys_in = c.take<double>((size_t)slots);
    cs.keys = c.take<double>((size_t)slots);
    cs.tmp = c.take<char>(gc::sort_temp_bytes(n_active, m_tile, false));
  };
  gc::Carver cull_size, merge_size;
  if (top) cull_layout(cull_size);
  if (merge) merge_layout(merge_size, G, m_tile, P, max_pairs);
  double *part, *sums, *thr_a;
  int32_t* n_sel;
  char* sub;
  if (int rc = gc::carve_scratch(ctx, [&](gc::Carver& c) {
        part = c.take<double>(4 * (size_t)part_blocks(m_tile) * n_active);
        sums = c.take<double>(4 * (size_t)n_active);
        thr_a = c.take<double>(n_active);
        n_sel = c.take<int32_t>(n_active);
        sub = c.take<char>(std::max(cull_size.bytes, merge_size.bytes));
      }))
    return rc;
  if (top) {
    gc::Carver c{sub};
    cull_layout(c);
  }
  if (merge) {
    gc::Carver c{sub};
    mg = merge_layout(c, G, m_tile, P, max_pairs);
  }

  // ---- the first launch; no host wait from here on
  const Tiles S{*map, 0, m_tile, d_active_dense};
  const dim3 per_tile(blocks_for(n_active));
  const double* thr_dev = nullptr;
  if (top) {  // the launches are host-known, the branch is each tile's own (k_tiles_cull_thr)
    if (int rc = reduce_into<4>(ctx, m_tile, n_active, part, sums, [&](dim3 grid) {
          hipLaunchKernelGGL((k_cull<false, false>), grid, dim3(256), 0, ctx->stream, S, thr0, thr_dev, gamma, part);
        }))
      return rc;
    hipLaunchKernelGGL(k_cull_keys, dim3(blocks_for(m_tile), (unsigned)n_active), dim3(256), 0, ctx->stream, S,
                       cs.keys_in);
    GC_LAUNCH_CHECK(ctx);
    if (int rc = sort_pairs(ctx, cs.keys_in, cs.keys, nullptr, nullptr, n_active, m_tile, true, cs.tmp)) return rc;
    hipLaunchKernelGGL(k_tiles_cull_thr, per_tile, dim3(256), 0, ctx->stream, (int)n_active, m_tile,
                       (const double*)sums, (const double*)cs.keys, thr0, max_primitives, thr_a);
    GC_LAUNCH_CHECK(ctx);
    thr_dev = thr_a;
  }
  // count at the tile's threshold, cull and forget in one streaming visit
  if (int rc = reduce_into<4>(ctx, m_tile, n_active, part, sums, [&](dim3 grid) {
        hipLaunchKernelGGL((k_cull<true, true>), grid, dim3(256), 0, ctx->stream, S, thr0, thr_dev, gamma, part);
      }))
    return rc;
  hipLaunchKernelGGL(k_tiles_cull_stats, per_tile, dim3(256), 0, ctx->stream, (int)n_active, m_tile,
                     (const double*)sums, thr_dev, thr0, (int)max_pairs, capped ? 1 : 0, d_stats);
  GC_LAUNCH_CHECK(ctx);
  if (!merge) return GC_OK;

  GC_HIP(ctx, hipMemsetAsync(n_sel, 0, sizeof(int32_t) * (size_t)n_active, ctx->stream));
  for (int64_t a0 = 0; a0 < n_active; a0 += G)
    if (int rc = merge_group(ctx, S, a0, std::min<int64_t>(G, n_active - a0), d_stats, mg, merge_thr, (int)max_pairs,
                             eps_psd, eps_lift, n_sel))
      return rc;
  const unsigned nb = part_blocks(m_tile);
  hipLaunchKernelGGL(k_count_valid, dim3(nb, (unsigned)n_active), dim3(256), 0, ctx->stream, S, part);
  GC_LAUNCH_CHECK(ctx);
  hipLaunchKernelGGL(k_tiles_merge_stats, per_tile, dim3(256), 0, ctx->stream, (int)n_active, (const double*)part,
                     (int)nb, (const int32_t*)n_sel, d_stats);
  GC_LAUNCH_CHECK(ctx);
  return GC_OK;
}

}  // extern "C"
