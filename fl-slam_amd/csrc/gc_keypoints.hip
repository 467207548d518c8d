// gc_keypoints.hip — the keypoint detector on the device: an rgb8 (or grey) image -> a table of
// (u, v, response) rows in HBM that gc_camera_features_lift reads in place. It covers the detector half
// of ORB as the visual feature node configures it (src/visual_feature_node.cpp:149-158, :512-535:
// nfeatures = max_features, scaleFactor 1.2, nlevels 8, edgeThreshold 31, firstLevel 0, HARRIS_SCORE,
// fastThreshold 20) and is BUILD-DEFINED: the definition in DESIGN.md §4 "Keypoint detector" follows the
// published algorithms (Rosten-Drummond FAST-9/16, Harris, ORB's per-level quotas) and was not checked
// against OpenCV; it does not claim OpenCV's bits. No angle, size, descriptor or blur.
//
// Every stage is integer arithmetic, or a fixed sequence of IEEE f64 operations with contraction off
// (the Harris tail on the device, the pyramid plan and the resize tables on the host), so the device
// agrees with the restatement (tests/keypoint_restatement.py) bit for bit.
//
//  k_kp_grey     Y = (4899 R + 9617 G + 1868 B + 8192) >> 14, four pixels per thread: three 32-bit loads,
//                one 32-bit store.
//  k_kp_resize   level l from level l - 1, 8-bit bilinear with 11-bit weights from the host's index and
//                weight tables; one launch per level (the chain is a true dependency).
//  k_kp_fast     one launch over the 32 x 32 tiles of all levels. A workgroup stages its tile plus a
//                4-pixel halo as bytes in LDS, scores the tile plus a 1-pixel ring (the ring is recomputed,
//                not exchanged), suppresses non-maxima, applies the border and appends the survivors' keys
//                [level | 255 - score | raster index] (4 + 8 + 26 bits, held in a double's bit image) to one
//                list. No two survivors are 8-adjacent, so a tile holds at most 16 x 16 of them and a level
//                at most ceil(W_l / 2) ceil(H_l / 2): the list cannot overflow. The appends land in any
//                order; the keys are distinct, so one gc::radix_sort_pairs over the list (five of its
//                passes: the keys end below bit 40) gives the order of the first cut whatever the arrival
//                order, level l's run starting at the sum of the lower levels' counts. Unused entries
//                hold a filler that sorts after every key.
//  k_kp_harris   one wavefront per survivor of the first cut; 49 lanes take one pixel of the 7 x 7 block
//                each, the three integer wave sums are order-free (gc_blocksum.h group_sum_xor), lane 0
//                does the seven f64 operations.
//  k_kp_select   the second cut by rank counting through LDS: a candidate's rank is the number of
//                candidates of its level that beat it (greater response, or equal with a lower raster
//                index); rank < n_l writes row offset_l + rank. The last row of workgroups writes the kept
//                counts and the total and zero-fills the rows past the total.
//
// Integer atomics only: a tile's two LDS counters, and per level two device counters (the corners after
// suppression; the border survivors, which is also the cursor of the level's part of the list), each on
// a 256-byte line of its own and zeroed on the stream in every call; k_kp_select copies them into the
// caller's counts. Wave64 throughout, no host wait inside the entry.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>
#include <vector>
#include "gc_blocksum.h"
#include "gc_internal.h"
#include "gc_math.h"
#include "gc_sort.h"

// no fused multiply-adds anywhere in this file: the Harris tail, the plan and the resize tables round
// once per operation
#pragma clang fp contract(off)

namespace gc {
namespace {

constexpr int kKpLevels = GC_KP_MAX_LEVELS;
constexpr int kKpT = 256;                          // threads of every workgroup here
constexpr int kKpTile = 32;                        // a FAST tile is kKpTile x kKpTile pixels
constexpr int kKpHalo = 4;                         // the ring of scores (1) plus the circle's radius (3)
constexpr int kKpStage = kKpTile + 2 * kKpHalo;    // staged bytes per side
constexpr int kKpRing = kKpTile + 2;               // scored pixels per side
constexpr int kKpTileCap = (kKpTile / 2) * (kKpTile / 2);  // survivors a tile can hold
constexpr int kKpBlock = 7;                        // the Harris block
constexpr int kKpPad = 64;                         // words between two device counters: a 256-byte line each,
                                                   // so the tiles' atomics of different levels do not share one
constexpr int64_t kKpMaxPixels = GC_IMAGE_MAX_PIXELS;
constexpr int kKpRasterBits = 26, kKpScoreBits = 8, kKpLevelBits = 4;
// The keys are 38-bit integers held in the doubles' bit images (small positive doubles order as their
// bits do), so five 8-bit passes of the library's sort order them; an unused list entry is filled with
// bytes of 0x7f, whose low 40 bits exceed every key.
constexpr int kKpSortPasses = (kKpRasterBits + kKpScoreBits + kKpLevelBits + 7) / 8;
static_assert(kKpMaxPixels <= (1ll << kKpRasterBits) && kKpLevels <= (1 << kKpLevelBits), "the key's fields");
static_assert(0x7f7f7f7f7fll >= (1ll << (kKpRasterBits + kKpScoreBits + kKpLevelBits)), "the filler sorts last");
constexpr int kKpMaxFeatures = GC_CAM_MAX_QUERIES;  // the rows of one camera batch
static_assert(kKpTileCap <= kKpT, "one key slot per thread is enough for a tile");
static_assert(kKpBlock * kKpBlock <= 64, "one lane per block pixel");
static_assert(49 * 1020 * 1020 < (1ll << 31), "the Harris sums fit int32");

// what the kernels know about the levels (by value in the kernel arguments)
struct KpDev {
  int nlevels, nfeatures, edge, thr;
  int W[kKpLevels], H[kKpLevels], quota[kKpLevels], slots[kKpLevels], tiles_x[kKpLevels];
  int slot_off[kKpLevels + 1], tile_off[kKpLevels + 1];
  int cap[kKpLevels];
  long long pyr_off[kKpLevels], cap_off[kKpLevels];
  double scale[kKpLevels];
};

struct KpPlan {
  KpDev d;
  double harris_k;
  int64_t cap[kKpLevels], cap_total, pyr_bytes, tab_off[kKpLevels], tab_ints;
  int max_slots;
};

struct KpScratch {
  int32_t* tab;
  double *keys_in, *keys, *resp;
  void* sort_tmp;
  int32_t* ctr;  // [nms | border] x kKpLevels counters, kKpPad words apart
};

void kp_layout(Carver& c, const KpPlan& p, KpScratch* s) {
  s->tab = c.take<int32_t>((size_t)p.tab_ints);
  s->keys_in = c.take<double>((size_t)p.cap_total);
  s->keys = c.take<double>((size_t)p.cap_total);
  s->resp = c.take<double>((size_t)p.d.slot_off[p.d.nlevels]);
  s->sort_tmp = c.take<char>(sort_temp_bytes(1, p.cap_total, false));
  s->ctr = c.take<int32_t>((size_t)2 * kKpLevels * kKpPad);
}

bool kp_is_int(double v, double lo, double hi) { return v == floor(v) && v >= lo && v <= hi; }  // false for NaN

// the checks of the configuration and the plan of step 2 (host arithmetic, contraction off)
int kp_plan(gc_ctx* ctx, int64_t H, int64_t W, const gc_kp_cfg* h, KpPlan* p) {
  GC_CHECK_ARG(ctx, H >= 1 && W >= 1 && H * W <= kKpMaxPixels, "H and W must be >= 1 and H W <= 2^26");
  GC_CHECK_ARG(ctx, kp_is_int(h->nfeatures, 1.0, (double)kKpMaxFeatures), "nfeatures must be an integer in [1, 4096]");
  GC_CHECK_ARG(ctx, fabs(h->scale_factor) <= 3.40282347e38, "scale_factor must be finite as float32");  // false for NaN
  const float sf = (float)h->scale_factor;
  GC_CHECK_ARG(ctx, sf > 1.0f, "scale_factor must be > 1 as float32");
  GC_CHECK_ARG(ctx, kp_is_int(h->nlevels, 1.0, (double)kKpLevels), "nlevels must be an integer in [1, 16]");
  GC_CHECK_ARG(ctx, kp_is_int(h->edge_threshold, 4.0, 1024.0), "edge_threshold must be an integer in [4, 1024]");
  GC_CHECK_ARG(ctx, kp_is_int(h->fast_threshold, 1.0, 254.0), "fast_threshold must be an integer in [1, 254]");
  GC_CHECK_ARG(ctx, fabs(h->harris_k) <= 1.79769313486231570815e308, "harris_k must be finite");
  memset(p, 0, sizeof(*p));
  KpDev& d = p->d;
  d.nfeatures = (int)h->nfeatures; d.nlevels = (int)h->nlevels; d.edge = (int)h->edge_threshold;
  d.thr = (int)h->fast_threshold; p->harris_k = h->harris_k;
  // quotas
  const double f = 1.0 / (double)sf;
  double nd = (double)d.nfeatures * (1.0 - f) / (1.0 - pow(f, (double)d.nlevels));
  int sum = 0;
  for (int l = 0; l + 1 < d.nlevels; ++l) {
    d.quota[l] = (int)rint(nd);
    sum += d.quota[l];
    nd *= f;
  }
  d.quota[d.nlevels - 1] = d.nfeatures - sum > 0 ? d.nfeatures - sum : 0;
  for (int l = 0; l < d.nlevels; ++l) {
    d.scale[l] = (double)(float)pow((double)sf, (double)l);
    const double wl = rint((double)W / d.scale[l]), hl = rint((double)H / d.scale[l]);
    d.W[l] = wl < 1.0 ? 1 : (int)wl;  // a level never vanishes
    d.H[l] = hl < 1.0 ? 1 : (int)hl;
    p->cap[l] = (int64_t)((d.W[l] + 1) / 2) * ((d.H[l] + 1) / 2);
    d.pyr_off[l] = p->pyr_bytes;
    p->pyr_bytes += (int64_t)align256((size_t)d.W[l] * d.H[l]);
    d.cap[l] = (int)p->cap[l];
    d.cap_off[l] = p->cap_total;  // level l's part of the list
    p->cap_total += p->cap[l];
    const int64_t two_n = 2 * (int64_t)d.quota[l];
    d.slots[l] = (int)(two_n < p->cap[l] ? two_n : p->cap[l]);
    d.slot_off[l + 1] = d.slot_off[l] + d.slots[l];
    if (d.slots[l] > p->max_slots) p->max_slots = d.slots[l];
    d.tiles_x[l] = (d.W[l] + kKpTile - 1) / kKpTile;
    d.tile_off[l + 1] = d.tile_off[l] + d.tiles_x[l] * ((d.H[l] + kKpTile - 1) / kKpTile);
    p->tab_off[l] = p->tab_ints;
    if (l > 0) p->tab_ints += 2 * ((int64_t)d.W[l] + d.H[l]);  // i0 and w1 of the x axis, then of the y axis
  }
  return GC_OK;
}

// step 3, one axis: the index and the weight (of 2048) per destination index
void kp_resize_table(int64_t n_s, int64_t n_d, int32_t* i0, int32_t* w1) {
  const double sc = (double)n_s / (double)n_d;
  for (int64_t j = 0; j < n_d; ++j) {
    const double f = ((double)j + 0.5) * sc - 0.5;
    const double fl = floor(f);
    int64_t i = (int64_t)fl;
    int32_t w = (int32_t)rint((f - fl) * 2048.0);
    if (i < 0) { i = 0; w = 0; }
    if (i >= n_s - 1) { i = n_s - 1; w = 0; }
    i0[j] = (int32_t)i;
    w1[j] = w;
  }
}

// ---- step 1
__global__ void __launch_bounds__(kKpT) k_kp_grey(const uint8_t* __restrict__ rgb, uint8_t* __restrict__ grey,
                                                  int n, int vec) {
  const int i4 = 4 * (blockIdx.x * kKpT + threadIdx.x);
  if (i4 >= n) return;
  if (vec && i4 + 3 < n) {
    const uint32_t* src = (const uint32_t*)(rgb + 3 * (int64_t)i4);
    const uint32_t w0 = src[0], w1 = src[1], w2 = src[2];  // R0 G0 B0 R1 | G1 B1 R2 G2 | B2 R3 G3 B3
    const uint32_t r[4] = {w0 & 255u, w0 >> 24, (w1 >> 16) & 255u, (w2 >> 8) & 255u};
    const uint32_t g[4] = {(w0 >> 8) & 255u, w1 & 255u, w1 >> 24, (w2 >> 16) & 255u};
    const uint32_t b[4] = {(w0 >> 16) & 255u, (w1 >> 8) & 255u, w2 & 255u, w2 >> 24};
    uint32_t out = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) out |= ((4899u * r[q] + 9617u * g[q] + 1868u * b[q] + 8192u) >> 14) << (8 * q);
    *(uint32_t*)(grey + i4) = out;
    return;
  }
  for (int i = i4; i < n && i < i4 + 4; ++i) {
    const uint8_t* px = rgb + 3 * (int64_t)i;
    grey[i] = (uint8_t)((4899u * px[0] + 9617u * px[1] + 1868u * px[2] + 8192u) >> 14);
  }
}

// ---- step 3: tab = [x i0 (Wd), x w1 (Wd), y i0 (Hd), y w1 (Hd)]
__global__ void __launch_bounds__(kKpT) k_kp_resize(const uint8_t* __restrict__ src, int Ws, int Hs,
                                                    uint8_t* __restrict__ dst, int Wd, int Hd,
                                                    const int32_t* __restrict__ tab) {
  const int i = blockIdx.x * kKpT + threadIdx.x;
  if (i >= Wd * Hd) return;
  const int y = i / Wd, x = i - y * Wd;
  const int x0 = tab[x], wx = tab[Wd + x], y0 = tab[2 * Wd + y], wy = tab[2 * Wd + Hd + y];
  const int x1 = x0 + 1 < Ws ? x0 + 1 : Ws - 1, y1 = y0 + 1 < Hs ? y0 + 1 : Hs - 1;
  const uint8_t *r0 = src + (int64_t)y0 * Ws, *r1 = src + (int64_t)y1 * Ws;
  const int top = (int)r0[x0] * (2048 - wx) + (int)r0[x1] * wx;
  const int bot = (int)r1[x0] * (2048 - wx) + (int)r1[x1] * wx;
  dst[i] = (uint8_t)((top * (2048 - wy) + bot * wy + (1 << 21)) >> 22);  // below 2^31
}

// the level of item `i` of a list whose per-level runs start at off[0 .. nlevels]
GC_DEV int kp_level_of(const int* off, int nlevels, int i) {
  int l = 0;
  while (l + 1 < nlevels && i >= off[l + 1]) ++l;
  return l;
}

// step 4 for the staged pixel at index c: m - 1 where m > thr, else 0
GC_DEV int kp_fast_score(const uint8_t* px, int c, int thr) {
  const int ip = px[c];
  int d[16];
#define KP_LOAD(k, dx, dy) d[k] = (int)px[c + (dy) * kKpStage + (dx)] - ip;
  KP_LOAD(0, 0, 3) KP_LOAD(1, 1, 3) KP_LOAD(2, 2, 2) KP_LOAD(3, 3, 1) KP_LOAD(4, 3, 0) KP_LOAD(5, 3, -1)
  KP_LOAD(6, 2, -2) KP_LOAD(7, 1, -3) KP_LOAD(8, 0, -3) KP_LOAD(9, -1, -3) KP_LOAD(10, -2, -2) KP_LOAD(11, -3, -1)
  KP_LOAD(12, -3, 0) KP_LOAD(13, -3, 1) KP_LOAD(14, -2, 2) KP_LOAD(15, -1, 3)
#undef KP_LOAD
  // min and max over every arc of 9: windows of 2, 4, 8, then one more
  int lo2[16], hi2[16], lo4[16], hi4[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    lo2[k] = min(d[k], d[(k + 1) & 15]);
    hi2[k] = max(d[k], d[(k + 1) & 15]);
  }
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    lo4[k] = min(lo2[k], lo2[(k + 2) & 15]);
    hi4[k] = max(hi2[k], hi2[(k + 2) & 15]);
  }
  int bright = -255, dark_neg = 255;  // max over arcs of min(I_k - I_p); min over arcs of max(I_k - I_p)
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const int lo9 = min(min(lo4[k], lo4[(k + 4) & 15]), d[(k + 8) & 15]);
    const int hi9 = max(max(hi4[k], hi4[(k + 4) & 15]), d[(k + 8) & 15]);
    bright = max(bright, lo9);
    dark_neg = min(dark_neg, hi9);
  }
  const int m = max(bright, -dark_neg);  // max over arcs of min(I_p - I_k) = -dark_neg
  return m > thr ? m - 1 : 0;
}

// ---- steps 4-6
__global__ void __launch_bounds__(kKpT) k_kp_fast(KpDev L, const uint8_t* __restrict__ pyr, double* __restrict__ keys,
                                                  int32_t* ctr) {
  __shared__ uint8_t s_px[kKpStage * kKpStage];
  __shared__ uint8_t s_sc[kKpRing * kKpRing];
  __shared__ double s_key[kKpTileCap];
  __shared__ int s_n[3];  // corners after suppression, after the border, the list base
  const int t = threadIdx.x;
  const int l = kp_level_of(L.tile_off, L.nlevels, (int)blockIdx.x);
  const int tile = (int)blockIdx.x - L.tile_off[l];
  const int W = L.W[l], H = L.H[l];
  const int x0 = (tile % L.tiles_x[l]) * kKpTile, y0 = (tile / L.tiles_x[l]) * kKpTile;
  const uint8_t* img = pyr + L.pyr_off[l];
  if (t < 3) s_n[t] = 0;
  {
    // every load of the thread issued before the first LDS store, so they share one trip to memory
    constexpr int kRounds = (kKpStage * kKpStage + kKpT - 1) / kKpT;
    uint8_t v[kRounds];
#pragma unroll
    for (int k = 0; k < kRounds; ++k) {
      const int i = t + k * kKpT;
      const int gx = x0 - kKpHalo + i % kKpStage, gy = y0 - kKpHalo + i / kKpStage;
      v[k] = (i < kKpStage * kKpStage && gx >= 0 && gx < W && gy >= 0 && gy < H) ? img[(int64_t)gy * W + gx] : (uint8_t)0;
    }
#pragma unroll
    for (int k = 0; k < kRounds; ++k)
      if (t + k * kKpT < kKpStage * kKpStage) s_px[t + k * kKpT] = v[k];
  }
  __syncthreads();
  for (int i = t; i < kKpRing * kKpRing; i += kKpT) {
    const int sx = i % kKpRing, sy = i / kKpRing;
    const int gx = x0 - 1 + sx, gy = y0 - 1 + sy;
    int s = 0;
    if (gx >= 3 && gx < W - 3 && gy >= 3 && gy < H - 3) s = kp_fast_score(s_px, (sy + 3) * kKpStage + sx + 3, L.thr);
    s_sc[i] = (uint8_t)s;
  }
  __syncthreads();
  for (int i = t; i < kKpTile * kKpTile; i += kKpT) {
    const int px = i % kKpTile, py = i / kKpTile;
    const int gx = x0 + px, gy = y0 + py;
    const int c = (py + 1) * kKpRing + px + 1;
    const int s = s_sc[c];
    if (s == 0 || gx >= W || gy >= H) continue;
    const bool peak = s > s_sc[c - kKpRing - 1] && s > s_sc[c - kKpRing] && s > s_sc[c - kKpRing + 1] &&
                      s > s_sc[c - 1] && s > s_sc[c + 1] && s > s_sc[c + kKpRing - 1] && s > s_sc[c + kKpRing] &&
                      s > s_sc[c + kKpRing + 1];
    if (!peak) continue;
    atomicAdd(&s_n[0], 1);
    if (gx >= L.edge && gx < W - L.edge && gy >= L.edge && gy < H - L.edge) {
      const int slot = atomicAdd(&s_n[1], 1);
      const long long key = ((long long)l << (kKpRasterBits + kKpScoreBits)) | ((long long)(255 - s) << kKpRasterBits) |
                            (long long)(gy * W + gx);
      if (slot < kKpTileCap) s_key[slot] = __longlong_as_double(key);
    }
  }
  __syncthreads();
  if (t == 0) {
    int base = 0;
    if (s_n[0]) atomicAdd(&ctr[l * kKpPad], s_n[0]);
    if (s_n[1]) base = atomicAdd(&ctr[(kKpLevels + l) * kKpPad], s_n[1]);  // the border count is the level's cursor
    s_n[2] = base;
  }
  __syncthreads();
  const int n = s_n[1] < kKpTileCap ? s_n[1] : kKpTileCap;
  const int base = s_n[2];
  if (t < n && base + t < L.cap[l]) keys[L.cap_off[l] + base + t] = s_key[t];  // the second always holds (step 5)
}

GC_DEV int kp_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// per level: the survivors of the first cut m_l = min(slots_l, border count_l) and where level l's run
// starts in the sorted list (the fillers between the levels' parts of the list sort behind every key)
GC_DEV void kp_runs(const KpDev& L, const int32_t* ctr, int l, int* start, int* m_l) {
  // all GC_KP_MAX_LEVELS border counts (zero past nlevels) in one unrolled batch of independent loads
  int s = 0, c = 0;
#pragma unroll
  for (int q = 0; q < kKpLevels; ++q) {
    const int cq = ctr[(kKpLevels + q) * kKpPad];
    s += q < l ? cq : 0;
    c = q == l ? cq : c;
  }
  *start = s;
  *m_l = c < L.slots[l] ? c : L.slots[l];
}

// ---- steps 7-8: one wavefront per survivor of the first cut
__global__ void __launch_bounds__(kKpT) k_kp_harris(KpDev L, const uint8_t* __restrict__ pyr,
                                                    const double* __restrict__ keys, long long cap_total,
                                                    const int32_t* __restrict__ ctr, double harris_k, double s4,
                                                    double* __restrict__ resp) {
  const int lane = threadIdx.x & 63;
  const int slot = (int)blockIdx.x * (kKpT / 64) + (threadIdx.x >> 6);
  if (slot >= L.slot_off[L.nlevels]) return;
  const int l = kp_level_of(L.slot_off, L.nlevels, slot);
  const int j = slot - L.slot_off[l];
  int start, m_l;
  kp_runs(L, ctr, l, &start, &m_l);
  if (j >= m_l || start + j >= cap_total) return;  // the second never holds; it guards the address
  const long long key = __double_as_longlong(keys[start + j]);
  const int ras = (int)(key & ((1ll << kKpRasterBits) - 1));
  const int W = L.W[l], H = L.H[l];
  const int y = ras / W, x = ras - y * W;
  const uint8_t* img = pyr + L.pyr_off[l];
  int ix = 0, iy = 0;
  if (lane < kKpBlock * kKpBlock) {
    // edge >= 4 keeps these reads inside the image; the clamps only guard the addresses
    const int cx = x + lane % kKpBlock - kKpBlock / 2, cy = y + lane / kKpBlock - kKpBlock / 2;
    const int xm = kp_clampi(cx - 1, 0, W - 1), xc = kp_clampi(cx, 0, W - 1), xp = kp_clampi(cx + 1, 0, W - 1);
    const int ym = kp_clampi(cy - 1, 0, H - 1), yc = kp_clampi(cy, 0, H - 1), yp = kp_clampi(cy + 1, 0, H - 1);
    const uint8_t *rm = img + (int64_t)ym * W, *rc = img + (int64_t)yc * W, *rp = img + (int64_t)yp * W;
    const int mm = rm[xm], mc = rm[xc], mp = rm[xp], cm = rc[xm], cp = rc[xp], pm = rp[xm], pc = rp[xc], pp = rp[xp];
    ix = 2 * (cp - cm) + (mp - mm) + (pp - pm);
    iy = 2 * (pc - mc) + (pm - mm) + (pp - mp);
  }
  const int a_i = group_sum_xor<64>(ix * ix), b_i = group_sum_xor<64>(iy * iy), c_i = group_sum_xor<64>(ix * iy);
  if (lane != 0) return;
  const double a = (double)(long long)a_i, b = (double)(long long)b_i, c = (double)(long long)c_i;
  const double t1 = a * b;
  const double t2 = c * c;
  const double t3 = t1 - t2;
  const double s = a + b;
  const double t4 = s * s;
  const double t5 = harris_k * t4;
  resp[slot] = (t3 - t5) * s4;
}

// ---- steps 9-10. grid (ceil(max slots / kKpT), nlevels + 1)
__global__ void __launch_bounds__(kKpT) k_kp_select(KpDev L, const double* __restrict__ keys, long long cap_total,
                                                    const int32_t* __restrict__ ctr, int32_t* __restrict__ counts,
                                                    const double* __restrict__ resp, double* __restrict__ kp,
                                                    int32_t* __restrict__ meta) {
  __shared__ double s_r[kKpT];
  __shared__ int s_ras[kKpT];
  __shared__ int s_cnt[kKpLevels], s_nms[kKpLevels];
  const int t = threadIdx.x, l = blockIdx.y;
  // the levels' border counts in one trip to memory (a loop of loads would pay one trip per level)
  if (t < kKpLevels) {
    s_cnt[t] = ctr[(kKpLevels + t) * kKpPad];
    s_nms[t] = ctr[t * kKpPad];
  }
  __syncthreads();
  // the kept counts of every level; the rounded quotas never overrun the table
  int start = 0, off = 0, m_l = 0, kept_l = 0, total = 0, run = 0;
  const bool writer = l == L.nlevels && blockIdx.x == 0 && t == 0;
  for (int q = 0; q < L.nlevels; ++q) {
    const int c = s_cnt[q];
    const int m = c < L.slots[q] ? c : L.slots[q];
    int kept = m < L.quota[q] ? m : L.quota[q];
    if (kept > L.nfeatures - total) kept = L.nfeatures - total;
    if (q == l) { start = run; off = total; m_l = m; kept_l = kept; }
    if (writer) { counts[3 * q] = s_nms[q]; counts[3 * q + 1] = c; counts[3 * q + 2] = kept; }
    run += c;
    total += kept;
  }
  if (l == L.nlevels) {
    if (writer) {
      for (int q = 3 * L.nlevels; q < 3 * kKpLevels; ++q) counts[q] = 0;
      counts[3 * kKpLevels] = total;
    }
    for (int row = total + (int)blockIdx.x * kKpT + t; row < L.nfeatures; row += (int)gridDim.x * kKpT) {
      kp[3 * row] = 0.0; kp[3 * row + 1] = 0.0; kp[3 * row + 2] = 0.0;
      meta[4 * row] = 0; meta[4 * row + 1] = 0; meta[4 * row + 2] = 0; meta[4 * row + 3] = 0;
    }
    return;
  }
  if (start + m_l > cap_total) m_l = cap_total > start ? (int)(cap_total - start) : 0;  // never; guards the address
  if ((int)blockIdx.x * kKpT >= m_l) return;  // the whole workgroup
  const int i = (int)blockIdx.x * kKpT + t;
  const bool have = i < m_l;
  const long long key = have ? __double_as_longlong(keys[start + i]) : 0ll;
  const int ras = (int)(key & ((1ll << kKpRasterBits) - 1));
  const double r = have ? resp[L.slot_off[l] + i] : 0.0;
  int rank = 0;
  for (int j0 = 0; j0 < m_l; j0 += kKpT) {
    const int nj = m_l - j0 < kKpT ? m_l - j0 : kKpT;
    // past the run: a response that beats nobody, so the count below runs in whole groups of eight
    s_r[t] = t < nj ? resp[L.slot_off[l] + j0 + t] : -__builtin_inf();
    s_ras[t] = t < nj ? (int)(__double_as_longlong(keys[start + j0 + t]) & ((1ll << kKpRasterBits) - 1)) : 0;
    __syncthreads();
    for (int j = 0; j < nj; j += 8) {
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const double rj = s_r[j + q];
        const int sj = s_ras[j + q];
        rank += (int)(rj > r) | ((int)(rj == r) & (int)(sj < ras));  // no branch between the LDS reads
      }
    }
    __syncthreads();
  }
  if (!have || rank >= kept_l) return;
  const int row = off + rank;
  const int W = L.W[l];
  const int y = ras / W, x = ras - y * W;
  kp[3 * row] = (double)x * L.scale[l];
  kp[3 * row + 1] = (double)y * L.scale[l];
  kp[3 * row + 2] = r;
  meta[4 * row] = l;
  meta[4 * row + 1] = x;
  meta[4 * row + 2] = y;
  meta[4 * row + 3] = 255 - (int)((key >> kKpRasterBits) & 255);
}

}  // namespace
}  // namespace gc

using namespace gc;

extern "C" {

int32_t gc_keypoints_plan(int32_t H, int32_t W, const gc_kp_cfg* cfg, int64_t* h_levels, double* h_scales,
                          int64_t* h_bytes) {
  GC_CHECK_ARG(nullptr, cfg && h_levels && h_scales && h_bytes, "NULL argument");
  KpPlan p;
  if (int rc = kp_plan(nullptr, H, W, cfg, &p)) return rc;
  for (int l = 0; l < kKpLevels; ++l) {
    int64_t* row = h_levels + GC_KP_PLAN_ROW * l;
    const bool on = l < p.d.nlevels;
    row[0] = on ? p.d.W[l] : 0;
    row[1] = on ? p.d.H[l] : 0;
    row[2] = on ? p.d.quota[l] : 0;
    row[3] = on ? p.cap[l] : 0;
    row[4] = on ? p.d.pyr_off[l] : 0;
    h_scales[l] = on ? p.d.scale[l] : 0.0;
  }
  Carver size;
  KpScratch s;
  kp_layout(size, p, &s);
  h_bytes[0] = p.pyr_bytes;
  h_bytes[1] = (int64_t)size.bytes;
  return GC_OK;
}

int32_t gc_keypoints_resize_table(int64_t n_src, int64_t n_dst, int32_t* h_i0, int32_t* h_w1) {
  GC_CHECK_ARG(nullptr, h_i0 && h_w1, "NULL argument");
  GC_CHECK_ARG(nullptr, n_src >= 1 && n_dst >= 1 && n_src <= kKpMaxPixels && n_dst <= kKpMaxPixels,
               "n_src and n_dst must be in [1, 2^26]");
  kp_resize_table(n_src, n_dst, h_i0, h_w1);
  return GC_OK;
}

int32_t gc_keypoints_detect(gc_ctx* ctx, int32_t H, int32_t W, int32_t channels, const uint8_t* d_image,
                            const gc_kp_cfg* cfg, uint8_t* d_pyramid, double* d_kp, int32_t* d_meta,
                            int32_t* d_counts) {
  GC_CHECK_ARG(nullptr, ctx != nullptr, "ctx is NULL");
  if (int rc_j = gc::join_side(ctx)) return rc_j;
  GC_CHECK_ARG(ctx, cfg != nullptr, "NULL configuration");
  GC_CHECK_ARG(ctx, channels == 1 || channels == 3, "channels must be 1 or 3");
  KpPlan p;
  if (int rc = kp_plan(ctx, H, W, cfg, &p)) return rc;
  GC_CHECK_ARG(ctx, d_image && d_pyramid && d_kp && d_meta && d_counts, "NULL image or output buffer");
  const KpDev& L = p.d;
  KpScratch s;
  if (int rc = carve_scratch(ctx, [&](Carver& c) { kp_layout(c, p, &s); })) return rc;
  hipStream_t st = ctx->stream;
  // the counters start from zero in every call; an unused list entry sorts after every key
  GC_HIP(ctx, hipMemsetAsync(s.ctr, 0, sizeof(int32_t) * 2 * kKpLevels * kKpPad, st));
  GC_HIP(ctx, hipMemsetAsync(s.keys_in, 0x7f, sizeof(double) * (size_t)p.cap_total, st));
  const int n0 = H * W;
  if (channels == 3) {
    const int vec = (((uintptr_t)d_image | (uintptr_t)d_pyramid) & 3u) == 0;
    hipLaunchKernelGGL(k_kp_grey, dim3((unsigned)((n0 + 4 * kKpT - 1) / (4 * kKpT))), dim3(kKpT), 0, st, d_image, d_pyramid,
                       n0, vec);
    GC_LAUNCH_CHECK(ctx);
  } else {
    GC_HIP(ctx, hipMemcpyAsync(d_pyramid, d_image, (size_t)n0, hipMemcpyDeviceToDevice, st));
  }
  // the resize tables of every level, staged through the context's pinned ring: one upload and no wait
  // while they fit one of its segments (33 KB at 640 x 480), else one upload per level
  std::vector<int32_t> tab((size_t)p.tab_ints);
  for (int l = 1; l < L.nlevels; ++l) {
    int32_t* t = tab.data() + p.tab_off[l];
    kp_resize_table(L.W[l - 1], L.W[l], t, t + L.W[l]);
    kp_resize_table(L.H[l - 1], L.H[l], t + 2 * L.W[l], t + 2 * L.W[l] + L.H[l]);
  }
  const bool one_upload = sizeof(int32_t) * tab.size() <= gc_ctx::kStageSeg;
  if (one_upload && !tab.empty())
    if (int rc = gc_buffer_upload(ctx, s.tab, tab.data(), sizeof(int32_t) * tab.size())) return rc;
  for (int l = 1; l < L.nlevels; ++l) {
    const int Ws = L.W[l - 1], Hs = L.H[l - 1], Wd = L.W[l], Hd = L.H[l];
    int32_t* d_tab = s.tab + p.tab_off[l];
    if (!one_upload)
      if (int rc = gc_buffer_upload(ctx, d_tab, tab.data() + p.tab_off[l], sizeof(int32_t) * 2 * ((size_t)Wd + Hd)))
        return rc;
    hipLaunchKernelGGL(k_kp_resize, dim3((unsigned)((Wd * Hd + kKpT - 1) / kKpT)), dim3(kKpT), 0, st,
                       (const uint8_t*)d_pyramid + L.pyr_off[l - 1], Ws, Hs, d_pyramid + L.pyr_off[l], Wd, Hd,
                       (const int32_t*)d_tab);
    GC_LAUNCH_CHECK(ctx);
  }
  hipLaunchKernelGGL(k_kp_fast, dim3((unsigned)L.tile_off[L.nlevels]), dim3(kKpT), 0, st, L, (const uint8_t*)d_pyramid,
                     s.keys_in, s.ctr);
  GC_LAUNCH_CHECK(ctx);
  if (radix_sort_pairs(st, s.keys_in, s.keys, nullptr, nullptr, 1, p.cap_total, false, s.sort_tmp, kKpSortPasses) !=
      hipSuccess) {
    set_error(ctx, "the keypoint candidate sort failed");
    return GC_ERR_RUNTIME;
  }
  const int n_slots = L.slot_off[L.nlevels];
  if (n_slots > 0) {
    // q = 1 / (4 * 7 * 255), s4 = q^4
    const double q = 1.0 / (4.0 * 7.0 * 255.0), q2 = q * q, s4 = q2 * q2;
    hipLaunchKernelGGL(k_kp_harris, dim3((unsigned)((n_slots + kKpT / 64 - 1) / (kKpT / 64))), dim3(kKpT), 0, st, L,
                       (const uint8_t*)d_pyramid, (const double*)s.keys, (long long)p.cap_total, (const int32_t*)s.ctr,
                       p.harris_k, s4, s.resp);
    GC_LAUNCH_CHECK(ctx);
  }
  const int chunks = p.max_slots > 0 ? (p.max_slots + kKpT - 1) / kKpT : 1;
  hipLaunchKernelGGL(k_kp_select, dim3((unsigned)chunks, (unsigned)(L.nlevels + 1)), dim3(kKpT), 0, st, L,
                     (const double*)s.keys, (long long)p.cap_total, (const int32_t*)s.ctr, d_counts, (const double*)s.resp,
                     d_kp, d_meta);
  GC_LAUNCH_CHECK(ctx);
  return GC_OK;
}

}  // extern "C"
