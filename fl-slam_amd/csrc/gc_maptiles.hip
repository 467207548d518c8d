// gc_maptiles.hip — tile residency of the device PrimitiveMap: one tile's slots as a host image
// (export / import) and the empty tile of create_empty_tile (backend/structures/primitive_map.py:148-175).
//
// The reference's AtlasMap creates tiles on demand (primitive_map.py:183-211); the device map holds a
// fixed number of slabs, so a tile that leaves a slab is kept by the host as an image and comes back
// into whichever slab is free then. The image is n_slots records of gc_primitive_map_record_layout,
// whatever the map's own layout, so an image written by a packed map loads into a per-field one.
//
// A packed map whose sixteen fields all sit at the layout's offsets is its own image: one copy. Any
// other map goes through one kernel, one thread per 8-byte word of the image: the word's field and
// element come from a table built from the layout on the host, the slot's address from the map's own
// layout (gc_mapslot.h). Every field is 8-byte words but valid_mask, whose byte is the low byte of its
// word. Nothing here waits for the stream.
#include <hip/hip_runtime.h>
#include <string.h>
#include "gc_internal.h"
#include "gc_math.h"
#include "gc_mapslot.h"
#include "gc_mapupdate.h"

namespace gc {
namespace {

constexpr int kMaxRecWords = 64;  // 512 B: the record of 8 lobes
constexpr int kFieldValid = 13;   // the struct's field order (gc_primitive_map_record_layout)
constexpr int kFieldRgb = 11;

// word w of a record: the field it belongs to (-1: padding) and its 8-byte element of that field
struct RecTable {
  int8_t field[kMaxRecWords];
  int8_t elem[kMaxRecWords];
  int32_t words;
};

int64_t field_words(int k, int n_lobes) {
  const int64_t w[kRecFields] = {9, 3, 3 * (int64_t)n_lobes, 1, 1, 1, 1, 1, 1, 3, 1, 3, 3, 1, 1, 1};
  return w[k];
}

bool rec_table(int n_lobes, RecTable* R, int64_t* slot_bytes) {
  int64_t off[kRecFields], sb = 0;
  map_record_layout(n_lobes, off, &sb);
  if (sb % 8 != 0 || sb / 8 > kMaxRecWords) return false;
  R->words = (int32_t)(sb / 8);
  for (int w = 0; w < kMaxRecWords; ++w) R->field[w] = R->elem[w] = -1;
  for (int k = 0; k < kRecFields; ++k) {
    if (off[k] % 8 != 0) return false;
    for (int64_t e = 0; e < field_words(k, n_lobes); ++e) {
      const int64_t w = off[k] / 8 + e;
      if (w >= R->words || R->field[w] != -1) return false;
      R->field[w] = (int8_t)k;
      R->elem[w] = (int8_t)e;
    }
  }
  *slot_bytes = sb;
  return true;
}

// the map's own storage of field f at slot g: base (nullptr: the map does not hold the field), and the
// field's width in 8-byte words (valid_mask: bytes)
GC_DEV char* field_base(const gc_primitive_map& m, int f, int* width) {
  int w = 1;
  void* p = nullptr;
  switch (f) {
    case 0: p = m.Lambdas; w = 9; break;
    case 1: p = m.thetas; w = 3; break;
    case 2: p = m.etas; w = 3 * m.n_lobes; break;
    case 3: p = m.weights; break;
    case 4: p = m.timestamps; break;
    case 5: p = m.last_supported_scan_seq; break;
    case 6: p = m.last_update_scan_seq; break;
    case 7: p = m.cam_mass; break;
    case 8: p = m.lidar_mass; break;
    case 9: p = m.rgb_cam_accum; w = 3; break;
    case 10: p = m.rgb_cam_denom; break;
    case 11: p = m.rgb; w = 3; break;
    case 12: p = m.colors; w = 3; break;
    case 13: p = m.valid_mask; break;
    case 14: p = m.created_timestamps; break;
    case 15: p = m.primitive_ids; break;
    default: break;
  }
  *width = w;
  return (char*)p;
}

// create_empty_tile (primitive_map.py:148-175): zeros everywhere, rgb = 0.5
GC_DEV uint64_t empty_word(int f) { return f == kFieldRgb ? 0x3FE0000000000000ull /* 0.5 */ : 0ull; }

enum { kExport = 0, kImport = 1, kReset = 2 };

// One thread per word (slot s, word w) of the tile's image. kExport: img <- map, fields the map does
// not hold as create_empty_tile, padding zero. kImport: map <- img, fields the map does not hold and
// padding skipped. kReset: map <- create_empty_tile (img unused).
template <int MODE>
__global__ void __launch_bounds__(256) k_tile_words(gc_primitive_map m, int64_t s0, int64_t n, RecTable R,
                                                    uint64_t* img) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t s = i / R.words;
  const int w = (int)(i - s * R.words);
  if (s >= n) return;
  const int f = R.field[w], e = R.elem[w];
  if (f < 0) {
    if (MODE == kExport) img[i] = 0ull;
    return;
  }
  int width;
  char* base = field_base(m, f, &width);
  if (!base) {
    if (MODE == kExport) img[i] = empty_word(f);
    return;
  }
  const int64_t g = s0 + s;
  if (f == kFieldValid) {
    uint8_t* v = (uint8_t*)(m.slot_bytes ? base + g * m.slot_bytes : base + g);
    if (MODE == kExport) img[i] = (uint64_t)*v;
    if (MODE == kImport) *v = (uint8_t)(img[i] & 0xFFull);
    if (MODE == kReset) *v = 0;
    return;
  }
  uint64_t* p = (uint64_t*)(m.slot_bytes ? base + g * m.slot_bytes : base + g * (int64_t)width * 8) + e;
  if (MODE == kExport) img[i] = *p;
  if (MODE == kImport) *p = img[i];
  if (MODE == kReset) *p = empty_word(f);
}

// a packed map with every field at the layout's offset: the slots are the image
bool map_is_image(const gc_primitive_map& m) {
  if (m.slot_bytes == 0) return false;
  int64_t off[kRecFields], sb = 0;
  map_record_layout(m.n_lobes, off, &sb);
  const void* f[kRecFields] = {m.Lambdas, m.thetas, m.etas, m.weights, m.timestamps, m.last_supported_scan_seq,
                               m.last_update_scan_seq, m.cam_mass, m.lidar_mass, m.rgb_cam_accum, m.rgb_cam_denom,
                               m.rgb, m.colors, m.valid_mask, m.created_timestamps, m.primitive_ids};
  for (int k = 0; k < kRecFields; ++k)
    if (!f[k] || (const char*)f[k] - (const char*)m.Lambdas != off[k]) return false;
  return m.slot_bytes == sb;
}

template <int MODE>
int launch_words(gc_ctx* ctx, const gc_primitive_map* map, int64_t slot0, int64_t n_slots, const RecTable& R,
                 uint64_t* img) {
  const int64_t words = n_slots * R.words;
  hipLaunchKernelGGL(k_tile_words<MODE>, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, ctx->stream, *map,
                     slot0, n_slots, R, img);
  GC_LAUNCH_CHECK(ctx);
  return GC_OK;
}

int tile_args(gc_ctx* ctx, const gc_primitive_map* map, int64_t slot0, int64_t n_slots, RecTable* R, int64_t* sb) {
  if (int rc = check_tile(ctx, map, slot0, n_slots, false)) return rc;
  GC_CHECK_ARG(ctx, n_slots < ((int64_t)1 << 31) / kMaxRecWords, "tile too large");
  if (!rec_table(map->n_lobes, R, sb)) {
    set_error(ctx, "the packed record layout is not made of whole 8-byte words");
    return GC_ERR_RUNTIME;
  }
  return GC_OK;
}

}  // namespace
}  // namespace gc

using namespace gc;

extern "C" {

int32_t gc_primitive_map_tile_export(gc_ctx* ctx, const gc_primitive_map* map, int64_t slot0, int64_t n_slots,
                                     void* h_image) {
  RecTable R;
  int64_t sb = 0;
  if (int rc = tile_args(ctx, map, slot0, n_slots, &R, &sb)) return rc;
  if (n_slots == 0) return GC_OK;
  GC_CHECK_ARG(ctx, h_image != nullptr, "h_image is NULL");
  const size_t bytes = (size_t)n_slots * (size_t)sb;
  if (map_is_image(*map)) {
    GC_HIP(ctx, hipMemcpyAsync(h_image, (const char*)map->Lambdas + slot0 * sb, bytes, hipMemcpyDeviceToHost,
                               ctx->stream));
    return GC_OK;
  }
  uint64_t* img;
  if (int rc = carve_scratch(ctx, [&](Carver& c) { img = c.take<uint64_t>(bytes / 8); })) return rc;
  if (int rc = launch_words<kExport>(ctx, map, slot0, n_slots, R, img)) return rc;
  GC_HIP(ctx, hipMemcpyAsync(h_image, img, bytes, hipMemcpyDeviceToHost, ctx->stream));
  return GC_OK;
}

int32_t gc_primitive_map_tile_import(gc_ctx* ctx, const gc_primitive_map* map, int64_t slot0, int64_t n_slots,
                                     const void* h_image) {
  RecTable R;
  int64_t sb = 0;
  if (int rc = tile_args(ctx, map, slot0, n_slots, &R, &sb)) return rc;
  if (n_slots == 0) return GC_OK;
  GC_CHECK_ARG(ctx, h_image != nullptr, "h_image is NULL");
  const size_t bytes = (size_t)n_slots * (size_t)sb;
  if (map_is_image(*map)) {
    GC_HIP(ctx, hipMemcpyAsync((char*)map->Lambdas + slot0 * sb, h_image, bytes, hipMemcpyHostToDevice, ctx->stream));
    return GC_OK;
  }
  uint64_t* img;
  if (int rc = carve_scratch(ctx, [&](Carver& c) { img = c.take<uint64_t>(bytes / 8); })) return rc;
  GC_HIP(ctx, hipMemcpyAsync(img, h_image, bytes, hipMemcpyHostToDevice, ctx->stream));
  return launch_words<kImport>(ctx, map, slot0, n_slots, R, img);
}

int32_t gc_primitive_map_tile_reset(gc_ctx* ctx, const gc_primitive_map* map, int64_t slot0, int64_t n_slots) {
  RecTable R;
  int64_t sb = 0;
  if (int rc = tile_args(ctx, map, slot0, n_slots, &R, &sb)) return rc;
  if (n_slots == 0) return GC_OK;
  return launch_words<kReset>(ctx, map, slot0, n_slots, R, nullptr);
}

}  // extern "C"
