// gc_mapupdate.h — the launch halves of the fuse (gc_map.hip) and the masked insert (gc_mapops.hip),
// shared with gc_primitive_map_update (gc_mapupdate.hip), which chains them with no host wait in
// between. Both take validated arguments and their scratch from the caller.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "gc_internal.h"

namespace gc {

size_t fuse_scratch_bytes(int64_t K);
int fuse_launch(gc_ctx* ctx, const gc_primitive_map* map, const gc_fuse_batch* meas, const double* h_pose6,
                double eps_lift, double eps_mass, double timestamp, int64_t scan_seq, void* scr,
                uint32_t** d_counts, unsigned* n_counts);

// "Is this gc_primitive_map sound" for every entry that takes one (gc_mapops.hip): 0 < m_slots < max_slots,
// the lobe count, the layout, the seven core fields, valid_mask where the entry needs it, and the colour
// fields all set or all NULL. check_map_core stops before the colour fields, for the pipeline's attach, which
// takes some of them as optional.
int check_map_core(gc_ctx* ctx, const gc_primitive_map* map, int64_t max_slots, bool need_valid);
int check_map(gc_ctx* ctx, const gc_primitive_map* map, int64_t max_slots, bool need_valid);

// The argument check every per-tile entry starts with (also gc_maptiles.hip): joins the context's side
// stream, then the tile range and check_map.
int check_tile(gc_ctx* ctx, const gc_primitive_map* map, int64_t slot0, int64_t n_slots, bool need_valid);

size_t insert_scratch_bytes(int64_t n_slots);
int insert_launch(gc_ctx* ctx, const gc_primitive_map* map, int64_t slot0, int64_t n_slots,
                  const gc_insert_batch* batch, double timestamp, int64_t scan_seq, double recency_decay_lambda,
                  int64_t next_global_id, const int64_t* d_id_offset, int32_t* d_target_slots_out,
                  int64_t* d_new_ids_out, void* scr, double* d_out2);

}  // namespace gc
