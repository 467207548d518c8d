"""The post-pose map update composed from the project's per-tile drop-ins, as a caller had to do it
before primitive_map_update_from_association: block_associations_for_fuse on the
host, one primitive_map_fuse per block and active tile, the insert plan in NumPy
(mapupdate_restatement.insert_plan), one primitive_map_insert_masked per active tile, then cull /
forget / merge-reduce per tile. Every device entry it reaches predates the fused operator. Used by
test_gpu_mapupdate.py as a second route and by tools/probe/time_map_update.py as the baseline."""

import numpy as np

from oracle import gc_oracle as O

import mapupdate_restatement as MR


class _Res:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def dropin_map_update(dm, assoc, meas, active_tile_ids, pose, timestamp, scan_seq, cfg=None, maintenance=True):
    """dm: DevicePrimitiveMap (updated in place). assoc / meas: dicts of host arrays. Returns the counters
    and plan arrays under the names of PrimitiveMapUpdateResult."""
    from gcslam.association import block_associations_for_fuse
    from gcslam.primitive_map import (primitive_map_cull, primitive_map_forget, primitive_map_fuse,
                                      primitive_map_insert_masked, primitive_map_merge_reduce)
    c = dict(MR.DEFAULTS, **(cfg or {}))
    active = [int(t) for t in active_tile_ids]
    dense = [dm.dense_tile(t) for t in active]
    K = assoc["responsibilities"].shape[1]
    out = dict(n_fused=0, n_inserted=0, n_culled=0, n_merged=0, fused_mass_total=0.0, evicted_mass_total=0.0)
    res = _Res(**assoc)
    idx_b, tile_b, slot_b, resp_b, valid_b = block_associations_for_fuse(res, meas["valid_mask"], c["block_size"])
    for b in range(idx_b.shape[0]):
        idx = idx_b[b]
        tids, target, r = tile_b[b].reshape(-1), slot_b[b].reshape(-1), resp_b[b].reshape(-1)
        vflat = np.repeat(valid_b[b], K)
        rows = [np.repeat(np.asarray(meas[k])[idx], K, axis=0) for k in ("Lambdas", "thetas", "etas", "weights",
                                                                         "colors", "sources")]
        for tid, d in zip(active, dense):
            vt = vflat & (tids == tid)
            out["fused_mass_total"] += float(np.sum(rows[3] * r * vt.astype(np.float64)))
            fr, _, _ = primitive_map_fuse(dm, d, target, rows[0], rows[1], rows[2], rows[3], r, timestamp, scan_seq,
                                          valid_mask=vt, colors_meas=rows[4], sources_meas=rows[5],
                                          eps_mass=c["eps_mass"], world_pose=pose, eps_lift=c["eps_lift"])
            out["n_fused"] += fr.n_fused
    plan = MR.insert_plan(assoc, meas, active, pose, c)
    out["insert_mass_total"], out["insert_mass_p95"] = plan["insert_mass_total"], plan["insert_mass_p95"]
    slots, ids = [], []
    for d, ins_idx, valid_new, w_ins in zip(dense, plan["indices"], plan["valid_new"], plan["weights_ins"]):
        Lw, tw, ew = O.transform_gaussian_to_world(meas["Lambdas"][ins_idx], meas["thetas"][ins_idx],
                                                   meas["etas"][ins_idx], np.asarray(pose, np.float64), c["eps_lift"])
        ir, _, _ = primitive_map_insert_masked(dm, d, Lw, tw, ew, w_ins, timestamp, valid_new, scan_seq,
                                               c["recency_decay_lambda"], colors_new=meas["colors"][ins_idx],
                                               sources_new=meas["sources"][ins_idx])
        out["n_inserted"] += ir.n_inserted
        slots.append(ir.target_slots)
        ids.append(ir.new_ids)
    if maintenance:
        for d in dense:
            cr, _, _ = primitive_map_cull(dm, d, c["primitive_cull_weight_threshold"])
            out["n_culled"] += cr.n_culled
            out["evicted_mass_total"] += cr.mass_dropped
            primitive_map_forget(dm, d, c["primitive_forgetting_factor"])
            mr, _, _ = primitive_map_merge_reduce(dm, d, c["primitive_merge_threshold"], int(c["k_merge_pairs_tile"]),
                                                  int(c["max_tile_size"]), c["eps_psd"], c["eps_lift"])
            out["n_merged"] += mr.n_merged
    shape = (len(active), int(c["k_insert_tile"]))
    out.update(insert_indices=np.asarray(plan["indices"], np.int32).reshape(shape),
               insert_valid=np.asarray(plan["valid_new"], bool).reshape(shape),
               insert_target_slots=np.asarray(slots, np.int32).reshape(shape),
               new_ids=np.asarray(ids, np.int64).reshape(shape))
    return out
