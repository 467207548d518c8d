"""The reference's post-pose map update (backend/pipeline.py:1232-1492, step 12b) restated in NumPy
over the oracle's per-tile operators, block by block and tile by tile in the reference's own order:

    block_associations_for_fuse          operators/primitive_association.py:561-588
    transform_gaussian_to_world          pipeline.py:1248-1256        O.transform_gaussian_to_world
    the per-block, per-tile fuse         pipeline.py:1272-1327        O.primitive_map_fuse
    the novelty insert plan              pipeline.py:1331-1371        O.tile_cells_from_xyz / O.tile_ids_from_cells
    the per-tile insert                  pipeline.py:1373-1392        O.primitive_map_insert_masked
    cull, forget, merge-reduce           pipeline.py:1412-1447        O.primitive_map_cull / _forget / _merge_reduce

It does not use the device path's single flat fuse, stamp pass or rank-by-counting, so the two are
independent routes to the same map. The reference ships no test vectors for this step and JAX is
absent here: parity with the reference is pinned by this restatement ("parity unpinned" against
reference outputs), as the association's is by oracle/gc_oracle.py.

Besides the updated tiles, the counters of pipeline.py:930-937 and the plan arrays, map_update
returns the margins of its own discrete decisions (tile boundaries, eviction keys, cull and merge
thresholds), which the tests use to show that a comparison of discrete outputs is well posed."""

import numpy as np

from oracle import gc_oracle as O

DEFAULTS = dict(k_insert_tile=64, h_tile=2.0, block_size=256, eps_lift=O.EPS_LIFT, eps_mass=O.EPS_MASS,
                eps_psd=O.EPS_PSD, recency_decay_lambda=0.02, primitive_cull_weight_threshold=1e-4,
                primitive_forgetting_factor=0.995, primitive_merge_threshold=0.1, k_merge_pairs_tile=4,
                max_tile_size=2048)


def _rel_gap(a, b):
    return abs(a - b) / max(abs(a), abs(b), 1e-300)


def _merge_distances(tile, eps_lift):
    """The Bhattacharyya distances O.primitive_map_merge_reduce sorts (primitive_map.py:1908-1930), valid pairs."""
    valid = np.asarray(tile["valid_mask"], bool)
    M = valid.shape[0]
    Lr = tile["Lambdas"] + eps_lift * np.eye(3)[None]
    mu = np.linalg.solve(Lr, tile["thetas"][..., None])[..., 0]
    Sig = np.linalg.inv(Lr)
    det = np.linalg.det(Sig)
    ii, jj = np.triu_indices(M, k=1)
    keep = valid[ii] & valid[jj]
    ii, jj = ii[keep], jj[keep]
    S = 0.5 * (Sig[ii] + Sig[jj])
    Sinv = np.linalg.inv(S + eps_lift * np.eye(3)[None])
    dmu = mu[ii] - mu[jj]
    quad = 0.125 * np.einsum("ni,nij,nj->n", dmu, Sinv, dmu)
    with np.errstate(invalid="ignore", divide="ignore"):
        logt = 0.5 * np.log(np.linalg.det(S) / np.sqrt(det[ii] * det[jj] + 1e-24))
    return quad + logt


def insert_plan(assoc, meas, active, pose, c):
    """pipeline.py:1331-1371: novelty, score, the world-frame tile of every measurement, and per active
    tile the chosen rows, valid_new (after the placeholder rule) and weights_ins; the mass statistics."""
    valid = np.asarray(meas["valid_mask"], bool).reshape(-1)
    Lam, th = np.asarray(meas["Lambdas"], np.float64), np.asarray(meas["thetas"], np.float64)
    w = np.asarray(meas["weights"], np.float64)
    pose = np.asarray(pose, np.float64)
    a = valid.astype(np.float64)
    a = a / max(float(a.sum()), c["eps_mass"])
    novelty = np.maximum(a - np.asarray(assoc["row_masses"], np.float64), 0.0)
    score = novelty * w
    score = score - (1.0 - valid.astype(np.float64)) * 1e6
    k_ins = int(c["k_insert_tile"])
    R_t, t_t = O.so3_exp(pose[3:6]), pose[:3]
    mu_body = np.linalg.solve(Lam + c["eps_lift"] * np.eye(3)[None], th[..., None])[..., 0]
    mu_world = mu_body @ R_t.T + t_t[None]
    c1, c2, cz = O.tile_cells_from_xyz(mu_world, c["h_tile"])
    meas_tile_ids = O.tile_ids_from_cells(c1, c2, cz)
    h = max(float(c["h_tile"]), 1e-12)
    s = np.stack([mu_world[:, 0], mu_world[:, 0] * 0.5 + mu_world[:, 1] * (np.sqrt(3.0) * 0.5), mu_world[:, 2]],
                 axis=1) / h
    frac = np.abs(s - np.round(s))
    out = dict(novelty=novelty, score=score, meas_tile_ids=meas_tile_ids,
               margin_tile=float(frac[valid].min()) if valid.any() else np.inf, indices=[], valid_new=[],
               weights_ins=[], in_tile_counts=[], placeholder=[], chosen_invalid=0, insert_mass_total=0.0,
               insert_mass_p95=0.0)
    for tid in active:  # pipeline.py:1348-1371
        in_tile = meas_tile_ids == tid
        score_t = np.where(in_tile, score, -1e30)
        ins_idx = np.argsort(-score_t, kind="stable")[:k_ins].astype(np.int32)
        valid_new = in_tile[ins_idx] & (score_t[ins_idx] > -1e20)
        out["chosen_invalid"] += int(np.sum(valid_new & ~valid[ins_idx]))
        ph = not valid_new.any()
        if ph:
            valid_new = np.ones_like(valid_new)
        w_ins = np.where(in_tile[ins_idx], novelty[ins_idx] * w[ins_idx], 0.0)
        out["insert_mass_total"] += float(np.sum(w_ins))
        ws = np.sort(w_ins)
        out["insert_mass_p95"] = max(out["insert_mass_p95"], float(ws[min(int(0.95 * float(k_ins)), k_ins - 1)]))
        out["indices"].append(ins_idx)
        out["valid_new"].append(valid_new)
        out["weights_ins"].append(w_ins)
        out["in_tile_counts"].append(int(in_tile.sum()))
        out["placeholder"].append(ph)
    return out


def map_update(tiles, assoc, meas, active_tile_ids, pose, timestamp, scan_seq, cfg=None, next_global_id=0,
               maintenance=True):
    """tiles: {tile key: oracle tile dict} (not modified); assoc: responsibilities, candidate_tile_ids,
    candidate_slots, row_masses; meas: Lambdas, thetas, etas, weights, valid_mask, colors, sources."""
    c = dict(DEFAULTS, **(cfg or {}))
    tiles = {int(k): {f: np.array(v, copy=True) for f, v in t.items()} for k, t in tiles.items()}
    active = [int(t) for t in active_tile_ids]
    pose = np.asarray(pose, np.float64)
    resp = np.asarray(assoc["responsibilities"], np.float64)
    ctile = np.asarray(assoc["candidate_tile_ids"], np.int64)
    cslot = np.asarray(assoc["candidate_slots"], np.int64)
    N, K = resp.shape
    valid = np.asarray(meas["valid_mask"], bool).reshape(-1)
    Lam, th, et = (np.asarray(meas[k], np.float64) for k in ("Lambdas", "thetas", "etas"))
    w = np.asarray(meas["weights"], np.float64)
    col = np.asarray(meas["colors"], np.float64)
    src = np.asarray(meas["sources"], np.int32)
    out = dict(n_fused=0, n_inserted=0, n_culled=0, n_merged=0, fused_mass_total=0.0, insert_mass_total=0.0,
               insert_mass_p95=0.0, evicted_mass_total=0.0)

    # ---- fuse, block by block and tile by tile (pipeline.py:1258-1327)
    block = int(max(1, c["block_size"]))
    n_blocks = (N + block - 1) // block
    for b in range(n_blocks):
        raw = np.arange(b * block, (b + 1) * block)
        idx = np.minimum(raw, N - 1)
        valid_rows = (raw < N) & valid[idx]
        target = cslot[idx].reshape(-1)
        tids = ctile[idx].reshape(-1)
        r = (resp[idx] * valid_rows[:, None]).reshape(-1)
        vflat = np.repeat(valid_rows, K)
        wm = np.repeat(w[idx], K)
        Lw, tw, ew = O.transform_gaussian_to_world(np.repeat(Lam[idx], K, axis=0), np.repeat(th[idx], K, axis=0),
                                                   np.repeat(et[idx], K, axis=0), pose, c["eps_lift"])
        cm, sm = np.repeat(col[idx], K, axis=0), np.repeat(src[idx], K)
        for tid in active:
            vt = vflat & (tids == tid)
            out["fused_mass_total"] += float(np.sum(wm * r * vt.astype(np.float64)))
            tiles[tid], n = O.primitive_map_fuse(tiles[tid], target, Lw, tw, ew, wm, r, timestamp, scan_seq, valid=vt,
                                                 colors=cm, sources=sm, eps_mass=c["eps_mass"])
            out["n_fused"] += n

    # ---- insert (pipeline.py:1331-1392)
    plan = insert_plan(assoc, meas, active, pose, c)
    novelty, score, meas_tile_ids = plan["novelty"], plan["score"], plan["meas_tile_ids"]
    k_ins = int(c["k_insert_tile"])
    out["insert_mass_total"], out["insert_mass_p95"] = plan["insert_mass_total"], plan["insert_mass_p95"]
    plan_idx, plan_valid, plan_slots, plan_ids = [], [], [], []
    evicted_valid = 0
    margin_evict = np.inf
    next_id = int(next_global_id)
    for tid, ins_idx, valid_new, w_ins in zip(active, plan["indices"], plan["valid_new"], plan["weights_ins"]):
        Lw, tw, ew = O.transform_gaussian_to_world(Lam[ins_idx], th[ins_idx], et[ins_idx], pose, c["eps_lift"])
        tile = tiles[tid]
        # the eviction order's own margin: consecutive keys among the first k_ins + 1 (-inf ties exempt)
        key = np.where(tile["valid_mask"], tile["weights"] * O._recency_decay(scan_seq, tile["last_supported_scan_seq"],
                                                                            c["recency_decay_lambda"]), -np.inf)
        first = np.sort(key, kind="stable")[:k_ins + 1]
        for x, y in zip(first[:-1], first[1:]):
            if np.isfinite(x) or np.isfinite(y):
                margin_evict = min(margin_evict, _rel_gap(x, y) if np.isfinite(x) and np.isfinite(y) else np.inf)
        tiles[tid], n_ins, ids, slots = O.primitive_map_insert_masked(
            tile, Lw, tw, ew, w_ins, timestamp, valid_new, scan_seq, c["recency_decay_lambda"], next_id,
            colors=col[ins_idx], sources=src[ins_idx])
        evicted_valid += int(np.sum(np.asarray(tile["valid_mask"], bool)[slots[valid_new]]))
        next_id += n_ins
        out["n_inserted"] += n_ins
        plan_idx.append(ins_idx)
        plan_valid.append(valid_new)
        plan_slots.append(slots)
        plan_ids.append(ids)

    # ---- maintenance (pipeline.py:1412-1447)
    margin_cull = margin_merge = np.inf
    if maintenance:
        thr = c["primitive_cull_weight_threshold"]
        for tid in active:
            t = tiles[tid]
            vm = np.asarray(t["valid_mask"], bool)
            if vm.any():
                margin_cull = min(margin_cull, float(np.min(np.abs(t["weights"][vm] - thr)) / thr))
            t, n, mass = O.primitive_map_cull(t, thr)
            out["n_culled"] += n
            out["evicted_mass_total"] += mass
            t = O.primitive_map_forget(t, c["primitive_forgetting_factor"])
            M = t["weights"].shape[0]
            if not (int(c["max_tile_size"]) > 0 and M > int(c["max_tile_size"])):  # the budget cap (:1881-1890)
                if M >= 2 and int(np.sum(t["valid_mask"])) >= 2 and c["k_merge_pairs_tile"] > 0:
                    d = _merge_distances(t, c["eps_lift"])
                    d = d[np.isfinite(d)]
                    if d.size:
                        mt = c["primitive_merge_threshold"]
                        margin_merge = min(margin_merge, float(np.min(np.abs(d - mt)) / mt))
                t, n = O.primitive_map_merge_reduce(t, c["primitive_merge_threshold"], int(c["k_merge_pairs_tile"]),
                                                    c["eps_psd"], c["eps_lift"])
                out["n_merged"] += n
            tiles[tid] = t

    shape = (len(active), k_ins)
    out.update(tiles=tiles, next_global_id=next_id,
               insert_indices=np.asarray(plan_idx, np.int32).reshape(shape),
               insert_valid=np.asarray(plan_valid, bool).reshape(shape),
               insert_target_slots=np.asarray(plan_slots, np.int32).reshape(shape),
               new_ids=np.asarray(plan_ids, np.int64).reshape(shape),
               novelty=novelty, score=score, meas_tile_ids=meas_tile_ids, in_tile_counts=plan["in_tile_counts"],
               placeholder=plan["placeholder"], evicted_valid=evicted_valid, chosen_invalid=plan["chosen_invalid"],
               margin_tile=plan["margin_tile"], margin_evict=float(margin_evict), margin_cull=float(margin_cull),
               margin_merge=float(margin_merge))
    return out
