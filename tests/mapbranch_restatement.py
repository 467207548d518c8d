"""NumPy restatement of the candidate statistics of the reference's map branch
(backend/pipeline.py:879-905), line by line, and the hand-made cases the CPU and GPU tests share.

    cand_valid  = map_view.valid_mask[candidate_pool_indices]                  (:885)
    cand_tiles  = where(cand_valid, candidate_tile_ids, -1)                     (:886)
    cand_counts = sum(cand_valid, axis=1)                                       (:887)
    distinct    = per row, the distinct values of cand_tiles other than -1      (:889-895)
    denom       = max(sum(valid rows), eps_mass)                                (:897-898)
    means       = sum(distinct * valid) / denom, sum(cand_counts * valid) / denom   (:899-900)
    p95         = sort(where(valid, cand_counts, -1))[min(int(0.95 N), N - 1)]   (:901-905)

With no valid measurement row all three stay 0.0 (:879-884). Every sum is of small integers held in
float64, so the results are exact and the tests compare with ==."""

import numpy as np

NAMES = ("candidate_tiles_per_meas_mean", "candidate_primitives_per_meas_mean", "candidate_primitives_per_meas_p95")
EPS_MASS = 1e-12


def candidate_stats(valid_meas, pool_indices, tile_ids, view_valid, eps_mass=EPS_MASS):
    valid_meas = np.asarray(valid_meas).astype(bool).reshape(-1)
    out = dict.fromkeys(NAMES, 0.0)
    if int(np.sum(valid_meas)) <= 0:
        return out
    view_valid = np.asarray(view_valid).astype(bool).reshape(-1)
    idx = np.clip(np.asarray(pool_indices, np.int64), 0, view_valid.shape[0] - 1)  # a JAX gather clamps
    cand_valid = view_valid[idx]
    cand_tiles = np.where(cand_valid, np.asarray(tile_ids, np.int64), -1)
    cand_counts = np.sum(cand_valid.astype(np.float64), axis=1)
    srt = np.sort(cand_tiles, axis=1)
    is_new = np.concatenate([np.ones((srt.shape[0], 1), bool), srt[:, 1:] != srt[:, :-1]], axis=1)
    distinct = np.sum((is_new & (srt != -1)).astype(np.float64), axis=1)
    vf = valid_meas.astype(np.float64)
    denom = max(float(np.sum(vf)), eps_mass)
    out[NAMES[0]] = float(np.sum(distinct * vf) / denom)
    out[NAMES[1]] = float(np.sum(cand_counts * vf) / denom)
    cs = np.sort(np.where(valid_meas, cand_counts, -1.0))
    out[NAMES[2]] = float(cs[min(int(0.95 * float(cs.shape[0])), cs.shape[0] - 1)])
    return out


def _case(valid_meas, pool, tiles, view_valid):
    pool = np.asarray(pool, np.int32)
    return dict(valid_meas=np.asarray(valid_meas, bool), pool=pool.reshape(len(valid_meas), -1),
                tiles=np.asarray(tiles, np.int64).reshape(pool.shape[0], -1) if pool.size else
                np.zeros(pool.shape, np.int64), view_valid=np.asarray(view_valid, bool))


def _n21():
    """21 rows, K = 4, a view of 12 entries of which 3 are invalid: int(0.95 * 21) = 19, neither 0 nor 20.
    Row i has i % 5 valid candidates among its four; rows 3 and 17 are invalid measurements."""
    view_valid = np.ones(12, bool)
    view_valid[[2, 7, 11]] = False
    good, bad = [0, 1, 3, 4, 5, 6, 8, 9, 10], [2, 7, 11]
    pool, tiles = [], []
    for i in range(21):
        nv = min(i % 5, 4)
        pool.append([good[(i + k) % 9] if k < nv else bad[(i + k) % 3] for k in range(4)])
        tiles.append([100 + ((i * 3 + k) % 3 if i % 2 else 0) for k in range(4)])  # even rows: one tile
    valid = np.ones(21, bool)
    valid[[3, 17]] = False
    return _case(valid, pool, tiles, view_valid)


# name -> (case, expected by hand: tiles mean, primitives mean, p95)
HAND = {
    # K = 1: one valid candidate per row
    "k1": (_case([1, 1], [[0], [1]], [[5], [6]], [1, 1]), (1.0, 1.0, 1.0)),
    # all four candidates of the row share tile 9
    "one_tile": (_case([1], [[0, 1, 2, 3]], [[9, 9, 9, 9]], [1, 1, 1, 1]), (1.0, 4.0, 4.0)),
    # K distinct tiles
    "k_tiles": (_case([1], [[0, 1, 2, 3]], [[4, 3, 2, 1]], [1, 1, 1, 1]), (4.0, 4.0, 4.0)),
    # the invalid row's candidates count for nothing; sorted counts [-1, 3, 3], index min(int(2.85), 2) = 2
    "invalid_rows": (_case([1, 0, 1], [[0, 1, 2], [0, 1, 2], [0, 0, 1]], [[1, 2, 2], [7, 8, 9], [1, 1, 2]], [1, 1, 1]),
                     (2.0, 3.0, 3.0)),
    # view entries 1 and 3 invalid: row 0 keeps tiles {1, 1}, row 1 keeps none
    "invalid_view": (_case([1, 1], [[0, 1, 2, 3], [1, 3, 1, 3]], [[1, 2, 1, 3], [4, 5, 6, 7]], [1, 0, 1, 0]),
                     (0.5, 1.0, 2.0)),
    # N = 1: index min(int(0.95), 0) = 0
    "n1": (_case([1], [[0, 1]], [[3, 4]], [1, 0]), (1.0, 1.0, 1.0)),
    # no valid row: zeros, not -1
    "no_valid_row": (_case([0, 0], [[0, 1], [1, 0]], [[1, 2], [2, 1]], [1, 1]), (0.0, 0.0, 0.0)),
}
CASES = dict({k: v[0] for k, v in HAND.items()}, n21=_n21())


def expected(case, eps_mass=EPS_MASS):
    return candidate_stats(case["valid_meas"], case["pool"], case["tiles"], case["view_valid"], eps_mass)
