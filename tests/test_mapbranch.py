"""The map branch's host side without a GPU: the NumPy restatement of the candidate statistics
(tests/mapbranch_restatement.py, backend/pipeline.py:879-905) on hand-made cases, the names the device
operator returns them under, and MapBranchConfig against the reference's defaults."""

import numpy as np
import pytest

import mapbranch_restatement as MB


@pytest.mark.parametrize("name", list(MB.HAND))
def test_restatement_on_hand_made_cases(name):
    case, want = MB.HAND[name]
    got = MB.expected(case)
    assert tuple(got[k] for k in MB.NAMES) == want, (name, got)


def test_restatement_n21_p95_index_is_inside():
    """N = 21: int(0.95 * 21) = 19 is neither 0 nor N - 1. Counts are i % 5 on the 19 valid rows."""
    case = MB.CASES["n21"]
    N = case["valid_meas"].shape[0]
    assert N == 21 and int(0.95 * N) == 19
    valid = case["valid_meas"]
    counts = np.array([i % 5 for i in range(N)], np.float64)
    srt = np.sort(np.where(valid, counts, -1.0))
    assert srt[0] == srt[1] == -1.0 and srt[19] == 4.0 and srt[20] == 4.0 and srt[19 - 4] == 3.0
    got = MB.expected(case)
    assert got[MB.NAMES[2]] == 4.0
    assert got[MB.NAMES[1]] == counts[valid].sum() / 19.0
    # even rows name one tile (or none when they have no valid candidate); odd rows up to three
    distinct = []
    for i in range(N):
        t = {int(case["tiles"][i, k]) for k in range(4) if case["view_valid"][case["pool"][i, k]]}
        distinct.append(len(t))
    assert got[MB.NAMES[0]] == float(np.sum(np.array(distinct, np.float64)[valid])) / 19.0
    assert max(distinct) > 1 and min(distinct) == 0


def test_restatement_clamps_pool_indices_and_skips_tile_minus_one():
    """An index past the view reads its last entry, as a JAX gather does; a valid candidate whose tile id
    is -1 counts as a candidate and as no tile (:886-895)."""
    c = MB._case([1], [[0, 7, -3]], [[-1, 4, 4]], [1, 0, 1])
    got = MB.candidate_stats(c["valid_meas"], c["pool"], c["tiles"], c["view_valid"])
    assert tuple(got[k] for k in MB.NAMES) == (1.0, 3.0, 3.0)


def test_names_and_config_defaults():
    from gcslam.association import CANDIDATE_STATS
    from gcslam.map_branch import MapBranch, MapBranchConfig  # noqa: F401
    from gcslam.primitive_map import MapUpdateConfig
    assert CANDIDATE_STATS == MB.NAMES
    cfg = MapBranchConfig()
    # constants.py:408-436 and pipeline.py:181-207
    assert (cfg.H_TILE, cfg.N_ACTIVE_TILES, cfg.R_ACTIVE_TILES_XY, cfg.R_ACTIVE_TILES_Z) == (2.0, 7, 1, 0)
    assert (cfg.N_STENCIL_TILES, cfg.R_STENCIL_TILES_XY, cfg.R_STENCIL_TILES_Z, cfg.M_TILE_VIEW) == (7, 1, 0, 1024)
    assert (cfg.k_assoc, cfg.k_sinkhorn, cfg.ot_epsilon, cfg.ot_tau_a, cfg.ot_tau_b) == (8, 50, 0.1, 0.5, 0.5)
    assert (cfg.RECENCY_DECAY_LAMBDA, cfg.RECENCY_MIN_SCALE, cfg.eps_lift, cfg.eps_mass) == (0.02, 0.05, 1e-9, 1e-12)
    assert isinstance(cfg.map_update, MapUpdateConfig) and cfg.map_update is not MapBranchConfig().map_update
    a = cfg.association_config(17)
    assert (a.k_assoc, a.k_sinkhorn, a.epsilon, a.tau_a, a.tau_b, a.h_tile, a.scan_seq) == (8, 50, 0.1, 0.5, 0.5, 2.0, 17)
    assert (a.r_stencil_tiles_xy, a.r_stencil_tiles_z, a.recency_decay_lambda, a.eps_mass) == (1, 0, 0.02, 1e-12)


def test_new_entries_are_bound():
    from gcslam import _abi
    for name in ("gc_primitive_map_tile_export", "gc_primitive_map_tile_import", "gc_primitive_map_tile_reset",
                 "gc_primitive_map_recency_inflate_tiles", "gc_association_candidate_stats"):
        assert name in _abi.SIGNATURES, name
