"""Inputs of the VisualPoseEvidence tests, built on the CPU alone: a hex-tiled map, the oracle's
map view and OT association of a measurement batch with it (the pattern of test_association.py),
and H linearisation poses. The device tests feed the operator these association arrays, so both
sides see the same inputs.

Each case has one responsibility row zeroed after the association (s_i = 0), hypothesis 0 with
rotvec = 0, and — where the row count allows — invalid rows. The seeds are picked so that the
conditions under which the rotation outputs are well determined hold (check_conditions; the
comparison of an SVD's U Vᵀ needs separated, non-zero singular values, and so3_log a rotation
away from π). test_visual_pose.py asserts them for every case without a GPU."""

import numpy as np

from oracle import gc_oracle as O
from test_association import _hex_map, _meas

import vpe_restatement as VR

L = 3

#          N    K  cells                                              m_tile n_valid view H  seed
CASES = {
    "smallest": (1, 1, [(0, 0, 0)], 8, 8, 8, 1, 1),
    "ragged": (70, 8, [(0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0)], 64, 60, 32, 3, 5),
    "multi_wg": (300, 8, [(a, b, 0) for a in range(-2, 3) for b in range(-2, 3)], 64, 60, 32, 5, 3),
}
# "smallest": one row and one candidate give a rank-one scatter, so S's conditions cannot hold there
# (see test_gpu_visual_pose.py); its single row is kept non-zero and the zeroed row is a second variant.
_cache = {}


def build(name, seed=None):
    """dict(tiles, ids, m_tile, m_view, view, meas, assoc, poses, zero_row) — computed once per case
    and shared; callers must not modify it."""
    key = (name, seed)
    if key in _cache:
        return _cache[key]
    N, K, cells, m_tile, n_valid, m_view, H, seed0 = CASES[name]
    rng = np.random.default_rng(seed0 if seed is None else seed)
    tiles = _hex_map(rng, m_tile, n_valid, cells)
    ids = list(tiles)
    view = O.extract_atlas_map_view(tiles, ids, m_view, m_tile)
    lo = 2.0 * min(c[0] for c in cells)
    hi = 2.0 * (max(c[0] for c in cells) + 1)
    meas = _meas(rng, N, lo, hi)
    meas["valid_mask"][:] = True
    zero_row = None
    if name == "ragged":  # one invalid row in each of the 8 row positions of a wave (i % 8 = 0..7)
        meas["valid_mask"][[9 * p for p in range(8)]] = False
        zero_row = 5
    elif name == "multi_wg":
        meas["valid_mask"][rng.uniform(0, 1, N) > 0.85] = False
        meas["valid_mask"][100] = True
        zero_row = 100
    res, _ = O.associate_primitives_ot(meas, view, dict(k_assoc=K, scan_seq=9))
    assoc = {k: np.array(res[k]) for k in ("responsibilities", "candidate_pool_indices", "row_masses")}
    if zero_row is not None:
        assoc["responsibilities"][zero_row] = 0.0
    poses = np.zeros((H, 6))
    poses[:, :3] = rng.normal(size=(H, 3)) * 0.3
    poses[1:, 3:] = rng.normal(size=(H - 1, 3)) * 0.15  # hypothesis 0 keeps rotvec = 0
    out = dict(tiles=tiles, ids=ids, m_tile=m_tile, m_view=m_view, view=view, meas=meas, assoc=assoc, poses=poses,
               zero_row=zero_row, N=N, K=K, H=H)
    _cache[key] = out
    return out


def reference(case):
    """The restatement's result for every hypothesis of a case (computed once)."""
    if "ref" not in case:
        case["ref"] = [VR.visual_pose_evidence(case["assoc"], case["meas"], case["view"], p) for p in case["poses"]]
    return case["ref"]


def conditions(ref):
    """(s3/s1, smallest pairwise relative singular-value gap, ‖so3_log(R_sc Rᵀ)‖) of one result."""
    s = ref["sing"]
    gap = min((s[0] - s[1]) / s[0], (s[1] - s[2]) / s[0], (s[0] - s[2]) / s[0])
    return s[2] / s[0], gap, float(np.linalg.norm(ref["rotvec_delta"]))


def check_conditions(refs):
    for r in refs:
        ratio, gap, ang = conditions(r)
        assert ratio >= 1e-2 and gap >= 1e-2 and ang <= 2.0, (ratio, gap, ang)


def mirrored(case):
    """The case with every measurement lobe mirrored in z: S -> S diag(1, 1, -1), so det S changes sign
    (same singular values). Returns whichever of the two has det(U Vᵀ) < 0."""
    if reference(case)[0]["reflected"]:
        return case
    m = dict(case)
    m.pop("ref", None)
    m["meas"] = dict(case["meas"], etas=case["meas"]["etas"] * np.array([1.0, 1.0, -1.0]))
    return m
