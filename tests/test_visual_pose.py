"""VisualPoseEvidence without a GPU: self-checks of the NumPy restatement (tests/vpe_restatement.py,
visual_pose_evidence.py:261-436 — the reference ships no vectors for this operator, so parity is
pinned by the restatement: "parity unpinned"), the conditions the device cases rely on, and the
wrapper's host-side index validation."""

import os

import numpy as np
import pytest

from oracle import gc_oracle as O

import vpe_cases as VC
import vpe_restatement as VR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "fl-slam_amd", "gcslam", "libgcslam.so")


def _posed_scene(rng, n, pose0, mirror=False):
    """n map primitives and one measurement each: the map primitive seen from pose0 = [t0, rotvec0]
    (m_i = R0ᵀ(c_i − t0), μ_i = R0ᵀ d_i), associated one to one with π = 1. With mirror, the
    measurement lobes are reflected in z, so the scatter has a negative determinant."""
    R0, t0 = O.so3_exp(pose0[3:]), pose0[:3]
    c = rng.uniform(-3.0, 3.0, (n, 3))
    eta = rng.normal(size=(n, 3, 3)) * np.array([3.0, 2.0, 1.0])  # anisotropic: separated singular values
    view = dict(positions=c, directions=None, kappas=None, valid_mask=np.ones(n, bool))
    es = eta.sum(axis=1)
    view["kappas"] = np.linalg.norm(es, axis=1)
    view["directions"] = es / (view["kappas"][:, None] + O.EPS_MASS)
    B = rng.normal(size=(n, 3, 3)) * 0.3
    Lam = B @ np.swapaxes(B, 1, 2) + 2.0 * np.eye(3)
    m = (c - t0) @ R0  # rows R0ᵀ (c − t0)
    meta = eta @ R0    # each lobe R0ᵀ η
    if mirror:
        meta = meta * np.array([1.0, 1.0, -1.0])
    meas = dict(Lambdas=Lam, thetas=np.einsum("nij,nj->ni", Lam, m), etas=meta, valid_mask=np.ones(n, bool))
    assoc = dict(responsibilities=np.ones((n, 1)), candidate_pool_indices=np.arange(n, dtype=np.int32)[:, None],
                 row_masses=np.ones(n))
    return assoc, meas, view


def test_restatement_recovers_known_pose():
    rng = np.random.default_rng(0)
    pose0 = np.array([0.4, -0.7, 0.2, 0.3, -0.2, 0.5])
    assoc, meas, view = _posed_scene(rng, 40, pose0)
    r = VR.visual_pose_evidence(assoc, meas, view, pose0)
    # at the true rotation the WLS optimum is t0 and the scatter's polar factor is R0
    np.testing.assert_allclose(np.linalg.solve(r["L_trans"], r["h_trans"]), pose0[:3], rtol=0, atol=1e-7)
    np.testing.assert_allclose(r["R_scatter"], O.so3_exp(pose0[3:]), rtol=0, atol=1e-9)
    assert np.linalg.norm(r["rotvec_delta"]) < 1e-9 and np.linalg.norm(r["h_rot"]) < 1e-7
    assert r["cost_trans"] < 1e-12 and abs(r["cost_rot"]) < 1e-9 * r["W"] and not r["reflected"]
    # linearised elsewhere, h_rot points from the linearisation rotation to R0
    lin = pose0 + np.array([0.0, 0.0, 0.0, 0.1, 0.05, -0.08])
    r2 = VR.visual_pose_evidence(assoc, meas, view, lin)
    np.testing.assert_allclose(O.so3_exp(r2["rotvec_delta"]) @ O.so3_exp(lin[3:]), O.so3_exp(pose0[3:]), atol=1e-9)
    assert r2["n_associations"] == 40 and r2["mean_transported_mass"] == 1.0 and r2["sum_row_masses"] == 40.0
    assert np.array_equal(r2["L_pose"][6:, 6:], O.EPS_LIFT * np.eye(16)) and not r2["h_pose"][6:].any()
    assert np.array_equal(r2["L_pose"][3:6, 3:6], r2["L_rot"]) and np.array_equal(r2["h_pose"][:3], r2["h_trans"])


def test_restatement_empty_branch():
    rng = np.random.default_rng(1)
    assoc, meas, view = _posed_scene(rng, 6, np.zeros(6))
    for kill in ("meas", "view"):
        m, v = dict(meas), dict(view)
        if kill == "meas":
            m["valid_mask"] = np.zeros(6, bool)
        else:
            v["valid_mask"] = np.zeros(6, bool)
        r = VR.visual_pose_evidence(assoc, m, v, np.zeros(6))
        assert r["empty"] and np.array_equal(r["L_pose"], O.EPS_LIFT * np.eye(22)) and not r["h_pose"].any()
        assert r["n_associations"] == 0 and r["total_weighted_cost"] == 0.0 and not r["L_trans"].any()


def test_restatement_reflection_branch():
    rng = np.random.default_rng(2)
    pose0 = np.array([0.1, 0.2, -0.3, 0.2, 0.1, -0.4])
    assoc, meas, view = _posed_scene(rng, 40, pose0, mirror=True)
    r = VR.visual_pose_evidence(assoc, meas, view, pose0)
    assert r["reflected"] and np.linalg.det(r["S"]) < 0
    Rs = r["R_scatter"]
    np.testing.assert_allclose(Rs @ Rs.T, np.eye(3), atol=1e-12)
    assert abs(np.linalg.det(Rs) - 1.0) < 1e-12  # a proper rotation after the diag(1, 1, -1) fix
    # the fixed factor maximises ⟨R, S⟩ over proper rotations: no worse than R0, I or random ones
    for R in [O.so3_exp(pose0[3:]), np.eye(3)] + [O.so3_exp(w) for w in rng.normal(size=(20, 3))]:
        assert np.trace(Rs.T @ r["S"]) >= np.trace(R.T @ r["S"]) - 1e-12


@pytest.mark.parametrize("name", ["ragged", "multi_wg"])
def test_device_case_inputs_meet_conditions(name):
    case = VC.build(name)
    VC.check_conditions(VC.reference(case))
    assert not case["assoc"]["responsibilities"][case["zero_row"]].any() and case["meas"]["valid_mask"][case["zero_row"]]
    assert not case["poses"][0, 3:].any()
    if name == "ragged":
        bad = np.where(~case["meas"]["valid_mask"])[0]
        assert sorted(bad % 8) == list(range(8)) and case["N"] % 8 != 0
    m = VC.mirrored(VC.build("ragged"))
    assert VC.reference(m)[0]["reflected"]
    VC.check_conditions(VC.reference(m))


def test_smallest_case_is_rank_one():
    r = VC.reference(VC.build("smallest"))[0]
    assert r["sing"][0] > 0 and r["sing"][1] < 1e-12 * r["sing"][0]


@pytest.mark.skipif(not os.path.exists(LIB), reason="libgcslam.so not built")
def test_wrapper_rejects_out_of_range_pool_index():
    from gcslam.ops import visual_pose_evidence, visual_pose_evidence_batched

    class View:  # no context: a launch, an upload or an allocation would fail on it
        ctx, count = None, 8

    class Batch:
        Lambdas, thetas = np.tile(np.eye(3), (2, 1, 1)), np.zeros((2, 3))
        etas, valid_mask = np.ones((2, 3, 3)), np.ones(2, bool)

    class Assoc:
        responsibilities = np.full((2, 2), 0.25)
        candidate_pool_indices = np.array([[0, 7], [3, 8]], np.int32)
        row_masses = np.full(2, 0.5)
        device = None

    with pytest.raises(ValueError, match="outside the view"):
        visual_pose_evidence(Assoc, Batch, View, None, z_lin_pose=np.zeros(6))
    Assoc.candidate_pool_indices = np.array([[0, 7], [-1, 2]], np.int32)
    with pytest.raises(ValueError, match="outside the view"):
        visual_pose_evidence_batched(Assoc, Batch, View, np.zeros((3, 6)))
