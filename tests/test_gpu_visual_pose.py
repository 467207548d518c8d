"""VisualPoseEvidence on the device (gc_vpe.hip, gcslam/ops/visual_pose_evidence.py) against the
NumPy restatement of visual_pose_evidence.py:261-436 (tests/vpe_restatement.py; the reference
ships no vectors for this operator: "parity unpinned"). The map and view are built as in
test_association.py — the oracle's view and association on the CPU, DevicePrimitiveMap and the
device view on the GPU — and the operator is fed the oracle's association arrays, so both sides
see the same inputs. Every output is compared at 1e-10 relative to its array's max-abs (the _cmp
convention of test_association.py); cost_rot = W − ⟨R, S⟩ is compared relative to W.

The rotation outputs compare an SVD's U Vᵀ, which is determined only for separated non-zero
singular values, so each case asserts on the restatement's own values s₃/s₁ >= 1e-2, pairwise
relative gaps >= 1e-2 and ‖so3_log(R_sc Rᵀ)‖ <= 2 before comparing. The smallest shape
(N, K, V, H) = (1, 1, 8, 1) cannot meet them: one row with one candidate gives a rank-one scatter,
so R_sc (hence h_rot) depends on the basis an SVD picks for the null space. There every other
output is compared, with the single row non-zero and again with it zeroed (s_i = 0, S = 0)."""

import numpy as np
import pytest

from oracle import gc_oracle as O
from test_association import _cmp, _device_map

import vpe_cases as VC
import vpe_restatement as VR

RTOL = 1e-10
_FIELDS = ("L_pose", "h_pose", "L_trans", "h_trans", "L_rot", "h_rot")


class _Obj:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def _device_view(ctx, case):
    from gcslam.association import extract_atlas_map_view
    if "dview" not in case:
        dm = _device_map(ctx, case["tiles"], case["m_tile"])
        case["dview"] = (extract_atlas_map_view(dm, case["ids"], case["m_view"]), dm)
    return case["dview"][0]


def _assoc(case, **over):
    from gcslam.association import PrimitiveAssociationResult
    a = dict(case["assoc"], **over)
    z = np.zeros(a["responsibilities"].shape, np.int64)
    return PrimitiveAssociationResult(a["responsibilities"], a["candidate_pool_indices"], z, z, a["row_masses"],
                                      np.zeros(a["responsibilities"].shape))


def _check_parts(parts, ref, skip=()):
    got = dict(L_trans=parts[0:9].reshape(3, 3), h_trans=parts[9:12], L_rot=parts[12:21].reshape(3, 3),
               h_rot=parts[21:24], cost_trans=parts[24])
    _cmp(got, {k: ref[k] for k in got if k not in skip}, (), RTOL)
    assert abs(parts[25] - ref["cost_rot"]) <= RTOL * max(1.0, ref["W"]), (parts[25], ref["cost_rot"], ref["W"])


def _check_result(res, cert, eff, ref, skip=()):
    _cmp(res.__dict__, {k: ref[k] for k in _FIELDS if k not in skip}, (), RTOL)
    assert res.n_associations == ref["n_associations"]
    np.testing.assert_allclose(res.mean_transported_mass, ref["mean_transported_mass"], rtol=RTOL)
    assert abs(res.total_weighted_cost - ref["total_weighted_cost"]) <= RTOL * max(1.0, ref["W"], ref["cost_trans"])
    assert not cert.exact and cert.approximation_triggers == ["linearization", "ot_soft_correspondence"]
    assert cert.frobenius_applied and cert.support.support_frac == 1.0 and cert.influence.lift_strength == O.EPS_LIFT
    np.testing.assert_allclose(cert.support.ess_total, ref["sum_row_masses"], rtol=RTOL)
    assert eff.objective_name == "visual_pose_evidence" and eff.predicted == eff.realized == res.total_weighted_cost


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ragged", "multi_wg"])
def test_gpu_visual_pose_matches_restatement(ctx, name):
    from gcslam.ops import visual_pose_evidence, visual_pose_evidence_batched
    case = VC.build(name)
    refs = VC.reference(case)
    VC.check_conditions(refs)
    assert not case["assoc"]["responsibilities"][case["zero_row"]].any() and not case["poses"][0, 3:].any()
    view, batch = _device_view(ctx, case), _Obj(**case["meas"])
    Lp, hp, parts, cv = visual_pose_evidence_batched(_assoc(case), batch, view, case["poses"])
    assert Lp.shape == (case["H"], 22, 22) and hp.shape == (case["H"], 22) and parts.shape == (case["H"], 26)
    nv = int(case["meas"]["valid_mask"].sum())
    assert cv[0] == nv and cv[1] == int(case["view"]["valid_mask"].sum())
    np.testing.assert_allclose(cv[2:], [refs[0]["sum_row_masses"], refs[0]["mean_transported_mass"]], rtol=RTOL)
    for h, ref in enumerate(refs):
        _cmp(dict(L_pose=Lp[h], h_pose=hp[h]), {k: ref[k] for k in ("L_pose", "h_pose")}, (), RTOL)
        _check_parts(parts[h], ref)
    res, cert, eff = visual_pose_evidence(_assoc(case), batch, view, None, z_lin_pose=case["poses"][1])
    _check_result(res, cert, eff, refs[1])


@pytest.mark.gpu
def test_gpu_visual_pose_smallest(ctx):
    """(N, K, V, H) = (1, 1, 8, 1): a rank-one scatter (see the module docstring) — every output but
    h_rot, with the row non-zero and with it zeroed."""
    from gcslam.ops import visual_pose_evidence
    case = VC.build("smallest")
    view, batch = _device_view(ctx, case), _Obj(**case["meas"])
    assert case["assoc"]["responsibilities"].shape == (1, 1) and view.count == 8 and case["poses"].shape == (1, 6)
    assert not case["poses"][0, 3:].any()
    skip = ("h_rot", "h_pose")
    for resp in (case["assoc"]["responsibilities"], np.zeros((1, 1))):
        a = dict(case["assoc"], responsibilities=resp)
        ref = VR.visual_pose_evidence(a, case["meas"], case["view"], case["poses"][0])
        assert ref["sing"][1] <= 1e-12 * max(ref["sing"][0], 1e-300)  # rank <= 1
        res, cert, eff = visual_pose_evidence(_assoc(case, responsibilities=resp), batch, view, None,
                                              z_lin_pose=case["poses"][0])
        _check_result(res, cert, eff, ref, skip)
        _cmp(dict(h=res.h_pose[:3]), dict(h=ref["h_pose"][:3]), (), RTOL)
        assert not res.h_pose[6:].any() and np.all(np.isfinite(res.h_pose))
        assert abs(res.total_weighted_cost - ref["total_weighted_cost"]) <= RTOL * max(1.0, ref["W"])


@pytest.mark.gpu
def test_gpu_visual_pose_reflection(ctx):
    from gcslam.ops import visual_pose_evidence_batched
    case = VC.mirrored(VC.build("ragged"))
    refs = VC.reference(case)
    assert all(r["reflected"] for r in refs)  # det(U Vᵀ) < 0: the diag(1, 1, -1) branch
    VC.check_conditions(refs)
    view = _device_view(ctx, VC.build("ragged"))
    Lp, hp, parts, _ = visual_pose_evidence_batched(_assoc(case), _Obj(**case["meas"]), view, case["poses"])
    for h, ref in enumerate(refs):
        _cmp(dict(L_pose=Lp[h], h_pose=hp[h]), {k: ref[k] for k in ("L_pose", "h_pose")}, (), RTOL)
        _check_parts(parts[h], ref)


@pytest.mark.gpu
def test_gpu_visual_pose_empty_cases(ctx):
    """All measurements invalid, and a view with no valid entry: exactly eps_lift I₂₂, zeros elsewhere,
    an exact certificate, n_associations == 0 (visual_pose_evidence.py:297-318)."""
    from gcslam.association import extract_atlas_map_view
    from gcslam.ops import visual_pose_evidence, visual_pose_evidence_batched
    case = VC.build("ragged")
    view = _device_view(ctx, case)
    dead = dict(case["meas"], valid_mask=np.zeros(case["N"], bool))
    missing = [int(O.tile_ids_from_cells(40 + i, 40, 0)) for i in range(len(case["ids"]))]  # tiles the map lacks
    empty_view = extract_atlas_map_view(case["dview"][1], missing, case["m_view"])
    assert not empty_view.download("valid_mask")["valid_mask"].any()
    for meas, v in ((dead, view), (case["meas"], empty_view)):
        res, cert, eff = visual_pose_evidence(_assoc(case), _Obj(**meas), v, None, z_lin_pose=case["poses"][1])
        assert np.array_equal(res.L_pose, O.EPS_LIFT * np.eye(22)) and not res.h_pose.any()
        assert not res.L_trans.any() and not res.h_trans.any() and not res.L_rot.any() and not res.h_rot.any()
        assert res.total_weighted_cost == 0.0 and res.n_associations == 0 and res.mean_transported_mass == 0.0
        assert cert.exact and cert.approximation_triggers == [] and eff.predicted == 0.0 and eff.realized == 0.0
        Lp, hp, parts, cv = visual_pose_evidence_batched(_assoc(case), _Obj(**meas), v, case["poses"])
        assert np.array_equal(Lp, np.broadcast_to(O.EPS_LIFT * np.eye(22), Lp.shape)) and not hp.any() and not parts.any()
        assert cv[0] == 0 or cv[1] == 0
    # no hypotheses: pass 1 alone fills the certificate vector
    Lp, hp, parts, cv = visual_pose_evidence_batched(_assoc(case), _Obj(**case["meas"]), view, np.zeros((0, 6)))
    assert Lp.shape == (0, 22, 22) and hp.shape == (0, 22) and parts.shape == (0, 26)
    ref = VC.reference(case)[0]
    assert cv[0] == int(case["meas"]["valid_mask"].sum()) and cv[1] == int(case["view"]["valid_mask"].sum())
    np.testing.assert_allclose(cv[2:], [ref["sum_row_masses"], ref["mean_transported_mass"]], rtol=RTOL)


@pytest.mark.gpu
def test_gpu_visual_pose_batched_equals_single_bitwise(ctx):
    from gcslam.ops import visual_pose_evidence, visual_pose_evidence_batched
    case = VC.build("multi_wg")
    view, batch = _device_view(ctx, case), _Obj(**case["meas"])
    out1 = visual_pose_evidence_batched(_assoc(case), batch, view, case["poses"])
    out2 = visual_pose_evidence_batched(_assoc(case), batch, view, case["poses"])
    for a, b in zip(out1, out2):
        assert np.array_equal(a, b)
    Lp, hp, parts, _ = out1
    for h in range(case["H"]):
        res, _, _ = visual_pose_evidence(_assoc(case), batch, view, None, z_lin_pose=case["poses"][h])
        assert np.array_equal(res.L_pose, Lp[h]) and np.array_equal(res.h_pose, hp[h])
        assert np.array_equal(res.L_trans.reshape(-1), parts[h, 0:9]) and np.array_equal(res.h_trans, parts[h, 9:12])
        assert np.array_equal(res.L_rot.reshape(-1), parts[h, 12:21]) and np.array_equal(res.h_rot, parts[h, 21:24])
        assert res.total_weighted_cost == float(parts[h, 24] + parts[h, 25])


@pytest.mark.gpu
def test_gpu_visual_pose_device_chain(ctx):
    """Device association -> visual pose evidence through result.device, against the oracle chain at
    1e-7 (the association's own bar is 1e-8). The host copies are poisoned after the association:
    the operator must have read the device arrays."""
    from gcslam.association import AssociationConfig, associate_primitives_ot
    from gcslam.ops import visual_pose_evidence
    case = VC.build("multi_wg")
    view, batch = _device_view(ctx, case), _Obj(**case["meas"])
    res_a, _, _ = associate_primitives_ot(batch, view, AssociationConfig(k_assoc=case["K"], scan_seq=9))
    assert res_a.device is not None and set(res_a.device) >= {"responsibilities", "candidate_pool_indices", "row_masses"}
    ores, _ = O.associate_primitives_ot(case["meas"], case["view"], dict(k_assoc=case["K"], scan_seq=9))
    np.testing.assert_array_equal(res_a.candidate_pool_indices, ores["candidate_pool_indices"])
    res_a.responsibilities[:] = np.nan
    res_a.row_masses[:] = np.nan
    res_a.candidate_pool_indices[:] = view.count + 7  # would raise ValueError if the host copy were read
    pose = case["poses"][2]
    ref = VR.visual_pose_evidence(ores, case["meas"], case["view"], pose)
    VC.check_conditions([ref])
    res, cert, eff = visual_pose_evidence(res_a, batch, view, None, z_lin_pose=pose)
    _cmp(res.__dict__, {k: ref[k] for k in _FIELDS}, (), 1e-7)
    assert abs(res.total_weighted_cost - ref["total_weighted_cost"]) <= 1e-7 * max(1.0, ref["W"], ref["cost_trans"])
    np.testing.assert_allclose(cert.support.ess_total, ref["sum_row_masses"], rtol=1e-7)
    assert res.n_associations == ref["n_associations"]


@pytest.mark.gpu
def test_gpu_visual_pose_fusion_handoff(ctx):
    """build_visual_pose_evidence_22d(result) + a synthetic L_imu_odom through info_fusion_additive
    equals the same sum fed from the restatement at 1e-10."""
    from gcslam.belief import BeliefGaussianInfo
    from gcslam.ops import build_visual_pose_evidence_22d, info_fusion_additive, visual_pose_evidence
    case = VC.build("ragged")
    view, batch = _device_view(ctx, case), _Obj(**case["meas"])
    ref = VC.reference(case)[1]
    res, _, _ = visual_pose_evidence(_assoc(case), batch, view, None, z_lin_pose=case["poses"][1])
    L_vis, h_vis = build_visual_pose_evidence_22d(res)
    assert L_vis is res.L_pose and h_vis is res.h_pose
    rng = np.random.default_rng(4)
    B = rng.normal(size=(22, 22)) * 0.2
    L_io, h_io = B @ B.T + 0.5 * np.eye(22), rng.normal(size=22)
    belief = BeliefGaussianInfo.create_identity_prior("a", 0.0, 1e-3)
    # without z_lin_pose the linearisation pose is the belief's world pose: the anchor here (h = 0)
    belief.X_anchor = case["poses"][1].copy()
    res_b, _, _ = visual_pose_evidence(_assoc(case), batch, view, belief)
    _cmp(res_b.__dict__, {k: ref[k] for k in _FIELDS}, (), RTOL)
    post, cert, _ = info_fusion_additive(belief, L_io + L_vis, h_io + h_vis, 1.0, ctx=ctx)
    post_r, _, _ = info_fusion_additive(belief, L_io + ref["L_pose"], h_io + ref["h_pose"], 1.0, ctx=ctx)
    _cmp(dict(L=post.L, h=post.h), dict(L=post_r.L, h=post_r.h), (), RTOL)
    assert np.all(np.isfinite(post.L)) and np.all(np.isfinite(post.h))
