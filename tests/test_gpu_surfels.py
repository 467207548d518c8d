"""LiDAR surfel extraction on the device (gc_surfel.hip, gcslam/ops/lidar_surfel_extraction.py)
against the NumPy restatement of lidar_surfel_extraction.py:69-331 (tests/surfel_restatement.py; the
reference ships no vectors for this operator: "parity unpinned"). The cases and the preconditions
asserted on the restatement alone are in tests/surfel_cases.py. Floating-point outputs are compared
at 1e-10 relative to the array's max-abs (the _cmp convention of test_association.py, as
test_gpu_visual_pose.py uses it); counts, masks, indices and the slot -> cell mapping exactly.

The normal of a cell is an eigenvector: it is determined only where the two smallest eigenvalues
are separated, its sign only where n_z is away from 0, and the in-plane basis only where |n_z| is away
from 0.9. Lambdas, thetas, etas and colors are therefore compared on the orientation-determined slots
(surfel_cases.py); weights, timestamps and the position solve(Λ + eps_lift I, θ) on every valid slot."""

import numpy as np
import pytest

from gcslam import _abi
from gcslam.certificates import InfluenceCert
from gcslam.measurement_batch import BATCH_ARRAYS
from gcslam.ops import (MeasurementBatch, SurfelExtractionConfig, create_empty_measurement_batch,
                        extract_lidar_surfels)
from oracle import gc_oracle as O
from test_association import _cmp, _device_map, _hex_map

import surfel_cases as SC

RTOL = 1e-10
TRIGGERS = ["ma_hex3d_binning", "plane_fit_batched", "wishart_regularization"]


class _Obj:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def _run(ctx, name, **kw):
    c = SC.build(name)
    return extract_lidar_surfels(c["points"], c["timestamps"], c["weights"], SurfelExtractionConfig(**c["cfg"]),
                                 ctx=ctx, **kw)


def _same(a: MeasurementBatch, b: MeasurementBatch):
    for k in BATCH_ARRAYS:
        x, y = np.asarray(getattr(a, k)), np.asarray(getattr(b, k))
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), k
    assert (a.n_feat, a.n_surfel, a.n_camera_valid, a.n_lidar_valid) == (b.n_feat, b.n_surfel, b.n_camera_valid,
                                                                         b.n_lidar_valid)


def _check_cert(cert, eff, n_use, n_surfel, anchor="surfel_extraction"):
    assert not cert.exact and cert.approximation_triggers == TRIGGERS and not cert.frobenius_applied
    assert cert.chart_id == "GC-RIGHT-01" and cert.anchor_id == anchor
    assert cert.support.ess_total == float(n_use) and cert.support.support_frac == n_use / max(n_surfel, 1)
    assert cert.influence == InfluenceCert.identity()
    assert eff.objective_name == "surfel_extraction" and eff.predicted == eff.realized == float(n_use)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["smoke", "overflow_truncate", "default_grid", "kappa_open"])
def test_gpu_surfels_match_restatement(ctx, name):
    ref = SC.reference(name)
    SC.check_conditions(ref)
    batch, cert, eff = _run(ctx, name)
    nf, ns, nv = ref["n_feat"], ref["n_surfel"], ref["n_lidar_valid"]
    assert isinstance(batch, MeasurementBatch) and batch.device is None
    assert (batch.n_feat, batch.n_surfel, batch.n_camera_valid, batch.n_lidar_valid) == (nf, ns, 0, nv)
    assert batch.n_total == nf + ns and batch.n_valid == nv and nv > 0
    for k, (shp, dt, _) in BATCH_ARRAYS.items():
        a = getattr(batch, k)
        assert a.shape == (nf + ns,) + shp and a.dtype == dt, k
    # exact: the mask, the sources, the indices, which cell every slot came from
    _cmp(batch.__dict__, {k: ref[k] for k in ("valid_mask", "sources", "source_indices")},
         ("valid_mask", "sources", "source_indices"), 0.0)
    np.testing.assert_array_equal(batch.lidar_slot_cells[:nv], ref["slot_cells"])
    assert (batch.lidar_slot_cells[nv:] == -1).all() and batch.lidar_slot_cells.shape == (ns,)
    rows = slice(nf, nf + nv)
    # every valid slot: weight, timestamp, position
    _cmp({k: getattr(batch, k)[rows] for k in ("weights", "timestamps")},
         {k: ref[k][rows] for k in ("weights", "timestamps")}, (), RTOL)
    pos = np.linalg.solve(batch.Lambdas[rows] + O.EPS_LIFT * np.eye(3)[None], batch.thetas[rows][..., None])[..., 0]
    _cmp(dict(positions=pos), dict(positions=ref["positions"]), (), RTOL)
    # orientation-determined slots: everything that depends on the normal
    det = ref["slot_determined"]
    assert det.sum() >= 0.98 * nv - 1
    _cmp({k: getattr(batch, k)[rows][det] for k in ("Lambdas", "thetas", "etas", "colors")},
         {k: ref[k][rows][det] for k in ("Lambdas", "thetas", "etas", "colors")}, (), RTOL)
    assert not batch.etas[rows, 1:].any()
    if name == "kappa_open":  # κ = ‖η₀‖ does not depend on the normal's direction: every valid slot
        kap = np.linalg.norm(batch.etas[rows, 0], axis=1)
        assert ((ref["kappas"] > 0.1) & (ref["kappas"] < 100.0)).sum() >= 0.9 * nv
        _cmp(dict(kappa=kap), dict(kappa=ref["kappas"]), (), RTOL)
    # the tail of the LiDAR slice and the whole camera slice are exactly zero
    for k in BATCH_ARRAYS:
        a = getattr(batch, k)
        assert not a[:nf].any() and not a[nf + nv:].any(), k
    _check_cert(cert, eff, nv, ns)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["empty_sentinel", "empty_weightless"])
def test_gpu_surfels_empty(ctx, name):
    ref = SC.reference(name)
    SC.check_conditions(ref)
    assert ref["n_lidar_valid"] == 0
    batch, cert, eff = _run(ctx, name)
    assert batch.n_lidar_valid == 0 and batch.n_valid == 0
    for k in BATCH_ARRAYS:
        a = getattr(batch, k)
        assert np.all(np.isfinite(a.astype(np.float64))) and not a.any(), k
    assert (batch.lidar_slot_cells == -1).all()
    _check_cert(cert, eff, 0, ref["n_surfel"])
    assert not cert.exact and cert.support.ess_total == 0.0


@pytest.mark.gpu
def test_gpu_surfels_base_batch(ctx):
    """A camera slice comes back bitwise; the LiDAR slice equals the LiDAR-only run bitwise; rows of the
    LiDAR slice past n_valid keep the base batch's values (measurement_batch.py:314-331)."""
    rng = np.random.default_rng(7)
    for name, host_base in (("overflow_truncate", True), ("smoke", False)):
        c = SC.build(name)
        cfg = SurfelExtractionConfig(**c["cfg"])
        plain, _, _ = _run(ctx, name)
        nf, nv = cfg.n_feat, plain.n_lidar_valid
        base = create_empty_measurement_batch(cfg.n_feat, cfg.n_surfel)
        upto = nf if host_base else base.n_total  # the second base also fills the LiDAR slice
        for k, (shp, dt, _) in BATCH_ARRAYS.items():
            getattr(base, k)[:upto] = rng.uniform(0.1, 5.0, (upto,) + shp).astype(dt)
        base.n_camera_valid = 3
        want = {k: getattr(base, k).copy() for k in BATCH_ARRAYS}
        if not host_base:  # the same base resident on the device
            dev = {k: _abi.DeviceArray.from_host(ctx, getattr(base, k), BATCH_ARRAYS[k][2]) for k in BATCH_ARRAYS}
            base = MeasurementBatch(**dev, n_feat=base.n_feat, n_surfel=base.n_surfel, n_camera_valid=3,
                                    n_lidar_valid=0, device=dev)
        got, cert, eff = extract_lidar_surfels(c["points"], c["timestamps"], c["weights"], cfg, base_batch=base, ctx=ctx)
        assert (got.n_camera_valid, got.n_lidar_valid, got.n_valid) == (3, nv, 3 + nv)
        for k in BATCH_ARRAYS:
            g, p = getattr(got, k), getattr(plain, k)
            assert g[:nf].tobytes() == want[k][:nf].tobytes(), k
            assert g[nf:nf + nv].tobytes() == p[nf:nf + nv].tobytes(), k
            assert g[nf + nv:].tobytes() == want[k][nf + nv:].tobytes(), k
        if not host_base:
            assert nv < cfg.n_surfel and got.weights[nf + nv:].all()  # a non-trivial tail was carried over
        _check_cert(cert, eff, nv, cfg.n_surfel)


@pytest.mark.gpu
def test_gpu_surfels_reproducible(ctx):
    c = SC.build("overflow_truncate")
    a, _, _ = _run(ctx, "overflow_truncate")
    b, _, _ = _run(ctx, "overflow_truncate")
    _same(a, b)
    dp, dt, dw = (_abi.DeviceArray.from_host(ctx, c[k]) for k in ("points", "timestamps", "weights"))
    d, _, _ = extract_lidar_surfels(dp, dt, dw, SurfelExtractionConfig(**c["cfg"]), ctx=ctx)
    _same(a, d)
    e, _, _ = extract_lidar_surfels(dp, dt, dw, SurfelExtractionConfig(**c["cfg"]), ctx=ctx, device_out=True)
    assert e.device is not None and all(isinstance(getattr(e, k), _abi.DeviceArray) for k in BATCH_ARRAYS)
    assert all(e.device[k] is getattr(e, k) for k in BATCH_ARRAYS)
    host = MeasurementBatch(**{k: e.device[k].download().astype(BATCH_ARRAYS[k][1]) for k in BATCH_ARRAYS},
                            n_feat=e.n_feat, n_surfel=e.n_surfel, n_camera_valid=0, n_lidar_valid=e.n_lidar_valid)
    _same(a, host)
    np.testing.assert_array_equal(e.lidar_slot_cells.download(), a.lidar_slot_cells)


@pytest.mark.gpu
def test_gpu_surfels_device_chain(ctx):
    """extract_lidar_surfels(device_out=True) -> associate_primitives_ot -> visual_pose_evidence with the
    batch read in HBM equals, bitwise, the same chain fed the downloaded batch as a plain host object."""
    from gcslam.association import (AssociationConfig, MeasurementMassPolicy, associate_primitives_ot,
                                    extract_atlas_map_view)
    from gcslam.ops import visual_pose_evidence
    rng = np.random.default_rng(13)
    tiles = _hex_map(rng, 64, 60, [(a, b, cz) for a in range(-1, 1) for b in range(-1, 1) for cz in (-1, 0)])
    dm = _device_map(ctx, tiles, 64)
    view = extract_atlas_map_view(dm, list(tiles), 32)
    c = SC.build("overflow_truncate")
    cfg = SurfelExtractionConfig(**c["cfg"])
    batch, _, _ = extract_lidar_surfels(c["points"], c["timestamps"], c["weights"], cfg, ctx=ctx, device_out=True)
    assert batch.device is not None and batch.n_lidar_valid == cfg.n_surfel
    host = _Obj(**{k: batch.device[k].download() for k in BATCH_ARRAYS})
    host.valid_mask = host.valid_mask.astype(bool)
    assert not hasattr(host, "device")
    acfg = AssociationConfig(scan_seq=9)
    pose = np.array([0.02, -0.01, 0.03, 0.01, -0.02, 0.015])
    out = []
    for b in (batch, host):
        res, cert, eff = associate_primitives_ot(b, view, acfg)
        assert res.device is not None and set(res.device) >= {"responsibilities", "candidate_pool_indices", "row_masses"}
        vres, vcert, _ = visual_pose_evidence(res, b, view, None, z_lin_pose=pose)
        out.append((res, cert, eff, vres, vcert))
    (ra, ca, ea, va, vca), (rb, cb, eb, vb, vcb) = out
    assert ra.responsibilities.any() and ra.row_masses.any() and not ca.exact
    for k in ("responsibilities", "candidate_pool_indices", "candidate_tile_ids", "candidate_slots", "row_masses",
              "cost_matrix"):
        assert getattr(ra, k).tobytes() == getattr(rb, k).tobytes(), k
    assert ca.to_dict() == cb.to_dict() and ea.realized == eb.realized
    for k in ("L_pose", "h_pose", "L_trans", "h_trans", "L_rot", "h_rot"):
        assert getattr(va, k).tobytes() == getattr(vb, k).tobytes(), k
    assert va.total_weighted_cost == vb.total_weighted_cost and va.n_associations == vb.n_associations > 0
    assert vca.to_dict() == vcb.to_dict() and np.all(np.isfinite(va.L_pose)) and va.h_pose[:6].any()
    # the weight-proportional masses read the batch's weights: the same from HBM as from the host
    wcfg = AssociationConfig(scan_seq=9, a_policy=MeasurementMassPolicy.WEIGHT_PROPORTIONAL)
    (rw, cw, _), (rh, ch, _) = (associate_primitives_ot(b, view, wcfg) for b in (batch, host))
    assert rw.responsibilities.tobytes() == rh.responsibilities.tobytes() and cw.to_dict() == ch.to_dict()
    assert rw.responsibilities.tobytes() != ra.responsibilities.tobytes()


@pytest.mark.gpu
def test_gpu_surfels_cert_and_effect(ctx):
    c = SC.build("smoke")
    batch, cert, eff = extract_lidar_surfels(c["points"], c["timestamps"], c["weights"],
                                             SurfelExtractionConfig(**c["cfg"]), chart_id="GC-RIGHT-01",
                                             anchor_id="test_surfel_extraction", ctx=ctx)
    # the reference's property test (test_lidar_surfel_extraction_mahex3d.py:46-61) on the device
    assert batch.n_surfel == 8 and batch.n_feat == 4 and 0 < batch.n_lidar_valid <= 8
    assert int(batch.valid_mask[batch.lidar_slice].sum()) == batch.n_lidar_valid
    assert np.all(np.isfinite(batch.Lambdas[batch.lidar_slice][:batch.n_lidar_valid]))
    assert cert.exact is False and cert.approximation_triggers
    _check_cert(cert, eff, batch.n_lidar_valid, 8, anchor="test_surfel_extraction")
    assert cert.chart_id == "GC-RIGHT-01" and cert.support.support_frac == batch.n_lidar_valid / 8
