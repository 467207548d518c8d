"""LiDAR surfel extraction, the CPU side: the NumPy restatement (tests/surfel_restatement.py; the
reference ships only a property test for this operator: "parity unpinned") checked against that
property test and against the bucket's ordering rules, the preconditions of the GPU comparison for
every case (tests/surfel_cases.py), and the operator's argument errors, which must be raised before
any device is touched."""

import numpy as np
import pytest

from gcslam import _abi
from gcslam.measurement_batch import BATCH_ARRAYS
from gcslam.ops import (MeasurementBatch, SurfelExtractionConfig, create_empty_measurement_batch,
                        extract_lidar_surfels)

import surfel_cases as SC
import surfel_restatement as SR


def test_restatement_passes_the_reference_property_test():
    """test/test_lidar_surfel_extraction_mahex3d.py:46-61 on its own inputs."""
    r = SC.reference("smoke")
    assert r["n_surfel"] == 8 and r["n_feat"] == 4
    assert 0 <= r["n_lidar_valid"] <= r["n_surfel"]
    lidar = slice(r["n_feat"], r["n_feat"] + r["n_surfel"])
    assert int(r["valid_mask"][lidar].sum()) == r["n_lidar_valid"]
    assert r["n_lidar_valid"] > 0  # two tight clusters, a coarse grid: at least one cell is valid
    assert np.all(np.isfinite(r["Lambdas"][lidar][:r["n_lidar_valid"]]))
    assert np.all(np.isfinite(r["weights"][lidar][:r["n_lidar_valid"]]))
    assert not r["valid_mask"][:r["n_feat"]].any() and r["n_camera_valid"] == 0


def test_restatement_keeps_lowest_indices_in_ascending_cells():
    c, r = SC.build("overflow_truncate"), SC.reference("overflow_truncate")
    cfg = dict(SR.DEFAULTS, **c["cfg"])
    max_occ, n1, n2, nz = (cfg[k] for k in ("hex3d_max_occupants", "hex3d_num_cells_1", "hex3d_num_cells_2",
                                             "hex3d_num_cells_z"))
    # cell of every unmasked point, straight from the definition (floor, then Python's floor-mod)
    sc = np.floor(SR.hex_coords(c["points"] - r["center"], cfg["voxel_size_m"]))
    lin = np.array([(int(a) % n1) * n2 * nz + (int(b) % n2) * nz + (int(z) % nz) if m else -1
                    for (a, b, z), m in zip(sc, r["mask"])])
    assert (lin[r["mask"]] >= 0).all() and (sc[r["mask"]] < 0).any()  # negative cells wrap to non-negative ones
    overflowed = 0
    for cell in range(n1 * n2 * nz):
        members = np.flatnonzero(lin == cell)  # ascending point index
        assert r["count"][cell] == len(members) and r["count_used"][cell] == min(len(members), max_occ)
        kept = r["bucket"][cell][r["bucket"][cell] >= 0]
        np.testing.assert_array_equal(kept, members[:max_occ])
        overflowed += len(members) > max_occ
    assert overflowed >= 64  # about half of the 256 cells
    assert not r["mask"][::97].any() and r["mask"].sum() == len(lin) - len(lin[::97])
    # slots: ascending cell id, the first n_surfel valid cells, more valid cells than budget
    assert r["cell_valid"].sum() > cfg["n_surfel"] == r["n_lidar_valid"]
    np.testing.assert_array_equal(r["slot_cells"], np.flatnonzero(r["cell_valid"])[:cfg["n_surfel"]])
    assert (np.diff(r["slot_cells"]) > 0).all()


@pytest.mark.parametrize("name", SC.NAMES)
def test_case_preconditions(name):
    r = SC.reference(name)
    s = SC.check_conditions(r)
    if name == "default_grid":  # fewer valid cells than budget: the padded tail is exercised
        assert 0 < s["valid"] < r["n_surfel"] and s["overflow"] > 0
        tail = slice(r["n_feat"] + r["n_lidar_valid"], r["n_feat"] + r["n_surfel"])
        assert not r["valid_mask"][tail].any() and not r["Lambdas"][tail].any()
    if name == "kappa_open":  # κ is not pinned at kappa_max
        k = r["kappas"]
        assert ((k > 0.1) & (k < 100.0)).sum() >= 0.9 * len(k)
    if name.startswith("empty"):
        assert r["n_lidar_valid"] == 0 and not r["valid_mask"].any() and not r["Lambdas"].any()
        assert all(np.all(np.isfinite(r[k])) for k in ("Lambdas", "thetas", "etas", "weights", "colors"))


def test_restatement_base_batch_is_carried_over():
    c = SC.build("smoke")
    plain = SC.reference("smoke")
    rng = np.random.default_rng(1)
    n_total = plain["n_feat"] + plain["n_surfel"]
    base = {k: rng.uniform(0.1, 1.0, (n_total,) + shp).astype(dt) for k, (shp, dt, _) in BATCH_ARRAYS.items()}
    base["n_camera_valid"] = 3
    r = SR.extract(c["points"], c["timestamps"], c["weights"], c["cfg"], base=base)
    nf, nv = plain["n_feat"], plain["n_lidar_valid"]
    for k in BATCH_ARRAYS:
        np.testing.assert_array_equal(r[k][:nf], base[k][:nf])
        np.testing.assert_array_equal(r[k][nf:nf + nv], plain[k][nf:nf + nv])
        np.testing.assert_array_equal(r[k][nf + nv:], base[k][nf + nv:])  # the tail keeps the base's values
    assert r["n_camera_valid"] == 3 and r["n_lidar_valid"] == nv


def test_create_empty_measurement_batch():
    from gcslam.constants import GC_N_FEAT, GC_N_SURFEL, GC_NONFINITE_SENTINEL, GC_VMF_N_LOBES
    assert (GC_N_FEAT, GC_N_SURFEL, GC_VMF_N_LOBES, GC_NONFINITE_SENTINEL) == (512, 1024, 3, 1e6)
    b = create_empty_measurement_batch()
    assert isinstance(b, MeasurementBatch) and (b.n_feat, b.n_surfel, b.n_total, b.n_valid) == (512, 1024, 1536, 0)
    b = create_empty_measurement_batch(n_feat=4, n_surfel=8)
    want = dict(Lambdas=((12, 3, 3), np.float64), thetas=((12, 3), np.float64), etas=((12, 3, 3), np.float64),
                weights=((12,), np.float64), sources=((12,), np.int32), source_indices=((12,), np.int32),
                valid_mask=((12,), np.bool_), timestamps=((12,), np.float64), colors=((12, 3), np.float64))
    for k, (shp, dt) in want.items():
        a = getattr(b, k)
        assert a.shape == shp and a.dtype == dt and not a.any(), k
    assert b.camera_slice == slice(0, 4) and b.lidar_slice == slice(4, 12)
    assert b.n_camera_valid == 0 and b.n_lidar_valid == 0 and b.device is None
    b.n_camera_valid, b.n_lidar_valid = 2, 5
    assert b.n_valid == 7


def test_argument_errors_need_no_device(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("a device context was requested before the arguments were checked")

    monkeypatch.setattr(_abi, "default_context", no_device)
    monkeypatch.setattr(_abi, "call", no_device)
    p, t, w = np.zeros((10, 3)), np.zeros(10), np.ones(10)
    C = SurfelExtractionConfig
    with pytest.raises(ValueError, match="match"):
        extract_lidar_surfels(p, t[:9], w)
    with pytest.raises(ValueError, match="match"):
        extract_lidar_surfels(p, t, w[:3])
    with pytest.raises(ValueError, match="rows of 3"):
        extract_lidar_surfels(np.zeros(10), t, w)
    for field in ("hex3d_num_cells_1", "hex3d_num_cells_2", "hex3d_num_cells_z"):
        for bad in (0, -2):
            with pytest.raises(ValueError, match="grid"):
                extract_lidar_surfels(p, t, w, C(**{field: bad}))
    with pytest.raises(ValueError, match="cells"):
        extract_lidar_surfels(p, t, w, C(hex3d_num_cells_1=64, hex3d_num_cells_2=64, hex3d_num_cells_z=8))
    for bad in (0, -1):
        with pytest.raises(ValueError, match="n_surfel"):
            extract_lidar_surfels(p, t, w, C(n_surfel=bad))
    for bad in (0.0, -0.1, float("nan")):
        with pytest.raises(ValueError, match="voxel_size_m"):
            extract_lidar_surfels(p, t, w, C(voxel_size_m=bad))
    with pytest.raises(ValueError, match="too small"):
        extract_lidar_surfels(p, t, w, C(voxel_size_m=2e5 / 2.0 ** 31))
    for bad in (0, -3, _abi.GC_SURFEL_MAX_OCCUPANTS + 1):
        with pytest.raises(ValueError, match=r"hex3d_max_occupants must be in \[1, 1024\]"):
            extract_lidar_surfels(p, t, w, C(hex3d_max_occupants=bad))
    with pytest.raises(ValueError, match="base_batch"):
        extract_lidar_surfels(p, t, w, C(n_feat=4, n_surfel=8), base_batch=create_empty_measurement_batch(4, 16))
    with pytest.raises(ValueError, match="base_batch"):
        extract_lidar_surfels(p, t, w, C(n_feat=4, n_surfel=8), base_batch=create_empty_measurement_batch(2, 8))
    # the reference's names and defaults (lidar_surfel_extraction.py:43-62)
    assert C().__dict__ == dict(SR.DEFAULTS)
