"""gc_extract_map_view and gc_associate_primitives_ot against the oracle at the edges of
assoc_cases.py (the conditions that make the comparison fair are asserted without a GPU by
test_association_edges.py).

Per case: the view by the rules of test_gpu_map_view_matches_oracle (ids, slots, valid, primitive
ids and scan seq exact, the rest at 1e-12); candidate indices, tile ids, slots and the non-zero
counts exact; the cost matrix at 1e-10 per element, |got - ref| <= 1e-10 max(1, |ref_ij|) (the helper
of test_association.py scales its atol by the array's largest value, which near filler costs of
~100 would pass a 1e-6 relative error on a real candidate); the Sinkhorn outputs at 1e-8 as
test_gpu_association_matches_oracle applies it; invalid rows exactly zero; and
association_candidate_stats of the device result equal to the restatement on the downloaded arrays.

Largest observed |got - ref| on the MI355X (raw absolute differences; the bars are on the scaled
ones, of which the largest over all cases was 6e-4 of the cost bar and 7.5e-7 of the Sinkhorn bar).
The next change to these kernels has this baseline. defect_a/b = marginal_defect_a/b, mass =
transport_mass_total; sum_a differed only in edge1025 (5.7e-14), sum_novel only in ties (6.3e-17).
The per-field runs of lobes1 / lobes8 gave the packed runs' figures digit for digit.

    case       cost      resp      row_mass  defect_a  defect_b  mass      sum_m     ess       total_cost
    strided    1.14e-13  7.55e-15  6.77e-15  8.88e-16  1.42e-13  0         0         6.82e-13  0
    edge1025   8.88e-15  3.12e-15  4.00e-15  8.88e-16  1.42e-14  2.84e-14  5.68e-14  3.41e-13  0
    sparse     6.00e-15  5.27e-15  4.72e-15  8.88e-16  3.55e-15  0         1.42e-14  1.42e-14  2.22e-16
    ties       3.55e-15  6.25e-16  6.25e-16  1.11e-16  1.33e-15  8.88e-16  8.88e-16  0         4.44e-16
    longpool   5.33e-15  1.60e-15  8.77e-15  0         1.78e-15  0         3.55e-15  7.11e-15  0
    lobes1     2.55e-15  1.55e-15  2.55e-15  8.88e-16  0         3.55e-15  7.11e-15  2.13e-14  0
    lobes8     1.67e-15  3.00e-15  2.78e-15  4.44e-16  1.78e-15  0         3.55e-15  7.11e-15  6.66e-16
    full_view  1.78e-15  9.99e-16  1.44e-15  4.44e-16  0         0         0         8.88e-16  0
    iters0     3.55e-15  5.00e-15  7.55e-15  3.55e-15  0         0         0         0         2.66e-15
    iters1     3.55e-15  1.08e-15  1.55e-15  4.44e-16  0         0         3.55e-15  4.26e-14  6.66e-16

(ess is ~1e3 in strided and edge1025, the defects of iters0 are ~30 and ~80: their differences are a
few ulp.) Before the final pass of k_sinkhorn read u as 1 when k_sinkhorn = 0, iters0 missed every
Sinkhorn bar: the responsibilities by 1.0, the row masses by 8, the transport mass by 166.
"""

import numpy as np
import pytest

import assoc_cases as AC
import mapbranch_restatement as MR
from oracle import gc_oracle as O

_VIEW_EXACT = ("candidate_tile_ids", "candidate_slots", "valid_mask", "primitive_ids", "last_supported_scan_seq")
_RUNS = [(n, True) for n in AC.CASES] + [(n, False) for n in AC.BOTH_LAYOUTS]


class _Batch:
    def __init__(self, meas):
        self.__dict__.update(meas)


def _config(cfg, **over):
    from gcslam.association import AssociationConfig, MeasurementMassPolicy
    c = dict(O.OT_DEFAULTS, **cfg)
    c.update(over)
    return AssociationConfig(
        k_assoc=c["k_assoc"], k_sinkhorn=c["k_sinkhorn"], cost_subtract_row_min=c["cost_subtract_row_min"],
        a_policy=MeasurementMassPolicy.WEIGHT_PROPORTIONAL if c["weight_proportional"] else MeasurementMassPolicy.UNIFORM,
        r_stencil_tiles_xy=c["r_xy"], r_stencil_tiles_z=c["r_z"], scan_seq=c["scan_seq"])


def _device_map(ctx, case, packed=True):
    """The case's tiles in a map with one more, unlisted, dense tile behind them."""
    from gcslam.primitive_map import DevicePrimitiveMap
    tiles, m_tile, L = case["tiles"], case["m_tile"], case["L"]
    keys = list(tiles) + [-1]
    dm = DevicePrimitiveMap(len(keys), m_tile, n_lobes=L, ctx=ctx, packed=packed)
    dm.set_tile_keys(keys)
    empty = O.empty_tile(m_tile, L)
    full = {k: np.concatenate([tiles[kk][k] if kk in tiles else empty[k] for kk in keys]) for k in empty}
    full["valid_mask"] = full["valid_mask"].astype(np.uint8)
    dm.upload(**full)
    return dm


def _absmax(got, ref):
    return float(np.max(np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64))))


@pytest.mark.gpu
@pytest.mark.parametrize("name,packed", _RUNS, ids=[n if p else n + "-fields" for n, p in _RUNS])
def test_gpu_association_edge_case(ctx, name, packed):
    from gcslam.association import association_candidate_stats, associate_primitives_ot, extract_atlas_map_view
    case = AC.build(name)
    ref_view, ref, rc = case["view"], case["assoc"], case["cert"]
    dm = _device_map(ctx, case, packed)
    view = extract_atlas_map_view(dm, case["ids"], case["m_view"])
    got_view = view.download()
    for k, v in ref_view.items():
        if k in ("tile_ids", "m_tile_view"):
            continue
        g = got_view[k]
        if k in _VIEW_EXACT:
            np.testing.assert_array_equal(g.astype(np.asarray(v).dtype), v, err_msg=k)
        else:
            np.testing.assert_allclose(g, v, rtol=1e-12, atol=1e-12 * max(1.0, float(np.max(np.abs(v)))), err_msg=k)
    batch = _Batch(case["meas"])
    res, cert, eff = associate_primitives_ot(batch, view, _config(case["cfg"]))
    for k in ("candidate_pool_indices", "candidate_tile_ids", "candidate_slots"):
        np.testing.assert_array_equal(getattr(res, k), ref[k], err_msg=k)
    got_scal = {k: getattr(cert.ot, k) for k in AC.CERT_SCALARS}
    got_scal.update(ess=cert.support.ess_total, total_cost=eff.realized)
    # every figure first, then the bars
    excess = dict(cost=AC.cost_excess(res.cost_matrix, ref["cost_matrix"]),
                  responsibilities=AC.sinkhorn_excess(res.responsibilities, ref["responsibilities"]),
                  row_masses=AC.sinkhorn_excess(res.row_masses, ref["row_masses"]))
    excess.update(AC.sinkhorn_scalar_excesses(got_scal, rc))
    diffs = dict(cost=_absmax(res.cost_matrix, ref["cost_matrix"]),
                 responsibilities=_absmax(res.responsibilities, ref["responsibilities"]),
                 row_masses=_absmax(res.row_masses, ref["row_masses"]))
    diffs.update({k: abs(float(got_scal[k]) - float(rc[k])) for k in got_scal})
    print("\nASSOC_EDGE %s%s absdiff %s" % (name, "" if packed else "-fields",
                                           " ".join("%s=%.3g" % kv for kv in diffs.items())))
    print("ASSOC_EDGE %s%s of-bar %s" % (name, "" if packed else "-fields",
                                         " ".join("%s=%.3g" % kv for kv in excess.items())))
    assert excess["cost"] <= 1.0, excess
    assert all(v <= 1.0 for v in excess.values()), excess
    assert cert.ot.nonzero_a == rc["nonzero_a"] and cert.ot.nonzero_b == rc["nonzero_b"]
    assert cert.ot.n_iters == dict(O.OT_DEFAULTS, **case["cfg"])["k_sinkhorn"]
    invalid = ~np.asarray(case["meas"]["valid_mask"], bool)
    assert not res.responsibilities[invalid].any() and not res.candidate_pool_indices[invalid].any()
    stats = association_candidate_stats(res, batch, view)
    assert stats == MR.candidate_stats(case["meas"]["valid_mask"], res.candidate_pool_indices, res.candidate_tile_ids,
                                       got_view["valid_mask"])


@pytest.mark.gpu
def test_gpu_association_rejections_leave_the_context_usable(ctx):
    """A stencil of 185 tiles, K = 17, K = 0 and a pool smaller than K are refused; the good call after
    each still matches the oracle."""
    from gcslam.association import associate_primitives_ot, extract_atlas_map_view
    case = AC.build("iters1")
    ref = case["assoc"]
    dm = _device_map(ctx, case)
    view = extract_atlas_map_view(dm, case["ids"], case["m_view"])
    small = extract_atlas_map_view(dm, case["ids"], 4)
    batch = _Batch(case["meas"])
    bad = [(view, dict(r_xy=3, r_z=2)), (view, dict(k_assoc=17)), (view, dict(k_assoc=0)),
           (small, dict(r_xy=0, r_z=0, k_assoc=8))]
    for v, over in bad:
        with pytest.raises(ValueError):
            associate_primitives_ot(batch, v, _config(case["cfg"], **over))
        res, _, _ = associate_primitives_ot(batch, view, _config(case["cfg"]))
        np.testing.assert_array_equal(res.candidate_pool_indices, ref["candidate_pool_indices"])
        assert AC.cost_excess(res.cost_matrix, ref["cost_matrix"]) <= 1.0
        assert AC.sinkhorn_excess(res.responsibilities, ref["responsibilities"]) <= 1.0
