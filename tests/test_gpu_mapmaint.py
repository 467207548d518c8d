"""gc_primitive_map_maintain / primitive_map_maintain on the device against the oracle's per-tile
operators looped over the active tiles (tests/mapmaint_cases.py) and against the project's own
per-tile drop-ins looped on a second device map. Discrete outputs (valid_mask, ids, the scan-seq
fields, timestamps, every count) must be equal; every float field of every tile, active or not,
meets the 1e-10 bar of test_gpu_mapupdate (_cmp: relative to the array's max-abs); the weights of
slots no merge touched equal the drop-ins' bit for bit (one multiply); mass sums agree to 1e-12
relative (the bar of test_map_ops.py for the per-tile cull). The cases' margins (test_mapmaint.py)
make the discrete comparison well posed. Then the pass's grouping and layouts, that neither entry
of step 12b waits for the stream, and maintenance="device" of
primitive_map_update_from_association against the restatement and against maintenance=True."""

import ctypes as C
import time

import numpy as np
import pytest

from test_association import _cmp
from test_gpu_mapupdate import _check_map, _check_result, _fresh_map, _same_bits, _tiles_of, _update

import mapmaint_cases as MM
import mapupdate_cases as MC

RTOL = 1e-10
_EXACT = ("valid_mask", "primitive_ids", "last_supported_scan_seq", "last_update_scan_seq", "timestamps")


def _fresh(ctx, case, packed=True):
    from gcslam.primitive_map import DevicePrimitiveMap
    dm = DevicePrimitiveMap(len(case["tiles"]), case["m_tile"], ctx=ctx, packed=packed)
    dm.upload(**MM.flat(case))
    dm.tile_count = {d: int(t["valid_mask"].sum()) for d, t in enumerate(case["tiles"])}
    dm.total_count = sum(dm.tile_count.values())
    dm.colors_current = True  # so that only what the maintenance marks stale is stale afterwards
    return dm


def _config(case):
    from gcslam.primitive_map import MapUpdateConfig
    return MapUpdateConfig(**case["cfg"])


def _maintain(ctx, case, max_sort_keys=0, packed=True):
    from gcslam.primitive_map import primitive_map_maintain
    dm = _fresh(ctx, case, packed)
    return dm, primitive_map_maintain(dm, case["active"], _config(case), case["max_primitives"], max_sort_keys)


def _dropins(ctx, case):
    """The per-tile operators looped as step 12b does (pipeline.py:1412-1447) on a second map."""
    from gcslam import primitive_map as PM
    cfg = _config(case)
    dm = _fresh(ctx, case)
    out = dict(n_culled=[], mass_dropped=[], n_merged=[], certs=[])
    for d in case["active"]:
        rc, cc, _ = PM.primitive_map_cull(dm, d, cfg.primitive_cull_weight_threshold, case["max_primitives"])
        _, cf, _ = PM.primitive_map_forget(dm, d, cfg.primitive_forgetting_factor)
        rm, cm, _ = PM.primitive_map_merge_reduce(dm, d, cfg.primitive_merge_threshold, int(cfg.k_merge_pairs_tile),
                                                  int(cfg.max_tile_size), cfg.eps_psd, cfg.eps_lift,
                                                  anchor_id="primitive_map_merge_reduce")
        out["n_culled"].append(rc.n_culled)
        out["mass_dropped"].append(rc.mass_dropped)
        out["n_merged"].append(rm.n_merged)
        out["certs"].append((cc, cf, cm))
    return dm, out


def _dense_tiles(dm):
    full = dm.download()
    full["valid_mask"] = full["valid_mask"].astype(bool)
    m = dm.m_tile
    return [{f: v[d * m:(d + 1) * m] for f, v in full.items()} for d in range(dm.n_tiles)]


def _close(a, b, rtol=1e-12):
    return abs(a - b) <= rtol * max(abs(a), abs(b))


@pytest.mark.gpu
@pytest.mark.parametrize("name", MM.CASES)
def test_gpu_maintain_matches_oracle_and_dropins(ctx, name):
    from gcslam.certificates import aggregate_certificates
    case = MM.build(name)
    ref = MM.expected(case)
    cfg = _config(case)
    dm, (res, cert, eff) = _maintain(ctx, case)
    got = _dense_tiles(dm)
    # ---- the oracle loop
    for d, t in enumerate(got):
        _cmp(t, ref["tiles"][d], _EXACT, RTOL)
    assert res.tile_ids == case["active"]
    for a, (d, row) in enumerate(zip(case["active"], ref["rows"])):
        assert (res.n_culled[a], res.n_merged[a]) == (row["n_culled"], row["n_merged"]), d
        assert _close(res.mass_dropped[a], row["mass_dropped"]), (d, res.mass_dropped[a], row["mass_dropped"])
        assert dm.tile_count[d] == row["n_after"], d
        tc = res.tile_certs[a]
        assert tc[0].exact == (row["n_culled"] == 0) and tc[1].exact
        assert ("merge_reduce_budget_cap" in tc[2].approximation_triggers) == (row["state"] == "capped")
        assert tc[2].exact == (row["state"] == "noop" or (row["state"] == "ran" and row["n_merged"] == 0))
    assert res.n_culled_total == sum(r["n_culled"] for r in ref["rows"])
    assert res.n_merged_total == sum(r["n_merged"] for r in ref["rows"])
    assert _close(res.mass_dropped_total, sum(r["mass_dropped"] for r in ref["rows"]))
    assert (eff.objective_name, eff.predicted, eff.realized) == \
        ("primitive_map_maintain", float(len(case["active"]) * cfg.k_merge_pairs_tile), float(res.n_merged_total))
    # ---- the per-tile drop-ins on a second map
    dm2, dr = _dropins(ctx, case)
    got2 = _dense_tiles(dm2)
    gamma = cfg.primitive_forgetting_factor
    merged_of = dict(zip(case["active"], dr["n_merged"]))
    for d, (t, t2) in enumerate(zip(got, got2)):
        _cmp(t, t2, _EXACT, RTOL)
        w0 = case["tiles"][d]["weights"]
        unmerged = t2["weights"] == (gamma * w0 if d in merged_of else w0)
        assert int((~unmerged).sum()) <= 2 * merged_of.get(d, 0), d
        assert t["weights"][unmerged].tobytes() == t2["weights"][unmerged].tobytes(), d
        if d not in merged_of:  # an inactive tile: bit-identical to what was uploaded
            for f in t:
                assert t[f].tobytes() == t2[f].tobytes(), (d, f)
    np.testing.assert_array_equal(res.n_culled, dr["n_culled"])
    np.testing.assert_array_equal(res.n_merged, dr["n_merged"])
    for a in range(len(case["active"])):
        assert _close(res.mass_dropped[a], dr["mass_dropped"][a]), a
        for got_c, want_c in zip(res.tile_certs[a], dr["certs"][a]):
            assert got_c.to_dict() == want_c.to_dict(), (a, got_c.anchor_id)
    assert (dm.tile_count, dm.total_count, dm._tile_cc) == (dm2.tile_count, dm2.total_count, dm2._tile_cc)
    assert cert.to_dict() == aggregate_certificates([c for t in dr["certs"] for c in t]).to_dict()
    if name == "cap":
        assert res.tile_certs[0][2].influence.mass_epsilon_ratio == 0.5
    if name in ("kat", "tiny_m2", "ragged", "topk"):
        stale = [d for d, cc in enumerate(dm._tile_cc) if not cc]
        assert stale == sorted(d for d, n in merged_of.items() if n > 0) and stale


def _bits(dm, res):
    full = dm.download()
    return ({k: v.tobytes() for k, v in full.items()}, res.n_culled.tobytes(), res.mass_dropped.tobytes(),
            res.n_merged.tobytes(), [[c.to_dict() for c in t] for t in res.tile_certs],
            dict(dm.tile_count), dm.total_count, list(dm._tile_cc))


@pytest.mark.gpu
def test_gpu_maintain_grouping_layouts_and_reruns_bitwise(ctx):
    """ragged: groups of 1, of 2 + 1 and one group; the per-field layout; the same call twice."""
    case = MM.build("ragged")
    ref = MM.expected(case)
    P = case["P"]
    runs = {k: _maintain(ctx, case, k) for k in (P, 2 * P, 0)}
    base = _bits(runs[0][0], runs[0][1][0])
    for k in (P, 2 * P):
        assert _bits(runs[k][0], runs[k][1][0]) == base, k
    dm, (res, _, _) = _maintain(ctx, case, 0)
    assert _bits(dm, res) == base
    dmf, (resf, _, _) = _maintain(ctx, case, 0, packed=False)
    assert not dmf.packed and _bits(dmf, resf) == base
    for d, t in enumerate(_dense_tiles(dmf)):
        _cmp(t, ref["tiles"][d], _EXACT, RTOL)


def _device_call_args(ctx, case, dm):
    """The arguments of gc_primitive_map_update and gc_primitive_map_maintain on pre-uploaded device
    arrays, marshalled as primitive_map_update_from_association does."""
    from gcslam import _abi
    from gcslam import primitive_map as PM
    cfg = PM.MapUpdateConfig(**case["cfg"])
    N, K, k_ins, L = case["N"], case["K"], case["k_ins"], dm.n_lobes
    dense = [dm.dense_tile(t) for t in case["active"]]
    A = len(dense)
    h_dense = np.asarray(dense, np.int32)
    host_in = [np.ascontiguousarray(case["meas"][k], dt).reshape((N,) if w == 1 else (N, w or 3 * L))
               for k, dt, w in PM._MU_BATCH] + \
              [np.ascontiguousarray(case["assoc"][k], dt).reshape((N,) if k == "row_masses" else (N, K))
               for k, dt in PM._MU_ASSOC] + [np.asarray(case["active"], np.int64), h_dense]
    dts = [dt for _, dt, _ in PM._MU_BATCH] + [dt for _, dt in PM._MU_ASSOC] + [np.int64, np.int32]
    d_in = _abi.upload_many(ctx, host_in, dts)
    AK = A * k_ins
    d_out = _abi.alloc_many(ctx, [((AK,), np.int32), ((AK,), np.uint8), ((AK,), np.int32), ((AK,), np.int64),
                                  ((AK, 9), np.float64), ((AK, 3), np.float64), ((AK,), np.float64),
                                  ((PM._MU_HEAD + PM._MU_TILE * A,), np.float64), ((A * PM._MM_TILE,), np.float64)])
    s_in = PM._MapUpdateIn(N, dm.m_tile, K, A, k_ins, int(cfg.block_size), *[d.ptr for d in d_in],
                           h_dense.ctypes.data)
    s_out = PM._MapUpdateOut(*[d.ptr for d in d_out[:8]])
    pose = np.ascontiguousarray(case["pose"], np.float64)
    u_cfg = np.array([cfg.eps_lift, cfg.eps_mass, cfg.h_tile, cfg.recency_decay_lambda], np.float64)
    m_cfg = np.array([cfg.primitive_cull_weight_threshold, cfg.primitive_forgetting_factor,
                      cfg.primitive_merge_threshold, cfg.eps_psd, cfg.eps_lift], np.float64)
    keep = (d_in, d_out, s_in, s_out, pose, u_cfg, m_cfg, h_dense)
    update = ("gc_primitive_map_update", ctx.handle, C.byref(dm.struct()), C.byref(s_in), pose.ctypes.data,
              u_cfg.ctypes.data, float(MC.TIMESTAMP), int(MC.SCAN_SEQ), int(dm.next_global_id), C.byref(s_out))
    maintain = ("gc_primitive_map_maintain", ctx.handle, C.byref(dm.struct()), dm.m_tile, A, d_in[-1].ptr,
                h_dense.ctypes.data, m_cfg.ctypes.data, -1, int(cfg.k_merge_pairs_tile), int(cfg.max_tile_size), 0,
                d_out[8].ptr)
    return update, maintain, d_out, cfg, dense, keep


@pytest.mark.gpu
def test_gpu_update_and_maintain_do_not_wait_for_the_stream(ctx):
    """Behind a 0.5 s device spin both entries return at once; a call that waited for the stream would
    take the spin's time. The result, read after the synchronise, is the restatement's."""
    from gcslam import _abi
    from gcslam import primitive_map as PM
    case = MC.build("ragged")
    ref = MC.reference(case, True)
    _update(ctx, case, "device")  # warm-up: sizes the context's scratch (growing it synchronises)
    dm = _fresh_map(ctx, case)
    update, maintain, d_out, cfg, dense, keep = _device_call_args(ctx, case, dm)
    ctx.sync()
    _abi.call("gc_test_device_spin", ctx.handle, 0.5, ctx=ctx)
    t0 = time.perf_counter()
    _abi.call(*update, ctx=ctx)
    t1 = time.perf_counter()
    _abi.call(*maintain, ctx=ctx)
    t2 = time.perf_counter()
    ctx.sync()
    t3 = time.perf_counter()
    print(f"update {t1 - t0:.4f} s, maintain {t2 - t1:.4f} s, synchronise {t3 - t2:.4f} s")
    assert t1 - t0 < 0.25 and t2 - t1 < 0.25, (t1 - t0, t2 - t1)
    mstats = _abi.download_many(d_out)[8]
    _check_map(_tiles_of(dm), ref["tiles"], case["m_tile"])
    mr = PM._maintain_finish(dm, dense, mstats, cfg, "chart")
    assert (mr.n_culled_total, mr.n_merged_total) == (ref["n_culled"], ref["n_merged"])
    assert abs(mr.mass_dropped_total - ref["evicted_mass_total"]) <= RTOL * max(1.0, abs(ref["evicted_mass_total"]))
    del keep


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ragged", "placeholder"])
def test_gpu_map_update_device_maintenance(ctx, name):
    """maintenance="device": the restatement's result, and the bits of maintenance=True."""
    case = MC.build(name)
    ref = MC.reference(case, True)
    MC.check_margins(ref)
    one = _update(ctx, case, "device")
    dm, (res, cert, eff) = one
    _check_result(res, ref)
    _check_map(_tiles_of(dm), ref["tiles"], case["m_tile"])
    assert dm.next_global_id == ref["next_global_id"]
    for d, k in enumerate(dm.tile_keys):
        if k in case["active"]:
            assert dm.tile_count[d] == int(ref["tiles"][k]["valid_mask"].sum()), k
    loop = _update(ctx, case, True)
    _same_bits(one, loop)
    assert dm._tile_cc == loop[0]._tile_cc
    assert cert.map_update.merged_count == ref["n_merged"] and cert.map_update.evicted_count == ref["n_culled"]
    assert eff.to_dict() == loop[1][2].to_dict()
    if name == "placeholder":  # 21 active tiles, the cz != 0 ones empty before their inserts
        assert len(case["active"]) == 21
