"""The lean feature set of the persistent bins form (k_bins_io, gc_bins.hip): the per-bin direction scatter
has one reader in a scan, the bin map's increment of global hypothesis 0, so every other hypothesis's bin
statistics carry 0.0 in columns 4:13, and its long tasks accumulate 13 of the 19 per-bin moment features.

Shapes (B = 48 but for the last, two scans each):
  h3        H = 3, 4,096-point scans, n_points_cap = 4,096: hypothesis 0 full, 1 and 2 lean, 16 one-iteration
            chunks per hypothesis, the finalize folded into the evidence kernel;
  h3_pad    the same with n_points_cap = 4,000: the last chunk takes the padded form (stride 2 selection);
  h1        H = 1: every task full;
  shard     H = 4 as two shards of 2 with host-gathered records (test_gpu_shards.ShardSet): no task of rank 1
            (h_begin = 2) is full;
  h2_split  H = 2, 16,384-point scans: 64 chunks per hypothesis, more than the fold takes, so the zeros come
            from the split finalize kernel;
  h2_long   H = 2, 65,536-point scans with the chunk geometry of 256 hypotheses (geometry_hyps = 256): the
            late-ticket instantiation with its 32-iteration tasks, the only one whose tasks run the lean
            set (13 features and, in chunks without padding, the entropy partial on the matrix core) and
            write lean records; hypothesis 0 full, hypothesis 1 lean;
  h2_long_pad  the same with n_points_cap = 65,000 (stride 2 selection): the last chunk of the lean hypothesis
            takes the lean set's padded form (valid flag from the lean slab, the entropy partial kept on the
            VALU for that chunk and taken from the matrix core for the others);
  h2_long_b64  h2_long with B = 64: the chunk record no longer fits the evidence kernel's table, so lean records
            go through the split finalize kernel (at B = 48 that needs more than 32 long chunks per
            hypothesis, over 250,000 points per scan).

Every other shape runs the look-ahead instantiation (tasks shorter than 32 iterations), which computes the
full set for every task: there the zeros of a lean-set hypothesis come from the finalize alone, and the
outputs keep the bits tests/test_gpu_bins_zbatch.py pins. The C3 / C5 tests of test_gpu_configs.py hold the
late-ticket instantiation to the oracle at full size.

Bars: against the oracle those of test_gpu_configs.py (its _run_and_compare, every hypothesis sampled; the map
at its 1e-8 / 1e-12), the raw sums and hypothesis 0's scatter at 1e-10; against the unchanged grid-form kernel
gc_scan_bins_fused and between the two modes 1e-12, both relative to the array's (column group's) largest
entry as everywhere in this suite, so a nearly empty bin cannot trip a bar by itself."""

import numpy as np
import pytest

from oracle import cases
from oracle import gc_oracle as O
from test_gpu_configs import _FAILS, _close, _pipeline, _record_to_map, _run_and_compare
from test_gpu_shards import ShardSet

pytestmark = pytest.mark.gpu

SHAPES = {  # name: (H, n_az, cap, world, geometry_hyps, B)
    "h3": (3, 256, 4096, 1, 0, 48),
    "h3_pad": (3, 256, 4000, 1, 0, 48),
    "h1": (1, 256, 4096, 1, 0, 48),
    "shard": (4, 256, 4096, 2, 0, 48),
    "h2_split": (2, 1024, 16384, 1, 0, 48),
    "h2_long": (2, 4096, 65536, 1, 256, 48),
    "h2_long_pad": (2, 4096, 65000, 1, 256, 48),
    "h2_long_b64": (2, 4096, 65536, 1, 256, 64),
}
# column groups of a GC_BIN_STATS row outside the direction scatter 4:13
GROUPS = (("N", 0, 1), ("s_dir", 1, 4), ("p_bar", 13, 16), ("Sigma_p", 16, 25), ("kappa", 25, 26),
          ("sum_p", 26, 29), ("sum_ppT", 29, 38))
_CASES, _DEFAULT = {}, {}


@pytest.fixture(autouse=True)
def _report():
    _FAILS.clear()
    yield
    assert not _FAILS, "\n".join(_FAILS[:60])


def _case(name):
    if name not in _CASES:
        H, n_az, cap, _, _, B = SHAPES[name]
        case = cases.build(H=H, n_az=n_az, n_scans=2, io="computed", cap=cap)
        if B != 48:  # cases.build's atlas and warm-up map have 48 bins: the same construction with B
            from gcslam import synth
            case = dict(case, bins=O.fibonacci_atlas(B))
            m0 = cases.warmup_map(synth.make_scan(0, n_az=n_az), case["n"], case["cfg"].lidar_origin, case["bins"], 0.0)
            case["map_record"] = cases.map_to_record(m0)
        _CASES[name] = case
    return _CASES[name]


def _pipeline_bins(case, ctx, H, cap, geom, B):
    """test_gpu_configs._pipeline (one rank, the IMU/odom branch computed) with B bins."""
    from gcslam.pipeline import BatchedScanPipeline, PipelineConfig
    n_in = case["scans"][0]["points"].shape[0]
    pipe = BatchedScanPipeline(H, n_in, PipelineConfig(n_points_cap=cap, n_bins=B), ctx=ctx, geometry_hyps=geom)
    hy = case["hyp"]
    pipe.set_beliefs(hy["X_anchor"], hy["z_lin"], hy["L"], hy["h"], hy["stamp"])
    pipe.set_weights(hy["weights"])
    pipe.set_io_mode(True)
    pipe.set_iw(*case["iw"])
    pipe.set_map(case["map_record"])
    return pipe


def _make(ctx, name, scatter_all=False):
    H, _, cap, world, geom, B = SHAPES[name]
    case = _case(name)
    if B != 48:
        pipe = _pipeline_bins(case, ctx, H, cap, geom, B)
        parts = [pipe]
    elif world == 1:
        pipe = _pipeline(case, ctx, H, cap, True, geometry_hyps=geom)
        parts = [pipe]
    else:
        pipe = ShardSet(case, ctx, H, cap, world, geometry_hyps=geom)
        parts = pipe.shards
    if scatter_all:
        for p in parts:
            p.set_bin_scatter_all(True)
    return pipe, parts


def _outputs(pipe):
    b, c, iw, mp = pipe.get_beliefs(), pipe.combined(), pipe.get_iw(), pipe.get_map()
    st, bc, xi = pipe.bin_stats()
    return dict(stats=st, bincert=bc, xi=xi, X_anchor=b["X_anchor"], z_lin=b["z_lin"], L=b["L"], h=b["h"],
                hyp_diag=pipe.hyp_diag(), comb_L=c["L"], comb_h=c["h"], comb_z=c["z_lin"], nu_proc=iw["nu_proc"],
                Psi_proc=iw["Psi_proc"], nu_meas=iw["nu_meas"], Psi_meas=iw["Psi_meas"], Q=iw["Q"], map=mp["map"])


def _fused(ctx, cfg, s, cap, xi):
    """The grid-form fused kernel (all 19 features for every hypothesis) on scan s with the twists xi."""
    from gcslam import _abi
    n_in, H, B = s["points"].shape[0], xi.shape[0], cfg.n_bins
    dP, dT, dW = (_abi.DeviceArray.from_host(ctx, s[k]) for k in ("points", "timestamps", "weights"))
    scal = _abi.DeviceArray(ctx, 8)
    _abi.call("gc_budget_stats", ctx.handle, dW.ptr, n_in, cap, scal.ptr, ctx=ctx)
    dX = _abi.DeviceArray.from_host(ctx, np.ascontiguousarray(xi))
    dB = _abi.DeviceArray.from_host(ctx, O.fibonacci_atlas(B))
    st, ce = _abi.DeviceArray(ctx, (H, B, 38)), _abi.DeviceArray(ctx, (H, 8))
    oa, op = _abi.f64p(np.array(cfg.lidar_origin, dtype=np.float64))
    _abi.call("gc_scan_bins_fused", ctx.handle, H, n_in, cap, B, dP.ptr, dT.ptr, dW.ptr, scal.ptr, s["scan_start"],
              s["scan_end"], dX.ptr, dB.ptr, cfg.tau, op, cfg.eps_psd, cfg.eps_mass, st.ptr, ce.ptr, 0, ctx=ctx)
    return st.download()


def _vs_fused(stats, full, tag, scatter_rows):
    """The pipeline's rows against the grid form's outside 4:13, and inside for scatter_rows, at 1e-12."""
    for i in range(stats.shape[0]):
        for g, a, b in GROUPS:
            _close(stats[i, :, a:b], full[i, :, a:b], 1e-12, 0.0, f"{tag} hyp{i} {g} vs grid form")
        if i in scatter_rows:
            _close(stats[i, :, 4:13], full[i, :, 4:13], 1e-12, 0.0, f"{tag} hyp{i} scatter vs grid form")


def _run_default(ctx, name):
    """Two scans in the default mode with checks 1, 2 and 4 around every scan; the outputs after them."""
    H, _, cap, _, _, _ = SHAPES[name]
    case = _case(name)
    pipe, parts = _make(ctx, name)
    ocfg = O.PipeConfig(n_points_cap=cap)

    def before(k):
        return pipe.get_beliefs(), pipe.get_iw(), pipe.get_map()

    def after(k, x):
        bel0, iw0, mp0 = x
        s = case["scans"][k]
        stats, _, xi = pipe.bin_stats()
        mapst = _record_to_map(mp0["map"])
        Q = O.iw_process_Q(iw0["nu_proc"], iw0["Psi_proc"])
        Sga = (O.iw_meas_mode(iw0["nu_meas"], iw0["Psi_meas"], 0), O.iw_meas_mode(iw0["nu_meas"], iw0["Psi_meas"], 1))
        md = O.map_derived(mapst)
        for i in range(H):
            b_prev = O.Belief(bel0["X_anchor"][i].copy(), bel0["z_lin"][i].copy(), bel0["L"][i].copy(),
                              bel0["h"][i].copy(), float(bel0["stamp"][i]))
            with O.exact_inactive_deltas():
                m = O.scan_hypothesis(b_prev, cases.scan_input(s), Q, None, mapst, md, case["bins"], ocfg, Sga)["moments"]
            tag = f"{name} scan{k} hyp{i}"
            _close(stats[i, :, 26:29], m["sum_p"], 1e-10, 0.0, f"{tag} sum_p")
            _close(stats[i, :, 29:38].reshape(-1, 3, 3), m["sum_ppT"], 1e-10, 0.0, f"{tag} sum_ppT")
            if i == 0:
                _close(stats[i, :, 4:13].reshape(-1, 3, 3), m["S_dir_scatter"], 1e-10, 0.0, f"{tag} scatter")
                assert np.any(stats[i, :, 4:13] != 0.0)
            elif not np.all(stats[i, :, 4:13] == 0.0):  # exactly +-0.0: no NaN, no stale value
                _FAILS.append(f"{tag}: columns 4:13 of a lean hypothesis are not all 0.0")
        _vs_fused(stats, _fused(ctx, parts[0].cfg, s, cap, xi), f"{name} scan{k}", scatter_rows=(0,))

    # N, s_dir, p_bar, Sigma_p, bincert and the rest of a scan for every hypothesis, the couplings and the map
    _run_and_compare(ctx, case, H, cap, list(range(H)), 2, True, pipe=pipe, hooks=(before, after))
    out = _outputs(pipe)
    for p in parts:
        p.close()
    return out


def _default(ctx, name):
    if name not in _DEFAULT:
        _DEFAULT[name] = _run_default(ctx, name)
    return _DEFAULT[name]


def _run_plain(ctx, name, scatter_all):
    case = _case(name)
    pipe, parts = _make(ctx, name, scatter_all)
    for k, s in enumerate(case["scans"][:2]):
        pipe.stage_scan(0, s)
        pipe.run_scan(0, s, k)
        ctx.sync()
    out = _outputs(pipe)
    cfg = parts[0].cfg
    for p in parts:
        p.close()
    return out, cfg


@pytest.mark.parametrize("name", list(SHAPES))
def test_lean_bins_match_oracle_and_grid_form(ctx, name):
    """Checks 1, 2 and 4: every hypothesis of every scan against the oracle (hypothesis 0 with its scatter,
    the others with exact zeros there), against gc_scan_bins_fused on the same scan and twists outside 4:13,
    and the bin map after each scan against the oracle's (hypothesis 0's scatter reaches its increment)."""
    out = _default(ctx, name)
    assert np.all(np.isfinite(out["stats"]))
    if name == "shard":  # rank 1's hypotheses (global 2, 3): none is full
        assert np.all(out["stats"][2:, :, 4:13] == 0.0)


@pytest.mark.parametrize("name", [n for n in SHAPES if n != "h1"])
def test_bin_scatter_all_restores_every_scatter(ctx, name):
    """Check 3: with set_bin_scatter_all(True) every hypothesis's columns 4:13 agree with the grid form's, and
    every other output with the default mode's, to 1e-12 (where the lean set has every feature on the matrix
    core, two features sum in another order than in the full set)."""
    H, _, cap, _, _, _ = SHAPES[name]
    ref = _default(ctx, name)
    out, cfg = _run_plain(ctx, name, True)
    full = _fused(ctx, cfg, _case(name)["scans"][1], cap, out["xi"])
    _vs_fused(out["stats"], full, f"{name} scatter_all", scatter_rows=range(H))
    for key, a in out.items():
        if key == "stats":
            for g, c0, c1 in GROUPS:
                _close(a[..., c0:c1], ref[key][..., c0:c1], 1e-12, 0.0, f"{name} scatter_all {g} vs default mode")
            _close(a[0, :, 4:13], ref[key][0, :, 4:13], 1e-12, 0.0, f"{name} hypothesis 0's scatter vs default mode")
        else:
            _close(a, ref[key], 1e-12, 0.0, f"{name} scatter_all {key} vs default mode")


@pytest.mark.parametrize("name", list(SHAPES))
def test_lean_bins_are_bit_reproducible(ctx, name):
    """Check 5: a second run equals the first bit for bit in the bin statistics (the zeros of the lean rows
    included), the beliefs and the map."""
    ref = _default(ctx, name)
    out, _ = _run_plain(ctx, name, False)
    for key in ("stats", "X_anchor", "z_lin", "L", "h", "map"):
        assert np.array_equal(out[key], ref[key]), key
