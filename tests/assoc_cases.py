"""Inputs of the association edge tests (test_association_edges.py, test_gpu_association_edges.py),
built on the CPU alone in the pattern of vpe_cases.py: a hex-tiled map, a measurement batch, the
oracle's map view and OT association. Each case reaches a path of csrc/gc_assoc.hip that the parity
test of test_association.py does not: the row-strided Sinkhorn (N > 1024), zero and one Sinkhorn
iteration, the outer branches and the kappa = 0 gate of A_vmf, stencils past 64 tiles and with
r_z > 0, K = 16 / odd K, rows with fewer than K valid candidates, bit-equal costs within one lane and
across lanes, a pool of 112 candidates per lane, L = 1 and 8 lobes, m_tile_view == m_tile, a tile of
more than 2048 slots, a tile id listed twice and equal weights among valid slots.

check_conditions holds what makes exact index equality a fair demand of the device (separated
costs, measurements away from cell boundaries, bounded raw costs), that each case reaches its path,
and that the float64 oracle agrees with a long-double restatement of the cost and of the Sinkhorn
loop (written here, not in the oracle) to 1/100 of every bar the GPU test applies."""

import numpy as np

from oracle import gc_oracle as O
from test_association import _hex_map, _meas

LD = np.longdouble
_RAGGED = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0)]  # the geometry of vpe_cases "ragged"
_GRID3 = [(a, b, 0) for a in range(3) for b in range(3)]

# cfg: oracle keys (O.OT_DEFAULTS). n_valid: populated slots per tile (int, or one per cell).
CASES = {
    "strided": dict(N=2501, L=3, cells=[(a, b, c) for a in range(-2, 3) for b in range(-2, 3) for c in (-1, 0, 1)],
                    m_tile=64, n_valid=60, m_view=32, seed=7,
                    cfg=dict(k_assoc=16, r_xy=2, r_z=2, scan_seq=9)),
    "edge1025": dict(N=1025, L=3, cells=[(a, b, c) for a in range(3) for b in range(3) for c in (0, 1)],
                     m_tile=64, n_valid=60, m_view=32, seed=11,
                     cfg=dict(k_assoc=13, r_xy=1, r_z=1, scan_seq=9, weight_proportional=True)),
    "sparse": dict(N=70, L=3, cells=_GRID3, m_tile=16, n_valid=[0, 1, 2, 3, 5, 6, 7, 9, 12], m_view=16, seed=13,
                   cfg=dict(k_assoc=8, r_xy=0, r_z=0, scan_seq=9)),
    "ties": dict(N=64, L=3, cells=_RAGGED, m_tile=160, n_valid=140, m_view=128, seed=17,
                 cfg=dict(k_assoc=5, scan_seq=9, cost_subtract_row_min=False)),
    "longpool": dict(N=37, L=3, cells=[(0, 0, 0), (1, 0, 0), (0, 1, 0)], m_tile=2049, n_valid=2049, m_view=1024,
                     seed=19, cfg=dict(k_assoc=16, scan_seq=9)),
    "lobes1": dict(N=70, L=1, cells=_RAGGED, m_tile=64, n_valid=60, m_view=32, seed=23,
                   cfg=dict(k_assoc=3, scan_seq=9)),
    "lobes8": dict(N=70, L=8, cells=_RAGGED, m_tile=64, n_valid=60, m_view=32, seed=29,
                   cfg=dict(k_assoc=3, scan_seq=9)),
    "full_view": dict(N=9, L=3, cells=[(0, 0, 0)], m_tile=16, n_valid=16, m_view=16, seed=31,
                      cfg=dict(k_assoc=16, scan_seq=9)),
    "iters0": dict(N=70, L=3, cells=_RAGGED, m_tile=64, n_valid=60, m_view=32, seed=5,
                   cfg=dict(k_assoc=8, scan_seq=9, k_sinkhorn=0)),
    "iters1": dict(N=70, L=3, cells=_RAGGED, m_tile=64, n_valid=60, m_view=32, seed=5,
                   cfg=dict(k_assoc=8, scan_seq=9, k_sinkhorn=1)),
}
# cases the GPU test also runs on the per-field map layout
BOTH_LAYOUTS = ("lobes1", "lobes8")

# the GPU test's bars; check_conditions holds the oracle to 1/100 of each against the restatement
COST_BAR = 1e-10      # |got - ref| <= COST_BAR max(1, |ref_ij|), per element
SINKHORN_BAR = 1e-8   # as test_gpu_association_matches_oracle applies it (sinkhorn_excess)
CERT_SCALARS = ("marginal_defect_a", "marginal_defect_b", "transport_mass_total", "sum_a", "sum_m", "sum_novel")

_cache = {}


def _tiles(rng, spec):
    """_hex_map, one call per cell so that the populated count may differ per tile; every populated
    slot beyond the count stays the empty tile's zeros. L != 3: the lobes are redrawn."""
    cells, L = spec["cells"], spec["L"]
    counts = spec["n_valid"] if isinstance(spec["n_valid"], list) else [spec["n_valid"]] * len(cells)
    tiles = {}
    for cell, n in zip(cells, counts):
        (tid, t), = _hex_map(rng, spec["m_tile"], n, [cell]).items()
        if L != 3:
            etas = np.zeros((spec["m_tile"], L, 3))
            etas[:n] = rng.normal(size=(n, L, 3)) * 2.0
            t["etas"] = etas
        tiles[tid] = t
    return tiles


def _kappa_scales(rng, n):
    """10^U(-4, 1.5) per primitive, about one in ten exactly zero: kappa from 0 over < 1e-2 to > 20."""
    s = 10.0 ** rng.uniform(-4.0, 1.5, n)
    s[rng.uniform(0, 1, n) < 0.1] = 0.0
    return s


def _build_inputs(name, spec, rng):
    tiles = _tiles(rng, spec)
    ids = list(tiles)
    cells, N, L = spec["cells"], spec["N"], spec["L"]
    lo = 2.0 * min(c[0] for c in cells)
    hi = 2.0 * (max(c[0] for c in cells) + 1)
    meas = _meas(rng, N, lo, hi)
    if L != 3:
        meas["etas"] = rng.normal(size=(N, L, 3)) * 2.0
    if name == "strided":
        for t in tiles.values():
            t["etas"] *= _kappa_scales(rng, t["etas"].shape[0])[:, None, None]
        meas["etas"] *= _kappa_scales(rng, N)[:, None, None]
        meas["thetas"][:, 2] = 4.0 * rng.uniform(-4.0, 6.0, N)  # z over cells -2 .. 2: tiles hold -1 .. 1
        meas["thetas"][:, 0] = 4.0 * rng.uniform(-9.0, 11.0, N)  # x past the stencil's reach: rows with no candidate
    elif name == "edge1025":
        meas["thetas"][:, 2] = 4.0 * rng.uniform(0.0, 4.0, N)
    elif name == "sparse":
        for t in tiles.values():  # a populated slot or two that is not valid: a filler with a real entry
            pop = np.flatnonzero(t["weights"] > 0)
            t["valid_mask"][pop] = True
            t["valid_mask"][pop[4::5]] = False
        meas["valid_mask"][:] = True
        meas["valid_mask"][[3, 17, 40, 66]] = False
    elif name == "ties":
        # weights strictly decreasing in the slot, so the view's rank is the slot and a copy's pool position
        # is known: slot j + 1 (the next lane) or slot j + 64 (the same lane). Rows 0..31 sit next to a copied
        # primitive, so the tie is among their best candidates.
        spots = []
        for t in tiles.values():
            n = spec["n_valid"]
            t["valid_mask"][:n] = True
            t["weights"][:n] = np.linspace(1.0, 0.1, n)
            for j, d in ((2, 1), (9, 1), (20, 64), (31, 64), (40, 1), (50, 64)):
                for k in ("Lambdas", "thetas", "etas", "last_supported_scan_seq"):
                    t[k][j + d] = t[k][j]
                spots.append(np.linalg.solve(t["Lambdas"][j], t["thetas"][j]))
        spots = np.array(spots)
        k = min(32, len(spots))
        meas["thetas"][:k] = 4.0 * (spots[:k] + rng.uniform(-0.05, 0.05, (k, 3)))
        meas["valid_mask"][:k] = True
    elif name == "longpool":
        for t in tiles.values():  # equal weights among valid slots, heavy enough to be in the view
            idx = rng.choice(spec["m_tile"], 600, replace=False)
            t["weights"][idx] = rng.choice([0.95, 0.9, 0.85], 600)
        ids = [ids[0], ids[1], ids[0], ids[2]]  # one tile listed twice: the stencil takes the first
    elif name in ("iters0", "iters1"):
        meas["valid_mask"][:] = True
        meas["valid_mask"][[9 * p for p in range(8)]] = False
    return tiles, ids, meas


def build(name):
    """dict(name, tiles, ids, m_tile, m_view, L, N, K, meas, cfg, view, assoc, cert) — computed once per
    case and shared; callers must not modify it. ids is the view's tile list (it may repeat a tile)."""
    if name in _cache:
        return _cache[name]
    spec = CASES[name]
    rng = np.random.default_rng(spec["seed"])
    tiles, ids, meas = _build_inputs(name, spec, rng)
    view = O.extract_atlas_map_view(tiles, ids, spec["m_view"], spec["m_tile"], L=spec["L"])
    assoc, cert = O.associate_primitives_ot(meas, view, spec["cfg"])
    out = dict(name=name, tiles=tiles, ids=ids, m_tile=spec["m_tile"], m_view=spec["m_view"], L=spec["L"],
               N=spec["N"], K=int(spec["cfg"]["k_assoc"]), meas=meas, cfg=dict(spec["cfg"]), view=view, assoc=assoc,
               cert=cert)
    _cache[name] = out
    return out


# ------------------------------------------------------------------ the bars, shared with the GPU test
def cost_excess(got, ref, bar=COST_BAR):
    """max over elements of |got - ref| / (bar max(1, |ref|)): the bar holds iff <= 1."""
    got, ref = np.asarray(got, LD), np.asarray(ref, LD)
    return float(np.max(np.abs(got - ref) / (bar * np.maximum(1.0, np.abs(ref)))))


def sinkhorn_excess(got, ref, bar=SINKHORN_BAR):
    """assert_allclose(rtol=bar, atol=bar max(1, max|ref|)) as a ratio (<= 1 passes): the rule of
    test_association._cmp."""
    got, ref = np.asarray(got, LD), np.asarray(ref, LD)
    atol = bar * max(1.0, float(np.max(np.abs(ref))))
    return float(np.max(np.abs(got - ref) / (atol + bar * np.abs(ref))))


def scalar_excess(got, ref, rtol, atol):
    return float(abs(LD(got) - LD(ref)) / (LD(atol) + LD(rtol) * abs(LD(ref))))


def sinkhorn_scalar_excesses(got, ref, bar=SINKHORN_BAR):
    """{name: ratio} for the cert scalars (rtol bar, atol 1e-12 bar / 1e-8), ess and total_cost (rtol bar)."""
    out = {k: scalar_excess(got[k], ref[k], bar, 1e-12 * bar / SINKHORN_BAR) for k in CERT_SCALARS}
    out["ess"] = scalar_excess(got["ess"], ref["ess"], bar, 0.0)
    out["total_cost"] = scalar_excess(got["total_cost"], ref["total_cost"], bar, 0.0)
    return out


# ------------------------------------------------------------------ the pool, restated for the conditions
def pool_scan(case):
    """Per measurement row, from the whole stencil pool in float64 (the steps of
    primitive_association.py:307-372): the K + 1 smallest costs and their pool positions (stable
    order), the number of valid candidates, and over valid (row, candidate) pairs the counts of
    k_m > 20 and k_m < 1e-2. Also the distance of each scaled cell coordinate from an integer."""
    if "pool" in case:
        return case["pool"]
    cfg = dict(O.OT_DEFAULTS, **case["cfg"])
    meas, view, K, N = case["meas"], case["view"], case["K"], case["N"]
    Lr = meas["Lambdas"] + O.EPS_LIFT * np.eye(3)[None]
    mp = np.linalg.solve(Lr, meas["thetas"][..., None])[..., 0]
    es = meas["etas"].sum(axis=1)
    mk = np.linalg.norm(es, axis=1)
    md = es / (mk[:, None] + O.EPS_MASS)
    h = max(float(cfg["h_tile"]), 1e-12)
    scaled = np.column_stack([mp[:, 0] / h, (mp[:, 0] * 0.5 + mp[:, 1] * (np.sqrt(3.0) * 0.5)) / h, mp[:, 2] / h])
    c1, c2, cz = O.tile_cells_from_xyz(mp, cfg["h_tile"])
    disk = O.hex_disk_axial(cfg["r_xy"])
    kv = int(view["m_tile_view"])
    first, first_pos, n_valid = np.zeros((N, K + 1)), np.zeros((N, K + 1), np.int64), np.zeros(N, np.int64)
    first_idx = np.zeros((N, K + 1), np.int64)
    n_big = n_small = 0
    valid = np.asarray(meas["valid_mask"], bool)
    for r0 in range(0, N, 128):
        r = slice(r0, min(N, r0 + 128))
        st = np.stack([O.tile_ids_from_cells(c1[r] + q, c2[r] + rr, cz[r] + dz)
                       for dz in range(-int(cfg["r_z"]), int(cfg["r_z"]) + 1) for (q, rr) in disk], axis=1)
        eq = st[:, :, None] == view["tile_ids"][None, None, :]
        has = eq.any(axis=2)
        tix = np.where(has, eq.argmax(axis=2), 0)
        pool = ((tix * kv)[:, :, None] + np.arange(kv)[None, None, :]).reshape(st.shape[0], -1)
        pv = view["valid_mask"][pool] & np.repeat(has, kv, axis=1)
        vk = view["kappas"][pool]
        cost = O.ot_cost(mp[r], md[r], mk[r], view["positions"][pool], view["directions"][pool], vk, cfg["beta"])
        cost = np.where(pv, cost, 1e12)
        km = 0.5 * np.linalg.norm(mk[r, None, None] * md[r, None, :] + vk[:, :, None] * view["directions"][pool], axis=-1)
        live = pv & valid[r, None]
        n_big += int(np.sum(live & (km > 20.0)))
        n_small += int(np.sum(live & (km < 1e-2)))
        order = np.argsort(cost, axis=1, kind="stable")[:, :K + 1]
        first[r] = np.take_along_axis(cost, order, axis=1)
        first_pos[r] = order
        first_idx[r] = np.take_along_axis(pool, order, axis=1)
        n_valid[r] = pv.sum(axis=1)
    case["pool"] = dict(first=first, first_pos=first_pos, first_idx=first_idx, n_valid=n_valid, n_big=n_big, n_small=n_small,
                        cell_margin=float(np.min(np.abs(scaled - np.round(scaled)))), mk=mk)
    return case["pool"]


# ------------------------------------------------------------------ the long-double restatement
def _A_vmf_ld(k):
    """_A_vmf_vec_jax (primitive_association.py:141-149): log(4 pi) + log sinh k - log k."""
    k = np.maximum(k, LD(1e-12))
    with np.errstate(over="ignore", invalid="ignore"):
        ls = np.where(k > 20.0, k - np.log(LD(2.0)),
                      np.where(k >= 1e-2, np.log(np.sinh(np.minimum(k, LD(20.0)))), np.log(k + k * k * k / LD(6.0))))
    return np.log(LD(4.0) * LD(np.pi)) + ls - np.log(k)


def _solve3_ld(A, b):
    """Cramer's rule on (n, 3, 3), (n, 3) long doubles."""
    def det(M):
        return (M[:, 0, 0] * (M[:, 1, 1] * M[:, 2, 2] - M[:, 1, 2] * M[:, 2, 1])
                - M[:, 0, 1] * (M[:, 1, 0] * M[:, 2, 2] - M[:, 1, 2] * M[:, 2, 0])
                + M[:, 0, 2] * (M[:, 1, 0] * M[:, 2, 1] - M[:, 1, 1] * M[:, 2, 0]))
    d = det(A)
    out = np.zeros(b.shape, LD)
    for q in range(3):
        Aq = A.copy()
        Aq[:, :, q] = b
        out[:, q] = det(Aq) / d
    return out


def restate_ld(case):
    """The cost of the oracle's chosen candidates (:152-197, recency :389-397, row minimum), the
    unbalanced Sinkhorn (:105-138) and the cert sums, in np.longdouble from the float64 inputs
    (measurement info form, the oracle's view)."""
    if "ld" in case:
        return case["ld"]
    cfg = dict(O.OT_DEFAULTS, **case["cfg"])
    meas, view, cand, K, N = case["meas"], case["view"], case["assoc"]["candidate_pool_indices"], case["K"], case["N"]
    mp = _solve3_ld(meas["Lambdas"].astype(LD) + LD(O.EPS_LIFT) * np.eye(3, dtype=LD)[None], meas["thetas"].astype(LD))
    es = meas["etas"].astype(LD).sum(axis=1)
    mk = np.sqrt(np.sum(es * es, axis=1))
    md = es / (mk[:, None] + LD(O.EPS_MASS))
    vp, vd, vk = (view[k][cand].astype(LD) for k in ("positions", "directions", "kappas"))
    diff = mp[:, None, :] - vp
    d_pos = np.sum(diff * diff, axis=-1)
    e = mk[:, None, None] * md[:, None, :] + vk[:, :, None] * vd
    km = LD(0.5) * np.sqrt(np.sum(e * e, axis=-1))
    bc = np.exp(_A_vmf_ld(km) - LD(0.5) * (_A_vmf_ld(mk[:, None]) + _A_vmf_ld(vk)))
    d_dir = np.where((mk[:, None] > 0) & (vk > 0), np.maximum(LD(0.0), LD(1.0) - bc), LD(0.0))
    raw = d_pos + LD(cfg["beta"]) * d_dir
    dt = np.maximum(0, np.int64(cfg["scan_seq"]) - view["last_supported_scan_seq"][cand]).astype(LD)
    raw = raw + LD(cfg["epsilon"]) * LD(cfg["recency_decay_lambda"]) * dt
    Cm = raw - raw.min(axis=1, keepdims=True) if cfg["cost_subtract_row_min"] else raw
    vf = np.asarray(meas["valid_mask"], bool).astype(LD)
    wv = vf * meas["weights"].astype(LD) if cfg["weight_proportional"] else vf
    sum_a = max(wv.sum(), LD(cfg["eps_mass"]))
    a = wv / sum_a
    b = np.ones(K, LD) / LD(K)
    eps = max(LD(cfg["epsilon"]), LD(1e-12))
    Km = np.exp(-Cm / eps)
    ua, vb = LD(1.0) / (LD(1.0) + LD(cfg["tau_a"]) / eps), LD(1.0) / (LD(1.0) + LD(cfg["tau_b"]) / eps)
    u, v = np.ones(N, LD), np.ones(K, LD)
    for _ in range(int(cfg["k_sinkhorn"])):
        u = (a / (Km @ v + LD(1e-12))) ** ua
        v = (b / (Km.T @ u + LD(1e-12))) ** vb
    pi = u[:, None] * Km * v[None, :]
    rows, cols = pi.sum(axis=1), pi.sum(axis=0)
    em = LD(cfg["eps_mass"])
    cert = dict(marginal_defect_a=np.sqrt(np.sum((rows - a) ** 2)), marginal_defect_b=np.sqrt(np.sum((cols - b) ** 2)),
                transport_mass_total=pi.sum(), sum_a=sum_a, sum_m=rows.sum(),
                sum_novel=np.maximum(a - rows, LD(0.0)).sum(), ess=rows.sum() ** 2 / (np.sum(rows ** 2) + em),
                total_cost=np.sum(pi * Cm))
    case["ld"] = dict(raw_cost=raw, cost_matrix=Cm, responsibilities=pi * vf[:, None], row_masses=rows, cert=cert)
    return case["ld"]


# ------------------------------------------------------------------ the conditions
def check_conditions(case):
    """Asserts the conditions of the module docstring; returns the measured margins."""
    name, K = case["name"], case["K"]
    valid = np.asarray(case["meas"]["valid_mask"], bool)
    p = pool_scan(case)
    # the restated pool picks what the oracle picked (valid rows; invalid rows are index 0)
    cand = case["assoc"]["candidate_pool_indices"]
    assert np.array_equal(p["first_idx"][valid][:, :K], cand[valid])
    assert not cand[~valid].any() and not case["assoc"]["responsibilities"][~valid].any()
    # cost gaps among the first K + 1 real candidates of every valid row
    f, fp = p["first"][valid], p["first_pos"][valid]
    real = f[:, 1:] < 1e11
    gap = f[:, 1:] - f[:, :-1]
    tied = real & (gap == 0.0)
    small = real & (gap != 0.0) & (gap < 1e-9 * np.maximum(1.0, f[:, 1:]))
    assert not small.any(), (name, float(gap[small].min()))
    same_lane = cross_lane = 0
    if name == "ties":
        dpos = (fp[:, 1:] - fp[:, :-1])[tied]
        same_lane, cross_lane = int(np.sum(dpos % 64 == 0)), int(np.sum(dpos % 64 != 0))
        assert same_lane >= 1 and cross_lane >= 1, (same_lane, cross_lane)
    else:
        assert not tied.any(), (name, int(tied.sum()))
    min_gap = float(np.min((gap / np.maximum(1.0, f[:, 1:]))[real & ~tied])) if (real & ~tied).any() else np.inf
    # cell boundaries
    assert p["cell_margin"] >= 1e-9, (name, p["cell_margin"])
    # raw cost cap, and the oracle against the long-double restatement at 1/100 of each bar
    ld = restate_ld(case)
    raw_max = float(np.max(ld["raw_cost"]))
    assert raw_max <= 1e3, (name, raw_max)
    assoc, cert = case["assoc"], case["cert"]
    own = dict(cost=cost_excess(assoc["cost_matrix"], ld["cost_matrix"], COST_BAR / 100),
               responsibilities=sinkhorn_excess(assoc["responsibilities"], ld["responsibilities"], SINKHORN_BAR / 100),
               row_masses=sinkhorn_excess(assoc["row_masses"], ld["row_masses"], SINKHORN_BAR / 100))
    own.update(sinkhorn_scalar_excesses(cert, ld["cert"], SINKHORN_BAR / 100))
    assert all(v <= 1.0 for v in own.values()), (name, own)
    # paths reached
    nv = p["n_valid"]
    n_none = int(np.sum(valid & (nv == 0)))
    n_partial = int(np.sum(valid & (nv > 0) & (nv < K)))
    n_kappa0 = int(np.sum(p["mk"] == 0.0) + np.sum(case["view"]["valid_mask"] & (case["view"]["kappas"] == 0.0)))
    if name == "strided":
        assert p["n_big"] >= 100 and p["n_small"] >= 100 and n_kappa0 >= 10 and n_none >= 10, \
            (p["n_big"], p["n_small"], n_kappa0, n_none)
    if name == "sparse":
        assert n_partial >= 10 and int(np.sum(~valid)) >= 1, n_partial
    if name == "longpool":
        w = case["view"]["weights"][case["view"]["valid_mask"]]
        assert len(set(case["ids"])) < len(case["ids"]) and np.unique(w).size < w.size
    return dict(min_gap=min_gap, cell_margin=p["cell_margin"], raw_max=raw_max, own=own, n_big=p["n_big"],
                n_small=p["n_small"], n_kappa0=n_kappa0, n_none=n_none, n_partial=n_partial, same_lane=same_lane,
                cross_lane=cross_lane)
