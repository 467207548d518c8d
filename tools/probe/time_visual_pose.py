"""Time gc_visual_pose_evidence at the reference's per-scan shape: N = 1536 measurement primitives
(1024 surfels + 512 features), K = 8 candidates, a view of 7 tiles x 1024 entries, H in {1, 4, 256}
hypotheses. Each timed sample is one call between two events on the context's stream (the call's
three launches and its 24-byte certificate download); warm-up calls first, then the median of
--iters samples. H = 0 runs the pose-independent pass alone, so pass 2 is the difference.

Beside each time: the bytes the passes move and the rate that implies.
  pass 1 reads N x (Λ 72 + θ 24 + η 24 L + valid 1 + π 8 K + idx 4 K + row mass 8) streamed once, gathers
         N x K x 56 B (position, direction, κ) from the view pool (V x 56 B unique, L2-resident), reads the
         view's valid mask (V B), and writes N x 128 B of row records;
  pass 2 reads the N x 128 B records once per hypothesis (from L2 after the first) and writes
         H x (484 + 22 + 26) x 8 B.

--assoc times associate_primitives_ot (host wall clock per call, median) at (N, K, V) = (300, 8,
25 x 32); --parent-association FILE loads another version of gcslam/association.py beside the
current one and times both alternately on the same inputs.

    python tools/probe/time_visual_pose.py [--iters 100] [--json OUT]
    python tools/probe/time_visual_pose.py --assoc [--parent-association FILE]
"""

import argparse
import ctypes as C
import importlib.util
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "fl-slam_amd"))
sys.path.insert(0, ROOT)

from gcslam import _abi  # noqa: E402
from gcslam.association import DeviceMapView  # noqa: E402

L = 3


def synthetic_view(ctx, rng, n_tiles, m_view):
    view = DeviceMapView(ctx, np.arange(n_tiles), m_view, L)
    V = view.count
    d = rng.normal(size=(V, 3))
    view.arrays["positions"].upload(rng.uniform(-8.0, 8.0, (V, 3)))
    view.arrays["directions"].upload(d / np.linalg.norm(d, axis=1, keepdims=True))
    view.arrays["kappas"].upload(rng.uniform(0.5, 6.0, V))
    view.arrays["valid_mask"].upload((rng.uniform(0, 1, V) < 0.9).astype(np.uint8))
    return view


def time_evidence(ctx, iters, warmup):
    rng = np.random.default_rng(0)
    N, K, n_tiles, m_view = 1536, 8, 7, 1024
    view = synthetic_view(ctx, rng, n_tiles, m_view)
    V = view.count
    B = rng.normal(size=(N, 3, 3)) * 0.3
    Lam = B @ np.swapaxes(B, 1, 2) + 2.0 * np.eye(3)
    pi = rng.uniform(0, 1, (N, K)) / (N * K)
    host = [Lam.reshape(N, 9), np.einsum("nij,nj->ni", Lam, rng.uniform(-8, 8, (N, 3))),
            rng.normal(size=(N, L * 3)) * 2.0, (rng.uniform(0, 1, N) < 0.9).astype(np.uint8), pi,
            rng.integers(0, V, (N, K)).astype(np.int32), pi.sum(axis=1)]
    dev = [_abi.DeviceArray.from_host(ctx, a, a.dtype) for a in host]
    cert = np.zeros(_abi.GC_VPE_CERT)
    e0, e1 = _abi.Event(ctx), _abi.Event(ctx)
    rows = []
    b1_stream = N * (72 + 24 + 24 * L + 1 + 8 * K + 4 * K + 8) + V
    b1_gather, b1_write = N * K * 56, N * 128
    med = {}
    for H in (0, 1, 4, 256):
        P = np.zeros((max(H, 1), 6))
        P[:, :3] = rng.normal(size=P[:, :3].shape)
        P[:, 3:] = rng.normal(size=P[:, 3:].shape) * 0.2
        dP = _abi.DeviceArray.from_host(ctx, P)
        dL, dh, dp = (_abi.DeviceArray(ctx, (max(H, 1), 22, 22)), _abi.DeviceArray(ctx, (max(H, 1), 22)),
                      _abi.DeviceArray(ctx, (max(H, 1), _abi.GC_VPE_PARTS)))

        def call():
            _abi.call("gc_visual_pose_evidence", ctx.handle, N, K, L, *[d.ptr for d in dev], C.byref(view.struct), H,
                      dP.ptr, 1e-9, 1e-12, dL.ptr, dh.ptr, dp.ptr, cert.ctypes.data, ctx=ctx)

        for _ in range(warmup):
            call()
        ms = []
        for _ in range(iters):
            e0.record()
            call()
            e1.record()
            ctx.sync()
            ms.append(e0.elapsed_ms(e1))
        ms.sort()
        med[H] = statistics.median(ms)
        row = dict(H=H, median_us=1e3 * med[H], p10_us=1e3 * ms[len(ms) // 10], p90_us=1e3 * ms[(9 * len(ms)) // 10],
                   iters=iters)
        if H == 0:
            row.update(pass1_bytes_streamed=b1_stream, pass1_bytes_gathered=b1_gather, pass1_bytes_written=b1_write,
                       pass1_GBps=(b1_stream + b1_gather + b1_write) / (med[0] * 1e-3) / 1e9)
        else:
            p2 = max(med[H] - med[0], 1e-6)
            b2 = H * (N * 128 + (484 + 22 + _abi.GC_VPE_PARTS) * 8)
            row.update(pass2_us=1e3 * p2, pass2_bytes=b2, pass2_GBps=b2 / (p2 * 1e-3) / 1e9)
        rows.append(row)
        print(json.dumps(row), flush=True)
    return dict(shape=dict(N=N, K=K, V=V, n_lobes=L), rows=rows)


def _load_association(path):
    spec = importlib.util.spec_from_file_location("gcslam._association_other", path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


def time_association(ctx, iters, warmup, parent_path):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from gcslam import association as cur
    from test_association import _device_map, _hex_map, _meas
    rng = np.random.default_rng(5)
    tiles = _hex_map(rng, 64, 60, [(a, b, 0) for a in range(-2, 3) for b in range(-2, 3)])
    dm = _device_map(ctx, tiles, 64)
    view = cur.extract_atlas_map_view(dm, list(tiles), 32)
    meas = _meas(rng, 300)

    class Batch:
        pass

    for k, v in meas.items():
        setattr(Batch, k, v)
    mods = {"current": cur}
    if parent_path:
        mods["parent"] = _load_association(parent_path)
    samples = {k: [] for k in mods}
    for it in range(warmup + iters):
        for name, m in mods.items():  # alternate, so drift hits both alike
            cfg = m.AssociationConfig(scan_seq=9)
            t0 = time.perf_counter()
            m.associate_primitives_ot(Batch, view, cfg)
            if it >= warmup:
                samples[name].append(1e3 * (time.perf_counter() - t0))
    out = {}
    for name, s in samples.items():
        s.sort()
        out[name] = dict(median_ms=statistics.median(s), p10_ms=s[len(s) // 10], p90_ms=s[(9 * len(s)) // 10], iters=iters)
        print(json.dumps({name: out[name]}), flush=True)
    return dict(shape=dict(N=300, K=8, V=25 * 32), association=out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--assoc", action="store_true")
    ap.add_argument("--parent-association", default=None)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    ctx = _abi.default_context()
    res = time_association(ctx, a.iters, a.warmup, a.parent_association) if a.assoc else time_evidence(ctx, a.iters,
                                                                                                      a.warmup)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
