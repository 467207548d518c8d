"""TEST INFRASTRUCTURE — a NumPy restatement of the keypoint detector (csrc/gc_keypoints.hip,
gcslam/ops/keypoint_detector.py), written from the definition in DESIGN.md §4 "Keypoint detector" and
from nothing else. The detector is build-defined: it follows the published algorithms (Rosten-Drummond
FAST-9/16, Harris, ORB's per-level quotas) and was not checked against OpenCV. Every stage is integer
arithmetic or a fixed sequence of IEEE f64 operations, one rounding each, so the device and this file
agree bit for bit and no comparison here carries a tolerance.

detect() returns every intermediate: the grey image, each pyramid level, each level's score map, the
candidate lists, both cuts and the output table."""

from __future__ import annotations

import math

import numpy as np

# the radius-3 circle in order (dx, dy)
CIRCLE = ((0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2), (-3, -1),
          (-3, 0), (-3, 1), (-2, 2), (-1, 3))
ARC = 9
HARRIS_BLOCK = 7
MAX_LEVELS = 16
COUNTS_LEN = 3 * MAX_LEVELS + 1


def grey(image) -> np.ndarray:
    """Step 1. (H, W, 3) rgb8 -> (H, W) uint8; an (H, W) image is grey already."""
    a = np.asarray(image)
    assert a.dtype == np.uint8
    if a.ndim == 2:
        return a.copy()
    r, g, b = (a[..., q].astype(np.int32) for q in range(3))
    return ((4899 * r + 9617 * g + 1868 * b + 8192) >> 14).astype(np.uint8)


def plan(H: int, W: int, nfeatures: int = 512, scale_factor: float = 1.2, nlevels: int = 8):
    """Step 2. The scales, the level sizes (W_l, H_l), the quotas and the candidate capacities."""
    sf = float(np.float32(scale_factor))
    scales = [float(np.float32(math.pow(sf, float(l)))) for l in range(nlevels)]
    sizes = [(max(1, int(np.rint(W / s))), max(1, int(np.rint(H / s)))) for s in scales]
    f = 1.0 / sf
    nd = nfeatures * (1.0 - f) / (1.0 - math.pow(f, float(nlevels)))
    quotas = []
    for _ in range(nlevels - 1):
        quotas.append(int(np.rint(nd)))
        nd *= f
    quotas.append(max(nfeatures - sum(quotas), 0))
    caps = [((w + 1) // 2) * ((h + 1) // 2) for w, h in sizes]
    return dict(scales=scales, sizes=sizes, quotas=quotas, caps=caps)


def resize_table(n_src: int, n_dst: int):
    """Step 3, one axis: i0 (int32) and w1 (int32, of 2048) per destination index."""
    j = np.arange(n_dst, dtype=np.float64)
    sc = float(n_src) / float(n_dst)
    f = (j + 0.5) * sc - 0.5
    fl = np.floor(f)
    w1 = np.rint((f - fl) * 2048.0).astype(np.int64)
    i0 = fl.astype(np.int64)
    lo = i0 < 0
    i0[lo], w1[lo] = 0, 0
    hi = i0 >= n_src - 1
    i0[hi], w1[hi] = n_src - 1, 0
    return i0.astype(np.int32), w1.astype(np.int32)


def resize(src: np.ndarray, W_d: int, H_d: int) -> np.ndarray:
    """Step 3. 8-bit bilinear with 11-bit weights, integer throughout."""
    H_s, W_s = src.shape
    x0, wx = (a.astype(np.int64) for a in resize_table(W_s, W_d))
    y0, wy = (a.astype(np.int64) for a in resize_table(H_s, H_d))
    x1, y1 = np.minimum(x0 + 1, W_s - 1), np.minimum(y0 + 1, H_s - 1)
    p = src.astype(np.int64)
    top = p[y0][:, x0] * (2048 - wx)[None, :] + p[y0][:, x1] * wx[None, :]
    bot = p[y1][:, x0] * (2048 - wx)[None, :] + p[y1][:, x1] * wx[None, :]
    acc = top * (2048 - wy)[:, None] + bot * wy[:, None]
    assert acc.max(initial=0) + (1 << 21) < (1 << 31)
    return ((acc + (1 << 21)) >> 22).astype(np.uint8)


def fast_scores(img: np.ndarray, threshold: int) -> np.ndarray:
    """Step 4. The score map (H, W) int32: m - 1 at the corners (m > threshold), 0 elsewhere."""
    H, W = img.shape
    out = np.zeros((H, W), np.int32)
    if H < 7 or W < 7:
        return out
    p = img.astype(np.int32)
    c = p[3:H - 3, 3:W - 3]
    d = np.stack([p[3 + dy:H - 3 + dy, 3 + dx:W - 3 + dx] - c for dx, dy in CIRCLE])   # I_k - I_p
    lo = np.stack([np.min(np.stack([d[(k + q) % 16] for q in range(ARC)]), axis=0) for k in range(16)])
    hi = np.stack([np.min(np.stack([-d[(k + q) % 16] for q in range(ARC)]), axis=0) for k in range(16)])
    m = np.maximum(lo.max(axis=0), hi.max(axis=0))
    out[3:H - 3, 3:W - 3] = np.where(m > threshold, m - 1, 0)
    return out


def nms(score: np.ndarray) -> np.ndarray:
    """Step 5. True where the score is a corner's and strictly above all eight neighbours'."""
    H, W = score.shape
    pad = np.zeros((H + 2, W + 2), score.dtype)
    pad[1:-1, 1:-1] = score
    keep = score > 0
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx or dy:
                keep &= score > pad[1 + dy:H + 1 + dy, 1 + dx:W + 1 + dx]
    return keep


def harris_sums(img: np.ndarray, xs, ys):
    """Step 8, the integer half: a, b, c (int64) of the 7 x 7 block about each (x, y)."""
    p = img.astype(np.int64)
    xs, ys = np.asarray(xs, np.int64), np.asarray(ys, np.int64)
    r = HARRIS_BLOCK // 2
    oy, ox = np.meshgrid(np.arange(-r, r + 1), np.arange(-r, r + 1), indexing="ij")
    Y = ys[:, None, None] + oy[None]
    X = xs[:, None, None] + ox[None]
    g = lambda dy, dx: p[Y + dy, X + dx]
    Ix = 2 * (g(0, 1) - g(0, -1)) + (g(-1, 1) - g(-1, -1)) + (g(1, 1) - g(1, -1))
    Iy = 2 * (g(1, 0) - g(-1, 0)) + (g(1, -1) - g(-1, -1)) + (g(1, 1) - g(-1, 1))
    return (Ix * Ix).sum(axis=(1, 2)), (Iy * Iy).sum(axis=(1, 2)), (Ix * Iy).sum(axis=(1, 2))


def harris_scale() -> float:
    q = 1.0 / (4.0 * 7.0 * 255.0)
    q2 = q * q
    return q2 * q2


def harris_tail(a, b, c, harris_k: float) -> np.ndarray:
    """Step 8, the seven f64 operations, one rounding each."""
    a, b, c = (np.asarray(v, np.int64).astype(np.float64) for v in (a, b, c))
    t1 = a * b
    t2 = c * c
    t3 = t1 - t2
    s = a + b
    t4 = s * s
    t5 = np.float64(harris_k) * t4
    return (t3 - t5) * np.float64(harris_scale())


def detect(image, nfeatures=512, scale_factor=1.2, nlevels=8, edge=31, fast_threshold=20, harris_k=0.04):
    """Steps 1-10. Returns grey, levels, scores, per level the candidate list (after the border), the
    first cut and the second cut, the (nfeatures, 3) table and (nfeatures, 4) meta with their zero
    tails, counts (COUNTS_LEN int32: [nms, border, kept] per level, the total last) and total."""
    g = grey(image)
    H, W = g.shape
    pl = plan(H, W, nfeatures, scale_factor, nlevels)
    levels, scores, cands, cut1, cut2 = [g], [], [], [], []
    counts = np.zeros(COUNTS_LEN, np.int32)
    table = np.zeros((nfeatures, 3), np.float64)
    meta = np.zeros((nfeatures, 4), np.int32)
    row = 0
    for l in range(nlevels):
        W_l, H_l = pl["sizes"][l]
        if l > 0:
            levels.append(resize(levels[l - 1], W_l, H_l))
        img = levels[l]
        sc = fast_scores(img, fast_threshold)
        scores.append(sc)
        keep = nms(sc)
        ys, xs = np.nonzero(keep)                       # raster order
        counts[3 * l] = xs.shape[0]
        assert xs.shape[0] <= pl["caps"][l]
        inb = (xs >= edge) & (xs < W_l - edge) & (ys >= edge) & (ys < H_l - edge)
        xs, ys = xs[inb], ys[inb]
        counts[3 * l + 1] = xs.shape[0]
        fs = sc[ys, xs]
        ras = ys.astype(np.int64) * W_l + xs
        cands.append(dict(x=xs, y=ys, score=fs, raster=ras))
        n_l = pl["quotas"][l]
        o1 = np.lexsort((ras, -fs))[:2 * n_l]           # descending score, then ascending raster index
        xs, ys, fs, ras = xs[o1], ys[o1], fs[o1], ras[o1]
        a, b, c = harris_sums(img, xs, ys) if xs.shape[0] else (np.zeros(0, np.int64),) * 3
        resp = harris_tail(a, b, c, harris_k)
        cut1.append(dict(x=xs, y=ys, score=fs, raster=ras, response=resp, a=a, b=b, c=c))
        o2 = np.lexsort((ras, -resp))[:n_l]             # descending response, then ascending raster index
        o2 = o2[:nfeatures - row]                       # rounded quotas never overrun the table
        xs, ys, fs, ras, resp = xs[o2], ys[o2], fs[o2], ras[o2], resp[o2]
        cut2.append(dict(x=xs, y=ys, score=fs, raster=ras, response=resp))
        k = xs.shape[0]
        counts[3 * l + 2] = k
        s_l = np.float64(pl["scales"][l])
        table[row:row + k, 0] = xs.astype(np.float64) * s_l
        table[row:row + k, 1] = ys.astype(np.float64) * s_l
        table[row:row + k, 2] = resp
        meta[row:row + k, 0] = l
        meta[row:row + k, 1] = xs
        meta[row:row + k, 2] = ys
        meta[row:row + k, 3] = fs
        row += k
    counts[COUNTS_LEN - 1] = row
    return dict(grey=g, plan=pl, levels=levels, scores=scores, cands=cands, cut1=cut1, cut2=cut2, table=table,
                meta=meta, counts=counts, total=row)
