"""The float64 / int64 referee of swf_gftt_detect_batch (include/swf_solver.h): stages A to D and the packing, written from
the specification and from nothing else.  Everything up to D is int64 arithmetic, the eigenvalue is one float64 expression evaluated
operation by operation (numpy does not contract), and the selection is the sequential walk itself.  free() is evaluated from the list
of kept centres, as on the device; tests/test_gftt.py holds it to a restatement that rasterises a byte mask, as the reference does."""
import math
import zlib

import numpy as np

OK, BAD_INPUT, TOO_MANY = 0, 1, 2
KEPT, OUTSIDE, CROWDED = 0, 1, 2
NMAX = 1024
SCALE = 18727200.0                                  # (255 * 4 * 3)^2 * 2
DEFAULTS = dict(max_cnt=350, min_dist=30, quality=0.01, cand_cap=1 << 15, flags=1)


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes()) & 0xFFFFFFFF


def default_halfwidth(r):
    return [math.isqrt(r * r - d * d) for d in range(r + 1)]


def tensor(img):
    """Ix, Iy and the 3 x 3 sums A, B, C, D of an 8-bit image, all int64"""
    P = np.pad(img.astype(np.int64), 1, mode="reflect")
    ix = (P[:-2, 2:] - P[:-2, :-2]) + 2 * (P[1:-1, 2:] - P[1:-1, :-2]) + (P[2:, 2:] - P[2:, :-2])
    iy = (P[2:, :-2] - P[:-2, :-2]) + 2 * (P[2:, 1:-1] - P[:-2, 1:-1]) + (P[2:, 2:] - P[:-2, 2:])
    h, w = img.shape

    def box(v):
        Q = np.pad(v, 1, mode="reflect")
        return sum(Q[j:j + h, i:i + w] for j in range(3) for i in range(3))
    A, B, C = box(ix * ix), box(ix * iy), box(iy * iy)
    return dict(ix=ix, iy=iy, A=A, B=B, C=C, D=(A - C) ** 2 + 4 * B * B)


def eig_image(img):
    T = tensor(img)
    return ((T["A"] + T["C"]).astype(np.float64) - np.sqrt(T["D"].astype(np.float64))) / SCALE


def staged(px, flags):
    px = np.asarray(px, np.float64).reshape(-1, 2)
    with np.errstate(over="ignore"):
        return px.astype(np.float32).astype(np.float64) if flags & 1 else px.copy()


def in_disc(c, x, y, r, hw):
    dy = abs(y - c[1])
    return dy <= r and abs(x - c[0]) <= hw[dy]


def is_free(x, y, kept, r, hw, mask):
    if mask is not None and mask[y, x] == 0:
        return False
    return not any(in_disc(c, x, y, r, hw) for c in kept)


def free_map(rows, cols, kept, r, hw, mask):
    """free() of every pixel, from the centres"""
    Y, X = np.mgrid[0:rows, 0:cols]
    table = np.asarray(hw, np.int64)
    fm = np.ones((rows, cols), bool) if mask is None else mask != 0
    for cx, cy in kept:
        dy = np.abs(Y - cy)
        fm &= ~((dy <= r) & (np.abs(X - cx) <= table[np.minimum(dy, r)]))
    return fm


def stage_a(rows, cols, px, track_cnt, r, hw, mask):
    """the walk of setMask over staged positions -> (order, why, kept centres)"""
    n = px.shape[0]
    why = np.full(n, -1, np.int32)
    order, kept = [], []
    for i in sorted(range(n), key=lambda i: (-int(track_cnt[i]), i)):
        cx, cy = np.rint(px[i, 0]), np.rint(px[i, 1])
        if not (0 <= cx < cols and 0 <= cy < rows):
            why[i] = OUTSIDE
        elif not is_free(int(cx), int(cy), kept, r, hw, mask):
            why[i] = CROWDED
        else:
            why[i] = KEPT
            order.append(i)
            kept.append((int(cx), int(cy)))
    return order, why, kept


def candidates(eig, fm, quality):
    """stage C -> (m or None, t image, boolean candidate image)"""
    rows, cols = eig.shape
    none = np.zeros((rows, cols), bool)
    if not fm.any():
        return None, np.zeros_like(eig), none
    m = float(eig[fm].max())
    if m == 0.0:
        return m, np.zeros_like(eig), none
    thr = quality * m
    t = np.where(eig > thr, eig, 0.0)
    top = np.ones((rows - 2, cols - 2), bool)
    for j in range(3):
        for i in range(3):
            top &= t[1:-1, 1:-1] >= t[j:j + rows - 2, i:i + cols - 2]
    cand = none.copy()
    cand[1:-1, 1:-1] = top & (t[1:-1, 1:-1] != 0)
    return m, t, cand & fm


def select(t, cand, cols, r, budget):
    """stage D -> the new points [n_new][2] in selection order"""
    idx = np.flatnonzero(cand.ravel())
    tv = t.ravel()[idx]
    walk = idx[np.lexsort((idx, tv))[::-1]]              # t descending, then the linear index descending
    kept = np.zeros((0, 2), np.int64)
    for p in walk:
        if kept.shape[0] >= budget:
            break
        q = np.array([p % cols, p // cols], np.int64)
        if kept.shape[0] == 0 or (((kept - q) ** 2).sum(axis=1) >= r * r).all():
            kept = np.vstack([kept, q])
    return kept


def detect_frame(img, px, track_cnt, mask=None, max_cnt=350, min_dist=30, quality=0.01, disc_halfwidth=None, cand_cap=1 << 15, flags=1):
    """one frame -> dict(info, order, why, n_old, new_px, n_new, n_cand, max_eig, eig, pack_px, pack_src); a BAD_INPUT frame has its
    info only, a TOO_MANY frame info and n_cand.  order is padded with -1 to the number of tracked points; eig is None where the
    detector was skipped."""
    rows, cols = img.shape
    p = staged(px, flags)
    tc = np.asarray(track_cnt, np.int64).reshape(-1)
    assert p.shape[0] == tc.size <= NMAX
    if not np.isfinite(p).all() or (tc < 0).any():
        return dict(info=BAD_INPUT)
    r = int(min_dist)
    hw = default_halfwidth(r) if disc_halfwidth is None else [int(v) for v in disc_halfwidth]
    order, why, kept = stage_a(rows, cols, p, tc, r, hw, mask)
    n_old = len(order)
    out = dict(info=OK, why=why, n_old=n_old, order=np.array(order + [-1] * (p.shape[0] - n_old), np.int32).reshape(-1))
    budget = max_cnt - n_old
    if budget <= 0:
        out.update(new_px=np.zeros((0, 2)), n_new=0, n_cand=0, max_eig=0.0, eig=None)
    else:
        eig = eig_image(img)
        m, t, cand = candidates(eig, free_map(rows, cols, kept, r, hw, mask), quality)
        n_cand = int(cand.sum())
        if n_cand > cand_cap:
            return dict(info=TOO_MANY, n_cand=n_cand)
        new = select(t, cand, cols, r, budget)
        out.update(new_px=new.astype(np.float64), n_new=new.shape[0], n_cand=n_cand, max_eig=0.0 if m is None else m, eig=eig)
    out["pack_px"] = np.concatenate([p[order].reshape(-1, 2), out["new_px"]])
    out["pack_src"] = np.array(order + [-1] * out["n_new"], np.int32).reshape(-1)
    return out


def pack(results):
    """the packed outputs of a call from its frames' results -> (pack_first, pack_px, pack_src)"""
    tot = [r["pack_src"].size if r["info"] == OK else 0 for r in results]
    first = np.concatenate([[0], np.cumsum(tot)]).astype(np.int32)
    px = np.concatenate([r["pack_px"] for r in results if r["info"] == OK] + [np.zeros((0, 2))])
    src = np.concatenate([r["pack_src"] for r in results if r["info"] == OK] + [np.zeros(0, np.int32)]).astype(np.int32)
    return first, px, src
