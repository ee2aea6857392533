"""The float64 referee of swf_klt_track_batch, written from the specification in include/swf_solver.h: integer pyramids,
integer Scharr derivatives, OpenCV's fixed-point bilinear weights, exact integer sums for A and b, and a fixed sequence of double
operations for everything else.  Vectorised over the patch of one point; one point at a time otherwise.  No part of it is shared with
the library."""
import zlib

import numpy as np

OK, BAD_INPUT = 0, 1
TRACKED, FWD_LOST, FWD_FLAT, BACK_LOST, BACK_FLAT, BACK_FAR, BORDER = 0, 1, 2, 3, 4, 5, 6
WMAX, LMAX, NMAX = 21, 4, 4096
DEFAULTS = dict(win=21, max_level=3, back_level=1, max_count=30, eps=0.01, min_eig=1e-4, back_dist=0.5, flags=5)
K5 = np.array([1, 4, 6, 4, 1], np.int64)


def r101(i, n):
    """reflect-101 of an index array into 0 .. n - 1 (one reflection; what is still outside is clamped and never used)"""
    i = np.abs(np.asarray(i, np.int64))
    i = np.where(i > n - 1, 2 * (n - 1) - i, i)
    return np.clip(i, 0, n - 1)


def pyr_down(src):
    h, w = src.shape
    hd, wd = (h + 1) // 2, (w + 1) // 2
    s = src.astype(np.int64)
    acc = np.zeros((hd, wd), np.int64)
    ys, xs = 2 * np.arange(hd), 2 * np.arange(wd)
    for j in range(5):
        rows = s[r101(ys + j - 2, h)]
        for i in range(5):
            acc += K5[j] * K5[i] * rows[:, r101(xs + i - 2, w)]
    return ((acc + 128) >> 8).astype(np.uint8)


def level_sizes(rows, cols, win, max_level):
    """[(h, w)] of the levels 0 .. top: building stops before a level whose width or height would be <= win"""
    out = [(rows, cols)]
    while len(out) <= max_level:
        h, w = (out[-1][0] + 1) // 2, (out[-1][1] + 1) // 2
        if h <= win or w <= win:
            break
        out.append((h, w))
    return out


def pyramid(img, win, max_level):
    sizes = level_sizes(img.shape[0], img.shape[1], win, max_level)
    out = [np.ascontiguousarray(img, np.uint8)]
    for _ in sizes[1:]:
        out.append(pyr_down(out[-1]))
    return out


def pyramid_bytes(rows, cols, max_level):
    """the workspace of one pair: both images, levels 1 .. max_level whether they are built or not (win = 0 never stops)"""
    return 2 * sum(h * w for h, w in level_sizes(rows, cols, 0, max_level)[1:])


def pack_pyr(prev_pyr, cur_pyr, nbytes, fill=0):
    """the workspace layout of one pair: the levels 1 .. of prev from 0, of cur from nbytes / 2; what is not built keeps `fill`"""
    out = np.full(nbytes, fill, np.uint8)
    for base, pyr in ((0, prev_pyr), (nbytes // 2, cur_pyr)):
        for lv in pyr[1:]:
            out[base:base + lv.size] = lv.ravel()
            base += lv.size
    return out


def scharr(img, ys, xs):
    """(Ix, Iy) at the grid ys x xs (int64 coordinate vectors, any values): 0 outside the image, neighbours through r101"""
    h, w = img.shape
    P = img.astype(np.int64)
    inside = ((ys >= 0) & (ys < h))[:, None] & ((xs >= 0) & (xs < w))[None, :]

    def at(dy, dx):
        return P[r101(ys + dy, h)][:, r101(xs + dx, w)]
    ix = 3 * (at(-1, 1) - at(-1, -1)) + 10 * (at(0, 1) - at(0, -1)) + 3 * (at(1, 1) - at(1, -1))
    iy = 3 * (at(1, -1) - at(-1, -1)) + 10 * (at(1, 0) - at(-1, 0)) + 3 * (at(1, 1) - at(-1, 1))
    return np.where(inside, ix, 0), np.where(inside, iy, 0)


def weights(px, py):
    fx, fy = np.floor(px), np.floor(py)
    a, b = px - fx, py - fy
    w00 = int(np.rint((1.0 - a) * (1.0 - b) * 16384.0))
    w01 = int(np.rint(a * (1.0 - b) * 16384.0))
    w10 = int(np.rint((1.0 - a) * b * 16384.0))
    return w00, w01, w10, 16384 - w00 - w01 - w10


def outside(px, py, h, w, win):
    fx, fy = np.floor(px), np.floor(py)
    return bool(fx < -win or fx >= w or fy < -win or fy >= h) or not (np.isfinite(px) and np.isfinite(py))


def descale(v, n):
    return (v + (1 << (n - 1))) >> n


def interp(grid, wts):
    """grid [(win + 1)][(win + 1)] int64 -> win x win weighted sums"""
    w00, w01, w10, w11 = wts
    return grid[:-1, :-1] * w00 + grid[:-1, 1:] * w01 + grid[1:, :-1] * w10 + grid[1:, 1:] * w11


def intensity_grid(img, ix, iy, win):
    h, w = img.shape
    ys, xs = iy + np.arange(win + 1, dtype=np.int64), ix + np.arange(win + 1, dtype=np.int64)
    return img.astype(np.int64)[r101(ys, h)][:, r101(xs, w)]


def track_pass(pyr_i, pyr_j, prev, init, top, win, max_count, eps, min_eig, sums=None):
    """One pass for one point: template in pyr_i at prev, search in pyr_j from init.  Returns (q, lost, flat, iters [LMAX + 1],
    px [LMAX + 1][2]).  `sums`, a list, receives every exact integer sum formed (for the exactness test)."""
    half = float((win - 1) // 2)
    iters = np.full(LMAX + 1, -1, np.int32)
    px = np.zeros((LMAX + 1, 2))
    lost = flat = False
    eps2 = eps * eps
    qx = qy = 0.0
    for l in range(top, -1, -1):
        I, J = pyr_i[l], pyr_j[l]
        h, w = I.shape
        scale = 2.0 ** -l
        p_x, p_y = prev[0] * scale, prev[1] * scale
        if l == top:
            qx, qy = init[0] * scale, init[1] * scale
        else:
            qx, qy = 2.0 * qx, 2.0 * qy
        px[l] = (qx, qy)
        p_x, p_y = p_x - half, p_y - half
        if outside(p_x, p_y, h, w, win):
            lost = lost or l == 0
            continue
        ix, iy = int(np.floor(p_x)), int(np.floor(p_y))
        wts = weights(p_x, p_y)
        ys, xs = iy + np.arange(win + 1, dtype=np.int64), ix + np.arange(win + 1, dtype=np.int64)
        gx, gy = scharr(I, ys, xs)
        It = descale(interp(intensity_grid(I, ix, iy, win), wts), 9)
        Itx, Ity = descale(interp(gx, wts), 14), descale(interp(gy, wts), 14)
        s11, s12, s22 = int((Itx * Itx).sum()), int((Itx * Ity).sum()), int((Ity * Ity).sum())
        if sums is not None:
            sums.extend([(Itx * Itx), (Itx * Ity), (Ity * Ity)])
        A11, A12, A22 = float(s11) * 2.0 ** -20, float(s12) * 2.0 ** -20, float(s22) * 2.0 ** -20
        D = A11 * A22 - A12 * A12
        min_e = (A22 + A11 - np.sqrt((A11 - A22) * (A11 - A22) + 4.0 * A12 * A12)) / float(2 * win * win)
        if min_e < min_eig or D < 2.0 ** -23:
            flat = flat or l == 0
            continue
        D = 1.0 / D
        qx, qy = qx - half, qy - half
        pdx = pdy = 0.0
        n = 0
        for j in range(max_count):
            if outside(qx, qy, h, w, win):
                lost = lost or l == 0
                break
            jx, jy = int(np.floor(qx)), int(np.floor(qy))
            d = descale(interp(intensity_grid(J, jx, jy, win), weights(qx, qy)), 9) - It
            if sums is not None:
                sums.extend([d * Itx, d * Ity])
            b1, b2 = float(int((d * Itx).sum())) * 2.0 ** -20, float(int((d * Ity).sum())) * 2.0 ** -20
            dx, dy = (A12 * b2 - A22 * b1) * D, (A12 * b1 - A11 * b2) * D
            qx, qy = qx + dx, qy + dy
            n += 1
            if dx * dx + dy * dy <= eps2:
                break
            if j > 0 and abs(dx + pdx) < 0.01 and abs(dy + pdy) < 0.01:
                qx, qy = qx - dx * 0.5, qy - dy * 0.5
                break
            pdx, pdy = dx, dy
        qx, qy = qx + half, qy + half
        iters[l] = n
        px[l] = (qx, qy)
    return (qx, qy), lost, flat, iters, px


def f32(v):
    with np.errstate(over="ignore"):
        return np.asarray(v, np.float64).astype(np.float32).astype(np.float64)


def track_pair(prev_img, cur_img, prev_px, guess_px=None, win=21, max_level=3, back_level=1, max_count=30, eps=0.01, min_eig=1e-4,
               back_dist=0.5, flags=5, sums=None, pyr_fill=0):
    """One pair.  Returns dict(info, cur_px, back_px, status, why, keep_idx, n_keep, trace_iters, trace_px, pyr); a BAD_INPUT pair
    returns its info only."""
    rows, cols = prev_img.shape
    pts = np.asarray(prev_px, np.float64).reshape(-1, 2)
    n = pts.shape[0]
    as_float, use_guess, back = bool(flags & 1), bool(flags & 2), bool(flags & 4)
    gs = np.asarray(guess_px, np.float64).reshape(-1, 2) if use_guess else pts
    if as_float:
        pts, gs = f32(pts), f32(gs)
    if not (np.isfinite(pts).all() and np.isfinite(gs).all()):
        return dict(info=BAD_INPUT)
    build = max(max_level, back_level)
    pp, pc = pyramid(prev_img, win, build), pyramid(cur_img, win, build)
    top_f, top_b = min(max_level, len(pp) - 1), min(back_level, len(pp) - 1)
    cur, bk = np.zeros((n, 2)), np.zeros((n, 2))
    why = np.zeros(n, np.int32)
    t_it = np.full((n, 2, LMAX + 1), -1, np.int32)
    t_px = np.zeros((n, 2, LMAX + 1, 2))
    for i in range(n):
        q, lost, flat, it, px = track_pass(pp, pc, pts[i], gs[i], top_f, win, max_count, eps, min_eig, sums)
        c = f32(q) if as_float else np.array(q)
        cur[i], t_it[i, 0], t_px[i, 0] = c, it, px
        code = FWD_LOST if lost else FWD_FLAT if flat else TRACKED
        if back:
            q, lost, flat, it, px = track_pass(pc, pp, c, pts[i], top_b, win, max_count, eps, min_eig, sums)
            b = f32(q) if as_float else np.array(q)
            bk[i], t_it[i, 1], t_px[i, 1] = b, it, px
            dx, dy = pts[i, 0] - b[0], pts[i, 1] - b[1]
            if code == TRACKED:
                code = BACK_LOST if lost else BACK_FLAT if flat else BACK_FAR if np.sqrt(dx * dx + dy * dy) > back_dist else TRACKED
        if code == TRACKED:
            rx, ry = np.rint(c[0]), np.rint(c[1])
            if not (1.0 <= rx < cols - 1 and 1.0 <= ry < rows - 1):
                code = BORDER
        why[i] = code
    status = (why == TRACKED).astype(np.uint8)
    keep = np.flatnonzero(status).astype(np.int32)
    keep_idx = np.full(n, -1, np.int32)
    keep_idx[:keep.size] = keep
    return dict(info=OK, cur_px=cur, back_px=bk, status=status, why=why, keep_idx=keep_idx, n_keep=int(keep.size), trace_iters=t_it,
                trace_px=t_px, pyr=pack_pyr(pp, pc, pyramid_bytes(rows, cols, build), pyr_fill), levels=pp + pc)


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes()) & 0xFFFFFFFF
