"""NumPy / Python restatement of the in-painting masks (adm_amd/csrc/inpaint_data.hip), for the tests and for
tools/make_golden_inpaint.py.  No GPU, no PIL, no reference import.

``candidate`` consumes one slab of the fixed slot table as ddm.data.InpaintDataset.random_mask / RandomBrush (ddm/data.py:404-476
of the reference) consume their numpy draws, in Python float64 and in their operation order; ``geometry`` walks the candidates of one
sample and keeps the first that covers a pixel; ``pack`` lays samples out as the kernel does; ``raster`` is the integer definition
of the mask; ``analytic_gap`` measures how far a pixel lies from the analytic boundary of the strokes."""
import math

import numpy as np
import torch

from adm_amd.ddm.inpaint_data import (CANDIDATES, NU, NZ, RECTS, S_ANGLE_MAX, S_ANGLE_MIN, S_ANGLES, S_NUM_VERTEX, S_START, S_WIDTH,
                                      SEGMENTS, STROKE_U, STROKES, U_FLIP, U_NRECT_BIG, U_NRECT_SMALL, U_NSTROKE, U_RECT, U_STROKE,
                                      VERTS)


def randint(u, lo, hi):
    return lo + int(math.floor(float(u) * (hi - lo)))


def uniform(u, a, b):
    return a + (b - a) * float(u)


def clip(v, lo, hi):
    return lo if v < lo else (hi if v > hi else v)


def raw_rect(u4, max_size, S):
    """Fill(max_size) (data.py:408-412): the drawn (x, y, w, h), not clipped."""
    w, h = randint(u4[0], 0, max_size), randint(u4[1], 0, max_size)
    ww, hh = w // 2, h // 2
    return randint(u4[2], -ww, S - w + ww), randint(u4[3], -hh, S - h + hh), w, h


def clip_rect(x, y, w, h, S):
    """{x0, y0, x1, y1} clipped to the image; zeros when it covers no pixel."""
    r = (max(x, 0), max(y, 0), min(x + w, S), min(y + h, S))
    return r if r[0] < r[2] and r[1] < r[3] else (0, 0, 0, 0)


def candidate(u, z, S):
    """One slab (u [NU], z [NZ]) -> {'raw_rects': [(slot, x, y, w, h)], 'strokes': [(vertices, width)], 'flips': (axis 0, axis 1)}."""
    rects = [(j,) + raw_rect(u[U_RECT + 4 * j:U_RECT + 4 * j + 4], S // 2, S) for j in range(randint(u[U_NRECT_SMALL], 0, RECTS))]
    if randint(u[U_NRECT_BIG], 0, 2):
        rects.append((RECTS - 1,) + raw_rect(u[U_RECT + 4 * (RECTS - 1):U_RECT + 4 * RECTS], S, S))
    two_pi = 2 * math.pi
    mean_angle, angle_range = two_pi / 5, two_pi / 15
    avg = math.sqrt(S * S + S * S) / 8
    scale = avg // 2
    strokes = []
    for s in range(randint(u[U_NSTROKE], 0, STROKES + 1)):
        us = u[U_STROKE + s * STROKE_U:U_STROKE + (s + 1) * STROKE_U]
        nv = randint(us[S_NUM_VERTEX], 4, VERTS)
        amin = mean_angle - uniform(us[S_ANGLE_MIN], 0, angle_range)
        amax = mean_angle + uniform(us[S_ANGLE_MAX], 0, angle_range)
        v = [(randint(us[S_START], 0, S), randint(us[S_START + 1], 0, S))]
        for i in range(nv):
            a = uniform(us[S_ANGLES + i], amin, amax)
            if i % 2 == 0:
                a = two_pi - a
            r = clip(avg + scale * float(z[s * SEGMENTS + i]), 0, 2 * avg)
            v.append((int(clip(v[-1][0] + r * math.cos(a), 0, S)), int(clip(v[-1][1] + r * math.sin(a), 0, S))))
        strokes.append((v, int(uniform(us[S_WIDTH], 12, 48))))
    return {"raw_rects": rects, "strokes": strokes, "flips": (int(float(u[U_FLIP]) > 0.5), int(float(u[U_FLIP + 1]) > 0.5))}


def is_empty(c, S):
    """Hole ratio 0, decided from the parameters: no stroke (a stroke always covers pixels of the image) and no rectangle with a
    non-empty clipped area."""
    return not c["strokes"] and not any(clip_rect(*r[1:], S) != (0, 0, 0, 0) for r in c["raw_rects"])


def geometry(u, z, S):
    """u [K, NU], z [K, NZ] -> (chosen candidate index, that candidate, whether all were empty)."""
    for k in range(u.shape[0]):
        c = candidate(u[k], z[k], S)
        if not is_empty(c, S):
            return k, c, False
    return u.shape[0] - 1, c, True


def pack(cands, S):
    """Candidates -> the kernel's arrays: rects [B,4,4] clipped, verts [B,7,18,2], nverts / widths [B,7], flips [B,2] (int32)."""
    B = len(cands)
    p = {"rects": np.zeros((B, RECTS, 4), np.int32), "verts": np.zeros((B, STROKES, VERTS, 2), np.int32),
         "nverts": np.zeros((B, STROKES), np.int32), "widths": np.zeros((B, STROKES), np.int32), "flips": np.zeros((B, 2), np.int32)}
    for b, c in enumerate(cands):
        for j, x, y, w, h in c["raw_rects"]:
            p["rects"][b, j] = clip_rect(x, y, w, h, S)
        for s, (v, w) in enumerate(c["strokes"]):
            p["verts"][b, s, :len(v)] = v
            p["nverts"][b, s], p["widths"][b, s] = len(v), w
        p["flips"][b] = c["flips"]
    return p


def geometry_batch(u, z, S):
    """u [B, K, NU], z [B, K, NZ] -> (packed arrays with 'chosen' [B], number of samples that fell back)."""
    u, z = np.asarray(u), np.asarray(z)
    picks = [geometry(u[b], z[b], S) for b in range(u.shape[0])]
    p = pack([c for _, c, _ in picks], S)
    p["chosen"] = np.array([k for k, _, _ in picks], np.int32)
    return p, sum(f for _, _, f in picks)


def raster(rects, verts, nverts, widths, flips, S):
    """The integer definition, one sample: uint8 [S, S], hole = 0 / keep = 1.  int64 throughout.  The two flips mirror the
    strokes (RandomBrush flips the mask it returns, data.py:472-475), not the rectangles."""
    py, px = np.mgrid[0:S, 0:S].astype(np.int64)
    hole = np.zeros((S, S), bool)
    for s in range(len(nverts)):
        n, w = int(nverts[s]), int(widths[s])
        v = np.asarray(verts[s], np.int64)
        d = 2 * (w // 2) + 1
        for i in range(n):
            ex, ey = px - v[i, 0], py - v[i, 1]
            hole |= 4 * (ex * ex + ey * ey) <= d * d
            if i + 1 < n:
                dx, dy = v[i + 1, 0] - v[i, 0], v[i + 1, 1] - v[i, 1]
                L2 = dx * dx + dy * dy
                if L2 > 0:
                    dot, cross = ex * dx + ey * dy, ex * dy - ey * dx
                    hole |= (dot >= 0) & (dot <= L2) & (4 * cross * cross <= w * w * L2)
    if flips[0]:
        hole = np.flip(hole, 0)
    if flips[1]:
        hole = np.flip(hole, 1)
    for x0, y0, x1, y1 in np.asarray(rects, np.int64):
        hole = hole | ((px >= x0) & (px < x1) & (py >= y0) & (py < y1))
    return np.ascontiguousarray((~hole).astype(np.uint8))


def raster_batch(p, S):
    return np.stack([raster(p["rects"][b], p["verts"][b], p["nverts"][b], p["widths"][b], p["flips"][b], S)
                     for b in range(p["rects"].shape[0])])


def host_batch(images, idx, img_flip, masks):
    """The host expression of InpaintDataset.__getitem__ (data.py:396-403) in torch on the CPU: images uint8 [N,S,S,3], masks uint8
    [B,S,S] -> (image, cond [B,3,S,S], ori_mask [B,1,S,S]) float32.  The image flip mirrors the image only."""
    x = np.stack([images[i][:, ::-1] if f else images[i] for i, f in zip(idx, img_flip)])
    img = torch.from_numpy(np.ascontiguousarray(x)).permute(0, 3, 1, 2).to(torch.float32) / 255          # ToTensor
    mask = torch.from_numpy(np.ascontiguousarray(masks))[:, None].to(torch.float32)
    mask_img = mask * img
    return img * 2 - 1, mask_img * 2 - 1, mask


def stroke_distance(px, py, strokes):
    """Distance (float64, >= 0) from points to the analytic union of the strokes -- bands of half-width w / 2 between consecutive
    vertices and discs of radius w // 2 + 1/2 at the vertices -- 0 inside it."""
    px, py = np.asarray(px, np.float64), np.asarray(py, np.float64)
    best = np.full(px.shape, np.inf)
    for v, w in strokes:
        v = np.asarray(v, np.float64)
        for i in range(len(v)):
            best = np.minimum(best, np.maximum(np.hypot(px - v[i, 0], py - v[i, 1]) - (w // 2 + 0.5), 0))
            if i + 1 < len(v):
                d = v[i + 1] - v[i]
                L = math.hypot(d[0], d[1])
                if L > 0:
                    t = ((px - v[i, 0]) * d[0] + (py - v[i, 1]) * d[1]) / L          # along the segment
                    n = np.abs((px - v[i, 0]) * d[1] - (py - v[i, 1]) * d[0]) / L    # across it
                    ox, oy = np.maximum(np.maximum(-t, t - L), 0), np.maximum(n - w / 2, 0)
                    best = np.minimum(best, np.hypot(ox, oy))
    return best


GAP_RADII = np.arange(1, 41) * 0.05          # 0.05 .. 2.0
GAP_ANGLES = np.arange(64) * (2 * math.pi / 64)
GAP_FINE_RADII = np.arange(1, 201) * 0.01
GAP_FINE_ANGLES = np.arange(1440) * (2 * math.pi / 1440)


def _escape_radius(qx, qy, strokes, radii, angles, start):
    """Per point: the smallest of ``radii`` at which one of the points at ``angles`` on the circle around it lies outside the stroke
    union (``start`` where none does)."""
    depth = np.array(start, np.float64)
    found = np.zeros(depth.shape, bool)
    for r in radii:
        todo = ~found & (depth > r)
        if not todo.any():
            continue
        sx = qx[todo, None] + r * np.cos(angles)[None]
        sy = qy[todo, None] + r * np.sin(angles)[None]
        hit = np.nonzero(todo)[0][(stroke_distance(sx, sy, strokes) > 0).any(axis=1)]
        depth[hit], found[hit] = r, True
    return depth


def analytic_gap(px, py, strokes):
    """|signed distance| from pixel centres to the boundary of the analytic stroke union.  Outside the union it is the exact
    distance to it.  Inside, it is a radius at which a point on the circle around the pixel lies outside the union, so an UPPER
    bound of the depth: the smallest on a 0.05 px ladder with 64 directions, refined on a 0.01 px ladder with 1440 directions where the
    first exceeds 1 px (the way out of a slit between two bands is narrow); 2.05 when no radius up to 2 px escapes."""
    px, py = np.asarray(px, np.float64), np.asarray(py, np.float64)
    out = stroke_distance(px, py, strokes)
    inside = out == 0
    if inside.any():
        qx, qy = px[inside], py[inside]
        depth = _escape_radius(qx, qy, strokes, GAP_RADII, GAP_ANGLES, np.full(qx.shape, GAP_RADII[-1] + 0.05))
        deep = depth > 1.0
        if deep.any():
            depth[deep] = _escape_radius(qx[deep], qy[deep], strokes, GAP_FINE_RADII, GAP_FINE_ANGLES, depth[deep])
        out = out.copy()
        out[inside] = depth
    return out


def brush_only(c, S):
    """The restated strokes of one candidate alone (no rectangles), as RandomBrush returns its mask: 1 = covered, flipped."""
    p = pack([dict(c, raw_rects=[])], S)
    return 1 - raster(p["rects"][0], p["verts"][0], p["nverts"][0], p["widths"][0], p["flips"][0], S)


def compare_strokes(cands, pil_brush, S):
    """Restated strokes vs the masks the reference's RandomBrush returned (uint8 [B,S,S], 1 = covered, flipped): (largest
    analytic_gap of a differing pixel, differing pixels, PIL's covered pixels)."""
    band, differ, covered = 0.0, 0, 0
    for c, p in zip(cands, pil_brush):
        if not c["strokes"]:
            assert not p.any()
            continue
        a = brush_only(c, S)
        if c["flips"][1]:
            a, p = np.flip(a, 1), np.flip(p, 1)
        if c["flips"][0]:
            a, p = np.flip(a, 0), np.flip(p, 0)
        covered += int((p != 0).sum())
        ys, xs = np.nonzero(a != p)
        differ += len(ys)
        if len(ys):
            band = max(band, float(analytic_gap(xs, ys, c["strokes"]).max()))
    return band, differ, covered
