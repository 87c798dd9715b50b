"""Scenes that make the footprint cull and the compositors decide AGAINST the image's far edges: the last tile column, the
last tile row and the corner tile of images whose width and height leave 1 .. 9 live columns or rows there, images smaller
than a tile or one pixel thin, and the two images of 65520 px.  Built with the machinery of tests/list_edge_scenes.py
(identity-rotation camera, entries at known depths, `model()` for the designed facts and its refusals of anything near a
threshold); tests/test_far_edges_cpu.py holds every scene against oracle-R.

A far-edge tile with w live columns and h live rows (tile-relative coordinates, pixel centres on the integers) gets
  in         thin (0.9 px, 0.016) centred in a pixel of the last live column / row, 0.05 px off its centre.  (Not ON the
             centre: a float32 centre an ulp off it makes `power` a rounding-sized number of either sign, which oracle-R
             rightly calls fragile.)
  over       wide (1.4 px, 0.04), 2 px beyond the image border (2.5 px beyond the last pixel centre): it reaches the last
             live column / row and not the one before it (3.5 px);
  corner     wide at (w + 1.5, h + 0.5): d^2 = 8.5 to pixel (w - 1, h - 1), 12.5 and 14.5 to its two neighbours;
  miss       wide, 3.5 px beyond the last pixel centre: the 3 sigma square (radius 5) still holds the tile, the footprint
             reaches no live pixel and no clipped strip: in the list under FLAG_NO_CULL, absent under the default cull;
  dead-drop  (h <= 12) wide, centred in a strip without a live row, at least 3.5 rows below the last live one: dropped;
  dead-keep  (h <= 12) thin, centred 1.05 rows below the last live row, which it reaches: kept.
Wide entries sit midway between pixel centres and thin ones 0.05 px off a centre.  With the 6 % anisotropy turned any way, a
wide entry's alpha >= 1/255 footprint ends at d^2 = 9.4 .. 11.6 and a thin one's at 2.9 .. 3.4; squared distances from such
centres to pixel centres are 8.5 or 12.5 and 2.2 or 3.8 around those bands, so no pixel of any tile sits on a footprint's rim.
LONG adds a stack of thin entries on the live pixels of the corner tile so that its KEPT list has exactly 65 / 257 entries.

n_contrib is a position in the list the device walks, which under the default cull is the kept list, while oracle-R
numbers the whole list.  The depths are therefore assigned so that in every tile the pairs the cull drops lie behind every
entry a pixel of that tile blends: a topological order of those constraints, with the entry kinds as the tie-break.  Then
n_contrib is the same number in both lists (asserted), and the GPU tests compare it with the oracle's unchanged.  Every
Gaussian has its own depth (2 + 0.01 k), so no list has a near-tie.
The shifted views of the batch scene admit no such order (inside the image two neighbours drop each other's pairs in the
tiles either spills into, a cycle), so it holds for their view 0 only; for the other views `kept_numbering` maps the oracle's
n_contrib to a position in the kept list, through the model's `kept` masks, whose counts the device's list lengths are held to.
"""
import heapq
import math

import numpy as np
import torch

import list_edge_scenes as S

TILE = S.TILE
WIDE, THIN = (1.4, 1.4, 0.04), (0.9, 0.9, 0.016)
CORE = ((33, 17), (47, 20), (34, 41))                                  # (W, H)
SIZES = ((33, 17), (18, 35), (47, 20), (17, 21), (31, 24), (34, 41))
SMALL = ((1, 1), (16, 1), (1, 16), (3, 2), (257, 1), (1, 257))
LONG = {(33, 17): 257, (47, 20): 65}                                   # kept entries of the corner tile (H % 16 = 1 and 4)
KINDS = ("in", "dead-keep", "stack", "over", "corner", "miss", "dead-drop")
BIG = 65520
BIG_FOCAL = 65520.0                                                    # tan(fov / 2) = 0.5 on the long axis


def name_of(size):
    return f"{size[0]}x{size[1]}"


def tile_entries(w, h, last_col, last_row):
    """-> [(kind, cx, cy, sigma_x, sigma_y, opacity)] of one far-edge tile, tile-relative."""
    xl, yl, xd = min(w - 1, 6), min(h - 1, 6), min(w - 1, 9)           # live places; in a whole tile their 3 sigma squares stay inside
    # (an entry beyond one edge keeps 2.5 px from the tile's other near edge: in a tile of one or two live rows an over-x entry
    # would reach the tile above, which drops the over-y entry, while the tile to the left blends that one and drops this)
    xo, yo = xl + (0.5 if xl >= 2 else 1.5), yl + (0.5 if yl >= 2 else 1.5)
    out = []
    if last_col:
        out += [("in", w - 0.95, yl + 0.05) + THIN, ("over", w + 1.5, yo) + WIDE, ("miss", w + 2.5, yo) + WIDE]
    if last_row:
        out += [("in", xl + 0.05, h - 0.95) + THIN, ("over", xo, h + 1.5) + WIDE, ("miss", xo, h + 2.5) + WIDE]
        if h <= 12:
            out += [("dead-drop", xd + 0.5, max(h + 2.5, 4 * math.ceil(h / 4) + 0.5)) + WIDE, ("dead-keep", xd + 0.05, h + 0.05) + THIN]
    if last_col and last_row:
        out.append(("corner", w + 1.5, h + 0.5) + WIDE)
    return out


def stack_entries(w, h, n):
    """n thin entries on live places of a tile, taken in turn."""
    cs = sorted({(min(w - 1, cx) + 0.05, min(h - 1, cy) + 0.05) for cx in (0, 5, 10) for cy in (0, 2, 6)})
    return [("stack",) + cs[i % len(cs)] + THIN for i in range(n)]


def far_tiles(W, H):
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    return [(tx, ty) for ty in range(gy) for tx in range(gx) if tx == gx - 1 or ty == gy - 1]


def live(W, H, tx, ty):
    return min(TILE, W - TILE * tx), min(TILE, H - TILE * ty)


def _place(W, H, tiles, extra):
    """-> rows [(px, py, sx, sy, o, kind, tx, ty)] of the far-edge entries of `tiles` plus extra[(tx, ty)] stack entries."""
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    rows = []
    for (tx, ty) in tiles:
        w, h = live(W, H, tx, ty)
        ent = tile_entries(w, h, tx == gx - 1, ty == gy - 1) + stack_entries(w, h, extra.get((tx, ty), 0))
        rows += [(TILE * tx + cx, TILE * ty + cy, sx, sy, o, kind, tx, ty) for kind, cx, cy, sx, sy, o in ent]
    return rows


def _finish(name, W, H, rows, order, seed, views, focal, depth_sigma):
    b = S._Builder(H, W, seed, focal=focal, depth_sigma=depth_sigma)
    for k, i in enumerate(order):
        px, py, sx, sy, o, kind, tx, ty = rows[i]
        b.rows.append((px, py, 2.0 + 0.01 * k, sx, sy, o, tx, ty, i))       # (the `pos` column carries the entry's index in rows)
    return b.finish(name, views=views)


def _order(rows, sc, corner):
    """Depth order: in every tile of view 0 the dropped pairs behind the blended ones; ties by (kind, corner tile last)."""
    n = len(rows)
    back = sc.pos                                                      # Gaussian -> rows index
    succ, indeg = [set() for _ in range(n)], np.zeros(n, dtype=np.int64)
    for f in sc.facts[:1]:
        for t, ids in f.lists.items():
            ids = np.asarray(ids)
            for d in back[ids[~f.kept[t]]]:
                for u in back[ids[f.blended_in[t]]]:
                    if d not in succ[u]:
                        succ[u].add(d)
                        indeg[d] += 1
    key = lambda i: (KINDS.index(rows[i][5]), rows[i][6:8] == corner, i)
    heap = [key(i) for i in range(n) if indeg[i] == 0]
    heapq.heapify(heap)
    out = []
    while heap:
        i = heapq.heappop(heap)[2]
        out.append(i)
        for d in succ[i]:
            indeg[d] -= 1
            if indeg[d] == 0:
                heapq.heappush(heap, key(d))
    assert len(out) == n, "the scene has no depth order that keeps the dropped pairs behind the blended ones"
    return out


def build(name, W, H, tiles=None, long_corner=0, seed=0, views=None, focal=S.FOCAL, depth_sigma=1.0, stacks=None):
    """The far-edge entries in `tiles` (default: every far-edge tile); long_corner: kept length wanted for the corner tile;
    stacks: {tile: thin entries to add}."""
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    corner = (gx - 1, gy - 1)
    tiles = far_tiles(W, H) if tiles is None else tiles
    extra = dict(stacks or {})
    for _ in range(3):
        rows = _place(W, H, tiles, extra)
        sc = _finish(name, W, H, rows, range(len(rows)), seed, views, focal, depth_sigma)
        have = int(sc.facts[0].tile_len_cull[corner[1], corner[0]])
        if not long_corner or have == long_corner:
            break
        extra[corner] = extra.get(corner, 0) + long_corner - have      # (every stack entry is kept: one correction suffices)
    sc = _finish(name, W, H, rows, _order(rows, sc, corner), seed, views, focal, depth_sigma)
    sc.rows, sc.corner, sc.far_tiles = rows, corner, tiles
    sc.kind = np.array([rows[i][5] for i in sc.pos])
    sc.home = np.array([rows[i][6:8] for i in sc.pos], dtype=np.int64)
    _assert_designed(sc, long_corner)
    return sc


def _assert_designed(sc, long_corner):
    """What the scene was built for, from model().  In view 0 the kept list numbers like the whole one, and for
    every far-edge tile: each of its entries is in its list; the miss and dead-drop entries are dropped by the cull and
    reach no live pixel, every other entry is kept; an `in` entry reaches the pixel it is centred in, an `over` entry the
    last live column (row) and nothing else, the corner entry pixel (w - 1, h - 1) alone, a dead-keep entry the last live
    row alone; the corner entry is the last the corner pixel blends (n_contrib there is its list position); exactly the
    miss and dead-drop Gaussians are dead."""
    W, H = sc.W, sc.H
    f = sc.facts[0]
    assert np.array_equal(f.n_contrib_cull, f.n_contrib), f"{sc.name}: a dropped pair lies in front of a blended one"
    drops = 0
    for t in sc.far_tiles:
        ids = np.asarray(f.lists[t])
        w, h = live(W, H, *t)
        last_col, last_row = t[0] == sc.corner[0], t[1] == sc.corner[1]
        mine = np.nonzero((sc.home[ids] == np.array(t)).all(axis=1))[0]
        want = tile_entries(w, h, last_col, last_row)
        assert sorted(sc.kind[ids[mine]][sc.kind[ids[mine]] != "stack"]) == sorted(k for k, *_ in want), f"{sc.name} {t}: an entry is not in its tile's list"
        for j in mine:
            kind, cx, cy = sc.rows[sc.pos[ids[j]]][5], sc.rows[sc.pos[ids[j]]][0] - TILE * t[0], sc.rows[sc.pos[ids[j]]][1] - TILE * t[1]
            hit = f.hits[t][:, j].reshape(TILE, TILE)
            tag = f"{sc.name} tile {t}: {kind} at ({cx:.2f}, {cy:.2f})"
            if kind in ("miss", "dead-drop"):
                assert not f.kept[t][j] and not hit.any(), tag
                drops += 1
                continue
            assert f.kept[t][j] and f.blended_in[t][j], tag + " is not kept"
            if kind == "in":
                assert hit[int(round(cy)), int(round(cx))], tag
            elif kind == "over" and cy < h + 1:              # beyond the last column (an over-y entry sits at h + 1.5)
                assert hit[:, w - 1].any() and not hit[:, :w - 1].any(), tag
            elif kind in ("over", "dead-keep"):
                assert hit[h - 1].any() and not hit[:h - 1].any(), tag
            elif kind == "corner":
                assert hit[h - 1, w - 1] and hit.sum() == 1, tag
                assert f.n_contrib[TILE * t[1] + h - 1, TILE * t[0] + w - 1] == j + 1, tag + " is not the corner pixel's last"
        assert f.tile_len_cull[t[1], t[0]] < f.tile_len[t[1], t[0]]
    gone = np.isin(sc.kind, ("miss", "dead-drop"))
    assert not f.blended[gone].any() and f.blended[~gone].all(), f"{sc.name}: the Gaussians no pixel of view 0 blends"
    sc.designed_drops = drops                                          # miss / dead-drop pairs of the far-edge tiles' own entries
    if long_corner:
        cx, cy = sc.corner
        assert f.tile_len_cull[cy, cx] == long_corner and f.final_T.min() > 1e-3, (f.tile_len_cull[cy, cx], f.final_T.min())


def batch_views(W, H):
    """Three views of one scene: as built; the image moved a whole tile left and half a tile up, so that what sat against
    the far edges lies inside it (or crosses the top edge); and half a tile left and half a tile down, so that the last tile
    row leaves the image while the last tile column's entries lie inside it."""
    return [S.camera(H, W), S.camera(H, W, yaw_px=-16.0, pitch_px=-8.0), S.camera(H, W, yaw_px=-8.0, pitch_px=8.0)]


def big(horizontal):
    """65520 x 17 (or 17 x 65520): 4095 tiles along the long axis, one live row (column) in the second tile row (column).
    Entries in the first, the middle and the last tile of the long axis, in both tile rows; the last one holds in, over and
    miss entries against the far end.  Compared with oracle-R on `tile_windows` around the three places."""
    W, H = (BIG, 17) if horizontal else (17, BIG)
    places = (0, 2047, 4094)
    tiles = [(p, s) if horizontal else (s, p) for p in places for s in (0, 1)]
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    tiles = [t for t in tiles if t[0] == gx - 1 or t[1] == gy - 1]     # (tile_entries places nothing in an inner tile)
    stacks = {t: 6 for t in tiles}
    cam = S.camera(H, W, focal=BIG_FOCAL)
    sc = build(name_of((W, H)), W, H, tiles=tiles, seed=41 + horizontal, views=[cam], focal=BIG_FOCAL, depth_sigma=0.02,
               stacks=stacks)
    win = [(max(0, p - 1), p + 2) for p in places]
    sc.tile_windows = [(a, 0, b, gy) if horizontal else (0, a, gx, b) for a, b in win]
    sc.tile_windows = [(x0, y0, min(x1, gx), min(y1, gy)) for x0, y0, x1, y1 in sc.tile_windows]
    sc.horizontal = horizontal
    return sc


def crop(sc, t):
    """The scene's tile windows of an [..., H, W] tensor, side by side along the long axis."""
    parts = [t[..., TILE * y0:TILE * y1, TILE * x0:TILE * x1] for (x0, y0, x1, y1) in sc.tile_windows]
    return torch.cat(parts, dim=-1 if sc.horizontal else -2)


_CACHE = {}


def get(key):
    """key: a (W, H) of SIZES / SMALL, ('batch', 3), or ('big', horizontal).  Built once per process."""
    if key not in _CACHE:
        if key[0] == "batch":
            W, H = 33, 17
            _CACHE[key] = build("33x17 batch", W, H, seed=31, views=batch_views(W, H))
            _CACHE[key].oracle_key = "33x17 batch"
        elif key[0] == "big":
            _CACHE[key] = big(key[1])
        else:
            W, H = key
            _CACHE[key] = build(name_of(key), W, H, long_corner=LONG.get(key, 0), seed=100 + W + 7 * H)
    return _CACHE[key]


def first_blended(f):
    """facts of a view -> first kept entry of every list, where some pixel blends it: its gradient must not be zero."""
    out = set()
    for t, ids in f.lists.items():
        k = np.nonzero(f.kept[t])[0]
        if len(k) and f.blended[ids[k[0]]]:
            out.add(int(ids[k[0]]))
    return sorted(out)


def kept_numbering(f, n_contrib):
    """An [H, W] n_contrib that numbers whole lists (oracle-R's) -> the same entries numbered along the kept lists."""
    out = np.array(n_contrib, dtype=np.int64)
    H, W = out.shape
    for (tx, ty), kept in f.kept.items():
        rank = np.concatenate([[0], np.cumsum(kept)])
        blk = out[TILE * ty:min(TILE * (ty + 1), H), TILE * tx:min(TILE * (tx + 1), W)]
        blk[...] = rank[blk]
    return out
