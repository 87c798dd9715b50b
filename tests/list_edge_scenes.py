"""Scenes built to sit on the compositors' list-length and stop-index edges (64-entry staging batches, the walk unrolled
by two, segments of 2^GSR_SEG_SHIFT entries, the T < 1e-4 stop, strip_done), with every decision far from its threshold.

Construction.  Identity-rotation pinhole camera with a long focal length (FOCAL px: perspective stretches a footprint by
(x / z)^2 <= 1e-3), Gaussians in STACKS: the entries of one stack share a tile, sit at depths z = 2 + 0.01 i (position i in
the tile's list) and are scaled by sigma_px * z / FOCAL, so that a stack's list length and order are known by construction.
Entry kinds (sigma_px, opacity, centre in the tile):
  thin     0.9 px, 0.016: reaches the 12 pixels around its centre; six centres taken in turn, so that a pixel is reached
           by a sixth of a stack and T stays above 0.05 after 1025 entries (an alpha is at least 1/255);
  wide     1.4 px, 0.04: every 64th position (the last slot of a staging batch) and the last three of a stack;
  tiny     0.141 px, 0.999, isotropic: touches exactly the 3 x 3 pixels around its centre; runs of them finish the
           neighbours of pixel (8, 8) and then (8, 8) itself at a designed entry that stops every pixel it touches, with
           never-blended entries behind it (_blocked);
  blocker  0.854 px, 0.999 at (8.05, 8.05), isotropic (stop index 2 only);
  bar      90.3 x BAR_SY px, 0.999 (single-tile images only, where no footprint can spill): covers one strip of 4 rows.
Scales are 6 % anisotropic with a rotation about the view axis, so that dL/drotation is a well-conditioned number.

The designed facts (list length per tile with and without the default footprint cull, n_contrib per pixel as a position
in either list, Gaussians that no pixel ever blends) come from `model()`: a
plain float64 numpy statement of the forward decisions, written here independently of oracle-R, which also REFUSES a scene
whose decisions sit near an edge (radius within 0.02 of an integer, alpha within 1 % of 1/255, T' within 0.2 % of 1e-4).
Each family then asserts what it was built for (a stack of L entries gives a list of L; pixel (8, 8) stops at s).
tests/test_list_edges_cpu.py holds all of it against oracle-R.

Not reachable: a stop index of 1.  alpha is capped at 0.99, so two entries leave T' >= 1e-4 -- in float32 a coin toss, the
definition of a fragile pixel.  The smallest designed stop index is 2 (three capped entries: T' = 1e-6).
"""
import math
from types import SimpleNamespace

import numpy as np
import torch

TILE = 16
FOCAL = 2000.0
ZNEAR, ZFAR = 0.01, 100.0
SH_C0 = 0.28209479177387814
A_LENGTHS = (1, 2, 3, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 258, 319, 320, 321, 511, 512, 513,
             767, 768, 769, 1023, 1024, 1025)
B_STOPS = (2, 63, 64, 65, 66, 128, 255, 256, 257, 258, 320, 511, 512, 513)
B_LEN = 640

THIN_C = ((4.5, 4.5), (11.5, 4.5), (4.5, 11.5), (11.5, 11.5), (8.5, 8.5), (8.5, 4.5))
WIDE_C = ((7.5, 7.5), (9.5, 9.5), (5.5, 9.5), (9.5, 6.5))
BLOCK_C = (8.05, 8.05)
BAR_SY = 1.0                # (a bar's centre row within its strip is chosen per scene: the one the model accepts)
T_MARGIN = 0.002            # no T' of a reached entry within 0.2 % of 1e-4 (oracle-R's own band is about 0.01 %)
TINY_S = 0.141              # isotropic, lambda = 0.32: alpha >= 1/255 within d^2 = 3.5 -- the 3 x 3 pixels (2.2), not the next ring (3.8)
BLOCK_S = 0.854            # isotropic: its alpha = 1/255 ring (d^2 = 11.4) lies between the pixel rings 10.4 and 12.5


# ---------------------------------------------------------------------------------------------------------------------
# cameras
# ---------------------------------------------------------------------------------------------------------------------
def camera(H, W, yaw_px=0.0, pitch_px=0.0, forward=0.0, focal=FOCAL):
    """World -> view in the row-vector convention ([p, 1] @ V).  yaw_px / pitch_px: rotation that moves the image by that
    many pixels at the optical axis (a rotation moves a stack by the same amount whatever its depth); forward: translation
    along the view axis; focal: focal length in pixels (the images of 65520 px need one that keeps tan(fov / 2) at 0.5)."""
    ay, ax = math.atan(yaw_px / focal), math.atan(pitch_px / focal)
    Ry = np.array([[math.cos(ay), 0, math.sin(ay)], [0, 1, 0], [-math.sin(ay), 0, math.cos(ay)]])
    Rx = np.array([[1, 0, 0], [0, math.cos(ax), math.sin(ax)], [0, -math.sin(ax), math.cos(ax)]])
    R = Rx @ Ry                                            # column-vector rotation world -> view
    V = np.eye(4)
    V[:3, :3] = R.T
    V[3, :3] = (0.0, 0.0, -forward)
    tanx, tany = W / (2.0 * focal), H / (2.0 * focal)
    Pm = np.zeros((4, 4))
    Pm[0, 0], Pm[1, 1] = 1.0 / tanx, 1.0 / tany
    Pm[2, 2], Pm[2, 3], Pm[3, 2] = ZFAR / (ZFAR - ZNEAR), -(ZFAR * ZNEAR) / (ZFAR - ZNEAR), 1.0
    V32 = torch.tensor(V, dtype=torch.float32)
    full = V32 @ torch.tensor(Pm, dtype=torch.float32).t()
    return SimpleNamespace(H=H, W=W, tanx=tanx, tany=tany, V=V32, full=full, campos=V32.inverse()[3, :3].contiguous())


def settings(cam, bg, cls, device=None):
    """The 12-field settings tuple (oracle_r.Settings or the package's GaussianRasterizationSettings), SH degree 3."""
    mv = (lambda t: t) if device is None else (lambda t: t.to(device))
    return cls(cam.H, cam.W, cam.tanx, cam.tany, mv(bg), 1.0, mv(cam.V), mv(cam.full), 3, mv(cam.campos), False, False)


# ---------------------------------------------------------------------------------------------------------------------
# the designer's model of the forward decisions (numpy, float64)
# ---------------------------------------------------------------------------------------------------------------------
def _quat_rot(q):
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                     2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                     2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], axis=1).reshape(-1, 3, 3)


def model(means, scales, quats, opac, cam):
    """-> facts of one view: tile_len [gy, gx], n_contrib [H, W], final_T [H, W], blended [P] (some pixel blends it),
    listed [P] (it is in a list), lists {tile: Gaussian ids in list order}.  Raises if a decision sits near its edge."""
    H, W = cam.H, cam.W
    V = cam.V.double().numpy()
    pv = np.concatenate([means, np.ones((len(means), 1))], axis=1) @ V
    z = pv[:, 2]
    assert np.all(np.abs(z - 0.2) > 1.5e-4), "a Gaussian sits on the near plane"
    front = z > 0.2
    zs = np.where(front, z, 1.0)
    fx, fy = W / (2 * cam.tanx), H / (2 * cam.tany)
    J = np.zeros((len(means), 2, 3))
    J[:, 0, 0], J[:, 0, 2] = fx / zs, -fx * pv[:, 0] / zs ** 2
    J[:, 1, 1], J[:, 1, 2] = fy / zs, -fy * pv[:, 1] / zs ** 2
    Rq = _quat_rot(quats / np.linalg.norm(quats, axis=1, keepdims=True))
    S3 = Rq @ (scales[:, :, None] ** 2 * np.eye(3)[None]) @ Rq.transpose(0, 2, 1)
    M = J @ V[:3, :3].T[None]
    c2 = M @ S3 @ M.transpose(0, 2, 1)
    a, b, c = c2[:, 0, 0] + 0.3, c2[:, 0, 1], c2[:, 1, 1] + 0.3
    det = a * c - b * b
    mid = 0.5 * (a + c)
    rr = 3.0 * np.sqrt(mid + np.sqrt(np.maximum(mid * mid - det, 0.1)))
    rad = np.ceil(rr)
    px, py = fx * pv[:, 0] / zs + (W - 1) * 0.5, fy * pv[:, 1] / zs + (H - 1) * 0.5
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    edges = np.stack([(px - rad) / TILE, (px + rad + TILE - 1) / TILE, (py - rad) / TILE, (py + rad + TILE - 1) / TILE])
    near_img = front & (px > -4 * TILE) & (px < W + 4 * TILE) & (py > -4 * TILE) & (py < H + 4 * TILE)
    assert np.all(np.abs(edges - np.round(edges))[:, near_img] > 1e-3), "a tile rectangle sits on a tile edge"
    x0, x1 = np.clip(np.trunc(edges[0]), 0, gx).astype(int), np.clip(np.trunc(edges[1]), 0, gx).astype(int)
    y0, y1 = np.clip(np.trunc(edges[2]), 0, gy).astype(int), np.clip(np.trunc(edges[3]), 0, gy).astype(int)
    listed = front & ((x1 - x0) * (y1 - y0) > 0)
    assert np.all(np.abs(rr - np.round(rr))[listed] > 0.02), "a radius sits on an integer"
    order = np.argsort(z.astype(np.float32), kind="stable")
    lists = {}
    for g in order:
        if listed[g]:
            for ty in range(y0[g], y1[g]):
                for tx in range(x0[g], x1[g]):
                    lists.setdefault((tx, ty), []).append(g)
    tile_len = np.zeros((gy, gx), dtype=np.int64)
    tile_len_cull = np.zeros((gy, gx), dtype=np.int64)
    ncon = np.zeros((gy * TILE, gx * TILE), dtype=np.int64)
    ncon_cull = np.zeros((gy * TILE, gx * TILE), dtype=np.int64)
    fT = np.ones((gy * TILE, gx * TILE))
    blended = np.zeros(len(means), dtype=bool)
    # per tile, along its list: kept by the default cull / blended by a pixel of the tile / [256, L] alpha >= 1/255 at a live pixel
    keptd, blendd, hitd = {}, {}, {}
    yy, xx = np.meshgrid(np.arange(TILE), np.arange(TILE), indexing="ij")
    for (tx, ty), ids in lists.items():
        ids = np.array(ids)
        zl = z[ids]
        assert np.all(np.diff(zl) > 1e-4 * zl[:-1]) if len(ids) > 1 else True, "depths of a list are not well separated"
        tile_len[ty, tx] = len(ids)
        X, Y = (tx * TILE + xx).reshape(-1, 1), (ty * TILE + yy).reshape(-1, 1)
        inside = ((X < W) & (Y < H))[:, 0]
        dx, dy = px[ids][None] - X, py[ids][None] - Y
        power = -0.5 * (c[ids] / det[ids] * dx * dx + a[ids] / det[ids] * dy * dy) + b[ids] / det[ids] * dx * dy
        araw = opac[ids][None] * np.exp(power)
        alpha = np.minimum(0.99, araw)
        valid = alpha >= 1.0 / 255.0
        Tin = np.cumprod(np.where(valid, 1.0 - alpha, 1.0), axis=1)
        stop = valid & (Tin < 1e-4)
        alive = np.cumsum(stop, axis=1) == 0
        reach = (alive | (np.cumsum(stop, axis=1) == 1) & stop) & inside[:, None]
        near = reach & (np.abs(araw * 255.0 - 1.0) < 0.01)
        assert not np.any(near), f"tile {tx},{ty}: an alpha sits on 1/255: (pixel, position, 255 alpha) {[(int(p_), int(e_) + 1, float(araw[p_, e_] * 255)) for p_, e_ in zip(*np.nonzero(near))][:6]}"
        near = reach & valid & (np.abs(Tin * 1e4 - 1.0) < T_MARGIN)
        assert not np.any(near), f"tile {tx},{ty}: a T' sits on 1e-4: (pixel, position, T') {[(int(p_), int(e_) + 1, float(Tin[p_, e_])) for p_, e_ in zip(*np.nonzero(near))][:6]}"
        con = alive & valid
        pos = np.arange(1, len(ids) + 1)[None]
        n = np.where(con, pos, 0).max(axis=1)
        Tf = np.prod(np.where(con, 1.0 - alpha, 1.0), axis=1)
        ncon[ty * TILE:(ty + 1) * TILE, tx * TILE:(tx + 1) * TILE] = n.reshape(TILE, TILE)
        fT[ty * TILE:(ty + 1) * TILE, tx * TILE:(tx + 1) * TILE] = Tf.reshape(TILE, TILE)
        blended[ids] |= (con & inside[:, None]).any(axis=0)
        blendd[(tx, ty)] = (con & inside[:, None]).any(axis=0)
        # The default footprint cull (include/gsraster.h, GSR_FLAG_NO_CULL) drops a pair whose Gaussian cannot reach
        # alpha >= 1/255 anywhere on the tile's strips clipped to the image -- on the continuous rectangles, not only on the
        # pixel centres.  The kept entries, the list length under the cull, and n_contrib as a position in the kept list:
        kept = _reaches_tile(px[ids], py[ids], c[ids] / det[ids], -b[ids] / det[ids], a[ids] / det[ids], opac[ids], tx, ty, H, W)
        assert not np.any((valid & inside[:, None]).any(axis=0) & ~kept), f"tile {tx},{ty}: the cull would drop a pair a pixel blends"
        tile_len_cull[ty, tx] = int(kept.sum())
        keptd[(tx, ty)] = kept
        hitd[(tx, ty)] = valid & inside[:, None]
        rank = np.concatenate([[0], np.cumsum(kept)])
        ncon_cull[ty * TILE:(ty + 1) * TILE, tx * TILE:(tx + 1) * TILE] = rank[n].reshape(TILE, TILE)
    return SimpleNamespace(cam=cam, tile_len=tile_len, n_contrib=ncon[:H, :W], final_T=fT[:H, :W], blended=blended,
                           listed=listed, lists=lists, tile_len_cull=tile_len_cull, n_contrib_cull=ncon_cull[:H, :W],
                           kept=keptd, blended_in=blendd, hits=hitd)


def _reaches_tile(cx, cy, A, B, C, o, tx, ty, H, W):
    """[L] bool: the conic's minimum over one of the tile's 16 x 4 strips (clipped to the image) stays under
    2 ln(255 o).  The minimum of a convex quadratic over a box the centre lies outside of is on the box's edges."""
    tau = 2.0 * np.log(255.0 * o)
    x0, x1 = float(tx * TILE), float(min(tx * TILE + TILE - 1, W - 1))
    dxl, dxh = x0 - cx, x1 - cx
    hit_any = np.zeros(len(cx), dtype=bool)
    for k in range(4):
        ya = float(ty * TILE + 4 * k)
        if ya > H - 1:
            break
        yb = min(ya + 3.0, float(H - 1))
        dyl, dyh = ya - cy, yb - cy
        inside = (dxl <= 0) & (dxh >= 0) & (dyl <= 0) & (dyh >= 0)
        q = np.full(len(cx), np.inf)
        for dxe in (dxl, dxh):                              # the two columns: minimise over dy in [dyl, dyh]
            d = np.clip(-B * dxe / C, dyl, dyh)
            q = np.minimum(q, A * dxe * dxe + 2 * B * dxe * d + C * d * d)
        for dye in (dyl, dyh):                              # the two rows
            e = np.clip(-B * dye / A, dxl, dxh)
            q = np.minimum(q, A * e * e + 2 * B * e * dye + C * dye * dye)
        q = np.where(inside, 0.0, q)
        assert np.all(np.abs(q - tau) > 0.02), f"tile {tx},{ty}: a footprint touches a strip's edge"
        hit_any |= q <= tau
    return hit_any


def records(tile_len, seg_shift=8):
    """Boundary records the tile scheduler counts: (len + seg - 1) >> shift for every tile longer than one segment."""
    seg = 1 << seg_shift
    lens = np.asarray(tile_len).reshape(-1)
    return int(sum((int(n) + seg - 1) >> seg_shift for n in lens if n > seg))


# ---------------------------------------------------------------------------------------------------------------------
# stacks
# ---------------------------------------------------------------------------------------------------------------------
def _base_entry(pos, L):
    """(cx, cy, sigma_x, sigma_y, opacity) of position pos (1-based) of an L-entry stack without blockers."""
    if pos > L - 3 or pos % 64 == 0:
        cx, cy = WIDE_C[pos % 4]
        return (cx, cy, 1.4, 1.4, 0.04)
    cx, cy = THIN_C[pos % 6]
    return (cx, cy, 0.9, 0.9, 0.016)


def stack(L, blockers=None):
    """blockers: (first position, count) of a run of blockers replacing the base entries there."""
    ent = [_base_entry(p, L) for p in range(1, L + 1)]
    if blockers is not None:
        b, m = blockers
        for p in range(b, min(b + m, L + 1)):
            ent[p - 1] = (BLOCK_C[0], BLOCK_C[1], BLOCK_S, BLOCK_S, 0.999)
        # behind the run only the four corner centres: no later entry reaches a pixel the blockers dimmed, so no T' creeps
        # towards 1e-4 in steps of one per cent
        for p in range(b + m, L + 1):
            ent[p - 1] = (THIN_C[p % 4][0], THIN_C[p % 4][1], 0.9, 0.9, 0.016)
    return ent


class _Builder:
    def __init__(self, H, W, seed, focal=FOCAL, depth_sigma=1.0):
        """focal: of the cameras the scene is built for; depth_sigma: factor on the scale along the view axis (a wide
        field of view stretches a footprint by (x / z)^2 of it)."""
        self.H, self.W, self.rows, self.focal, self.depth_sigma = H, W, [], focal, depth_sigma
        self.rng = np.random.default_rng(seed)

    def add(self, tx, ty, entries, z0=2.0, dz=0.01):
        for i, (cx, cy, sx, sy, o) in enumerate(entries):
            self.rows.append((TILE * tx + cx, TILE * ty + cy, z0 + dz * i, sx, sy, o, tx, ty, i + 1))

    def add_raw(self, px, py, z, sx, sy, o):
        self.rows.append((px, py, z, sx, sy, o, -1, -1, 0))

    def finish(self, name, views=None):
        r = np.array(self.rows, dtype=np.float64)
        r = r[self.rng.permutation(len(r))]                 # storage order is not depth order
        P = len(r)
        z = r[:, 2]
        means = np.stack([(r[:, 0] - (self.W - 1) * 0.5) * z / self.focal, (r[:, 1] - (self.H - 1) * 0.5) * z / self.focal, z], axis=1)
        an = np.where(np.arange(P) % 2 == 0, 1.06, 0.94)
        iso = (r[:, 3] == r[:, 4]) & (r[:, 3] != BLOCK_S) & (r[:, 3] != TINY_S)
        an = np.where(iso, an, 1.0)                          # (a bar keeps its two widths and stays along x)
        scales = np.stack([r[:, 3] * an, r[:, 4] / an, self.depth_sigma * 0.5 * (r[:, 3] + r[:, 4])], axis=1) * (z / self.focal)[:, None]
        th = np.where(iso, self.rng.uniform(0, math.pi, P), 0.0)
        quats = np.stack([np.cos(th / 2), np.zeros(P), np.zeros(P), np.sin(th / 2)], axis=1)
        opac = r[:, 5]
        # what the tests hand to both sides: float32 values (the model and the oracle see exactly these)
        t32 = lambda a_: torch.tensor(a_, dtype=torch.float32)
        g = torch.Generator().manual_seed(int(self.rng.integers(1 << 30)))
        raw = dict(_xyz=t32(means),
                   _features_dc=(torch.rand(P, 1, 3, generator=g) - 0.5) / SH_C0 * 0.6,
                   _features_rest=(torch.rand(P, 15, 3, generator=g) - 0.5) * 0.04,
                   _objects_dc=torch.rand(P, 1, 16, generator=g),
                   _opacity=torch.logit(t32(opac)).view(P, 1),
                   _scaling=torch.log(t32(scales)),
                   _rotation=t32(quats) * (0.5 + 1.5 * torch.rand(P, 1, generator=g)))
        act = activate(raw)
        m64 = lambda k: act[k].double().numpy()
        cams = views if views is not None else [camera(self.H, self.W, focal=self.focal)]
        facts = [model(m64("means3D"), m64("scales"), m64("rotations"), m64("opacities")[:, 0], c) for c in cams]
        return SimpleNamespace(name=name, H=self.H, W=self.W, P=P, raw=raw, cams=cams, facts=facts,
                               tile=r[:, 6:8].astype(int), pos=r[:, 8].astype(int))


def activate(raw):
    """The getters of the reference model on raw leaves, in the leaves' dtype (differentiable)."""
    return dict(means3D=raw["_xyz"], shs=torch.cat([raw["_features_dc"], raw["_features_rest"]], dim=1),
                sh_objs=raw["_objects_dc"], opacities=torch.sigmoid(raw["_opacity"]), scales=torch.exp(raw["_scaling"]),
                rotations=torch.nn.functional.normalize(raw["_rotation"]))


def _expect_lengths(sc, want, view=0):
    got = sc.facts[view].tile_len
    for ty in range(got.shape[0]):
        for tx in range(got.shape[1]):
            assert got[ty, tx] == want.get((tx, ty), 0), f"{sc.name}: tile {tx},{ty} has {got[ty, tx]} entries, designed {want.get((tx, ty), 0)}"
    sc.designed_len = want


NEIGH = ((-1, -1), (1, -1), (-1, 1), (1, 1), (-1, 0), (1, 0), (0, -1), (0, 1))     # corners first: a run ends on an edge
KILL, STOPPERS = 40, 8


def _blocked(s, tiny=True):
    """The 640-entry stack whose pixel (8, 8) has n_contrib = s, whose stopping entry s + 1 stops EVERY pixel it touches,
    and behind which lie entries that no pixel blends.
    A tiny entry (TINY_S) touches the 3 x 3 pixels around its centre and nothing else.  Positions s - 39 .. s: five rounds of
    tiny entries on the eight neighbours of (8, 8) -- each neighbour takes the 0.99 cap five times and is finished after
    three, while (8, 8) is dimmed to T = 3e-3 and blends the last of them, an edge neighbour, at position s.  Positions
    s + 1 .. s + 8: tiny entries on (8, 8) itself: the first stops it (T' = 3e-5), so all nine pixels it touches have
    stopped at or before it, and neither it nor the seven behind it are ever blended: exactly zero gradients, and the
    entry one beyond n_contrib is one of them.  Behind them only the four corner centres (no later entry reaches a dimmed
    pixel, so no T' creeps towards 1e-4).
    s = 2 leaves no room for the neighbours' run: there a run of blockers (BLOCK_S) starts at position 2 behind a wide
    entry; pixel (8, 8) stops on 3, but the blockers' outer ring (alpha 0.006) keeps blending them: no dead entry.
    tiny=False: that blocker run for any s (the batch family: under its rotated views a tiny entry's alpha leaves the 0.99
    cap, and oracle-R then flags the T' of its neighbours as fragile)."""
    ent = stack(B_LEN)
    if s > KILL and tiny:
        for k, p in enumerate(range(s - KILL + 1, s + 1)):
            ent[p - 1] = (BLOCK_C[0] + NEIGH[k % 8][0], BLOCK_C[1] + NEIGH[k % 8][1], TINY_S, TINY_S, 0.999)
        for p in range(s + 1, s + 1 + STOPPERS):
            ent[p - 1] = (BLOCK_C[0], BLOCK_C[1], TINY_S, TINY_S, 0.999)
        behind = s + 1 + STOPPERS
    else:
        ent = stack(B_LEN, (s, 8))
        ent[0] = (WIDE_C[0][0], WIDE_C[0][1], 1.4, 1.4, 0.04)
        behind = B_LEN + 1
    for p in range(behind, B_LEN + 1):
        ent[p - 1] = (THIN_C[p % 4][0], THIN_C[p % 4][1], 0.9, 0.9, 0.016)
    probe = _Builder(TILE, TILE, 0)
    probe.add(0, 0, ent)
    sc = probe.finish("probe")
    got = sc.facts[0].n_contrib[8, 8]
    assert got == s, f"pixel (8, 8) stops at {got}, designed {s}"
    if s > KILL and tiny:
        stoppers = (sc.pos > s) & (sc.pos <= s + STOPPERS)
        assert not sc.facts[0].blended[stoppers].any(), f"s = {s}: a pixel blends an entry behind the stop"
    return ent


def stopper_ids(sc, view=0):
    """Gaussians that are the designed stopping entries (and the seven behind each) of a scene with `stops`."""
    ids = []
    for (tx, ty), s in sc.stops.items():
        if s > KILL and getattr(sc, "tiny", True):
            ids += list(np.nonzero((sc.tile[:, 0] == tx) & (sc.tile[:, 1] == ty) & (sc.pos > s) & (sc.pos <= s + STOPPERS))[0])
    return np.array(ids, dtype=np.int64)


# ---------------------------------------------------------------------------------------------------------------------
# families
# ---------------------------------------------------------------------------------------------------------------------
def family_a():
    """28 stacks, no stopping: every second tile of a 10 x 6 grid (empty tiles between), 256 beside 257."""
    b = _Builder(6 * TILE, 10 * TILE, seed=11)
    want = {}
    slots = [(tx, ty) for ty in range(6) for tx in range(10) if (tx + ty) % 2 == 0]
    lens = [n for n in A_LENGTHS if n not in (256, 257)]
    for (tx, ty), L in zip([s for s in slots if s not in ((4, 2),)], lens):
        want[(tx, ty)] = L
    want[(4, 2)], want[(5, 2)] = 256, 257                   # one segment beside two
    for (tx, ty), L in want.items():
        b.add(tx, ty, stack(L))
    sc = b.finish("A lengths")
    _expect_lengths(sc, want)
    assert sorted(want.values()) == sorted(A_LENGTHS)
    assert sc.facts[0].final_T.min() > 0.05, sc.facts[0].final_T.min()
    return sc


def _family_b_like(name, H, W, places, seed):
    b = _Builder(H, W, seed)
    want, stops = {}, {}
    for (tx, ty), s in places:
        ent = _blocked(s)
        b.add(tx, ty, ent)
        want[(tx, ty)], stops[(tx, ty)] = B_LEN, s
    sc = b.finish(name)
    _expect_lengths(sc, want)
    f = sc.facts[0]
    for (tx, ty), s in stops.items():
        y, x = TILE * ty + 8, TILE * tx + 8
        if y < H and x < W:
            assert f.n_contrib[y, x] == s, (name, tx, ty, s, f.n_contrib[y, x])
        t = f.n_contrib[TILE * ty:TILE * (ty + 1), TILE * tx:TILE * (tx + 1)]
        assert t.max() == B_LEN and len(np.unique(t)) >= 4    # unblocked pixels walk the whole list; lanes stop apart
    sc.stops = stops
    dead = dead_gaussians(sc)
    assert len(stopper_ids(sc)) == STOPPERS * sum(s > KILL for s in stops.values()) and dead[stopper_ids(sc)].all()
    return sc


def family_b():
    """14 stacks of 640 entries, pixel (8, 8) of each stopping at one of B_STOPS; pixels out of the blockers' reach
    walk all 640 entries (three segments at the default length)."""
    slots = [(tx, ty) for ty in range(5) for tx in range(7) if (tx + ty) % 2 == 0]
    return _family_b_like("B stops", 5 * TILE, 7 * TILE, list(zip(slots, B_STOPS)), seed=12)


def _bars(H, W, name, runs, seed, cy, L=B_LEN):
    """One tile = the whole image (no footprint can spill): an L-entry stack with runs of bars, each run covering one
    strip.  runs: (strip, first position, count)."""
    ent = stack(L)
    for strip, first, count in runs:
        for p in range(first, first + count):
            ent[p - 1] = (7.5, 4 * strip + cy, 90.3, BAR_SY, 0.999)
    b = _Builder(H, W, seed)
    b.add(0, 0, ent)
    sc = b.finish(name)
    _expect_lengths(sc, {(0, 0): L})
    return sc


def family_b_strips():
    """Strips 0, 1, 2 finish in batch 1, batch 2 and the second segment; strip 3 walks all 640 entries."""
    sc = _bars(TILE, TILE, "B strips", ((0, 10, 50), (1, 70, 50), (2, 290, 50)), seed=13, cy=1.44)
    n = sc.facts[0].n_contrib
    assert n[0:4].max() < 64 and 64 < n[4:8].min() and n[4:8].max() < 128 and 256 < n[8:12].min() and n[8:12].max() < 384
    assert n[12:16].max() >= B_LEN - 3
    return sc


def family_b_first_segment():
    """All four strips finish inside the first segment of a split tile: the later records are read by nobody."""
    sc = _bars(TILE, TILE, "B first segment", ((0, 20, 50), (1, 75, 50), (2, 130, 50), (3, 185, 50)), seed=14, cy=1.4)
    assert sc.facts[0].n_contrib.max() < 256 and sc.facts[0].n_contrib.min() > 0
    return sc


def family_c():
    """Width and height not multiples of 16 (5 x 4 tiles of a 77 x 61 image): stacks in the last tile column (13 pixel
    columns inside) and the last tile row (13 rows inside), lengths and stops from A and B.  Every entry still reaches the
    part of its tile inside the image, so the default footprint cull drops nothing and the lengths stay the designed ones."""
    H, W = 3 * TILE + 13, 4 * TILE + 13
    b = _Builder(H, W, seed=15)
    want = {}
    col = [(4, 0, 257), (4, 1, 64), (4, 2, 513), (0, 3, 65), (1, 3, 255), (2, 3, 256), (3, 3, 1025)]
    for tx, ty, L in col:
        b.add(tx, ty, stack(L))
        want[(tx, ty)] = L
    stops = {}
    for (tx, ty), s in (((4, 3), 256), ((2, 0), 2), ((0, 1), 64), ((2, 2), 257), ((0, 0), 512)):
        ent = _blocked(s)
        b.add(tx, ty, ent)
        want[(tx, ty)], stops[(tx, ty)] = B_LEN, s
    sc = b.finish("C ragged")
    _expect_lengths(sc, want)
    assert sc.facts[0].n_contrib[3 * TILE + 8, 4 * TILE + 8] == 256
    sc.stops = stops
    assert len(stopper_ids(sc)) == 4 * STOPPERS and dead_gaussians(sc)[stopper_ids(sc)].all()
    return sc


def family_c_strips():
    """The strip scene on a 13 x 12 image: strip 0 finishes in batch 1, strip 1 in the second segment, strip 2 walks the
    whole list, strip 3 lies outside the image."""
    sc = _bars(12, 13, "C strips", ((0, 10, 50), (1, 290, 50)), seed=16, cy=1.5)
    n = sc.facts[0].n_contrib
    assert n[0:4].max() < 64 and 256 < n[4:8].min() and n[4:8].max() < 384 and n[8:12].max() >= B_LEN - 3
    return sc


D_SHIFTS = ((0, 0), (16, 0), (-16, 16), (32, -16), (4000, 0), (0, 16), (-32, 0), (16, 16), (48, 0), (-16, -16), (0, -16),
            (32, 16), (-48, 16), (16, -16), (-32, -16), (64, 0))


def family_d(B):
    """One scene of 9 x 7 tiles, B views: all of A's lengths from 255 up and all of B's stop indices (plus one 65-entry list), every
    second tile.  The views are rotations that move the image by whole tiles (so the same stacks land in other tiles and,
    at the image border, leave it); view 1 also moves 0.001 forward, which takes the two nearest entries of the on-axis
    257-entry stack (z = 0.2004, 0.2008) across the near plane (255 there); view 4 looks away and sees nothing."""
    H, W = 7 * TILE, 9 * TILE
    cams = [camera(H, W, yaw_px=D_SHIFTS[v][0], pitch_px=D_SHIFTS[v][1], forward=0.001 if v == 1 else 0.0) for v in range(B)]
    b = _Builder(H, W, seed=17)
    ent = stack(257)
    b.add(4, 3, ent[2:], z0=2.02)                           # on the optical axis: (71.5, 55.5) = tile (4, 3) + (7.5, 7.5)
    b.add(4, 3, ent[:2], z0=0.2004, dz=0.0004)                # its two nearest entries, just behind the near plane
    want, stops = {(4, 3): 257}, {}
    slots = [(tx, ty) for ty in range(7) for tx in range(9) if (tx + ty) % 2 == 1 and (tx, ty) != (4, 3)]
    lens = [n for n in A_LENGTHS if n >= 255 and n != 257] + [65]
    for (tx, ty), L in zip(slots, lens):
        b.add(tx, ty, stack(L))
        want[(tx, ty)] = L
    for (tx, ty), s in zip(slots[len(lens):], B_STOPS):
        b.add(tx, ty, _blocked(s, tiny=False))
        want[(tx, ty)], stops[(tx, ty)] = B_LEN, s
    assert len(stops) == len(B_STOPS)
    sc = b.finish(f"D batch of {B}", views=cams)
    sc.oracle_key = "D"                                     # (the views of the smaller batches are the first of the larger)
    _expect_lengths(sc, want)
    sc.stops, sc.tiny = stops, False
    if B > 1:
        assert sc.facts[1].tile_len[3, 5] == 255, sc.facts[1].tile_len      # view 1: one tile to the right, two entries culled
    if B > 4:
        assert sc.facts[4].tile_len.sum() == 0
    return sc


SINGLE_VIEW = dict(A=family_a, B=family_b, Bstrips=family_b_strips, Bfirst=family_b_first_segment, C=family_c,
                   Cstrips=family_c_strips)
_CACHE = {}


def get(key):
    """key: a SINGLE_VIEW name or ('D', B).  Built once per process."""
    if key not in _CACHE:
        _CACHE[key] = family_d(key[1]) if isinstance(key, tuple) else SINGLE_VIEW[key]()
    return _CACHE[key]


def dead_gaussians(sc):
    """[P] bool: in no view does any pixel blend the Gaussian (it lies at or behind the stop index of every pixel it
    touches, or it touches none, or it is culled): its gradient is exactly zero in every attribute."""
    live = np.zeros(sc.P, dtype=bool)
    for f in sc.facts:
        live |= f.blended
    return ~live


# ---------------------------------------------------------------------------------------------------------------------
# oracle-R on a scene (shared by the CPU and the GPU tests)
# ---------------------------------------------------------------------------------------------------------------------
BG = (0.2, 0.3, 0.1)
RAW = ("_xyz", "_features_dc", "_features_rest", "_objects_dc", "_opacity", "_scaling", "_rotation")
CLASSIC = ("means3D", "shs", "sh_objs", "opacities", "scales", "rotations")
_ORACLE = {}


def loss_weights(sc, view, tile_windows=None):
    """Seeded dL/dC [3,H,W], dL/dobjects [16,H,W], dL/ddepth [H,W], dL/dalpha [H,W] of one view; tile_windows (half-open tile
    rectangles (tx0, ty0, tx1, ty1)): zero outside them."""
    g = torch.Generator().manual_seed(1000 + 17 * view + sc.P)
    w = dict(C=torch.randn(3, sc.H, sc.W, generator=g), O=torch.randn(16, sc.H, sc.W, generator=g),
             D=torch.randn(sc.H, sc.W, generator=g), A=torch.randn(sc.H, sc.W, generator=g))
    if tile_windows is not None:
        keep = window_px(sc, tile_windows).to(torch.float32)
        w = {k: v * keep for k, v in w.items()}
    return w


def window_px(sc, tile_windows):
    """[H, W] bool: the pixels inside the tile windows."""
    m = torch.zeros(sc.H, sc.W, dtype=torch.bool)
    for (x0, y0, x1, y1) in tile_windows:
        m[TILE * y0:TILE * y1, TILE * x0:TILE * x1] = True
    return m


def oracle_run(sc, view=0, dtype=torch.float64, tile_windows=None):
    """oracle-R on one view (with tile_windows: on those tiles alone, the loss weights zero elsewhere), once per process: outputs
    (colour on BG, objects, depth = sum z alpha T and alpha on black,
    final_T, n_contrib, fragile counts) and, for each of the four loss terms alone (gradients are linear in them), the
    gradient of every raw leaf, of every activated tensor (the classic surface's inputs) and of means2D."""
    key = (getattr(sc, "oracle_key", sc.name), view, dtype, None if tile_windows is None else tuple(tile_windows))
    if key in _ORACLE:
        return _ORACLE[key]
    from oracle import oracle_r as O
    cam = sc.cams[view]
    L = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in sc.raw.items()}
    a = activate(L)
    tw = tile_windows
    m2d = torch.zeros(sc.P, 3, dtype=dtype, requires_grad=True)
    st = settings(cam, torch.tensor(BG), O.Settings)
    col = O.rasterize(a["means3D"], m2d, a["opacities"], st, shs=a["shs"], sh_objs=a["sh_objs"], scales=a["scales"],
                      rotations=a["rotations"], dtype=dtype, tile_windows=tw)
    z = (torch.cat([a["means3D"], torch.ones_like(a["means3D"][:, :1])], dim=1) @ cam.V.to(dtype))[:, 2]
    zc = torch.stack([z, torch.ones_like(z), torch.zeros_like(z)], dim=1)
    aux = O.rasterize(a["means3D"], m2d, a["opacities"], st._replace(bg=torch.zeros(3)), colors_precomp=zc,
                      scales=a["scales"], rotations=a["rotations"], dtype=dtype, tile_windows=tw)
    outs = dict(C=col.color, O=col.objects, D=aux.color[0], A=aux.color[1])
    leaves = dict(L)
    leaves.update(a)
    leaves["means2D"] = m2d
    w = loss_weights(sc, view, tile_windows)
    grads = {}
    for c, o in outs.items():
        loss = (o * w[c].to(dtype)).sum()
        if loss.requires_grad:
            gs = torch.autograd.grad(loss, list(leaves.values()), retain_graph=True, allow_unused=True)
        else:
            gs = [None] * len(leaves)
        grads[c] = {k: (torch.zeros_like(v) if g_ is None else g_).detach() for (k, v), g_ in zip(leaves.items(), gs)}
    seen = col.radii > 0
    res = SimpleNamespace(color=col.color.detach(), objects=col.objects.detach(), depth=aux.color[0].detach(),
                          alpha=aux.color[1].detach(), final_T=col.final_T.detach(), n_contrib=col.n_contrib,
                          fragile_px=int(col.fragile_px.sum()) + int(aux.fragile_px.sum()),
                          fragile_gauss=int(col.fragile_gauss.sum()), radii=col.radii, grads=grads,
                          num_rendered=col.num_rendered, z_far=float(z.detach()[seen].max()) if bool(seen.any()) else 1.0)
    _ORACLE[key] = res
    return res


def grad_sum(res, terms, name):
    """Gradient of leaf `name` for the loss made of `terms` (a string over 'C', 'O', 'D', 'A')."""
    return sum(res.grads[c][name] for c in terms)
