"""Shared by test_deteval_host_cpu.py and test_gpu_deteval.py (not a test module): the float64 oracle of the detection metrics, the
cases, and the runners of the host build.

The oracle restates COCOeval.evaluateImg, accumulate and summarize for boxes from their published behaviour in plain loops over
Python floats (IEEE doubles, one rounding per operation, no contraction), in the operation order include/gsraster.h writes down.
pycocotools is not a dependency of this project, so this is the yardstick: every integer output is compared for equality and every
double bit for bit (`same`)."""
import ctypes
import functools

import numpy as np

import host_build

EPS = 2.220446049250313e-16
COCO_AREAS = ((0.0, 1e5 ** 2), (0.0, 32.0 ** 2), (32.0 ** 2, 96.0 ** 2), (96.0 ** 2, 1e5 ** 2))
COCO_IOUS = np.linspace(0.5, 0.95, 10)
COCO_RECS = np.linspace(0.0, 1.0, 101)
STAT_NAMES = ("AP", "AP50", "AP75", "AP_small", "AP_medium", "AP_large", "AR_1", "AR_10", "AR_100", "AR_small", "AR_medium", "AR_large",
              "ap_ref", "ar_ref")
MATCH_KEYS = ("dt_order", "dt_rank", "dt_match", "dt_ignore", "gt_ignore", "gt_match")
ACC_KEYS = ("precision", "scores", "recall", "npig")
NAN = float("nan")


class Spec:
    def __init__(self, K, D, M, iou_thrs=COCO_IOUS, areas=COCO_AREAS, max_dets=(1, 10, 100), rec_thrs=COCO_RECS):
        self.K, self.D, self.M = int(K), int(D), int(M)
        self.iou = np.asarray(iou_thrs, np.float64)
        self.areas = tuple((float(lo), float(hi)) for lo, hi in areas)
        self.caps = tuple(int(c) for c in max_dets)
        self.rec = np.asarray(rec_thrs, np.float64)
        self.T, self.A, self.Mx, self.R = len(self.iou), len(self.areas), len(self.caps), len(self.rec)

    def replace(self, **kw):
        d = dict(K=self.K, D=self.D, M=self.M, iou_thrs=self.iou, areas=self.areas, max_dets=self.caps, rec_thrs=self.rec)
        d.update(kw)
        return Spec(**d)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same(a, b):
    """bit for bit, -0 and +0 apart, NaN payloads included"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        return False
    if a.dtype == np.float64 or b.dtype == np.float64:
        return bool(np.array_equal(bits(a), bits(b)))
    return bool(np.array_equal(a, b))


# ---- the oracle -------------------------------------------------------------------------------------------------------------------
def _area(b):
    return (b[2] - b[0]) * (b[3] - b[1])


def _iou(d, ad, g, ag):
    iw = min(d[2], g[2]) - max(d[0], g[0])
    ih = min(d[3], g[3]) - max(d[1], g[1])
    inter = 0.0 if (iw <= 0.0 or ih <= 0.0) else iw * ih
    den = (ad + ag) - inter
    with np.errstate(all="ignore"):
        v = float(np.float64(inter) / np.float64(den))
    return 0.0 if v != v else v


# (Python's min / max and the header's ternaries differ only in which of two EQUAL operands they return: the same value, or -0
# against +0, whose difference cannot survive the comparison with 0 that follows.  The operands are never NaN: live rows only.)


def oracle_match(spec, dets, counts, gt_boxes, gt_cls):
    B, D, M, A, T, K = dets.shape[0], spec.D, spec.M, spec.A, spec.T, spec.K
    out = dict(dt_order=np.full((B, D), -1, np.int32), dt_rank=np.full((B, D), -1, np.int32),
               dt_match=np.full((B, A, T, D), -1, np.int32), dt_ignore=np.zeros((B, A, T, D), np.uint8),
               gt_ignore=np.zeros((B, A, M), np.uint8), gt_match=np.full((B, A, T, M), -1, np.int32))
    for b in range(B):
        cnt = min(max(int(counts[b, 0]), 0), D)
        live = []
        for i in range(cnt):
            row = dets[b, i]
            c = float(row[5])
            if np.isnan(row).any() or not (0.0 <= c < K) or c != int(c):
                continue
            live.append(i)
        live.sort(key=lambda i: (-float(dets[b, i, 4]), i))
        cls = [int(dets[b, i, 5]) for i in live]
        seen = {}
        for j, i in enumerate(live):
            out["dt_order"][b, j] = i
            out["dt_rank"][b, j] = seen.get(cls[j], 0)
            seen[cls[j]] = seen.get(cls[j], 0) + 1
        gbox = [[float(v) for v in gt_boxes[b, g]] for g in range(M)]
        glive = [0 <= int(gt_cls[b, g]) < K and not np.isnan(gt_boxes[b, g]).any() for g in range(M)]
        garea = [_area(g) for g in gbox]
        dbox = [[float(v) for v in dets[b, i, :4]] for i in live]
        darea = [_area(d) for d in dbox]
        for a, (lo, hi) in enumerate(spec.areas):
            ign = [2 if not glive[g] else int(garea[g] < lo or garea[g] > hi) for g in range(M)]
            out["gt_ignore"][b, a] = ign
            for t in range(T):
                matched = set()
                for j in range(len(live)):
                    order = [g for g in range(M) if glive[g] and ign[g] == 0 and int(gt_cls[b, g]) == cls[j]] + \
                            [g for g in range(M) if glive[g] and ign[g] == 1 and int(gt_cls[b, g]) == cls[j]]
                    best, m = min(float(spec.iou[t]), 1 - 1e-10), -1
                    for g in order:
                        if g in matched:
                            continue
                        if m > -1 and ign[m] == 0 and ign[g] == 1:
                            break
                        v = _iou(dbox[j], darea[j], gbox[g], garea[g])
                        if v < best:
                            continue
                        best, m = v, g
                    if m > -1:
                        matched.add(m)
                        out["gt_match"][b, a, t, m] = j
                        out["dt_ignore"][b, a, t, j] = ign[m]
                    else:
                        out["dt_ignore"][b, a, t, j] = int(darea[j] < lo or darea[j] > hi)
                    out["dt_match"][b, a, t, j] = m
    return out


def oracle_accumulate(spec, dets, m, gt_cls, rec_thrs=None):
    rec = spec.rec if rec_thrs is None else np.asarray(rec_thrs, np.float64)
    N, D, M, A, T, K, R, Mx = dets.shape[0], spec.D, spec.M, spec.A, spec.T, spec.K, len(rec), spec.Mx
    precision = -np.ones((T, R, K, A, Mx))
    scores = -np.ones((T, R, K, A, Mx))
    recall = -np.ones((T, K, A, Mx))
    npig = np.zeros((K, A), np.int32)
    for n in range(N):
        for a in range(A):
            for g in range(M):
                if m["gt_ignore"][n, a, g] == 0:
                    npig[int(gt_cls[n, g]), a] += 1
    per_class = {}
    for n in range(N):
        for j in range(D):
            i = int(m["dt_order"][n, j])
            if i >= 0:
                per_class.setdefault(int(dets[n, i, 5]), []).append((float(dets[n, i, 4]), n, int(m["dt_rank"][n, j]), j))
    for k in range(K):
        for a in range(A):
            if npig[k, a] == 0:
                continue
            for mi, cap in enumerate(spec.caps):
                lst = [e for e in per_class.get(k, ()) if e[2] < cap]           # image order, rank order within an image
                lst.sort(key=lambda e: -e[0])                                   # stable
                for t in range(T):
                    tp = fp = 0
                    rc, pr = [], []
                    for s, n, _, j in lst:
                        if not m["dt_ignore"][n, a, t, j]:
                            if m["dt_match"][n, a, t, j] >= 0:
                                tp += 1
                            else:
                                fp += 1
                        rc.append(float(tp) / float(npig[k, a]))
                        pr.append(float(tp) / ((float(fp) + float(tp)) + EPS))
                    nd = len(lst)
                    recall[t, k, a, mi] = rc[-1] if nd else 0.0
                    for i in range(nd - 1, 0, -1):
                        if pr[i] > pr[i - 1]:
                            pr[i - 1] = pr[i]
                    idx = np.searchsorted(np.asarray(rc, np.float64), rec, side="left")
                    for r, i in enumerate(idx):
                        precision[t, r, k, a, mi] = pr[i] if i < nd else 0.0
                        scores[t, r, k, a, mi] = lst[i][0] if i < nd else 0.0
    return dict(precision=precision, scores=scores, recall=recall, npig=npig)


def stat_slices(spec, precision, recall):
    """The 14 slices COCOeval.summarize (and the reference's two) average, areas and caps by position; None: no such slice."""
    last = spec.Mx - 1

    def ap(t, a, m):
        if a >= spec.A or m >= spec.Mx:
            return None
        if t is not None:
            hit = np.where(spec.iou == t)[0]
            if len(hit) == 0:
                return None
            return precision[hit[0]:hit[0] + 1, :, :, a, m]
        return precision[:, :, :, a, m]

    def ar(a, m):
        return None if a >= spec.A or m >= spec.Mx else recall[:, :, a, m]
    return [ap(None, 0, last), ap(0.5, 0, last), ap(0.75, 0, last), ap(None, 1, last), ap(None, 2, last), ap(None, 3, last),
            ar(0, 0), ar(0, 1), ar(0, 2), ar(1, last), ar(2, last), ar(3, last), ap(None, 0, last), ar(0, 0)]


def oracle_summarize(spec, precision, recall):
    stats = np.empty(14)
    for i, sl in enumerate(stat_slices(spec, precision, recall)):
        total, n = 0.0, 0
        for v in (() if sl is None else np.ascontiguousarray(sl).ravel().tolist()):
            if v > -1.0:
                total, n = total + v, n + 1
        stats[i] = total / n if n else -1.0
    return stats


def oracle_run(spec, batches, rec_thrs=None):
    ms = [oracle_match(spec, *b) for b in batches]
    m = {k: np.concatenate([x[k] for x in ms]) for k in MATCH_KEYS}
    dets = np.concatenate([b[0] for b in batches])
    gt_cls = np.concatenate([b[3] for b in batches])
    out = dict(m)
    out.update(oracle_accumulate(spec, dets, m, gt_cls, rec_thrs))
    out["stats"] = oracle_summarize(spec, out["precision"], out["recall"])
    return out


# ---- the host build ---------------------------------------------------------------------------------------------------------------
class CSpec(ctypes.Structure):
    _fields_ = [("K", ctypes.c_int32), ("D", ctypes.c_int32), ("M", ctypes.c_int32), ("T", ctypes.c_int32), ("A", ctypes.c_int32),
                ("n_caps", ctypes.c_int32), ("max_dets", ctypes.c_int32 * 3), ("R", ctypes.c_int32), ("iou_thrs", ctypes.c_double * 10),
                ("area_lo", ctypes.c_double * 4), ("area_hi", ctypes.c_double * 4)]


def c_spec(spec, R=None):
    cs = CSpec(spec.K, spec.D, spec.M, spec.T, spec.A, spec.Mx)
    for i, c in enumerate(spec.caps):
        cs.max_dets[i] = c
    cs.R = spec.R if R is None else R
    for i, v in enumerate(spec.iou):
        cs.iou_thrs[i] = v
    for i, (lo, hi) in enumerate(spec.areas):
        cs.area_lo[i], cs.area_hi[i] = lo, hi
    return cs


@functools.lru_cache(None)
def host_lib():
    lib = host_build.host_lib("deteval")
    V = ctypes.c_void_p
    lib.deh_limits.restype = None
    lib.deh_limits.argtypes = [V]
    lib.deh_iou.restype = ctypes.c_double
    lib.deh_iou.argtypes = [V, V]
    lib.deh_score_key.restype = ctypes.c_uint32
    lib.deh_score_key.argtypes = [ctypes.c_float]
    lib.deh_match.restype = ctypes.c_int
    lib.deh_match.argtypes = [V, ctypes.c_int32] + [V] * 10
    lib.deh_accumulate.restype = ctypes.c_int
    lib.deh_accumulate.argtypes = [V, ctypes.c_int64] + [V] * 12
    lib.deh_summarize.restype = ctypes.c_int
    lib.deh_summarize.argtypes = [V] * 4
    return lib


def limits():
    out = (ctypes.c_int64 * 8)()
    host_lib().deh_limits(out)
    return dict(zip(("ACC_CHUNK", "MAX_D", "MAX_M", "MAX_T", "MAX_A", "MAX_K", "MAX_R", "MAX_ROWS"), out))


def _p(a):
    return a.ctypes.data if a.size else None


def host_match(spec, dets, counts, gt_boxes, gt_cls):
    B, D, M, A, T = dets.shape[0], spec.D, spec.M, spec.A, spec.T
    dets, counts = np.ascontiguousarray(dets, np.float32), np.ascontiguousarray(counts, np.int32)
    gt_boxes, gt_cls = np.ascontiguousarray(gt_boxes, np.float32), np.ascontiguousarray(gt_cls, np.int32)
    out = dict(dt_order=np.full((B, D), -7, np.int32), dt_rank=np.full((B, D), -7, np.int32), dt_match=np.full((B, A, T, D), -7, np.int32),
               dt_ignore=np.full((B, A, T, D), 9, np.uint8), gt_ignore=np.full((B, A, M), 9, np.uint8), gt_match=np.full((B, A, T, M), -7, np.int32))
    cs = c_spec(spec)
    rc = host_lib().deh_match(ctypes.byref(cs), B, _p(dets), _p(counts), _p(gt_boxes), _p(gt_cls), *[_p(out[k]) for k in MATCH_KEYS])
    assert rc == 0
    return out


def host_run(spec, batches, rec_thrs=None):
    rec = np.ascontiguousarray(spec.rec if rec_thrs is None else rec_thrs, np.float64)
    ms = [host_match(spec, *b) for b in batches]
    m = {k: np.concatenate([x[k] for x in ms]) for k in MATCH_KEYS}
    dets = np.ascontiguousarray(np.concatenate([b[0] for b in batches]), np.float32)
    gt_cls = np.ascontiguousarray(np.concatenate([b[3] for b in batches]), np.int32)
    T, R, K, A, Mx = spec.T, len(rec), spec.K, spec.A, spec.Mx
    out = dict(m)
    out.update(precision=np.full((T, R, K, A, Mx), 7.0), scores=np.full((T, R, K, A, Mx), 7.0), recall=np.full((T, K, A, Mx), 7.0),
               npig=np.full((K, A), -7, np.int32), stats=np.full(14, 7.0))
    cs = c_spec(spec, R)
    lib = host_lib()
    assert lib.deh_accumulate(ctypes.byref(cs), dets.shape[0], _p(dets), _p(m["dt_order"]), _p(m["dt_rank"]), _p(m["dt_match"]),
                              _p(m["dt_ignore"]), _p(gt_cls), _p(m["gt_ignore"]), _p(rec), *[_p(out[k]) for k in ACC_KEYS]) == 0
    assert lib.deh_summarize(ctypes.byref(cs), _p(out["precision"]), _p(out["recall"]), _p(out["stats"])) == 0
    return out


def check(tag, got, ref):
    for k in MATCH_KEYS + ACC_KEYS + ("stats",):
        g = got[k]
        g = g.detach().cpu().numpy() if hasattr(g, "detach") else np.asarray(g)
        assert g.shape == ref[k].shape, (tag, k, g.shape, ref[k].shape)
        if not same(g, ref[k]):
            bad = np.argwhere(bits(g) != bits(ref[k])) if ref[k].dtype == np.float64 else np.argwhere(g != ref[k])
            i = tuple(bad[0])
            raise AssertionError(f"{tag}: {k} differs at {len(bad)} of {g.size} entries, first {i}: got {g[i]!r}, oracle {ref[k][i]!r}")


# ---- the cases --------------------------------------------------------------------------------------------------------------------
def _scene(rng, B, D, M, K, counts, ties=False, big=False):
    """gt boxes of mixed sizes; detections that jitter a gt box (some exactly), or lie anywhere; scores from a few values with ties"""
    size = rng.choice([8.0, 20.0, 50.0, 120.0] if big else [8.0, 20.0, 50.0], size=(B, max(M, 1), 2))
    xy = rng.uniform(0, 200, size=(B, max(M, 1), 2))
    gt = np.concatenate([xy, xy + size * rng.uniform(0.8, 1.2, size.shape)], -1).astype(np.float32)[:, :M]
    gt_cls = rng.integers(0, K, size=(B, M)).astype(np.int32)
    dets = np.zeros((B, D, 6), np.float32)
    for b in range(B):
        for i in range(D):
            if M and rng.random() < 0.7:
                g = rng.integers(0, M)
                box = gt[b, g] + (np.zeros(4) if rng.random() < 0.2 else rng.normal(0, 3.0, 4)).astype(np.float32)
                c = gt_cls[b, g] if rng.random() < 0.8 else rng.integers(0, K)
            else:
                p = rng.uniform(0, 200, 2)
                box = np.concatenate([p, p + rng.uniform(4, 130, 2)])
                c = rng.integers(0, K)
            s = rng.choice([0.25, 0.5, 0.75, 0.9]) if ties else rng.random()
            dets[b, i] = (*box, s, c)
    return dets, np.stack([np.asarray(counts, np.int32)[:B], np.zeros(B, np.int32)], 1), gt, gt_cls


def _rows(D, rows):
    d = np.zeros((1, D, 6), np.float32)
    for i, r in enumerate(rows):
        d[0, i] = r
    return d, np.array([[len(rows), 0]], np.int32)


def _gt(M, rows):
    g = np.zeros((1, M, 4), np.float32)
    c = np.full((1, M), -1, np.int32)
    for i, (box, k) in enumerate(rows):
        g[0, i], c[0, i] = box, k
    return g, c


@functools.lru_cache(None)
def case(name):
    """-> (spec, [batch, ...]); batch = (dets [B,D,6] f32, counts [B,2] i32, gt_boxes [B,M,4] f32, gt_cls [B,M] i32)"""
    rng = np.random.default_rng(sum(map(ord, name)))
    if name.startswith("counts-D"):                     # counts on either side of a wave and of the sort's power of two
        D = int(name[8:])
        counts = [0, 1, 63, 64, 65, D, D + 7, -3]
        return Spec(3, D, 5, max_dets=(1, min(10, D), D) if D > 10 else (1,)), [_scene(rng, 8, D, 5, 3, counts, ties=True, big=True)]
    if name.startswith("gt-M"):                         # gt-M<m>-B<b>
        M, B = int(name[4:].split("-B")[0]), int(name.split("-B")[1])
        return Spec(2, 20, M, max_dets=(1, 10, 20)), [_scene(rng, B, 20, M, 2, [20, 13, 7], big=True)]
    if name == "ties":                                  # equal scores within an image and across images, -0 against +0
        d, c, g, k = _scene(rng, 3, 40, 5, 2, [40, 40, 31], ties=True)
        d[1] = d[0]
        d[2, :6, 4] = [0.0, -0.0, 0.0, -0.0, 0.5, 0.5]
        return Spec(2, 40, 5, max_dets=(1, 10, 40)), [(d, c, g, k)]
    if name == "dead-rows":
        box = [10, 10, 40, 40]
        d, c = _rows(8, [(*box, NAN, 0), (NAN, 10, 40, 40, 0.9, 0), (*box, 0.8, 2.5), (*box, 0.7, 3), (*box, 0.6, -1), (*box, 0.5, 0),
                         (11, 10, 40, 40, 0.4, 1), (*box, 0.3, 0)])
        c[0, 0] = 7                                     # the eighth row lies beyond the count
        g, k = _gt(5, [(box, 0), ([10, NAN, 40, 40], 1), (box, 3), (box, -1), ([11, 10, 40, 40], 1)])
        return Spec(3, 8, 5, max_dets=(1, 8)), [(d, c, g, k)]
    if name == "iou-at-threshold":                      # exactly 0.5 must match at 0.5; exactly 1 against 1 - 1e-10
        d, c = _rows(4, [(0, 0, 1, 1, 0.9, 0), (5, 5, 9, 9, 0.8, 0), (20, 20, 21, 21, 0.7, 0)])
        g, k = _gt(3, [([0, 0, 2, 1], 0), ([5, 5, 9, 9], 0), ([20, 20, 21, 21.000002], 0)])
        return Spec(1, 4, 3, iou_thrs=[0.5, 1.0], max_dets=(4,)), [(d, c, g, k)]
    if name == "equal-iou":                             # two rows of equal IoU: the later one wins
        d, c = _rows(2, [(0, 0, 10, 10, 0.9, 0), (0, 0, 10, 10, 0.8, 0)])
        g, k = _gt(3, [([0, 0, 10, 5], 0), ([0, 5, 10, 10], 0), ([0, 0, 5, 10], 0)])
        return Spec(1, 2, 3, iou_thrs=[0.5], max_dets=(2,)), [(d, c, g, k)]
    if name == "ignore-rules":
        # Area range 1 counts areas 100..500, range 2 areas from 500.  Image 0 under range 1: a counted row (IoU 0.6) and an ignored
        # larger row (IoU 0.91): at 0.5 the counted row is taken and the walk stops; at 0.75 only the ignored row qualifies; the second
        # detection falls to the ignored row.  Image 1: only an ignored row overlaps.  Image 2: no ground truth, unmatched detections
        # of area 25, 400 and 8100.
        d = np.zeros((3, 3, 6), np.float32)
        d[0, 0] = (0, 0, 20, 30, 0.9, 0)
        d[0, 1] = (0, 0, 20, 31, 0.8, 0)
        d[1, 0] = (0, 0, 50, 50, 0.9, 0)
        d[2, 0] = (100, 100, 105, 105, 0.9, 0)
        d[2, 1] = (100, 100, 120, 120, 0.8, 0)
        d[2, 2] = (100, 100, 190, 190, 0.7, 0)
        g = np.zeros((3, 2, 4), np.float32)
        k = np.full((3, 2), -1, np.int32)
        g[0, 0], k[0, 0] = (0, 0, 20, 33), 0            # area 660
        g[0, 1], k[0, 1] = (0, 0, 20, 18), 0
        g[1, 0], k[1, 0] = (0, 0, 50, 52), 0
        g[1, 1], k[1, 1] = (60, 60, 70, 75), 0
        counts = np.array([[2, 0], [1, 0], [3, 0]], np.int32)
        return Spec(1, 3, 2, iou_thrs=[0.5, 0.75], areas=((0, 1e10), (100, 500), (500, 1e10)), max_dets=(1, 3)), [(d, counts, g, k)]
    if name == "caps":                                  # 12 detections of one class in one image under caps (1, 10, 100)
        d, c, g, k = _scene(rng, 2, 100, 5, 2, [100, 100], ties=True)
        d[0, :12, 5] = 1
        d[0, 12:, 5] = 0
        k[0, :3] = 1
        return Spec(2, 100, 5), [(d, c, g, k)]
    if name == "empty-classes":                         # class 1: detections, no gt; class 2: gt, no detections; class 3: neither
        d, c, g, k = _scene(rng, 2, 12, 4, 1, [12, 9])
        d[:, ::3, 5] = 1
        k[:, 3] = 2
        return Spec(4, 12, 4, max_dets=(1, 12)), [(d, c, g, k)]
    if name == "recall-100":                            # npig = 100 over 10 images: tp / 100 meets the thresholds themselves
        B, D, M = 10, 16, 10
        g = np.zeros((B, M, 4), np.float32)
        for b in range(B):
            for i in range(M):
                g[b, i] = (20 * i, 0, 20 * i + 10, 10)
        k = np.zeros((B, M), np.int32)
        d = np.zeros((B, D, 6), np.float32)
        d[:, :M, :4] = g
        d[:, M:, :4] = (500, 500, 510, 510)
        d[:, :, 4] = rng.permutation(B * D).reshape(B, D).astype(np.float32) / (B * D)
        return Spec(1, D, M, iou_thrs=[0.5], areas=COCO_AREAS[:1], max_dets=(D,)), [(d, np.full((B, 2), D, np.int32), g, k)]
    if name == "scan-carry":                            # class segments on either side of the curve kernel's step, and past it
        ch = limits()["ACC_CHUNK"]
        sizes = [ch - 1, ch, ch + 1, 2 * ch + 1, 1]
        K, D, B = len(sizes), 40, 9
        d, c, g, k = _scene(rng, B, D, 6, K, [D] * B, ties=True)
        flat = d.reshape(-1, 6)
        flat[:, 5] = K + 1                              # dead, but for the rows below
        at = 0
        for cls, n in enumerate(sizes):
            flat[at:at + n, 5] = cls
            at += n + 3
        return Spec(K, D, 6, iou_thrs=[0.5, 0.75], areas=COCO_AREAS[:2], max_dets=(2, D)), [(d, c, g, k)]
    if name == "many-classes":                          # class offsets past the exclusive scan's 2048-word block
        K = 2100
        d, c, g, k = _scene(rng, 2, 30, 4, 6, [30, 30])
        d[:, :, 5] += 2045
        k += 2045
        return Spec(K, 30, 4, iou_thrs=[0.5], areas=COCO_AREAS[:1], max_dets=(30,), rec_thrs=[0.0, 0.5, 1.0]), [(d, c, g, k)]
    if name == "T1":
        return Spec(3, 30, 5, iou_thrs=[0.5], max_dets=(1, 10, 30)), [_scene(rng, 3, 30, 5, 3, [30, 30, 30], big=True)]
    if name == "T10-batches":                           # three batches of unequal size
        return Spec(3, 30, 5, max_dets=(1, 10, 30)), [_scene(rng, b, 30, 5, 3, [30, 22, 30], big=True) for b in (2, 1, 3)]
    if name == "literal":
        return literal()
    raise KeyError(name)


def literal():
    """One class, three gt rows, detections TP, FP, TP by score, one threshold: rc = [1/3, 1/3, 2/3], envelope [1, 2/3, 2/3],
    precision 1 for thresholds 0 .. 0.33 (34), 2/3 for 0.34 .. 0.66 (33), 0 for the other 34: AP = 56/101, AR = 2/3."""
    d, c = _rows(3, [(0, 0, 10, 10, 0.9, 0), (50, 50, 60, 60, 0.8, 0), (20, 0, 30, 10, 0.7, 0)])
    g, k = _gt(3, [([0, 0, 10, 10], 0), ([20, 0, 30, 10], 0), ([80, 80, 90, 90], 0)])
    return Spec(1, 3, 3, iou_thrs=[0.5], areas=COCO_AREAS[:1], max_dets=(3,)), [(d, c, g, k)]


ALL = ["counts-D1", "counts-D100", "counts-D129", "gt-M0-B1", "gt-M0-B3", "gt-M1-B1", "gt-M1-B3", "gt-M5-B1", "gt-M5-B3", "ties", "dead-rows",
       "iou-at-threshold", "equal-iou", "ignore-rules", "caps", "empty-classes", "recall-100", "scan-carry", "many-classes", "T1", "T10-batches",
       "literal"]


@functools.lru_cache(None)
def oracle(name):
    spec, batches = case(name)
    return oracle_run(spec, batches)
