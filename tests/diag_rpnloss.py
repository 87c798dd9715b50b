"""Times the RPN loss stage's launches on the device (not a test) at two working sizes -- C4: B = 5, A = 15, a 50 x 68 map,
M = 1; FPN: B = 5, five levels of A = 3 on an 800 x 1088 frame (strides 4 .. 64), M = 4 -- beside a torch-ops restatement on
the same device (a dense [M,R] IoU matrix, Matcher with low-quality matches, randperm subsampling, binary cross-entropy
and L1 through autograd).  Device events around the C entries on preallocated buffers (the binding is not in the time),
the median of REPS calls after WARM warm-up calls; prints what profiles/rpnloss_times.txt holds.

    python tests/diag_rpnloss.py
"""
import ctypes
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "3d-gaussian-splat-attack_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import rpnloss_cases as RC  # noqa: E402

WARM, REPS = 3, 21
DEV = "cuda:0"
BATCH, QUOTA = 256, 128
SIZES = {
    "C4": dict(B=5, M=1, levels=(RC.Level(RC.cells((32.0, 64.0, 128.0, 256.0, 512.0), (0.5, 1.0, 2.0)), 16, 50, 68),)),
    "FPN": dict(B=5, M=4, levels=tuple(RC.Level(RC.cells((float(32 << l),), (0.5, 1.0, 2.0)), 4 << l, -(-800 // (4 << l)), -(-1088 // (4 << l)))
                                       for l in range(5))),
}


def timed(fn):
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def torch_label(anc, gt, lo=0.3, hi=0.7):
    """Detectron2's label_and_sample_anchors in torch ops, one image: -> labels [R], matched [R]"""
    area_a, area_g = (anc[:, 2] - anc[:, 0]) * (anc[:, 3] - anc[:, 1]), (gt[:, 2] - gt[:, 0]) * (gt[:, 3] - gt[:, 1])
    wh = (torch.min(gt[:, None, 2:], anc[None, :, 2:]) - torch.max(gt[:, None, :2], anc[None, :, :2])).clamp(min=0)
    inter = wh[..., 0] * wh[..., 1]
    iou = torch.where(inter > 0, inter / (area_g[:, None] + area_a[None, :] - inter), torch.zeros_like(inter))
    vals, matched = iou.max(0)
    labels = torch.where(vals < lo, 0, torch.where(vals < hi, -1, 1))
    labels[(iou == iou.max(1, keepdim=True).values).any(0)] = 1
    pos, neg = (labels == 1).nonzero()[:, 0], (labels == 0).nonzero()[:, 0]
    n_pos = min(QUOTA, pos.numel())
    n_neg = min(BATCH - n_pos, neg.numel())
    out = torch.full_like(labels, -1)
    out[pos[torch.randperm(pos.numel(), device=pos.device)[:n_pos]]] = 1
    out[neg[torch.randperm(neg.numel(), device=neg.device)[:n_neg]]] = 0
    return out, matched


def torch_loss(c, logits, deltas, anc, gt, labels, matched):
    x, d = RC.flat_head(c, logits, deltas)
    valid, pos = labels >= 0, labels == 1
    cls = torch.nn.functional.binary_cross_entropy_with_logits(x[valid], labels[valid].float(), reduction="sum")
    bi, ri = pos.nonzero(as_tuple=True)
    src, dst = anc[ri], gt[bi, matched[bi, ri]]
    sw, sh, dw, dh = src[:, 2] - src[:, 0], src[:, 3] - src[:, 1], dst[:, 2] - dst[:, 0], dst[:, 3] - dst[:, 1]
    t = torch.stack([(dst[:, 0] + 0.5 * dw - src[:, 0] - 0.5 * sw) / sw, (dst[:, 1] + 0.5 * dh - src[:, 1] - 0.5 * sh) / sh,
                     (dw / sw).log(), (dh / sh).log()], -1)
    loc = (d[bi, ri] - t).abs().sum()
    total = (cls + loc) / float(BATCH * x.shape[0])
    return torch.autograd.grad(total, list(logits) + list(deltas))


def run(name, B, M, levels):
    import diff_gaussian_rasterization as D
    from diff_gaussian_rasterization import rpnloss_ops as RO
    lib = D._load()
    c = RC.Case(name, levels, B=B, n_gt=M, batch=BATCH, quota=QUOTA)
    R = RC.total(c)
    rs = np.random.RandomState(3)
    W, H = RC.extent(c)
    size, cx, cy = rs.uniform(60, 300, (B, M, 2)), rs.uniform(0.2 * W, 0.8 * W, (B, M)), rs.uniform(0.2 * H, 0.8 * H, (B, M))
    gt = torch.tensor(np.stack([cx - size[..., 0] / 2, cy - size[..., 1] / 2, cx + size[..., 0] / 2, cy + size[..., 1] / 2], -1).astype(np.float32)).to(DEV)
    cls = torch.zeros((B, M), dtype=torch.int32, device=DEV)
    lg = [torch.tensor(rs.normal(0, 2, (B, len(l.cells), l.hf, l.wf)).astype(np.float32)).to(DEV) for l in levels]
    dl = [torch.tensor(rs.normal(0, 0.5, (B, 4 * len(l.cells), l.hf, l.wf)).astype(np.float32)).to(DEV) for l in levels]
    cells = [torch.tensor(a).to(DEV) for a in RC.cell_arrays(c)]
    cs = RC.c_spec(c, M=M)
    n = ctypes.c_int64(0)
    assert lib.gsr_rpnloss_workspace_bytes(ctypes.byref(cs), ctypes.byref(n)) == 0
    ws = torch.empty(((n.value + 15) // 16 * 2,), dtype=torch.int64, device=DEV)
    labels, matched = (torch.empty((B, R), dtype=torch.int32, device=DEV) for _ in range(2))
    counts, loss = torch.empty((B, 4), dtype=torch.int32, device=DEV), torch.empty((3,), device=DEV)
    gl, gd = [torch.empty_like(x) for x in lg], [torch.empty_like(d) for d in dl]
    pp = lambda ts: (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
    p_cells, p_lg, p_dl, p_gl, p_gd = pp(cells), pp(lg), pp(dl), pp(gl), pp(gd)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def label():
        assert lib.gsr_rpnloss_label(ctypes.byref(cs), p_cells, gt.data_ptr(), cls.data_ptr(), ws.data_ptr(), n.value, labels.data_ptr(),
                                     matched.data_ptr(), counts.data_ptr(), None, st) == 0

    def terms():
        assert lib.gsr_rpnloss(ctypes.byref(cs), labels.data_ptr(), matched.data_ptr(), p_lg, p_dl, p_cells, gt.data_ptr(), ws.data_ptr(), n.value,
                               loss.data_ptr(), p_gl, p_gd, st) == 0

    def both():
        label()
        terms()

    anc = torch.tensor(RC.anchors(c, np.float32)).to(DEV)
    lg_t, dl_t = [x.clone().requires_grad_(True) for x in lg], [d.clone().requires_grad_(True) for d in dl]
    state = {}

    def t_label():
        out = [torch_label(anc, gt[b]) for b in range(B)]
        state["labels"], state["matched"] = torch.stack([o[0] for o in out]), torch.stack([o[1] for o in out])

    def t_terms():
        torch_loss(c, lg_t, dl_t, anc, gt, state["labels"], state["matched"])

    def t_both():
        t_label()
        t_terms()

    rows = [("gsr_rpnloss_label (5 launches)", timed(label)), ("gsr_rpnloss (2 launches)", timed(terms)), ("both entries", timed(both)),
            ("torch ops: label and sample", timed(t_label)), ("torch ops: loss and gradients", timed(t_terms)), ("torch ops: both", timed(t_both))]
    torch.cuda.synchronize()
    print(f"RPN losses at {name}: B={B} M={M} levels {[(len(l.cells), l.hf, l.wf) for l in levels]} R={R}; counts of image 0: {counts[0].tolist()}")
    for what, (med, lo, hi) in rows:
        print(f"  {what:34s} {med:8.3f} ms  (min {lo:.3f}, max {hi:.3f})")


def main():
    assert torch.cuda.is_available(), "diag_rpnloss needs a device"
    for name, kw in SIZES.items():
        run(name, **kw)
    print(f"  (device events around the calls, median of {REPS} after {WARM} warm-up calls; the torch restatement is timed with its host work)")


if __name__ == "__main__":
    main()
