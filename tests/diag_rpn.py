"""Times the RPN proposal stage's launches on the device (not a test): the C4 training shape -- B = 5, A = 15, a 50 x 68 map,
the best 12 000 of 51 000 logits, NMS at 0.7, keep 2 000 -- on random logits with spatially correlated scores, Detectron2's
anchors and random deltas.  Device events around the C entries on preallocated buffers (the binding is not in the time),
the median of REPS calls after WARM warm-up calls; prints what profiles/rpn_times.txt holds.

    python tests/diag_rpn.py
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

import rpn_cases as PC  # noqa: E402

B, A, HF, WF, STRIDE = 5, 15, 50, 68, 16
FRAME = (1088.0, 800.0)
PRE, POST, THR = 12000, 2000, 0.7
WARM, REPS = 3, 21
DEV = "cuda:0"


def inputs(seed=0):
    rs = np.random.RandomState(seed)
    y, x = np.mgrid[0:HF, 0:WF].astype(np.float64)
    logits = np.empty((B, A, HF, WF), np.float32)
    for b in range(B):
        f = np.zeros((HF, WF))
        for _ in range(4):                                                   # four objects per image
            cy, cx, s = rs.uniform(0.15, 0.85), rs.uniform(0.15, 0.85), rs.uniform(0.06, 0.2)
            f += np.exp(-(((y / HF - cy) / s) ** 2 + ((x / WF - cx) / s) ** 2))
        logits[b] = 6.0 * f[None] * (1.0 + 0.3 * rs.randn(A)[:, None, None]) - 4.0 + 1.5 * rs.randn(A, HF, WF)
    deltas = rs.randn(B, A, 4, HF, WF) * np.array([0.15, 0.15, 0.25, 0.25])[None, None, :, None, None]
    return logits, deltas.reshape(B, 4 * A, HF, WF).astype(np.float32), PC.real_cell_anchors()


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


def main():
    import diff_gaussian_rasterization as D
    from diff_gaussian_rasterization import rpn_ops as PO
    assert torch.cuda.is_available(), "diag_rpn needs a device"
    lib = D._load()
    lg, dl, ca = (torch.tensor(a).to(DEV) for a in inputs())
    N = min(PRE, A * HF * WF)
    cs = PO.c_spec(PO.RpnSpec(FRAME[0], FRAME[1], 0.0, PRE, POST, THR), B=B, A=A, Hf=HF, Wf=WF, stride=STRIDE, N=N)
    cb, csc, cl = PO.new_candidates(B, N, DEV)
    n = ctypes.c_int64(0)
    assert lib.gsr_rpn_workspace_bytes(ctypes.byref(cs), ctypes.byref(n)) == 0
    ws = torch.empty(((n.value + 7) // 8,), dtype=torch.int64, device=DEV)
    prop, sc = torch.empty((B, POST, 4), device=DEV), torch.empty((B, POST), device=DEV)
    keep, cnt = torch.empty((B, POST), dtype=torch.int32, device=DEV), torch.empty((B,), dtype=torch.int32, device=DEV)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def select():
        assert lib.gsr_rpn_select(ctypes.byref(cs), lg.data_ptr(), dl.data_ptr(), ca.data_ptr(), cb.data_ptr(), csc.data_ptr(), cl.data_ptr(), st) == 0

    def nms():
        assert lib.gsr_rpn_nms(ctypes.byref(cs), cb.data_ptr(), csc.data_ptr(), cl.data_ptr(), ws.data_ptr(), n.value, prop.data_ptr(),
                               sc.data_ptr(), keep.data_ptr(), cnt.data_ptr(), st) == 0

    def both():
        select()
        nms()

    t_sel, t_nms, t_both = timed(select), timed(nms), timed(both)
    torch.cuda.synchronize()
    kept = cnt.cpu().tolist()
    # how far the walk went: the rank of the last kept slot in the walk's order
    walked = []
    for b in range(B):
        order = PC.walk_order(csc[b].cpu().numpy(), cl[b].cpu().numpy()).tolist()
        walked.append(order.index(int(keep[b, kept[b] - 1])) + 1 if kept[b] else 0)
    print(f"RPN proposals at B={B} A={A} map {HF}x{WF} ({A * HF * WF} logits per image) pre_topk {PRE} post_topk {POST} nms {THR}")
    print(f"  candidates per image {[int((cl[b] >= 0).sum()) for b in range(B)]}, kept {kept}, last kept at rank {walked}")
    for name, (med, lo, hi) in (("gsr_rpn_select (1 launch)", t_sel), ("gsr_rpn_nms (order + walk, 2 launches)", t_nms),
                                ("both", t_both)):
        print(f"  {name:42s} {med:8.3f} ms  (min {lo:.3f}, max {hi:.3f})")
    print(f"  (device events around the C entries, median of {REPS} calls after {WARM} warm-up calls; one workgroup per image)")


if __name__ == "__main__":
    main()
