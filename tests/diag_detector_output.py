"""Diagnostic (not collected by pytest): the detector output stage, HIP against the same contract written in torch
device ops (class max, filter, stable sort, IoU matrix, and a Python greedy loop that reads one flag from the device per
box -- what a per-view host loop costs), on one device in one process.  Three heads: YOLOv8-shaped (B=8, A=8400, C=80,
[B,K,A]) at conf 0.7 and at conf 0.001 (more candidates than the cap), and YOLOv5-shaped (A=25200, objectness,
[B,A,K]).  Times come from device events after a warm-up, the two variants alternating.

    python tests/diag_detector_output.py [--iters 200] [--rounds 5] [--out profiles/detector_output_times.txt]
    python tests/diag_detector_output.py --hip-only v8_conf0.7 --iters 200          # under a kernel profiler
    python tests/diag_detector_output.py --report times.json --kernel-stats v8_conf0.7=stats.csv ... --out FILE

The second form runs only the library's calls of one case (the program to put behind a kernel-tracing profiler, whose
per-kernel statistics file the third form folds, with the first form's JSON, into the text report).  The score pass is
the one kernel that streams the head's output; its bytes (pred read once, 8 bytes per anchor written) over its time are
set against 6.3 TB/s, the streaming bandwidth one MI355X reaches.
"""
import argparse
import csv
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "3d-gaussian-splat-attack_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

STREAM_TBPS = 6.3
CASES = {
    "v8_conf0.7": dict(B=8, A=8400, C=80, layout=1, has_obj=False, conf=0.7),
    "v8_conf0.001": dict(B=8, A=8400, C=80, layout=1, has_obj=False, conf=0.001),
    "v5_obj_conf0.7": dict(B=8, A=25200, C=80, layout=0, has_obj=True, conf=0.7),
}


def make_raw(torch, dev, B, A, C, layout, has_obj, conf, seed=0):
    """A head's output as a detector gives it: most class scores near zero, about 3 % of the anchors confident, boxes in
    clusters (jittered copies around 40 objects), (xc, yc, w, h) in pixels of a 640 canvas."""
    g = torch.Generator(device=dev).manual_seed(seed)
    K = 4 + int(has_obj) + C
    obj_c = torch.rand(B, 40, 4, device=dev, generator=g) * torch.tensor([560.0, 560.0, 150.0, 150.0], device=dev) + \
        torch.tensor([40.0, 40.0, 30.0, 30.0], device=dev)
    which = torch.randint(0, 40, (B, A), device=dev, generator=g)
    box = torch.gather(obj_c, 1, which[..., None].expand(B, A, 4)) * (1 + 0.1 * (torch.rand(B, A, 4, device=dev, generator=g) - 0.5))
    cls = torch.rand(B, A, C, device=dev, generator=g) ** 8 * 0.5
    hot = torch.rand(B, A, device=dev, generator=g) < 0.03
    top = (which % C)[..., None]
    cls.scatter_(2, top, torch.where(hot[..., None], 0.72 + 0.27 * torch.rand(B, A, 1, device=dev, generator=g), cls.gather(2, top)))
    parts = [box] + ([torch.where(hot, 0.99, 0.3)[..., None].to(torch.float32)] if has_obj else []) + [cls]
    raw = torch.cat(parts, 2)
    assert raw.shape[2] == K
    return (raw.transpose(1, 2) if layout == 1 else raw).contiguous()


def torch_postprocess(torch, raw, layout, has_obj, conf, iou_thr, max_cand, max_det):
    """The contract in torch device ops, image by image; returns the kept anchors per image."""
    p = raw if layout == 0 else raw.transpose(1, 2)
    out = []
    for b in range(p.shape[0]):
        cls = p[b, :, 4 + int(has_obj):]
        s = cls * p[b, :, 4:5] if has_obj else cls
        score, best = s.max(dim=1)
        cand = torch.nonzero(score > conf)[:, 0]
        order = cand[torch.sort(score[cand], descending=True, stable=True).indices][:max_cand]
        xywh = p[b, order, :4]
        half = xywh[:, 2:] * 0.5
        box = torch.cat([xywh[:, :2] - half, xywh[:, :2] + half], 1)
        area = (box[:, 2] - box[:, 0]) * (box[:, 3] - box[:, 1])
        lt = torch.maximum(box[:, None, :2], box[None, :, :2])
        rb = torch.minimum(box[:, None, 2:], box[None, :, 2:])
        wh = (rb - lt).clamp(min=0)
        inter = wh[..., 0] * wh[..., 1]
        iou = inter / ((area[:, None] + area[None, :]) - inter)
        sup = torch.triu((iou > iou_thr) & (best[order][:, None] == best[order][None, :]), diagonal=1)
        alive = torch.ones(len(order), dtype=torch.bool, device=raw.device)
        keep = []
        for i in range(len(order)):
            if not bool(alive[i]):                   # one device-to-host read per box
                continue
            keep.append(i)
            if len(keep) == max_det:
                break
            alive &= ~sup[i]
        out.append(order[torch.tensor(keep, dtype=torch.long, device=raw.device)] if keep else order[:0])
    return out


def timed(torch, fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def measure(args):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("diag_detector_output: needs a HIP device (no CPU timing is meaningful)")
    import diff_gaussian_rasterization as D
    from diff_gaussian_rasterization import detect_ops as DO
    D._load()
    dev = torch.device("cuda:0")
    names = [args.hip_only] if args.hip_only else list(CASES)
    res = {}
    for name in names:
        c = CASES[name]
        raw = make_raw(torch, dev, **c)
        spec = DO.DetSpec(c["layout"], c["has_obj"], 0, c["conf"], 0.45, 4096, 300)
        gt = torch.tensor([[100.0, 100.0, 300.0, 300.0]], device=dev).repeat(c["B"], 1)

        def hip():
            dets, counts = DO.postprocess(raw, spec)
            return DO.verdict(dets, counts, gt, 0, None, True, 0.5)

        def hip_to_host():
            return hip()[0].cpu()

        def base():
            return torch_postprocess(torch, raw, c["layout"], c["has_obj"], c["conf"], 0.45, 4096, 300)

        for _ in range(10):
            hip()
        torch.cuda.synchronize()
        if args.hip_only:
            for _ in range(args.iters):
                hip()
            torch.cuda.synchronize()
            continue
        dets, counts = DO.postprocess(raw, spec)
        kept = base()                                # also the baseline's warm-up
        cn = counts.cpu().numpy()
        K = 4 + int(c["has_obj"]) + c["C"]
        r = {"shape": c, "kept": cn[:, 0].tolist(), "above_thr": cn[:, 1].tolist(),
             "baseline_kept": [int(len(k)) for k in kept],
             "score_pass_bytes": 4 * c["B"] * c["A"] * K + 8 * c["B"] * c["A"]}
        runs = {"hip_ms": [], "hip_with_copy_to_host_ms": [], "torch_baseline_ms": []}
        for _ in range(args.rounds):                 # alternate the variants: other work shares the host
            runs["hip_ms"].append(timed(torch, hip, args.iters))
            runs["hip_with_copy_to_host_ms"].append(timed(torch, hip_to_host, args.iters))
            runs["torch_baseline_ms"].append(timed(torch, base, max(1, args.iters // 100)))
        for k, v in runs.items():
            r[k] = min(v)
            r[k + "_all"] = [round(t, 4) for t in v]
        res[name] = r
    if not args.hip_only:
        print(json.dumps(res))
    return res


def report(args):
    res = json.load(open(args.report))
    lines = ["Detector output stage on one MI355X: tests/diag_detector_output.py (device events, best of the rounds; the",
             "per-kernel rows are a kernel-tracing profiler's averages over a run of the library's calls alone).", ""]
    stats = dict(s.split("=", 1) for s in args.kernel_stats)
    for name, r in res.items():
        c = r["shape"]
        lines.append(f"{name}: B={c['B']} A={c['A']} C={c['C']} layout={c['layout']} has_obj={int(c['has_obj'])} conf={c['conf']}")
        lines.append(f"  candidates above the threshold per image {r['above_thr']}, kept {r['kept']} (torch baseline kept {r['baseline_kept']})")
        lines.append(f"  postprocess + verdict, enqueue to completion      {r['hip_ms'] * 1e3:10.1f} us   rounds {r['hip_ms_all']}")
        lines.append(f"  ... with the copy of the B verdicts to the host    {r['hip_with_copy_to_host_ms'] * 1e3:10.1f} us")
        lines.append(f"  torch device ops + Python greedy loop (baseline)   {r['torch_baseline_ms'] * 1e3:10.1f} us   rounds {r['torch_baseline_ms_all']}")
        if name in stats:
            for row in csv.DictReader(open(stats[name])):
                if "gsr_detect::" not in row["Name"]:
                    continue
                avg = float(row["AverageNs"])
                k = row["Name"].split("(")[0].replace("void ", "")
                extra = ""
                if "k_det_score" in k:
                    tbps = r["score_pass_bytes"] / avg / 1e3
                    extra = f"   {r['score_pass_bytes']} bytes -> {tbps:.2f} TB/s = {100 * tbps / STREAM_TBPS:.0f} % of {STREAM_TBPS} TB/s streaming"
                lines.append(f"    {k:44s} {avg / 1e3:9.1f} us avg over {row['Calls']} calls{extra}")
        lines.append("")
    text = "\n".join(lines)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--hip-only", choices=list(CASES), default=None)
    ap.add_argument("--report", default=None, help="the JSON a plain run printed")
    ap.add_argument("--kernel-stats", nargs="*", default=[], help="case=kernel statistics csv (Name, Calls, AverageNs)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "detector_output_times.txt"))
    args = ap.parse_args()
    if args.report:
        report(args)
    else:
        measure(args)


if __name__ == "__main__":
    main()
