"""The N > 1 code path with the REAL rasteriser: two processes (gloo; both on the box's one GPU) shard a batch of views,
run the fused backward, all-reduce the flat 59-floats-per-Gaussian bucket it hands out and take the PGD step; the
replicas end up identical and equal to the single-process run over the whole batch.  (RCCL itself needs N GPUs: this is
everything short of the transport.)"""
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

GROUPS = ("color", "position", "scaling", "rotation", "opacity")
KW = dict(P=20000, width=320, height=192)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _attack(model, cams, **kw):
    from gsplat_attack.attack import pgd_attack
    return pgd_attack(model, cams, iters=2, alpha=0.05, epsilon=0.5, groups=GROUPS, norm="l2", streams=1, **kw)


def _worker(rank, world, port, n_views, out_dir, accumulate):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK="0", HSA_ENABLE_IPC_MODE_LEGACY="0")
    import torch.distributed as dist
    from gsplat_attack import dist as gdist
    from gsplat_attack.renderer import PipelineParams, render
    from gsplat_attack.scenes import make_scene
    r, w, _ = gdist.init_from_env("gloo")
    assert (r, w) == (rank, world)
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    model, cams, _ = make_scene("nyc-1M", device=dev, n_views=n_views, **KW)
    # the fused backward hands out ONE flat bucket: the collective is a single all-reduce of 59 floats per Gaussian
    render(cams[rank % n_views], model, PipelineParams(skip_objects=True), torch.zeros(3, device=dev))["render"].sum().backward()
    flat = gdist._flat_view_of([getattr(model, n).grad for n in gdist.ATTACK_PARAMS])
    assert flat is not None and flat.numel() == 59 * model.get_xyz.shape[0]
    assert gdist.allreduce_attribute_grads(model) == flat.numel() * 4
    model.zero_grad()
    hist = _attack(model, cams, accumulate_grads=accumulate)
    torch.save({n: getattr(model, n).detach().cpu() for n in gdist.ATTACK_PARAMS} | {"hist": hist},
               os.path.join(out_dir, f"r{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("n_views,accumulate", [(4, False), (3, True), (1, False)])    # one view: rank 1 folds a bucket nothing wrote
def test_two_rank_attack_equals_the_single_process_batch(tmp_path, n_views, accumulate):
    from gsplat_attack import dist as gdist
    from gsplat_attack.scenes import make_scene
    import diff_gaussian_rasterization as D
    D._load()
    world, port = 2, _free_port()
    mp.spawn(_worker, args=(world, port, n_views, str(tmp_path), accumulate), nprocs=world, join=True)
    r0 = torch.load(tmp_path / "r0.pt")
    r1 = torch.load(tmp_path / "r1.pt")
    for k in gdist.ATTACK_PARAMS:
        assert torch.equal(r0[k], r1[k]), f"replicas diverged on {k}"      # an all-reduce returns the same bits everywhere
    assert r0["hist"] == r1["hist"]
    model, cams, _ = make_scene("nyc-1M", device=torch.device("cuda:0"), n_views=n_views, **KW)
    start = {n: getattr(model, n).detach().clone() for n in gdist.ATTACK_PARAMS}
    hist = _attack(model, cams, accumulate_grads=accumulate)
    assert hist == pytest.approx(r0["hist"], rel=1e-4)
    for n in gdist.ATTACK_PARAMS:
        moved = (getattr(model, n).detach() - start[n]).abs().max().item()
        assert moved > 0, n
        # same sum of per-view gradients in another order: float32 rounding of a normalised step
        assert (getattr(model, n).detach().cpu() - r0[n]).abs().max().item() <= 2e-3 * moved, n


def _nccl_worker(rank, world, port, n_views, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank), HSA_ENABLE_IPC_MODE_LEGACY="0")
    import torch.distributed as dist
    from gsplat_attack import dist as gdist
    from gsplat_attack.scenes import make_scene
    r, w, local = gdist.init_from_env("nccl")
    dev = torch.device("cuda", local)
    torch.cuda.set_device(dev)
    model, cams, _ = make_scene("nyc-1M", device=dev, n_views=n_views, **KW)
    hist = _attack(model, cams)
    torch.save({n: getattr(model, n).detach().cpu() for n in gdist.ATTACK_PARAMS} | {"hist": hist},
               os.path.join(out_dir, f"r{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs (RCCL over xGMI); lights up by itself on a bigger box")
def test_two_ranks_on_two_devices_over_rccl(tmp_path):
    """The same attack with one rank per DEVICE and the bucket all-reduced by RCCL ("nccl" backend): replicas bitwise
    equal, equal to the single-process batch within float32 rounding of a normalised step."""
    from gsplat_attack import dist as gdist
    from gsplat_attack.scenes import make_scene
    world, port, n_views = 2, _free_port(), 4
    mp.spawn(_nccl_worker, args=(world, port, n_views, str(tmp_path)), nprocs=world, join=True)
    r0 = torch.load(tmp_path / "r0.pt")
    r1 = torch.load(tmp_path / "r1.pt")
    for k in gdist.ATTACK_PARAMS:
        assert torch.equal(r0[k], r1[k]), f"replicas diverged on {k}"
    model, cams, _ = make_scene("nyc-1M", device=torch.device("cuda:0"), n_views=n_views, **KW)
    start = {n: getattr(model, n).detach().clone() for n in gdist.ATTACK_PARAMS}
    hist = _attack(model, cams)
    assert hist == pytest.approx(r0["hist"], rel=1e-4)
    for n in gdist.ATTACK_PARAMS:
        moved = (getattr(model, n).detach() - start[n]).abs().max().item()
        assert (getattr(model, n).detach().cpu() - r0[n]).abs().max().item() <= 2e-3 * moved, n


def test_bench_pgd_loop_rehearsal_prints_the_multi_gpu_fields(tmp_path):
    """bench.py --gpus 2 as the driver launches it (torch.distributed.run), rehearsed on the one GPU over gloo: the N > 1
    line times whole PGD iterations and carries allreduce_ms / bytes_reduced / views_per_rank."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, BENCH_REHEARSE_GLOO="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
           "--regions", "2", "--views-per-rank", "2", "--P", "20000", "--width", "320", "--height", "192", "--no-cpu-baseline",
           "--no-extras", "--full"]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1]
    d = json.loads(line)
    assert d["n_gpus"] == 2 and d["views_per_rank"] == 2 and d["config"]["loop"] == "pgd"
    assert d["bytes_reduced"] == 59 * 4 * 20000 and d["allreduce_ms"] > 0
    assert len(d["regions_ms"]) == 2 and d["value"] > 0 and d["steps"] == 2
    assert abs(d["value"] - 2 * 2 * 2 / (sorted(d["regions_ms"])[1] * 1e-3)) / d["value"] < 0.02
    # first contact with the 8-GPU node must not fail on trivia: every field the driver's checks need
    for k in ("n_gpus", "ranks_seen", "rccl", "allreduce_ms", "bytes_reduced", "views_per_rank", "independent_views",
              "collective_backend"):
        assert k in d, k
    iv = d["independent_views"]
    assert iv["value"] > 0 and abs(iv["value"] - 2 * iv["per_gpu"]) <= 0.02 * iv["value"] and iv["unit"] == "views/s"
    # config 4's shape: one view per rank, the bucket all-reduced in four ranges behind K9
    cmd2 = [c for c in cmd]
    cmd2[cmd2.index("--views-per-rank") + 1] = "1"
    cmd2[cmd2.index("--master-port") + 1] = str(_free_port())
    cmd2 += ["--ar-chunks", "4"]
    out = subprocess.run(cmd2, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    d = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
    assert d["views_per_rank"] == 1 and d["allreduce_chunks"] == 4 and d["bytes_reduced"] == 59 * 4 * 20000


def test_bench_started_as_a_plain_command_fans_out_by_itself():
    """`python3 bench.py --gpus 2 ...` WITHOUT torchrun (the shape of the driver's N = 1 command) must start
    its two ranks itself and measure both -- it used to print a note and time one GPU.  Rehearsed over gloo on the one
    GPU: the line says n_gpus 2 and ranks_seen 2 (an all-reduced 1)."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    env.update(BENCH_REHEARSE_GLOO="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--regions", "2",
           "--P", "20000", "--width", "320", "--height", "192", "--no-cpu-baseline", "--no-extras", "--full"]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, lines                              # ONE line, from rank 0
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["ranks_seen"] == 2 and d["collective_backend"] == "gloo" and d["config"]["loop"] == "pgd"
    assert d["bytes_reduced"] == 59 * 4 * 20000 and d["value"] > 0
    assert d["independent_views"]["value"] > 0 and d["views_per_rank"] == 1 and "rccl" in d and d["allreduce_ms"] > 0


def _chunk_worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK="0", HSA_ENABLE_IPC_MODE_LEGACY="0")
    import torch.distributed as dist
    import diff_gaussian_rasterization as D
    from gsplat_attack import dist as gdist
    from gsplat_attack.renderer import PipelineParams, render
    from gsplat_attack.scenes import make_scene
    gdist.init_from_env("gloo")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    model, cams, _ = make_scene("nyc-1M", device=dev, n_views=2, **KW)
    P = model.get_xyz.shape[0]
    gc = torch.randn(3, KW["height"], KW["width"], generator=torch.Generator().manual_seed(rank)).to(dev)
    res = {}
    for chunks in (1, 4, 7):
        bucket = D.GradBucket(P, dev)
        pipe = PipelineParams(skip_objects=True, grad_bucket=bucket)
        out = render(cams[rank], model, pipe, torch.zeros(3, device=dev))["render"]
        seen = []
        ar = gdist.BucketAllReduce(bucket, chunks)
        if chunks > 1:
            inner = bucket.on_chunk
            bucket.on_chunk = lambda c, g0, g1: (seen.append((c, g0, g1)), inner(c, g0, g1))
        out.backward(gc)
        nbytes = ar.wait()
        torch.cuda.synchronize()
        assert nbytes == 59 * 4 * P
        if chunks > 1:
            assert len(seen) == chunks and seen[0][1] == 0 and seen[-1][2] == P
            assert all(a[2] == b[1] and a[2] % 64 == 0 for a, b in zip(seen, seen[1:]))
        res[chunks] = bucket.flat.detach().cpu()
    torch.save(res, os.path.join(out_dir, f"c{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_bucket_all_reduce_in_ranges_equals_the_single_collective(tmp_path):
    """gsr_backward_raw_chunked + BucketAllReduce: the bucket all-reduced range by range from the backward's per-chunk
    callback holds, bit for bit, what one all-reduce of the whole bucket gives, on both ranks."""
    world, port = 2, _free_port()
    mp.spawn(_chunk_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    r0, r1 = torch.load(tmp_path / "c0.pt"), torch.load(tmp_path / "c1.pt")
    for chunks in (1, 4, 7):
        assert torch.equal(r0[chunks], r1[chunks]), chunks            # replicas agree
        assert torch.equal(r0[chunks], r0[1]), chunks                 # and the ranges add up to the single collective
    assert float(r0[1].abs().max()) > 0
