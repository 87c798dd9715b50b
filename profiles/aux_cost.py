"""What the depth / alpha maps cost, by gsr_profile stage times (HIP events around every stage, one stream):
S-nyc-1M at 1080p, forward + backward of one view, N views of the ring in turn.

  plain          colour only (rasterize_gaussians_raw)
  aux            colour + depth + alpha in ONE pass (aux=True, all three gradients)
  aux alpha only colour + alpha gradient (the segmented walk is kept)
  plain noseg    colour only under GSR_FLAG_NO_SEGMENTS (what the whole-list walk costs by itself)
  workaround     what the parent commit needs for the same maps and gradients: the colour pass PLUS a second classic-surface
                 forward + backward with colors_precomp = (z, 1, 0) on black, z through torch from the means

usage: python profiles/aux_cost.py [views]      (prints one table; profiles/aux_cost.txt is its output on one MI355X)
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "3d-gaussian-splat-attack_amd"), ROOT]
import diff_gaussian_rasterization as D                    # noqa: E402
from gsplat_attack.renderer import PipelineParams, _settings  # noqa: E402
from gsplat_attack.scenes import make_scene                # noqa: E402

STAGES = ("preprocess", "depth_sort", "bin", "tile_sort", "render_fwd", "render_bwd", "preprocess_bwd")


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 16
    dev = torch.device("cuda:0")
    model, cams, _ = make_scene("nyc-1M", device=dev, n_views=8)
    pipe = PipelineParams(skip_objects=True)
    black = torch.zeros(3, device=dev)
    H, W = cams[0].image_height, cams[0].image_width
    g = torch.Generator().manual_seed(1)
    gC, gD, gA = (torch.randn(3, H, W, generator=g).to(dev), torch.randn(1, H, W, generator=g).to(dev),
                  torch.randn(1, H, W, generator=g).to(dev))
    P = int(model._xyz.shape[0])

    def raw(cam, aux, flags=0):
        st = _settings(cam, model, pipe, black, 1.0)
        m2 = torch.zeros(P, 3, device=dev, requires_grad=True)
        with D.extra_flags(flags):
            return D.rasterize_gaussians_raw(model._xyz, m2, model._features_dc, model._features_rest, None, model._opacity,
                                             model._scaling, model._rotation, st, aux=aux)

    def plain(cam, flags=0):
        (raw(cam, False, flags)[0] * gC).sum().backward()

    def aux(cam):
        o = raw(cam, True)
        ((o[0] * gC).sum() + (o[3] * gD).sum() + (o[4] * gA).sum()).backward()

    def aux_alpha(cam):
        o = raw(cam, True)
        ((o[0] * gC).sum() + (o[4] * gA).sum()).backward()

    def second_pass(cam):
        st = _settings(cam, model, pipe, black, 1.0)
        xyz = model.get_xyz
        z = xyz @ cam.world_view_transform[:3, 2] + cam.world_view_transform[3, 2]
        col = torch.stack([z, torch.ones_like(z), torch.zeros_like(z)], dim=1)
        m2 = torch.zeros(P, 3, device=dev, requires_grad=True)
        c, _, _ = D.GaussianRasterizer(raster_settings=st)(means3D=xyz, means2D=m2, opacities=model.get_opacity,
                                                           colors_precomp=col, scales=model.get_scaling,
                                                           rotations=model.get_rotation)
        ((c[0:1] * gD).sum() + (c[1:2] * gA).sum()).backward()

    def workaround(cam):
        plain(cam)
        second_pass(cam)

    rows = {}
    for name, fn in (("plain", plain), ("aux", aux), ("aux alpha only", aux_alpha),
                     ("plain noseg", lambda c: plain(c, D.FLAG_NO_SEGMENTS)), ("workaround", workaround)):
        for i in range(3):                                   # warm-up: pools, capacity cache
            model.zero_grad()
            fn(cams[i % len(cams)])
        torch.cuda.synchronize()
        D.profile(True)
        for i in range(n):
            model.zero_grad()
            fn(cams[i % len(cams)])
        torch.cuda.synchronize()
        r = D.profile_read()
        D.profile(False)
        rows[name] = {k: r[k][0] / n for k in r}
    names = list(next(iter(rows.values())).keys())
    print(f"S-nyc-1M {W}x{H}, {P} Gaussians, {n} views, ms per view (device time of each stage, HIP events)")
    print(f"{'':16s}" + "".join(f"{k[:14]:>15s}" for k in names) + f"{'sum':>10s}")
    for name, r in rows.items():
        print(f"{name:16s}" + "".join(f"{r[k]:15.4f}" for k in names) + f"{sum(r.values()):10.4f}")
    a, w = sum(rows["aux"].values()), sum(rows["workaround"].values())
    print(f"aux / workaround = {a / w:.3f}   (aux - plain = {a - sum(rows['plain'].values()):.4f} ms)")


if __name__ == "__main__":
    main()
