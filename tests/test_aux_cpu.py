"""Depth / alpha maps, the parts that need no GPU: version, symbols and argument counts of the new entry points, the aux
keyword on CPU tensors (no fallback), argument checks of the two consumers."""
import ctypes

import pytest
import torch

import diff_gaussian_rasterization as D


def test_version_and_new_symbols():
    lib = D._load()
    out = ctypes.c_int64(0)
    assert lib.gsr_query(0, ctypes.byref(out)) == 0 and out.value == 604
    # the documented argument lists: the plain call's plus (out_depth, out_alpha) in front of `stream`
    assert len(lib.gsr_forward_aux.argtypes) == len(lib.gsr_forward.argtypes) + 2 == 19
    assert len(lib.gsr_forward_raw_aux.argtypes) == len(lib.gsr_forward_raw.argtypes) + 2 == 17
    assert len(lib.gsr_forward_raw_batch_aux.argtypes) == len(lib.gsr_forward_raw_batch.argtypes) + 2 == 16
    assert len(lib.gsr_ctx_set_aux_grads.argtypes) == 3
    # a null context is refused with a message, before anything touches a device
    assert lib.gsr_ctx_set_aux_grads(None, None, None) == 4
    assert b"gsr_ctx_set_aux_grads" in lib.gsr_last_error()


def _settings():
    eye = torch.eye(4)
    return D.GaussianRasterizationSettings(16, 16, 1.0, 1.0, torch.zeros(3), 1.0, eye, eye, 3, torch.zeros(3), False, False)


def test_aux_keyword_on_cpu_tensors_raises_like_the_existing_surface():
    P = 4
    st = _settings()
    with pytest.raises(RuntimeError, match="no CPU path"):
        D.GaussianRasterizer(st)(means3D=torch.zeros(P, 3), means2D=torch.zeros(P, 3), opacities=torch.ones(P, 1),
                                 shs=torch.zeros(P, 16, 3), scales=torch.ones(P, 3), rotations=torch.ones(P, 4), aux=True)
    with pytest.raises(RuntimeError, match="no CPU path"):
        D.rasterize_gaussians_raw(torch.zeros(P, 3), torch.zeros(P, 3), torch.zeros(P, 1, 3), torch.zeros(P, 15, 3), None,
                                  torch.zeros(P, 1), torch.zeros(P, 3), torch.ones(P, 4), st, aux=True)
    with pytest.raises(RuntimeError, match="no CPU path"):
        D.rasterize_gaussians_raw_batch(torch.zeros(P, 3), None, torch.zeros(P, 1, 3), torch.zeros(P, 15, 3),
                                        torch.zeros(P, 1), torch.zeros(P, 3), torch.ones(P, 4), [st, st], aux=True)


def test_pipeline_switch_defaults_off():
    from gsplat_attack.renderer import PipelineParams
    assert PipelineParams().aux_outputs is False and PipelineParams(aux_outputs=True).aux_outputs is True


def test_composite_over_argument_checks_and_values():
    from gsplat_attack import composite_over
    H, W = 4, 5
    alpha = torch.zeros(1, H, W)
    alpha[0, 1:3, 1:4] = 0.75
    image = torch.zeros(3, H, W)
    image[:, 1:3, 1:4] = 0.5
    photo = torch.rand(3, H, W, generator=torch.Generator().manual_seed(1))
    res = {"render": image.clone().requires_grad_(True), "render_alpha": alpha.clone().requires_grad_(True)}
    out = composite_over(res, photo)
    assert torch.equal(out.detach(), image + (1.0 - alpha) * photo)
    out.sum().backward()
    assert torch.equal(res["render_alpha"].grad[0], -photo.sum(0))
    batch = {"render": image.expand(2, 3, H, W), "render_alpha": alpha.expand(2, 1, H, W)}
    assert composite_over(batch, photo).shape == (2, 3, H, W)
    assert composite_over(batch, photo.expand(2, 3, H, W)).shape == (2, 3, H, W)
    with pytest.raises(KeyError, match="aux_outputs"):
        composite_over({"render": image}, photo)
    with pytest.raises(ValueError, match="does not match"):
        composite_over(res, photo[:, :3])
    with pytest.raises(ValueError, match="does not match"):
        composite_over(res, photo.expand(2, 3, H, W))
    with pytest.raises(ValueError, match="do not belong together"):
        composite_over({"render": image, "render_alpha": alpha[:, :2]}, photo)
    grey = image.clone()
    grey[:, 0, 0] = 0.25                               # an uncovered pixel that is not black: the render's background was not
    with pytest.raises(ValueError, match="black"):
        composite_over({"render": grey, "render_alpha": alpha}, photo)


def test_alpha_boxes_argument_checks():
    from gsplat_attack import benign_bboxes, bbox_from_alpha
    a = torch.zeros(6, 8)
    a[2:5, 3:7] = 0.9
    a[1, 1] = 0.3
    assert bbox_from_alpha(a, 0.5) == (3, 2, 7, 5) and bbox_from_alpha(a[None], 0.2) == (1, 1, 7, 5)
    assert bbox_from_alpha(a, 0.95) is None
    with pytest.raises(ValueError, match=r"\[H,W\]"):
        bbox_from_alpha(torch.zeros(2, 6, 8), 0.5)
    for bad in (-0.1, 1.0, 2.0):
        with pytest.raises(ValueError, match="alpha_threshold"):
            benign_bboxes(None, [], alpha_threshold=bad)
