"""Losses that compare two images: the counterparts of the reference's utils/loss_utils.py (l1_loss, l2_loss, ssim) and
utils/image_utils.py (psnr) on the fused HIP stage (diff_gaussian_rasterization.imgloss_ops: one summation order, the same
bits on every run), and what an attack builds from them.

  l1_loss, l2_loss, ssim, psnr   the reference's names, signatures and return shapes
  ImageLoss                      (renders [B,C,H,W], reference [B,C,H,W]) -> scalar: the batch mean of
                                 w_l1 l1_b + w_l2 l2_b + w_ssim (1 - ssim_b)
  photometric_loss               (1 - lambda) L1 + lambda (1 - SSIM), the loss a 3DGS fit minimises
  with_image_term                a pgd_attack loss_fn plus weight x an ImageLoss against per-view reference renders: a stealth
                                 term that keeps the adversarial render close to the benign one

Deviations from the reference: the gradient flows to the first image alone (a second argument that requires grad raises);
the SSIM window is the reference's eleven float32 taps applied separably, one rounding per weight from its 2-D window;
window_size is 11; tensors live on a HIP device (no CPU path).
"""
from __future__ import annotations

from typing import Callable, Sequence, Union

import torch

from diff_gaussian_rasterization import imgloss_ops as IL


def _batch(t: torch.Tensor, fn: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or t.dim() not in (3, 4):
        raise ValueError(f"{fn}: images must be [C,H,W] or [B,C,H,W]")
    return t if t.dim() == 4 else t.unsqueeze(0)


def _terms(a: torch.Tensor, b: torch.Tensor, fn: str, w=(0.0, 0.0, 0.0)) -> torch.Tensor:
    return IL.image_loss(_batch(a, fn), _batch(b, fn), w[0], w[1], w[2])


def l1_loss(network_output: torch.Tensor, gt: torch.Tensor) -> torch.Tensor:
    """torch.abs(network_output - gt).mean(): a scalar."""
    return _terms(network_output, gt, "l1_loss", (1.0, 0.0, 0.0))[:, 3].mean()


def l2_loss(network_output: torch.Tensor, gt: torch.Tensor) -> torch.Tensor:
    """((network_output - gt) ** 2).mean(): a scalar."""
    return _terms(network_output, gt, "l2_loss", (0.0, 1.0, 0.0))[:, 3].mean()


def ssim(img1: torch.Tensor, img2: torch.Tensor, window_size: int = 11, size_average: bool = True) -> torch.Tensor:
    """The reference's ssim: the mean of the map (a scalar), or with size_average=False one mean per image ([B])."""
    if int(window_size) != 11:
        raise ValueError(f"ssim: window_size must be 11 (the kernels hold the eleven taps), got {window_size}")
    t = _terms(img1, img2, "ssim", (0.0, 0.0, 1.0))
    per_image = t[:, 2] + (t[:, 3].detach() - t[:, 3])      # the ssim column's bits; the gradient is minus loss_b = 1 - ssim_b's
    return per_image.mean() if size_average else per_image


def psnr(img1: torch.Tensor, img2: torch.Tensor) -> torch.Tensor:
    """20 log10(1 / sqrt(mse)) with the reference's mse: one mean per entry of the first dimension, [shape[0], 1] -- per
    image of a batch, per channel of a single [C,H,W] image."""
    if img1.dim() == 3:
        img1, img2 = img1.unsqueeze(1), img2.unsqueeze(1)
    mse = _terms(img1, img2, "psnr", (0.0, 1.0, 0.0))[:, 3:4]
    return 20 * torch.log10(1.0 / torch.sqrt(mse))


class ImageLoss:
    """(renders, reference) -> the batch mean of w_l1 l1_b + w_l2 l2_b + w_ssim (1 - ssim_b); clamp: both images clamped to
    [0,1] inside the kernel (renders are not clamped otherwise)."""

    def __init__(self, w_l1: float = 0.0, w_l2: float = 0.0, w_ssim: float = 1.0, clamp: bool = False):
        self.spec = IL.ImgLossSpec(float(w_l1), float(w_l2), float(w_ssim), bool(clamp))
        IL.c_spec(self.spec)                               # the weights are checked here

    def terms(self, renders: torch.Tensor, reference: torch.Tensor) -> torch.Tensor:
        s = self.spec
        return IL.image_loss(_batch(renders, "ImageLoss"), _batch(reference, "ImageLoss"), s.w_l1, s.w_l2, s.w_ssim, s.clamp)

    def __call__(self, renders: torch.Tensor, reference: torch.Tensor) -> torch.Tensor:
        return self.terms(renders, reference)[:, 3].mean()


def photometric_loss(img: torch.Tensor, gt: torch.Tensor, lambda_dssim: float = 0.2) -> torch.Tensor:
    """(1 - lambda_dssim) l1_loss(img, gt) + lambda_dssim (1 - ssim(img, gt)) in one call of the stage."""
    lam = float(lambda_dssim)
    return ImageLoss(1.0 - lam, 0.0, lam)(img, gt)


def with_image_term(loss_fn: Callable, reference_renders: torch.Tensor, image_loss: Callable, weight: float) -> Callable:
    """-> a loss_fn for pgd_attack(loss_fn=...): loss_fn(renders) + weight * image_loss(renders, reference_renders[idx]).
    reference_renders: [V,3,H,W], one per view (the benign renders); the returned function takes the global view indices
    (takes_view_index) and passes them on iff the inner loss_fn takes them.  weight == 0 calls the inner loss_fn alone."""
    if not isinstance(reference_renders, torch.Tensor) or reference_renders.dim() != 4:
        raise ValueError("with_image_term: reference_renders must be [V,3,H,W]")
    refs = reference_renders.detach()
    inner_takes = bool(getattr(loss_fn, "takes_view_index", False))
    weight = float(weight)

    def combined(renders: torch.Tensor, idx: Union[Sequence[int], None] = None) -> torch.Tensor:
        base = loss_fn(renders, idx=idx) if inner_takes else loss_fn(renders)
        if weight == 0.0:
            return base
        batch = _batch(renders, "with_image_term")
        ids = list(range(batch.shape[0])) if idx is None else [int(i) for i in idx]
        if len(ids) != batch.shape[0]:
            raise ValueError(f"with_image_term: {batch.shape[0]} renders for {len(ids)} view indices")
        ref = refs[torch.as_tensor(ids, device=refs.device)].to(batch.device)
        return base + weight * image_loss(batch, ref)

    combined.takes_view_index = True
    return combined
