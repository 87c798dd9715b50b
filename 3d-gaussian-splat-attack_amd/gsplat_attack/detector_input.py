"""What a detector does to the renders before its network sees them, on the image front end's HIP kernels
(diff_gaussian_rasterization.image_ops): one launch forward, one backward, and a backward that sums in a fixed order, so
that dL/dC reaches the rasteriser with the same bits on every run (torch's upsample_bilinear2d backward scatters with
float atomics).

  letterbox            the YOLO wrappers' resize + grey pad (detectors/yolov5_detector.py:59-76 and its siblings)
  letterbox_boxes      their boxes in the letterboxed frame, normalised xywh (yolov5_detector.py:79-90)
  resize_shorter_side  torchvision's Resize(int) + Normalize, DETR's input (detr_detector.py:129-134)
  resize_to_multiple   predict_and_save's resize to a multiple of 32 (yolov5_detector.py:115-119)
  DetectorInput        one of these as a callable; with_detector_input(loss_fn, di) composes it in front of a loss
"""
from __future__ import annotations

from typing import Callable, Optional, Sequence, Tuple

import torch

from diff_gaussian_rasterization.image_ops import ResampleSpec, resample

GREY = 114.0 / 255.0


def letterbox_geometry(H: int, W: int, new_shape=(640, 640)):
    """-> (scale, resized_h, resized_w, pad_top, pad_left): the aspect-preserving fit of H x W into new_shape, centred,
    the odd pixel of the padding going below / to the right."""
    new_h, new_w = int(new_shape[0]), int(new_shape[1])
    scale = min(new_h / H, new_w / W)
    rh, rw = int(round(H * scale)), int(round(W * scale))
    return scale, rh, rw, (new_h - rh) // 2, (new_w - rw) // 2


def _affine(mean, std):
    if mean is None and std is None:
        return None, None
    m = None if mean is None else tuple(float(v) for v in mean)
    s = None if std is None else tuple(1.0 / float(v) for v in std)
    return m, s


def _as_batch(images: torch.Tensor) -> torch.Tensor:
    x = images[None] if images.dim() == 3 else images
    return x.to(torch.float32)


def letterbox(images: torch.Tensor, new_shape=(640, 640), pad_value: float = GREY, clamp: bool = False):
    """images [B,3,H,W] -> (img [B,3,new_h,new_w], scale, pad_left, pad_top)."""
    x = _as_batch(images)
    H, W = int(x.shape[2]), int(x.shape[3])
    scale, rh, rw, top, left = letterbox_geometry(H, W, new_shape)
    spec = ResampleSpec(int(new_shape[0]), int(new_shape[1]), rh, rw, top, left, float(pad_value), None, None, bool(clamp))
    return resample(x, spec), scale, left, top


def letterbox_boxes(bboxes: torch.Tensor, scale: float, pad_left: int, pad_top: int, new_shape=(640, 640)) -> torch.Tensor:
    """bboxes [...,4] as pixel (x1, y1, x2, y2) of the unscaled image -> normalised (xc, yc, w, h) of the letterboxed one."""
    new_h, new_w = int(new_shape[0]), int(new_shape[1])
    b = bboxes * scale
    x1, y1 = (b[..., 0] + pad_left) / new_w, (b[..., 1] + pad_top) / new_h
    x2, y2 = (b[..., 2] + pad_left) / new_w, (b[..., 3] + pad_top) / new_h
    return torch.stack([(x1 + x2) / 2, (y1 + y2) / 2, x2 - x1, y2 - y1], dim=-1)


def shorter_side_size(H: int, W: int, size: int = 800) -> Tuple[int, int]:
    """torchvision's Resize(int): the shorter side becomes `size`, the longer int(size * long / short)."""
    short, long = (H, W) if H <= W else (W, H)
    new_long = int(size * long / short)
    return (size, new_long) if H <= W else (new_long, size)


def resize_shorter_side(images: torch.Tensor, size: int = 800, mean: Optional[Sequence[float]] = None,
                        std: Optional[Sequence[float]] = None, clamp: bool = False) -> torch.Tensor:
    x = _as_batch(images)
    rh, rw = shorter_side_size(int(x.shape[2]), int(x.shape[3]), int(size))
    m, s = _affine(mean, std)
    return resample(x, ResampleSpec(rh, rw, rh, rw, 0, 0, 0.0, m, s, bool(clamp)))


def resize_to_multiple(images: torch.Tensor, multiple: int = 32, clamp: bool = False) -> torch.Tensor:
    x = _as_batch(images)
    k = int(multiple)
    rh, rw = (int(x.shape[2]) + k - 1) // k * k, (int(x.shape[3]) + k - 1) // k * k
    return resample(x, ResampleSpec(rh, rw, rh, rw, 0, 0, 0.0, None, None, bool(clamp)))


class DetectorInput:
    """One detector's input stage as a callable renders [B,3,H,W] -> network input.  Exactly one of
    letterbox=(h, w) | shorter_side=size | multiple=k; clamp=True clamps the renders to [0,1] inside the same launch."""

    def __init__(self, letterbox: Optional[Tuple[int, int]] = None, shorter_side: Optional[int] = None,
                 multiple: Optional[int] = None, pad_value: float = GREY, mean: Optional[Sequence[float]] = None,
                 std: Optional[Sequence[float]] = None, clamp: bool = False):
        if sum(v is not None for v in (letterbox, shorter_side, multiple)) != 1:
            raise ValueError("DetectorInput: give exactly one of letterbox, shorter_side, multiple")
        if (mean is not None or std is not None) and shorter_side is None:
            raise ValueError("DetectorInput: mean / std go with shorter_side")
        self.letterbox, self.shorter_side, self.multiple = letterbox, shorter_side, multiple
        self.pad_value, self.mean, self.std, self.clamp = pad_value, mean, std, clamp

    def __call__(self, renders: torch.Tensor) -> torch.Tensor:
        if self.letterbox is not None:
            return letterbox(renders, self.letterbox, self.pad_value, self.clamp)[0]
        if self.shorter_side is not None:
            return resize_shorter_side(renders, self.shorter_side, self.mean, self.std, self.clamp)
        return resize_to_multiple(renders, self.multiple, self.clamp)


def with_detector_input(loss_fn: Callable[[torch.Tensor], torch.Tensor], detector_input: Callable) -> Callable:
    return lambda renders: loss_fn(detector_input(renders))
