"""Consumers of render()'s 16-channel object map (``render_object``).

The attack itself never reads that output; the reference's evaluation viewer does (``render.py:126-131``): a 1x1
convolution classifies the 16 composited object features per pixel, the arg-max is the object id map, and ids are
painted with a golden-ratio hue palette (``render.py:45-73``).  ``feature_to_rgb`` (``render.py:25-43``) shows the
features themselves through their first three principal components.

``segment_objects``, ``object_boxes``, ``group_bboxes`` and ``object_ce`` are the fused HIP counterparts
(``diff_gaussian_rasterization.objmap_ops``, ``gsr_objmap``): the id map without the [K,H,W] logit tensor, per-class boxes
and pixel counts taken inside the full scene, the painted image, and a cross-entropy loss on the segmentation whose
gradient reaches ``_objects_dc`` through the rasteriser.  They need a HIP device; the torch functions above stay as they are.
"""
from __future__ import annotations

import colorsys
from typing import NamedTuple, Optional, Sequence

import numpy as np
import torch
from torch import nn

NUM_OBJECTS = 16


class ObjectClassifier(nn.Module):
    """The per-pixel classifier of the object map: Conv2d(16, num_classes, kernel_size=1) (Gaussian-Grouping's;
    render.py:126 applies it to the [16,H,W] map as is)."""

    def __init__(self, num_classes: int = 256, num_objects: int = NUM_OBJECTS):
        super().__init__()
        self.conv = nn.Conv2d(num_objects, num_classes, kernel_size=1)

    def forward(self, render_object: torch.Tensor) -> torch.Tensor:
        return self.conv(render_object)


def predict_objects(render_object: torch.Tensor, classifier: nn.Module) -> torch.Tensor:
    """[16,H,W] object map -> [H,W] object ids (render.py:126-127)."""
    return torch.argmax(classifier(render_object), dim=0)


def id2rgb(id: int, max_num_obj: int = 256) -> np.ndarray:
    """Colour of an object id (render.py:45-63): hue by the golden ratio, saturation alternating, id 0 black."""
    if not 0 <= id <= max_num_obj:
        raise ValueError("ID should be in range(0, max_num_obj)")
    h = (id * 1.6180339887) % 1
    s = 0.5 + (id % 2) * 0.5
    rgb = np.zeros((3,), dtype=np.uint8)
    if id == 0:
        return rgb
    r, g, b = colorsys.hls_to_rgb(h, 0.5, s)
    rgb[0], rgb[1], rgb[2] = int(r * 255), int(g * 255), int(b * 255)
    return rgb


def visualize_obj(objects: np.ndarray) -> np.ndarray:
    """[H,W] ids -> [H,W,3] uint8 (render.py:65-71)."""
    out = np.zeros((*objects.shape[-2:], 3), dtype=np.uint8)
    for i in np.unique(objects):
        out[objects == i] = id2rgb(int(i))
    return out


def feature_to_rgb(features: torch.Tensor) -> np.ndarray:
    """[C,H,W] features -> [H,W,3] uint8: first three principal components, jointly normalised to 0..255
    (render.py:25-43).  Component signs follow the convention of making each component's largest-magnitude loading
    positive; a constant map gives zeros."""
    C, H, W = features.shape
    X = features.detach().reshape(C, -1).T.double().cpu()
    X = X - X.mean(dim=0, keepdim=True)
    _, _, Vt = torch.linalg.svd(X, full_matrices=False)
    Vt = Vt[:3]
    sign = torch.sign(Vt[torch.arange(Vt.shape[0]), Vt.abs().argmax(dim=1)])
    Vt = Vt * torch.where(sign == 0, torch.ones_like(sign), sign)[:, None]
    proj = (X @ Vt.T).reshape(H, W, -1).numpy()
    if proj.shape[2] < 3:
        proj = np.concatenate([proj, np.zeros((H, W, 3 - proj.shape[2]))], axis=2)
    span = proj.max() - proj.min()
    if span == 0:
        return np.zeros((H, W, 3), dtype=np.uint8)
    return (255 * (proj - proj.min()) / span).astype("uint8")


# ---- the fused stage (gsr_objmap) ---------------------------------------------------------------------------------------------
class ObjectMaps(NamedTuple):
    ids: torch.Tensor                  # [B,H,W] int32 ([H,W] for a [16,H,W] map); -1 where no logit compared greater than -inf
    conf: Optional[torch.Tensor]       # the arg-max's softmax probability, shaped like ids
    stats: torch.Tensor                # [B,K,5] int32 ([K,5]): count, left, upper, right, lower (right / lower exclusive)
    paint: Optional[torch.Tensor]      # [B,H,W,3] uint8 ([H,W,3]): id2rgb of every id, -1 black


def classifier_parameters(classifier):
    """(weight [K,16], bias [K]) of an ObjectClassifier, an nn.Conv2d(16, K, 1) or a (weight, bias) pair, detached."""
    if isinstance(classifier, ObjectClassifier):
        classifier = classifier.conv
    if isinstance(classifier, nn.Conv2d):
        if tuple(classifier.kernel_size) != (1, 1) or classifier.in_channels != NUM_OBJECTS or classifier.groups != 1:
            raise ValueError(f"the object classifier must be Conv2d({NUM_OBJECTS}, K, 1), got {classifier}")
        weight, bias = classifier.weight, classifier.bias
    elif isinstance(classifier, (tuple, list)) and len(classifier) == 2:
        weight, bias = classifier
    else:
        raise TypeError("classifier must be an ObjectClassifier, an nn.Conv2d(16, K, 1) or a (weight, bias) pair")
    weight = weight.detach().reshape(weight.shape[0], -1)
    if bias is None:
        bias = torch.zeros(weight.shape[0], dtype=weight.dtype, device=weight.device)
    return weight, bias.detach()


def object_palette(num_classes: int, device=None) -> torch.Tensor:
    """uint8 [K,3]: id2rgb of every class id."""
    rows = np.stack([id2rgb(i, max(256, num_classes)) for i in range(num_classes)])
    return torch.from_numpy(rows).to(device)


def segment_objects(render_object: torch.Tensor, classifier, *, conf: bool = False, paint: bool = False) -> ObjectMaps:
    """[B,16,H,W] or [16,H,W] object map -> ObjectMaps: predict_objects' ids (the first maximum; a NaN logit never wins),
    every class's pixel count and box, and on request the confidence and the painted image, in one fused call."""
    from diff_gaussian_rasterization import objmap_ops
    weight, bias = classifier_parameters(classifier)
    dev = render_object.device
    weight, bias = weight.to(dev), bias.to(dev)
    pal = object_palette(int(weight.shape[0]), dev) if paint else None
    out = objmap_ops.objmap_forward(render_object, weight, bias, palette=pal, want_conf=conf, want_stats=True, want_paint=paint)
    if render_object.dim() == 3:
        first = lambda t: None if t is None else t[0]
        return ObjectMaps(out.ids[0], first(out.conf), out.stats[0], first(out.paint))
    return ObjectMaps(out.ids, out.conf, out.stats, out.paint)


def object_boxes(stats: torch.Tensor, ids: Sequence[int]):
    """stats [B,K,5] (or [K,5]) of segment_objects, ids: the selected class ids -> per image (box, count): the union box
    (left, upper, right, lower) of the pixels the selected ids own, right / lower exclusive as PIL's getbbox gives them, or
    None when they own no pixel, and the number of those pixels.  A list for [B,K,5], one pair for [K,5].  One read-back."""
    if stats.dim() not in (2, 3) or stats.shape[-1] != 5:
        raise ValueError(f"object_boxes: stats must be [B,K,5] or [K,5], got {tuple(stats.shape)}")
    K = int(stats.shape[-2])
    sel = sorted({int(i) for i in ids})
    if any(not 0 <= i < K for i in sel):
        raise ValueError(f"object_boxes: ids must lie in 0..{K - 1}, got {sel}")
    rows = (stats if stats.dim() == 3 else stats.unsqueeze(0))[:, sel].cpu().numpy().astype(np.int64)
    out = []
    for r in rows:
        r = r[r[:, 0] > 0]
        if len(r) == 0:
            out.append((None, 0))
        else:
            out.append(((int(r[:, 1].min()), int(r[:, 2].min()), int(r[:, 3].max()), int(r[:, 4].max())), int(r[:, 0].sum())))
    return out if stats.dim() == 3 else out[0]


@torch.no_grad()
def group_bboxes(model, cameras: Sequence, classifier, ids: Sequence[int], pipe=None) -> list:
    """The object-map counterpart of attack.benign_bboxes: every view of the WHOLE scene rendered with its object channels, the
    map classified per pixel, and the box of the pixels the selected ids own returned per view (None where they own none)
    -- the visible extent of the selected object inside its scene, with no render of the object alone."""
    from .renderer import PipelineParams, render_views
    pipe = pipe or PipelineParams()
    black = torch.zeros(3, device=model.get_xyz.device)
    return [object_boxes(segment_objects(r["render_object"], classifier).stats, ids)[0]
            for r in render_views(cameras, model, pipe, black)]


def object_ce(render_object: torch.Tensor, target: torch.Tensor, classifier) -> torch.Tensor:
    """[B,16,H,W] (or [16,H,W]) object map, target ids [B,H,W] (or [H,W]; an id outside 0..K-1 is ignored) -> loss [B]: the
    mean cross entropy of the frozen classifier's per-pixel softmax against the target, differentiable with respect to the
    map -- and through render() to the model's object features."""
    from diff_gaussian_rasterization import objmap_ops
    weight, bias = classifier_parameters(classifier)
    dev = render_object.device
    return objmap_ops.object_ce(render_object, weight.to(dev), bias.to(dev), target)
