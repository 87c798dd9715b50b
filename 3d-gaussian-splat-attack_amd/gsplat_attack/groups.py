"""Groups mode: select one object of a Gaussian-Grouping scene and attack it inside its scene.

Counterpart of the reference's third attack set-up (attack.py:292-323): a 1x1-conv classifier over the 16 per-Gaussian
object features picks the Gaussians of the selected object ids, every Gaussian inside the convex hull of those joins
them (attack.py:306-315), and the scene is split into the attacked group and the frozen rest (:321-323).  Then

    group, rest = split_group(model, mask3d)
    run_attack(group, cams, background=rest, ...)

-- the attack's renders see the group alone (reference :482), the success renders see group + rest (render_pair*).

Where the reference cannot run (its points_inside_convex_hull is not defined in attack.py: the import at :20 is commented
out) the semantics are ours (groups mode):
  * the hull is built on the host in double from the IQR-filtered selected positions; a position is inside iff it lies
    within the hull's bounding box grown by tau and n . x - c <= tau for every facet, tau = 1e-9 x the box's diagonal;
  * a degenerate hull (fewer than 4 points, or all of them on a point, a line or a plane -- Qhull raises there) selects
    nothing beyond the classifier's mask, and is reported;
  * an empty selection is an error of split_group: no attack starts on an empty model.
Classification and inclusion are HIP kernels (gsr_group_classify, gsr_points_in_hull): a few bytes per Gaussian instead
of the reference's [C,P] logits and softmax (2 GB at C = 256, P = 1 M).
"""
from __future__ import annotations

import os
import warnings
from typing import Sequence, Tuple

import numpy as np
import torch

from diff_gaussian_rasterization import groups as _G


def load_classifier(source) -> Tuple[torch.Tensor, torch.Tensor]:
    """A Conv2d(16, C, 1) classifier -> (weight [C,16], bias [C]) float32 on the host.  `source`: a path to a saved state
    dict, a state dict, or a module.  Both key styles load: a bare Conv2d's (``weight`` / ``bias``, as the reference's
    classifier.pth) and ObjectClassifier's (``conv.weight`` / ``conv.bias``)."""
    if isinstance(source, (str, os.PathLike)):
        source = torch.load(os.fspath(source), map_location="cpu", weights_only=True)
    if isinstance(source, torch.nn.Module):
        source = source.state_dict()
    sd = dict(source)
    for pre in ("", "conv."):
        if pre + "weight" in sd and pre + "bias" in sd:
            w, b = sd[pre + "weight"], sd[pre + "bias"]
            break
    else:
        raise KeyError(f"load_classifier: no weight/bias or conv.weight/conv.bias in the state dict (keys {sorted(sd)})")
    w = torch.as_tensor(w).detach().to("cpu", torch.float32)
    b = torch.as_tensor(b).detach().to("cpu", torch.float32).reshape(-1)
    C = int(w.shape[0])
    if w.dim() not in (2, 4) or w.reshape(C, -1).shape[1] != 16 or (w.dim() == 4 and tuple(w.shape[2:]) != (1, 1)) \
            or b.numel() != C:
        raise ValueError(f"load_classifier: weight {tuple(w.shape)} / bias {tuple(b.shape)} are not a Conv2d(16, C, 1)")
    if C > _G.MAX_CLASSES:
        raise ValueError(f"load_classifier: {C} classes; the classification kernel takes at most {_G.MAX_CLASSES}")
    return w.reshape(C, 16).contiguous(), b.contiguous()


def classify_gaussians(model, classifier, ids: Sequence[int], thresh: float = 0.5):
    """-> (mask [P] bool, psel [P] float32) on the model's device: psel = the largest softmax probability over `ids` of
    the classifier's logits of each Gaussian's object features, mask = psel > thresh (the reference's
    (prob[ids] > thresh).any(0), attack.py:306-309).  classifier: anything load_classifier takes, or its (weight, bias)."""
    w, b = classifier if isinstance(classifier, tuple) else load_classifier(classifier)
    obj = model._objects_dc
    dev = obj.device
    return _G.group_classify(obj, w.to(dev), b.to(dev), [int(i) for i in ids], thresh)


def _iqr_filter(pts: np.ndarray, outlier_factor: float) -> np.ndarray:
    # exactly scratch/edit_object_removal.py:52-56 (float32 percentiles of the float32 positions)
    Q1 = np.percentile(pts, 25, axis=0)
    Q3 = np.percentile(pts, 75, axis=0)
    IQR = Q3 - Q1
    outlier = (pts < (Q1 - outlier_factor * IQR)) | (pts > (Q3 + outlier_factor * IQR))
    return pts[~np.any(outlier, axis=1)]


def _hull_of(xyz: torch.Tensor, mask: torch.Tensor, remove_outliers: bool, outlier_factor: float):
    pts = xyz.detach()[mask.reshape(-1).bool()].float().cpu().numpy()
    if remove_outliers and pts.shape[0]:
        pts = _iqr_filter(pts, outlier_factor)
    return _G.convex_hull_planes(pts.astype(np.float64)), int(pts.shape[0])


def points_inside_convex_hull(xyz: torch.Tensor, mask: torch.Tensor, remove_outliers: bool = True,
                              outlier_factor: float = 1.0) -> torch.Tensor:
    """The reference's scratch function (edit_object_removal.py:31-69), same signature and meaning: the masked positions
    go to the host, optionally through the IQR outlier filter, their convex hull is built there, and [P] bool says which
    of ALL positions are inside it (here: a HIP kernel over the P positions).  A degenerate hull selects nothing and
    warns."""
    hull, _ = _hull_of(xyz, mask, remove_outliers, outlier_factor)
    if hull.degenerate:
        warnings.warn("points_inside_convex_hull: the filtered points span no volume (degenerate hull): nothing is inside",
                      stacklevel=2)
    return _G.points_in_hull(xyz.detach(), hull)


@torch.no_grad()
def select_group(model, classifier, ids: Sequence[int], select_thresh: float = 0.5, outlier_factor: float = 1.0):
    """The reference's selection (attack.py:306-315): the classifier's mask OR the Gaussians inside the convex hull of the
    IQR-filtered selected positions.  -> (mask3d [P] bool, info) with info = {"classified", "hull_points", "facets",
    "degenerate", "selected", "tau"}."""
    mask, _ = classify_gaussians(model, classifier, ids, select_thresh)
    xyz = model._xyz.detach()
    hull, kept = _hull_of(xyz, mask, True, outlier_factor)
    mask3d = _G.points_in_hull(xyz, hull, mask_in=mask)
    info = {"classified": int(mask.sum()), "hull_points": kept, "facets": int(hull.planes.shape[0]),
            "degenerate": bool(hull.degenerate), "selected": int(mask3d.sum()), "tau": float(hull.tau)}
    return mask3d, info


def split_group(model, mask3d: torch.Tensor):
    """-> (group, rest): the selected Gaussians (attacked) and the others (the frozen background), as the reference's
    attack.py:321-323 -- clone() + removal_setup on each side.  Storage order is kept on both sides."""
    sel = mask3d.reshape(-1).bool()
    if sel.numel() != model._xyz.shape[0]:
        raise ValueError(f"split_group: mask of {sel.numel()} entries for {model._xyz.shape[0]} Gaussians")
    n = int(sel.sum())
    if n == 0:
        raise ValueError("split_group: no Gaussian is selected (check the object ids, the classifier and the threshold); "
                         "an attack on an empty group changes nothing")
    group = model.clone()
    group.removal_setup(~sel)
    rest = model.clone()
    rest.removal_setup(sel)
    return group, rest


def fill_group(model, mask3d: torch.Tensor, k: int = 5):
    """-> (filled_model, new_mask): a clone of `model` with the selected Gaussians taken out and the hole filled as the
    reference's inpaint_setup does it (GaussianModel.inpaint_setup: one new Gaussian per removed one, every raw attribute
    the mean over the k nearest remaining Gaussians), and the bool mask of the new rows in the clone.  `model` itself is
    untouched.  The deviations from the reference are inpaint_setup's (ties to the lower index, fewer than k remaining
    Gaussians are averaged as they are, none remaining is a ValueError, no distance thresholds, no optimiser)."""
    sel = mask3d.reshape(-1).bool()
    if sel.numel() != model._xyz.shape[0]:
        raise ValueError(f"fill_group: mask of {sel.numel()} entries for {model._xyz.shape[0]} Gaussians")
    filled = model.clone()
    return filled, filled.inpaint_setup(sel, k=k)
