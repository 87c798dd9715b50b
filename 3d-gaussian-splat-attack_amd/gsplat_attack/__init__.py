"""Counterparts of the reference's callers and data formats either side of the rasteriser."""
import os

# View pipelining (gsplat_attack.streams) deals a batch's views over four HIP streams; the HIP runtime maps a process's
# streams onto GPU_MAX_HW_QUEUES hardware queues (default 4, read at its first call) and streams sharing a queue
# serialise.  Ask for eight unless the user chose a value; harmless when the runtime is already initialised.
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")


def patch_reference(module_name: str = "gaussian_renderer") -> int:
    """Opt-in for a running reference checkout: make its ``render`` the fused one of this package.

    The reference's ``gaussian_renderer.render`` reaches the rasteriser through the classic surface (activated tensors
    built with PyTorch ops first).  This replaces that function object -- in ``gaussian_renderer`` itself and in every
    already-imported module that did ``from gaussian_renderer import render`` (``attack.py:20``) -- by
    ``gsplat_attack.renderer.render``: same signature, same returned dict, raw parameters straight into the kernels.
    Returns the number of bindings replaced.  Call it once after the reference's modules are imported."""
    import importlib
    import sys
    from .renderer import render as fused
    mod = sys.modules.get(module_name) or importlib.import_module(module_name)
    original = getattr(mod, "render")
    n = 0
    for m in list(sys.modules.values()):
        if m is not None and getattr(m, "render", None) is original:
            setattr(m, "render", fused)
            n += 1
    return n


def __getattr__(name):
    # the consumers of the depth / alpha maps, importable from the package without loading the attack loop up front
    if name in ("composite_over", "bbox_from_alpha", "benign_bboxes"):
        from . import attack
        return getattr(attack, name)
    # both sides of a set-prediction (DETR-style) detector
    if name in ("SetDetectorLoss", "SetDetectorOutput", "make_set_loss_fn"):
        from . import set_detector
        return getattr(set_detector, name)
    # both sides of a two-stage (R-CNN-style) detector
    if name in ("ProposalSampler", "RoIHeadLoss", "RoIHeadOutput", "FpnRoIPooler", "make_roi_loss_fn"):
        from . import roi_detector
        return getattr(roi_detector, name)
    # the region proposer in front of it
    if name in ("RpnProposer", "RpnLoss", "Proposals", "cell_anchors"):
        from . import proposals
        return getattr(proposals, name)
    # losses that compare two images, and the stealth term built from them
    if name in ("l1_loss", "l2_loss", "ssim", "psnr", "ImageLoss", "photometric_loss", "with_image_term"):
        from . import image_loss
        return getattr(image_loss, name)
    # the consumers of the object map: ids, boxes and a loss on the segmentation
    if name in ("segment_objects", "object_boxes", "group_bboxes", "object_ce", "ObjectMaps"):
        from . import objects
        return getattr(objects, name)
    # fitting a model: the optimiser of the reference's set-ups and the plain loop
    if name in ("OptimizationParams", "GaussianAdam", "get_expon_lr_func", "refit"):
        from . import optim
        return getattr(optim, name)
    # scoring an attack: COCO-style AP / AR on the device, the attack success rate, the evaluation sweep
    if name in ("DetectionEval", "reference_eval", "attack_success_rate", "evaluate_views", "to_coco_json", "from_coco_json"):
        from . import metrics
        return getattr(metrics, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
