"""What the ctypes bindings of the image front end and the detector stages share (image_ops, detect_ops, detloss_ops,
setdet_ops, rcnn_ops, rpn_ops, fpn_ops, imgloss_ops, rpnloss_ops, objmap_ops): the device check, the error of a non-zero
return code, the capability test, the workspace, the cache of workspaces (one per sizer, device, stream and variant) and the
one way a C entry point is called."""
from __future__ import annotations

import ctypes
from typing import Dict, Hashable, Optional, Tuple

import torch

from . import _err, _load, _stream  # noqa: F401  (_stream: for the modules that import it from here)


def _need_device(t, fn: str, name: str) -> None:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{fn}: {name} must be a tensor")
    if not t.is_cuda:
        raise RuntimeError(f"{fn}: {name} must live on a HIP device (got {t.device}); there is no CPU path")


def _raise(lib, rc: int):
    raise (ValueError if rc == 1 else RuntimeError)(_err(lib))


def capability(item: int, bit: int) -> bool:
    """A bit of gsr_query(item) is set; a library that refuses the item has none of its stages."""
    out = ctypes.c_int64(0)
    return _load().gsr_query(item, ctypes.byref(out)) == 0 and bool(out.value & bit)


def workspace_bytes(symbol: str, cs) -> int:
    """The bytes `symbol` (a gsr_*_workspace_bytes) asks for the C spec `cs`."""
    lib = _load()
    n = ctypes.c_int64(0)
    rc = getattr(lib, symbol)(ctypes.byref(cs), ctypes.byref(n))
    if rc != 0:
        _raise(lib, rc)
    return int(n.value)


def workspace(nbytes: int, dev) -> torch.Tensor:
    """At least nbytes on dev as int64 words, a whole number of 16 bytes; its size in bytes is numel() * 8."""
    return torch.empty(((nbytes + 15) // 16 * 2,), dtype=torch.int64, device=dev)


# The cached workspaces of the stages that keep one (imgloss_ops, rpnloss_ops, objmap_ops): per sizer symbol, device, stream
# and variant, each of the last size asked for.  Calls on one stream run in order, so they may share a workspace; two
# streams never do.
_WS: Dict[Tuple[str, str, int, Hashable], Tuple[int, torch.Tensor]] = {}


def cached_workspace(symbol: str, cs, dev, variant: Hashable = None) -> torch.Tensor:
    """The workspace `symbol` sizes for the C spec `cs`, on dev's current stream: the one held for (symbol, dev, stream,
    variant) when it has that byte count, else a new one in its place.  variant tells apart the kinds of call a loop
    alternates between (with and without a gradient, say), so that they do not replace each other's workspace."""
    n = workspace_bytes(symbol, cs)
    key = (symbol, str(dev), int(torch.cuda.current_stream(dev).cuda_stream), variant)
    held = _WS.get(key)
    if held is None or held[0] != n:
        held = _WS[key] = (n, workspace(n, dev))
    return held[1]


def _ptr(t: Optional[torch.Tensor]):
    return t.data_ptr() if t is not None else None


def _f32(t: torch.Tensor, dev=None) -> torch.Tensor:
    return t.detach().to(device=dev, dtype=torch.float32).contiguous()


def _i32(t: torch.Tensor, dev=None) -> torch.Tensor:
    return t.detach().to(device=dev, dtype=torch.int32).contiguous()


def call(fn_name: str, dev, *args) -> None:
    """lib.<fn_name>(*args, current stream of dev) with dev selected; a non-zero return code raises the library's text."""
    lib = _load()
    with torch.cuda.device(dev):
        rc = getattr(lib, fn_name)(*args, _stream(dev))
    if rc != 0:
        _raise(lib, rc)
