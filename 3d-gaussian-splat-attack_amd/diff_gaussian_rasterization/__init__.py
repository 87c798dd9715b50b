"""diff_gaussian_rasterization -- MI355X-native drop-in for the rasteriser the reference imports.

The reference does ``from diff_gaussian_rasterization import GaussianRasterizationSettings,
GaussianRasterizer`` (reference gaussian_renderer/__init__.py:14), builds the settings with the 12
keyword fields of :36-49, constructs ``GaussianRasterizer(raster_settings=...)`` (:51) and calls it with
the keyword arguments of :86-95, getting ``(color[3,H,W], radii[P] int32, objects[16,H,W])``.  This
package provides exactly that surface on top of ``libgsraster.so`` (hand-written HIP for gfx950, C ABI
declared in include/gsraster.h), bound with ctypes: PyTorch only supplies device memory, the current
stream and autograd plumbing.

There is NO fallback: without the compiled library or without a HIP device every entry point raises.
"""
from __future__ import annotations

import contextlib
import ctypes
import weakref
import os
from typing import NamedTuple, Optional

import torch
from torch import nn

from ._signatures import CHUNK_FN as _CHUNK_FN, SIGNATURES

NUM_OBJECTS = 16
_LIB_NAME = "libgsraster.so"
_lib = None

FLAG_NO_CULL = 1          # GSR_FLAG_NO_CULL (include/gsraster.h)
FLAG_NO_SEGMENTS = 1 << 16
FLAG_FWD_SHARED = 1 << 17   # the forward waves of a tile share one staging of the list (opt-in; include/gsraster.h)
FLAG_ASYNC_COUNT = 1 << 18  # GSR_FLAG_ASYNC_COUNT: never wait for the pair count (capacity guess + overflow flag)
FLAG_NO_SIDE_STREAM = 1 << 19   # GSR_FLAG_NO_SIDE_STREAM: SH -> RGB on the caller's stream instead of the side stream
FLAG_NEEDLE_DOUBLE = 1 << 20    # GSR_FLAG_NEEDLE_DOUBLE: needles' conic (and its backward) from the double chain (opt-in)
FLAG_OBJECTS_FOR_BACKWARD_ONLY = 1 << 21    # GSR_FLAG_OBJECTS_FOR_BACKWARD_ONLY: sh_objs kept for the backward, not composited
_FLAGS = int(os.environ.get("GSR_FLAGS", "0"), 0)


def flag_fwd_split(npx: int) -> int:
    """GSR_FLAG_FWD_SPLIT: pixels per lane (1|2|4) of the forward compositor, 0 = library's choice."""
    return {0: 0, 1: 1, 2: 2, 4: 3}[npx] << 4


def flag_bwd_split(npx: int) -> int:
    """GSR_FLAG_BWD_SPLIT: pixels per lane (2|4) of the backward compositor, 0 = library's choice."""
    return {0: 0, 2: 1, 4: 2}[npx] << 8


def flag_tile_map(mode: int) -> int:
    """GSR_FLAG_TILE_MAP: block -> tile map 0..3 (3 = longest list first, the default)."""
    return ((mode & 3) + 1) << 12


def set_flags(flags: int) -> None:
    """Extension flags passed in GsrSettings.flags by every later call (0 = default behaviour)."""
    global _FLAGS
    _FLAGS = int(flags)



@contextlib.contextmanager
def extra_flags(flags: int):
    """`with extra_flags(FLAG_NO_CULL): ...` -- the given bits are OR-ed into every call's flags inside the block."""
    global _FLAGS
    old = _FLAGS
    _FLAGS = old | int(flags)
    try:
        yield
    finally:
        _FLAGS = old


GSR_STAGES = ("preprocess", "depth_sort", "bin", "tile_sort", "render_fwd", "render_bwd", "preprocess_bwd")


class _CSettings(ctypes.Structure):
    # field order and types mirror `struct GsrSettings` in include/gsraster.h
    _fields_ = [
        ("image_height", ctypes.c_int32),
        ("image_width", ctypes.c_int32),
        ("tanfovx", ctypes.c_float),
        ("tanfovy", ctypes.c_float),
        ("bg", ctypes.c_void_p),
        ("scale_modifier", ctypes.c_float),
        ("viewmatrix", ctypes.c_void_p),
        ("projmatrix", ctypes.c_void_p),
        ("sh_degree", ctypes.c_int32),
        ("campos", ctypes.c_void_p),
        ("prefiltered", ctypes.c_int32),
        ("debug", ctypes.c_int32),
        ("flags", ctypes.c_uint32),
    ]


def library_path() -> str:
    # GSR_LIBRARY: another build of the same library (A/B runs of kernel variants on one box); default: the in-tree one
    return os.environ.get("GSR_LIBRARY") or os.path.join(os.path.dirname(os.path.abspath(__file__)), _LIB_NAME)


def _load():
    """Load libgsraster.so once; raise (never fall back) when it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    path = library_path()
    if not os.path.exists(path):
        raise RuntimeError(
            f"diff_gaussian_rasterization: {path} is missing. Build it with "
            f"`make -C {os.path.join(os.path.dirname(os.path.dirname(path)), 'csrc')}` (hipcc, gfx950); "
            "there is no CPU or PyTorch fallback for the raster path.")
    lib = ctypes.CDLL(path)
    # one declarative table (name -> restype, argtypes), applied to what this build exports: a library chosen through
    # GSR_LIBRARY for A/B runs may lack the newer entry points and still loads
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = restype, list(argtypes)
    _lib = lib
    return lib


GSR_ERR_INVALID, GSR_ERR_OVERFLOW = 1, 5          # include/gsraster.h


class PairCapacityExceeded(RuntimeError):
    """FLAG_ASYNC_COUNT only: a forward emitted more (tile, Gaussian) pairs than the capacity guessed from earlier views;
    its image is NaN.  Render again (the library counts synchronously on the next forward of that size)."""


def _err(lib) -> str:
    msg = lib.gsr_last_error()
    return msg.decode("utf-8", "replace") if msg else "unknown error"


def _rc_error(lib, rc: int, note: str = "", invalid=Exception) -> Exception:
    """The exception of a non-zero return code: GSR_ERR_INVALID -> `invalid` (the forwards have always raised a plain
    Exception for refused arguments and the backwards a RuntimeError: callers match on both), GSR_ERR_OVERFLOW ->
    PairCapacityExceeded, anything else -> RuntimeError; the text is gsr_last_error() plus `note`."""
    kind = invalid if rc == GSR_ERR_INVALID else PairCapacityExceeded if rc == GSR_ERR_OVERFLOW else RuntimeError
    return kind(_err(lib) + note)


class GaussianRasterizationSettings(NamedTuple):
    """The 12 fields of the call site, in its order (reference gaussian_renderer/__init__.py:36-49)."""
    image_height: int
    image_width: int
    tanfovx: float
    tanfovy: float
    bg: torch.Tensor
    scale_modifier: float
    viewmatrix: torch.Tensor
    projmatrix: torch.Tensor
    sh_degree: int
    campos: torch.Tensor
    prefiltered: bool
    debug: bool


def _f32c(t: torch.Tensor, device) -> torch.Tensor:
    if t.device != device:
        t = t.to(device)
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None or t.numel() == 0 else ctypes.c_void_p(t.data_ptr())


def _prep(t: Optional[torch.Tensor], device) -> Optional[torch.Tensor]:
    """What the library is handed for an input: detached, dense float32 on `device`; None for an absent or empty one."""
    return None if t is None or t.numel() == 0 else _f32c(t.detach(), device)


def _hip_device(t: torch.Tensor):
    if not t.is_cuda:
        raise RuntimeError(f"diff_gaussian_rasterization: tensors must live on a HIP device (got {t.device}); "
                           "there is no CPU path")
    return t.device


def _check_sh_storage(P: int, features_dc, features_rest) -> None:
    if tuple(features_dc.shape) != (P, 1, 3) or tuple(features_rest.shape) != (P, 15, 3):
        raise ValueError("fused path needs _features_dc [P,1,3] and _features_rest [P,15,3] (SH degree 3 storage)")


def _stream(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


_SMALL = {}      # (id(tensor), device) -> (weakref to it, its _version, dense float32 device copy, copy event, stream)


def _small_dense(t: torch.Tensor, device) -> torch.Tensor:
    """Dense float32 device form of a tiny settings tensor.  The reference's Camera keeps world_view_transform as a
    transposed VIEW and camera_center as a row of a column-major inverse (scene/cameras.py:54-57): both would cost a copy
    kernel on every render call.  The copy is made once per tensor object and version (weak reference: a dead or
    modified tensor is never served from here)."""
    if t.device == device and t.dtype == torch.float32 and t.is_contiguous():
        return t
    key = (id(t), str(device))
    hit = _SMALL.get(key)
    cur = torch.cuda.current_stream(device) if device.type == "cuda" else None
    if hit is not None and hit[0]() is t and hit[1] == t._version:
        if cur is not None and hit[4] != cur.cuda_stream:
            cur.wait_event(hit[3])          # the copy was enqueued on another stream: order this stream behind it
        return hit[2]
    d = _f32c(t.detach(), device)
    if d is t or d.data_ptr() == t.data_ptr():
        return d
    if len(_SMALL) > 512:
        _SMALL.clear()
    try:
        ev = None
        if cur is not None:
            ev = torch.cuda.Event()
            ev.record(cur)
        _SMALL[key] = (weakref.ref(t), t._version, d, ev, cur.cuda_stream if cur is not None else 0)
    except TypeError:
        pass
    return d


class _SettingsPack:
    """C settings + the device tensors it points into (kept alive as long as the pack lives)."""

    def __init__(self, rs: GaussianRasterizationSettings, device):
        self.device = device
        self.bg = _f32c(rs.bg.detach().flatten(), device)
        if self.bg.numel() < 3:
            raise ValueError("bg must hold at least 3 values")
        self.vm = _small_dense(rs.viewmatrix, device)
        self.pm = _small_dense(rs.projmatrix, device)
        self.cam = _small_dense(rs.campos, device).flatten()
        if self.vm.numel() != 16 or self.pm.numel() != 16 or self.cam.numel() < 3:
            raise ValueError("viewmatrix / projmatrix must be 4x4 and campos must hold 3 values")
        self.c = _CSettings(int(rs.image_height), int(rs.image_width), float(rs.tanfovx), float(rs.tanfovy),
                            self.bg.data_ptr(), float(rs.scale_modifier), self.vm.data_ptr(), self.pm.data_ptr(),
                            int(rs.sh_degree), self.cam.data_ptr(), int(bool(rs.prefiltered)), int(bool(rs.debug)),
                            _FLAGS)


class _CtxHolder:
    """Owns one GsrCtx; the workspace returns to the library's pool when the autograd graph dies."""

    def __init__(self, lib, handle):
        self.lib, self.handle = lib, handle

    def info(self, what: int) -> int:
        out = ctypes.c_int64(0)
        self.lib.gsr_ctx_info(self.handle, what, ctypes.byref(out))
        return out.value

    def __del__(self):
        if getattr(self, "handle", None):
            try:
                self.lib.gsr_ctx_free(self.handle)
            except Exception:
                pass
            self.handle = None


def _versions(tensors):
    return tuple(None if t is None else t._version for t in tensors)


def _check_versions(tensors, versions):
    """The kept buffers are aliases of the caller's tensors (no copy when they are already dense float32): the library
    re-reads them in backward, so an in-place modification in between would silently change the gradients."""
    for t, v in zip(tensors, versions):
        if t is not None and t._version != v:
            raise RuntimeError("one of the tensors given to the rasteriser's forward was modified in place before its "
                               f"backward ran (version {t._version}, expected {v}); clone it or step after backward()")


def _empty_if(cond, shape, device):
    """A gradient buffer for the backward to fill, or None when that gradient is not wanted."""
    return torch.empty(shape, dtype=torch.float32, device=device) if cond else None


def _shaped(t, shape, wanted=True):
    return None if (t is None or not wanted) else t.reshape(shape)


_ZERO = {}


def _zero_scalar(device):
    """One cached 1x1x1 zero per device: the object map handed back when no object features were composited."""
    z = _ZERO.get(device)
    if z is None:
        z = _ZERO[device] = torch.zeros(1, 1, 1, dtype=torch.float32, device=device)
    return z


_OBJ_ZERO = {}        # data_ptr -> (numel, _version, all zero?, weakref to the tensor) of object-feature tensors looked at


def _objects_all_zero(t: torch.Tensor, src: torch.Tensor) -> bool:
    """True when the object features `t` (dense float32 device tensor made from the caller's `src`) are all zero: their 16
    channels then composite to exactly zero, and the forward can run without them (the rasteriser's object variant of the
    forward compositor costs 0.27 ms against 0.16 at 1 M Gaussians / 1080p, plus 133 MB of output).  That is the attack's
    case: `combine_splats` gives every Gaussian of a combined scene zero object features (reference
    scene/gaussian_model.py:528), and the reference's render() passes them all the same (gaussian_renderer/__init__.py:81).
    The answer is cached per tensor object, storage and autograd version: one reduction and one host read the first time a
    tensor (version) is seen.  A tensor found non-zero is not looked at again while it keeps its storage (a training loop
    that steps the features every iteration never pays a second read); a zero one is re-checked when its version changes.
    An entry is served to the very tensor object it was made for only (weak reference, as RenderCache holds its geometry):
    the allocator hands a freed tensor's block to the next one of the same size, whose version starts at 0 again.
    No shortcut (False) when `t` is a temporary copy of a strided or non-float32 `src` -- its address says nothing about
    the caller's tensor -- and for an unseen tensor while the stream is being captured, where no host read is possible."""
    if not _OBJ_SHORTCUT:
        return False
    key = t.data_ptr()
    if key != src.data_ptr():
        return False
    ver = src._version
    hit = _OBJ_ZERO.get(key)
    if hit is not None and hit[0] == t.numel() and hit[3]() is src:
        if not hit[2]:
            return False                    # seen non-zero before: assume it still is
        if hit[1] == ver:
            return True
    if t.is_cuda and torch.cuda.is_current_stream_capturing():
        return False
    zero = not bool(torch.any(t != 0).item())
    if len(_OBJ_ZERO) > 256:
        _OBJ_ZERO.clear()
    _OBJ_ZERO[key] = (t.numel(), ver, zero, weakref.ref(src))
    return zero


_OBJ_SHORTCUT = os.environ.get("GSR_ZERO_OBJECT_SHORTCUT", "1") != "0"


def _arm_aux_grads(lib, holder, grad_depth, grad_alpha, shape, device):
    """Hands the two maps' incoming gradients (either may be None = zero) to the context's next backward
    (gsr_ctx_set_aux_grads).  -> the tensors to keep alive until that backward has been enqueued."""
    gd = None if grad_depth is None else _f32c(grad_depth.reshape(shape), device)
    ga = None if grad_alpha is None else _f32c(grad_alpha.reshape(shape), device)
    if gd is None and ga is None:
        return ()
    if lib.gsr_ctx_set_aux_grads(holder.handle, _ptr(gd), _ptr(ga)) != 0:
        raise RuntimeError(_err(lib))
    return (gd, ga)


class _CallOpts(NamedTuple):
    """Everything a render's autograd.Function is told besides its tensors, as ONE argument of .apply -- its last, so every
    backward returns one gradient per tensor input plus the same fixed tail, whatever options exist.  A new option is a
    new member here (with a default), read as `opts.<name>`; a new tensor input is a new position of .apply."""
    keep: bool = True               # keep backward state (decided by the caller of apply(): see _wants_backward)
    aux: bool = False               # also return the depth and alpha maps
    bucket: object = None           # GradBucket / GradBucketSet the attribute gradients are written into
    norms: Optional["GradNorms"] = None
    cache_slot: Optional[tuple] = None      # (RenderCache, key)
    color_only: bool = False        # no geometry gradient can be asked for: a re-render keeps no geometry backward state
    settings_list: tuple = ()       # (batch) the views' GaussianRasterizationSettings


class _RasterizeGaussians(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means3D, means2D, sh, sh_objs, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                raster_settings, opts):
        lib = _load()
        keep, aux = opts.keep, opts.aux
        ctx.aux = aux
        device = _hip_device(means3D)
        P = int(means3D.shape[0])
        m3, shc, shoc, colc = (_prep(t, device) for t in (means3D, sh, sh_objs, colors_precomp))
        opc, scc, roc, covc = (_prep(t, device) for t in (opacities, scales, rotations, cov3Ds_precomp))
        # all-zero object features composite to exactly zero: the forward runs without them and hands back a broadcast
        # zero; the context keeps the features, so a backward that IS given dL/dobjects still produces dL/dsh_objs
        obj_zero = shoc is not None and shoc.numel() == P * NUM_OBJECTS and _objects_all_zero(shoc, sh_objs)
        K = 0
        if shc is not None:
            if shc.dim() != 3 or shc.shape[2] != 3 or shc.shape[0] != P:
                raise ValueError(f"shs must be [P,K,3], got {tuple(shc.shape)}")
            K = int(shc.shape[1])
        if shoc is not None and shoc.numel() != P * NUM_OBJECTS:
            raise ValueError(f"sh_objs must hold P*{NUM_OBJECTS} values, got {tuple(shoc.shape)}")
        H, W = int(raster_settings.image_height), int(raster_settings.image_width)
        pack = _SettingsPack(raster_settings, device)
        color = torch.empty(3, H, W, dtype=torch.float32, device=device)
        # without object features the 16 object channels are identically zero: hand back a broadcast zero instead of
        # writing 16*H*W floats per view
        with_obj = shoc is not None and not obj_zero
        if obj_zero:
            pack.c.flags |= FLAG_OBJECTS_FOR_BACKWARD_ONLY
        objects = (torch.empty(NUM_OBJECTS, H, W, dtype=torch.float32, device=device) if with_obj
                   else _zero_scalar(device).expand(NUM_OBJECTS, H, W))
        radii = torch.empty(P, dtype=torch.int32, device=device)
        handle = ctypes.c_void_p(None)
        nren = ctypes.c_int64(0)
        # `keep` was decided by the caller of apply() (inside forward grad mode is always off and needs_input_grad is
        # True for a requires_grad tensor even under torch.no_grad()): a forward-only call keeps no backward state
        # (segment boundaries, d colour / d direction)
        with torch.cuda.device(device):
            head = (ctypes.byref(pack.c), P, K, _ptr(m3), _ptr(shc), _ptr(shoc), _ptr(colc), _ptr(opc), _ptr(scc), _ptr(roc),
                    _ptr(covc), _ptr(color), _ptr(objects) if with_obj else None, _ptr(radii),
                    ctypes.byref(handle) if keep else None, ctypes.byref(nren))
            if aux:
                depth = torch.empty(1, H, W, dtype=torch.float32, device=device)
                alpha = torch.empty(1, H, W, dtype=torch.float32, device=device)
                rc = lib.gsr_forward_aux(*head, _ptr(depth), _ptr(alpha), _stream(device))
            else:
                rc = lib.gsr_forward(*head, _stream(device))
        if rc != 0:
            note = ""
            if raster_settings.debug:
                torch.save({"means3D": m3, "sh": shc, "sh_objs": shoc, "colors_precomp": colc, "opacities": opc,
                            "scales": scc, "rotations": roc, "cov3D_precomp": covc,
                            "settings": raster_settings._asdict()}, "snapshot_fw.dump")
                note = " (inputs saved to snapshot_fw.dump)"
            raise _rc_error(lib, rc, note)
        ctx.holder = _CtxHolder(lib, handle) if keep else None
        ctx.pack = pack
        ctx._nren = nren.value
        ctx.shapes = tuple(None if t is None else t.shape for t in (means3D, means2D, sh, sh_objs, colors_precomp, opacities,
                                                                     scales, rotations, cov3Ds_precomp))
        # the library reads these again in backward: keep the exact (contiguous fp32) buffers alive, and remember
        # their versions -- an in-place edit between forward and backward must raise, as a saved tensor would
        ctx.kept = (m3, shc, shoc, colc, opc, scc, roc, covc)
        ctx.versions = _versions(ctx.kept)
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(radii)
        if aux:
            return color, radii, objects, depth, alpha
        return color, radii, objects

    @staticmethod
    def backward(ctx, grad_color, grad_radii, grad_objects, grad_depth=None, grad_alpha=None):
        lib = ctx.holder.lib
        _check_versions(ctx.kept, ctx.versions)
        m3, shc, shoc, colc, opc, scc, roc, covc = ctx.kept
        device = m3.device
        P = int(m3.shape[0])
        H, W = ctx.pack.c.image_height, ctx.pack.c.image_width
        if grad_color is None:
            grad_color = torch.zeros(3, H, W, dtype=torch.float32, device=device)
        gcol = _f32c(grad_color, device)
        gobj = None if (grad_objects is None or shoc is None) else _f32c(grad_objects, device)
        need = ctx.needs_input_grad
        # (input given?, its gradient's shape) per tensor input, in .apply's order -- which is gsr_backward's too
        outs = ((True, (P, 3)),                                                 # means3D
                (True, (P, 3)),                                                 # means2D
                (shc is not None, shc.shape if shc is not None else (0,)),      # sh
                (shoc is not None, (P, NUM_OBJECTS)),                           # sh_objs
                (colc is not None, (P, 3)),                                     # colors_precomp
                (True, (P,)),                                                   # opacities
                (scc is not None, (P, 3)),                                      # scales
                (roc is not None, (P, 4)),                                      # rotations
                (covc is not None, (P, 6)))                                     # cov3Ds_precomp
        grads = [_empty_if(wanted and given, shape, device) for wanted, (given, shape) in zip(need, outs)]
        with torch.cuda.device(device):
            # (the maps reach geometry and opacity only: with none of those gradients wanted theirs are not handed over)
            geo = need[0] or need[1] or need[5] or need[6] or need[7] or need[8]
            aux_keep = _arm_aux_grads(lib, ctx.holder, grad_depth, grad_alpha, (H, W), device) if (ctx.aux and P > 0 and geo) else ()
            rc = lib.gsr_backward(ctx.holder.handle, _ptr(gcol), _ptr(gobj), *[_ptr(g) for g in grads], _stream(device))
        if rc != 0:
            note = ""
            if ctx.pack.c.debug:
                torch.save({"grad_color": gcol, "grad_objects": gobj}, "snapshot_bw.dump")
                note = " (gradients saved to snapshot_bw.dump)"
            raise _rc_error(lib, rc, note, invalid=RuntimeError)
        if P == 0:
            for t in grads:
                if t is not None:
                    t.zero_()
        return tuple(_shaped(g, s) for g, s in zip(grads, ctx.shapes)) + _NO_GRAD


_NO_GRAD = (None, None)       # the two non-tensor arguments a single-view .apply ends with: the settings, the _CallOpts


class _RenderToken:
    """Held by the autograd node of a differentiable render through a kept context: while it is alive and not `done`,
    that render's backward may still come and the context must not be rendered again."""
    __slots__ = ("done", "__weakref__")

    def __init__(self):
        self.done = False


class _CacheEntry:
    __slots__ = ("holder", "sig", "refs", "pack", "gen", "event", "stream", "nren", "token")

    def __init__(self, holder, sig, refs, pack, nren):
        self.holder, self.sig, self.refs, self.pack, self.nren = holder, sig, refs, pack, nren
        self.gen = 0          # bumped by every render through this entry: a backward belongs to ONE generation
        self.event = None     # recorded after the entry's last use, on `stream`
        self.stream = None
        self.token = None     # weak reference to the _RenderToken of the entry's last differentiable render

    def busy(self) -> bool:
        t = self.token() if self.token is not None else None
        return t is not None and not t.done


class RenderCache:
    """Kept rasteriser contexts for renders whose GEOMETRY does not change from call to call -- a colour attack
    (reference attack.py:25-49: only _features_dc / _features_rest are stepped; BASELINE configs 2 and 3) renders the
    same cameras iteration after iteration with the same means, scales, rotations and opacities.  The first render of a
    key (one per camera) is an ordinary forward whose context is kept here; later renders of that key whose geometry
    inputs are the SAME tensor objects at the SAME autograd versions, under the same camera tensors / image size /
    scale modifier / SH degree / flags, run gsr_ctx_rerender: the colour half of K1 and the compositor K6 over the kept
    lists -- projection, both sorts, the emission and the schedule are not redone.  Anything else (a stepped geometry
    tensor, another camera behind the key, a non-dense input) silently takes the full forward and replaces the entry.
    Image and gradients are bit for bit those of the uncached call (tests/test_gpu_rerender.py).  "Unchanged" is what
    autograd itself goes by: an edit that bypasses a tensor's version counter (through `.data`, or a kernel writing
    through the raw pointer without bumping it) is not seen -- the reference's step functions (attack.py:25-173) and
    this package's fused step both go through the counter.

    One context per key: a render overwrites the per-pixel state the previous render's backward reads.  While the
    previous differentiable render of a key is still waiting for its backward (its graph is alive and has not been
    differentiated), another render of that key takes the full forward with a context of its own and leaves the entry
    alone; a second backward through a graph whose context has been rendered again since (retain_graph) raises.
    About 250 MB of HBM per entry
    at 1 M Gaussians and 1080p; the least recently used entry goes when `max_entries` is exceeded."""

    def __init__(self, max_entries: int = 64):
        import collections
        self.max_entries = int(max_entries)
        self.entries = collections.OrderedDict()
        self.hits = self.misses = self.bypassed = 0
        self.dropped_overflow = 0        # entries dropped because their (asynchronously counted) forward had overflowed

    def clear(self):
        self.entries.clear()

    def _lookup(self, key, sig, tensors):
        """-> (entry or None, may_store): a busy entry (see the class comment) is neither used nor replaced."""
        e = self.entries.get(key)
        if e is not None and e.busy():
            self.bypassed += 1
            return None, False
        if e is None or e.sig != sig or any(r() is not t for r, t in zip(e.refs, tensors)):
            self.misses += 1
            return None, True
        self.entries.move_to_end(key)
        self.hits += 1
        return e, True

    def _store(self, key, entry):
        self.entries[key] = entry
        self.entries.move_to_end(key)
        while len(self.entries) > self.max_entries:
            self.entries.popitem(last=False)


def _cache_sig(tensors, rs: "GaussianRasterizationSettings", extra=()):
    """What must be unchanged for a kept context to be re-rendered: storage and autograd version of the geometry and
    the camera tensors (their identity is checked through weak references besides: same object + same version means same
    shape and contents), and the scalar settings.  One flat tuple: this runs on every cached render."""
    sig = [int(rs.image_height), int(rs.image_width), float(rs.tanfovx), float(rs.tanfovy), float(rs.scale_modifier),
           int(rs.sh_degree), _FLAGS]
    for t in tensors:
        if t is None:
            sig.append(None)
        else:
            sig.append(t.data_ptr())
            sig.append(t._version)
    for t in (rs.viewmatrix, rs.projmatrix, rs.campos):
        sig.append(t.data_ptr())
        sig.append(t._version)
    sig.extend(extra)
    return tuple(sig)


def _entry_enter(entry: _CacheEntry, device):
    """Orders the current stream behind the entry's last use (a no-op on the same stream)."""
    cur = torch.cuda.current_stream(device)
    if entry.event is not None and entry.stream != cur.cuda_stream:
        cur.wait_event(entry.event)


def _entry_leave(entry: _CacheEntry, device):
    cur = torch.cuda.current_stream(device)
    if entry.event is None:
        entry.event = torch.cuda.Event()
    entry.event.record(cur)
    entry.stream = cur.cuda_stream


def _views_sig(geo, views, kind: str, obj):
    """(signature, tensors to hold weak references to) of a render of `views` (one GaussianRasterizationSettings per view;
    a single-view render has one) over the geometry tensors `geo`.  `kind` names the context's kind -- "view", "batch",
    "pair", "pair-batch": a key never re-renders a context of another kind -- and `obj` how it treats the object channels.
    The later views add their field of view and camera tensor versions to view 0's signature; every view's camera tensors
    are identity-checked besides: a new camera object that happens to get the id, the addresses and the versions of a dead
    one is never mistaken for it."""
    extra = [kind, len(views), obj]
    for rs in views[1:]:
        extra += [float(rs.tanfovx), float(rs.tanfovy)]
        for t in (rs.viewmatrix, rs.projmatrix, rs.campos):
            extra += [t.data_ptr(), t._version]
    refs = tuple(geo) + tuple(t for rs in views for t in (rs.viewmatrix, rs.projmatrix, rs.campos))
    return _cache_sig(geo, views[0], extra=extra), refs


def _cache_probe(cache: RenderCache, key, geo, used, views, kind: str, obj, honour_busy: bool):
    """-> (entry to re-render or None, signature to store the coming forward's context under or None, refs).
    `geo` are the caller's geometry tensors and `used` the dense forms the library is handed: a context is kept only when
    they are the same storage (the address of a temporary copy says nothing about the caller's tensor).  `honour_busy`:
    an entry waiting for its backward is left alone and nothing is stored (RenderCache); the forward-only pair renders,
    whose contexts have no backward, pass False."""
    if not all(a is None or a.data_ptr() == b.data_ptr() for a, b in zip(geo, used)):
        return None, None, None
    sig, refs = _views_sig(geo, views, kind, obj)
    entry, may_store = cache._lookup(key, sig, refs)
    if honour_busy and not may_store:
        sig = None                      # the key's context is waiting for a backward: plain forward, not stored
    return entry, sig, refs


def _cache_rerender(lib, cache: RenderCache, key, entry: _CacheEntry, device, dc, rest, dc_b, rest_b, bg, color, objects,
                    flags: int):
    """Renders through the kept context of a hit: colour kernel + compositor only (gsr_ctx_rerender).
    -> (rc, entry); entry is None when the kept context's forward (GSR_FLAG_ASYNC_COUNT) turned out to have overflowed its
    guessed pair capacity: it can never be re-rendered.  The entry is dropped, and the caller takes the full forward in
    this very call (which counts synchronously after an overflow) instead of poisoning the key."""
    _entry_enter(entry, device)
    rc = lib.gsr_ctx_rerender(entry.holder.handle, _ptr(dc), _ptr(rest), _ptr(dc_b), _ptr(rest_b), _ptr(bg), _ptr(color),
                              _ptr(objects), flags, _stream(device))
    entry.gen += 1
    if rc == GSR_ERR_OVERFLOW:
        cache.entries.pop(key, None)
        cache.dropped_overflow += 1
        return rc, None
    return rc, entry


def _cache_store(cache: RenderCache, key, holder: _CtxHolder, sig, refs, pack, nren: int) -> _CacheEntry:
    """Keeps a forward's context under `key`.  `pack` is what the context's pointers point into plus the radii of this
    render: the kept context does not recompute them, later renders of the key return these."""
    entry = _CacheEntry(holder, sig, tuple(weakref.ref(t) if t is not None else (lambda: None) for t in refs), pack, nren)
    cache._store(key, entry)
    return entry


def _cache_leave(entry: _CacheEntry, device, node=None, keep: bool = False) -> None:
    """After a render through `entry` has been enqueued: records the entry's last use and, for a differentiable path, ties
    its autograd `node` to this generation of the entry (`keep`: a backward may come, so the entry is busy until then).
    The forward-only pair renders have no node."""
    _entry_leave(entry, device)
    if node is not None:
        node.entry, node.entry_gen = entry, entry.gen
        if keep:
            node.token = _RenderToken()
            entry.token = weakref.ref(node.token)


def _cache_backward_enter(node, device, what: str) -> None:
    if node.entry is not None:
        if node.entry.gen != node.entry_gen:
            raise RuntimeError(f"diff_gaussian_rasterization: this {what}'s kept context (RenderCache) was rendered again "
                               "before its backward ran; call backward() first, or render without the cache")
        _entry_enter(node.entry, device)


def _cache_backward_leave(node, device) -> None:
    if node.entry is not None:
        _entry_leave(node.entry, device)
        node.token.done = True


def _coeff_sig(src_dc, src_rest, dc, rest):
    """Storage and version of the second model's two coefficient tensors (a pair render's frozen background, reference
    attack.py:513-530), or None when the library was handed temporary dense copies of them."""
    if src_dc.data_ptr() != dc.data_ptr() or src_rest.data_ptr() != rest.data_ptr():
        return None
    return tuple((t.data_ptr(), t._version) for t in (src_dc, src_rest))


def _pair_rerender_args(kept, b_sig, dc_b, rest_b):
    """-> (features_dc_b, features_rest_b, flags) of a pair context's gsr_ctx_rerender: while the second model's
    coefficient tensors are the ones of the entry's last render, unmodified, the colour kernel runs over the first model's
    Gaussians only (flag 2).  `kept` (the entry's pack) remembers this render's for the next."""
    same = b_sig is not None and kept.b_sig == b_sig
    kept.b_sig = b_sig
    return (None, None, 1 | 2) if same else (dc_b, rest_b, 1)


class GradNorms:
    """The six sums of squares the reference's L2 steps divide by (attack.py:53-119, 138-173: one global norm per raw
    attribute tensor, _features_dc and _features_rest separately), taken from the raster backward that WRITES the
    gradients instead of from a second pass over 236 MB of them (gsr_ctx_request_sumsq).  A rasterise call that is given
    one arms its backward when that backward overwrites its outputs; `sumsq_of(name)` hands the step the device scalar
    only while exactly ONE backward has contributed since begin() -- a second view's gradients added on top (autograd
    accumulation, a GradBucket in add mode, a folded or all-reduced bucket) make the sums stale, and the caller falls
    back to summing the gradient itself."""
    NAMES = ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation")

    def __init__(self, device):
        self.sumsq = torch.zeros(6, dtype=torch.float64, device=device)
        self.writes = 0            # backwards that contributed since begin()
        self.names = ()            # tensors whose sums the one arming backward wrote

    def begin(self):
        self.writes, self.names = 0, ()

    def invalidate(self):
        self.writes = 2

    def sumsq_of(self, name: str):
        if self.writes != 1 or name not in self.names:
            return None
        i = self.NAMES.index(name)
        return self.sumsq[i:i + 1]


class GradBucket:
    """Caller-owned gradient bucket of a reference-style GaussianModel: ONE flat float32 buffer of 59 floats per Gaussian
    in the order xyz | f_dc | f_rest | opacity | scaling | rotation (the layout of the flat buffer the fused backward
    hands to autograd, and of the all-reduce bucket of gsplat_attack.dist).  A rasterise call that is given a bucket
    writes its attribute gradients straight into it -- the first backward after reset() overwrites, later ones add
    (gsr_backward_raw_into) -- and returns no gradient for those inputs to autograd: the per-view 236-byte-per-Gaussian
    gradient buffer and the framework's read-modify-write accumulation into .grad both disappear (reference
    attack.py:476-494 accumulates B views' gradients in .grad).  One bucket per stream: concurrent backwards must not
    share one."""
    CUTS = (0, 3, 6, 51, 52, 55, 59)
    NAMES = ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation")
    SHAPES = ((3,), (1, 3), (15, 3), (1,), (3,), (4,))

    def __init__(self, P: int, device):
        self.P = int(P)
        self.flat = torch.empty(59 * self.P, dtype=torch.float32, device=device)
        self.fresh = True          # the next backward overwrites instead of adding
        self.used = False          # some backward has written since reset()
        # The next backward runs its per-Gaussian stage in `chunks` launches over ranges of Gaussians and calls
        # on_chunk(chunk, g_begin, g_end) after each one is enqueued (gsr_backward_raw_chunked): the hook of a
        # multi-GPU caller that all-reduces range by range while the rest is still being computed.  One-shot:
        # both are cleared by that backward.
        self.chunks = 1
        self.on_chunk = None

    def reset(self):
        self.fresh, self.used = True, False

    @staticmethod
    def carve(flat: torch.Tensor, P: int):
        """The six attribute pieces of a flat buffer of 59 P floats."""
        return [flat[c0 * P:c1 * P] for c0, c1 in zip(GradBucket.CUTS[:-1], GradBucket.CUTS[1:])]

    def slices(self):
        return self.carve(self.flat, self.P)

    def range_slices(self, g_begin: int, g_end: int):
        """The six pieces of the flat buffer that hold the gradients of Gaussians [g_begin, g_end)."""
        P, W = self.P, (3, 3, 45, 1, 3, 4)
        return [self.flat[c0 * P + g_begin * w:c0 * P + g_end * w] for c0, w in zip(self.CUTS[:-1], W)]

    def views(self) -> dict:
        """name -> tensor view shaped like the model's parameter (e.g. _features_rest: [P,15,3])."""
        return {n: sl.view(self.P, *shp) for n, sl, shp in zip(self.NAMES, self.slices(), self.SHAPES)}

    def add_(self, other: "GradBucket"):
        """Fold another (stream's) bucket into this one.  Buckets no backward wrote to hold nothing."""
        if other.used:
            if self.used:
                self.flat.add_(other.flat)
            else:
                self.flat.copy_(other.flat)
                self.used, self.fresh = True, False
        return self

    def assign_to(self, model):
        """model.<param>.grad = the bucket's view of it (no copy).  An unused bucket means zero gradients."""
        if not self.used:
            self.flat.zero_()
            self.used, self.fresh = True, False
        for n, v in self.views().items():
            p = getattr(model, n)
            p.grad = v.view(p.shape)


class GradBucketSet:
    """B gradient buckets of one model, one per view of a batch, in ONE flat buffer [B, 59 P] (each bucket laid out like a
    GradBucket: xyz | f_dc | f_rest | opacity | scaling | rotation).  Handed to rasterize_gaussians_raw_batch / render_batch
    (PipelineParams.grad_bucket) in place of a GradBucket, it receives every view's OWN attribute gradients
    (gsr_backward_raw_batch_views): the views share one launch chain and one backward composite, and view v's bucket holds
    bit for bit what the single-view backward of that view writes.  For callers that need per-view gradients -- independent
    views, per-view clipping or statistics; the attack's batch wants their sum and takes a GradBucket."""

    def __init__(self, B: int, P: int, device):
        self.B, self.P = int(B), int(P)
        self.flat = torch.empty(self.B * 59 * self.P, dtype=torch.float32, device=device)
        self.used = 0              # views written by the last backward

    def bucket(self, v: int) -> "GradBucket":
        """View v's gradients as a GradBucket over this set's memory (no copy)."""
        b = GradBucket.__new__(GradBucket)
        b.P = self.P
        b.flat = self.flat[v * 59 * self.P:(v + 1) * 59 * self.P]
        b.fresh, b.used, b.chunks, b.on_chunk = False, v < self.used, 1, None
        return b


class _GradPlan(NamedTuple):
    """Where a raw backward writes the six attribute gradients (xyz, f_dc, f_rest, opacity, scaling, rotation)."""
    bufs: list                  # one tensor per attribute, None = not wanted
    bucket: object              # the caller's GradBucket / GradBucketSet when `bufs` are its slices, else None
    per_view: bool              # ... a GradBucketSet: `bufs` are view 0's bucket, view v's lie 59 P floats further
    chunked: bool               # the bucket asked for the per-Gaussian stage in ranges (GradBucket.chunks)
    overwrites: bool            # the backward overwrites `bufs` with ONE summed gradient (what GradNorms can describe)


def _plan_attr_grads(want, P: int, device, bucket=None, B: int = 1) -> _GradPlan:
    """`want`: is the gradient of (xyz, the SH coefficients, opacity, scaling, rotation) needed?  A caller's bucket is used
    only when all of them are: it then receives the 59 attribute gradients directly (overwritten by the first backward
    after reset(), added to by the others) and autograd gets no gradient for those inputs."""
    w_x, w_sh, w_op, w_sc, w_ro = want
    if not (w_x and w_sh and w_op and w_sc and w_ro):
        wanted = (w_x, w_sh, w_sh, w_op, w_sc, w_ro)
        shapes = ((P, 3), (P, 1, 3), (P, 15, 3), (P,), (P, 3), (P, 4))
        return _GradPlan([_empty_if(w, shp, device) for w, shp in zip(wanted, shapes)], None, False, False, True)
    if isinstance(bucket, GradBucketSet):
        if bucket.P != P or bucket.B < B or bucket.flat.device != device:
            raise ValueError("grad bucket set does not match the batch (views, P or device)")
        return _GradPlan(bucket.bucket(0).slices(), bucket, True, False, False)
    if bucket is not None:
        if bucket.P != P or bucket.flat.device != device:
            raise ValueError("grad bucket does not match the model (P or device)")
        chunked = bucket.chunks > 1
        return _GradPlan(bucket.slices(), bucket, False, chunked, bucket.fresh and not chunked)
    # All 59 attack-relevant floats per Gaussian are wanted (the normal case): carve them out of ONE flat buffer, in the
    # order xyz | f_dc | f_rest | opacity | scaling | rotation.  autograd hands these views to .grad as they are, so a
    # data-parallel caller can sum the whole gradient with a single collective
    # (gsplat_attack.dist.allreduce_attribute_grads) instead of one per tensor.
    flat = torch.empty(59 * P, dtype=torch.float32, device=device)
    return _GradPlan(GradBucket.carve(flat, P), None, False, False, True)


def _autograd_attr_grads(plan: _GradPlan):
    """The six attribute gradients as autograd gets them after the backward ran: none when they went into the caller's
    bucket, which is marked written."""
    if plan.bucket is None:
        return plan.bufs
    if not plan.per_view:
        plan.bucket.fresh, plan.bucket.used = False, True
    return (None,) * 6


def _arm_norms(lib, norms: GradNorms, holder: _CtxHolder, plan: _GradPlan, want, strict: bool) -> None:
    """Asks the coming backward for the sums of squares of what it writes (gsr_ctx_request_sumsq), if it is the first since
    norms.begin() and overwrites its outputs with one summed gradient.  When the library refuses: `strict` raises (the
    single-view backward); otherwise the norms are invalidated and the step sums the gradient itself (the batch
    backward: a build or a mode that cannot serve it)."""
    norms.writes += 1
    if norms.writes == 1 and plan.overwrites:
        if lib.gsr_ctx_request_sumsq(holder.handle, ctypes.c_void_p(norms.sumsq.data_ptr())) != 0:
            if strict:
                raise RuntimeError(_err(lib))
            norms.invalidate()
            return
        w_x, w_sh, w_op, w_sc, w_ro = want
        norms.names = tuple(n for n, w in zip(GradNorms.NAMES, (w_x, w_sh, w_sh, w_op, w_sc, w_ro)) if w)
    elif not plan.overwrites:
        norms.invalidate()


def _chunk_trampoline(bucket: GradBucket):
    """-> (the gsr_chunk_fn that calls the bucket's one-shot on_chunk hook, the list its exception lands in): an exception
    must not unwind through the C frames, so the caller raises it after the library has returned."""
    hook, bucket.on_chunk = bucket.on_chunk, None
    errs = []

    def _done(_user, chunk, g0, g1):
        try:
            if hook is not None:
                hook(int(chunk), int(g0), int(g1))
        except BaseException as e:
            errs.append(e)
    return _CHUNK_FN(_done), errs


# Which entry point a raw backward calls.  Key: (batch context, per-view bucket set, object channels, chunked, into a
# bucket); value: (name, does it take grad_objects and dobjects_dc, what follows the gradient pointers).  Exactly the
# combinations the two backwards can reach: the entry points refuse other context kinds under their own names.
_BWD_PICK = {
    (False, False, False, False, False): ("gsr_backward_raw", True, ""),
    (False, False, True, False, False): ("gsr_backward_raw", True, ""),
    (False, False, False, False, True): ("gsr_backward_raw_into", True, "accumulate"),
    (False, False, True, False, True): ("gsr_backward_raw_into", True, "accumulate"),
    (False, False, False, True, True): ("gsr_backward_raw_chunked", True, "chunks"),
    (False, False, True, True, True): ("gsr_backward_raw_chunked", True, "chunks"),
    (True, False, False, False, False): ("gsr_backward_raw_batch_into", False, "accumulate"),
    (True, False, False, False, True): ("gsr_backward_raw_batch_into", False, "accumulate"),
    (True, False, True, False, False): ("gsr_backward_raw_batch_obj_into", True, "accumulate"),
    (True, False, True, False, True): ("gsr_backward_raw_batch_obj_into", True, "accumulate"),
    # the per-Gaussian stage in ranges, each announced as soon as its launch is enqueued (all-reduce overlap)
    (True, False, False, True, True): ("gsr_backward_raw_chunked", True, "chunks"),
    (True, False, True, True, True): ("gsr_backward_raw_chunked", True, "chunks"),
    (True, True, False, False, True): ("gsr_backward_raw_batch_views", False, "view_stride"),
    (True, True, True, False, True): ("gsr_backward_raw_batch_obj_views", True, "view_stride"),
}


def _call_raw_backward(lib, batch: bool, with_obj: bool, holder: _CtxHolder, plan: _GradPlan, gcol, gobj, d_m2, d_obj,
                       P: int, device) -> int:
    """The one C call of a raw backward, picked from _BWD_PICK.  -> its return code."""
    name, obj_args, tail = _BWD_PICK[(batch, plan.per_view, with_obj, plan.chunked, plan.bucket is not None)]
    fn = getattr(lib, name)
    d_x, d_dc, d_rest, d_op, d_sc, d_ro = (_ptr(t) for t in plan.bufs)
    if obj_args:
        args = (holder.handle, _ptr(gcol), _ptr(gobj), d_x, _ptr(d_m2), d_dc, d_rest, _ptr(d_obj), d_op, d_sc, d_ro)
    else:
        args = (holder.handle, _ptr(gcol), d_x, _ptr(d_m2), d_dc, d_rest, d_op, d_sc, d_ro)
    bucket, stream = plan.bucket, _stream(device)
    if tail == "":
        return fn(*args, stream)
    if tail == "view_stride":
        return fn(*args, 59 * P, stream)
    accumulate = 0 if (bucket is None or bucket.fresh) else 1
    if tail == "accumulate":
        return fn(*args, accumulate, stream)
    cb, errs = _chunk_trampoline(bucket)
    rc = fn(*args, accumulate, int(bucket.chunks), cb, None, stream)
    bucket.chunks = 1
    if errs:
        raise errs[0]
    return rc


class _RasterizeGaussiansRaw(torch.autograd.Function):
    """Same path with the activation getters fused into the kernels (gsr_forward_raw / gsr_backward_raw): takes the
    RAW parameter tensors of a reference-style GaussianModel."""

    @staticmethod
    def forward(ctx, xyz, means2D, features_dc, features_rest, objects_dc, opacity, scaling, rotation, raster_settings,
                opts):
        lib = _load()
        keep, aux = opts.keep, opts.aux
        cache_slot = None if aux else opts.cache_slot   # a kept context is never re-rendered with maps: aux bypasses the cache
        ctx.opts = opts
        ctx.entry = None
        device = _hip_device(xyz)
        P = int(xyz.shape[0])
        _check_sh_storage(P, features_dc, features_rest)
        x, dc, rest, obj = (_prep(t, device) for t in (xyz, features_dc, features_rest, objects_dc))
        op, sc, ro = (_prep(t, device) for t in (opacity, scaling, rotation))
        if obj is not None and obj.numel() != P * NUM_OBJECTS:
            raise ValueError(f"objects_dc must hold P*{NUM_OBJECTS} values, got {tuple(obj.shape)}")
        H, W = int(raster_settings.image_height), int(raster_settings.image_width)
        pack = _SettingsPack(raster_settings, device)
        color = torch.empty(3, H, W, dtype=torch.float32, device=device)
        # all-zero object features (the attack's combined scenes, reference scene/gaussian_model.py:528) composite to exactly
        # zero: as on the classic surface, the forward then runs without the 16 object channels and hands back a broadcast
        # zero; the context keeps the features for a backward that is given dL/dobjects
        obj_zero = obj is not None and _objects_all_zero(obj, objects_dc)
        with_obj = obj is not None and not obj_zero
        if obj_zero:
            pack.c.flags |= FLAG_OBJECTS_FOR_BACKWARD_ONLY
        objects = (torch.empty(NUM_OBJECTS, H, W, dtype=torch.float32, device=device) if with_obj
                   else _zero_scalar(device).expand(NUM_OBJECTS, H, W))
        handle = ctypes.c_void_p(None)
        nren = ctypes.c_int64(0)
        entry = sig = refs = None
        if cache_slot is not None and P > 0:
            cache, key = cache_slot
            geo = (xyz, opacity, scaling, rotation, objects_dc if obj is not None else None)
            entry, sig, refs = _cache_probe(cache, key, geo, (x, op, sc, ro, obj), [raster_settings], "view", obj_zero, True)
        with torch.cuda.device(device):
            if entry is not None:
                # the geometry of this key is what its kept context was built from
                radii = entry.pack.radii.detach()      # geometry is unchanged: so are the radii of the key's first render
                nren.value = entry.nren
                rc, entry = _cache_rerender(lib, cache, key, entry, device, dc, rest, None, None, pack.bg, color,
                                            objects if with_obj else None, 1 if opts.color_only else 0)
            if entry is None:
                radii = torch.empty(P, dtype=torch.int32, device=device)
                head = (ctypes.byref(pack.c), P, _ptr(x), _ptr(dc), _ptr(rest), _ptr(obj), _ptr(op), _ptr(sc), _ptr(ro),
                        _ptr(color), _ptr(objects) if with_obj else None, _ptr(radii),
                        ctypes.byref(handle) if (keep or sig is not None) else None, ctypes.byref(nren))
                if aux:
                    depth = torch.empty(1, H, W, dtype=torch.float32, device=device)
                    alpha = torch.empty(1, H, W, dtype=torch.float32, device=device)
                    rc = lib.gsr_forward_raw_aux(*head, _ptr(depth), _ptr(alpha), _stream(device))
                else:
                    rc = lib.gsr_forward_raw(*head, _stream(device))
        if rc != 0:
            note = ""
            if raster_settings.debug:
                torch.save({"xyz": x, "features_dc": dc, "features_rest": rest, "objects_dc": obj, "opacity": op,
                            "scaling": sc, "rotation": ro, "settings": raster_settings._asdict()}, "snapshot_fw.dump")
                note = " (raw parameters saved to snapshot_fw.dump)"
            raise _rc_error(lib, rc, note)
        if entry is not None:
            ctx.holder = entry.holder
        else:
            ctx.holder = _CtxHolder(lib, handle) if handle.value else None
            if sig is not None and ctx.holder is not None:
                pack.radii = radii
                entry = _cache_store(cache, key, ctx.holder, sig, refs, pack, nren.value)
        if entry is not None:
            _cache_leave(entry, device, ctx, keep)
        if not keep:
            ctx.holder = None
        ctx.pack = pack
        ctx._nren = nren.value
        ctx.shapes = (xyz.shape, means2D.shape, features_dc.shape, features_rest.shape,
                      None if objects_dc is None else objects_dc.shape, opacity.shape, scaling.shape, rotation.shape)
        ctx.kept = (x, dc, rest, obj, op, sc, ro)
        ctx.versions = _versions(ctx.kept)
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(radii)
        if aux:
            return color, radii, objects, depth, alpha
        return color, radii, objects

    @staticmethod
    def backward(ctx, grad_color, grad_radii, grad_objects, grad_depth=None, grad_alpha=None):
        lib = ctx.holder.lib
        _check_versions(ctx.kept, ctx.versions)
        x, dc, rest, obj, op, sc, ro = ctx.kept
        device = x.device
        _cache_backward_enter(ctx, device, "render")
        P = int(x.shape[0])
        H, W = ctx.pack.c.image_height, ctx.pack.c.image_width
        if grad_color is None:
            grad_color = torch.zeros(3, H, W, dtype=torch.float32, device=device)
        gcol = _f32c(grad_color, device)
        gobj = None if (grad_objects is None or obj is None) else _f32c(grad_objects, device)
        # inputs: xyz, means2D, features_dc, features_rest, objects_dc, opacity, scaling, rotation
        need = ctx.needs_input_grad
        want = (need[0], need[2] or need[3], need[5], need[6], need[7])
        plan = _plan_attr_grads(want, P, device, ctx.opts.bucket)
        d_m2 = _empty_if(need[1], (P, 3), device)
        d_obj = _empty_if(need[4] and obj is not None, (P, NUM_OBJECTS), device)
        if ctx.opts.norms is not None:
            _arm_norms(lib, ctx.opts.norms, ctx.holder, plan, want, strict=True)
        with torch.cuda.device(device):
            # (the maps reach geometry and opacity only: with none of those gradients wanted theirs are not handed over)
            geo = need[0] or need[1] or need[5] or need[6] or need[7]
            aux_keep = _arm_aux_grads(lib, ctx.holder, grad_depth, grad_alpha, (H, W), device) if (ctx.opts.aux and geo) else ()
            rc = _call_raw_backward(lib, False, obj is not None, ctx.holder, plan, gcol, gobj, d_m2, d_obj, P, device)
        if rc != 0:
            raise _rc_error(lib, rc, invalid=RuntimeError)
        _cache_backward_leave(ctx, device)
        s = ctx.shapes
        d_x, d_dc, d_rest, d_op, d_sc, d_ro = _autograd_attr_grads(plan)
        return (_shaped(d_x, s[0]), _shaped(d_m2, s[1]), _shaped(d_dc, s[2], need[2]), _shaped(d_rest, s[3], need[3]),
                _shaped(d_obj, s[4]), _shaped(d_op, s[5]), _shaped(d_sc, s[6]), _shaped(d_ro, s[7])) + _NO_GRAD


MAX_BATCH = 16                # views per gsr_forward_raw_batch call (csrc/gsr_kernels.hip.h)


class _BatchPack:
    """What a kept BATCH context's cache entry holds on to: the views' settings packs (their device tensors are what the
    context's pointers point into), the radii of the key's first render, and -- once a render came with other background
    tensors than the forward's -- the [B,3] tensor of background values the context reads instead."""
    __slots__ = ("packs", "radii", "bg_src", "bgt", "b_sig", "last_inputs")

    def __init__(self, packs, radii):
        self.packs, self.radii = packs, radii
        self.bg_src = tuple(pk.bg.data_ptr() for pk in packs)
        self.bgt = None
        self.b_sig = self.last_inputs = None      # (pair batches: the second model's coefficient versions, the inputs in flight)

    def background(self, packs):
        """What a re-render of the kept context is handed as background: None while the views' background tensors are the
        forward's own, else (and from then on) their values restacked as one [B,3] tensor."""
        ptrs = tuple(pk.bg.data_ptr() for pk in packs)
        if ptrs == self.bg_src and self.bgt is None:
            return None
        self.bgt, self.bg_src = torch.stack([pk.bg[:3] for pk in packs]).contiguous(), ptrs
        return self.bgt                         # (self.packs stays: the context's camera pointers point into them)


def _view_packs(settings_list, device):
    """-> (the views' settings packs, the same as the C array `const GsrSettings[B]` a batch entry point takes)."""
    B = len(settings_list)
    if not 1 <= B <= MAX_BATCH:
        raise ValueError(f"a batch holds 1..{MAX_BATCH} views, got {B}")
    packs = [_SettingsPack(rs, device) for rs in settings_list]
    carr = (_CSettings * B)()
    for v, pk in enumerate(packs):
        carr[v] = pk.c
    return packs, carr


class _RasterizeGaussiansRawBatch(torch.autograd.Function):
    """B views of one set of RAW parameters through ONE launch chain (gsr_forward_raw_batch / gsr_backward_raw_batch_into):
    what the reference's batch loop does with B render() calls and one accumulated .grad (attack.py:476-494).
    -> (color[B,3,H,W], radii[B,P]); the attribute gradients are the SUM over the views of dL/dC[v] pulled back.
    With objects_dc ([P,16] object features): the _obj entry points, -> (color, radii, objects[B,16,H,W]), and the object
    features' gradient is the view-ordered sum of the single-view ones."""

    @staticmethod
    def forward(ctx, xyz, means2D, features_dc, features_rest, opacity, scaling, rotation, objects_dc, opts):
        lib = _load()
        keep, aux, settings_list = opts.keep, opts.aux, opts.settings_list
        cache_slot = None if aux else opts.cache_slot     # aux renders bypass the cache (see _RasterizeGaussiansRaw)
        with_obj = objects_dc is not None
        if aux and with_obj:
            raise ValueError("rasterize_gaussians_raw_batch: aux=True with objects_dc is not supported (render the object "
                             "channels in a batch of their own)")
        ctx.opts = opts
        ctx.entry = None
        device = _hip_device(xyz)
        P = int(xyz.shape[0])
        packs, carr = _view_packs(settings_list, device)
        B = len(packs)
        _check_sh_storage(P, features_dc, features_rest)
        x, dc, rest = (_prep(t, device) for t in (xyz, features_dc, features_rest))
        op, sc, ro = (_prep(t, device) for t in (opacity, scaling, rotation))
        obj = _prep(objects_dc, device)
        if obj is not None and obj.numel() != P * NUM_OBJECTS:
            raise ValueError(f"objects_dc must hold P*{NUM_OBJECTS} values, got {tuple(objects_dc.shape)}")
        H, W = int(settings_list[0].image_height), int(settings_list[0].image_width)
        color = torch.empty(B, 3, H, W, dtype=torch.float32, device=device)
        objects = torch.empty(B, NUM_OBJECTS, H, W, dtype=torch.float32, device=device) if with_obj else None
        handle = ctypes.c_void_p(None)
        nren = ctypes.c_int64(0)
        # a kept batch context (RenderCache): the key's geometry tensors and ALL its views' camera tensors unchanged since the
        # key's last render -> the batch's colour kernel + one compositor launch over the kept lists (gsr_ctx_rerender)
        entry = sig = refs = None
        if cache_slot is not None and P > 0:
            cache, key = cache_slot
            # (the object features belong to the geometry: the context reads them through the forward's pointer)
            geo = (xyz, opacity, scaling, rotation, objects_dc if obj is not None else None)
            entry, sig, refs = _cache_probe(cache, key, geo, (x, op, sc, ro, obj), settings_list, "batch", with_obj, True)
        with torch.cuda.device(device):
            if entry is not None:
                radii = entry.pack.radii.detach()      # geometry is unchanged: so are the radii of the key's first render
                nren.value = entry.nren
                rc, entry = _cache_rerender(lib, cache, key, entry, device, dc, rest, None, None, entry.pack.background(packs),
                                            color, objects, 1 if opts.color_only else 0)
            if entry is None:
                radii = torch.empty(B, P, dtype=torch.int32, device=device)
                want_ctx = ctypes.byref(handle) if (keep or sig is not None) else None
                if with_obj:
                    rc = lib.gsr_forward_raw_batch_obj(carr, B, P, _ptr(x), _ptr(dc), _ptr(rest), _ptr(obj), _ptr(op), _ptr(sc),
                                                       _ptr(ro), _ptr(color), _ptr(objects), _ptr(radii), want_ctx,
                                                       ctypes.byref(nren), _stream(device))
                else:
                    head = (carr, B, P, _ptr(x), _ptr(dc), _ptr(rest), _ptr(op), _ptr(sc), _ptr(ro), _ptr(color), _ptr(radii),
                            want_ctx, ctypes.byref(nren))
                    if aux:
                        depth = torch.empty(B, 1, H, W, dtype=torch.float32, device=device)
                        alpha = torch.empty(B, 1, H, W, dtype=torch.float32, device=device)
                        rc = lib.gsr_forward_raw_batch_aux(*head, _ptr(depth), _ptr(alpha), _stream(device))
                    else:
                        rc = lib.gsr_forward_raw_batch(*head, _stream(device))
        if rc != 0:
            raise _rc_error(lib, rc)
        if entry is not None:
            ctx.holder = entry.holder
        else:
            ctx.holder = _CtxHolder(lib, handle) if handle.value else None
            if sig is not None and ctx.holder is not None:
                entry = _cache_store(cache, key, ctx.holder, sig, refs, _BatchPack(packs, radii), nren.value)
        if entry is not None:
            _cache_leave(entry, device, ctx, keep)
        if not keep:
            ctx.holder = None
        ctx.packs = packs
        ctx.pack = packs[0]
        ctx.B = B
        ctx._nren = nren.value
        ctx.shapes = tuple(None if t is None else t.shape for t in (xyz, means2D, features_dc, features_rest, opacity, scaling,
                                                                     rotation, objects_dc))
        ctx.kept = (x, dc, rest, op, sc, ro)
        ctx.obj = obj
        ctx.versions = _versions(ctx.kept + (obj,))
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(radii)
        if aux:
            return color, radii, depth, alpha
        if with_obj:
            return color, radii, objects
        return color, radii

    @staticmethod
    def backward(ctx, grad_color, grad_radii, *grad_maps):
        # outputs: (color, radii), (color, radii, objects) with objects_dc, (color, radii, depth, alpha) with aux
        grad_objects = grad_depth = grad_alpha = None
        if ctx.opts.aux:
            grad_depth, grad_alpha = grad_maps
        elif grad_maps:
            grad_objects, = grad_maps
        _check_versions(ctx.kept + (ctx.obj,), ctx.versions)
        x, dc, rest, op, sc, ro = ctx.kept
        # inputs: xyz, means2D, features_dc, features_rest, opacity, scaling, rotation, objects_dc; then the _CallOpts
        need = ctx.needs_input_grad
        s = ctx.shapes
        if x is None:                                  # an empty scene: empty gradients
            dev0 = ctx.packs[0].device
            return tuple(torch.zeros(shp, dtype=torch.float32, device=dev0) if (need[i] and shp is not None) else None
                         for i, shp in enumerate(s)) + (None,)
        lib = ctx.holder.lib
        device = x.device
        _cache_backward_enter(ctx, device, "batch")
        P, B = int(x.shape[0]), ctx.B
        H, W = ctx.pack.c.image_height, ctx.pack.c.image_width
        if grad_color is None:
            grad_color = torch.zeros(B, 3, H, W, dtype=torch.float32, device=device)
        gcol = _f32c(grad_color, device)
        want = (need[0], need[2] or need[3], need[4], need[5], need[6])
        plan = _plan_attr_grads(want, P, device, ctx.opts.bucket, B)
        d_m2 = _empty_if(need[1], (B, P, 3), device)
        # object channels: dL/dobjects [B,16,H,W] (or None: the segmented composite of the no-object batch runs) and the
        # object features' gradient [P,16], always written (zeros without dL/dobjects)
        with_obj = s[7] is not None
        gobj = _f32c(grad_objects, device) if (with_obj and grad_objects is not None and ctx.obj is not None) else None
        d_obj = _empty_if(with_obj and need[7], (P, NUM_OBJECTS), device)
        # a bucket set receives per-view object gradients [B,P,16], summed below in view order (autograd's association)
        d_objv = _empty_if(plan.per_view and d_obj is not None, (B, P, NUM_OBJECTS), device)
        if ctx.opts.norms is not None:
            # the batch's ONE backward writes the summed gradient: its sums of squares are the L2 steps' norms (GradNorms)
            _arm_norms(lib, ctx.opts.norms, ctx.holder, plan, want, strict=False)
        with torch.cuda.device(device):
            geo = need[0] or need[1] or need[4] or need[5] or need[6]
            aux_keep = _arm_aux_grads(lib, ctx.holder, grad_depth, grad_alpha, (B, H, W), device) if (ctx.opts.aux and geo) else ()
            rc = _call_raw_backward(lib, True, with_obj, ctx.holder, plan, gcol, gobj, d_m2,
                                    d_objv if plan.per_view else d_obj, P, device)
            if plan.per_view:
                plan.bucket.used = B
                if rc == 0 and d_objv is not None:
                    d_obj.copy_(d_objv[0])
                    for v in range(1, B):
                        d_obj.add_(d_objv[v])
        if rc != 0:
            raise _rc_error(lib, rc, invalid=RuntimeError)
        _cache_backward_leave(ctx, device)
        d_x, d_dc, d_rest, d_op, d_sc, d_ro = _autograd_attr_grads(plan)
        return (_shaped(d_x, s[0]), _shaped(d_m2, s[1]), _shaped(d_dc, s[2], need[2]), _shaped(d_rest, s[3], need[3]),
                _shaped(d_op, s[4]), _shaped(d_sc, s[5]), _shaped(d_ro, s[6]), _shaped(d_obj, s[7]), None)


def _wants_backward(*tensors) -> bool:
    """A forward keeps backward state only if autograd can reach it: grad mode on and an input that requires grad.
    Decided here, before Function.apply (inside forward() grad mode is off and needs_input_grad ignores no_grad())."""
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors)


def rasterize_gaussians_raw_batch(xyz, means2D, features_dc, features_rest, opacity, scaling, rotation, settings_list,
                                  grad_bucket: Optional["GradBucket"] = None, grad_norms: Optional["GradNorms"] = None,
                                  cache: Optional["RenderCache"] = None, cache_key=None, objects_dc=None, aux: bool = False):
    """(color[B,3,H,W], radii[B,P]) of B views (a list of GaussianRasterizationSettings that agree in image size, scale
    modifier and SH degree) of one set of RAW parameters, through one launch chain: every image and radius is bit for bit
    what rasterize_gaussians_raw gives for that view alone, and the backward leaves the SUM over the views of the
    attribute gradients, written once.  means2D: a [B,P,3] tensor whose .grad receives the per-view screen-space gradient
    (viewspace_points.grad of the reference, one slice per view), or None.
    objects_dc ([P,16] or [P,1,16] object features, or None = no object channels): -> (color, radii, objects[B,16,H,W]),
    every object map bit for bit rasterize_gaussians_raw's for that view; objects_dc.grad receives the single-view object
    gradients summed in view order (a GradBucket or GradBucketSet does not hold it).
    aux=True (not with objects_dc): -> (color, radii, depth[B,1,H,W], alpha[B,1,H,W]), both differentiable; every map bit for
    bit rasterize_gaussians_raw(..., aux=True)'s for that view; the render cache is bypassed."""
    # `cache` (a RenderCache) + `cache_key` (one per tuple of cameras): a batch whose geometry inputs and cameras are unchanged
    # since the key's last render re-uses that render's binning for all B views (gsr_ctx_rerender on the batch context)
    opts = _CallOpts(keep=_wants_backward(xyz, means2D, features_dc, features_rest, opacity, scaling, rotation, objects_dc),
                     aux=bool(aux), bucket=grad_bucket, norms=grad_norms,
                     cache_slot=(cache, cache_key) if cache is not None else None,
                     color_only=not _wants_backward(xyz, means2D, opacity, scaling, rotation),
                     settings_list=tuple(settings_list))
    return _RasterizeGaussiansRawBatch.apply(xyz, means2D, features_dc, features_rest, opacity, scaling, rotation, objects_dc,
                                             opts)


def rasterize_gaussians_raw(xyz, means2D, features_dc, features_rest, objects_dc, opacity, scaling, rotation,
                            raster_settings, grad_bucket: Optional["GradBucket"] = None, cache: Optional["RenderCache"] = None,
                            cache_key=None, grad_norms: Optional["GradNorms"] = None, aux: bool = False):
    """(color[3,H,W], radii[P], objects[16,H,W]) from the RAW parameters of a reference-style GaussianModel
    (_xyz, _features_dc, _features_rest, _objects_dc or None, _opacity, _scaling, _rotation): equal to the
    getters (scene/gaussian_model.py:97-124) followed by GaussianRasterizer.forward, in one fused pass.
    aux=True: -> (color, radii, objects, depth[1,H,W], alpha[1,H,W]) -- alpha = 1 - final transmittance, depth = sum of
    z_i alpha_i T_i (not divided by alpha; depth / alpha is the expected depth of the covered part) -- both differentiable
    w.r.t. xyz, opacity, scaling and rotation; the render cache is bypassed."""
    # `cache` (a RenderCache) + `cache_key` (one per camera): a render whose geometry inputs are unchanged since the key's
    # last render re-uses that render's binning (gsr_ctx_rerender)
    opts = _CallOpts(keep=_wants_backward(xyz, means2D, features_dc, features_rest, objects_dc, opacity, scaling, rotation),
                     aux=bool(aux), bucket=grad_bucket, norms=grad_norms,
                     cache_slot=(cache, cache_key) if cache is not None else None,
                     color_only=not _wants_backward(xyz, means2D, opacity, scaling, rotation))
    return _RasterizeGaussiansRaw.apply(xyz, means2D, features_dc, features_rest, objects_dc, opacity, scaling, rotation,
                                        raster_settings, opts)


@torch.no_grad()
def rasterize_gaussians_raw2(params_a, params_b, raster_settings, objects: bool = True,
                             cache: Optional["RenderCache"] = None, cache_key=None):
    """Forward-only render of two reference-style parameter sets as ONE scene -- `params_a` followed by `params_b`,
    each (xyz, features_dc, features_rest, objects_dc or None, opacity, scaling, rotation), RAW tensors -- without
    concatenating them (gsr_forward_raw2; reference attack.py:513-530 deep-copies the model and concatenates all seven
    tensors for this).  -> (color[3,H,W], radii[Pa+Pb], objects[16,H,W]); bitwise equal to rasterize_gaussians_raw on
    the concatenated tensors.  Not differentiable (the reference never calls backward on this render)."""
    lib = _load()
    device = _hip_device(params_a[0])
    a = [_prep(t, device) for t in params_a]
    b = [_prep(t, device) for t in params_b]
    Pa, Pb = int(params_a[0].shape[0]), int(params_b[0].shape[0])
    for P, params in ((Pa, params_a), (Pb, params_b)):
        if P:
            _check_sh_storage(P, params[1], params[2])
    with_obj = objects and (Pa == 0 or a[3] is not None) and (Pb == 0 or b[3] is not None)
    H, W = int(raster_settings.image_height), int(raster_settings.image_width)
    pack = _SettingsPack(raster_settings, device)
    color = torch.empty(3, H, W, dtype=torch.float32, device=device)
    objs = (torch.empty(NUM_OBJECTS, H, W, dtype=torch.float32, device=device) if with_obj
            else _zero_scalar(device).expand(NUM_OBJECTS, H, W))
    nren = ctypes.c_int64(0)
    if not with_obj:
        a[3] = b[3] = None
    # cache: with both models' geometry unchanged since the key's last render, only the colour kernel and the compositor
    # run (gsr_ctx_rerender on a context kept by gsr_forward_raw2_keep) -- the success re-render of a colour attack
    entry = sig = refs = b_sig = None
    if cache is not None and Pa > 0 and Pb > 0:
        geo = tuple(params_a[i] for i in (0, 4, 5, 6)) + tuple(params_b[i] for i in (0, 4, 5, 6)) + \
            ((params_a[3], params_b[3]) if with_obj else (None, None))
        used = (a[0], a[4], a[5], a[6], b[0], b[4], b[5], b[6], a[3], b[3])
        entry, sig, refs = _cache_probe(cache, cache_key, geo, used, [raster_settings], "pair", with_obj, False)
        b_sig = _coeff_sig(params_b[1], params_b[2], b[1], b[2])
    with torch.cuda.device(device):
        if entry is not None:
            radii = entry.pack.radii.detach()
            dc_b, rest_b, flags = _pair_rerender_args(entry.pack, b_sig, b[1], b[2])
            # the context reads the coefficient tensors of THIS call on the stream: they stay referenced until the next render
            entry.pack.last_inputs = (a, b, pack)
            rc, entry = _cache_rerender(lib, cache, cache_key, entry, device, a[1], a[2], dc_b, rest_b, pack.bg, color,
                                        objs if with_obj else None, flags)
        if entry is None:
            radii = torch.empty(Pa + Pb, dtype=torch.int32, device=device)
            handle = ctypes.c_void_p(None)
            rc = lib.gsr_forward_raw2_keep(ctypes.byref(pack.c), Pa, *[_ptr(t) for t in a], Pb, *[_ptr(t) for t in b],
                                           _ptr(color), _ptr(objs) if with_obj else None, _ptr(radii),
                                           ctypes.byref(handle) if sig is not None else None, ctypes.byref(nren), _stream(device))
            if rc == 0 and handle.value:
                pack.radii, pack.last_inputs, pack.b_sig = radii, (a, b), b_sig
                entry = _cache_store(cache, cache_key, _CtxHolder(lib, handle), sig, refs, pack, nren.value)
        if entry is not None and rc == 0:
            _cache_leave(entry, device)
    if rc != 0:
        raise _rc_error(lib, rc)
    return color, radii, objs


@torch.no_grad()
def rasterize_gaussians_raw2_batch(params_a, params_b, settings_list, cache: Optional["RenderCache"] = None, cache_key=None,
                                   objects_dc=None):
    """rasterize_gaussians_raw2 for a BATCH of views through one launch chain (gsr_forward_raw2_batch): the success renders
    of a batch of cameras (reference attack.py:513-530 renders the combined scene once per camera).  `params_*`: (xyz,
    features_dc, features_rest, opacity, scaling, rotation), RAW tensors, both non-empty.  -> (color[B,3,H,W],
    radii[B,Pa+Pb]); every image bit for bit rasterize_gaussians_raw2's for that view.  No object channels, not
    differentiable.  With a cache the batch's context is kept: while both models' geometry and the cameras are unchanged a
    render is the batch's colour kernel -- over the first model's Gaussians only while the second model's coefficient
    tensors are untouched -- and one compositor launch.
    objects_dc = (objects_dc_a [Pa,16], objects_dc_b [Pb,16]) (gsr_forward_raw2_batch_obj): -> (color, radii,
    objects[B,16,H,W]), every object map bit for bit rasterize_gaussians_raw2's for that view."""
    lib = _load()
    device = _hip_device(params_a[0])
    packs, carr = _view_packs(settings_list, device)
    B = len(packs)
    Pa, Pb = int(params_a[0].shape[0]), int(params_b[0].shape[0])
    if Pa == 0 or Pb == 0:
        raise ValueError("rasterize_gaussians_raw2_batch needs two non-empty models")
    a = [_prep(t, device) for t in params_a]
    b = [_prep(t, device) for t in params_b]
    _check_sh_storage(Pa, params_a[1], params_a[2])
    _check_sh_storage(Pb, params_b[1], params_b[2])
    with_obj = objects_dc is not None
    oa = ob = None
    if with_obj:
        oa, ob = (_f32c(t.detach(), device) for t in objects_dc)
        if oa.numel() != Pa * NUM_OBJECTS or ob.numel() != Pb * NUM_OBJECTS:
            raise ValueError(f"objects_dc must hold Pa*{NUM_OBJECTS} and Pb*{NUM_OBJECTS} values")
    H, W = int(settings_list[0].image_height), int(settings_list[0].image_width)
    color = torch.empty(B, 3, H, W, dtype=torch.float32, device=device)
    objs = torch.empty(B, NUM_OBJECTS, H, W, dtype=torch.float32, device=device) if with_obj else None
    nren = ctypes.c_int64(0)
    entry = sig = refs = None
    if cache is not None:
        geo = tuple(params_a[i] for i in (0, 3, 4, 5)) + tuple(params_b[i] for i in (0, 3, 4, 5))
        used = (a[0], a[3], a[4], a[5], b[0], b[3], b[4], b[5])
        if with_obj:                                # (the context reads the object features through the forward's pointers)
            geo, used = geo + tuple(objects_dc), used + (oa, ob)
        entry, sig, refs = _cache_probe(cache, cache_key, geo, used, settings_list, "pair-batch", with_obj, False)
    b_sig = _coeff_sig(params_b[1], params_b[2], b[1], b[2])
    with torch.cuda.device(device):
        if entry is not None:
            bp = entry.pack
            radii = bp.radii.detach()
            dc_b, rest_b, flags = _pair_rerender_args(bp, b_sig, b[1], b[2])
            bp.last_inputs = (a, b, packs, oa, ob)     # read on the stream: referenced until the next render
            rc, entry = _cache_rerender(lib, cache, cache_key, entry, device, a[1], a[2], dc_b, rest_b, bp.background(packs),
                                        color, objs, flags)
        if entry is None:
            radii = torch.empty(B, Pa + Pb, dtype=torch.int32, device=device)
            handle = ctypes.c_void_p(None)
            want_ctx = ctypes.byref(handle) if sig is not None else None
            if with_obj:
                rc = lib.gsr_forward_raw2_batch_obj(carr, B, Pa, *[_ptr(t) for t in a[:3]], _ptr(oa), *[_ptr(t) for t in a[3:]],
                                                    Pb, *[_ptr(t) for t in b[:3]], _ptr(ob), *[_ptr(t) for t in b[3:]],
                                                    _ptr(color), _ptr(objs), _ptr(radii), want_ctx, ctypes.byref(nren),
                                                    _stream(device))
            else:
                rc = lib.gsr_forward_raw2_batch(carr, B, Pa, *[_ptr(t) for t in a], Pb, *[_ptr(t) for t in b], _ptr(color),
                                                _ptr(radii), want_ctx, ctypes.byref(nren), _stream(device))
            if rc == 0 and handle.value:
                bp = _BatchPack(packs, radii)
                bp.b_sig, bp.last_inputs = b_sig, (a, b, packs, oa, ob)
                entry = _cache_store(cache, cache_key, _CtxHolder(lib, handle), sig, refs, bp, nren.value)
        if entry is not None and rc == 0:
            _cache_leave(entry, device)
    if rc != 0:
        raise _rc_error(lib, rc)
    if with_obj:
        return color, radii, objs
    return color, radii


def rasterize_gaussians(means3D, means2D, sh, sh_objs, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                        raster_settings, aux: bool = False):
    keep = _wants_backward(means3D, means2D, sh, sh_objs, colors_precomp, opacities, scales, rotations, cov3Ds_precomp)
    return _RasterizeGaussians.apply(means3D, means2D, sh, sh_objs, colors_precomp, opacities, scales, rotations,
                                     cov3Ds_precomp, raster_settings, _CallOpts(keep=keep, aux=bool(aux)))


class GaussianRasterizer(nn.Module):
    def __init__(self, raster_settings: GaussianRasterizationSettings):
        super().__init__()
        self.raster_settings = raster_settings

    def markVisible(self, positions: torch.Tensor) -> torch.Tensor:
        """Frustum test (view-space z > 0.2) -> bool[P]."""
        lib = _load()
        if not positions.is_cuda:
            raise RuntimeError("diff_gaussian_rasterization: positions must live on a HIP device; there is no CPU path")
        with torch.no_grad():
            device = positions.device
            pos = _f32c(positions, device)
            pack = _SettingsPack(self.raster_settings, device)
            present = torch.empty(pos.shape[0], dtype=torch.uint8, device=device)
            with torch.cuda.device(device):
                rc = lib.gsr_mark_visible(ctypes.byref(pack.c), int(pos.shape[0]), _ptr(pos), _ptr(present), _stream(device))
            if rc != 0:
                raise RuntimeError(_err(lib))
            return present.bool()

    def forward(self, means3D, means2D, opacities, shs=None, sh_objs=None, colors_precomp=None, scales=None,
                rotations=None, cov3D_precomp=None, aux=False):
        """-> (color[3,H,W], radii[P], objects[16,H,W]); with aux=True -> (color, radii, objects, depth[1,H,W], alpha[1,H,W]):
        alpha = 1 - final transmittance, depth = sum of z_i alpha_i T_i over the blended splats (view depth z_i; not divided
        by alpha, no background term), both differentiable w.r.t. means, opacities, scales and rotations / cov3D."""
        if (shs is None and colors_precomp is None) or (shs is not None and colors_precomp is not None):
            raise Exception('Please provide excatly one of either SHs or precomputed colors!')
        if ((scales is None or rotations is None) and cov3D_precomp is None) or \
                ((scales is not None or rotations is not None) and cov3D_precomp is not None):
            raise Exception('Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!')
        return rasterize_gaussians(means3D, means2D, shs, sh_objs, colors_precomp, opacities, scales, rotations,
                                   cov3D_precomp, self.raster_settings, aux)


# ---- introspection used by the benchmark / tests -----------------------------------------------------------
def last_num_rendered(output: torch.Tensor) -> int:
    """Number of (tile, Gaussian) pairs of the forward that produced `output` (its grad_fn's context).  An
    asynchronous-count forward (FLAG_ASYNC_COUNT) learns it here, from the context (waits for the early device copy)."""
    fn = output.grad_fn
    if fn is None:
        return -1
    n = int(getattr(fn, "_nren", -1))
    if n < 0 and getattr(fn, "holder", None) is not None:
        n = fn.holder.info(0)
    return n


_EXPORTS = {"ranges": (0, torch.int32), "pair_rank": (1, torch.int32), "n_contrib": (2, torch.int32),
            "final_T": (3, torch.float32), "order": (4, torch.int32), "off": (5, torch.int32),
            "R": (7, torch.float32), "G": (7, torch.float32), "dv": (8, torch.int32), "offg": (9, torch.int32)}


def export_state(output: torch.Tensor, name: str) -> torch.Tensor:
    """Copy one internal array of the forward that produced `output` (tests / diagnostics only)."""
    fn = output.grad_fn
    holder = fn.holder
    what, dt = _EXPORTS[name]
    P = int(fn.kept[0].shape[0])
    H, W = fn.pack.c.image_height, fn.pack.c.image_width
    T = ((W + 15) // 16) * ((H + 15) // 16)
    nb = max(holder.info(4), 1)                      # a batch context: B views as one virtual scene of B * Ppad Gaussians
    if nb > 1:
        P, T, H = nb * holder.info(5), nb * T, nb * H
    n = {"ranges": 2 * T, "pair_rank": holder.info(0), "n_contrib": H * W, "final_T": H * W, "order": P,
         "off": P + 1, "R": 12 * P, "G": 12 * P, "dv": 16, "offg": P + 1}[name]
    live = None
    if name in ("order", "off") and P > 0:
        # only the Gaussians that emit pairs are ranked: dv[1] = V of them (order[:V], off[:V + 1] are meaningful)
        live = int(export_state(output, "dv")[1].item()) + (1 if name == "off" else 0)
    dst = torch.empty(max(n, 1), dtype=dt, device=output.device)
    if holder.lib.gsr_ctx_export(holder.handle, what, dst.data_ptr(), dst.numel() * 4, _stream(output.device)) != 0:
        raise RuntimeError(_err(holder.lib))
    return dst[:n if live is None else live]


def profile(enable, stages=None) -> None:
    """Start (and reset) / stop the library's per-stage HIP-event timing.  `stages`: iterable of names from
    GSR_STAGES to time only those (each timed stage costs two event records per call)."""
    if not enable:
        mask = 0
    elif stages is None:
        mask = (1 << len(GSR_STAGES)) - 1
    else:
        mask = sum(1 << GSR_STAGES.index(s) for s in stages)
    _load().gsr_profile(mask)


def profile_read() -> dict:
    lib = _load()
    ms = (ctypes.c_float * len(GSR_STAGES))()
    calls = (ctypes.c_int64 * len(GSR_STAGES))()
    if lib.gsr_profile_read(ms, calls) != 0:
        raise RuntimeError(_err(lib))
    return {n: (float(ms[i]), int(calls[i])) for i, n in enumerate(GSR_STAGES)}


def pool_bytes() -> int:
    out = ctypes.c_int64(0)
    _load().gsr_query(1, ctypes.byref(out))
    return out.value


def trim_pool() -> None:
    _load().gsr_trim_pool()


__all__ = ["GaussianRasterizationSettings", "GaussianRasterizer", "rasterize_gaussians", "rasterize_gaussians_raw",
           "rasterize_gaussians_raw2", "rasterize_gaussians_raw_batch", "MAX_BATCH", "GradBucketSet", "PairCapacityExceeded", "GradBucket", "GradNorms",
           "NUM_OBJECTS",
           "library_path", "profile", "profile_read", "pool_bytes", "trim_pool", "last_num_rendered", "export_state"]


def _auto_patch_reference():
    """GSR_PATCH_REFERENCE=1 in the environment: the reference's ``gaussian_renderer.render`` becomes this package's fused
    ``gsplat_attack.renderer.render`` WITHOUT a line of the reference being edited and without a call to
    ``gsplat_attack.patch_reference()``.  The module object of ``gaussian_renderer`` is given a subclass of
    ``types.ModuleType`` whose attribute lookup answers ``render`` with the fused function once the reference has defined
    its own -- so ``from gaussian_renderer import render`` (reference attack.py:20) and ``gaussian_renderer.render`` both
    bind the fused one.  Two ways in, whichever comes first: the reference imports this package from INSIDE
    ``gaussian_renderer/__init__.py`` (line 14), while that module is still being executed -- it is then in sys.modules
    already and is re-classed on the spot; or this package was imported earlier (``scene/gaussian_model.py:17`` imports
    ``simple_knn._C``, which loads the same library) -- then a meta-path finder re-classes ``gaussian_renderer`` right after
    its own import has run.  Same signature, same returned dict (tests/test_golden_glue.py pins the fused function against
    the EXECUTED reference one); the raw parameters go straight into the kernels: no activated copies, no 192 MB ``cat`` per
    view, no PyTorch backward of the getters.  GSR_PATCH_MODULE names another module than ``gaussian_renderer``.  Off by
    default: an installed package does not rebind a caller's functions unasked."""
    if os.environ.get("GSR_PATCH_REFERENCE", "0") in ("", "0"):
        return None
    import importlib.abc
    import importlib.util
    import sys
    import types
    want = os.environ.get("GSR_PATCH_MODULE", "gaussian_renderer")

    class _FusedRenderModule(types.ModuleType):
        def __getattribute__(self, name):
            if name == "render" and "render" in types.ModuleType.__getattribute__(self, "__dict__"):
                from gsplat_attack.renderer import render as fused
                return fused
            return types.ModuleType.__getattribute__(self, name)

    def reclass(module):
        try:
            if isinstance(module, types.ModuleType) and type(module) is not _FusedRenderModule:
                module.__class__ = _FusedRenderModule
        except TypeError:
            pass

    if want in sys.modules:                    # being imported right now (or imported already): re-class it on the spot
        reclass(sys.modules[want])
        return "reclassed"

    class _Finder(importlib.abc.MetaPathFinder):
        busy = False

        def find_spec(self, fullname, path, target=None):
            if fullname != want or _Finder.busy:
                return None
            _Finder.busy = True
            try:
                spec = importlib.util.find_spec(fullname)
            finally:
                _Finder.busy = False
            if spec is None or spec.loader is None:
                return None
            inner = spec.loader

            class _Loader(importlib.abc.Loader):
                def create_module(self, spec_):
                    return inner.create_module(spec_)

                def exec_module(self, module):
                    inner.exec_module(module)
                    reclass(module)
            spec.loader = _Loader()
            return spec

    sys.meta_path.insert(0, _Finder())
    return "finder"


_auto_patch_reference()
