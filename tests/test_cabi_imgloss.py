"""The fused image losses' C ABI and Python surface, the parts that need no GPU: both symbols and their signatures, the
struct layout, every argument check (refused before any device call: the pointers handed over are never followed), the
capability items left as they were, and what the Python layer refuses (CPU tensors, window sizes, a reference that requires
grad)."""
import ctypes

import pytest
import torch

from diff_gaussian_rasterization import _signatures as SG
from diff_gaussian_rasterization import imgloss_ops as IL
from gsplat_attack import image_loss as GL

INVALID = 1
FAKE = 0x1000          # a non-null, 16-byte aligned pointer that is never followed: every call below is refused first
NAN, INF = float("nan"), float("inf")
BIG = 1 << 40


@pytest.fixture(scope="module")
def lib():
    return IL._lib()


def _spec(**kw):
    cs = IL.c_spec(IL.ImgLossSpec(0.8, 0.0, 0.2), (2, 3, 37, 45))
    for k, v in kw.items():
        setattr(cs, k, v)
    return cs


def _ref(cs):
    return ctypes.byref(cs) if cs is not None else None


def _call(lib, cs, img=FAKE, ref=FAKE, ws=FAKE, ws_bytes=BIG, terms=FAKE, grad=FAKE, smap=FAKE):
    return lib.gsr_imgloss(_ref(cs), img, ref, ws, ws_bytes, terms, grad, smap, None)


def _bytes(lib, cs):
    n = ctypes.c_int64(-1)
    return lib.gsr_imgloss_workspace_bytes(_ref(cs), ctypes.byref(n)), n.value


def test_symbols_signatures_layout_and_capability(lib):
    assert IL.available()
    for name, n in (("gsr_imgloss_workspace_bytes", 2), ("gsr_imgloss", 9)):
        assert hasattr(lib, name) and list(getattr(lib, name).argtypes) == list(SG.SIGNATURES[name][1]) and len(SG.SIGNATURES[name][1]) == n
        assert getattr(lib, name).restype is SG.SIGNATURES[name][0] is ctypes.c_int
    assert SG.SIGNATURES["gsr_imgloss"][1][4] is ctypes.c_int64                  # ws_bytes
    out = ctypes.c_int64(0)
    assert lib.gsr_query(0, ctypes.byref(out)) == 0 and out.value == 604       # no new version, bit or item
    assert lib.gsr_query(5, ctypes.byref(out)) == 0 and out.value == 63
    assert lib.gsr_query(6, ctypes.byref(out)) == INVALID
    names = [f[0] for f in IL._CImgLossSpec._fields_]
    assert names == ["B", "C", "H", "W", "w_l1", "w_l2", "w_ssim", "flags"]
    assert ctypes.sizeof(IL._CImgLossSpec) == 32
    assert [getattr(IL._CImgLossSpec, n).offset for n in names] == [0, 4, 8, 12, 16, 20, 24, 28]
    assert IL.ImgLossSpec() == (0.0, 0.0, 1.0, False) and (IL.CLAMP01, IL.NO_GRAD, IL.MAX_CHANNELS) == (1, 2, 4)
    assert len(IL.TILE) == 2


BAD = [dict(B=0), dict(B=-1), dict(C=0), dict(C=5), dict(H=0), dict(W=0), dict(W=-3),
       dict(B=1 << 15, C=4, H=128, W=128),                         # B C H W = 2^31
       dict(B=1, C=1, H=46341, W=46341),                           # 46341^2 > 2^31 - 1
       dict(B=2147483647, C=4, H=2147483647, W=2147483647),        # every product overflows 64 bits' lower half
       dict(w_l1=NAN), dict(w_l2=INF), dict(w_ssim=-INF), dict(flags=4), dict(flags=0x80000001)]


def test_spec_checks(lib):
    for bad in BAD:
        assert _call(lib, _spec(**bad)) == INVALID, bad
        assert b"gsr_imgloss:" in lib.gsr_last_error(), bad
        rc, _ = _bytes(lib, _spec(**bad))
        assert rc == INVALID and b"gsr_imgloss_workspace_bytes:" in lib.gsr_last_error(), bad
    assert _call(lib, None) == INVALID and b"null spec" in lib.gsr_last_error()
    assert lib.gsr_imgloss_workspace_bytes(None, ctypes.byref(ctypes.c_int64())) == INVALID and b"null spec" in lib.gsr_last_error()
    assert lib.gsr_imgloss_workspace_bytes(_ref(_spec()), None) == INVALID and b"null bytes" in lib.gsr_last_error()


def test_workspace_bytes_and_pointer_checks(lib):
    cs = _spec()
    rc, full = _bytes(lib, cs)
    rc2, small = _bytes(lib, _spec(flags=IL.NO_GRAD))
    th, tw = IL.TILE
    tiles = 2 * 3 * (-(-37 // th)) * (-(-45 // tw))
    assert rc == 0 and rc2 == 0 and small >= 12 * tiles and full >= small + 12 * 2 * 3 * 37 * 45 and full % 16 == 0 and small % 16 == 0
    assert _bytes(lib, _spec(flags=IL.CLAMP01))[1] == full and _bytes(lib, _spec(flags=IL.CLAMP01 | IL.NO_GRAD))[1] == small
    for n in ("img", "ref", "ws", "terms"):
        assert _call(lib, cs, **{n: None}) == INVALID and b"null" in lib.gsr_last_error(), n
    for n in ("img", "ref", "terms", "grad", "smap"):
        assert _call(lib, cs, **{n: FAKE + 2}) == INVALID and b"4-byte aligned" in lib.gsr_last_error(), n
    assert _call(lib, cs, ws_bytes=full - 1) == INVALID and b"workspace of" in lib.gsr_last_error()
    assert _call(lib, cs, ws_bytes=0) == INVALID and _call(lib, cs, ws_bytes=-5) == INVALID
    assert _call(lib, cs, grad=None, ws_bytes=small - 1) == INVALID and b"workspace of" in lib.gsr_last_error()
    for off in (4, 8, 12):
        assert _call(lib, cs, ws=FAKE + off) == INVALID and b"16-byte aligned" in lib.gsr_last_error(), off
    assert _call(lib, _spec(flags=IL.NO_GRAD)) == INVALID and b"GSR_IMGLOSS_NO_GRAD" in lib.gsr_last_error()      # grad given
    # (a call that passes every check is never made with the fake pointers)


def test_python_layer_refuses_without_a_device():
    x, y = torch.rand(1, 3, 12, 13), torch.rand(1, 3, 12, 13)
    with pytest.raises(RuntimeError, match="no CPU path"):
        IL.image_loss(x, y, 1.0, 0.0, 0.0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        IL.imgloss_forward(x, y, IL.ImgLossSpec())
    for fn in (GL.l1_loss, GL.l2_loss, GL.ssim, GL.psnr, GL.photometric_loss, GL.ImageLoss()):
        with pytest.raises(RuntimeError, match="no CPU path"):
            fn(x, y)
    with pytest.raises(ValueError, match="window_size"):
        GL.ssim(x, y, window_size=7)
    with pytest.raises(ValueError, match="must not require grad"):
        IL.image_loss(x, y.clone().requires_grad_(True), 0.0, 0.0, 1.0)
    with pytest.raises(ValueError, match="must not require grad"):
        GL.ssim(x, y.clone().requires_grad_(True))
    for bad in (dict(w_l1=NAN), dict(w_ssim=INF)):
        with pytest.raises(ValueError):
            GL.ImageLoss(**bad)
    with pytest.raises(ValueError):
        GL.with_image_term(lambda r: r.sum(), torch.zeros(3, 4, 5), GL.ImageLoss(), 1.0)
    import gsplat_attack
    for n in ("l1_loss", "l2_loss", "ssim", "psnr", "ImageLoss", "photometric_loss", "with_image_term"):
        assert getattr(gsplat_attack, n) is getattr(GL, n)


def test_with_image_term_plumbing_on_the_cpu():
    """weight == 0 calls the inner loss alone (no device needed), and the view indices go on iff the inner loss takes them."""
    seen = []

    def inner(r, idx=None):
        seen.append(idx)
        return r.sum()
    inner.takes_view_index = True
    refs = torch.zeros(4, 3, 5, 6)
    f = GL.with_image_term(inner, refs, GL.ImageLoss(), 0.0)
    assert f.takes_view_index is True
    r = torch.ones(2, 3, 5, 6)
    assert f(r, idx=[3, 1]).item() == r.sum().item() and seen == [[3, 1]]
    plain = GL.with_image_term(lambda t: t.mean(), refs, GL.ImageLoss(), 0.0)
    assert plain(r, idx=[0, 2]).item() == 1.0
    with pytest.raises(RuntimeError, match="no CPU path"):
        GL.with_image_term(lambda t: t.mean(), refs, GL.ImageLoss(), 0.5)(r, idx=[0, 2])
