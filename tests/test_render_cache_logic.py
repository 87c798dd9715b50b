"""RenderCache bookkeeping without a device: what is a hit, what is a miss, what is left alone (the GPU side -- that a hit
renders the same bits -- is tests/test_gpu_rerender.py)."""
import gc
import weakref

import torch


def _entry(D, sig, tensors):
    return D._CacheEntry(object(), sig, tuple(weakref.ref(t) for t in tensors), object(), 123)


def test_hit_needs_the_same_signature_and_the_same_tensor_objects():
    import diff_gaussian_rasterization as D
    cache = D.RenderCache(max_entries=2)
    a, b = torch.zeros(4, 3), torch.zeros(4)
    e = _entry(D, ("sig", 1), (a, b))
    cache._store("k", e)
    assert cache._lookup("k", ("sig", 1), (a, b)) == (e, True) and cache.hits == 1
    assert cache._lookup("k", ("sig", 2), (a, b)) == (None, True)                 # another signature
    assert cache._lookup("other", ("sig", 1), (a, b)) == (None, True)             # another key
    a2 = torch.zeros(4, 3)                                                         # an equal tensor is not THE tensor
    assert cache._lookup("k", ("sig", 1), (a2, b)) == (None, True)
    assert cache.misses == 3
    del a
    gc.collect()                                                                   # a dead tensor can never match again
    a3 = torch.zeros(4, 3)
    assert cache._lookup("k", ("sig", 1), (a3, b)) == (None, True)


def test_signature_follows_versions_shapes_and_settings():
    import diff_gaussian_rasterization as D
    x = torch.zeros(5, 3)
    cam = [torch.eye(4), torch.eye(4), torch.zeros(3)]
    rs = D.GaussianRasterizationSettings(64, 96, 0.5, 0.4, torch.zeros(3), 1.0, cam[0], cam[1], 3, cam[2], False, False)
    s0 = D._cache_sig((x, None), rs)
    assert s0 == D._cache_sig((x, None), rs)
    x.add_(1.0)                                                                    # in place: the version moves
    assert D._cache_sig((x, None), rs) != s0
    s1 = D._cache_sig((x, None), rs)
    cam[0].mul_(2.0)                                                               # the camera edited in place
    assert D._cache_sig((x, None), rs) != s1
    s2 = D._cache_sig((x, None), rs)
    assert D._cache_sig((x, None), rs._replace(scale_modifier=1.5)) != s2
    assert D._cache_sig((x, None), rs._replace(sh_degree=2)) != s2
    assert D._cache_sig((x, None), rs._replace(image_width=97)) != s2
    assert D._cache_sig((x, None), rs._replace(bg=torch.ones(3))) == s2            # the background is read per render
    assert D._cache_sig((x, None), rs, extra=("pair", True)) != s2


def _views(n):
    import diff_gaussian_rasterization as D
    cams = [[torch.eye(4), torch.eye(4), torch.zeros(3)] for _ in range(n)]
    views = [D.GaussianRasterizationSettings(64, 96, 0.5, 0.4, torch.zeros(3), 1.0, c[0], c[1], 3, c[2], False, False)
             for c in cams]
    return cams, views


def test_multi_view_signature_follows_every_view():
    import diff_gaussian_rasterization as D
    x = torch.zeros(5, 3)
    cams, views = _views(3)
    s0, refs = D._views_sig((x, None), views, "batch", False)
    assert s0 == D._views_sig((x, None), views, "batch", False)[0]
    # identity is checked on the geometry and on EVERY view's camera tensors
    assert len(refs) == 2 + 3 * 3 and refs[0] is x and refs[1] is None
    assert all(any(r is t for r in refs) for c in cams for t in c)
    assert D._views_sig((x, None), views[:2], "batch", False)[0] != s0              # another B
    assert D._views_sig((x, None), views[:2], "batch", False)[0] != D._views_sig((x, None), views[:1], "batch", False)[0]
    assert D._views_sig((x, None), views, "batch", True)[0] != s0                   # the object flag
    assert D._views_sig((x, None), views[:2] + [views[2]._replace(tanfovx=0.6)], "batch", False)[0] != s0
    cams[2][0].mul_(2.0)                                                           # a LATER view's camera edited in place
    assert D._views_sig((x, None), views, "batch", False)[0] != s0
    s1 = D._views_sig((x, None), views, "batch", False)[0]
    cams[1][2].add_(1.0)
    assert D._views_sig((x, None), views, "batch", False)[0] != s1


def test_pair_signatures_differ_from_the_plain_ones():
    """One key never re-renders a context of another kind: the same tensors and cameras give four different signatures."""
    import diff_gaussian_rasterization as D
    x = torch.zeros(5, 3)
    _, views = _views(2)
    one = [D._views_sig((x,), views[:1], kind, False)[0] for kind in ("view", "pair")]
    many = [D._views_sig((x,), views, kind, False)[0] for kind in ("batch", "pair-batch")]
    assert len(set(one + many)) == 4
    assert D._views_sig((x,), views[:1], "batch", False)[0] != one[0]              # a batch of one view is still a batch


def test_probe_needs_dense_inputs_and_leaves_a_busy_entry_alone():
    import diff_gaussian_rasterization as D
    cache = D.RenderCache()
    x = torch.zeros(5, 3)
    _, views = _views(1)
    # the library was handed a temporary copy: no lookup, nothing to store
    assert D._cache_probe(cache, "k", (x, None), (x.clone(), None), views, "view", False, True) == (None, None, None)
    assert cache.misses == 0
    entry, sig, refs = D._cache_probe(cache, "k", (x, None), (x, None), views, "view", False, True)
    assert entry is None and sig == D._views_sig((x, None), views, "view", False)[0] and cache.misses == 1
    e = D._cache_store(cache, "k", object(), sig, refs, object(), 5)
    assert D._cache_probe(cache, "k", (x, None), (x, None), views, "view", False, True) == (e, sig, refs)
    token = D._RenderToken()
    e.token = weakref.ref(token)                                                   # waiting for its backward
    assert D._cache_probe(cache, "k", (x, None), (x, None), views, "view", False, True) == (None, None, refs)
    assert D._cache_probe(cache, "k", (x, None), (x, None), views, "view", False, False) == (None, sig, refs)
    assert cache.bypassed == 2


def test_second_model_coefficients_unchanged_logic():
    """A pair context's re-render covers the first model only (flag 2) while the second model's coefficient tensors are
    the dense ones of the entry's last render at the same versions."""
    import diff_gaussian_rasterization as D

    class Kept:
        b_sig = None
    dc, rest = torch.zeros(4, 1, 3), torch.zeros(4, 15, 3)
    sig = D._coeff_sig(dc, rest, dc, rest)
    assert sig is not None and D._coeff_sig(dc, rest, dc.clone(), rest) is None    # a temporary copy says nothing
    kept = Kept()
    assert D._pair_rerender_args(kept, sig, dc, rest) == (dc, rest, 1) and kept.b_sig == sig
    assert D._pair_rerender_args(kept, sig, dc, rest) == (None, None, 3)
    rest.add_(1.0)                                                                 # stepped in place: handed over again
    sig2 = D._coeff_sig(dc, rest, dc, rest)
    assert sig2 != sig and D._pair_rerender_args(kept, sig2, dc, rest) == (dc, rest, 1)
    assert D._pair_rerender_args(kept, None, dc, rest) == (dc, rest, 1) and kept.b_sig is None
    assert D._pair_rerender_args(kept, None, dc, rest) == (dc, rest, 1)            # None never counts as "the same"


def test_an_entry_waiting_for_its_backward_is_bypassed_and_lru_evicts():
    import diff_gaussian_rasterization as D
    cache = D.RenderCache(max_entries=2)
    t = torch.zeros(2)
    e = _entry(D, "s", (t,))
    cache._store("k", e)
    token = D._RenderToken()
    e.token = weakref.ref(token)
    assert e.busy()
    assert cache._lookup("k", "s", (t,)) == (None, False) and cache.bypassed == 1   # neither used nor replaced
    token.done = True                                                               # its backward ran
    assert not e.busy() and cache._lookup("k", "s", (t,)) == (e, True)
    e.token = weakref.ref(D._RenderToken())                                         # the graph died without a backward
    gc.collect()
    assert not e.busy()
    cache._store("k2", _entry(D, "s", (t,)))
    cache._lookup("k", "s", (t,))                                                   # k is now the most recently used
    cache._store("k3", _entry(D, "s", (t,)))
    assert list(cache.entries) == ["k", "k3"]                                       # k2 went


def test_zero_object_cache_serves_only_the_tensor_it_was_made_for(monkeypatch):
    """_objects_all_zero on CPU tensors: an entry left by a dead all-zero tensor, planted under a live non-zero tensor's
    address with its size and version (what the allocator produces when it hands the block on), is not served; a temporary
    copy (another address than the caller's tensor) is never cached; the live tensor's own entries still are."""
    import diff_gaussian_rasterization as D
    monkeypatch.setattr(D, "_OBJ_SHORTCUT", True)
    D._OBJ_ZERO.clear()
    a = torch.zeros(10, 16)
    assert D._objects_all_zero(a, a) is True
    entry = D._OBJ_ZERO[a.data_ptr()]
    assert entry[:3] == (160, a._version, True)
    del a
    gc.collect()
    b = torch.ones(10, 16)
    assert b._version == entry[1]
    D._OBJ_ZERO[b.data_ptr()] = entry
    assert D._objects_all_zero(b, b) is False, "a dead tensor's entry was served to the tensor that got its address"
    assert D._OBJ_ZERO[b.data_ptr()][2] is False                                   # ... and replaced by b's own
    z = torch.zeros(10, 16)
    assert D._objects_all_zero(z, z) is True and D._objects_all_zero(z, z) is True
    z.add_(1.0)                                                                    # a zero tensor is re-checked when its version moves
    assert D._objects_all_zero(z, z) is False
    # a dense float32 temporary made from a float16 / strided source: no shortcut, nothing cached under its address
    D._OBJ_ZERO.clear()
    half = torch.zeros(10, 16, dtype=torch.float16)
    tmp = half.float()
    assert D._objects_all_zero(tmp, half) is False and not D._OBJ_ZERO
