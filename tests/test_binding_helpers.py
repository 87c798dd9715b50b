"""The shared host-side steps of the Python rasteriser binding that need no device: which C entry point a raw backward
calls, and where it writes the six attribute gradients.

Where the shared steps are reached ON a device, per caller (every test named asserts bit equality with the uncached or
single-view path):
  _prep / _hip_device / _check_sh_storage / _stream / _rc_error
                        every GPU test; the CPU refusals are test_cabi.py and test_aux_cpu.py
  _view_packs           batch: test_gpu_batch.py; pair batch: test_gpu_batch_rerender.py::test_pair_batch_equals_...
  _cache_probe, _cache_rerender, _cache_store, _cache_leave
      single view       test_gpu_rerender.py::test_rerender_is_bit_equal_to_a_fresh_forward, ::test_changed_geometry_...,
                        ::test_a_key_waiting_for_its_backward_is_left_alone; test_gpu_zero_objects.py::..._kept_context
      batch             test_gpu_batch_rerender.py::test_batch_rerender_is_bit_equal_to_a_fresh_batch,
                        ::test_a_batch_key_waiting_...; test_gpu_batch_objects.py::test_kept_batch_context_rerenders_objects
      pair              test_gpu_rerender.py::test_cached_pair_render_equals_the_uncached_one
      pair batch        test_gpu_batch_rerender.py::test_pair_batch_equals_the_per_camera_pair_renders,
                        test_gpu_batch_objects.py::test_pair_batch_objects_equal_render_pair
    the overflow drop   test_gpu_rerender.py::test_overflowed_async_forward_... (single view), ::test_overflowed_async_batch_...
                        (batch); the two pair callers reach it on no device (test_render_cache_logic.py covers their logic)
  _BatchPack.background batch: test_gpu_batch_rerender.py::test_backgrounds_cameras_and_geometry_behind_a_batch_key;
                        pair batch: the attack's success renders, ::test_attack_with_batched_success_renders_...
  _coeff_sig, _pair_rerender_args
                        pair: test_cached_pair_render_...; pair batch: test_pair_batch_equals_... (steps the second model too)
  _plan_attr_grads, _call_raw_backward, _chunk_trampoline, _autograd_attr_grads
                        test_gpu_backward_modes.py (every mode of both backwards), test_gpu_buckets.py, test_gpu_batch.py,
                        test_gpu_batch_objects.py::test_per_view_object_gradients, test_gpu_dist.py (chunks + hook)
  _arm_norms            strict (single view): test_gpu_buckets.py::test_backward_leaves_the_sums_of_squares_...,
                        ::test_colour_attack_with_fused_norms_...; lenient (batch): the batched L2 attacks (fused_norms is their
                        default), test_gpu_batch.py::test_pgd_attack_batched_..., test_gpu_batch_rerender.py::test_batched_colour_attack_...
  _cache_backward_enter / _cache_backward_leave
                        test_gpu_rerender.py::test_a_key_waiting_..., test_gpu_batch_rerender.py::test_a_batch_key_waiting_...
  _CallOpts             every render; aux: test_gpu_aux.py
"""
import itertools

import pytest
import torch

P = 7


def test_backward_pick_table_covers_every_reachable_mode_and_nothing_else():
    import diff_gaussian_rasterization as D
    from diff_gaussian_rasterization._signatures import SIGNATURES
    reachable = set()
    for batch, per_view, obj, chunked, into in itertools.product((False, True), repeat=5):
        if per_view and not (batch and into and not chunked):
            continue            # a GradBucketSet is a batch's bucket, written whole
        if chunked and not into:
            continue            # chunks are a GradBucket's request
        reachable.add((batch, per_view, obj, chunked, into))
    assert set(D._BWD_PICK) == reachable
    for (batch, per_view, obj, chunked, into), (name, obj_args, tail) in D._BWD_PICK.items():
        want = ("gsr_backward_raw_chunked" if chunked else
                "gsr_backward_raw_batch" + ("_obj" if obj else "") + ("_views" if per_view else "_into") if batch else
                "gsr_backward_raw_into" if into else "gsr_backward_raw")
        assert name == want
        # the call passes handle + grad_color + 8 pointers, grad_objects and dobjects_dc besides when the entry point takes
        # them, then the tail and the stream: that must be the declared parameter count
        n_tail = {"": 0, "accumulate": 1, "view_stride": 1, "chunks": 4}[tail]
        assert len(SIGNATURES[name][1]) == 9 + (2 if obj_args else 0) + n_tail + 1
    assert {v[0] for v in D._BWD_PICK.values()} == {
        "gsr_backward_raw", "gsr_backward_raw_into", "gsr_backward_raw_chunked", "gsr_backward_raw_batch_into",
        "gsr_backward_raw_batch_obj_into", "gsr_backward_raw_batch_views", "gsr_backward_raw_batch_obj_views"}


def test_planner_carves_one_flat_buffer_when_everything_is_wanted():
    import diff_gaussian_rasterization as D
    plan = D._plan_attr_grads((True,) * 5, P, torch.device("cpu"))
    assert plan.bucket is None and not plan.per_view and not plan.chunked and plan.overwrites
    base = plan.bufs[0].untyped_storage().data_ptr()
    assert plan.bufs[0].untyped_storage().nbytes() == 59 * P * 4
    for buf, c0, c1 in zip(plan.bufs, D.GradBucket.CUTS[:-1], D.GradBucket.CUTS[1:]):
        assert buf.untyped_storage().data_ptr() == base
        assert buf.storage_offset() == c0 * P and buf.numel() == (c1 - c0) * P and buf.dtype == torch.float32


def test_planner_hands_out_the_buckets_slices():
    import diff_gaussian_rasterization as D
    dev = torch.device("cpu")
    bucket = D.GradBucket(P, dev)
    plan = D._plan_attr_grads((True,) * 5, P, dev, bucket)
    assert plan.bucket is bucket and not plan.per_view and not plan.chunked and plan.overwrites
    for buf, sl in zip(plan.bufs, bucket.slices()):
        assert buf.data_ptr() == sl.data_ptr() and buf.shape == sl.shape
    bucket.fresh = False                                    # a later backward adds: not one summed gradient any more
    assert not D._plan_attr_grads((True,) * 5, P, dev, bucket).overwrites
    bucket.reset()
    bucket.chunks = 3
    plan = D._plan_attr_grads((True,) * 5, P, dev, bucket)
    assert plan.chunked and not plan.overwrites
    bset = D.GradBucketSet(2, P, dev)
    plan = D._plan_attr_grads((True,) * 5, P, dev, bset, B=2)
    assert plan.bucket is bset and plan.per_view and not plan.chunked and not plan.overwrites
    for buf, sl in zip(plan.bufs, bset.bucket(0).slices()):
        assert buf.data_ptr() == sl.data_ptr() and buf.shape == sl.shape


def test_planner_refuses_a_bucket_of_another_size():
    import diff_gaussian_rasterization as D
    dev = torch.device("cpu")
    with pytest.raises(ValueError, match=r"grad bucket does not match the model \(P or device\)"):
        D._plan_attr_grads((True,) * 5, P, dev, D.GradBucket(P + 1, dev))
    with pytest.raises(ValueError, match=r"grad bucket set does not match the batch \(views, P or device\)"):
        D._plan_attr_grads((True,) * 5, P, dev, D.GradBucketSet(2, P + 1, dev), B=2)
    with pytest.raises(ValueError, match=r"grad bucket set does not match the batch \(views, P or device\)"):
        D._plan_attr_grads((True,) * 5, P, dev, D.GradBucketSet(2, P, dev), B=3)


@pytest.mark.parametrize("want", [(True, False, False, False, False), (False, True, False, False, False),
                                  (True, True, True, True, False), (False, False, False, False, False)])
def test_planner_allocates_exactly_the_wanted_gradients(want):
    import diff_gaussian_rasterization as D
    dev = torch.device("cpu")
    bucket = D.GradBucket(P, dev)
    plan = D._plan_attr_grads(want, P, dev, bucket)
    assert plan.bucket is None and plan.overwrites          # a bucket is used only when all 59 floats are wanted
    w_x, w_sh, w_op, w_sc, w_ro = want
    shapes = ((P, 3), (P, 1, 3), (P, 15, 3), (P,), (P, 3), (P, 4))
    for buf, wanted, shape in zip(plan.bufs, (w_x, w_sh, w_sh, w_op, w_sc, w_ro), shapes):
        assert (buf is not None) == wanted
        if wanted:
            assert tuple(buf.shape) == shape and buf.dtype == torch.float32
    assert D._autograd_attr_grads(plan) is plan.bufs and bucket.fresh and not bucket.used


def test_a_written_bucket_is_marked_and_autograd_gets_nothing():
    import diff_gaussian_rasterization as D
    dev = torch.device("cpu")
    bucket = D.GradBucket(P, dev)
    assert D._autograd_attr_grads(D._plan_attr_grads((True,) * 5, P, dev, bucket)) == (None,) * 6
    assert bucket.used and not bucket.fresh
