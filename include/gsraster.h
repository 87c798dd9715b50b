/* gsraster.h -- C ABI of libgsraster.so, the MI355X (gfx950) differentiable 3D-Gaussian-splat rasteriser.
 *
 * This is the drop-in boundary for the one hot path of poloclub/3d-gaussian-splat-attack: what the
 * reference reaches through `from diff_gaussian_rasterization import GaussianRasterizationSettings,
 * GaussianRasterizer` (reference gaussian_renderer/__init__.py:14) and calls at
 * gaussian_renderer/__init__.py:36-49 (settings), :51 (constructor) and :86-95 (forward); the backward
 * is reached by `loss.backward()` at attack.py:494.  The third-party CUDA extension behind that import
 * is not vendored in the reference; the entry points below are what a Python binding for it needs.
 *
 * Conventions
 *   - plain C, no torch types: raw DEVICE pointers (float32 / int32, contiguous) + sizes + a hipStream_t
 *     passed as void*;
 *   - every call enqueues on the given stream of the CURRENT hip device; the only host synchronisation is
 *     inside gsr_forward: the host polls a pinned word for the number of (tile, Gaussian) pairs, which a kernel early
 *     in the forward writes there, to size the sort buffers (GSR_FLAG_ASYNC_COUNT removes even that);
 *   - return value 0 = success, otherwise a GSR_ERR_* code and gsr_last_error() describes it
 *     (thread-local string);
 *   - the caller owns all inputs / outputs / gradient buffers and must keep the INPUT tensors of
 *     gsr_forward alive and unmodified until gsr_backward / gsr_ctx_free for that context;
 *     the library owns an internal caching workspace pool per device and the opaque GsrCtx.
 *   - gradient outputs are fully written (zeros for culled Gaussians): no pre-zeroing needed.
 *
 * Host threads (tests/test_gpu_reentrancy.py).  Exactly this is promised:
 *   - calls on DIFFERENT contexts -- forwards, which create one, included -- may run concurrently from different host
 *     threads: forwards beside each other when every thread passes a stream of its own, and a forward beside the
 *     backward / free of another context on one shared stream.  (Two forwards at once on the SAME stream would share that
 *     stream's side stream and its event pair; that is neither tested nor promised.)  The pool, the pinned count slots
 *     and the other process-wide tables are locked inside.  Results are bit for bit those of the same calls made one
 *     after another;
 *   - ONE context is used by one thread at a time.  It may change hands (forward on one thread, gsr_ctx_set_aux_grads,
 *     gsr_backward* and gsr_ctx_free on another -- the autograd engine's pattern) if the caller orders the calls, e.g.
 *     through a queue; nothing inside a context is locked;
 *   - gsr_last_error() is per thread: a thread reads the text of its own last refused call;
 *   - streams: a call's work is ordered by the stream it is given: whatever the caller enqueues on that stream afterwards
 *     runs behind it.  (A forward forks part of its work onto a side stream the library keeps per caller stream and
 *     joins it back into the caller's stream before it returns.)  A context's backward or re-render (gsr_ctx_rerender) on ANOTHER stream than its previous use is
 *     legal when the caller has ordered that stream behind the previous use (an event, or a host wait); the context's
 *     workspace then follows the new stream, and gsr_ctx_free returns it to the pool for that stream.
 *     gsr_ctx_export does NOT move the workspace: it only enqueues a copy out of it.  An export on another stream than
 *     the context's last forward / re-render / backward needs that stream ordered behind that use, as above, and before
 *     the context's next use or its gsr_ctx_free the caller must join the export's stream back into the context's stream
 *     (an event) or wait for it on the host: the freed blocks are re-used in the order of the context's stream, which
 *     knows nothing of the copy.  gsr_ctx_free itself waits for nothing: the context's last use must have been
 *     enqueued, on whatever thread, before it is called.  A free block last used on one stream is handed
 *     to a request on another only once the pool holds its soft cap (an eighth of the device memory, GSR_POOL_CAP_MB
 *     overrides; read once per process) or the device is out of memory, and then behind a host wait for the old stream;
 *   - gsr_trim_pool and gsr_profile* act on the whole process: gsr_trim_pool waits for the device and may be called while
 *     contexts are alive (their blocks stay), but not while another thread is inside a call.
 *
 * Non-finite and extreme inputs (a position or scale step of the attack can produce them: reference attack.py:500-511).
 * The published kernels turn them into undefined float -> int conversions and fully opaque garbage splats; here:
 *   - a Gaussian whose projected conic, pixel centre or view depth is not finite -- NaN or +-inf in its mean, scale,
 *     rotation or covariance, or finite values whose products overflow float32 (exp(log_scale) beyond ~1e19) -- and a
 *     Gaussian whose (activated) opacity is NaN is CULLED: radius 0, no pairs, zero gradients, exactly as if it were behind
 *     the camera.  Every other Gaussian renders and differentiates bit for bit as if the bad one were not in the scene;
 *   - a finite but enormous footprint keeps the published behaviour (its tile rect is the rect clamped to the image: it
 *     reaches every tile) with the radius saturated at 2^24 pixels; num_rendered never exceeds (Gaussians with radius > 0)
 *     x (tiles of the image), and more than 2^31 - 1 pairs in one forward is GSR_ERR_NOMEM, not a wrapped counter;
 *   - a NaN colour (NaN spherical-harmonics coefficients) composites as 0; an infinite one reaches the pixels of the tiles
 *     that Gaussian touches and nothing else; a zero quaternion is the identity rotation times zero (a point: the 0.3 px^2
 *     dilation renders it), as F.normalize's 1e-12 floor makes it in the reference.
 * tests/test_gpu_nonfinite.py; the scalar arithmetic also runs under -fsanitize=undefined,float-cast-overflow on the host
 * (tests/test_host_math.py).
 */
#ifndef GSRASTER_H_
#define GSRASTER_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GSR_VERSION 604 /* 0.6.4: depth and alpha maps (gsr_forward*_aux, gsr_ctx_set_aux_grads); 0.6.3: the groups set-up (gsr_group_classify, gsr_convex_hull_planes, gsr_points_in_hull); 0.6.2: the batch entry points with object channels (gsr_*_batch_obj*); 0.6.1: the batch entry points, gsr_pgd_step_multi, gsr_forward_raw2_batch, gsr_ctx_rerender on batch contexts */
#define GSR_NUM_OBJECTS 16 /* object-feature channels, reference scene/gaussian_model.py:52 */

enum {
  GSR_OK = 0,
  GSR_ERR_INVALID = 1,  /* bad argument combination / sizes */
  GSR_ERR_DEVICE = 2,   /* a HIP call failed (message names the stage) */
  GSR_ERR_NOMEM = 3,
  GSR_ERR_STATE = 4,    /* e.g. backward called twice on a released context */
  GSR_ERR_OVERFLOW = 5, /* GSR_FLAG_ASYNC_COUNT only: the forward emitted more pairs than the guessed capacity */
  GSR_ERR_HULL = 6      /* gsr_convex_hull_planes: the hull failed its own check (no planes returned) */
};

/* flags */
#define GSR_FLAG_NONE 0u
/* Keep every (tile, Gaussian) pair of the 3-sigma tile rect.  By default pairs whose Gaussian cannot reach
 * alpha >= 1/255 on any pixel of the tile are dropped before the sort: outputs are identical, only
 * num_rendered-internal work shrinks.  The flag exists for A/B tests of exactly that claim. */
#define GSR_FLAG_NO_CULL 1u
/* Per-call overrides of launch heuristics -- results do not depend on them (bitwise for the tile map; the tile split
 * only changes which wave owns which strip, and how many partial rows a pair has); they exist so that tests can drive
 * every kernel instantiation on small inputs.  0 in a field = the library's own choice from the tile count.
 *   GSR_FLAG_FWD_SPLIT(n)  n = 1|2|4 pixels per lane in the forward compositor (4|2|1 waves per 16x16 tile)
 *   GSR_FLAG_BWD_SPLIT(n)  n = 2|4   pixels per lane in the backward compositor
 *   GSR_FLAG_TILE_MAP(m)   m = 0..3  block -> tile map: 0 image order, 1 one band per XCD, 2 32-tile bands round
 *                                    robin, 3 longest list first (default)
 *   GSR_FLAG_NO_SEGMENTS             never split a long tile list over several waves (see gsr_backward)
 *   GSR_FLAG_FWD_SHARED              the forward waves of a tile form one workgroup that stages each batch of the list
 *                                    once for all of them (two or four waves per tile only): 38 % less gather traffic,
 *                                    14 % slower on the benchmark scene -- off by default */
#define GSR_FLAG_FWD_SPLIT(n) ((uint32_t)((n) == 1 ? 1u : (n) == 2 ? 2u : (n) == 4 ? 3u : 0u) << 4)
#define GSR_FLAG_BWD_SPLIT(n) ((uint32_t)((n) == 2 ? 1u : (n) == 4 ? 2u : 0u) << 8)
#define GSR_FLAG_TILE_MAP(m) ((uint32_t)(((m) & 3u) + 1u) << 12)
#define GSR_FLAG_NO_SEGMENTS (1u << 16)
#define GSR_FLAG_FWD_SHARED (1u << 17)
/* Asynchronous pair count.  By default gsr_forward waits (once, early, behind work it has already enqueued) for the
 * number of (tile, Gaussian) pairs before it sizes the pair buffers -- the only host synchronisation of the path.
 * With this flag a forward whose (P, H, W) has been rendered before on this device sizes them from the count that
 * earlier forward saw, plus 25 % + 64 K pairs of head-room, and never waits: *num_rendered is then -1 (ask
 * gsr_ctx_info(ctx, 0) later).  If the scene emits more pairs than that capacity, nothing is composited, out_color is
 * filled with NaN, gsr_backward on the context returns GSR_ERR_OVERFLOW, and the next forward counts synchronously
 * again.  Opt-in: a caller that never looks at the image or calls gsr_backward would not notice an overflow. */
#define GSR_FLAG_ASYNC_COUNT (1u << 18)
/* gsr_forward runs the colour half of its per-Gaussian stage (SH -> RGB) on a library-owned side stream, beside the
 * binning chain of the same view, and joins it before compositing (events; the caller's stream semantics are
 * unchanged).  This flag keeps everything on the caller's stream. */
#define GSR_FLAG_NO_SIDE_STREAM (1u << 19)
/* GSR_FLAG_NEEDLE_DOUBLE: splats whose dilated 2D covariance has eigenvalues more than 256 apart ("needles") get their
 * conic -- and, in the backward, their whole per-Gaussian chain rule -- from the published chain evaluated in double on
 * the same float32 inputs (the conic is rounded to its float32 record so that the form along the long axis is preserved).  The float32 chain leaves 1e-7 x that ratio in every conic entry, which a needle's exponent
 * (terms of radius^2 cancelling to O(1)) and gradients (cancelling once more) amplify: a 1500:1 needle's dL/dmean2D is 2.3 %
 * off in float32 -- in the reference's kernels as in any float32 statement of the formula.  Integer decisions (radius, tile
 * rect, culls) and every ordinary splat are unchanged.  Opt-in: it costs the geometry kernel 20 registers and a view
 * 1.3 % (one stream) to 2.8 % (four) on S-nyc-1M, whose splats are not needles (EXPERIMENTS.md, round 5). */
#define GSR_FLAG_NEEDLE_DOUBLE (1u << 20)

/* GSR_FLAG_OBJECTS_FOR_BACKWARD_ONLY: gsr_forward / gsr_forward_raw are given sh_objs but out_objects == NULL -- the object
 * channels are not composited (the caller knows they come out as zeros: all features are zero, which is what the reference's
 * combine_splats gives every Gaussian of an attack scene, scene/gaussian_model.py:528 -- or does not look at them), but the
 * context keeps the features, so that a gsr_backward WITH grad_objects still produces dL/dsh_objs (and the features'
 * share of dL/dalpha) exactly as after a forward that composited them.  Without the flag, sh_objs without out_objects is
 * ignored altogether (no object gradients).  The forward then runs the compositor without object channels: 0.16 ms
 * instead of 0.27 at 1 M Gaussians / 1080p, and 133 MB of output less. */
#define GSR_FLAG_OBJECTS_FOR_BACKWARD_ONLY (1u << 21)

/* Mirrors the 12 fields of GaussianRasterizationSettings in call-site order
 * (reference gaussian_renderer/__init__.py:36-49).  Tensor-valued fields are DEVICE pointers, read by the
 * kernels themselves (no host copy, no sync):
 *   bg          >= 3 floats (the reference passes 4 for black, attack.py:396: only the first 3 are read)
 *   viewmatrix  16 floats, row-major as stored by the reference, i.e. the TRANSPOSED world->view matrix:
 *               p_view = [x y z 1] * viewmatrix          (reference scene/cameras.py:54)
 *   projmatrix  16 floats, full projection in the same convention (reference scene/cameras.py:56)
 *   campos      3 floats                                  (reference scene/cameras.py:57)            */
typedef struct GsrSettings {
  int32_t image_height;
  int32_t image_width;
  float tanfovx;
  float tanfovy;
  const float* bg;
  float scale_modifier;
  const float* viewmatrix;
  const float* projmatrix;
  int32_t sh_degree; /* active degree, 0..3 */
  const float* campos;
  int32_t prefiltered;
  int32_t debug;
  uint32_t flags; /* GSR_FLAG_* (extension; 0 reproduces the reference) */
} GsrSettings;

typedef struct GsrCtx GsrCtx; /* opaque: geometry / binning / per-pixel state of one forward */

/* Forward: replaces GaussianRasterizer.forward (call site reference gaussian_renderer/__init__.py:86-95).
 *   P              number of Gaussians
 *   K              SH coefficients stored per Gaussian and channel in `shs` (16 for max degree 3)
 *   means3D        [P,3]
 *   shs            [P,K,3] coefficient-major then channel (reference scene/gaussian_model.py:113-116), or NULL
 *   sh_objs        [P,16] object features (reference scene/gaussian_model.py:118-120), or NULL (objects = 0)
 *   colors_precomp [P,3] or NULL            (exactly one of shs / colors_precomp)
 *   opacities      [P]   (already sigmoid-activated)
 *   scales         [P,3] (already exp-activated), rotations [P,4] (w,x,y,z, used as given), or both NULL
 *   cov3D_precomp  [P,6] xx,xy,xz,yy,yz,zz or NULL     (exactly one of (scales,rotations) / cov3D_precomp)
 *   out_color      [3,H,W]  (background blended in, not clamped)
 *   out_objects    [16,H,W] or NULL
 *   radii          [P] int32, 0 for culled Gaussians
 *   ctx_out        receives the context for gsr_backward (pass NULL for a forward-only call: nothing is kept)
 *   num_rendered   receives the number of (tile, Gaussian) pairs, may be NULL                               */
int gsr_forward(const GsrSettings* settings, int32_t P, int32_t K, const float* means3D, const float* shs,
                const float* sh_objs, const float* colors_precomp, const float* opacities, const float* scales,
                const float* rotations, const float* cov3D_precomp, float* out_color, float* out_objects,
                int32_t* radii, GsrCtx** ctx_out, int64_t* num_rendered, void* stream);

/* Backward: what loss.backward() (reference attack.py:494) reaches through the extension's autograd function.
 *   grad_color   [3,H,W]; grad_objects [16,H,W] or NULL (treated as zero)
 *   outputs (any may be NULL = not wanted):
 *   dmeans3D [P,3], dmeans2D [P,3] (gradient w.r.t. the screen-space means in NDC units, z = 0; this is what
 *   lands in viewspace_points.grad, reference gaussian_renderer/__init__.py:26-30), dshs [P,K,3],
 *   dsh_objs [P,16], dcolors_precomp [P,3], dopacities [P], dscales [P,3], drotations [P,4], dcov3D [P,6].
 * When every geometry-side output (dmeans3D, dmeans2D, dopacities, dscales, drotations, dcov3D) is NULL the
 * backward runs its colour-only kernels (no conic / mean / opacity sums, no projection chain rule); the colour-side
 * gradients are the same numbers either way.
 * May be called more than once on a context (retain_graph).                                                  */
int gsr_backward(GsrCtx* ctx, const float* grad_color, const float* grad_objects, float* dmeans3D, float* dmeans2D,
                 float* dshs, float* dsh_objs, float* dcolors_precomp, float* dopacities, float* dscales,
                 float* drotations, float* dcov3D, void* stream);

/* Fused-activation variants of the same path for callers that hold a reference-style GaussianModel: the seven RAW
 * parameter tensors go in (reference scene/gaussian_model.py:42-59) and the activation getters the reference's render()
 * applies first (exp / sigmoid / normalize / cat, scene/gaussian_model.py:97-124, gaussian_renderer/__init__.py:53-83)
 * and their chain rule run inside the per-Gaussian kernels, so no activated copy of the attributes is written to HBM.
 *   xyz [P,3]; features_dc [P,1,3]; features_rest [P,15,3]; objects_dc [P,16] or NULL; opacity_logit [P];
 *   log_scaling [P,3]; rotation_raw [P,4] (un-normalised; normalised as v / max(|v|, 1e-12)).
 * Results equal gsr_forward / gsr_backward composed with those PyTorch ops; gradients are w.r.t. the RAW tensors. */
int gsr_forward_raw(const GsrSettings* settings, int32_t P, const float* xyz, const float* features_dc,
                    const float* features_rest, const float* objects_dc, const float* opacity_logit,
                    const float* log_scaling, const float* rotation_raw, float* out_color, float* out_objects,
                    int32_t* radii, GsrCtx** ctx_out, int64_t* num_rendered, void* stream);
int gsr_backward_raw(GsrCtx* ctx, const float* grad_color, const float* grad_objects, float* dxyz, float* dmeans2D,
                     float* dfeatures_dc, float* dfeatures_rest, float* dobjects_dc, float* dopacity_logit,
                     float* dlog_scaling, float* drotation_raw, void* stream);

/* gsr_backward_raw with a choice of what happens to the output buffers.  accumulate == 0: they are overwritten (zeros
 * for Gaussians without pairs), exactly gsr_backward_raw.  accumulate != 0: the 59 attribute gradients (dxyz, dfeatures_dc,
 * dfeatures_rest, dopacity_logit, dlog_scaling, drotation_raw) are ADDED to what the buffers hold and Gaussians without
 * pairs are not touched at all; dmeans2D and dobjects_dc, which belong to ONE view (the screen-space gradient the
 * reference reads from viewspace_points.grad, the object-feature gradient), are overwritten in either mode, zeros for
 * Gaussians without pairs included.  That is what a batch of views needs (reference
 * attack.py:476-494: the B renders' gradients add up in .grad): the first view of a PGD iteration overwrites a
 * caller-owned [P,59] bucket, the others add to it, and the per-view gradient buffer plus the framework's
 * read-modify-write accumulation of 236 bytes per Gaussian and view disappear.  Concurrent calls (views on different
 * streams) must use different buckets. */
int gsr_backward_raw_into(GsrCtx* ctx, const float* grad_color, const float* grad_objects, float* dxyz, float* dmeans2D,
                          float* dfeatures_dc, float* dfeatures_rest, float* dobjects_dc, float* dopacity_logit,
                          float* dlog_scaling, float* drotation_raw, int32_t accumulate, void* stream);

/* gsr_backward_raw_into with the per-Gaussian stage run as `nchunks` launches over consecutive ranges of Gaussians
 * (boundaries at multiples of 64).  After each range's launch has been enqueued, chunk_done(user, chunk, g_begin, g_end) is
 * called on the calling thread: every gradient of Gaussians [g_begin, g_end) is then complete in stream order, so the caller
 * can issue the multi-GPU sum of that range (six slices of the bucket) while the next range is still being computed
 * ("reduce while K9 finishes").  Results are bit for bit those of the unchunked call. */
typedef void (*gsr_chunk_fn)(void* user, int32_t chunk, int64_t g_begin, int64_t g_end);
int gsr_backward_raw_chunked(GsrCtx* ctx, const float* grad_color, const float* grad_objects, float* dxyz, float* dmeans2D,
                             float* dfeatures_dc, float* dfeatures_rest, float* dobjects_dc, float* dopacity_logit,
                             float* dlog_scaling, float* drotation_raw, int32_t accumulate, int32_t nchunks,
                             gsr_chunk_fn chunk_done, void* user, void* stream);

/* A BATCH of views of one set of raw parameters through ONE launch chain.  The reference's batch is a Python loop of B
 * render() calls on the same attributes (reference attack.py:476-485; :522-530 for the success renders) whose B backward
 * passes add up in .grad (:494); every call repeats the latency-bound binning chain (scan, two sorts, emission, schedule:
 * ~20 short launches), re-reads the 192-byte SH rows and re-writes 236 bytes of gradient per Gaussian.  Here the B views
 * form one virtual scene -- view v owns the virtual Gaussians [v * Ppad, v * Ppad + P) and the tiles [v * T, (v + 1) * T) --
 * and the scans, both sorts, the emission, the tile schedule and the two compositors run once over it.
 *   settings     [B] (1 <= B <= 16): per view the camera tensors, tan(fov / 2) and background; image size, scale_modifier,
 *                sh_degree and flags must be the same in all of them (GSR_FLAG_NEEDLE_DOUBLE is not available)
 *   out_color    [B,3,H,W]; radii [B,P]; no object channels
 *   num_rendered receives the (tile, Gaussian) pairs of all B views together
 * Every view's image and radii are bit for bit those of gsr_forward_raw on that view's settings.
 * gsr_backward_raw_batch_into: grad_color [B,3,H,W]; the 59 attribute gradients are the SUM over the B views, written once
 * (accumulate == 0; Gaussians without pairs in any view: zeros) or added to what the buffers hold (accumulate != 0) -- bit
 * for bit what B calls of gsr_backward_raw_into in view order leave, the first with the caller's `accumulate` and the
 * others adding; dmeans2D [B,P,3] or NULL is per view (overwritten).  gsr_backward_raw / _into / _chunked accept a batch
 * context with these shapes too, and so do gsr_ctx_request_sumsq (the batch's one fused per-Gaussian launch leaves the sums
 * of squares of the SUMMED gradient) and gsr_ctx_rerender (below: the batch's colour kernel + the compositor over the kept
 * lists of all B views). */
int gsr_forward_raw_batch(const GsrSettings* settings, int32_t B, int32_t P, const float* xyz, const float* features_dc,
                          const float* features_rest, const float* opacity_logit, const float* log_scaling,
                          const float* rotation_raw, float* out_color, int32_t* radii, GsrCtx** ctx_out,
                          int64_t* num_rendered, void* stream);
int gsr_backward_raw_batch_into(GsrCtx* ctx, const float* grad_color, float* dxyz, float* dmeans2D, float* dfeatures_dc,
                                float* dfeatures_rest, float* dopacity_logit, float* dlog_scaling, float* drotation_raw,
                                int32_t accumulate, void* stream);
/* The same backward with PER-VIEW attribute gradients, for callers that need every view's own gradient (independent views
 * that merely share a launch chain): the six attribute-gradient pointers are VIEW 0's buffers, view v's lie v * view_stride
 * floats further (e.g. B gradient buckets of 59 * P floats one after another: view_stride = 59 * P); dmeans2D is [B,P,3] as
 * above.  One forward-batch chain and one backward composite for all views, then one per-Gaussian launch per view: view v's
 * buffers receive bit for bit what gsr_backward_raw on that view alone writes (zeros for Gaussians the view does not see). */
int gsr_backward_raw_batch_views(GsrCtx* ctx, const float* grad_color, float* dxyz, float* dmeans2D, float* dfeatures_dc,
                                 float* dfeatures_rest, float* dopacity_logit, float* dlog_scaling, float* drotation_raw,
                                 int64_t view_stride, void* stream);

/* The batch entry points WITH the 16 object channels (the map the reference's render() returns as render_object and its
 * evaluation loop hands to the object classifier, reference render.py:125-131).  Same checks as gsr_forward_raw_batch
 * (messages name the function), plus objects_dc [P,16] non-NULL.
 *   out_objects  [B,16,H,W], or NULL: no object map; as in gsr_forward_raw the features are then kept for the backward only
 *                under GSR_FLAG_OBJECTS_FOR_BACKWARD_ONLY
 * Every view's image, radii and object map are bit for bit those of gsr_forward_raw with objects_dc on that view's settings.
 * gsr_backward_raw_batch_obj_into: as gsr_backward_raw_batch_into, plus grad_objects [B,16,H,W] or NULL and dobjects_dc
 * [P,16] or NULL.  dobjects_dc is always OVERWRITTEN (like gsr_backward_raw's, it is not part of the 59-float bucket and
 * ignores `accumulate`) with ((s_0 + s_1) + s_2) + ..., s_v the object gradient gsr_backward_raw on view v alone writes: bit
 * for bit what .grad of the object features holds after B single-view backwards in view order (zeros for a Gaussian no view
 * sees).  With grad_objects the backward composite walks whole tile lists (as a single view given dL/dobjects does);
 * without it, it is the segmented composite of gsr_backward_raw_batch_into, and the 59 gradients are the same bits as the
 * no-object batch's.
 * gsr_backward_raw_batch_obj_views: as gsr_backward_raw_batch_views, plus grad_objects and dobjects_dc [B,P,16]: view v's
 * s_v at dobjects_dc + v * 16 P.
 * gsr_forward_raw2_batch_obj: gsr_forward_raw2_batch with objects_dc_a [Pa,16] / objects_dc_b [Pb,16] (both or neither) and
 * out_objects [B,16,H,W] or NULL; every object map bit for bit gsr_forward_raw2's for that view.
 * gsr_ctx_rerender on a context of these forwards takes out_objects [B,16,H,W] when the forward composited object channels. */
int gsr_forward_raw_batch_obj(const GsrSettings* settings, int32_t B, int32_t P, const float* xyz, const float* features_dc,
                              const float* features_rest, const float* objects_dc, const float* opacity_logit,
                              const float* log_scaling, const float* rotation_raw, float* out_color, float* out_objects,
                              int32_t* radii, GsrCtx** ctx_out, int64_t* num_rendered, void* stream);
int gsr_forward_raw2_batch_obj(const GsrSettings* settings, int32_t B, int32_t Pa, const float* xyz_a,
                               const float* features_dc_a, const float* features_rest_a, const float* objects_dc_a,
                               const float* opacity_logit_a, const float* log_scaling_a, const float* rotation_raw_a, int32_t Pb,
                               const float* xyz_b, const float* features_dc_b, const float* features_rest_b,
                               const float* objects_dc_b, const float* opacity_logit_b, const float* log_scaling_b,
                               const float* rotation_raw_b, float* out_color, float* out_objects, int32_t* radii,
                               GsrCtx** ctx_out, int64_t* num_rendered, void* stream);
int gsr_backward_raw_batch_obj_into(GsrCtx* ctx, const float* grad_color, const float* grad_objects, float* dxyz,
                                    float* dmeans2D, float* dfeatures_dc, float* dfeatures_rest, float* dobjects_dc,
                                    float* dopacity_logit, float* dlog_scaling, float* drotation_raw, int32_t accumulate,
                                    void* stream);
int gsr_backward_raw_batch_obj_views(GsrCtx* ctx, const float* grad_color, const float* grad_objects, float* dxyz,
                                     float* dmeans2D, float* dfeatures_dc, float* dfeatures_rest, float* dobjects_dc,
                                     float* dopacity_logit, float* dlog_scaling, float* drotation_raw, int64_t view_stride,
                                     void* stream);

/* Forward-only render of TWO parameter sets as one scene: the attacked target (a) followed by the frozen background (b),
 * Gaussians numbered a then b (radii [Pa+Pb]).  Replaces what the reference does after every PGD step to check the
 * attack: deep-copy the attacked model, append the background to each of its seven tensors (seven concat_setup calls,
 * ~300 MB at 1 M Gaussians) and render the copy (reference attack.py:513-530).  Same image, bit for bit, as
 * gsr_forward_raw on the concatenated tensors; nothing is copied, no context is kept (the reference never
 * differentiates this render).  objects_dc_*: both or neither. */
int gsr_forward_raw2(const GsrSettings* settings, int32_t Pa, const float* xyz_a, const float* features_dc_a,
                     const float* features_rest_a, const float* objects_dc_a, const float* opacity_logit_a,
                     const float* log_scaling_a, const float* rotation_raw_a, int32_t Pb, const float* xyz_b,
                     const float* features_dc_b, const float* features_rest_b, const float* objects_dc_b,
                     const float* opacity_logit_b, const float* log_scaling_b, const float* rotation_raw_b,
                     float* out_color, float* out_objects, int32_t* radii, int64_t* num_rendered, void* stream);

/* gsr_forward_raw2 that can keep its context -- for gsr_ctx_rerender ONLY: the context holds the binning and the splat
 * records but no backward state (gsr_backward* on it return GSR_ERR_STATE), as the reference never differentiates this
 * render.  ctx_out == NULL: exactly gsr_forward_raw2. */
int gsr_forward_raw2_keep(const GsrSettings* settings, int32_t Pa, const float* xyz_a, const float* features_dc_a,
                          const float* features_rest_a, const float* objects_dc_a, const float* opacity_logit_a,
                          const float* log_scaling_a, const float* rotation_raw_a, int32_t Pb, const float* xyz_b,
                          const float* features_dc_b, const float* features_rest_b, const float* objects_dc_b,
                          const float* opacity_logit_b, const float* log_scaling_b, const float* rotation_raw_b,
                          float* out_color, float* out_objects, int32_t* radii, GsrCtx** ctx_out, int64_t* num_rendered,
                          void* stream);

/* gsr_forward_raw2_keep for a BATCH of views: the attacked target (a) followed by the frozen background (b) rendered from B
 * cameras through one launch chain -- the success renders of a batch of views (reference attack.py:513-530 renders the
 * combined scene once per camera of the batch, inside the loop of :476-485).  Forward only: settings [B], out_color
 * [B,3,H,W], radii [B,Pa+Pb], no object channels; Pa, Pb > 0.  Every image and radius is bit for bit gsr_forward_raw2's
 * for that view.  A kept context serves gsr_ctx_rerender ONLY (gsr_backward* return GSR_ERR_STATE). */
int gsr_forward_raw2_batch(const GsrSettings* settings, int32_t B, int32_t Pa, const float* xyz_a, const float* features_dc_a,
                           const float* features_rest_a, const float* opacity_logit_a, const float* log_scaling_a,
                           const float* rotation_raw_a, int32_t Pb, const float* xyz_b, const float* features_dc_b,
                           const float* features_rest_b, const float* opacity_logit_b, const float* log_scaling_b,
                           const float* rotation_raw_b, float* out_color, int32_t* radii, GsrCtx** ctx_out,
                           int64_t* num_rendered, void* stream);

/* Re-render of a kept context after ONLY its colour inputs changed.  A colour attack (reference attack.py:25-49 steps
 * _features_dc / _features_rest and nothing else; configs/config.yaml attack groups = ["color"]; BASELINE configs 2, 3)
 * renders the same cameras iteration after iteration with the same means, scales, rotations and opacities: projection,
 * tile rects, depth order, the sorted (tile, Gaussian) lists, the tile schedule and the geometric words of the splat
 * records are then the same every time.  The reference's extension rebuilds them per call; a context kept in HBM
 * (about 250 MB per camera at 1 M Gaussians / 1080p, of 288 GB) makes a render of such a view two kernels: the colour half
 * of K1 (SH -> RGB over the Gaussians that emit pairs, into the colour words of the kept records) and the compositor K6
 * over the kept lists.  Image, radii-independent outputs and every gradient of a following gsr_backward* are bit for bit
 * those of a fresh gsr_forward* with the same inputs (tests/test_gpu_rerender.py).
 *   ctx            from gsr_forward / gsr_forward_raw (SH input: raw parameters, or shs with K = 16) with ctx_out, or from
 *                  gsr_forward_raw2_keep.  The CALLER guarantees that since that forward nothing but the SH coefficients
 *                  and bg changed: same means / opacities / scales / rotations contents, same camera, sizes, flags.
 *   features_dc, features_rest   the coefficients to render with ([P,1,3], [P,15,3]; a gsr_forward context: NULL and
 *                  shs [P,16,3]); NULL = the pointers of the previous render (their CONTENTS may have changed).  The
 *                  context re-reads them in gsr_backward*: keep them alive and unmodified until then, as after a forward.
 *   features_*_b   the same for the second segment of a gsr_forward_raw2_keep context (else NULL)
 *   bg             >= 3 floats, or NULL = the previous background pointer
 *   out_color      [3,H,W]; out_objects [16,H,W] or NULL (only if the context's forward composited them)
 *   flags          GSR_RERENDER_COLOR_GRADS_ONLY: the backward of this render will ask for colour-side gradients only
 *                  (dfeatures_*, dcolors): the colour kernel then skips the 36 bytes per Gaussian of d colour / d view
 *                  direction it leaves for dL/dmeans; a geometry backward on the context returns GSR_ERR_STATE until
 *                  the next re-render without the flag.
 *                  GSR_RERENDER_FIRST_SEGMENT_ONLY (two-segment contexts): the second segment's coefficients have not
 *                  changed since the context's last render (the frozen background of reference attack.py:513-530): the
 *                  colour kernel covers the first segment's Gaussians only; features_*_b must be NULL.
 * A BATCH context (gsr_forward_raw_batch): out_color [B,3,H,W]; bg [B,3] (view v's background at bg + 3 v) or NULL = the
 *                  views' previous background pointers, whose contents are read again; out_objects [B,16,H,W] if the
 *                  forward composited object channels (gsr_*_batch_obj), else NULL
 *                  (features_*_b and GSR_RERENDER_FIRST_SEGMENT_ONLY as above for a gsr_forward_raw2_batch context).  One launch of the batch's colour kernel (every SH row read once for all views that see the
 *                  Gaussian) and one compositor launch over the B views' kept lists: images and the gradients of a following
 *                  gsr_backward_raw_batch_* are bit for bit those of a fresh gsr_forward_raw_batch with the same inputs.
 * The per-pixel state the backward reads (final T, last contributor, segment-boundary records) is overwritten: a
 * backward of the PREVIOUS render of this context must have been enqueued before, on the same stream or ordered
 * before it by the caller. */
#define GSR_RERENDER_COLOR_GRADS_ONLY 1u
#define GSR_RERENDER_FIRST_SEGMENT_ONLY 2u
int gsr_ctx_rerender(GsrCtx* ctx, const float* features_dc, const float* features_rest, const float* features_dc_b,
                     const float* features_rest_b, const float* bg, float* out_color, float* out_objects, uint32_t flags,
                     void* stream);

/* Releases the context's workspace back to the pool (stream-ordered: safe right after enqueueing backward). */
void gsr_ctx_free(GsrCtx* ctx);

/*
 * Depth and alpha maps from the compositors (0.6.4).  Two optional per-pixel outputs of the forward, accumulated in the
 * same walk of the tile list that blends the colour, and two optional incoming gradients of the backward.
 *   out_alpha [H,W]  A = 1 - T_final: the sum of alpha_i T_i over exactly the entries the colour walk blends (same
 *                    alpha >= 1/255 test, power <= 0, min(0.99, .) cap, stop when T (1 - alpha) < 1e-4).  No background
 *                    term.  Bit for bit 1.0f - final_T of the same forward (gsr_ctx_export item 3).
 *   out_depth [H,W]  D = sum of z_i alpha_i T_i over the same entries, z_i the float32 view depth of the splat (the value
 *                    the depth sort keys on).  A colour channel whose colour is z_i and whose background is 0: NOT divided
 *                    by alpha and with no background term.  The expected depth of the covered part of a pixel is D / A,
 *                    one tensor division for a caller who wants it (undefined where A = 0).
 * The _aux entry points take the argument list of the function they are named after plus (out_depth, out_alpha) in front
 * of `stream`; either may be NULL (not wanted; both NULL: the plain call).  Batch shapes are [B,H,W].  Everything else
 * the plain call writes is bit for bit unchanged.  GSR_FLAG_NEEDLE_DOUBLE is refused (GSR_ERR_INVALID).
 * Backward: gsr_ctx_set_aux_grads(ctx, grad_depth, grad_alpha) arms the NEXT gsr_backward / gsr_backward_raw /
 * gsr_backward_raw_into / gsr_backward_raw_batch_into of this context (grad_depth, grad_alpha: [H,W] or [B,H,W] device
 * pointers that must stay valid until that backward has run; either may be NULL = zero; both NULL disarms).  The armed
 * backward adds, to the gradients of opacity, means (3D and dmeans2D), scales, rotations / cov3D, what the two maps
 * contribute through alpha_i -- per pixel the colour walk's c_i . g_C becomes c_i . g_C + z_i g_D + g_A, both extra
 * channels having background 0 -- and grad_depth additionally through z_i: dL/dz_i = sum over pixels of alpha_i T_i g_D,
 * dz_i / dmean = viewmatrix[0..2][2].  The 0.99 cap is transparent as for colour.  SH / colour / object-feature gradients
 * receive nothing from the maps.  With all-zero aux gradients every gradient is bit for bit that of the unarmed backward
 * taking the same walk (the nine sums of the colour backward keep their arithmetic; see "Long tile lists" below).
 * One-shot: every backward takes the request and disarms the context at its top, whatever its own fate.
 * Long tile lists: a backward with grad_alpha alone walks segments as the colour backward does; one with grad_depth walks
 * whole lists (the boundary records hold no running depth), like a backward with grad_objects.
 * Refused with GSR_ERR_STATE: arming a context whose forward was not an _aux call, a forward-only or re-rendered (
 * gsr_ctx_rerender refuses aux contexts) one.  Refused with GSR_ERR_INVALID by the backward that finds the context armed:
 * gsr_backward_raw_batch_views / _obj_views (per-view gradients), gsr_backward_raw_chunked with more than one range, a
 * backward that is also handed grad_objects, one that asks for no geometry gradient at all, and a gsr_forward context with
 * K != 16 SH coefficients.  Never silently ignored.
 * Non-finite inputs: a culled Gaussian leaves both maps and their gradients bit for bit as if it were not in the scene.
 */
int gsr_forward_aux(const GsrSettings* settings, int32_t P, int32_t K, const float* means3D, const float* shs,
                    const float* sh_objs, const float* colors_precomp, const float* opacities, const float* scales,
                    const float* rotations, const float* cov3D_precomp, float* out_color, float* out_objects,
                    int32_t* radii, GsrCtx** ctx_out, int64_t* num_rendered, float* out_depth, float* out_alpha,
                    void* stream);
int gsr_forward_raw_aux(const GsrSettings* settings, int32_t P, const float* xyz, const float* features_dc,
                        const float* features_rest, const float* objects_dc, const float* opacity_logit,
                        const float* log_scaling, const float* rotation_raw, float* out_color, float* out_objects,
                        int32_t* radii, GsrCtx** ctx_out, int64_t* num_rendered, float* out_depth, float* out_alpha,
                        void* stream);
int gsr_forward_raw_batch_aux(const GsrSettings* settings, int32_t B, int32_t P, const float* xyz,
                              const float* features_dc, const float* features_rest, const float* opacity_logit,
                              const float* log_scaling, const float* rotation_raw, float* out_color, int32_t* radii,
                              GsrCtx** ctx_out, int64_t* num_rendered, float* out_depth, float* out_alpha, void* stream);
int gsr_ctx_set_aux_grads(GsrCtx* ctx, const float* grad_depth, const float* grad_alpha);


/* Frustum test only (view-space z > 0.2): present[P] = 1/0.  Replaces GaussianRasterizer.markVisible. */
int gsr_mark_visible(const GsrSettings* settings, int32_t P, const float* means3D, uint8_t* present, void* stream);

/*
 * gsr_pgd_step: one projected-gradient update of a raw attribute tensor x[rows, cols] in place (reference
 * attack.py:25-173, the ten gaussian_*_{linf,l2}_attack functions; the colour rules call it once for _features_rest
 * [P,45] and once for _features_dc [P,3]).  l2 == 0: x += -alpha*sign(grad); x = clamp(x - x0, -eps, eps) + x0.
 * l2 != 0: x += -alpha*grad/||grad||_2 with the norm over the whole tensor (no step when it is 0), then every ROW of
 * x - x0 longer than eps is scaled by eps/(norm + 1e-7) (torch.renorm(p=2, dim=0, maxnorm=eps)).  cols <= 48.
 * A row exactly eps long is not scaled.  Only x is written; grad and x0 are read.
 * Non-finite and out-of-range inputs follow the tensor formulation (gsplat_attack/pgd.py on the CPU; csrc/gsr_pgd.h has
 * the full list): sign(NaN) = 0; a NaN in x or x0 comes out NaN at that element under both rules, and under L2 its row
 * is not scaled; an infinite x or x0 element gives x0 +- eps resp. +-inf under L-inf, and under L2 NaN at that element
 * and x0 in the rest of its row.  L2: a NaN gradient element or a NaN sum of squares means NO step for the whole tensor
 * (the projection still runs); an infinite gradient element means no step at the finite elements and NaN at that one.
 * The norm is a float32 and the squares are summed in float32 per thread: gradients of magnitude <= 1e-23 (every square
 * underflows) or >= 1e19 on 12 elements or more (the sum overflows) lose the L2 step, x stays finite; squares that are
 * float32 denormals (|grad| below about 1e-19) make the step's length approximate.  A sum handed in as a double
 * (gsr_pgd_step_normed, sumsq[] of gsr_pgd_step_multi) is used down to a norm of FLT_MIN.  eps = 0 returns x0.
 */
int gsr_pgd_step(float* x, const float* grad, const float* x0, int64_t rows, int32_t cols, float alpha, float epsilon,
                 int32_t l2, void* stream);

/*
 * The L2 rules' global norm without a second pass over the gradient (round 5).  gsr_ctx_request_sumsq arms the NEXT
 * overwrite-mode gsr_backward_raw / gsr_backward_raw_into (accumulate == 0, not chunked) of this context: besides the
 * gradients it leaves, in out6 (DEVICE memory, 6 doubles, written in stream order), the sums of squares of the gradients
 * it writes for xyz, features_dc, features_rest, opacity_logit, log_scaling, rotation_raw -- the quantities whose roots
 * reference attack.py:61-62,70-71,...,145-146,154-155 divide by (a tensor whose gradient pointer is NULL gets 0).  The
 * sums are those of THAT launch's output: a caller that adds other views' gradients to the buffers afterwards must not
 * use them.  One-shot: the request is consumed by the backward it serves.
 * gsr_pgd_step_normed is gsr_pgd_step's L2 rule with ||grad||^2 read from `sumsq` (device, one double) instead of being
 * summed by a launch of its own: one launch per tensor, one read of the gradient.
 */
int gsr_ctx_request_sumsq(GsrCtx* ctx, double* out6);
int gsr_pgd_step_normed(float* x, const float* grad, const float* x0, int64_t rows, int32_t cols, float alpha, float epsilon,
                        const double* sumsq, void* stream);

/*
 * gsr_pgd_step_multi (round 6): the update of gsr_pgd_step / gsr_pgd_step_normed on n <= 8 tensors of one model in ONE
 * launch (the attack steps _xyz, _features_dc, _features_rest, _opacity, _scaling, _rotation in one iteration, reference
 * attack.py:496-520: six short bandwidth-bound launches whose tails nothing on the stream covers).  Arrays of n host
 * entries: x / grad / x0 device pointers, rows, cols (<= 48), alpha, epsilon; sumsq[t] = device pointer to ||grad_t||^2
 * (one double, as gsr_pgd_step_normed takes it) or NULL -- with l2 != 0 a tensor without one has its norm summed by a
 * launch of its own in front (sumsq == NULL: all of them).  Results are bit for bit those of the per-tensor calls.
 */
int gsr_pgd_step_multi(int32_t n, float* const* x, const float* const* grad, const float* const* x0, const int64_t* rows,
                       const int32_t* cols, const float* alpha, const float* epsilon, int32_t l2, const double* const* sumsq,
                       void* stream);

/*
 * gsr_adam_step_multi: one Adam step (torch.optim.Adam without weight decay, amsgrad or maximize; reference
 * scene/gaussian_model.py:160-214,350-367, the optimiser of training_setup / finetune_setup / inpaint_setup) on n <= 8
 * tensors of one model in ONE launch, in place.  No change of GSR_VERSION, no capability bit: the stage is present iff
 * the library exports this symbol.  Arrays of n HOST entries: x / g / m / v device pointers to float32 [rows, cols]
 * (parameter, gradient, first and second moment; g is only read), rows, cols (1..48), lr, beta1, beta2, eps.  Per element,
 * every operation rounded once in this order (csrc/gsr_adam.h):
 *     m'  = m + (1 - beta1) * (g - m)
 *     v'  = beta2 * v + (1 - beta2) * (g * g)
 *     den = sqrtf(v') / sqrt_bc2 + eps
 *     x'  = x - step_size * (m' / den)
 * step_size = lr / (1 - beta1^step) and sqrt_bc2 = sqrt(1 - beta2^step) are formed on the host in double from the
 * integer count `step` >= 1 of THIS step and rounded once to float32: no device scalar, no read-back.  Results are
 * bitwise reproducible and bit for bit those of the host build of csrc/gsr_adam.h.
 * Row selection, shared by all tensors of the call (which must then have equal row counts): row_mask = NULL or a device
 * uint8 [rows] (non-zero = the row moves); [row_begin, row_end) with row_end = -1 meaning rows.  A row outside the range
 * or with a zero byte is neither read nor written in x, m and v.  A workgroup (one wave, 1024 consecutive floats of a
 * tensor) whose rows are all left out returns after reading their mask bytes.
 * Non-finite and range (what torch.optim.Adam does on CPU float32 tensors, element by element; csrc/gsr_adam.h has the
 * list): a NaN or infinite gradient element poisons m, v and x at that element only; g = 0 with zero moments moves
 * nothing; a square that underflows leaves den = eps; |g| up to 1.84e19 keeps g * g and v finite (beyond it v = +inf and x stays); lr = 0 updates the moments
 * and leaves x bit for bit.
 * Refused before the launch: n outside 1..8, step < 1, a null array, cols outside 1..48, negative rows, a null pointer
 * among the four of a tensor with rows > 0, unequal row counts with a mask or a range, a range outside
 * 0 <= begin <= end <= rows, a beta outside [0, 1), eps < 0, a non-finite lr, beta or eps.  A tensor without rows is
 * skipped; a call without any row to move launches nothing and returns 0.
 */
int gsr_adam_step_multi(int32_t n, void* const* x, const void* const* g, void* const* m, void* const* v, const int64_t* rows,
                        const int32_t* cols, const float* lr, const float* beta1, const float* beta2, const float* eps,
                        int64_t step, const uint8_t* row_mask /* or null */, int64_t row_begin, int64_t row_end /* -1: rows */,
                        void* stream);

/*
 * Adaptive density control (reference scene/gaussian_model.py:591-712: add_densification_stats, densify_and_prune with its
 * clone, split and prune passes, prune_points) as one launch chain with ONE read-back; the scalar contract, its deviations
 * from the reference and the non-finite rules are in csrc/gsr_densify.h.  No change of GSR_VERSION, no capability bit: the
 * stage is present iff the library exports these symbols.  All tensors are contiguous float32 on the device unless said.
 *
 * gsr_densify_stats: for the B views of grad [B, P, 3] in view order, where filter [B, P] (uint8) is non-zero -- or, with
 *   filter NULL, where radii [B, P] (int32) > 0 --: accum[i] += sqrtf(gx gx + gy gy), denom[i] += 1 and, with radii and
 *   max_radii given, max_radii[i] = max(max_radii[i], radii).  One lane per Gaussian; bit for bit B single-view calls.
 *
 * gsr_densify_plan: classifies the P rows from accum / denom (NaN -> 0) >= max_grad, the row's largest raw scale against
 *   log(percent_dense extent) and, with GSR_DENSIFY_WORLD_PRUNE, log(0.1 extent), the raw opacity against logit(min_opacity),
 *   a child's scale (raw - log(0.8 N)), and with GSR_DENSIFY_SCREEN_PRUNE max_radii [P] > max_screen_size; scans the three
 *   counts into `ws` (device, 16-byte aligned, gsr_densify_plan_bytes(P) bytes) and returns counts[3] (HOST) = {kept originals,
 *   kept clones, split parents whose children stay}: P' = counts[0] + counts[1] + N counts[2].  Waits for the stream once.
 *
 * gsr_densify_plan_prune: the plan of a plain prune (reference prune_points :591-606) from a byte mask [P] (non-zero = the row
 *   goes): counts = {kept rows, 0, 0}, the same workspace, the same one wait.
 *
 * gsr_densify_apply: moves n <= 8 tensors src[t] [P, cols[t] <= 48] to dst[t] [P', cols[t]] in ONE launch, in the reference's
 *   order: kept originals in row order, clones in parent order, children j-major (child j of the k-th split parent at
 *   counts[0] + counts[1] + j counts[2] + k).  roles[t]: 0 copy; 1 xyz (a child is xyz + R(q) (z * exp(scale)), q = `rotation`
 *   [P, 4], scale = the source of the role-2 tensor, z = normals [P, N, 3] or, with normals NULL, the keyed normal of (seed,
 *   row, child, axis)); 2 scale (a child gets raw - log(0.8 N)).  m_src / v_src / m_dst / v_dst (all four NULL, or per tensor a
 *   pair in and out or NULL): kept rows carry their moments, new rows get zeros.  mask_in [P] / mask_out [P'] (uint8): the
 *   optimiser's row mask follows its rows, new rows get 1 (mask_in NULL: kept rows get 1).  origin / kind [P'] (int32, both or
 *   neither): the source row, and 0 keep, 1 clone, 2 + j child j.  Every element of every destination is written exactly once;
 *   the sources are not written.  ws, P, N and counts must be those of the plan.  counts[1] = counts[2] = 0 is a fused prune.
 *
 * GSR_ERR_INVALID before any launch: N outside 1..8, more than 8 tensors, cols outside 1..48, P or P' above 2^28, anything
 * written (a destination, a moment out, mask_out, origin, kind) that overlaps anything read (a source, a moment in, the rotation,
 * the normals, mask_in, the workspace) or another output, a max_grad / extent (with percent_dense) / min_opacity / max_screen_size whose
 * threshold is not a finite float32 (the message names which), unknown flags, a workspace too small or misaligned.
 */
#define GSR_DENSIFY_WORLD_PRUNE 1u
#define GSR_DENSIFY_SCREEN_PRUNE 2u
int gsr_densify_stats(const float* grad, const int32_t* radii /* or null */, const uint8_t* filter /* or null */, int32_t B,
                      int64_t P, float* accum, float* denom, float* max_radii /* or null */, void* stream);
int gsr_densify_plan_bytes(int64_t P, int64_t* bytes);
int gsr_densify_plan(const float* accum, const float* denom, const float* scaling, const float* opacity,
                     const float* max_radii /* or null */, int64_t P, double max_grad, double min_opacity, double extent,
                     double percent_dense, double max_screen_size, int32_t N, uint32_t flags, void* ws, int64_t ws_bytes,
                     int64_t* counts, void* stream);
int gsr_densify_plan_prune(const uint8_t* prune_mask, int64_t P, void* ws, int64_t ws_bytes, int64_t* counts, void* stream);
int gsr_densify_apply(const void* ws, int64_t ws_bytes, int64_t P, const int64_t* counts, int32_t n, const void* const* src,
                      void* const* dst, const void* const* m_src, const void* const* v_src, void* const* m_dst,
                      void* const* v_dst, const int32_t* cols, const int32_t* roles, const float* rotation, int32_t N,
                      uint32_t seed, const float* normals /* or null */, const uint8_t* mask_in /* or null */,
                      uint8_t* mask_out /* or null */, int32_t* origin /* or null */, int32_t* kind /* or null */, void* stream);

/* Mean squared distance of every point to its 3 nearest other points (exact): replaces the reference's second native
 * import, simple_knn._C.distCUDA2 (reference scene/gaussian_model.py:17, called at :144 to seed the initial scales).
 * points [P,3] float32 device, mean_dist2 [P] float32 device.  Synchronises the stream once (scene set-up routine, not
 * part of the per-view path).  With fewer than 4 points the missing neighbours count as FLT_MAX, like the original:
 * the sum and the division are float32, so P <= 2 gives +inf and P = 3 gives (d0 + d1 + FLT_MAX) / 3.  A point with a
 * NaN or an infinite coordinate gets +inf and is no neighbour of any other point (csrc/gsr_knn.h).  Known limit: the
 * grid is uniform over the bounding box, so one far (or infinite) point puts the rest into a few cells and the search
 * turns quadratic in the points that share a cell; exact still, run time not measured. */
int gsr_knn_dist2(const float* points, int32_t P, float* mean_dist2, void* stream);

/* Exact k-nearest-neighbour query WITH INDICES between two point sets, 1 <= k <= 8, and the gather-mean that the
 * reference's inpaint_setup does on the host (scene/gaussian_model.py:264-307: scipy KDTree, k = 5, numpy mean).  No
 * change of GSR_VERSION, no capability bit: the stage is present iff the library exports these two symbols.
 *
 * gsr_knn_query: ref [R,3], qry [Q,3] float32 device; out_idx [Q,k] int32 device; out_d2 [Q,k] float32 device or NULL.
 *   Distance   d2 = (dx*dx + dy*dy) + dz*dz in double from the float32 coordinates, each difference formed in double,
 *              in exactly that order without contraction (the bits of numpy float64); out_d2 is that value rounded once.
 *              Double was chosen for exactness, not from a timing.
 *   Order      a query's neighbours are the k smallest references under the total order (d2 ascending, reference index
 *              ascending), written in that order: ties are decided, the result does not depend on any scan order.
 *   Non-finite a d2 that is NaN or +inf is never a neighbour; a query with a non-finite coordinate has no neighbours; a
 *              non-finite reference is invisible to every query.
 *   Missing    with fewer than k neighbours (R < k, the excluded reference, non-finite references) the remaining slots
 *              have index -1 and d2 = +inf.  R = 0 is valid: every slot is missing and no grid is built.  Q = 0 writes
 *              nothing.
 *   flags      GSR_KNNQ_EXCLUDE_SAME_INDEX (bit 0): query i never takes reference i -- the self-query, which requires
 *              Q == R.  Any other bit is refused.
 *   Synchronises the stream once, where gsr_knn_dist2 does (the references' bounding box); workspace from the pool.
 *   Known limit, as for gsr_knn_dist2: the grid is uniform over the references' bounding box, so one far (or infinite)
 *   reference puts the rest into a few cells and the search turns quadratic in the references that share a cell; a
 *   query far outside the box scans more shells or all references.  Exact still; run time of such clouds not measured.
 *
 * gsr_knn_gather_mean: for each of n_tensors (1..8) source tensors src[t] [R, cols[t]] float32, dst[t] [Q, cols[t]]
 *   receives per element (((v0 + v1) + v2) ...) / m in float32 over the m present neighbours of idx [Q,k] in rank order,
 *   0 when m == 0.  An index outside 0 .. R-1 (-1 included) counts as missing and is never followed.  src, cols and dst
 *   are HOST arrays (of device pointers / of ints): 1 <= cols[t] <= 128 and the sum of cols <= 128.  No atomics, no wait.
 *
 * Both refuse, before the first device call: k outside 1..8, negative R or Q, a null pointer where one is needed, unknown
 * flags, EXCLUDE_SAME_INDEX with Q != R, n_tensors outside 1..8, cols outside 1..128 or summing to more than 128. */
#define GSR_KNNQ_EXCLUDE_SAME_INDEX 1u
int gsr_knn_query(const float* ref, int32_t R, const float* qry, int32_t Q, int32_t k, uint32_t flags, int32_t* out_idx,
                  float* out_d2, void* stream);
int gsr_knn_gather_mean(const int32_t* idx, int32_t Q, int32_t k, int32_t R, int32_t n_tensors, const float* const* src,
                        const int32_t* cols, float* const* dst, void* stream);

/* ---- groups set-up (C ABI 603) -----------------------------------------------------------------------------------
 * The reference's third way to set up an attack (attack.py:292-323): one Gaussian-Grouping scene, a 1x1-conv classifier
 * over the 16 object features, and the Gaussians of the selected object ids -- plus every Gaussian inside the convex
 * hull of those -- are the attacked group; the rest of the scene is the frozen background.  Semantics where the
 * reference cannot run (its points_inside_convex_hull is not defined in attack.py): INTEGRATION.md, groups mode.
 *
 * gsr_group_classify: per Gaussian, psel[i] = max over the selected ids of softmax_c(b[c] + sum_k W[c,k] objects[i,k])
 * and mask[i] = psel[i] > thresh, which is the reference's (softmax(logits)[ids] > thresh).any(0).  The logits are
 * formed in double (k = 0..15 in order) and never stored: no [C,P] buffer.  objects [P,16] float32 (the [P,1,16]
 * _objects_dc), W [C,16] float32 (a Conv2d(16, C, 1) weight), b [C] float32, psel [P] float32 and mask [P] uint8 are
 * DEVICE pointers; ids [nids] int32 is a HOST array (checked before any device call): 1 <= C <= 1024, 1 <= nids <= C,
 * every id in [0, C), no id twice.  Bitwise reproducible. */
int gsr_group_classify(const float* objects, int32_t P, const float* W, const float* b, int32_t C, const int32_t* ids,
                       int32_t nids, float thresh, float* psel, uint8_t* mask, void* stream);

/* gsr_convex_hull_planes: HOST only (no device needed).  Quickhull in double over pts [M,3] (host, double): the hull's
 * facets as planes[4 * f .. 4 * f + 3] = (nx, ny, nz, c) with a unit outward normal, so that x is inside iff
 * n . x - c <= tau for every facet, tau = 1e-9 * D, D the diagonal of the points' bounding box; bbox[6] (host) = min
 * xyz, max xyz of the points, always written (zeros for M = 0).  *nfacets = the number of facets; 0 with GSR_OK = a
 * DEGENERATE point set (fewer than 4 points, or all within tau of a point, a line or a plane; Qhull raises there).
 * Before it returns, every point is checked against every plane within tau; GSR_ERR_HULL if that fails, with no planes.
 * More than max_facets facets: GSR_ERR_NOMEM, *nfacets = the number needed and nothing written to planes (call again
 * with a buffer that size). */
int gsr_convex_hull_planes(const double* pts, int64_t M, double* planes, int64_t max_facets, int64_t* nfacets, double* bbox);

/* gsr_points_in_hull: per Gaussian, inside = xyz[i] lies within bbox grown by tau on every side AND
 * n_f . xyz[i] - c_f <= tau for every facet f, evaluated in double as ((nx*x + ny*y) + nz*z) - c with every operation
 * rounded on its own (bit for bit the host's evaluation).  xyz [P,3] float32, planes [F,4] double (from
 * gsr_convex_hull_planes), bbox [6] double, mask_in [P] uint8 or NULL, out [P] uint8: DEVICE pointers.
 * out[i] = inside, or (mask_in[i] != 0) | inside.  F = 0 (a degenerate hull): nothing is inside.  F >= 0, tau >= 0. */
int gsr_points_in_hull(const float* xyz, int32_t P, const double* planes, int32_t F, const double* bbox, double tau,
                       const uint8_t* mask_in, uint8_t* out, void* stream);

/* ---- Image front end: what sits between the renders and a detector -------------------------------------------------
 * gsr_image_resample: bilinear resize of src [B,C,H,W] to rh x rw, placed at (top, left) of dst [B,C,out_h,out_w], the
 * rest of dst filled with pad_value (a letterbox; rh = out_h, rw = out_w, top = left = 0: a plain resize).  These are
 * torch.nn.functional.interpolate's mode="bilinear", align_corners=False, size=(rh, rw) semantics.  Per axis (input
 * size `in`, resized size `out`, output index d), all in float32 with every operation rounded on its own (no fused
 * multiply-add):
 *     scale = (float)in / (float)out
 *     src   = scale * (d + 0.5f) - 0.5f;   if (src < 0) src = 0
 *     i0    = min((int)src, in - 1);       i1 = i0 + (i0 < in - 1 ? 1 : 0)
 *     l1    = clamp(src - (float)i0, 0, 1); l0 = 1 - l1
 *     value = h0*(w0*a + w1*b) + h1*(w0*c + w1*d)     a, b from row i0; c, d from row i1; a, c from column i0
 * GSR_RESAMPLE_CLAMP01: every source value is taken as v < 0 ? 0 : v > 1 ? 1 : v first.  mean / inv_std (HOST arrays of
 * C floats, read during the call; NULL = 0 / 1; both NULL: no affine at all): value -> (value - mean[c]) * inv_std[c].
 * pad_value is written as given, not normalised.
 *
 * gsr_image_resample_backward: grad_src [B,C,H,W] from grad_dst [B,C,out_h,out_w] in GATHER form.  grad_src[y,x] is the
 * sum of ((h*w) * g) terms -- the weight product rounded, the product with g rounded, then added -- over the destination
 * pixels that sample (y,x): output rows ascending, inside a row output columns ascending, inside one output pixel the
 * roles (row i0, col i0), (i0, i1), (i1, i0), (i1, i1).  A role counts only if it names (y,x); at the clamped last row or
 * column i0 and i1 name the same pixel and both terms count.  The total is multiplied by inv_std[c] under the affine and
 * by (0 <= v && v <= 1) under GSR_RESAMPLE_CLAMP01 (torch.clamp's inclusive mask; a NaN source gives 0; src is read
 * only then and may be NULL otherwise).  Every source pixel is written exactly once (zero where nothing samples it), or
 * added to what grad_src holds when accumulate != 0: no memset, no atomics, the same bits on every run.  16-byte stores
 * when W % 4 == 0 and the tensors start on 16-byte boundaries.
 *
 * gsr_image_to_u8: src [B,3,H,W] float -> dst [B,H,W,3] uint8, (uint8)(clamp(v,0,1) * 255.0f) with truncation, NaN -> 0:
 * integer-equal to (x.clamp(0,1) * 255).byte().permute(0,2,3,1) for finite input.
 *
 * All three: src, dst, grad_* are DEVICE pointers; 1 <= C <= 4; every size >= 1; 0 <= top, top + rh <= out_h, 0 <= left,
 * left + rw <= out_w; at most 2^31 - 1 elements per tensor.  Violations return GSR_ERR_INVALID before any device call.
 * One kernel launch on `stream`, no allocation, no copy, no host synchronisation: capturable and re-entrant. */
#define GSR_RESAMPLE_CLAMP01 1u
typedef struct GsrResample {
  int32_t B, C, H, W;        /* source [B,C,H,W], 1 <= C <= 4 */
  int32_t out_h, out_w;      /* destination [B,C,out_h,out_w] */
  int32_t rh, rw, top, left; /* resized image and where it sits in the destination */
  float pad_value;
  const float* mean;         /* HOST, C floats, or NULL (0) */
  const float* inv_std;      /* HOST, C floats, or NULL (1) */
  uint32_t flags;
} GsrResample;
int gsr_image_resample(const GsrResample* spec, const float* src, float* dst, void* stream);
int gsr_image_resample_backward(const GsrResample* spec, const float* src, const float* grad_dst, float* grad_src,
                                int32_t accumulate, void* stream);
int gsr_image_to_u8(const float* src, int32_t B, int32_t H, int32_t W, uint8_t* dst, void* stream);

/* ---- Detector output stage: what sits behind a detector's network ----------------------------------------------------
 * The reference runs this per view in host Python (predict_and_save of each detector wrapper under detectors/: score filter,
 * ultralytics' NMS, torchvision's box_iou, an argmax and a Python bool).  Here it is four entries whose results are
 * fixed bit for bit; csrc/gsr_detect.h holds the arithmetic, compiled for the kernels and for a host harness alike.
 *
 * gsr_det_postprocess: raw head output `pred` -> dets [B,max_det,6] (x1 y1 x2 y2 score class-as-float) and
 * counts [B,2] (kept, above_thr).
 *   Candidates.  One per anchor: score_c = cls_c, or with has_obj the single rounded float32 product obj * cls_c; the
 *   anchor's class is the first maximum of score_c over c (lowest index on ties; a NaN score_c is never the maximum; if
 *   no class compares above -inf the anchor has class 0 and score -inf), its score that maximum.  The anchor is a
 *   candidate iff score > conf_thr, so a NaN score is dropped.  With has_obj, ultralytics also tests obj > conf_thr on
 *   its own; for class scores in [0,1] the product cannot exceed obj, so that test is implied and is not made here.  One
 *   label per anchor: ultralytics' multi_label mode (one candidate per class above the threshold) is not provided.
 *   counts[b,1] is the number of candidates before any cap; if it exceeds max_candidates the first max_candidates of the
 *   order below are kept, whatever the launch geometry.
 *   Order, within an image: score descending (-0 and +0 equal), then anchor index ascending -- a total order, so every
 *   output is identical on every run.
 *   Boxes.  box_format 0: x1 = xc - w*0.5f, y1 = yc - h*0.5f, x2 = xc + w*0.5f, y2 = yc + h*0.5f; 1: as given.
 *   IoU, float32, every operation rounded on its own (no fused multiply-add), torchvision's box_iou:
 *       area = (x2 - x1) * (y2 - y1)
 *       iw = max(min(ax2,bx2) - max(ax1,bx1), 0);  ih likewise;  inter = iw * ih
 *       iou = inter / ((area_a + area_b) - inter)
 *   NMS.  Greedy in the order above: a box is suppressed iff an earlier KEPT box has iou > iou_thr (strict; a NaN IoU,
 *   from 0/0, suppresses nothing) and -- unless GSR_DET_CLASS_AGNOSTIC -- the same class integer.  ultralytics instead
 *   shifts every box by class * 7680 and runs an agnostic NMS: boxes of different classes then never overlap, and boxes
 *   of one class overlap as before up to the rounding of the shifted coordinates; the integer compare is that rule
 *   without the rounding.  The walk stops after max_det keeps; counts[b,0] is their number.
 *   Output.  Kept boxes in walk order, mapped x' = (x - ox) * sx, y' = (y - oy) * sy (each operation rounded on its
 *   own; ox = oy = 0, sx = sy = 1 leaves them as they are), the score and the class; rows beyond counts[b,0] are zero.
 *   ws: gsr_det_workspace_bytes(spec) bytes of device memory, 8-byte aligned, scratch for the duration of the call's
 *   kernels.  Three launches on `stream`.
 *
 * gsr_det_nms: the same order and walk on caller boxes [B,n,4] (x1 y1 x2 y2), scores [B,n] and classes [B,n] (NULL:
 * agnostic); entries at or beyond n_valid[b] (NULL: n) do not take part.  1 <= n <= 4096, 1 <= max_det <= n.  Scores
 * order by their float comparison; NaN scores order by their bit image (above +inf with a clear sign bit, below -inf
 * with a set one).  keep [B,max_det]: indices into the n entries in walk order, -1 beyond counts[b].  ws: what
 * gsr_det_workspace_bytes reports for a spec with this B, A = max_candidates = n and this max_det.  Two launches.
 *
 * gsr_det_box_iou: iou [n,m] of boxes a [n,4] against b [m,4] (x1 y1 x2 y2), the arithmetic above.  One launch.
 *
 * gsr_det_verdict: the reference's success test (yolov5_detector.py:175-193, 239-245) for every image of a batch.
 * dets / counts as gsr_det_postprocess writes them (counts [B,2]; only counts[b,0] is read, clamped to 0..max_det).
 * gt [B,4] x1 y1 x2 y2 in the frame of dets; gt == NULL or a row holding a NaN: that image has no gt box.
 *   with a gt box and rows: best = the first maximum of IoU(row, gt) over the kept rows, a NaN IoU counting as 0;
 *       target_exists = best_iou > iou_match && class == target
 *       untarget_absent = !(best_iou > iou_match && class == untarget)
 *   without a gt box: target_exists = some kept class equals target; untarget_absent = none equals untarget
 *   with no rows: target_exists = false, untarget_absent = true
 * untarget < 0: none.  verdict[b]: bit 0 = success (is_targeted: target_exists && (untarget < 0 || untarget_absent);
 * otherwise untarget_absent), bit 1 = target_exists, bit 2 = untarget_absent.  best [B,4]: (iou, score, class, row) of
 * that best row, all -1 where there is none (no gt box or no rows).  The reference compares against 0.5; pass it as
 * iou_match.  One launch, one wave per image.
 *
 * All entries: every tensor argument is a DEVICE pointer.  Sizes < 1, max_candidates > 4096, max_det > max_candidates
 * (gsr_det_nms: n > 4096, max_det > n), layout / has_obj / box_format outside {0,1}, unknown flags, a workspace that
 * is too small or not 8-byte aligned, a NULL required pointer, or more than 2^31 - 1 elements in a tensor return
 * GSR_ERR_INVALID with a gsr_last_error text before any device call.  No allocation, no copy, no host synchronisation:
 * everything is enqueued on `stream`; calls are re-entrant from several host threads (each with its own workspace). */
#define GSR_DET_CLASS_AGNOSTIC 1u
typedef struct GsrDetSpec {
  int32_t B, A, C;           /* images, anchors per image, classes; all >= 1 */
  int32_t layout;            /* 0: pred[B, A, 4+has_obj+C] (YOLOv3/v5);  1: pred[B, 4+has_obj+C, A] (YOLOv8/v11) */
  int32_t has_obj;           /* 1: channel 4 is objectness, score = obj * cls (one rounded float32 product); 0: score = cls */
  int32_t box_format;        /* 0: (xc, yc, w, h) -> x1 = xc - w*0.5f, x2 = xc + w*0.5f, ...;  1: (x1, y1, x2, y2) */
  float   conf_thr, iou_thr;
  int32_t max_candidates;    /* 1 .. 4096 */
  int32_t max_det;           /* 1 .. max_candidates */
  uint32_t flags;            /* GSR_DET_CLASS_AGNOSTIC */
  float   ox, oy, sx, sy;    /* after NMS: x' = (x - ox) * sx, y' = (y - oy) * sy, each operation rounded on its own */
} GsrDetSpec;
int gsr_det_workspace_bytes(const GsrDetSpec* spec, int64_t* bytes);
int gsr_det_postprocess(const GsrDetSpec* spec, const float* pred, void* ws, int64_t ws_bytes, float* dets, int32_t* counts,
                        void* stream);
int gsr_det_nms(int32_t B, int32_t n, const float* boxes, const float* scores, const int32_t* classes, const int32_t* n_valid,
                float iou_thr, int32_t max_det, void* ws, int64_t ws_bytes, int32_t* keep, int32_t* counts, void* stream);
int gsr_det_box_iou(const float* a, int32_t n, const float* b, int32_t m, float* iou, void* stream);
int gsr_det_verdict(const float* dets, const int32_t* counts, int32_t B, int32_t max_det, const float* gt, int32_t target,
                    int32_t untarget, int32_t is_targeted, float iou_match, int32_t* verdict, float* best, void* stream);

/* ---- Detection metrics: COCO-style matching, AP / AR and the summary ----------------------------------------------------
 * The reference scores an attack on the host (utils/render.py:223-298 dumps COCO JSON, utils/analyze_ap_ar.py runs
 * pycocotools.COCOeval on it).  These three entries are COCOeval's evaluateImg, accumulate and summarize for boxes, on the
 * device, from the dets [B,D,6] (x1 y1 x2 y2 score class) and counts [B,2] every detector output stage writes.  No change of
 * GSR_VERSION, no capability bit, no gsr_query item: the stage is present iff the library exports gsr_deteval_match.
 *
 * Arithmetic (csrc/gsr_deteval.h, compiled for kernels and host alike): everything is DOUBLE.  Float32 inputs are widened
 * once; every operation is rounded on its own, no contraction, no library call -- the same bits on every run and every build.
 *   live rows    a detection row is live iff its index is below counts[b,0] (clamped to 0..D), none of its six floats is a NaN
 *                and its class float is an integer in 0..K-1.  A ground-truth row (gt_boxes [B,M,4], gt_cls [B,M] int32) is
 *                live iff its class is in 0..K-1 and its box holds no NaN.  Dead rows take part in nothing.
 *   area, IoU    area = (x2-x1)*(y2-y1); iw = min(ax2,bx2) - max(ax1,bx1), ih likewise; inter = (iw <= 0 || ih <= 0) ? 0 : iw*ih;
 *                iou = inter / ((area_d + area_g) - inter); a NaN IoU counts as 0 (a deviation: COCOeval would match it).
 *   orders       detections of an image: score descending, then row ascending, -0 == +0 (COCOeval's stable mergesort).
 *                Ground truth under area range a: rows with area in [lo_a, hi_a] first, ignored rows (area < lo_a ||
 *                area > hi_a) after them, each part in row order.  No crowd, no `ignore` flag.
 *   the walk     per area range a, threshold t, detection d in order: best = min(iou_thrs[t], 1 - 1e-10), m = none; through the
 *                live ground truth of d's class in the order above: a row already matched under (a,t) is skipped; if m is set
 *                and counted and this row is ignored, stop; iou < best: continue; else best = iou, m = row (a later row of
 *                equal IoU replaces an earlier one).  A matched d takes dt_ignore = its row's ignore; an unmatched d is ignored
 *                iff its own area is outside [lo_a, hi_a].
 *   accumulate   per class k, area a, cap max_dets[m]: the live detections of class k whose dt_rank < max_dets[m], over all
 *                images, by score descending, then image ascending, then rank ascending.  npig[k,a] = live counted rows of
 *                class k.  npig == 0: every output of (k,a,m) is -1.  Else tp / fp = cumulative counts over the detections that
 *                are not ignored (matched / unmatched), rc = tp / npig, pr = tp / ((fp + tp) + 2.220446049250313e-16);
 *                recall[t,k,a,m] = the last rc (0 with no detections); pr is made non-increasing from the back; for each
 *                rec_thrs[r] the first index with rc >= rec_thrs[r] gives precision[t,r,k,a,m] = pr and scores[t,r,k,a,m] = the
 *                score there, both 0 past the end.  The comparison sees the caller's doubles: the library generates no threshold.
 *   summarize    stats[14]: COCOeval.summarize's twelve -- AP over all thresholds / at the threshold equal to 0.5 / equal to
 *                0.75 (area 0, last cap), AP for areas 1, 2, 3 (last cap), AR for caps 0, 1, 2 (area 0), AR for areas 1, 2, 3
 *                (last cap) -- then the reference's AP (all thresholds, area 0, last cap) and AR (area 0, cap 0).  Each is the
 *                mean of the slice's entries above -1, added in index order ([t,r,k] / [t,k]), or -1 when there are none, when
 *                no threshold equals 0.5 / 0.75, or when the area range or cap does not exist.  Areas and caps go by POSITION.
 *
 * gsr_deteval_match, one batch of B images (B * D <= 2^20), one launch, one workgroup per image.  Writes
 *   dt_order [B,D] int32    the live rows in order, -1 beyond them          dt_rank [B,D] int32   rank within image and class, -1
 *   dt_match [B,A,T,D] int32  per POSITION of dt_order: the matched ground-truth row or -1
 *   dt_ignore [B,A,T,D] uint8 per position: 1 ignored, 0 not (0 beyond the live rows)
 *   gt_ignore [B,A,M] uint8   0 counted, 1 ignored by area, 2 a dead row    gt_match [B,A,T,M] int32  position in dt_order or -1
 *   With M == 0 the four ground-truth pointers are not read and may be NULL.
 * gsr_deteval_accumulate, over the concatenated outputs of N images (N * D <= 2^20; dets as given to the match).  rec_thrs [R]
 *   doubles on the DEVICE.  Writes precision and scores [T,R,K,A,Mx] double, recall [T,K,A,Mx] double, npig [K,A] int32.  ws:
 *   device, 16-byte aligned, gsr_deteval_workspace_bytes(spec, N) bytes.  Two stable radix sorts of 32-bit keys (score, then
 *   class), a scan of the class histogram, then one wave per (k,a,m,t).
 * gsr_deteval_summarize: one launch; stats [14] double on the device.
 *
 * All entries: every tensor argument is a DEVICE pointer, the spec a HOST struct.  A NULL spec or required pointer, K outside
 * 1..65535, D outside 1..4096, M outside 0..256, T outside 1..10, A outside 1..4, R outside 1..1024, n_caps outside 1..3, caps
 * that descend or lie outside 1..D, a NaN among iou_thrs / area bounds, B or N < 1, more than 2^20 detection rows, a misaligned
 * tensor (4 bytes; doubles 8), a workspace too small or misaligned return GSR_ERR_INVALID with a gsr_last_error text before
 * any device call.  No allocation, no copy, no host synchronisation: everything is enqueued on `stream`; calls are re-entrant
 * from several host threads (each with its own workspace). */
typedef struct GsrDetEvalSpec {
  int32_t K, D, M;           /* classes, detection rows per image, ground-truth rows per image */
  int32_t T, A, n_caps;      /* IoU thresholds, area ranges, max_dets in use */
  int32_t max_dets[3];       /* ascending (equal caps are allowed), each 1..D */
  int32_t R;                 /* recall thresholds */
  double  iou_thrs[10];
  double  area_lo[4], area_hi[4];
} GsrDetEvalSpec;
int gsr_deteval_workspace_bytes(const GsrDetEvalSpec* spec, int64_t N, int64_t* bytes);
int gsr_deteval_match(const GsrDetEvalSpec* spec, int32_t B, const float* dets, const int32_t* counts, const float* gt_boxes,
                      const int32_t* gt_cls, int32_t* dt_order, int32_t* dt_rank, int32_t* dt_match, uint8_t* dt_ignore,
                      uint8_t* gt_ignore, int32_t* gt_match, void* stream);
int gsr_deteval_accumulate(const GsrDetEvalSpec* spec, int64_t N, const float* dets, const int32_t* dt_order, const int32_t* dt_rank,
                           const int32_t* dt_match, const uint8_t* dt_ignore, const int32_t* gt_cls, const uint8_t* gt_ignore,
                           const double* rec_thrs, void* ws, int64_t ws_bytes, double* precision, double* scores, double* recall,
                           int32_t* npig, void* stream);
int gsr_deteval_summarize(const GsrDetEvalSpec* spec, const double* precision, const double* recall, double* stats, void* stream);

/* ---- Detector loss stage: the anchor-free YOLO detection loss and its gradient -----------------------------------------
 * The reference's four YOLO wrappers end infer() by calling the ultralytics DetectionModel in training mode
 * (detectors/yolov8_detector.py:140-156): a task-aligned assigner, BCE on the class logits, CIoU on the decoded boxes
 * and the distribution focal loss (DFL) on the 4 x 16 distance bins, returned as box*7.5 + cls*0.5 + dfl*1.5.
 * gsr_detloss computes that loss and d total / d pred in four launches.  The formulas below are the specification
 * (written from ultralytics 8.x's v8DetectionLoss, TaskAlignedAssigner and bbox_iou; INTEGRATION.md lists the stated
 * deviations); csrc/gsr_detloss.h holds the arithmetic, compiled for the kernels and for a host harness alike.  All
 * arithmetic is float32, index-valued results are int32.
 *
 * Inputs.  pred [B, 64 + C, A] (channel-major: channels 0..63 are the sides l, t, r, b x 16 bins, channels 64.. the
 * class logits; ultralytics' cat(feats, 2)).  The levels: nl <= 5 entries (h_i, w_i, stride_i) with sum h_i * w_i = A;
 * anchor a of level i at row y, column x has the grid point (gx, gy) = (x + 0.5, y + 0.5) and the pixel point
 * p = grid * stride_i -- derived by the kernels, there is no anchor tensor.  gt_boxes [B, M, 4]: x1 y1 x2 y2 in
 * network-input pixels; gt_cls [B, M] int32; 1 <= M <= 32.  A row is PRESENT iff 0 <= gt_cls < C: gt_cls lives in device
 * memory, so a class >= C cannot be refused without a device read and the row is treated as absent, like a negative one.
 *
 * Decode.  Per anchor and side: d = sum_k k * softmax(bins)_k (max-subtracted); the predicted box in grid units is
 * (gx - d_l, gy - d_t, gx + d_r, gy + d_b); times the stride: pixels.
 *
 * CIoU(b1, b2), eps = 1e-7:
 *     w1 = b1.x2 - b1.x1        h1 = b1.y2 - b1.y1 + eps        (w2, h2 alike)
 *     inter = max(min(x2s) - max(x1s), 0) * max(min(y2s) - max(y1s), 0)
 *     union = w1*h1 + w2*h2 - inter + eps;   iou = inter / union
 *     cw, ch = extent of the enclosing box;  c2 = cw^2 + ch^2 + eps
 *     rho2 = ((b2.x1 + b2.x2 - b1.x1 - b1.x2)^2 + (b2.y1 + b2.y2 - b1.y1 - b1.y2)^2) / 4
 *     v = 4/pi^2 * (atan(w2/h2) - atan(w1/h1))^2;   a = v / (v - iou + (1 + eps));   ciou = iou - (rho2/c2 + v*a)
 * `a` is a constant in the backward; a max / min of two equal arguments shares its gradient in halves and the clamp at 0
 * passes it where its argument is >= 0, as torch does.
 *
 * Assignment (nothing here is differentiated).  Per image and present row m:
 *   candidate:  anchor a iff min(p.x - x1, p.y - y1, x2 - p.x, y2 - p.y) > 1e-9
 *   for candidates: ov[m,a] = max(CIoU(gt, pred_px), 0), s = sigmoid(logit[cls_m, a]), metric[m,a] = s^alpha * ov^beta;
 *               both are 0 for non-candidates
 *   top-k:      the candidates ordered by metric descending, then anchor index ascending; the first
 *               min(topk, #candidates) are positive for m (where torch.topk is arbitrary among equal metrics, the anchor
 *               index decides here)
 *   conflict:   an anchor positive for more than one row goes to the row with the largest ov[m,a] over ALL present rows
 *               (the lowest m on ties); as in the library, that row need not be one whose top-k held the anchor
 *   result:     tgt[b,a] = the row, or -1 for background; for foreground, with pos(m) the final positives of row m,
 *               ts[b,a] = metric[m,a] * max_{a' in pos(m)} ov[m,a'] / (max_{a' in pos(m)} metric[m,a'] + 1e-9); 0 elsewhere
 *   tss = max(sum_{b,a} ts, 1), over the whole batch
 *
 * Loss.
 *   cls = sum_{b,c,a} BCEWithLogits(x, t) / tss, t = ts[b,a] at the row's class of a foreground anchor, 0 elsewhere, in
 *         the stable form max(x,0) - x*t + log1p(exp(-|x|))
 *   box = sum_fg (1 - CIoU(pred_grid, gt_grid)) * ts / tss, both boxes in grid units, gt_grid = gt / stride
 *   dfl = sum_fg ts * 1/4 sum_sides [CE(bins, tl) * wl + CE(bins, tl+1) * wr] / tss, the target distance being
 *         clamp(side distance of gt_grid from the grid point, 0, 14.99), tl = floor(target), wl = tl + 1 - target,
 *         wr = 1 - wl
 *   total = B * (w_box*box + w_cls*cls + w_dfl*dfl)
 *
 * Outputs.  loss[4] = (box, cls, dfl, total), the first three unweighted.  grad_pred [B, 64+C, A] = d total / d pred, or
 * NULL (the loss bits are the same either way); when given, every element is written exactly once, background anchors
 * getting zeros in their 64 box channels.  Optional tgt [B,A] int32 and ts [B,A] float32.
 *
 * Determinism.  Every sum is taken in an order fixed by the sizes (and by whether the 16-byte path runs: A % 4 == 0 with
 * pred and grad_pred on 16-byte boundaries) alone -- per-thread runs, LDS trees, per-block partials added by one block --
 * and there are no float atomics: two calls on the same input give the same bits, on any stream and from any host thread
 * (each with its own workspace).  No allocation, no copy, no host synchronisation: capturable.  Non-finite pred gives
 * unspecified floats, but every index stays in range and every loop ends.
 *   ws: gsr_detloss_workspace_bytes(spec) bytes of device memory, 16-byte aligned, scratch for the duration of the call's
 *   kernels.
 * B, A, C < 1, B > 65535, M outside 1..32, nl outside 1..5, a level with a size < 1 or a stride that is not finite and
 * > 0, levels that do not add up to A, reg_max != 16, topk outside 1..16, a negative or non-finite alpha / beta / weight,
 * non-zero flags, a workspace that is too small or misaligned, a NULL required pointer, or more than 2^31 - 1 elements
 * in a tensor return GSR_ERR_INVALID with a gsr_last_error text before any device call. */
typedef struct GsrDetLossSpec {
  int32_t B, A, C, M, nl;    /* images, anchors per image, classes, gt rows per image (1..32), levels (1..5) */
  int32_t level_h[5], level_w[5];
  float   level_stride[5];
  int32_t reg_max;           /* 16 */
  int32_t topk;              /* 1..16; ultralytics: 10 */
  float   alpha, beta;       /* ultralytics: 0.5, 6.0 */
  float   w_box, w_cls, w_dfl; /* ultralytics: 7.5, 0.5, 1.5 */
  uint32_t flags;            /* 0 */
} GsrDetLossSpec;
int gsr_detloss_workspace_bytes(const GsrDetLossSpec* spec, int64_t* bytes);
int gsr_detloss(const GsrDetLossSpec* spec, const float* pred, const float* gt_boxes, const int32_t* gt_cls, void* ws,
                int64_t ws_bytes, float* loss, float* grad_pred, int32_t* tgt, float* ts, void* stream);

/* ---- Set-prediction (DETR-style) detector stage: matching, set criterion, output ------------------------------------------
 * The reference's second detector family (detectors/detr_detector.py) emits Q queries per image, each with C + 1 logits
 * whose LAST entry is "no object" and a box (cx, cy, w, h) normalised to the image.  Its infer() hands DETR's set
 * criterion to backward() (:98-115): a one-to-one match of ground-truth rows to queries, then weighted cross-entropy, L1
 * and GIoU; its success test is a softmax, a threshold and an IoU, without NMS (:186-243).  gsr_setdet_loss computes the
 * match, the loss and its gradients in four launches, gsr_setdet_postprocess the detections in one.  The formulas below
 * are the specification (written from the published DETR HungarianMatcher, SetCriterion and box_ops.generalized_box_iou;
 * INTEGRATION.md lists the stated deviations); csrc/gsr_setdet.h holds the arithmetic, compiled for the kernels and for a
 * host harness alike.  All arithmetic is float32, every operation rounded on its own; index-valued results are int32.
 *
 * Inputs.  logits [B, Q, C + 1] (channel C: no object); boxes [B, Q, 4] (cx, cy, w, h) normalised, what the head emits
 * after its sigmoid; gt_boxes [B, M, 4]: x1 y1 x2 y2 in pixels of a frame of size (img_w, img_h) -- gsr_detloss's box
 * format; gt_cls [B, M] int32.  A row is PRESENT iff 0 <= gt_cls < C (gt_cls lives in device memory, so another value
 * cannot be refused without a device read: the row is absent).  Ground truth is normalised by the stage:
 *     cx = (x1 + x2) * 0.5f / img_w    w = (x2 - x1) / img_w    (cy, h alike with img_h)
 * 1 <= B <= 65535, 1 <= Q <= 1024, 1 <= C <= 1024, 1 <= M <= 32, Q >= M.
 *
 * xyxy(b) = (cx - 0.5f*w, cy - 0.5f*h, cx + 0.5f*w, cy + 0.5f*h).
 * GIoU(a, b) on xyxy, no epsilon (as published):
 *     area = (x2 - x1) * (y2 - y1)
 *     inter = max(min(x2s) - max(x1s), 0) * max(min(y2s) - max(y1s), 0)
 *     union = area_a + area_b - inter;   iou = inter / union
 *     encl = max(max(x2s) - min(x1s), 0) * max(max(y2s) - min(y1s), 0)
 *     giou = iou - (encl - union) / encl
 *
 * Cost, per image, query q and present row m, with p = softmax(logits[q]) (max-subtracted, p_c = exp(x_c - max) / sum):
 *     cost[m,q] = -c_class * p[cls_m] + c_l1 * sum_4 |box_q - gt_m| + -c_giou * GIoU(xyxy(box_q), xyxy(gt_m))
 * (DETR: c_class = 1, c_l1 = 5, c_giou = 2.)
 *
 * Match (nothing here is differentiated): every present row gets a distinct query such that the sum of cost is minimal,
 * by shortest augmenting paths with dual potentials.  Columns are 1..Q (column j is query j - 1) and a virtual column 0,
 * rows 1..M.  u[0..M] = 0, v[0..Q] = 0, p[0..Q] = 0 (the row held by a column, 0: free).  For every present row i in
 * ascending order:
 *     p[0] = i; j0 = 0; minv[j] = +inf, way[j] = 0, all columns unmarked
 *     repeat:  mark j0; i0 = p[j0]
 *              for every unmarked column j = 1..Q:  cur = (cost[i0,j] - u[i0]) - v[j];
 *                  if cur < minv[j]: minv[j] = cur, way[j] = j0
 *              (delta, j1) = the smallest minv[j] over the unmarked columns, the LOWEST j among equal values
 *              if no minv[j] compares below +inf: j1 = the lowest unmarked column, delta = 0
 *              marked columns j: u[p[j]] += delta, v[j] -= delta;   unmarked: minv[j] -= delta
 *              j0 = j1
 *     until p[j0] == 0 (at most M + 1 passes: every pass marks one more column, and marked columns hold rows)
 *     then, at most M + 1 times while j0 != 0:  j1 = way[j0]; p[j0] = p[j1]; j0 = j1
 * This fixes the result among assignments of equal cost, where scipy.optimize.linear_sum_assignment leaves it open.
 * match[b,m] = the query of row m, -1 for an absent row; tgt[b,q] = the row of query q, -1 for an unmatched one.  Every
 * loop is bounded by M and Q alone: with non-finite costs the result is unspecified, but every index stays in range and
 * every loop ends.
 *
 * Loss.  t(b,q) = the class of the matched row, C for an unmatched query; wt = 1 for every class, eos_coef for C (DETR:
 * 0.1); n = max(number of present rows in the batch, 1); W = sum_{b,q} wt[t], taken as
 * (float)matched + eos_coef * (float)(B*Q - matched).
 *     ce    = sum_{b,q} wt[t] * -(x_t - max - log(sum)) / W
 *     l1    = sum_matched sum_4 |box_q - gt_m| / n
 *     giou  = sum_matched (1 - GIoU(xyxy(box_q), xyxy(gt_m))) / n
 *     total = w_ce*ce + w_l1*l1 + w_giou*giou                   (DETR: 1, 5, 2)
 * loss[4] = (ce, l1, giou, total), the first three unweighted.  eos_coef = 0 with no present row divides 0 by 0, as the
 * published code does.
 *
 * Backward (hand-written).  grad_logits [B,Q,C+1] = d total / d logits = (w_ce / W * wt[t]) * (p_c - [c == t]);
 * grad_boxes [B,Q,4] = d total / d boxes: sign(0) = 0; a max or min of two equal arguments shares its gradient in halves;
 * a clamp at 0 passes it where its argument is >= 0, as torch does; unmatched queries get zeros.  Either may be NULL (the
 * loss bits are the same either way); when given, every element is written exactly once.  match [B,M] and tgt [B,Q] are
 * optional outputs.
 *
 * Determinism.  Every sum is taken in an order fixed by the sizes alone -- per-thread runs, wave butterflies, LDS trees,
 * per-block partials added by one block -- and there are no float atomics: two calls on the same input give the same
 * bits, on any stream and from any host thread (each with its own workspace).  No allocation, no copy, no host
 * synchronisation: capturable.
 *   ws: gsr_setdet_workspace_bytes(spec) bytes of device memory, 16-byte aligned, scratch for the duration of the call's
 *   kernels.
 *
 * gsr_setdet_postprocess (detr_detector.py:186-202): per query p = softmax(logits); the class is the first maximum of p_c
 * over c < C (lowest index on ties; a NaN is never the maximum), the score that maximum; the query is kept iff
 * score > conf_thr, so a NaN score is dropped.  Box: x1 = (cx - 0.5f*w) * img_w, x2 = (cx + 0.5f*w) * img_w, y alike with
 * img_h.  Kept queries are written in QUERY ORDER (the reference does not sort and its argmax takes the first best IoU);
 * no NMS.  dets [B,max_det,6] (x1 y1 x2 y2 score class-as-float) and counts [B,2] (kept = min(above_thr, max_det),
 * above_thr), the layout gsr_det_postprocess writes; rows beyond the count are zero.  gsr_det_verdict on them gives the
 * reference's verdict (:216-243).  One launch, no workspace.  M and the loss weights are checked but not used.
 *
 * All entries: every tensor argument is a DEVICE pointer.  A size out of range, Q < M, max_det outside 1..1024, a
 * non-finite or negative c_* / w_* / eos_coef, a frame size that is not finite and > 0, non-zero flags, a workspace that
 * is too small or misaligned, a NULL required pointer, a tensor that is not 4-byte aligned or more than 2^31 - 1 logits
 * return GSR_ERR_INVALID with a gsr_last_error text before any device call. */
typedef struct GsrSetDetSpec {
  int32_t B, Q, C, M;        /* images, queries per image (1..1024), classes without "no object" (1..1024), gt rows (1..32) */
  float   img_w, img_h;      /* the frame gt_boxes and dets are in */
  float   c_class, c_l1, c_giou; /* matching cost; DETR: 1, 5, 2 */
  float   w_ce, w_l1, w_giou;    /* loss weights; DETR: 1, 5, 2 */
  float   eos_coef;          /* weight of the no-object class; DETR: 0.1 */
  float   conf_thr;          /* gsr_setdet_postprocess; the reference: 0.7 */
  int32_t max_det;           /* gsr_setdet_postprocess: rows of dets per image, 1..1024 */
  uint32_t flags;            /* 0 */
} GsrSetDetSpec;
int gsr_setdet_workspace_bytes(const GsrSetDetSpec* spec, int64_t* bytes);
int gsr_setdet_loss(const GsrSetDetSpec* spec, const float* logits, const float* boxes, const float* gt_boxes,
                    const int32_t* gt_cls, void* ws, int64_t ws_bytes, float* loss, float* grad_logits, float* grad_boxes,
                    int32_t* match, int32_t* tgt, void* stream);
int gsr_setdet_postprocess(const GsrSetDetSpec* spec, const float* logits, const float* boxes, float* dets, int32_t* counts,
                           void* stream);

/* ---- Two-stage (R-CNN-style) detector stage: proposal sampler, RoIAlign, box-head loss, output ------------------------------
 * The reference's default detector is Detectron2's Faster R-CNN in its C4 form (detectors/detectron2_detector.py with
 * Base-RCNN-C4.yaml): Res5ROIHeads on one stride-16 feature map, a 14 x 14 aligned RoIAlign with adaptive sampling, and
 * infer() descends on loss_cls alone.  Five entries carry what sits around the network's own layers: gsr_rcnn_sample
 * (label_and_sample_proposals, made deterministic), gsr_roi_align and gsr_roi_align_backward (ROIAlignV2, the backward a
 * gather), gsr_rcnn_loss (FastRCNNOutputLayers.losses with its gradient) and gsr_rcnn_postprocess (fast_rcnn_inference).
 * The formulas below are the specification (written from the published Detectron2 sources; INTEGRATION.md lists the stated
 * deviations); csrc/gsr_rcnn.h holds the arithmetic, compiled for the kernels and for a host harness alike.  All
 * arithmetic is float32, every operation rounded on its own; index-valued results are int32.  One GsrRcnnSpec serves all
 * entries; each checks the members it names below and ignores the others.  Proposals are an input: the RPN's own proposal
 * generation (the RPN proposal stage below) and masks are not part of this stage; pooling from a feature pyramid is the
 * FPN RoI pooler's and the two RPN losses the RPN loss stage's, both further below.
 *
 * gsr_rcnn_sample (members B, R, M, S, C, max_pos, append_gt, seed, fg_iou).  proposals [B,R,4]: x1 y1 x2 y2 in pixels, in
 * the proposer's order; n_prop [B] int32 or NULL (= R; clamped to 0..R); gt_boxes [B,M,4]; gt_cls [B,M] int32, a row being
 * PRESENT iff 0 <= gt_cls < C as in the other stages.  1 <= M <= 32, 1 <= S <= 1024 (Detectron2: 512), 0 <= max_pos <= S
 * (Detectron2: 128), R >= 1, R + M <= 4096, 1 <= C <= 1024.
 *   Candidates.  Candidate i < R is proposal i, valid iff i < n_prop[b]; with append_gt != 0 (Detectron2: on) candidate
 *   R + m is ground-truth row m, valid iff the row is present.
 *   IoU of a candidate against row m (Detectron2's pairwise_iou): areas and intersection as in gsr_det_box_iou,
 *       iou = inter > 0 ? inter / ((area_a + area_b) - inter) : 0
 *   Match: the first maximum over the present rows in ascending m (the lowest m wins ties; a NaN is never the maximum).  The
 *   candidate is FOREGROUND iff that maximum is >= fg_iou (non-strict, as Matcher is; Detectron2: 0.5) and then has its
 *   row's class; every other valid candidate -- all of them when no row is present -- is BACKGROUND, class C.
 *   Quota.  n_pos = min(#foreground, max_pos);  n_neg = min(#background, S - n_pos).
 *   Choice.  Where Detectron2 draws a randperm, each kind is ordered by (key, i) ascending and its first n_pos / n_neg taken:
 *       mix32(x):  x ^= x >> 16;  x *= 0x7feb352d;  x ^= x >> 15;  x *= 0x846ca68b;  x ^= x >> 16        (uint32)
 *       key(b, i) = mix32(mix32(seed ^ (uint32)b * 0x9E3779B9) + (uint32)i)
 *   The same seed gives the same sample on every run; a caller who wants a fresh draw per step changes seed.
 *   Outputs, the taken candidates in ASCENDING CANDIDATE INDEX: idx [B,S] (-1 beyond the count), rois [B,S,4] (the gathered
 *   boxes, zero rows beyond), labels [B,S] (the class, C for background, -1 beyond), gt_row [B,S] (the matched row, -1 for
 *   background and beyond), counts [B,2] = (taken, foreground taken).  Every element of every output is written.  With NaN
 *   boxes the result is unspecified, but every index stays in range and every loop ends.  One launch, one workgroup per image.
 *
 * gsr_roi_align (members B, S, Cf, Hf, Wf, PH, PW, spatial_scale, sampling_ratio): ROIAlignV2, aligned = True.
 * features [B,Cf,Hf,Wf]; rois [B,S,4] in image pixels; n_roi: NULL (= S) or int32, image b's count at
 * n_roi[b * n_roi_stride] (clamped to 0..S; gsr_rcnn_sample's counts with stride 2); pooled [B,S,Cf,PH,PW].
 * 1 <= B, Cf <= 65535, 1 <= S <= 1024, 1 <= PH, PW <= 14, sampling_ratio >= 0, spatial_scale finite and > 0 (the C4 model:
 * 1/16).  Per axis (x shown):
 *       start = x1 * scale - 0.5f;  end = x2 * scale - 0.5f;  len = end - start  (no clamp to 1);  bin = len / PW
 *       grid = sampling_ratio > 0 ? sampling_ratio : ceil(len / PW), clamped to 0..16
 *   count = max(grid_h * grid_w, 1).  Sample (iy, ix) of bin (ph, pw): y = start_h + ph * bin_h + (iy + 0.5f) * bin_h / grid_h,
 *   x alike.  The bilinear read is 0 when y < -1 || y > Hf || x < -1 || x > Wf; otherwise y = max(y, 0), y_low = (int)y; if
 *   y_low >= Hf - 1 both rows are Hf - 1 and y = y_low; ly = y - y_low, hy = 1 - ly (x alike) and the value is
 *   hy*hx*v1 + hy*lx*v2 + ly*hx*v3 + ly*lx*v4.  pooled = (the sum over the bin's samples in (iy, ix) order) / count.  Rows
 *   at or beyond n_roi[b] and RoIs holding a non-finite coordinate give zeros; every element of pooled is written.  The
 *   clamp of grid at 16 is a stated deviation (reached only by a RoI longer than 16 * PW feature cells).  One launch.
 *
 * gsr_roi_align_backward: grad_features [B,Cf,Hf,Wf] from grad_pooled [B,S,Cf,PH,PW]; nothing flows to the RoIs (Detectron2
 * detaches proposals).  A gather, no float atomics: with wy[ph][y] = the sum, in sample order, of the shares hy / ly that
 * the samples of bin ph give row y (wx alike),
 *       grad_features[b,c,y,x] = sum over RoIs s ascending of
 *                                (sum over ph ascending, then pw ascending, of (wy[ph][y] * wx[pw][x]) * grad_pooled[b,s,c,ph,pw]) / count_s
 *   an order fixed by the sizes and the RoI values alone: two calls on the same input give the same bits, on any stream.
 *   Every element is written exactly once; with accumulate != 0 the sum is added to what is there, as
 *   gsr_image_resample_backward does.  One launch.
 *
 * gsr_rcnn_loss (members B, S, C, M, bw_*, beta, w_cls, w_box, flags).  scores [B,S,C+1] (channel C: background);
 * deltas [B,S,4*C], or [B,S,4] with GSR_RCNN_CLASS_AGNOSTIC; rois, labels, gt_row as the sampler wrote them; gt_boxes
 * [B,M,4].  Rows with label -1 take no part (a label above C counts as -1); n = max(rows with label >= 0 in the batch, 1).
 *       cls = sum_rows -(x_t - max - log(sum exp(x - max))) / n
 *       target deltas of a foreground row (label < C, 0 <= gt_row < M; Box2BoxTransform.get_deltas, src = roi, dst = gt):
 *           sw = x2 - x1, scx = x1 + 0.5f * sw (dst alike);  tx = bw_x * (dcx - scx) / sw;  tw = bw_w * log(dw / sw);  y, h alike
 *       box = sum_fg sum_4 smooth_l1(delta[4*cls + k] - t_k, beta) / n
 *             beta = 0 (Detectron2): |x| with sign(0) = 0;  beta > 0: 0.5 x^2 / beta where |x| < beta, |x| - 0.5 beta elsewhere
 *       total = w_cls * cls + w_box * box                        (Detectron2: bw = 10, 10, 5, 5; the reference descends on cls)
 *   loss[3] = (cls, box, total), the first two unweighted.  grad_scores = (w_cls / n) * (p_c - [c == t]), zero on rows that
 *   take no part; grad_deltas is zero except in the four channels of a foreground row's class, (w_box / n) * smooth_l1'.
 *   Either may be NULL (the loss bits are the same either way); when given, every element is written exactly once.  A
 *   foreground row has IoU >= fg_iou > 0 with its box, hence sw, sh > 0.  Sums: per-row terms, four rows per block, the
 *   blocks' partials added by one block in index order (per-thread runs, an LDS tree).  ws: gsr_rcnn_workspace_bytes(spec)
 *   bytes of device memory, 16-byte aligned.  Three launches.
 *
 * gsr_rcnn_postprocess (members B, R, C, bw_*, conf_thr, iou_thr, max_det, img_w, img_h, flags): fast_rcnn_inference.
 * scores [B,R,C+1], deltas [B,R,4*C] (or [B,R,4]), proposals [B,R,4], n_prop as above; 1 <= R <= 4096, 1 <= max_det <= R.
 * Per proposal p = softmax(scores); the class is the first maximum of p_c over c < C (a NaN is never the maximum), the score
 * that maximum; the proposal is a candidate iff score > conf_thr (the reference: 0.5; a softmax has at most one entry above
 * 0.5, so from 0.5 up this is Detectron2's per-class filter; below, one label per proposal is a stated deviation).  Box
 * (Box2BoxTransform.apply_deltas on the class's four deltas, w = x2 - x1, cx = x1 + 0.5f * w of the proposal):
 *       dx = d0 / bw_x;  dw = min(d2 / bw_w, log(1000 / 16));  pcx = dx * w + cx;  pw = exp(dw) * w
 *       x1' = pcx - 0.5f * pw, x2' = pcx + 0.5f * pw, clipped to [0, img_w]; y alike with [0, img_h]
 * A candidate with a non-finite box is dropped.  counts[b,1] = the candidates.  They are compacted in proposal order and
 * walked by gsr_det_nms's kernels (class-aware, iou_thr -- Detectron2: 0.5 --, max_det -- 100): score descending, then
 * proposal order.  dets [B,max_det,6] (x1 y1 x2 y2 score class-as-float, zero rows beyond) and counts [B,2] (kept,
 * candidates): the layout gsr_det_verdict reads.  ws as above.  Four launches.
 *
 * All entries: every tensor argument is a DEVICE pointer.  A size out of range, a non-finite or negative weight, beta, fg_iou
 * or threshold, box weights or a frame that are not finite and > 0, unknown flags, a workspace that is too small or
 * misaligned, a NULL required pointer, a tensor that is not 4-byte aligned or more than 2^31 - 1 elements in a tensor
 * return GSR_ERR_INVALID with a gsr_last_error text before any device call.  No allocation, no copy, no host
 * synchronisation: everything is enqueued on `stream`; capturable and re-entrant (each caller with its own workspace). */
#define GSR_RCNN_CLASS_AGNOSTIC 1u
typedef struct GsrRcnnSpec {
  int32_t B, R, M, S, C;     /* images, proposals per image, gt rows (1..32), sampled RoIs (1..1024), classes without background */
  int32_t max_pos;           /* sampler: foreground quota, 0..S; Detectron2: 128 */
  int32_t append_gt;         /* sampler: ground-truth rows are candidates; Detectron2: 1 */
  uint32_t seed;             /* sampler */
  float   fg_iou;            /* sampler; Detectron2: 0.5 */
  int32_t Cf, Hf, Wf;        /* RoIAlign: the feature map */
  int32_t PH, PW;            /* RoIAlign: 1..14 */
  float   spatial_scale;     /* RoIAlign; the C4 model: 1/16 */
  int32_t sampling_ratio;    /* RoIAlign: 0 = adaptive */
  float   bw_x, bw_y, bw_w, bw_h; /* Box2BoxTransform weights; Detectron2: 10, 10, 5, 5 */
  float   beta;              /* loss: smooth-L1 beta; Detectron2: 0 */
  float   w_cls, w_box;      /* loss weights; the reference descends on cls alone: 1, 0 */
  float   conf_thr, iou_thr; /* output; the reference: 0.5, 0.5 */
  int32_t max_det;           /* output: rows of dets per image, 1..R; Detectron2: 100 */
  float   img_w, img_h;      /* output: boxes are clipped to this frame */
  uint32_t flags;            /* GSR_RCNN_CLASS_AGNOSTIC */
} GsrRcnnSpec;
int gsr_rcnn_sample(const GsrRcnnSpec* spec, const float* proposals, const int32_t* n_prop, const float* gt_boxes,
                    const int32_t* gt_cls, int32_t* idx, float* rois, int32_t* labels, int32_t* gt_row, int32_t* counts,
                    void* stream);
int gsr_roi_align(const GsrRcnnSpec* spec, const float* features, const float* rois, const int32_t* n_roi,
                  int32_t n_roi_stride, float* pooled, void* stream);
int gsr_roi_align_backward(const GsrRcnnSpec* spec, const float* rois, const int32_t* n_roi, int32_t n_roi_stride,
                           const float* grad_pooled, float* grad_features, int32_t accumulate, void* stream);
int gsr_rcnn_workspace_bytes(const GsrRcnnSpec* spec, int64_t* bytes);
int gsr_rcnn_loss(const GsrRcnnSpec* spec, const float* scores, const float* deltas, const float* rois, const int32_t* labels,
                  const int32_t* gt_row, const float* gt_boxes, void* ws, int64_t ws_bytes, float* loss, float* grad_scores,
                  float* grad_deltas, void* stream);
int gsr_rcnn_postprocess(const GsrRcnnSpec* spec, const float* scores, const float* deltas, const float* proposals,
                         const int32_t* n_prop, void* ws, int64_t ws_bytes, float* dets, int32_t* counts, void* stream);

/* ---- RPN proposal stage (capability bit GSR_CAP_RPN of gsr_query(5)) -----------------------------------------------------
 * The step in front of gsr_rcnn_sample: from the RPN head's objectness logits and anchor deltas to the proposals, as
 * Detectron2's DefaultAnchorGenerator, Box2BoxTransform, find_top_rpn_proposals and batched_nms compute them (the reference
 * runs its C4 Faster R-CNN in training mode: the best 12 000 of 15 * Hf * Wf anchors, NMS at 0.7, keep 2 000).  Two
 * entries: gsr_rpn_select, once per feature level, fills that level's range of the candidate slots; gsr_rpn_nms walks all
 * slots.  These are the formulas of record (INTEGRATION.md section 8i lists the deviations); csrc/gsr_rpn.h holds the
 * arithmetic, compiled for the kernels and for a host harness alike.  All arithmetic is float32, every operation rounded
 * on its own; index-valued results are int32.  One GsrRpnSpec serves both entries, each reading the members named with it.
 *
 * gsr_rpn_select (members B, A, Hf, Wf, stride, shift0, img_w, img_h, min_size, pre_topk, level, cand_offset, N).
 * logits [B,A,Hf,Wf] and deltas [B,4A,Hf,Wf] are the RPN head's own layouts; delta k of anchor a is channel 4a + k.
 * cell_anchors [A,4] (a device tensor): x1 y1 x2 y2 relative to a cell's shift.  The candidate index of anchor a at cell
 * (x, y) is i = (y * Wf + x) * A + a, its anchor
 *       cell_anchors[a] + ((float)(x * stride) + shift0, (float)(y * stride) + shift0)      added to both corners
 * (shift0 = Detectron2's offset * stride).  The candidates are the first n_l = min(pre_topk, A * Hf * Wf) indices in the
 * order (logit descending by float comparison, index ascending): +0.0 and -0.0 are equal, and a NaN logit is never a
 * candidate (with fewer than n_l logits that are not NaN the last ranks stay unused).  The candidate of rank r is decoded
 * (Box2BoxTransform.apply_deltas with weights 1, 1, 1, 1; w = x2 - x1, cx = x1 + 0.5f * w of the anchor):
 *       dw = min(d2, log(1000 / 16));  pcx = d0 * w + cx;  pw = exp(dw) * w;  x1' = pcx - 0.5f * pw, x2' = pcx + 0.5f * pw
 * and y alike.  It is dropped if any of the four unclipped coordinates is not finite; otherwise the box is clipped to
 * [0, img_w] x [0, img_h] and dropped unless x2' - x1' > min_size and y2' - y1' > min_size.  A dropped candidate does not
 * free its place for rank pre_topk (Detectron2 filters after its top-k as well).  Slot cand_offset + r of cand_boxes
 * [B,N,4], cand_scores [B,N] and cand_level [B,N] receives the box, the logit and `level`; a dropped or unused rank
 * receives zeros and level -1.  Every slot cand_offset .. cand_offset + n_l - 1 is written, no other.  1 <= N <= 16384,
 * cand_offset >= 0, cand_offset + n_l <= N, level >= 0, pre_topk >= 1, stride >= 1 with Hf * stride, Wf * stride <= 2^24.
 * One launch, one workgroup per image: a radix select of the n_l-th (logit, index) key, the survivors sorted in LDS.
 *
 * gsr_rpn_nms (members B, N, post_topk, iou_thr): 1 <= N <= 16384, 1 <= post_topk <= min(N, 4096).  The slots with
 * level >= 0 (and a score that is not NaN) are walked in the order (score descending by float comparison with +-0 equal,
 * slot ascending).  A box is suppressed iff an earlier KEPT box of the same level (levels compared as integers) has
 * iou > iou_thr -- strict; a NaN IoU is inert; the IoU is gsr_det_nms's, operation by operation:
 *       inter = max(min(ax2,bx2) - max(ax1,bx1), 0) * max(min(ay2,by2) - max(ay1,by1), 0)
 *       iou = inter / ((area_a + area_b) - inter),   area = (x2 - x1) * (y2 - y1)
 * The walk stops after post_topk keeps.  proposals [B,post_topk,4] and scores [B,post_topk] in walk order, zeros beyond
 * the count; keep [B,post_topk]: the kept slots, -1 beyond; counts [B].  Every element is written.  ws:
 * gsr_rpn_workspace_bytes(spec) bytes (members B, N) of device memory, 16-byte aligned; gsr_rpn_select needs none.  Two
 * launches, one workgroup per image each: the order (an LDS sort), then the walk with the kept boxes in LDS.
 *
 * Both entries: every tensor argument is a DEVICE pointer.  A size out of range, a frame that is not finite and > 0, a
 * shift0 that is not finite, a min_size or iou_thr that is not finite and >= 0, unknown flags (none are defined), a
 * workspace that is too small or misaligned, a NULL required pointer, a tensor that is not 4-byte aligned or more than
 * 2^31 - 1 elements in a tensor return GSR_ERR_INVALID with a gsr_last_error text before any device call.  No allocation,
 * no copy, no host synchronisation, no float atomics: everything is enqueued on `stream`; capturable and re-entrant (each
 * caller with its own workspace and candidate arrays). */
typedef struct GsrRpnSpec {
  int32_t B, A, Hf, Wf;      /* images, anchors per cell, the level's feature map */
  int32_t stride;            /* select: pixels per cell */
  float   shift0;            /* select: Detectron2's offset * stride */
  float   img_w, img_h;      /* select: boxes are clipped to this frame */
  float   min_size;          /* select: both sides must exceed it; Detectron2: 0 */
  int32_t pre_topk;          /* select: candidates per level and image; Detectron2 in training: 12000 */
  int32_t level;             /* select: what cand_level receives, >= 0 */
  int32_t cand_offset;       /* select: the level's first slot */
  int32_t N;                 /* candidate slots per image, 1..16384 */
  int32_t post_topk;         /* nms: rows of proposals per image, 1..min(N, 4096); Detectron2 in training: 2000 */
  float   iou_thr;           /* nms; Detectron2: 0.7 */
  uint32_t flags;            /* none defined: 0 */
} GsrRpnSpec;
int gsr_rpn_workspace_bytes(const GsrRpnSpec* spec, int64_t* bytes);
int gsr_rpn_select(const GsrRpnSpec* spec, const float* logits, const float* deltas, const float* cell_anchors,
                   float* cand_boxes, float* cand_scores, int32_t* cand_level, void* stream);
int gsr_rpn_nms(const GsrRpnSpec* spec, const float* cand_boxes, const float* cand_scores, const int32_t* cand_level, void* ws,
                int64_t ws_bytes, float* proposals, float* scores, int32_t* keep, int32_t* counts, void* stream);

/* ---- FPN RoI pooler (present iff the library exports gsr_fpn_pool) ---------------------------------------------------------
 * The step between gsr_rcnn_sample and the box head of a detector with a feature pyramid: Detectron2's ROIPooler with
 * assign_boxes_to_levels.  Every RoI is pooled from ONE of nl feature maps, chosen by its size; the pooling is
 * gsr_roi_align's, and the backward gsr_roi_align_backward's, operation by operation: a RoI of level l gives the bits
 * gsr_roi_align gives on features[l] with spatial_scale = scale[l], and grad_features[l] the bits gsr_roi_align_backward gives
 * over the RoIs of level l alone.  csrc/gsr_fpn.h holds the level arithmetic, compiled for the kernels and for a host
 * harness alike (INTEGRATION.md section 8j lists the deviations).  All arithmetic is float32, every operation rounded on its
 * own; index-valued results are int32.
 *
 * Level of row s of image b (rois [B,S,4] in image pixels; n_roi as gsr_roi_align reads it):
 *       -1                                                          if s >= n_roi[b] or a coordinate is not finite
 *       area = (x2 - x1) * (y2 - y1);   q = sqrt(area) / canonical_size + 1e-8f
 *       level = the number of l in 1 .. nl - 1 with q >= thr[l]
 *   thr[l] = 2^(log2(stride_0) + l - canonical_level) makes this Detectron2's floor(canonical_level + log2(q)) clamped to
 *   the levels (canonical_size 224, canonical_level 4; strides 4, 8, 16, 32: thr = -, 0.5, 1, 2), without the logarithm: a
 *   stated deviation, differing only where log2f's rounding crosses an integer.  A q that is NaN (a negative area) passes
 *   no threshold: level 0, where Detectron2's result is undefined.  A row of level -1 belongs to no level.
 *
 * gsr_fpn_pool.  features: a HOST array of nl device pointers, level l being [B,Cf,Hf[l],Wf[l]].  Outputs: pooled
 * [B,S,Cf,PH,PW] (zeros for a row of level -1; every element written), roi_level [B,S] and level_count [B,nl] (every
 * element written), level_list [B,nl,S]: the rows of level l of image b in ASCENDING order in its first level_count[b,l]
 * entries, the others untouched.  The three integer outputs are what gsr_fpn_pool_backward reads; the caller keeps them.
 * Two launches: the assignment (one workgroup per image, one lane per RoI, ballots and a scan), then the pooling.
 *
 * gsr_fpn_pool_backward.  grad_features: a HOST array of nl device pointers, level l being [B,Cf,Hf[l],Wf[l]].  With the
 * weights and the order of gsr_roi_align_backward,
 *       grad_features[l][b,c,y,x] = sum over i ascending in 0 .. level_count[b,l] - 1, s = level_list[b,l,i], of
 *                                   (sum over ph, then pw ascending of (wy[ph][y] * wx[pw][x]) * grad_pooled[b,s,c,ph,pw]) / count_s
 *   Every element of every level is written exactly once (zeros where a level received no RoI); with accumulate != 0 the
 *   sum is added to what is there.  level_count is clamped to 0..S and an entry of level_list outside 0..S-1 is skipped:
 *   neither is trusted for an address.  A gather, no float atomics: two calls on the same input give the same bits, on any
 *   stream.  One launch for all levels; a tile walks the RoIs of its own level alone.
 *
 * Both entries: 1 <= B, Cf <= 65535, 1 <= S <= 1024, 1 <= PH, PW <= 14, sampling_ratio >= 0, 1 <= nl <= 5, Hf[l], Wf[l] >= 1,
 * scale[l] finite and > 0, thr[1 .. nl-1] finite, > 0 and strictly ascending (thr[0] is not read), canonical_size finite
 * and > 0, at most 2^31 - 1 elements in a tensor and 8 x 8 tiles in all levels together.  Every tensor argument is a DEVICE
 * pointer; the two pointer arrays live on the HOST and are read before the call returns.  A size out of range, a NULL
 * required pointer (each of the nl level pointers is one), a tensor that is not 4-byte aligned return GSR_ERR_INVALID with
 * a gsr_last_error text before any device call.  No allocation, no copy, no host synchronisation, no workspace: everything
 * is enqueued on `stream`; capturable and re-entrant (each caller with its own outputs). */
typedef struct GsrFpnSpec {
  int32_t B, S, Cf;          /* images, RoIs per image (1..1024), channels of every level */
  int32_t PH, PW;            /* 1..14; Detectron2's FPN box head: 7, 7 */
  int32_t sampling_ratio;    /* 0 = adaptive */
  int32_t nl;                /* levels, 1..5 */
  int32_t Hf[5], Wf[5];      /* the level's feature map */
  float   scale[5];          /* the level's spatial_scale: 1 / stride */
  float   thr[5];            /* level thresholds on q, entry 0 unused; strides 4..32: -, 0.5, 1, 2 */
  float   canonical_size;    /* Detectron2: 224 */
} GsrFpnSpec;
int gsr_fpn_pool(const GsrFpnSpec* spec, const float* const* features, const float* rois, const int32_t* n_roi,
                 int32_t n_roi_stride, float* pooled, int32_t* roi_level, int32_t* level_list, int32_t* level_count,
                 void* stream);
int gsr_fpn_pool_backward(const GsrFpnSpec* spec, const float* rois, const int32_t* level_list, const int32_t* level_count,
                          const float* grad_pooled, float* const* grad_features, int32_t accumulate, void* stream);

/* ---- Fused image losses (present iff the library exports gsr_imgloss) -----------------------------------------------------
 * L1, L2 and SSIM of an image x against a reference image y, and the gradient of their weighted sum with respect to x: the
 * reference's utils/loss_utils.py (l1_loss, l2_loss, ssim) per image of a batch.  csrc/gsr_imgloss.h holds the per-pixel
 * arithmetic, compiled for the kernels and for a host harness alike (INTEGRATION.md section 8k lists the deviations).  All
 * per-pixel arithmetic is float32, every operation rounded on its own.
 *
 * x = img, y = ref, both [B,C,H,W] float32, 1 <= C <= 4; per image b, with n = C H W:
 *       l1_b   = sum |x - y| / n          l2_b = sum (x - y)^2 / n          ssim_b = sum map / n
 *       loss_b = w_l1 l1_b + w_l2 l2_b + w_ssim (1 - ssim_b)
 *   map is the reference's _ssim per channel: win = an 11 x 11 Gaussian window with sigma 1.5 and zero padding of 5;
 *       mu1 = win * x, mu2 = win * y, E11 = win * x^2, E22 = win * y^2, E12 = win * xy
 *       s1 = E11 - mu1^2, s2 = E22 - mu2^2, s12 = E12 - mu1 mu2, C1 = 0.01^2, C2 = 0.03^2
 *       map = (2 mu1 mu2 + C1)(2 s12 + C2) / ((mu1^2 + mu2^2 + C1)(s1 + s2 + C2))
 *   The window is DEFINED as the eleven float32 taps the reference constructs, exp(-(k - 5)^2 / 4.5) as float32 divided by
 *   their float32 sum, applied separably: rows first, then columns, each an 11-term sum in ascending k.  The reference's
 *   2-D window is the rounded outer product of the same taps: one rounding per weight apart (a stated deviation).
 *
 * Gradient with respect to x (grad_img, when given): L1 gives sign(x - y) / n with sign(0) = 0, L2 gives 2 (x - y) / n, and
 *       d ssim_b / d x(p) = [win * (dmap/dmu1) + 2 x(p) win * (dmap/dE11) + y(p) win * (dmap/dE12)](p) / n
 *   where dmap/dmu1 is total (the paths through s1 and s12 included) and the three derivative maps are zero beyond the image:
 *   a gather over the symmetric window, rows then columns, no float atomics.  Nothing flows to y.
 *
 * GSR_IMGLOSS_CLAMP01: both images are clamped to [0,1] on the way in, and the gradient gets gsr_image_resample's inclusive
 * mask (0 <= x <= 1 passes; a NaN gives 0).  Without it nothing is clamped.  A NaN in image b makes image b's terms NaN
 * and touches no other image.
 * GSR_IMGLOSS_NO_GRAD: the caller will pass grad_img == NULL; gsr_imgloss_workspace_bytes then reports the bytes of the
 * per-tile partial sums alone (without it: those plus three float maps of B C H W elements, needed only for a gradient).
 * A non-null grad_img with this flag is refused.  The flag changes no output bit.
 *
 * Outputs: terms [B,4] = l1, l2, ssim, loss; grad_img [B,C,H,W] or NULL; ssim_map [B,C,H,W] or NULL.  Every element of
 * every output given is written; what the workspace held before the call has no influence; terms are the same bits with
 * and without grad_img and ssim_map.  Sums: a 16 x 32 tile's pixels by a fixed butterfly and wave order (float32), an
 * image's tiles in a fixed order (double).  Three launches with a gradient, two without.
 *
 * B, C, H, W >= 1, C <= 4, B C H W < 2^31, finite weights, no unknown flag bits, ws_bytes >= what
 * gsr_imgloss_workspace_bytes reports for what the call needs, ws 16-byte aligned, the tensors 4-byte aligned: otherwise
 * GSR_ERR_INVALID with a gsr_last_error text before any pointer is followed.  No allocation, no copy, no host
 * synchronisation: everything is enqueued on `stream`; capturable and re-entrant (each caller with its own workspace). */
#define GSR_IMGLOSS_CLAMP01 1u
#define GSR_IMGLOSS_NO_GRAD 2u
typedef struct GsrImgLossSpec {
  int32_t B, C, H, W;
  float   w_l1, w_l2, w_ssim;
  uint32_t flags;
} GsrImgLossSpec;
int gsr_imgloss_workspace_bytes(const GsrImgLossSpec* spec, int64_t* bytes);
int gsr_imgloss(const GsrImgLossSpec* spec, const float* img, const float* ref, void* ws, int64_t ws_bytes,
                float* terms /* [B,4]: l1, l2, ssim, loss */, float* grad_img /* [B,C,H,W] or null */,
                float* ssim_map /* [B,C,H,W] or null */, void* stream);

/* ---- RPN loss stage (present iff the library exports gsr_rpnloss) ---------------------------------------------------------
 * The two losses of the region proposal network, loss_rpn_cls and loss_rpn_loc, with their gradient: Detectron2's
 * RPN.label_and_sample_anchors, Matcher (with low-quality matches), subsample_labels and RPN.losses.  Two entries:
 * gsr_rpnloss_label labels and samples the anchors of every image from the anchors and the ground truth alone;
 * gsr_rpnloss turns labels, the head's logits and deltas into loss[3] and both gradients.  These are the formulas of record
 * (INTEGRATION.md section 8l lists the deviations); csrc/gsr_rpnloss.h holds the arithmetic, compiled for the kernels and
 * for a host harness alike.  All arithmetic is float32, every operation rounded on its own; index-valued results are int32.
 *
 * Anchors.  Up to 5 levels in the head's order; level l has A[l] cell anchors (cell_anchors[l]: a device tensor [A,4], x1 y1
 * x2 y2 relative to a cell's shift) on Hf[l] x Wf[l] cells, and anchor a of cell (x, y) is
 *       cell_anchors[l][a] + ((float)(x * stride[l]) + shift0[l], (float)(y * stride[l]) + shift0[l])   added to both corners
 * as in gsr_rpn_select.  Its flat index is r = level_offset[l] + (y * Wf + x) * A + a with level_offset[l] the anchors of
 * the levels before l: Detectron2's concatenation order and gsr_rpn_select's candidate index.  R = sum A Hf Wf <= 2^24.
 * gt_boxes [B,M,4]; gt_cls [B,M] int32, a row being PRESENT iff gt_cls >= 0 (the RPN is class-agnostic); 1 <= M <= 256.
 *
 * gsr_rpnloss_label, per image:
 *   Match.  iou(m, r) is gsr_rcnn_sample's IoU (pairwise_iou).  best[r] = the first maximum of iou(m, r) over the present
 *   rows in ascending m (the lowest m wins ties; a NaN is never the maximum), matched[r] that row; -1 without a present row.
 *   Pre-label: 0 where best < iou_lo, -1 where iou_lo <= best < iou_hi, 1 where best >= iou_hi (Detectron2: 0.3, 0.7).  An
 *   image without a present row has pre-label 0 everywhere.
 *   Low-quality matches.  rowmax[m] = the maximum of iou(m, r) over all R anchors (NaN ignored).  Every anchor r with
 *   iou(m, r) == rowmax[m] for some present row m with rowmax[m] > 0 gets pre-label 1; matched[r] stays its own best row, as
 *   in Detectron2.  A row with rowmax[m] = 0 promotes nothing (a stated deviation: Detectron2 would promote every anchor).
 *   Keyed sample.  key(b, r) as in gsr_rcnn_sample with r in the place of i.  #pos / #neg = the anchors of pre-label 1 / 0;
 *       n_pos = min(pos_quota, #pos);   n_neg = min(batch_per_image - n_pos, #neg)
 *   (pos_quota = int(batch_per_image * positive_fraction), computed by the caller; Detectron2: 256, 128).  The n_pos
 *   smallest (key, r) among pre-label 1 keep label 1, the n_neg smallest among pre-label 0 keep label 0; every other anchor
 *   gets -1.  This takes the place of Detectron2's randperm (a stated deviation): the same seed gives the same sample.
 *   Outputs: labels [B,R], matched [B,R], counts [B,4] = #pos, #neg, n_pos, n_neg, and, when given, prelabels [B,R].  Every
 *   element is written.  Five launches: a clear of the workspace's maxima and counts, the rows' maxima (an integer
 *   atomicMax on the bit image of a non-negative float: a maximum does not depend on the order of arrival), the pre-labels,
 *   a radix select of each kind's quota-th (key, r), labels.
 *
 * gsr_rpnloss.  logits[l] [B,A,Hf,Wf] and deltas[l] [B,4A,Hf,Wf] are the head's own layouts (delta k of anchor a is channel
 * 4a + k); labels and matched as gsr_rpnloss_label wrote them (a label other than 0 or 1 counts as -1; a label 1 whose
 * matched row is outside 0..M-1 takes part in cls alone).  With norm = (float)(batch_per_image * B) -- Detectron2's
 * normaliser, not the sampled count -- and bce(x, t) = max(x, 0) - x t + log1p(exp(-|x|)):
 *       S_cls = sum over label >= 0 of bce(logit, label)
 *       S_loc = sum over label == 1, k < 4 of smooth_l1(delta_k - t_k, beta)
 *               t = Box2BoxTransform(1, 1, 1, 1).get_deltas(anchor, gt[matched]) as in gsr_rcnn_loss; smooth_l1 as there
 *               (Detectron2: beta = 0)
 *       loss[3] = (total, cls, loc):  cls = (w_cls * S_cls) / norm,  loc = (w_loc * S_loc) / norm,  total = cls + loc
 *       grad_logits = (w_cls / norm) * (sigmoid(logit) - label)  where label >= 0, else 0
 *       grad_deltas = (w_loc / norm) * smooth_l1'(delta_k - t_k) in the four channels of an anchor of label 1, else 0
 *   grad_logits[l] and grad_deltas[l] have the inputs' own layouts; either array may be NULL (the loss bits are the same
 *   either way); when given, every element is written exactly once.  The logit and the deltas of an anchor that is not
 *   sampled, and the deltas of one that is not positive, are never read: a NaN there reaches neither the loss nor a
 *   gradient.  A non-finite value of a sampled anchor makes the loss non-finite and leaves every other anchor's gradient as
 *   it is.  Sums: a block's 256 terms by an LDS tree, the blocks' partials by one block in index order.  Two launches.
 *
 * The four pointer arrays (cell_anchors, logits, deltas, grad_*) live on the HOST, hold nl device pointers each and are read
 * before the call returns; every other tensor argument is a DEVICE pointer.  1 <= B <= 65535, 1 <= M <= 256, 1 <= nl <= 5,
 * A, Hf, Wf >= 1, stride >= 1 with Hf * stride, Wf * stride <= 2^24, shift0 finite, R <= 2^24, B * R and the elements of a
 * deltas tensor <= 2^31 - 1, 1 <= batch_per_image <= 65536, 0 <= pos_quota <= batch_per_image, 0 <= iou_lo <= iou_hi finite,
 * beta and the weights finite and >= 0, flags 0.  ws: gsr_rpnloss_workspace_bytes(spec) bytes of device memory, 16-byte
 * aligned, for either entry; what it held before has no influence.  A size out of range, a NULL required pointer (each of
 * the nl level pointers is one), a tensor that is not 4-byte aligned, a workspace that is too small or misaligned return
 * GSR_ERR_INVALID with a gsr_last_error text before any device call.  No allocation, no copy, no host synchronisation, no
 * float atomics: everything is enqueued on `stream`; capturable and re-entrant (each caller with its own workspace). */
typedef struct GsrRpnLossSpec {
  int32_t B, M;              /* images, gt rows (1..256) */
  int32_t nl;                /* levels, 1..5 */
  int32_t A[5], Hf[5], Wf[5]; /* anchors per cell and the feature map of each level */
  int32_t stride[5];         /* pixels per cell */
  float   shift0[5];         /* Detectron2's offset * stride */
  int32_t batch_per_image;   /* Detectron2: 256 */
  int32_t pos_quota;         /* int(batch_per_image * positive_fraction); Detectron2: 128 */
  uint32_t seed;             /* the sample's key */
  float   iou_lo, iou_hi;    /* Detectron2: 0.3, 0.7 */
  float   beta;              /* smooth-L1 beta; Detectron2: 0 */
  float   w_cls, w_loc;      /* loss weights; Detectron2: 1, 1 */
  uint32_t flags;            /* none defined: 0 */
} GsrRpnLossSpec;
int gsr_rpnloss_workspace_bytes(const GsrRpnLossSpec* spec, int64_t* bytes);
int gsr_rpnloss_label(const GsrRpnLossSpec* spec, const float* const* cell_anchors, const float* gt_boxes, const int32_t* gt_cls,
                      void* ws, int64_t ws_bytes, int32_t* labels, int32_t* matched, int32_t* counts,
                      int32_t* prelabels /* [B,R] or null */, void* stream);
int gsr_rpnloss(const GsrRpnLossSpec* spec, const int32_t* labels, const int32_t* matched, const float* const* logits,
                const float* const* deltas, const float* const* cell_anchors, const float* gt_boxes, void* ws, int64_t ws_bytes,
                float* loss /* [3]: total, cls, loc */, float* const* grad_logits, float* const* grad_deltas, void* stream);

/* ---- Object-map classifier (present iff the library exports gsr_objmap) ----------------------------------------------------
 * What consumes render()'s 16-channel object map: the reference's torch.argmax(Conv2d(16, K, 1)(map), 0) (render.py:126-131)
 * per pixel, fused with the arg-max's confidence, per-class boxes, a painted image, and the cross entropy against a target
 * id map with its gradient with respect to the map.  No logit is stored: at K = 256 the torch expression writes and reads
 * a [256,H,W] tensor, this call reads the map once.  csrc/gsr_objmap.h holds the per-pixel arithmetic, compiled for the
 * kernels and for a host harness alike (INTEGRATION.md section 8m lists the deviations).  All arithmetic is float32; the
 * softmax sum alone is carried in double and rounded to float32 once.
 *
 * objmap [B,16,H,W], weight [K,16] and bias [K] (the Conv2d's, row-major), 1 <= K <= 1024; per pixel with features f:
 *       l_c  = fma chain: l = bias[c]; for k = 0..15: l = fmaf(weight[c,k], f[k], l)
 *       id   = the first maximum of l_c over c = 0..K-1 under l > best, from -inf.  A NaN logit is never the maximum
 *              (torch.argmax lets a NaN win: a stated deviation); a pixel none of whose logits compares greater than -inf
 *              gets id -1
 *       conf = 1 / sum_c exp(l_c - m), m the maximum, c ascending: the arg-max's softmax probability; 0 for id -1
 *   stats [B,K,5] = (count, x0, y0, x1, y1) of each class's pixels in each image: PIL's getbbox convention, x1 and y1
 *   exclusive; five zeros for a class without a pixel.  Accumulated per workgroup, then with integer atomicAdd / atomicMin /
 *   atomicMax: commutative integer updates, the same bits whatever the order of arrival.
 *   paint [B,H,W,3] uint8 = palette[id] (palette [K,3] uint8), black for id -1.
 *
 * GSR_OBJMAP_LOSS with a target [B,H,W] int32: a pixel is COUNTED iff its id >= 0 and its target lies in 0..K-1; valid_b is
 * the number of counted pixels of image b.
 *       ce(pixel) = (m - l_t) + log sum_c exp(l_c - m)
 *       terms [B,2] = (sum of ce over the counted pixels / valid_b, valid_b as float); (0, 0) when valid_b = 0
 *       grad [B,16,H,W]: d terms[b,0] / d objmap = (1 / valid_b) sum_c weight[c,k] (p_c - [c = t]), c ascending, one fmaf per
 *       term, p_c = exp(l_c - m) conf; zeros at every pixel that is not counted.  The classifier is frozen: there is no
 *       gradient to weight or bias.
 *   A NaN logit beside a finite maximum makes that pixel's conf, ce and gradient NaN and image b's terms[b,0] NaN, and
 *   touches no other image.  Sums: a workgroup's 256 terms by an LDS tree, an image's workgroups in index order (float32).
 *
 * ids is required; conf, stats, paint, terms and grad may each be NULL.  Every element of every output given is written;
 * what the workspace held before the call has no influence; each output is the same bits whichever others are given.
 * Two to three launches with stats or a loss, one without.
 *
 * B, H, W >= 1, B <= 65535, 1 <= K <= 1024, at most 2^31 - 1 elements in a tensor, no unknown flag bits; paint needs palette;
 * terms and grad need target and GSR_OBJMAP_LOSS; ws_bytes >= what gsr_objmap_workspace_bytes reports (0 without
 * GSR_OBJMAP_LOSS, and ws may then be NULL), ws 16-byte aligned, the float and int tensors 4-byte aligned: otherwise
 * GSR_ERR_INVALID with a gsr_last_error text before any device call.  No allocation, no copy, no host synchronisation:
 * everything is enqueued on `stream`; capturable and re-entrant (each caller with its own workspace). */
#define GSR_OBJMAP_LOSS 1u
typedef struct GsrObjMapSpec {
  int32_t B, H, W, K;
  uint32_t flags;
} GsrObjMapSpec;
int gsr_objmap_workspace_bytes(const GsrObjMapSpec* spec, int64_t* bytes);
int gsr_objmap(const GsrObjMapSpec* spec, const float* objmap, const float* weight /* [K,16] */, const float* bias /* [K] */,
               const int32_t* target /* [B,H,W] or null */, const uint8_t* palette /* [K,3] or null */, void* ws,
               int64_t ws_bytes, int32_t* ids, float* conf, int32_t* stats /* [B,K,5] */, uint8_t* paint,
               float* terms /* [B,2] */, float* grad, void* stream);

/* Introspection. what: 0 version, 1 bytes held by the workspace pool on the current device,
 * 2 number of pairs of a context (ctx as int64 handle in *out on input is NOT used; see gsr_ctx_info),
 * 3 capability bits of this build (features added without a change of GSR_VERSION): GSR_CAP_IMAGE = the image front end
 * (gsr_image_resample, gsr_image_resample_backward, gsr_image_to_u8); GSR_CAP_DETECT = the detector output stage
 * (gsr_det_workspace_bytes, gsr_det_postprocess, gsr_det_nms, gsr_det_box_iou, gsr_det_verdict); GSR_CAP_DETLOSS = the
 * detector loss stage (gsr_detloss_workspace_bytes, gsr_detloss); GSR_CAP_SETDET = the set-prediction detector stage
 * (gsr_setdet_workspace_bytes, gsr_setdet_loss, gsr_setdet_postprocess).  Item 3 is closed at these four bits: callers
 * compare its value as a whole, so a build with later stages still reports 15 there;
 * 4 the five bits up to GSR_CAP_RCNN: the four above and GSR_CAP_RCNN = the two-stage detector stage
 * (gsr_rcnn_sample, gsr_roi_align, gsr_roi_align_backward, gsr_rcnn_workspace_bytes, gsr_rcnn_loss, gsr_rcnn_postprocess).
 * A library that predates item 4 answers it with GSR_ERR_INVALID: no later stage.  Item 4 is closed at these five bits
 * (31), for the same reason as item 3;
 * 5 every capability bit of this build: the five above and GSR_CAP_RPN = the RPN proposal stage
 * (gsr_rpn_workspace_bytes, gsr_rpn_select, gsr_rpn_nms).  A library that predates item 5 refuses it alike.
 * The FPN RoI pooler (gsr_fpn_pool, gsr_fpn_pool_backward) has no bit and no item: items 3 to 5 are compared as whole
 * values by their callers and stay as they are.  That stage is present iff the library exports gsr_fpn_pool, and the
 * fused image losses (gsr_imgloss_workspace_bytes, gsr_imgloss) likewise iff it exports gsr_imgloss, the RPN loss stage
 * (gsr_rpnloss_workspace_bytes, gsr_rpnloss_label, gsr_rpnloss) iff it exports gsr_rpnloss, the object-map classifier
 * (gsr_objmap_workspace_bytes, gsr_objmap) iff it exports gsr_objmap. */
#define GSR_CAP_IMAGE 1
#define GSR_CAP_DETECT 2
#define GSR_CAP_DETLOSS 4
#define GSR_CAP_SETDET 8
#define GSR_CAP_RCNN 16
#define GSR_CAP_RPN 32
int gsr_query(int32_t what, int64_t* out);

/* Per-context numbers for roofline accounting: what 0 = num_rendered (N; waits for the forward's count if it was
 * asynchronous), 1 = visible Gaussians (V; -1: not counted on the host), 2 = workspace bytes of this context,
 * 3 = the pair capacity the forward's buffers were sized for (= N unless GSR_FLAG_ASYNC_COUNT).
 * A context kept for backward holds, besides 100 bytes per Gaussian and 16 per pixel, 4 bytes per pair and -- unless
 * object channels are composited or GSR_FLAG_NO_SEGMENTS is set -- (N/256 + min(tiles, N/256) + 1) boundary records of
 * 4 KB: 50-190 MB at N = 3-10 M pairs.  num_rendered counts the pairs of the TIGHTENED tile rects (the tiles the
 * alpha >= 1/255 footprint's bounding box touches); under GSR_FLAG_NO_CULL it is the reference's count. */
int gsr_ctx_info(const GsrCtx* ctx, int32_t what, int64_t* out);   /* also: 4 = views of the context's batch (1: an ordinary forward), 5 = Ppad */
/* Items 6-9: which of the size-gated variants of the binning front end the context's forward took (tests assert them):
 * 6 = passes of the depth sort: 3 (digits of <= 11 bits, 2048-bin kernels) or 4 (<= 8 bits, 256-bin kernels; from 3 << 20
 *     virtual Gaussians on, or GSR_DEPTH_PASSES=4 in the environment),
 * 7 = 64-element rounds per wave of the pair emission and the tile sort: 8 (2048-element chunks) or 16 (4096; above 4 << 20
 *     pairs of capacity -- item 3 -- or GSR_RS_ROUNDS=16); 0 when the forward had no pairs.  Under 4 depth passes, passes
 *     1-3 of the depth sort use the rounds the same rule gives for the number of virtual Gaussians,
 * 8 = items per thread of the rank-order scan: 8, or 16 above 2 << 20 virtual Gaussians,
 * 9 = 1 when the storage-order scan read the preprocess workgroups' sums through group sums (more than 4096 * 256
 *     virtual Gaussians), else 0. */

/* Copies one internal array of a context into a caller DEVICE buffer (tests / diagnostics):
 * what 0 = tile ranges [T][2] u32, 1 = sorted pair list [N] u32 (Gaussian index | strip mask << 28, tile by tile, depth
 * order inside a tile), 2 = n_contrib [H*W] u32, 3 = final_T [H*W] f32, 4 = order (depth rank -> Gaussian; the first
 * V = scalars[1] entries are meaningful: only Gaussians that emit pairs are ranked) [P] u32, 5 = off [P+1] u32 (pairs
 * emitted in front of rank r; V+1 entries), 7 (and, for old callers, 6) = splat records [P][3] float4 in storage order
 * (layout: csrc/gsr_kernels.hip.h; written for Gaussians that emit pairs), 8 = the forward's device-side scalars [16]
 * u32 (0 pairs, 1 V, 2 smallest depth key, 3 depth digit width, 4 overflow flag, 5 boundary records, 6-7 64-bit pair
 * count), 9 = offg [P+1] u32 (storage-order scan of tiles touched). */
int gsr_ctx_export(const GsrCtx* ctx, int32_t what, void* dst, int64_t dst_bytes, void* stream);

/* Frees every cached workspace block of the current device (blocks in use by live contexts are kept). */
void gsr_trim_pool(void);

/* Per-stage timing of all calls of this process since the last reset, measured with hip events on the
 * stream the kernels were launched on.  Enable with gsr_profile(1): every stage is then bracketed by event
 * records (adds a few microseconds per stage); gsr_profile_read synchronises and fills
 * ms[GSR_STAGE_COUNT] with accumulated milliseconds and calls[GSR_STAGE_COUNT] with launch counts. */
enum {
  GSR_STAGE_PREPROCESS = 0,
  GSR_STAGE_DEPTH_SORT = 1,
  GSR_STAGE_BIN = 2,       /* pack + scan + emit */
  GSR_STAGE_TILE_SORT = 3, /* + tile ranges */
  GSR_STAGE_RENDER_FWD = 4,
  GSR_STAGE_RENDER_BWD = 5,
  GSR_STAGE_PREPROCESS_BWD = 6,
  GSR_STAGE_COUNT = 7
};
/* gsr_profile(mask): bit i of mask times stage i (0x7F = all stages, 0 = off; also resets the accumulators).  Each
 * timed stage costs two event records on the stream (a few microseconds of queue time each). */
void gsr_profile(int32_t stage_mask);
int gsr_profile_read(float* ms, int64_t* calls);

/* Diagnostic: writes (stage, start_ms, end_ms) triples of every span recorded since the last read, relative to the
 * first span's start, into out[3 * max_spans]; returns the number written and clears the spans. */
int gsr_profile_timeline(float* out, int max_spans);

const char* gsr_last_error(void);

/*
 * gsr_debug_wave_clock: diagnostic.  While `buf` (device, [ntiles][2] uint64) is set, every backward composite (K7)
 * stamps the 100 MHz wall clock at which each tile's wave started and ended; pass NULL to stop.  Process-wide.
 */
int gsr_debug_wave_clock(unsigned long long* buf);
/* Same for the forward composite (K6): [ntiles * waves per tile][2]. */
int gsr_debug_wave_clock_fwd(unsigned long long* buf);

/* Test hooks (used by tests/ only): the scan and sort primitives of the binning stage on caller buffers.
 * gsr_test_scan: out[0..n] = exclusive prefix sums of in[0..n) (out[n] = total), uint32.
 * gsr_test_sort_pairs: stable ascending sort of (keys, vals) on key bits [begin_bit, end_bit), in place;
 *                      iota != 0: vals are ignored on input and the result is the sorting permutation. */
int gsr_test_scan(const uint32_t* in, uint32_t* out, uint32_t n, void* stream);
int gsr_test_sort_pairs(uint32_t* keys, uint32_t* vals, uint32_t n, int32_t begin_bit, int32_t end_bit, int32_t iota,
                        void* stream);
/* The same primitives with every argument the forward uses.
 * gsr_test_scan_ex: n_dev (device, may be NULL): the live count is min(n, *n_dev); out[0..live) are the prefix sums and
 *   out[live] the total, words behind it are not written.  out == in is allowed.  chunk_first (device, may be NULL): the
 *   scanned values are run lengths of output slots (element r owns [out[r], out[r] + in[r])), and chunk_first[c] receives the
 *   element that owns slot c * chunk_len, for every c < chunk_cap with c * chunk_len below the total; other entries are
 *   not written.  chunk_len must be > 0 when chunk_first is given.
 * gsr_test_sort_pairs_ex: n_dev as above (positions at and behind the live count hold nothing meaningful afterwards);
 *   rounds: 64-element rounds per wave, 8 or 16 (chunks of 2048 / 4096 elements), 0 = what the library picks for n;
 *   key_ranges (device, may be NULL; needs begin_bit == 0 and [0, end_bit) covering every key): 2 * key_limit words the
 *   caller has set to (0xFFFFFFFF, 0); the last pass leaves [first, last + 1) of the run of every key < key_limit that is
 *   present, in positions of the sorted output.
 * Both return GSR_ERR_INVALID before any launch for NULL in / out / keys / vals, rounds outside {0, 8, 16}, a bit range
 * outside [0, 32], and key_ranges with begin_bit != 0. */
int gsr_test_scan_ex(const uint32_t* in, uint32_t* out, uint32_t n, const uint32_t* n_dev, uint32_t* chunk_first,
                     uint32_t chunk_len, uint32_t chunk_cap, void* stream);
int gsr_test_sort_pairs_ex(uint32_t* keys, uint32_t* vals, uint32_t n, const uint32_t* n_dev, int32_t begin_bit,
                           int32_t end_bit, int32_t iota, int32_t rounds, uint32_t* key_ranges, uint32_t key_limit,
                           void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GSRASTER_H_ */
