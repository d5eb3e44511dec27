/*
 * s360.h — C ABI of the MI355X-native panoramic Gaussian-splat rasteriser (libs360.so).
 *
 * Drop-in boundary for the one native dependency of thucz/splatter360's render path: the
 * `diff_gaussian_rasterization` extension imported at
 *     /root/reference/src/model/decoder/cuda_splatting.py:5-8
 * and called at cuda_splatting.py:99-124 (forward) / by autograd (backward).  The reference
 * defines no C ABI itself (its extension is a pybind11 module that is not vendored); each entry
 * point below names the upstream pybind function / reference call site it replaces.
 *
 * Conventions
 *   - plain pointers and sizes only; every data pointer is DEVICE memory (HIP, gfx950) unless
 *     the name ends in _host;  all tensors are contiguous float32 / int32 / uint32;
 *   - the caller owns every buffer (outputs and workspaces); sizes come from s360_layout();
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*), performs NO host
 *     synchronisation and allocates nothing; kernels are re-entrant across streams/devices;
 *   - return value: 0 on success, negative S360_E_* otherwise; nothing throws across the ABI;
 *   - a call renders V views of ONE Gaussian cloud (V = 1 reproduces one reference rasteriser
 *     call; V = 6 renders the six cube faces of an equirectangular view in one fused pass,
 *     replacing the per-face Python loop at src/model/decoder/decoder_splatting_cuda.py:47-59).
 */
#ifndef S360_H
#define S360_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define S360_ABI_VERSION 25
#define S360_MAX_VIEWS 8
#define S360_TILE 16

enum {
    S360_OK = 0,
    S360_E_BADARG = -1,    /* null pointer / non-positive size / V > S360_MAX_VIEWS */
    S360_E_WORKSPACE = -2, /* workspace smaller than s360_layout() reports */
    S360_E_LAUNCH = -3,    /* hipGetLastError() != hipSuccess after a launch */
    S360_E_UNSUPPORTED = -4
};

/* flags */
#define S360_FLAG_SHARED_CAMPOS 1u    /* all V views share campos (and scale): SH->RGB evaluated once per Gaussian */
#define S360_FLAG_FORWARD_ONLY 8u     /* inference: skip the instance-slot tables (only s360_backward needs them);
                                         s360_backward returns S360_E_BADARG on a workspace rendered with this flag */
#define S360_FLAG_COV9 2u             /* covariances given (and their gradient returned) as [P,3,3] row-major, the
                                         reference's Gaussians.covariances layout (src/model/types.py:9); only the
                                         upper triangle is read / receives gradient, exactly like the
                                         cov[:, row, col] gather at cuda_splatting.py:115,123 */
#define S360_FLAG_SH_CHANNEL_MAJOR 4u /* SH given (and gradient returned) as [P,3,M], the reference's
                                         Gaussians.harmonics layout (types.py:10) — no "b g xyz n -> b g n xyz"
                                         rearrange copy (cuda_splatting.py:75) */

/*
 * One camera: the per-call fields of GaussianRasterizationSettings (cuda_splatting.py:99-112)
 * plus the scale-invariant factor of cuda_splatting.py:64-71 and the view's near/far.  44 floats, DEVICE memory (array
 * of V).  `scale` multiplies means3D (and scale^2 the covariances) inside the kernels — pass the
 * UNSCALED cloud and scale = 1/near to fuse the reference's three full-size rescale copies; pass
 * 1.0 when the cloud is already scaled (drop-in rasteriser call).
 * viewmatrix / projmatrix are the flat [4,4] tensors handed over at cuda_splatting.py:86-87
 * (row-vector convention: element [r][c] of the transposed matrix at index 4*r+c).
 */
#define S360_FLAG_SH_DEG4_IGNORED 16u  /* treat sh_degree 4 as degree 3: coefficients 16..24 are ignored (zero gradient).
                                         The reference always passes sh_degree = 4 (config/model/encoder/costvolume.yaml:16)
                                         to a rasteriser fork whose degree-4 table cannot be verified here;
                                         default (flag clear) = the standard real-SH degree-4 table, this flag = the
                                         behaviour of a fork that stops at the upstream 3DGS degree 3. */

#define S360_FLAG_SPHERICAL 32u        /* native equirectangular splat mode (NO reference counterpart — the
                                         reference only ever renders cube faces — specified by oracle/s360_oracle.c geo_sph):
                                         every image is an H x W equirectangular panorama rendered with the spherical
                                         projection of the encoder's ERP ray convention (src/geometry/utils360.py:93-104,
                                         148-153) and its Jacobian; views come in PAIRS (2i = the panorama camera, 2i+1 = its
                                         seam ghost: the same camera, splat centres shifted by +-W), V must be even, the call
                                         renders V/2 images [V/2,3,H,W]; viewmatrix = inverse(panorama c2w)^T, projmatrix
                                         and tanfov are ignored; sort key and near cull use the RADIAL distance;
                                         d_means2D is in pixel units */

#define S360_FLAG_LEAN_LISTS 64u       /* binning-time exact cull: a (Gaussian, tile) instance is counted, emitted, sorted and given an
                                         instance slot only if the splat can reach alpha >= 1/255 on some pixel of that 16x16 tile
                                         (the tile-sized instance of the composites' own quadrant test; upstream bins the whole 3-sigma
                                         rectangle; rectangles of more than 32 tiles are binned whole).  Skipped
                                         instances contribute to no pixel, so images, final_T, radii and every gradient are
                                         BIT-IDENTICAL to a call without the flag; tiles_touched, the sorted lists, num_instances and
                                         n_contrib (list positions) differ.  Flag clear = the upstream-compatible lists (what the
                                         integer-state parity tests compare with the oracle). */

#define S360_FLAG_DEFER_LOSS 128u       /* s360_forward_mse on a training call with loss_out != NULL: do not launch the loss reduction at
                                         the end of the forward; the first launch of s360_backward / _split / _composite on this
                                         workspace performs it (same arithmetic, same fixed order).  loss_out / partials must stay
                                         allocated until then; loss_out holds the loss only after that backward.  For training loops
                                         that read the scalar after the backward (logging) — one launch less per step. */

#define S360_FLAG_ATOMIC_GRADS 256u     /* opt-in, training calls: the backward composite adds its per-(entry, quadrant) sums straight
                                         into the pair's raster-gradient record with return-less float32 atomics instead of leaving
                                         one partial record per (instance slot, quadrant) for a deterministic gather.  No partial
                                         slots, no validity flags, no gather launch: s360_layout's backward_bytes drops from
                                         ~256 B per instance of capacity to 48 B per (view, Gaussian) pair.  The summation ORDER is
                                         then run-dependent: gradients are NOT bit-reproducible (upstream's backward is atomic and
                                         non-deterministic too).  Default (flag clear): no float atomics anywhere. */

#define S360_FLAG_SPLIT_LISTS 512u      /* long tile lists are composited SEGMENT-PARALLEL (forward and backward).  Upstream's composite (and this
                                         library's without the flag) walks a tile's depth-sorted list front to back as ONE sequential
                                         chain per pixel block; a tile list of 10-17 K entries whose pixels do not saturate — the pole
                                         clumps of a panorama: the 1 024 Gaussians of every polar ERP row land on a few face pixels,
                                         /root/reference/src/geometry/utils360.py:93-104 — then costs one wave hundreds of microseconds
                                         while the rest of the chip idles.  With the flag, an 8x8 quadrant that after the first 1 024
                                         entries of a list of more than 2 048 still holds a pixel far from saturating (T >= 1/16) hands
                                         the rest over in segments of 512 entries, one wave each: phase 1 forms every segment's own
                                         transmittance T_k per pixel, phase 2 composites the segment with the sequential rule from the
                                         pixel's true incoming transmittance T_head T_2 ... T_(k-1) (pixels that stopped earlier are
                                         skipped), a combine adds the contributions in list order.  The backward composites the same
                                         segments in parallel from the forward's transmittance behind each segment and the colour
                                         accumulated behind it.  What changes: floating-point association — a pixel's transmittance
                                         at a segment start is a product of segment products (images within 1e-6 of the sequential
                                         composite; north_star's bar is 1e-5) — and with it a stop decision where a product lands
                                         within rounding of 1e-4.  Every (pixel, entry) pair is evaluated with the same arithmetic and
                                         the same stop rule in list order.  Quadrants that do not split — every list up to 2 048
                                         entries, every quadrant that is (nearly) saturated after 1 024 — are bit-identical with and
                                         without the flag. */

#define S360_FLAG_RAW_INPUTS 1024u      /* the call is s360_forward_raw / s360_backward_raw (the workspace also keeps the 7 raw geometry
                                         words per Gaussian for the backward); required by those two, rejected by the others */

#define S360_FLAG_COOP_WALK 2048u       /* binning variant for clouds with many LARGE footprints: a rectangle of more than 32 tiles is
                                         counted (k_preprocess) and emitted (k_emit) by all 64 lanes of its wave, one tile per lane,
                                         instead of by the one lane that owns the Gaussian while 63 wait (a near splat of a uniform
                                         random cloud covers a whole 16x16-tile face).  Separately compiled instances of the two
                                         kernels: the default ones carry none of it.  Every result of the call is bit-identical with
                                         and without the flag (same counts, same slots; the order of a tile's unsorted bucket is
                                         irrelevant).  header_mirror word 2 reports how many such rectangles a call had. */

typedef struct S360View {
    float viewmatrix[16];
    float projmatrix[16];
    float campos[3];
    float tanfovx, tanfovy;
    float bg[3];
    float scale;
    float near_plane, far_plane; /* UNSCALED near / far of the view (only read when a depth map is requested) */
    float _pad;
} S360View;

typedef struct S360Params {
    int32_t P;              /* Gaussians */
    int32_t V;              /* views rendered by this call (1..S360_MAX_VIEWS) */
    int32_t H, W;           /* image size of every view */
    int32_t sh_degree;      /* active SH degree 0..4 (settings.sh_degree) */
    int32_t M;              /* SH coefficients stored per Gaussian per channel (shs.shape[1]); 0 = colors_precomp */
    uint32_t flags;         /* S360_FLAG_* */
    uint32_t max_instances; /* capacity of the binning buffers ((Gaussian,tile) pairs, "num_rendered") */
    uint32_t max_segments;  /* S360_FLAG_SPLIT_LISTS: segment slots to reserve in the workspace (44 x 256 B each); 0 = enough for every
                               list of the binning capacity to be long (max_instances / 256 slots).  A quadrant whose segments
                               do not fit is composited sequentially (never an error).  header_mirror reports how many a call used. */
    uint32_t _reserved;
    void* header_mirror;    /* NULL, or a HOST-visible (pinned / mapped) 8-byte aligned address: the forward also stores
                               (num_instances | overflow flag << 32 | sort chunks of the long lists << 33) there as one 64-bit word,
                               1 into the low half of the NEXT 64-bit word when some 8x8 quadrant of the call was worth
                               splitting (or was split) under S360_FLAG_SPLIT_LISTS's criterion — callers that set that flag
                               adaptively clear the word before a call and read it after — and the number of (Gaussian, view)
                               pairs binned over more than 32 tiles into the THIRD word (24 bytes in all; what a caller sets
                               S360_FLAG_COOP_WALK by) — the caller can size its next
                               call from the previous call's count without a device synchronisation (upstream reads the count
                               back synchronously inside every forward; this library's callers may run without that read,
                               and this is how they learn the count and the overflow flag anyway) */
} S360Params;

/* Byte offsets of every array inside the forward workspace (state kept for backward and exposed
 * for parity tests: upstream's geomBuffer / binningBuffer / imgBuffer). */
typedef struct S360Layout {
    size_t total_bytes;         /* forward workspace size */
    size_t header;              /* uint32[64]: [0]=num_instances [1]=overflow flag [2]=max tile list length [3]=merge passes needed
                                   [4]=pairs with more than 32 instance slots [5]=split (tile, quadrant) units of this call
                                   [6]=their segments (work items in seg_info) */
    size_t tiles_touched;       /* uint32[V*P] */
    size_t vis_mask;            /* uint8[P]  bit v set: Gaussian visible in view v (V <= 8).  tiles_touched is written for
                                   visible pairs only; the kernels test visibility on this byte, not on V words */
    size_t slot_base;           /* uint32[V*P][2]  word 0 (training calls): first instance slot of a visible pair (it owns
                                   `tiles_touched` consecutive slots; upstream's point_offsets scan is replaced by a block-wise
                                   reservation, so which range a pair gets is run-dependent — the ranges tile [0, num_instances));
                                   word 1 (S360_FLAG_LEAN_LISTS): bit i set = tile i of the pair's rectangle (scan order, at most
                                   32 tiles) holds an instance; the pair's slots follow its set bits */
    /* one 48-byte record per pair, stride 48 B: rec_b / rec_c = rec_a + 16 / + 32 (one cache line per gather) */
    size_t rec_a;               /* float4  x, y, -log2(e)/2 * conic.a, -log2(e) * conic.b */
    size_t rec_b;               /* float4  -log2(e)/2 * conic.c, opacity, r, g */
    size_t rec_c;               /* float4  b, radius (int32 bits), conservative cull half-extents wx, wy */
    size_t clamped;             /* uint8[V*P]   bit c set: colour channel c was clamped at 0 */
    size_t depths;              /* float[V*P]   view-space z of visible pairs (sort key) */
    size_t tile_count;          /* uint32[V*T] */
    size_t slot_ticket;         /* per-image instance-slot tickets, 256 B apart (cleared together with tile_count) */
    size_t merge_done;          /* uint32[V*T][4] completion counters of the merge passes of the long lists, + 1 ticket counter of the
                                   merge units, + uint32[V*T] sorted 4 096-key chunks per tile (cleared together with tile_count) */
    size_t seg_flag;            /* uint32[V*T*4] S360_FLAG_SPLIT_LISTS: 1 = this (tile, quadrant) handed the rest of its list over to
                                   segment waves after SEG_HEAD entries (cleared together with tile_count) */
    size_t seg_arrive;          /* uint32[V*T*4] segment waves of a split quadrant that have delivered their phase-1 result (the
                                   segment's own transmittance); cleared together with tile_count */
    size_t seg_arrive2;         /* uint32[V*T*4 + 1] ... their phase-2 result (the segment composited from its true incoming
                                   transmittance): the last one to arrive runs the per-pixel combine; + the ticket counter of the
                                   work queue; cleared together with tile_count */
    size_t tile_start;          /* uint32[V*T+1] exclusive scan (upstream ranges: [start[t], start[t+1])) */
    size_t tile_cursor;         /* uint32[V*T] */
    size_t chunk_start;         /* uint32[V*T+1] number of 4096-key sort chunks of long lists before tile t */
    size_t tile_order;          /* uint32[V*T] tile ids, longest list first (dispatch order of the composite) */
    size_t keys;                /* uint64[max_instances]  (depth bits << 32 | pair index), sorted per tile */
    size_t keys_alt;            /* uint64[max_instances]  ping-pong buffer of the long-list merge passes */
    size_t list;                /* uint32[max_instances]  sorted pair indices p = v*P + g (upstream point_list) */
    size_t final_T;             /* float[V*H*W] */
    size_t n_contrib;           /* uint32[V*H*W] */
    size_t tile_max_contrib;    /* uint32[V*T] */
    size_t strip_last;          /* uint32[V*T*4] max n_contrib of each of the four 8x8 quadrants of a tile */
    size_t slot_pair;           /* uint32[max_instances] pair index p of every instance slot (training calls): lets the backward
                                   sum the per-(instance, quadrant) partial gradients slot-parallel.  Bit 31 is set on the slots
                                   of a pair that owns more than 32 of them (a long_pairs entry): the slot-parallel pass skips
                                   those — the wave-parallel pass reads them (V * P < 2^31 is required) */
    size_t long_pairs;          /* uint32[max_instances/32 + 1]  training calls: the pairs that own more than 32 instance slots
                                   (header[4] of them, in no particular order): the backward sums their slots wave-parallel */
    size_t rgbc;                /* float4[P]  SH colour of every Gaussian (r, g, b, clamp bits) when the views share a camera
                                   centre: evaluated once per call by a streaming kernel ahead of the geometry pass */
    size_t sh_jac;              /* float[P,3,3] d(rgb_c)/d(mean) through the view direction (training calls only): lets the
                                   backward add that term to dL/dmean without re-reading the 300-byte SH slab */
    size_t surv;                /* training calls: 48-byte records of the list entries that survive the exact cull of each
                                   8x8 quadrant, in list order, written by the forward composite (centre, conic, opacity,
                                   colour, radius, list position, pair): unit (tile t, quadrant q) owns records
                                   [4 start_t + q n_t, ... + n_t), n_t = the tile's list length.  The backward composite
                                   streams them back to front instead of walking and culling the tile list a second time */
    size_t surv_count;          /* uint32[V*T*4] survivor records of a unit that lie in front of its last contributor */
    /* S360_FLAG_SPLIT_LISTS state.  Segment SLOT s = 8 * chunk_start[t] + k is segment k (list positions [512 k, 512 (k+1)))
     * of long tile t; NSEG = S360Params.max_segments slots.  Slots k = 0 of a split quadrant hold what its head wave
     * published (the exact sequential state after the head); k >= 2 the segment waves' results. */
    size_t part_c;              /* float4[NSEG*4*64]  per (slot, quadrant, pixel): the segment's colour contribution (r, g, b, depth) */
    size_t part_t;              /* float [NSEG*4*64]  ... transmittance of the segment alone (phase 1; 0: the pixel stops inside it) */
    size_t part_e;              /* float [NSEG*4*64]  ... transmittance behind the segment (phase 2) */
    size_t part_l;              /* uint32[NSEG*4*64]  ... last contributing list position + 1 (0: none); slot 0: | done << 31 */
    size_t part_n;              /* uint32[NSEG*4]     survivor records the segment appended (slot k = 1: the head's count when no
                                   later segment contributes) */
    size_t seg_c;               /* float4[NSEG*4*64]  after the combine: colour accumulated BEHIND the segment (what the backward
                                   starts its colour-behind sum from) */
    size_t seg_t;               /* float [NSEG*4*64]  after the combine: transmittance behind the segment's last entry */
    size_t seg_cnt;             /* uint32[NSEG*4]     survivor records of the segment the backward replays (0: none / not split) */
    size_t seg_info;            /* uint32[NSEG*4][2]  the segment work items of the call (header[6] of them): (tile, segment k << 2 | quadrant) */
    size_t geo7;                /* float[P,7]  S360_FLAG_RAW_INPUTS training calls: the raw scale logits + quaternion of every Gaussian */
    size_t backward_bytes;      /* size of the separate backward scratch workspace */
} S360Layout;

/*
 * The encoder's raw per-pixel outputs, as GaussianAdapterERP.forward receives them
 * (/root/reference/src/model/encoder/common/gaussian_adapter_erp.py:50-61): what s360_forward_raw / s360_backward_raw consume instead
 * of the adapter's materialised means / covariances / harmonics.  All pointers DEVICE memory.
 */
typedef struct S360RawInputs {
    const float* extrinsics;    /* [n_views,4,4] context-panorama camera-to-world (row-major) */
    const float* depths;        /* [n_views*per_view] */
    const float* raw_gaussians; /* raw_gaussians [P, 7 + 3*M]: 3 scale logits, quaternion (x,y,z,w), 3 x M SH coefficients channel-major,
                                   M = prm->M = (prm->sh_degree + 1)^2 (record widths 10, 19, 34, 55, 82 at degrees 0..4) */
    const float* sh_rotation;   /* sh_rotation [n_views, M, M]: block-diagonal Wigner-D matrices of rotate_sh (s360_sh_rotation_blocks) or NULL = identity */
    int32_t n_views, per_view;  /* P = n_views * per_view Gaussians, view-major */
    int32_t H, W, per_ray;      /* context panorama size; per_view = H*W*per_ray, ray-major */
    int32_t erp_convention;     /* as s360_adapter_forward */
    float scale_min, scale_max, eps;
} S360RawInputs;

/*
 * Where the raw words lie when the encoder's last convolution output is read in place (the *_planes entry points): channel planes
 * [n_views, C_total, H, W] instead of records.  Strides in FLOATS; word c of Gaussian gi (gi = ray * per_ray + surface) of view v is at
 *     raw_gaussians + v * view_stride + (gi % per_ray) * surface_stride + c * channel_stride + gi / per_ray
 * (ray stride 1); raw_gaussians / d_raw_gaussians point at word 0 of view 0, surface 0, ray 0 — channels in front of the record (the
 * reference's two offset_xy channels) are skipped by the caller's pointer, never by the kernels.
 */
typedef struct S360RawPlanes {
    int64_t view_stride;        /* >= (per_ray - 1) * surface_stride + (7 + 3*M - 1) * channel_stride + H*W */
    int64_t surface_stride;     /* >= (7 + 3*M) * channel_stride when per_ray > 1 (ignored when per_ray == 1) */
    int64_t channel_stride;     /* >= H*W */
} S360RawPlanes;

/* ABI version of the loaded library (== S360_ABI_VERSION). */
int s360_abi_version(void);
const char* s360_error_string(int code);

/* Workspace layout / sizes for the given problem (pure host arithmetic). */
int s360_layout(const S360Params* prm, S360Layout* out);

/*
 * Forward: replaces upstream `rasterize_gaussians(...)` as reached from
 * GaussianRasterizer.forward (call site cuda_splatting.py:117-124).
 *   views[V] (device)  means3D[P,3]  cov6[P,6] (cov3D_precomp, order 00,01,02,11,12,22; [P,3,3] with
 *   S360_FLAG_COV9)  opacities[P]  shs[P,M,3] ([P,3,M] with S360_FLAG_SH_CHANNEL_MAJOR) or NULL
 *   colors_precomp[P,3] or NULL (exactly one of shs / colors_precomp non-NULL)
 * Outputs: images[V,3,H,W], radii[V,P] (int32), plus state in `workspace`.
 */
int s360_forward(const S360Params* prm, const S360View* views, const float* means3D,
                 const float* cov6, const float* opacities, const float* shs,
                 const float* colors_precomp, float* images, int32_t* radii, void* workspace,
                 size_t workspace_bytes, void* stream);

/*
 * Forward with a fused depth map: colour AND the alpha-premultiplied expected depth of
 * render_depth_cuda (cuda_splatting.py:226-269: camera-space z of every Gaussian composited with the
 * colour weights, background 0, not normalised) in ONE pass instead of a second full rasterisation
 * (decoder_splatting_cuda.py:72-97 renders every face twice when depth is wanted).
 *   depth_mode: S360_DEPTH_* (the reference's DepthRenderingMode); depth_maps[V,H,W].
 * The depth map is differentiable: pass dL_ddepth to s360_backward — the reference's
 * training step can request depth (model_wrapper_erp.py:228, train_cfg.depth_mode) and LossDepth
 * (src/loss/loss_depth.py:37-60) back-propagates through it into means, covariances and opacities.
 */
#define S360_DEPTH_DEPTH 0
#define S360_DEPTH_DISPARITY 1
#define S360_DEPTH_RELATIVE_DISPARITY 2
#define S360_DEPTH_LOG 3
int s360_forward_depth(const S360Params* prm, const S360View* views, const float* means3D,
                       const float* cov6, const float* opacities, const float* shs,
                       const float* colors_precomp, float* images, float* depth_maps, int32_t depth_mode,
                       int32_t* radii, void* workspace, size_t workspace_bytes, void* stream);

/*
 * Forward with the cube-face loss epilogue fused into the composite store: replaces the
 * torch ops the reference runs on the rendered faces right after the decoder —
 *   LossMse.forward       src/loss/loss_mse.py:30-31   weight * mean((color - target)^2)
 *   compute_psnr          src/evaluation/metrics.py:11-21   -10 log10(mean((clip01(gt) - clip01(pred))^2))
 * and the loss's autograd seed.  target[V,3,H,W]; d_images[V,3,H,W] = grad_scale * (image - target) (pass
 * grad_scale = 2*weight/N, N = elements averaged over); partials[V*tiles*4, 2] = per 8x8 quadrant of every tile (in
 * tile order) the sums of squared differences, plain and clipped — summed in a fixed order
 * by the caller, or (loss_out != NULL) by one more small launch of the same call: loss_out[0] = (grad_scale / 2) * sum
 * of all plain partials (= weight * mean over the N elements), loss_out[1 + v] = clipped MSE of view v.  Deterministic
 * either way.  depth_maps may be null (no depth channel).
 */
int s360_forward_mse(const S360Params* prm, const S360View* views, const float* means3D,
                     const float* cov6, const float* opacities, const float* shs,
                     const float* colors_precomp, float* images, float* depth_maps, int32_t depth_mode,
                     int32_t* radii, const float* target, float grad_scale, float* d_images, float* partials,
                     float* loss_out, void* workspace, size_t workspace_bytes, void* stream);

/*
 * Backward: replaces upstream `rasterize_gaussians_backward(...)` (autograd backward of the
 * call above).  `workspace` is the forward workspace, unmodified since s360_forward.
 *   dL_dimages[V,3,H,W]; dL_dimages_scale: NULL, or a DEVICE pointer to one float every element of dL_dimages is
 *   multiplied by as it is read (the scalar autograd hands back for a loss whose seed is already stored — the
 *   d_images of s360_forward_mse — or an AMP loss scale: no separate elementwise pass, no host read)
 *   dL_ddepth[V,H,W] / depth_mode: gradient of the fused depth map of s360_forward_depth (same depth_mode as the
 *   forward); NULL: no depth channel (e.g. the forward was s360_forward).
 * Outputs (all written, no accumulation into caller data):
 *   d_means3D[P,3]  d_means2D[V,P,3] (NDC-scaled screen-space gradient, z = 0)
 *   d_cov6[P,6]  d_opacities[P]  d_shs[P,M,3] or NULL  d_colors[P,3] or NULL  (d_cov6 / d_shs in the
 *   layouts selected by the flags; gradients are w.r.t. the UNSCALED inputs).  d_shs == NULL (harmonics
 *   frozen) still propagates dRGB/d(view direction) into d_means3D, as upstream does.
 * Gradients are summed over the V views with a fixed (deterministic) order; no float atomics anywhere.
 */
int s360_backward(const S360Params* prm, const S360View* views, const float* means3D,
                  const float* cov6, const float* opacities, const float* shs,
                  const float* colors_precomp, const void* workspace, size_t workspace_bytes,
                  const float* dL_dimages, const float* dL_dimages_scale,
                  const float* dL_ddepth, int32_t depth_mode, float* d_means3D, float* d_means2D,
                  float* d_cov6, float* d_opacities, float* d_shs, float* d_colors, void* bwd_workspace,
                  size_t bwd_workspace_bytes, void* stream);

/*
 * Split backward for multi-GPU view sharding (no reference counterpart: the reference all-reduces encoder
 * parameters under DDP, src/main.py:117-130).  dL/dSH of one rendered panorama is, per Gaussian, the rank-1
 * product Y(dir) (x) dL/dRGB; summing it over N ranks by all-reducing N full 300-byte slabs moves 25x more
 * bytes than exchanging the factors.  s360_backward_split() is s360_backward() for views sharing one camera
 * centre (S360_FLAG_SHARED_CAMPOS) WITHOUT the dL/dSH pass: it returns d_means3D (complete, including this rank's
 * view-direction term — the forward keeps d(rgb)/d(mean) per Gaussian, S360Layout.sh_jac), d_cov6, d_opacities and
 * d_rgb_sum[P,4] = (clamp-masked sum of dL/dRGB, index of the first view that saw the Gaussian or -1 as int32
 * bits).  After all-gathering d_rgb_sum (with .w rewritten to the index of the owning rank's representative view,
 * or -1) and one S360View per rank, s360_sh_backward() writes the summed dL/dSH = sum_ranks Y(dir_rank) (x) dRGB_rank
 * (it reads neither the SH coefficients nor any gradient buffer: 16 B in per Gaussian and rank, 300 B out).
 */
int s360_backward_split(const S360Params* prm, const S360View* views, const float* means3D,
                        const float* cov6, const float* opacities, const float* shs,
                        const void* workspace, size_t workspace_bytes,
                        const float* dL_dimages, const float* dL_dimages_scale, const float* dL_ddepth,
                        int32_t depth_mode, float* d_means3D, float* d_means2D, float* d_cov6,
                        float* d_opacities, float* d_rgb_sum, void* bwd_workspace,
                        size_t bwd_workspace_bytes, void* stream);
int s360_sh_backward(const S360Params* prm, int32_t n_groups, const S360View* views,
                     const float* means3D, const float* d_rgb_sums /* [n_groups,P,4] */, float* d_shs,
                     void* stream);

/*
 * The backward in two parts, for the chunked multi-GPU gradient exchange (no reference counterpart: the reference leaves the
 * gradient exchange to Lightning DDP, src/main.py:117-130; here the per-Gaussian gradients of one panorama per rank are summed
 * over the ranks INSIDE the rasteriser's backward, and the exchange of one Gaussian range runs while the next range is still
 * being computed):
 *   s360_backward_composite   every (tile, quadrant) replay + the per-pair sum -> state in bwd_workspace (no outputs);
 *   s360_backward_gaussians   the per-Gaussian chains of Gaussians [g_begin, g_begin + g_count) from that state (views sharing
 *                             one camera centre, SH given): d_packed[P,10] rows (d_mean 3 | the 6 unique d_covariance entries |
 *                             d_opacity — the unit one all-reduce moves; complete d_mean incl. this rank's view-direction term),
 *                             d_rgb_sum[P,4] rows (clamp-masked sum of dL/dRGB; .w = rank_stamp as int32 bits where the Gaussian
 *                             was visible to this call, else -1 — what s360_sh_backward expects after the all-gather),
 *                             optional d_means2D[V,P,3].  s360_backward_split == composite + gaussians over the whole cloud.
 *   s360_unpack_gradients     packed[P,10] (after the all-reduce) -> d_means3D[P,3], d_cov ([P,3,3] upper triangle with cov9 != 0,
 *                             else [P,6]), d_opacities[P].
 */
int s360_backward_composite(const S360Params* prm, const S360View* views, const void* workspace, size_t workspace_bytes,
                            const float* dL_dimages, const float* dL_dimages_scale, const float* dL_ddepth, int32_t depth_mode,
                            void* bwd_workspace, size_t bwd_workspace_bytes, void* stream);
int s360_backward_gaussians(const S360Params* prm, const S360View* views, const float* means3D, const float* cov6,
                            const float* shs, const void* workspace, size_t workspace_bytes, int32_t with_depth,
                            int32_t depth_mode, int32_t g_begin, int32_t g_count, int32_t rank_stamp, float* d_packed,
                            float* d_means2D, float* d_rgb_sum, void* bwd_workspace, size_t bwd_workspace_bytes, void* stream);
int s360_unpack_gradients(const float* packed, int32_t P, int32_t cov9, float* d_means3D, float* d_cov, float* d_opacities,
                          void* stream);
/* Where s360_backward* leave the per-pair raster-gradient records inside bwd_workspace (ABI v25): byte offset of float[V*P][12],
 * pair v P + g — words 0..1 dL/dx, dL/dy of the centre in pixels | 2..4 dL/dA, dL/dB, dL/dC of the conic | 5 dL/dopacity |
 * 6..8 dL/dr, g, b | 9 dL/d(depth value) | 10..11 unused —, valid after s360_backward_composite or any s360_backward* call on that
 * workspace (the per-Gaussian kernels only read them; records of pairs the forward culled are never written nor read).  The
 * records start on a 256-byte boundary of the ADDRESS, so the offset belongs to the bwd_workspace pointer it was asked for.
 * Host arithmetic only; launches nothing and dereferences nothing.  A null prm / bwd_workspace / byte_offset or a
 * S360_FLAG_FORWARD_ONLY parameter set: S360_E_BADARG; bwd_workspace_bytes < backward_bytes: S360_E_WORKSPACE.  For tests and
 * diagnostics: it covers the S360_FLAG_ATOMIC_GRADS layout and the default one. */
int s360_backward_pair_records(const S360Params* prm, const void* bwd_workspace, size_t bwd_workspace_bytes, size_t* byte_offset);
/* The all-gather form of the exchange (up to two ranks: one collective per Gaussian range instead of two): packed_blocks holds n_blocks
 * gathered [g_count,10] row blocks, one per rank, back to back; their sum (rank order: the same bits on every rank) is written to rows
 * [g_begin, g_begin + g_count) of d_means3D / d_cov / d_opacities — the local reduction and s360_unpack_gradients in one pass. */
int s360_reduce_unpack_gradients(const float* packed_blocks, int32_t n_blocks, int32_t g_begin, int32_t g_count, int32_t cov9,
                                 float* d_means3D, float* d_cov, float* d_opacities, void* stream);

/*
 * Camera records of a call in one launch: replaces the reference's per-call camera glue
 * (cuda_splatting.py:64-71 scale-invariant rescale, :80-84 get_fov / get_projection_matrix, :85-87 the two
 * transposed matrices; src/geometry/projection.py:233-247) — ~60 tiny torch / rocSOLVER launches for six cameras.
 *   extrinsics[N,4,4] camera-to-world (OpenCV), intrinsics[N,3,3] normalised, near / far[N],
 *   background[3] (background_per_view = 0) or [N,3] (1), scale_invariant as in render_cuda.
 *   views_out[N]: S360View records (near_plane / far_plane = the UNSCALED planes).
 * Same formulas in the same order as the reference; the two matrix inverses are Gauss-Jordan eliminations
 * with partial pivoting, so the records agree with the torch glue to a few ulp, not bit for bit.
 */
int s360_pack_views(const float* extrinsics, const float* intrinsics, const float* near_planes,
                    const float* far_planes, const float* background, int32_t background_per_view,
                    int32_t n_views, int32_t scale_invariant, S360View* views_out, void* stream);

/*
 * Gaussian-adapter tail: the producer of the per-Gaussian buffers this library rasterises — replaces
 * GaussianAdapterERP.forward (/root/reference/src/model/encoder/common/gaussian_adapter_erp.py:50-119: scale map :63-78,
 * quaternion normalisation :82, sh_mask :38-47,86, world covariance :89-92 with build_covariance of
 * common/gaussians.py:33-44, sphere un-projection src/geometry/sphere_projection.py:6-86 in the ERP convention of the dataset,
 * src/geometry/utils360.py:37-153: erp_convention 0 = 'hm3d' / 'replica' (the reference's configs), 1 = 'm3d',
 * 2 = 'residential', 3 = 'CoffeeArea' / 'outdoor_colmap') in one launch.
 *   extrinsics[V,4,4] context-panorama camera-to-world; depths[V,Gv]; raw_gaussians[V,Gv,7+3*d_sh] = 3 scale logits,
 *   quaternion (x,y,z,w), 3*d_sh SH coefficients channel-major; Gv = H*W*per_ray Gaussians per view, ray-major;
 *   sh_rotation[V,d_sh,d_sh] or NULL (= identity): per-view SH rotation, only the (2l+1)x(2l+1) diagonal blocks are
 *   read — the Wigner-D matrices rotate_sh (src/misc/sh_rotation.py:10-30) obtains from e3nn, built by the caller.
 * Outputs: means[V*Gv,3], covariances[V*Gv,3,3] (cov9 != 0) or [V*Gv,6] upper triangle (the rasteriser's
 * cov3D_precomp layout), harmonics[V*Gv,3,d_sh]; optional scales_out[V*Gv,3] / rotations_out[V*Gv,4] (the adapter's
 * export-only fields).  Opacities pass through the adapter unchanged and are not touched here.
 * s360_adapter_backward: gradients of (means, covariances, harmonics) -> d_depths[V,Gv], d_raw_gaussians (same layout).
 *   d_means == NULL (the reference's behaviour): the means are detached — the reference un-projects under torch.no_grad()
 *   (src/geometry/sphere_projection.py:14-86), so depth receives gradient through the scales only; a non-NULL d_means adds
 *   the un-projection's own term (this project's opt-in deviation).
 */
/*
 * The matrices of rotate_sh (src/misc/sh_rotation.py:10-30: per degree l, e3nn.o3.wigner_D(l, *matrix_to_angles(R)), applied to
 * the SH coefficient blocks at gaussian_adapter_erp.py:113 with R = the context view's camera-to-world rotation).
 *   rotations: n_views row-major 3x3 matrices, row_major_stride = 9 ([n,3,3]) or 16 (the rotation part of [n,4,4] poses);
 *   sh_rotation_out[n_views, d_sh, d_sh]: block-diagonal, block l = D^l(R) with Y^l(R d) = D^l(R) Y^l(d) in e3nn's real basis
 *   (polar axis y, azimuth from z towards x, m = -l..l, no Condon-Shortley phase; D^1 = R) — the `sh_rotation` argument of
 *   s360_adapter_forward / backward.  e3nn itself is not available where this was written: the convention is restated from its
 *   documentation and pinned by properties only (oracle/adapter_ref.py).
 */
/*
 * The adapter tail FUSED into the rasteriser: replaces GaussianAdapterERP.forward
 * (gaussian_adapter_erp.py:63-119) + the decoder's rasteriser call on its output (cuda_splatting.py:99-124) for views sharing one
 * camera centre, at SH degrees 0..4 (the reference's configuration is degree 4).  The call's first kernel reads the raw records once
 * (40 / 76 / 136 / 220 / 328 B per Gaussian at degrees 0..4), writes means_out[P,3] and cov6_out[P,6] (the adapter's values: what the
 * geometry pass then reads, and what a caller may keep) and evaluates the view-dependent colour with the SH basis carried through
 * sh_mask and the per-view rotation — the [P,3,M] harmonics and [P,3,3] covariances are never materialised (340 B/Gaussian written +
 * 340 read by the two-step path at degree 4).
 * prm: P = raw->n_views * raw->per_view, sh_degree in 0..4, M = (sh_degree + 1)^2 exactly (the record holds that many coefficients per
 * channel), flags must hold S360_FLAG_RAW_INPUTS | S360_FLAG_SHARED_CAMPOS and not S360_FLAG_COV9.  All three raw entry points answer
 * a degree outside 0..4 or M > (sh_degree + 1)^2 with S360_E_UNSUPPORTED, and M < (sh_degree + 1)^2 with S360_E_BADARG (as s360_forward).
 * target == NULL: no loss epilogue (d_images / partials / loss_out ignored); depth_maps == NULL: no depth channel.
 * s360_backward_raw: the backward of that call down to the encoder's outputs — d_depths[P], d_raw_gaussians [P, 7 + 3*M] (dL/d(SH
 * coefficient) formed as (mask . D^T Y) (x) dL/dRGB: the [P,3,M] dL/dSH round trip of the two-step path does not exist),
 * d_opacities[P]; d_means3D[P,3], d_cov6[P,6], d_rgb_sum[P,4] are caller-provided intermediates (valid results themselves).
 * differentiable_means = 0: the reference's detached means (sphere_projection.py:14-86 runs under torch.no_grad()); 1 adds the
 * un-projection's own depth term.  means / cov6: what s360_forward_raw wrote.
 */
int s360_forward_raw(const S360Params* prm, const S360View* views, const S360RawInputs* raw, const float* opacities,
                     float* means_out, float* cov6_out, float* images, float* depth_maps, int32_t depth_mode, int32_t* radii,
                     const float* target, float grad_scale, float* d_images, float* partials, float* loss_out, void* workspace,
                     size_t workspace_bytes, void* stream);
int s360_backward_raw(const S360Params* prm, const S360View* views, const S360RawInputs* raw, const float* means, const float* cov6,
                      const float* opacities, const void* workspace, size_t workspace_bytes, const float* dL_dimages,
                      const float* dL_dimages_scale, const float* dL_ddepth, int32_t depth_mode, int32_t differentiable_means,
                      float* d_means3D, float* d_cov6, float* d_opacities, float* d_rgb_sum, float* d_depths, float* d_raw_gaussians,
                      void* bwd_workspace, size_t bwd_workspace_bytes, void* stream);
/*
 * The last kernel of s360_backward_raw on its own, for the multi-GPU exchange on the raw path (no reference counterpart: the reference
 * leaves the gradient exchange to Lightning DDP, /root/reference/src/main.py:117-130): s360_backward_composite +
 * s360_backward_gaussians produce the rows the exchange moves (packed[P,10], d_rgb_sum[P,4]); after it, d_cov6 [, d_means3D] hold the
 * sums over the ranks and d_rgb_sums[n_groups,P,4] one clamp-masked dL/dRGB sum per rank (.w = index of that rank's record in
 * group_views[n_groups], int32 bits, or -1) — exactly k_raw_bwd's inputs: dL/d(SH coefficient) = sum over groups of
 * (mask . D^T Y(dir_group)) (x) dL/dRGB_group.  d_means3D == NULL: the reference's detached means.
 */
int s360_backward_raw_tail(const S360Params* prm, const S360View* group_views, int32_t n_groups, const S360RawInputs* raw,
                           const float* means, const void* workspace, size_t workspace_bytes, const float* d_means3D,
                           const float* d_cov6, const float* d_rgb_sums, float* d_depths, float* d_raw_gaussians, void* stream);
/*
 * The three raw entry points with the raw words read, and their gradient written, as CHANNEL PLANES (S360RawPlanes above) — the
 * layout the reference's encoder leaves them in ("(v b) c h w" out of its last convolution, depth_predictor_multiview_360.py:672-674):
 * raw->raw_gaussians and d_raw_gaussians are addressed through `planes`, everything else is the record entry's argument, rule and
 * result, bit for bit (the kernels differ in their staging loads and their last stores only).  d_raw_gaussians: the kernel writes the
 * 7 + 3*M gradient words of every one of the P records at the addresses above and nothing else — channels the records do not cover,
 * and padding between views, belong to the caller (zero them, or not).  S360_E_BADARG before any GPU work for planes == NULL,
 * channel_stride < H*W, surface_stride < (7 + 3*M) * channel_stride with per_ray > 1, or a view_stride below the extent of one view's
 * per_ray surfaces; otherwise the record entries' own answers.  The S360_RAW_MFMA=1 experiment rotates records and has no plane form:
 * s360_forward_raw_planes answers S360_E_UNSUPPORTED under it.
 */
int s360_forward_raw_planes(const S360Params* prm, const S360View* views, const S360RawInputs* raw, const S360RawPlanes* planes,
                            const float* opacities, float* means_out, float* cov6_out, float* images, float* depth_maps,
                            int32_t depth_mode, int32_t* radii, const float* target, float grad_scale, float* d_images, float* partials,
                            float* loss_out, void* workspace, size_t workspace_bytes, void* stream);
int s360_backward_raw_planes(const S360Params* prm, const S360View* views, const S360RawInputs* raw, const S360RawPlanes* planes,
                             const float* means, const float* cov6, const float* opacities, const void* workspace, size_t workspace_bytes,
                             const float* dL_dimages, const float* dL_dimages_scale, const float* dL_ddepth, int32_t depth_mode,
                             int32_t differentiable_means, float* d_means3D, float* d_cov6, float* d_opacities, float* d_rgb_sum,
                             float* d_depths, float* d_raw_gaussians, void* bwd_workspace, size_t bwd_workspace_bytes, void* stream);
int s360_backward_raw_tail_planes(const S360Params* prm, const S360View* group_views, int32_t n_groups, const S360RawInputs* raw,
                                  const S360RawPlanes* planes, const float* means, const void* workspace, size_t workspace_bytes,
                                  const float* d_means3D, const float* d_cov6, const float* d_rgb_sums, float* d_depths,
                                  float* d_raw_gaussians, void* stream);
int s360_sh_rotation_blocks(const float* rotations, int32_t row_major_stride, int32_t n_views, int32_t d_sh,
                            float* sh_rotation_out, void* stream);
int s360_adapter_forward(const float* extrinsics, const float* depths, const float* raw_gaussians,
                         const float* sh_rotation, int32_t n_views, int32_t per_view, int32_t H, int32_t W,
                         int32_t per_ray, int32_t d_sh, float scale_min, float scale_max, float eps, float* means,
                         float* covariances, int32_t cov9, float* harmonics, float* scales_out,
                         float* rotations_out, int32_t erp_convention, void* stream);
int s360_adapter_backward(const float* extrinsics, const float* depths, const float* raw_gaussians,
                          const float* sh_rotation, int32_t n_views, int32_t per_view, int32_t H, int32_t W,
                          int32_t per_ray, int32_t d_sh, float scale_min, float scale_max, float eps,
                          const float* d_means, const float* d_covariances, int32_t cov9, const float* d_harmonics,
                          float* d_depths, float* d_raw_gaussians, int32_t erp_convention, void* stream);

/*
 * Cube -> equirectangular stitch: replaces Cube2Equirec.forward
 * (/root/reference/src/geometry/layers.py:108-116, F.grid_sample trilinear / border /
 * align_corners=True over the [C,6,fw,fw] face stack).
 *   faces[6,C,fw,fw] in Cube2Equirec's slot order (F R B L U D) when face_map == NULL, else
 *   slot s reads faces[face_map[s] & 7] and, when bit 3 of face_map[s] is set, flipped on both
 *   image axes — face_map = {3, 4, 1, 2, 0|8, 5|8} applies the reference's change_order()
 *   (src/model/model_wrapper_erp.py:135-145) to faces given in rendered order (U B L F R D)
 *   without materialising the permuted copy.  face_map_host is read on the HOST.
 *   grid[eh,ew,3] = Cube2Equirec.sample_grid (u, v, face-z);  erp[C,eh,ew].
 *   strides_host (HOST, 3 x int64, element units, may be NULL = dense [6,C,fw,fw]): strides between
 *   faces, channels and rows of `faces`; {fw, fw*6*fw, 6*fw} reads the reference's own
 *   [C,fw,6*fw] "faces side by side" input of Cube2Equirec.forward (layers.py:108-113) in place.
 */
int s360_cube2erp_forward(const float* faces, const float* grid, float* erp, int32_t channels,
                          int32_t face_w, int32_t equ_h, int32_t equ_w,
                          const int32_t* face_map_host, const int64_t* strides_host, void* stream);

/* Adjoint of the stitch (ABI v24): every element of d_faces[6,C,fw,fw] (same face order / face_map as forward) is WRITTEN,
 * no memset and no atomics: the result is bit-identical from call to call.
 *   plan_offsets[6*fw*fw + 1], plan_entries[plan_offsets[6*fw*fw]] (device, int32): the grid's inverse in Cube2Equirec's
 *   SLOT space — texel t = s*fw*fw + y*fw + x of slot s is read by the pixels plan_entries[plan_offsets[t] .. plan_offsets[t+1])
 *   as pixel*8 + tap (tap = 4*dz + 2*dy + dx), sorted by pixel; every in-range tap appears once, weight-0 taps included
 *   (splatter360_amd/stitch.py adjoint_plan builds it from the grid; one plan serves every face_map).  The kernel recomputes
 *   each weight from `grid` with the forward's float32 expressions and sums a texel's entries in plan order.  A face that no
 *   slot reads gets zeros.  equ_h * equ_w * 8 must fit in int32.  strides_host must be NULL (dense output only). */
int s360_cube2erp_backward(const float* d_erp, const float* grid, const int32_t* plan_offsets,
                           const int32_t* plan_entries, float* d_faces,
                           int32_t channels, int32_t face_w, int32_t equ_h, int32_t equ_w,
                           const int32_t* face_map_host, const int64_t* strides_host, void* stream);

/*
 * z-depth -> ray distance (csrc/s360_stitch.hip): replaces depth_to_distance_map_batch
 * (/root/reference/src/geometry/z_depth_to_distance.py:4-34), sqrt(X^2 + Y^2 + d^2) with X = (u - cx) d / fx, Y = (v - cy) d / fy,
 * computed as |d| s, s = sqrt(((u - cx) / fx)^2 + ((v - cy) / fy)^2 + 1), in float64 from the float32 inputs and rounded once.
 * Additive entries: the ABI version stays.  One launch per call on `stream`, no workspace, no atomics, no host synchronisation.
 *   depth[n, height, width] float32; fxfycxcy[n, 4] float32 (fx, fy, cx, cy in pixels), one row per map, read on the device (the
 *   reference's [n, 4, h, w] broadcast, src/model/model_wrapper_erp.py:450-455, is never formed); distance[n, height, width].
 *   convention S360_D2D_REFERENCE: u is the ROW index and v the column index, as the reference's "ij" meshgrid of
 *     (arange(width), arange(height)) pairs them (:18-21); height == width is required, as it is for the reference to broadcast.
 *   convention S360_D2D_PIXEL: u is the column (x with fx, cx), v the row (y with fy, cy); any height, width.
 *   d = 0 gives 0, d < 0 gives |d| s, inf and NaN propagate.
 * s360_depth_to_distance_backward: d_depth = d_distance sign(d) s in float64, rounded once; 0 at d = 0, where torch's autograd of
 *   the reference's sqrt gives NaN.  The intrinsics take no gradient.
 * Null pointers, sizes < 1, an unknown convention, height != width under S360_D2D_REFERENCE: S360_E_BADARG before any GPU work.
 */
#define S360_D2D_REFERENCE 0
#define S360_D2D_PIXEL 1
int s360_depth_to_distance_forward(const float* depth, const float* fxfycxcy, float* distance, int32_t n, int32_t height,
                                   int32_t width, int32_t convention, void* stream);
int s360_depth_to_distance_backward(const float* d_distance, const float* depth, const float* fxfycxcy, float* d_depth, int32_t n,
                                    int32_t height, int32_t width, int32_t convention, void* stream);

/*
 * Depth faces -> ERP distance panorama in one launch: replaces change_order_batch, depth_to_distance_map_batch and Cube2Equirec as
 * the evaluation step chains them (/root/reference/src/model/model_wrapper_erp.py:445-463, :147-158), without the flipped /
 * reordered copy, the distance faces or the intrinsics broadcast, and without writing to the input.  It is s360_cube2erp_forward
 * with one channel, n panoramas (gridDim.y) and each tap value replaced by float32(|d_tap| s): bit-identical to
 * s360_depth_to_distance_forward followed by s360_cube2erp_forward.
 *   depth_faces[n, 6, fw, fw] float32, face order / face_map_host as for s360_cube2erp_forward; fxfycxcy[n, 6, 4]; grid[eh, ew, 3];
 *   erp[n, eh, ew].
 *   convention S360_D2D_REFERENCE: converted in SLOT space, after the reorder, as the reference does — slot s uses row s of
 *     fxfycxcy and the slot-space texel position (u = row), so a flipped face sees (fw - 1 - u) - cx where its own image has u - cx.
 *   convention S360_D2D_PIXEL: each face converted in its own image — slot s uses row face_map[s] & 7 and the source texel position.
 *   strides_host (HOST, 3 x int64, element units, may be NULL = dense): strides between panoramas, faces and rows of depth_faces.
 * s360_cube2erp_distance_backward: d_depth_faces[n, 6, fw, fw], every element written, no atomics — per slot-space texel the
 *   plan-ordered float32 sum of s360_cube2erp_backward (same plan_offsets / plan_entries), then one multiply by sign(d) s in
 *   float64, rounded once.  strides_host must be NULL (S360_E_UNSUPPORTED otherwise).
 * Null pointers, sizes < 1, n > 65535, n eh ew 8 or 6 fw fw + 1 beyond int32, a face-map source > 5, an unknown convention:
 * S360_E_BADARG before any GPU work.
 */
int s360_cube2erp_distance_forward(const float* depth_faces, const float* fxfycxcy, const float* grid, float* erp, int32_t n,
                                   int32_t face_w, int32_t equ_h, int32_t equ_w, int32_t convention,
                                   const int32_t* face_map_host, const int64_t* strides_host, void* stream);
int s360_cube2erp_distance_backward(const float* d_erp, const float* depth_faces, const float* fxfycxcy, const float* grid,
                                    const int32_t* plan_offsets, const int32_t* plan_entries, float* d_depth_faces, int32_t n,
                                    int32_t face_w, int32_t equ_h, int32_t equ_w, int32_t convention,
                                    const int32_t* face_map_host, const int64_t* strides_host, void* stream);

/*
 * Mean SSIM per image for the evaluation step: replaces compute_ssim (src/evaluation/metrics.py:38-54), which copies every
 * face to the host and calls skimage.metrics.structural_similarity(gt, hat, win_size=11, gaussian_weights=True,
 * channel_axis=0, data_range=1.0) one image at a time.  Same algorithm:
 *   Gaussian window sigma 1.5, truncate 3.5 (11 taps, normalised);  sample covariance, cov_norm = 121 / 120;
 *   C1 = (0.01 * 1)^2, C2 = (0.03 * 1)^2;
 *   S = (2 mx my + C1)(2 vxy + C2) / ((mx^2 + my^2 + C1)(vx + vy + C2)) per pixel;
 *   per channel the float64 mean of S over the interior rows / columns [5, H-5) x [5, W-5) (the reflect-padded border is
 *   cropped away and never reaches it), per image the mean over channels.  Inputs are not clipped.
 *   pred, gt[n_images, channels, height, width] contiguous float32 (the score is symmetric in them);  ssim_out[n_images] float32.
 *   height or width < 11: S360_E_BADARG (skimage raises ValueError there).
 * workspace == NULL: *workspace_bytes receives the size of the workspace (8-byte aligned, device memory) and nothing runs.
 * Otherwise two kernels run on `stream`; no atomics: the result is bit-identical from call to call, and image i's score does
 * not depend on the other images of the call.
 */
int s360_ssim(const float* pred, const float* gt, int32_t n_images, int32_t channels, int32_t height, int32_t width,
              float* ssim_out, void* workspace, size_t* workspace_bytes, void* stream);

/*
 * The training step's context-depth loss (src/model/model_wrapper_erp.py:242-287), forward and backward, on the GPU.
 *
 * s360_erode replaces erode (src/model/model_wrapper_helper.py:4-24): out = 1 - max over the ksize x ksize window of (1 - x),
 * with reflect padding by (ksize - 1) / 2 (index -1 -> 1, H -> H - 2; no longitude wrap), on n_planes contiguous float32
 * [height, width] planes.  Bit-identical to torch's 1 - max_pool2d(F.pad(1 - x, mode="reflect")) for any input; a NaN in the
 * window gives NaN.  ksize odd and (ksize - 1) / 2 < height, width, else S360_E_BADARG.
 *
 * s360_l1_sphere_forward replaces compute_l1_sphere_loss (model_wrapper_helper.py:63-90):
 *   loss = sum |t - p| (w_h m) / den',  den' = clamp_away_from(sum w_h m, 0, 1e-10)  (>= 0: max(den, 1e-10), else
 *   min(den, -1e-10), NaN stays NaN), over [views, height, width] per batch element (keep_batch != 0: loss_out[batch],
 *   den_out[batch]) or over everything (loss_out[1], den_out[1]).  pred, target, mask[batch, views, height, width] contiguous
 *   float32 device memory; row_weights[height] = sin((h + 0.5) pi / height) as the caller computes it (the reference's float32
 *   expression).  Each term is the float32 |t - p| * (w_h * m), summed in float64; num and den are rounded to float32 before the
 *   clamp and the float32 division.  A zero-weight term is still added (NaN * 0 gives NaN, as in the reference).
 *   mask == NULL selects the fused closure of model_wrapper_erp.py:245-258: m = erode(target > near_threshold, ksize) and
 *   t = *far where target < fill_below, else target (target is the unfilled depth; far is a DEVICE float scalar; ksize odd,
 *   <= 17).  The erosion is unconditional: eroding an all-ones mask gives all ones, so no `.all()` test is needed.  The fused
 *   loss is bit-identical to this function fed with s360_erode's mask and the filled target.  far, near_threshold,
 *   fill_below and ksize are ignored when mask != NULL.
 *   workspace == NULL: *workspace_bytes receives the workspace size (16-byte aligned device memory) and nothing runs.
 *   Otherwise two kernels run on `stream`; no atomics, no memset, no host synchronisation: results are bit-identical from
 *   call to call, and with keep_batch element i's loss does not depend on the other elements.
 *
 * s360_l1_sphere_backward: torch's autograd chain of the forward, elementwise, given grad_loss (the incoming gradient: [batch]
 * with keep_batch, else [1]) and den (the forward's den_out):
 *   grad_pred = -(((grad_loss / den) * (w_h * m)) * sgn(t - p)),  sgn(0) = 0 and sgn(NaN) = 0 (torch's sign),
 *   grad_target = -grad_pred, written only when grad_target != NULL.
 * mask, target, far, near_threshold, fill_below and ksize as in the forward (mask == NULL: the fused mode, mask recomputed).
 * One kernel on `stream`; every element of grad_pred (and grad_target) is written.
 */
int s360_erode(const float* x, float* out, int32_t n_planes, int32_t height, int32_t width, int32_t ksize, void* stream);
int s360_l1_sphere_forward(const float* pred, const float* target, const float* mask, const float* row_weights,
                           int32_t batch, int32_t views, int32_t height, int32_t width, int32_t keep_batch,
                           const float* far, float near_threshold, float fill_below, int32_t ksize,
                           float* loss_out, float* den_out, void* workspace, size_t* workspace_bytes, void* stream);
int s360_l1_sphere_backward(const float* pred, const float* target, const float* mask, const float* row_weights,
                            int32_t batch, int32_t views, int32_t height, int32_t width, int32_t keep_batch,
                            const float* far, float near_threshold, float fill_below, int32_t ksize,
                            const float* grad_loss, const float* den, float* grad_pred, float* grad_target, void* stream);

/*
 * The training step's depth-smoothness loss, LossDepth (src/loss/loss_depth.py:26-60), forward and backward, on the GPU
 * (csrc/s360_depth_smooth.hip).
 *
 * s360_depth_smooth_forward: depth[batch, views, height, width] contiguous float32 device memory; log_near, log_far
 * [batch, bound_views] float32 device memory, the natural logs of the bounds as the caller computes them (the reference's
 * float32 .log()); bound_views divides views and view v uses bound v / (views / bound_views).  Per pixel, in float64 on those
 * float32 values and with no FMA contraction:
 *   n = (max(min(d, log_far), log_near) - log_near) / (log_far - log_near)  (torch's minimum / maximum: a NaN stays a NaN);
 *   dx[x] = n[x + 1] - n[x] along width, dy likewise along height;  S360_DS_SECOND: dx[x] = (n[x + 2] - n[x + 1]) - (n[x + 1] - n[x]);
 *   S360_DS_BILATERAL: image[batch, views, channels, height, width] contiguous float32 (never written), c[x] = max over channels
 *   of the SIGNED difference image[x + 1] - image[x] (with S360_DS_SECOND: max(c[x + 1], c[x])), t = dx exp(-c sigma_image);
 *   else t = dx and image, channels and sigma_image are ignored;
 *   loss[1] = sum |tx| / Nx + sum |ty| / Ny, Nx = batch views height (width - order), Ny = batch views (height - order) width,
 *   order 1 or 2: float64 sums, rounded to float32 once.  log_near >= log_far or a non-finite bound gives a non-finite loss, as in
 *   the reference.
 *   workspace == NULL: *workspace_bytes receives the workspace size (16-byte aligned device memory) and nothing runs.
 *   Otherwise two kernels run on `stream`: every 32 x 64 tile writes its float64 pair to its own slot, one workgroup adds the
 *   slots in index order.  No atomics, no memset, no host synchronisation: the loss is bit-identical from call to call and
 *   from stream to stream.
 *
 * s360_depth_smooth_backward: torch's autograd chain of the forward as a gather, given grad_loss (a DEVICE float scalar):
 *   grad_depth = grad_loss (Sx / Nx + Sy / Ny) gate / (log_far - log_near),  S = sum over the terms of the axis that hold the
 *   pixel of coef sgn(t) e, coef (+1, -1) for the first and (+1, -2, +1) for the second derivative, e = exp(-c sigma_image) (or 1),
 *   sgn(0) = sgn(NaN) = 0, gate = (d > log_far ? 0 : d == log_far ? 0.5 : 1) (m < log_near ? 0 : m == log_near ? 0.5 : 1) with
 *   m = min(d, log_far): the halves torch's minimum / maximum give at a tie.  Float64, rounded to float32 once; nothing but the
 *   inputs is read.  One kernel on `stream`, no atomics; every element of grad_depth is written.  The image takes no gradient.
 *
 * Both: bound_views not dividing views, height or width <= the derivative order, channels < 1 with S360_DS_BILATERAL, an unknown
 * flag, a size < 1, a null required pointer or more than 2^31 / 256 tiles: S360_E_BADARG before any GPU work; a workspace
 * smaller than reported: S360_E_WORKSPACE.
 */
#define S360_DS_SECOND 1    /* flags bit 0: second derivative */
#define S360_DS_BILATERAL 2 /* flags bit 1: weight every term with exp(-c sigma_image) from `image` */
int s360_depth_smooth_forward(const float* depth, const float* log_near, const float* log_far, const float* image, int32_t batch,
                              int32_t views, int32_t bound_views, int32_t channels, int32_t height, int32_t width,
                              float sigma_image, int32_t flags, float* loss, void* workspace, size_t* workspace_bytes,
                              void* stream);
int s360_depth_smooth_backward(const float* depth, const float* log_near, const float* log_far, const float* image, int32_t batch,
                               int32_t views, int32_t bound_views, int32_t channels, int32_t height, int32_t width,
                               float sigma_image, int32_t flags, const float* grad_loss, float* grad_depth, void* stream);

/*
 * The other weight-free scores of the evaluation step (csrc/s360_eval_scores.hip).
 *
 * s360_depth_metrics replaces compute_depth_metrics_batched (src/scripts/compute_depth_metrics.py:47-116, called at
 * src/model/model_wrapper_erp.py:526-531) in one pass over gt, pred and the validity, for n_rows rows of n float32 elements:
 *   row r of gt starts at gt + (r / rows_per_group) * gt_group_stride + (r % rows_per_group) * gt_row_stride (elements), pred
 *   likewise — [B, N] tensors with a row stride need no copy (rows_per_group = n_rows), and faces 1..5 of every six of a
 *   [views, 6, H, W] block are rows_per_group = 5 with the pointer at face 1 and a group stride of 6 H W;
 *   validity: valid[r * valid_row_stride + e] != 0 (uint8 / bool), or, valid == NULL, gt > threshold;
 *   pred_height > 0: pred rows are [pred_height, pred_width] planes looked up at gt's [gt_height, gt_width] (= n) positions by
 *   F.interpolate(mode="nearest")'s rule, src = min(floor(float(dst) * (float(pred size) / float(gt size))), pred size - 1);
 *   pred_height == pred_width == 0: no lookup, the four sizes are ignored.
 * Per valid element, float32 IEEE operations: d = gt - pred; terms |d|, |d| / gt, (d d) / gt, d d, (log gt - log pred)^2.
 * metrics_out[12, n_rows] float32, in this order:
 *   0 abs_diff, 1 abs_rel, 2 sq_rel, 3 rmse, 4 rmse_log: the float64 sum of the term over the valid elements where that term is
 *     not NaN, divided by their number, rounded to float32 (rmse, rmse_log: then the float32 square root);
 *   5 a5, 6 a10, 7 a25, 8 a0 (= a10), 9 a1 (= a25), 10 a2, 11 a3: the number of valid elements with gt / pred < t and
 *     pred / gt < t (a NaN quotient is a miss) for the float32 t = 1.05, 1.10, 1.25, 1.25^2, 1.25^3, divided in float32 by the
 *     number of valid elements, times 100 in float32 when mult_a != 0.
 *   A row without a valid element gives NaN twelve times.  valid_count[n_rows] int32: the valid elements per row.
 * scores_out != NULL: also the evaluation step's reduction over rows (model_wrapper_erp.py:537-541), scores_out[12] float32:
 *   the float64 sum of each metric over the rows with valid_count > 0, divided by the number of such rows (none: NaN).
 * workspace == NULL: *workspace_bytes receives the workspace size (8-byte aligned device memory) and nothing runs.  Otherwise
 * two kernels (three with scores_out) run on `stream`; no atomics, no host synchronisation: results are bit-identical from
 * call to call, row r's numbers do not depend on the other rows, nor on the alignment or strides of the inputs.
 *
 * s360_psnr replaces compute_psnr (src/evaluation/metrics.py:11-21; the evaluation step at model_wrapper_erp.py:485-487, the
 * training step at :234-238): per image of pred, gt[n_images, channels, height, width] contiguous float32, both clipped to
 * [0, 1] (NaN stays NaN), the float64 sum of the float32 (gt - pred)^2, the mean rounded to float32, 0 replaced by 1e-10,
 * psnr_out[n_images] = -10 log10(mean).  Workspace, stream and determinism as above; two kernels.
 */
int s360_depth_metrics(const float* gt, const float* pred, const uint8_t* valid, int32_t n_rows, int32_t n,
                       size_t gt_row_stride, size_t pred_row_stride, size_t valid_row_stride, int32_t rows_per_group,
                       size_t gt_group_stride, size_t pred_group_stride, float threshold, int32_t gt_height, int32_t gt_width,
                       int32_t pred_height, int32_t pred_width, int32_t mult_a, float* metrics_out, int32_t* valid_count,
                       float* scores_out, void* workspace, size_t* workspace_bytes, void* stream);
int s360_psnr(const float* pred, const float* gt, int32_t n_images, int32_t channels, int32_t height, int32_t width,
              float* psnr_out, void* workspace, size_t* workspace_bytes, void* stream);

/*
 * The encoder's spherical plane-sweep cost volume (csrc/s360_cost_volume.hip): the closure of the reference's
 * src/model/encoder/costvolume/depth_predictor_multiview_360.py:588-630 — warp_with_pose_depth_candidates (:159-214), the product
 * with the own view's features and the sum over channels — without the [n, C, D, h, w] warped tensor.
 *
 * s360_cost_volume_forward:
 *   out[i, d, y, x] = scale * sum_{k < pairs} sum_c f_own[i, c, y, x] * bilinear(f_partner[partner_slot[k, i], c], warp(k, i, d, y, x))
 *   f_own[n, C, h, w], f_partner[m, C, h, w], out[n, D, h, w]: contiguous float32 device memory (f_partner may be f_own);
 *   partner_slot[pairs, n] int32 device memory (NULL: slot i, needs m == n; an entry outside [0, m) contributes nothing);
 *   poses[pairs, n, 4, 4] float32 row-major, partner from own; depths[n, D] float32 depth candidates.
 *   The reference's volume is scale = 1 / (pairs sqrt(C)) with every rolled pairing in one call; one pairing's sum over channels
 *   is pairs = 1, scale = 1.
 *   warp, convention S360_CV_HM3D ('hm3d' and 'replica' of src/geometry/utils360.py:93-104,148-153,193-198,250-263; the only value,
 *   anything else is S360_E_BADARG): theta = (0.5 - (x + 0.5) / w) 2 pi, phi = -((y + 0.5) / h - 0.5) pi, p = (cos phi sin theta,
 *   sin phi, cos phi cos theta) depth, q = R p + t, theta' = atan2(q_x, q_z), phi' = atan2(q_y, sqrt(q_x^2 + q_z^2)),
 *   x' = (-theta' / 2 pi + 0.5) w - 0.5, u = (x' + 0.5) / w * 2 - 1, ix = (u + 1) / 2 * (w - 1) (y likewise with pi and h): the
 *   reference's normalisation fed to an align_corners=True sampler, off by half on purpose.  Evaluated in float64 from the float32
 *   inputs.  Taps outside the map contribute zero; so does a sample whose position is not finite.
 *   workspace == NULL: *workspace_bytes receives the workspace size (16-byte aligned device memory: channels-last copies of the
 *   features; nothing in either direction has C * D elements) and nothing runs.  h, w <= 65534.
 *   Kernels run on `stream`; no atomics, no host synchronisation: bit-identical from call to call and stream to stream, and
 *   slot i's numbers depend on no other slot of f_own.
 * s360_cost_volume_backward: given grad_out[n, D, h, w], writes every element of
 *   grad_own[i, c, y, x]    = scale * sum_k sum_d grad_out[i, d, y, x] * bilinear(f_partner[slot, c], warp)   (deterministic)
 *   grad_partner[s, c, tap] = scale * sum over the samples that touch the tap of grad_out * weight * f_own      (float32 atomics:
 *   arrival order shows in the last bits)
 *   as two tensors; a caller whose f_partner is f_own adds them.  Poses and depths take no gradient.  Workspace as above.
 * s360_cost_volume_warp: warped[n, C, D, h, w] = bilinear(f_partner[partner_slot[i], c], warp(i, d, y, x)) for one pairing
 *   (poses[n, 4, 4], partner_slot[n] or NULL): the materialised tensor of warp_with_pose_depth_candidates, for callers that use
 *   that function alone.  One kernel, no workspace.
 */
#define S360_CV_HM3D 0
int s360_cost_volume_forward(const float* f_own, const float* f_partner, const int32_t* partner_slot, const float* poses,
                             const float* depths, int32_t n, int32_t m, int32_t pairs, int32_t C, int32_t h, int32_t w, int32_t D,
                             int32_t convention, float scale, float* out, void* workspace, size_t* workspace_bytes, void* stream);
int s360_cost_volume_backward(const float* f_own, const float* f_partner, const int32_t* partner_slot, const float* poses,
                              const float* depths, int32_t n, int32_t m, int32_t pairs, int32_t C, int32_t h, int32_t w, int32_t D,
                              int32_t convention, float scale, const float* grad_out, float* grad_own, float* grad_partner,
                              void* workspace, size_t* workspace_bytes, void* stream);
int s360_cost_volume_warp(const float* f_partner, const int32_t* partner_slot, const float* poses, const float* depths, int32_t n,
                          int32_t m, int32_t C, int32_t h, int32_t w, int32_t D, int32_t convention, float* warped, void* stream);

/*
 * The encoder's softmax depth head (csrc/s360_depth_head.hip): the other end of the plane sweep, the reference's
 * src/model/encoder/costvolume/depth_predictor_multiview_360.py:643-651 — softmax over the D logits of a pixel, the expected
 * depth under it and its largest probability — without the [n, D, h, w] softmax.  An additive entry pair: the ABI version stays.
 *
 * s360_depth_head_forward: with pdf = softmax(logits, dim 1),
 *   depth[i, y, x] = sum_d candidates[i, d] pdf[i, d, y, x],   pmax[i, y, x] = max_d pdf[i, d, y, x] = 1 / sum_d exp(z_d - max z),
 *   lse[i, y, x] = max z + log sum_d exp(z_d - max z),          argmax[i, y, x] = the first d that attains max z.
 *   logits[n, D, h, w], candidates[n, D], depth, pmax, lse [n, h, w] float32, argmax[n, h, w] int32: contiguous device memory.
 *   One read of the logits (the running maximum is moved and the sums rescaled as the walk goes); D is split over the four waves
 *   of a block, whose partial (max, argmax, sums) are merged in a fixed order, on equal maxima the lower index.  exp, sums and
 *   quotients in float64, one rounding to float32 per output.  Finite logits of any size give finite outputs; non-finite logits
 *   give unspecified values with argmax still in [0, D).  n <= 65535, h w < 2^30.
 * s360_depth_head_backward: given g_depth, g_pmax [n, h, w] (either may be NULL: zero), writes every element of
 *   g_logits[i, d, y, x] = p_d (g_depth (c_d - depth) - g_pmax pmax) + [d == argmax] g_pmax pmax,   p_d = exp(z_d - lse),
 *   from the forward's lse, depth and argmax.  The kernel does not take the float32 lse and depth at their word: half an ulp of
 *   |lse| is a relative error of every p_d (3.8e-6 at |z| = 75).  It first sums q = sum_d exp(z_d - lse) and
 *   r = sum_d (c_d - depth) exp(z_d - lse) / q over the block's logits (1 and 0 for exact scalars; the second pass finds the
 *   logits in cache), takes pmax = exp(z_argmax - lse) / q, and evaluates the formula with p_d / q and (c_d - depth) - r, in
 *   float64.  float4 loads and stores along x when h w is a multiple of 4 and the pointers are 16-byte aligned, scalar otherwise.
 *   An argmax entry outside [0, D) contributes no pmax term.  The candidates take no gradient.
 * Both: kernels run on `stream`; no workspace, no memset, no atomics, no host synchronisation: bit-identical from call to call
 * and stream to stream.  Null required pointers or non-positive sizes: S360_E_BADARG before any GPU work.
 */
int s360_depth_head_forward(const float* logits, const float* candidates, int32_t n, int32_t d, int32_t h, int32_t w, float* depth,
                            float* pmax, float* lse, int32_t* argmax, void* stream);
int s360_depth_head_backward(const float* logits, const float* candidates, const float* lse, const float* depth, const int32_t* argmax,
                             const float* g_depth, const float* g_pmax, int32_t n, int32_t d, int32_t h, int32_t w, float* g_logits,
                             void* stream);

/*
 * The encoder's fine-depth and opacity tail (csrc/s360_depth_tail.hip): the elementwise stretch between the depth head and the
 * adapter.  Additive entries: the ABI version stays.  All of them: contiguous float32 device memory, kernels on `stream`, float64
 * arithmetic rounded once per output, no workspace, no memset, no atomics, no host synchronisation, every output element written:
 * bit-identical from call to call and stream to stream.  Null required pointers, non-positive sizes, s < 1, an unknown mode,
 * gpp < 1, v < 1, n % v != 0 or an exponent that is not finite and positive: S360_E_BADARG before any GPU work.  n <= 65535 and
 * fewer than 2^30 pixels per map.
 *
 * s360_upsample_forward (depth_predictor_multiview_360.py:650-658, one map per call): dst[n, 1, h s, w s] from src[n, 1, h, w].
 *   mode S360_UP_NEAREST: dst[Y, X] = src[Y / s, X / s] (integer division; F.interpolate(src, scale_factor=s)).
 *   mode S360_UP_BILINEAR: F.interpolate(..., mode="bilinear", align_corners=True) with the source coordinate exact in 64-bit
 *   integers: t = Y (h - 1), y0 = t / (H - 1), upper weight (t % (H - 1)) / (H - 1), upper neighbour min(y0 + 1, h - 1); H == 1: y0 = 0,
 *   weight 0; the same along x.  reciprocal != 0 samples 1 / src (:650, coarse_disps = 1 / coarse_depths, never stored).
 * s360_upsample_backward: the adjoint, gathered: g_src[y, x] = sum over the fine (Y, X) whose taps include (y, x), in ascending
 *   (Y, X), of their weights times g_dst[Y, X] — the forward's own index rule read the other way, at most about 2s x 2s terms —
 *   times -1 / src^2 if reciprocal.  src is read only then and may be NULL otherwise.
 * s360_depth_tail_forward (:694-719 and encoder_costvolume.py:228-241, :420): fullres_disps[n, 1, H, W] and
 *   delta_density[n, 2 gpp, H, W] (disparity deltas, then density logits) in the reference's (v b) order, n = v b; lo[n] = 1 / far,
 *   hi[n] = 1 / near as the caller computed them in float32.  Per pixel and surface k < gpp:
 *     fine = clamp(fullres + delta[k], lo, hi) of the unrounded sum,  depth = 1 / fine;
 *     p = sigmoid(delta[gpp + k]),  opacity = (1 - (1 - p)^exponent + p^(1 / exponent)) / (2 gpp),  density = p.
 *   depths_out, opacities_out, densities_out (may be NULL): [b, v, H W, 1, gpp], the layout the adapter and the raw render path
 *   consume: the (v b) -> (b v) transposition and the channel-last move happen in the store.
 * s360_depth_tail_backward: from the same inputs alone and g_depths, g_opacities, g_densities [b, v, H W, 1, gpp] (each may be NULL:
 *   zero), writes g_delta_density[n, 2 gpp, H, W]: its disparity half is -g_depth / fine^2 where lo <= sum <= hi and 0 elsewhere,
 *   with sum = float32(fullres + delta[k]) and the bounds included: torch's clamp backward decides on that same float32 sum, so
 *   the two agree on every element; its density half is g_opacity d opacity / d x + g_density p (1 - p) with
 *     d opacity / d x = (e (1 - p)^e p + (1 / e) p^(1 / e) (1 - p)) / (2 gpp),
 *   formed from log p and log(1 - p): finite for every finite logit, where the float32 statement's autograd gives NaN once the
 *   sigmoid rounds to 0 or 1.  g_fullres_disps[n, 1, H, W] is the sum of the disparity half over k = 0 .. gpp - 1 in that order.
 *   exponent is a float32, as torch takes a Python scalar for a float32 tensor; the kernels widen it to float64.
 * s360_opacity_map_forward / _backward (encoder_costvolume.py:241 alone, on count probabilities): out = (1 - (1 - p)^e + p^(1 / e)) / 2,
 *   g_pdf = g_out (e (1 - p)^(e - 1) + p^(1 / e - 1) / e) / 2: the derivative in p, infinite where the float64 statement's is.
 */
#define S360_UP_NEAREST 0
#define S360_UP_BILINEAR 1
int s360_upsample_forward(const float* src, float* dst, int32_t n, int32_t h, int32_t w, int32_t s, int32_t mode, int32_t reciprocal,
                          void* stream);
int s360_upsample_backward(const float* g_dst, const float* src, float* g_src, int32_t n, int32_t h, int32_t w, int32_t s, int32_t mode,
                           int32_t reciprocal, void* stream);
int s360_depth_tail_forward(const float* fullres_disps, const float* delta_density, const float* lo, const float* hi, float exponent,
                            int32_t gpp, int32_t v, float* depths_out, float* opacities_out, float* densities_out, int32_t n, int32_t H,
                            int32_t W, void* stream);
int s360_depth_tail_backward(const float* g_depths, const float* g_opacities, const float* g_densities, const float* fullres_disps,
                             const float* delta_density, const float* lo, const float* hi, float exponent, int32_t gpp, int32_t v,
                             float* g_fullres_disps, float* g_delta_density, int32_t n, int32_t H, int32_t W, void* stream);
int s360_opacity_map_forward(const float* pdf, float* out, size_t count, float exponent, void* stream);
int s360_opacity_map_backward(const float* pdf, const float* g_out, float* g_pdf, size_t count, float exponent, void* stream);

/*
 * Equirectangular -> cube resampler (csrc/s360_equirec2cube.hip): the opposite direction of s360_cube2erp_forward.  Replaces
 * Equirec2Cube.sample_equirec / run (src/geometry/util.py:71-96: numpy + scipy.ndimage.map_coordinates per channel on the host,
 * called per frame at src/dataset/dataset_hm3d.py:67,200) and, through face_map_host and strides_host, the reorder + flip that
 * makes image_cubes_supervise (dataset_hm3d.py:204-213).  Additive entries: the ABI version stays.  One launch per call on
 * `stream`, no workspace, no memset, no atomics, no host synchronisation, every output element written.
 *   erp[B, C, H, W] (float32, or uint8 when dtype == S360_E2C_UINT8) -> cube, the same element type.
 *   coor[fw, 6 fw, 2] float32 (y, x): Equirec2Cube.coor_y / coor_x (util.py:59-69), six faces side by side in slot order F R B L U D.
 *   mode S360_E2C_BILINEAR (map_coordinates order=1) or S360_E2C_NEAREST (order=0).
 *   boundary S360_E2C_REFERENCE: the two pole rows of util.py:72-74 (row H = row H-1 rolled by W/2, row H+1 = row 0 rolled by W/2)
 *     and scipy's mode='wrap', whose period is n - 1 over n = H + 2 rows and n = W columns:
 *       s = n - 1;  c < 0: c += s (trunc(-c / s) + 1);  c > n - 1: c -= s trunc(c / s);
 *       i0 = floor(c), upper weight c - i0, i1 = i0 + 1 and, if i1 > n - 1, i1 -= s (i1 / s);  nearest: floor(c + 0.5).
 *   boundary S360_E2C_PERIODIC: x modulo W with taps floor(x) mod W and (floor(x) + 1) mod W; y held in [-1, H], row -1 = row 0
 *     rolled by W/2 and row H = row H-1 rolled by W/2.  Both rules agree wherever no coordinate leaves [0, n - 1].
 *   Arithmetic after the float32 coordinate is float64 in scipy's order, t = sum over (ky, kx) of (v wy) wx; rounded once to
 *   float32, or floor(t + 0.5) clipped to 0..255 for uint8 (util.py's uint8 image contract).  Every tap index is clamped into the
 *   plane after conversion: no value in coor makes a read leave erp.
 *   scale[fw, 6 fw] float32 (may be NULL; float32 only, else S360_E_UNSUPPORTED): each texel's value is multiplied by it before the
 *     rounding — Equirec2Cube.cosmaps with S360_E2C_NEAREST is run(equ_img, equ_dep)'s z-depth (util.py:22-24,93-96).
 *   face_map_host (HOST, 6 x int32, may be NULL = identity): output face j shows slot face_map[j] & 7, flipped on both image axes
 *     when bit 3 is set (the encoding of the stitch's face_map); {4|8, 2, 3, 0, 1, 5|8} gives the rendered order U B L F R D.
 *   strides_host (HOST, 4 x int64, element units, may be NULL = dense [B, C, fw, 6 fw]): strides between batches, faces, channels
 *     and rows of `cube`; {6 C fw fw, C fw fw, fw fw, fw} writes [B, 6, C, fw, fw] directly.
 * s360_erp2cube_backward (float32): d_erp[B, C, H, W] from d_cube (face map and strides as in the forward).
 *   plan_offsets[H W + 1], plan_entries[plan_offsets[H W]] (device, int32): the inverse of coor for this boundary and mode — ERP
 *   texel e = row W + col is read by plan_entries[plan_offsets[e] .. plan_offsets[e + 1]) = cube_texel * 4 + tap, sorted, with
 *   cube_texel the index into the [fw, 6 fw] slot plane, tap = 2 ky + kx (0 for nearest) and pole-row taps already folded onto
 *   their real texel; weight-0 taps are listed.  Each weight is recomputed from coor with the forward's expressions; a texel's
 *   terms are summed in float64 in plan order and rounded once: bit-identical from call to call.  A texel nobody reads gets 0.
 * Null required pointers, non-positive sizes, equ_w < 2, an unknown mode / boundary / dtype, a face code outside 0..5 (| 8), a
 * negative stride, H W + 1 or 24 fw fw beyond int32, or more than 4 x 65535 planes in the backward: S360_E_BADARG.
 */
#define S360_E2C_BILINEAR 0
#define S360_E2C_NEAREST 1
#define S360_E2C_REFERENCE 0
#define S360_E2C_PERIODIC 1
#define S360_E2C_FLOAT32 0
#define S360_E2C_UINT8 1
int s360_erp2cube_forward(const void* erp, const float* coor, const float* scale, void* cube, int32_t batch, int32_t channels,
                          int32_t equ_h, int32_t equ_w, int32_t face_w, int32_t mode, int32_t boundary, int32_t dtype,
                          const int32_t* face_map_host, const int64_t* strides_host, void* stream);
int s360_erp2cube_backward(const float* d_cube, const float* coor, const float* scale, const int32_t* plan_offsets,
                           const int32_t* plan_entries, float* d_erp, int32_t batch, int32_t channels, int32_t equ_h, int32_t equ_w,
                           int32_t face_w, int32_t mode, int32_t boundary, const int32_t* face_map_host, const int64_t* strides_host,
                           void* stream);

/*
 * The pictures of the evaluation step (csrc/s360_visualize.hip): depth colour maps, colour tables, 8-bit frames and error maps
 * without a sort and without the host.  Additive entries: the ABI version stays.  All of them: float32 device memory in, kernels
 * on `stream`, no float atomics, no global atomics, no memset, no host synchronisation, every output element written:
 * bit-identical from call to call.  tests/depth_vis_reference.py is the numpy statement of each.
 * Colour maps (color_map): S360_CMAP_TURBO, S360_CMAP_VIRIDIS, S360_CMAP_INFERNO, 256 colours each from matplotlib
 * (csrc/s360_colormap_tables.h, written by scripts/make_colormap_tables.py).  The colour of a float32 x is row
 *   NaN: the "bad" colour, RGB 0 0 0;  otherwise min(floor(clip(x, 0, 1) * 256), 255)   (matplotlib's rule for float input)
 * as float32 (the float64 entry rounded) or as the byte trunc(float32 * 255) that prep_image makes of that float.
 *
 * s360_depth_colormap replaces depth_map (src/model/model_wrapper_erp.py:122-133: two torch.quantile sorts, log, normalise) with
 * apply_color_map_to_image(., "turbo") (src/visualization/color_map.py:9-27: a host round trip through matplotlib) and,
 * for bytes_out, the prep_image that follows (src/misc/image_io.py:38-54), for n_maps maps in one call, each normalised on its own.
 *   depth: map i is the height x width contiguous float32 elements at depth + i * map_stride (map_stride >= height * width,
 *     in elements: a strided selection of faces is read in place).  A map of more than 16 000 000 elements: S360_E_UNSUPPORTED
 *     (the reference truncates what it hands to torch.quantile there; that is not reproduced).
 *   pos = the elements > 0, n_pos their number.  n_pos > 0:
 *     near_q = Q(sort(pos), 0.01), far_q = Q(sort(all), 0.99) (NaN if the map holds a NaN), Q ATen's linear rule:
 *       rank = float32(q) * float32(n - 1) (a float32 product), lo = floor, hi = ceil, w = float32(rank - lo),
 *       a + w (b - a) if w < 0.5 else b - (b - a)(1 - w) in float64, rounded once to float32;
 *     ln = float32(log near_q), lf = float32(log far_q), L = float32(log(float64 d)) per pixel,
 *     x = float32(1 - (L - ln) / (lf - ln)), subtraction and division in float64.
 *   n_pos == 0 (the reference's except branch): near_q = min, far_q = max (NaN if the map holds a NaN),
 *     x = float32(1 - (d - near_q) / (far_q - near_q)) in float64.
 *   So a zero depth takes colour 255, a negative one the NaN colour, inf colour 0, and a constant map is all NaN colour.
 *   The quantiles are an exact selection (radix select on the order-preserving key, digits of 11, 11 and 10 bits, four ranks in
 *   the same passes, integer histograms in LDS, per-workgroup partial histograms in the workspace summed by the next launch).
 *   Outputs, each may be NULL (not all three): rgb_out[n_maps, 3, height, width] float32; bytes_out[n_maps, height, width, 3]
 *   uint8; range_out[n_maps, 4] float32 = near_q, far_q, ln, lf (ln, lf NaN when n_pos == 0).
 *   workspace == NULL: *workspace_bytes receives the workspace size (16-byte aligned device memory, contents need no
 *   initialisation) and nothing runs.  Otherwise four kernels (five with rgb_out or bytes_out) for any n_maps.
 * s360_colorize replaces apply_color_map (color_map.py:9-19) for count float32 elements: rgb_out / bytes_out (either may be NULL)
 *   hold [count, 3], or with channels_first != 0 [count / plane, 3, plane] (count a multiple of plane).
 * s360_prep_image replaces prep_image (image_io.py:38-54): image[batch, channels, height, width], channels 1, 3 or 4 ->
 *   bytes_out[height, batch * width, 3 or 4] uint8, batch entries side by side, one channel replicated to three,
 *   trunc(float32(clip(v, 0, 1)) * 255), NaN -> 0 (the reference's cast of NaN is undefined).
 * s360_error_map replaces |a - b|.mean(0) -> convert_single_colormap (model_wrapper_erp.py:369-371, :109-120, get_colormap :88-92):
 *   a, b[3, height, width] -> bytes_out[height, width, 3] uint8, viridis with the byte (float64 c * 255).astype(uint8) of
 *   get_colormap, at the row of m = float32(((|a0 - b0| + |a1 - b1|) + |a2 - b2|) / 3) in float64; Normalize(0, 1) does not clip,
 *   so m > 1 takes the last colour.
 * Null required pointers, sizes < 1, channels outside {1, 3, 4}, an unknown colour map, map_stride < height * width, or more
 * than 2^31 work-items: S360_E_BADARG before any GPU work; a workspace smaller than reported: S360_E_WORKSPACE.
 */
#define S360_CMAP_TURBO 0
#define S360_CMAP_VIRIDIS 1
#define S360_CMAP_INFERNO 2
int s360_depth_colormap(const float* depth, int32_t n_maps, int32_t height, int32_t width, size_t map_stride, float* rgb_out,
                        uint8_t* bytes_out, float* range_out, void* workspace, size_t* workspace_bytes, void* stream);
int s360_colorize(const float* x, size_t count, size_t plane, int32_t color_map, int32_t channels_first, float* rgb_out,
                  uint8_t* bytes_out, void* stream);
int s360_prep_image(const float* image, int32_t batch, int32_t channels, int32_t height, int32_t width, uint8_t* bytes_out,
                    void* stream);
int s360_error_map(const float* a, const float* b, int32_t height, int32_t width, uint8_t* bytes_out, void* stream);

/*
 * The multi-view transformer's single-head (shifted-)window attention, forward and backward (the reference's
 * single_head_split_window_attention and single_head_full_attention, src/model/encoder/backbone/multiview_transformer.py:8-16,
 * :60-210): roll, window split, q k^T / sqrt(C), shifted-window mask, softmax, times v, merge and roll back as ONE kernel; no
 * [B K^2, Lw, Lk] score tensor and no mask tensor is formed, forward or backward.
 *   q[batch, L, channels], L = height * width tokens in (y, x) order; k, v[batch, M, L, channels] with M = max(partners, 1):
 *   partners = 0 is the reference's same-shape branch (k.dim() == 3), partners >= 1 its multi-view branch, whose window keys are
 *   ordered j = p * M + u (window token p, view u fastest); partners 0 and 1 index identically.
 *   K = num_splits must divide height and width; wh = height / K, ww = width / K, Lw = wh * ww, Lk = Lw * M.  Token p = i * ww + j
 *   of window (wy, wx) sits at the ROLLED position ry = wy * wh + i, rx = wx * ww + j and is the original token
 *   ((ry + sh) mod height) * width + (rx + sw) mod width, sh = wh / 2, sw = ww / 2 if with_shift, else 0.
 *   score = float32((q . k) / sqrt(channels)) + mask, q . k summed in float64 over float32 fma chains of 8 channels.  With with_shift, mask = 0 where region(query) == region(key) and the
 *   FINITE -100.0f elsewhere (the reference's value: a masked key keeps its weight), region(ry, rx) = 3 r(ry, height, wh, sh) +
 *   r(rx, width, ww, sw), r(i, n, win, s) = [i >= n - win] + [i >= n - s].  mask_rule S360_WA_MASK_REFERENCE gives key j the region
 *   of window token j mod Lw (the reference applies its [K^2, Lw, Lw] mask as attn_mask.repeat(b, 1, m), which tiles it);
 *   S360_WA_MASK_ALIGNED gives it the region of its own token j / M.  The two coincide for M = 1 and without shift.
 *   out[batch, L, channels] = softmax over the window's keys times v, written at the query's original token; lse[batch, L]
 *   FLOAT64 = max + log(sum exp(score - max)) of the query's row (float32 running maximum, float64 running sum).
 * Products run on v_mfma_f32_32x32x2_f32: the scores and dP as float32 fma chains of 8 channels whose results are added in float64
 * and rounded once, the products over the keys as exact float32 fma chains (in tiles of 32); exp is the accurate float32 one.
 * s360_window_attention_backward takes the forward's lse and g_out[batch, L, channels] and writes g_q[batch, L, channels],
 * g_k and g_v[batch, M, L, channels]; any of the three may be null and its part is skipped.  Probabilities are recomputed as
 * exp(score - lse), dS = P (dP - Delta).  delta[batch, L] FLOAT64 is scratch the call fills, when g_q or g_k is asked for,
 * with Delta = sum_k P dP per query — from the dP values dS subtracts it from, as torch's softmax backward does (at rows with
 * few effective keys the rounding of dP cancels; rowsum(g_out * out) is the same number with independent rounding, and the
 * forward's out is therefore not an argument).  The pass owned by query tiles runs first (Delta, then g_q), the pass owned by
 * key tiles second (g_k / g_v): every output element is written once, by one wave, in a fixed order — no atomics,
 * bit-identical from run to run and across streams.
 * No host synchronisation, no allocation.  channels outside {32, 64, 96, 128}: S360_E_UNSUPPORTED.  A null required pointer, a
 * pointer that is not 16-byte aligned (q, k, v, out, lse, g_out, delta and every g_q, g_k, g_v that is given), an output that is an
 * input or another output (q, k and v may be one another), sizes < 1, num_splits not dividing height and width, an unknown
 * mask_rule, or 2^31 or more rows or workgroups: S360_E_BADARG before any GPU work, the pointers before the sizes.
 */
#define S360_WA_MASK_REFERENCE 0
#define S360_WA_MASK_ALIGNED 1
int s360_window_attention_forward(const float* q, const float* k, const float* v, int32_t batch, int32_t partners, int32_t height,
                                  int32_t width, int32_t channels, int32_t num_splits, int32_t with_shift, int32_t mask_rule,
                                  float* out, double* lse, void* stream);
int s360_window_attention_backward(const float* q, const float* k, const float* v, const double* lse, const float* g_out,
                                   int32_t batch, int32_t partners, int32_t height, int32_t width, int32_t channels,
                                   int32_t num_splits, int32_t with_shift, int32_t mask_rule, double* delta, float* g_q, float* g_k,
                                   float* g_v, void* stream);

/*
 * The "high" precision mode of the window attention above: the same function, arguments and outputs, with each of the six
 * products (S = Q K^T and O = P V; dP = G V^T, g_v = P^T G, g_q = dS K, g_k = dS^T Q) as a bf16x3 product on
 * v_mfma_f32_32x32x16_bf16 — what torch.set_float32_matmul_precision('high') asks for.  split(x) = (hi, lo): hi = bf16(x),
 * round to nearest even, lo = bf16(x - float32(hi)) (the difference is exact); A B = Ah Bh + Ah Bl + Al Bh, accumulated in float32
 * by the MFMA over all channels (keys, queries); Al Bl is dropped.  Both operands of every product are split, P, dS and g_out from
 * their float32 values.  Roll, split and merge, the finite -100 mask and both mask rules, the 1 / sqrt(channels) scaling (one
 * rounding of the float32 sum times the float64 factor), the softmax with its float32 running maximum and float64 running sum,
 * lse, Delta = sum_k P dP (float64) and the token order of every output are those of s360_window_attention_*; the backward
 * recomputes every score and dP tile from the forward's split operands with the terms in the forward's order.
 * A pre-pass splits q, k, v (and g_out) once per call into bf16 planes in window order in `scratch`: rows [batch K^2 Lw or Lk,
 * channels] for the first products and, for the second ones, transposed planes [batch K^2, channels, Lw or Lk rounded up to a
 * multiple of 4].  s360_window_attention_high_scratch_bytes returns the size for a forward (backward == 0: rows of q and k,
 * transposed v) or a backward (rows of q, k, v and g_out, transposed q, k and g_out), 0 for arguments the calls refuse: at most
 * 2 x the bytes of (q, k, v) and, for Lw >= 6, of (q, k, v, g_out).  The contents need no initialisation and nothing in it
 * is read by a later call: the backward splits again.
 * No atomics, no host synchronisation, no allocation; bit-identical from run to run and across streams.  Refusals as for
 * s360_window_attention_*, the scratch being one more output: null, not 16-byte aligned, or an input or another output:
 * S360_E_BADARG; or 2^31 or more work-items in a pre-pass launch: S360_E_BADARG; then scratch_bytes smaller than reported:
 * S360_E_WORKSPACE, all before any GPU work.
 */
size_t s360_window_attention_high_scratch_bytes(int32_t batch, int32_t partners, int32_t height, int32_t width, int32_t channels,
                                                int32_t num_splits, int32_t backward);
int s360_window_attention_high_forward(const float* q, const float* k, const float* v, int32_t batch, int32_t partners,
                                       int32_t height, int32_t width, int32_t channels, int32_t num_splits, int32_t with_shift,
                                       int32_t mask_rule, float* out, double* lse, void* scratch, size_t scratch_bytes, void* stream);
int s360_window_attention_high_backward(const float* q, const float* k, const float* v, const double* lse, const float* g_out,
                                        int32_t batch, int32_t partners, int32_t height, int32_t width, int32_t channels,
                                        int32_t num_splits, int32_t with_shift, int32_t mask_rule, double* delta, float* g_q,
                                        float* g_k, float* g_v, void* scratch, size_t scratch_bytes, void* stream);

/*
 * The U-Nets' multi-head QKV attention, forward and backward (the reference's QKVAttentionLegacy and QKVAttention,
 * src/model/encoder/costvolume/ldm_unet/unet.py:527-599), on the channel-major qkv tensor where it lies: no [b heads, L, L]
 * weight tensor, no softmax of it and no permuted copy of q, k, v or the output is formed, forward or backward.
 *   qkv[rows, heads * 3 * ch, tokens] float32 contiguous; B = rows / views batch elements.  The joint sequence of batch element bi
 *   has L = views * tokens tokens; joint token s is token s mod tokens of view u = s / tokens and lives in row u * B + bi (the
 *   reference's "(v b) n t -> b n (v t)"); views = 1 is attention within every row (use_cross_view_self_attn off).
 *   order S360_QKV_LEGACY: head hd owns channel rows [hd * 3 * ch, (hd + 1) * 3 * ch), ch rows of q, then k, then v;
 *   S360_QKV_NEW: the channel axis is q | k | v chunks of heads * ch rows and head hd owns [hd * ch, (hd + 1) * ch) of each.
 *   score = float32((q . k) / sqrt(ch)) (the reference scales q and k by ch^-1/4 each; here the scale is applied once, to the sum),
 *   q . k summed in float64 over float32 fma chains of 8 channels; out[rows, heads * ch, tokens] = softmax over the L keys times v,
 *   in the rows' order of qkv; lse[B, heads, L] FLOAT64 = max + log(sum exp(score - max)) (float32 running maximum, float64 running sum).
 * Products run on v_mfma_f32_32x32x2_f32 exactly as in s360_window_attention_* above, with the scores kept in float64 until the
 * maximum or lse is subtracted and the products over the keys added in float64 from float32 chains of 32 keys.  A workgroup is
 * four waves on one tile of 32 queries (keys in the key-owned pass): each wave walks every fourth tile of the other side, staged
 * through LDS from reads along the token axis, one dword per lane, so tokens may be any number and rows need no alignment; the
 * four partial results are combined in a fixed order.
 * s360_qkv_attention_backward takes the forward's lse and g_out[rows, heads * ch, tokens] and writes g_qkv in qkv's layout:
 * probabilities recomputed as exp(score - lse), dS = P (dP - Delta); delta[B, heads, L] FLOAT64 is scratch the call fills with
 * Delta = sum_s P dP / sum_s P per query (sum P is 1 but for rounding; dividing by it makes sum_s dS = 0 hold for the P in use).  The pass owned by query tiles runs first (Delta, then the q rows), the pass owned by key tiles
 * second (the k and v rows): every element of g_qkv is written once, by one wave, in a fixed order — no atomics, bit-identical
 * from run to run and across streams.
 * No host synchronisation, no allocation.  ch != 32: S360_E_UNSUPPORTED.  A null pointer, a pointer that is not 4-byte aligned
 * (the float32 tensors move one dword per lane, and the float64 lse and delta are held to no more than these 4 bytes, though
 * every float64 tensor has 8), an output that is an input or another output (g_qkv == qkv among them), sizes < 1, views not dividing rows, an unknown order, or 2^31 or more joint tokens or workgroups: S360_E_BADARG before
 * any GPU work, the pointers before the sizes.
 */
#define S360_QKV_LEGACY 0
#define S360_QKV_NEW 1
int s360_qkv_attention_forward(const float* qkv, int32_t rows, int32_t views, int32_t heads, int32_t ch, int32_t tokens, int32_t order,
                               float* out, double* lse, void* stream);
int s360_qkv_attention_backward(const float* qkv, const double* lse, const float* g_out, int32_t rows, int32_t views, int32_t heads,
                                int32_t ch, int32_t tokens, int32_t order, double* delta, float* g_qkv, void* stream);

/*
 * The "high" precision mode of the QKV attention: the function of s360_qkv_attention_* with each of its six products (scores
 * Q^T K and O = V P^T in the forward; dP = dO^T V, g_q = K dS^T, g_k = Q dS and g_v = dO P in the backward) as a bf16x3 product on
 * v_mfma_f32_32x32x16_bf16 — the specification of s360_window_attention_high_* above: split(x) = (hi, lo), hi = bf16(x) round to
 * nearest even, lo = bf16(x - float32(hi)); A B = Ah Bh + Ah Bl + Al Bh accumulated in float32 by the MFMA, Al Bl dropped.  Both
 * operands of every product are split from their float32 values: q and k UNSCALED (1 / sqrt(ch) multiplies the summed score and
 * g_q, g_k once), P and dS as the softmax and its backward leave them.  The softmax with its float32 running maximum and float64
 * running sum, lse[B, heads, L] FLOAT64, Delta = sum_s P dP / sum_s P, the layout rules (both orders, the (v b) rows of the joint
 * sequence, in-place writes of out and g_qkv), the four waves on one owner tile and their fixed-order combine are those of
 * s360_qkv_attention_*; the backward recomputes every score and dP from the forward's split operands with the terms in the
 * forward's order and takes the lse of a "high" forward.
 * A pre-pass splits q, k, v (and g_out) once per call into bf16 planes in joint-sequence order per (batch element, head) in
 * `scratch`, L rounded up to a multiple of 32 (Lpad) and the padding written as zeros: rows [B, heads, Lpad, 32] for the products
 * over the channels, transposed [B, heads, 32, Lpad] for those over the walked tokens.  s360_qkv_attention_high_scratch_bytes
 * returns the size for a forward (backward == 0: rows of q and k, transposed v — the bytes of qkv at Lpad tokens) or a backward
 * (rows of q, k, v and g_out, transposed q, k and g_out — 1.75 x the bytes of qkv and g_out at Lpad tokens), 0 for arguments the
 * calls refuse.  The contents need no initialisation and nothing in it is read by a later call: the backward splits again.
 * No atomics, no host synchronisation, no allocation; bit-identical from run to run and across streams.  Refusals as for
 * s360_qkv_attention_*, the scratch being one more output: null, not 16-byte aligned (its planes are read 16 bytes at a time), or
 * an input or another output: S360_E_BADARG; then scratch_bytes smaller than reported: S360_E_WORKSPACE, all before any GPU work.
 */
size_t s360_qkv_attention_high_scratch_bytes(int32_t rows, int32_t views, int32_t heads, int32_t ch, int32_t tokens, int32_t backward);
int s360_qkv_attention_high_forward(const float* qkv, int32_t rows, int32_t views, int32_t heads, int32_t ch, int32_t tokens,
                                    int32_t order, float* out, double* lse, void* scratch, size_t scratch_bytes, void* stream);
int s360_qkv_attention_high_backward(const float* qkv, const double* lse, const float* g_out, int32_t rows, int32_t views,
                                     int32_t heads, int32_t ch, int32_t tokens, int32_t order, double* delta, float* g_qkv,
                                     void* scratch, size_t scratch_bytes, void* stream);

/*
 * The encoder's normalise-then-activate pair, forward and backward: GroupNorm (the reference's GroupNorm8 / GroupNorm4,
 * src/model/encoder/costvolume/ldm_unet/util.py:199-238, and nn.GroupNorm at depth_predictor_multiview_360.py:425-427, :480-482)
 * or InstanceNorm2d without affine (groups == channels; backbone/unimatch/backbone.py:28-36), the activation that follows it
 * (SiLU in ResBlock, ldm_unet/unet.py:217-222, :249-256; GELU; ReLU; none in the postnorm AttentionBlock, :370-380) and the
 * residual add behind it (:307, :380) as ONE operator; the activation's input is never stored, forward or backward.
 *   x[n, channels, spatial] float32 contiguous, spatial the product of all trailing dims; cpg = channels / groups; the slab of
 *   (i, g) is the M = cpg * spatial contiguous floats of channels g cpg .. (g + 1) cpg - 1 of batch element i.
 *   mu and var are the slab's mean and BIASED variance, r = 1 / sqrt(var + eps), xh = (x - mu) r, z = xh weight[c] + bias[c]
 *   (weight and bias [channels], both or neither; neither is weight = 1, bias = 0), out = residual + a(z) (residual[n, channels,
 *   spatial] or NULL), a = identity, max(z, 0), z / (1 + exp(-z)) or 0.5 z erfc(-z / sqrt 2) (the erf form, nn.GELU()'s default).
 *   stats[n * groups, 2] FLOAT64 receives (mu, r) of every slab.
 * A workgroup takes one chunk of 4096 floats of one (i, c) row — a fixed split, whatever the device.  The forward is two
 * launches: per-chunk (mean, M2) from sums shifted by the chunk's first element into scratch, then every workgroup merges its
 * slab's chunks in a fixed order (mu = sum n_k mean_k / M, var = sum (M2_k + n_k (mean_k - mu)^2) / M: a constant slab gives
 * var = 0 and mu exactly, a large mean over a small spread loses nothing) and streams x (and residual) to out.
 * s360_group_norm_backward takes the forward's stats and g_out[n, channels, spatial]: dz = g_out a'(z) with z recomputed,
 * m1 = sum_c weight[c] sum dz / M and m2 = sum_c weight[c] sum dz xh / M over the slab, g_x = r (weight[c] dz - m1 - xh m2),
 * g_weight[c] = sum dz xh and g_bias[c] = sum dz over i and spatial.  Launches: per-chunk (sum dz, sum dz xh) into scratch; the
 * sweep that writes g_x (skipped when g_x is NULL); one workgroup per channel for g_weight / g_bias (skipped when both are NULL).
 * Any of the three may be NULL; g_weight / g_bias need weight.  The residual's gradient is g_out itself and has no kernel.
 * Every per-element operation and every sum is float64 on the float32 inputs, rounded once; rows move as 16-byte vectors where
 * all pointers of the launch are 16-byte aligned (scalar head and tail per row), element by element otherwise.  Every output
 * element is written once, sums run in a fixed order: no atomics, bit-identical from run to run and across streams.
 * eps is a HOST pointer to one float64, read before the first launch (scalars of this ABI are 32-bit integers, size_t and float32;
 * a float32 1e-5 is 2.5e-8 away from the float64 one, which a slab of zero variance shows in full).
 * No host synchronisation, no allocation.  scratch: s360_group_norm_scratch_doubles(n, channels, spatial) doubles of device
 * memory (8-byte aligned, contents need no initialisation; 0 is returned for sizes < 1); forward and backward may share it.
 * Null required pointers, sizes < 1, channels % groups != 0, only one of weight and bias, out or g_x overlapping x, an unknown
 * activation, eps null or *eps <= 0 (or NaN), g_weight / g_bias without weight, or 2^31 or more workgroups: S360_E_BADARG before any GPU work.
 */
#define S360_GN_ACT_NONE 0
#define S360_GN_ACT_RELU 1
#define S360_GN_ACT_SILU 2
#define S360_GN_ACT_GELU 3
size_t s360_group_norm_scratch_doubles(int32_t n, int32_t channels, int64_t spatial);
int s360_group_norm_forward(const float* x, const float* weight, const float* bias, const float* residual, int32_t n, int32_t channels,
                            size_t spatial, int32_t groups, const double* eps, int32_t activation, double* scratch, double* stats,
                            float* out, void* stream);
int s360_group_norm_backward(const float* x, const float* weight, const float* bias, const double* stats, const float* g_out, int32_t n,
                             int32_t channels, size_t spatial, int32_t groups, const double* eps, int32_t activation, double* scratch,
                             float* g_x, float* g_weight, float* g_bias, void* stream);

/*
 * The tail of the multi-view transformer's TransformerLayer behind its attention (the reference's
 * src/model/encoder/backbone/multiview_transformer.py:407-414: message = norm1(merge(message)); message = mlp(cat([source, message], -1));
 * message = norm2(message); return source + message), forward and backward, without the [tokens, 2 * channels] concatenation and
 * without either [tokens, hidden] activation, and that of the layer with no_ffn (source + norm1(merge(message))).
 *   source[tokens, channels], m[tokens, channels] (merge's output, before norm1) float32 contiguous; norm1 / norm2 weight and bias
 *   [channels]; w1[hidden, 2 * channels] and w2[channels, hidden] in nn.Linear's layout, no biases; channels = 128, hidden = 1024.
 *   LN(x) = (x - mean) rstd weight + bias over the channels, mean and the BIASED variance in float64 (two passes),
 *   rstd = 1 / sqrt(var + eps), every element formed in float64 and rounded once; eps is a HOST pointer to one float64, read before
 *   the launch (as in s360_group_norm_*).
 *   X = cat(source, LN1(m)); h = gelu(X w1^T), gelu(v) = 0.5 v erfc(-v / sqrt 2) (the erf form, nn.GELU()'s default); z = h w2^T;
 *   out[tokens, channels] = source + LN2(z).  The call also writes z[tokens, channels] (float32; norm2's statistics are those of
 *   these float32 values) and stats[2, tokens, 2] FLOAT64: (mean, rstd) per token of norm1, then of norm2.
 * Products run on v_mfma_f32_32x32x2_f32.  A workgroup owns 128 tokens, 32 per wave, on the lanes; the hidden width is walked in
 * chunks of 32 units whose slices of w1 and w2 are staged once per workgroup in LDS; X w1^T is float32 chains of 64 channels
 * added in float64 (32 in the weight-owned backward pass; the backward's dz w2c: chains of 8), z one float32 chain per chunk added in float64; norm2 and the residual are the epilogue.
 * s360_ffn_tail_backward takes the forward's inputs, z, stats and g_out[tokens, channels] and recomputes the hidden activations:
 * a pass owned by token tiles (norm2's backward, dH = (dz w2c) gelu'(X w1c^T), dX += dH w1c, one float32 chain per chunk added in float32,
 * g_source = g_out + dX[:, :channels], norm1's backward on dX[:, channels:] -> g_m, and float64 partial sums of the four LayerNorm
 * parameter gradients per workgroup, of which at most 512 walk the tiles) and a pass owned by (128 hidden units, token chunk)
 * (g_w1[j, :] = sum_t dH[t, j] X[t, :], g_w2[:, j] = sum_t dz[t, :] h[t, j], float32 over a chunk's tokens) that writes per-chunk
 * partials into scratch; a last launch adds the partials in the order 0, 1, ... in float64.  The token chunks are
 * s360_ffn_tail_weight_chunks(tokens) <= 16 runs of a multiple of 32 tokens.  Every output element is written once — g_source and
 * g_m by the token pass, the six parameter gradients by the last launch; no atomics; bit-identical from run to run and across streams.
 * s360_layer_norm_residual_forward: out = residual + LN(x) (one launch), stats[tokens, 2] FLOAT64;
 * s360_layer_norm_residual_backward: g_x, g_residual (= g_out, written by the call), g_weight, g_bias from the same row code and the
 * same chunked float64 reduction (two launches).
 * Measured on one MI355X (profiles/transformer_ffn_timing.json; medians of 50 calls, launch overhead included; this / float32 torch):
 * 65 536 tokens forward 1.071 / 0.677 ms, forward + backward 6.429 / 2.448 ms — BEHIND torch by 1.58 x and 2.63 x; the forward is
 * 48.1 TFLOP/s, 30.7 % of the float32 MFMA peak; forward + backward peak memory 223 / 962 MiB.  The gain is memory, not time.
 * No host synchronisation, no allocation.  scratch: s360_ffn_tail_scratch_bytes(tokens) bytes of device memory for either backward
 * (16-byte aligned, contents need no initialisation; 0 for tokens < 1; at most 26 MiB whatever tokens); smaller: S360_E_WORKSPACE.
 * channels != 128 or hidden != 1024: S360_E_UNSUPPORTED.  Null pointers, sizes < 1, eps null or *eps <= 0, a pointer that is not
 * 16-byte aligned, an output that is an input or another output, or 2^31 or more elements or workgroups: S360_E_BADARG before any
 * GPU work.
 */
size_t s360_ffn_tail_scratch_bytes(int32_t tokens);
int s360_ffn_tail_weight_chunks(int32_t tokens);
int s360_ffn_tail_forward(const float* source, const float* m, const float* norm1_weight, const float* norm1_bias, const float* w1,
                          const float* w2, const float* norm2_weight, const float* norm2_bias, int32_t tokens, int32_t channels,
                          int32_t hidden, const double* eps, float* out, float* z, double* stats, void* stream);
int s360_ffn_tail_backward(const float* source, const float* m, const float* norm1_weight, const float* norm1_bias, const float* w1,
                           const float* w2, const float* norm2_weight, const float* norm2_bias, const float* z, const double* stats,
                           const float* g_out, int32_t tokens, int32_t channels, int32_t hidden, const double* eps, void* scratch,
                           size_t scratch_bytes, float* g_source, float* g_m, float* g_w1, float* g_w2, float* g_norm1_weight,
                           float* g_norm1_bias, float* g_norm2_weight, float* g_norm2_bias, void* stream);
/*
 * The "high" precision mode of the FFN tail: the same function and the same tensors with the two products of the forward and the
 * four of the backward as bf16x3 products on v_mfma_f32_32x32x16_bf16 — each float32 operand the sum of two bfloat16 numbers
 * (hi = bf16(x) round to nearest even, lo = bf16(x - hi)), A B = Ah Bh + Ah Bl + Al Bh accumulated in float32 by the MFMA — which
 * is what torch.set_float32_matmul_precision('high') asks for.  The LayerNorm rows, statistics and parameter gradients stay
 * float64, h, z, dz and dpre are rounded to float32 as above, the launch geometry, the partials and the last launch are those
 * above.  A pre-pass (one launch per call) splits w1 and w2 into bf16 planes at the start of `scratch`, each in the two layouts
 * its two uses need: 3 MiB whatever tokens.  The token-side operands are split in registers and LDS: no plane grows with tokens.
 * s360_ffn_tail_high_scratch_bytes(tokens, backward): the planes (backward == 0) or the planes and s360_ffn_tail_scratch_bytes
 * (backward != 0); 0 for tokens < 1.  The contents need no initialisation and nothing in it is read by a later call: the backward
 * splits again.  z and stats of a "high" forward go to the "high" backward.
 * Refusals as s360_ffn_tail_*, and for the forward's scratch as for the backward's: null or not 16-byte aligned S360_E_BADARG,
 * smaller than reported S360_E_WORKSPACE, both before any GPU work.  No atomics, no host synchronisation, bit-identical from run
 * to run and across streams.
 */
size_t s360_ffn_tail_high_scratch_bytes(int32_t tokens, int32_t backward);
int s360_ffn_tail_high_forward(const float* source, const float* m, const float* norm1_weight, const float* norm1_bias, const float* w1,
                               const float* w2, const float* norm2_weight, const float* norm2_bias, int32_t tokens, int32_t channels,
                               int32_t hidden, const double* eps, float* out, float* z, double* stats, void* scratch,
                               size_t scratch_bytes, void* stream);
int s360_ffn_tail_high_backward(const float* source, const float* m, const float* norm1_weight, const float* norm1_bias, const float* w1,
                                const float* w2, const float* norm2_weight, const float* norm2_bias, const float* z, const double* stats,
                                const float* g_out, int32_t tokens, int32_t channels, int32_t hidden, const double* eps, void* scratch,
                                size_t scratch_bytes, float* g_source, float* g_m, float* g_w1, float* g_w2, float* g_norm1_weight,
                                float* g_norm1_bias, float* g_norm2_weight, float* g_norm2_bias, void* stream);
int s360_layer_norm_residual_forward(const float* x, const float* weight, const float* bias, const float* residual, int32_t tokens,
                                     int32_t channels, const double* eps, float* out, double* stats, void* stream);
int s360_layer_norm_residual_backward(const float* x, const float* weight, const double* stats, const float* g_out, int32_t tokens,
                                      int32_t channels, void* scratch, size_t scratch_bytes, float* g_x, float* g_residual,
                                      float* g_weight, float* g_bias, void* stream);

/*
 * The mono-feature fusion of the cost-volume encoder (the reference's src/model/encoder/encoder_costvolume.py:297 and :351-354 with
 * the rgbd_fusion of :119-125: features_mono = c2e(features_mono) under no_grad; cat([trans_features, features_mono], 1); Linear(C + Cm,
 * C), LayerNorm(C), ReLU, Linear(C, C) over the channel-last tokens), forward and backward, without the stitched [n, Cm, h, w] map,
 * without the [n, C + Cm, h, w] concatenation and without its channel-last copy.
 *   erp_feat[n, channels, equ_h, equ_w] float32 contiguous (takes a gradient); mono_cube[n, mono_channels, face_w, 6 face_w] float32
 *   contiguous, the six faces side by side in slot order F R B L U D, what Cube2Equirec.forward receives (a constant: no gradient);
 *   grid[equ_h, equ_w, 3] the stitch's sampling grid (s360_cube2erp_forward's); w1[channels, channels + mono_channels] and
 *   w2[channels, channels] in nn.Linear's layout, no biases; ln_weight, ln_bias[channels]; channels = 128, mono_channels a multiple
 *   of 64 in 64 .. 1024; eps a HOST pointer to one float64, read before the launch.
 *   Token t = (panorama, y, x), tokens = n equ_h equ_w.  m[k] = the stitch of mono_cube[panorama, k] at grid[y, x]: the eight taps
 *   4 dz + 2 dy + dx, the border clamp and the float32 expressions of s360_cube2erp_forward (for finite inputs its float32 value; a
 *   tap outside the volume has weight 0, is clamped to a valid address and not added), formed once per token for all channels.
 *   yv = [e, m] w1^T; a = relu(LN(yv)), LN(x) = (x - mean) rstd weight + bias with mean and the BIASED variance in float64 (two
 *   passes) over the float32 yv, every element formed in float64 and rounded once; out[n, channels, equ_h, equ_w] = a w2^T.  The
 *   call also writes y[tokens, channels] (yv, float32) and stats[tokens, 2] FLOAT64 (mean, rstd) for the backward.
 * Products run on v_mfma_f32_32x32x2_f32.  A workgroup owns 128 consecutive tokens (a tile may span two panoramas), 32 per wave, on
 * the lanes; K = channels + mono_channels is walked in chunks of 64 whose slice of w1 is staged once per workgroup in LDS; each
 * chunk is one float32 chain per output tile and the chunks are added in float64; a w2^T is float32 chains of 32 added in float64.
 * s360_mono_fusion_backward takes the forward's inputs, y, stats and g_out[n, channels, equ_h, equ_w]: a pass owned by token tiles
 * (g_a = g_out w2, ReLU's mask from the forward's own LN value with derivative 0 at exactly 0, LayerNorm's backward -> g_y,
 * g_erp_feat = g_y w1[:, :channels] written in erp_feat's layout, float64 partial sums of g_ln_weight and g_ln_bias per workgroup,
 * one per tile; g_y is handed to the next pass through scratch, tokens channels 4 bytes, not recomputed), a
 * pass owned by (64 columns of g_w1 or g_w2, token chunk) (g_w1 = sum_t g_y[t] (x) [e, m][t] with the taps gathered again,
 * g_w2 = sum_t g_out[t] (x) a[t]; tiles of 64 tokens, one float32 chain per tile added in float64 over the chunk) that writes
 * per-chunk float32 partials into scratch, and a last launch that adds the partials in the order 0, 1, ... in float64.  The token
 * chunks are s360_mono_fusion_weight_chunks(tokens) = min(32, ceil(tokens / 64)) runs of 64-token tiles, as even as integer division
 * makes them.  Every output element is written exactly once, no atomics; bit-identical from run to run and across streams.
 * Measured on one MI355X (profiles/mono_fusion_timing.json; N = 2, 128 x 256 tokens a panorama, medians of 50 calls, three collections,
 * launch overhead included; this / the reference's lines in float32 torch): Cm = 384: forward 0.408 / 1.136 ms, forward + backward 1.190 / 1.999 ms — ahead of torch by 2.79 x and 1.68 x;
 * Cm = 768: 0.736 / 2.169 ms and 1.802 / 3.174 ms, 2.95 x and 1.76 x.  The forward is 26.3 TFLOP/s (23.3 at Cm = 768), 16.8 % (14.9 %) of the float32 MFMA peak, the stitch's work not counted;
 * forward + backward peak memory 246 / 553 MiB (324 / 913 MiB).
 * No host synchronisation, no allocation.  scratch: s360_mono_fusion_scratch_bytes(tokens, mono_channels) bytes of device memory
 * (16-byte aligned, contents need no initialisation; 0 for tokens < 1 or an unsupported mono_channels): tokens channels 4 +
 * chunks channels (2 channels + mono_channels) 4 + ceil(tokens / 128) 2 channels 8; smaller: S360_E_WORKSPACE.
 * channels != 128 or mono_channels not a multiple of 64 in 64 .. 1024: S360_E_UNSUPPORTED.  Null pointers, sizes < 1, eps null or
 * *eps <= 0, a pointer that is not 16-byte aligned, an output that is an input or another output, 2^31 or more elements or
 * workgroups, or equ_h equ_w 8 beyond int32: S360_E_BADARG before any GPU work.
 */
size_t s360_mono_fusion_scratch_bytes(int32_t tokens, int32_t mono_channels);
int s360_mono_fusion_weight_chunks(int32_t tokens);
int s360_mono_fusion_forward(const float* erp_feat, const float* mono_cube, const float* grid, const float* w1, const float* ln_weight,
                             const float* ln_bias, const float* w2, int32_t n, int32_t channels, int32_t mono_channels, int32_t face_w,
                             int32_t equ_h, int32_t equ_w, const double* eps, float* out, float* y, double* stats, void* stream);
int s360_mono_fusion_backward(const float* erp_feat, const float* mono_cube, const float* grid, const float* w1, const float* ln_weight,
                              const float* ln_bias, const float* w2, const float* y, const double* stats, const float* g_out, int32_t n,
                              int32_t channels, int32_t mono_channels, int32_t face_w, int32_t equ_h, int32_t equ_w, const double* eps,
                              void* scratch, size_t scratch_bytes, float* g_erp_feat, float* g_w1, float* g_ln_weight, float* g_ln_bias,
                              float* g_w2, void* stream);
/*
 * The "high" precision mode of the mono-feature fusion: the same function and the same tensors with the two products of the
 * forward ([e, m] w1^T, a w2^T) and the four of the backward (g_out w2, g_y w1[:, :channels], g_y^T [e, m], g_out^T a) as bf16x3
 * products on v_mfma_f32_32x32x16_bf16 — each float32 operand the sum of two bfloat16 numbers (hi = bf16(x) round to nearest
 * even, lo = bf16(x - hi)), A B = Ah Bh + Ah Bl + Al Bh accumulated in float32 by the MFMA — which is what
 * torch.set_float32_matmul_precision('high') asks for.  m is the float32 8-tap stitch as above, taken inside the kernels; the
 * LayerNorm rows, statistics, the ReLU mask and the parameter gradients' partial sums stay float64; y, a, g_y and the partials are
 * rounded to float32 as above; the launch geometry, g_y's hand-over through scratch and the last launch are those above.  A
 * pre-pass (one launch per call) splits w1 and w2 into bf16 planes at the start of `scratch`, in the layouts their uses need:
 * 4 channels (4 channels + mono_channels) bytes (0.75 MiB at mono_channels = 1024) whatever tokens.  The token-side operands
 * are split in registers and LDS: no plane grows with tokens, and neither the stitched map nor the concatenation exists.
 * s360_mono_fusion_high_scratch_bytes(tokens, mono_channels, backward): the planes (backward == 0) or the planes and
 * s360_mono_fusion_scratch_bytes (backward != 0); a multiple of 16; 0 for tokens < 1 or an unsupported mono_channels.  The
 * contents need no initialisation and nothing in it is read by a later call: the backward splits again.  y and stats of a "high"
 * forward go to the "high" backward.
 * Refusals as s360_mono_fusion_*, and for the forward's scratch as for the backward's: null or not 16-byte aligned S360_E_BADARG,
 * smaller than reported S360_E_WORKSPACE, unsupported widths S360_E_UNSUPPORTED, all before any GPU work.  No atomics, no host
 * synchronisation, bit-identical from run to run and across streams.
 */
size_t s360_mono_fusion_high_scratch_bytes(int32_t tokens, int32_t mono_channels, int32_t backward);
int s360_mono_fusion_high_forward(const float* erp_feat, const float* mono_cube, const float* grid, const float* w1, const float* ln_weight,
                                  const float* ln_bias, const float* w2, int32_t n, int32_t channels, int32_t mono_channels,
                                  int32_t face_w, int32_t equ_h, int32_t equ_w, const double* eps, float* out, float* y, double* stats,
                                  void* scratch, size_t scratch_bytes, void* stream);
int s360_mono_fusion_high_backward(const float* erp_feat, const float* mono_cube, const float* grid, const float* w1,
                                   const float* ln_weight, const float* ln_bias, const float* w2, const float* y, const double* stats,
                                   const float* g_out, int32_t n, int32_t channels, int32_t mono_channels, int32_t face_w, int32_t equ_h,
                                   int32_t equ_w, const double* eps, void* scratch, size_t scratch_bytes, float* g_erp_feat, float* g_w1,
                                   float* g_ln_weight, float* g_ln_bias, float* g_w2, void* stream);

/*
 * Optional measurement aid (no reference counterpart; the reference's Benchmarker is an
 * un-synchronised wall clock, src/misc/benchmarker.py:15-33).  While enabled, every kernel group
 * is bracketed by HIP events recorded on the launch stream; s360_profile_collect() synchronises
 * on those events and returns, per slot, the summed milliseconds and the number of launches since
 * the previous collect.  Arrays must hold s360_profile_slots() entries.
 */
/* Second measurement aid: counts[0] = (pixel, list entry) pairs that contribute to the images rendered into a TRAINING workspace
 * (alpha >= 1/255, in front of the pixel's last contributor), counts[1] = pairs the backward composite evaluates for them
 * (survivor records in front of each 8x8 quadrant's last contributor x 64 pixels).  counts: DEVICE uint64[2], written
 * asynchronously on `stream`.  bench.py derives the work-based VALU fraction of the composites from it. */
int s360_count_contributions(const S360Params* prm, const void* workspace, size_t workspace_bytes, uint64_t* counts, void* stream);
/* Second measurement aid: where the backward composite's evaluated (entry, pixel) slots go — counts[32]: [0] slots executed, [1] padding
 * lanes, [2] entry at / behind the pixel's last contributor, [3] splat does not reach the pixel (power > 0 or alpha < 1/255),
 * [4] contributing, [5] slots of skipped four-pixel runs, [6] units, [7] groups, [8..17] executed slots by the unit's contributing
 * fraction (deciles), [18..25] executed runs by how many of the group's records contribute to the run (0, 1-4, 5-8, 9-16, 17-24, 25-32,
 * 33-48, 49-64).  Training workspaces of unsplit calls only. */
int s360_count_backward_slots(const S360Params* prm, const void* workspace, size_t workspace_bytes, uint64_t* counts, void* stream);
int s360_profile_slots(void);
const char* s360_profile_slot_name(int slot);
int s360_profile_enable(int on);
int s360_profile_collect(float* total_ms, int32_t* calls);

#ifdef __cplusplus
}
#endif
#endif /* S360_H */
