/*
 * bih.h -- C ABI of the MI355X-native BIH ray tracer (libbih_amd.so).
 *
 * Drop-in boundary for the reference's hot path (rehakvoj1/BIH-GPU-Raytracer,
 * paths relative to BIH_Raytracer/BIH_Raytracer/):
 *
 *   bih_build   replaces Renderer::Render steps 1-7 (src/Renderer.cpp:422-503:
 *               Morton transform, stable_sort_by_key, reduce_by_key,
 *               unique_by_key_copy, Launch_BuildTree, Launch_FindClipPlanes)
 *               plus the host scene prep of App::LoadModels (src/App.cpp:95-164).
 *   bih_render  replaces Renderer::Launch_cudaRender (src/Renderer.h:27,
 *               src/CUDAKernels.cu:425-447 -> cudaRender :391-423) including the
 *               persistent cuRAND state of InitRandGPU (:450-463) and the
 *               framebuffer writeback g_odata[j*W+i] = rgbToInt(col) (:420-422).
 *   bih_camera_reference  replaces `new Camera(vec3(2,0,-2), (float)W/H)`
 *               (src/Renderer.cpp:99, src/Camera.cu:5-9).
 *
 * Conventions: every call is synchronous, returns 0 or a negative BIH_ERR_*
 * code (never exits; the reference's checkCudaErrors calls exit(99),
 * src/Renderer.cpp:63-73), and touches exactly one device (the one the tree
 * was built on).  The caller owns scenes and host framebuffers; the library
 * owns device memory (scene, tree, per-pixel RNG state).  Distinct trees may
 * be used concurrently from distinct host threads.  No HIP/torch types cross
 * this boundary: streams are passed as void* (hipStream_t), device buffers as
 * plain pointers.
 */
#ifndef BIH_H
#define BIH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BIH_ABI_VERSION 4   /* 2: bih_tree_info.device_allocs, bih_reserve, bih_tree_set_param;
                               3: bih_whitted_work, BIH_PARAM_WHITTED_COUNTERS;
                               4: bih_host_register / bih_host_unregister, bih_render_history;
                               (4, added since: bih_trace*, bih_render_gbuffer*, BIH_PARAM_GBUFFER_MASK,
                                bih_render_direct*, BIH_QUERY_T_HI and bih_ray.t_hi, bih_render_lights*,
                                bih_render_area_lights*, bih_area_light_sample, bih_render_indirect*,
                                bih_bounce_sample, bih_render_path*, bih_path_sample, BIH_MAX_BOUNCES,
                                bih_tree_set_materials, bih_material, BIH_MAX_MATERIALS,
                                bih_render_path_rgb*, bih_path_rgb, bih_material.kind, BIH_MAT_DIFFUSE,
                                BIH_MAT_MIRROR, bih_render_path_spec*, bih_denoise*, bih_denoise_params,
                                BIH_DENOISE_MAX_PASSES, BIH_DENOISE_MAX_SQUARINGS, BIH_DENOISE_MAX_PIXELS) */

/* error codes */
#define BIH_OK               0
#define BIH_ERR_INVALID     -1   /* bad argument / shape                     */
#define BIH_ERR_NO_DEVICE   -2   /* no HIP device, or device index invalid   */
#define BIH_ERR_HIP         -3   /* HIP runtime error                        */
#define BIH_ERR_OOM         -4   /* device or host allocation failed         */
#define BIH_ERR_NONFINITE   -5   /* scene holds a NaN/Inf coordinate         */
#define BIH_ERR_TOO_LARGE   -6   /* more than BIH_MAX_TRIS triangles         */
#define BIH_ERR_MISMATCH    -7   /* scene does not belong to this tree       */
#define BIH_ERR_IO          -8   /* file could not be opened / read          */
#define BIH_ERR_PARSE       -9   /* malformed scene file                     */

#define BIH_MAX_TRIS (1u << 27)

/* Triangle soup, file order (App.cpp:108-121 flattening): v[9*i .. 9*i+8] =
 * v0.xyz, v1.xyz, v2.xyz of triangle i.  Host-owned. */
typedef struct bih_scene {
    uint32_t n_tris;
    const float *v;
} bih_scene;

/* Opaque BIH; built by bih_build*, owned by the library, freed by bih_free. */
typedef struct bih_tree bih_tree;

/* == Camera members m_origin, m_lowerLeftCorner, m_horizontal, m_vertical
 * (src/Camera.h:14-17).  Ray(u,v) = Ray(origin,
 * lower_left + u*horizontal + v*vertical - origin), Camera.cu:18-20. */
typedef struct bih_camera {
    float origin[3], lower_left[3], horizontal[3], vertical[3];
} bih_camera;

/* Host framebuffer: w*h uint32 0x00BBGGRR, row 0 = bottom (GL convention).
 * Frame f consumes cuRAND draws [2*spp*f, 2*spp*(f+1)) of the XORWOW
 * subsequence `pixel = y*w + x` seeded with `seed` (reference: 1984). */
typedef struct bih_framebuffer {
    uint32_t w, h, spp, frame;
    uint64_t seed;
    uint32_t *rgba;
} bih_framebuffer;

/* Traversal flavours; both produce bit-identical RGBA.
 * BIH_TRAVERSE_REFERENCE visits exactly the nodes/leaves/triangles of
 * TraverseTree (CUDAKernels.cu:227-368).  BIH_TRAVERSE_ANYHIT (default)
 * computes only the one bit per sample Color() (:370-389) consumes: does the
 * reference walk reach a triangle that sets rec.triangleIdx.  It answers
 * through the camera's frustum bins (per 4x4-pixel tile the triangles whose
 * proven edge pre-test a sample can pass, each candidate hit verified against
 * the reference walk's decisions on its root path),
 * and whatever a tile list cannot decide -- or a render the bins do not
 * cover -- takes the any-hit BIH walk, which stops at the first such
 * triangle. */
#define BIH_TRAVERSE_ANYHIT     0u
#define BIH_TRAVERSE_REFERENCE  1u

/* Row tiling for bih_render_device: local row r (0 <= r < nrows) is global
 * row y = row0 + (r / band_h) * band_h * band_step + (r % band_h).
 * {row0, nrows, band_h=nrows, band_step=1} = contiguous block;
 * {rank*B, rows_of_rank, B, world} = interleaved bands of B rows. */
typedef struct bih_rows {
    uint32_t row0, nrows, band_h, band_step;
} bih_rows;

typedef struct bih_tree_info {
    uint32_t n_tris, n_unique;            /* N, U (U-1 internal nodes)        */
    float scene_lo[3], scene_hi[3];       /* App.cpp:133-137 scene AABB        */
    int device;
    uint64_t device_bytes;                /* device memory held by the tree    */
    double build_ms;                      /* device time of the last build     */
    uint64_t device_allocs;               /* device allocations the tree made so
                                             far (a steady-state frame loop adds
                                             none: see bih_reserve)              */
} bih_tree_info;

/* Canonical arrays for parity checks (reference buffer names in brackets). */
enum bih_array {
    BIH_ARR_MORTON_SORTED = 0, /* u32[N]  [m_mortonCodes after sort]          */
    BIH_ARR_TRI_INDEX,         /* u32[N]  [m_trisIndexes]                      */
    BIH_ARR_UNIQUE_MC,         /* u32[U]  [m_uniqueMortonCodes]                */
    BIH_ARR_DUP_COUNT,         /* u32[U]  [m_duplicatesCnts]                   */
    BIH_ARR_FIRST_IDX,         /* i32[U]  [m_firstIdxs]                        */
    BIH_ARR_LEAF_PARENT,       /* i32[U]  [m_leafParents]                      */
    BIH_ARR_CLIP,              /* f32[2*(U-1)] [TreeInternalNode::t_clipPlanes]*/
    BIH_ARR_AXIS,              /* i32[U-1]    [t_axis]                         */
    BIH_ARR_CHILDREN,          /* i32[2*(U-1)] [children]                      */
    BIH_ARR_IS_LEAF,           /* u8[2*(U-1)]  [isLeaf]                        */
    BIH_ARR_PARENT,            /* i32[U-1]    [parent]                         */
    BIH_ARR_TRI_LO,            /* f32[3N] [AABBs::arrLo]                       */
    BIH_ARR_TRI_HI,            /* f32[3N] [AABBs::arrHi]                       */
    BIH_ARR_COUNT
};

int bih_device_count(void);
const char *bih_strerror(int code);
int bih_abi_version(void);

int bih_camera_reference(uint32_t w, uint32_t h, bih_camera *out);
/* Host only: an upper bound, per component, of |D| over every primary ray of
 * `camera` as the render kernel evaluates D = ((llc + u*h) + v*vert) - origin
 * in f32 for u, v in [0, 1] (Camera.cu:18-20).  The any-hit walk's miss-proof
 * boxes are sized with it. */
int bih_camera_ray_bound(const bih_camera *camera, float dmax[3]);
/* Host only: out[i] = the quotient n[i] / (float)size as the primary render's
 * kernel forms a pixel coordinate (x + ru) / w, (y + rv) / h: through the
 * image side's reciprocal and two fma up to a side of 65536, where that is
 * proved to be the IEEE quotient, by the division
 * itself above it.  *reciprocal (may be NULL) is set to 1 or 0 accordingly. */
int bih_pixel_divide(uint32_t size, const float *n, size_t count, float *out, uint32_t *reciprocal);

/* Scene ingestion (host only, no device): a Wavefront OBJ file flattened to a
 * triangle soup in file order, replacing Model::LoadModel's assimp import
 * (src/Model.cpp:10-95, aiProcess_Triangulate) and the mesh -> triangle walk
 * of App::LoadModels (src/App.cpp:65-121).  On success out->v is allocated by
 * the library (free it with bih_scene_free); on BIH_ERR_PARSE *err_line (may
 * be NULL) holds the 1-based offending line. */
int bih_scene_load_obj(const char *path, bih_scene *out, uint32_t *err_line);
void bih_scene_free(bih_scene *scene);

/* Build from a host soup (copied H2D) or a device-resident soup. */
int bih_build(const bih_scene *scene, int device, bih_tree **out);
int bih_build_device(const float *d_v, uint32_t n_tris, int device, void *stream,
                     bih_tree **out);
/* Rebuild in place (per-frame rebuild as in Renderer::Render).  Renders issued
 * afterwards on any stream see the new tree.  When the soup cannot have
 * changed (BIH_PARAM_STATIC_SOUP) the call does not wait for the device; else
 * it returns after the build, with BIH_ERR_NONFINITE for a non-finite soup. */
int bih_rebuild(bih_tree *tree);
void bih_free(bih_tree *tree);

int bih_tree_get_info(const bih_tree *tree, bih_tree_info *info);
/* Copies one canonical array to host memory; *bytes in/out. */
int bih_tree_export(const bih_tree *tree, int which, void *host_dst, size_t *bytes);

/* Full frame into a host framebuffer (reference render() entry point). */
int bih_render(const bih_scene *scene, const bih_tree *tree, const bih_camera *camera,
               bih_framebuffer *fb);
/* Rows [row0, row0+nrows) into fb->rgba[(y-row0)*w + x]; RNG subsequence and
 * jitter use the GLOBAL pixel index, so tiles reassemble the full frame. */
int bih_render_rows(const bih_scene *scene, const bih_tree *tree, const bih_camera *camera,
                    bih_framebuffer *fb, uint32_t row0, uint32_t nrows);

/* Device-resident render (bench / multi-GPU): writes nrows*w pixels to d_out
 * (device memory on the tree's device) in local row order, on `stream`
 * (NULL = the tree's stream), asynchronously; bih_sync waits for it.
 * traverse = BIH_TRAVERSE_*.  d_ray_stats (optional, device u32[3*rays], ray =
 * (local pixel)*spp + sample) gets per-ray {node visits, leaf visits, triangle
 * tests} for parity checks against the oracle. */
int bih_render_device(const bih_tree *tree, const bih_camera *camera, uint32_t w, uint32_t h,
                      uint32_t spp, uint32_t frame, uint64_t seed, const bih_rows *rows,
                      uint32_t traverse, uint32_t *d_out, uint32_t *d_ray_stats, void *stream);
/* nframes consecutive frames (frame0 .. frame0+nframes-1, any-hit) in one
 * call: frame j's nrows*w pixels at d_out + j*out_stride (out_stride >=
 * nrows*w pixels; 1 <= nframes <= 64).  Each frame is exactly the frame
 * bih_render_device renders at that index; through the frustum bins the
 * frames share one launch of each kernel (the host issue cost and the
 * render's drain are paid once per call -- DESIGN.md section 5), otherwise
 * they are rendered one by one. */
int bih_render_device_frames(const bih_tree *tree, const bih_camera *camera, uint32_t w, uint32_t h,
                             uint32_t spp, uint32_t frame0, uint32_t nframes, uint64_t seed,
                             const bih_rows *rows, uint32_t *d_out, uint64_t out_stride, void *stream);
int bih_sync(const bih_tree *tree, void *stream);

/* Sizes, ahead of time, every per-call device buffer that renders of this
 * shape need (w x h image, spp, rows = NULL for the whole frame, calls of up to
 * max_frames frames through bih_render_device_frames): the XORWOW ring, the
 * per-slot tile-queue state, fallback records and frame-split start states.
 * After it (and after one render with each camera) a frame loop of that shape
 * allocates nothing (bih_tree_info.device_allocs stays put).  The reference
 * allocates these once in Renderer::CreateCUDABuffers (src/Renderer.cpp:
 * 762-797); here they also depend on the call shape, hence the explicit call.
 * Renders of a larger shape still grow the buffers on demand. */
int bih_reserve(bih_tree *tree, uint32_t w, uint32_t h, uint32_t spp, const bih_rows *rows,
                uint32_t max_frames);

/* Per-tree parameters.  None changes a pixel; they only reorder work or
 * force the exact-walk fallback, for A/B runs and tests.  Defaults are read
 * once per process from the environment variable of the same name
 * (BIH_ITEM_TILES, ...), never on the render path. */
#define BIH_PARAM_ITEM_TILES      1  /* tile count below which a multi-frame
                                        launch splits an item's frames (65536);
                                        unset, the render kernel splits by the
                                        launch's live tiles (~16384 items)     */
#define BIH_PARAM_PAIR_CAP        2  /* (triangle, tile) pair-result slots of
                                        the bins build (tests: 0 = recompute)  */
#define BIH_PARAM_BINS_CAP        3  /* cap on bin list entries (tests: force
                                        the overflow path; 0 = none)           */
#define BIH_PARAM_FORCE_FALLBACK  4  /* 1: every live packet of a frustum-bin
                                        render takes the exact walk (tests)    */
#define BIH_PARAM_WHITTED_COUNTERS 5 /* 1: Whitted renders count the nodes and
                                        triangles each bounce's walks visit
                                        (bih_whitted_work; costs time)         */
#define BIH_PARAM_STATIC_SOUP     6  /* 1: the caller does not change the device
                                        soup of a bih_build_device tree between
                                        builds, so bih_rebuild need not read the
                                        new tree's header back: it returns once
                                        the build is enqueued (renders order
                                        after it on the device).  Implied for
                                        bih_build trees (the tree owns its copy) */
#define BIH_PARAM_TEST_ALLOC_FAIL 7  /* tests, one-shot: the next build that
                                        allocates its buffers fails at its k-th
                                        allocation (1..64; BIH_ERR_OOM); the tree
                                        frees what it had allocated and stays
                                        usable (0 = off)                       */
#define BIH_PARAM_TRACE_LDS_SLOTS 8  /* tests: 2 = ray queries (bih_trace*) run
                                        the kernel instantiation that keeps only
                                        2 stack slots per lane on chip, so that
                                        the memory part of the stack is used;
                                        0 = the default; no result changes     */
#define BIH_PARAM_GBUFFER_MASK     9  /* tests / A-B: 0 = bih_render_gbuffer*
                                        walks every sample (no frustum-bin hit
                                        mask); default 1; no result changes    */
int bih_tree_set_param(bih_tree *tree, int param, uint64_t value);

/* Ray queries: closest hit and occlusion for the caller's own rays (what
 * Embree calls rtcIntersect / rtcOccluded; the reference stops at Color()).
 *
 * Semantics: config C4's closest hit below, the
 * oracle's traverse_closest, not a new rule.
 *  - Closest: the hit is min (t, sorted position) over the triangles the
 *    reference walk tests (TraverseTree, CUDAKernels.cu:227-368), with
 *    t_lo < t < FLT_MAX.  Once a hit is known, a node entered beyond it is
 *    popped unvisited and tMax is clamped to it.  With t_lo > 0 the walk
 *    interval starts at max(scene-box entry, t_lo).  Every f32 expression is in
 *    the oracle's order, separately rounded.  This is the WALK's closest hit:
 *    the walk culls with f32 plane distances, so in rare plane-rounding cases
 *    it differs from a brute-force minimum over all triangles
 *    (tests/test_whitted.py::test_oracle_closest_equals_brute_force shows the
 *    size of that effect).
 *  - Hit record: t = hit distance (in units of |d|: P = o + t*d); prim = the
 *    triangle's index in file order (BIH_ARR_TRI_INDEX[sorted position]; of
 *    equal t the lower sorted position wins); u, v = the Moeller-Trumbore
 *    barycentrics of the accepted triangle as the reference's test computes
 *    them (e1 = v1-v0, e2 = v2-v0, p = cross(d, e2), det = e1.p,
 *    inv = 1.0f/det, s = o-v0, u = (s.p)*inv, q = cross(s, e1), v = (d.q)*inv,
 *    dot = (x+y)+z), so P = (1-u-v) v0 + u v1 + v v2.  A miss is
 *    {FLT_MAX, 0, 0, BIH_NO_HIT}.
 *  - Occluded: 1 exactly when the closest query of the same ray has
 *    prim != BIH_NO_HIT, else 0.  The walk stops at the first accepted
 *    triangle; until then it is the closest walk (same visit order, interval
 *    clamp and accept test).
 *  - Segment queries (BIH_QUERY_T_HI: the ray ends at t_hi, Embree's tfar; the
 *    last float of bih_ray).  Both are defined on the BIH_QUERY_CLOSEST result
 *    of the same {o, t_lo, d}; there is no new walk rule, and t_hi bounds no
 *    walk interval.
 *    BIH_QUERY_OCCLUDED_WITHIN: 1 exactly when that result has
 *    prim != BIH_NO_HIT and t < t_hi (one strict f32 compare), else 0.  So a
 *    NaN t_hi gives 0, t_hi <= t_lo gives 0, and t_hi = FLT_MAX or +inf gives
 *    exactly BIH_QUERY_OCCLUDED's byte.  The walk is the closest walk (the
 *    same accepts, best-hit updates and interval clamp, also for hits at or
 *    beyond t_hi) ended at the first accepted triangle with t < t_hi: the best
 *    t only decreases, so the closest walk's final t is below t_hi exactly
 *    when some accepted t was.  It is a prefix of the closest walk.
 *    BIH_QUERY_CLOSEST_WITHIN: that record when its t < t_hi, else the miss
 *    record {FLT_MAX, 0, 0, BIH_NO_HIT}.
 *    Output sizes, alignment, errors, ordering and memory are those of
 *    BIH_QUERY_CLOSEST resp. BIH_QUERY_OCCLUDED.
 *  - Rays: d need not be normalised.  BIH_QUERY_CLOSEST and BIH_QUERY_OCCLUDED
 *    do not read the last float (`reserved`; set it to 0, which does NOT mean
 *    "infinite" to the segment queries).
 *    Like the reference's test, triangles are one-sided (det > 1e-6 only).
 *    Non-finite or zero directions and origins are legal: the result is
 *    whatever the arithmetic above gives (the walk descends or pops on every
 *    step, so it ends).
 * Errors, checked in this order before the tree or a device is touched: NULL
 * tree -> BIH_ERR_INVALID; unknown query -> BIH_ERR_INVALID; n_rays >
 * BIH_MAX_RAYS -> BIH_ERR_TOO_LARGE; n_rays > 0 with NULL rays or out ->
 * BIH_ERR_INVALID; n_rays == 0 -> BIH_OK, nothing launched.
 * Ordering: a trace runs after the last bih_build / bih_rebuild, and a
 * rebuild runs after the traces in flight.  No RNG state is read, and renders
 * are not ordered against traces.  The tree owns one ray cursor and one stack
 * spill area, sized by the kernel's persistent grid (not by n_rays; allocated
 * by the first trace, counted in bih_tree_info): two traces of one tree on
 * two streams are both right because the second is ordered after the first
 * with an event -- they do not overlap on the device. */
#define BIH_NO_HIT      0xFFFFFFFFu
#define BIH_MAX_RAYS    (1u << 30)
#define BIH_QUERY_CLOSEST   0u
#define BIH_QUERY_OCCLUDED  1u
#define BIH_QUERY_T_HI      0x10u   /* flag: the ray ends at bih_ray.t_hi */
#define BIH_QUERY_CLOSEST_WITHIN   (BIH_QUERY_CLOSEST | BIH_QUERY_T_HI)    /* 0x10 */
#define BIH_QUERY_OCCLUDED_WITHIN  (BIH_QUERY_OCCLUDED | BIH_QUERY_T_HI)   /* 0x11 */

/* The last float: `reserved` to the two first queries, `t_hi` to the segment
 * queries (one member, two names). */
typedef struct bih_ray {
    float o[3]; float t_lo; float d[3];
    union { float reserved; float t_hi; };
} bih_ray;                                                                              /* 32 B */
typedef struct bih_hit { float t, u, v; uint32_t prim; } bih_hit;                       /* 16 B */

/* d_rays, d_out: device memory on the tree's device, 16-byte aligned (else
 * BIH_ERR_INVALID).  Asynchronous on `stream` (NULL = the tree's stream);
 * bih_sync waits.  d_out: bih_hit[n_rays] (CLOSEST, CLOSEST_WITHIN) or
 * uint8_t[n_rays] (OCCLUDED, OCCLUDED_WITHIN: 1 / 0), in the rays' order. */
int bih_trace_device(const bih_tree *tree, const bih_ray *d_rays, uint64_t n_rays,
                     uint32_t query, void *d_out, void *stream);
/* Host rays in, host results out; synchronous.  Stages through device buffers
 * the tree owns (grown on demand). */
int bih_trace(const bih_tree *tree, const bih_ray *rays, uint64_t n_rays,
              uint32_t query, void *out);

/* Config C4 (BASELINE.json configs[3]): 8 bounces of mirror (Whitted)
 * reflection per primary ray.  The reference has primary rays only
 * (Color, src/CUDAKernels.cu:370-389), so these semantics are this
 * library's own, stated in DESIGN.md section 4.5 and restated by the oracle
 * (ob_render_whitted): closest hit = min (t, sorted index) over the triangles
 * a front-to-back walk tests -- the reference walk's decisions and order
 * (TraverseTree, :227-368) until the first hit, after which a stacked node
 * entered beyond the best hit (tMin > best) is popped unvisited and tMax is
 * clamped to the best hit; a bounce's walk interval starts at max(scene-box
 * entry, 1e-4) (its origin lies inside the box: nothing behind it can be
 * accepted); P = O + tD, n = cross(e1, e2), R = D - (2 D.n / n.n) n;
 * secondary hits need t > 1e-4; a sample's shade halves towards (255,255,0)
 * per hit and ends at (20,20,40) on a miss (or (255,255,0) after 8 bounces).
 * Same primary rays, RNG draws and framebuffer format as bih_render.
 * d_hits (optional, device u32[rays]): hits along each sample's mirror path
 * (0..9), ray = local pixel * spp + sample. */
#define BIH_WHITTED_BOUNCES 8
int bih_render_whitted_device(const bih_tree *tree, const bih_camera *camera, uint32_t w, uint32_t h,
                              uint32_t spp, uint32_t frame, uint64_t seed, const bih_rows *rows,
                              uint32_t *d_out, uint32_t *d_hits, void *stream);
int bih_render_whitted(const bih_scene *scene, const bih_tree *tree, const bih_camera *camera,
                       bih_framebuffer *fb);
/* Work of the last Whitted render, which must have run with
 * BIH_PARAM_WHITTED_COUNTERS on (else BIH_ERR_INVALID): per bounce d = 0..8
 * the rays traced, the BIH nodes their walks entered and the triangles they
 * tested (the closest-hit walk of section 4.5; no counts for a one-leaf
 * tree, whose walks have no nodes).  Waits for that render. */
int bih_whitted_work(const bih_tree *tree, uint32_t rays[BIH_WHITTED_BOUNCES + 1],
                     uint64_t nodes[BIH_WHITTED_BOUNCES + 1], uint64_t tris[BIH_WHITTED_BOUNCES + 1]);

/* G-buffer render: depth, primitive id, barycentrics, normal and coverage of
 * the frame bih_render renders, plus (optionally) every primary sample's hit
 * record -- one fused pass.
 *
 * Any plane may be NULL (not written); all NULL -> BIH_ERR_INVALID.
 * P = rows->nrows * w local pixels, local pixel p = local_row * w + x. */
typedef struct bih_gbuffer {
    bih_hit  *hits;      /* bih_hit[P*spp], sample p*spp + s; 16-byte aligned */
    float    *depth;     /* f32[P]    */
    uint32_t *prim;      /* u32[P]    */
    float    *bary;      /* f32[2*P]  u, v   */
    float    *normal;    /* f32[3*P]  x, y, z */
    uint32_t *coverage;  /* u32[P]    samples of the pixel that hit, 0..spp */
} bih_gbuffer;

/* Semantics: bih_trace's BIH_QUERY_CLOSEST applied to the rays bih_render
 * casts, no new rule.
 *  - Ray of sample (x, y, s) of frame f: r0, r1 = draws 2*spp*f + 2s and
 *    2*spp*f + 2s + 1 of XORWOW subsequence y*w + x seeded with `seed`;
 *    u = ((float)x + r0) / (float)w, v = ((float)y + r1) / (float)h;
 *    d[a] = ((lower_left[a] + u*horizontal[a]) + v*vertical[a]) - origin[a];
 *    o = origin, t_lo = 0: bit for bit the ray bih_render traces for that
 *    sample.  y is the global row under bih_rows.
 *  - hits[p*spp + s] is exactly the bih_hit bih_trace(.., BIH_QUERY_CLOSEST)
 *    returns for that ray (the order of d_ray_stats; the same miss record).
 *  - The pixel planes come from the pixel's representative sample, the hit
 *    sample with the smallest (t, s): depth = its t, prim, bary = (u, v);
 *    coverage = the number of hit samples; normal = cross(e1, e2) / |..| of
 *    the hit triangle (e1 = v1-v0, e2 = v2-v0; n = (e1y*e2z - e2y*e1z,
 *    e1z*e2x - e2z*e1x, e1x*e2y - e2x*e1y), len = sqrtf((nx*nx + ny*ny) +
 *    nz*nz), normal = n / len, each operation one correctly rounded f32 op).
 *    Triangles are one-sided, so an accepted triangle's normal faces the ray.
 *    A pixel with no hit gets FLT_MAX, BIH_NO_HIT, (0,0), (0,0,0) and 0.
 *  - depth is in units of |d| (P = o + t*d, d not normalised): for a camera
 *    whose image plane is perpendicular to the view axis at distance L from
 *    the origin it is the planar z-depth divided by L.
 * Limits and errors, checked in this order before a device is touched: NULL
 * tree, camera or planes -> BIH_ERR_INVALID; w, h or spp == 0 ->
 * BIH_ERR_INVALID; spp > 64 -> BIH_ERR_INVALID (a limit of this call); all
 * planes NULL -> BIH_ERR_INVALID; rows as bih_render_whitted_device
 * (band_h or band_step == 0, or a row outside the frame -> BIH_ERR_INVALID);
 * h*w*spp above 2^32 - 2^20 - 1 -> BIH_ERR_TOO_LARGE; hits not 16-byte aligned
 * -> BIH_ERR_INVALID; nrows == 0 -> BIH_OK, nothing launched.
 * RNG: the call counts as the render of frame f for the tree's persistent
 * XORWOW state, as bih_render_whitted_device does; a bih_render of any frame
 * before or after it is unchanged.
 * Ordering: runs after the last bih_build / bih_rebuild, and a rebuild waits
 * for it.  It borrows the ray queries' cursor and stack spill area (counted in
 * bih_tree_info, allocated once), so G-buffer calls and traces of one tree
 * order after each other; the hit mask and its scratch image are the tree's
 * own, sized by the call's shape: after the first call of a shape further
 * calls allocate nothing. */
int bih_render_gbuffer_device(const bih_tree *tree, const bih_camera *camera, uint32_t w, uint32_t h,
                              uint32_t spp, uint32_t frame, uint64_t seed, const bih_rows *rows,
                              const bih_gbuffer *d_planes, void *stream);   /* async; bih_sync waits */
int bih_render_gbuffer(const bih_tree *tree, const bih_camera *camera, uint32_t w, uint32_t h,
                       uint32_t spp, uint32_t frame, uint64_t seed, const bih_rows *rows,
                       const bih_gbuffer *host_planes);                     /* synchronous, host memory */

/* Direct-lighting render: which of up to BIH_MAX_LIGHTS directional lights
 * reach each primary sample's hit point (hard shadows, sky visibility), and
 * the pixel's irradiance and grey shade summed from them -- the G-buffer's
 * closest hit, then shadow rays, in one call.
 *
 * Any plane may be NULL (not written); all NULL -> BIH_ERR_INVALID.
 * P = rows->nrows * w local pixels, local pixel p = local_row * w + x. */
#define BIH_MAX_LIGHTS   64
#define BIH_SHADOW_T_LO  1e-4f            /* Whitted's bounce epsilon */
/* A directional light: dir points from the surface TOWARDS the light (the
 * shadow ray's direction); it is used as given, not normalised. */
typedef struct bih_light { float dir[3]; float weight; } bih_light;   /* 16 B */
typedef struct bih_direct {
    uint64_t *lit;         /* u64[P*spp], sample p*spp + s: bit k = light k reaches it; 8-byte aligned */
    float    *irradiance;  /* f32[P] */
    uint32_t *rgba;        /* u32[P] 0x00BBGGRR */
} bih_direct;

/* Semantics: the G-buffer's closest hit, then bih_trace's BIH_QUERY_OCCLUDED
 * on rays stated here bit for bit, then sums in a stated order; no new rule.
 * Every f32 operation below is one separately rounded IEEE operation.
 *  - Sample (x, y, s) of frame f has bih_render_gbuffer's ray (o = origin, d)
 *    and its bih_hit {t, u, v, prim}.  A missed sample has lit = 0.
 *  - Hit point: P[a] = o[a] + t*d[a] (one multiply, then one add).
 *  - Normal: n = the G-buffer's `normal` formula on the sample's own triangle
 *    `prim` (cross(e1, e2) in glm order, divided by its length).
 *  - Facing test of light k, L = lights[k].dir as given:
 *    c_k = (n.x*L.x + n.y*L.y) + n.z*L.z; the light is facing exactly when
 *    c_k > 0.0f.  L is not normalised by the library (normalise it to make c_k
 *    a cosine); a zero or NaN direction never lights a sample.
 *  - Bit k of lit is 1 exactly when light k is facing and
 *    bih_trace(.., BIH_QUERY_OCCLUDED) of the ray {o = P, t_lo =
 *    BIH_SHADOW_T_LO, d = L} returns 0.  Bits n_lights and above are 0.
 *    Triangles are one-sided, as everywhere in this library: a triangle blocks
 *    a shadow ray only when its front faces the ray (det > 1e-6).  The
 *    In exact arithmetic the originating triangle has det = e1.cross(L, e2)
 *    = -(L.cross(e1, e2)) < 0 for a facing light, so it cannot block its own
 *    ray, whatever t_lo.  In f32 c_k comes from the normalised normal and det
 *    from the edges and L as given, so for a light almost in the triangle's
 *    plane, or a huge L, the two signs can disagree; the result is then
 *    whatever bih_trace answers for the ray above, by definition.
 *  - Per sample e_s = 0, then for k ascending over the lit bits
 *    e_s = e_s + lights[k].weight * c_k.  Per pixel
 *    E = (((e_0 + e_1) + ..) + e_{spp-1}) / (float)spp; a miss contributes 0.
 *    irradiance = E.  rgba: g = (int)fmaxf(0, fminf(255, 255.0f*E)) (a NaN E
 *    gives 255), pixel = g | g<<8 | g<<16; a pixel none of whose samples hit
 *    gets 0x00281414, bih_render_whitted's miss shade (20, 20, 40).
 * lights is HOST memory in both entries, copied by the call (it may be freed
 * or changed as soon as the call returns).
 * Errors, checked in this order before a device is touched: the checks of
 * bih_render_gbuffer_device, "all planes NULL" being about the three planes
 * here; lights == NULL, n_lights == 0 or n_lights > BIH_MAX_LIGHTS ->
 * BIH_ERR_INVALID; lit not 8-byte aligned -> BIH_ERR_INVALID; nrows == 0 ->
 * BIH_OK, nothing launched.
 * RNG, ordering, memory: exactly the G-buffer call's.  The call counts as the
 * render of frame f; it runs after the last bih_build / bih_rebuild and a
 * rebuild waits for it; it borrows the ray queries' cursor and spill area, so
 * it orders with G-buffer calls and traces of the tree.  Its scratch is the
 * tree's, sized by the call's shape and counted in bih_tree_info: 28 bytes
 * per sample of the rows (a hit record, a facing mask, a list entry), and 8
 * more (the lit word) once a call passes no `lit`.  After the first call of a
 * shape, light count and choice of planes further calls allocate nothing. */
int bih_render_direct_device(const bih_tree *tree, const bih_camera *camera, uint32_t w, uint32_t h,
                             uint32_t spp, uint32_t frame, uint64_t seed, const bih_rows *rows,
                             const bih_light *lights, uint32_t n_lights,
                             const bih_direct *d_planes, void *stream);     /* async; bih_sync waits */
int bih_render_direct(const bih_tree *tree, const bih_camera *camera, uint32_t w, uint32_t h,
                      uint32_t spp, uint32_t frame, uint64_t seed, const bih_rows *rows,
                      const bih_light *lights, uint32_t n_lights,
                      const bih_direct *host_planes);                       /* synchronous, host memory */

/* Direct lighting with point lights (lamps) next to directional ones, in one
 * call.  A triangle BEHIND a lamp does not shadow it, which BIH_QUERY_OCCLUDED
 * cannot say: a lamp's shadow ray is a segment query.
 *
 * Bit k < n_dir of lit is directional light k; bit n_dir + j is point light j.
 * n_dir + n_point is in 1..BIH_MAX_LIGHTS; an array may be NULL exactly when
 * its count is 0.  Both arrays are HOST memory, copied by the call.
 *
 * Semantics: bih_render_direct's, every f32 operation separately rounded;
 * directional lights work exactly as there.  For a hit sample with hit point P
 * and normal n (both as bih_render_direct defines them) and a point light
 * {pos = Q, weight = W}:
 *  - L[a] = Q[a] - P[a].
 *  - c = (n.x*L.x + n.y*L.y) + n.z*L.z; the light is facing exactly when
 *    c > 0.0f.
 *  - The light is lit when it is facing and BIH_QUERY_OCCLUDED_WITHIN on
 *    {o = P, t_lo = BIH_SHADOW_T_LO, d = L, t_hi = 1.0f} returns 0: the lamp
 *    sits at t = 1, and a triangle at or beyond it does not shadow.  A lamp
 *    exactly at P (L = 0) is never facing.
 *  - Contribution, in this order: r2 = (L.x*L.x + L.y*L.y) + L.z*L.z;
 *    len = sqrtf(r2); e_s = e_s + (W * (c / len)) / r2 -- the cosine over the
 *    squared distance.  Whatever inf or NaN the arithmetic gives is the
 *    result (rgba's clamp is defined for both).
 *  - The sum runs over the lit bits in ascending k, so directional lights come
 *    first.  The per-pixel E, rgba and miss shade are bih_render_direct's.
 *  - With n_point == 0 every plane is bit-identical to bih_render_direct's.
 * Errors, in bih_render_direct's order, its light checks replaced by: n_dir +
 * n_point == 0 or > BIH_MAX_LIGHTS -> BIH_ERR_INVALID; an array NULL with a
 * non-zero count -> BIH_ERR_INVALID.
 * Planes, RNG accounting, ordering and scratch: exactly bih_render_direct's. */
typedef struct bih_point_light { float pos[3]; float weight; } bih_point_light;  /* 16 B */
int bih_render_lights_device(const bih_tree *tree, const bih_camera *camera, uint32_t w, uint32_t h,
                             uint32_t spp, uint32_t frame, uint64_t seed, const bih_rows *rows,
                             const bih_light *dir_lights, uint32_t n_dir,
                             const bih_point_light *point_lights, uint32_t n_point,
                             const bih_direct *d_planes, void *stream);     /* async; bih_sync waits */
int bih_render_lights(const bih_tree *tree, const bih_camera *camera, uint32_t w, uint32_t h,
                      uint32_t spp, uint32_t frame, uint64_t seed, const bih_rows *rows,
                      const bih_light *dir_lights, uint32_t n_dir,
                      const bih_point_light *point_lights, uint32_t n_point,
                      const bih_direct *host_planes);                       /* synchronous, host memory */

/* Direct lighting with area lights (soft shadows) next to directional and
 * point lights, in one call.  An area light is a
 * lamp whose position differs per sample, plus the emitter's own cosine: one
 * shadow ray per (sample, light) to a point of the panel, no new walk rule.
 *
 * Bit k < n_dir of lit is directional light k; bit n_dir + i is point light i;
 * bit n_dir + n_point + j is area light j.  n_dir + n_point + n_area is in
 * 1..BIH_MAX_LIGHTS and n_area <= BIH_MAX_AREA_LIGHTS; an array may be NULL
 * exactly when its count is 0.  The set and its arrays are HOST memory, copied
 * by the call.
 *
 * Semantics: bih_render_lights', every f32 operation one separately rounded
 * IEEE operation; directional and point lights work exactly as there.  For a
 * hit sample s of global pixel gp = y*w + x (y the global row under bih_rows,
 * so bands reassemble) with hit point P and normal n (both as
 * bih_render_direct defines them) and area light j {corner = C, weight = W,
 * edge_u = U, edge_v = V}:
 *  - Sample point, all arithmetic u32 and wrapping.  It does not come from the
 *    pixel's XORWOW subsequence (no draw of any frame moves) but from a
 *    counter-based hash:
 *      mix(x): x ^= x>>16; x *= 0x7feb352d; x ^= x>>15; x *= 0x846ca68b; x ^= x>>16
 *      h = mix((uint32_t)seed); h = mix(h ^ (uint32_t)(seed>>32)); h = mix(h ^ gp);
 *      h = mix(h ^ (frame*spp + s)); h = mix(h ^ j);
 *      ha = mix(h + 0x9E3779B9); hb = mix(h + 0x3C6EF372);
 *      a = (float)(ha>>8) * 0x1p-24f; b = (float)(hb>>8) * 0x1p-24f
 *    (both exact, in [0,1)); Q[c] = (C[c] + a*U[c]) + b*V[c].
 *    bih_area_light_sample returns exactly this Q.
 *  - L[c] = Q[c] - P[c].  nl = (U.y*V.z - V.y*U.z, U.z*V.x - V.z*U.x,
 *    U.x*V.y - V.x*U.y): cross(U, V), not normalised, so |nl| is the area.
 *  - c = (n.x*L.x + n.y*L.y) + n.z*L.z; g = -((nl.x*L.x + nl.y*L.y) + nl.z*L.z).
 *    The light is facing exactly when c > 0.0f and g > 0.0f: a panel emits
 *    from ONE side, the side nl points to.  A zero-area panel (nl = 0), a NaN
 *    panel and a panel seen from behind never light a sample.
 *  - The light is lit when it is facing and BIH_QUERY_OCCLUDED_WITHIN on
 *    {o = P, t_lo = BIH_SHADOW_T_LO, d = L, t_hi = 1.0f} returns 0: a lamp's
 *    ray.  Geometry coincident with the panel (its fixture) has t = 1 up to
 *    rounding and may or may not shadow it: set a panel a little in front of
 *    its fixture.
 *  - Contribution, in this order: r2 = (L.x*L.x + L.y*L.y) + L.z*L.z;
 *    len = sqrtf(r2); e_s = e_s + ((W * (c / len)) * (g / len)) / r2 --
 *    radiance x cosine at the surface x (area x cosine at the emitter) over the
 *    squared distance, the one-sample estimator with pdf 1/area.  Whatever inf
 *    or NaN the arithmetic gives is the result.
 *  - The sums run over the lit bits in ascending k.  The per-pixel E, rgba and
 *    miss shade are bih_render_direct's.
 *  - With n_area == 0 every plane is byte-identical to bih_render_lights' (and
 *    the call launches its kernels).
 * Errors, in bih_render_lights' order, its light checks replaced by: lights ==
 * NULL -> BIH_ERR_INVALID; n_dir + n_point + n_area == 0 or > BIH_MAX_LIGHTS
 * -> BIH_ERR_INVALID; n_area > BIH_MAX_AREA_LIGHTS -> BIH_ERR_INVALID; an
 * array NULL with a non-zero count -> BIH_ERR_INVALID.
 * Planes, RNG accounting, ordering and scratch: exactly bih_render_direct's. */
#define BIH_MAX_AREA_LIGHTS 16
/* A parallelogram: the points corner + a*edge_u + b*edge_v, a, b in [0,1).  It
 * emits from ONE side, the side its normal cross(edge_u, edge_v) points to.
 * weight = its radiance. */
typedef struct bih_area_light {
    float corner[3]; float weight;
    float edge_u[3]; float reserved0;
    float edge_v[3]; float reserved1;
} bih_area_light;                                                            /* 48 B */
typedef struct bih_light_set {
    const bih_light *dir;          uint32_t n_dir;
    const bih_point_light *point;  uint32_t n_point;
    const bih_area_light *area;    uint32_t n_area;
} bih_light_set;                                        /* host memory, copied by the call */
int bih_render_area_lights_device(const bih_tree *tree, const bih_camera *camera, uint32_t w, uint32_t h,
                                  uint32_t spp, uint32_t frame, uint64_t seed, const bih_rows *rows,
                                  const bih_light_set *lights,
                                  const bih_direct *d_planes, void *stream); /* async; bih_sync waits */
int bih_render_area_lights(const bih_tree *tree, const bih_camera *camera, uint32_t w, uint32_t h,
                           uint32_t spp, uint32_t frame, uint64_t seed, const bih_rows *rows,
                           const bih_light_set *lights,
                           const bih_direct *host_planes);                  /* synchronous, host memory */
/* Host only, no device: the point Q of area light j (`light`, the j-th of its
 * call) that sample s of global pixel `pixel` = y*w + x uses in frame `frame`
 * of a render with `spp` samples per pixel.  light or q NULL, spp == 0 or
 * s >= spp -> BIH_ERR_INVALID. */
int bih_area_light_sample(const bih_area_light *light, uint32_t j, uint64_t seed, uint32_t pixel,
                          uint32_t frame, uint32_t spp, uint32_t s, float q[3]);

/* One-bounce indirect lighting with a sky (ambient) term on top of
 * bih_render_area_lights, in one call: per hit sample
 * one hashed, cosine-distributed bounce ray, its closest hit lit by the same
 * lights under the same rules; a bounce ray that escapes the scene collects the
 * sky.  No new walk rule.  With no lights at all it is the ambient-occlusion
 * render.
 *
 * Any plane may be NULL (not written); all five NULL -> BIH_ERR_INVALID.
 * P = rows->nrows * w local pixels, sample index p*spp + s.
 *
 * Semantics.  Every f32 operation is one separately rounded IEEE operation.
 * The primary sample:
 *  - Sample (x, y, s) of frame f, global pixel gp = y*w + x, has
 *    bih_render_area_lights' hit {t, u, v, prim}, hit point P, normal n, `lit`
 *    word and direct sum e_dir, exactly as that call defines them.
 *  - `lit` is byte-identical to bih_render_area_lights' `lit` for the same light
 *    set, whatever `bounce` holds.
 *  - A missed sample has lit = 0, bounce = the miss record, lit2 = 0 and e_s = 0.
 * Bounce direction:
 *  - mix is the area lights' mix.
 *      h = mix((uint32_t)seed); h = mix(h ^ (uint32_t)(seed>>32)); h = mix(h ^ gp);
 *      h = mix(h ^ (frame*spp + s)); h = mix(h ^ BIH_BOUNCE_SLOT);
 *      ha = mix(h + 0x9E3779B9); hb = mix(h + 0x3C6EF372);
 *      a = (float)(ha>>8) * 0x1p-24f; b = (float)(hb>>8) * 0x1p-24f   (both exact)
 *  - A point w of the unit sphere, without library trigonometry (host and
 *    device sinf differ, so none is used):
 *      z = 1.0f - 2.0f*a; r = sqrtf(fmaxf(0.0f, 1.0f - z*z));
 *      b4 = 4.0f*b; q = (int)b4 (0..3); f = b4 - (float)q (exact);
 *      S(x) = ((((C9*x2 + C7)*x2 + C5)*x2 + C3)*x2 + C1) * x  with x2 = x*x,
 *      C1 = 0x1.921fb6p+0f, C3 = -0x1.4abbcep-1f, C5 = 0x1.466bc6p-4f,
 *      C7 = -0x1.32d2ccp-8f, C9 = 0x1.507834p-13f
 *    (the f32 values nearest to +-(pi/2)^k / k!: S is the Taylor sine of
 *    (pi/2)x, within 3.8e-6 of sin on [0, 1]);
 *      sn = S(f); cs = S(1.0f - f)   (1 - f is exact);
 *      (cx, sx) = (cs, sn) for q = 0, (-sn, cs) for 1, (-cs, -sn) for 2,
 *      (sn, -cs) for 3;  w = (r*cx, r*sx, z).
 *  - B[c] = n[c] + w[c].  With n of unit length B is cosine-distributed about
 *    n.  bih_bounce_sample returns exactly this B.  A (near-)zero B is legal, as
 *    for any ray query.
 * Bounce record:
 *  - bounce[i] is exactly the bih_hit of bih_trace(.., BIH_QUERY_CLOSEST) for
 *    {o = P, t_lo = BIH_SHADOW_T_LO, d = B}; prim is in file order, the miss
 *    record marks an escape.  Triangles are one-sided, so the originating
 *    triangle (B.n >= 0) cannot stop its own ray, and an accepted triangle
 *    faces the ray.
 * Escaped bounce: e_ind = sky.
 * Bounce hit {t2, prim2}:
 *  - P2[c] = P[c] + t2*B[c]; n2 = the `normal` formula on triangle prim2.
 *  - lit2 and e2 are the lit word and per-sample sum bih_render_area_lights'
 *    rules give with P2, n2 in place of P, n: the same facing tests,
 *    BIH_QUERY_OCCLUDED for directional lights, BIH_QUERY_OCCLUDED_WITHIN with
 *    t_hi = 1 for lamps and panels from o = P2, the same contributions in
 *    ascending k.  An area light's point Q is the same Q the sample's primary
 *    hit uses (same gp, frame*spp + s, j).
 *  - e_ind = albedo * e2 (one multiply).
 * Sums: e_s = e_dir + e_ind (one add).  E, rgba and the miss shade are
 * bih_render_direct's.
 * Sky only: lights may be NULL or empty (all three counts 0).  Then lit = lit2
 * = 0, no shadow kernel runs, and E = sky x (escaped bounce rays of the pixel)
 * / spp: the ambient-occlusion render.
 * Errors, in bih_render_area_lights' order with these changes: "all planes
 * NULL" is about the five planes; lights == NULL and an empty set are legal;
 * counts above the limits and a NULL array with a non-zero count stay
 * BIH_ERR_INVALID; then lit not 8-byte aligned, bounce (the bih_bounce) ==
 * NULL, lit2 not 8-byte aligned or the bounce plane not 16-byte aligned ->
 * BIH_ERR_INVALID; nrows == 0 -> BIH_OK, nothing launched.
 * RNG accounting, ordering (the ev_trace chain, rebuilds) and memory are
 * bih_render_direct's.  Scratch: next to its 28 bytes per sample 29 more (the
 * bounce's record and a hit-list entry, 20; and, since the call runs
 * bih_render_path's levels with n_bounces = 1, that call's 9: the sample's sum,
 * an entry of a second live list, a hit flag), and 8 more (the lit2 word) once a
 * call passes no `lit2`.  After the first call of a shape, light count and
 * choice of planes further calls allocate nothing. */
#define BIH_BOUNCE_SLOT 0x80000000u   /* the hash slot of the bounce direction: no area light index takes it */
typedef struct bih_bounce {
    float albedo;   /* the diffuse reflectance applied to the bounced light */
    float sky;      /* the irradiance an unoccluded sky gives: an escaped bounce ray contributes it */
} bih_bounce;
typedef struct bih_indirect {
    uint64_t *lit;         /* u64[P*spp] the primary hit's lit word; 8-byte aligned */
    bih_hit  *bounce;      /* bih_hit[P*spp] the bounce ray's closest hit; 16-byte aligned */
    uint64_t *lit2;        /* u64[P*spp] the bounce hit's lit word; 8-byte aligned */
    float    *irradiance;  /* f32[P] */
    uint32_t *rgba;        /* u32[P] 0x00BBGGRR */
} bih_indirect;
int bih_render_indirect_device(const bih_tree *tree, const bih_camera *camera, uint32_t w, uint32_t h,
                               uint32_t spp, uint32_t frame, uint64_t seed, const bih_rows *rows,
                               const bih_light_set *lights, const bih_bounce *bounce,
                               const bih_indirect *d_planes, void *stream);  /* async; bih_sync waits */
int bih_render_indirect(const bih_tree *tree, const bih_camera *camera, uint32_t w, uint32_t h,
                        uint32_t spp, uint32_t frame, uint64_t seed, const bih_rows *rows,
                        const bih_light_set *lights, const bih_bounce *bounce,
                        const bih_indirect *host_planes);                    /* synchronous, host memory */
/* Host only, no device: the bounce direction B that sample s of global pixel
 * `pixel` = y*w + x uses in frame `frame` of a render with `spp` samples per
 * pixel, for the normal n.  n or d NULL, spp == 0 or s >= spp ->
 * BIH_ERR_INVALID. */
int bih_bounce_sample(uint64_t seed, uint32_t pixel, uint32_t frame, uint32_t spp, uint32_t s,
                      const float n[3], float d[3]);

/* Multi-bounce paths: bih_render_indirect carried on for n_bounces = 1 ..
 * BIH_MAX_BOUNCES levels, in one call.  A sample's
 * path goes on from each bounce hit with one more hashed, cosine-distributed
 * ray until a ray escapes (it collects the sky) or level n_bounces is reached.
 * Every level is lit by the same lights under bih_render_area_lights' rules.
 * No new walk rule.
 *
 * Any plane may be NULL (not written); all five NULL -> BIH_ERR_INVALID.
 * P = rows->nrows * w local pixels, sample index i = p*spp + s.  `bounces` and
 * `lits` are level-major: level k's whole plane of P*spp elements starts at
 * (k-1)*P*spp, k = 1 .. n_bounces.
 *
 * Semantics.  Every f32 operation is one separately rounded IEEE operation.
 * Level 0 is bih_render_indirect's primary sample:
 *  - hit {t, u, v, prim}, hit point P_0, normal n_0, the `lit` word and the
 *    direct sum e_0 (bih_render_indirect's e_dir), exactly as defined there.
 *  - `lit` is byte-identical to bih_render_area_lights' `lit` for the same
 *    light set, whatever `bounce` and n_bounces hold.
 *  - A sample is alive at level 0 when it hit.
 * Level k = 1 .. n_bounces of a sample alive at level k-1:
 *  - B_k[c] = n_{k-1}[c] + w_k[c], where w_k is bih_render_indirect's point of
 *    the unit sphere with the hash's last mix taking the slot
 *    BIH_BOUNCE_SLOT + (k-1) (wrapping uint32_t) in place of BIH_BOUNCE_SLOT:
 *      h = mix(h ^ (frame*spp + s)); h = mix(h ^ (BIH_BOUNCE_SLOT + (k-1)));
 *    No area light index (below BIH_MAX_AREA_LIGHTS = 16) reaches such a slot.
 *    bih_path_sample(.., level = k, ..) returns exactly this B_k; at level 1 it
 *    equals bih_bounce_sample on every bit.
 *  - bounces[(k-1)*P*spp + i] is exactly the bih_hit of bih_trace(..,
 *    BIH_QUERY_CLOSEST) for {o = P_{k-1}, t_lo = BIH_SHADOW_T_LO, d = B_k}; prim
 *    is in file order, the miss record marks an escape.
 *  - At a hit {t_k, prim_k} the sample is alive at level k: P_k[c] = P_{k-1}[c] +
 *    t_k*B_k[c]; n_k = the `normal` formula on triangle prim_k;
 *    lits[(k-1)*P*spp + i] and e_k are the lit word and per-sample sum
 *    bih_render_area_lights' rules give with P_k, n_k in place of P, n (as
 *    bih_render_indirect's lit2 and e2).  An area light's point Q is the same Q
 *    at every level: same gp, same frame*spp + s, same j.
 * Sums, forward along the path:
 *  - thr_0 = 1.0f; acc = e_0.
 *  - A hit at level k: thr_k = thr_{k-1} * albedo (one multiply), then
 *    acc = acc + thr_k * e_k (one multiply, one add).
 *  - An escape at level k: acc = acc + thr_{k-1} * sky (one multiply, one add);
 *    the path ends.
 *  - A hit at level n_bounces ends the path with no further term.
 *  - e_s = acc; a missed primary sample has e_s = 0.  E, rgba and the miss shade
 *    are bih_render_direct's.
 * Ended paths: at every level after the one a sample's path ended at, and at
 * every level of a missed primary sample, `bounces` holds the miss record
 * {FLT_MAX, 0, 0, BIH_NO_HIT} and `lits` holds 0: every element of every plane
 * passed is defined.
 * n_bounces == 1: lit, bounces, lits, irradiance and rgba are byte-identical to
 * bih_render_indirect's lit, bounce, lit2, irradiance and rgba (1.0f * x is x).
 * Sky only: lights may be NULL or empty, as for bih_render_indirect; then lit
 * and lits are 0, no shadow kernel runs, and with albedo = 1 E = sky x (paths
 * of the pixel that escape at a level <= n_bounces) / spp.
 * Errors: bih_render_indirect's, in its order, with one more right after
 * bounce (the bih_bounce) == NULL: n_bounces == 0 or n_bounces >
 * BIH_MAX_BOUNCES -> BIH_ERR_INVALID.  The alignment checks are lit and lits
 * (8 bytes) and bounces (16 bytes).  nrows == 0 -> BIH_OK, nothing launched.
 * RNG accounting, ordering (the ev_trace chain, rebuilds) and memory are
 * bih_render_indirect's.  Scratch: its 57 bytes per sample (48 and the 9 of
 * the sample's sum, an entry of a second live list, a hit flag), and 8 more (one
 * lit word, reused by every level) once a call passes no `lits`; two record
 * buffers and two live lists serve every n_bounces.  All of it is counted in
 * bih_tree_info.device_bytes.  After the first call of a shape, light set,
 * choice of planes and n_bounces further calls allocate nothing.  Nothing is
 * read back between the levels: the device entry is asynchronous. */
#define BIH_MAX_BOUNCES 8
typedef struct bih_path {
    uint64_t *lit;         /* u64[P*spp]       level 0's lit word; 8-byte aligned */
    bih_hit  *bounces;     /* bih_hit[B*P*spp] level k's bounce record at (k-1)*P*spp + i; 16-byte aligned */
    uint64_t *lits;        /* u64[B*P*spp]     level k's lit word at (k-1)*P*spp + i; 8-byte aligned */
    float    *irradiance;  /* f32[P] */
    uint32_t *rgba;        /* u32[P] 0x00BBGGRR */
} bih_path;
int bih_render_path_device(const bih_tree *tree, const bih_camera *camera, uint32_t w, uint32_t h,
                           uint32_t spp, uint32_t frame, uint64_t seed, const bih_rows *rows,
                           const bih_light_set *lights, const bih_bounce *bounce, uint32_t n_bounces,
                           const bih_path *d_planes, void *stream);          /* async; bih_sync waits */
int bih_render_path(const bih_tree *tree, const bih_camera *camera, uint32_t w, uint32_t h,
                    uint32_t spp, uint32_t frame, uint64_t seed, const bih_rows *rows,
                    const bih_light_set *lights, const bih_bounce *bounce, uint32_t n_bounces,
                    const bih_path *host_planes);                            /* synchronous, host memory */
/* Host only, no device: the direction B_k of level `level` = k that sample s of
 * global pixel `pixel` = y*w + x uses in frame `frame` of a render with `spp`
 * samples per pixel, for the normal n (n_{k-1}).  n or d NULL, spp == 0, s >=
 * spp, level == 0 or level > BIH_MAX_BOUNCES -> BIH_ERR_INVALID. */
int bih_path_sample(uint64_t seed, uint32_t pixel, uint32_t frame, uint32_t spp, uint32_t s,
                    uint32_t level, const float n[3], float d[3]);

/* Colour paths: bih_render_path with a material per triangle -- a diffuse
 * reflectance and an emitted radiance, R G B -- and an RGB sky (DESIGN.md
 * section 4.5.8).  Surfaces have a colour, lamps glow, light that bounces off a
 * red wall is red.  Lights stay scalar (white).  No new walk rule.
 *
 * Materials belong to the tree.  bih_tree_set_materials copies a palette of
 * n_materials records and, per triangle in FILE order (bih_hit.prim's index),
 * the index of its material; tri_material == NULL: every triangle uses
 * material 0.  Both are host memory, copied by the call, which is synchronous
 * and orders after the tree's work in flight: renders issued after it see the
 * new set.  A second call replaces the first; n_materials == 0 (materials and
 * tri_material NULL) removes the tree's materials.  Ids are by file position:
 * they stay valid across bih_rebuild (which keeps n_tris), also the rebuild of a
 * bih_build_device tree whose soup changed.  The device copies are counted in
 * bih_tree_info.device_bytes and device_allocs.  Non-finite and negative
 * values are legal: the arithmetic below decides the result.
 * Errors, in this order: tree NULL; n_materials > BIH_MAX_MATERIALS;
 * (materials == NULL) != (n_materials == 0); n_materials == 0 with tri_material
 * != NULL; an id >= n_materials among the tree's n_tris entries -- all
 * BIH_ERR_INVALID, and the tree's earlier materials stay unchanged.
 *
 * bih_render_path_rgb*.  Any plane may be NULL (not written); all five NULL ->
 * BIH_ERR_INVALID.  P, i, and the level-major `bounces` and `lits` as bih_path.
 * Semantics.  Every f32 operation is one separately rounded IEEE operation; c is
 * a channel 0..2; m_k = tri_material[prim_k] of level k's hit (prim in file
 * order, bih_hit's; 0 with a NULL tri_material).
 *  - Paths: levels, rays, hash slots, bounce records, lit words and the
 *    per-level sums e_k are exactly bih_render_path's.  Materials and sky never
 *    steer a path: lit, bounces and lits are byte-identical to bih_render_path's
 *    for the same light set and n_bounces, whatever the materials and sky hold.
 *  - A hit at level 0: acc[c] = emission(m_0)[c]; thr_0[c] = albedo(m_0)[c];
 *    acc[c] = acc[c] + thr_0[c] * e_0.
 *  - A hit at level k >= 1, in this order:
 *      acc[c] = acc[c] + thr_{k-1}[c] * emission(m_k)[c]
 *      thr_k[c] = thr_{k-1}[c] * albedo(m_k)[c]
 *      acc[c] = acc[c] + thr_k[c] * e_k
 *  - An escape at level k: acc[c] = acc[c] + thr_{k-1}[c] * sky[c]; the path ends.
 *  - A hit at level n_bounces ends the path after its three steps.
 *  - A missed primary sample: acc = (0, 0, 0).
 *  - Pixel: E[c] = (((acc_0[c] + acc_1[c]) + ..) + acc_{spp-1}[c]) / (float)spp,
 *    written to radiance[3p + c].
 *  - rgba: g_c = (int)fmaxf(0, fminf(255, 255.0f * E[c])) (NaN gives 255); the
 *    pixel is g_0 | g_1 << 8 | g_2 << 16.  A pixel none of whose samples hit
 *    gets bih_render_direct's miss shade 0x00281414.
 * Emission is collected wherever a path lands, with no weighting against the
 * light set: a lamp modelled both as emissive triangles and as an area light
 * counts twice at levels >= 1.  Use one or the other for bounce light.  An
 * accepted triangle faces the ray (one-sided triangles), so emission is
 * one-sided as well.
 * Identity: with the one material {albedo (1,1,1), emission (0,0,0)} and sky =
 * (s,s,s) every channel of radiance is byte-identical to bih_render_path's
 * irradiance with bounce = {1.0f, s}, and rgba equals its rgba (1.0f * x is x,
 * x + 0.0f is x for the values that occur, e_k and acc start from +0).
 * Errors: bih_render_path's, in its order, with sky == NULL in the place of
 * bounce == NULL; then n_bounces == 0 or > BIH_MAX_BOUNCES; the alignment
 * checks are lit and lits (8 bytes) and bounces (16 bytes), radiance needs 4
 * bytes only -- all BIH_ERR_INVALID.  nrows == 0 -> BIH_OK, nothing launched,
 * the tree never dereferenced.  After that, the first check that touches the
 * tree: a tree without materials -> BIH_ERR_INVALID.
 * RNG accounting, ordering (the ev_trace chain, rebuilds), memory and the
 * asynchrony of the device entry are bih_render_path's.  Scratch: next to
 * bih_render_path's per sample 32 bytes more, two 16-byte records {R, G, B, -}
 * (the RGB sum and the RGB throughput, in place of the scalar sum, which stays
 * allocated and unused).  All of it is counted in bih_tree_info.device_bytes.
 * After the first call of a shape, light set, choice of planes and n_bounces
 * further calls allocate nothing. */
#define BIH_MAX_MATERIALS 65536
#define BIH_MAT_DIFFUSE 0u   /* a Lambertian surface: the one kind bih_render_path_rgb* knows */
#define BIH_MAT_MIRROR  1u   /* a perfect mirror tinted by albedo (bih_render_path_spec* only) */
/* The fourth word: `reserved0` to bih_render_path_rgb*, which never reads it;
 * `kind` to bih_render_path_spec* (one member, two names, as bih_ray's last
 * float).  Positional initialisers written before `kind` existed, such as
 * {{1, 1, 1}, 0, {0, 0, 0}, 0}, go on meaning what they meant: brace elision
 * reaches the union's first member.  C compilers that know -Wmissing-braces
 * (part of -Wall there) warn about exactly that elision, so for C translation
 * units the header turns that one warning off from here on; define
 * BIH_KEEP_MISSING_BRACES_WARNING before including it to keep the warning and
 * write {{1, 1, 1}, {0}, {0, 0, 0}, 0}. */
#if defined(__GNUC__) && !defined(__cplusplus) && !defined(BIH_KEEP_MISSING_BRACES_WARNING)
#pragma GCC diagnostic ignored "-Wmissing-braces"
#endif
typedef struct bih_material {
    float albedo[3];   union { float reserved0; uint32_t kind; };  /* BIH_MAT_*; +0.0f's bits are DIFFUSE */
    float emission[3]; float reserved1;    /* emitted radiance,   R G B */
} bih_material;                                                     /* 32 B */
int bih_tree_set_materials(bih_tree *tree, const bih_material *materials, uint32_t n_materials,
                           const uint32_t *tri_material);            /* synchronous, host memory */
typedef struct bih_path_rgb {
    uint64_t *lit;         /* as bih_path */
    bih_hit  *bounces;     /* as bih_path */
    uint64_t *lits;        /* as bih_path */
    float    *radiance;    /* f32[3*P], pixel p's R, G, B at 3p, 3p+1, 3p+2 */
    uint32_t *rgba;        /* u32[P] 0x00BBGGRR */
} bih_path_rgb;
int bih_render_path_rgb_device(const bih_tree *tree, const bih_camera *camera, uint32_t w, uint32_t h,
                               uint32_t spp, uint32_t frame, uint64_t seed, const bih_rows *rows,
                               const bih_light_set *lights, const float sky[3], uint32_t n_bounces,
                               const bih_path_rgb *d_planes, void *stream);  /* async; bih_sync waits */
int bih_render_path_rgb(const bih_tree *tree, const bih_camera *camera, uint32_t w, uint32_t h,
                        uint32_t spp, uint32_t frame, uint64_t seed, const bih_rows *rows,
                        const bih_light_set *lights, const float sky[3], uint32_t n_bounces,
                        const bih_path_rgb *host_planes);                    /* synchronous, host memory */

/* Mirror materials: bih_render_path_rgb with a material kind that steers the
 * path.  A material whose `kind` is BIH_MAT_MIRROR
 * reflects the ray that found it; BIH_MAT_DIFFUSE (the bits of +0.0f, so every
 * palette written for bih_render_path_rgb is all diffuse) bounces as before.  A
 * call of its own: bih_render_path_rgb* goes on ignoring the word.  One-sided
 * triangles rule out glass; there are no glossy lobes.  No new walk rule.
 * bih_tree_set_materials accepts what it accepts and notes, on the host,
 * whether every kind of the palette is BIH_MAT_DIFFUSE or BIH_MAT_MIRROR.
 *
 * Planes, P, i, level-major `bounces` and `lits`: bih_path_rgb's.
 * Semantics, as a delta on bih_render_path_rgb.  Every f32 operation is one
 * separately rounded IEEE operation.  kind_k = kind(m_k) of a sample alive at
 * level k (level 0: the primary hit).
 *  - Incoming direction D_k, the direction of the ray that found level k's hit:
 *    D_0 is the primary d, bit for bit the G-buffer's; D_k, k >= 1, is the
 *    direction of level k's ray below.
 *  - The ray of level k+1 from a sample alive at level k is {o = P_k, t_lo =
 *    BIH_SHADOW_T_LO, d}.  kind_k == BIH_MAT_DIFFUSE: d = B_{k+1}, exactly
 *    bih_render_path's, hash slot BIH_BOUNCE_SLOT + k.  kind_k == BIH_MAT_MIRROR:
 *      dn = (D_k.x*n_k.x + D_k.y*n_k.y) + D_k.z*n_k.z
 *      k2 = 2.0f*dn
 *      d[c] = D_k[c] - k2*n_k[c]        (one multiply, one subtract)
 *    with n_k the `normal` formula's unit normal; the level's hash slot is not
 *    used (slots are counter-based: nothing shifts).
 *  - bounces[k*P*spp + i] is the BIH_QUERY_CLOSEST record of that ray, as in
 *    bih_render_path.  An accepted triangle faces its ray, so dn < 0 in exact
 *    arithmetic and d leaves the surface; the originating triangle cannot stop
 *    its own ray, for the reason given for bounce rays.
 *  - Light at a hit of level k: a diffuse hit has bih_render_path's lit word and
 *    e_k.  A mirror hit has lit word 0 and e_k = +0.0f; no shadow ray is traced
 *    for it.  At level 0 too: `lit` is byte-identical to
 *    bih_render_area_lights' only on samples whose primary hit is diffuse.
 *  - Sums: exactly bih_render_path_rgb's steps in its order with those e_k --
 *    the emission of m_k, thr_k = thr_{k-1} * albedo(m_k), acc += thr_k * e_k
 *    (performed as written at a mirror hit, with e_k = +0: one rule, also for
 *    -0 and NaN).  A mirror's albedo tints what it reflects.
 *  - The escape, radiance, rgba, miss shade, ended-path fill and n_bounces
 *    rules are unchanged.
 * Identity: with every kind BIH_MAT_DIFFUSE all five planes are byte-identical
 * to bih_render_path_rgb's.
 * Errors: bih_render_path_rgb's, in its order; then, right after "a tree
 * without materials", a palette holding a kind other than BIH_MAT_DIFFUSE and
 * BIH_MAT_MIRROR -> BIH_ERR_INVALID.  nrows == 0, RNG accounting, ordering (the
 * ev_trace chain, rebuilds) and the asynchrony of the device entry are
 * bih_render_path_rgb's.  Scratch: next to bih_render_path_rgb's per sample 16
 * bytes more, one record {D.x, D.y, D.z, kind} of the sample's latest hit;
 * counted in bih_tree_info.device_bytes.  The host entry stages through the
 * colour call's device planes.  After the first call of a shape, light set,
 * choice of planes and n_bounces further calls allocate nothing. */
int bih_render_path_spec_device(const bih_tree *tree, const bih_camera *camera, uint32_t w, uint32_t h,
                                uint32_t spp, uint32_t frame, uint64_t seed, const bih_rows *rows,
                                const bih_light_set *lights, const float sky[3], uint32_t n_bounces,
                                const bih_path_rgb *d_planes, void *stream);  /* async; bih_sync waits */
int bih_render_path_spec(const bih_tree *tree, const bih_camera *camera, uint32_t w, uint32_t h,
                         uint32_t spp, uint32_t frame, uint64_t seed, const bih_rows *rows,
                         const bih_light_set *lights, const float sky[3], uint32_t n_bounces,
                         const bih_path_rgb *host_planes);                    /* synchronous, host memory */

/* Denoiser: the edge-avoiding a-trous wavelet filter (Dammertz et al. 2010; the
 * spatial filter of SVGF) over a colour render's `radiance`, guided by the
 * G-buffer's `depth` and `normal`.  A few passes of
 * a 5 x 5 B3-spline stencil with holes; each tap is weighted by how well its
 * normal, its position on the centre's tangent plane and its colour agree with
 * the centre's.  An image filter: it walks no tree and draws no random number.
 *
 * The frame is always whole: P = w*h pixels, pixel p = y*w + x, row 0 at the
 * bottom (a frame rendered in bands is denoised after it is assembled).
 * radiance: f32[3P], bih_path_rgb.radiance's layout; depth: f32[P] and normal:
 * f32[3P], bih_gbuffer's planes; `camera`: the camera they were rendered under.
 * Either output may be NULL (not written): radiance_out f32[3P], rgba_out
 * u32[P].  radiance_out may equal radiance exactly (in place); any other
 * overlap of an output with an input or with the other output is undefined.
 *
 * Semantics.  Every f32 operation is one separately rounded IEEE operation;
 * dots are (x+y)+z; fmaxf returns the non-NaN operand; a is an axis and c a
 * channel, 0..2.
 *  - Pixel p is valid exactly when depth[p] < FLT_MAX (one f32 compare): the
 *    G-buffer's miss value, inf and NaN are all invalid.
 *  - An invalid pixel's radiance passes through every pass unchanged, it never
 *    contributes to another pixel, and its rgba_out is the miss shade 0x00281414.
 *  - Position of a valid pixel (x, y), the G-buffer's ray formula at the pixel
 *    centre: u = ((float)x + 0.5f) / (float)w; v = ((float)y + 0.5f) / (float)h;
 *    d[a] = ((lower_left[a] + u*horizontal[a]) + v*vertical[a]) - origin[a];
 *    Pos[a] = origin[a] + depth*d[a].
 *  - Pass i = 0 .. passes-1 has the step s = 1 << i, the input C_i (C_0 = the
 *    caller's radiance) and the output C_{i+1}.
 *  - A valid pixel p = (x, y) visits its taps with dy = -2..2 as the outer and
 *    dx = -2..2 as the inner loop, both ascending: q = (x + dx*s, y + dy*s).  A
 *    tap outside the image or on an invalid pixel is skipped.
 *      k = K[|dx|] * K[|dy|], K = {0.375f, 0.25f, 0.0625f} (exact).
 *    The centre tap (dx = dy = 0) has the weight w = k.  Any other tap:
 *      dn = n_p . n_q; m = fmaxf(0.0f, dn); m = m*m, normal_squarings times; wn = m
 *      e[a] = Pos_q[a] - Pos_p[a]; pd = n_p . e; wp = g(fabsf(pd) / sigma_plane)
 *      dc[c] = C_i[q][c] - C_i[p][c]; d2 = (dc0*dc0 + dc1*dc1) + dc2*dc2
 *      sc = sigma_colour * 2^-i (an exact scaling); wc = g(d2 / (sc*sc))
 *      g(x) = t*t with t = fmaxf(0.0f, 1.0f - x)
 *      w = ((k * wn) * wp) * wc
 *    (g has compact support: no expf, which differs between host and device,
 *    and an edge stops the filter hard.)  A tap contributes exactly when
 *    w > 0.0f: sum[c] = sum[c] + w * C_i[q][c] (a multiply, then an add), wsum =
 *    wsum + w, both from +0.0f.  C_{i+1}[p][c] = sum[c] / wsum.
 *  - radiance_out = C_passes.  rgba_out follows bih_render_path_rgb's rgba rule
 *    on C_passes for valid pixels.
 * Non-finite values are legal and decided by the arithmetic above.  A NaN or
 * inf colour gets the weight 0 at every other pixel through g, so a firefly
 * never spreads, and the pixel keeps its own non-finite value (the centre tap:
 * (k*C)/k).  Non-finite guides are decided likewise: a NaN anywhere in a tap's
 * terms gives it the weight 0, while +inf in a normal can give a tap the weight
 * +inf and the pixels whose stencil reaches it NaN (inf/inf).  sigma_colour = +inf or sigma_plane = +inf switches that term off
 * (g(0) = 1); a sigma of 0 leaves the centre tap alone.  sigma_plane is in scene
 * units.
 * Errors, checked in this order before a device is touched: NULL tree, camera
 * or params -> BIH_ERR_INVALID; w or h == 0 -> BIH_ERR_INVALID; passes == 0 or
 * > BIH_DENOISE_MAX_PASSES -> BIH_ERR_INVALID; normal_squarings >
 * BIH_DENOISE_MAX_SQUARINGS -> BIH_ERR_INVALID; w*h > BIH_DENOISE_MAX_PIXELS ->
 * BIH_ERR_TOO_LARGE; radiance, depth or normal NULL -> BIH_ERR_INVALID; both
 * outputs NULL -> BIH_ERR_INVALID.
 * Ordering: the call reads nothing of the tree's geometry and no RNG state, so
 * builds, rebuilds, renders and traces are not ordered against it.  It runs on
 * `stream` (NULL: the tree's); the caller orders it after the renders that
 * wrote its inputs, by using the same stream or events of its own.  Two denoise
 * calls of one tree order after each other, whatever their streams, through an
 * event of their own -- not the ray queries': a denoise may overlap the next
 * frame's walks.  bih_free waits for it.
 * Memory: the tree owns the scratch, 64 bytes per pixel -- a position record
 * {Pos, valid}, a normal record and two ping-pong colour records of 16 bytes
 * each (pass 0 reads a copy, so in place is safe) -- counted in
 * bih_tree_info.device_bytes and device_allocs; after the first call of a
 * shape further calls allocate nothing.  The host entry stages its five planes
 * through device planes of the tree's, counted likewise. */
#define BIH_DENOISE_MAX_PASSES 8
#define BIH_DENOISE_MAX_SQUARINGS 8
#define BIH_DENOISE_MAX_PIXELS (1u << 28)
typedef struct bih_denoise_params {
    uint32_t passes;            /* 1..8; pass i = 0.. uses step 1<<i            */
    uint32_t normal_squarings;  /* 0..8; normal weight = max(0, n.n')^(2^this)  */
    float    sigma_colour;      /* colour support of pass 0; halves every pass  */
    float    sigma_plane;       /* scene units: distance from the centre's tangent plane */
} bih_denoise_params;
int bih_denoise_device(const bih_tree *tree, const bih_camera *camera, uint32_t w, uint32_t h,
                       const bih_denoise_params *params,
                       const float *d_radiance, const float *d_depth, const float *d_normal,
                       float *d_radiance_out, uint32_t *d_rgba_out, void *stream);  /* async; bih_sync waits */
int bih_denoise(const bih_tree *tree, const bih_camera *camera, uint32_t w, uint32_t h,
                const bih_denoise_params *params,
                const float *radiance, const float *depth, const float *normal,
                float *radiance_out, uint32_t *rgba_out);                           /* synchronous, host memory */

/* The drop-in host loop (bih_render into a caller's framebuffer) ends in a
 * device-to-host copy of w*h*4 bytes.  Into pageable memory the runtime
 * stages it; page-locking the framebuffer once lets the copy run at DMA rate
 * (the reference copies device-to-device into its GL buffer instead,
 * src/Renderer.cpp:645-655).  Optional: any host buffer works without it.
 * bih_host_unregister undoes it (before the buffer is freed). */
int bih_host_register(void *ptr, size_t bytes);
int bih_host_unregister(void *ptr);

/* Per-render device timing (HIP events on the render stream around the main
 * render kernel and at the end of the render's device work), off by default:
 * the events cost host time on every render call.  bih_last_render_ms gives
 * the main kernel's device time (ms) of the last render, which must have been
 * issued with timing on (else BIH_ERR_INVALID). */
int bih_set_timing(bih_tree *tree, int on);
int bih_last_render_ms(const bih_tree *tree, double *ms);
/* The same render split in two: *kernel_ms as bih_last_render_ms (the main
 * render kernel, the figure rocprofv3 reports for it) and *tail_ms from its
 * end to the end of the render call's device work (k_render_fallback, the
 * exact walk of packets the frustum-bin kernel left undecided). */
int bih_last_render_times(const bih_tree *tree, double *kernel_ms, double *tail_ms);
/* The last n renders (1 <= n <= 3; all issued with timing on), oldest first:
 * t[3*i .. 3*i+2] = {main kernel start, main kernel end, end of the render's
 * device work} in ms after the oldest one's kernel start.  Renders of a frame
 * loop in flight on several streams overlap: the union of their kernel
 * intervals is the loop's kernel time (bench.py's roofline). */
int bih_render_history(const bih_tree *tree, uint32_t n, double *t);

/* The frustum bins of the tree's current camera and image (any-hit renders):
 * usable = 1 when renders walk them; list entries over all tiles, entries of
 * the global list (triangles across the eye plane, which every packet tests),
 * tiles (TW x TH pixels, one 64-ray packet each).  The two counts are those of
 * the latest bins build, also when it ended without usable bins (a global list
 * past 4096 entries, lists too long); a camera no bins can be built for
 * reports zeros. */
typedef struct bih_bins_stats {
    uint32_t usable;
    uint32_t tiles_x, tiles_y;
    uint64_t list_entries;
    uint32_t global_entries;
} bih_bins_stats;
int bih_bins_get_stats(const bih_tree *tree, bih_bins_stats *out);
/* Diagnostic (tests): the sure words of the current camera's bins, one per
 * tile in row-major order (n_bins = tiles_x * tiles_y of bih_bins_get_stats,
 * else BIH_ERR_INVALID).  Bit 4 * row + col of a 4 x 4-pixel tile is set when
 * every sample of that pixel is proven to hit whatever its jitter; a tile
 * whose word covers all its pixels inside the image is solid (*n_solid counts
 * them) and any-hit renders write it as a constant.  All zero when nothing is
 * classified: a sample count other than 4, a non-empty global list, unusable
 * bins, BIH_SOLID_TILES=0.  Waits for the device. */
int bih_bins_solid_masks(const bih_tree *tree, uint16_t *out, size_t n_bins, uint32_t *n_solid);

#ifdef __cplusplus
}
#endif
#endif /* BIH_H */
