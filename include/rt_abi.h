/*
 * rt_abi.h — C ABI of the MI355X-native path tracer (libbwrt.so).
 *
 * This is the drop-in boundary for the reference renderer's hot path
 * (IndaPlus22/bwidman-raytracer, paths relative to /root/reference):
 *
 *   reference                                   | replaced by
 *   --------------------------------------------+-----------------------------------------
 *   structs vec3d/material/sphere/plane/        | rt_vec3 / rt_material / rt_sphere /
 *   triangle/quad/camera/scene                  | rt_plane / rt_triangle / rt_quad /
 *   (Math.cuh:35-39, WorldTypes.cuh:9-53)       | rt_camera / rt_scene (byte-compatible)
 *   scene allocateScene()  (Main.cu:38-109)     | rt_set_scene()  (library uploads a copy)
 *   initializeRand<<<>>>   (Main.cu:369-380)    | done lazily by the first render of a frame
 *   cudaMalloc randStates/frameSum              |   size (rt_init_rand() forces it)
 *   (Main.cu:460-465)                           |
 *   render(scene,grid,block,cell,randStates,    | rt_render() / rt_render_ex() /
 *          accumulatedFrames,frameSum)          | rt_render_device()
 *   (Main.cu:317-366, kernel Main.cu:274-315)   |
 *   accumulatedFrames++ / controls() reset      | frame counter kept in the context;
 *   (Main.cu:467,480; Controls.cuh:15..69)      | rt_reset_accumulation(), rt_set_camera()
 *
 * Conventions
 *  - Every function returns RT_OK (0) or a negative rt_status; no exceptions
 *    cross the ABI.  rt_last_error() gives a human-readable message.
 *  - One context = one GPU (HIP device) and one pixel-row shard.  A context
 *    must be used by one host thread at a time.  All calls except
 *    rt_render_device()/rt_render_adaptive_device()/rt_denoise_device()/
 *    rt_denoise_var_device()/rt_temporal_device()/rt_temporal_var_device()/
 *    rt_temporal_var_counted_device()/rt_render_adaptive_reprojected_device()/
 *    rt_deinterleave_rows_device() are synchronous.
 *  - Output RGBA8 buffers are row-major, row 0 = BOTTOM of the screen
 *    (the reference draws texcoord (0,0) at the bottom-left, Main.cu:358).
 *  - Semantics of one "sample" (progressive frame) follow the reference
 *    exactly: jittered camera ray, one path of up to max_bounces+1
 *    closest-hit queries, frameSum reset when the frame number is 1,
 *    frameSum/n -> ACES -> gamma -> *255 -> round -> u8.
 *  - The per-pixel RNG is cuRAND-XORWOW seeded with the global pixel index
 *    y*width+x (Main.cu:377); results are independent of sharding.
 *  - Launch-policy overrides for tuning and diagnostics are environment
 *    variables read ONLY when the process sets BWRT_TUNING=1 (otherwise a
 *    context always takes the measured launch policy); none changes a
 *    result, only kernel choice and speed (BWRT_PRECISION excepted: it sets
 *    the context's initial rt_set_precision mode):
 *      at rt_create:    BWRT_KERNEL=simple, BWRT_BLOCK, BWRT_TILE, BWRT_TILE_SQ,
 *                       BWRT_GREC, BWRT_GRID_MULT, BWRT_LEAF_BATCH, BWRT_REFILL,
 *                       BWRT_SPREAD, BWRT_ORDER, BWRT_ORDER_PERIOD,
 *                       BWRT_SKY=0 (no sky table: every tile group runs the
 *                       round loop, see rt_sky_table),
 *                       BWRT_STREAM_PRIO=0 (the context's stream at normal
 *                       instead of the highest priority), BWRT_DEINT_BLOCKS,
 *                       BWRT_PRECISION=fast|exact,
 *                       BWRT_DENOISE_KERNEL=direct|tiled (filter kernel variant,
 *                       rt_denoise and rt_denoise_var),
 *                       BWRT_ADAPTIVE_KERNEL=simple|queued (list render kernel of
 *                       rt_render_adaptive on brute-force scenes)
 *      at rt_set_scene: BWRT_BVH_MIN, BWRT_BVH_LEAF, BWRT_BVH_CT, BWRT_BVH_SBVH,
 *                       BWRT_BVH_REFS, BWRT_BVH_ALPHA, BWRT_BVH_ORDER_MASK,
 *                       BWRT_BVH_N16, BWRT_NO_CULL, BWRT_BVH_STATS (report)
 *      per launch:      BWRT_STAMPS, BWRT_GTIMES (diagnostic builds only)
 */
#ifndef RT_ABI_H
#define RT_ABI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define RT_API __attribute__((visibility("default")))
#else
#define RT_API
#endif

/* ---- world types (byte-compatible with the reference) ------------------ */

/* Math.cuh:35-39 (vec3d, also used as `color`): 12 bytes */
typedef struct rt_vec3 {
    float x, y, z;
} rt_vec3;

/* WorldTypes.cuh:15-20: 24 bytes.
 * Reference defaults: albedo {0,0,0}, emittance 0, roughness 1,
 * refractiveIndex 1.05 (see rt_material_default()). */
typedef struct rt_material {
    rt_vec3 albedo;
    float emittance;
    float roughness;
    float refractive_index;
} rt_material;

/* WorldTypes.cuh:22-26: 40 bytes (mat at offset 16) */
typedef struct rt_sphere {
    rt_vec3 position;
    float radius;
    rt_material mat;
} rt_sphere;

/* WorldTypes.cuh:28-32: 60 bytes (mat at offset 36).
 * The plane normal is cross(directions[0], directions[1]), NOT normalised
 * (Intersection.cuh:69). */
typedef struct rt_plane {
    rt_vec3 origin;
    rt_vec3 directions[2];
    rt_material mat;
} rt_plane;

/* WorldTypes.cuh:34-37: 60 bytes */
typedef struct rt_triangle {
    rt_vec3 vertices[3];
    rt_material mat;
} rt_triangle;

/* WorldTypes.cuh:39-42: 72 bytes */
typedef struct rt_quad {
    rt_vec3 vertices[4];
    rt_material mat;
} rt_quad;

/* WorldTypes.cuh:9-13: 24 bytes.  angle[0] = yaw (RotY), angle[1] = pitch
 * (RotX), fov in radians (horizontal). */
typedef struct rt_camera {
    rt_vec3 position;
    float angle[2];
    float fov;
} rt_camera;

/* WorldTypes.cuh:44-53: 88 bytes on LP64 (same offsets).  Unlike the
 * reference (device pointers produced by allocateScene), the pointers here
 * are HOST pointers: rt_set_scene() copies the arrays to the GPU; the caller
 * keeps ownership of its arrays. */
typedef struct rt_scene {
    rt_camera camera;
    const rt_sphere* spheres;
    int sphere_count;
    const rt_plane* planes;
    int plane_count;
    const rt_triangle* triangles;
    int triangle_count;
    const rt_quad* quads;
    int quad_count;
} rt_scene;

/* ---- status codes ------------------------------------------------------- */

typedef enum rt_status {
    RT_OK = 0,
    RT_ERR_INVALID_ARGUMENT = -1,
    RT_ERR_NO_DEVICE = -2,
    RT_ERR_HIP = -3,         /* a HIP runtime call or kernel launch failed */
    RT_ERR_OUT_OF_MEMORY = -4,
    RT_ERR_NO_SCENE = -5,    /* render before rt_set_scene()              */
    RT_ERR_UNSUPPORTED = -6  /* e.g. max_bounces above RT_MAX_BOUNCES      */
} rt_status;

#define RT_MAX_BOUNCES 32
#define RT_DEFAULT_MAX_BOUNCES 5 /* Main.cu:26 */

/* Render request for the extended entry points. */
typedef struct rt_render_params {
    int width;          /* full image width  (Main.cu:23, windowWidth)  */
    int height;         /* full image height (Main.cu:24, windowHeight) */
    int samples;        /* progressive frames rendered by this call (>=1)  */
    int max_bounces;    /* Main.cu:26; B allows B+1 closest-hit queries    */
    unsigned first_frame; /* accumulatedFrames of the first frame of this
                             call; 1 restarts accumulation (Main.cu:301);
                             0 = continue from the context's frame counter */
    int row_offset;     /* shard: render global rows y = row_offset +      */
    int row_stride;     /*        j*row_stride, j = 0..rows-1 (0,1 = all)  */
} rt_render_params;

/* ---- context ------------------------------------------------------------ */

typedef struct rt_context rt_context;

/* Library / ABI version, "major.minor.patch". */
RT_API const char* rt_version(void);

/* Reference material defaults (WorldTypes.cuh:16-19). */
RT_API rt_material rt_material_default(void);

/* Number of visible HIP devices (0 when none; never fails). */
RT_API int rt_device_count(void);

/* Create a context on HIP device `device`.  Without a HIP device this
 * returns RT_ERR_NO_DEVICE: a GPU context never falls back to the CPU. */
RT_API int rt_create(int device, rt_context** out);
RT_API void rt_destroy(rt_context* ctx);

/* ---- scalar C++ CPU fallback ------------------------------------------------
 * The same per-ray arithmetic as the HIP kernels (csrc/rt_path.h, compiled
 * for the host), bit-identical results, one pixel per loop iteration on a
 * pool of `threads` host threads (256-pixel chunks).  It is an explicit
 * backend, never chosen implicitly: only a context made by rt_create_cpu()
 * renders on the CPU, and every entry point behaves on it as on a GPU
 * context (rt_set_scene, rt_init_rand, rt_render, rt_render_ex, rt_controls,
 * rt_get_state / rt_set_state, ...; rt_last_kernel_ms gives the last render's
 * wall time) except rt_render_device, rt_render_adaptive_device, rt_adaptive_export_rows_device,
 * rt_render_adaptive_shard_device, rt_denoise_device, rt_denoise_var_device,
 * rt_temporal_device, rt_temporal_var_device, rt_temporal_var_counted_device,
 * rt_render_adaptive_reprojected_device, rt_render_multi and rt_deinterleave_rows_device (RT_ERR_UNSUPPORTED: no
 * device memory).
 * Replaces the reference's config-1 CPU path and is the CPU baseline of
 * bench.py (SURVEY §8(b) rt_render_cpu, §8(d)). */

/* Host threads the process may run on: its sched affinity, capped by a
 * cgroup v2 CPU quota (/sys/fs/cgroup/cpu.max) when one is set. */
RT_API int rt_cpu_threads(void);

/* Create a CPU context rendering on `threads` host threads (0 = all of
 * rt_cpu_threads()).  Needs an x86-64-v3 host (AVX2 + FMA), else
 * RT_ERR_UNSUPPORTED. */
RT_API int rt_create_cpu(int threads, rt_context** out);

/* Host threads of a CPU context (0 for a GPU context). */
RT_API int rt_context_threads(const rt_context* ctx);

/* rt_render_ex() on a CPU context with an explicit thread count for this call
 * (0 = the context's).  RT_ERR_INVALID_ARGUMENT on a GPU context. */
RT_API int rt_render_cpu(rt_context* ctx, const rt_render_params* p, int threads,
                         uint8_t* rgba_out, float* accum_out);

/* Upload a copy of the scene (≈ allocateScene, Main.cu:38-109).  Resets the
 * frame counter to 1, like any camera change in controls().  Waits for a
 * render still running on a caller's stream (rt_render_device) first; so do
 * rt_init_rand and rt_set_state.  Scenes with 2^24 or more spheres +
 * triangles + quads in the BVH return RT_ERR_UNSUPPORTED. */
RT_API int rt_set_scene(rt_context* ctx, const rt_scene* scene);

/* Move the camera (controls(), Controls.cuh:5-75): resets accumulation. */
RT_API int rt_set_camera(rt_context* ctx, const rt_camera* camera);

/* accumulatedFrames = 1 (Controls.cuh:15..69).  RNG streams continue. */
RT_API int rt_reset_accumulation(rt_context* ctx);

/* The frame number the next continuing render will use (accumulatedFrames). */
RT_API unsigned rt_frame_counter(const rt_context* ctx);

/* Default max_bounces for rt_render() (initially RT_DEFAULT_MAX_BOUNCES). */
RT_API int rt_set_max_bounces(rt_context* ctx, int max_bounces);

/* backgroundColor (Main.cu:27, a compile-time constant {0,0,0} there): the
 * radiance of a miss and of the depth cut-off (Main.cu:209-211).  Takes
 * effect at the next render; does not reset accumulation. */
RT_API int rt_set_background(rt_context* ctx, float r, float g, float b);

/* Arithmetic of the GPU render kernels.
 * RT_PRECISION_EXACT (the default): every float operation is one IEEE
 * rounding in the reference's source order; results are bit-identical to the
 * CPU fallback and the oracle.
 * RT_PRECISION_REFERENCE_FAST: the trade-off of the reference's own
 * --use_fast_math build: contracted FMAs, hardware reciprocal / square root /
 * reciprocal square root (1 ulp) with every per-ray division as x * rcp(y),
 * and hardware sine / cosine.  Images agree with the exact mode within 1 LSB
 * per channel on at least 99.5 % of the pixels (mean |delta| <= 0.25 LSB);
 * the rare pixel whose path takes another branch differs arbitrarily.
 * Per context; takes effect at the next render; resets neither the
 * accumulation, nor the frame counter, nor the RNG streams.  An unknown value
 * returns RT_ERR_INVALID_ARGUMENT.  A CPU context accepts EXACT only
 * (REFERENCE_FAST: RT_ERR_UNSUPPORTED): the CPU fallback exists to be
 * bit-identical to the exact kernels. */
typedef enum rt_precision { RT_PRECISION_EXACT = 0, RT_PRECISION_REFERENCE_FAST = 1 } rt_precision;
RT_API int rt_set_precision(rt_context* ctx, int precision);
RT_API int rt_get_precision(const rt_context* ctx);

/* Next-event estimation: with the switch on (1; 0 the
 * default, everything as without it) the render calls — rt_render*, shards,
 * BVH scenes, and the rt_render_adaptive* family's list renders — sample the
 * scene's emissive spheres directly at every diffuse bounce whose scattered ray
 * will be traced, and in exchange drop the emission such a scattered ray finds
 * on a light it could have sampled.  It is another estimator of the same
 * expectation with far less noise where small lights dominate; GPU and CPU
 * contexts agree bit for bit.  With an empty light table, or max_bounces 0, a
 * render is bit-identical to the default estimator's.
 * Frames of both estimators may share one accumulation: both are unbiased for
 * the same value.  Moment tracking (rt_set_moments) assumes equally noisy
 * frames, so restart the accumulation when toggling while tracking.
 * Per context; takes effect at the next render; resets neither the
 * accumulation, nor the frame counter, nor the RNG streams.  Values other than
 * 0 / 1 return RT_ERR_INVALID_ARGUMENT.  With RT_PRECISION_REFERENCE_FAST and
 * the switch on (set in either order), render calls return RT_ERR_UNSUPPORTED
 * and touch nothing. */
RT_API int rt_set_light_sampling(rt_context* ctx, int on);
RT_API int rt_get_light_sampling(const rt_context* ctx);
/* How next-event estimation picks the light of a bounce (DESIGN.md section
 * 24).  RT_LIGHT_PICK_UNIFORM (the default): every table light with the same
 * probability.  RT_LIGHT_PICK_WEIGHTED: with a probability proportional to a
 * bound of what the light can contribute at the shading point — its emitted
 * power, the solid angle of its cone and the largest cosine inside the cone —
 * so shadow rays go to the lights that matter there.  The path itself does not
 * change (same draws, same rays, same RNG state); both picks are unbiased for
 * the same image, the weighted one with less noise where the lights' shares
 * differ, and frames of both may share one accumulation.  Cost: two passes
 * over the light table per diffuse bounce, linear in the number of lights.
 * The mode acts only while light sampling is on; with it off the value is
 * stored and changes nothing, bit for bit.  GPU and CPU contexts agree bit for
 * bit.  Per context; takes effect at the next render; resets neither the
 * accumulation, nor the frame counter, nor the RNG streams.  Other values
 * return RT_ERR_INVALID_ARGUMENT. */
typedef enum rt_light_pick { RT_LIGHT_PICK_UNIFORM = 0, RT_LIGHT_PICK_WEIGHTED = 1 } rt_light_pick;
RT_API int rt_set_light_picking(rt_context* ctx, int mode);
RT_API int rt_get_light_picking(const rt_context* ctx);
/* Which emitters next-event estimation samples.
 * RT_LIGHT_SHAPES_SPHERES (the default): the emissive spheres alone, everything
 * as before this switch, bit for bit.  RT_LIGHT_SHAPES_ALL: emissive triangles
 * and quads as well — a point uniform on the polygon's area, weighed by
 * area * cos / distance^2; polygons emit to both sides, as they are hit from
 * both.  A triangle is sampled when its emittance is finite and > 0, its
 * vertices are finite and its normal cross(v1 - v0, v2 - v1) is finite and not
 * 0; a quad when in addition its projection along that normal into the plane
 * through v0 (what a ray can hit) is convex with both halves (v0, v1, v2) and
 * (v0, v2, v3) of positive area.  Every other emitter (planes, non-convex
 * quads, ...) is found by chance as ever, which is always unbiased.  A scene
 * without such a polygon renders under ALL what it renders under SPHERES, with
 * the same kernel.  The paths draw the same numbers under both modes (same RNG
 * state); both are unbiased for the same image, and frames of both may share
 * one accumulation.  Combines with both pick modes.
 * The mode acts only while light sampling is on; with it off the value is
 * stored and changes nothing, bit for bit.  GPU and CPU contexts agree bit for
 * bit.  Per context; takes effect at the next render; resets neither the
 * accumulation, nor the frame counter, nor the RNG streams.  Other values
 * return RT_ERR_INVALID_ARGUMENT. */
typedef enum rt_light_shapes { RT_LIGHT_SHAPES_SPHERES = 0, RT_LIGHT_SHAPES_ALL = 1 } rt_light_shapes;
RT_API int rt_set_light_shapes(rt_context* ctx, int mode);
RT_API int rt_get_light_shapes(const rt_context* ctx);
/* The light table the scene compiler built at rt_set_scene, as the current
 * shapes mode sees it: one record of RT_LIGHT_RECORD_FLOATS floats per sphere
 * with finite emittance > 0 and finite radius > 0, in sphere order: {cx, cy,
 * cz, r*r, emitted.r, emitted.g, emitted.b, primitive id as int32 bits},
 * emitted = emittance * albedo; under RT_LIGHT_SHAPES_ALL followed by one
 * record per sampled triangle and then per sampled quad, in primitive order
 * (the ids of the whole table ascend): {centre and squared radius of a sphere
 * that contains the vertices, emitted, primitive id}.  (Other emitters are
 * found by chance as ever.)  Returns the number of records (or a negative
 * error) and copies at most `capacity` of them to `out` (may be null with
 * capacity 0). */
#define RT_LIGHT_RECORD_FLOATS 8
RT_API int rt_get_lights(rt_context* ctx, float* out, int capacity);
/* A light hierarchy for weighted picking.  With the
 * switch on (1; 0 the default), RT_LIGHT_PICK_WEIGHTED picks its light by a
 * stochastic descent of a binary tree that rt_set_scene builds over the light
 * table — at every node one of the two children, with a probability
 * proportional to a bound of what the lights below it can contribute at the
 * shading point (summed power over squared distance, times the largest cosine
 * towards the node's bounding sphere; a child that is a single light takes
 * that light's own weight) — instead of walking the whole table twice: the
 * cost per diffuse bounce is the depth of the tree, at most
 * ceil(log2 n) + 1 levels, where the walk's is linear in n.  The pick
 * probabilities approximate the walk's, they do not equal them; both are
 * unbiased for the same image, and the path itself does not change (same
 * draws, same rays, same RNG state), so frames of every pick mode may share one
 * accumulation.
 * The value is stored independently of the other switches and acts only while
 * light sampling is on, picking is weighted and the table the render sees
 * (rt_set_light_shapes) holds at least 2 records; everywhere else a render is
 * bit for bit what it is without the switch.  GPU and CPU contexts agree bit
 * for bit.  Per context; takes effect at the next render; resets neither the
 * accumulation, nor the frame counter, nor the RNG streams.  Values other than
 * 0 / 1 return RT_ERR_INVALID_ARGUMENT. */
RT_API int rt_set_light_hierarchy(rt_context* ctx, int on);
RT_API int rt_get_light_hierarchy(const rt_context* ctx);
/* The light tree of the table that the current shapes mode sees, as
 * rt_get_lights returns that table: 2 n - 1 nodes of RT_LIGHT_NODE_FLOATS
 * floats for a table of n >= 2 records, none for a smaller one.  Nodes
 * [0, n - 1) are internal, the root first and every parent in front of its
 * children; node n - 1 + j is the leaf of table record j.
 *   {cx, cy, cz, R*R, phi, a, b, parent}      (a, b, parent: int32 bits)
 * {c, R*R}: a bounding sphere — a leaf's is its record's, an internal node's
 * contains both children's, in exact arithmetic on the stored floats.  phi:
 * the power term, a leaf's (|e.r| + |e.g| + |e.b|) r*r for a sphere and
 * (|e.r| + |e.g| + |e.b|) area / pi for a polygon, an internal node's the float
 * sum phi(a) + phi(b).  a, b: the children's node indices; a leaf has
 * {j, -1}.  parent: -1 for the root.  Returns the number of nodes (or a
 * negative error) and copies at most `capacity` of them to `out` (may be null
 * with capacity 0).  The tree is built whether or not the switch is on. */
#define RT_LIGHT_NODE_FLOATS 8
RT_API int rt_get_light_tree(rt_context* ctx, float* out, int capacity);
/* Where the shadow rays go: the probability with which next-event estimation,
 * under the context's current pick mode (rt_set_light_picking,
 * rt_set_light_hierarchy) and shapes mode, picks each table light at `count`
 * shading points.  Point i is points[6 i ..] = {P.xyz, n.xyz}, n the shading
 * normal as the path has it (a sphere's is of unit length, a plane's or
 * polygon's is its unnormalised one), on primitive prims[i] (-1: on none).
 * out takes count x n floats, n the number of table lights (the return value;
 * 0: nothing is written): row i holds 1 / n under uniform picking, w_j / W
 * under weighted picking and, with the hierarchy, the product of the branch
 * probabilities down to light j's leaf — computed by the functions the sampler
 * itself picks with, whether or not light sampling is on.  A row is all 0
 * where the pick rule gives no direct term (no light has a positive weight
 * there) or where a hit with that normal takes no light sample.  A GPU context
 * computes it on the device, a CPU context on the host; they agree bit for
 * bit.  Returns n or a negative error. */
RT_API int rt_light_pick_probabilities(rt_context* ctx, const float* points, const int* prims, int count, float* out);

/* samplesPerPixel (Main.cu:27, a compile-time constant 1 there): each
 * progressive frame traces n paths from the frame's one jittered camera ray
 * and, like the reference's loop (Main.cu:296-299, `pixel = tracePath(...)`
 * assigns), keeps the LAST one, scaled by 1/n; the RNG draws of all n are
 * consumed.  Default 1, the reference build (and the only value whose frames
 * are unbiased).  n > 1 renders with the one-path-per-lane kernel.  Takes
 * effect at the next render; does not reset accumulation. */
#define RT_MAX_SAMPLES_PER_PIXEL 1024
RT_API int rt_set_samples_per_pixel(rt_context* ctx, int n);

/* Copy of the context's current camera (after rt_controls()). */
RT_API int rt_get_camera(const rt_context* ctx, rt_camera* camera);

/* ---- camera controls (Controls.cuh:5-75) ----------------------------------
 * `keys` = OR of the RT_KEY_* held during the frame, `delta_time` = that
 * frame's duration in seconds (Main.cu:482).  Movement speed 5/s, rotation
 * speed 2 rad/s, directions from rotY(angle[0]) * rotX(angle[1]) applied to
 * (0,0,-1) / (1,0,0), evaluated in float in the reference's operation order.
 * Returns an OR of RT_CONTROLS_MOVED (any movement key: accumulation restarts,
 * accumulatedFrames = 1) and RT_CONTROLS_QUIT (escape), or a negative
 * rt_status. */
#define RT_KEY_W          (1u << 0)  /* forward */
#define RT_KEY_A          (1u << 1)  /* left */
#define RT_KEY_S          (1u << 2)  /* back */
#define RT_KEY_D          (1u << 3)  /* right */
#define RT_KEY_SPACE      (1u << 4)  /* up (world y) */
#define RT_KEY_LEFT_SHIFT (1u << 5)  /* down (world y) */
#define RT_KEY_LEFT       (1u << 6)  /* yaw +   (angle[0]) */
#define RT_KEY_RIGHT      (1u << 7)  /* yaw -   */
#define RT_KEY_UP         (1u << 8)  /* pitch + (angle[1]) */
#define RT_KEY_DOWN       (1u << 9)  /* pitch - */
#define RT_KEY_ESCAPE     (1u << 10) /* glfwSetWindowShouldClose */
#define RT_CONTROLS_MOVED 1
#define RT_CONTROLS_QUIT 2

/* Apply one frame of controls to a camera (no context, no GPU). */
RT_API int rt_apply_controls(rt_camera* camera, unsigned keys, float delta_time);

/* Apply one frame of controls to the context's camera; on movement the
 * frame counter restarts at 1 (the next render resets frameSum). */
RT_API int rt_controls(rt_context* ctx, unsigned keys, float delta_time);

/* Allocate and seed the per-pixel state for a (width,height) image shard:
 * curand_init(y*width+x, 0, 0) per pixel (Main.cu:369-380) and a frameSum
 * buffer (Main.cu:464-465).  Called implicitly by the render entry points
 * when the shard changes; calling it again reseeds the RNG. */
RT_API int rt_init_rand(rt_context* ctx, int width, int height,
                        int row_offset, int row_stride);

/* Drop-in render(width, height, samples): renders `samples` progressive
 * frames continuing the context's frame counter, with the context's
 * max_bounces, over the full image, and writes the final RGBA8 image
 * (width*height*4 bytes, row 0 = bottom) to host memory.  rgba_out may be
 * NULL. */
RT_API int rt_render(rt_context* ctx, int width, int height, int samples,
                     uint8_t* rgba_out);

/* Extended synchronous render.  Output rows are the shard's rows in order
 * (rows = number of y with y = row_offset + j*row_stride < height).
 * rgba_out: rows*width*4 bytes or NULL; accum_out: rows*width*3 floats
 * (frameSum, interleaved r,g,b) or NULL. */
RT_API int rt_render_ex(rt_context* ctx, const rt_render_params* p,
                        uint8_t* rgba_out, float* accum_out);

/* Asynchronous render into DEVICE memory (rows*width*4 bytes, 4-byte
 * aligned) on HIP stream `stream` (hipStream_t; NULL = the context's own
 * stream).  Returns after the launch; the frame counter advances.  A render
 * on a different stream than the context's previous render is ordered after
 * it on the device (stream wait on an event; no host synchronisation). */
RT_API int rt_render_device(rt_context* ctx, const rt_render_params* p,
                            void* rgba_device, void* stream);

/* The context's own HIP stream (hipStream_t), valid until rt_destroy (NULL
 * for a CPU context), created at the device's highest stream priority, so a
 * render on it dispatches ahead of work on the caller's other streams (a
 * gather of the previous frame).  Renders on it (rt_render_device with this stream or
 * NULL) record their completion event lazily — when a later call needs it:
 * a render on another stream, a state read or write, rt_synchronize — so
 * back-to-back renders carry no marker packet between them (1.5-3 us per
 * launch on MI355X).  Such a deferred event is recorded at the end of the
 * stream when the later call comes, so it also covers any work the caller
 * queued on this stream after the render (a gather, a copy): calls that wait
 * for the render wait for that work too.  A render on a caller's stream
 * records it at once (the caller may destroy that stream). */
RT_API void* rt_get_stream(rt_context* ctx);

/* Wait for all work of the context: its stream, the last render launch
 * (also on a caller's stream, rt_render_device) and the last
 * rt_deinterleave_rows_device. */
RT_API int rt_synchronize(rt_context* ctx);

/* One image across n contexts in ONE process (one context per GPU, the same
 * scene / camera / max_bounces set on each; the C++ host's multi-GPU path,
 * SURVEY §8e): context i renders rows y = i (mod n) of the frames that
 * continue its own frame counter, all contexts concurrently on their own
 * streams; the RGBA8 rows are gathered into rgba_out (host, width*height*4,
 * row 0 = bottom; may be NULL).  Keep the contexts' frame counters in step by
 * always rendering them together.  Equal to one context rendering the whole
 * image (tests/test_gpu_parity.py).  On failure every context's queued work
 * has finished when the call returns, but the contexts that did launch have
 * advanced their RNG state and frame counter while the others have not:
 * re-seed all of them (rt_init_rand) before rendering together again. */
RT_API int rt_render_multi(rt_context* const* ctxs, int n, int width, int height, int samples,
                           uint8_t* rgba_out);

/* Duration (ms, HIP events on the launch stream) of the last render kernel
 * launch; -1 when unavailable (no render yet, or kernel timing off).
 * Synchronises on that launch's end event. */
RT_API float rt_last_kernel_ms(rt_context* ctx);

/* Name of the render kernel the context's last GPU render launched, with
 * its workgroup lanes and variant, e.g. "rt_render_sorted_kernel<256,grec>+order"
 * (full frames), "rt_render_pair_kernel<128>+order" (small frames and
 * shards), "rt_render_bvh_refill_kernel<64,n16>" (BVH scenes); a
 * RT_PRECISION_REFERENCE_FAST launch carries ",fast" inside the angle
 * brackets, e.g. "rt_render_pair_kernel<128,fast>+order"; a sorted-kernel
 * launch that was given a sky table (rt_sky_table) ends in "+sky"; "" before
 * the first render and on a CPU context.  A diagnostic of the launch
 * policy (tests assert which kernel a workload runs); valid until the next
 * render on the context.  An adaptive call reports its list render kernel:
 * "rt_render_list_kernel<256,grec>" (queued) or "rt_render_kernel<256,list>"
 * (one path per lane; ",bvh,list" on BVH scenes).  The reference launches one
 * kernel, Main.cu:342. */
RT_API const char* rt_last_kernel_name(const rt_context* ctx);

/* Per-launch kernel timing (default on): every render records a start event
 * before its kernels; its end event (recorded either way: later calls are
 * ordered after it) closes the interval rt_last_kernel_ms reports.  Each event
 * is a marker packet the GPU drains between two launches (MI355X, config 3:
 * the start marker costs 5-7 us per launch, ~1 %; tools/ev_ab.sh,
 * profiles/r03d/launch_events/).  Off, rt_last_kernel_ms returns -1.  The
 * reference times nothing on the device (it prints host-side FPS,
 * Main.cu:486-495). */
RT_API int rt_set_kernel_timing(rt_context* ctx, int enable);

/* The sky table of the view (p: width, height, row_offset, row_stride; the
 * context's scene and camera): one bit per 64-pixel wave tile of the launch
 * order (tile t: bit t % 32 of word t / 32), set when every camera ray of
 * the tile, under any jitter, provably misses every primitive.  A full frame's
 * sorted brute-force launch renders tile groups whose bits are all set
 * without the path machinery (per frame: the jitter's rejection loop and
 * frameSum += background; bit-identical results).  tile_w: the tile's width in
 * pixels (a power of two up to 64; 64 / tile_w rows), -1 = the launch policy's
 * for this view; tile_sq: every 4 consecutive tiles as a 2 x 2 block.  Writes
 * the first `words` words of the table (zero past its end), the number of
 * tiles and the number of tables the context has built so far (it keeps the
 * last one and rebuilds only when the scene, the camera or the view changes).
 * No bit is set when nothing can be proven: scenes scaled beyond 1e9,
 * non-finite values, the camera inside a bounding sphere, skinny triangles,
 * non-convex or non-planar quads, BVH scenes, samplesPerPixel > 1, tile_w 0.
 * Host arithmetic only: works on CPU contexts too.  No counterpart in the
 * reference. */
RT_API int rt_sky_table(rt_context* ctx, const rt_render_params* p, int tile_w, int tile_sq,
                        uint32_t* bits, size_t words, long long* tiles_out,
                        unsigned long long* builds_out);

/* Number of pixel rows in the shard (row_offset, row_stride) of `height`. */
RT_API int rt_shard_rows(int height, int row_offset, int row_stride);

/* Multi-GPU gather epilogue: `gathered` holds `shards` consecutive blocks
 * of rows_per_shard*width RGBA8 pixels, block r = rows r, r+shards, ...
 * (row_stride = shards) padded to rows_per_shard.  Writes the full
 * height*width image to `image` (both device pointers) on `stream`. */
RT_API int rt_deinterleave_rows_device(rt_context* ctx, const void* gathered,
                                       void* image, int width, int height,
                                       int shards, int rows_per_shard,
                                       void* stream);

/* Checkpoint / resume of the progressive state of the current shard.
 * rng: 6*rows*width uint32 as planes (d, v0..v4), accum: 3*rows*width floats
 * interleaved r,g,b.  Either pointer may be NULL. */
RT_API int rt_get_state(rt_context* ctx, uint32_t* rng, float* accum);
RT_API int rt_set_state(rt_context* ctx, const uint32_t* rng,
                        const float* accum, unsigned frame_counter);

/* ---- first-hit feature buffers (AOVs) and the denoiser -----------------------
 * Neither reads or writes the RNG state, frameSum or the frame counter: a
 * render that continues after them is bit-identical to one never interrupted.
 * Both always use the exact arithmetic, whatever rt_set_precision says, and
 * give bit-identical results on GPU and CPU contexts. */

/* First-hit feature buffers of the shard (p->width, height, row_offset,
 * row_stride; the other fields of p are ignored), from the un-jittered primary
 * ray of each pixel (no RNG draw): the material's raw albedo, the path
 * tracer's shading normal (unit length, not flipped towards the camera), the
 * hit distance and the primitive id (spheres, planes, triangles, quads in
 * turn).  A miss gives the background colour, normal 0, depth +inf, prim -1.
 * Rows as rt_render_ex; any output pointer may be NULL. */
RT_API int rt_render_aov(rt_context* ctx, const rt_render_params* p,
                         float* albedo /*rows*w*3*/, float* normal /*rows*w*3*/,
                         float* depth /*rows*w*/, int32_t* prim /*rows*w*/);

/* Edge-avoiding a-trous wavelet filter (Dammertz et al. 2010; a plane-distance
 * term for their position term) over frameSum / n, guided by the first-hit
 * normal, hit point and hit / miss class; DESIGN.md has the exact definition. */
#define RT_DENOISE_MAX_ITERATIONS 6
typedef struct rt_denoise_params {
    int iterations;      /* 0..RT_DENOISE_MAX_ITERATIONS; level i has tap step 1<<i */
    float sigma_color;   /* > 0, +inf allowed (term off); level i uses sigma_color * 2^-i */
    float sigma_normal;  /* > 0, +inf allowed */
    float sigma_plane;   /* > 0, +inf allowed; world units */
} rt_denoise_params;
RT_API rt_denoise_params rt_denoise_params_default(void);

/* Filter the context's accumulated full frame.  rgba_out: w*h*4 bytes or NULL;
 * color_out: w*h*3 linear floats (the filtered frameSum / n) or NULL.  With
 * iterations == 0 the RGBA equals the last render's.  RT_ERR_INVALID_ARGUMENT:
 * iterations out of range, a sigma <= 0 or NaN, or no frame accumulated yet
 * (frame counter < 2); RT_ERR_NO_SCENE; RT_ERR_UNSUPPORTED: the context's
 * pixel state is a row shard (row_offset != 0 or row_stride > 1: the
 * neighbours of its rows live on other contexts) and it has no current
 * assembled frame (rt_assemble below: with one, the filter reads that frame and
 * its frame count instead; the same holds for rt_denoise_var and rt_temporal). */
RT_API int rt_denoise(rt_context* ctx, const rt_denoise_params* params,
                      uint8_t* rgba_out, float* color_out);
/* As above into DEVICE memory (w*h*4 bytes, 4-byte aligned, or NULL) on HIP
 * stream `stream`, with rt_render_device's ordering rules: returns after the
 * launches; ordered after the context's last render and before its next one
 * on the device, whatever streams they use.  CPU context: RT_ERR_UNSUPPORTED. */
RT_API int rt_denoise_device(rt_context* ctx, const rt_denoise_params* params,
                             void* rgba_device, void* stream);
/* Duration (ms) of all levels of the last denoise call (HIP events on its
 * stream; wall time on a CPU context); -1 when unavailable. */
RT_API float rt_last_denoise_ms(rt_context* ctx);

/* ---- temporal reprojection across camera moves ---------------------------------
 * A camera change restarts the accumulation (frameSum is reset by the next
 * render).  rt_temporal() keeps what the previous view had accumulated: it
 * reprojects that view's colour into the current one through the first-hit
 * geometry (the temporal stage of SVGF, Schied et al. 2017) and blends it with
 * frameSum / n by effective sample counts; DESIGN.md section 10 has the exact
 * definition.  Like the denoiser it reads neither the RNG state nor writes
 * frameSum or the frame counter, always uses the exact arithmetic, and gives
 * bit-identical results on GPU and CPU contexts.
 *
 * The context counts views: a new one starts at rt_set_scene, rt_set_camera, a
 * moving rt_controls and a change of the frame shape.  A call writes the
 * *pending* result of the current view {colour, effective sample count, the
 * view's first-hit guides and camera}; the first call in a later view promotes
 * the pending result to the *history* (a buffer swap) and reprojects from it.
 * Repeated calls in one view leave the history alone and overwrite the pending
 * result.  rt_set_scene (primitive ids change meaning), a change of width or
 * height and rt_temporal_reset drop both.  The scene is static between
 * rt_set_scene calls: equal primitive ids are the occlusion test.  Nothing is
 * allocated before the first call. */
typedef struct rt_temporal_params {
    float max_history;     /* > 0: cap on the reprojected effective sample count */
    float normal_cos_min;  /* -1..1: least cosine between the normals of a pixel and a history tap */
    float plane_tol;       /* > 0: largest distance of a tap's hit point from the pixel's tangent
                              plane, relative to the pixel's hit distance */
} rt_temporal_params;
RT_API rt_temporal_params rt_temporal_params_default(void);

/* Reproject into the context's accumulated full frame.  dn == NULL: no spatial
 * filter; else the a-trous levels of rt_denoise run over the temporal colour
 * instead of frameSum / n (dn->iterations == 0: as NULL), and rgba_out /
 * color_out are the filtered result; the stored history is always the
 * unfiltered colour.  rgba_out: w*h*4 bytes or NULL; color_out: w*h*3 linear
 * floats or NULL; length_out: w*h effective sample counts or NULL (n where
 * nothing was reprojected).  Errors as rt_denoise: RT_ERR_INVALID_ARGUMENT (a
 * parameter out of range or NaN, no frame accumulated yet), RT_ERR_NO_SCENE,
 * RT_ERR_UNSUPPORTED (a row shard). */
RT_API int rt_temporal(rt_context* ctx, const rt_temporal_params* params, const rt_denoise_params* dn,
                       uint8_t* rgba_out, float* color_out, float* length_out);
/* As above into DEVICE memory (w*h*4 bytes, 4-byte aligned, or NULL) on HIP
 * stream `stream` (NULL = the context's), with rt_denoise_device's ordering
 * rules: after the context's last render, denoise and temporal call, before
 * its next ones, whatever streams they use.  CPU context: RT_ERR_UNSUPPORTED. */
RT_API int rt_temporal_device(rt_context* ctx, const rt_temporal_params* params, const rt_denoise_params* dn,
                              void* rgba_device, void* stream);
/* Drop the history and the pending result (the buffers stay allocated). */
RT_API int rt_temporal_reset(rt_context* ctx);
/* Duration (ms) of the reprojection pass alone of the last temporal call (HIP
 * events on its stream; wall time on a CPU context); -1 when unavailable. */
RT_API float rt_last_temporal_ms(rt_context* ctx);

/* ---- luminance moment tracking (per-pixel noise estimate) -----------------------
 * Opt-in, off by default.  While on, every render entry point (rt_render,
 * rt_render_ex, rt_render_device, rt_render_cpu, rt_render_multi per context)
 * runs one small extra pass over the context's shard behind the render (on a
 * GPU context on the same stream, before the launch's end event, so
 * rt_last_kernel_ms includes it and every call ordered after the render is
 * ordered after it).  It treats the k frames of the call as one *batch*: from
 * frameSum before and after the call it takes the batch's mean luminance l
 * (Rec. 709 weights) and updates, per pixel, the weighted mean M of the batch
 * luminances and M2 = sum_j k_j (l_j - M)^2 (weighted Welford; DESIGN.md
 * section 11 and csrc/rt_moments.h have the exact arithmetic).  The pass reads
 * frameSum and writes only its own buffers: RGBA, frameSum, RNG state and
 * frame counter of any sequence of calls are bit-identical with tracking on
 * and off, and GPU and CPU contexts compute the same moments bit for bit.
 *
 * Tracking goes *live* at a render whose first frame is 1 (the render that
 * resets frameSum; so after rt_reset_accumulation, rt_set_camera, a moving
 * rt_controls and rt_set_scene the next render restarts it) and stays live
 * while each following render's first frame is the frame after the last
 * tracked one.  It ends (no batches) at rt_set_state, rt_init_rand (also the
 * implicit one of a shape change), a render whose first frame is neither 1 nor
 * the expected next, rt_set_moments(ctx, 0), and when it is enabled in
 * mid-accumulation.  A render while not live skips the pass.  Nothing is
 * allocated before tracking is on and a render runs (20 bytes per pixel). */
RT_API int rt_set_moments(rt_context* ctx, int enable);
RT_API int rt_get_moments(const rt_context* ctx);
/* Tracked batches J (render calls) of the current accumulation; 0 when not live. */
RT_API int rt_moments_batches(const rt_context* ctx);
/* The shard's rows * width estimates, rows as rt_render_ex; either pointer may
 * be NULL.  var_out = M2 / ((J - 1) n): an unbiased estimate of the variance of
 * the pixel's MEAN luminance after the n accumulated frames (its square root
 * is the standard error of frameSum / n in luminance), whatever the batch
 * sizes; lum_out = M, that mean luminance.  RT_ERR_INVALID_ARGUMENT when
 * tracking is not live or J < 2 (one batch has no spread).  Synchronous. */
RT_API int rt_get_variance(rt_context* ctx, float* var_out, float* lum_out);

/* ---- variance-guided a-trous filter ------------------------------------------------
 * rt_denoise with its colour term replaced by SVGF's (Schied et al. 2017): the
 * luminance difference of a tap is measured in standard deviations of the
 * pixel's own noise, so no colour sigma has to be chosen for a scene's
 * brightness or a frame's sample count, and a per-pixel variance is filtered
 * along with the colour (sum of w^2 v / (sum of w)^2).  The variance of the
 * frame comes from the moment tracking when it is live with at least
 * min_batches batches, else (also with tracking off) from a spatial estimate
 * over the 7 x 7 neighbourhood; DESIGN.md section 11 and csrc/rt_denoise_var.h
 * have the exact definition.  Errors, ordering and neutrality are rt_denoise's:
 * full frames only, frame counter >= 2, exact arithmetic whatever
 * rt_set_precision says, the same bits on GPU and CPU contexts, and neither the
 * RNG state, frameSum, the frame counter nor the tracked moments are written. */
typedef struct rt_denoise_var_params {
    int iterations;      /* 0..RT_DENOISE_MAX_ITERATIONS; level i has tap step 1<<i */
    float sigma_lum;     /* > 0: luminance sigma in standard deviations (SVGF: 4) */
    float sigma_normal;  /* as rt_denoise_params */
    float sigma_plane;   /* as rt_denoise_params */
    int min_batches;     /* >= 2: below this many tracked batches, use the spatial estimate (SVGF: 4) */
} rt_denoise_var_params;
RT_API rt_denoise_var_params rt_denoise_var_params_default(void);
/* rgba_out: w*h*4 bytes or NULL; color_out: w*h*3 linear floats or NULL;
 * var_out: w*h filtered variances of the mean luminance or NULL.  With
 * iterations == 0 the colour is frameSum / n, the variance the input estimate
 * and the RGBA equals the last render's.  Errors as rt_denoise, and
 * RT_ERR_INVALID_ARGUMENT for sigma_lum <= 0 or NaN and min_batches < 2. */
RT_API int rt_denoise_var(rt_context* ctx, const rt_denoise_var_params* params, uint8_t* rgba_out,
                          float* color_out, float* var_out);
/* As above into DEVICE memory on HIP stream `stream`, with rt_denoise_device's
 * ordering rules (after the context's last render, denoise, temporal and
 * variance-guided call, before its next ones).  CPU context: RT_ERR_UNSUPPORTED. */
RT_API int rt_denoise_var_device(rt_context* ctx, const rt_denoise_var_params* params, void* rgba_device,
                                 void* stream);
/* Duration (ms) of all passes of the last rt_denoise_var call; -1 when unavailable. */
RT_API float rt_last_denoise_var_ms(rt_context* ctx);

/* ---- temporal reprojection of the luminance moments ---------------------------------
 * rt_temporal that also carries a per-pixel estimate of the luminance variance
 * across camera moves (SVGF's temporal stage with its variance estimate), so a
 * host that renders one call per view can still ask how noisy a pixel is, and
 * the variance-guided levels can run behind the reprojection.  Beside colour
 * and length every history set holds {s2, dof}: the pooled estimate of the
 * pixel's PER-FRAME luminance variance and its degrees of freedom; s2 / length
 * is the variance of the mean luminance.  A call merges the history's estimate,
 * the current frame's tracked moments when rt_set_moments is on and live with
 * two batches or more (else nothing: tracking may stay off), and the squared
 * difference between the history's and the current view's luminance (the
 * pairwise merge of two Welford accumulators; DESIGN.md section 21 and
 * csrc/rt_temporal_var.h have the exact definition).  Real signal change
 * between views counts as noise: the estimate errs towards "noisier".
 *
 * Colour, length and RGBA of the unfiltered call are rt_temporal's bit for bit.
 * The call shares rt_temporal's history sets, view counting, promotion rule
 * and drops, and the two may follow each other in any order: a set that
 * rt_temporal wrote has no moments, and its taps count with s2 = dof = 0.  The
 * moment planes (8 bytes per pixel and set) are allocated by the first
 * rt_temporal_var call.  Neutrality and arithmetic as rt_temporal; the tracked
 * moments are only read.
 *
 * dv == NULL or dv->iterations == 0: no filter.  Else the levels of
 * rt_denoise_var run over the reprojected colour; their input variance is
 * s2 / length where dof >= dv->min_batches - 1.5, else the spatial estimate of
 * rt_denoise_var over the reprojected colours.  The stored history is always
 * the unfiltered one.  rgba_out, color_out, length_out as rt_temporal;
 * moments_out: w*h pairs {variance of the mean luminance, dof} or NULL:
 * unfiltered s2 / length (0 where dof is 0), filtered the levels' final
 * variance; dof is the unfiltered one in both.
 * Errors as rt_temporal and rt_denoise_var, and RT_ERR_UNSUPPORTED for a
 * non-uniform accumulation or a counted assembled frame, with or without
 * rt_set_adaptive_filters (rt_temporal_var_counted below takes those). */
RT_API int rt_temporal_var(rt_context* ctx, const rt_temporal_params* params, const rt_denoise_var_params* dv,
                           uint8_t* rgba_out, float* color_out, float* length_out, float* moments_out);
/* As above into DEVICE memory, with rt_temporal_device's rules. */
RT_API int rt_temporal_var_device(rt_context* ctx, const rt_temporal_params* params,
                                  const rt_denoise_var_params* dv, void* rgba_device, void* stream);
/* Duration (ms) of the reprojection pass alone of the last rt_temporal_var call
 * (the levels behind it: rt_last_denoise_var_ms); -1 when unavailable. */
RT_API float rt_last_temporal_var_ms(rt_context* ctx);

/* ---- variance-driven adaptive sampling ---------------------------------------------
 * The tracked moments say how noisy each pixel still is; rt_render_adaptive()
 * spends the next `samples` frames only on the pixels whose neighbourhood has
 * not converged.  Per pixel q, v_q = M2_q / ((J_q - 1) n_q) estimates the
 * variance of its mean luminance.  Over the window |dx|, |dy| <= radius
 * (clipped to the image; taps with a non-finite v or M are skipped; c taps)
 * a pixel is *hot* when
 *     sqrt(sum v / c)  >  tolerance * (sum M / c + lum_floor)
 * evaluated without a division as (sum v) c > (tolerance (sum M + c lum_floor))^2
 * (csrc/rt_adaptive.h and DESIGN.md section 14 have the exact float
 * operations; GPU and CPU contexts select the same pixels).  Then
 *     selected = (max_frames == 0 || n_p + samples <= max_frames) &&
 *                (n_p < min_frames || hot)
 * Every pixel owns its RNG stream, so a pixel that has received n_p frames
 * holds exactly the frameSum, RNG state and RGBA a uniform render stopped at
 * n_p frames would have given it, on both backends.
 *
 * The first adaptive call of an accumulation allocates one {n_p, J_p} pair per
 * pixel (frames accumulated, moment batches tracked), filled with the
 * context's counts; nothing is allocated before.  From then on the
 * accumulation is *non-uniform*, until a render whose first frame is 1,
 * rt_set_scene, rt_init_rand (also the implicit one), rt_set_state or
 * rt_set_moments(ctx, 0) (after rt_reset_accumulation, rt_set_camera and a
 * moving rt_controls the next render starts at frame 1).  While non-uniform:
 *  - a uniform render that continues (first_frame 0 or any value but 1) and
 *    rt_render_multi return RT_ERR_UNSUPPORTED;
 *  - rt_denoise*, rt_denoise_var* and rt_temporal* return RT_ERR_UNSUPPORTED
 *    unless rt_set_adaptive_filters() (below) is on;
 *  - rt_get_state and rt_render_aov work as ever; rt_get_variance uses each
 *    pixel's own J_p and n_p; rt_frame_counter and rt_moments_batches keep
 *    reporting the uniform base (adaptive calls do not advance them);
 *  - the counts are not part of rt_get_state / rt_set_state: a non-uniform
 *    accumulation cannot be checkpointed (rt_set_state ends it).
 * A context that never calls these entry points behaves bit for bit as before.
 *
 * Errors: RT_ERR_NO_SCENE; RT_ERR_INVALID_ARGUMENT when moment tracking is not
 * live or has fewer than 2 batches, when the accumulation was restarted
 * (rt_reset_accumulation, rt_set_camera, a moving rt_controls, rt_set_scene)
 * and nothing rendered since (the moments describe the old one: render first;
 * nothing is touched), a parameter is out of range or NaN, or a
 * count could pass 2^32 - 1; RT_ERR_UNSUPPORTED when the context's pixel state
 * is a row shard (the window needs neighbours), in RT_PRECISION_REFERENCE_FAST
 * (a list schedule would be a new arithmetic form of that mode, whose results
 * depend on the schedule), for max_bounces above RT_MAX_BOUNCES, and for the
 * device variant on a CPU context.  The view is the context's current full
 * frame: width and height are the context's. */
#define RT_ADAPTIVE_MAX_RADIUS 4
typedef struct rt_adaptive_params {
    int samples;         /* k >= 1: frames added to every selected pixel */
    float tolerance;     /* > 0: root of the window-mean variance of the mean over window-mean luminance */
    float lum_floor;     /* >= 0: added to the window-mean luminance */
    int radius;          /* 0..RT_ADAPTIVE_MAX_RADIUS: window half-width in pixels */
    unsigned min_frames; /* a pixel with n_p < min_frames is always selected (0: none forced) */
    unsigned max_frames; /* a pixel with n_p + k > max_frames is never selected (0: no cap) */
} rt_adaptive_params;
typedef struct rt_adaptive_stats {
    long long selected;      /* pixels the last call rendered */
    long long frames_total;  /* sum of n_p after it */
    float select_ms, render_ms, resolve_ms;  /* -1 when unavailable (GPU: kernel timing off) */
} rt_adaptive_stats;
RT_API rt_adaptive_params rt_adaptive_params_default(void);
/* Select, render `samples` frames of the selected pixels (max_bounces < 0: the
 * context's), update their moments and counts, and resolve the whole frame:
 * RGBA = tone map of frameSum / n_p for every pixel (complete whatever earlier
 * renders wrote).  rgba_out: w*h*4 bytes or NULL; color_out: w*h*3 floats
 * (frameSum / n_p) or NULL; stats_out may be NULL.  Synchronous. */
RT_API int rt_render_adaptive(rt_context* ctx, const rt_adaptive_params* params, int max_bounces,
                              uint8_t* rgba_out, float* color_out, rt_adaptive_stats* stats_out);
/* As above with the RGBA into DEVICE memory (w*h*4 bytes, 4-byte aligned, or
 * NULL) on HIP stream `stream` (NULL = the context's), with rt_render_device's
 * ordering rules; asynchronous like it.  No host synchronisation happens
 * inside the call: the list of selected pixels and its length stay on the
 * device. */
RT_API int rt_render_adaptive_device(rt_context* ctx, const rt_adaptive_params* params, int max_bounces,
                                     void* rgba_device, void* stream);
/* The statistics of the last adaptive call; synchronises on it. */
RT_API int rt_adaptive_last_stats(rt_context* ctx, rt_adaptive_stats* stats_out);
/* Per-pixel counts, w*h each, either may be NULL: frames accumulated and moment
 * batches tracked.  In the uniform state every pixel reports the context's
 * (frame counter - 1, rt_moments_batches).  Synchronous. */
RT_API int rt_get_counts(rt_context* ctx, uint32_t* frames_out, uint32_t* batches_out);

/* ---- adaptive sampling for a moving camera ------------------
 * rt_render_adaptive needs two batches of one accumulation, which a host that
 * renders one call per view never has.  rt_temporal_var carries {s2, dof} and a
 * length per pixel across camera moves; rt_render_adaptive_reprojected selects
 * from those PENDING planes of the current view and rt_temporal_var_counted
 * merges the then non-uniform frame with the same history.  Per view:
 *   1. rt_render: k0 frames, uniform, rt_set_moments on;
 *   2. rt_temporal_var: the pending {out, len, s2, dof} of this view;
 *   3. rt_render_adaptive_reprojected: k more frames for the selected pixels;
 *   4. rt_temporal_var_counted (+ levels): the displayed frame
 * (rt_set_adaptive_filters on).  Steps 3 and 4 may repeat within a view.
 *
 * Selection (csrc/rt_adaptive.h has the float operations): per pixel q of the
 * pending planes v_q = s2_q / len_q, m_q = luminance of out_q; a tap counts in
 * the window iff dof_q > 0 and v_q, m_q are finite; hot is rt_render_adaptive's
 * expression over the window;
 *     fresh    = prim_p >= 0 && !(dof_p >= min_dof)
 *     selected = (max_frames == 0 || n_p + samples <= max_frames) &&
 *                (n_p < min_frames || hot || fresh)
 * A hit pixel about which the history says nothing or too little is rendered
 * (disocclusions, the first view); miss pixels are not forced.  Every stage
 * behind the selection is rt_render_adaptive's, the outputs and
 * rt_adaptive_last_stats too, and afterwards the accumulation is non-uniform
 * exactly as after it (the replay property holds).  The pending set is only
 * read.  Repeated calls in one view read whatever pending set is current.
 *
 * From a one-batch base the pixels a call does not select keep J_p = 1: they
 * have no tracked variance.  rt_get_variance then reports a non-finite value
 * for them (NaN), rt_denoise_var takes its spatial estimate there,
 * rt_temporal_var_counted merges no within-view term, rt_get_counts and the
 * counted export report the 1, and rt_render_adaptive itself keeps refusing
 * (its base needs two batches).
 *
 * Errors: rt_render_adaptive's with one batch in place of two, and
 * RT_ERR_INVALID_ARGUMENT when min_dof is negative or NaN, or when the context
 * has no pending temporal set of the current view with moments (none, one of an
 * older view, one of another frame shape, or one that rt_temporal wrote).  A
 * refused call touches nothing. */
typedef struct rt_adaptive_reprojected_params {
    int samples;         /* these six: rt_adaptive_params' */
    float tolerance;
    float lum_floor;
    int radius;
    unsigned min_frames;
    unsigned max_frames;
    float min_dof;       /* >= 0: a hit pixel whose pending dof is below it (or NaN) is always selected */
} rt_adaptive_reprojected_params;
RT_API rt_adaptive_reprojected_params rt_adaptive_reprojected_params_default(void);
RT_API int rt_render_adaptive_reprojected(rt_context* ctx, const rt_adaptive_reprojected_params* params,
                                          int max_bounces, uint8_t* rgba_out, float* color_out,
                                          rt_adaptive_stats* stats_out);
/* As rt_render_adaptive_device: one stream, inside one render pass, ordered
 * behind the rt_temporal_var call that wrote the pending set whatever stream
 * that ran on; no host synchronisation. */
RT_API int rt_render_adaptive_reprojected_device(rt_context* ctx, const rt_adaptive_reprojected_params* params,
                                                 int max_bounces, void* rgba_device, void* stream);
/* rt_temporal_var on a non-uniform frame: a full-frame context after an adaptive
 * call, or a shard context whose current assembled frame is counted (4 or 7
 * planes; only 7 carry moments), both with rt_set_adaptive_filters on (off:
 * RT_ERR_UNSUPPORTED).  Every pixel blends and counts with its own n_p
 * (rt_temporal's count-aware colour, length and RGBA bit for bit) and brings its
 * own within-view estimate M2_p / (J_p - 1) with J_p - 1 degrees of freedom where
 * the frame carries moments and J_p >= 2, else none (csrc/rt_temporal_var.h).
 * Arguments, outputs, history sets, promotion and errors otherwise as
 * rt_temporal_var, with which and with rt_temporal it may alternate in any
 * order; on a uniform frame it is rt_temporal_var.  rt_last_temporal_var_ms
 * reports this pass too. */
RT_API int rt_temporal_var_counted(rt_context* ctx, const rt_temporal_params* params,
                                   const rt_denoise_var_params* dv, uint8_t* rgba_out, float* color_out,
                                   float* length_out, float* moments_out);
RT_API int rt_temporal_var_counted_device(rt_context* ctx, const rt_temporal_params* params,
                                          const rt_denoise_var_params* dv, void* rgba_device, void* stream);

/* ---- adaptive sampling on row shards ------------------------
 * rt_render_adaptive refuses a context that holds a row shard: the window's
 * column taps lie on other ranks.  The two-phase form lifts that.  Only the
 * row sums cross ranks: phase 1 writes a context's ROW-SUM BLOCK, the ranks
 * all-gather the blocks, phase 2 tests the context's own rows against the
 * gathered blocks and then runs every later stage of rt_render_adaptive on its
 * rows.  N shard contexts end with, interleaved, exactly the bits of one
 * context that ran rt_render_adaptive on the whole frame, on both backends.
 *
 * Block layout, the contract between ranks.  A block is 3 planes of
 * rows_per_shard * width 32-bit words: plane 0 the row sums of v (float), plane
 * 1 of M (float), plane 2 the tap counts (int32).  A plane holds the shard's
 * rows in shard order (row j = image row row_offset + j * row_stride), then
 * padding rows up to rows_per_shard: phase 1 zero-fills them, phase 2 never
 * reads them (rt_export_shard's block shape).  GATHERED is `shards` consecutive
 * blocks, block r = rows r, r + shards, ...: word k of image pixel (x, y) is
 * gathered[(((y % shards) * 3 + k) * rows_per_shard + y / shards) * width + x].
 * Every rank needs every block (an all-gather); copies must keep the bits.
 *
 * Phase 1.  The row sums of the context's own rows with params->radius into
 * block_host (3 * rows_per_shard * width words; synchronous), or into DEVICE
 * memory (4-byte aligned) on HIP stream `stream` (NULL = the context's) with
 * rt_export_shard_device's ordering and no host synchronisation.  It does not
 * change the accumulation: a continuing uniform render, rt_export_shard and
 * rt_get_counts afterwards behave as if it had not been called.  Checks and
 * errors are rt_render_adaptive's without the shard refusal, and
 * RT_ERR_INVALID_ARGUMENT for rows_per_shard below the context's rows. */
RT_API int rt_adaptive_export_rows(rt_context* ctx, const rt_adaptive_params* params, int rows_per_shard,
                                   float* block_host);
RT_API int rt_adaptive_export_rows_device(rt_context* ctx, const rt_adaptive_params* params, int rows_per_shard,
                                          void* block_device, void* stream);
/* Phase 2.  [count fill on the first call of an accumulation,] the test from
 * the gathered blocks, scan, scatter, list render, moment update, resolve; the
 * outputs are the shard's rows in shard order (rows * width), as rt_render_ex's.
 * RT_ERR_INVALID_ARGUMENT when the context's last phase 1 is not current (none
 * was made, a render, reset, scene or camera call came since, or it was made
 * with another radius), shards is not the context's row stride (1 on a
 * full-frame context, which then gives rt_render_adaptive's bits),
 * rows_per_shard * shards < height, or params or gathered is NULL.  Afterwards
 * the accumulation is non-uniform exactly as after rt_render_adaptive.  The
 * device form runs on one stream inside one render pass with
 * rt_render_adaptive_device's ordering rules and never synchronises with the
 * host; the caller orders the gather between the phases, as with
 * rt_assemble_device.  CPU context: RT_ERR_UNSUPPORTED for the device forms. */
RT_API int rt_render_adaptive_shard(rt_context* ctx, const rt_adaptive_params* params, int max_bounces,
                                    const float* gathered_host, int shards, int rows_per_shard, uint8_t* rgba_out,
                                    float* color_out, rt_adaptive_stats* stats_out);
RT_API int rt_render_adaptive_shard_device(rt_context* ctx, const rt_adaptive_params* params, int max_bounces,
                                           const void* gathered_device, int shards, int rows_per_shard,
                                           void* rgba_device, void* stream);
/* The one-process companion of rt_render_multi / rt_assemble_multi: phase 1 on
 * every context with rows on its own stream, every block copied to every
 * context's device, phase 2 on every context, the RGBA rows gathered into the
 * full image (w*h*4 bytes, row 0 = bottom, or NULL); synchronises before
 * returning.  stats_out (may be NULL): the sums of selected and frames_total
 * and the maxima of the three stage times.  The contexts must be all GPU or
 * all CPU contexts, distinct, hold shards i (mod n) of one frame and have equal
 * frame counters and equal batches; anything else is RT_ERR_INVALID_ARGUMENT
 * and nothing is touched.  Contexts beyond the image height are skipped. */
RT_API int rt_render_adaptive_multi(rt_context* const* ctxs, int n, const rt_adaptive_params* params, int max_bounces,
                                    uint8_t* rgba_out, rt_adaptive_stats* stats_out);

/* Post-render passes on a non-uniform accumulation.  Off
 * (the default) rt_denoise*, rt_denoise_var* and rt_temporal* refuse the
 * non-uniform state as described above.  On, they accept it and take every
 * pixel's own counts {n_p, J_p}:
 *  - the input colour of every pass, centre or tap, is rt_div(1, n_p) *
 *    frameSum_p, rt_render_adaptive's color_out (level 0 of rt_denoise and its
 *    iterations-0 pass, the input stage of rt_denoise_var with every tap of its
 *    7 x 7 window, rt_temporal's new colour);
 *  - rt_denoise_var chooses its variance source per pixel: the tracked variance
 *    M2_p / ((J_p - 1) n_p) (rt_get_variance's value) where J_p >= min_batches,
 *    the spatial estimate elsewhere, so one frame may mix both;
 *  - rt_temporal blends and counts with n_p: length n_p without usable history,
 *    else a = n_p / (len + n_p) and length len + n_p; the history it leaves
 *    carries per-pixel lengths.
 * With all counts equal the results are those of the uniform passes bit for
 * bit, and GPU and CPU contexts agree bit for bit.  No pass writes the
 * accumulation, the counts or the moments.  The switch has no other effect: a
 * uniform accumulation runs the same code whatever it says, and uniform renders
 * that continue a non-uniform accumulation, rt_render_multi and
 * RT_PRECISION_REFERENCE_FAST stay unsupported.  On a shard context the same
 * switch lets the passes read a counted assembled frame (rt_assemble_adaptive
 * below).  It may be changed at any time. */
RT_API int rt_set_adaptive_filters(rt_context* ctx, int enable);
RT_API int rt_get_adaptive_filters(const rt_context* ctx);

/* ---- row shards into one frame: the assembled frame ----------------------------
 *   A frame rendered as row shards by several contexts
 * (rt_render_multi, one process per rank) has the neighbours of every row on
 * another context, so rt_denoise*, rt_denoise_var* and rt_temporal* refuse a
 * shard context.  An ASSEMBLED FRAME lifts that: a full-frame snapshot
 * {frameSum, optionally the moments {M, M2}, n, J} that one context keeps,
 * de-interleaved from the ranks' gathered blocks.  While it is current, the
 * three passes on a context whose own pixel state is a row shard read it
 * instead, with its n (and, with moments, its J): bit for bit what a single
 * context that rendered the whole frame gives.  A context whose pixel state is
 * the full frame always reads its own accumulation, whatever was assembled.
 * Nothing here has a counterpart in the reference (one GPU, Main.cu:342).
 *
 * Block layout, the contract between ranks.  A context's BLOCK is `planes`
 * planes of rows_per_shard * width floats; planes = 3: R, G, B of frameSum;
 * planes = 5: the same, then M, then M2.  A plane holds the shard's rows in
 * shard order (row j = image row row_offset + j * row_stride) followed by
 * padding rows up to rows_per_shard: export zero-fills them, assembly never
 * reads them.  GATHERED is `shards` consecutive blocks, block r = rows r,
 * r + shards, ... (rt_deinterleave_rows_device's layout).  With r = y % shards
 * and j = y / shards, plane k of the assembled frameSum at pixel y * width + x
 * is gathered[((r * planes + k) * rows_per_shard + j) * width + x], and the
 * assembled moments of that pixel are {plane 3, plane 4}. */

/* Write the context's block and report the frames accumulated (frame counter -
 * 1) and the tracked batches (either may be NULL).  block: host memory,
 * planes * rows_per_shard * width floats; GPU and CPU contexts; synchronous.
 * RT_ERR_INVALID_ARGUMENT: a null pointer, planes not 3 or 5, rows_per_shard
 * below the shard's rows, no frame accumulated yet, or planes == 5 while the
 * tracked moments do not describe the accumulation (tracking off, or not live
 * up to the frame counter); RT_ERR_UNSUPPORTED: a non-uniform accumulation. */
RT_API int rt_export_shard(rt_context* ctx, int rows_per_shard, int planes, float* block,
                           unsigned* frames_out, unsigned* batches_out);
/* As above into DEVICE memory (4-byte aligned; 16 bytes per lane when width % 4
 * == 0 and the pointer is 16-byte aligned) on HIP stream `stream` (NULL = the
 * context's): ordered after the context's last render and its moment update,
 * and the context's next render after it, whatever streams they use; no host
 * synchronisation.  CPU context: RT_ERR_UNSUPPORTED. */
RT_API int rt_export_shard_device(rt_context* ctx, int rows_per_shard, int planes, void* block_device,
                                  void* stream, unsigned* frames_out, unsigned* batches_out);

/* Make the context's assembled frame for its current view from `gathered`
 * (host memory; GPU and CPU contexts; synchronous): width and height are the
 * context's, `frames` is the snapshot's n and `batches` its J (used only with
 * 5 planes).  shards == 1 is accepted (a world of one rank takes the same
 * path).  Buffers are allocated on first use.  RT_ERR_NO_SCENE;
 * RT_ERR_INVALID_ARGUMENT: a null pointer, no frame shape yet (render or
 * rt_init_rand first), planes not 3 or 5, shards < 1, rows_per_shard * shards
 * < height, frames < 1.  A refused call leaves an earlier assembled frame as
 * it was. */
RT_API int rt_assemble(rt_context* ctx, const float* gathered, int shards, int rows_per_shard, int planes,
                       unsigned frames, unsigned batches);
/* As above from DEVICE memory (4-byte aligned) on HIP stream `stream` (NULL =
 * the context's), without host synchronisation: ordered after every earlier
 * pass that reads the assembled frame (denoise, variance-guided denoise,
 * temporal), and those passes after it, whatever streams they use.  The caller
 * orders the gather between export and assembly, as with
 * rt_deinterleave_rows_device.  CPU context: RT_ERR_UNSUPPORTED. */
RT_API int rt_assemble_device(rt_context* ctx, const void* gathered_device, int shards, int rows_per_shard,
                              int planes, unsigned frames, unsigned batches, void* stream);

/* The one-process companion of rt_render_multi: every context with rows
 * exports its block on its own stream, the blocks are copied to ctxs[dst]'s
 * device, ctxs[dst] assembles them; synchronises before returning.  planes: 3,
 * 5, or 0 = 5 if every context's moments are current (with equal batches) and
 * 3 otherwise.  The contexts must be all GPU or all CPU contexts, distinct,
 * hold shards i (mod n) of one width x height, and have equal frame counters
 * (and equal batches with 5 planes); anything else is RT_ERR_INVALID_ARGUMENT
 * and nothing is touched.  Contexts beyond the image height are skipped. */
RT_API int rt_assemble_multi(rt_context* const* ctxs, int n, int planes, int dst);

/* 1 while an assembled frame is CURRENT (then *frames_out and *batches_out,
 * either may be NULL, get its n and J), else 0.  Current: one was made, and the
 * context's view, width and height are those of its assembly: rt_set_scene,
 * rt_set_camera, a moving rt_controls and a change of the frame shape end it;
 * rt_reset_accumulation and further renders do not (a snapshot with its own
 * n).  A shard context whose assembled frame is not current is refused by the
 * three passes with RT_ERR_UNSUPPORTED, as one that never assembled. */
RT_API int rt_assembled(const rt_context* ctx, unsigned* frames_out, unsigned* batches_out);
/* Host readout of the last assembled frame (tests, checkpoints): accum_rgb
 * w*h*3 floats interleaved r,g,b as rt_get_state's, moments w*h*2 floats {M,
 * M2} per pixel; either may be NULL.  RT_ERR_INVALID_ARGUMENT: none was made,
 * or moments asked of a 3-plane frame. */
RT_API int rt_get_assembled(rt_context* ctx, float* accum_rgb, float* moments);
/* Forget the assembled frame; its buffers stay allocated. */
RT_API int rt_assemble_drop(rt_context* ctx);
/* Duration (ms) of the last assembly (HIP events on its stream; wall time on
 * a CPU context); -1 when unavailable. */
RT_API float rt_last_assemble_ms(rt_context* ctx);

/* ---- counted assembled frames: adaptive frames of row shards --------------------
 *   After an adaptive call on row shards
 * (rt_render_adaptive_shard*, rt_render_adaptive_multi) the accumulation is
 * non-uniform and the calls above refuse it: their block carries one frame
 * count.  A COUNTED block carries every pixel's {n_p, J_p}, and a COUNTED
 * ASSEMBLED FRAME keeps them as a full-frame plane.  With
 * rt_set_adaptive_filters() on, the three passes on the shard context read it
 * through their count-aware forms: bit for bit what a single full-frame context
 * gives after the same rt_render_adaptive calls with the switch on.  With the
 * switch off they refuse a counted frame with RT_ERR_UNSUPPORTED.  Everything
 * above keeps its behaviour and its refusals; an uncounted assembled frame is
 * read as a uniform frame whatever the switch says and whatever state the
 * shard's own accumulation is in.
 *
 * A counted block is `planes` planes of rows_per_shard * width 32-bit words;
 * planes = 4: R, G, B of frameSum, then n_p (uint32); planes = 7: R, G, B, M,
 * M2, n_p, J_p.  Rows, padding, GATHERED and the addressing are those above
 * with this `planes`.  Every copy keeps every bit.  An assembled frame of 4
 * planes has J_p = 0 for every pixel: rt_denoise_var takes the spatial estimate
 * everywhere, whatever min_batches is.
 *
 * rt_export_shard_adaptive: as rt_export_shard, for a non-uniform accumulation
 * (the counts are the context's, rt_get_counts) and for a uniform one (every
 * pixel gets the context's {n, J}; nothing of the context is allocated or
 * written, so a continuing uniform render behaves as if it had not been
 * called).  Reports the uniform base (frame counter - 1, rt_moments_batches).
 * RT_ERR_INVALID_ARGUMENT: a null pointer, planes not 4 or 7, rows_per_shard
 * below the shard's rows, no frame accumulated yet, or planes == 7 while the
 * tracked moments do not describe the accumulation.  The device form is
 * ordered after the context's last render or adaptive call with its update and
 * resolve passes, and the next render after it; CPU context:
 * RT_ERR_UNSUPPORTED. */
RT_API int rt_export_shard_adaptive(rt_context* ctx, int rows_per_shard, int planes, float* block,
                                    unsigned* frames_out, unsigned* batches_out);
RT_API int rt_export_shard_adaptive_device(rt_context* ctx, int rows_per_shard, int planes, void* block_device,
                                           void* stream, unsigned* frames_out, unsigned* batches_out);
/* Make the context's assembled frame, with its count plane, from gathered
 * counted blocks.  `frames` and `batches` are the uniform base, which
 * rt_assembled reports and no pass reads.  Arguments (planes 4 or 7), errors,
 * currency, drop, timing and ordering are rt_assemble's and
 * rt_assemble_device's; a refused call leaves an earlier assembled frame as it
 * was.  A context has one assembled frame: rt_assemble and
 * rt_assemble_adaptive replace each other's. */
RT_API int rt_assemble_adaptive(rt_context* ctx, const float* gathered, int shards, int rows_per_shard, int planes,
                                unsigned frames, unsigned batches);
RT_API int rt_assemble_adaptive_device(rt_context* ctx, const void* gathered_device, int shards,
                                       int rows_per_shard, int planes, unsigned frames, unsigned batches,
                                       void* stream);
/* The one-process companion of rt_render_adaptive_multi: rt_assemble_multi
 * with counted blocks.  Every context may be uniform or non-uniform; the other
 * conditions are rt_assemble_multi's, all checked before anything is touched.
 * planes: 4, 7, or 0 = 7 if every context's moments are current (with equal
 * batches) and 4 otherwise. */
RT_API int rt_assemble_adaptive_multi(rt_context* const* ctxs, int n, int planes, int dst);
/* Host readout of the last assembled frame's counts, w*h uint32 each (either
 * may be NULL), as rt_get_counts'.  RT_ERR_INVALID_ARGUMENT: no assembled
 * frame, or one without counts (rt_assemble).  rt_get_assembled reads a
 * counted frame too, its moments only with 7 planes. */
RT_API int rt_get_assembled_counts(rt_context* ctx, uint32_t* frames_out, uint32_t* batches_out);

RT_API const char* rt_error_string(int status);
RT_API const char* rt_last_error(const rt_context* ctx);

#ifdef __cplusplus
}
#endif

#endif /* RT_ABI_H */
