/*
 * oracle.h — CPU restatement of the reference path tracer (TEST
 * INFRASTRUCTURE ONLY).
 *
 * Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may
 * load this library, and only as the checker / CPU baseline — never as the
 * thing measured or shipped.  The product (libbwrt.so) does not link it and
 * has no CPU fallback.
 *
 * Parity pinning, two ways:
 *  - to the reference's own source text: Main.cu and its headers compile
 *    unmodified as host C++ over this project's stand-in CUDA / GLFW headers
 *    (recipe oracle/ref/ -> oracle/_ref/libreftext.so, never committed), and
 *    tests/test_reference_text.py holds this restatement — and the product's
 *    CPU fallback — bit for bit to that library, every ORC_MUTANT rejected.
 *    Under the stand-ins' assumptions: float min / max are fminf / fmaxf, the
 *    device sin / cos / atan are orc_sinf / orc_cosf / orc_atanf below,
 *    curand_init / curand are orc_curand_init / orc_curand below;
 *  - to the reference's rendered outputs: Renders/01_red_circle.png (disc
 *    geometry) and Renders/07_specular_BRDF.png (converged image, block
 *    means), through fixtures under tests/golden/.
 * The exact cuRAND stream and the nvcc --use_fast_math transcendentals are NOT
 * pinned by either (both sides of the first comparison share this file's
 * restatement of them; statistical parity only, through the PNGs).
 */
#ifndef BWRT_ORACLE_H
#define BWRT_ORACLE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* WorldTypes.cuh / Math.cuh layouts (same bytes as include/rt_abi.h). */
typedef struct { float x, y, z; } orc_vec3;
typedef struct { orc_vec3 albedo; float emittance, roughness, refractive_index; } orc_material;
typedef struct { orc_vec3 position; float radius; orc_material mat; } orc_sphere;
typedef struct { orc_vec3 origin; orc_vec3 directions[2]; orc_material mat; } orc_plane;
typedef struct { orc_vec3 vertices[3]; orc_material mat; } orc_triangle;
typedef struct { orc_vec3 vertices[4]; orc_material mat; } orc_quad;
typedef struct { orc_vec3 position; float angle[2]; float fov; } orc_camera;
typedef struct {
    orc_camera camera;
    const orc_sphere* spheres;   int sphere_count;
    const orc_plane* planes;     int plane_count;
    const orc_triangle* triangles; int triangle_count;
    const orc_quad* quads;       int quad_count;
} orc_scene;

/* cuRAND XORWOW restated (CUDA 12.0 curand_kernel.h, external dependency,
 * not in /root/reference).  state = {d, v0, v1, v2, v3, v4}. */
void orc_curand_init(unsigned long long seed, uint32_t state[6]);
uint32_t orc_curand(uint32_t state[6]);

/* Transcendentals used on the path (Main.cu:175-182): single-precision
 * Cody-Waite + minimax approximations, specified in DESIGN.md; the product
 * kernel implements the same operation sequence. */
float orc_atanf(float x);
float orc_sinf(float x);
float orc_cosf(float x);

/* Render `passes` progressive frames (frame numbers first_frame ..
 * first_frame+passes-1) for the shard rows y = row_offset + j*row_stride,
 * j < rows.  State arrays are per shard pixel p = j*width + x:
 *   rng:   6 planes of rows*width uint32 (d, v0..v4)
 *   accum: rows*width*3 floats (frameSum, interleaved)
 *   rgba:  rows*width*4 bytes (may be NULL)
 * If init_rng != 0 the RNG is seeded first with curand_init(y*W+x,0,0).
 * threads <= 0 uses the OpenMP default.  Returns 0 or -1 on bad arguments. */
int orc_render_rows(const orc_scene* scene, int width, int height,
                    int row_offset, int row_stride, int rows,
                    unsigned first_frame, int passes, int max_bounces,
                    uint32_t* rng, float* accum, uint8_t* rgba,
                    int init_rng, int threads);

/* The first hit of the un-jittered primary ray (the camera ray of
 * Main.cu:287-290 before its jitter, no RNG draw) of every shard pixel
 * p = j*width + x, through the same camera prelude and the same closest-hit
 * loop (Main.cu:214-234) as orc_render_rows: the plain reference of the
 * product's first-hit feature buffers (rt_render_aov).  All outputs required:
 *   kind, index:  which primitive made the last accepted hit (ORC_KIND_*, its
 *                 index in its own array); ORC_KIND_MISS, -1 on a miss
 *   distance:     HitInfo.distance (INFINITY on a miss; may be inf or NaN on
 *                 a hit when the scene's scale overflows the tests)
 *   intersection, raw_normal: HitInfo.intersection / .normal, 3 floats each
 *                 (the normal is unit for a sphere, cross(d0, d1) otherwise)
 *   unit_normal:  raw_normal for a sphere, normalize(raw_normal) otherwise
 *   albedo:       the hit material's albedo; backgroundColor on a miss
 * On a miss intersection and both normals are 0.  Returns 0 or -1. */
enum { ORC_KIND_MISS = -1, ORC_KIND_SPHERE = 0, ORC_KIND_PLANE = 1, ORC_KIND_TRIANGLE = 2, ORC_KIND_QUAD = 3 };
int orc_first_hit_rows(const orc_scene* scene, int width, int height,
                       int row_offset, int row_stride, int rows,
                       int32_t* kind, int32_t* index, float* distance,
                       float* intersection, float* raw_normal, float* unit_normal,
                       float* albedo);

/* Per-step entry points: the three steps of orc_render_rows' path loop, each
 * for a batch of n independent items, through the very functions the render
 * runs (no arithmetic of their own).  A driver that advances paths level by
 * level (tests/nee_path_ref.py) composes them.  states: n x 6 words
 * {d, v0 .. v4} per item, advanced in place.  Every array is required.
 * Return 0, or -1 on bad arguments.
 *
 * orc_camera_rays: the frame's jittered, normalised camera ray of pixel
 *   (x[i], y[i]) (Main.cu:287-292: primary ray, random_direction's draws from
 *   the item's state, the jitter of the render's width, normalize).
 * orc_closest_hits: the closest hit of ray (origin, direction) by the loop of
 *   Main.cu:214-234.  kind / index as orc_first_hit_rows; distance,
 *   intersection and normal are HitInfo's (the normal trace_path shades with:
 *   unit for a sphere, the raw cross product otherwise); material: the six
 *   floats of orc_material.  A miss: kind -1, distance INFINITY, the rest 0.
 * orc_scatter: Main.cu:240-258 for a hit with this normal and material, the
 *   incoming ray's direction given: the brdfChoice draw, then the branch's own
 *   draws.  specular: choice < SPECULAR_CHANCE; scatter: the scattered
 *   direction; brdf: the vector trace_path multiplies the incoming light by. */
int orc_camera_rays(const orc_scene* scene, int width, int height, int n, const int32_t* x,
                    const int32_t* y, uint32_t* states, float* origin, float* direction);
int orc_closest_hits(const orc_scene* scene, int n, const float* origin, const float* direction,
                     int32_t* kind, int32_t* index, float* distance, float* intersection,
                     float* normal, float* material);
int orc_scatter(int n, uint32_t* states, const float* incoming, const float* normal,
                const float* material, int32_t* specular, float* scatter, float* brdf);

/* backgroundColor (Main.cu:27; {0,0,0} in the reference build) used by the
 * next orc_render_rows / orc_first_hit_rows calls. */
void orc_set_background(float r, float g, float b);

/* samplesPerPixel (Main.cu:27; 1 in the reference build): the in-frame loop
 * of Main.cu:296-299 traces that many paths from the frame's one jittered
 * camera ray, keeps the LAST (assignment, not a sum) and scales it by
 * 1/samplesPerPixel.  Used by the next orc_render_rows calls. */
void orc_set_samples_per_pixel(int n);

/* Work counters of the last orc_render_rows call (closest-hit queries and
 * paths), for the measured work profile in DESIGN.md. */
void orc_last_counters(unsigned long long* queries, unsigned long long* paths);

#ifdef __cplusplus
}
#endif

#endif
