/*
 * harness.cpp — the reference's own source text, built for the CPU (TEST
 * INFRASTRUCTURE ONLY; see oracle/ref/README.md and DESIGN.md section 2).
 *
 * This translation unit includes the generated host copy of the reference's
 * Main.cu (oracle/ref/rewrite.py: launch syntax, main's name and six
 * `constexpr`s, nothing else) over the stand-in headers of oracle/ref/include,
 * and exports C entry points that CALL the reference's functions:
 *
 *   ref_render_rows   initializeRand / render() -> launchRaytracer -> tracePath
 *                     with orc_render_rows' argument list (oracle/oracle.h)
 *   ref_controls      controls() for a key mask and a frame time
 *   ref_set_*         the five settings of Main.cu:23-28
 *
 * No arithmetic of the reference is restated here: the camera prelude is
 * render()'s own (its GL and interop calls are stubs), the pixels are written
 * by the kernel's own surf2Dwrite into this file's buffer, and the loop over
 * frames is main()'s `render(...); accumulatedFrames++`.
 */
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#ifdef _OPENMP
#include <omp.h>
#endif

#include "oracle.h"
#include "rt_abi.h"

#include ORC_REF_MAIN /* the generated copy, e.g. "../_ref/Main_host.cpp" */

/* the device-trigonometry redirection of the stand-in curand_kernel.h ends
 * with the reference's text */
#undef sin
#undef cos
#undef atan

/* ---- layout: WorldTypes.cuh / Math.cuh against the ABI and the oracle ------ */
#define SAME_SIZE(ref, abi, orc) \
    static_assert(sizeof(ref) == sizeof(abi) && sizeof(ref) == sizeof(orc), #ref ": size")
#define SAME_OFFSET(ref, rm, abi, orc, m)                                                             \
    static_assert(offsetof(ref, rm) == offsetof(abi, m) && offsetof(ref, rm) == offsetof(orc, m) &&   \
                      sizeof(ref::rm) == sizeof(abi::m) && sizeof(ref::rm) == sizeof(orc::m),         \
                  #ref "::" #rm ": offset or size")

SAME_SIZE(vec3d, rt_vec3, orc_vec3);
SAME_OFFSET(vec3d, x, rt_vec3, orc_vec3, x);
SAME_OFFSET(vec3d, y, rt_vec3, orc_vec3, y);
SAME_OFFSET(vec3d, z, rt_vec3, orc_vec3, z);
static_assert(offsetof(vec3d, r) == offsetof(vec3d, x) && offsetof(vec3d, g) == offsetof(vec3d, y) &&
                  offsetof(vec3d, b) == offsetof(vec3d, z), "color aliases vec3d");

SAME_SIZE(material, rt_material, orc_material);
SAME_OFFSET(material, albedo, rt_material, orc_material, albedo);
SAME_OFFSET(material, emittance, rt_material, orc_material, emittance);
SAME_OFFSET(material, roughness, rt_material, orc_material, roughness);
SAME_OFFSET(material, refractiveIndex, rt_material, orc_material, refractive_index);

SAME_SIZE(sphere, rt_sphere, orc_sphere);
SAME_OFFSET(sphere, position, rt_sphere, orc_sphere, position);
SAME_OFFSET(sphere, radius, rt_sphere, orc_sphere, radius);
SAME_OFFSET(sphere, mat, rt_sphere, orc_sphere, mat);

SAME_SIZE(plane, rt_plane, orc_plane);
SAME_OFFSET(plane, origin, rt_plane, orc_plane, origin);
SAME_OFFSET(plane, directions, rt_plane, orc_plane, directions);
SAME_OFFSET(plane, mat, rt_plane, orc_plane, mat);

SAME_SIZE(triangle, rt_triangle, orc_triangle);
SAME_OFFSET(triangle, vertices, rt_triangle, orc_triangle, vertices);
SAME_OFFSET(triangle, mat, rt_triangle, orc_triangle, mat);

SAME_SIZE(quad, rt_quad, orc_quad);
SAME_OFFSET(quad, vertices, rt_quad, orc_quad, vertices);
SAME_OFFSET(quad, mat, rt_quad, orc_quad, mat);

SAME_SIZE(camera, rt_camera, orc_camera);
SAME_OFFSET(camera, position, rt_camera, orc_camera, position);
SAME_OFFSET(camera, angle, rt_camera, orc_camera, angle);
SAME_OFFSET(camera, FOV, rt_camera, orc_camera, fov);

SAME_SIZE(scene, rt_scene, orc_scene);
SAME_OFFSET(scene, camera, rt_scene, orc_scene, camera);
SAME_OFFSET(scene, spheres, rt_scene, orc_scene, spheres);
SAME_OFFSET(scene, sphereCount, rt_scene, orc_scene, sphere_count);
SAME_OFFSET(scene, planes, rt_scene, orc_scene, planes);
SAME_OFFSET(scene, planeCount, rt_scene, orc_scene, plane_count);
SAME_OFFSET(scene, triangles, rt_scene, orc_scene, triangles);
SAME_OFFSET(scene, triangleCount, rt_scene, orc_scene, triangle_count);
SAME_OFFSET(scene, quads, rt_scene, orc_scene, quads);
SAME_OFFSET(scene, quadCount, rt_scene, orc_scene, quad_count);

/* the RNG state planes of orc_render_rows / rt_get_state: {d, v0..v4} */
static_assert(sizeof(curandStateXORWOW) == 6 * sizeof(uint32_t), "XORWOW state: six words");

#define REF_API extern "C" __attribute__((visibility("default")))

/* ---- the five settings (Main.cu:23-28) -------------------------------------- */
REF_API void ref_set_window(int width, int height) {
    windowWidth = width;
    windowHeight = height;
}
REF_API void ref_set_max_bounces(int n) { maxBounces = n; }
REF_API void ref_set_samples_per_pixel(int n) { samplesPerPixel = n > 0 ? n : 1; }
REF_API void ref_set_background(float r, float g, float b) { backgroundColor = color{r, g, b}; }

/* ---- render ------------------------------------------------------------------- */
/* orc_render_rows' contract (oracle/oracle.h): `passes` progressive frames,
 * frame numbers first_frame.., of the shard rows y = row_offset + j*row_stride;
 * rng as 6 planes of rows*width words, accum rows*width*3 floats, rgba
 * rows*width*4 bytes or NULL; init_rng seeds through the reference's
 * initializeRand first.  Frame size and bounce limit are set from the
 * arguments; background and samplesPerPixel are whatever ref_set_* last said.
 *
 * The reference indexes randStates / frameSum / the surface by the global
 * pixel index without a bounds check, so full-frame arrays are allocated and
 * only the shard's rows are filled in, run (orc_ref_block_rows) and read back.
 * The launch geometry is one thread per pixel, one block per image row:
 * grid (1, height), block (width, 1), cell (1, 1).
 * Not re-entrant: the settings are the reference's globals, and the screen and
 * the block-row selection are the stand-ins'; one call at a time. */
REF_API int ref_render_rows(const orc_scene* sc, int width, int height, int row_offset, int row_stride, int rows,
                            unsigned first_frame, int passes, int max_bounces, uint32_t* rng, float* accum,
                            uint8_t* rgba, int init_rng, int threads) {
    if (!sc || width <= 0 || height <= 0 || rows < 0 || row_stride <= 0 || row_offset < 0 || passes < 0 ||
        max_bounces < 0 || !rng || !accum || first_frame == 0)
        return -1;
    if (rows > 0 && (long long)row_offset + (long long)(rows - 1) * row_stride >= height) return -1;
    if ((long long)first_frame + passes > 0x7fffffffLL) return -1; /* accumulatedFrames is an int */
#ifdef _OPENMP
    if (threads > 0) omp_set_num_threads(threads);
#else
    (void)threads;
#endif
    ref_set_window(width, height);
    ref_set_max_bounces(max_bounces);

    const size_t W = (size_t)width, pixels = W * (size_t)height, shard = W * (size_t)rows;
    curandStateXORWOW* randStates = nullptr;
    color* frameSum = nullptr;
    unsigned char* screen = static_cast<unsigned char*>(std::malloc(pixels * 4));
    if (cudaMalloc(&randStates, pixels * sizeof *randStates) != cudaSuccess ||
        cudaMalloc(&frameSum, pixels * sizeof *frameSum) != cudaSuccess || !screen) {
        cudaFree(randStates);
        cudaFree(frameSum);
        std::free(screen);
        return -1;
    }
    for (int j = 0; j < rows; j++) {
        const size_t y = (size_t)row_offset + (size_t)j * row_stride;
        for (size_t x = 0; x < W; x++) {
            const size_t p = (size_t)j * W + x, q = y * W + x;
            for (int k = 0; k < 6; k++) randStates[q].s[k] = rng[(size_t)k * shard + p];
            std::memcpy(&frameSum[q], &accum[3 * p], sizeof(color));
            std::memset(screen + 4 * q, 0, 3);
            screen[4 * q + 3] = 255; /* what a call with passes == 0 reports, as the oracle */
        }
    }

    scene world;
    std::memcpy(&world, sc, sizeof world); /* same bytes: asserted above */
    const dim3 grid(1, (unsigned)height), block((unsigned)width, 1), cell(1, 1);
    orc_ref_block_rows = {(unsigned)row_offset, (unsigned)row_stride, (unsigned)rows};
    orc_ref_screen = {screen, W * 4};
    if (rows > 0) {
        if (init_rng) ORC_REF_LAUNCH(initializeRand, grid, block, randStates, cell);
        int accumulatedFrames = (int)first_frame;
        for (int f = 0; f < passes; f++) {
            render(world, grid, block, cell, randStates, accumulatedFrames, frameSum);
            accumulatedFrames++;
        }
    }
    orc_ref_block_rows = {0, 1, 0};
    orc_ref_screen = {nullptr, 0};

    for (int j = 0; j < rows; j++) {
        const size_t y = (size_t)row_offset + (size_t)j * row_stride;
        for (size_t x = 0; x < W; x++) {
            const size_t p = (size_t)j * W + x, q = y * W + x;
            for (int k = 0; k < 6; k++) rng[(size_t)k * shard + p] = randStates[q].s[k];
            std::memcpy(&accum[3 * p], &frameSum[q], sizeof(color));
            if (rgba) std::memcpy(&rgba[4 * p], screen + 4 * q, 4);
        }
    }
    cudaFree(randStates);
    cudaFree(frameSum);
    std::free(screen);
    return 0;
}

/* ---- controls ------------------------------------------------------------------ */
/* One frame of the reference's controls() (Controls.cuh) on *cam with the
 * RT_KEY_* of `keys` held down and deltaTime `dt`.  Returns rt_apply_controls'
 * flags: RT_CONTROLS_MOVED when controls() set accumulatedFrames to 1,
 * RT_CONTROLS_QUIT when it asked the window to close; -1 for a null camera. */
REF_API int ref_controls(rt_camera* cam, unsigned keys, float dt) {
    static const struct {
        unsigned bit;
        int key;
    } map[] = {{RT_KEY_W, GLFW_KEY_W},         {RT_KEY_A, GLFW_KEY_A},
               {RT_KEY_S, GLFW_KEY_S},         {RT_KEY_D, GLFW_KEY_D},
               {RT_KEY_SPACE, GLFW_KEY_SPACE}, {RT_KEY_LEFT_SHIFT, GLFW_KEY_LEFT_SHIFT},
               {RT_KEY_LEFT, GLFW_KEY_LEFT},   {RT_KEY_RIGHT, GLFW_KEY_RIGHT},
               {RT_KEY_UP, GLFW_KEY_UP},       {RT_KEY_DOWN, GLFW_KEY_DOWN},
               {RT_KEY_ESCAPE, GLFW_KEY_ESCAPE}};
    if (!cam) return -1;
    int pressed[sizeof map / sizeof map[0]], n = 0;
    for (const auto& m : map)
        if (keys & m.bit) pressed[n++] = m.key;
    GLFWwindow window = {pressed, n, GLFW_FALSE};
    camera view;
    std::memcpy(&view, cam, sizeof view);
    int accumulatedFrames = 2; /* any value but 1: controls() writes 1 on movement */
    controls(&window, view, dt, accumulatedFrames);
    std::memcpy(cam, &view, sizeof view);
    return (accumulatedFrames == 1 ? RT_CONTROLS_MOVED : 0) | (window.should_close ? RT_CONTROLS_QUIT : 0);
}
