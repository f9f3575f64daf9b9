// bwrt_render — C++ host driver over the C ABI: the reference's main loop
// (/root/reference/bwidman-raytracer/src/Main.cu:401-517) without the GLFW
// window.  Frames are rendered progressively; after each frame controls()
// (Controls.cuh:5-75) is applied with the keys a scripted timeline holds
// (--keys) and the frame's duration (or a fixed --dt); FPS / sample count
// are printed once per second like Main.cu:486-495; the final image is
// written as PNG or PPM (top row first: the buffer's row 0 is the bottom).
//
//   bwrt_render [--scene 07|01|04|04_box | --scene-file FILE] [--save-scene FILE]
//               [--width 1920] [--height 1080] [--frames 8] [--frames-per-call 1]
//               [--max-bounces 5] [--background r,g,b] [--spp 1] [--device 0] [--gpus 1]
//               [--cpu [THREADS]] [--precision exact|fast] [--keys "W*10,W+LEFT*5,*3"]
//               [--dt SECONDS] [--out image.png|image.ppm] [--dump-scene file.bin]
//               [--denoise [N]] [--sigma-color S] [--sigma-normal S] [--sigma-plane S]
//               [--temporal] [--max-history F] [--normal-cos F] [--plane-tol F]
//               [--temporal-var [N]] [--adaptive-temporal TOL] [--adaptive-rounds R]
//               [--aov PREFIX] [--moments] [--denoise-var [N]] [--sigma-lum F] [--min-batches N]
//               [--adaptive TOL] [--adaptive-after 4] [--adaptive-radius R] [--adaptive-floor F]
//               [--min-frames N] [--max-frames N]
//
// --keys: comma-separated steps KEY[+KEY...]*FRAMES (keys W A S D SPACE
// LEFT_SHIFT LEFT RIGHT UP DOWN ESCAPE; an empty key list holds nothing);
// the timeline repeats its last step.  ESCAPE ends the loop like
// glfwSetWindowShouldClose.  --gpus N renders every frame across N contexts
// (devices device..device+N-1, modulo the visible count) with rt_render_multi;
// before every --denoise, --denoise-var or --temporal call the contexts' row
// shards are assembled into one frame on context 0 (rt_assemble_multi, with the
// moments for --denoise-var), which that call then reads, and the assembly's
// duration is printed.
// --cpu renders on the library's scalar C++ CPU fallback instead (THREADS
// host threads, 0 or omitted = all; BASELINE config 1's "scalar C++ CPU
// path").  --spp sets samplesPerPixel (Main.cu:27; the in-frame loop keeps
// the last of n paths, Main.cu:296-299), and "Samples:" prints
// accumulatedFrames * samplesPerPixel like Main.cu:491.  --precision fast
// renders with the reference's fast-math trade-off (rt_set_precision: GPU
// only; the default, exact, is bit-identical to the CPU fallback).
// --light-sampling turns next-event estimation on (rt_set_light_sampling): every
// render call, the adaptive ones included, samples the emissive spheres at its
// diffuse bounces; it combines with every other flag but --precision fast.
// --light-picking uniform|weighted (rt_set_light_picking) chooses how such a
// bounce picks its light; it needs --light-sampling.
// --light-hierarchy (rt_set_light_hierarchy) lets the weighted pick descend the
// light tree instead of walking the table; it needs --light-picking weighted.
// --light-shapes spheres|all (rt_set_light_shapes) chooses whether emissive
// triangles and quads are sampled as well; it needs --light-sampling.
// --denoise [N] filters the final frame with rt_denoise (N a-trous levels,
// default rt_denoise_params_default(); the --sigma-* flags replace its
// sigmas): the file from --out is then the denoised frame.
// --temporal calls rt_temporal after every render call, before controls(): a
// view's accumulated colour is kept when the keys move the camera and is
// reprojected into the next view (--max-history, --normal-cos and --plane-tol
// replace the fields of rt_temporal_params_default()).  The file from --out is
// then the temporal frame of the last render call, filtered when --denoise is
// also given.
// --temporal-var [N] calls rt_temporal_var where --temporal calls rt_temporal:
// the reprojection also carries a per-pixel variance estimate across the camera
// moves (--max-history, --normal-cos and --plane-tol as above), and the call
// after the last render runs N variance-guided levels behind it (--sigma-lum,
// --min-batches, --sigma-normal, --sigma-plane; no N: unfiltered).  It prints
// the mean standard error over the pixels with degrees of freedom, and with
// --aov PREFIX writes PREFIX_tvar in PREFIX_var's encoding.  It cannot be
// combined with --temporal, --denoise, --denoise-var, --adaptive or --gpus
// above 1.
// --adaptive-temporal TOL [--adaptive-rounds R], only with --temporal-var [N]:
// adaptive sampling for a moving camera.  It turns the tracking and
// rt_set_adaptive_filters on; in each loop iteration, after the uniform render
// call and the unfiltered rt_temporal_var, it runs R (default 1) rounds of
// rt_render_adaptive_reprojected with the call's frame count and tolerance TOL
// (--adaptive-radius, --adaptive-floor, --min-frames, --max-frames and
// --adaptive-min-dof replace the other fields of
// rt_adaptive_reprojected_params_default()), each followed by
// rt_temporal_var_counted.  The N levels and the written image come from the
// last one of the last iteration; it prints every round's selected share.  An
// iteration in a view the keys did not leave is the rounds alone (a uniform
// render cannot continue a non-uniform accumulation).  It
// cannot be combined with --gpus above 1 or --precision fast.
// --aov PREFIX writes the first-hit feature buffers (rt_render_aov) as
// PREFIX_albedo, PREFIX_normal (n * 0.5 + 0.5) and PREFIX_depth (1 / (1 +
// depth), a miss black) images in --out's format (PNG without --out).
// --moments turns the luminance moment tracking on (rt_set_moments: one batch
// per render call, so it needs --frames-per-call below --frames) and prints
// the tracked batches and the frame's mean relative standard error; --aov
// PREFIX then also writes PREFIX_var, the standard error s = sqrt(variance of
// the pixel's mean luminance) as s / (1 + s) (one context only).
// --denoise-var [N] turns the tracking on and filters the final frame with
// rt_denoise_var (N levels; --sigma-lum, --min-batches, --sigma-normal and
// --sigma-plane replace the fields of rt_denoise_var_params_default()); it
// cannot be combined with --denoise (and so not with --temporal's filter).
// --adaptive TOL turns the tracking on and, after the first --adaptive-after
// (default 4) uniform render calls of an accumulation, makes every later call
// of the frame loop an rt_render_adaptive call with the loop's frames per call:
// only the pixels whose window (--adaptive-radius) is noisier than TOL times
// its mean luminance (plus --adaptive-floor) get the frames; --min-frames and
// --max-frames force and cap per-pixel frame counts.  It prints the mean
// frames per pixel and the last call's selected share; --aov PREFIX also
// writes PREFIX_count (n_p over the largest n_p).  It cannot be combined with
// --denoise, --denoise-var, --temporal, --precision fast or --gpus above 1
// (adaptive sampling needs the whole frame on one context).
// --adaptive-filters (rt_set_adaptive_filters) lifts that for --denoise,
// --denoise-var and --temporal: the passes then take every pixel's own frame
// count (--precision fast and --gpus above 1 stay refused).
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "image_io.hpp"
#include "rt_abi.h"
#include "scene_file.hpp"
#include "scenes.hpp"

static int die(rt_context* ctx, int rc, const char* what) {
    std::fprintf(stderr, "%s failed: %s (%s)\n", what, rt_error_string(rc), ctx ? rt_last_error(ctx) : "");
    return 1;
}

static const char* kUsage =
    "usage: bwrt_render [--scene 07|01|04|04_box | --scene-file FILE] [--save-scene FILE]\n"
    "                   [--width 1920] [--height 1080] [--frames 8] [--frames-per-call 1]\n"
    "                   [--max-bounces 5] [--background r,g,b] [--spp 1] [--device 0] [--gpus 1]\n"
    "                   [--cpu [THREADS]] [--precision exact|fast]\n"
    "                   [--light-sampling [--light-picking uniform|weighted [--light-hierarchy]]\n"
    "                    [--light-shapes spheres|all]]\n"
    "                   [--keys \"W*10,W+LEFT*5,*3\"]\n"
    "                   [--dt SECONDS] [--out image.png|image.ppm] [--dump-scene file.bin]\n"
    "                   [--denoise [N]] [--sigma-color S] [--sigma-normal S] [--sigma-plane S]\n"
    "                   [--temporal] [--max-history F] [--normal-cos F] [--plane-tol F]\n"
    "                   [--temporal-var [N]] [--adaptive-temporal TOL] [--adaptive-rounds R] [--adaptive-min-dof F]\n"
    "                   [--aov PREFIX] [--moments] [--denoise-var [N]] [--sigma-lum F] [--min-batches N]\n"
    "                   [--adaptive TOL] [--adaptive-after 4] [--adaptive-radius R] [--adaptive-floor F]\n"
    "                   [--min-frames N] [--max-frames N] [--adaptive-filters]\n"
    "  --gpus N with --denoise, --denoise-var or --temporal: the contexts' row shards are assembled\n"
    "  on context 0 (rt_assemble_multi) before each filter call; --moments (the readout) and --adaptive\n"
    "  need --gpus 1\n";

struct KeyStep {
    unsigned keys;
    int frames;
};

static bool parse_keys(const std::string& spec, std::vector<KeyStep>& steps) {
    static const struct {
        const char* name;
        unsigned bit;
    } names[] = {{"W", RT_KEY_W},         {"A", RT_KEY_A},       {"S", RT_KEY_S},
                 {"D", RT_KEY_D},         {"SPACE", RT_KEY_SPACE}, {"LEFT_SHIFT", RT_KEY_LEFT_SHIFT},
                 {"LEFT", RT_KEY_LEFT},   {"RIGHT", RT_KEY_RIGHT}, {"UP", RT_KEY_UP},
                 {"DOWN", RT_KEY_DOWN},   {"ESCAPE", RT_KEY_ESCAPE}};
    size_t pos = 0;
    while (pos <= spec.size()) {
        size_t end = spec.find(',', pos);
        if (end == std::string::npos) end = spec.size();
        std::string step = spec.substr(pos, end - pos);
        pos = end + 1;
        if (step.empty()) {
            if (end == spec.size()) break;
            continue;
        }
        int frames = 1;
        const size_t star = step.find('*');
        if (star != std::string::npos) {
            frames = std::atoi(step.c_str() + star + 1);
            step = step.substr(0, star);
            if (frames < 1) return false;
        }
        unsigned keys = 0;
        size_t k = 0;
        while (k < step.size()) {
            size_t plus = step.find('+', k);
            if (plus == std::string::npos) plus = step.size();
            const std::string name = step.substr(k, plus - k);
            bool found = false;
            for (const auto& n : names)
                if (name == n.name) {
                    keys |= n.bit;
                    found = true;
                }
            if (!found) return false;
            k = plus + 1;
        }
        steps.push_back({keys, frames});
    }
    return true;
}

int main(int argc, char** argv) {
    std::string scene_name = "07", scene_file, save, out, dump, keys_spec;
    int width = 1920, height = 1080, frames = 8, per_call = 1, max_bounces = RT_DEFAULT_MAX_BOUNCES, device = 0;
    int gpus = 1, spp = 1, cpu_threads = -1;  // -1: GPU
    int precision = RT_PRECISION_EXACT;
    bool light_sampling = false;
    int light_picking = -1;  // -1: not given
    int light_shapes = -1;
    bool light_hierarchy = false;
    float bg[3] = {0.0f, 0.0f, 0.0f};
    double fixed_dt = -1.0;
    bool denoise = false;
    rt_denoise_params dn = rt_denoise_params_default();
    bool temporal = false, temporal_var = false;
    int temporal_var_levels = 0;
    rt_temporal_params tp = rt_temporal_params_default();
    std::string aov;
    bool moments = false, moments_readout = false, denoise_var = false;
    rt_denoise_var_params dv = rt_denoise_var_params_default();
    bool adaptive = false, adaptive_filters = false;
    int adaptive_after = 4;
    rt_adaptive_params ad = rt_adaptive_params_default();
    bool adaptive_temporal = false, rounds_given = false;
    int adaptive_rounds = 1;
    rt_adaptive_reprojected_params adr = rt_adaptive_reprojected_params_default();
    bool radius_given = false, floor_given = false;
    for (int i = 1; i < argc; i++) {
        auto next = [&](void) -> const char* { return i + 1 < argc ? argv[++i] : ""; };
        if (!std::strcmp(argv[i], "--help") || !std::strcmp(argv[i], "-h")) {
            std::fputs(kUsage, stdout);
            return 0;
        } else if (!std::strcmp(argv[i], "--scene")) scene_name = next();
        else if (!std::strcmp(argv[i], "--scene-file")) scene_file = next();
        else if (!std::strcmp(argv[i], "--save-scene")) save = next();
        else if (!std::strcmp(argv[i], "--width")) width = std::atoi(next());
        else if (!std::strcmp(argv[i], "--height")) height = std::atoi(next());
        else if (!std::strcmp(argv[i], "--frames")) frames = std::atoi(next());
        else if (!std::strcmp(argv[i], "--frames-per-call")) per_call = std::atoi(next());
        else if (!std::strcmp(argv[i], "--max-bounces")) max_bounces = std::atoi(next());
        else if (!std::strcmp(argv[i], "--background")) {
            if (std::sscanf(next(), "%f,%f,%f", &bg[0], &bg[1], &bg[2]) != 3) {
                std::fprintf(stderr, "--background expects r,g,b\n");
                return 2;
            }
        } else if (!std::strcmp(argv[i], "--device")) device = std::atoi(next());
        else if (!std::strcmp(argv[i], "--gpus")) gpus = std::atoi(next());
        else if (!std::strcmp(argv[i], "--spp")) spp = std::atoi(next());
        else if (!std::strcmp(argv[i], "--cpu")) {
            cpu_threads = 0;
            if (i + 1 < argc && argv[i + 1][0] >= '0' && argv[i + 1][0] <= '9') cpu_threads = std::atoi(argv[++i]);
        }
        else if (!std::strcmp(argv[i], "--precision")) {
            const char* v = next();
            if (!std::strcmp(v, "exact")) precision = RT_PRECISION_EXACT;
            else if (!std::strcmp(v, "fast")) precision = RT_PRECISION_REFERENCE_FAST;
            else {
                std::fprintf(stderr, "unknown --precision '%s'\n%s", v, kUsage);
                return 2;
            }
        }
        else if (!std::strcmp(argv[i], "--light-sampling")) light_sampling = true;
        else if (!std::strcmp(argv[i], "--light-picking")) {
            const char* v = next();
            if (!std::strcmp(v, "uniform")) light_picking = RT_LIGHT_PICK_UNIFORM;
            else if (!std::strcmp(v, "weighted")) light_picking = RT_LIGHT_PICK_WEIGHTED;
            else {
                std::fprintf(stderr, "unknown --light-picking '%s'\n%s", v, kUsage);
                return 2;
            }
        }
        else if (!std::strcmp(argv[i], "--light-hierarchy")) light_hierarchy = true;
        else if (!std::strcmp(argv[i], "--light-shapes")) {
            const char* v = next();
            if (!std::strcmp(v, "spheres")) light_shapes = RT_LIGHT_SHAPES_SPHERES;
            else if (!std::strcmp(v, "all")) light_shapes = RT_LIGHT_SHAPES_ALL;
            else {
                std::fprintf(stderr, "unknown --light-shapes '%s'\n%s", v, kUsage);
                return 2;
            }
        }
        else if (!std::strcmp(argv[i], "--keys")) keys_spec = next();
        else if (!std::strcmp(argv[i], "--dt")) fixed_dt = std::atof(next());
        else if (!std::strcmp(argv[i], "--out")) out = next();
        else if (!std::strcmp(argv[i], "--dump-scene")) dump = next();
        else if (!std::strcmp(argv[i], "--denoise")) {
            denoise = true;
            if (i + 1 < argc && argv[i + 1][0] >= '0' && argv[i + 1][0] <= '9') dn.iterations = std::atoi(argv[++i]);
        }
        else if (!std::strcmp(argv[i], "--sigma-color")) dn.sigma_color = (float)std::atof(next());
        else if (!std::strcmp(argv[i], "--sigma-normal")) dn.sigma_normal = dv.sigma_normal = (float)std::atof(next());
        else if (!std::strcmp(argv[i], "--sigma-plane")) dn.sigma_plane = dv.sigma_plane = (float)std::atof(next());
        else if (!std::strcmp(argv[i], "--denoise-var")) {
            denoise_var = moments = true;
            if (i + 1 < argc && argv[i + 1][0] >= '0' && argv[i + 1][0] <= '9') dv.iterations = std::atoi(argv[++i]);
        }
        else if (!std::strcmp(argv[i], "--sigma-lum")) dv.sigma_lum = (float)std::atof(next());
        else if (!std::strcmp(argv[i], "--min-batches")) dv.min_batches = std::atoi(next());
        else if (!std::strcmp(argv[i], "--temporal")) temporal = true;
        else if (!std::strcmp(argv[i], "--temporal-var")) {
            temporal_var = true;
            if (i + 1 < argc && argv[i + 1][0] >= '0' && argv[i + 1][0] <= '9') temporal_var_levels = std::atoi(argv[++i]);
        }
        else if (!std::strcmp(argv[i], "--max-history")) tp.max_history = (float)std::atof(next());
        else if (!std::strcmp(argv[i], "--normal-cos")) tp.normal_cos_min = (float)std::atof(next());
        else if (!std::strcmp(argv[i], "--plane-tol")) tp.plane_tol = (float)std::atof(next());
        else if (!std::strcmp(argv[i], "--aov")) aov = next();
        else if (!std::strcmp(argv[i], "--moments")) moments = moments_readout = true;
        else if (!std::strcmp(argv[i], "--adaptive")) {
            adaptive = moments = true;
            ad.tolerance = (float)std::atof(next());
        }
        else if (!std::strcmp(argv[i], "--adaptive-filters")) adaptive_filters = true;
        else if (!std::strcmp(argv[i], "--adaptive-after")) adaptive_after = std::atoi(next());
        else if (!std::strcmp(argv[i], "--adaptive-temporal")) {
            adaptive_temporal = true;
            adr.tolerance = (float)std::atof(next());
        }
        else if (!std::strcmp(argv[i], "--adaptive-rounds")) {
            rounds_given = true;
            adaptive_rounds = std::atoi(next());
        }
        else if (!std::strcmp(argv[i], "--adaptive-min-dof")) adr.min_dof = (float)std::atof(next());
        else if (!std::strcmp(argv[i], "--adaptive-radius")) {
            ad.radius = std::atoi(next());
            radius_given = true;
        }
        else if (!std::strcmp(argv[i], "--adaptive-floor")) {
            ad.lum_floor = (float)std::atof(next());
            floor_given = true;
        }
        else if (!std::strcmp(argv[i], "--min-frames")) ad.min_frames = (unsigned)std::strtoul(next(), nullptr, 10);
        else if (!std::strcmp(argv[i], "--max-frames")) ad.max_frames = (unsigned)std::strtoul(next(), nullptr, 10);
        else {
            std::fprintf(stderr, "unknown option %s\n%s", argv[i], kUsage);
            return 2;
        }
    }
    if (light_sampling && precision == RT_PRECISION_REFERENCE_FAST) {
        std::fprintf(stderr, "--light-sampling cannot be combined with --precision fast: its estimator is exact arithmetic only\n");
        return 2;
    }
    if (light_picking >= 0 && !light_sampling) {
        std::fprintf(stderr, "--light-picking needs --light-sampling: it chooses how light sampling picks its light\n");
        return 2;
    }
    if (light_hierarchy && light_picking != RT_LIGHT_PICK_WEIGHTED) {
        std::fprintf(stderr, "--light-hierarchy needs --light-picking weighted: it is the weighted pick through a light tree\n");
        return 2;
    }
    if (light_shapes >= 0 && !light_sampling) {
        std::fprintf(stderr, "--light-shapes needs --light-sampling: it chooses which emitters light sampling samples\n");
        return 2;
    }
    if (denoise && denoise_var) {
        std::fprintf(stderr, "--denoise and --denoise-var cannot be combined: one filter writes the frame\n");
        return 2;
    }
    if (adaptive && (((denoise || denoise_var || temporal) && !adaptive_filters) ||
                     precision == RT_PRECISION_REFERENCE_FAST || gpus > 1)) {
        std::fprintf(stderr,
                     "--adaptive cannot be combined with --denoise, --denoise-var, --temporal, --precision fast or "
                     "--gpus above 1: the filters and the fast mode take one frame count for all pixels\n");
        return 2;
    }
    if ((adaptive_temporal || rounds_given) &&
        (!adaptive_temporal || !temporal_var || adaptive_rounds < 1 || gpus > 1 || precision == RT_PRECISION_REFERENCE_FAST)) {
        std::fprintf(stderr,
                     "--adaptive-temporal TOL [--adaptive-rounds R >= 1] needs --temporal-var and cannot be combined with "
                     "--gpus above 1 or --precision fast: it selects from the pending planes of rt_temporal_var on one "
                     "full frame\n");
        return 2;
    }
    if (temporal_var && (temporal || denoise || denoise_var || adaptive || gpus > 1)) {
        std::fprintf(stderr,
                     "--temporal-var cannot be combined with --temporal, --denoise, --denoise-var, --adaptive or --gpus "
                     "above 1: it is the one pass behind every render call, on one uniform full frame\n");
        return 2;
    }
    if (adaptive_temporal) {
        if (radius_given) adr.radius = ad.radius;
        if (floor_given) adr.lum_floor = ad.lum_floor;
        adr.min_frames = ad.min_frames;
        adr.max_frames = ad.max_frames;
    }
    if (adaptive && adaptive_after < 2) {
        std::fprintf(stderr, "--adaptive-after must be at least 2: the selection needs two tracked batches\n");
        return 2;
    }
    std::vector<KeyStep> steps;
    if (!keys_spec.empty()) {
        if (!parse_keys(keys_spec, steps)) {
            std::fprintf(stderr, "bad --keys '%s'\n", keys_spec.c_str());
            return 2;
        }
        per_call = 1;  // controls() runs between frames
    }
    bwrt::SceneData sd;
    if (!scene_file.empty()) {
        const std::string err = bwrt::load_scene(scene_file, sd);
        if (!err.empty()) {
            std::fprintf(stderr, "%s: %s\n", scene_file.c_str(), err.c_str());
            return 2;
        }
    } else {
        sd = scene_name == "01"       ? bwrt::scene01()
             : scene_name == "04"     ? bwrt::scene04()
             : scene_name == "04_box" ? bwrt::scene04box()
                                      : bwrt::scene07();
    }
    if (!save.empty() && !bwrt::save_scene(save, sd)) {
        std::fprintf(stderr, "cannot write %s\n", save.c_str());
        return 1;
    }
    if (!dump.empty()) {  // camera + primitive bytes (compared with bwrt.scenes by the tests)
        FILE* f = std::fopen(dump.c_str(), "wb");
        if (!f) return 1;
        std::fwrite(&sd.camera, sizeof sd.camera, 1, f);
        std::fwrite(sd.spheres.data(), sizeof(rt_sphere), sd.spheres.size(), f);
        std::fwrite(sd.planes.data(), sizeof(rt_plane), sd.planes.size(), f);
        std::fwrite(sd.triangles.data(), sizeof(rt_triangle), sd.triangles.size(), f);
        std::fwrite(sd.quads.data(), sizeof(rt_quad), sd.quads.size(), f);
        std::fclose(f);
    }
    if (!dump.empty() || (!save.empty() && frames <= 0)) return 0;

    if (gpus < 1 || cpu_threads >= 0) gpus = 1;
    if (moments_readout && gpus != 1) {
        std::fprintf(stderr, "--moments needs --gpus 1 (each GPU of a gathered frame tracks its own rows)\n");
        return 2;
    }
    const int ndev = cpu_threads >= 0 ? 1 : rt_device_count() > 0 ? rt_device_count() : 1;
    std::vector<rt_context*> ctxs(gpus, nullptr);
    int rc = 0;
    rt_scene view = sd.view();
    for (int g = 0; g < gpus; g++) {
        if (cpu_threads >= 0) {
            if ((rc = rt_create_cpu(cpu_threads, &ctxs[g]))) return die(ctxs[g], rc, "rt_create_cpu");
            std::printf("CPU fallback: %d threads\n", rt_context_threads(ctxs[g]));
        } else if ((rc = rt_create((device + g) % ndev, &ctxs[g]))) {
            return die(ctxs[g], rc, "rt_create");
        }
        if ((rc = rt_set_precision(ctxs[g], precision))) return die(ctxs[g], rc, "rt_set_precision");
        if ((rc = rt_set_light_sampling(ctxs[g], light_sampling ? 1 : 0))) return die(ctxs[g], rc, "rt_set_light_sampling");
        if (light_picking >= 0 && (rc = rt_set_light_picking(ctxs[g], light_picking))) return die(ctxs[g], rc, "rt_set_light_picking");
        if (light_hierarchy && (rc = rt_set_light_hierarchy(ctxs[g], 1))) return die(ctxs[g], rc, "rt_set_light_hierarchy");
        if (light_shapes >= 0 && (rc = rt_set_light_shapes(ctxs[g], light_shapes))) return die(ctxs[g], rc, "rt_set_light_shapes");
        if ((rc = rt_set_samples_per_pixel(ctxs[g], spp))) return die(ctxs[g], rc, "rt_set_samples_per_pixel");
        if ((rc = rt_set_scene(ctxs[g], &view))) return die(ctxs[g], rc, "rt_set_scene");
        if ((rc = rt_set_max_bounces(ctxs[g], max_bounces))) return die(ctxs[g], rc, "rt_set_max_bounces");
        if ((rc = rt_set_background(ctxs[g], bg[0], bg[1], bg[2]))) return die(ctxs[g], rc, "rt_set_background");
        if ((moments || adaptive_temporal) && (rc = rt_set_moments(ctxs[g], 1))) return die(ctxs[g], rc, "rt_set_moments");
        if ((adaptive_filters || adaptive_temporal) && (rc = rt_set_adaptive_filters(ctxs[g], 1))) return die(ctxs[g], rc, "rt_set_adaptive_filters");
    }
    rt_context* ctx = ctxs[0];
    std::vector<uint8_t> rgba((size_t)width * height * 4);
    using clk = std::chrono::steady_clock;
    double delta = 0.0;
    int frame_count = 0;
    size_t step = 0;
    int step_left = steps.empty() ? 0 : steps[0].frames;
    int calls = 0;  // render calls of the current accumulation
    rt_adaptive_stats ast{};
    bool ast_valid = false;
    std::vector<float> tvar;  // --temporal-var: {variance of the mean luminance, dof} of the last call
    // several contexts: their row shards into one frame on context 0, which the next filter call reads
    auto assemble = [&](int planes) -> int {
        if (gpus == 1) return RT_OK;
        const int arc = rt_assemble_multi(ctxs.data(), gpus, planes, 0);
        if (arc == RT_OK) std::printf("assemble: %d shards, %.3f ms\n", gpus, rt_last_assemble_ms(ctx));
        return arc;
    };
    for (int done = 0; done < frames;) {  // Main.cu:471-496
        const int n = std::min(per_call, frames - done);
        auto t0 = clk::now();
        if (rt_frame_counter(ctx) == 1u) calls = 0;  // the accumulation restarts (controls())
        // --adaptive-temporal in a view the keys did not leave: the accumulation is non-uniform and a uniform
        // render cannot continue it; the iteration is the rounds alone, over the pending set of the last one
        const bool rounds_only = adaptive_temporal && calls > 0;
        if (rounds_only) {  // (nothing is rendered before the rounds)
        } else if (adaptive && calls >= adaptive_after) {
            ad.samples = n;
            if ((rc = rt_render_adaptive(ctx, &ad, -1, rgba.data(), nullptr, &ast))) return die(ctx, rc, "rt_render_adaptive");
            ast_valid = true;
        } else {
            rc = gpus == 1 ? rt_render(ctx, width, height, n, rgba.data())
                           : rt_render_multi(ctxs.data(), gpus, width, height, n, rgba.data());
            if (rc) return die(ctx, rc, "rt_render");
            ast_valid = false;
        }
        calls++;
        done += n;
        const double frame_s = std::chrono::duration<double>(clk::now() - t0).count();
        if (temporal) {
            // before controls() restarts the accumulation.  The call after the
            // last render gives the frame that is written (filtered with --denoise)
            const bool last = done == frames || (!steps.empty() && (steps[step].keys & RT_KEY_ESCAPE));
            if ((rc = assemble(3))) return die(ctx, rc, "rt_assemble_multi");
            rc = rt_temporal(ctx, &tp, last && denoise ? &dn : nullptr, last ? rgba.data() : nullptr, nullptr, nullptr);
            if (rc) return die(ctx, rc, "rt_temporal");
            if (last) {
                std::printf("temporal: %.3f ms\n", rt_last_temporal_ms(ctx));
                if (denoise) std::printf("denoise: %d levels, %.3f ms\n", dn.iterations, rt_last_denoise_ms(ctx));
            }
        }
        if (temporal_var) {  // likewise; the levels run behind the last call only
            const bool last = done == frames || (!steps.empty() && (steps[step].keys & RT_KEY_ESCAPE));
            rt_denoise_var_params lv = dv;
            lv.iterations = temporal_var_levels;
            if (last) tvar.resize((size_t)width * height * 2);
            if (adaptive_temporal) {
                // the pending planes of this view, then the rounds: select from them, render, merge again
                if (!rounds_only && (rc = rt_temporal_var(ctx, &tp, nullptr, nullptr, nullptr, nullptr, nullptr)))
                    return die(ctx, rc, "rt_temporal_var");
                adr.samples = n;
                for (int round = 0; round < adaptive_rounds; round++) {
                    if ((rc = rt_render_adaptive_reprojected(ctx, &adr, -1, nullptr, nullptr, &ast)))
                        return die(ctx, rc, "rt_render_adaptive_reprojected");
                    std::printf("adaptive-temporal: call %d round %d selected %.1f %%, mean %.2f frames per pixel\n", calls,
                                round + 1, 100.0 * (double)ast.selected / ((double)width * height),
                                (double)ast.frames_total / ((double)width * height));
                    const bool final = last && round == adaptive_rounds - 1;
                    rc = rt_temporal_var_counted(ctx, &tp, final ? &lv : nullptr, final ? rgba.data() : nullptr, nullptr,
                                                 nullptr, final ? tvar.data() : nullptr);
                    if (rc) return die(ctx, rc, "rt_temporal_var_counted");
                }
            } else {
                rc = rt_temporal_var(ctx, &tp, last ? &lv : nullptr, last ? rgba.data() : nullptr, nullptr, nullptr,
                                     last ? tvar.data() : nullptr);
                if (rc) return die(ctx, rc, "rt_temporal_var");
            }
            if (last) {
                double se = 0.0;
                size_t known = 0;
                for (size_t i = 0; i < tvar.size(); i += 2)
                    if (tvar[i + 1] > 0.0f) {
                        se += std::sqrt((double)tvar[i]);
                        known++;
                    }
                std::printf("temporal-var: %.3f ms, mean standard error %.4g over %zu pixels with history or moments\n",
                            rt_last_temporal_var_ms(ctx), known ? se / (double)known : 0.0, known);
                if (lv.iterations > 0)
                    std::printf("denoise-var: %d levels behind the reprojection, %.3f ms\n", lv.iterations,
                                rt_last_denoise_var_ms(ctx));
            }
        }
        bool quit = false;
        if (!steps.empty()) {  // controls(window, camera, deltaTime, accumulatedFrames)
            const unsigned keys = steps[step].keys;
            if (--step_left == 0 && step + 1 < steps.size()) step_left = steps[++step].frames;
            int flags = 0;
            for (int g = 0; g < gpus; g++) {  // every context keeps the same camera / frame counter
                flags = rt_controls(ctxs[g], keys, (float)(fixed_dt >= 0 ? fixed_dt : frame_s));
                if (flags < 0) return die(ctxs[g], flags, "rt_controls");
            }
            quit = flags & RT_CONTROLS_QUIT;
        }
        delta += frame_s;
        frame_count += n;
        if (delta > 1.0 || done == frames || quit) {  // Main.cu:486-495
            // Main.cu:491 prints accumulatedFrames * samplesPerPixel after
            // accumulatedFrames++ and controls(): the next frame's index
            // (rendered frames since the last reset + 1), which is
            // rt_frame_counter() after rt_controls()
            std::printf("FPS: %d | Samples: %u | kernel %.3f ms\n", (int)(frame_count / delta),
                        rt_frame_counter(ctx) * (unsigned)spp, rt_last_kernel_ms(ctx));
            delta = 0.0;
            frame_count = 0;
        }
        if (quit) break;
    }
    if (denoise && !temporal) {
        if ((rc = assemble(3))) return die(ctx, rc, "rt_assemble_multi");
        if ((rc = rt_denoise(ctx, &dn, rgba.data(), nullptr))) return die(ctx, rc, "rt_denoise");
        std::printf("denoise: %d levels, %.3f ms\n", dn.iterations, rt_last_denoise_ms(ctx));
    }
    if (denoise_var) {
        const int batches = rt_moments_batches(ctx);
        if ((rc = assemble(0))) return die(ctx, rc, "rt_assemble_multi");
        if ((rc = rt_denoise_var(ctx, &dv, rgba.data(), nullptr, nullptr))) return die(ctx, rc, "rt_denoise_var");
        if (adaptive && ast_valid)  // non-uniform: each pixel by its own batches
            std::printf("denoise-var: %d levels, per-pixel variance source (tracked from %d batches), %.3f ms\n",
                        dv.iterations, dv.min_batches, rt_last_denoise_var_ms(ctx));
        else if (batches >= dv.min_batches)
            std::printf("denoise-var: %d levels, tracked variance of %d batches, %.3f ms\n", dv.iterations, batches,
                        rt_last_denoise_var_ms(ctx));
        else
            std::printf("denoise-var: %d levels, spatial variance (%d batches < %d), %.3f ms\n", dv.iterations,
                        batches, dv.min_batches, rt_last_denoise_var_ms(ctx));
    }
    std::vector<float> var;  // of the mean luminance, per pixel
    // (several contexts: --denoise-var tracks the moments without the readout; each holds its own rows)
    const bool moments_out = moments && gpus == 1;
    if (moments_out) {
        const int batches = rt_moments_batches(ctx);
        std::printf("moments: %d batches", batches);
        if (batches >= 2 || !aov.empty()) {
            const size_t npix = (size_t)width * height;
            std::vector<float> lum(npix);
            var.resize(npix);
            if ((rc = rt_get_variance(ctx, var.data(), lum.data()))) {
                std::printf("\n");
                return die(ctx, rc, "rt_get_variance");
            }
            double se = 0.0, mean = 0.0;
            for (size_t i = 0; i < npix; i++) {
                se += std::sqrt((double)var[i]);
                mean += lum[i];
            }
            std::printf(", mean standard error %.4g of mean luminance %.4g", se / (double)npix, mean / (double)npix);
        }
        std::printf("\n");
    }
    std::vector<uint32_t> counts;
    if (adaptive) {
        const size_t npix = (size_t)width * height;
        counts.resize(npix);
        if ((rc = rt_get_counts(ctx, counts.data(), nullptr))) return die(ctx, rc, "rt_get_counts");
        double total = 0.0;
        for (const uint32_t c : counts) total += c;
        std::printf("adaptive: mean %.2f frames per pixel, last call selected %.1f %%\n", total / (double)npix,
                    ast_valid ? 100.0 * (double)ast.selected / (double)npix : 0.0);
    }
    if (!aov.empty()) {
        const size_t npix = (size_t)width * height;
        std::vector<float> albedo(npix * 3), normal(npix * 3), depth(npix);
        rt_render_params ap{};
        ap.width = width;
        ap.height = height;
        ap.row_stride = 1;
        if ((rc = rt_render_aov(ctx, &ap, albedo.data(), normal.data(), depth.data(), nullptr)))
            return die(ctx, rc, "rt_render_aov");
        const bool ppm = out.size() > 4 && out.compare(out.size() - 4, 4, ".ppm") == 0;
        auto u8 = [](float v) { return (uint8_t)(v >= 1.0f ? 255 : v > 0.0f ? (int)(v * 255.0f + 0.5f) : 0); };
        std::vector<uint8_t> img(npix * 4);
        uint32_t cmax = 1;
        for (const uint32_t c : counts) cmax = std::max(cmax, c);
        for (int k = 0; k < (adaptive ? 5 : moments_out ? 4 : 3); k++) {
            for (size_t i = 0; i < npix; i++) {
                const float se = k == 3 ? std::sqrt(var[i]) : k == 4 ? (float)counts[i] / (float)cmax : 0.0f;
                for (int ch = 0; ch < 3; ch++)
                    img[4 * i + ch] = k == 0   ? u8(albedo[3 * i + ch])
                                      : k == 1 ? u8(normal[3 * i + ch] * 0.5f + 0.5f)
                                      : k == 2 ? u8(1.0f / (1.0f + depth[i]))
                                      : k == 3 ? u8(se / (1.0f + se))
                                               : u8(se);
                img[4 * i + 3] = 255;
            }
            const std::string name =
                aov + (k == 0 ? "_albedo" : k == 1 ? "_normal" : k == 2 ? "_depth" : k == 3 ? "_var" : "_count") + (ppm ? ".ppm" : ".png");
            if (!(ppm ? bwrt::write_ppm(name, width, height, img.data()) : bwrt::write_png(name, width, height, img.data()))) {
                std::fprintf(stderr, "cannot write %s\n", name.c_str());
                return 1;
            }
        }
    }
    if (!aov.empty() && !tvar.empty()) {  // the reprojected standard error, as PREFIX_var
        const size_t npix = (size_t)width * height;
        const bool ppm = out.size() > 4 && out.compare(out.size() - 4, 4, ".ppm") == 0;
        std::vector<uint8_t> img(npix * 4, 255);
        for (size_t i = 0; i < npix; i++) {
            const float se = std::sqrt(tvar[2 * i]), v = se / (1.0f + se);
            const uint8_t b = (uint8_t)(v >= 1.0f ? 255 : v > 0.0f ? (int)(v * 255.0f + 0.5f) : 0);
            img[4 * i] = img[4 * i + 1] = img[4 * i + 2] = b;
        }
        const std::string name = aov + "_tvar" + (ppm ? ".ppm" : ".png");
        if (!(ppm ? bwrt::write_ppm(name, width, height, img.data()) : bwrt::write_png(name, width, height, img.data()))) {
            std::fprintf(stderr, "cannot write %s\n", name.c_str());
            return 1;
        }
    }
    if (!out.empty()) {
        const bool png = out.size() > 4 && out.compare(out.size() - 4, 4, ".png") == 0;
        const bool ok = png ? bwrt::write_png(out, width, height, rgba.data())
                            : bwrt::write_ppm(out, width, height, rgba.data());
        if (!ok) {
            std::fprintf(stderr, "cannot write %s\n", out.c_str());
            return 1;
        }
    }
    rt_camera cam;
    if (!steps.empty() && rt_get_camera(ctx, &cam) == RT_OK)
        std::printf("camera %.9g %.9g %.9g %.9g %.9g\n", cam.position.x, cam.position.y, cam.position.z,
                    cam.angle[0], cam.angle[1]);
    for (rt_context* c : ctxs) rt_destroy(c);
    return 0;
}
