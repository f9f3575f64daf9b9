// rt_scene.h — the host scene compiler: an rt_scene (include/rt_abi.h) to the
// float buffer the kernels and the CPU fallback read (layout: rt_layout.h).
//
// Pure host arithmetic: no HIP, no context, no environment.  rt_set_scene
// (rt_context.cpp) fills the options from the BWRT_* tuning knobs, compiles,
// uploads, and only then replaces the context's scene.
#pragma once

#include <cstddef>
#include <string>
#include <vector>

#include "../../include/rt_abi.h"

// One field per scene knob of rt_abi.h, with the defaults of an untuned context
struct rt_scene_options {
    bool no_cull = false;     // BWRT_NO_CULL: no polygon cull spheres
    int bvh_min = 64;         // BWRT_BVH_MIN: bounded primitives from which a BVH is built
    int bvh_leaf = 8;         // BWRT_BVH_LEAF: primitives per leaf, 1..127
    float bvh_ct = 0.0f;      // BWRT_BVH_CT: SAH cost of a node step relative to a primitive test
    bool bvh_sbvh = true;     // BWRT_BVH_SBVH: spatial splits (0: object splits only)
    double bvh_refs = 2.0;    // BWRT_BVH_REFS: reference budget, x the primitives
    double bvh_alpha = 1e-5;  // BWRT_BVH_ALPHA: overlap threshold of a spatial split
    int bvh_order_mask = -1;  // BWRT_BVH_ORDER_MASK: octant bits with their own arrays (-1: from the extents)
    bool bvh_n16 = true;      // BWRT_BVH_N16: 0 hides the 16-byte nodes from the kernels
    bool bvh_stats = false;   // BWRT_BVH_STATS: one line about the tree on stderr
};

// The knobs above by name, and the parsing of one's value (false: no such knob)
extern const char* const rt_scene_option_names[10];
bool rt_scene_option_set(rt_scene_options& o, const char* name, const char* value);

struct rt_compiled_scene {
    // spheres | planes | triangles | quads | hit table | bvh nodes | leaf records | vertex-form leaves | 16-byte nodes
    std::vector<float> data;
    int n_sph = 0, n_pln = 0, n_tri = 0, n_quad = 0;
    size_t off_pln = 0, off_tri = 0, off_quad = 0, off_hit = 0;              // in floats
    size_t off_bvh = 0, off_bvh_prims = 0, off_bvh_vtx = 0, off_bvh16 = 0;  // 0 = no BVH / no 16-byte nodes
    int bvh_nodes_per_order = 0;
    int bvh_order_mask = 7;
    float cull_omax = 0.0f, cull_dmax = -1.0f;          // polygon culling bounds (rt_layout.h)
    float ovf_sc = 0.0f, ovf_nm = 0.0f, ovf_im = 0.0f;  // overflow bounds (rt_layout.h)
    // light table of next-event estimation (rt_layout.h rt_nee_args): RT_LIGHT_FLOATS per emissive sphere
    // (the first n_sphere_lights records), then per admissible emissive triangle and quad, whose sampling
    // blocks (RT_POLY_LIGHT_FLOATS each) are light_polys; not part of `data` (a buffer of its own on the
    // context: the records, then the blocks)
    std::vector<float> lights;
    std::vector<float> light_polys;
    int n_sphere_lights = 0;
    // light trees (rt_layout.h RT_LIGHT_NODE_FLOATS; rt_set_light_hierarchy): one over the sphere prefix
    // and one over the whole table, each empty where its form has fewer than 2 records (the second also
    // where the table holds no polygon record: it would be the first again)
    std::vector<float> light_tree_spheres, light_tree_all;
};

// RT_OK, or RT_ERR_UNSUPPORTED with the reason in err; `out` is written only on
// success.  The primitive arrays of `s` must match its counts (the caller checks).
int rt_compile_scene(const rt_scene& s, const rt_scene_options& opt, rt_compiled_scene& out, std::string& err);
