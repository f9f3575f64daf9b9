// rt_sky.h — the host-side sky table of a view: one bit per wave tile of the
// launch order, set when every camera ray of the tile provably misses every
// primitive (rt_sky.cpp has the argument).  The sorted kernel renders tile
// groups whose bits are all set without the path machinery (rt_kernel_sorted.h).
//
// Pure host arithmetic in double precision: no HIP, no context, no environment.
#pragma once

#include <cstdint>
#include <vector>

#include "../../include/rt_abi.h"

struct rt_kparams;
struct rt_compiled_scene;

// What the classifier needs of a compiled scene, kept on the host (the
// compiled float buffer goes to the device and is dropped)
struct rt_sky_prims {
    bool ok = false;          // every primitive has a clearing test (else: no tile is ever sky)
    double scale = 0.0;       // rt_compiled_scene::cull_omax: >= 2 x every coordinate and the camera position
    double cull_dmax = -1.0;  // rt_compiled_scene::cull_dmax
    std::vector<double> sph;   // {cx, cy, cz, R^2} as the kernel reads them
    std::vector<double> pln;   // {nx, ny, nz, d} as the kernel reads them
    // triangles and quads: {cx, cy, cz, Rc^2, nx, ny, nz, d}, the cull sphere (a
    // quad's: computed here) and the compiled plane
    std::vector<double> poly;
};

// `out` from the scene and its compiled records (r.data still held)
void rt_sky_collect(const rt_scene& s, const rt_compiled_scene& r, rt_sky_prims& out);

// Wave tiles of the launch order of K (rt_pixel.h launch_items / 64); 0
// for the linear order (tile_w <= 0)
long rt_sky_tiles(const rt_kparams& K);
// Words of a table the sorted kernel may read for K: a group's bits start at
// bit group * (BLOCK / 64), and the last group may reach past the last tile
inline size_t rt_sky_words(long tiles) { return (size_t)(tiles / 32 + 2); }

// The table of view K (camera, rot, screen_z, jitter, shard, tile shape,
// spp_inner as the kernel gets them) over the primitives P: rt_sky_words()
// words, bit t of word t / 32 for tile t.  All zero when nothing can be proven.
void rt_sky_build(const rt_kparams& K, const rt_sky_prims& P, std::vector<uint32_t>& bits);
