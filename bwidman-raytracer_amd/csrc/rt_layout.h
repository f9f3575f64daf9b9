// rt_layout.h — device-side data layout shared by the host scene compiler
// (rt_scene.cpp) and the HIP kernels (rt_kernel_*.h).
//
// The scene is "compiled" once on upload: every quantity the reference
// recomputes per ray but that depends only on the primitive (plane normal
// cross(d0,d1) Intersection.cuh:69, d = -dot(n,origin) :83, triangle/quad
// edges + normal + inner edge normals :109-127 / :142-162, r*r :38,
// ior^2/1^2 - 1 Main.cu:125) is precomputed with the SAME float operations
// in the same order, so the per-ray arithmetic stays bit-identical to the
// reference semantics while doing less work.
//
// HBM layout (all float32, records padded to 16 B):
//   spheres   : n_sph  x  4 floats  {cx, cy, cz, r*r}
//   planes    : n_pln  x  4 floats  {nx, ny, nz, d}
//   triangles : n_tri  x 28 floats  {nx,ny,nz,d, v0[3],in0[3], v1[3],in1[3], v2[3],in2[3], pad2,
//                                    cull sphere {cx,cy,cz,Rc^2}}
//   quads     : n_quad x 32 floats  {nx,ny,nz,d, v0[3],in0[3], .. v3[3],in3[3], cull {.., Rc^2 = inf}}
//   hit table : n_prim x 16 floats  {n_or_centre[3], is_sphere,
//                                    emittance*albedo[3], albedo.x,
//                                    roughness, ior^2-1, roughness^2, albedo.y,
//                                    4*albedo[3], albedo.z}
//                                   (the raw albedo for the feature buffers, in
//                                    lanes no render kernel uses)
//   primitive id = index within its kind + kind offset, kinds ordered
//   spheres, planes, triangles, quads.
//
// Per-pixel progressive state (SoA planes over the shard's pixels
// p = j*width + x, so a wave's 64 lanes touch 256 contiguous bytes):
//   rng   : 6 planes of u32 {d, v0, v1, v2, v3, v4}   (24 B/pixel)
//   accum : 3 planes of f32 {r, g, b}                 (12 B/pixel)
//   rgba  : 1 plane of u32 (bytes r,g,b,255)          ( 4 B/pixel)
#pragma once

#define RT_SPH_FLOATS 4
#define RT_PLN_FLOATS 4
#define RT_TRI_FLOATS 28
#define RT_QUAD_FLOATS 32
#define RT_TRI_CULL 24   // offset of the cull sphere in a triangle record
#define RT_QUAD_CULL 28
#define RT_POLY_EDGES 4  // offset of {v0, in0, v1, in1, ...} in a polygon record
#define RT_LEAF_FLOATS 32  // BVH leaf record: RT_KEY + the record without its cull sphere (<= 28 floats)
#define RT_LEAF_VFLOATS 16 // BVH leaf record, vertex form: RT_KEY + a sphere's {c, r^2} or a polygon's vertices
#ifndef RT_HIT_FLOATS
#define RT_HIT_FLOATS 16
#endif

#define RT_NEAR_ZERO 0.0001f       // Intersection.cuh:4
#define RT_SPECULAR_CHANCE 0.5f    // Main.cu:29
#define RT_PI 3.1415926535f        // Math.cuh:5
#define RT_MAX_LEVELS 33           // recursion records per path: RT_MAX_BOUNCES (rt_abi.h) + 1
// dwords per level per lane of the one-path-per-lane kernels' LDS record stack
// (max_bounces + 1 levels): code, k, cosAngle, and under next-event estimation
// aux (rt_light.h).  The kernels' layout and the host's LDS sizes both take it.
#define RT_LANE_REC_DWORDS(nee) ((nee) ? 4 : 3)

// diagnostic builds (-DRT_GTIMES, BWRT_GTIMES): words of the group / lane
// time buffer (rt_diag.h; rt_render.cpp allocates it)
#define RT_GTIMES_WORDS (1ull << 22)

struct rt_kparams {
    int width, height;          // full image
    int row_offset, row_stride; // shard rows y = row_offset + j*row_stride
    int rows;                   // shard rows
    int samples;                // progressive frames in this launch
    int max_bounces;
    unsigned first_frame;
    float cam_pos[3];
    float rot[9];               // rotationMatrix3DY(a0) * rotationMatrix3DX(a1), row-major
    float screen_z;             // Main.cu:336
    float jitter;               // (float)(0.001 * (width / 1000)), Main.cu:291
    float bg[3];                // backgroundColor, Main.cu:27
    int n_sph, n_pln, n_tri, n_quad, n_max;
    const float* sph;
    const float* pln;
    const float* tri;
    const float* quad;
    const float* hit;
    unsigned* rng;              // 6 planes of rows*width
    float* accum;               // 3 planes of rows*width
    unsigned* rgba;             // rows*width (may be null)
    unsigned long long* stamps; // diagnostic builds (-DRT_STAMPS) only: per-phase cycle sums
    int tile_w;                 // wave tile width in pixels (1..64, power of 2); 0 = linear order
    int tile_sq;                // waves of a 4-wave group as 2 x 2 tiles (else 4 tiles in a row)
    // bounding-volume hierarchy over spheres/triangles/quads (large scenes;
    // null = brute-force loop): 8 threaded node arrays (one per ray-direction
    // octant, bit a = d[a] < 0; bvh_order_stride floats apart).  Node: 8
    // floats {bmin.xyz, miss, bmax.xyz, leaf}, depth-first (first child =
    // node + 1, near side of the split first for that octant), miss = next node when
    // the subtree is skipped (-1 = done), leaf = -1 (internal) or
    // (count << 24) | first index into bvh_leafrec: {RT_KEY (kind = key & 3:
    // 0 sphere, 2 triangle, 3 quad; index = key >> 2), then the compiled
    // record without its cull sphere}.
    const float* bvh_nodes;
    const float* bvh_leafrec;   // leaf records in leaf order, RT_LEAF_FLOATS each
    // the same leaves in vertex form (RT_LEAF_VFLOATS each: polygons as
    // {key, v0, v1, v2[, v3]}, the kernel forms their planes and inner
    // normals with compile_polygon's own float operations: three loads in
    // one round trip instead of six in three) — the ray-refill kernel's form
    const float* bvh_leafvtx;
    int bvh_order_stride;
    int bvh_order_mask;         // octant bits with their own arrays (7 = all three axes)
    // the same arrays as 16-byte nodes (null when a box exceeds the fp16
    // range), bvh_n_nodes x 4 words per octant: {lo.x | lo.y << 16,
    // lo.z | hi.x << 16, hi.y | hi.z << 16} as fp16 rounded outward (lo down,
    // hi up: the boxes only grow) and w = the miss link of an internal node
    // (-1 = done) or ~leaf for a leaf, whose miss link is the next node
    const unsigned* bvh_nodes16;
    int bvh_n_nodes;
    // overflow bounds of the bounded primitives' tests (kernel bvh_safe):
    // largest |coordinate| of a vertex / sphere centre plus the largest
    // radius, largest |component| of a triangle / quad normal cross(e0, e1)
    // and of an inner edge normal cross(n, e_k)
    float ovf_sc, ovf_nm, ovf_im;
    // conservative polygon culling (see polygon_test): only rays whose origin
    // satisfies max|o_i| <= cull_omax and whose direction max|d_i| <=
    // cull_dmax (no polygon test can overflow) may skip a polygon's exact test
    float cull_omax;
    float cull_dmax;
    // recursion record stack in global memory (sorted kernel, deep paths and
    // full frames): levels 0 .. RT_GREC_LDS_LEVELS-1 stay in LDS, the deeper
    // ones take 3 * (max_bounces - RT_GREC_LDS_LEVELS) floats per lane of the
    // grid, [group][level - RT_GREC_LDS_LEVELS][field][lane]; null = all
    // records in LDS
    float* rec;
    int rec_stride;             // lanes in the grid (set by the launcher)
    // launch-order feedback (sorted kernel): workgroup g renders tile-group
    // group_order[g] (null = g itself; a permutation of the grid's groups,
    // valid only when order_n equals this launch's grid) and writes that
    // tile-group's duration to group_cost[]; the launcher then sorts the
    // costs so the next launch starts the most expensive tile-groups first
    // and the frame ends on cheap ones.  Null group_cost = feature off.
    int* group_order;
    unsigned* group_cost;
    long order_n;               // grid the current group_order was built for (0 = none)
    long order_cap;             // capacity of group_order / group_cost
    int order_sort;             // sort this launch's costs into group_order (else the order is kept)
    int leaf_batch;             // BVH refill kernel: leaf tests once this many lanes are ready
    int refill;                 // BVH refill kernel: new rays once this many of 64 (relative) wait
    // samplesPerPixel (Main.cu:27, 296-299): paths traced per frame from the
    // frame's one jittered camera ray; the LAST one, scaled by 1/n, is the
    // frame's sample.  1 (the reference build) everywhere but the simple
    // kernel and the CPU fallback, which the launch policy picks for n > 1
    int spp_inner;
    // sky table (rt_sky.h; sorted kernel): bit t of word t / 32 set when every
    // camera ray of wave tile t of the launch order provably misses; a group
    // whose tiles are all sky skips the round loop.  Null = feature off.
    const unsigned* sky;
};

// leaf-batch thresholds of the launch policy (full frames / small shards)
#ifndef RT_LEAF_BATCH
#define RT_LEAF_BATCH 60
#endif
#ifndef RT_LEAF_BATCH_SMALL
#define RT_LEAF_BATCH_SMALL 62
#endif
// (refill 40 on full frames since the round-5 node-step trimming: config 5
// 80.8 -> 80.1 ms over five alternating pairs; small shards flat between 28
// and 36, profiles/r05h/ab_refill5.txt)
#ifndef RT_REFILL
#define RT_REFILL 40
#endif
// (small shards: 32 since the round-5 leaf-load change, config 5's 1/8
// shard 17.86 -> 17.64 ms over two alternating pairs and ahead in the
// earlier sweep too, profiles/r05h/ab_refill5.txt, ab_knobs6.txt)
#ifndef RT_REFILL_SMALL
#define RT_REFILL_SMALL 32
#endif

// Interleaved test order of Main.cu:221-234 (sphere i, plane i, triangle i,
// quad i, then i+1): a primitive's key; among equal distances the reference
// keeps the LAST tested primitive, i.e. the largest key.
#define RT_KEY(kind, i) ((i) * 4 + (kind))

// The frame of one a-trous pass over a full width x height image: what the two
// filters (rt_denoise.h, rt_denoise_var.h) share and the common code
// (rt_atrous.h, rt_atrous_tile.h) takes (float4: every includer has
// <hip/hip_runtime.h> first).
struct rt_at_frame {
    int width, height;
    int step;            // level: 1 << level
    int last;            // also write tone_map(c, 1) to rgba (when non-null)
    float in, ip;        // 1 / sigma^2 of the normal and plane terms
    float inv;           // rt_div(1, n), n = frame counter - 1
    const float* accum;  // frameSum, 3 planes of width * height
    const float4* src;   // colour of the previous level or stage
    float4* dst;         // colour of this one
    unsigned* rgba;
    const float4* ga;    // guides {n.xyz, prim as bits}
    const float4* gb;    //        {P.xyz, depth}
};

// The argument structs of the post-render passes come in two parts.  The
// `_uniform` base is what the kernels of a uniform accumulation take (by value,
// with the tile count behind it: their kernel arguments keep their offsets).
// The full struct appends the per-pixel counts {n_p, J_p} of the non-uniform
// state (rt_render_adaptive), which only the count-aware kernels take; null =
// uniform.

// One level of the denoiser (rt_denoise.h): dst holds {r, g, b, 0}.
struct rt_dn_uniform {
    rt_at_frame f;
    int first;           // colour in = inv * frameSum (tone_map's first step), else src
    float ic;            // 1 / sigma^2 of the colour term (this level's)
};
struct rt_dn_level : rt_dn_uniform {
    const uint2* cnt;    // `first` reads rt_div(1, n_q) * frameSum_q
};

// One temporal reprojection pass (rt_temporal.h) over a full width x height
// frame: the current view's frameSum and guides, the history view's colour,
// guides and camera, and the pending buffers of the current view.
struct rt_tp_uniform {
    int width, height;
    int has_history;     // 0: every pixel takes the no-history path (h_* are not read)
    float n;             // (float)(frame counter - 1)
    float inv;           // 1 / n, formed as rt_dn_level::inv
    float max_history, normal_cos_min, plane_tol;
    float h_cam[3];      // the history view's rt_kparams::cam_pos, rot, screen_z
    float h_rot[9];
    float h_screen_z;
    const float* accum;  // frameSum, 3 planes of width * height
    const float4* ga;    // current guides {n.xyz, prim as bits}
    const float4* gb;    //                {P.xyz, depth}
    const float4* h_col; // history {r, g, b, len}
    const float4* h_ga;
    const float4* h_gb;
    float4* p_col;       // pending {out.rgb, len_out}
    float4* p_ga;        // pending copy of the current guides
    float4* p_gb;
    unsigned* rgba;      // tone_map(out, 1) when non-null
};
struct rt_tp_args : rt_tp_uniform {
    const uint2* cnt;    // (float)n_p and rt_div(1, (float)n_p) replace n and inv
};

// One luminance-moment update (rt_moments.h) over the npix pixels of the
// context's shard: the batch of k frames first .. first + k - 1 that a render
// call just added to frameSum.
struct rt_mom_args {
    long npix;
    int first;           // the batch starts the accumulation (frame 1): prev, M, M2 count as 0 and are not read
    float kf;            // (float)k
    float invk;          // 1.0f / kf
    float kw;            // kf / (float)(n0 + k), n0 = frames accumulated before the batch
    const float* accum;  // frameSum after the batch, 3 planes of npix
    float* prev;         // frameSum before the batch, same layout; becomes frameSum
    float2* mom;         // {M, M2}: weighted mean of the batch luminances and sum of k_j (l_j - mean)^2
};

// One export or assembly pass (rt_assemble.h; rt_export_shard*, rt_assemble*;
// DESIGN.md sections 17, 19 and 20).  A context's BLOCK is `planes` planes of
// rows_per_shard * width 4-byte words:
//
//   planes   0  1  2   3    4    5    6     moments   counts
//     3      R  G  B                          no        no
//     5      R  G  B   M    M2                yes       no
//     4      R  G  B   n_p                    no        yes
//     7      R  G  B   M    M2   n_p  J_p     yes       yes
//
// R, G, B (the context's frameSum) and M, M2 (its tracked moments) are float
// words, n_p and J_p (the pixels' counts) uint32 words; rt_block_shape derives
// the two columns on the right from `planes`.  A plane holds the shard's rows in
// shard order (row j is image row row_offset + j * row_stride), then padding
// rows up to rows_per_shard, which export zero-fills and assembly never reads.
// GATHERED is `shards` consecutive blocks, block r = rows r, r + shards, ...
// (the layout of rt_deinterleave_rows_device and bwrt.dist.gather_rows).  The
// assembled frame has the context's full-frame layouts: with r = y % shards,
// j = y / shards and
//   word(k) = gathered[((r * planes + k) * rows_per_shard + j) * width + x],
//   sum[k * width * height + y * width + x] = word(k)                  k < 3
//   mom[y * width + x] = {word(3), word(4)}                            moments
//   cnt[y * width + x] = {word(first count plane), word(the next) or 0 without moments}
struct rt_block_shape {
    bool moments, counted;
    int slots;           // items per pixel group of a pass: one per colour plane, one for {M, M2}, one for the counts
    int count_plane;     // the first count plane
};
#ifdef __HIPCC__
__host__ __device__
#endif
inline rt_block_shape rt_block_shape_of(int planes) {
    const bool moments = planes == 5 || planes == 7, counted = planes == 4 || planes == 7;
    return {moments, counted, 3 + (int)moments + (int)counted, moments ? 5 : 3};
}
struct rt_asm_args {
    // (the count fields first: what the passes of an uncounted block read then
    // lies in one run that ends at the kernel's last argument, and its scalar
    // loads are grouped as before the fields came)
    uint2* cnt;          // counted blocks, {n_p, J_p} per pixel: assembly writes it; export reads it, or, when null,
    unsigned n, j;       // writes these two constants for every pixel of the shard (a uniform accumulation)
    int width;
    int rows;            // export: the shard's rows; assembly: the frame's height
    int shards;          // assembly: blocks in `gathered` (export: 1)
    int rows_per_shard;  // rows of one block plane (>= the shard's rows; shards * it >= height)
    int planes;          // 3, 5, 4 or 7
    float* sum;          // frameSum, 3 planes of rows * width: export reads it, assembly writes it
    float2* mom;         // {M, M2} per pixel, likewise; only with moments
    float* block;        // export writes the block; assembly reads `gathered` here
};

// One pass of the variance-guided filter (rt_denoise_var.h): the input stage
// (reads accum, writes dst), a sigma pass (reads src) or a level; src and dst
// hold {colour, variance}.
struct rt_dv_uniform {
    rt_at_frame f;
    int tracked;         // input stage: v0 from the tracked moments, else the spatial estimate
    float rd;            // tracked: 1 / ((J - 1) n)
    float sigma_lum;     // sigma pass
    const float2* mom;   // input stage, tracked: {M, M2}
    float* rs;           // reciprocal luminance sigma: the sigma pass writes it, the level reads its centre
};
struct rt_dv_args : rt_dv_uniform {
    // input stage (`tracked` and rd are not read): pixel p is tracked when
    // J_p >= min_batches, and every tap's colour takes its own count
    unsigned min_batches;
    const uint2* cnt;
};

// One reprojection pass that carries the luminance moments (rt_temporal_var.h):
// rt_temporal's pass over a uniform accumulation, and one {s2, dof} plane beside
// each colour + length plane.
struct rt_tv_args {
    rt_tp_uniform t;
    int tracked;         // the frame's tracked moments are current with J >= 2 batches: mom is read
    float dof_c;         // tracked: (float)(J - 1), else 0
    const float2* mom;   // tracked: {M, M2} of the current frame
    const float2* h_mom; // history {s2, dof}; null: the set was written by rt_temporal and has none
    float2* p_mom;       // pending {s2_out, dof_out}
};

// The same pass over a non-uniform frame (rt_temporal_var_counted): the counts
// behind the uniform struct, whose kernel takes rt_tv_args alone and keeps its
// argument offsets.  `tracked` then says that the frame carries moments at all
// (the choice J_p >= 2 is per pixel) and dof_c is not read.
struct rt_tv_cnt_args : rt_tv_args {
    const uint2* cnt;    // {n_p, J_p}
};

// The input stage of the variance-guided levels behind that pass: f.dst takes
// {out.xyz, v0} (f.ga, f.gb, f.in, f.ip: the spatial estimate's window)
struct rt_tv_input {
    rt_at_frame f;
    float dof_min;       // (float)min_batches - 1.5f: at or above it v0 = s2 / len, below the spatial estimate
    const float4* col;   // pending {out.rgb, len_out}
    const float2* mom;   // pending {s2_out, dof_out}
};

// The list of an adaptive render (rt_adaptive.h): what the list render kernels
// (rt_kernel_list.h) take besides rt_kparams, whose layout they leave alone.
struct rt_list_args {
    const int* list;         // selected shard pixel indices, ascending
    const unsigned* list_n;  // their number (stays on the device)
    const uint2* cnt;        // {n_p, J_p} per pixel: item i starts at frame n_p + 1
};

// The light table of next-event estimation (rt_light.h; rt_set_light_sampling):
// what the NEE render kernel (rt_kernel_nee.h) and its CPU twin take besides
// rt_kparams, whose layout they leave alone.  One record of RT_LIGHT_FLOATS per
// sphere with finite emittance > 0 and finite radius > 0, in sphere order:
//   {cx, cy, cz, r*r, emitted.r, emitted.g, emitted.b, primitive id as int bits}
// (emitted = the hit table's emittance * albedo, the same floats).
#define RT_LIGHT_FLOATS 8
// pick modes of nee_sample (rt_light.h; include/rt_abi.h RT_LIGHT_PICK_*)
#define RT_PICK_UNIFORM 0
#define RT_PICK_WEIGHTED 1
#define RT_PICK_TREE 2  // internal: weighted picking through the light tree (rt_set_light_hierarchy)
// shape modes of nee_sample (rt_light.h; include/rt_abi.h RT_LIGHT_SHAPES_*)
#define RT_SHAPES_SPHERES 0
#define RT_SHAPES_ALL 1
// Polygon lights (rt_set_light_shapes, RT_LIGHT_SHAPES_ALL; DESIGN.md section
// 25).  The sphere records come first and stay as above; behind them one record
// per admissible emissive triangle and then per admissible emissive quad
// (rt_scene.cpp has the rules), in primitive-id order, so the ids of the whole
// table ascend:
//   {bounding-sphere centre, R*R, emitted.r, emitted.g, emitted.b, primitive id}
// What the sampler needs besides lies in `poly`, RT_POLY_LIGHT_FLOATS per
// polygon record (record n_sphere_lights + i takes block i):
//   {v0.xyz, A0,  v1.xyz, A1,  v2.xyz, |n|,  v3'.xyz, 0,  n.xyz, 0}
// v3' = the quad's fourth vertex projected along n into the plane through v0
// (a triangle: v2 again), A0 and A1 the areas of the halves (v0, v1, v2) and
// (v0, v2, v3') (a triangle: A1 = 0), n the hit table's normal floats and |n|
// its float length.
#define RT_POLY_LIGHT_FLOATS 20
// The light tree (rt_set_light_hierarchy; rt_light.h has the descent, DESIGN.md
// section 29; rt_scene.cpp builds it): a binary tree over a table of n >= 2
// records, 2n - 1 nodes of RT_LIGHT_NODE_FLOATS floats.  Nodes [0, n - 1) are
// internal, the root first and every parent in front of its children; node
// n - 1 + j is the leaf of table record j.  So a child reference k is a leaf
// iff k >= n - 1, and the descent reads a leaf's light record, never its node.
//   {cx, cy, cz, R*R, phi, a, b, parent}       a, b, parent: int32 bits
// {c, R*R}: a leaf's is its record's; an internal node's is a sphere that
// contains both children's, rounded outwards so that
// sqrt(R*R) >= |c - c_child| + sqrt(R*R_child) holds in exact arithmetic on the
// stored floats.  phi: a leaf's is pw r*r (sphere light) or (pw area) / pi
// (polygon light, area = A0 + A1 of its sampling block), pw = |e.x| + |e.y| +
// |e.z|; an internal node's is phi(a) + phi(b), one float addition.  a, b: an
// internal node's left and right child; a leaf's are {j, -1}.  parent: -1 for
// the root.  A record whose centre, R*R or phi is not finite is a leaf with
// phi = 0 that the bounds above it leave out.  With a centre or R*R that is not
// finite no pick mode gives it a weight; a phi that overflows (emission near
// 1e30) can belong to a light the table walk still weighs, and the tree then
// reaches it only through siblings that have power: such inputs are outside
// what the hierarchy supports.
#define RT_LIGHT_NODE_FLOATS 8
struct rt_nee_args {
    const float* lights;
    int n_lights;            // 0: the estimator is the default one, bit for bit
    int pick;                // rt_set_light_picking (RT_LIGHT_PICK_*), for the host: the launcher picks the
                             // instantiation and the CPU twin its path by it; no kernel reads it (the
                             // struct's tail padding before: size and the fields in front unchanged)
    const float* poly;       // polygon lights' sampling data; read only where n_lights > n_sphere_lights
    int n_sphere_lights;     // records [0, n_sphere_lights) are spheres, [n_sphere_lights, n_lights) polygons; the
                             // launcher and the CPU twin take the polygon-aware form iff the latter is not empty
    const float* tree;       // the light tree over records [0, n_lights) (above); read only where pick is
                             // RT_PICK_TREE, which the host sets only with n_lights >= 2 (behind the existing
                             // fields: none of them moves)
};

// One adaptive call (rt_adaptive.h) over the full width x height frame of a
// context in the non-uniform state: the selection passes, the moment update of
// the listed pixels and the resolve pass share it.
struct rt_ad_args {
    int width, height;
    long npix;
    int words_per_row;       // 64-pixel mask words per row
    int k;                   // frames added to every selected pixel
    int radius;
    float tolerance, lum_floor;
    unsigned min_frames, max_frames;
    float kf, invk;          // (float)k, 1.0f / kf
    const float2* mom_in;    // {M, M2} (selection)
    float2* mom;             // (update)
    uint2* cnt;              // {n_p, J_p}
    float* accum;            // frameSum, 3 planes
    float* prev;             // frameSum before the pixel's last tracked batch
    float* rowv;             // row sums of the window: variance, luminance, taps
    float* rowm;
    int* rowc;
    unsigned long long* mask;  // one word per 64 consecutive pixels of a row
    unsigned* pop;           // its popcount, then (scan) the exclusive prefix
    int* list;
    unsigned* list_n;
    unsigned long long* total;  // sum of n_p over the frame
    unsigned* rgba;          // resolve: tone_map(frameSum, n_p) (may be null)
    float* color;            // resolve: rt_div(1, n_p) * frameSum, interleaved r,g,b (may be null)
};

// The selection of rt_render_adaptive_reprojected (rt_adaptive.h, ad_row_sums_reproj
// and ad_selected_reproj): the window's variance and luminance come from the
// pending planes of the context's current view (rt_temporal_var), which are only
// read.  The existing kernels take rt_ad_args alone: its layout stays as it is.
struct rt_ad_reproj_args {
    rt_ad_args A;            // (mom_in is not read by the selection)
    const float4* p_col;     // pending {out.rgb, len}
    const float2* p_mom;     // pending {s2, dof}
    const float4* p_ga;      // pending guide copy: .w = prim as bits
    float min_dof;           // a hit pixel with !(dof >= min_dof) is always selected
};

// The selection of an adaptive call on a row shard (rt_adaptive.h,
// ad_selected_shard): A describes the shard (height = its rows, npix = rows *
// width; rowv / rowm / rowc unused), the column taps come from the ranks'
// gathered row-sum blocks.  A block is 3 planes of rows_per_shard * width
// 32-bit words (sum v float, sum M float, tap count int32), the shard's rows in
// shard order, then zero padding rows; `gathered` is `shards` blocks, so word k
// of image pixel (x, y) is
//   gathered[(((y % shards) * 3 + k) * rows_per_shard + y / shards) * width + x].
// The existing kernels take rt_ad_args alone: its layout stays as it is.
struct rt_ad_shard_args {
    rt_ad_args A;
    const float* gathered;
    int shards, rows_per_shard;
    int image_height;        // of the whole frame: the window clips there
    int row_offset;          // shard row j is image row row_offset + j * shards
};
