/*
 * device_launch_parameters.h — stand-in (TEST INFRASTRUCTURE ONLY; this
 * project's own text, see oracle/ref/README.md).
 *
 * The launch built-ins and the loop that stands for a kernel launch.  The
 * build rewrites `kernel<<<grid, block>>>(args);` into
 * `ORC_REF_LAUNCH(kernel, grid, block, args);`, which calls the kernel once
 * per thread of the grid with blockIdx / threadIdx set.
 *
 * Assumptions made here (also listed in DESIGN.md section 2):
 *  - The reference's kernels use no shared memory, barrier or atomic, and
 *    every thread touches only its own pixels' randStates / frameSum / surface
 *    texels, so the order in which the threads run cannot change a result.
 *    Blocks run in parallel under OpenMP when it is enabled.
 *  - orc_ref_block_rows can restrict a launch to some rows of blocks
 *    (blockIdx.y = begin + j * step, j < count).  A CUDA launch always runs
 *    the whole grid; by the independence above, the blocks that do run compute
 *    what they would have computed in it.  The harness uses this to render a
 *    row shard without paying for the whole frame.
 */
#ifndef ORC_REF_DEVICE_LAUNCH_PARAMETERS_H
#define ORC_REF_DEVICE_LAUNCH_PARAMETERS_H

#include "cuda_runtime.h"

inline thread_local uint3 threadIdx, blockIdx;
inline thread_local dim3 blockDim, gridDim;

struct orc_ref_block_rows_t {
    unsigned begin, step, count; /* count 0: the whole grid */
};
inline orc_ref_block_rows_t orc_ref_block_rows = {0, 1, 0};

template <class F>
inline void orc_ref_launch(dim3 grid, dim3 block, F&& thread_body) {
    const orc_ref_block_rows_t sel = orc_ref_block_rows;
    const long rows = sel.count ? (long)sel.count : (long)grid.y;
    const long nblocks = rows * (long)grid.x;
#ifdef _OPENMP
#pragma omp parallel for schedule(dynamic, 1)
#endif
    for (long b = 0; b < nblocks; b++) {
        const unsigned by = sel.count ? sel.begin + (unsigned)(b / grid.x) * sel.step : (unsigned)(b / grid.x);
        if (by >= grid.y) continue;
        gridDim = grid;
        blockDim = block;
        blockIdx = uint3{(unsigned)(b % grid.x), by, 0};
        for (unsigned ty = 0; ty < block.y; ty++)
            for (unsigned tx = 0; tx < block.x; tx++) {
                threadIdx = uint3{tx, ty, 0};
                thread_body();
            }
    }
}

#define ORC_REF_LAUNCH(kernel, grid, block, ...) orc_ref_launch((grid), (block), [&] { kernel(__VA_ARGS__); })

#endif
