// rt_assemble.hip — the kernels behind rt_export_shard* and rt_assemble*
// (gfx950): a context's frameSum (and moments, and counts) into its block, and
// the ranks' gathered blocks into the assembled full frame (DESIGN.md sections
// 17, 19 and 20).  One kernel source per pass serves the four plane counts,
// instantiated per access width and for blocks with and without counts.
//
// rt_assemble.h has the indexing (shared with the CPU backend); this unit is
// built once with the exact flags, whatever precision mode the context renders
// in.  All kernels are copies with the shape of rt_deinterleave_kernel: one
// item per lane, 16 bytes per access when the width and the pointers allow it
// (VEC = 4) and 4 bytes otherwise, plain vector loads and stores, no LDS, and a
// grid-stride loop, so the launch may cap its grid (BWRT_DEINT_BLOCKS) and
// leave the CUs to a render running beside it.  Consecutive lanes write
// consecutive words; a wave reads one row segment of one block plane.
#include <hip/hip_runtime.h>

#include "rt_assemble.h"

template <int VEC, bool COUNTED>
__global__ void __launch_bounds__(256) rt_export_shard_kernel(const rt_asm_args A, long n) {
    for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < n; q += (long)gridDim.x * 256)
        asm_export_item<VEC, COUNTED>(A, q);
}

template <int VEC, bool COUNTED>
__global__ void __launch_bounds__(256) rt_assemble_kernel(const rt_asm_args A, long n) {
    for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < n; q += (long)gridDim.x * 256)
        asm_assemble_item<VEC, COUNTED>(A, q);
}

namespace {

bool args_ok(const rt_asm_args& A) {
    const bool valid = A.planes == 3 || A.planes == 5 || A.planes == 4 || A.planes == 7;
    return A.width > 0 && A.rows > 0 && A.shards > 0 && A.rows_per_shard > 0 && valid && A.sum && A.block &&
           (!rt_block_shape_of(A.planes).moments || A.mom) &&
           (long long)A.rows_per_shard * A.width <= RT_ASM_MAX_PLANE && (long long)A.rows * A.width <= RT_ASM_MAX_PLANE;
}

// 16 bytes per lane: rows of whole words and every base 16-byte aligned (then
// every plane and row of the block and of the frame is, too).  A null count
// pointer — an uncounted block, or the constants of a uniform export —
// constrains nothing.
bool takes_vec(const rt_asm_args& A) {
    uintptr_t bits = reinterpret_cast<uintptr_t>(A.sum) | reinterpret_cast<uintptr_t>(A.block) |
                     reinterpret_cast<uintptr_t>(A.cnt);
    if (rt_block_shape_of(A.planes).moments) bits |= reinterpret_cast<uintptr_t>(A.mom);
    return A.width % 4 == 0 && (bits & 15) == 0;
}

// one lane per item; max_blocks > 0 caps the grid (the loop strides over the rest)
unsigned grid_of(long n, int max_blocks) {
    long grid = (n + 255) / 256;
    if (max_blocks > 0 && grid > max_blocks) grid = max_blocks;
    if (grid > 0x7fffffffl) grid = 0x7fffffffl;
    return (unsigned)grid;
}

}  // namespace

hipError_t rt_launch_export_shard(const rt_asm_args& A, int max_blocks, hipStream_t stream) {
    if (!args_ok(A) || A.rows > A.rows_per_shard) return hipErrorInvalidValue;
    const bool vec = takes_vec(A);
    const long n = asm_items(A, A.rows_per_shard, vec ? 4 : 1);
    const bool counted = rt_block_shape_of(A.planes).counted;
    const auto kernel = vec ? (counted ? rt_export_shard_kernel<4, true> : rt_export_shard_kernel<4, false>)
                            : (counted ? rt_export_shard_kernel<1, true> : rt_export_shard_kernel<1, false>);
    hipLaunchKernelGGL(kernel, dim3(grid_of(n, max_blocks)), dim3(256), 0, stream, A, n);
    return hipGetLastError();
}

hipError_t rt_launch_assemble(const rt_asm_args& A, int max_blocks, hipStream_t stream) {
    // (rows = the frame's height: row y comes from row y / shards of a block; the
    // assembly of a counted block always writes the count plane)
    if (!args_ok(A) || (rt_block_shape_of(A.planes).counted && !A.cnt) || (long)A.rows_per_shard * A.shards < A.rows)
        return hipErrorInvalidValue;
    const bool vec = takes_vec(A);
    const long n = asm_items(A, A.rows, vec ? 4 : 1);
    const bool counted = rt_block_shape_of(A.planes).counted;
    const auto kernel = vec ? (counted ? rt_assemble_kernel<4, true> : rt_assemble_kernel<4, false>)
                            : (counted ? rt_assemble_kernel<1, true> : rt_assemble_kernel<1, false>);
    hipLaunchKernelGGL(kernel, dim3(grid_of(n, max_blocks)), dim3(256), 0, stream, A, n);
    return hipGetLastError();
}
