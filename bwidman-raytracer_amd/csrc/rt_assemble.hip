// rt_assemble.hip — the kernels behind rt_export_shard and rt_assemble (gfx950):
// a context's frameSum (and moments) into its block, and the ranks' gathered
// blocks into the assembled full frame, and their twins
// for counted blocks, which also carry the pixels' {n_p, J_p} (section 19).
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

template <int VEC>
__global__ void __launch_bounds__(256) rt_export_shard_kernel(const rt_asm_args A, long n) {
    for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < n; q += (long)gridDim.x * 256) asm_export_item<VEC>(A, q);
}

template <int VEC>
__global__ void __launch_bounds__(256) rt_assemble_kernel(const rt_asm_args A, long n) {
    for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < n; q += (long)gridDim.x * 256) asm_assemble_item<VEC>(A, q);
}

// The same two passes over a counted block (rt_export_shard_adaptive,
// rt_assemble_adaptive): one slot more, the same shape.
template <int VEC>
__global__ void __launch_bounds__(256) rt_export_shard_adaptive_kernel(const rt_asmc_args C, long n) {
    for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < n; q += (long)gridDim.x * 256) asmc_export_item<VEC>(C, q);
}

template <int VEC>
__global__ void __launch_bounds__(256) rt_assemble_adaptive_kernel(const rt_asmc_args C, long n) {
    for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < n; q += (long)gridDim.x * 256) asmc_assemble_item<VEC>(C, q);
}

namespace {

bool args_ok(const rt_asm_args& A) {
    return A.width > 0 && A.rows > 0 && A.shards > 0 && A.rows_per_shard > 0 && (A.planes == 3 || A.planes == 5) &&
           A.sum && A.block && (A.planes == 3 || A.mom) &&
           (long long)A.rows_per_shard * A.width <= RT_ASM_MAX_PLANE && (long long)A.rows * A.width <= RT_ASM_MAX_PLANE;
}

// 16 bytes per lane: rows of whole words and every base 16-byte aligned (then
// every plane and row of the block and of the frame is, too)
bool takes_vec(const rt_asm_args& A) {
    uintptr_t bits = reinterpret_cast<uintptr_t>(A.sum) | reinterpret_cast<uintptr_t>(A.block);
    if (A.planes == 5) bits |= reinterpret_cast<uintptr_t>(A.mom);
    return A.width % 4 == 0 && (bits & 15) == 0;
}

bool counted_ok(const rt_asmc_args& C) {
    const rt_asm_args& A = C.a;
    return A.width > 0 && A.rows > 0 && A.shards > 0 && A.rows_per_shard > 0 && (A.planes == 4 || A.planes == 7) &&
           A.sum && A.block && (A.planes == 4 || A.mom) &&
           (long long)A.rows_per_shard * A.width <= RT_ASM_MAX_PLANE && (long long)A.rows * A.width <= RT_ASM_MAX_PLANE;
}

// (a null count pointer, the constants of a uniform export, constrains nothing)
bool counted_takes_vec(const rt_asmc_args& C) {
    uintptr_t bits = reinterpret_cast<uintptr_t>(C.a.sum) | reinterpret_cast<uintptr_t>(C.a.block) |
                     reinterpret_cast<uintptr_t>(C.cnt);
    if (C.a.planes == 7) bits |= reinterpret_cast<uintptr_t>(C.a.mom);
    return C.a.width % 4 == 0 && (bits & 15) == 0;
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
    if (vec)
        hipLaunchKernelGGL(rt_export_shard_kernel<4>, dim3(grid_of(n, max_blocks)), dim3(256), 0, stream, A, n);
    else
        hipLaunchKernelGGL(rt_export_shard_kernel<1>, dim3(grid_of(n, max_blocks)), dim3(256), 0, stream, A, n);
    return hipGetLastError();
}

hipError_t rt_launch_assemble(const rt_asm_args& A, int max_blocks, hipStream_t stream) {
    // (rows = the frame's height: row y comes from row y / shards of a block)
    if (!args_ok(A) || (long)A.rows_per_shard * A.shards < A.rows) return hipErrorInvalidValue;
    const bool vec = takes_vec(A);
    const long n = asm_items(A, A.rows, vec ? 4 : 1);
    if (vec)
        hipLaunchKernelGGL(rt_assemble_kernel<4>, dim3(grid_of(n, max_blocks)), dim3(256), 0, stream, A, n);
    else
        hipLaunchKernelGGL(rt_assemble_kernel<1>, dim3(grid_of(n, max_blocks)), dim3(256), 0, stream, A, n);
    return hipGetLastError();
}

hipError_t rt_launch_export_shard_adaptive(const rt_asmc_args& C, int max_blocks, hipStream_t stream) {
    if (!counted_ok(C) || C.a.rows > C.a.rows_per_shard) return hipErrorInvalidValue;
    const bool vec = counted_takes_vec(C);
    const long n = asmc_items(C, C.a.rows_per_shard, vec ? 4 : 1);
    if (vec)
        hipLaunchKernelGGL(rt_export_shard_adaptive_kernel<4>, dim3(grid_of(n, max_blocks)), dim3(256), 0, stream, C, n);
    else
        hipLaunchKernelGGL(rt_export_shard_adaptive_kernel<1>, dim3(grid_of(n, max_blocks)), dim3(256), 0, stream, C, n);
    return hipGetLastError();
}

hipError_t rt_launch_assemble_adaptive(const rt_asmc_args& C, int max_blocks, hipStream_t stream) {
    // (the assembly always writes the count plane)
    if (!counted_ok(C) || !C.cnt || (long)C.a.rows_per_shard * C.a.shards < C.a.rows) return hipErrorInvalidValue;
    const bool vec = counted_takes_vec(C);
    const long n = asmc_items(C, C.a.rows, vec ? 4 : 1);
    if (vec)
        hipLaunchKernelGGL(rt_assemble_adaptive_kernel<4>, dim3(grid_of(n, max_blocks)), dim3(256), 0, stream, C, n);
    else
        hipLaunchKernelGGL(rt_assemble_adaptive_kernel<1>, dim3(grid_of(n, max_blocks)), dim3(256), 0, stream, C, n);
    return hipGetLastError();
}
