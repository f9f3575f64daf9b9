// rt_adaptive.hip — the passes of an adaptive render call around its list
// render kernel (gfx950): count fill, selection (row sums, column sums and
// test, scan, scatter), the moment update of the listed pixels and the resolve
// pass.
//
// rt_adaptive.h has the arithmetic (shared with the CPU backend); this unit is
// built once with the exact flags (-ffp-contract=off, no RT_FAST).
//
// The list of selected pixels and its length stay on the device: the column
// pass writes one 64-bit mask word per 64 consecutive pixels of a row (wave
// ballot) with its popcount, one workgroup scans the popcounts, and the scatter
// writes pixel indices in ascending order — no atomic decides a position, so
// the list is the same every time.
//
// On a row shard the row sums go into the context's
// block for the ranks' all-gather (rt_launch_adaptive_rows_block) and the test
// reads its column taps from the gathered blocks (rt_launch_adaptive_shard);
// scan, scatter, update and resolve are the same kernels over the shard's rows.
//
// For a moving camera (rt_render_adaptive_reprojected) the
// row sums and the test have twins that read the pending planes of
// rt_temporal_var instead of the tracked moments (rt_launch_adaptive_reproj);
// everything behind the test is unchanged.
#include <hip/hip_runtime.h>

#include "rt_adaptive.h"

namespace {

__global__ void __launch_bounds__(256) rt_adaptive_fill_kernel(uint2* cnt, unsigned long long* total, long npix,
                                                               unsigned n, unsigned J) {
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p < npix) cnt[p] = make_uint2(n, J);
    if (p == 0) *total = (unsigned long long)npix * n;
}

// one lane per pixel: 2 * radius + 1 taps of {M, M2} and {n, J} (16 bytes each,
// neighbouring lanes share all but one), 12 bytes written
__global__ void __launch_bounds__(256) rt_adaptive_rows_kernel(const rt_ad_args A) {
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p >= A.npix) return;
    const int y = (int)(p / A.width);
    ad_row_sums(A, (int)(p - (long)y * A.width), y, p);
}

// one wave per mask word: lane l tests pixel (64 * word + l, row)
__global__ void __launch_bounds__(256) rt_adaptive_test_kernel(const rt_ad_args A) {
    const long wi = ((long)blockIdx.x * 256 + threadIdx.x) >> 6;
    const long nwords = (long)A.words_per_row * A.height;
    if (wi >= nwords) return;  // wave-uniform
    const int y = (int)(wi / A.words_per_row);
    const int x = (int)(wi - (long)y * A.words_per_row) * 64 + (int)(threadIdx.x & 63);
    const bool sel = x < A.width && ad_selected(A, x, y, (long)y * A.width + x);
    const unsigned long long m = __ballot(sel);
    if ((threadIdx.x & 63) == 0) {
        A.mask[wi] = m;
        A.pop[wi] = (unsigned)__popcll(m);
    }
}

// rt_adaptive_rows_kernel over the pending planes of the current view
// (rt_render_adaptive_reprojected): 2 * radius + 1 taps of {out.rgb, len} and
// {s2, dof} (24 bytes each), 12 bytes written
__global__ void __launch_bounds__(256) rt_adaptive_rows_reproj_kernel(const rt_ad_reproj_args R) {
    const rt_ad_args& A = R.A;
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p >= A.npix) return;
    const int y = (int)(p / A.width);
    ad_row_sums_reproj(R, (int)(p - (long)y * A.width), y, p);
}

// rt_adaptive_test_kernel with the `fresh` term of that selection
__global__ void __launch_bounds__(256) rt_adaptive_test_reproj_kernel(const rt_ad_reproj_args R) {
    const rt_ad_args& A = R.A;
    const long wi = ((long)blockIdx.x * 256 + threadIdx.x) >> 6;
    const long nwords = (long)A.words_per_row * A.height;
    if (wi >= nwords) return;  // wave-uniform
    const int y = (int)(wi / A.words_per_row);
    const int x = (int)(wi - (long)y * A.words_per_row) * 64 + (int)(threadIdx.x & 63);
    const bool sel = x < A.width && ad_selected_reproj(R, x, y, (long)y * A.width + x);
    const unsigned long long m = __ballot(sel);
    if ((threadIdx.x & 63) == 0) {
        A.mask[wi] = m;
        A.pop[wi] = (unsigned)__popcll(m);
    }
}

// exclusive scan of the popcounts in place, one workgroup: lane t sums the
// words t * per .. t * per + per - 1, the 1024 sums are scanned through LDS,
// then every lane writes the prefixes of its words.  Also the list length
// and the frame total behind this call.
__global__ void __launch_bounds__(1024) rt_adaptive_scan_kernel(const rt_ad_args A) {
    __shared__ unsigned wsum[16];
    const int tid = threadIdx.x;
    const long nwords = (long)A.words_per_row * A.height;
    const long per = (nwords + 1023) / 1024;
    const long i0 = (long)tid * per, i1 = i0 + per < nwords ? i0 + per : nwords;
    unsigned s = 0;
    for (long i = i0; i < i1; i++) s += A.pop[i];
    unsigned incl = s;
    for (int m = 1; m < 64; m <<= 1) {
        const unsigned u = __shfl_up(incl, m);
        if ((tid & 63) >= m) incl += u;
    }
    if ((tid & 63) == 63) wsum[tid >> 6] = incl;
    __syncthreads();
    unsigned base = 0, total = 0;
    for (int w = 0; w < 16; w++) {
        if (w < (tid >> 6)) base += wsum[w];
        total += wsum[w];
    }
    unsigned run = base + incl - s;
    for (long i = i0; i < i1; i++) {
        const unsigned v = A.pop[i];
        A.pop[i] = run;
        run += v;
    }
    if (tid == 0) {
        *A.list_n = total;
        *A.total = *A.total + (unsigned long long)total * (unsigned)A.k;
    }
}

// one wave per mask word: the set bits' pixels at the word's prefix, in lane order
__global__ void __launch_bounds__(256) rt_adaptive_scatter_kernel(const rt_ad_args A) {
    const long wi = ((long)blockIdx.x * 256 + threadIdx.x) >> 6;
    const long nwords = (long)A.words_per_row * A.height;
    if (wi >= nwords) return;
    const int lane = (int)(threadIdx.x & 63);
    const unsigned long long m = A.mask[wi];
    if (!((m >> lane) & 1ull)) return;
    const int y = (int)(wi / A.words_per_row);
    const int x = (int)(wi - (long)y * A.words_per_row) * 64 + lane;
    const unsigned below = (unsigned)__popcll(m & ((1ull << lane) - 1ull));
    A.list[A.pop[wi] + below] = (int)((long)y * A.width + x);  // a set bit has x < width: at most npix entries
}

// one lane per list item (the grid covers the worst case, npix)
__global__ void __launch_bounds__(256) rt_adaptive_update_kernel(const rt_ad_args A) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)*A.list_n) return;
    ad_update(A, (long)A.list[i]);
}

// streaming, one lane per pixel: 20 bytes read, 4 (+ 12 with colour) written
__global__ void __launch_bounds__(256) rt_adaptive_resolve_kernel(const rt_ad_args A) {
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p < A.npix) ad_resolve(A, p);
}

// rt_adaptive_test_kernel on a row shard: one wave per mask word of a shard
// row, the column taps from the ranks' gathered row sums (ad_selected_shard).
// The word index goes through readfirstlane, so the shard row, the image row
// and every tap row's block and row inside it (one division by `shards` per
// wave, then increments) are scalar: a lane adds its x and loads.
__global__ void __launch_bounds__(256) rt_adaptive_test_shard_kernel(const rt_ad_shard_args S) {
    const rt_ad_args& A = S.A;
    const long wl = ((long)blockIdx.x * 256 + threadIdx.x) >> 6;
    const long nwords = (long)A.words_per_row * A.height;
    if (wl >= nwords) return;  // wave-uniform
    const int wi = __builtin_amdgcn_readfirstlane((int)wl);  // nwords <= npix < 2^31
    const int j = wi / A.words_per_row;
    const int x = (wi - j * A.words_per_row) * 64 + (int)(threadIdx.x & 63);
    const bool sel = x < A.width && ad_selected_shard(S, x, j, (long)j * A.width + x);
    const unsigned long long m = __ballot(sel);
    if ((threadIdx.x & 63) == 0) {
        A.mask[wi] = m;
        A.pop[wi] = (unsigned)__popcll(m);
    }
}

// the padding rows of a row-sum block: words used .. plane - 1 of each of its 3 planes
__global__ void __launch_bounds__(256) rt_adaptive_pad_kernel(unsigned* block, long used, long plane) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const long pad = plane - used;
    if (i >= 3 * pad) return;
    const long k = i / pad;
    block[k * plane + used + (i - k * pad)] = 0u;
}

unsigned blocks_of(long n) { return (unsigned)((n + 255) / 256); }

}  // namespace

hipError_t rt_launch_adaptive_fill(uint2* cnt, unsigned long long* total, long npix, unsigned n, unsigned J,
                                   hipStream_t stream) {
    if (npix <= 0 || !cnt || !total) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rt_adaptive_fill_kernel, dim3(blocks_of(npix)), dim3(256), 0, stream, cnt, total, npix, n, J);
    return hipGetLastError();
}

// stage 0: row sums; 1: column sums, test, scan and scatter; 2: update; 3: resolve
hipError_t rt_launch_adaptive(const rt_ad_args& A, int stage, hipStream_t stream) {
    if (A.npix <= 0 || A.npix > 0x7fffffffl || !A.cnt) return hipErrorInvalidValue;
    const long nwords = (long)A.words_per_row * A.height;
    if (stage == 0) {
        hipLaunchKernelGGL(rt_adaptive_rows_kernel, dim3(blocks_of(A.npix)), dim3(256), 0, stream, A);
    } else if (stage == 1) {
        hipLaunchKernelGGL(rt_adaptive_test_kernel, dim3(blocks_of(nwords * 64)), dim3(256), 0, stream, A);
        hipLaunchKernelGGL(rt_adaptive_scan_kernel, dim3(1), dim3(1024), 0, stream, A);
        hipLaunchKernelGGL(rt_adaptive_scatter_kernel, dim3(blocks_of(nwords * 64)), dim3(256), 0, stream, A);
    } else if (stage == 2) {
        hipLaunchKernelGGL(rt_adaptive_update_kernel, dim3(blocks_of(A.npix)), dim3(256), 0, stream, A);
    } else {
        hipLaunchKernelGGL(rt_adaptive_resolve_kernel, dim3(blocks_of(A.npix)), dim3(256), 0, stream, A);
    }
    return hipGetLastError();
}

// stages 0 and 1 of rt_render_adaptive_reprojected
hipError_t rt_launch_adaptive_reproj(const rt_ad_reproj_args& R, hipStream_t stream) {
    const rt_ad_args& A = R.A;
    if (A.npix <= 0 || A.npix > 0x7fffffffl || !A.cnt || !R.p_col || !R.p_mom || !R.p_ga) return hipErrorInvalidValue;
    const long nwords = (long)A.words_per_row * A.height;
    hipLaunchKernelGGL(rt_adaptive_rows_reproj_kernel, dim3(blocks_of(A.npix)), dim3(256), 0, stream, R);
    hipLaunchKernelGGL(rt_adaptive_test_reproj_kernel, dim3(blocks_of(nwords * 64)), dim3(256), 0, stream, R);
    hipLaunchKernelGGL(rt_adaptive_scan_kernel, dim3(1), dim3(1024), 0, stream, A);
    hipLaunchKernelGGL(rt_adaptive_scatter_kernel, dim3(blocks_of(nwords * 64)), dim3(256), 0, stream, A);
    return hipGetLastError();
}

// The row sums of a shard's own rows (A.rowv / rowm / rowc aimed at the planes
// of its block of `plane` words each, A.height = its rows), then the block's
// padding rows
hipError_t rt_launch_adaptive_rows_block(const rt_ad_args& A, long plane, hipStream_t stream) {
    if (A.npix <= 0 || A.npix > 0x7fffffffl || !A.cnt || !A.rowv || plane < A.npix) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rt_adaptive_rows_kernel, dim3(blocks_of(A.npix)), dim3(256), 0, stream, A);
    if (plane > A.npix)
        hipLaunchKernelGGL(rt_adaptive_pad_kernel, dim3(blocks_of(3 * (plane - A.npix))), dim3(256), 0, stream,
                           reinterpret_cast<unsigned*>(A.rowv), A.npix, plane);
    return hipGetLastError();
}

// stage 1 of a shard: the sharded test, then the scan and the scatter as ever
hipError_t rt_launch_adaptive_shard(const rt_ad_shard_args& S, hipStream_t stream) {
    const rt_ad_args& A = S.A;
    if (A.npix <= 0 || A.npix > 0x7fffffffl || !A.cnt || !S.gathered || S.shards < 1 ||
        (long)S.rows_per_shard * S.shards < S.image_height || S.row_offset + (long)(A.height - 1) * S.shards >= S.image_height)
        return hipErrorInvalidValue;
    const long nwords = (long)A.words_per_row * A.height;
    hipLaunchKernelGGL(rt_adaptive_test_shard_kernel, dim3(blocks_of(nwords * 64)), dim3(256), 0, stream, S);
    hipLaunchKernelGGL(rt_adaptive_scan_kernel, dim3(1), dim3(1024), 0, stream, A);
    hipLaunchKernelGGL(rt_adaptive_scatter_kernel, dim3(blocks_of(nwords * 64)), dim3(256), 0, stream, A);
    return hipGetLastError();
}
