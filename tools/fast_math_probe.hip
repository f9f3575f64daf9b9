// Per-site probe of bwidman-raytracer_amd/csrc/rt_path.h's arithmetic
// primitives (tests/test_gpu_fast_math.py): evaluates one function of the
// header for each float32 tuple of a file, one tuple per lane, and writes the
// result bits.
//
//   mathprobe <function id> <in.bin> <out.bin> [host_out.bin]
//
// in.bin: raw float32 tuples of the function's arity; out.bin: the function's
// uint32 result words per tuple, computed by the device pass.  With a fourth
// argument the host pass of the same header evaluates the same tuples into
// host_out.bin (functions that exist on the host).
//
//   id  function                 in  out
//    0  rt_sqrt(x)                1   1
//    1  rt_rcp(x)                 1   1
//    2  rt_inv_len(x)             1   1
//    3  rt_div(x, y)              2   1
//    4  rt_div_spec_chance(x)     1   1
//    5  rt_sincos(x) -> s, c      1   2
//    6  atan_nn(x)                1   1
//    7  tone_map(ax, ay, az, n)   4   1   (n: the uint32 in the fourth word)
//    8  __builtin_amdgcn_sinf(t)  1   1   (device only; t in turns)
//    9  __builtin_amdgcn_cosf(t)  1   1   (device only)
//
// Build: make -C bwidman-raytracer_amd mathprobe -> build/mathprobe (the
// library's exact flags) and build/mathprobe_fast (-DRT_FAST and the fast
// units' flags: the reference-fast device pass).
// Exit status 0 on success, 2 on a HIP error, 3 on a usage or file error.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <vector>

#include "rt_path.h"

namespace {
constexpr int kFunctions = 10;
constexpr int kArity[kFunctions] = {1, 1, 1, 2, 1, 1, 1, 4, 1, 1};
constexpr int kOuts[kFunctions] = {1, 1, 1, 1, 1, 2, 1, 1, 1, 1};
constexpr bool kOnHost[kFunctions] = {true, true, true, true, true, true, true, true, false, false};

RT_HD unsigned bits_of(float x) { return __builtin_bit_cast(unsigned, x); }

RT_HD void eval(int fid, const float* in, unsigned* out) {
    switch (fid) {
        case 0: out[0] = bits_of(rt_sqrt(in[0])); break;
        case 1: out[0] = bits_of(rt_rcp(in[0])); break;
        case 2: out[0] = bits_of(rt_inv_len(in[0])); break;
        case 3: out[0] = bits_of(rt_div(in[0], in[1])); break;
        case 4: out[0] = bits_of(rt_div_spec_chance(in[0])); break;
        case 5: {
            float s, c;
            rt_sincos(in[0], s, c);
            out[0] = bits_of(s);
            out[1] = bits_of(c);
            break;
        }
        case 6: out[0] = bits_of(atan_nn(in[0])); break;
        case 7: out[0] = tone_map(in[0], in[1], in[2], bits_of(in[3])); break;
#if defined(__HIP_DEVICE_COMPILE__)
        case 8: out[0] = bits_of(__builtin_amdgcn_sinf(in[0])); break;
        case 9: out[0] = bits_of(__builtin_amdgcn_cosf(in[0])); break;
#endif
        default: break;
    }
}

__global__ void probe_kernel(int fid, int arity, int outs, const float* in, unsigned* out, long n) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float a[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int k = 0; k < arity; k++) a[k] = in[i * arity + k];
    unsigned r[2] = {0u, 0u};
    eval(fid, a, r);
    for (int k = 0; k < outs; k++) out[i * outs + k] = r[k];
}

bool write_words(const char* path, const std::vector<unsigned>& w) {
    FILE* f = std::fopen(path, "wb");
    if (!f) return false;
    const bool ok = std::fwrite(w.data(), sizeof(unsigned), w.size(), f) == w.size();
    return std::fclose(f) == 0 && ok;
}
}  // namespace

#define HIP_OK(x)                                                    \
    do {                                                             \
        const hipError_t e_ = (x);                                   \
        if (e_ != hipSuccess) {                                      \
            fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); \
            return 2;                                                \
        }                                                            \
    } while (0)

int main(int argc, char** argv) {
    if (argc != 4 && argc != 5) {
        fprintf(stderr, "usage: %s <function id> <in.bin> <out.bin> [host_out.bin]\n", argv[0]);
        return 3;
    }
    const int fid = std::atoi(argv[1]);
    if (fid < 0 || fid >= kFunctions || (argc == 5 && !kOnHost[fid])) {
        fprintf(stderr, "function id %d: %s\n", fid, argc == 5 ? "no host pass" : "unknown");
        return 3;
    }
    const int arity = kArity[fid], outs = kOuts[fid];
    std::vector<float> in;
    {
        FILE* f = std::fopen(argv[2], "rb");
        if (!f) {
            fprintf(stderr, "cannot read %s\n", argv[2]);
            return 3;
        }
        std::fseek(f, 0, SEEK_END);
        const long bytes = std::ftell(f);
        std::fseek(f, 0, SEEK_SET);
        if (bytes < 0 || bytes % (long)(arity * sizeof(float)) != 0) {
            fprintf(stderr, "%s: %ld bytes is no whole number of %d-float tuples\n", argv[2], bytes, arity);
            std::fclose(f);
            return 3;
        }
        in.resize((size_t)bytes / sizeof(float));
        const size_t got = std::fread(in.data(), sizeof(float), in.size(), f);
        std::fclose(f);
        if (got != in.size()) return 3;
    }
    const long n = (long)(in.size() / (size_t)arity);
    std::vector<unsigned> out((size_t)n * outs, 0u);
    if (n > 0) {
        float* din;
        unsigned* dout;
        HIP_OK(hipMalloc(&din, in.size() * sizeof(float)));
        HIP_OK(hipMalloc(&dout, out.size() * sizeof(unsigned)));
        HIP_OK(hipMemcpy(din, in.data(), in.size() * sizeof(float), hipMemcpyHostToDevice));
        HIP_OK(hipMemset(dout, 0, out.size() * sizeof(unsigned)));
        probe_kernel<<<(unsigned)((n + 255) / 256), 256>>>(fid, arity, outs, din, dout, n);
        HIP_OK(hipGetLastError());
        HIP_OK(hipDeviceSynchronize());
        HIP_OK(hipMemcpy(out.data(), dout, out.size() * sizeof(unsigned), hipMemcpyDeviceToHost));
        HIP_OK(hipFree(din));
        HIP_OK(hipFree(dout));
    }
    if (!write_words(argv[3], out)) {
        fprintf(stderr, "cannot write %s\n", argv[3]);
        return 3;
    }
    if (argc == 5) {
        std::vector<unsigned> host((size_t)n * outs, 0u);
        for (long i = 0; i < n; i++) {
            float a[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            for (int k = 0; k < arity; k++) a[k] = in[(size_t)i * arity + k];
            unsigned r[2] = {0u, 0u};
            eval(fid, a, r);
            for (int k = 0; k < outs; k++) host[(size_t)i * outs + k] = r[k];
        }
        if (!write_words(argv[4], host)) {
            fprintf(stderr, "cannot write %s\n", argv[4]);
            return 3;
        }
    }
    printf("function %d: %ld tuples\n", fid, n);
    return 0;
}
