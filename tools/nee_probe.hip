// Probe of bwidman-raytracer_amd/csrc/rt_light.h (tests/test_nee_reference.py,
// tests/test_gpu_nee_probe.py): evaluates one function of the header for each
// case of a file against a light table of a file, one case per lane, in the
// device pass and/or the host pass, and writes the result words.  It includes
// the header and nothing of the context.
//
//   neeprobe FID table.bin cases.bin out.bin [out.host.bin]
//   neeprobe --host FID table.bin cases.bin out.host.bin    (no HIP call at all)
//
// table.bin, 32-bit words: {n_lights, n_sphere_lights, n_sph, n_hit}, then
// n_lights records of RT_LIGHT_FLOATS, n_lights - n_sphere_lights sampling
// blocks of RT_POLY_LIGHT_FLOATS, n_hit hit-table rows of RT_HIT_FLOATS
// (rt_layout.h).  The SHAPES = spheres functions see the first n_sphere_lights
// records only, as a render in that mode does.
//
//   id  function                               case words                      out words
//    0  nee_sample<uniform, spheres>           state[6] P[3] n[3] prim kind    j prim trace k wi[3] state[6]
//    1  nee_sample<weighted, spheres>          (state: d, v0 .. v4)
//    2  nee_sample<uniform, all>
//    3  nee_sample<weighted, all>
//    4  nee_pick_weight                        m P[3] n[3] nl prim             w
//    5  nee_pick_weight_poly                   (m: the table index of the light)
//    6  light_suppressed<spheres>              P[3] prim id                    0 / 1
//    7  light_suppressed<all>
//    8  fold_level_nee                         c0 k c aux lx ly lz             lx ly lz
//    9  nee_normal_kind                        sphere n[3]                     kind
//
// Every index a case carries (m; the hit row of c0 and the light of aux) is
// checked against the table before anything runs; ids 0 .. 3 need a light.
//
// Build: make -C bwidman-raytracer_amd neeprobe -> build/neeprobe and
// build/neeprobe_bvh (the flags of the two NEE kernel units) and
// build/neeprobe_cpu (the CPU twin's flags, -DNEEPROBE_HOST_ONLY: host pass only).
// Exit status 0 on success, 2 on a HIP error, 3 on a usage or file error.
#if !defined(NEEPROBE_HOST_ONLY)
#include <hip/hip_runtime.h>
#endif

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rt_light.h"

namespace {
constexpr int kFunctions = 10;
constexpr int kIn[kFunctions] = {14, 14, 14, 14, 9, 9, 5, 5, 7, 4};
constexpr int kOut[kFunctions] = {13, 13, 13, 13, 1, 1, 1, 1, 3, 1};

struct Table {
    int n_lights, n_sphere_lights, n_sph, n_hit;
    const float* lights;
    const float* poly;
    const float* hit;
};

RT_HD unsigned bits_of(float x) { return __builtin_bit_cast(unsigned, x); }
RT_HD float float_of(unsigned x) { return __builtin_bit_cast(float, x); }

template <int PICK, int SHAPES>
RT_HD void sample(const rt_nee_args& N, const unsigned* in, unsigned* out) {
    Xorwow rs;
    rs.d = in[0], rs.v0 = in[1], rs.v1 = in[2], rs.v2 = in[3], rs.v3 = in[4], rs.v4 = in[5];
    const f3 P = mk(float_of(in[6]), float_of(in[7]), float_of(in[8]));
    const f3 n = mk(float_of(in[9]), float_of(in[10]), float_of(in[11]));
    const NeeSample s = nee_sample<PICK, SHAPES>(rs, N, P, n, (int)in[12], (int)in[13]);
    out[0] = (unsigned)s.j;
    out[1] = (unsigned)s.prim;
    out[2] = s.trace ? 1u : 0u;
    out[3] = bits_of(s.k);
    out[4] = bits_of(s.wi.x), out[5] = bits_of(s.wi.y), out[6] = bits_of(s.wi.z);
    out[7] = rs.d, out[8] = rs.v0, out[9] = rs.v1, out[10] = rs.v2, out[11] = rs.v3, out[12] = rs.v4;
}

RT_HD void eval(int fid, const Table& T, const unsigned* in, unsigned* out) {
    rt_nee_args N;
    N.lights = T.lights;
    N.n_lights = T.n_lights;
    N.pick = 0;
    N.poly = T.poly;
    N.n_sphere_lights = T.n_sphere_lights;
    if (fid == 0 || fid == 1 || fid == 6) N.n_lights = T.n_sphere_lights;
    switch (fid) {
        case 0: sample<RT_PICK_UNIFORM, RT_SHAPES_SPHERES>(N, in, out); break;
        case 1: sample<RT_PICK_WEIGHTED, RT_SHAPES_SPHERES>(N, in, out); break;
        case 2: sample<RT_PICK_UNIFORM, RT_SHAPES_ALL>(N, in, out); break;
        case 3: sample<RT_PICK_WEIGHTED, RT_SHAPES_ALL>(N, in, out); break;
        case 4:
        case 5: {
            const LightRec l = light_load(T.lights, (int)in[0]);
            const f3 P = mk(float_of(in[1]), float_of(in[2]), float_of(in[3]));
            const f3 n = mk(float_of(in[4]), float_of(in[5]), float_of(in[6]));
            const float nl = float_of(in[7]);
            out[0] = bits_of(fid == 4 ? nee_pick_weight(l, P, n, nl, (int)in[8]) : nee_pick_weight_poly(l, P, n, nl, (int)in[8]));
            break;
        }
        case 6:
        case 7: {
            rt_kparams K{};
            K.n_sph = T.n_sph;
            const f3 P = mk(float_of(in[0]), float_of(in[1]), float_of(in[2]));
            const bool s = fid == 6 ? light_suppressed<RT_SHAPES_SPHERES>(K, N, P, (int)in[3], (int)in[4])
                                    : light_suppressed<RT_SHAPES_ALL>(K, N, P, (int)in[3], (int)in[4]);
            out[0] = s ? 1u : 0u;
            break;
        }
        case 8: {
            float lx = float_of(in[4]), ly = float_of(in[5]), lz = float_of(in[6]);
            fold_level_nee((int)in[0], float_of(in[1]), float_of(in[2]), (int)in[3], T.hit, N, lx, ly, lz);
            out[0] = bits_of(lx), out[1] = bits_of(ly), out[2] = bits_of(lz);
            break;
        }
        case 9: out[0] = (unsigned)nee_normal_kind(in[0] != 0u, mk(float_of(in[1]), float_of(in[2]), float_of(in[3]))); break;
        default: break;
    }
}

#if !defined(NEEPROBE_HOST_ONLY)
// one case per lane; the table in global memory, shared by all lanes, so the
// weight passes' index m is uniform across a wave (light_load_uniform)
__global__ void probe_kernel(int fid, Table T, int nin, int nout, const unsigned* in, unsigned* out, long n) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    unsigned a[14], r[13];
    for (int k = 0; k < 14; k++) a[k] = k < nin ? in[i * nin + k] : 0u;
    for (int k = 0; k < 13; k++) r[k] = 0u;
    eval(fid, T, a, r);
    for (int k = 0; k < nout; k++) out[i * nout + k] = r[k];
}
#endif

bool read_words(const char* path, std::vector<unsigned>& w) {
    FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    std::fseek(f, 0, SEEK_END);
    const long bytes = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    if (bytes < 0 || bytes % 4 != 0) {
        std::fclose(f);
        return false;
    }
    w.resize((size_t)bytes / 4);
    const size_t got = w.empty() ? 0 : std::fread(w.data(), 4, w.size(), f);
    std::fclose(f);
    return got == w.size();
}

bool write_words(const char* path, const std::vector<unsigned>& w) {
    FILE* f = std::fopen(path, "wb");
    if (!f) return false;
    const bool ok = std::fwrite(w.data(), sizeof(unsigned), w.size(), f) == w.size();
    return std::fclose(f) == 0 && ok;
}

// every index of a case lies inside the table
bool case_in_bounds(int fid, const Table& T, const unsigned* in) {
    if (fid == 4 || fid == 5) return (int)in[0] >= 0 && (int)in[0] < T.n_lights;
    if (fid == 8) {
        const int c0 = (int)in[0], aux = (int)in[3];
        const int row = c0 < 0 ? ~c0 : c0;
        if (row < 0 || row >= T.n_hit) return false;
        if (aux < 0) return false;
        if ((aux & RT_NEE_LEVEL) && (aux & RT_NEE_VISIBLE) && (aux >> RT_NEE_JSHIFT) >= T.n_lights) return false;
    }
    return true;
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
    const bool host_only = argc > 1 && !std::strcmp(argv[1], "--host");
    if (host_only ? argc != 6 : (argc != 5 && argc != 6)) {
        fprintf(stderr, "usage: %s FID table.bin cases.bin out.bin [out.host.bin]\n       %s --host FID table.bin cases.bin out.host.bin\n",
                argv[0], argv[0]);
        return 3;
    }
    char** a = argv + (host_only ? 2 : 1);
    const int fid = std::atoi(a[0]);
    if (fid < 0 || fid >= kFunctions) {
        fprintf(stderr, "function id %d: unknown\n", fid);
        return 3;
    }
    const char* dev_path = host_only ? nullptr : a[3];
    const char* host_path = host_only ? a[3] : (argc == 6 ? a[4] : nullptr);
#if defined(NEEPROBE_HOST_ONLY)
    if (dev_path) {
        fprintf(stderr, "this build has the host pass only: use --host\n");
        return 3;
    }
#endif
    std::vector<unsigned> tw, cases;
    if (!read_words(a[1], tw) || !read_words(a[2], cases)) {
        fprintf(stderr, "cannot read %s or %s\n", a[1], a[2]);
        return 3;
    }
    Table T;
    if (tw.size() < 4) return fprintf(stderr, "%s: no header\n", a[1]), 3;
    T.n_lights = (int)tw[0], T.n_sphere_lights = (int)tw[1], T.n_sph = (int)tw[2], T.n_hit = (int)tw[3];
    if (T.n_lights < 0 || T.n_lights > (1 << 20) || T.n_sphere_lights < 0 || T.n_sphere_lights > T.n_lights || T.n_hit < 0 ||
        T.n_hit > (1 << 20)) {
        fprintf(stderr, "%s: bad header\n", a[1]);
        return 3;
    }
    const size_t n_poly = (size_t)(T.n_lights - T.n_sphere_lights);
    const size_t lw = (size_t)T.n_lights * RT_LIGHT_FLOATS, pw = n_poly * RT_POLY_LIGHT_FLOATS, hw = (size_t)T.n_hit * RT_HIT_FLOATS;
    if (tw.size() != 4 + lw + pw + hw) {
        fprintf(stderr, "%s: %zu words, the header asks for %zu\n", a[1], tw.size(), 4 + lw + pw + hw);
        return 3;
    }
    // (16-byte aligned copies: the header reads float4s; one spare record so no pointer is null)
    std::vector<float4> lights(lw / 4 + 2), poly(pw / 4 + 5), hit(hw / 4 + 4);
    std::memcpy(lights.data(), tw.data() + 4, lw * 4);
    std::memcpy(poly.data(), tw.data() + 4 + lw, pw * 4);
    std::memcpy(hit.data(), tw.data() + 4 + lw + pw, hw * 4);
    const int nin = kIn[fid], nout = kOut[fid];
    if (cases.size() % (size_t)nin != 0) {
        fprintf(stderr, "%s: %zu words is no whole number of %d-word cases\n", a[2], cases.size(), nin);
        return 3;
    }
    const long n = (long)(cases.size() / (size_t)nin);
    const int seen = (fid == 0 || fid == 1) ? T.n_sphere_lights : T.n_lights;
    if (fid <= 3 && seen < 1) {
        fprintf(stderr, "function %d needs a light in the table\n", fid);
        return 3;
    }
    for (long i = 0; i < n; i++)
        if (!case_in_bounds(fid, T, cases.data() + (size_t)i * nin)) {
            fprintf(stderr, "case %ld: an index outside the table\n", i);
            return 3;
        }
#if !defined(NEEPROBE_HOST_ONLY)
    if (dev_path) {
        std::vector<unsigned> out((size_t)n * nout, 0u);
        if (n > 0) {
            float4 *dl, *dp, *dh;
            unsigned *din, *dout;
            HIP_OK(hipMalloc(&dl, lights.size() * sizeof(float4)));
            HIP_OK(hipMalloc(&dp, poly.size() * sizeof(float4)));
            HIP_OK(hipMalloc(&dh, hit.size() * sizeof(float4)));
            HIP_OK(hipMalloc(&din, cases.size() * 4));
            HIP_OK(hipMalloc(&dout, out.size() * 4));
            HIP_OK(hipMemcpy(dl, lights.data(), lights.size() * sizeof(float4), hipMemcpyHostToDevice));
            HIP_OK(hipMemcpy(dp, poly.data(), poly.size() * sizeof(float4), hipMemcpyHostToDevice));
            HIP_OK(hipMemcpy(dh, hit.data(), hit.size() * sizeof(float4), hipMemcpyHostToDevice));
            HIP_OK(hipMemcpy(din, cases.data(), cases.size() * 4, hipMemcpyHostToDevice));
            HIP_OK(hipMemset(dout, 0, out.size() * 4));
            Table D = T;
            D.lights = (const float*)dl, D.poly = (const float*)dp, D.hit = (const float*)dh;
            probe_kernel<<<(unsigned)((n + 255) / 256), 256>>>(fid, D, nin, nout, din, dout, n);
            HIP_OK(hipGetLastError());
            HIP_OK(hipDeviceSynchronize());
            HIP_OK(hipMemcpy(out.data(), dout, out.size() * 4, hipMemcpyDeviceToHost));
            HIP_OK(hipFree(dl));
            HIP_OK(hipFree(dp));
            HIP_OK(hipFree(dh));
            HIP_OK(hipFree(din));
            HIP_OK(hipFree(dout));
        }
        if (!write_words(dev_path, out)) {
            fprintf(stderr, "cannot write %s\n", dev_path);
            return 3;
        }
    }
#endif
    if (host_path) {
        T.lights = (const float*)lights.data(), T.poly = (const float*)poly.data(), T.hit = (const float*)hit.data();
        std::vector<unsigned> host((size_t)n * nout, 0u);
        for (long i = 0; i < n; i++) {
            unsigned r[13] = {0u};
            eval(fid, T, cases.data() + (size_t)i * nin, r);
            for (int k = 0; k < nout; k++) host[(size_t)i * nout + k] = r[k];
        }
        if (!write_words(host_path, host)) {
            fprintf(stderr, "cannot write %s\n", host_path);
            return 3;
        }
    }
    printf("function %d: %ld cases\n", fid, n);
    return 0;
}
