/*
 * cuda_runtime.h — stand-in for the CUDA runtime header (TEST INFRASTRUCTURE
 * ONLY; this project's own text, see oracle/ref/README.md).
 *
 * Only what the reference's Main.cu and its four headers name.  "Device"
 * memory is host memory, a surface is a pitched RGBA8 host buffer, and the
 * device built-ins the reference calls are given their documented meaning.
 *
 * Assumptions made here (also listed in DESIGN.md section 2):
 *  - min / max: CUDA's float overloads are fminf / fmaxf (a NaN operand gives
 *    the other operand; CUDA math API, "fminf"/"fmaxf" and the min/max
 *    overloads of the device headers); the int overloads are the plain
 *    comparisons.
 *  - make_uchar4 of float arguments: nvcc converts float to unsigned char
 *    with cvt.rzi.u8.f32, which saturates and maps NaN to 0 (PTX ISA, "cvt").
 *    Plain C++ leaves that conversion undefined, so it is spelled out here.
 *    The reference only passes round()-ed values in [0, 255] or NaN.
 *  - Everything else (cudaMalloc, cudaMemcpy, the graphics-interop and
 *    surface-object calls) moves bytes or does nothing.
 */
#ifndef ORC_REF_CUDA_RUNTIME_H
#define ORC_REF_CUDA_RUNTIME_H

#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <math.h>

#include "host_defines.h"

/* ---- vector types and launch geometry ---------------------------------- */
struct dim3 {
    unsigned int x, y, z;
    dim3(unsigned int x_ = 1, unsigned int y_ = 1, unsigned int z_ = 1) : x(x_), y(y_), z(z_) {}
};
struct uint3 {
    unsigned int x, y, z;
};
struct uchar4 {
    unsigned char x, y, z, w;
};

/* float -> unsigned char as cvt.rzi.u8.f32 does it: NaN -> 0, saturating */
struct orc_ref_u8 {
    unsigned char v;
    orc_ref_u8(float f) : v(f != f ? 0 : f <= 0.0f ? 0 : f >= 255.0f ? 255 : (unsigned char)f) {}
    orc_ref_u8(int i) : v(i <= 0 ? 0 : i >= 255 ? 255 : (unsigned char)i) {}
};
inline uchar4 make_uchar4(orc_ref_u8 x, orc_ref_u8 y, orc_ref_u8 z, orc_ref_u8 w) {
    return uchar4{x.v, y.v, z.v, w.v};
}

/* ---- device math overloads --------------------------------------------- */
inline float min(float a, float b) { return fminf(a, b); }
inline float max(float a, float b) { return fmaxf(a, b); }
inline int min(int a, int b) { return a < b ? a : b; }
inline int max(int a, int b) { return a > b ? a : b; }

/* ---- errors, memory ------------------------------------------------------ */
enum cudaError { cudaSuccess = 0, cudaErrorUnknown = 999 };
typedef cudaError cudaError_t;
enum cudaMemcpyKind { cudaMemcpyHostToHost, cudaMemcpyHostToDevice, cudaMemcpyDeviceToHost, cudaMemcpyDeviceToDevice };
typedef struct orc_ref_stream* cudaStream_t;

template <class T>
inline cudaError_t cudaMalloc(T** p, size_t bytes) {
    *p = static_cast<T*>(std::malloc(bytes ? bytes : 1));
    return *p ? cudaSuccess : cudaErrorUnknown;
}
inline cudaError_t cudaMemcpy(void* dst, const void* src, size_t bytes, cudaMemcpyKind) {
    std::memcpy(dst, src, bytes);
    return cudaSuccess;
}
inline cudaError_t cudaFree(void* p) {
    std::free(p);
    return cudaSuccess;
}
inline cudaError_t cudaStreamSynchronize(cudaStream_t) { return cudaSuccess; }
inline cudaError_t cudaDeviceReset() { return cudaSuccess; }

/* ---- surfaces: a pitched RGBA8 host buffer ------------------------------ */
struct orc_ref_surface {
    unsigned char* data; /* row y starts at data + y * pitch */
    size_t pitch;
};
typedef orc_ref_surface* cudaArray_t;
typedef orc_ref_surface* cudaSurfaceObject_t;
enum cudaResourceType { cudaResourceTypeArray };
struct cudaResourceDesc {
    cudaResourceType resType;
    struct {
        struct {
            cudaArray_t array;
        } array;
    } res;
};
inline cudaError_t cudaCreateSurfaceObject(cudaSurfaceObject_t* out, const cudaResourceDesc* desc) {
    *out = desc->res.array.array;
    return *out ? cudaSuccess : cudaErrorUnknown;
}
inline cudaError_t cudaDestroySurfaceObject(cudaSurfaceObject_t) { return cudaSuccess; }
/* x is a byte offset, as in CUDA */
inline void surf2Dwrite(uchar4 v, cudaSurfaceObject_t s, int x_bytes, int y) {
    std::memcpy(s->data + (size_t)y * s->pitch + (size_t)x_bytes, &v, sizeof v);
}

#endif
