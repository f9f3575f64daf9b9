/*
 * cuda_gl_interop.h — stand-in (TEST INFRASTRUCTURE ONLY; this project's own
 * text, see oracle/ref/README.md).
 *
 * The reference draws into an OpenGL texture mapped as a CUDA surface.  Here
 * the "registered image" is whatever host buffer the harness put into
 * orc_ref_screen before calling render(): mapping hands that buffer out,
 * everything else does nothing.  No arithmetic passes through this header.
 */
#ifndef ORC_REF_CUDA_GL_INTEROP_H
#define ORC_REF_CUDA_GL_INTEROP_H

#include "cuda_runtime.h"

typedef struct orc_ref_graphics_resource* cudaGraphicsResource_t;
enum { cudaGraphicsRegisterFlagsSurfaceLoadStore = 4 };

/* the harness's frame buffer: what surf2Dwrite lands in */
inline orc_ref_surface orc_ref_screen = {nullptr, 0};

inline cudaError_t cudaGraphicsGLRegisterImage(cudaGraphicsResource_t* res, unsigned int, unsigned int, unsigned int) {
    *res = nullptr;
    return cudaSuccess;
}
inline cudaError_t cudaGraphicsMapResources(int, cudaGraphicsResource_t*, cudaStream_t = nullptr) { return cudaSuccess; }
inline cudaError_t cudaGraphicsUnmapResources(int, cudaGraphicsResource_t*, cudaStream_t = nullptr) { return cudaSuccess; }
inline cudaError_t cudaGraphicsSubResourceGetMappedArray(cudaArray_t* array, cudaGraphicsResource_t, unsigned int,
                                                         unsigned int) {
    *array = &orc_ref_screen;
    return cudaSuccess;
}

#endif
