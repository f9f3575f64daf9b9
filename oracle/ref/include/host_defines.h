/*
 * host_defines.h — stand-in for the CUDA header of this name (TEST
 * INFRASTRUCTURE ONLY; this project's own text, see oracle/ref/README.md).
 *
 * Lets the reference's sources compile as plain host C++.  Assumption made
 * here: the CUDA function-space qualifiers carry no arithmetic meaning, so
 * they expand to nothing and every function is an ordinary host function.
 */
#ifndef ORC_REF_HOST_DEFINES_H
#define ORC_REF_HOST_DEFINES_H

#define __device__
#define __host__
#define __global__

#endif
