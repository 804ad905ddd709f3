/*
 * cudecomp_amd.h -- extensions of the cuDecomp API a solver may use.
 *
 * cudecomp.h stays the drop-in boundary (exactly the reference's API); cudecomp_ext.h is for test harnesses and
 * tools.  What is declared here is accepted by this library only.
 *
 * 2-byte element types.  Every entry point that takes a cudecompDataType_t accepts these values in addition to the
 * four of cudecomp.h: cudecompGetDataTypeSize, the four transposes, the three halo updates and
 * cudecompGridDescAutotuneOptions_t::dtype.  Data movement is bit-exact: no value is ever converted, so NaN payloads,
 * -0, subnormals and infinities arrive exactly as they were sent.
 *
 * The values are 1..3: the reference's enumerators are -1..-4, which makes [-4, 3] the range of values of the enum in
 * C++, so these are valid cudecompDataType_t values in C and C++ alike and cannot collide with the reference's.
 */
#ifndef CUDECOMP_AMD_H
#define CUDECOMP_AMD_H

#include "cudecomp.h"

#define CUDECOMP_AMD_HALF ((cudecompDataType_t)1)         /* IEEE binary16, 2 bytes */
#define CUDECOMP_AMD_BFLOAT16 ((cudecompDataType_t)2)     /* bfloat16, 2 bytes */
#define CUDECOMP_AMD_HALF_COMPLEX ((cudecompDataType_t)3) /* interleaved binary16 (re, im), 4 bytes */

#endif /* CUDECOMP_AMD_H */
