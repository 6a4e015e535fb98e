// stamps.h — the s_memtime stamp macros of the diagnostic build (-DF110QP_STAMPS) of the wave kernel
// and the two lane kernels. Each kernel header keeps its own __device__ buffer and read-back call
// (the stamps build compiles them in different translation units). The shipped library never
// executes a stamp: without F110QP_STAMPS the macros expand to nothing.
#pragma once

#ifdef F110QP_STAMPS
#define STAMP(var) unsigned long long var = __builtin_amdgcn_s_memtime()
#define STAMP_SET(var) var = __builtin_amdgcn_s_memtime()
#define STAMP_ACC(acc, since) acc += __builtin_amdgcn_s_memtime() - (since)
#else
#define STAMP(var)
#define STAMP_SET(var)
#define STAMP_ACC(acc, since)
#endif
