// qg_tree_io.h — how the tree and one-column kernels read an operand container, pick a component of a vector load and write a
// result into C: once, for qg_tree.hip, qg_tree_fast.hip, qg_tree_cplx.hip, qg_tree64.hip and qg_gemv.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// element idx of an array of 4- or 8-byte containers
__device__ __forceinline__ int64_t qg_load_c(const char* p, int64_t idx, int cbytes)
{
    return cbytes == 4 ? (int64_t)((const int32_t*)p)[idx] : ((const int64_t*)p)[idx];
}

// r into element idx of C, whose containers have 1, 2, 4 or 8 bytes (the planner has shown that r fits)
template <class T>
__device__ __forceinline__ void qg_store_c(char* C, int64_t idx, int cbytes, T r)
{
    switch (cbytes) {
    case 1: ((int8_t*)C)[idx] = (int8_t)r; break;
    case 2: ((int16_t*)C)[idx] = (int16_t)r; break;
    case 4: ((int32_t*)C)[idx] = (int32_t)r; break;
    default: ((int64_t*)C)[idx] = (int64_t)r; break;
    }
}

// component E (a compile-time value once the loop over it is unrolled) of an int4 load; QG_LANE2: of an int2.  Macros: as a
// __forceinline__ function, by reference or by value, the pick changed the four run-time-mode symbols of k_tree_fast with a split
// product (19383 -> 17721 instructions, 227 -> 213 VGPRs at MAXL 12) and reordered the other four (tools/isa_diff.py)
#define QG_LANE(X, E) ((E) == 0 ? (X).x : (E) == 1 ? (X).y : (E) == 2 ? (X).z : (X).w)
#define QG_LANE2(X, E) ((E) == 0 ? (X).x : (X).y)

// the root of a packed 16-bit form: half j (0: low) of x holds a value left-justified by s16 bits; floor(half / 2^s16), the value
template <bool UNS>
__device__ __forceinline__ int qg_pk16_root(int x, int j, int s16)
{
    if (j == 0) return UNS ? (int)(((unsigned)x & 0xffffu) >> s16) : ((int)((unsigned)x << 16) >> 16) >> s16;
    return UNS ? (int)(((unsigned)x >> 16) >> s16) : (x >> 16) >> s16;
}
