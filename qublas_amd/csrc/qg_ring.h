// qg_ring.h — launch interface of the RING plans of the linear class (qg_mfma_ring.hip; the rule and its proof: qg_plan.cpp,
// ring_plan).  Product and every tree level wrap into ONE signed WRP::TCPL format R of n <= 32 bits, so the whole tree is
//     C[i,j] = cvt_C( wrap_R( 2^s * sum_k a_ik b_kj ) ),     wrap_R = reduction modulo 2^n to R's range,
// and everything before the wrap is arithmetic modulo 2^32: int8 limb products of weight 256^w >= 2^n never reach the result,
// and the MFMA's int32 accumulators may wrap, whatever K is.
// (Declared here and not in qg_kernels.h: that header is part of the source hashes the committed counter profiles are keyed on,
// qublas_amd/profmeta.py, and no kernel of those profiles changes with this one.)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "qg_geom.h"   // QG_RING_*, qg_ring_digits, qg_ring_products: the planner's part
#include "qg_ops.h"

struct QRingArgs {
    const int8_t* A;   // [row tile][k tile][LA][128 rows][64 bytes]: the first LA balanced base-256 digits of a (QPackedGeom)
    const int8_t* B;   // [col tile][k tile][LB][128 rows][64 bytes]
    void* C;           // packed C, 128 x 128 tiles, column-major inside, cbytes containers
    int64_t Mp, Np, Kp;
    int32_t cbytes;    // 1 | 2 | 4 | 8
    int32_t n;         // bits of the ring (1 .. 32)
    int32_t s;         // exact left shift of the product into R (0 <= s < n)
    int32_t pad_;
    QStep to_c;        // R -> C (identity when C is R)
};

// LA, LB: planes stored per operand (1 .. 4, at most L); L: digits of the ring.  hipErrorInvalidValue for anything else
hipError_t qg_launch_mfma_ring(int LA, int LB, int L, const QRingArgs& a, hipStream_t st);
