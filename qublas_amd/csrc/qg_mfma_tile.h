// qg_mfma_tile.h — device-side pieces shared by the matrix-core kernels of the linear class (qg_mfma*.hip): what surrounds their
// main loops.  The loops themselves (cursors, issue schedules, fragment reads, accumulator layouts) are each kernel's own.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <utility>

#include "qg_tile_walk.h"

typedef int v4i __attribute__((ext_vector_type(4)));

#define QG_GLOBAL_PTR(p) ((const __attribute__((address_space(1))) void*)(p))
#define QG_LDS_PTR(p) ((__attribute__((address_space(3))) void*)(p))

// Issue-order hint for one basic block that holds NM MFMAs, NDS LDS reads and NVM LDS-DMA issues: the reads and DMA issues
// are spread evenly between the MFMAs (sched_group_barrier masks: 0x008 MFMA, 0x100 DS read, 0x020 VMEM read) instead of the
// compiler's default of a burst of reads / a burst of DMA issues and then the MFMAs back to back.  Both waves of a SIMD leave
// the k-tile barrier together, so bursts collide and the matrix pipe idles while both issue ~100-cycle DMA instructions;
// interleaved, one wave's MFMAs cover the other's issue slots.  Measured on the 3x3 kernel at 4096^3: 0.432 vs 0.4525 ms.
template <int NM, int NDS, int NVM, int... M>
__device__ __forceinline__ void interleave_hint(std::integer_sequence<int, M...>)
{
    ((__builtin_amdgcn_sched_group_barrier(0x008, 1, 0),
      __builtin_amdgcn_sched_group_barrier(0x100, (M + 1) * NDS / NM - M * NDS / NM, 0),
      __builtin_amdgcn_sched_group_barrier(0x020, (M + 1) * NVM / NM - M * NVM / NM, 0)),
     ...);
}

// Issue-order hint for one basic block that holds NP + NT MFMAs and NP * NV vector ALU instructions beside them (operand sums of a
// Karatsuba form, address updates): NP times (one MFMA, NV vector instructions), then the last NT MFMAs back to back.  The block
// opens with an MFMA, and an in-order wave never holds an MFMA back behind a run of vector instructions longer than the issue
// slots a 16-cycle MFMA leaves free; a value formed NV instructions or more ahead of its MFMA needs no s_nop in front of it.
template <int NV, int... P>
__device__ __forceinline__ void paced_valu_pairs(std::integer_sequence<int, P...>)
{
    (((void)P, __builtin_amdgcn_sched_group_barrier(0x008, 1, 0), __builtin_amdgcn_sched_group_barrier(0x002, NV, 0)), ...);
}
template <int NP, int NV, int NT>
__device__ __forceinline__ void paced_valu_hint()
{
    paced_valu_pairs<NV>(std::make_integer_sequence<int, NP>{});
    __builtin_amdgcn_sched_group_barrier(0x008, NT, 0);
}

// Packed C is tiled [tile_m][tile_n][col][row] (column-major inside the tile, the order of the host tensor), and every lane of an
// MFMA's C/D layout owns runs of 4 consecutive rows of one column: a run is ONE store of 4 / 8 / 16 / 32 bytes.  base: element
// index of the run's first row; q: its four values (int32 or int64), stored in containers of CB bytes (4 or 8: the kernels that
// know CB at compile time give narrower containers a transposing store of their own, k_mfma_pp).  The lock-step kernels and
// k_mfma_ring choose the container at run time and keep that switch in their epilogues.
template <int CB, class S>
__device__ __forceinline__ void qg_store_run4(char* C, int64_t base, const S* q)
{
    static_assert(CB == 4 || CB == 8, "container bytes of packed C");
    if constexpr (CB == 4) {
        *(int4*)(C + base * 4) = make_int4((int)q[0], (int)q[1], (int)q[2], (int)q[3]);
    } else {
        int64_t* p = (int64_t*)(C + base * 8);
        *(longlong2*)p = make_longlong2((int64_t)q[0], (int64_t)q[1]);
        *(longlong2*)(p + 2) = make_longlong2((int64_t)q[2], (int64_t)q[3]);
    }
}
