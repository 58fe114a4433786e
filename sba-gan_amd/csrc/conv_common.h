// Shared by the convolution units igemm.hip (forward / data gradient) and wgrad.hip (weight gradient): the LDS-DMA
// primitives of their ring-staged kernels and the argument check of their entry points.  Internal linkage, as common.h.
#pragma once
#include "common.h"

namespace {

// M0 = LDS destination of the DMA.  M0 is compiler-reserved; nothing else in these kernels uses it (LDS
// instructions need no M0 on gfx9+, no dynamic register indexing, no LDS-DMA builtins), so it is simply
// overwritten: saving and restoring it around every load cost two of the ~10 scalar instructions per load, and
// with one wave per SIMD the main loop is instruction-ISSUE bound (rocprofv3: SQ_ACTIVE_INST_ANY 45 % of the wave
// cycles against 10 % SQ_VALU_MFMA_BUSY_CYCLES on the 17x17 layers, profiles/r02_pmc_igemm_dma_v1.txt).
// voff: per-lane byte offset (bounds-checked: 0xFFFFFFFF -> zeros); soff: wave-uniform byte offset added after
// the bounds check -- the walk along K costs no per-lane arithmetic.
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"
__device__ __forceinline__ void lds_dma16(const __amdgpu_buffer_rsrc_t rsrc, const uint32_t voff, const uint32_t soff,
                                          const uint32_t lds_dst) {
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tbuffer_load_dwordx4 %0, %1, %3 offen lds"
                 :: "v"(voff), "s"(rsrc), "s"(lds_dst), "s"(soff) : "memory", "m0");
}
#pragma clang diagnostic pop
template <int N> __device__ __forceinline__ void wait_vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" :: "n"(N) : "memory"); }
__device__ __forceinline__ void wg_barrier() { asm volatile("s_barrier" ::: "memory"); }

// argument check of the sba_conv_* entry points
bool geom_ok(const sba_conv_geom* g, int dtype) {
    if (!g) return false;
    const int ks = dtype == SBA_BF16 ? 32 : 16;
    if (g->ntaps < 1 || g->ntaps > SBA_MAX_TAPS) return false;
    for (int t = 0; t < g->ntaps; ++t)
        if (g->ty[t] < -8 || g->ty[t] > 7 || g->tx[t] < -8 || g->tx[t] > 7) return false;
    if (g->Cin <= 0 || g->Cin % ks != 0) return false;
    if (g->N <= 0 || g->IH <= 0 || g->IW <= 0 || g->OH <= 0 || g->OW <= 0 || g->Cout <= 0) return false;
    if (g->OHs <= 0 || g->OWs <= 0 || g->osy <= 0 || g->osx <= 0) return false;
    // every written output pixel must lie inside OH x OW
    if ((g->OHs - 1) * g->osy + g->ooy >= g->OH || (g->OWs - 1) * g->osx + g->oox >= g->OW) return false;
    if (g->ooy < 0 || g->oox < 0) return false;
    if ((int64_t)g->N * g->OHs * g->OWs > 0x7fffffff) return false;
    const int64_t esz = dtype == SBA_BF16 ? 2 : 4;
    const int vec = dtype == SBA_BF16 ? 8 : 4;
    const int xcs = g->x_cstride ? g->x_cstride : g->Cin, ycs = g->y_cstride ? g->y_cstride : g->Cout;
    if (xcs < g->Cin + g->x_coff || ycs < g->Cout + g->y_coff || g->x_coff < 0 || g->y_coff < 0) return false;
    if (xcs % vec || g->x_coff % vec || ycs % vec || g->y_coff % vec) return false;
    if ((int64_t)g->N * g->IH * g->IW * xcs * esz >= ((int64_t)1 << 32)) return false;    // 32-bit byte offsets
    if ((int64_t)g->Cout * g->ntaps * g->Cin * esz >= ((int64_t)1 << 32)) return false;
    if ((int64_t)g->N * g->IH * g->IW > 0x7fffffff / 2 || (int64_t)g->N * g->OH * g->OW > 0x7fffffff / 2)
        return false;
    return true;
}

}  // namespace
