// Shared by prdc.hip and knn.hip: the finished 64 x 64 tile of float64 squared distances between 64 A rows and 64 B rows
// of f32 features, on the pair tile of f64_tile.h.
//   d2(i, j) = max((na[i] + nb[j]) - 2 g(i, j), 0)
// g is the dot product on the f64 matrix instruction over the feature axis in ascending order, na / nb the squared norms
// in f64 in one fixed order that depends on the feature index alone: per staged row 8 partials (the thread that stages
// features 4 q .. 4 q + 3 of every 32-feature chunk adds them over the chunks in ascending order), added in q order.  The
// f32 inputs are widened in registers, so every product is exact in f64, and 2 g is exact too: whether the compiler
// contracts the subtraction into an fma or not, the value is the same.  Both units call this one function, so d2(i, j)
// has the same bits in either, whichever tile, column split or launch computed it, and d2(i, j) == d2(j, i) bitwise when
// both sets are the same rows.  Internal linkage, as f64_tile.h.
#pragma once
#include "f64_tile.h"

namespace {

constexpr int D2T_LD = F64T_TILE + 1;           // row stride of the finished d2 tile in doubles

struct D2TShared {
    __attribute__((aligned(16))) float stage[2][F64T_STAGE];
    double part[2 * F64T_TILE][8];              // per staged row: the norm partials of its 8 feature groups
    double norm[2 * F64T_TILE];
};
static_assert(sizeof(double) * F64T_TILE * D2T_LD <= sizeof(D2TShared::stage), "the d2 tile lives in the staging buffers");

// the finished tile, afterwards whatever a unit's row-wise epilogue leaves there: over the staging buffers, which are idle
// by then
__device__ __forceinline__ double* d2t_tile_of(D2TShared& s) { return reinterpret_cast<double*>(&s.stage[0][0]); }

// KEEP_NAN: a NaN stays one (v_max_f64 returns its other operand, so the plain maximum turns a NaN into 0)
template <bool KEEP_NAN>
__device__ __forceinline__ double d2t_value(double na, double nb, double g) {
    const double t = (na + nb) - 2.0 * g;
    return (KEEP_NAN && t != t) ? t : fmax(t, 0.0);
}

// d2t_tile_of(s)[i * D2T_LD + j] = d2 of staged A row i and staged B row j, for the whole tile.  row: f64t_row of this
// thread's four slots (0, 1: A rows sr, sr + 32 of the block; 2, 3: B rows of the tile), chunks = D / F64T_KC.  Starts
// with a barrier (the previous tile's epilogue has read the buffers) and ends with one (the tile is complete).
template <bool KEEP_NAN>
__device__ __forceinline__ void d2t_tile(D2TShared& s, const float* (&row)[F64T_VEC], const F64Lanes& l, int chunks) {
    const int sr = threadIdx.x >> 3;                            // staged row of slot 0; slot v: + 32 v
    double* sh_d2 = d2t_tile_of(s);
    f64x4_t acc[2][2];
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y) acc[x][y] = f64x4_t{0.0, 0.0, 0.0, 0.0};
    double nrm[F64T_VEC];
#pragma unroll
    for (int v = 0; v < F64T_VEC; ++v) nrm[v] = 0.0;
    // the squared norm of the staged rows: slot v of this thread always holds the same 4 features of the same row, so
    // nrm[v] adds those features over the chunks in ascending order
    const auto norms = [&](int v, const float4& x) {
        const double x0 = (double)x.x, x1 = (double)x.y, x2 = (double)x.z, x3 = (double)x.w;
        nrm[v] = fma(x3, x3, fma(x2, x2, fma(x1, x1, fma(x0, x0, nrm[v]))));
    };

    float4 v[F64T_VEC];
    f64t_fetch(v, row, 0);
    __syncthreads();                // the previous tile's epilogue has read the d2 tile these buffers held
    f64t_stage(s.stage[0], v, norms);
    __syncthreads();
    for (int c = 0; c < chunks; ++c) {
        const bool more = c + 1 < chunks;
        if (more) f64t_fetch(v, row, (c + 1) * F64T_KC);
        f64t_chunk(s.stage[c & 1], l, acc);
        if (more) f64t_stage(s.stage[(c + 1) & 1], v, norms);   // last read in iteration c - 1, which every wave has left
        __syncthreads();
    }

    // squared norms of the 128 staged rows: 8 partials per row, added in feature order
#pragma unroll
    for (int q = 0; q < F64T_VEC; ++q) s.part[sr + 32 * q][threadIdx.x & 7] = nrm[q];
    __syncthreads();
    if (threadIdx.x < 2 * F64T_TILE) {
        const double* __restrict__ p = s.part[threadIdx.x];
        s.norm[threadIdx.x] = ((((((p[0] + p[1]) + p[2]) + p[3]) + p[4]) + p[5]) + p[6]) + p[7];
    }
    __syncthreads();
    f64t_each(l, acc, [&](int i, int j, double g) {
        sh_d2[i * D2T_LD + j] = d2t_value<KEEP_NAN>(s.norm[i], s.norm[F64T_TILE + j], g);
    });
    __syncthreads();
}

}  // namespace
