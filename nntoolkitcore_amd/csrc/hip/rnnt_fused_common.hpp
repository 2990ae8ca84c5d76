// rnnt_fused_common.hpp -- what the two fused transducer training losses share (rnnt_fused.hip: the classic loss; rnnt_tdt_fused.hip:
// the token-and-duration loss, two heads in one matrix): the tile's frame, the z build, the logits chain and its row mapping, and the
// launchers of the two small kernels rnnt_fused.hip owns and the other unit reuses unchanged (the W transpose, the partial-block
// reduce).  A tile record `Tile` has live[FT_M], eoff[FT_M], poff[FT_M]; what else it carries is its unit's.
#pragma once
#include "rnnt_common.hpp"

#define FT_M 32
#define FT_PITCH 33
#define FT_THREADS 512
#define FT_WAVES 8
#define FT_NP 32                           // partial blocks of d W: a constant, so that the workspace grows with J and V monotonically
#define FT_GW_WIDE_MAX_J 896              // up to here 8 column blocks of g fit the LDS next to z, above 4

static inline int ft_njb(int J) { return J <= 256 ? 1 : J <= 512 ? 2 : 4; }

template <class Tile>
__device__ __forceinline__ int ft_any_live(const Tile &s) {
    int any = 0;
#pragma unroll
    for (int m = 0; m < FT_M; ++m) any |= s.live[m];
    return any;
}

// Zs[j][m] = act(enc + pred) of the tile's cells; a dead cell's row: zeros, its inputs never read
template <class Tile>
__device__ __forceinline__ void ft_build_z(float *Zs, const Tile &s, const float *__restrict__ enc, const float *__restrict__ pred, int J,
                                           int kind) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int m = wv; m < FT_M; m += FT_WAVES) {
        const int live = s.live[m];
        const float *e = enc + s.eoff[m] * J, *p = pred + s.poff[m] * J;
        for (int j = lane; j < J; j += 64) Zs[j * FT_PITCH + m] = live ? rnnt_act(kind, e[j] + p[j]) : 0.0f;
    }
}

// the [32 cells x 32 columns] block of z W, column col = n0 + c per lane (colv: col < V); one fmaf chain over j = 0 .. J - 1 per element
__device__ __forceinline__ f32x16 ft_logits(const float *Zs, const float *__restrict__ W, int J, int V, int col, bool colv, int c, int kk) {
    f32x16 acc;
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[v] = 0.0f;
    const float *wp = W + (long)kk * V + (colv ? col : 0);
    const float *zp = Zs + kk * FT_PITCH + c;
    int j = 0;
    for (; j + 8 <= J; j += 8) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const float a = zp[(j + 2 * u) * FT_PITCH];
            const float b = colv ? wp[(long)(j + 2 * u) * V] : 0.0f;
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
        }
    }
    for (; j + 2 <= J; j += 2) {
        const float a = zp[j * FT_PITCH];
        const float b = colv ? wp[(long)j * V] : 0.0f;
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
    }
    if (j < J) {                                                            // odd J: the last pair's second term is a zero
        const float a = kk == 0 ? zp[j * FT_PITCH] : 0.0f;
        const float b = kk == 0 && colv ? wp[(long)j * V] : 0.0f;
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
    }
    return acc;
}

__device__ __forceinline__ int ft_row(int v, int kk) { return 8 * (v >> 2) + 4 * kk + (v & 3); }

// rnnt_fused.hip: rnnt_fused_transpose_kernel, WT[v][j] = W[j][v]
int nntk_rnnt_fused_transpose_launch(const float *d_W, float *d_WT, int J, int V);
// rnnt_fused.hip: rnnt_fused_dw_reduce_kernel, dout[e] = partial[e] + partial[n + e] + ... over np blocks of n elements, in order
int nntk_rnnt_fused_dw_reduce_launch(const float *d_partial, float *d_dout, long n, int np);
