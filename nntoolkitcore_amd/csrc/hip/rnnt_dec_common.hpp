// rnnt_dec_common.hpp -- what the transducer decoders (rnnt_decode.hip: greedy; rnnt_beam.hip: beam search) share, so that a logits
// vector for a given (frame, prediction-network state) has the same bits in both: the matrix-vector product that serves R states with
// one pass over a matrix, the joiner's activation, the gates' sigmoid and the butterflies of the max / sum-exp reduction.
//
// Bits.  Every output element of a matrix-vector product is  ((p0 + p1) + (p2 + p3)) + bias  with p_i the fmaf chain over k = i mod 4,
// ascending -- whatever R.  The maximum is exact; ties go to the lowest index in the lane scan, the butterfly and the scan over the
// wavefronts.  sum exp(x - max): expf per element, added in double in a fixed order (a lane's elements ascending, the xor butterfly, the
// wavefronts ascending).
#pragma once
#include <stdint.h>
#include "nntk_common.hpp"

#define RD_THREADS 1024
#define RD_WAVES (RD_THREADS / 64)
#define RD_LDS_MAX (152 * 1024)            // of the 160 KiB of a CU

__device__ __forceinline__ float rd_act(int kind, float x) { return kind == 1 ? tanhf(x) : kind == 2 ? fmaxf(x, 0.0f) : x; }
__device__ __forceinline__ float rd_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

// column n of x [R][Kp] (LDS, rows 16-byte aligned) times Wm [K][N]: four interleaved fmaf chains per row, combined pairwise
template <int R>
__device__ __forceinline__ void rd_matvec(const float *__restrict__ Wm, int K, int N, int n, const float *x, int Kp, float (&res)[R]) {
    float p[R][4];
#pragma unroll
    for (int r = 0; r < R; ++r) p[r][0] = p[r][1] = p[r][2] = p[r][3] = 0.0f;
    const float *w = Wm + n;
    int k = 0;
#pragma unroll 2
    for (; k + 4 <= K; k += 4) {
        const float w0 = w[(size_t)k * N], w1 = w[(size_t)(k + 1) * N], w2 = w[(size_t)(k + 2) * N], w3 = w[(size_t)(k + 3) * N];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const f32x4 v = *(const f32x4 *)(x + r * Kp + k);
            p[r][0] = fmaf(v[0], w0, p[r][0]);
            p[r][1] = fmaf(v[1], w1, p[r][1]);
            p[r][2] = fmaf(v[2], w2, p[r][2]);
            p[r][3] = fmaf(v[3], w3, p[r][3]);
        }
    }
    for (int i = 0; k < K; ++k, ++i) {                                       // at most three left: chains 0, 1, 2
        const float wk = w[(size_t)k * N];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const float v = x[r * Kp + k];
            if (i == 0) p[r][0] = fmaf(v, wk, p[r][0]);
            else if (i == 1) p[r][1] = fmaf(v, wk, p[r][1]);
            else p[r][2] = fmaf(v, wk, p[r][2]);
        }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) res[r] = (p[r][0] + p[r][1]) + (p[r][2] + p[r][3]);
}

// the wavefront's part of the argmax: the greater value, on equal values the lower index
__device__ __forceinline__ void rd_wave_argmax(float &m, int &mi) {
    for (int off = 32; off > 0; off >>= 1) {
        const float om = __shfl_xor(m, off);
        const int oi = __shfl_xor(mi, off);
        if (om > m || (om == m && oi < mi)) { m = om; mi = oi; }
    }
}

// a lane's part of sum exp(x[n] - m), n = tid, tid + RD_THREADS, ... ascending, then the xor butterfly: the wavefront's sum in every lane
__device__ __forceinline__ double rd_wave_sum_exp(const float *x, int V, int tid, float m) {
    double sum = 0.0;
    for (int n = tid; n < V; n += RD_THREADS) sum += (double)expf(x[n] - m);
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
    return sum;
}
