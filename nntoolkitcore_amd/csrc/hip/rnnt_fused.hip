// rnnt_fused.hip -- the transducer training loss straight from the joiner's inputs: with logits[b][t][u] = act(enc[b][t] + pred[b][u]) W + b,
// the loss rows of rnnt.hip and the gradients of their plain sum with respect to enc, pred and the Dense block W | b.  Neither the
// [B][T][U1][V] scores nor their gradient ever exist in memory: a tile of them lives in MFMA accumulators, is folded into per-cell
// scalars (forward) or into the two products that need it (backward), and is gone.
//
// Everything is done on tiles of FT_M = 32 consecutive cells c = (b T + t) U1 + u; a tile without a live cell is skipped, and in a mixed
// tile a dead cell's operand row is SELECTED to zero (never multiplied by zero: enc / pred may hold NaN there).  The operand
// z = act(enc + pred) of a tile is built once per tile in LDS, transposed (Zs[j][m], pitch 33: conflict-free both ways).  All products
// are exact-f32 v_mfma_f32_32x32x2_f32; lane (c = lane % 32, kk = lane / 32) supplies A[k = kk][m = c] and B[k = kk][n = c] and holds
// D[row = 8 (v / 4) + 4 kk + v % 4][n = c] in acc[v] (train.hip's outer_mfma_kernel).  A logit is one k-ordered fmaf chain over j, the
// same chain in every kernel here (ft_logits), so the backward passes see the forward's bits.
//
//  rnnt_fused_forward_kernel, a 512-lane workgroup per tile: wave w takes the 32-column blocks w, w + 8, ... of V; per block one
//    [32 x 32] logits tile (J / 2 MFMAs), then per cell the block's maximum (a 32-lane butterfly), the running maximum, and the sum of
//    exp(x - max) kept per lane in double and rescaled (double exp) only when the cell's maximum grows.  The lane that holds the
//    blank's / the next label's column hands that logit over.  At the end the 8 waves' (max, sum) pairs are merged in wave order, and
//    the emissions (mantissa and exponent, rnnt_emission) and lse are the only things written: 16 + 8 bytes per cell.
//  rnnt_lattice_kernel: rnnt.hip's, unchanged, on those emissions; the workspace starts with rnnt.hip's layout (FtLayout::base), so the
//    entry's prologue -- int upload, pointers into the layout -- is rnnt_common.hpp's, as in rnnt.hip and rnnt_align.hip.
//  rnnt_fused_dz_kernel, a workgroup per tile: per group of gw (8, or 4 above J = 896: LDS) column blocks, phase A: wave w < gw
//    recomputes a logits block and forms g = occupancy exp(x - lse) - flows (rnnt_grad_kernel's formula) into LDS, transposed; phase
//    B: every wave owns the 32-wide blocks w, w + 8, ... of J and accumulates d z += g W^T over the group's columns (W^T: a transposed
//    copy made once per call, so that the B operand loads are coalesced).  d z act'(z) is written once, [cells][J]; rnnt.hip's
//    rnnt_joint_reduce_kernel sums it over u and over t (ascending, one accumulator per element) into d_enc and d_pred.
//  rnnt_fused_dw_kernel<NJB>, grid (column groups of V, NP slices of the tiles): the same phase A on NB = 4 / NJB column blocks, then
//    phase C: d W[j][v] += sum over the tile's 32 cells of z[m][j] g[m][v] (16 MFMAs per [32 x 32] block), all NJB x NB blocks of a
//    wave held in accumulators across the whole slice, plus the column sums of g (d b).  Each (slice) writes its own [J + 1][V] block;
//    rnnt_fused_dw_reduce_kernel adds the NP = 32 blocks in order.
// No atomics; every sum has a fixed order; a cell's scalars and its d z depend on nothing but the cell.
#include "rnnt_common.hpp"

#define FT_M 32
#define FT_PITCH 33
#define FT_THREADS 512
#define FT_WAVES 8
#define FT_NP 32                           // partial blocks of d W: a constant, so that the workspace grows with J and V monotonically
#define FT_GW_WIDE_MAX_J 896              // up to here 8 column blocks of g fit the LDS next to z, above 4

struct FtLayout { RnntLayout base; size_t wt, partial, dz, total; int np, njb; };
static int ft_njb(int J) { return J <= 256 ? 1 : J <= 512 ? 2 : 4; }
static FtLayout ft_layout(int B, int T, int maxL, int J, int V, int want_grad) {
    FtLayout l;
    auto up = [](size_t x) { return (x + 3) & ~(size_t)3; };
    const size_t j = J > 0 ? (size_t)J : 0, v = V > 0 ? (size_t)V : 0;
    l.base = rnnt_layout(B, T, maxL, want_grad);
    l.njb = ft_njb(J);
    l.np = FT_NP;
    const size_t cells = (size_t)(B > 0 ? B : 0) * (size_t)(T > 0 ? T : 0) * ((size_t)(maxL > 0 ? maxL : 0) + 1);
    l.wt = up(l.base.total);
    l.partial = l.wt + (want_grad ? up(j * v) : 0);
    l.dz = l.partial + (want_grad ? up((size_t)l.np * (j + 1) * v) : 0);
    l.total = l.dz + (want_grad ? up(cells * j) : 0) + 4;
    return l;
}

struct FtTile {                            // one tile's cells, in LDS
    long eoff[FT_M], poff[FT_M];           // rows of enc and pred
    double lse[FT_M];
    float occ[FT_M], fb[FT_M], fy[FT_M];   // occupancy alpha beta / P and the two outgoing flows (rnnt_grad_kernel)
    int live[FT_M], y[FT_M];               // y: the next label, -1 where there is none
};

// GRAD: a cell of a row with P = 0 counts as dead, and the gradient's three scalars are worked out.  Returns nothing; barrier after.
template <bool GRAD>
__device__ __forceinline__ void ft_tile_cells(FtTile &s, long tile, long cells, int B, int T, int U1, const int *__restrict__ ints,
                                              const float4 *__restrict__ em, const double *__restrict__ lse_in,
                                              const float2 *__restrict__ wa, const float2 *__restrict__ wb, const float *__restrict__ hdr) {
    const int m = threadIdx.x;
    if (m >= FT_M) return;
    const long c = tile * FT_M + m;
    int live = 0, y = -1;
    long eo = 0, po = 0;
    if (c < cells) {
        const RnntCell q = rnnt_cell(c, T, U1);
        const int Tb = ints[q.b], Ub = ints[B + q.b];
        live = q.t < Tb && q.u <= Ub;
        if (GRAD && live && !(hdr[2 * q.b] > 0.0f)) live = 0;
        if (live) {
            eo = (long)q.b * T + q.t;
            po = (long)q.b * U1 + q.u;
            if (q.u < Ub) y = ints[2L * B + (long)q.b * (U1 - 1) + q.u];
            if (GRAD) {
                const float mP = hdr[2 * q.b];
                const int eP = __float_as_int(hdr[2 * q.b + 1]);
                const xf a = xf_unpack(wa[c]);
                const float4 e4 = em[c];
                xf pb, py;
                pb.m = e4.x; pb.e = __float_as_int(e4.y);
                py.m = e4.z; py.e = __float_as_int(e4.w);
                s.occ[m] = xf_to_float(xf_times(a, xf_unpack(wb[c])), eP) / mP;
                const xf bt = q.t + 1 < Tb ? xf_unpack(wb[c + U1]) : q.u == Ub ? xf_one() : xf_zero();
                s.fb[m] = xf_to_float(xf_times(xf_times(a, pb), bt), eP) / mP;
                s.fy[m] = q.u < Ub ? xf_to_float(xf_times(xf_times(a, py), xf_unpack(wb[c + 1])), eP) / mP : 0.0f;
                s.lse[m] = lse_in[c];
            }
        }
    }
    s.live[m] = live; s.y[m] = y; s.eoff[m] = eo; s.poff[m] = po;
}

__device__ __forceinline__ int ft_any_live(const FtTile &s) {
    int any = 0;
#pragma unroll
    for (int m = 0; m < FT_M; ++m) any |= s.live[m];
    return any;
}

// Zs[j][m] = act(enc + pred) of the tile's cells; a dead cell's row: zeros, its inputs never read
__device__ __forceinline__ void ft_build_z(float *Zs, const FtTile &s, const float *__restrict__ enc, const float *__restrict__ pred, int J,
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

__global__ __launch_bounds__(FT_THREADS) void rnnt_fused_forward_kernel(const float *__restrict__ enc, const float *__restrict__ pred,
                                                                        const float *__restrict__ W, int B, int T, int U1, int J, int V,
                                                                        int kind, int blank, const int *__restrict__ ints,
                                                                        float4 *__restrict__ em, double *__restrict__ lse_out, long cells,
                                                                        long tiles) {
    extern __shared__ __align__(16) float ft_smem[];
    float *Zs = ft_smem;
    __shared__ FtTile s;
    __shared__ float s_xb[FT_M], s_xy[FT_M], s_M[FT_WAVES][FT_M];
    __shared__ double s_S[FT_WAVES][FT_M];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, c = lane & 31, kk = lane >> 5;
    const float *bias = W + (long)J * V;
    for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        ft_tile_cells<false>(s, tile, cells, B, T, U1, ints, nullptr, nullptr, nullptr, nullptr, nullptr);
        __syncthreads();
        if (!ft_any_live(s)) { __syncthreads(); continue; }
        ft_build_z(Zs, s, enc, pred, J, kind);
        if (tid < FT_M) { s_xb[tid] = -INFINITY; s_xy[tid] = -INFINITY; }
        __syncthreads();
        float M[16];
        double S[16];
#pragma unroll
        for (int v = 0; v < 16; ++v) { M[v] = -INFINITY; S[v] = 0.0; }
        for (int n0 = wv * 32; n0 < V; n0 += FT_WAVES * 32) {
            const int col = n0 + c;
            const bool colv = col < V;
            const f32x16 acc = ft_logits(Zs, W, J, V, col, colv, c, kk);
            const float bv = colv ? bias[col] : 0.0f;
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int row = ft_row(v, kk);
                const float x = colv ? acc[v] + bv : -INFINITY;
                if (col == blank) s_xb[row] = x;
                if (col == s.y[row]) s_xy[row] = x;
                float mt = x;
#pragma unroll
                for (int off = 16; off > 0; off >>= 1) mt = fmaxf(mt, __shfl_xor(mt, off));
                if (mt > M[v]) {                                            // the same for the 32 lanes of a row
                    S[v] = M[v] > -INFINITY ? S[v] * exp((double)M[v] - (double)mt) : 0.0;
                    M[v] = mt;
                }
                S[v] += (double)expf(x - M[v]);
            }
        }
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            double t = S[v];
#pragma unroll
            for (int off = 16; off > 0; off >>= 1) t += __shfl_xor(t, off);
            if (c == 0) { s_M[wv][ft_row(v, kk)] = M[v]; s_S[wv][ft_row(v, kk)] = t; }
        }
        __syncthreads();
        if (tid < FT_M && s.live[tid]) {
            float mx = s_M[0][tid];
            for (int w = 1; w < FT_WAVES; ++w) mx = fmaxf(mx, s_M[w][tid]);
            double sum = 0.0;
            for (int w = 0; w < FT_WAVES; ++w)
                if (s_M[w][tid] > -INFINITY) sum += s_M[w][tid] == mx ? s_S[w][tid] : s_S[w][tid] * exp((double)s_M[w][tid] - (double)mx);
            const double lse = (double)mx + log(sum);
            const xf pb = rnnt_emission(s_xb[tid], lse);
            const xf py = s.y[tid] >= 0 ? rnnt_emission(s_xy[tid], lse) : xf_zero();
            const long cc = tile * FT_M + tid;
            em[cc] = make_float4(pb.m, __int_as_float(pb.e), py.m, __int_as_float(py.e));
            if (lse_out) lse_out[cc] = lse;
        }
        __syncthreads();
    }
}

// phase A of both backward kernels: wave `slot`'s logits block at columns n0 .. n0 + 31 -> g, transposed into Gs[slot * 32 + c][row]
__device__ __forceinline__ void ft_g_block(float *Gs, const float *Zs, const FtTile &s, const float *__restrict__ W, int J, int V, int blank,
                                           int slot, int n0, int c, int kk) {
    float *gp = Gs + (slot * 32 + c) * FT_PITCH;
    if (n0 >= V) {
#pragma unroll
        for (int v = 0; v < 16; ++v) gp[ft_row(v, kk)] = 0.0f;
        return;
    }
    const int col = n0 + c;
    const bool colv = col < V;
    const f32x16 acc = ft_logits(Zs, W, J, V, col, colv, c, kk);
    const float bv = colv ? W[(long)J * V + col] : 0.0f;
#pragma unroll
    for (int v = 0; v < 16; ++v) {
        const int row = ft_row(v, kk);
        const float x = acc[v] + bv;
        float r = s.occ[row] == 0.0f ? 0.0f : s.occ[row] * expf((float)((double)x - s.lse[row]));      // rnnt_grad_value's selection
        if (col == blank) r -= s.fb[row];
        if (col == s.y[row]) r -= s.fy[row];
        gp[row] = colv && s.live[row] ? r : 0.0f;
    }
}

__global__ __launch_bounds__(FT_THREADS) void rnnt_fused_dz_kernel(const float *__restrict__ enc, const float *__restrict__ pred,
                                                                   const float *__restrict__ W, const float *__restrict__ WT, int B, int T,
                                                                   int U1, int J, int V, int kind, int blank, const int *__restrict__ ints,
                                                                   const float4 *__restrict__ em, const double *__restrict__ lse_in,
                                                                   const float2 *__restrict__ wa, const float2 *__restrict__ wb,
                                                                   const float *__restrict__ hdr, float *__restrict__ dzt, long cells,
                                                                   long tiles, int gw) {
    extern __shared__ __align__(16) float ft_smem[];
    float *Zs = ft_smem, *Gs = ft_smem + (size_t)J * FT_PITCH;
    __shared__ FtTile s;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, c = lane & 31, kk = lane >> 5;
    for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        ft_tile_cells<true>(s, tile, cells, B, T, U1, ints, em, lse_in, wa, wb, hdr);
        __syncthreads();
        const long c0 = tile * FT_M;
        if (!ft_any_live(s)) {                                              // every element of d z is written: the reduction reads them all
            const long n = (cells - c0 < FT_M ? cells - c0 : FT_M) * J;
            for (long i = tid; i < n; i += FT_THREADS) dzt[c0 * J + i] = 0.0f;
            __syncthreads();
            continue;
        }
        ft_build_z(Zs, s, enc, pred, J, kind);
        __syncthreads();
        f32x16 acc[4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int v = 0; v < 16; ++v) acc[i][v] = 0.0f;
        for (int v0 = 0; v0 < V; v0 += gw * 32) {
            if (wv < gw) ft_g_block(Gs, Zs, s, W, J, V, blank, wv, v0 + wv * 32, c, kk);
            __syncthreads();
            const int left = (V - v0 + 31) & ~31, nv = left < gw * 32 ? left : gw * 32;
#pragma unroll 4
            for (int k = 0; k < nv; k += 2) {
                const float a = Gs[(k + kk) * FT_PITCH + c];
                const int vr = v0 + k + kk;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int jb = (wv + FT_WAVES * i) * 32;
                    if (jb < J) {
                        const float b = vr < V && jb + c < J ? WT[(long)vr * J + jb + c] : 0.0f;
                        acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc[i], 0, 0, 0);
                    }
                }
            }
            __syncthreads();
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int jc = (wv + FT_WAVES * i) * 32 + c;
            if (jc < J) {
#pragma unroll
                for (int v = 0; v < 16; ++v) {
                    const int row = ft_row(v, kk);
                    if (c0 + row < cells) dzt[(c0 + row) * J + jc] = s.live[row] ? acc[i][v] * rnnt_dact(kind, Zs[jc * FT_PITCH + row]) : 0.0f;
                }
            }
        }
        __syncthreads();
    }
}

template <int NJB>
__global__ __launch_bounds__(FT_THREADS) void rnnt_fused_dw_kernel(const float *__restrict__ enc, const float *__restrict__ pred,
                                                                   const float *__restrict__ W, int B, int T, int U1, int J, int V, int kind,
                                                                   int blank, const int *__restrict__ ints, const float4 *__restrict__ em,
                                                                   const double *__restrict__ lse_in, const float2 *__restrict__ wa,
                                                                   const float2 *__restrict__ wb, const float *__restrict__ hdr,
                                                                   float *__restrict__ partial, long cells, long tiles) {
    constexpr int NB = 4 / NJB, VTW = 32 * NB;
    extern __shared__ __align__(16) float ft_smem[];
    float *Zs = ft_smem, *Gs = ft_smem + (size_t)J * FT_PITCH;
    __shared__ FtTile s;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, c = lane & 31, kk = lane >> 5;
    const int v0 = blockIdx.x * VTW;
    const long t0 = tiles * blockIdx.y / gridDim.y, t1 = tiles * (blockIdx.y + 1) / gridDim.y;
    f32x16 acc[NJB][NB];
#pragma unroll
    for (int i = 0; i < NJB; ++i)
#pragma unroll
        for (int n = 0; n < NB; ++n)
#pragma unroll
            for (int v = 0; v < 16; ++v) acc[i][n][v] = 0.0f;
    float bs = 0.0f;
    for (long tile = t0; tile < t1; ++tile) {
        ft_tile_cells<true>(s, tile, cells, B, T, U1, ints, em, lse_in, wa, wb, hdr);
        __syncthreads();
        if (!ft_any_live(s)) { __syncthreads(); continue; }
        ft_build_z(Zs, s, enc, pred, J, kind);
        __syncthreads();
        if (wv < NB) ft_g_block(Gs, Zs, s, W, J, V, blank, wv, v0 + wv * 32, c, kk);
        __syncthreads();
#pragma unroll 4
        for (int k = 0; k < FT_M; k += 2) {
            float b[NB];
#pragma unroll
            for (int n = 0; n < NB; ++n) b[n] = Gs[(n * 32 + c) * FT_PITCH + k + kk];
#pragma unroll
            for (int i = 0; i < NJB; ++i) {
                const int jb = (wv + FT_WAVES * i) * 32;
                if (jb < J) {
                    const float a = jb + c < J ? Zs[(jb + c) * FT_PITCH + k + kk] : 0.0f;
#pragma unroll
                    for (int n = 0; n < NB; ++n) acc[i][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b[n], acc[i][n], 0, 0, 0);
                }
            }
        }
        if (tid < VTW) {                                                    // d b: the column's sum over the tile's cells, ascending
            float t = 0.0f;
#pragma unroll
            for (int m = 0; m < FT_M; ++m) t += Gs[tid * FT_PITCH + m];
            bs += t;
        }
        __syncthreads();
    }
    float *dst = partial + (size_t)blockIdx.y * ((size_t)J + 1) * V;
#pragma unroll
    for (int i = 0; i < NJB; ++i) {
        const int jb = (wv + FT_WAVES * i) * 32;
#pragma unroll
        for (int n = 0; n < NB; ++n) {
            const int col = v0 + n * 32 + c;
            if (col >= V) continue;
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int j = jb + ft_row(v, kk);
                if (j < J) dst[(size_t)j * V + col] = acc[i][n][v];
            }
        }
    }
    if (tid < VTW && v0 + tid < V) dst[(size_t)J * V + v0 + tid] = bs;
}

__global__ __launch_bounds__(256) void rnnt_fused_dw_reduce_kernel(const float *__restrict__ partial, float *__restrict__ dout, long n, int np) {
    for (long e = blockIdx.x * 256L + threadIdx.x; e < n; e += gridDim.x * 256L) {
        float t = partial[e];
        for (int p = 1; p < np; ++p) t += partial[(size_t)p * n + e];
        dout[e] = t;
    }
}

// WT[v][j] = W[j][v]
__global__ __launch_bounds__(256) void rnnt_fused_transpose_kernel(const float *__restrict__ W, float *__restrict__ WT, int J, int V) {
    __shared__ float t[32][33];
    const int x = threadIdx.x & 31, y = threadIdx.x >> 5;
    const int v0 = blockIdx.x * 32, j0 = blockIdx.y * 32;
    for (int r = y; r < 32; r += 8)
        if (j0 + r < J && v0 + x < V) t[r][x] = W[(long)(j0 + r) * V + v0 + x];
    __syncthreads();
    for (int r = y; r < 32; r += 8)
        if (v0 + r < V && j0 + x < J) WT[(long)(v0 + r) * J + j0 + x] = t[x][r];
}

// the emissions from the joiner's inputs, for this unit and for rnnt_align.hip; lse NULL: not kept (the loss-only form)
int nntk_rnnt_fused_emit_launch(const float *d_enc, const float *d_pred, const float *d_out, int B, int T, int U1, int J, int V, int kind,
                                int blank, const int *d_ints, float4 *em, double *lse) {
    const long cells = (long)B * T * U1, tiles = (cells + FT_M - 1) / FT_M;
    const size_t zbytes = (size_t)J * FT_PITCH * sizeof(float);
    if (zbytes > 48 * 1024 && nntk_set_max_dynamic_lds((const void *)rnnt_fused_forward_kernel, zbytes)) return -1;
    hipLaunchKernelGGL(rnnt_fused_forward_kernel, dim3(rnnt_grid(tiles, 1)), dim3(FT_THREADS), zbytes, nntk_stream(), d_enc, d_pred, d_out, B,
                       T, U1, J, V, kind, blank, d_ints, em, lse, cells, tiles);
    NNTK_LAUNCH_CHECK("rnnt_fused_forward_kernel");
    return 0;
}

extern "C" {

size_t nntk_shim_rnnt_fused_workspace_floats(int batch, int T, int max_label_len, int J, int V, int want_grad) {
    return ft_layout(batch, T, max_label_len, J, V, want_grad).total;
}

int nntk_shim_rnnt_fused_loss(const float *d_enc, const float *d_pred, const float *d_out, int B, int T, int J, int V, int kind,
                              const int *h_input_lengths, const int *h_labels, const int *h_label_lengths, int maxL, int blank,
                              float *d_loss_rows, float *d_denc, float *d_dpred, float *d_dout, float *d_ws) {
    if (B <= 0) return 0;
    if (!rnnt_fused_fits(T, maxL, J, V, d_ws))
        return nntk_fail_msg("nntk_rnnt_fused_loss_device: a shape beyond the kernels' limits or a misaligned workspace");
    const bool grad = d_dout != nullptr;
    const int U1 = maxL + 1;
    const FtLayout lay = ft_layout(B, T, maxL, J, V, grad);
    const long cells = (long)B * T * U1, tiles = (cells + FT_M - 1) / FT_M;
    const RnntParts w = rnnt_parts(d_ws, lay.base, grad);
    if (rnnt_upload_ints(w.ints, B, maxL, h_input_lengths, h_labels, h_label_lengths)) return -1;
    const size_t zbytes = (size_t)J * FT_PITCH * sizeof(float);
    if (nntk_rnnt_fused_emit_launch(d_enc, d_pred, d_out, B, T, U1, J, V, kind, blank, w.ints, w.em, w.lse)) return -1;
    if (nntk_rnnt_lattice_launch(B, T, U1, w.ints, w.em, w.alpha, w.beta, w.hdr, d_loss_rows)) return -1;
    if (!grad) return 0;
    float *wt = d_ws + lay.wt, *partial = d_ws + lay.partial, *dzt = d_ws + lay.dz;
    hipLaunchKernelGGL(rnnt_fused_transpose_kernel, dim3((unsigned)((V + 31) / 32), (unsigned)((J + 31) / 32)), dim3(256), 0, nntk_stream(),
                       d_out, wt, J, V);
    NNTK_LAUNCH_CHECK("rnnt_fused_transpose_kernel");
    const int gw = J <= FT_GW_WIDE_MAX_J ? 8 : 4;
    const size_t dzbytes = zbytes + (size_t)gw * 32 * FT_PITCH * sizeof(float);
    if (dzbytes > 48 * 1024 && nntk_set_max_dynamic_lds((const void *)rnnt_fused_dz_kernel, dzbytes)) return -1;
    hipLaunchKernelGGL(rnnt_fused_dz_kernel, dim3(rnnt_grid(tiles, 1)), dim3(FT_THREADS), dzbytes, nntk_stream(), d_enc, d_pred, d_out, wt, B, T,
                       U1, J, V, kind, blank, w.ints, w.em, w.lse, w.alpha, w.beta, w.hdr, dzt, cells, tiles, gw);
    NNTK_LAUNCH_CHECK("rnnt_fused_dz_kernel");
    const int vtw = 32 * (4 / lay.njb);
    const dim3 wgrid((unsigned)((V + vtw - 1) / vtw), (unsigned)lay.np);
    const size_t dwbytes = zbytes + (size_t)vtw * FT_PITCH * sizeof(float);
#define FT_DW(NJB)                                                                                                                   \
    do {                                                                                                                             \
        if (dwbytes > 48 * 1024 && nntk_set_max_dynamic_lds((const void *)rnnt_fused_dw_kernel<NJB>, dwbytes)) return -1;             \
        hipLaunchKernelGGL(rnnt_fused_dw_kernel<NJB>, wgrid, dim3(FT_THREADS), dwbytes, nntk_stream(), d_enc, d_pred, d_out, B, T, U1, J, V, \
                           kind, blank, w.ints, w.em, w.lse, w.alpha, w.beta, w.hdr, partial, cells, tiles);                         \
    } while (0)
    if (lay.njb == 1) FT_DW(1);
    else if (lay.njb == 2) FT_DW(2);
    else FT_DW(4);
#undef FT_DW
    NNTK_LAUNCH_CHECK("rnnt_fused_dw_kernel");
    const long nw = ((long)J + 1) * V;
    hipLaunchKernelGGL(rnnt_fused_dw_reduce_kernel, dim3(rnnt_grid(nw, 256)), dim3(256), 0, nntk_stream(), partial, d_dout, nw, lay.np);
    NNTK_LAUNCH_CHECK("rnnt_fused_dw_reduce_kernel");
    // d_enc = the sum over u, d_pred = the sum over t of d z act'(z), which already holds the activation's factor: identity here
    return nntk_shim_rnnt_joint_backward(nullptr, dzt, B, T, U1, J, 0, d_denc, d_dpred);
}

}  // extern "C"
