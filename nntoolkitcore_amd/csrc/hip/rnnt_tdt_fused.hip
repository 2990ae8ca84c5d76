// rnnt_tdt_fused.hip -- the token-and-duration transducer (TDT) training loss straight from the joiner's inputs: with
// logits[b][t][u] = act(enc[b][t] + pred[b][u]) W + b, W [J][V + D] -- V token columns, then D duration columns, the block
// nntk_rnnt_tdt_decoder_create takes -- the loss rows of rnnt_tdt.hip and the gradients of their plain sum with respect to enc, pred and
// W | b.  Neither the [B][T][U1][V + D] scores nor their gradient ever exist in memory.
//
// The frame is rnnt_fused.hip's (rnnt_fused_common.hpp): tiles of FT_M = 32 consecutive cells, z = act(enc + pred) built once per tile in
// LDS, transposed at pitch 33, a dead cell's row selected to zero, exact-f32 v_mfma_f32_32x32x2_f32 products, a logit one k-ordered fmaf
// chain over j (ft_logits) that is the same in all three kernels.  What is this unit's own is TWO HEADS IN ONE MATRIX: the V + D columns
// are walked as one sequence of 32-column blocks, and a block may be all tokens, all durations, or both.
//
//  rnnt_tdt_fused_forward_kernel, a 512-lane workgroup per tile: wave w takes the column blocks w, w + 8, ... of V + D.  A lane's
//    column is a token (col < V) or a duration; the token head keeps rnnt_fused.hip's running (max, sum in double) per cell, a
//    duration column masked out of it (-inf into the butterfly, nothing into the sum; a block past V skips the head altogether).  The
//    D <= 8 duration columns sit in one block or straddle two -- two waves, or two passes of one wave -- so nothing is reduced across
//    lanes for them: the lane that holds column V + i hands its logit to LDS as x_dur[i][cell], exactly as the blank's and the label's
//    logits are handed over.  After the waves' merge the per-cell lane forms lse_dur from those D values alone: exact maximum, expf per
//    element, the sum in double with i ascending.  Written: what tdt_emit_kernel writes, into tdt_layout: em (16 B per cell, sigma in
//    the two token emissions), pdur (8 B per duration per cell) and, with a gradient, the (lse_tok, lse_dur) pair.
//  tdt_lattice_kernel: rnnt_tdt.hip's, unchanged, on those emissions (nntk_rnnt_tdt_lattice_launch).
//  rnnt_tdt_fused_dz_kernel / rnnt_tdt_fused_dw_kernel<NJB>: rnnt_fused.hip's two backward kernels on V + D columns.  The tile record
//    carries per cell the occupancy, the two token flows, both lse and -- in the dynamic LDS, D x 32 floats -- the D duration flows, all
//    from tdt_cell_flows by one lane per cell (over P, the terminal move included).  Phase A recomputes a logits block and forms
//    tdt_grad_value's g, transposed in LDS: a token column occ exp(x - lse_tok) - [blank] F_blank - [label] F_label, a duration column
//    occ exp(x - lse_dur) - F_dur(i).  d z += g W^T over groups of gw column blocks, each 32-column block summed on its own and then
//    added to the total; d W | d b per (column group, tile slice), 32 partial blocks added in order; rnnt_joint_reduce_kernel gives d_enc and d_pred.  A tile whose cells are all dead or all in rows with P = 0
//    zero-fills its d z and adds nothing to d W.
// LDS: z is J x 33 floats, g gw x 32 x 33 (d z) or 128 / NJB x 33 (d W), x_dur / F_dur D x 32; tf_lds_bytes sums them with the static
// part, and the entry refuses a (J, D) beyond one workgroup's LDS on the host.  J = 1024, D = 8: 154.4 of 160 KiB.
// No atomics; every sum has a fixed order; a cell's scalars and its d z depend on nothing but the cell.
#include "rnnt_tdt_common.hpp"
#include "rnnt_fused_common.hpp"

// workspace: tdt_layout (the loss's own, unchanged), then with a gradient d z act' [cells][J], W^T [V + D][J], FT_NP blocks [J + 1][V + D]
struct TfLayout { TdtLayout base; size_t dz, wt, partial, total; int njb; };
static TfLayout tf_layout(int B, int T, int maxL, int J, int V, int D, int want_grad) {
    TfLayout l;
    auto up = [](size_t x) { return (x + 3) & ~(size_t)3; };
    const size_t j = J > 0 ? (size_t)J : 0, vd = (V > 0 ? (size_t)V : 0) + (D > 0 ? (size_t)D : 0);
    const size_t cells = (size_t)(B > 0 ? B : 0) * (size_t)(T > 0 ? T : 0) * ((size_t)(maxL > 0 ? maxL : 0) + 1);
    l.base = tdt_layout(B, T, maxL, D, want_grad);
    l.njb = ft_njb(J);
    l.dz = l.base.total;                                                     // a multiple of 4 words
    l.wt = l.dz + (want_grad ? up(cells * j) : 0);
    l.partial = l.wt + (want_grad ? up(j * vd) : 0);
    l.total = l.partial + (want_grad ? up((size_t)FT_NP * (j + 1) * vd) : 0);
    return l;
}

struct TfTile {                            // one tile's cells, in LDS; the D duration flows: Fd[i][m], dynamic
    long eoff[FT_M], poff[FT_M];           // rows of enc and pred
    double lse_t[FT_M], lse_d[FT_M];
    float occ[FT_M], fb[FT_M], fy[FT_M];   // occupancy alpha beta / P and the two token flows (tdt_cell_flows)
    int live[FT_M], y[FT_M];               // y: the next label, -1 where there is none
};

// the kernels' LDS, sized explicitly: the static part (the tile record; forwards also the two handed-over logits and the waves' pairs)
// and the dynamic part in floats: z, the g blocks, x_dur or F_dur
#define TF_STATIC_BYTES (sizeof(TfTile) + 2 * FT_M * sizeof(float) + FT_WAVES * FT_M * (sizeof(float) + sizeof(double)))
static inline int tf_gw(int J) { return J <= FT_GW_WIDE_MAX_J ? 8 : 4; }
static inline size_t tf_dyn_bytes(int J, int D, int gblocks) {
    return ((size_t)J * FT_PITCH + (size_t)gblocks * 32 * FT_PITCH + (size_t)D * FT_M) * sizeof(float);
}
static inline size_t tf_lds_bytes(int J, int D) {                            // the largest of the three kernels: d z's
    const int dwb = 4 / ft_njb(J), g = tf_gw(J) > dwb ? tf_gw(J) : dwb;
    return TF_STATIC_BYTES + tf_dyn_bytes(J, D, g);
}

// GRAD: a cell of a row with P = 0 counts as dead, and the gradient's scalars are worked out.  Returns nothing; barrier after.
template <bool GRAD>
__device__ __forceinline__ void tf_tile_cells(TfTile &s, float *Fd, long tile, long cells, int B, int T, int U1, const TdtDur &dur,
                                              const int *__restrict__ ints, const float4 *__restrict__ em, const float2 *__restrict__ pdur,
                                              const double *__restrict__ lse_in, const float2 *__restrict__ wa,
                                              const float2 *__restrict__ wb, const float *__restrict__ hdr) {
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
                const TdtFlows f = tdt_cell_flows(c, q.t, q.u, Tb, Ub, U1, dur, em, pdur, wa, wb, hdr[2 * q.b], __float_as_int(hdr[2 * q.b + 1]));
                s.occ[m] = f.tok.occ; s.fb[m] = f.tok.fb; s.fy[m] = f.tok.fy;
#pragma unroll
                for (int i = 0; i < TDT_MAXD; ++i)
                    if (i < dur.n) Fd[i * FT_M + m] = f.fd[i];
                s.lse_t[m] = lse_in[2 * c];
                s.lse_d[m] = lse_in[2 * c + 1];
            }
        }
    }
    s.live[m] = live; s.y[m] = y; s.eoff[m] = eo; s.poff[m] = po;
}

__global__ __launch_bounds__(FT_THREADS) void rnnt_tdt_fused_forward_kernel(const float *__restrict__ enc, const float *__restrict__ pred,
                                                                            const float *__restrict__ W, int B, int T, int U1, int J, int V,
                                                                            int D, int kind, int blank, float sigma,
                                                                            const int *__restrict__ ints, float4 *__restrict__ em,
                                                                            float2 *__restrict__ pdur, double *__restrict__ lse_out,
                                                                            long cells, long tiles) {
    extern __shared__ __align__(16) float tf_smem[];
    float *Zs = tf_smem, *Xd = tf_smem + (size_t)J * FT_PITCH;             // Xd[i][cell]: the duration head's logits
    __shared__ TfTile s;
    __shared__ float s_xb[FT_M], s_xy[FT_M], s_M[FT_WAVES][FT_M];
    __shared__ double s_S[FT_WAVES][FT_M];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, c = lane & 31, kk = lane >> 5;
    const int VD = V + D;
    const float *bias = W + (long)J * VD;
    const TdtDur nodur = {};
    for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        tf_tile_cells<false>(s, nullptr, tile, cells, B, T, U1, nodur, ints, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
        __syncthreads();
        if (!ft_any_live(s)) { __syncthreads(); continue; }
        ft_build_z(Zs, s, enc, pred, J, kind);
        if (tid < FT_M) { s_xb[tid] = -INFINITY; s_xy[tid] = -INFINITY; }
        __syncthreads();
        float M[16];
        double S[16];
#pragma unroll
        for (int v = 0; v < 16; ++v) { M[v] = -INFINITY; S[v] = 0.0; }
        for (int n0 = wv * 32; n0 < VD; n0 += FT_WAVES * 32) {
            const int col = n0 + c;
            const bool colv = col < VD, tok = col < V;
            const f32x16 acc = ft_logits(Zs, W, J, VD, col, colv, c, kk);
            const float bv = colv ? bias[col] : 0.0f;
            if (colv && !tok) {                                             // a duration column: its 32 cells' logits, handed over
#pragma unroll
                for (int v = 0; v < 16; ++v) Xd[(col - V) * FT_M + ft_row(v, kk)] = acc[v] + bv;
            }
            if (n0 >= V) continue;                                          // a block without a token: uniform over the wave
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int row = ft_row(v, kk);
                const float x = tok ? acc[v] + bv : -INFINITY;
                if (col == blank) s_xb[row] = x;
                if (col == s.y[row]) s_xy[row] = x;
                float mt = x;
#pragma unroll
                for (int off = 16; off > 0; off >>= 1) mt = fmaxf(mt, __shfl_xor(mt, off));
                if (mt > M[v]) {                                            // the same for the 32 lanes of a row
                    S[v] = M[v] > -INFINITY ? S[v] * exp((double)M[v] - (double)mt) : 0.0;
                    M[v] = mt;
                }
                S[v] += (double)expf(x - M[v]);                             // the block holds a token, so M[v] is one's logit
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
            const double lse_t = (double)mx + log(sum);
            float md = Xd[tid];
            for (int i = 1; i < D; ++i) md = fmaxf(md, Xd[i * FT_M + tid]);
            double sd = 0.0;
            for (int i = 0; i < D; ++i) sd += (double)expf(Xd[i * FT_M + tid] - md);
            const double lse_d = (double)md + log(sd);
            const long cc = tile * FT_M + tid;
            for (int i = 0; i < D; ++i) pdur[cc * D + i] = xf_pack(rnnt_emission(Xd[i * FT_M + tid], lse_d));
            const double ls = lse_t + (double)sigma;                        // sigma = 0: lse_t itself
            const xf pb = rnnt_emission(s_xb[tid], ls);
            const xf py = s.y[tid] >= 0 ? rnnt_emission(s_xy[tid], ls) : xf_zero();
            em[cc] = make_float4(pb.m, __int_as_float(pb.e), py.m, __int_as_float(py.e));
            if (lse_out) {
                lse_out[2 * cc] = lse_t;
                lse_out[2 * cc + 1] = lse_d;
            }
        }
        __syncthreads();
    }
}

// phase A of both backward kernels: wave `slot`'s logits block at columns n0 .. n0 + 31 of V + D -> g, transposed into
// Gs[slot * 32 + c][row]; tdt_grad_value's formula, a lane's column one head or the other
__device__ __forceinline__ void tf_g_block(float *Gs, const float *Zs, const float *Fd, const TfTile &s, const float *__restrict__ W, int J,
                                           int V, int VD, int blank, int slot, int n0, int c, int kk) {
    float *gp = Gs + (slot * 32 + c) * FT_PITCH;
    if (n0 >= VD) {
#pragma unroll
        for (int v = 0; v < 16; ++v) gp[ft_row(v, kk)] = 0.0f;
        return;
    }
    const int col = n0 + c;
    const bool colv = col < VD, tok = col < V;
    const f32x16 acc = ft_logits(Zs, W, J, VD, col, colv, c, kk);
    const float bv = colv ? W[(long)J * VD + col] : 0.0f;
    const float *fd = Fd + (colv && !tok ? col - V : 0) * FT_M;
#pragma unroll
    for (int v = 0; v < 16; ++v) {
        const int row = ft_row(v, kk);
        const float x = acc[v] + bv;
        const double lse = tok ? s.lse_t[row] : s.lse_d[row];
        float r = s.occ[row] == 0.0f ? 0.0f : s.occ[row] * expf((float)((double)x - lse));             // the selected zero
        if (tok) {
            if (col == blank) r -= s.fb[row];
            if (col == s.y[row]) r -= s.fy[row];
        } else {
            r -= fd[row];
        }
        gp[row] = colv && s.live[row] ? r : 0.0f;
    }
}

__global__ __launch_bounds__(FT_THREADS) void rnnt_tdt_fused_dz_kernel(const float *__restrict__ enc, const float *__restrict__ pred,
                                                                       const float *__restrict__ W, const float *__restrict__ WT, int B,
                                                                       int T, int U1, int J, int V, const TdtDur dur, int kind, int blank,
                                                                       const int *__restrict__ ints, const float4 *__restrict__ em,
                                                                       const float2 *__restrict__ pdur, const double *__restrict__ lse_in,
                                                                       const float2 *__restrict__ wa, const float2 *__restrict__ wb,
                                                                       const float *__restrict__ hdr, float *__restrict__ dzt, long cells,
                                                                       long tiles, int gw) {
    extern __shared__ __align__(16) float tf_smem[];
    float *Zs = tf_smem, *Gs = Zs + (size_t)J * FT_PITCH, *Fd = Gs + (size_t)gw * 32 * FT_PITCH;
    __shared__ TfTile s;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, c = lane & 31, kk = lane >> 5;
    const int VD = V + dur.n;
    for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        tf_tile_cells<true>(s, Fd, tile, cells, B, T, U1, dur, ints, em, pdur, lse_in, wa, wb, hdr);
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
        for (int v0 = 0; v0 < VD; v0 += gw * 32) {
            if (wv < gw) tf_g_block(Gs, Zs, Fd, s, W, J, V, VD, blank, wv, v0 + wv * 32, c, kk);
            __syncthreads();
            const int left = (VD - v0 + 31) & ~31, nv = left < gw * 32 ? left : gw * 32;
            // two levels: a 32-column block is summed on its own (16 MFMA steps) and then added to the total.  One chain over all
            // V + D columns rounds every step at the size of the running sum, which the blank's -F_blank W sets early: measured
            // 7.8e-7 of the row's largest |d z| at V + D = 305, against 10 block sums' roundings here
            for (int k0 = 0; k0 < nv; k0 += 32) {
                f32x16 blk[4];
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int v = 0; v < 16; ++v) blk[i][v] = 0.0f;
#pragma unroll 4
                for (int k = k0; k < k0 + 32; k += 2) {
                    const float a = Gs[(k + kk) * FT_PITCH + c];
                    const int vr = v0 + k + kk;
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int jb = (wv + FT_WAVES * i) * 32;
                        if (jb < J) {
                            const float b = vr < VD && jb + c < J ? WT[(long)vr * J + jb + c] : 0.0f;
                            blk[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, blk[i], 0, 0, 0);
                        }
                    }
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[i] += blk[i];
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
__global__ __launch_bounds__(FT_THREADS) void rnnt_tdt_fused_dw_kernel(const float *__restrict__ enc, const float *__restrict__ pred,
                                                                       const float *__restrict__ W, int B, int T, int U1, int J, int V,
                                                                       const TdtDur dur, int kind, int blank, const int *__restrict__ ints,
                                                                       const float4 *__restrict__ em, const float2 *__restrict__ pdur,
                                                                       const double *__restrict__ lse_in, const float2 *__restrict__ wa,
                                                                       const float2 *__restrict__ wb, const float *__restrict__ hdr,
                                                                       float *__restrict__ partial, long cells, long tiles) {
    constexpr int NB = 4 / NJB, VTW = 32 * NB;
    extern __shared__ __align__(16) float tf_smem[];
    float *Zs = tf_smem, *Gs = Zs + (size_t)J * FT_PITCH, *Fd = Gs + VTW * FT_PITCH;
    __shared__ TfTile s;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, c = lane & 31, kk = lane >> 5;
    const int VD = V + dur.n, v0 = blockIdx.x * VTW;
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
        tf_tile_cells<true>(s, Fd, tile, cells, B, T, U1, dur, ints, em, pdur, lse_in, wa, wb, hdr);
        __syncthreads();
        if (!ft_any_live(s)) { __syncthreads(); continue; }
        ft_build_z(Zs, s, enc, pred, J, kind);
        __syncthreads();
        if (wv < NB) tf_g_block(Gs, Zs, Fd, s, W, J, V, VD, blank, wv, v0 + wv * 32, c, kk);
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
    float *dst = partial + (size_t)blockIdx.y * ((size_t)J + 1) * VD;
#pragma unroll
    for (int i = 0; i < NJB; ++i) {
        const int jb = (wv + FT_WAVES * i) * 32;
#pragma unroll
        for (int n = 0; n < NB; ++n) {
            const int col = v0 + n * 32 + c;
            if (col >= VD) continue;
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int j = jb + ft_row(v, kk);
                if (j < J) dst[(size_t)j * VD + col] = acc[i][n][v];
            }
        }
    }
    if (tid < VTW && v0 + tid < VD) dst[(size_t)J * VD + v0 + tid] = bs;
}

// the emissions of both heads from the joiner's inputs, for this unit and for an aligner to come; lse NULL: not kept
int nntk_rnnt_tdt_fused_emit_launch(const float *d_enc, const float *d_pred, const float *d_out, int B, int T, int U1, int J, int V, int D,
                                    int kind, int blank, float sigma, const int *d_ints, float4 *em, float2 *pdur, double *lse) {
    const long cells = (long)B * T * U1, tiles = (cells + FT_M - 1) / FT_M;
    const size_t lds = tf_dyn_bytes(J, D, 0);
    if (lds > 48 * 1024 && nntk_set_max_dynamic_lds((const void *)rnnt_tdt_fused_forward_kernel, lds)) return -1;
    hipLaunchKernelGGL(rnnt_tdt_fused_forward_kernel, dim3(rnnt_grid(tiles, 1)), dim3(FT_THREADS), lds, nntk_stream(), d_enc, d_pred, d_out, B,
                       T, U1, J, V, D, kind, blank, sigma, d_ints, em, pdur, lse, cells, tiles);
    NNTK_LAUNCH_CHECK("rnnt_tdt_fused_forward_kernel");
    return 0;
}

extern "C" {

size_t nntk_shim_rnnt_tdt_fused_workspace_floats(int batch, int T, int max_label_len, int J, int V, int n_durations, int want_grad) {
    return tf_layout(batch, T, max_label_len, J, V, n_durations, want_grad).total;
}

size_t nntk_shim_rnnt_tdt_fused_lds_bytes(int J, int n_durations) { return tf_lds_bytes(J, n_durations); }

int nntk_shim_rnnt_tdt_fused_loss(const float *d_enc, const float *d_pred, const float *d_out, int B, int T, int J, int V,
                                  const int *h_durations, int D, int kind, const int *h_input_lengths, const int *h_labels,
                                  const int *h_label_lengths, int maxL, int blank, float sigma, float *d_loss_rows, float *d_denc,
                                  float *d_dpred, float *d_dout, float *d_ws) {
    if (B <= 0) return 0;
    static_assert(NNTK_RNNT_TDT_LDS_BYTES <= CTC_LDS_LIMIT, "the kernels' budget is one workgroup's LDS");
    if (!tdt_fits(T, maxL, h_durations, D) || J < 1 || J > NNTK_RNNT_FUSED_MAX_J || V < 2 || V > NNTK_RNNT_FUSED_MAX_V ||
        tf_lds_bytes(J, D) > NNTK_RNNT_TDT_LDS_BYTES || ((uintptr_t)d_ws & 15) != 0)
        return nntk_fail_msg("nntk_rnnt_tdt_fused_loss_device: a shape beyond the kernels' limits or a misaligned workspace");
    const bool grad = d_dout != nullptr;
    const int U1 = maxL + 1, VD = V + D;
    const TfLayout lay = tf_layout(B, T, maxL, J, V, D, grad);
    const long cells = (long)B * T * U1, tiles = (cells + FT_M - 1) / FT_M;
    int *ints = (int *)d_ws;
    float *hdr = d_ws + lay.base.hdr;
    float4 *em = (float4 *)(d_ws + lay.base.em);
    float2 *pdur = (float2 *)(d_ws + lay.base.dur);
    double *lse = grad ? (double *)(d_ws + lay.base.lse) : nullptr;
    float2 *wa = grad ? (float2 *)(d_ws + lay.base.alpha) : nullptr, *wb = grad ? (float2 *)(d_ws + lay.base.beta) : nullptr;
    const TdtDur dur = tdt_dur(h_durations, D);
    if (rnnt_upload_ints(ints, B, maxL, h_input_lengths, h_labels, h_label_lengths)) return -1;
    if (nntk_rnnt_tdt_fused_emit_launch(d_enc, d_pred, d_out, B, T, U1, J, V, D, kind, blank, sigma, ints, em, pdur, lse)) return -1;
    if (nntk_rnnt_tdt_lattice_launch(B, T, U1, dur, ints, em, pdur, wa, wb, hdr, d_loss_rows)) return -1;
    if (!grad) return 0;
    float *dzt = d_ws + lay.dz, *wt = d_ws + lay.wt, *partial = d_ws + lay.partial;
    if (nntk_rnnt_fused_transpose_launch(d_out, wt, J, VD)) return -1;
    const int gw = tf_gw(J);
    const size_t dzbytes = tf_dyn_bytes(J, D, gw);
    if (dzbytes > 48 * 1024 && nntk_set_max_dynamic_lds((const void *)rnnt_tdt_fused_dz_kernel, dzbytes)) return -1;
    hipLaunchKernelGGL(rnnt_tdt_fused_dz_kernel, dim3(rnnt_grid(tiles, 1)), dim3(FT_THREADS), dzbytes, nntk_stream(), d_enc, d_pred, d_out, wt, B,
                       T, U1, J, V, dur, kind, blank, ints, em, pdur, lse, wa, wb, hdr, dzt, cells, tiles, gw);
    NNTK_LAUNCH_CHECK("rnnt_tdt_fused_dz_kernel");
    const int nb = 4 / lay.njb, vtw = 32 * nb;
    const dim3 wgrid((unsigned)((VD + vtw - 1) / vtw), (unsigned)FT_NP);
    const size_t dwbytes = tf_dyn_bytes(J, D, nb);
#define TF_DW(NJB)                                                                                                                       \
    do {                                                                                                                                 \
        if (dwbytes > 48 * 1024 && nntk_set_max_dynamic_lds((const void *)rnnt_tdt_fused_dw_kernel<NJB>, dwbytes)) return -1;             \
        hipLaunchKernelGGL(rnnt_tdt_fused_dw_kernel<NJB>, wgrid, dim3(FT_THREADS), dwbytes, nntk_stream(), d_enc, d_pred, d_out, B, T, U1, J, \
                           V, dur, kind, blank, ints, em, pdur, lse, wa, wb, hdr, partial, cells, tiles);                                \
    } while (0)
    if (lay.njb == 1) TF_DW(1);
    else if (lay.njb == 2) TF_DW(2);
    else TF_DW(4);
#undef TF_DW
    NNTK_LAUNCH_CHECK("rnnt_tdt_fused_dw_kernel");
    if (nntk_rnnt_fused_dw_reduce_launch(partial, d_dout, ((long)J + 1) * VD, FT_NP)) return -1;
    // d_enc = the sum over u, d_pred = the sum over t of d z act'(z), which already holds the activation's factor: identity here
    return nntk_shim_rnnt_joint_backward(nullptr, dzt, B, T, U1, J, 0, d_denc, d_dpred);
}

}  // extern "C"
