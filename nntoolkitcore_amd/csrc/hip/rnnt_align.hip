// rnnt_align.hip -- RNN-Transducer forced alignment: given a row's labels, the single most probable path through its lattice (Viterbi:
// the max twin of rnnt.hip's alpha recursion), as the frame in which every label is emitted, the label count at which every frame is
// left, the natural log of every emission on the path, and the natural log of the path's probability.  It runs on the 16 bytes per
// cell that either emission writer leaves: rnnt_emit_kernel (rnnt.hip, stored scores) or rnnt_fused_forward_kernel (rnnt_fused.hip,
// the joiner's inputs, no score tensor in memory).
//
// Range.  The best path's probability falls like V^-(T + U): every Viterbi variable is an xf (ctc_xf.hpp), as the emissions are.  A step
// is one multiply per outgoing move and one xf comparison: max never rounds, there is no add and no transcendental on the dependent
// chain, and the relative error of a variable is at most (t + u) 2^-24.
//
// Tie-break (part of the contract): into cell (t, u) the candidates are taken in the order v(t-1, u) p_blank(t-1, u) (the blank move),
// v(t, u-1) p_label(t, u-1) (the label move); the label move replaces the blank move only if it is strictly greater.
//
// Work split.  rnnt_viterbi_kernel<NJ>: one 256-lane workgroup per row walks the anti-diagonals n = t + u upwards, lanes over u -- the
// frame of rnnt_lattice_kernel<NJ>, direction 0: the previous diagonal in double-buffered LDS, one LDS-only barrier per diagonal, the
// next diagonal's emissions loaded before the barrier, so those loads and this diagonal's backpointer stores stay in flight across
// it.  What is stored per live cell is one byte, the move taken into it (0 blank, 1 label), laid out by diagonal: cell (t, u) of row b
// sits at ((b ND + n) P + u - max(0, n - (T - 1))) with ND = T + max_label_len diagonals of P = min(T, max_label_len + 1) bytes, so a
// wavefront's stores of one diagonal are 64 contiguous bytes (cell-major they would stride by max_label_len).  The one lane that owns
// (T_b - 1, U_b) leaves v p_blank there in the header and writes the score.  rnnt_align_backtrack_kernel: one workgroup per row walks
// the T_b + U_b moves back from (T_b - 1, U_b), a block of diagonals at a time: the block's bytes are staged into LDS with 16-byte
// loads, one lane walks them, then all lanes turn the block's moves into outputs, reading the emissions of the path's cells for the
// per-move logarithms.  No atomics anywhere: every output element has exactly one writer.  One entry point serves both score sources
// (nntk_shim_rnnt_src): it differs in the limit check and in the emission writer it calls, and in nothing else.
#include "rnnt_common.hpp"

#define RNNT_BT_BYTES (64 * 1024)         // backpointer bytes staged per block of diagonals ...
#define RNNT_BT_DIAGS 2048                // ... and the diagonals of a block at most (their u sit in LDS too)
static int rnnt_bt_block_diags(int P) {
    const int dc = RNNT_BT_BYTES / P;
    return dc < 1 ? 1 : dc > RNNT_BT_DIAGS ? RNNT_BT_DIAGS : dc;
}

// NJ as in rnnt_lattice_kernel.  LDS per u: v p_blank | v p_label of the lane's cell -- what moves on to (t + 1, u) and to (t, u + 1)
template <int NJ>
__global__ __launch_bounds__(CTC_THREADS) void rnnt_viterbi_kernel(int B, int T, int U1, const int *__restrict__ ints,
                                                                   const float4 *__restrict__ em, unsigned char *bp, float *hdr,
                                                                   float *scores) {
    extern __shared__ __align__(16) unsigned char rnnt_vit_smem[];
    float4 *st = (float4 *)rnnt_vit_smem;                                   // [2][U1]
    const int b = blockIdx.x, tid = threadIdx.x;
    const int Tb = ints[b], Ub = ints[B + b];
    const float4 *e = em + (long)b * T * U1;
    const int P = min(T, U1);
    unsigned char *brow = bp + (long)b * (T + U1 - 1) * P;
    const int ND = Tb + Ub;                                                 // diagonals n = t + u = 0 .. ND - 1
    constexpr int NR = NJ > 0 ? NJ : 1;
    const float4 none = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    auto live = [&](int n, int u) { return u <= Ub && n - u >= 0 && n - u < Tb; };
    float4 en[NR];
    if (NJ > 0) {
#pragma unroll
        for (int j = 0; j < NR; ++j) {
            const int u = tid + CTC_THREADS * j;
            en[j] = none;
            if (live(0, u)) en[j] = e[u];
        }
    }
    int cur = 0;
    for (int n = 0; n < ND; ++n) {
        float4 ec[NR];
        if (NJ > 0) {
#pragma unroll
            for (int j = 0; j < NR; ++j) ec[j] = en[j];
            if (n + 1 < ND) {                                               // the next diagonal's emissions: not on the dependent chain
#pragma unroll
                for (int j = 0; j < NR; ++j) {
                    const int u = tid + CTC_THREADS * j;
                    en[j] = none;
                    if (live(n + 1, u)) en[j] = e[(long)(n + 1 - u) * U1 + u];
                }
            }
        }
        const float4 *src = st + cur * U1;
        float4 *dst = st + (cur ^ 1) * U1;
        unsigned char *bd = brow + (long)n * P - max(0, n - (T - 1));
        auto cell = [&](int u, float4 e4) {
            const int t = n - u;
            xf pb, py;
            pb.m = e4.x; pb.e = __float_as_int(e4.y);
            py.m = e4.z; py.e = __float_as_int(e4.w);
            xf v;
            int step = 0;
            if (n == 0) {
                v = xf_one();
            } else {                                                        // from (t - 1, u) by a blank, then from (t, u - 1) by label u
                v = t >= 1 ? xf_unpack(make_float2(src[u].x, src[u].y)) : xf_zero();
                const xf fu = u >= 1 ? xf_unpack(make_float2(src[u - 1].z, src[u - 1].w)) : xf_zero();
                if (xf_greater(fu, v)) { v = fu; step = 1; }
            }
            bd[u] = (unsigned char)step;
            const xf vb = xf_times(v, pb), vy = xf_times(v, py);
            dst[u] = make_float4(vb.m, __int_as_float(vb.e), vy.m, __int_as_float(vy.e));
            if (n == ND - 1) {                                              // the one cell of the last diagonal: (Tb - 1, Ub)
                hdr[2 * b] = vb.m;
                hdr[2 * b + 1] = __int_as_float(vb.e);
                // once per row: double, libm log
                scores[b] = vb.m == 0.0f ? -INFINITY : (float)((double)vb.e * 0.69314718055994530942 + log((double)vb.m));
            }
        };
        if (NJ > 0) {
#pragma unroll
            for (int j = 0; j < NR; ++j)
                if (live(n, tid + CTC_THREADS * j)) cell(tid + CTC_THREADS * j, ec[j]);
        } else {
            for (int u = tid; u <= Ub; u += CTC_THREADS)
                if (live(n, u)) cell(u, e[(long)(n - u) * U1 + u]);
        }
        CTC_LDS_BARRIER();
        cur ^= 1;
    }
}

// ln of an emission kept as mantissa and exponent (never zero on a path of non-zero probability)
__device__ __forceinline__ float rnnt_align_ln(float m, float e) {
    return (float)((double)__float_as_int(e) * 0.69314718055994530942 + log((double)m));
}

// label_frames / label_logp [B][maxL] and frame_labels / frame_logp [B][T] (each may be NULL) of row blockIdx.x from its backpointers
__global__ __launch_bounds__(CTC_THREADS) void rnnt_align_backtrack_kernel(int B, int T, int U1, int DC, const int *__restrict__ ints,
                                                                           const float4 *__restrict__ em,
                                                                           const unsigned char *__restrict__ bp,
                                                                           const float *__restrict__ hdr, int *__restrict__ label_frames,
                                                                           int *__restrict__ frame_labels, float *__restrict__ label_logp,
                                                                           float *__restrict__ frame_logp) {
    extern __shared__ __align__(16) unsigned char rnnt_bt_smem[];
    const int b = blockIdx.x, tid = threadIdx.x, maxL = U1 - 1, P = min(T, U1);
    const bool has = hdr[2 * b] > 0.0f;                                      // a row without a path: nothing but -1 and 0
    const int Tb = has ? ints[b] : 0, Ub = has ? ints[B + b] : 0;
    int *path = (int *)rnnt_bt_smem;                                         // [DC + 1]: u of the block's diagonals n0 .. n1 (n1: one above)
    unsigned char *blk = rnnt_bt_smem + (((size_t)(DC + 1) * 4 + 15) & ~(size_t)15);
    const float4 *e = em + (long)b * T * U1;
    const unsigned char *brow = bp + (long)b * (T + U1 - 1) * P;
    int *lf = label_frames ? label_frames + (long)b * maxL : nullptr, *fl = frame_labels ? frame_labels + (long)b * T : nullptr;
    float *ll = label_logp ? label_logp + (long)b * maxL : nullptr, *fp = frame_logp ? frame_logp + (long)b * T : nullptr;
    // every element has one writer: the padding here, a label's or a frame's own move below
    for (int i = Ub + tid; i < maxL; i += CTC_THREADS) {
        if (lf) lf[i] = -1;
        if (ll) ll[i] = 0.0f;
    }
    for (int t = Tb + tid; t < T; t += CTC_THREADS) {
        if (fl) fl[t] = -1;
        if (fp) fp[t] = 0.0f;
    }
    // move n leaves the path's cell of diagonal n, (n - u_n, u_n): a label if u_{n+1} = u_n + 1, a blank otherwise; u_ND stands for U_b
    int u = Ub, above = Ub;                                                  // lane 0: u of diagonal n1 - 1, and of diagonal n1
    for (int n1 = Tb + Ub; n1 > 0; n1 -= DC) {
        const int n0 = max(0, n1 - DC);
        const uintptr_t lo = (uintptr_t)(brow + (long)n0 * P), hi = lo + (size_t)(n1 - n0) * P;
        const uintptr_t lo16 = lo & ~(uintptr_t)15;
        const int quads = (int)((hi - lo16 + 15) >> 4);
        __syncthreads();
        for (int q = tid; q < quads; q += CTC_THREADS) ((uint4 *)blk)[q] = ((const uint4 *)lo16)[q];
        __syncthreads();
        if (tid == 0) {
            const unsigned char *rec = blk + (lo - lo16);
            path[n1 - n0] = above;
            for (int n = n1 - 1; n >= n0; --n) {
                path[n - n0] = u;
                if (n > 0) {                                                // (a path of non-zero probability never leaves the lattice)
                    const int step = rec[(long)(n - n0) * P + u - max(0, n - (T - 1))];
                    if (u > 0 && (step || n - u == 0)) --u;
                }
            }
            above = path[0];
        }
        __syncthreads();
        for (int i = tid; i < n1 - n0; i += CTC_THREADS) {
            const int n = n0 + i, un = path[i], t = n - un;
            const float4 e4 = e[(long)t * U1 + un];
            if (path[i + 1] != un) {
                if (lf) lf[un] = t;
                if (ll) ll[un] = rnnt_align_ln(e4.z, e4.w);
            } else {
                if (fl) fl[t] = un;
                if (fp) fp[t] = rnnt_align_ln(e4.x, e4.y);
            }
        }
    }
}

// Viterbi and backtrace on the emissions em of a loss-only workspace whose ints and header are at their places; d_bp: the backpointers
static int rnnt_align_launch(int B, int T, int U1, const int *d_ints, const float4 *em, float *hdr, unsigned char *d_bp,
                             const nntk_shim_rnnt_path *out) {
    const size_t lds = 2 * (size_t)U1 * sizeof(float4);
#define RNNT_VIT(NJ)                                                                                                          \
    do {                                                                                                                      \
        if (lds > 48 * 1024 && nntk_set_max_dynamic_lds((const void *)rnnt_viterbi_kernel<NJ>, lds)) return -1;                \
        hipLaunchKernelGGL(rnnt_viterbi_kernel<NJ>, dim3((unsigned)B), dim3(CTC_THREADS), lds, nntk_stream(), B, T, U1, d_ints, em, \
                           d_bp, hdr, out->scores);                                                                            \
    } while (0)
    if (U1 <= CTC_THREADS) RNNT_VIT(1);
    else if (U1 <= 2 * CTC_THREADS) RNNT_VIT(2);
    else RNNT_VIT(0);
#undef RNNT_VIT
    NNTK_LAUNCH_CHECK("rnnt_viterbi_kernel");
    if (!out->label_frames && !out->frame_labels && !out->label_logp && !out->frame_logp) return 0;
    const int P = T < U1 ? T : U1, DC = rnnt_bt_block_diags(P);
    const size_t blds = (((size_t)(DC + 1) * 4 + 15) & ~(size_t)15) + (size_t)DC * P + 32;
    if (blds > 48 * 1024 && nntk_set_max_dynamic_lds((const void *)rnnt_align_backtrack_kernel, blds)) return -1;
    hipLaunchKernelGGL(rnnt_align_backtrack_kernel, dim3((unsigned)B), dim3(CTC_THREADS), blds, nntk_stream(), B, T, U1, DC, d_ints, em,
                       d_bp, hdr, out->label_frames, out->frame_labels, out->label_logp, out->frame_logp);
    NNTK_LAUNCH_CHECK("rnnt_align_backtrack_kernel");
    return 0;
}

// the loss-only workspace of the score source (either loss call's), then the backpointers
static RnntAlignLayout rnnt_align_layout_of(const nntk_shim_rnnt_src *src, int B, int T, int V, int maxL) {
    return rnnt_align_layout(src->fused ? nntk_shim_rnnt_fused_workspace_floats(B, T, maxL, src->J, V, 0) : rnnt_layout(B, T, maxL, 0).total,
                             B, T, maxL);
}

extern "C" {

size_t nntk_shim_rnnt_align_workspace_floats(const nntk_shim_rnnt_src *src, int batch, int T, int V, int max_label_len) {
    return rnnt_align_layout_of(src, batch, T, V, max_label_len).total;
}

int nntk_shim_rnnt_align(const nntk_shim_rnnt_src *src, int B, int T, int V, const int *h_input_lengths, const int *h_labels,
                         const int *h_label_lengths, int maxL, int blank, const nntk_shim_rnnt_path *out, float *d_ws) {
    if (B <= 0) return 0;
    if (src->fused) {
        if (!rnnt_fused_fits(T, maxL, src->J, V, d_ws))
            return nntk_fail_msg("nntk_rnnt_fused_align_device: a shape beyond the kernels' limits or a misaligned workspace");
    } else {
        if (!rnnt_lattice_fits(T, maxL))
            return nntk_fail_msg("nntk_rnnt_align_device: max_label_len or T + max_label_len is beyond the lattice kernel's limits");
        if ((((uintptr_t)d_ws | (uintptr_t)src->d_logits) & 15) != 0)
            return nntk_fail_msg("nntk_rnnt_align_device: the scores and the workspace must be 16-byte aligned");
    }
    const int U1 = maxL + 1;
    const RnntParts w = rnnt_parts(d_ws, rnnt_layout(B, T, maxL, 0), false);  // the fused loss-only workspace starts with these parts too
    if (rnnt_upload_ints(w.ints, B, maxL, h_input_lengths, h_labels, h_label_lengths)) return -1;
    if (src->fused ? nntk_rnnt_fused_emit_launch(src->d_enc, src->d_pred, src->d_out, B, T, U1, src->J, V, src->kind, blank, w.ints, w.em, nullptr)
                   : nntk_rnnt_emit_launch(src->d_logits, B, T, U1, V, blank, w.ints, w.em, nullptr)) return -1;
    return rnnt_align_launch(B, T, U1, w.ints, w.em, w.hdr, (unsigned char *)(d_ws + rnnt_align_layout_of(src, B, T, V, maxL).bp), out);
}

}  // extern "C"
