// rnnt_common.hpp -- what the four transducer loss / alignment units share (rnnt.hip: the loss on a stored score tensor;
// rnnt_fused.hip: the loss that makes its scores from the joiner's inputs and never stores them; rnnt_align.hip: Viterbi on either's
// emissions; rnnt_pruned.hip: the simple loss on a sum of two rows and the loss on a band of the lattice): the kernels' limits, the
// workspace layout of the per-cell scalars and its pointers, the upload of the host ints, the emission as mantissa and exponent, the
// cell index, the per-cell bodies of the emit and gradient kernels on a score source, the joiner's activation, and the launchers of
// the kernels that one unit owns and another reuses unchanged.
#pragma once
#include <stdint.h>
#include "nntk_common.hpp"
#include "ctc_xf.hpp"

#define RNNT_EMIN (-4000)                 // floor of an emission's base-2 exponent: NNTK_RNNT_MAX_DIAGONALS * 4000 < 2^28 = -CTC_EZERO
#define RNNT_MAX_GRID (1 << 20)

// workspace, in 4-byte words: [ints: input lengths B | label lengths B | labels B*maxL] [P per row: 2B] [emissions: 4 per cell]
// with a gradient: [lse: 2 per cell] [alpha: 2 per cell] [beta: 2 per cell]; every part starts on a 16-byte boundary
struct RnntLayout { size_t hdr, em, lse, alpha, beta, total; };
static inline RnntLayout rnnt_layout(int B, int T, int maxL, int want_grad) {
    RnntLayout l;
    const size_t b = B > 0 ? (size_t)B : 0, t = T > 0 ? (size_t)T : 0, ml = maxL > 0 ? (size_t)maxL : 0;
    auto up = [](size_t x) { return (x + 3) & ~(size_t)3; };
    const size_t cells = b * t * (ml + 1);
    l.hdr = up(b * (2 + ml));
    l.em = l.hdr + up(2 * b);
    l.lse = l.em + 4 * cells;
    l.alpha = l.lse + (want_grad ? up(2 * cells) : 0);
    l.beta = l.alpha + (want_grad ? up(2 * cells) : 0);
    l.total = l.beta + (want_grad ? up(2 * cells) : 0) + 4;
    return l;
}

// the layout as pointers into d_ws; lse / alpha / beta NULL without a gradient
struct RnntParts { int *ints; float *hdr; float4 *em; double *lse; float2 *alpha, *beta; };
static inline RnntParts rnnt_parts(float *d_ws, const RnntLayout &l, bool grad) {
    return {(int *)d_ws, d_ws + l.hdr, (float4 *)(d_ws + l.em), grad ? (double *)(d_ws + l.lse) : nullptr,
            grad ? (float2 *)(d_ws + l.alpha) : nullptr, grad ? (float2 *)(d_ws + l.beta) : nullptr};
}

// the three host int arrays (checked by rnnt.c) to the head of the workspace, in stream order
static inline int rnnt_upload_ints(int *d_ints, int B, int maxL, const int *h_input_lengths, const int *h_labels, const int *h_label_lengths) {
    if (nntk_shim_upload_ints(d_ints, h_input_lengths, B)) return -1;
    if (nntk_shim_upload_ints(d_ints + B, h_label_lengths, B)) return -1;
    if (maxL > 0 && nntk_shim_upload_ints(d_ints + 2L * B, h_labels, (long)B * maxL)) return -1;
    return 0;
}

// the limits of nntk_shim.h, for the entry points (rnnt.c checks them first; these guard a caller that bypasses it)
static inline bool rnnt_lattice_fits(int T, int maxL) { return maxL <= NNTK_RNNT_MAX_LABELS && (long)T + maxL <= NNTK_RNNT_MAX_DIAGONALS; }
static inline bool rnnt_fused_fits(int T, int maxL, int J, int V, const void *d_ws) {
    return rnnt_lattice_fits(T, maxL) && J >= 1 && J <= NNTK_RNNT_FUSED_MAX_J && V >= 2 && V <= NNTK_RNNT_FUSED_MAX_V && ((uintptr_t)d_ws & 15) == 0;
}

// forced alignment (rnnt_align.hip): a loss-only workspace of `base` words (either loss call's), then one backpointer byte per cell of
// the row's T + maxL diagonals, each min(T, maxL + 1) wide, then 16 bytes the staging loads may run into
struct RnntAlignLayout { size_t bp, total; };
static inline RnntAlignLayout rnnt_align_layout(size_t base, int B, int T, int maxL) {
    RnntAlignLayout l;
    const size_t b = B > 0 ? (size_t)B : 0, t = T > 0 ? (size_t)T : 0, ml = maxL > 0 ? (size_t)maxL : 0;
    auto up = [](size_t x) { return (x + 3) & ~(size_t)3; };
    l.bp = up(base);
    l.total = l.bp + up((b * (t + ml) * (t < ml + 1 ? t : ml + 1) + 3) / 4) + 4;
    return l;
}

// exp(x - lse) as mantissa and exponent; -inf (and NaN) scores: zero
__device__ __forceinline__ xf rnnt_emission(float x, double lse) {
    if (!(x > -INFINITY)) return xf_zero();
    double l2 = ((double)x - lse) * 1.44269504088896340736;
    l2 = l2 < (double)RNNT_EMIN ? (double)RNNT_EMIN : l2;
    const double fl = floor(l2);
    return xf_norm(exp2f((float)(l2 - fl)), (int)fl);
}

// cell c = (b * T + t) * U1 + u
struct RnntCell { int b, t, u; };
__device__ __forceinline__ RnntCell rnnt_cell(long c, int T, int U1) {
    RnntCell r;
    const long bt = c / U1;
    r.u = (int)(c - bt * U1);
    r.b = (int)(bt / T);
    r.t = (int)(bt - (long)r.b * T);
    return r;
}

// ---- the per-cell bodies of rnnt_emit_kernel and rnnt_grad_kernel, one wavefront per cell, on a score source: the V scores of a cell
//      are a stored row (rnnt.hip on [B][T][U1][V], rnnt_pruned.hip on the band [B][T][S][V]) or the f32 sum of two rows, rounded once
//      (rnnt_pruned.hip: am[b][t][:] + lm[b][u][:]).  The order of every operation is the same for all sources: the bits of a cell depend
//      on its V scores alone ----
template <bool SUM>
struct RnntRow {
    const float *a, *l;                                                     // l: the second term, SUM only
    __device__ __forceinline__ float at(int k) const { return SUM ? a[k] + l[k] : a[k]; }
    __device__ __forceinline__ f32x4 at4(int i) const {                     // rows on the 16-byte grid only
        f32x4 x = ((const f32x4 *)a)[i];
        if (SUM) x += ((const f32x4 *)l)[i];
        return x;
    }
};

__device__ __forceinline__ float rnnt_wave_max(float v) {
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
    return v;
}
__device__ __forceinline__ double rnnt_wave_sum(double v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// maximum, then the sum of exp(x - max) in double; lane 0 keeps the blank's and the label's emission (label NULL: the row's last
// column of cells, no label leaves it) and, where asked, lse.  VEC: V % 4 == 0 and the row(s) 16-byte aligned
template <bool VEC, bool SUM>
__device__ __forceinline__ void rnnt_emit_row(const RnntRow<SUM> row, int V, int blank, const int *label, int lane, float4 *em_c, double *lse_c) {
    float mx = -INFINITY;
    if (VEC) {
        for (int i = lane; i < (V >> 2); i += 64) {
            const f32x4 x = row.at4(i);
            mx = fmaxf(mx, fmaxf(fmaxf(x[0], x[1]), fmaxf(x[2], x[3])));
        }
    } else {
        for (int k = lane; k < V; k += 64) mx = fmaxf(mx, row.at(k));
    }
    mx = rnnt_wave_max(mx);
    double s = 0.0;
    if (VEC) {
        for (int i = lane; i < (V >> 2); i += 64) {
            const f32x4 x = row.at4(i);
            s += (double)expf(x[0] - mx);
            s += (double)expf(x[1] - mx);
            s += (double)expf(x[2] - mx);
            s += (double)expf(x[3] - mx);
        }
    } else {
        for (int k = lane; k < V; k += 64) s += (double)expf(row.at(k) - mx);
    }
    s = rnnt_wave_sum(s);
    if (lane == 0) {
        const double lse = (double)mx + log(s);
        const xf pb = rnnt_emission(row.at(blank), lse);
        const xf py = label ? rnnt_emission(row.at(*label), lse) : xf_zero();
        *em_c = make_float4(pb.m, __int_as_float(pb.e), py.m, __int_as_float(py.e));
        if (lse_c) *lse_c = lse;
    }
}

// the three scalars of a live cell c = (t, u) of a row with P = mP 2^eP > 0: the occupancy alpha beta / P and the two flows out of it
struct RnntFlows { float occ, fb, fy; };
__device__ __forceinline__ RnntFlows rnnt_cell_flows(long c, int t, int u, int Tb, int Ub, int U1, const float4 *__restrict__ em,
                                                     const float2 *__restrict__ wa, const float2 *__restrict__ wb, float mP, int eP) {
    const xf a = xf_unpack(wa[c]);
    const float4 e4 = em[c];
    xf pb, py;
    pb.m = e4.x; pb.e = __float_as_int(e4.y);
    py.m = e4.z; py.e = __float_as_int(e4.w);
    RnntFlows f;
    f.occ = xf_to_float(xf_times(a, xf_unpack(wb[c])), eP) / mP;                                  // alpha beta / P
    const xf bt = t + 1 < Tb ? xf_unpack(wb[c + U1]) : u == Ub ? xf_one() : xf_zero();
    f.fb = xf_to_float(xf_times(xf_times(a, pb), bt), eP) / mP;                                  // alpha p_blank beta(t + 1, u) / P
    f.fy = 0.0f;
    if (u < Ub) f.fy = xf_to_float(xf_times(xf_times(a, py), xf_unpack(wb[c + 1])), eP) / mP;    // alpha p_label beta(t, u + 1) / P
    return f;
}

// d loss / d score v of a cell: occ exp(x - lse) - [v = blank] fb - [v = y] fy (y = -1: no label leaves the cell).  An occupancy of
// exactly 0 is a first term of exactly 0, selected and not multiplied: a live cell whose V scores are all -inf has two zero emissions,
// so beta and the occupancy are 0, and lse = NaN (-inf - -inf).  On finite scores 0 exp(x - lse) was +0 already: the same bits
__device__ __forceinline__ float rnnt_grad_value(const RnntFlows f, double lse, int blank, int y, float x, int v) {
    float r = f.occ == 0.0f ? 0.0f : f.occ * expf((float)((double)x - lse));
    if (v == blank) r -= f.fb;
    if (v == y) r -= f.fy;
    return r;
}

template <bool VEC, bool SUM>
__device__ __forceinline__ void rnnt_grad_row(const RnntRow<SUM> row, float *g, int V, int blank, int y, const RnntFlows f, double lse, int lane) {
    if (VEC) {
        f32x4 *g4 = (f32x4 *)g;
        for (int i = lane; i < (V >> 2); i += 64) {
            const f32x4 x = row.at4(i);
            f32x4 r;
            r[0] = rnnt_grad_value(f, lse, blank, y, x[0], 4 * i);
            r[1] = rnnt_grad_value(f, lse, blank, y, x[1], 4 * i + 1);
            r[2] = rnnt_grad_value(f, lse, blank, y, x[2], 4 * i + 2);
            r[3] = rnnt_grad_value(f, lse, blank, y, x[3], 4 * i + 3);
            g4[i] = r;
        }
    } else {
        for (int k = lane; k < V; k += 64) g[k] = rnnt_grad_value(f, lse, blank, y, row.at(k), k);
    }
}

// V zeros at g (4-byte aligned), by one wavefront: 16-byte stores between a head and a tail
__device__ __forceinline__ void rnnt_zero_row(float *g, int V, int lane) {
    const int head = min(V, (int)((4 - (((uintptr_t)g >> 2) & 3)) & 3));
    const int quads = (V - head) >> 2;
    if (lane < head) g[lane] = 0.0f;
    f32x4 *g4 = (f32x4 *)(g + head);
    const f32x4 z = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int i = lane; i < quads; i += 64) g4[i] = z;
    const int done = head + 4 * quads;
    if (lane < V - done) g[done + lane] = 0.0f;
}

// ---- the joiner: out[b][t][u][:] = act(enc[b][t][:] + pred[b][u][:]); activation 0 identity, 1 tanh (tanhf), 2 relu (max(x, 0)) ----
__device__ __forceinline__ float rnnt_act(int kind, float x) { return kind == 1 ? tanhf(x) : kind == 2 ? fmaxf(x, 0.0f) : x; }
// d act / d x from the activation's OUTPUT
__device__ __forceinline__ float rnnt_dact(int kind, float o) { return kind == 1 ? 1.0f - o * o : kind == 2 ? (o > 0.0f ? 1.0f : 0.0f) : 1.0f; }

static inline unsigned rnnt_grid(long items, long per_block) {
    long g = (items + per_block - 1) / per_block;
    return (unsigned)(g < 1 ? 1 : g > RNNT_MAX_GRID ? RNNT_MAX_GRID : g);
}

// rnnt.hip: rnnt_lattice_kernel on the emissions em [cells] (float4 each); wa / wb NULL = the forward direction alone (loss only)
int nntk_rnnt_lattice_launch(int B, int T, int U1, const int *d_ints, const float4 *em, float2 *wa, float2 *wb, float *hdr,
                             float *d_loss_rows);
// rnnt.hip: rnnt_emit_kernel, the emissions of the stored scores d_logits [B][T][U1][V] into em; lse NULL = not kept (loss only)
int nntk_rnnt_emit_launch(const float *d_logits, int B, int T, int U1, int V, int blank, const int *d_ints, float4 *em, double *lse);
// rnnt.hip: rnnt_joint_reduce_kernel: dst[o][r] = sum over k < R, ascending, of dout[o * ostride + k * rstride + r] * act'(out[the same]),
// n elements of dst, M of them per o
int nntk_rnnt_joint_reduce_launch(const float *d_out_fwd, const float *d_dout, long n, long M, long ostride, int R, long rstride, int kind,
                                  float *d_dst);
// rnnt_fused.hip: rnnt_fused_forward_kernel, the same emissions from the joiner's inputs and the Dense block d_out
int nntk_rnnt_fused_emit_launch(const float *d_enc, const float *d_pred, const float *d_out, int B, int T, int U1, int J, int V, int kind,
                                int blank, const int *d_ints, float4 *em, double *lse);
