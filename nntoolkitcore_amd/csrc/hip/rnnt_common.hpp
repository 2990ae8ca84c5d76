// rnnt_common.hpp -- what the three transducer loss / alignment units share (rnnt.hip: the loss on a stored score tensor;
// rnnt_fused.hip: the loss that makes its scores from the joiner's inputs and never stores them; rnnt_align.hip: Viterbi on either's
// emissions): the kernels' limits, the workspace layout of the per-cell scalars and its pointers, the upload of the host ints, the
// emission as mantissa and exponent, the cell index, the joiner's activation, and the launchers of the kernels that one unit owns and
// another reuses unchanged.
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
// rnnt_fused.hip: rnnt_fused_forward_kernel, the same emissions from the joiner's inputs and the Dense block d_out
int nntk_rnnt_fused_emit_launch(const float *d_enc, const float *d_pred, const float *d_out, int B, int T, int U1, int J, int V, int kind,
                                int blank, const int *d_ints, float4 *em, double *lse);
