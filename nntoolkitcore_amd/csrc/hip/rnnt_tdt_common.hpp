// rnnt_tdt_common.hpp -- what the token-and-duration transducer units share (rnnt_tdt.hip: the loss and its gradient; rnnt_tdt_align.hip:
// Viterbi on the same per-cell emissions; rnnt_tdt_fused.hip: the loss from the joiner's inputs, the scores never stored): the duration
// table as the kernels take it, the workspace layout of the per-cell scalars, the ring's size and the limits, the record a lattice cell
// takes from global memory, a cell's flows and gradient value, and the launchers of the kernels that one unit owns and another reuses
// unchanged: rnnt_tdt.hip's emission writer and lattice, rnnt_tdt_fused.hip's emission writer.
#pragma once
#include "rnnt_common.hpp"

#define TDT_MAXD NNTK_RNNT_TDT_MAX_DURATIONS

struct TdtDur { int n, dmax; int d[TDT_MAXD]; };                             // the durations, by value: strictly ascending, d[0] >= 0
static inline TdtDur tdt_dur(const int *h_durations, int D) {
    TdtDur dur;
    dur.n = D;
    dur.dmax = h_durations[D - 1];
    for (int i = 0; i < TDT_MAXD; ++i) dur.d[i] = i < D ? h_durations[i] : 0;
    return dur;
}

// workspace, in 4-byte words: [ints: input lengths B | label lengths B | labels B*maxL] [P per row: 2B] [token emissions: 4 per cell]
// [duration probabilities: 2 D per cell]; with a gradient: [lse_tok, lse_dur: 4 per cell] [alpha: 2 per cell] [beta: 2 per cell]; every
// part starts on a 16-byte boundary
struct TdtLayout { size_t hdr, em, dur, lse, alpha, beta, total; };
static inline TdtLayout tdt_layout(int B, int T, int maxL, int D, int want_grad) {
    TdtLayout l;
    const size_t b = B > 0 ? (size_t)B : 0, t = T > 0 ? (size_t)T : 0, ml = maxL > 0 ? (size_t)maxL : 0, nd = D > 0 ? (size_t)D : 0;
    auto up = [](size_t x) { return (x + 3) & ~(size_t)3; };
    const size_t cells = b * t * (ml + 1);
    l.hdr = up(b * (2 + ml));
    l.em = l.hdr + up(2 * b);
    l.dur = l.em + 4 * cells;
    l.lse = l.dur + up(2 * nd * cells);
    l.alpha = l.lse + (want_grad ? 4 * cells : 0);
    l.beta = l.alpha + (want_grad ? up(2 * cells) : 0);
    l.total = l.beta + (want_grad ? up(2 * cells) : 0) + 4;
    return l;
}

static inline size_t tdt_ring_bytes(int U1, int dmax) { return (size_t)(dmax + 2) * (size_t)U1 * sizeof(float4); }

__device__ __forceinline__ xf tdt_xf(float2 w) { return xf_unpack(w); }
__device__ __forceinline__ float2 tdt_zero2() { return make_float2(0.0f, __int_as_float(CTC_EZERO)); }

// what a cell of the lattice takes from global memory: its own token emissions and, forwards, the duration probabilities of its
// sources -- a[i] of (t - d_i, u), the blank's; b[i] of (t - d_i, u - 1), the label's -- backwards its own, in a[i].  A term that does
// not exist has a zero there
struct TdtRec { float4 e; float2 a[TDT_MAXD], b[TDT_MAXD]; };

// the limits of nntk_shim.h, for a caller that bypasses rnnt.c
static inline bool tdt_fits(int T, int maxL, const int *dur, int D) {
    if (D < 1 || D > TDT_MAXD || dur[0] < 0 || dur[D - 1] < 1 || dur[D - 1] > NNTK_RNNT_TDT_MAX_DURATION) return false;
    for (int i = 1; i < D; ++i)
        if (dur[i] <= dur[i - 1]) return false;
    return maxL >= 0 && tdt_ring_bytes(maxL + 1, dur[D - 1]) <= NNTK_RNNT_TDT_LDS_BYTES && (long)T + maxL <= NNTK_RNNT_TDT_MAX_DIAGONALS;
}

// forced alignment (rnnt_tdt_align.hip): a loss-only workspace, then the terminal move's choice (one word per row), then one
// backpointer byte per cell of the row's T + maxL diagonals, each min(T, maxL + 1) wide, then 16 bytes the staging loads may run into
struct TdtAlignLayout { size_t term, bp, total; };
static inline TdtAlignLayout tdt_align_layout(int B, int T, int maxL, int D) {
    TdtAlignLayout l;
    const size_t b = B > 0 ? (size_t)B : 0, t = T > 0 ? (size_t)T : 0, ml = maxL > 0 ? (size_t)maxL : 0;
    auto up = [](size_t x) { return (x + 3) & ~(size_t)3; };
    l.term = up(tdt_layout(B, T, maxL, D, 0).total);
    l.bp = l.term + up(b);
    l.total = l.bp + up((b * (t + ml) * (t < ml + 1 ? t : ml + 1) + 3) / 4) + 4;
    return l;
}

// the scalars of a live cell of a row with P = mP 2^eP > 0: the occupancy and the flows out of it, all over P (rnnt_tdt.hip's gradient
// kernel, a wavefront per cell; rnnt_tdt_fused.hip's tile record, a lane per cell)
struct TdtFlows { RnntFlows tok; float fd[TDT_MAXD]; };
__device__ __forceinline__ TdtFlows tdt_cell_flows(long c, int t, int u, int Tb, int Ub, int U1, const TdtDur &dur,
                                                   const float4 *__restrict__ em, const float2 *__restrict__ pdur,
                                                   const float2 *__restrict__ wa, const float2 *__restrict__ wb, float mP, int eP) {
    const xf a = xf_unpack(wa[c]);
    const float4 e4 = em[c];
    xf pb, py;
    pb.m = e4.x; pb.e = __float_as_int(e4.y);
    py.m = e4.z; py.e = __float_as_int(e4.w);
    const xf ab = xf_times(a, pb), ay = xf_times(a, py);
    TdtFlows f;
    f.tok.occ = xf_to_float(xf_times(a, xf_unpack(wb[c])), eP) / mP;
    f.tok.fb = f.tok.fy = 0.0f;
#pragma unroll
    for (int i = 0; i < TDT_MAXD; ++i) {
        f.fd[i] = 0.0f;
        if (i >= dur.n) continue;
        const int k = dur.d[i], tt = t + k;
        const xf pdi = xf_unpack(pdur[c * dur.n + i]);
        float fb = 0.0f, fy = 0.0f;
        if (k > 0 && tt <= Tb) {                                            // alpha p_blank p_dur(i) beta(t + d_i, u) / P
            const xf bt = tt < Tb ? xf_unpack(wb[c + (long)k * U1]) : u == Ub ? xf_one() : xf_zero();
            fb = xf_to_float(xf_times(xf_times(ab, pdi), bt), eP) / mP;
        }
        if (u < Ub && tt < Tb)                                              // alpha p_label p_dur(i) beta(t + d_i, u + 1) / P
            fy = xf_to_float(xf_times(xf_times(ay, pdi), xf_unpack(wb[c + (long)k * U1 + 1])), eP) / mP;
        f.tok.fb += fb;
        f.tok.fy += fy;
        f.fd[i] = fb + fy;
    }
    return f;
}

// element k of a cell's row of V + D: a token's gradient (rnnt_grad_value) or a duration's, the same selected-not-multiplied zero
__device__ __forceinline__ float tdt_grad_value(const TdtFlows &f, double lse_t, double lse_d, int V, int blank, int y, float x, int k) {
    if (k < V) return rnnt_grad_value(f.tok, lse_t, blank, y, x, k);
    float r = f.tok.occ == 0.0f ? 0.0f : f.tok.occ * expf((float)((double)x - lse_d));
#pragma unroll
    for (int i = 0; i < TDT_MAXD; ++i)
        if (k - V == i) r -= f.fd[i];
    return r;
}

// rnnt_tdt.hip: tdt_lattice_kernel on the emissions em [cells] and the duration probabilities pdur [cells][D]; wa / wb NULL = the forward
// direction alone (loss only)
int nntk_rnnt_tdt_lattice_launch(int B, int T, int U1, const TdtDur &dur, const int *d_ints, const float4 *em, const float2 *pdur, float2 *wa,
                                 float2 *wb, float *hdr, float *d_loss_rows);
// rnnt_tdt_fused.hip: rnnt_tdt_fused_forward_kernel, the same emissions from the joiner's inputs and the Dense block d_out = W [J, V + D] |
// b [V + D]; lse NULL = not kept
int nntk_rnnt_tdt_fused_emit_launch(const float *d_enc, const float *d_pred, const float *d_out, int B, int T, int U1, int J, int V, int D,
                                    int kind, int blank, float sigma, const int *d_ints, float4 *em, float2 *pdur, double *lse);
// rnnt_tdt.hip: tdt_emit_kernel, the token emissions and duration probabilities of the stored scores d_logits [B][T][U1][V + D] into
// em / pdur; lse NULL = not kept (loss only, alignment)
int nntk_rnnt_tdt_emit_launch(const float *d_logits, int B, int T, int U1, int V, int D, int blank, float sigma, const int *d_ints,
                              float4 *em, float2 *pdur, double *lse);
