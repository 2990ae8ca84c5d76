// rnnt_tdt_common.hpp -- what the token-and-duration transducer units share (rnnt_tdt.hip: the loss and its gradient; rnnt_tdt_align.hip:
// Viterbi on the same per-cell emissions): the duration table as the kernels take it, the workspace layout of the per-cell scalars, the
// ring's size and the limits, the record a lattice cell takes from global memory, and the launcher of the emission writer, which
// rnnt_tdt.hip owns and the aligner reuses unchanged.
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

// rnnt_tdt.hip: tdt_emit_kernel, the token emissions and duration probabilities of the stored scores d_logits [B][T][U1][V + D] into
// em / pdur; lse NULL = not kept (loss only, alignment)
int nntk_rnnt_tdt_emit_launch(const float *d_logits, int B, int T, int U1, int V, int D, int blank, float sigma, const int *d_ints,
                              float4 *em, float2 *pdur, double *lse);
