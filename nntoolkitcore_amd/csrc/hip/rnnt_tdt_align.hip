// rnnt_tdt_align.hip -- forced alignment of the token-and-duration transducer: given a row's labels, the single most probable path through
// the lattice of rnnt_tdt.hip (Viterbi: the max twin of its alpha recursion) -- out of which frame every label is emitted and with which
// duration, which frames are left by a blank and with which duration, the natural log of every move on the path (token emission times
// duration probability) and of the path's probability.  It runs on what tdt_emit_kernel (rnnt_tdt.hip) leaves per cell, in the
// loss-only layout: 16 bytes of token emissions and D duration probabilities of 8 bytes.
//
// Range.  Every Viterbi variable is an xf (ctc_xf.hpp), as the emissions are.  A candidate is one multiply with the source's duration
// probability and one xf comparison: max never rounds, there is no add and no transcendental on the dependent chain.
//
// Tie-break (part of the contract): into a cell the candidates are taken in the loss's one order -- ascending i, for each i the blank
// term before the label term -- and a later candidate replaces the current one only if it is strictly greater.  The current one starts
// as zero: a cell that no candidate of non-zero mass reaches keeps value zero and the backpointer "none".
//
// Work split, three launches.
//  tdt_emit_kernel, through nntk_rnnt_tdt_emit_launch: unchanged, no lse part.
//  tdt_viterbi_kernel<REG>: one 256-lane workgroup per row walks the anti-diagonals n = t + u upwards, lanes over u -- the frame of
//    tdt_lattice_kernel, direction 0.  The ring of Dmax + 2 diagonals in LDS holds v p_blank | v p_label of the SOURCE cell (16 bytes
//    per u), diagonal m in slot m mod (Dmax + 2); one LDS-only barrier per diagonal, outside lane-dependent control flow; the trip
//    count T_b + U_b + 1 is uniform, the last step being the blank-only terminal cell (T_b, U_b).  Whether a term exists is decided
//    from the indices alone, and a term that does not exist never reads the ring.  REG (U1 <= 256): a lane owns u = tid and takes the
//    cell's record (its emissions, the up to 2 D duration probabilities of its sources) from registers, loaded a diagonal ahead and in
//    flight across the barrier, with this diagonal's backpointer stores.  Otherwise lanes stride over u and fetch inside the step.
//    Backpointers: one byte per cell, (i << 1) | is_label of the move taken INTO it, 0xFF for none, laid out by diagonal as
//    rnnt_align.hip has them -- cell (t, u) of row b at ((b ND + n) P + u - max(0, n - (T - 1))), ND = T + max_label_len diagonals of
//    P = min(T, max_label_len + 1) bytes -- so a wavefront's stores of one diagonal are 64 contiguous bytes.  The terminal cell is on
//    no stored diagonal: its choice goes into the row's HEADER, one word per row after the loss-only workspace (TdtAlignLayout::term),
//    next to the path's probability in the loss's P slot.
//  tdt_align_backtrack_kernel: one workgroup per row.  A move jumps d_i + is_label diagonals, so the path's cells are not on
//    consecutive diagonals: a block of up to DC diagonals ENDING at the current cell's is staged into LDS with 16-byte loads, lane 0
//    walks the moves whose cells lie in it and leaves them (source cell, i, is_label) in LDS, then all lanes turn the block's moves
//    into outputs, reading the emission and the duration probability of each move's source cell for the logarithm.  The next block
//    ends at the diagonal of the first cell the walk could not read, so a jump across a block's lower edge costs nothing and no
//    diagonal is staged that the path jumped over.  Lane 0 also sets one bit per frame that a blank leaves; the padding, and the
//    frames without that bit, are written at the end by the lanes that own them.  Every output element has exactly one writer.
// No atomics anywhere.  Plain stores only.
#include "rnnt_tdt_common.hpp"

// REG: U1 <= 256, a lane owns the cell u = tid of a diagonal; else any U1 whose ring fits the LDS.  bp NULL: only the score is asked for
template <bool REG>
__global__ __launch_bounds__(CTC_THREADS) void tdt_viterbi_kernel(int B, int T, int U1, const TdtDur dur, const int *__restrict__ ints,
                                                                  const float4 *__restrict__ em, const float2 *__restrict__ pdur,
                                                                  unsigned char *bp, float *hdr, int *term, float *scores) {
    extern __shared__ __align__(16) unsigned char tdt_vit_smem[];
    float4 *ring = (float4 *)tdt_vit_smem;                                  // [dmax + 2][U1]
    const int b = blockIdx.x, tid = threadIdx.x;
    const int Tb = ints[b], Ub = ints[B + b], D = dur.n, R = dur.dmax + 2;
    const long base = (long)b * T * U1;
    const float4 *e = em + base;
    const float2 *pd = pdur + base * D;
    const int P = min(T, U1);
    unsigned char *brow = bp ? bp + (long)b * (T + U1 - 1) * P : nullptr;
    const int steps = Tb + Ub + 1;                                          // diagonals 0 .. Tb + Ub, the last one the cell (Tb, Ub) alone
    auto live = [&](int n, int u) {
        const int t = n - u;
        return u <= Ub && t >= 0 && (t < Tb || (t == Tb && u == Ub));
    };
    auto fetch = [&](int n, int u, TdtRec &r) {
        const int t = n - u;
        r.e = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
        for (int i = 0; i < TDT_MAXD; ++i) r.a[i] = r.b[i] = tdt_zero2();
        if (!live(n, u)) return;
        if (t < Tb) r.e = e[(long)t * U1 + u];
#pragma unroll
        for (int i = 0; i < TDT_MAXD; ++i) {
            if (i >= D || t - dur.d[i] < 0) continue;
            const long s = (long)(t - dur.d[i]) * U1 + u;
            if (dur.d[i] > 0) r.a[i] = pd[s * D + i];
            if (u >= 1 && t < Tb) r.b[i] = pd[(s - 1) * D + i];
        }
    };
    // the slot of diagonal n is sl; of n - k, 0 <= k < R, k slots behind on the ring
    auto cell = [&](int n, int sl, int u, const TdtRec &r) {
        const int t = n - u;
        xf v = n == 0 ? xf_one() : xf_zero();
        int code = 0xFF;
#pragma unroll
        for (int i = 0; i < TDT_MAXD; ++i) {
            if (i >= D || t - dur.d[i] < 0) continue;
            const int k = dur.d[i];                                         // from (t - k, u) by a blank, then from (t - k, u - 1) by label u
            if (k > 0) {
                const float4 s = ring[(sl - k < 0 ? sl - k + R : sl - k) * U1 + u];
                const xf c = xf_times(tdt_xf(make_float2(s.x, s.y)), tdt_xf(r.a[i]));
                if (xf_greater(c, v)) { v = c; code = 2 * i; }
            }
            if (u >= 1 && t < Tb) {
                const float4 s = ring[(sl - k - 1 < 0 ? sl - k - 1 + R : sl - k - 1) * U1 + u - 1];
                const xf c = xf_times(tdt_xf(make_float2(s.z, s.w)), tdt_xf(r.b[i]));
                if (xf_greater(c, v)) { v = c; code = 2 * i + 1; }
            }
        }
        if (t == Tb) {                                                      // the one cell of the last diagonal: the path's probability
            hdr[2 * b] = v.m;
            hdr[2 * b + 1] = __int_as_float(v.e);
            term[b] = code;
            // once per row: double, libm log
            scores[b] = v.m == 0.0f ? -INFINITY : (float)((double)v.e * 0.69314718055994530942 + log((double)v.m));
            return;
        }
        if (brow) brow[(long)n * P + u - max(0, n - (T - 1))] = (unsigned char)code;
        xf pb, py;
        pb.m = r.e.x; pb.e = __float_as_int(r.e.y);
        py.m = r.e.z; py.e = __float_as_int(r.e.w);
        const xf vb = xf_times(v, pb), vy = xf_times(v, py);
        ring[sl * U1 + u] = make_float4(vb.m, __int_as_float(vb.e), vy.m, __int_as_float(vy.e));
    };
    TdtRec nx;
    if (REG) fetch(0, tid, nx);
    int sl = 0;
    for (int n = 0; n < steps; ++n) {
        if (REG) {
            const TdtRec cu = nx;
            if (n + 1 < steps) fetch(n + 1, tid, nx);                       // the next diagonal's records: not on the dependent chain
            if (live(n, tid)) cell(n, sl, tid, cu);
        } else {
            for (int u = tid; u <= Ub; u += CTC_THREADS)
                if (live(n, u)) {
                    TdtRec cu;
                    fetch(n, u, cu);
                    cell(n, sl, u, cu);
                }
        }
        CTC_LDS_BARRIER();
        sl = sl + 1 == R ? 0 : sl + 1;
    }
}

// the LDS of the backtrack: the block's moves [DC + 1] (8 bytes each), one bit per frame, 16 control words (moves in the block, where
// the next block ends, the durations), the staged backpointers
struct TdtBtLds { size_t bits, ctl, blk, total; };
static inline TdtBtLds tdt_bt_lds(int T, int P, int DC) {
    TdtBtLds l;
    auto up = [](size_t x) { return (x + 15) & ~(size_t)15; };
    l.bits = up((size_t)(DC + 1) * 8);
    l.ctl = l.bits + up((size_t)((T + 31) / 32) * 4);
    l.blk = l.ctl + 64;
    l.total = l.blk + (size_t)DC * P + 32;
    return l;
}

// the six arrays (each may be NULL) of row blockIdx.x from its backpointers; lb: the offsets of tdt_bt_lds
__global__ __launch_bounds__(CTC_THREADS) void tdt_align_backtrack_kernel(int B, int T, int U1, int DC, const TdtDur dur, const TdtBtLds lb,
                                                                          const int *__restrict__ ints, const float4 *__restrict__ em,
                                                                          const float2 *__restrict__ pdur,
                                                                          const unsigned char *__restrict__ bp,
                                                                          const float *__restrict__ hdr, const int *__restrict__ term,
                                                                          int *__restrict__ label_frames, int *__restrict__ label_durs,
                                                                          int *__restrict__ frame_labels, int *__restrict__ frame_durs,
                                                                          float *__restrict__ label_logp, float *__restrict__ frame_logp) {
    extern __shared__ __align__(16) unsigned char tdt_bt_smem[];
    const int b = blockIdx.x, tid = threadIdx.x, maxL = U1 - 1, P = min(T, U1), D = dur.n;
    const bool has = hdr[2 * b] > 0.0f;                                      // a row without a path: nothing but -1 and 0
    const int Tb = has ? ints[b] : 0, Ub = has ? ints[B + b] : 0;
    int2 *mv = (int2 *)tdt_bt_smem;                                          // {source t, source u << 4 | i << 1 | is_label}
    unsigned *blank_at = (unsigned *)(tdt_bt_smem + lb.bits);                // bit t: a blank of the path leaves frame t
    int *ctl = (int *)(tdt_bt_smem + lb.ctl), *dl = ctl + 4;
    unsigned char *blk = tdt_bt_smem + lb.blk;
    const long base = (long)b * T * U1;
    const float4 *e = em + base;
    const float2 *pd = pdur + base * D;
    const unsigned char *brow = bp + (long)b * (T + U1 - 1) * P;
    int *lf = label_frames ? label_frames + (long)b * maxL : nullptr, *ld = label_durs ? label_durs + (long)b * maxL : nullptr;
    int *fl = frame_labels ? frame_labels + (long)b * T : nullptr, *fd = frame_durs ? frame_durs + (long)b * T : nullptr;
    float *ll = label_logp ? label_logp + (long)b * maxL : nullptr, *fp = frame_logp ? frame_logp + (long)b * T : nullptr;
    for (int w = tid; w < (T + 31) / 32; w += CTC_THREADS) blank_at[w] = 0u;
    if (tid < TDT_MAXD) dl[tid] = dur.d[tid];
    // every element has one writer: the labels' padding here, a move's label or frame below, every other frame at the end
    for (int i = Ub + tid; i < maxL; i += CTC_THREADS) {
        if (lf) lf[i] = -1;
        if (ld) ld[i] = -1;
        if (ll) ll[i] = 0.0f;
    }
    int ct = Tb, cu = Ub;                                                    // lane 0: the cell the walk stands on
    for (int n1 = Tb + Ub; n1 > 0;) {                                        // the block: diagonals n0 .. n1 - 1
        const int n0 = max(0, n1 - DC);
        const uintptr_t lo = (uintptr_t)(brow + (long)n0 * P), hi = lo + (size_t)(n1 - n0) * P;
        const uintptr_t lo16 = lo & ~(uintptr_t)15;
        const int quads = (int)((hi - lo16 + 15) >> 4);
        for (int q = tid; q < quads; q += CTC_THREADS) ((uint4 *)blk)[q] = ((const uint4 *)lo16)[q];
        __syncthreads();
        if (tid == 0) {
            const unsigned char *rec = blk + (lo - lo16);
            auto at = [&](int t, int u) { return (int)rec[(long)(t + u - n0) * P + u - max(0, t + u - (T - 1))]; };
            // the move into the terminal cell is in the header; into any other cell, on the cell's diagonal n1 - 1
            int code = ct == Tb ? term[b] : at(ct, cu), cnt = 0, next = 0;
            while (code != 0xFF && cnt <= DC) {                              // (0xFF: the cell (0, 0), where every path begins)
                const int i = min(code >> 1, D - 1);
                ct -= dl[i];
                cu -= code & 1;
                if (ct < 0 || cu < 0) break;                                 // (a path of non-zero probability never leaves the lattice)
                mv[cnt++] = make_int2(ct, (cu << 4) | (i << 1) | (code & 1));
                if (!(code & 1)) blank_at[ct >> 5] |= 1u << (ct & 31);
                if (ct + cu < n0) {                                          // a jump across the block's lower edge
                    next = ct + cu + 1;
                    break;
                }
                code = ct + cu == 0 ? 0xFF : at(ct, cu);
            }
            ctl[0] = cnt;
            ctl[1] = next;
        }
        __syncthreads();
        const int cnt = ctl[0];
        n1 = ctl[1];
        for (int j = tid; j < cnt; j += CTC_THREADS) {
            const int2 m = mv[j];
            const int t = m.x, u = m.y >> 4, i = (m.y >> 1) & 7;
            const float4 e4 = e[(long)t * U1 + u];
            const float2 p = pd[((long)t * U1 + u) * D + i];
            const bool label = m.y & 1;
            // ln(p_tok p_dur) from the two mantissas and exponents, in double
            const float lp = (float)((double)(__float_as_int(label ? e4.w : e4.y) + __float_as_int(p.y)) * 0.69314718055994530942 +
                                     log((double)(label ? e4.z : e4.x) * (double)p.x));
            if (label) {
                if (lf) lf[u] = t;
                if (ld) ld[u] = dl[i];
                if (ll) ll[u] = lp;
            } else {
                if (fl) fl[t] = u;
                if (fd) fd[t] = dl[i];
                if (fp) fp[t] = lp;
            }
        }
    }
    __syncthreads();
    for (int t = tid; t < T; t += CTC_THREADS)
        if (t >= Tb || !((blank_at[t >> 5] >> (t & 31)) & 1u)) {
            if (fl) fl[t] = -1;
            if (fd) fd[t] = -1;
            if (fp) fp[t] = 0.0f;
        }
}

extern "C" {

size_t nntk_shim_rnnt_tdt_align_workspace_floats(int batch, int T, int max_label_len, int n_durations) {
    return tdt_align_layout(batch, T, max_label_len, n_durations).total;
}

int nntk_shim_rnnt_tdt_align(const float *d_logits, int B, int T, int V, const int *h_durations, int D, const int *h_input_lengths,
                             const int *h_labels, const int *h_label_lengths, int maxL, int blank, float sigma,
                             const nntk_shim_rnnt_tdt_path *out, float *d_ws) {
    if (B <= 0) return 0;
    if (!tdt_fits(T, maxL, h_durations, D))
        return nntk_fail_msg("nntk_rnnt_tdt_align_device: the durations, max_label_len or T + max_label_len are beyond the lattice kernel's limits");
    if ((((uintptr_t)d_ws | (uintptr_t)d_logits) & 15) != 0)
        return nntk_fail_msg("nntk_rnnt_tdt_align_device: the scores and the workspace must be 16-byte aligned");
    const int U1 = maxL + 1;
    const TdtLayout l = tdt_layout(B, T, maxL, D, 0);
    const TdtAlignLayout al = tdt_align_layout(B, T, maxL, D);
    int *ints = (int *)d_ws, *term = (int *)(d_ws + al.term);
    float *hdr = d_ws + l.hdr;
    float4 *em = (float4 *)(d_ws + l.em);
    float2 *pdur = (float2 *)(d_ws + l.dur);
    const bool path = out->label_frames || out->label_durations || out->frame_labels || out->frame_durations || out->label_logp || out->frame_logp;
    unsigned char *bp = path ? (unsigned char *)(d_ws + al.bp) : nullptr;
    const TdtDur dur = tdt_dur(h_durations, D);
    if (rnnt_upload_ints(ints, B, maxL, h_input_lengths, h_labels, h_label_lengths)) return -1;
    if (nntk_rnnt_tdt_emit_launch(d_logits, B, T, U1, V, D, blank, sigma, ints, em, pdur, nullptr)) return -1;
    const size_t lds = tdt_ring_bytes(U1, dur.dmax);
#define TDT_VIT(REG)                                                                                                             \
    do {                                                                                                                         \
        if (lds > 48 * 1024 && nntk_set_max_dynamic_lds((const void *)tdt_viterbi_kernel<REG>, lds)) return -1;                   \
        hipLaunchKernelGGL(tdt_viterbi_kernel<REG>, dim3((unsigned)B), dim3(CTC_THREADS), lds, nntk_stream(), B, T, U1, dur, ints, \
                           em, pdur, bp, hdr, term, out->scores);                                                                \
    } while (0)
    if (U1 <= CTC_THREADS) TDT_VIT(true);
    else TDT_VIT(false);
#undef TDT_VIT
    NNTK_LAUNCH_CHECK("tdt_viterbi_kernel");
    if (!path) return 0;
    const int P = T < U1 ? T : U1, DC = rnnt_bt_block_diags(P);
    const TdtBtLds lb = tdt_bt_lds(T, P, DC);
    if (lb.total > 48 * 1024 && nntk_set_max_dynamic_lds((const void *)tdt_align_backtrack_kernel, lb.total)) return -1;
    hipLaunchKernelGGL(tdt_align_backtrack_kernel, dim3((unsigned)B), dim3(CTC_THREADS), lb.total, nntk_stream(), B, T, U1, DC, dur, lb, ints,
                       em, pdur, bp, hdr, term, out->label_frames, out->label_durations, out->frame_labels, out->frame_durations,
                       out->label_logp, out->frame_logp);
    NNTK_LAUNCH_CHECK("tdt_align_backtrack_kernel");
    return 0;
}

}  // extern "C"
