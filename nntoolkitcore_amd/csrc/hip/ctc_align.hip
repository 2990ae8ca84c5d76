// ctc_align.hip -- CTC forced alignment on softmax probabilities [B][T][C], rows ragged: given a row's labels, the most probable
// single alignment (Viterbi: the max twin of ctc.hip's alpha recursion), as the extended state of every frame, the frame span of
// every label, and the natural log of the path's probability.
//
// Range.  The best path's probability falls like C^-T, so every Viterbi variable is an xf (ctc_xf.hpp).  A step is one multiply,
// two xf comparisons and one v_frexp pair: max never rounds, there is no add and no transcendental on the dependent chain, and the
// relative error of a variable is at most T * 2^-24.
//
// Tie-break (part of the contract): the predecessor candidates of state s are taken in the order s, s - 1, s - 2 and a later one
// replaces the current one only if it is strictly greater; the end state is 2L unless v(2L - 1) is strictly greater.
//
// Work split.  ctc_viterbi_kernel<NJ>: one 256-lane workgroup per row, lanes over the S = 2L + 1 extended states, the previous
// step's states exchanged through double-buffered LDS with one LDS-only barrier per step -- the frame of ctc_alpha_beta_kernel<NJ>,
// so the next step's probability gathers and this step's backpointer stores stay in flight across the barrier.  What is stored per
// (t >= 1, s) is one byte, the step 0 / 1 / 2 taken into s: a wavefront's stores of one frame are 64 contiguous bytes.  Lane 0
// leaves the row's end state (-1: no alignment) in the header and writes the score.  ctc_align_backtrack_kernel: one workgroup
// per row walks the backpointers from the end state, a block of frames at a time: the block's bytes are staged into LDS with
// 16-byte loads, one lane walks them, then all lanes write the block's states and derive its span edges.  No atomics anywhere:
// every output element has exactly one writer.
#include <stdint.h>
#include "nntk_common.hpp"
#include "ctc_xf.hpp"

#define ALIGN_BT_BYTES (64 * 1024)        // backpointer bytes staged per block of frames ...
#define ALIGN_BT_FRAMES 2048              // ... and the frames of a block at most (their states sit in LDS too)
static int align_block_frames(int Smax) {
    const int tc = ALIGN_BT_BYTES / Smax;
    return tc < 1 ? 1 : tc > ALIGN_BT_FRAMES ? ALIGN_BT_FRAMES : tc;
}

// workspace: [ints: input lengths B | label lengths B | labels B*maxL | end states B] [backpointers: B*T*Smax bytes, row-major in
// (row, frame, state)] [16 bytes the staging loads may run into]; every part starts on a 16-byte boundary
struct AlignLayout { size_t bp, total; };
static AlignLayout align_layout(int B, int T, int maxL) {
    AlignLayout l;
    const size_t b = B > 0 ? (size_t)B : 0, t = T > 0 ? (size_t)T : 0, ml = maxL > 0 ? (size_t)maxL : 0;
    auto up = [](size_t x) { return (x + 3) & ~(size_t)3; };
    l.bp = up(b * (3 + ml));
    l.total = l.bp + up((b * t * (2 * ml + 1) + 3) / 4) + 4;
    return l;
}

// NJ as in ctc_alpha_beta_kernel: NJ > 0 keeps a lane's (at most NJ) states' class, skip flag and next probability in registers
template <int NJ>
__global__ __launch_bounds__(CTC_THREADS) void ctc_viterbi_kernel(const float *__restrict__ probs, int B, int T, int C, int maxL,
                                                                  int blank, const int *__restrict__ ints, unsigned char *bp,
                                                                  int *ends, float *scores) {
    extern __shared__ __align__(16) unsigned char ctc_smem[];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int Tb = ints[b], L = ints[B + b], S = 2 * L + 1, Smax = 2 * maxL + 1;
    const int *lab = ints + 2L * B + (long)b * maxL;
    int *cls = (int *)ctc_smem;                                             // [Smax] class of every extended state
    const int pitch = Smax + 4;                                             // two zero states on either side: no bounds tests
    float2 *st = (float2 *)(ctc_smem + (((size_t)Smax * 4 + 15) & ~(size_t)15));   // [2][pitch]
    for (int s = tid; s < S; s += CTC_THREADS) cls[s] = (s & 1) ? lab[s >> 1] : blank;
    if (tid < 8) {
        const int q = tid & 3;
        st[(tid >> 2) * pitch + (q < 2 ? q : S + q)] = xf_pack(xf_zero());
    }
    __syncthreads();
    constexpr int NR = NJ > 0 ? NJ : 1;
    const int nj = NJ > 0 ? NJ : (S + CTC_THREADS - 1) / CTC_THREADS;
    auto skip_of = [&](int s) { return (s & 1) && s >= 3 && cls[s] != cls[s - 2]; };
    int cl[NR];
    bool sk[NR];
    float pn[NR];
    const float *prow = probs + (long)b * T * C;
    unsigned char *brow = bp + (long)b * T * Smax;
    if (NJ > 0) {
#pragma unroll
        for (int j = 0; j < NR; ++j) {
            const int s = tid + CTC_THREADS * j;
            cl[j] = s < S ? cls[s] : blank;
            sk[j] = s < S && skip_of(s);
            pn[j] = Tb > 0 ? prow[cl[j]] : 0.0f;
        }
    }
    int cur = 0;
    for (int t = 0; t < Tb; ++t) {
        float pc[NR];
        if (NJ > 0) {
#pragma unroll
            for (int j = 0; j < NR; ++j) pc[j] = pn[j];
            if (t + 1 < Tb) {                                               // the next step's gathers: not on the dependent chain
                const float *pr = prow + (long)(t + 1) * C;
#pragma unroll
                for (int j = 0; j < NR; ++j) pn[j] = pr[cl[j]];
            }
        }
        const float2 *src = st + cur * pitch + 2;
        float2 *dst = st + (cur ^ 1) * pitch + 2;
        for (int j = 0; j < nj; ++j) {
            const int s = tid + CTC_THREADS * j;
            if (s >= S) break;
            xf v;
            if (t == 0) {
                v = s < 2 ? xf_one() : xf_zero();
            } else {
                const bool k = NJ > 0 ? sk[j < NR ? j : 0] : skip_of(s);
                const xf a1 = xf_unpack(src[s - 1]);
                const xf a2 = k ? xf_unpack(src[s - 2]) : xf_zero();
                v = xf_unpack(src[s]);
                int step = 0;
                if (xf_greater(a1, v)) { v = a1; step = 1; }
                if (xf_greater(a2, v)) { v = a2; step = 2; }
                brow[(long)t * Smax + s] = (unsigned char)step;
            }
            const float p = NJ > 0 ? pc[j < NR ? j : 0] : prow[(long)t * C + cls[s]];
            dst[s] = xf_pack(xf_times_prob(v, p));
        }
        CTC_LDS_BARRIER();
        cur ^= 1;
    }
    if (tid == 0) {
        xf P;
        int end;
        if (Tb == 0) {
            P = L == 0 ? xf_one() : xf_zero();
            end = L == 0 ? 0 : -1;
        } else {
            const float2 *src = st + cur * pitch + 2;
            const xf lo = xf_unpack(src[S - 2]);                             // src[-1] is a zero state when S == 1
            P = xf_unpack(src[S - 1]);
            end = S - 1;
            if (xf_greater(lo, P)) { P = lo; end = S - 2; }
            if (P.m == 0.0f) end = -1;
        }
        ends[b] = end;
        // once per row: double, libm log
        scores[b] = P.m == 0.0f ? -INFINITY : (float)((double)P.e * 0.69314718055994530942 + log((double)P.m));
    }
}

// states [B][T] and spans [B][maxL][2] (either may be NULL) of row blockIdx.x from its backpointers
__global__ __launch_bounds__(CTC_THREADS) void ctc_align_backtrack_kernel(int B, int T, int maxL, int TC, const int *__restrict__ ints,
                                                                          const unsigned char *__restrict__ bp,
                                                                          int *__restrict__ states, int *__restrict__ spans) {
    extern __shared__ __align__(16) unsigned char align_smem[];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int Smax = 2 * maxL + 1, L = ints[B + b], end = ints[2L * B + (long)B * maxL + b];
    const int Tb = end < 0 ? 0 : ints[b];                                   // a row without an alignment: nothing but -1
    int *path = (int *)align_smem;                                           // [TC + 2]: a block's frames t0 - 1 .. t1 (-1: no frame)
    unsigned char *blk = align_smem + (((size_t)(TC + 2) * 4 + 15) & ~(size_t)15);
    int *srow = states ? states + (long)b * T : nullptr;
    int *prow = spans ? spans + 2L * b * maxL : nullptr;
    // every element has one writer: the -1 of a label the row does not have here, the edges of one it has below
    if (prow) for (int q = tid + 2 * (Tb > 0 ? L : 0); q < 2 * maxL; q += CTC_THREADS) prow[q] = -1;
    if (srow) for (int t = Tb + tid; t < T; t += CTC_THREADS) srow[t] = -1;
    int s = end, above = -1;                                                 // lane 0: the state of frame t1 - 1, and of frame t1
    for (int t1 = Tb; t1 > 0; t1 -= TC) {
        const int t0 = max(0, t1 - TC);
        const uintptr_t lo = (uintptr_t)(bp + ((long)b * T + t0) * Smax), hi = lo + (size_t)(t1 - t0) * Smax;
        const uintptr_t lo16 = lo & ~(uintptr_t)15;
        const int quads = (int)((hi - lo16 + 15) >> 4);
        __syncthreads();
        for (int q = tid; q < quads; q += CTC_THREADS) ((uint4 *)blk)[q] = ((const uint4 *)lo16)[q];
        __syncthreads();
        if (tid == 0) {
            const unsigned char *rec = blk + (lo - lo16);
            path[t1 - t0 + 1] = above;
            for (int t = t1 - 1; t >= t0; --t) {
                path[t - t0 + 1] = s;
                if (t > 0) s = max(0, s - rec[(long)(t - t0) * Smax + s]);     // (a path of non-zero probability never leaves [0, end])
            }
            path[0] = t0 > 0 ? s : -1;
            above = path[1];
        }
        __syncthreads();
        for (int i = tid; i < t1 - t0; i += CTC_THREADS) {
            const int t = t0 + i, c = path[i + 1];
            if (srow) srow[t] = c;
            if (prow && (c & 1)) {
                if (path[i] != c) prow[c - 1] = t;                           // label (c - 1) / 2: [2 * label] = first frame
                if (path[i + 2] != c) prow[c] = t + 1;                       //                    [2 * label + 1] = one past the last
            }
        }
    }
}

extern "C" {

size_t nntk_shim_ctc_align_workspace_floats(int batch, int T, int max_label_len) { return align_layout(batch, T, max_label_len).total; }

int nntk_shim_ctc_align(const float *d_probs, int B, int T, int C, const int *h_input_lengths, const int *h_labels,
                        const int *h_label_lengths, int maxL, int blank, int *d_states, int *d_spans, float *d_scores, float *d_ws) {
    if (B <= 0) return 0;
    if (((uintptr_t)d_ws & 15) != 0) return nntk_fail_msg("nntk_ctc_align_device: the workspace must be 16-byte aligned");
    const AlignLayout lay = align_layout(B, T, maxL);
    const int Smax = 2 * maxL + 1;
    const size_t lds = (((size_t)Smax * 4 + 15) & ~(size_t)15) + 2 * (size_t)(Smax + 4) * sizeof(float2);
    if (lds > CTC_LDS_LIMIT)
        return nntk_fail_msg("nntk_ctc_align_device: max_label_len is beyond what one workgroup's LDS holds (" NNTK_STR(NNTK_CTC_ALIGN_MAX_LABELS) ")");
    int *d_ints = (int *)d_ws, *d_ends = d_ints + 2L * B + (long)B * maxL;
    unsigned char *d_bp = (unsigned char *)(d_ws + lay.bp);
    if (nntk_shim_upload_ints(d_ints, h_input_lengths, B)) return -1;
    if (nntk_shim_upload_ints(d_ints + B, h_label_lengths, B)) return -1;
    if (maxL > 0 && nntk_shim_upload_ints(d_ints + 2L * B, h_labels, (long)B * maxL)) return -1;
#define CTC_VIT(NJ)                                                                                                             \
    do {                                                                                                                        \
        if (lds > 48 * 1024 && nntk_set_max_dynamic_lds((const void *)ctc_viterbi_kernel<NJ>, lds)) return -1;                   \
        hipLaunchKernelGGL(ctc_viterbi_kernel<NJ>, dim3((unsigned)B), dim3(CTC_THREADS), lds, nntk_stream(), d_probs, B, T, C, maxL, \
                           blank, d_ints, d_bp, d_ends, d_scores);                                                              \
    } while (0)
    if (Smax <= CTC_THREADS) CTC_VIT(1);
    else if (Smax <= 2 * CTC_THREADS) CTC_VIT(2);
    else if (Smax <= 4 * CTC_THREADS) CTC_VIT(4);
    else CTC_VIT(0);
#undef CTC_VIT
    NNTK_LAUNCH_CHECK("ctc_viterbi_kernel");
    if (!d_states && !d_spans) return 0;
    const int TC = align_block_frames(Smax);
    const size_t blds = (((size_t)(TC + 2) * 4 + 15) & ~(size_t)15) + (size_t)TC * Smax + 32;
    if (blds > 48 * 1024 && nntk_set_max_dynamic_lds((const void *)ctc_align_backtrack_kernel, blds)) return -1;
    hipLaunchKernelGGL(ctc_align_backtrack_kernel, dim3((unsigned)B), dim3(CTC_THREADS), blds, nntk_stream(), B, T, maxL, TC, d_ints, d_bp,
                       d_states, d_spans);
    NNTK_LAUNCH_CHECK("ctc_align_backtrack_kernel");
    return 0;
}

}  // extern "C"
