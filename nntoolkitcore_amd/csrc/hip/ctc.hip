// ctc.hip -- connectionist temporal classification (Graves et al., 2006) on softmax probabilities [B][T][C], rows ragged:
// the per-row negative log-likelihood, its gradient with respect to the probabilities, and best-path (greedy) decoding.
//
// Range.  Path probabilities fall like C^-T and, inside one timestep, the forward variable spans binomial(T, S)-sized ratios
// between states (1e145 at T = 500, S = 201 on flat posteriors): neither plain f32 nor f32 with one scale per timestep holds
// that.  Every forward / backward variable is therefore an f32 mantissa in [0.5, 1) with its own int32 exponent ("xf" below;
// zero = mantissa 0, exponent CTC_EZERO).  A step is three v_ldexp_f32, two adds, one multiply and one v_frexp pair: linear
// space, so the relative error of a variable grows like sqrt(T) * 2^-24 instead of |log alpha| * 2^-24 of a log-space
// recursion, and there is no transcendental and no normalising reduction on the dependent chain.
//
// Work split.  ctc_alpha_beta_kernel: one 256-lane workgroup per (row, direction) -- blockIdx.y = 0 runs alpha forward in time,
// 1 runs beta backward, concurrently -- lanes over the S = 2L + 1 extended states (a lane owns states tid, tid + 256, ...).  The
// previous step's states are exchanged through double-buffered LDS, one barrier per step; the barrier waits for LDS only, so the
// probability gathers of the NEXT step and the workspace stores stay in flight across it.  What is stored per (t, s) is the
// variable WITHOUT the emission at t (abar, btil), so that dP / dprobs[t][k] = sum_{s: class(s) = k} abar_t(s) btil_t(s) needs no
// division by a probability.  ctc_grad_kernel: one workgroup per (row, 8..16 timesteps) reduces the per-class occupancy into an
// LDS image of those gradient rows (every class once, a repeated label's positions summed in position order by the lane that owns
// its first occurrence: no atomics), then stores the image -- zeros included -- with 16-byte stores.
#include <stdint.h>
#include <limits.h>
#include "nntk_common.hpp"
#include "ctc_xf.hpp"

#define CTC_GRAD_LDS_FLOATS 8192          // gradient rows staged per workgroup: TT * C <= this (TT >= 1: C <= 32768 at 128 KiB)
#define CTC_GRAD_MAX_C 32768

// workspace, in 4-byte words: [ints: input lengths B | label lengths B | labels B*maxL | next B*maxL | first B*maxL] [P per row: 2B]
// [abar: B*T*Smax pairs] [btil: the same]; every part starts on a 16-byte boundary
struct CtcLayout { size_t ints, hdr, alpha, beta, total; };
static CtcLayout ctc_layout(int B, int T, int maxL) {
    CtcLayout l;
    const size_t b = B > 0 ? (size_t)B : 0, t = T > 0 ? (size_t)T : 0, ml = maxL > 0 ? (size_t)maxL : 0;
    auto up = [](size_t x) { return (x + 3) & ~(size_t)3; };
    l.ints = 0;
    l.hdr = up(b * (2 + 3 * ml));
    l.alpha = l.hdr + up(2 * b);
    const size_t ab = up(2 * b * t * (2 * ml + 1));
    l.beta = l.alpha + ab;
    l.total = l.beta + ab + 4;
    return l;
}

// next[i]: the next position with label i's class (-1: none); first[i]: no earlier position has it
__global__ __launch_bounds__(CTC_THREADS) void ctc_prep_kernel(int *ints, int B, int maxL) {
    const int b = blockIdx.x, L = ints[B + b];
    const int *lab = ints + 2L * B + (long)b * maxL;
    int *nxt = ints + 2L * B + (long)B * maxL + (long)b * maxL, *first = nxt + (long)B * maxL;
    for (int i = threadIdx.x; i < L; i += CTC_THREADS) {
        const int c = lab[i];
        int n = -1, f = 1;
        for (int j = i + 1; j < L; ++j) if (lab[j] == c) { n = j; break; }
        for (int j = 0; j < i; ++j) if (lab[j] == c) { f = 0; break; }
        nxt[i] = n;
        first[i] = f;
    }
}

// NJ > 0: a lane's states (at most NJ) keep class, skip flag and the next step's probability in registers; NJ = 0: any S that
// fits the LDS, class and probability fetched inside the step
template <int NJ>
__global__ __launch_bounds__(CTC_THREADS) void ctc_alpha_beta_kernel(const float *__restrict__ probs, int B, int T, int C, int maxL,
                                                                     int blank, const int *__restrict__ ints, float2 *ws_alpha,
                                                                     float2 *ws_beta, float *hdr, float *loss_rows) {
    extern __shared__ __align__(16) unsigned char ctc_smem[];
    const int b = blockIdx.x, dir = blockIdx.y, tid = threadIdx.x;
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
    const int d = dir ? 1 : -1;
    // may state s take the mass two states away?  forward: into s from s - 2; backward: into s from s + 2 (the test sits at s + 2)
    auto skip_of = [&](int s) {
        const int hi = dir ? s + 2 : s;
        return (s & 1) && hi >= 3 && hi < S && cls[hi] != cls[hi - 2];
    };
    int cl[NR];
    bool sk[NR];
    float pn[NR];
    const float *prow = probs + (long)b * T * C;
    float2 *ws = dir ? ws_beta : ws_alpha;
    if (ws) ws += (long)b * T * Smax;
    if (NJ > 0) {
#pragma unroll
        for (int j = 0; j < NR; ++j) {
            const int s = tid + CTC_THREADS * j;
            cl[j] = s < S ? cls[s] : blank;
            sk[j] = s < S && skip_of(s);
            pn[j] = Tb > 0 ? prow[(long)(dir ? Tb - 1 : 0) * C + cl[j]] : 0.0f;
        }
    }
    int cur = 0;
    for (int n = 0; n < Tb; ++n) {
        const int t = dir ? Tb - 1 - n : n;
        float pc[NR];
        if (NJ > 0) {
#pragma unroll
            for (int j = 0; j < NR; ++j) pc[j] = pn[j];
            if (n + 1 < Tb) {                                               // the next step's gathers: not on the dependent chain
                const float *pr = prow + (long)(t - d) * C;
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
            if (n == 0) {
                v = (dir ? s >= S - 2 : s < 2) ? xf_one() : xf_zero();
            } else {
                const bool k = NJ > 0 ? sk[j < NR ? j : 0] : skip_of(s);
                const xf a0 = xf_unpack(src[s]), a1 = xf_unpack(src[s + d]);
                const xf a2 = k ? xf_unpack(src[s + 2 * d]) : xf_zero();
                v = xf_add3(a0, a1, a2);
            }
            if (ws) ws[(long)t * Smax + s] = xf_pack(v);
            const float p = NJ > 0 ? pc[j < NR ? j : 0] : prow[(long)t * C + cls[s]];
            dst[s] = xf_pack(xf_times_prob(v, p));
        }
        CTC_LDS_BARRIER();
        cur ^= 1;
    }
    if (dir == 0 && tid == 0) {
        xf P;
        if (Tb == 0) {
            P = L == 0 ? xf_one() : xf_zero();
        } else {
            const float2 *src = st + cur * pitch + 2;
            P = xf_add3(xf_unpack(src[S - 1]), xf_unpack(src[S - 2]), xf_zero());      // src[-1] is a zero state when S == 1
        }
        hdr[2 * b] = P.m;
        hdr[2 * b + 1] = __int_as_float(P.e);
        // once per row: double, libm log
        loss_rows[b] = P.m == 0.0f ? INFINITY : (float)-((double)P.e * 0.69314718055994530942 + log((double)P.m));
    }
}

// the gradient rows [t0, t0 + TT) of row blockIdx.y
__global__ __launch_bounds__(CTC_THREADS) void ctc_grad_kernel(const float *__restrict__ probs, int B, int T, int C, int maxL, int blank,
                                                               int TT, const int *__restrict__ ints, const float2 *__restrict__ ws_alpha,
                                                               const float2 *__restrict__ ws_beta, const float *__restrict__ hdr,
                                                               float *__restrict__ dprobs) {
    extern __shared__ __align__(16) unsigned char ctc_smem[];
    float *img = (float *)ctc_smem;                                          // [nt][C]
    const int b = blockIdx.y, t0 = blockIdx.x * TT, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nt = min(TT, T - t0);
    const int total = nt * C;
    const int Tb = ints[b], L = ints[B + b], Smax = 2 * maxL + 1;
    const int *lab = ints + 2L * B + (long)b * maxL;
    const int *nxt = lab + (long)B * maxL, *first = nxt + (long)B * maxL;
    for (int i = tid; i < total; i += CTC_THREADS) img[i] = 0.0f;
    __syncthreads();
    const float mP = hdr[2 * b];
    const int eP = __float_as_int(hdr[2 * b + 1]);
    if (mP > 0.0f) {                                                         // an impossible row (P = 0) keeps its zeros
        for (int tt = wave; tt < nt; tt += CTC_THREADS / 64) {
            const int t = t0 + tt;
            if (t >= Tb) break;
            const float2 *wa = ws_alpha + ((long)b * T + t) * Smax, *wb = ws_beta + ((long)b * T + t) * Smax;
            const float *pr = probs + ((long)b * T + t) * C;
            auto occ = [&](int s) {                                          // abar_t(s) btil_t(s) / P
                const xf a = xf_unpack(wa[s]), bb = xf_unpack(wb[s]);
                return ldexpf(a.m * bb.m, a.e + bb.e - eP) / mP;
            };
            float part = 0.0f;
            for (int i = lane; i <= L; i += 64) part += occ(2 * i);
            for (int off = 32; off > 0; off >>= 1) part += __shfl_xor(part, off);
            if (lane == 0) img[tt * C + blank] = pr[blank] > 0.0f ? -part : 0.0f;
            for (int i = lane; i < L; i += 64) {
                if (!first[i]) continue;
                float sum = 0.0f;
                for (int j = i; j >= 0; j = nxt[j]) sum += occ(2 * j + 1);
                const int k = lab[i];
                img[tt * C + k] = pr[k] > 0.0f ? -sum : 0.0f;
            }
        }
    }
    __syncthreads();
    float *g = dprobs + ((long)b * T + t0) * C;
    const int head = min(total, (int)((4 - (((uintptr_t)g >> 2) & 3)) & 3));
    const int quads = (total - head) >> 2;
    if (tid < head) g[tid] = img[tid];
    f32x4 *g4 = (f32x4 *)(g + head);
    for (int q = tid; q < quads; q += CTC_THREADS) {
        const float *p = img + head + 4 * q;
        f32x4 v = {p[0], p[1], p[2], p[3]};
        g4[q] = v;
    }
    const int done = head + 4 * quads;
    if (tid < total - done) g[done + tid] = img[done + tid];
}

// ---- best-path decoding: a wavefront per frame takes the argmax (ties: lowest index), then a workgroup per row compacts in place
__global__ __launch_bounds__(CTC_THREADS) void ctc_argmax_kernel(const float *__restrict__ probs, int T, int C, const int *__restrict__ lens,
                                                                 int *__restrict__ out, long frames) {
    const int lane = threadIdx.x & 63;
    for (long f = blockIdx.x * 4L + (threadIdx.x >> 6); f < frames; f += gridDim.x * 4L) {
        const int b = (int)(f / T), t = (int)(f % T);
        if (t >= lens[b]) continue;
        const float *row = probs + f * C;
        float best = -INFINITY;
        int bi = INT_MAX;
        for (int k = lane; k < C; k += 64) {
            const float v = row[k];
            if (v > best) { best = v; bi = k; }
        }
        for (int off = 32; off > 0; off >>= 1) {
            const float ov = __shfl_xor(best, off);
            const int oi = __shfl_xor(bi, off);
            if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
        }
        if (lane == 0) out[f] = bi == INT_MAX ? 0 : bi;
    }
}

// lens_io[b]: the row's input length on entry, the decoded length on exit.  prev_io (streaming, else NULL): [B], the argmax of the frame
// before the row's first (-1: none), replaced by the argmax of the row's last frame when the row has one
__global__ __launch_bounds__(CTC_THREADS) void ctc_compact_kernel(int *__restrict__ out, int *__restrict__ lens_io, int T, int blank,
                                                                  int *__restrict__ prev_io) {
    __shared__ int sh[CTC_THREADS];
    __shared__ int wtot[CTC_THREADS / 64];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int *row = out + (long)b * T;
    const int len = lens_io[b];
    int base = 0, prev_last = prev_io ? prev_io[b] : -1;
    for (int t0 = 0; t0 < len; t0 += CTC_THREADS) {
        const int t = t0 + tid;
        const int a = t < len ? row[t] : -1;
        sh[tid] = a;
        __syncthreads();
        const int prev = tid > 0 ? sh[tid - 1] : prev_last;
        const bool keep = t < len && a != blank && a != prev;                 // frame 0: prev is -1, or the carried argmax
        const unsigned long long mask = __ballot(keep);
        if (lane == 0) wtot[wave] = __popcll(mask);
        const int last = sh[CTC_THREADS - 1];
        __syncthreads();
        int pos = base + __popcll(mask & ((1ull << lane) - 1));
        int tot = 0;
        for (int w = 0; w < CTC_THREADS / 64; ++w) {
            if (w < wave) pos += wtot[w];
            tot += wtot[w];
        }
        if (keep) row[pos] = a;                                               // pos <= t: never a frame of a later chunk
        if (prev_io && t == len - 1) prev_io[b] = a;                          // every lane read it two barriers ago
        base += tot;
        prev_last = last;
        __syncthreads();
    }
    for (int t = base + tid; t < T; t += CTC_THREADS) row[t] = -1;
    if (tid == 0) lens_io[b] = base;
}

extern "C" {

size_t nntk_shim_ctc_workspace_floats(int batch, int T, int max_label_len) { return ctc_layout(batch, T, max_label_len).total; }

int nntk_shim_ctc_loss(const float *d_probs, int B, int T, int C, const int *h_input_lengths, const int *h_labels,
                       const int *h_label_lengths, int maxL, int blank, float *d_loss_rows, float *d_dprobs, float *d_ws) {
    if (B <= 0) return 0;
    if (((uintptr_t)d_ws & 15) != 0) return nntk_fail_msg("nntk_ctc_loss_device: the workspace must be 16-byte aligned");
    const CtcLayout lay = ctc_layout(B, T, maxL);
    const int Smax = 2 * maxL + 1;
    const size_t lds = (((size_t)Smax * 4 + 15) & ~(size_t)15) + 2 * (size_t)(Smax + 4) * sizeof(float2);
    if (lds > CTC_LDS_LIMIT)
        return nntk_fail_msg("nntk_ctc_loss_device: max_label_len is beyond what one workgroup's LDS holds (" NNTK_STR(NNTK_CTC_ALIGN_MAX_LABELS) ")");
    if (d_dprobs && C > CTC_GRAD_MAX_C) return nntk_fail_msg("nntk_ctc_loss_device: the gradient takes at most 32768 classes");
    int *d_ints = (int *)d_ws;
    if (nntk_shim_upload_ints(d_ints, h_input_lengths, B)) return -1;
    if (nntk_shim_upload_ints(d_ints + B, h_label_lengths, B)) return -1;
    if (maxL > 0 && nntk_shim_upload_ints(d_ints + 2L * B, h_labels, (long)B * maxL)) return -1;
    float *hdr = d_ws + lay.hdr;
    float2 *wa = d_dprobs ? (float2 *)(d_ws + lay.alpha) : nullptr, *wb = d_dprobs ? (float2 *)(d_ws + lay.beta) : nullptr;
    const dim3 grid((unsigned)B, d_dprobs ? 2 : 1);
    if (d_dprobs && maxL > 0) {
        hipLaunchKernelGGL(ctc_prep_kernel, dim3((unsigned)B), dim3(CTC_THREADS), 0, nntk_stream(), d_ints, B, maxL);
        NNTK_LAUNCH_CHECK("ctc_prep_kernel");
    }
#define CTC_AB(NJ)                                                                                                              \
    do {                                                                                                                        \
        if (lds > 48 * 1024 && nntk_set_max_dynamic_lds((const void *)ctc_alpha_beta_kernel<NJ>, lds)) return -1;                \
        hipLaunchKernelGGL(ctc_alpha_beta_kernel<NJ>, grid, dim3(CTC_THREADS), lds, nntk_stream(), d_probs, B, T, C, maxL, blank, \
                           d_ints, wa, wb, hdr, d_loss_rows);                                                                   \
    } while (0)
    if (Smax <= CTC_THREADS) CTC_AB(1);
    else if (Smax <= 2 * CTC_THREADS) CTC_AB(2);
    else if (Smax <= 4 * CTC_THREADS) CTC_AB(4);
    else CTC_AB(0);
#undef CTC_AB
    NNTK_LAUNCH_CHECK("ctc_alpha_beta_kernel");
    if (d_dprobs && T > 0 && C > 0) {
        int TT = CTC_GRAD_LDS_FLOATS / C;
        TT = TT < 1 ? 1 : TT > 16 ? 16 : TT;
        const size_t glds = (size_t)TT * C * sizeof(float);
        if (glds > 48 * 1024 && nntk_set_max_dynamic_lds((const void *)ctc_grad_kernel, glds)) return -1;
        hipLaunchKernelGGL(ctc_grad_kernel, dim3((unsigned)nntk_cdiv(T, TT), (unsigned)B), dim3(CTC_THREADS), glds, nntk_stream(),
                           d_probs, B, T, C, maxL, blank, TT, d_ints, wa, wb, hdr, d_dprobs);
        NNTK_LAUNCH_CHECK("ctc_grad_kernel");
    }
    return 0;
}

// d_prev NULL: the one-shot call; else the chunk's labels, with the repeat rule reaching back to the row's previous frame
int nntk_shim_ctc_greedy_decode_stream(const float *d_probs, int B, int T, int C, const int *h_input_lengths, int blank, int *d_prev,
                                       int *d_labels_out, int *d_out_lengths) {
    if (B <= 0) return 0;
    if (nntk_shim_upload_ints(d_out_lengths, h_input_lengths, B)) return -1;   // the lengths ride in the output until the compaction
    const long frames = (long)B * T;
    if (frames > 0 && C > 0) {
        long g = (frames + 3) / 4;
        if (g > 16384) g = 16384;
        hipLaunchKernelGGL(ctc_argmax_kernel, dim3((unsigned)g), dim3(CTC_THREADS), 0, nntk_stream(), d_probs, T, C, d_out_lengths,
                           d_labels_out, frames);
        NNTK_LAUNCH_CHECK("ctc_argmax_kernel");
    }
    hipLaunchKernelGGL(ctc_compact_kernel, dim3((unsigned)B), dim3(CTC_THREADS), 0, nntk_stream(), d_labels_out, d_out_lengths, T, blank,
                       d_prev);
    NNTK_LAUNCH_CHECK("ctc_compact_kernel");
    return 0;
}

int nntk_shim_ctc_greedy_decode(const float *d_probs, int B, int T, int C, const int *h_input_lengths, int blank, int *d_labels_out,
                                int *d_out_lengths) {
    return nntk_shim_ctc_greedy_decode_stream(d_probs, B, T, C, h_input_lengths, blank, nullptr, d_labels_out, d_out_lengths);
}

}  // extern "C"
