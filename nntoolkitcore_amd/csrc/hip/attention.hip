// attention.hip -- the core of multi-head self-attention for inference, with the masks of a streaming encoder (nntk_attention_device):
//   out[b][i][h] = softmax_j(scale q[b][i][h] . k[b][j][h]) v[b][j][h]   over the keys j that are valid and visible to query i.
// One launch, a workgroup per (tile of 128 queries, head, row); the scores never exist in memory.
//
// Work split.  256 threads = 4 wavefronts, each owning 32 queries whose Q rows it keeps in registers for the whole walk.  The tile walks
// the key blocks (BK keys, aligned on ABSOLUTE stream positions) that hold a key visible to one of its valid queries; a block is staged
// once per workgroup in LDS (K and V, zero-padded in d_head to DP) and shared by the four wavefronts; a wavefront skips the 32-key
// sub-blocks that none of its own queries sees.
//
// Both products run on the exact-f32 MFMA (v_mfma_f32_32x32x2_f32).  The score tile is computed TRANSPOSED, S^T = K Q^T with K as the A
// operand and Q as the B operand: lane (n, kk) = (lane % 32, lane / 32) then holds for query n the scores of the 16 keys
// 8 (r / 4) + 4 kk + r % 4, r = 0 .. 15, in its accumulator.  That register set is the B operand of O^T += V^T P^T as it stands: k step r
// of the second product takes the two keys of register r (kk = 0, 1), and the A fragment is read from the V block in that key order.
// P never goes through LDS and is never transposed.  A query's running max and sum are a reduction over the lane's 16 registers and
// one exchange with lane ^ 32.
//
// Bits.  A query's state (max, sum, O) advances once per 32-key sub-block on absolute positions, in increasing order; a sub-block in
// which the query sees nothing leaves the state as it is (max unchanged, rescale exp(0) = 1, P = 0 by selection), so which blocks the
// tile or the wavefront happens to walk, and where the query sits in either, does not show in its output.  Masked scores are removed by
// selection; key rows outside the tile's visible range or beyond kv_lengths[b] are never read (their LDS rows are zeros).
#include "nntk_common.hpp"

#define ATT_THREADS 256
#define ATT_QT 128                      // queries per workgroup: 4 wavefronts x 32
#define ATT_ROWS 128                    // batch rows per launch: their key counts ride in the kernel's arguments

struct AttLens { int v[ATT_ROWS]; };

struct AttArgs {
    const float *q, *k, *v;
    float *out, *lse;
    long qfs, qbs, kfs, kbs, vfs, vbs;
    int heads, d_head, Tq, Tk, q_offset, pos0, chunk, left, right, row0, use_lens;
    float scale;
};

// the keys [lo, hi) that the valid query at key index p sees: g(p) - left <= g(j) <= g(p) + right, g(x) = (pos0 + x) / chunk, j < kvlen
__device__ __forceinline__ void att_range(const AttArgs &a, int p, int kvlen, int &lo, int &hi) {
    const long long g = (a.pos0 + p) / a.chunk;
    const long long l = a.left < 0 ? 0 : (g - a.left) * a.chunk - a.pos0;
    const long long h = a.right < 0 ? (long long)kvlen : (g + a.right + 1) * a.chunk - a.pos0;
    lo = (int)(l > 0 ? l : 0);
    hi = (int)(h < kvlen ? h : kvlen);
}

// the union of the ranges of the valid queries among the n queries from query index i on (both ends grow with p); empty: lo = hi = 0
__device__ __forceinline__ void att_span(const AttArgs &a, int i, int n, int kvlen, int &lo, int &hi) {
    const int p0 = a.q_offset + i;
    int p1 = p0 + n < a.q_offset + a.Tq ? p0 + n : a.q_offset + a.Tq;
    p1 = (p1 < kvlen ? p1 : kvlen) - 1;
    lo = hi = 0;
    if (p1 < p0) return;
    int x;
    att_range(a, p0, kvlen, lo, x);
    att_range(a, p1, kvlen, x, hi);
}

template <int DP, int BK>
__global__ __launch_bounds__(ATT_THREADS) void attention_kernel(const AttArgs a, const AttLens lens) {
    constexpr int KP = DP + 1;          // K rows are read down a column (lane = key): an odd pitch
    constexpr int VP = DP + 8;          // V rows are read along d (lane = d), the two lane halves four rows apart
    constexpr int NC = DP / 32, NS = DP / 2;
    __shared__ float Ks[BK * KP];
    __shared__ float Vs[BK * VP];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, n = lane & 31, kk = lane >> 5;
    // the query tile is the slowest grid dimension, last tile first: under a causal or windowed mask the late tiles walk the most keys,
    // and dispatching them first leaves the short ones to fill the tail of the launch
    const int h = blockIdx.x, b = a.row0 + blockIdx.y;
    const int kvlen = a.use_lens ? lens.v[blockIdx.y] : a.Tk;
    const int i0 = (gridDim.z - 1 - blockIdx.z) * ATT_QT, i = i0 + 32 * wv + n, p = a.q_offset + i;
    const bool qvalid = i < a.Tq && p < kvlen;
    const int hoff = h * a.d_head;

    int lo = 0, hi = 0, tlo, thi, wlo, whi;
    if (qvalid) att_range(a, p, kvlen, lo, hi);
    att_span(a, i0, ATT_QT, kvlen, tlo, thi);
    att_span(a, i0 + 32 * wv, 32, kvlen, wlo, whi);

    float qr[NS];                                               // Q^T as the B operand: element 2 s + kk of the lane's query
    {
        const float *qp = a.q + (long)b * a.qbs + (long)(qvalid ? i : 0) * a.qfs + hoff;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int d = 2 * s + kk;
            qr[s] = qvalid && d < a.d_head ? qp[d] : 0.0f;
        }
    }
    float m = -INFINITY, l = 0.0f;
    f32x16 o[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[c][r] = 0.0f;

    if (thi > tlo) {
        const float *kb = a.k + (long)b * a.kbs + hoff, *vb = a.v + (long)b * a.vbs + hoff;
        const int ab1 = (a.pos0 + thi - 1) / BK;
        for (int ab = (a.pos0 + tlo) / BK; ab <= ab1; ++ab) {
            const int j0 = ab * BK - a.pos0;                    // may be negative in the stream's first window: those rows are not keys
            __syncthreads();
            for (int e = tid; e < BK * DP; e += ATT_THREADS) {
                const int r = e / DP, c = e % DP, j = j0 + r;
                const bool live = j >= tlo && j < thi && c < a.d_head;
                Ks[r * KP + c] = live ? kb[(long)j * a.kfs + c] : 0.0f;
                Vs[r * VP + c] = live ? vb[(long)j * a.vfs + c] : 0.0f;
            }
            __syncthreads();
#pragma unroll 1
            for (int sub = 0; sub < BK / 32; ++sub) {
                const int jb = j0 + 32 * sub;
                if (whi <= wlo || jb + 32 <= wlo || jb >= whi) continue;      // none of this wavefront's queries sees a key here
                f32x16 s;
#pragma unroll
                for (int r = 0; r < 16; ++r) s[r] = 0.0f;
                const float *kp = Ks + (32 * sub + n) * KP + kk;
#pragma unroll
                for (int st = 0; st < NS; ++st) s = __builtin_amdgcn_mfma_f32_32x32x2f32(kp[2 * st], qr[st], s, 0, 0, 0);
                float mx = -INFINITY;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int j = jb + 8 * (r >> 2) + 4 * kk + (r & 3);
                    s[r] = j >= lo && j < hi ? __fmul_rn(s[r], a.scale) : -INFINITY;
                    mx = fmaxf(mx, s[r]);
                }
                mx = fmaxf(mx, __shfl_xor(mx, 32));
                const float mn = fmaxf(m, mx);
                const float alpha = mn == -INFINITY ? 1.0f : __expf(m - mn);      // nothing seen yet: the state stays as it is
                float ps = 0.0f;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    s[r] = s[r] == -INFINITY ? 0.0f : __expf(s[r] - mn);
                    ps += s[r];
                }
                ps += __shfl_xor(ps, 32);
                l = __fmaf_rn(l, alpha, ps);
                m = mn;
#pragma unroll
                for (int c = 0; c < NC; ++c) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) o[c][r] *= alpha;
                    const float *vp = Vs + (32 * sub + 4 * kk) * VP + 32 * c + n;
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        o[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(vp[(8 * (r >> 2) + (r & 3)) * VP], s[r], o[c], 0, 0, 0);
                }
            }
        }
    }
    if (i >= a.Tq) return;
    float *op = a.out + ((long)b * a.Tq + i) * ((long)a.heads * a.d_head) + hoff;
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int d = 32 * c + 8 * (r >> 2) + 4 * kk + (r & 3);
            if (d < a.d_head) op[d] = qvalid ? o[c][r] / l : 0.0f;
        }
    if (a.lse && kk == 0) a.lse[((long)b * a.heads + h) * a.Tq + i] = qvalid ? m + logf(l) : -INFINITY;
}

extern "C" int nntk_shim_attention(const float *d_q, const float *d_k, const float *d_v, int batch, int heads, int d_head, int Tq, int Tk,
                                   long q_frame_stride, long q_batch_stride, long k_frame_stride, long k_batch_stride, long v_frame_stride,
                                   long v_batch_stride, const int *h_kv_lengths, int q_offset, int pos0, int chunk, int left, int right,
                                   float scale, float *d_out, float *d_lse) {
    if (batch <= 0) return 0;
    if (d_head < 1 || d_head > NNTK_ATTENTION_MAX_D_HEAD || heads < 1 || heads > NNTK_ATTENTION_MAX_HEADS || Tq < 1 || Tk < 1 ||
        Tq > NNTK_ATTENTION_MAX_FRAMES || Tk > NNTK_ATTENTION_MAX_FRAMES || chunk < 1 || q_offset < 0 || q_offset + Tq > Tk)
        return nntk_fail_msg("nntk_attention_device: a shape is outside what the kernel takes");
    AttArgs a = {d_q, d_k, d_v, d_out, d_lse, q_frame_stride, q_batch_stride, k_frame_stride, k_batch_stride, v_frame_stride, v_batch_stride,
                 heads, d_head, Tq, Tk, q_offset, pos0, chunk, left, right, 0, h_kv_lengths != NULL, scale};
    for (int row0 = 0; row0 < batch; row0 += ATT_ROWS) {
        const int rows = batch - row0 < ATT_ROWS ? batch - row0 : ATT_ROWS;
        AttLens lens;
        for (int r = 0; r < ATT_ROWS; ++r) lens.v[r] = h_kv_lengths && r < rows ? h_kv_lengths[row0 + r] : 0;
        a.row0 = row0;
        const dim3 grid((unsigned)heads, (unsigned)rows, (unsigned)nntk_cdiv(Tq, ATT_QT));
        if (d_head <= 32) hipLaunchKernelGGL((attention_kernel<32, 64>), grid, dim3(ATT_THREADS), 0, nntk_stream(), a, lens);
        else if (d_head <= 64) hipLaunchKernelGGL((attention_kernel<64, 64>), grid, dim3(ATT_THREADS), 0, nntk_stream(), a, lens);
        else hipLaunchKernelGGL((attention_kernel<128, 32>), grid, dim3(ATT_THREADS), 0, nntk_stream(), a, lens);
        NNTK_LAUNCH_CHECK("attention_kernel");
    }
    return 0;
}
