// attention_bwd.hip -- the gradient of the attention core (attention.hip) with respect to q, k and v (nntk_attention_backward_device):
//   P_ij = exp(scale q_i . k_j - lse_i)   delta_i = dout_i . out_i   dS_ij = P_ij (dout_i . v_j - delta_i)
//   dq_i = scale sum_j dS_ij k_j          dk_j = scale sum_i dS_ij q_i          dv_j = sum_i P_ij dout_i
// over the keys j valid and visible to the valid query i.  P is recomputed from the forward's lse; no [Tq][Tk] array exists in memory.
//
// No atomics, so two kernels, each recomputing the score tile and each owning its outputs outright:
//   attention_dq_kernel   a workgroup per (128 queries, head, row) walks the key blocks its queries see; writes dq and the row norm
//   attention_dkv_kernel  a workgroup per (128 keys, head, row) walks the query blocks that see its keys; writes dk and dv
// 256 threads = 4 wavefronts of 32 queries (keys) each.  A lane (n, kk) = (lane % 32, lane / 32) keeps elements 2 s + kk of the Q and
// dout rows (K and V rows) of item n in registers; the walked blocks are staged once per workgroup in LDS, zero-padded in d_head.
//
// Every product runs on the exact-f32 MFMA (v_mfma_f32_32x32x2_f32), and as in the forward kernel the score tile is computed in the
// orientation whose accumulator is the B operand of the products that consume it.  dq: S^T = K Q^T and dP^T = V dout^T (A from LDS, read
// down a column; B from the lane's strips) leave in lane (n, kk), for query n, the 16 keys 8 (r / 4) + 4 kk + r % 4; dS^T is formed in
// place and dQ^T += K^T dS^T takes register r as k step r, its A fragment read along d from the K block in that key order.  dk / dv is
// the mirror image: S = Q K^T and dP = dout V^T with lane = key and registers = queries, then dV^T += dout^T P and dK^T += Q^T dS.
// P and dS never go through LDS and are never transposed.
//
// LDS pitch.  Each staged array is read both down a column (lane = row, for the score products) and along d (lane = d, the two lane
// halves four rows apart, for the gradient products).  One copy with the odd pitch DP + 1 serves both: the column read touches 32
// distinct banks per lane half, the read along d is 32 consecutive words per half, the halves 4 words apart.  A second copy with the
// forward's DP + 8 pitch would separate the halves by 32 banks at the price of half the workgroups per CU at d_head 64.
//
// delta is taken as the diagonal of out dout^T on the MFMA chain that computes dP (see the kernels), not as a lane-local dot product:
// summed in another order it would leave a rounding residue in dP - delta where the exact value is 0 (a query with one visible key).
// Either kernel computes it for the queries it holds, from the out rows.
//
// The caller's workspace [batch][heads][Tq] carries 1 / sum_j exp(scale s_ij - lse_i) from the dq kernel, which runs first, to the
// dk / dv kernel.  In exact arithmetic it is 1; with an f32 lse it is the inverse of the factor that the rounding of lse puts on every
// P of the query (up to exp(5e-4) at scores of 1e4, where an ulp of lse is 1e-3), and multiplying by it takes that factor out.
//
// Masked entries are removed by selection: P and dS are a selected 0, and the exponent's argument is fma(s, scale, -lse) <= ~0, so
// large scores cannot overflow.  Rows that nothing sees are never read: key rows beyond kv_lengths[b] or outside every query's range,
// and the Q, dout, out, lse rows of invalid queries; their gradients are written as exact zeros.
#include "nntk_common.hpp"

#define ATTB_THREADS 256
#define ATTB_TILE 128                   // queries (keys) per workgroup: 4 wavefronts x 32
#define ATTB_ROWS 128                   // batch rows per launch: their key counts ride in the kernel's arguments

struct AttbLens { int v[ATTB_ROWS]; };

struct AttbArgs {
    const float *q, *k, *v, *out, *lse, *dout;
    float *dq, *dk, *dv, *norm;
    long qfs, qbs, kfs, kbs, vfs, vbs, gfs;
    int heads, d_head, Tq, Tk, q_offset, pos0, chunk, left, right, row0, use_lens;
    float scale;
};

// the indices x in [x0, x1) with g(c) - below <= g(x) <= g(c) + above, g(x) = (pos0 + x) / chunk; empty: hi <= lo.
// The keys a query at key index p sees: (p, left, right, 0, kvlen).  The queries that see key j, as key indices: (j, right, left,
// q_offset, one past the last valid query) -- the same rule with left and right exchanged.
__device__ __forceinline__ void attb_range(const AttbArgs &a, int c, int below, int above, int x0, int x1, int &lo, int &hi) {
    const long long g = (a.pos0 + c) / a.chunk;
    const long long l = below < 0 ? (long long)x0 : (g - below) * a.chunk - a.pos0;
    const long long h = above < 0 ? (long long)x1 : (g + above + 1) * a.chunk - a.pos0;
    lo = (int)(l > x0 ? l : x0);
    hi = (int)(h < x1 ? h : x1);
}

// the union of the ranges of the items c0 .. c1 (both ends grow with c, and neighbouring ranges touch); c1 < c0 or nothing seen: lo = hi = 0
__device__ __forceinline__ void attb_span(const AttbArgs &a, int c0, int c1, int below, int above, int x0, int x1, int &lo, int &hi) {
    lo = hi = 0;
    if (c1 < c0) return;
    int x;
    attb_range(a, c0, below, above, x0, x1, lo, x);
    attb_range(a, c1, below, above, x0, x1, x, hi);
    if (hi <= lo) lo = hi = 0;
}

__device__ __forceinline__ int attb_min(int x, int y) { return x < y ? x : y; }

template <int DP, int BK>
__global__ __launch_bounds__(ATTB_THREADS) void attention_dq_kernel(const AttbArgs a, const AttbLens lens) {
    constexpr int KP = DP + 1;
    constexpr int NC = DP / 32, NS = DP / 2;
    constexpr int WPP = 2 * BK / 32;    // wavefronts whose 32 out rows fit the staging area at once
    __shared__ float sh[2 * BK * KP];
    float *const Ks = sh, *const Vs = sh + BK * KP;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, n = lane & 31, kk = lane >> 5;
    const int h = blockIdx.x, b = a.row0 + blockIdx.y;
    const int kvlen = a.use_lens ? lens.v[blockIdx.y] : a.Tk;
    // last query tile first, as in the forward: under a causal mask the late tiles walk the most keys
    const int i0 = (gridDim.z - 1 - blockIdx.z) * ATTB_TILE, i = i0 + 32 * wv + n, p = a.q_offset + i;
    const int qend = attb_min(a.q_offset + a.Tq, kvlen);                 // one past the last valid query, as a key index
    const bool qvalid = i < a.Tq && p < kvlen;
    const int hoff = h * a.d_head;

    int lo = 0, hi = 0, tlo, thi, wlo, whi;
    if (qvalid) attb_range(a, p, a.left, a.right, 0, kvlen, lo, hi);
    attb_span(a, a.q_offset + i0, attb_min(a.q_offset + i0 + ATTB_TILE, qend) - 1, a.left, a.right, 0, kvlen, tlo, thi);
    attb_span(a, a.q_offset + i0 + 32 * wv, attb_min(a.q_offset + i0 + 32 * wv + 32, qend) - 1, a.left, a.right, 0, kvlen, wlo, whi);

    float qr[NS], dor[NS];                                      // Q^T and dout^T as B operands: element 2 s + kk of the lane's query
    float delta = 0.0f, lse = 0.0f;
    const long hd = (long)a.heads * a.d_head;
    {
        const float *qp = a.q + (long)b * a.qbs + (long)(qvalid ? i : 0) * a.qfs + hoff;
        const float *dp = a.dout + ((long)b * a.Tq + (qvalid ? i : 0)) * hd + hoff;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int d = 2 * s + kk;
            const bool live = qvalid && d < a.d_head;
            qr[s] = live ? qp[d] : 0.0f;
            dor[s] = live ? dp[d] : 0.0f;
        }
        if (qvalid) lse = a.lse[((long)b * a.heads + h) * a.Tq + i];
    }
    // delta_i = dout_i . out_i, as the diagonal of out dout^T on the same MFMA chain as dP^T = V dout^T: with one visible key, where
    // out_i is v_j to the bit, dP - delta is an exact 0, as it is in exact arithmetic.  A wavefront stages the out rows of its own queries.
    for (int w0 = 0; w0 < 4; w0 += WPP) {
        const bool mine = wv >= w0 && wv < w0 + WPP;
        float *os = sh + (mine ? wv - w0 : 0) * 32 * KP;
        __syncthreads();
        if (mine)
            for (int e = lane; e < 32 * DP; e += 64) {
                const int r = e / DP, c = e % DP, x = i0 + 32 * wv + r;
                os[r * KP + c] = x < a.Tq && a.q_offset + x < kvlen && c < a.d_head ? a.out[((long)b * a.Tq + x) * hd + hoff + c] : 0.0f;
            }
        __syncthreads();
        if (mine) {
            f32x16 t;
#pragma unroll
            for (int r = 0; r < 16; ++r) t[r] = 0.0f;
#pragma unroll
            for (int st = 0; st < NS; ++st) t = __builtin_amdgcn_mfma_f32_32x32x2f32(os[n * KP + kk + 2 * st], dor[st], t, 0, 0, 0);
#pragma unroll
            for (int r = 0; r < 16; ++r) delta += 8 * (r >> 2) + 4 * kk + (r & 3) == n ? t[r] : 0.0f;      // row n of column n: in one lane half
            delta += __shfl_xor(delta, 32);
        }
    }
    float lsum = 0.0f;                                          // this lane's share of sum_j exp(scale s_ij - lse_i)
    f32x16 dq[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
        for (int r = 0; r < 16; ++r) dq[c][r] = 0.0f;

    if (thi > tlo) {
        const float *kb = a.k + (long)b * a.kbs + hoff, *vb = a.v + (long)b * a.vbs + hoff;
        const int ab1 = (a.pos0 + thi - 1) / BK;
        for (int ab = (a.pos0 + tlo) / BK; ab <= ab1; ++ab) {
            const int j0 = ab * BK - a.pos0;                    // may be negative in the stream's first window: those rows are not keys
            __syncthreads();
            for (int e = tid; e < BK * DP; e += ATTB_THREADS) {
                const int r = e / DP, c = e % DP, j = j0 + r;
                const bool live = j >= tlo && j < thi && c < a.d_head;
                Ks[r * KP + c] = live ? kb[(long)j * a.kfs + c] : 0.0f;
                Vs[r * KP + c] = live ? vb[(long)j * a.vfs + c] : 0.0f;
            }
            __syncthreads();
#pragma unroll 1
            for (int sub = 0; sub < BK / 32; ++sub) {
                const int jb = j0 + 32 * sub;
                if (whi <= wlo || jb + 32 <= wlo || jb >= whi) continue;      // none of this wavefront's queries sees a key here
                f32x16 s, dp;
#pragma unroll
                for (int r = 0; r < 16; ++r) s[r] = dp[r] = 0.0f;
                const float *kp = Ks + (32 * sub + n) * KP + kk, *vp = Vs + (32 * sub + n) * KP + kk;
#pragma unroll
                for (int st = 0; st < NS; ++st) {
                    s = __builtin_amdgcn_mfma_f32_32x32x2f32(kp[2 * st], qr[st], s, 0, 0, 0);
                    dp = __builtin_amdgcn_mfma_f32_32x32x2f32(vp[2 * st], dor[st], dp, 0, 0, 0);
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int j = jb + 8 * (r >> 2) + 4 * kk + (r & 3);
                    const bool vis = j >= lo && j < hi;
                    const float pr = vis ? __expf(__fmaf_rn(s[r], a.scale, -lse)) : 0.0f;
                    lsum += pr;
                    s[r] = vis ? pr * (dp[r] - delta) : 0.0f;
                }
#pragma unroll
                for (int c = 0; c < NC; ++c) {
                    const float *kd = Ks + (32 * sub + 4 * kk) * KP + 32 * c + n;
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        dq[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(kd[(8 * (r >> 2) + (r & 3)) * KP], s[r], dq[c], 0, 0, 0);
                }
            }
        }
    }
    // lse is an f32: at |lse| ~ 1e4 its rounding is a factor of up to exp(5e-4) on every P of the query.  The recomputed row sum
    // carries exactly that factor, so its inverse takes it out again, here and (through the workspace) in the dk / dv kernel.
    lsum += __shfl_xor(lsum, 32);
    const float norm = qvalid ? 1.0f / lsum : 0.0f;             // a valid query sees itself: lsum > 0
    if (i >= a.Tq) return;
    if (kk == 0) a.norm[((long)b * a.heads + h) * a.Tq + i] = norm;
    float *gp = a.dq + ((long)b * a.Tq + i) * a.gfs + hoff;
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int d = 32 * c + 8 * (r >> 2) + 4 * kk + (r & 3);
            if (d < a.d_head) gp[d] = qvalid ? __fmul_rn(__fmul_rn(dq[c][r], norm), a.scale) : 0.0f;
        }
}

template <int DP, int BQ>
__global__ __launch_bounds__(ATTB_THREADS) void attention_dkv_kernel(const AttbArgs a, const AttbLens lens) {
    constexpr int QP = DP + 1;
    constexpr int NC = DP / 32, NS = DP / 2;
    __shared__ float Qs[BQ * QP];
    __shared__ float Ds[BQ * QP];
    __shared__ float Os[BQ * QP];
    __shared__ float Ls[BQ];
    __shared__ float Ns[BQ];
    __shared__ float Es[BQ];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, n = lane & 31, kk = lane >> 5;
    const int h = blockIdx.x, b = a.row0 + blockIdx.y;
    const int kvlen = a.use_lens ? lens.v[blockIdx.y] : a.Tk;
    // first key tile first: under a causal mask the early keys are seen by the most queries
    const int j0t = blockIdx.z * ATTB_TILE, j = j0t + 32 * wv + n;
    const int qend = attb_min(a.q_offset + a.Tq, kvlen);
    const int hoff = h * a.d_head;
    const long hd = (long)a.heads * a.d_head;

    // the valid queries that see this lane's key, this tile's keys, this wavefront's keys, as key indices p = q_offset + i
    int lo = 0, hi = 0, tlo, thi, wlo, whi;
    if (j < kvlen) attb_range(a, j, a.right, a.left, a.q_offset, qend, lo, hi);
    const bool seen = j < kvlen && hi > lo;
    attb_span(a, j0t, attb_min(j0t + ATTB_TILE, kvlen) - 1, a.right, a.left, a.q_offset, qend, tlo, thi);
    attb_span(a, j0t + 32 * wv, attb_min(j0t + 32 * wv + 32, kvlen) - 1, a.right, a.left, a.q_offset, qend, wlo, whi);

    float kr[NS], vr[NS];                                       // K^T and V^T as B operands: element 2 s + kk of the lane's key
    {
        const float *kp = a.k + (long)b * a.kbs + (long)(seen ? j : 0) * a.kfs + hoff;
        const float *vp = a.v + (long)b * a.vbs + (long)(seen ? j : 0) * a.vfs + hoff;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int d = 2 * s + kk;
            const bool live = seen && d < a.d_head;
            kr[s] = live ? kp[d] : 0.0f;
            vr[s] = live ? vp[d] : 0.0f;
        }
    }
    f32x16 dk[NC], dv[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
        for (int r = 0; r < 16; ++r) dk[c][r] = dv[c][r] = 0.0f;

    if (thi > tlo) {
        const float *qb = a.q + (long)b * a.qbs + hoff, *db = a.dout + (long)b * a.Tq * hd + hoff;
        const float *ob = a.out + (long)b * a.Tq * hd + hoff;
        const float *lb = a.lse + ((long)b * a.heads + h) * a.Tq, *nb = a.norm + ((long)b * a.heads + h) * a.Tq;
        const int ab1 = (a.pos0 + thi - 1) / BQ;
        for (int ab = (a.pos0 + tlo) / BQ; ab <= ab1; ++ab) {
            const int p0 = ab * BQ - a.pos0;
            __syncthreads();
            for (int e = tid; e < BQ * DP; e += ATTB_THREADS) {
                const int r = e / DP, c = e % DP, p = p0 + r;
                const bool live = p >= tlo && p < thi && c < a.d_head;
                Qs[r * QP + c] = live ? qb[(long)(p - a.q_offset) * a.qfs + c] : 0.0f;
                Ds[r * QP + c] = live ? db[(long)(p - a.q_offset) * hd + c] : 0.0f;
                Os[r * QP + c] = live ? ob[(long)(p - a.q_offset) * hd + c] : 0.0f;
            }
            if (tid < BQ) {
                const int p = p0 + tid;
                const bool live = p >= tlo && p < thi;
                Ls[tid] = live ? lb[p - a.q_offset] : 0.0f;
                Ns[tid] = live ? nb[p - a.q_offset] : 0.0f;
            }
            __syncthreads();
            // delta of the block's queries: the diagonal of dout out^T on the MFMA chain of dP = dout V^T (see the dq kernel), one
            // wavefront per 32 queries
            if (wv < BQ / 32) {
                f32x16 t;
#pragma unroll
                for (int r = 0; r < 16; ++r) t[r] = 0.0f;
                const float *dop = Ds + (32 * wv + n) * QP + kk, *op = Os + (32 * wv + n) * QP + kk;
#pragma unroll
                for (int st = 0; st < NS; ++st) t = __builtin_amdgcn_mfma_f32_32x32x2f32(dop[2 * st], op[2 * st], t, 0, 0, 0);
                float delta = 0.0f;
#pragma unroll
                for (int r = 0; r < 16; ++r) delta += 8 * (r >> 2) + 4 * kk + (r & 3) == n ? t[r] : 0.0f;
                delta += __shfl_xor(delta, 32);
                if (kk == 0) Es[32 * wv + n] = delta;
            }
            __syncthreads();
#pragma unroll 1
            for (int sub = 0; sub < BQ / 32; ++sub) {
                const int pb = p0 + 32 * sub;
                if (whi <= wlo || pb + 32 <= wlo || pb >= whi) continue;      // no query here sees one of this wavefront's keys
                f32x16 s, dp;
#pragma unroll
                for (int r = 0; r < 16; ++r) s[r] = dp[r] = 0.0f;
                const float *qp = Qs + (32 * sub + n) * QP + kk, *dop = Ds + (32 * sub + n) * QP + kk;
#pragma unroll
                for (int st = 0; st < NS; ++st) {
                    s = __builtin_amdgcn_mfma_f32_32x32x2f32(qp[2 * st], kr[st], s, 0, 0, 0);
                    dp = __builtin_amdgcn_mfma_f32_32x32x2f32(dop[2 * st], vr[st], dp, 0, 0, 0);
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int x = 32 * sub + 8 * (r >> 2) + 4 * kk + (r & 3), p = p0 + x;
                    const bool vis = p >= lo && p < hi;
                    s[r] = vis ? __expf(__fmaf_rn(s[r], a.scale, -Ls[x])) * Ns[x] : 0.0f;
                    dp[r] = vis ? s[r] * (dp[r] - Es[x]) : 0.0f;
                }
#pragma unroll
                for (int c = 0; c < NC; ++c) {
                    const float *dt = Ds + (32 * sub + 4 * kk) * QP + 32 * c + n, *qt = Qs + (32 * sub + 4 * kk) * QP + 32 * c + n;
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        dv[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(dt[(8 * (r >> 2) + (r & 3)) * QP], s[r], dv[c], 0, 0, 0);
                        dk[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(qt[(8 * (r >> 2) + (r & 3)) * QP], dp[r], dk[c], 0, 0, 0);
                    }
                }
            }
        }
    }
    if (j >= a.Tk) return;
    float *gk = a.dk + ((long)b * a.Tk + j) * a.gfs + hoff, *gv = a.dv + ((long)b * a.Tk + j) * a.gfs + hoff;
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int d = 32 * c + 8 * (r >> 2) + 4 * kk + (r & 3);
            if (d < a.d_head) {
                gk[d] = seen ? __fmul_rn(dk[c][r], a.scale) : 0.0f;
                gv[d] = seen ? dv[c][r] : 0.0f;
            }
        }
}

template <int DP, int BLK>
static void attb_launch(const AttbArgs &a, const AttbLens &lens, int rows) {
    const dim3 gq((unsigned)a.heads, (unsigned)rows, (unsigned)nntk_cdiv(a.Tq, ATTB_TILE));
    const dim3 gk((unsigned)a.heads, (unsigned)rows, (unsigned)nntk_cdiv(a.Tk, ATTB_TILE));
    hipLaunchKernelGGL((attention_dq_kernel<DP, BLK>), gq, dim3(ATTB_THREADS), 0, nntk_stream(), a, lens);      // writes the workspace: runs first
    hipLaunchKernelGGL((attention_dkv_kernel<DP, BLK>), gk, dim3(ATTB_THREADS), 0, nntk_stream(), a, lens);
}

extern "C" int nntk_shim_attention_backward(const float *d_q, const float *d_k, const float *d_v, const float *d_out, const float *d_lse,
                                            const float *d_dout, int batch, int heads, int d_head, int Tq, int Tk, long q_frame_stride,
                                            long q_batch_stride, long k_frame_stride, long k_batch_stride, long v_frame_stride,
                                            long v_batch_stride, const int *h_kv_lengths, int q_offset, int pos0, int chunk, int left,
                                            int right, float scale, long grad_frame_stride, float *d_dq, float *d_dk, float *d_dv,
                                            float *d_ws) {
    if (batch <= 0) return 0;
    if (d_head < 1 || d_head > NNTK_ATTENTION_MAX_D_HEAD || heads < 1 || heads > NNTK_ATTENTION_MAX_HEADS || Tq < 1 || Tk < 1 ||
        Tq > NNTK_ATTENTION_MAX_FRAMES || Tk > NNTK_ATTENTION_MAX_FRAMES || chunk < 1 || q_offset < 0 || q_offset + Tq > Tk ||
        grad_frame_stride < (long)heads * d_head)
        return nntk_fail_msg("nntk_attention_backward_device: a shape is outside what the kernels take");
    AttbArgs a = {d_q, d_k, d_v, d_out, d_lse, d_dout, d_dq, d_dk, d_dv, d_ws, q_frame_stride, q_batch_stride, k_frame_stride, k_batch_stride,
                  v_frame_stride, v_batch_stride, grad_frame_stride, heads, d_head, Tq, Tk, q_offset, pos0, chunk, left, right, 0,
                  h_kv_lengths != NULL, scale};
    for (int row0 = 0; row0 < batch; row0 += ATTB_ROWS) {
        const int rows = batch - row0 < ATTB_ROWS ? batch - row0 : ATTB_ROWS;
        AttbLens lens;
        for (int r = 0; r < ATTB_ROWS; ++r) lens.v[r] = h_kv_lengths && r < rows ? h_kv_lengths[row0 + r] : 0;
        a.row0 = row0;
        if (d_head <= 32) attb_launch<32, 64>(a, lens, rows);
        else if (d_head <= 64) attb_launch<64, 64>(a, lens, rows);
        else attb_launch<128, 32>(a, lens, rows);
        NNTK_LAUNCH_CHECK("attention_backward kernels");
    }
    return 0;
}
