// rnnt.hip -- the RNN-Transducer (Graves, 2012): the per-row negative log-likelihood over the lattice of unnormalised scores
// [B][T][U1 = max_label_len + 1][V], its gradient with respect to those scores, and the joiner that makes the tensor the scores are
// projected from (out = act(enc[b][t] + pred[b][u])) with its backward.
//
// Range.  alpha(t, u) sums binomial(t + u, u) paths of t + u emissions each: like the CTC variables it is an f32 mantissa with an int32
// exponent of its own (ctc_xf.hpp).  The emissions exp(x - lse) are carried the same way, straight from the base-2 logarithm -- mantissa
// exp2(frac), exponent floor -- so a label 170 bits below its cell's maximum still has all its mantissa bits; the exponent is floored at
// RNNT_EMIN, which keeps every sum of T + U exponents inside an int32 and above CTC_EZERO (a finite score never becomes a zero).
//
// Work split, three launches; the score tensor is read twice and the gradient written once.
//  rnnt_emit_kernel: a wavefront per live cell: maximum, then the sum of exp(x - max) accumulated in double (the second read of the row
//    comes from the cache).  Kept per cell: the blank's and the next label's emission (16 bytes) and, for the gradient, lse as a double.
//  rnnt_lattice_kernel: one 256-lane workgroup per (row, direction) -- blockIdx.y = 0 runs alpha over the anti-diagonals t + u = n
//    upwards, 1 runs beta downwards, concurrently -- lanes over u (a lane owns u = tid, tid + 256, ...).  The previous diagonal sits in
//    double-buffered LDS, one LDS-only barrier per diagonal; the emissions of the NEXT diagonal's cells are loaded before the barrier.
//    P = alpha(T-1, U) p_blank(T-1, U) comes out of the forward direction alone: the loss bits do not depend on whether a gradient is asked.
//  rnnt_grad_kernel: a wavefront per cell: three scalars from alpha, beta, the emissions and P (the occupancy A = alpha beta / P, and
//    the two outgoing flows), then V scores in and g[v] = A exp(x[v] - lse) - [v = blank] flow_blank - [v = label] flow_label out.
//    Padding cells (t >= T_b or u > U_b) are zero-filled with 16-byte stores.
// No atomics anywhere; every reduction is a fixed butterfly or a fixed-order loop.
// The per-cell bodies of the emit and gradient kernels live in rnnt_common.hpp, on a score source: rnnt_pruned.hip runs them on a sum
// of two rows and on a band of the lattice, and its bit contracts with this unit rest on that.
#include "rnnt_common.hpp"                 // the layout and its pointers, the int upload, the emission: shared by the four units

#define RNNT_JOINT_UNROLL 4               // terms of a joiner-backward sum loaded together (added in ascending order all the same)

// VEC: V % 4 == 0 and the tensor 16-byte aligned, so every row is: 16-byte loads.  The cell's body: rnnt_emit_row (rnnt_common.hpp)
template <bool VEC>
__global__ __launch_bounds__(CTC_THREADS) void rnnt_emit_kernel(const float *__restrict__ logits, int B, int T, int U1, int V, int blank,
                                                                const int *__restrict__ ints, float4 *__restrict__ em,
                                                                double *__restrict__ lse_out, long cells) {
    const int lane = threadIdx.x & 63;
    for (long c = blockIdx.x * 4L + (threadIdx.x >> 6); c < cells; c += gridDim.x * 4L) {
        const RnntCell q = rnnt_cell(c, T, U1);
        const int Ub = ints[B + q.b];
        if (q.t >= ints[q.b] || q.u > Ub) continue;
        const RnntRow<false> row = {logits + c * V, nullptr};
        rnnt_emit_row<VEC, false>(row, V, blank, q.u < Ub ? ints + 2L * B + (long)q.b * (U1 - 1) + q.u : nullptr, lane, em + c,
                                  lse_out ? lse_out + c : nullptr);
    }
}

// NJ > 0: a lane's cells of a diagonal (at most NJ) take their emissions from registers, loaded one diagonal ahead; NJ = 0: any U1
// that fits the LDS, emissions fetched inside the step.  LDS per u: forward, alpha p_blank | alpha p_label of the lane's cell -- what
// flows on to (t + 1, u) and to (t, u + 1); backward, beta itself.
template <int NJ>
__global__ __launch_bounds__(CTC_THREADS) void rnnt_lattice_kernel(int B, int T, int U1, const int *__restrict__ ints,
                                                                   const float4 *__restrict__ em, float2 *ws_alpha, float2 *ws_beta,
                                                                   float *hdr, float *loss_rows) {
    extern __shared__ __align__(16) unsigned char rnnt_smem[];
    float4 *st = (float4 *)rnnt_smem;                                       // [2][U1]
    const int b = blockIdx.x, dir = blockIdx.y, tid = threadIdx.x;
    const int Tb = ints[b], Ub = ints[B + b];
    const long base = (long)b * T * U1;
    const float4 *e = em + base;
    float2 *ws = dir ? ws_beta : ws_alpha;
    if (ws) ws += base;
    const int ND = Tb + Ub;                                                 // diagonals n = t + u = 0 .. ND - 1
    constexpr int NR = NJ > 0 ? NJ : 1;
    const float4 none = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    auto live = [&](int n, int u) { return u <= Ub && n - u >= 0 && n - u < Tb; };
    float4 en[NR];
    if (NJ > 0) {
        const int n0 = dir ? ND - 1 : 0;
#pragma unroll
        for (int j = 0; j < NR; ++j) {
            const int u = tid + CTC_THREADS * j;
            en[j] = none;
            if (live(n0, u)) en[j] = e[(long)(n0 - u) * U1 + u];
        }
    }
    int cur = 0;
    for (int i = 0; i < ND; ++i) {
        const int n = dir ? ND - 1 - i : i;
        float4 ec[NR];
        if (NJ > 0) {
#pragma unroll
            for (int j = 0; j < NR; ++j) ec[j] = en[j];
            if (i + 1 < ND) {                                               // the next diagonal's emissions: not on the dependent chain
                const int nn = dir ? n - 1 : n + 1;
#pragma unroll
                for (int j = 0; j < NR; ++j) {
                    const int u = tid + CTC_THREADS * j;
                    en[j] = none;
                    if (live(nn, u)) en[j] = e[(long)(nn - u) * U1 + u];
                }
            }
        }
        const float4 *src = st + cur * U1;
        float4 *dst = st + (cur ^ 1) * U1;
        auto cell = [&](int u, float4 e4) {
            const int t = n - u;
            xf pb, py;
            pb.m = e4.x; pb.e = __float_as_int(e4.y);
            py.m = e4.z; py.e = __float_as_int(e4.w);
            if (dir == 0) {
                xf a;
                if (n == 0) {
                    a = xf_one();
                } else {                                                    // from (t - 1, u) by a blank, then from (t, u - 1) by label u
                    const xf ft = t >= 1 ? xf_unpack(make_float2(src[u].x, src[u].y)) : xf_zero();
                    const xf fu = u >= 1 ? xf_unpack(make_float2(src[u - 1].z, src[u - 1].w)) : xf_zero();
                    a = xf_add3(ft, fu, xf_zero());
                }
                if (ws) ws[(long)t * U1 + u] = xf_pack(a);
                const xf ab = xf_times(a, pb), ay = xf_times(a, py);
                dst[u] = make_float4(ab.m, __int_as_float(ab.e), ay.m, __int_as_float(ay.e));
                if (i == ND - 1) {                                          // the one cell of the last diagonal: (Tb - 1, Ub)
                    hdr[2 * b] = ab.m;
                    hdr[2 * b + 1] = __int_as_float(ab.e);
                    // once per row: double, libm log
                    loss_rows[b] = ab.m == 0.0f ? INFINITY : (float)-((double)ab.e * 0.69314718055994530942 + log((double)ab.m));
                }
            } else {                                                        // beta(Tb, Ub) stands for 1; beta(Tb, u < Ub) and beta(t, Ub + 1) are 0
                const xf bt = t + 1 < Tb ? xf_unpack(make_float2(src[u].x, src[u].y)) : u == Ub ? xf_one() : xf_zero();
                const xf bu = u < Ub ? xf_unpack(make_float2(src[u + 1].x, src[u + 1].y)) : xf_zero();
                const xf v = xf_add3(xf_times(bt, pb), xf_times(bu, py), xf_zero());
                ws[(long)t * U1 + u] = xf_pack(v);
                dst[u] = make_float4(v.m, __int_as_float(v.e), 0.0f, 0.0f);
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

// the cell's bodies: rnnt_cell_flows, rnnt_grad_row, rnnt_zero_row (rnnt_common.hpp)
template <bool VEC>
__global__ __launch_bounds__(CTC_THREADS) void rnnt_grad_kernel(const float *__restrict__ logits, int B, int T, int U1, int V, int blank,
                                                                const int *__restrict__ ints, const float4 *__restrict__ em,
                                                                const double *__restrict__ lse_in, const float2 *__restrict__ wa,
                                                                const float2 *__restrict__ wb, const float *__restrict__ hdr,
                                                                float *__restrict__ dlogits, long cells) {
    const int lane = threadIdx.x & 63;
    for (long c = blockIdx.x * 4L + (threadIdx.x >> 6); c < cells; c += gridDim.x * 4L) {
        const RnntCell q = rnnt_cell(c, T, U1);
        const int Tb = ints[q.b], Ub = ints[B + q.b];
        float *g = dlogits + c * V;
        const float mP = hdr[2 * q.b];
        if (q.t >= Tb || q.u > Ub || !(mP > 0.0f)) {                        // padding, or a row no path reaches (P = 0): zeros
            rnnt_zero_row(g, V, lane);
            continue;
        }
        const RnntFlows f = rnnt_cell_flows(c, q.t, q.u, Tb, Ub, U1, em, wa, wb, mP, __float_as_int(hdr[2 * q.b + 1]));
        const int y = q.u < Ub ? ints[2L * B + (long)q.b * (U1 - 1) + q.u] : -1;
        const RnntRow<false> row = {logits + c * V, nullptr};
        rnnt_grad_row<VEC, false>(row, g, V, blank, y, f, lse_in[c], lane);
    }
}

// ---- the joiner: out[b][t][u][:] = act(enc[b][t][:] + pred[b][u][:]); activation 0 identity, 1 tanh (tanhf), 2 relu (max(x, 0)) ----
// W = 4: J % 4 == 0 and the three tensors 16-byte aligned; n = elements / W
template <int W>
__global__ __launch_bounds__(256) void rnnt_joint_kernel(const float *__restrict__ enc, const float *__restrict__ pred, int T, int U1, int JW,
                                                         int kind, float *__restrict__ out, long n) {
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += gridDim.x * 256L) {
        const long cell = i / JW;
        const int j = (int)(i - cell * JW);
        const long bt = cell / U1;
        const int u = (int)(cell - bt * U1);
        const long bu = bt / T * U1 + u;
        if (W == 4) {
            const f32x4 a = ((const f32x4 *)enc)[bt * JW + j], p = ((const f32x4 *)pred)[bu * JW + j];
            f32x4 r;
#pragma unroll
            for (int k = 0; k < 4; ++k) r[k] = rnnt_act(kind, a[k] + p[k]);
            ((f32x4 *)out)[i] = r;
        } else {
            out[i] = rnnt_act(kind, enc[bt * JW + j] + pred[bu * JW + j]);
        }
    }
}

// dst[o][r] = sum over k < R, ascending, of dout[o * ostride + k * rstride + r] * act'(out[the same]); one accumulator per element.
// d_enc: o = (b, t), r = j, k = u; d_pred: o = b, r = (u, j), k = t
__global__ __launch_bounds__(256) void rnnt_joint_reduce_kernel(const float *__restrict__ out, const float *__restrict__ dout, long n, long M,
                                                                long ostride, int R, long rstride, int kind, float *__restrict__ dst) {
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += gridDim.x * 256L) {
        const long o = i / M;
        const long at = o * ostride + (i - o * M);
        float acc = 0.0f;
        int k = 0;
        for (; k + RNNT_JOINT_UNROLL <= R; k += RNNT_JOINT_UNROLL) {
            float d[RNNT_JOINT_UNROLL], f[RNNT_JOINT_UNROLL];
#pragma unroll
            for (int w = 0; w < RNNT_JOINT_UNROLL; ++w) {
                d[w] = dout[at + (k + w) * rstride];
                f[w] = kind ? out[at + (k + w) * rstride] : 0.0f;
            }
#pragma unroll
            for (int w = 0; w < RNNT_JOINT_UNROLL; ++w) acc += d[w] * rnnt_dact(kind, f[w]);
        }
        for (; k < R; ++k) acc += dout[at + k * rstride] * rnnt_dact(kind, kind ? out[at + k * rstride] : 0.0f);
        dst[i] = acc;
    }
}

// the lattice on the emissions, for this unit and for rnnt_fused.hip; wa / wb NULL: the forward direction alone
int nntk_rnnt_lattice_launch(int B, int T, int U1, const int *d_ints, const float4 *em, float2 *wa, float2 *wb, float *hdr,
                             float *d_loss_rows) {
    const size_t lds = 2 * (size_t)U1 * sizeof(float4);
    const dim3 grid((unsigned)B, wb ? 2 : 1);
#define RNNT_AB(NJ)                                                                                                          \
    do {                                                                                                                     \
        if (lds > 48 * 1024 && nntk_set_max_dynamic_lds((const void *)rnnt_lattice_kernel<NJ>, lds)) return -1;               \
        hipLaunchKernelGGL(rnnt_lattice_kernel<NJ>, grid, dim3(CTC_THREADS), lds, nntk_stream(), B, T, U1, d_ints, em, wa, wb, \
                           hdr, d_loss_rows);                                                                                \
    } while (0)
    if (U1 <= CTC_THREADS) RNNT_AB(1);
    else if (U1 <= 2 * CTC_THREADS) RNNT_AB(2);
    else RNNT_AB(0);
#undef RNNT_AB
    NNTK_LAUNCH_CHECK("rnnt_lattice_kernel");
    return 0;
}

// the emissions of the stored scores, for this unit and for rnnt_align.hip; d_logits 16-byte aligned; lse NULL: not kept
int nntk_rnnt_emit_launch(const float *d_logits, int B, int T, int U1, int V, int blank, const int *d_ints, float4 *em, double *lse) {
    const long cells = (long)B * T * U1;
    const dim3 cgrid(rnnt_grid(cells, 4));
    if ((V & 3) == 0)
        hipLaunchKernelGGL(rnnt_emit_kernel<true>, cgrid, dim3(CTC_THREADS), 0, nntk_stream(), d_logits, B, T, U1, V, blank, d_ints, em, lse, cells);
    else
        hipLaunchKernelGGL(rnnt_emit_kernel<false>, cgrid, dim3(CTC_THREADS), 0, nntk_stream(), d_logits, B, T, U1, V, blank, d_ints, em, lse, cells);
    NNTK_LAUNCH_CHECK("rnnt_emit_kernel");
    return 0;
}

// rnnt_joint_reduce_kernel, for this unit and for rnnt_pruned.hip (the banded joiner's d_enc: the same sum, S terms wide)
int nntk_rnnt_joint_reduce_launch(const float *d_out_fwd, const float *d_dout, long n, long M, long ostride, int R, long rstride, int kind,
                                  float *d_dst) {
    hipLaunchKernelGGL(rnnt_joint_reduce_kernel, dim3(rnnt_grid(n, 256)), dim3(256), 0, nntk_stream(), d_out_fwd, d_dout, n, M, ostride, R,
                       rstride, kind, d_dst);
    NNTK_LAUNCH_CHECK("rnnt_joint_reduce_kernel");
    return 0;
}

extern "C" {

size_t nntk_shim_rnnt_workspace_floats(int batch, int T, int max_label_len, int want_grad) {
    return rnnt_layout(batch, T, max_label_len, want_grad).total;
}

int nntk_shim_rnnt_loss(const float *d_logits, int B, int T, int V, const int *h_input_lengths, const int *h_labels,
                        const int *h_label_lengths, int maxL, int blank, float *d_loss_rows, float *d_dlogits, float *d_ws) {
    if (B <= 0) return 0;
    if (!rnnt_lattice_fits(T, maxL))
        return nntk_fail_msg("nntk_rnnt_loss_device: max_label_len or T + max_label_len is beyond the lattice kernel's limits");
    if ((((uintptr_t)d_ws | (uintptr_t)d_logits | (uintptr_t)d_dlogits) & 15) != 0)
        return nntk_fail_msg("nntk_rnnt_loss_device: the tensors and the workspace must be 16-byte aligned");
    const int U1 = maxL + 1;
    const long cells = (long)B * T * U1;
    const RnntParts w = rnnt_parts(d_ws, rnnt_layout(B, T, maxL, d_dlogits != nullptr), d_dlogits != nullptr);
    if (rnnt_upload_ints(w.ints, B, maxL, h_input_lengths, h_labels, h_label_lengths)) return -1;
    const bool vec = (V & 3) == 0;
    const dim3 cgrid(rnnt_grid(cells, 4));
    if (nntk_rnnt_emit_launch(d_logits, B, T, U1, V, blank, w.ints, w.em, w.lse)) return -1;
    if (nntk_rnnt_lattice_launch(B, T, U1, w.ints, w.em, w.alpha, w.beta, w.hdr, d_loss_rows)) return -1;
    if (d_dlogits) {
        if (vec)
            hipLaunchKernelGGL(rnnt_grad_kernel<true>, cgrid, dim3(CTC_THREADS), 0, nntk_stream(), d_logits, B, T, U1, V, blank, w.ints, w.em,
                               w.lse, w.alpha, w.beta, w.hdr, d_dlogits, cells);
        else
            hipLaunchKernelGGL(rnnt_grad_kernel<false>, cgrid, dim3(CTC_THREADS), 0, nntk_stream(), d_logits, B, T, U1, V, blank, w.ints, w.em,
                               w.lse, w.alpha, w.beta, w.hdr, d_dlogits, cells);
        NNTK_LAUNCH_CHECK("rnnt_grad_kernel");
    }
    return 0;
}

int nntk_shim_rnnt_joint(const float *d_enc, const float *d_pred, int B, int T, int U1, int J, int kind, float *d_out) {
    const long n = (long)B * T * U1 * J;
    if (n <= 0) return 0;
    if ((J & 3) == 0 && (((uintptr_t)d_enc | (uintptr_t)d_pred | (uintptr_t)d_out) & 15) == 0)
        hipLaunchKernelGGL(rnnt_joint_kernel<4>, dim3(rnnt_grid(n / 4, 256)), dim3(256), 0, nntk_stream(), d_enc, d_pred, T, U1, J / 4, kind,
                           d_out, n / 4);
    else
        hipLaunchKernelGGL(rnnt_joint_kernel<1>, dim3(rnnt_grid(n, 256)), dim3(256), 0, nntk_stream(), d_enc, d_pred, T, U1, J, kind, d_out, n);
    NNTK_LAUNCH_CHECK("rnnt_joint_kernel");
    return 0;
}

int nntk_shim_rnnt_joint_backward(const float *d_out_fwd, const float *d_dout, int B, int T, int U1, int J, int kind, float *d_denc,
                                  float *d_dpred) {
    if ((long)B * T * U1 * J <= 0) return 0;
    if (nntk_rnnt_joint_reduce_launch(d_out_fwd, d_dout, (long)B * T * J, (long)J, (long)U1 * J, U1, (long)J, kind, d_denc)) return -1;
    return nntk_rnnt_joint_reduce_launch(d_out_fwd, d_dout, (long)B * U1 * J, (long)U1 * J, (long)T * U1 * J, T, (long)U1 * J, kind, d_dpred);
}

}  // extern "C"
