// rnnt_pruned.hip -- the pruned RNN-Transducer training loss (Kuang et al., 2022), in its three steps and the joiner between them.
//  1. the simple loss: the lattice on score(t, u, v) = am[b][t][v] + lm[b][u][v], never stored: rnnt_emit_row (rnnt_common.hpp) on the sum
//     source, rnnt.hip's lattice kernel unchanged, then per cell the occupancy and the two flows (16 bytes a cell), then two reductions
//     of the per-cell gradient g(t, u, v) -- over u into d_am, over t into d_lm -- one thread per output element, lanes over v, the
//     summation index ascending, the accumulator double.  The scores are recomputed in each reduction: T U1 V exponentials a row each,
//     on operands that stay in the cache.
//  2. the prune ranges: per frame the window of S label positions with the largest occupancy (the lowest on a tie), then one forward
//     pass per row that makes the windows a connected band from (0, 0) to (T_b - 1, U_b).
//  3. the banded loss on scores [B][T][S][V], cell (t, s) standing for lattice cell (t, r[t] + s): the band's emissions scattered into
//     the full [B][T][U1] emission array, the arithmetic's zero elsewhere; rnnt.hip's lattice kernel unchanged; rnnt_grad_row per band
//     cell.  Mass that leaves the band meets a zero emission; beta is zero outside it, so no flow comes back.
//  The banded joiner gathers pred[b][r[t] + s] per frame; its backward sums d_enc over s with rnnt.hip's reduction and gathers d_pred
//  per (b, u) over the frames whose window holds u, t ascending.
// The ranges are device data the host never sees: every kernel clamps a value into [0, U1 - S] before it indexes anything with it.
// No atomics anywhere; every sum is a fixed-order loop or rnnt_common.hpp's butterfly.
#include "rnnt_common.hpp"

__device__ __forceinline__ int rnnt_range(const int *__restrict__ ranges, long bt, int U1, int S) { return min(max(ranges[bt], 0), U1 - S); }

// ---- 1. the simple loss ----
// VEC: V % 4 == 0 and both tensors 16-byte aligned
template <bool VEC>
__global__ __launch_bounds__(CTC_THREADS) void rnnt_simple_emit_kernel(const float *__restrict__ am, const float *__restrict__ lm, int B, int T,
                                                                       int U1, int V, int blank, const int *__restrict__ ints,
                                                                       float4 *__restrict__ em, double *__restrict__ lse_out, long cells) {
    const int lane = threadIdx.x & 63;
    for (long c = blockIdx.x * 4L + (threadIdx.x >> 6); c < cells; c += gridDim.x * 4L) {
        const RnntCell q = rnnt_cell(c, T, U1);
        const int Ub = ints[B + q.b];
        if (q.t >= ints[q.b] || q.u > Ub) continue;
        const RnntRow<true> row = {am + ((long)q.b * T + q.t) * V, lm + ((long)q.b * U1 + q.u) * V};
        rnnt_emit_row<VEC, true>(row, V, blank, q.u < Ub ? ints + 2L * B + (long)q.b * (U1 - 1) + q.u : nullptr, lane, em + c,
                                 lse_out ? lse_out + c : nullptr);
    }
}

// a thread per cell: coef (occupancy, flow by the blank, flow by the label, the label or -1) for the reductions, and the occupancy
// itself for the caller; zeros on padding and in rows with P = 0.  Either output may be NULL
__global__ __launch_bounds__(256) void rnnt_simple_cell_kernel(int B, int T, int U1, const int *__restrict__ ints, const float4 *__restrict__ em,
                                                               const float2 *__restrict__ wa, const float2 *__restrict__ wb,
                                                               const float *__restrict__ hdr, float4 *__restrict__ coef,
                                                               float *__restrict__ occ, long cells) {
    for (long c = blockIdx.x * 256L + threadIdx.x; c < cells; c += gridDim.x * 256L) {
        const RnntCell q = rnnt_cell(c, T, U1);
        const int Tb = ints[q.b], Ub = ints[B + q.b];
        const float mP = hdr[2 * q.b];
        RnntFlows f = {0.0f, 0.0f, 0.0f};
        int y = -1;
        if (q.t < Tb && q.u <= Ub && mP > 0.0f) {
            f = rnnt_cell_flows(c, q.t, q.u, Tb, Ub, U1, em, wa, wb, mP, __float_as_int(hdr[2 * q.b + 1]));
            if (q.u < Ub) y = ints[2L * B + (long)q.b * (U1 - 1) + q.u];
        }
        if (coef) coef[c] = make_float4(f.occ, f.fb, f.fy, __int_as_float(y));
        if (occ) occ[c] = f.occ;
    }
}

// OVER_U: d_am[b][t][v] = sum over u <= U_b of g(t, u, v); else d_lm[b][u][v] = sum over t < T_b.  A thread per output element, v fastest
template <bool OVER_U>
__global__ __launch_bounds__(256) void rnnt_simple_reduce_kernel(const float *__restrict__ am, const float *__restrict__ lm, int B, int T, int U1,
                                                                 int V, int blank, const int *__restrict__ ints, const float4 *__restrict__ coef,
                                                                 const double *__restrict__ lse, const float *__restrict__ hdr,
                                                                 float *__restrict__ dst, long n) {
    const int R = OVER_U ? T : U1;                                          // rows of dst per batch row
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += gridDim.x * 256L) {
        const long o = i / V;
        const int v = (int)(i - o * V);
        const int b = (int)(o / R), k = (int)(o - (long)b * R);
        const int Tb = ints[b], Ub = ints[B + b];
        double acc = 0.0;
        if (hdr[2 * b] > 0.0f && k < (OVER_U ? Tb : Ub + 1)) {
            const int N = OVER_U ? Ub + 1 : Tb;
            const float fixed = OVER_U ? am[i] : lm[i];
            for (int j = 0; j < N; ++j) {
                const int t = OVER_U ? k : j, u = OVER_U ? j : k;
                const long c = ((long)b * T + t) * U1 + u;
                const float4 q = coef[c];
                const RnntFlows f = {q.x, q.y, q.z};
                const float other = OVER_U ? lm[((long)b * U1 + u) * V + v] : am[((long)b * T + t) * V + v];
                acc += (double)rnnt_grad_value(f, lse[c], blank, __float_as_int(q.w), fixed + other, v);    // am + lm, as the emissions formed it
            }
        }
        dst[i] = (float)acc;
    }
}

// ---- 2. the prune ranges: a workgroup per row.  Threads over t pick s0[t] into ranges; after the barrier thread 0 walks the row ----
__global__ __launch_bounds__(256) void rnnt_prune_kernel(const float *__restrict__ occ, int B, int T, int U1, int S, const int *__restrict__ ints,
                                                         int *ranges) {
    const int b = blockIdx.x;
    const int Tb = ints[b], Ub = ints[B + b];
    const int fin = max(0, Ub + 1 - S);
    int *r = ranges + (long)b * T;
    for (int t = threadIdx.x; t < T; t += 256) {
        int s0 = fin;                                                       // frames past the row's end
        if (t < Tb) {
            const float *o = occ + ((long)b * T + t) * U1;
            double best = 0.0;
            s0 = 0;
            for (int s = 0; s <= fin; ++s) {
                double w = 0.0;
                for (int u = s; u < s + S; ++u) w += (double)o[u];
                if (s == 0 || w > best) { best = w; s0 = s; }
            }
        }
        r[t] = s0;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        long prev = 0;
        for (int t = 0; t < Tb; ++t) {
            const long lo = max(0L, fin - (long)(Tb - 1 - t) * (S - 1)), hi = min((long)fin, (long)t * (S - 1));
            const long L = max(lo, prev), H = min(hi, prev + S - 1);
            prev = min(max((long)r[t], L), H);
            r[t] = (int)prev;
        }
    }
}

// ---- the banded joiner: out[b][t][s][:] = act(enc[b][t][:] + pred[b][r[b][t] + s][:]); the clamp of r keeps r + s below U1 ----
// W = 4: J % 4 == 0 and the three tensors 16-byte aligned; n = elements / W
template <int W>
__global__ __launch_bounds__(256) void rnnt_pruned_joint_kernel(const float *__restrict__ enc, const float *__restrict__ pred,
                                                                const int *__restrict__ ranges, int T, int U1, int S, int JW, int kind,
                                                                float *__restrict__ out, long n) {
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += gridDim.x * 256L) {
        const long cell = i / JW;
        const int j = (int)(i - cell * JW);
        const long bt = cell / S;
        const int u = rnnt_range(ranges, bt, U1, S) + (int)(cell - bt * S);
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

// d_pred[b][u][j] = sum over the frames t whose window holds u, t ascending, of dout[b][t][u - r[t]][j] act'(out[the same]); a thread
// per element, j fastest; one accumulator
__global__ __launch_bounds__(256) void rnnt_pruned_joint_dpred_kernel(const float *__restrict__ out, const float *__restrict__ dout,
                                                                      const int *__restrict__ ranges, int T, int U1, int S, int J, int kind,
                                                                      float *__restrict__ dpred, long n) {
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += gridDim.x * 256L) {
        const long bu = i / J;
        const int j = (int)(i - bu * J);
        const long b = bu / U1;
        const int u = (int)(bu - b * U1);
        float acc = 0.0f;
        for (int t = 0; t < T; ++t) {
            const int s = u - rnnt_range(ranges, b * T + t, U1, S);
            if (s < 0 || s >= S) continue;
            const long at = ((b * T + t) * S + s) * J + j;
            acc += dout[at] * rnnt_dact(kind, kind ? out[at] : 0.0f);
        }
        dpred[i] = acc;
    }
}

// ---- 3. the banded loss ----
// every live cell of the full lattice: the emissions of its band row, or the arithmetic's zero outside the band
template <bool VEC>
__global__ __launch_bounds__(CTC_THREADS) void rnnt_band_emit_kernel(const float *__restrict__ logits, const int *__restrict__ ranges, int B, int T,
                                                                     int U1, int S, int V, int blank, const int *__restrict__ ints,
                                                                     float4 *__restrict__ em, double *__restrict__ lse_out, long cells) {
    const int lane = threadIdx.x & 63;
    for (long c = blockIdx.x * 4L + (threadIdx.x >> 6); c < cells; c += gridDim.x * 4L) {
        const RnntCell q = rnnt_cell(c, T, U1);
        const int Ub = ints[B + q.b];
        if (q.t >= ints[q.b] || q.u > Ub) continue;
        const long bt = (long)q.b * T + q.t;
        const int s = q.u - rnnt_range(ranges, bt, U1, S);
        if (s < 0 || s >= S) {
            const xf z = xf_zero();
            if (lane == 0) em[c] = make_float4(z.m, __int_as_float(z.e), z.m, __int_as_float(z.e));
            continue;
        }
        const RnntRow<false> row = {logits + (bt * S + s) * V, nullptr};
        rnnt_emit_row<VEC, false>(row, V, blank, q.u < Ub ? ints + 2L * B + (long)q.b * (U1 - 1) + q.u : nullptr, lane, em + c,
                                  lse_out ? lse_out + c : nullptr);
    }
}

// a wavefront per band cell; cells = B T S
template <bool VEC>
__global__ __launch_bounds__(CTC_THREADS) void rnnt_band_grad_kernel(const float *__restrict__ logits, const int *__restrict__ ranges, int B, int T,
                                                                     int U1, int S, int V, int blank, const int *__restrict__ ints,
                                                                     const float4 *__restrict__ em, const double *__restrict__ lse_in,
                                                                     const float2 *__restrict__ wa, const float2 *__restrict__ wb,
                                                                     const float *__restrict__ hdr, float *__restrict__ dlogits, long cells) {
    const int lane = threadIdx.x & 63;
    for (long bc = blockIdx.x * 4L + (threadIdx.x >> 6); bc < cells; bc += gridDim.x * 4L) {
        const long bt = bc / S;
        const int b = (int)(bt / T), t = (int)(bt - (long)b * T);
        const int u = rnnt_range(ranges, bt, U1, S) + (int)(bc - bt * S);
        const int Tb = ints[b], Ub = ints[B + b];
        float *g = dlogits + bc * V;
        const float mP = hdr[2 * b];
        if (t >= Tb || u > Ub || !(mP > 0.0f)) {                            // padding, or a row whose band carries no mass: zeros
            rnnt_zero_row(g, V, lane);
            continue;
        }
        const long c = bt * U1 + u;
        const RnntFlows f = rnnt_cell_flows(c, t, u, Tb, Ub, U1, em, wa, wb, mP, __float_as_int(hdr[2 * b + 1]));
        const int y = u < Ub ? ints[2L * B + (long)b * (U1 - 1) + u] : -1;
        const RnntRow<false> row = {logits + bc * V, nullptr};
        rnnt_grad_row<VEC, false>(row, g, V, blank, y, f, lse_in[c], lane);
    }
}

// the simple loss's workspace: rnnt_layout, then with a gradient or the occupancies asked 4 words per cell (coef)
static inline size_t rnnt_simple_coef(const RnntLayout &l) { return (l.total + 3) & ~(size_t)3; }

extern "C" {

size_t nntk_shim_rnnt_simple_workspace_floats(int batch, int T, int max_label_len, int want_grad) {
    const RnntLayout l = rnnt_layout(batch, T, max_label_len, want_grad);
    if (!want_grad) return l.total;
    const size_t b = batch > 0 ? (size_t)batch : 0, t = T > 0 ? (size_t)T : 0, ml = max_label_len > 0 ? (size_t)max_label_len : 0;
    return rnnt_simple_coef(l) + 4 * b * t * (ml + 1) + 4;
}

int nntk_shim_rnnt_simple_loss(const float *d_am, const float *d_lm, int B, int T, int V, const int *h_input_lengths, const int *h_labels,
                               const int *h_label_lengths, int maxL, int blank, float *d_loss_rows, float *d_dam, float *d_dlm, float *d_occ,
                               float *d_ws) {
    if (B <= 0) return 0;
    if (!rnnt_lattice_fits(T, maxL)) return nntk_fail_msg("nntk_rnnt_simple_loss_device: max_label_len or T + max_label_len is beyond the lattice kernel's limits");
    if ((((uintptr_t)d_ws | (uintptr_t)d_am | (uintptr_t)d_lm) & 15) != 0)
        return nntk_fail_msg("nntk_rnnt_simple_loss_device: d_am, d_lm and the workspace must be 16-byte aligned");
    const bool grad = d_dam != nullptr, back = grad || d_occ != nullptr;
    const int U1 = maxL + 1;
    const long cells = (long)B * T * U1;
    const RnntLayout l = rnnt_layout(B, T, maxL, back);
    const RnntParts w = rnnt_parts(d_ws, l, back);
    float4 *coef = grad ? (float4 *)(d_ws + rnnt_simple_coef(l)) : nullptr;
    if (rnnt_upload_ints(w.ints, B, maxL, h_input_lengths, h_labels, h_label_lengths)) return -1;
    const dim3 cgrid(rnnt_grid(cells, 4));
    if ((V & 3) == 0)
        hipLaunchKernelGGL(rnnt_simple_emit_kernel<true>, cgrid, dim3(CTC_THREADS), 0, nntk_stream(), d_am, d_lm, B, T, U1, V, blank, w.ints, w.em,
                           w.lse, cells);
    else
        hipLaunchKernelGGL(rnnt_simple_emit_kernel<false>, cgrid, dim3(CTC_THREADS), 0, nntk_stream(), d_am, d_lm, B, T, U1, V, blank, w.ints, w.em,
                           w.lse, cells);
    NNTK_LAUNCH_CHECK("rnnt_simple_emit_kernel");
    if (nntk_rnnt_lattice_launch(B, T, U1, w.ints, w.em, w.alpha, w.beta, w.hdr, d_loss_rows)) return -1;
    if (!back) return 0;
    hipLaunchKernelGGL(rnnt_simple_cell_kernel, dim3(rnnt_grid(cells, 256)), dim3(256), 0, nntk_stream(), B, T, U1, w.ints, w.em, w.alpha, w.beta,
                       w.hdr, coef, d_occ, cells);
    NNTK_LAUNCH_CHECK("rnnt_simple_cell_kernel");
    if (!grad) return 0;
    const long na = (long)B * T * V, nl = (long)B * U1 * V;
    hipLaunchKernelGGL(rnnt_simple_reduce_kernel<true>, dim3(rnnt_grid(na, 256)), dim3(256), 0, nntk_stream(), d_am, d_lm, B, T, U1, V, blank,
                       w.ints, coef, w.lse, w.hdr, d_dam, na);
    hipLaunchKernelGGL(rnnt_simple_reduce_kernel<false>, dim3(rnnt_grid(nl, 256)), dim3(256), 0, nntk_stream(), d_am, d_lm, B, T, U1, V, blank,
                       w.ints, coef, w.lse, w.hdr, d_dlm, nl);
    NNTK_LAUNCH_CHECK("rnnt_simple_reduce_kernel");
    return 0;
}

size_t nntk_shim_rnnt_prune_workspace_floats(int batch) { return ((2 * (size_t)(batch > 0 ? batch : 0) + 3) & ~(size_t)3) + 4; }

int nntk_shim_rnnt_prune_ranges(const float *d_occ, int B, int T, int U1, const int *h_input_lengths, const int *h_label_lengths, int S,
                                int *d_ranges, float *d_ws) {
    if (B <= 0 || T <= 0) return 0;
    if (S < 1 || S > U1) return nntk_fail_msg("nntk_rnnt_prune_ranges_device: S is outside [1, max_label_len + 1]");
    int *ints = (int *)d_ws;
    if (nntk_shim_upload_ints(ints, h_input_lengths, B) || nntk_shim_upload_ints(ints + B, h_label_lengths, B)) return -1;
    hipLaunchKernelGGL(rnnt_prune_kernel, dim3((unsigned)B), dim3(256), 0, nntk_stream(), d_occ, B, T, U1, S, ints, d_ranges);
    NNTK_LAUNCH_CHECK("rnnt_prune_kernel");
    return 0;
}

int nntk_shim_rnnt_pruned_joint(const float *d_enc, const float *d_pred, const int *d_ranges, int B, int T, int U1, int S, int J, int kind,
                                float *d_out) {
    const long n = (long)B * T * S * J;
    if (n <= 0) return 0;
    if (S < 1 || S > U1) return nntk_fail_msg("nntk_rnnt_pruned_joint_device: S is outside [1, U1]");
    if ((J & 3) == 0 && (((uintptr_t)d_enc | (uintptr_t)d_pred | (uintptr_t)d_out) & 15) == 0)
        hipLaunchKernelGGL(rnnt_pruned_joint_kernel<4>, dim3(rnnt_grid(n / 4, 256)), dim3(256), 0, nntk_stream(), d_enc, d_pred, d_ranges, T, U1, S,
                           J / 4, kind, d_out, n / 4);
    else
        hipLaunchKernelGGL(rnnt_pruned_joint_kernel<1>, dim3(rnnt_grid(n, 256)), dim3(256), 0, nntk_stream(), d_enc, d_pred, d_ranges, T, U1, S, J,
                           kind, d_out, n);
    NNTK_LAUNCH_CHECK("rnnt_pruned_joint_kernel");
    return 0;
}

int nntk_shim_rnnt_pruned_joint_backward(const float *d_out_fwd, const float *d_dout, const int *d_ranges, int B, int T, int U1, int S, int J,
                                         int kind, float *d_denc, float *d_dpred) {
    if ((long)B * T * S * J <= 0) return 0;
    if (S < 1 || S > U1) return nntk_fail_msg("nntk_rnnt_pruned_joint_backward_device: S is outside [1, U1]");
    // d_enc: the full joiner's sum over its second lattice axis, S wide here
    if (nntk_rnnt_joint_reduce_launch(d_out_fwd, d_dout, (long)B * T * J, (long)J, (long)S * J, S, (long)J, kind, d_denc)) return -1;
    const long np = (long)B * U1 * J;
    hipLaunchKernelGGL(rnnt_pruned_joint_dpred_kernel, dim3(rnnt_grid(np, 256)), dim3(256), 0, nntk_stream(), d_out_fwd, d_dout, d_ranges, T, U1, S,
                       J, kind, d_dpred, np);
    NNTK_LAUNCH_CHECK("rnnt_pruned_joint_dpred_kernel");
    return 0;
}

int nntk_shim_rnnt_pruned_loss(const float *d_logits, const int *d_ranges, int B, int T, int S, int V, const int *h_input_lengths,
                               const int *h_labels, const int *h_label_lengths, int maxL, int blank, float *d_loss_rows, float *d_dlogits,
                               float *d_ws) {
    if (B <= 0) return 0;
    if (!rnnt_lattice_fits(T, maxL)) return nntk_fail_msg("nntk_rnnt_pruned_loss_device: max_label_len or T + max_label_len is beyond the lattice kernel's limits");
    if (S < 1 || S > maxL + 1) return nntk_fail_msg("nntk_rnnt_pruned_loss_device: S is outside [1, max_label_len + 1]");
    if ((((uintptr_t)d_ws | (uintptr_t)d_logits | (uintptr_t)d_dlogits) & 15) != 0)
        return nntk_fail_msg("nntk_rnnt_pruned_loss_device: the tensors and the workspace must be 16-byte aligned");
    const int U1 = maxL + 1;
    const long cells = (long)B * T * U1, band = (long)B * T * S;
    const RnntParts w = rnnt_parts(d_ws, rnnt_layout(B, T, maxL, d_dlogits != nullptr), d_dlogits != nullptr);
    if (rnnt_upload_ints(w.ints, B, maxL, h_input_lengths, h_labels, h_label_lengths)) return -1;
    const bool vec = (V & 3) == 0;
    if (vec)
        hipLaunchKernelGGL(rnnt_band_emit_kernel<true>, dim3(rnnt_grid(cells, 4)), dim3(CTC_THREADS), 0, nntk_stream(), d_logits, d_ranges, B, T,
                           U1, S, V, blank, w.ints, w.em, w.lse, cells);
    else
        hipLaunchKernelGGL(rnnt_band_emit_kernel<false>, dim3(rnnt_grid(cells, 4)), dim3(CTC_THREADS), 0, nntk_stream(), d_logits, d_ranges, B, T,
                           U1, S, V, blank, w.ints, w.em, w.lse, cells);
    NNTK_LAUNCH_CHECK("rnnt_band_emit_kernel");
    if (nntk_rnnt_lattice_launch(B, T, U1, w.ints, w.em, w.alpha, w.beta, w.hdr, d_loss_rows)) return -1;
    if (!d_dlogits) return 0;
    if (vec)
        hipLaunchKernelGGL(rnnt_band_grad_kernel<true>, dim3(rnnt_grid(band, 4)), dim3(CTC_THREADS), 0, nntk_stream(), d_logits, d_ranges, B, T, U1,
                           S, V, blank, w.ints, w.em, w.lse, w.alpha, w.beta, w.hdr, d_dlogits, band);
    else
        hipLaunchKernelGGL(rnnt_band_grad_kernel<false>, dim3(rnnt_grid(band, 4)), dim3(CTC_THREADS), 0, nntk_stream(), d_logits, d_ranges, B, T, U1,
                           S, V, blank, w.ints, w.em, w.lse, w.alpha, w.beta, w.hdr, d_dlogits, band);
    NNTK_LAUNCH_CHECK("rnnt_band_grad_kernel");
    return 0;
}

}  // extern "C"
