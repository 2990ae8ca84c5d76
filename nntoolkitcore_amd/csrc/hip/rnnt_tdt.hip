// rnnt_tdt.hip -- the token-and-duration transducer (Xu et al., 2023): the per-row negative log-likelihood over the lattice of
// unnormalised scores [B][T][U1 = max_label_len + 1][V + D] and its gradient.  Columns 0 .. V-1 are the token head (one class the blank),
// columns V .. V+D-1 the duration head; each head has its own softmax, both fused in here.  A move out of (t, u) emits a token AND a
// duration d_i: a blank with d_i > 0 goes to (t + d_i, u), label y_{u+1} with any d_i goes to (t + d_i, u + 1); a path ends with a blank
// that lands exactly on T_b.  include/nntoolkitcore_hip.h has the recursion.
//
// Range: as rnnt.hip -- alpha, beta, the two token emissions and the D duration probabilities of a cell are each an f32 mantissa with an
// int32 exponent (ctc_xf.hpp), the exponent of every emission floored at RNNT_EMIN.  A move multiplies TWO emissions, so the exponents of
// a path sum inside 2^28 for T + max_label_len <= NNTK_RNNT_TDT_MAX_DIAGONALS, half of rnnt.hip's bound.
//
// Work split, three launches; the score tensor is read twice and the gradient written once.
//  tdt_emit_kernel: a wavefront per live cell.  Token head: maximum, then the sum of exp(x - max) in double over V (the order of
//    rnnt_emit_row); duration head: lanes 0 .. D-1 hold one score each, the same two butterflies.  Kept per cell: the blank's and the
//    next label's emission exp(x - lse_tok - sigma) (16 bytes), the D duration probabilities (8 bytes each) and, for the gradient, both
//    lse as doubles.  sigma, the paper's logit under-normalisation, is in the two token emissions and nowhere else.
//  tdt_lattice_kernel: one 256-lane workgroup per (row, direction) -- blockIdx.y = 0 runs alpha over the anti-diagonals t + u = n
//    upwards, 1 runs beta downwards, concurrently -- lanes over u.  A cell of diagonal n draws from the diagonals n - d_i (same u, a
//    blank) and n - d_i - 1 (u - 1, a label) for every duration, so the last Dmax + 1 diagonals stay in a RING of Dmax + 2 slots in LDS,
//    diagonal m in slot m mod (Dmax + 2): the slot being written is never one that this step reads, and one LDS-only barrier per
//    diagonal orders the steps.  The trip count (T_b + U_b, one more forwards for the terminal sum) is uniform over the workgroup and
//    every barrier stands outside lane-dependent control flow.
//    What a ring entry holds (16 bytes per u).  Forwards: alpha p_blank | alpha p_label of the SOURCE cell, as rnnt.hip has it: the two
//    token products are formed once per cell, not once per term, and a term is one product with the source's duration probability,
//    which does not depend on alpha and comes from global memory -- for U1 <= 256 it is loaded a diagonal ahead, in flight across the
//    barrier.  An entry of alpha alone would halve the ring but put two fetched factors and two products on every term.
//    Backwards: beta itself; the cell's own p_blank p_dur(i), p_label p_dur(i) are formed off the dependent chain.
//    Pull, never push: a cell sums its up to 2 D terms in ONE fixed order -- ascending i, for each i the blank term before the label
//    term -- aligned to the largest exponent, added left to right in f32, normalised once.  The bits depend on that order.
//    Whether a term exists is decided from the indices alone (t - d_i >= 0, d_i > 0 for a blank, u >= 1 for a label; backwards
//    t + d_i against T_b) and a term that does not exist never reads the ring: a slot of a diagonal that does not exist, or that is
//    narrower than the ring (n < Dmax + 1, T_b < Dmax), counts as zero mass whatever the slot holds.
//    P = sum over d_i in (0, T_b] of alpha(T_b - d_i, U_b) p_blank p_dur(i) is the blank-only cell (T_b, U_b) of diagonal T_b + U_b,
//    from the forward direction alone: the loss bits do not depend on whether a gradient is asked.
//  tdt_grad_kernel: a wavefront per cell: the occupancy alpha beta / P, the flows through the blank, the label and each duration
//    (ascending i, all divided by P, the terminal move included), then V + D scores in and
//    g[v] = occ exp(x_v - lse_tok) - [v = blank] F_blank - [v = label] F_label, g[V + i] = occ exp(x_{V+i} - lse_dur) - F_dur(i) out,
//    16 bytes at a time where (V + D) % 4 == 0.  Padding cells and the rows with P = 0 are zero-filled.
// No atomics anywhere; every reduction is a fixed butterfly or a fixed-order loop.
#include "rnnt_tdt_common.hpp"

// the up to 2 D terms of a cell, in their one order: aligned to the largest exponent, added left to right, normalised once
__device__ __forceinline__ xf tdt_sum(const xf (&tm)[2 * TDT_MAXD]) {
    int em = tm[0].e;
#pragma unroll
    for (int k = 1; k < 2 * TDT_MAXD; ++k) em = max(em, tm[k].e);
    float m = 0.0f;
#pragma unroll
    for (int k = 0; k < 2 * TDT_MAXD; ++k) m += ldexpf(tm[k].m, tm[k].e - em);
    return xf_norm(m, em);
}

// lse of n scores by one wavefront, on every lane: maximum, then the sum of exp(x - max) in double.  VEC: 16-byte loads of a row that
// starts on the 16-byte grid and whose quads may run past n into columns that are still the row's
template <bool VEC>
__device__ __forceinline__ double tdt_row_lse(const float *x, int n, int lane) {
    float mx = -INFINITY;
    if (VEC) {
        for (int i = lane; 4 * i < n; i += 64) {
            const f32x4 q = ((const f32x4 *)x)[i];
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (4 * i + k < n) mx = fmaxf(mx, q[k]);
        }
    } else {
        for (int k = lane; k < n; k += 64) mx = fmaxf(mx, x[k]);
    }
    mx = rnnt_wave_max(mx);
    double s = 0.0;
    if (VEC) {
        for (int i = lane; 4 * i < n; i += 64) {
            const f32x4 q = ((const f32x4 *)x)[i];
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (4 * i + k < n) s += (double)expf(q[k] - mx);
        }
    } else {
        for (int k = lane; k < n; k += 64) s += (double)expf(x[k] - mx);
    }
    s = rnnt_wave_sum(s);
    return (double)mx + log(s);
}

// VEC: (V + D) % 4 == 0 and the tensor 16-byte aligned, so every cell's row is
template <bool VEC>
__global__ __launch_bounds__(CTC_THREADS) void tdt_emit_kernel(const float *__restrict__ logits, int B, int T, int U1, int V, int D, int blank,
                                                               float sigma, const int *__restrict__ ints, float4 *__restrict__ em,
                                                               float2 *__restrict__ pdur, double *__restrict__ lse_out, long cells) {
    const int lane = threadIdx.x & 63;
    for (long c = blockIdx.x * 4L + (threadIdx.x >> 6); c < cells; c += gridDim.x * 4L) {
        const RnntCell q = rnnt_cell(c, T, U1);
        const int Ub = ints[B + q.b];
        if (q.t >= ints[q.b] || q.u > Ub) continue;
        const float *x = logits + c * (V + D);
        const double lse_t = tdt_row_lse<VEC>(x, V, lane);
        const float xd = lane < D ? x[V + lane] : -INFINITY;                 // the duration head: one score a lane
        const float md = rnnt_wave_max(xd);
        const double lse_d = (double)md + log(rnnt_wave_sum(lane < D ? (double)expf(xd - md) : 0.0));
        if (lane < D) pdur[c * D + lane] = xf_pack(rnnt_emission(xd, lse_d));
        if (lane == 0) {
            const double ls = lse_t + (double)sigma;                         // sigma = 0: lse_t itself
            const xf pb = rnnt_emission(x[blank], ls);
            const xf py = q.u < Ub ? rnnt_emission(x[ints[2L * B + (long)q.b * (U1 - 1) + q.u]], ls) : xf_zero();
            em[c] = make_float4(pb.m, __int_as_float(pb.e), py.m, __int_as_float(py.e));
            if (lse_out) {
                lse_out[2 * c] = lse_t;
                lse_out[2 * c + 1] = lse_d;
            }
        }
    }
}

// REG: U1 <= 256, a lane owns the cell u = tid of a diagonal and takes its record from registers, loaded one diagonal ahead; else any U1
// whose ring fits the LDS, lanes stride over u and the record is fetched inside the step
template <bool REG>
__global__ __launch_bounds__(CTC_THREADS) void tdt_lattice_kernel(int B, int T, int U1, const TdtDur dur, const int *__restrict__ ints,
                                                                  const float4 *__restrict__ em, const float2 *__restrict__ pdur,
                                                                  float2 *ws_alpha, float2 *ws_beta, float *hdr, float *loss_rows) {
    extern __shared__ __align__(16) unsigned char tdt_smem[];
    float4 *ring = (float4 *)tdt_smem;                                      // [dmax + 2][U1]
    const int b = blockIdx.x, dir = blockIdx.y, tid = threadIdx.x;
    const int Tb = ints[b], Ub = ints[B + b], D = dur.n, R = dur.dmax + 2;
    const long base = (long)b * T * U1;
    const float4 *e = em + base;
    const float2 *pd = pdur + base * D;
    float2 *ws = dir ? ws_beta : ws_alpha;
    if (ws) ws += base;
    const int ND = Tb + Ub;                                                 // diagonals n = t + u = 0 .. ND - 1; forwards ND too: the cell (Tb, Ub)
    const int steps = dir ? ND : ND + 1;
    auto live = [&](int n, int u) {
        const int t = n - u;
        return u <= Ub && t >= 0 && (t < Tb || (dir == 0 && t == Tb && u == Ub));
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
            if (i >= D) continue;
            if (dir) {
                r.a[i] = pd[((long)t * U1 + u) * D + i];
            } else if (t - dur.d[i] >= 0) {
                const long s = (long)(t - dur.d[i]) * U1 + u;
                if (dur.d[i] > 0) r.a[i] = pd[s * D + i];
                if (u >= 1 && t < Tb) r.b[i] = pd[(s - 1) * D + i];
            }
        }
    };
    // the slot of diagonal n is sl; of n - k (forwards) or n + k (backwards), 0 <= k < R, k slots behind or ahead on the ring
    auto cell = [&](int n, int sl, int u, const TdtRec &r) {
        const int t = n - u;
        xf pb, py, tm[2 * TDT_MAXD];
        pb.m = r.e.x; pb.e = __float_as_int(r.e.y);
        py.m = r.e.z; py.e = __float_as_int(r.e.w);
#pragma unroll
        for (int k = 0; k < 2 * TDT_MAXD; ++k) tm[k] = xf_zero();
        if (dir == 0) {
            xf a;
            if (n == 0) {
                a = xf_one();
            } else {
#pragma unroll
                for (int i = 0; i < TDT_MAXD; ++i) {
                    if (i >= D || t - dur.d[i] < 0) continue;
                    const int k = dur.d[i];                                 // from (t - k, u) by a blank, then from (t - k, u - 1) by label u
                    if (k > 0) {
                        const float4 s = ring[(sl - k < 0 ? sl - k + R : sl - k) * U1 + u];
                        tm[2 * i] = xf_times(tdt_xf(make_float2(s.x, s.y)), tdt_xf(r.a[i]));
                    }
                    if (u >= 1 && t < Tb) {
                        const float4 s = ring[(sl - k - 1 < 0 ? sl - k - 1 + R : sl - k - 1) * U1 + u - 1];
                        tm[2 * i + 1] = xf_times(tdt_xf(make_float2(s.z, s.w)), tdt_xf(r.b[i]));
                    }
                }
                a = tdt_sum(tm);
            }
            if (t == Tb) {                                                  // the one cell of the last diagonal: P, blanks only
                hdr[2 * b] = a.m;
                hdr[2 * b + 1] = __int_as_float(a.e);
                // once per row: double, libm log
                loss_rows[b] = a.m == 0.0f ? INFINITY : (float)-((double)a.e * 0.69314718055994530942 + log((double)a.m));
                return;
            }
            if (ws) ws[(long)t * U1 + u] = xf_pack(a);
            const xf ab = xf_times(a, pb), ay = xf_times(a, py);
            ring[sl * U1 + u] = make_float4(ab.m, __int_as_float(ab.e), ay.m, __int_as_float(ay.e));
        } else {                                                            // beta(Tb, Ub) stands for 1; beta(Tb, u < Ub) and beta(t > Tb, .) are 0
#pragma unroll
            for (int i = 0; i < TDT_MAXD; ++i) {
                if (i >= D) continue;
                const int k = dur.d[i], tt = t + k;
                const xf pdi = tdt_xf(r.a[i]);
                if (k > 0 && tt <= Tb) {
                    xf bt = u == Ub ? xf_one() : xf_zero();
                    if (tt < Tb) {
                        const float4 s = ring[(sl + k >= R ? sl + k - R : sl + k) * U1 + u];
                        bt = tdt_xf(make_float2(s.x, s.y));
                    }
                    tm[2 * i] = xf_times(bt, xf_times(pb, pdi));
                }
                if (u < Ub && tt < Tb) {
                    const float4 s = ring[(sl + k + 1 >= R ? sl + k + 1 - R : sl + k + 1) * U1 + u + 1];
                    tm[2 * i + 1] = xf_times(tdt_xf(make_float2(s.x, s.y)), xf_times(py, pdi));
                }
            }
            const xf v = tdt_sum(tm);
            ws[(long)t * U1 + u] = xf_pack(v);
            ring[sl * U1 + u] = make_float4(v.m, __int_as_float(v.e), 0.0f, 0.0f);
        }
    };
    TdtRec nx;
    if (REG) fetch(dir ? ND - 1 : 0, tid, nx);
    int sl = dir ? (ND - 1) % R : 0;
    for (int i = 0; i < steps; ++i) {
        const int n = dir ? ND - 1 - i : i;
        if (REG) {
            const TdtRec cu = nx;
            if (i + 1 < steps) fetch(dir ? n - 1 : n + 1, tid, nx);         // the next diagonal's records: not on the dependent chain
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
        sl = dir ? (sl == 0 ? R - 1 : sl - 1) : (sl + 1 == R ? 0 : sl + 1);
    }
}

template <bool VEC>
__global__ __launch_bounds__(CTC_THREADS) void tdt_grad_kernel(const float *__restrict__ logits, int B, int T, int U1, int V, const TdtDur dur,
                                                               int blank, const int *__restrict__ ints, const float4 *__restrict__ em,
                                                               const float2 *__restrict__ pdur, const double *__restrict__ lse_in,
                                                               const float2 *__restrict__ wa, const float2 *__restrict__ wb,
                                                               const float *__restrict__ hdr, float *__restrict__ dlogits, long cells) {
    const int lane = threadIdx.x & 63, W = V + dur.n;
    for (long c = blockIdx.x * 4L + (threadIdx.x >> 6); c < cells; c += gridDim.x * 4L) {
        const RnntCell q = rnnt_cell(c, T, U1);
        const int Tb = ints[q.b], Ub = ints[B + q.b];
        float *g = dlogits + c * W;
        const float mP = hdr[2 * q.b];
        if (q.t >= Tb || q.u > Ub || !(mP > 0.0f)) {                        // padding, or a row no path reaches (P = 0): zeros
            rnnt_zero_row(g, W, lane);
            continue;
        }
        const TdtFlows f = tdt_cell_flows(c, q.t, q.u, Tb, Ub, U1, dur, em, pdur, wa, wb, mP, __float_as_int(hdr[2 * q.b + 1]));
        const int y = q.u < Ub ? ints[2L * B + (long)q.b * (U1 - 1) + q.u] : -1;
        const double lse_t = lse_in[2 * c], lse_d = lse_in[2 * c + 1];
        const float *x = logits + c * W;
        if (VEC) {
            for (int i = lane; i < (W >> 2); i += 64) {
                const f32x4 x4 = ((const f32x4 *)x)[i];
                f32x4 r;
#pragma unroll
                for (int k = 0; k < 4; ++k) r[k] = tdt_grad_value(f, lse_t, lse_d, V, blank, y, x4[k], 4 * i + k);
                ((f32x4 *)g)[i] = r;
            }
        } else {
            for (int k = lane; k < W; k += 64) g[k] = tdt_grad_value(f, lse_t, lse_d, V, blank, y, x[k], k);
        }
    }
}

int nntk_rnnt_tdt_emit_launch(const float *d_logits, int B, int T, int U1, int V, int D, int blank, float sigma, const int *d_ints,
                              float4 *em, float2 *pdur, double *lse) {
    const long cells = (long)B * T * U1;
    const dim3 cgrid(rnnt_grid(cells, 4));
    if (((V + D) & 3) == 0)
        hipLaunchKernelGGL(tdt_emit_kernel<true>, cgrid, dim3(CTC_THREADS), 0, nntk_stream(), d_logits, B, T, U1, V, D, blank, sigma, d_ints, em,
                           pdur, lse, cells);
    else
        hipLaunchKernelGGL(tdt_emit_kernel<false>, cgrid, dim3(CTC_THREADS), 0, nntk_stream(), d_logits, B, T, U1, V, D, blank, sigma, d_ints, em,
                           pdur, lse, cells);
    NNTK_LAUNCH_CHECK("tdt_emit_kernel");
    return 0;
}

// the lattice on the emissions, for this unit and for rnnt_tdt_fused.hip; wa / wb NULL: the forward direction alone
int nntk_rnnt_tdt_lattice_launch(int B, int T, int U1, const TdtDur &dur, const int *d_ints, const float4 *em, const float2 *pdur, float2 *wa,
                                 float2 *wb, float *hdr, float *d_loss_rows) {
    const size_t lds = tdt_ring_bytes(U1, dur.dmax);
    const dim3 lgrid((unsigned)B, wa ? 2 : 1);
#define TDT_AB(REG)                                                                                                               \
    do {                                                                                                                          \
        if (lds > 48 * 1024 && nntk_set_max_dynamic_lds((const void *)tdt_lattice_kernel<REG>, lds)) return -1;                    \
        hipLaunchKernelGGL(tdt_lattice_kernel<REG>, lgrid, dim3(CTC_THREADS), lds, nntk_stream(), B, T, U1, dur, d_ints, em, pdur, \
                           wa, wb, hdr, d_loss_rows);                                                                             \
    } while (0)
    if (U1 <= CTC_THREADS) TDT_AB(true);
    else TDT_AB(false);
#undef TDT_AB
    NNTK_LAUNCH_CHECK("tdt_lattice_kernel");
    return 0;
}

extern "C" {

size_t nntk_shim_rnnt_tdt_workspace_floats(int batch, int T, int max_label_len, int n_durations, int want_grad) {
    return tdt_layout(batch, T, max_label_len, n_durations, want_grad).total;
}

int nntk_shim_rnnt_tdt_loss(const float *d_logits, int B, int T, int V, const int *h_durations, int D, const int *h_input_lengths,
                            const int *h_labels, const int *h_label_lengths, int maxL, int blank, float sigma, float *d_loss_rows,
                            float *d_dlogits, float *d_ws) {
    if (B <= 0) return 0;
    if (!tdt_fits(T, maxL, h_durations, D))
        return nntk_fail_msg("nntk_rnnt_tdt_loss_device: the durations, max_label_len or T + max_label_len are beyond the lattice kernel's limits");
    if ((((uintptr_t)d_ws | (uintptr_t)d_logits | (uintptr_t)d_dlogits) & 15) != 0)
        return nntk_fail_msg("nntk_rnnt_tdt_loss_device: the tensors and the workspace must be 16-byte aligned");
    static_assert(NNTK_RNNT_TDT_LDS_BYTES <= CTC_LDS_LIMIT, "the ring's budget is one workgroup's LDS");
    const int U1 = maxL + 1;
    const long cells = (long)B * T * U1;
    const bool grad = d_dlogits != nullptr, vec = ((V + D) & 3) == 0;
    const TdtLayout l = tdt_layout(B, T, maxL, D, grad);
    int *ints = (int *)d_ws;
    float *hdr = d_ws + l.hdr;
    float4 *em = (float4 *)(d_ws + l.em);
    float2 *pdur = (float2 *)(d_ws + l.dur);
    double *lse = grad ? (double *)(d_ws + l.lse) : nullptr;
    float2 *wa = grad ? (float2 *)(d_ws + l.alpha) : nullptr, *wb = grad ? (float2 *)(d_ws + l.beta) : nullptr;
    const TdtDur dur = tdt_dur(h_durations, D);
    if (rnnt_upload_ints(ints, B, maxL, h_input_lengths, h_labels, h_label_lengths)) return -1;
    const dim3 cgrid(rnnt_grid(cells, 4));
    if (nntk_rnnt_tdt_emit_launch(d_logits, B, T, U1, V, D, blank, sigma, ints, em, pdur, lse)) return -1;
    if (nntk_rnnt_tdt_lattice_launch(B, T, U1, dur, ints, em, pdur, wa, wb, hdr, d_loss_rows)) return -1;
    if (grad) {
        if (vec)
            hipLaunchKernelGGL(tdt_grad_kernel<true>, cgrid, dim3(CTC_THREADS), 0, nntk_stream(), d_logits, B, T, U1, V, dur, blank, ints, em,
                               pdur, lse, wa, wb, hdr, d_dlogits, cells);
        else
            hipLaunchKernelGGL(tdt_grad_kernel<false>, cgrid, dim3(CTC_THREADS), 0, nntk_stream(), d_logits, B, T, U1, V, dur, blank, ints, em,
                               pdur, lse, wa, wb, hdr, d_dlogits, cells);
        NNTK_LAUNCH_CHECK("tdt_grad_kernel");
    }
    return 0;
}

}  // extern "C"
