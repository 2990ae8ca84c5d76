/*
 * attention.c -- host layer of the self-attention core (csrc/hip/attention.hip).  Every argument and the host array of key counts are
 * checked here, before anything is enqueued or allocated: a refusal needs no device and writes nothing.
 */
#include <math.h>
#include <stdio.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include "nntk_internal.h"

/* scratch for the host-pointer form: per thread and device, freed at thread exit (nntk_thread_scratch, runtime.c) */
#define t_a (*nntk_thread_scratch(NNTK_TS_A))
#define t_b (*nntk_thread_scratch(NNTK_TS_B))

#define ATT_MAX_STRIDE (1L << 40)

static int att_fail(const char *who, const char *fmt, long a, long b, long c) {
    char msg[240];
    int n = snprintf(msg, sizeof msg, "%s: ", who);
    snprintf(msg + n, sizeof msg - (size_t)n, fmt, a, b, c);
    nntk_set_error(msg);
    return -1;
}

/* floats from the first to one past the last element of a strided [batch][T][hd] tensor */
static size_t att_span(int batch, int T, long fs, long bs, int hd) {
    return (size_t)(batch - 1) * (size_t)bs + (size_t)(T - 1) * (size_t)fs + (size_t)hd;
}

static int att_overlap(const void *a, size_t na, const void *b, size_t nb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return a && b && x < y + nb * 4 && y < x + na * 4;
}

/* everything but the pointers */
static int att_check(const char *who, int batch, int heads, int d_head, int Tq, int Tk, long qfs, long qbs, long kfs, long kbs, long vfs,
                     long vbs, const int *kv_lengths, int q_offset, int pos0, int chunk, int left, int right, float scale) {
    if (batch < 0) return att_fail(who, "batch %ld < 0", batch, 0, 0);
    if (d_head < 1 || d_head > NNTK_ATTENTION_MAX_D_HEAD) return att_fail(who, "d_head %ld is outside [1, %ld]", d_head, NNTK_ATTENTION_MAX_D_HEAD, 0);
    if (heads < 1 || heads > NNTK_ATTENTION_MAX_HEADS) return att_fail(who, "heads %ld is outside [1, %ld]", heads, NNTK_ATTENTION_MAX_HEADS, 0);
    if (Tq < 1 || Tq > NNTK_ATTENTION_MAX_FRAMES || Tk < 1 || Tk > NNTK_ATTENTION_MAX_FRAMES)
        return att_fail(who, "Tq %ld, Tk %ld: both must lie in [1, %ld]", Tq, Tk, NNTK_ATTENTION_MAX_FRAMES);
    if (q_offset < 0 || (long)q_offset + Tq > Tk) return att_fail(who, "q_offset %ld: q_offset >= 0 and q_offset + Tq (%ld) <= Tk (%ld)", q_offset, Tq, Tk);
    if (chunk < 1) return att_fail(who, "chunk %ld < 1", chunk, 0, 0);
    if (left < -1 || right < -1) return att_fail(who, "left %ld, right %ld: a context is >= 0, or -1 for unlimited", left, right, 0);
    if (pos0 < 0 || (long)pos0 + Tk > NNTK_ATTENTION_MAX_POSITION)
        return att_fail(who, "pos0 %ld: pos0 >= 0 and pos0 + Tk <= %ld", pos0, NNTK_ATTENTION_MAX_POSITION, 0);
    if (!isfinite(scale)) return att_fail(who, "scale is not finite", 0, 0, 0);
    const long hd = (long)heads * d_head;
    if (qfs < hd || kfs < hd || vfs < hd)
        return att_fail(who, "frame strides %ld / %ld / ... : each must be at least heads * d_head = %ld floats", qfs, kfs, hd);
    if (qfs > ATT_MAX_STRIDE || kfs > ATT_MAX_STRIDE || vfs > ATT_MAX_STRIDE || qbs < 0 || kbs < 0 || vbs < 0 || qbs > ATT_MAX_STRIDE ||
        kbs > ATT_MAX_STRIDE || vbs > ATT_MAX_STRIDE)
        return att_fail(who, "a stride is negative or beyond 2^40 floats", 0, 0, 0);
    if (kv_lengths)
        for (int b = 0; b < batch; ++b)
            if (kv_lengths[b] < 0 || kv_lengths[b] > Tk) return att_fail(who, "kv_lengths[%ld] = %ld is outside [0, Tk = %ld]", b, kv_lengths[b], Tk);
    return 0;
}

int nntk_attention_device(const float *d_q, const float *d_k, const float *d_v, int batch, int heads, int d_head, int Tq, int Tk,
                          long q_frame_stride, long q_batch_stride, long k_frame_stride, long k_batch_stride, long v_frame_stride,
                          long v_batch_stride, const int *kv_lengths, int q_offset, int pos0, int chunk, int left, int right, float scale,
                          float *d_out, float *d_lse) {
    static const char who[] = "nntk_attention_device";
    nntk_shim_clear_error();
    if (att_check(who, batch, heads, d_head, Tq, Tk, q_frame_stride, q_batch_stride, k_frame_stride, k_batch_stride, v_frame_stride,
                  v_batch_stride, kv_lengths, q_offset, pos0, chunk, left, right, scale))
        return -1;
    if (batch == 0) return 0;
    if (!d_q || !d_k || !d_v || !d_out) return att_fail(who, "NULL tensor", 0, 0, 0);
    if (((uintptr_t)d_q | (uintptr_t)d_k | (uintptr_t)d_v | (uintptr_t)d_out | (uintptr_t)d_lse) & 3)
        return att_fail(who, "a tensor is not 4-byte aligned", 0, 0, 0);
    const int hd = heads * d_head;
    const size_t n_out = (size_t)batch * Tq * hd, n_lse = (size_t)batch * heads * Tq;
    const void *in[3] = {d_q, d_k, d_v};
    const size_t n_in[3] = {att_span(batch, Tq, q_frame_stride, q_batch_stride, hd), att_span(batch, Tk, k_frame_stride, k_batch_stride, hd),
                            att_span(batch, Tk, v_frame_stride, v_batch_stride, hd)};
    for (int t = 0; t < 3; ++t)
        if (att_overlap(d_out, n_out, in[t], n_in[t]) || att_overlap(d_lse, n_lse, in[t], n_in[t]))
            return att_fail(who, "an output overlaps an input", 0, 0, 0);
    if (att_overlap(d_out, n_out, d_lse, n_lse)) return att_fail(who, "d_out and d_lse overlap", 0, 0, 0);
    return nntk_shim_attention(d_q, d_k, d_v, batch, heads, d_head, Tq, Tk, q_frame_stride, q_batch_stride, k_frame_stride, k_batch_stride,
                               v_frame_stride, v_batch_stride, kv_lengths, q_offset, pos0, chunk, left, right, scale, d_out, d_lse);
}

int nntk_attention(const float *q, const float *k, const float *v, int batch, int heads, int d_head, int Tq, int Tk, long q_frame_stride,
                   long q_batch_stride, long k_frame_stride, long k_batch_stride, long v_frame_stride, long v_batch_stride,
                   const int *kv_lengths, int q_offset, int pos0, int chunk, int left, int right, float scale, float *out, float *lse) {
    static const char who[] = "nntk_attention";
    nntk_shim_clear_error();
    if (att_check(who, batch, heads, d_head, Tq, Tk, q_frame_stride, q_batch_stride, k_frame_stride, k_batch_stride, v_frame_stride,
                  v_batch_stride, kv_lengths, q_offset, pos0, chunk, left, right, scale))
        return -1;
    if (batch == 0) return 0;
    if (!q || !k || !v || !out) return att_fail(who, "NULL array", 0, 0, 0);
    if (((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)out | (uintptr_t)lse) & 3)
        return att_fail(who, "an array is not 4-byte aligned", 0, 0, 0);
    const int hd = heads * d_head;
    const size_t n_out = (size_t)batch * Tq * hd, n_lse = (size_t)batch * heads * Tq;
    const size_t nq = att_span(batch, Tq, q_frame_stride, q_batch_stride, hd), nk = att_span(batch, Tk, k_frame_stride, k_batch_stride, hd),
                 nv = att_span(batch, Tk, v_frame_stride, v_batch_stride, hd);
    if (att_overlap(out, n_out, q, nq) || att_overlap(out, n_out, k, nk) || att_overlap(out, n_out, v, nv) || att_overlap(lse, n_lse, q, nq) ||
        att_overlap(lse, n_lse, k, nk) || att_overlap(lse, n_lse, v, nv))
        return att_fail(who, "an output overlaps an input", 0, 0, 0);
    if (att_overlap(out, n_out, lse, n_lse)) return att_fail(who, "out and lse overlap", 0, 0, 0);
    float *d_in = nntk_devbuf_reserve(&t_a, nq + nk + nv);                             /* q | k | v, each with its own strides */
    float *d_o = nntk_devbuf_reserve(&t_b, n_out + n_lse);                             /* out | lse */
    if (!d_in || !d_o) return -1;
    if (nntk_shim_upload(d_in, q, nq * 4) || nntk_shim_upload(d_in + nq, k, nk * 4) || nntk_shim_upload(d_in + nq + nk, v, nv * 4)) return -1;
    if (nntk_attention_device(d_in, d_in + nq, d_in + nq + nk, batch, heads, d_head, Tq, Tk, q_frame_stride, q_batch_stride, k_frame_stride,
                              k_batch_stride, v_frame_stride, v_batch_stride, kv_lengths, q_offset, pos0, chunk, left, right, scale, d_o,
                              lse ? d_o + n_out : NULL))
        return -1;
    if (nntk_shim_download(out, d_o, n_out * 4)) return -1;
    return lse ? nntk_shim_download(lse, d_o + n_out, n_lse * 4) : 0;
}

/* ---- the backward of the attention core (csrc/hip/attention_bwd.hip) ---- */

size_t nntk_attention_backward_workspace_floats(int batch, int heads, int Tq) {
    if (batch < 1 || heads < 1 || heads > NNTK_ATTENTION_MAX_HEADS || Tq < 1 || Tq > NNTK_ATTENTION_MAX_FRAMES) return 0;
    return (size_t)batch * (size_t)heads * (size_t)Tq;
}

/* two tensors of hd-float slices on the same frame stride gfs (a fused gradient buffer): their slices share a float */
static int att_slices_overlap(const float *a, size_t na, const float *b, size_t nb, long gfs, int hd) {
    if (!att_overlap(a, na, b, nb)) return 0;
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    const uintptr_t m = ((x > y ? x - y : y - x) / 4) % (uintptr_t)gfs;            /* the phase of one against the other's frames */
    return m < (uintptr_t)hd || m > (uintptr_t)(gfs - hd);
}

/* the pointers of a backward call (ws == NULL with need_ws == 0: the host form), after att_check */
static int att_bwd_check(const char *who, const float *q, const float *k, const float *v, const float *out, const float *lse,
                         const float *dout, int batch, int heads, int d_head, int Tq, int Tk, long qfs, long qbs, long kfs, long kbs,
                         long vfs, long vbs, long gfs, const float *dq, const float *dk, const float *dv, const float *ws, int need_ws) {
    const int hd = heads * d_head;
    if (!q || !k || !v || !out || !lse || !dout) return att_fail(who, "NULL input tensor (q, k, v, out, lse and dout are all needed)", 0, 0, 0);
    if (!dq || !dk || !dv) return att_fail(who, "NULL gradient tensor", 0, 0, 0);
    if (need_ws && !ws) return att_fail(who, "NULL workspace", 0, 0, 0);
    if (gfs < hd || gfs > ATT_MAX_STRIDE) return att_fail(who, "grad_frame_stride %ld: at least heads * d_head = %ld floats, at most 2^40", gfs, hd, 0);
    if (((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)out | (uintptr_t)lse | (uintptr_t)dout | (uintptr_t)dq | (uintptr_t)dk |
         (uintptr_t)dv | (uintptr_t)ws) & 3)
        return att_fail(who, "a tensor is not 4-byte aligned", 0, 0, 0);
    const size_t n_out = (size_t)batch * Tq * hd, n_lse = (size_t)batch * heads * Tq;
    const void *in[6] = {q, k, v, out, lse, dout};
    const size_t n_in[6] = {att_span(batch, Tq, qfs, qbs, hd), att_span(batch, Tk, kfs, kbs, hd), att_span(batch, Tk, vfs, vbs, hd), n_out, n_lse, n_out};
    const float *g[4] = {dq, dk, dv, ws};
    const size_t n_g[4] = {att_span(batch, Tq, gfs, Tq * gfs, hd), att_span(batch, Tk, gfs, Tk * gfs, hd), att_span(batch, Tk, gfs, Tk * gfs, hd), n_lse};
    for (int t = 0; t < 4; ++t)
        for (int u = 0; u < 6; ++u)
            if (att_overlap(g[t], n_g[t], in[u], n_in[u])) return att_fail(who, "a gradient tensor or the workspace overlaps an input", 0, 0, 0);
    for (int t = 0; t < 3; ++t) {
        if (att_overlap(g[t], n_g[t], ws, n_lse)) return att_fail(who, "a gradient tensor and the workspace overlap", 0, 0, 0);
        for (int u = t + 1; u < 3; ++u)
            if (att_slices_overlap(g[t], n_g[t], g[u], n_g[u], gfs, hd)) return att_fail(who, "two gradient tensors overlap", 0, 0, 0);
    }
    return 0;
}

int nntk_attention_backward_device(const float *d_q, const float *d_k, const float *d_v, const float *d_out, const float *d_lse,
                                   const float *d_dout, int batch, int heads, int d_head, int Tq, int Tk, long q_frame_stride,
                                   long q_batch_stride, long k_frame_stride, long k_batch_stride, long v_frame_stride, long v_batch_stride,
                                   const int *kv_lengths, int q_offset, int pos0, int chunk, int left, int right, float scale,
                                   long grad_frame_stride, float *d_dq, float *d_dk, float *d_dv, float *d_workspace) {
    static const char who[] = "nntk_attention_backward_device";
    nntk_shim_clear_error();
    if (att_check(who, batch, heads, d_head, Tq, Tk, q_frame_stride, q_batch_stride, k_frame_stride, k_batch_stride, v_frame_stride,
                  v_batch_stride, kv_lengths, q_offset, pos0, chunk, left, right, scale))
        return -1;
    if (batch == 0) return 0;
    if (att_bwd_check(who, d_q, d_k, d_v, d_out, d_lse, d_dout, batch, heads, d_head, Tq, Tk, q_frame_stride, q_batch_stride, k_frame_stride,
                      k_batch_stride, v_frame_stride, v_batch_stride, grad_frame_stride, d_dq, d_dk, d_dv, d_workspace, 1))
        return -1;
    return nntk_shim_attention_backward(d_q, d_k, d_v, d_out, d_lse, d_dout, batch, heads, d_head, Tq, Tk, q_frame_stride, q_batch_stride,
                                        k_frame_stride, k_batch_stride, v_frame_stride, v_batch_stride, kv_lengths, q_offset, pos0, chunk,
                                        left, right, scale, grad_frame_stride, d_dq, d_dk, d_dv, d_workspace);
}

/* rows of hd floats, packed at src, to a host tensor with frame stride gfs: the floats between the slices are not touched */
static void att_scatter_rows(float *dst, const float *src, size_t rows, long gfs, int hd) {
    for (size_t r = 0; r < rows; ++r) memcpy(dst + r * (size_t)gfs, src + r * (size_t)hd, (size_t)hd * 4);
}

int nntk_attention_backward(const float *q, const float *k, const float *v, const float *out, const float *lse, const float *dout, int batch,
                            int heads, int d_head, int Tq, int Tk, long q_frame_stride, long q_batch_stride, long k_frame_stride,
                            long k_batch_stride, long v_frame_stride, long v_batch_stride, const int *kv_lengths, int q_offset, int pos0,
                            int chunk, int left, int right, float scale, long grad_frame_stride, float *dq, float *dk, float *dv) {
    static const char who[] = "nntk_attention_backward";
    nntk_shim_clear_error();
    if (att_check(who, batch, heads, d_head, Tq, Tk, q_frame_stride, q_batch_stride, k_frame_stride, k_batch_stride, v_frame_stride,
                  v_batch_stride, kv_lengths, q_offset, pos0, chunk, left, right, scale))
        return -1;
    if (batch == 0) return 0;
    if (att_bwd_check(who, q, k, v, out, lse, dout, batch, heads, d_head, Tq, Tk, q_frame_stride, q_batch_stride, k_frame_stride,
                      k_batch_stride, v_frame_stride, v_batch_stride, grad_frame_stride, dq, dk, dv, NULL, 0))
        return -1;
    const int hd = heads * d_head;
    const size_t n_out = (size_t)batch * Tq * hd, n_kv = (size_t)batch * Tk * hd, n_lse = (size_t)batch * heads * Tq;
    const size_t nq = att_span(batch, Tq, q_frame_stride, q_batch_stride, hd), nk = att_span(batch, Tk, k_frame_stride, k_batch_stride, hd),
                 nv = att_span(batch, Tk, v_frame_stride, v_batch_stride, hd);
    float *d_in = nntk_devbuf_reserve(&t_a, nq + nk + nv + 2 * n_out + n_lse);         /* q | k | v | out | dout | lse */
    float *d_g = nntk_devbuf_reserve(&t_b, n_out + 2 * n_kv + n_lse);                  /* dq | dk | dv, dense, | workspace */
    if (!d_in || !d_g) return -1;
    float *d_k = d_in + nq, *d_v = d_k + nk, *d_o = d_v + nv, *d_do = d_o + n_out, *d_l = d_do + n_out;
    if (nntk_shim_upload(d_in, q, nq * 4) || nntk_shim_upload(d_k, k, nk * 4) || nntk_shim_upload(d_v, v, nv * 4) ||
        nntk_shim_upload(d_o, out, n_out * 4) || nntk_shim_upload(d_do, dout, n_out * 4) || nntk_shim_upload(d_l, lse, n_lse * 4))
        return -1;
    if (nntk_attention_backward_device(d_in, d_k, d_v, d_o, d_l, d_do, batch, heads, d_head, Tq, Tk, q_frame_stride, q_batch_stride,
                                       k_frame_stride, k_batch_stride, v_frame_stride, v_batch_stride, kv_lengths, q_offset, pos0, chunk, left,
                                       right, scale, hd, d_g, d_g + n_out, d_g + n_out + n_kv, d_g + n_out + 2 * n_kv))
        return -1;
    float *stage = malloc((n_out + 2 * n_kv) * 4);
    if (!stage) return att_fail(who, "out of host memory", 0, 0, 0);
    const int rc = nntk_shim_download(stage, d_g, (n_out + 2 * n_kv) * 4);
    if (!rc) {
        att_scatter_rows(dq, stage, (size_t)batch * Tq, grad_frame_stride, hd);
        att_scatter_rows(dk, stage + n_out, (size_t)batch * Tk, grad_frame_stride, hd);
        att_scatter_rows(dv, stage + n_out + n_kv, (size_t)batch * Tk, grad_frame_stride, hd);
    }
    free(stage);
    return rc;
}
