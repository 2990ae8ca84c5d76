/*
 * rnnt.c -- host layer of the RNN-Transducer calls (csrc/hip/rnnt.hip): the loss over the [batch][T][max_label_len + 1][V] lattice of
 * unnormalised scores with its gradient, and the joiner with its backward.  Every host array, shape, limit and pointer is checked
 * here, before anything is enqueued or allocated: a refusal needs no device.  The loss has a device-pointer form and a host-pointer
 * form (upload, device call, download).
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include "nntk_internal.h"

#define t_a (*nntk_thread_scratch(NNTK_TS_A))
#define t_b (*nntk_thread_scratch(NNTK_TS_B))
#define t_c (*nntk_thread_scratch(NNTK_TS_C))

static int rnnt_fail(const char *who, const char *fmt, int a, int b, int c) {
    char msg[200];
    int n = snprintf(msg, sizeof msg, "%s: ", who);
    snprintf(msg + n, sizeof msg - (size_t)n, fmt, a, b, c);
    nntk_set_error(msg);
    return -1;
}

/* everything that lives in host memory, and the limits of the kernels */
static int rnnt_check(const char *who, int batch, int T, int V, const int *input_lengths, const int *labels, const int *label_lengths,
                      int max_label_len, int blank) {
    if (batch < 0 || T < 0 || max_label_len < 0)
        return rnnt_fail(who, "batch %d, T %d, max_label_len %d: none may be negative", batch, T, max_label_len);
    if (V < 2) return rnnt_fail(who, "V %d < 2: a transducer has the blank and at least one label", V, 0, 0);
    if (blank < 0 || blank >= V) return rnnt_fail(who, "blank %d is outside [0, %d)", blank, V, 0);
    if (max_label_len > NNTK_RNNT_MAX_LABELS)
        return rnnt_fail(who, "max_label_len %d is beyond what one workgroup's LDS holds (%d)", max_label_len, NNTK_RNNT_MAX_LABELS, 0);
    if ((long long)T + max_label_len > NNTK_RNNT_MAX_DIAGONALS)
        return rnnt_fail(who, "T + max_label_len = %d is more than %d lattice diagonals", T + max_label_len, NNTK_RNNT_MAX_DIAGONALS, 0);
    if (batch > 0 && (!label_lengths || (max_label_len > 0 && !labels))) return rnnt_fail(who, "NULL labels / label_lengths", 0, 0, 0);
    if (batch > 0 && T < 1) return rnnt_fail(who, "T %d < 1", T, 0, 0);
    for (int b = 0; b < batch; ++b) {
        if (input_lengths && (input_lengths[b] < 1 || input_lengths[b] > T))
            return rnnt_fail(who, "input_lengths[%d] = %d is outside [1, %d]", b, input_lengths[b], T);
        const int L = label_lengths[b];
        if (L < 0 || L > max_label_len) return rnnt_fail(who, "label_lengths[%d] = %d is outside [0, %d]", b, L, max_label_len);
        for (int i = 0; i < L; ++i) {
            const int k = labels[(size_t)b * max_label_len + i];
            if (k < 0 || k >= V) return rnnt_fail(who, "labels[%d][%d] = %d is not a class", b, i, k);
            if (k == blank) return rnnt_fail(who, "labels[%d][%d] is the blank (%d)", b, i, k);
        }
    }
    return 0;
}

static int rnnt_check_ptr(const char *who, const char *name, const void *p, unsigned align) {
    char msg[200];
    if (p && ((uintptr_t)p & (align - 1)) == 0) return 0;
    if (p) snprintf(msg, sizeof msg, "%s: %s is not %u-byte aligned", who, name, align);
    else snprintf(msg, sizeof msg, "%s: %s is NULL", who, name);
    nntk_set_error(msg);
    return -1;
}

size_t nntk_rnnt_workspace_floats(int batch, int T, int max_label_len, int want_grad) {
    return nntk_shim_rnnt_workspace_floats(batch, T, max_label_len, want_grad != 0);
}

int nntk_rnnt_loss_device(const float *d_logits, int batch, int T, int V, const int *input_lengths, const int *labels,
                          const int *label_lengths, int max_label_len, int blank, float *d_loss_rows, float *d_dlogits,
                          float *d_workspace) {
    static const char who[] = "nntk_rnnt_loss_device";
    nntk_shim_clear_error();
    if (rnnt_check(who, batch, T, V, input_lengths, labels, label_lengths, max_label_len, blank)) return -1;
    if (batch == 0) return 0;
    if (rnnt_check_ptr(who, "d_logits", d_logits, 16) || rnnt_check_ptr(who, "d_loss_rows", d_loss_rows, 4) ||
        rnnt_check_ptr(who, "d_workspace", d_workspace, 16) || (d_dlogits && rnnt_check_ptr(who, "d_dlogits", d_dlogits, 16))) return -1;
    const size_t bytes = (size_t)batch * T * (max_label_len + 1) * V * sizeof(float);
    if (d_dlogits && (uintptr_t)d_dlogits < (uintptr_t)d_logits + bytes && (uintptr_t)d_logits < (uintptr_t)d_dlogits + bytes)
        return rnnt_fail(who, "d_dlogits overlaps d_logits", 0, 0, 0);
    int *len = (int *)malloc((size_t)batch * sizeof(int));
    if (!len) NNTK_FAIL("out of host memory");
    for (int b = 0; b < batch; ++b) len[b] = input_lengths ? input_lengths[b] : T;
    int rc = nntk_shim_rnnt_loss(d_logits, batch, T, V, len, labels, label_lengths, max_label_len, blank, d_loss_rows, d_dlogits,
                                 d_workspace);
    free(len);
    return rc;
}

int nntk_rnnt_loss(const float *logits, int batch, int T, int V, const int *input_lengths, const int *labels, const int *label_lengths,
                   int max_label_len, int blank, float *loss_rows, float *dlogits) {
    static const char who[] = "nntk_rnnt_loss";
    nntk_shim_clear_error();
    if (rnnt_check(who, batch, T, V, input_lengths, labels, label_lengths, max_label_len, blank)) return -1;
    if (batch == 0) return 0;
    if (rnnt_check_ptr(who, "logits", logits, 4) || rnnt_check_ptr(who, "loss_rows", loss_rows, 4) ||
        (dlogits && rnnt_check_ptr(who, "dlogits", dlogits, 4))) return -1;
    const size_t n = (size_t)batch * T * (max_label_len + 1) * V;
    float *d_x = nntk_devbuf_reserve(&t_a, n + (size_t)batch + 4);
    float *d_g = dlogits ? nntk_devbuf_reserve(&t_b, n + 4) : NULL;
    float *d_ws = nntk_devbuf_reserve(&t_c, nntk_shim_rnnt_workspace_floats(batch, T, max_label_len, dlogits != NULL));
    if (!d_x || (dlogits && !d_g) || !d_ws) return -1;
    float *d_loss = d_x + n;
    if (nntk_shim_upload(d_x, logits, n * sizeof(float))) return -1;
    if (nntk_rnnt_loss_device(d_x, batch, T, V, input_lengths, labels, label_lengths, max_label_len, blank, d_loss, d_g, d_ws)) return -1;
    if (nntk_shim_download(loss_rows, d_loss, (size_t)batch * sizeof(float))) return -1;
    return dlogits ? nntk_shim_download(dlogits, d_g, n * sizeof(float)) : 0;
}

/* ---- the joiner ---- */
static int joint_check(const char *who, int batch, int T, int U1, int J, int activation) {
    if (batch < 0 || T < 0 || U1 < 0) return rnnt_fail(who, "batch %d, T %d, U1 %d: none may be negative", batch, T, U1);
    if (J < 0) return rnnt_fail(who, "J %d < 0", J, 0, 0);
    if (activation < 0 || activation > 2) return rnnt_fail(who, "activation %d is none of 0 (identity), 1 (tanh), 2 (relu)", activation, 0, 0);
    return 0;
}

int nntk_rnnt_joint_device(const float *d_enc, const float *d_pred, int batch, int T, int U1, int J, int activation, float *d_out) {
    static const char who[] = "nntk_rnnt_joint_device";
    nntk_shim_clear_error();
    if (joint_check(who, batch, T, U1, J, activation)) return -1;
    if ((size_t)batch * T * U1 * J == 0) return 0;
    if (rnnt_check_ptr(who, "d_enc", d_enc, 4) || rnnt_check_ptr(who, "d_pred", d_pred, 4) || rnnt_check_ptr(who, "d_out", d_out, 4)) return -1;
    return nntk_shim_rnnt_joint(d_enc, d_pred, batch, T, U1, J, activation, d_out);
}

int nntk_rnnt_joint_backward_device(const float *d_out_fwd, const float *d_dout, int batch, int T, int U1, int J, int activation,
                                    float *d_denc, float *d_dpred) {
    static const char who[] = "nntk_rnnt_joint_backward_device";
    nntk_shim_clear_error();
    if (joint_check(who, batch, T, U1, J, activation)) return -1;
    if ((size_t)batch * T * U1 * J == 0) return 0;
    if ((activation != 0 && rnnt_check_ptr(who, "d_out_fwd", d_out_fwd, 4)) || rnnt_check_ptr(who, "d_dout", d_dout, 4) ||
        rnnt_check_ptr(who, "d_denc", d_denc, 4) || rnnt_check_ptr(who, "d_dpred", d_dpred, 4)) return -1;
    return nntk_shim_rnnt_joint_backward(d_out_fwd, d_dout, batch, T, U1, J, activation, d_denc, d_dpred);
}

/* ---- the fused training loss: joiner + vocabulary projection + loss, the scores never stored (csrc/hip/rnnt_fused.hip) ---- */
static int fused_check(const char *who, int batch, int T, int J, int V, int activation, const int *input_lengths, const int *labels,
                       const int *label_lengths, int max_label_len, int blank, const void *denc, const void *dpred, const void *ddout) {
    if (rnnt_check(who, batch, T, V, input_lengths, labels, label_lengths, max_label_len, blank)) return -1;
    if (joint_check(who, batch, T, max_label_len + 1, J, activation)) return -1;
    if (J < 1 || J > NNTK_RNNT_FUSED_MAX_J) return rnnt_fail(who, "J %d is outside [1, %d]", J, NNTK_RNNT_FUSED_MAX_J, 0);
    if (V > NNTK_RNNT_FUSED_MAX_V) return rnnt_fail(who, "V %d is more than %d", V, NNTK_RNNT_FUSED_MAX_V, 0);
    const int given = (denc != NULL) + (dpred != NULL) + (ddout != NULL);
    if (given != 0 && given != 3)
        return rnnt_fail(who, "the gradient outputs d_denc, d_dpred, d_dout are all NULL or all given (%d of 3 are)", given, 0, 0);
    return 0;
}

typedef struct { const char *name; uintptr_t at; size_t bytes; } fused_span;

size_t nntk_rnnt_fused_workspace_floats(int batch, int T, int max_label_len, int J, int V, int want_grad) {
    return nntk_shim_rnnt_fused_workspace_floats(batch, T, max_label_len, J, V, want_grad != 0);
}

int nntk_rnnt_fused_loss_device(const float *d_enc, const float *d_pred, const float *d_out, int batch, int T, int J, int V, int activation,
                                const int *input_lengths, const int *labels, const int *label_lengths, int max_label_len, int blank,
                                float *d_loss_rows, float *d_denc, float *d_dpred, float *d_dout, float *d_workspace) {
    static const char who[] = "nntk_rnnt_fused_loss_device";
    nntk_shim_clear_error();
    if (fused_check(who, batch, T, J, V, activation, input_lengths, labels, label_lengths, max_label_len, blank, d_denc, d_dpred, d_dout))
        return -1;
    if (batch == 0) return 0;
    if (rnnt_check_ptr(who, "d_enc", d_enc, 4) || rnnt_check_ptr(who, "d_pred", d_pred, 4) || rnnt_check_ptr(who, "d_out", d_out, 4) ||
        rnnt_check_ptr(who, "d_loss_rows", d_loss_rows, 4) || rnnt_check_ptr(who, "d_workspace", d_workspace, 16) ||
        (d_denc && (rnnt_check_ptr(who, "d_denc", d_denc, 4) || rnnt_check_ptr(who, "d_dpred", d_dpred, 4) ||
                    rnnt_check_ptr(who, "d_dout", d_dout, 4)))) return -1;
    const size_t U1 = (size_t)max_label_len + 1, f = sizeof(float);
    const size_t ne = (size_t)batch * T * J, npd = (size_t)batch * U1 * J, nw = ((size_t)J + 1) * V;
    /* outputs first: each of them against everything after it */
    const fused_span sp[] = {{"d_loss_rows", (uintptr_t)d_loss_rows, (size_t)batch * f}, {"d_denc", (uintptr_t)d_denc, ne * f},
                             {"d_dpred", (uintptr_t)d_dpred, npd * f}, {"d_dout", (uintptr_t)d_dout, nw * f},
                             {"d_enc", (uintptr_t)d_enc, ne * f}, {"d_pred", (uintptr_t)d_pred, npd * f}, {"d_out", (uintptr_t)d_out, nw * f},
                             {"d_workspace", (uintptr_t)d_workspace,
                              nntk_shim_rnnt_fused_workspace_floats(batch, T, max_label_len, J, V, d_denc != NULL) * f}};
    for (int o = 0; o < 4; ++o)
        for (int k = o + 1; k < 8; ++k)
            if (sp[o].at && sp[k].at && sp[o].at < sp[k].at + sp[k].bytes && sp[k].at < sp[o].at + sp[o].bytes) {
                char msg[200];
                snprintf(msg, sizeof msg, "%s: %s overlaps %s", who, sp[o].name, sp[k].name);
                nntk_set_error(msg);
                return -1;
            }
    int *len = (int *)malloc((size_t)batch * sizeof(int));
    if (!len) NNTK_FAIL("out of host memory");
    for (int b = 0; b < batch; ++b) len[b] = input_lengths ? input_lengths[b] : T;
    int rc = nntk_shim_rnnt_fused_loss(d_enc, d_pred, d_out, batch, T, J, V, activation, len, labels, label_lengths, max_label_len, blank,
                                       d_loss_rows, d_denc, d_dpred, d_dout, d_workspace);
    free(len);
    return rc;
}

int nntk_rnnt_fused_loss(const float *enc, const float *pred, const float *out, int batch, int T, int J, int V, int activation,
                         const int *input_lengths, const int *labels, const int *label_lengths, int max_label_len, int blank,
                         float *loss_rows, float *denc, float *dpred, float *dout) {
    static const char who[] = "nntk_rnnt_fused_loss";
    nntk_shim_clear_error();
    if (fused_check(who, batch, T, J, V, activation, input_lengths, labels, label_lengths, max_label_len, blank, denc, dpred, dout)) return -1;
    if (batch == 0) return 0;
    if (rnnt_check_ptr(who, "enc", enc, 4) || rnnt_check_ptr(who, "pred", pred, 4) || rnnt_check_ptr(who, "out", out, 4) ||
        rnnt_check_ptr(who, "loss_rows", loss_rows, 4) ||
        (denc && (rnnt_check_ptr(who, "denc", denc, 4) || rnnt_check_ptr(who, "dpred", dpred, 4) || rnnt_check_ptr(who, "dout", dout, 4))))
        return -1;
    const size_t up = 3, U1 = (size_t)max_label_len + 1;
    const size_t ne = ((size_t)batch * T * J + up) & ~up, npd = ((size_t)batch * U1 * J + up) & ~up, nw = (((size_t)J + 1) * V + up) & ~up;
    const size_t nl = ((size_t)batch + up) & ~up;
    /* inputs | loss rows in one block, the gradients in a second, the workspace in a third */
    float *d_in = nntk_devbuf_reserve(&t_a, ne + npd + nw + nl + 4);
    float *d_g = denc ? nntk_devbuf_reserve(&t_b, ne + npd + nw + 4) : NULL;
    float *d_ws = nntk_devbuf_reserve(&t_c, nntk_shim_rnnt_fused_workspace_floats(batch, T, max_label_len, J, V, denc != NULL));
    if (!d_in || (denc && !d_g) || !d_ws) return -1;
    float *d_enc = d_in, *d_pred = d_in + ne, *d_out = d_pred + npd, *d_loss = d_out + nw;
    if (nntk_shim_upload(d_enc, enc, (size_t)batch * T * J * sizeof(float)) || nntk_shim_upload(d_pred, pred, (size_t)batch * U1 * J * sizeof(float)) ||
        nntk_shim_upload(d_out, out, ((size_t)J + 1) * V * sizeof(float))) return -1;
    if (nntk_rnnt_fused_loss_device(d_enc, d_pred, d_out, batch, T, J, V, activation, input_lengths, labels, label_lengths, max_label_len, blank,
                                    d_loss, d_g, d_g ? d_g + ne : NULL, d_g ? d_g + ne + npd : NULL, d_ws)) return -1;
    if (nntk_shim_download(loss_rows, d_loss, (size_t)batch * sizeof(float))) return -1;
    if (!denc) return 0;
    if (nntk_shim_download(denc, d_g, (size_t)batch * T * J * sizeof(float)) ||
        nntk_shim_download(dpred, d_g + ne, (size_t)batch * U1 * J * sizeof(float))) return -1;
    return nntk_shim_download(dout, d_g + ne + npd, ((size_t)J + 1) * V * sizeof(float));
}

/* ---- forced alignment (csrc/hip/rnnt_align.hip): the best single path, on stored scores and on the joiner's inputs ---- */
/* the first `outputs` spans each against everything after it; a span at 0 is an output not asked for */
static int align_overlap(const char *who, const fused_span *sp, int outputs, int n) {
    for (int o = 0; o < outputs; ++o)
        for (int k = o + 1; k < n; ++k)
            if (sp[o].at && sp[k].at && sp[o].at < sp[k].at + sp[k].bytes && sp[k].at < sp[o].at + sp[o].bytes) {
                char msg[200];
                snprintf(msg, sizeof msg, "%s: %s overlaps %s", who, sp[o].name, sp[k].name);
                nntk_set_error(msg);
                return -1;
            }
    return 0;
}

static int align_check_outputs(const char *who, const int *label_frames, const int *frame_labels, const float *label_logp,
                               const float *frame_logp, const float *scores) {
    return rnnt_check_ptr(who, "scores", scores, 4) || (label_frames && rnnt_check_ptr(who, "label_frames", label_frames, 4)) ||
           (frame_labels && rnnt_check_ptr(who, "frame_labels", frame_labels, 4)) ||
           (label_logp && rnnt_check_ptr(who, "label_logp", label_logp, 4)) || (frame_logp && rnnt_check_ptr(who, "frame_logp", frame_logp, 4));
}

size_t nntk_rnnt_align_workspace_floats(int batch, int T, int max_label_len) {
    return nntk_shim_rnnt_align_workspace_floats(batch, T, max_label_len);
}

int nntk_rnnt_align_device(const float *d_logits, int batch, int T, int V, const int *input_lengths, const int *labels,
                           const int *label_lengths, int max_label_len, int blank, int *d_label_frames, int *d_frame_labels,
                           float *d_label_logp, float *d_frame_logp, float *d_scores, float *d_workspace) {
    static const char who[] = "nntk_rnnt_align_device";
    nntk_shim_clear_error();
    if (rnnt_check(who, batch, T, V, input_lengths, labels, label_lengths, max_label_len, blank)) return -1;
    if (batch == 0) return 0;
    if (rnnt_check_ptr(who, "d_logits", d_logits, 16) || rnnt_check_ptr(who, "d_workspace", d_workspace, 16) ||
        align_check_outputs(who, d_label_frames, d_frame_labels, d_label_logp, d_frame_logp, d_scores)) return -1;
    const size_t f = sizeof(float), nl = (size_t)batch * max_label_len * f, nt = (size_t)batch * T * f;
    const fused_span sp[] = {{"d_label_frames", (uintptr_t)d_label_frames, nl}, {"d_frame_labels", (uintptr_t)d_frame_labels, nt},
                             {"d_label_logp", (uintptr_t)d_label_logp, nl}, {"d_frame_logp", (uintptr_t)d_frame_logp, nt},
                             {"d_scores", (uintptr_t)d_scores, (size_t)batch * f},
                             {"d_logits", (uintptr_t)d_logits, (size_t)batch * T * (max_label_len + 1) * V * f},
                             {"d_workspace", (uintptr_t)d_workspace, nntk_shim_rnnt_align_workspace_floats(batch, T, max_label_len) * f}};
    if (align_overlap(who, sp, 5, 7)) return -1;
    int *len = (int *)malloc((size_t)batch * sizeof(int));
    if (!len) NNTK_FAIL("out of host memory");
    for (int b = 0; b < batch; ++b) len[b] = input_lengths ? input_lengths[b] : T;
    int rc = nntk_shim_rnnt_align(d_logits, batch, T, V, len, labels, label_lengths, max_label_len, blank, d_label_frames, d_frame_labels,
                                  d_label_logp, d_frame_logp, d_scores, d_workspace);
    free(len);
    return rc;
}

/* the outputs of both host-pointer forms live in one device block: label_frames | frame_labels | label_logp | frame_logp | scores,
 * a part that is not asked for taking no room */
typedef struct { size_t lf, fl, ll, fp, sc, total; } align_out;
static align_out align_out_layout(int batch, int T, int max_label_len, const void *label_frames, const void *frame_labels,
                                  const void *label_logp, const void *frame_logp) {
    align_out o;
    const size_t nl = (size_t)batch * max_label_len, nt = (size_t)batch * T;
    o.lf = 0;
    o.fl = o.lf + (label_frames ? nl : 0);
    o.ll = o.fl + (frame_labels ? nt : 0);
    o.fp = o.ll + (label_logp ? nl : 0);
    o.sc = o.fp + (frame_logp ? nt : 0);
    o.total = o.sc + (size_t)batch;
    return o;
}

static int align_download(const align_out *o, const float *d_o, int batch, int T, int max_label_len, int *label_frames, int *frame_labels,
                          float *label_logp, float *frame_logp, float *scores) {
    const size_t nl = (size_t)batch * max_label_len * sizeof(float), nt = (size_t)batch * T * sizeof(float);
    if (label_frames && nl && nntk_shim_download(label_frames, d_o + o->lf, nl)) return -1;
    if (frame_labels && nntk_shim_download(frame_labels, d_o + o->fl, nt)) return -1;
    if (label_logp && nl && nntk_shim_download(label_logp, d_o + o->ll, nl)) return -1;
    if (frame_logp && nntk_shim_download(frame_logp, d_o + o->fp, nt)) return -1;
    return nntk_shim_download(scores, d_o + o->sc, (size_t)batch * sizeof(float));
}

int nntk_rnnt_align(const float *logits, int batch, int T, int V, const int *input_lengths, const int *labels, const int *label_lengths,
                    int max_label_len, int blank, int *label_frames, int *frame_labels, float *label_logp, float *frame_logp,
                    float *scores) {
    static const char who[] = "nntk_rnnt_align";
    nntk_shim_clear_error();
    if (rnnt_check(who, batch, T, V, input_lengths, labels, label_lengths, max_label_len, blank)) return -1;
    if (batch == 0) return 0;
    if (rnnt_check_ptr(who, "logits", logits, 4) || align_check_outputs(who, label_frames, frame_labels, label_logp, frame_logp, scores))
        return -1;
    const size_t n = (size_t)batch * T * (max_label_len + 1) * V;
    const align_out o = align_out_layout(batch, T, max_label_len, label_frames, frame_labels, label_logp, frame_logp);
    float *d_x = nntk_devbuf_reserve(&t_a, n + 4);
    float *d_o = nntk_devbuf_reserve(&t_b, o.total + 4);
    float *d_ws = nntk_devbuf_reserve(&t_c, nntk_shim_rnnt_align_workspace_floats(batch, T, max_label_len));
    if (!d_x || !d_o || !d_ws) return -1;
    if (nntk_shim_upload(d_x, logits, n * sizeof(float))) return -1;
    if (nntk_rnnt_align_device(d_x, batch, T, V, input_lengths, labels, label_lengths, max_label_len, blank,
                               label_frames ? (int *)(d_o + o.lf) : NULL, frame_labels ? (int *)(d_o + o.fl) : NULL,
                               label_logp ? d_o + o.ll : NULL, frame_logp ? d_o + o.fp : NULL, d_o + o.sc, d_ws)) return -1;
    return align_download(&o, d_o, batch, T, max_label_len, label_frames, frame_labels, label_logp, frame_logp, scores);
}

size_t nntk_rnnt_fused_align_workspace_floats(int batch, int T, int max_label_len, int J, int V) {
    return nntk_shim_rnnt_fused_align_workspace_floats(batch, T, max_label_len, J, V);
}

int nntk_rnnt_fused_align_device(const float *d_enc, const float *d_pred, const float *d_out, int batch, int T, int J, int V, int activation,
                                 const int *input_lengths, const int *labels, const int *label_lengths, int max_label_len, int blank,
                                 int *d_label_frames, int *d_frame_labels, float *d_label_logp, float *d_frame_logp, float *d_scores,
                                 float *d_workspace) {
    static const char who[] = "nntk_rnnt_fused_align_device";
    nntk_shim_clear_error();
    if (fused_check(who, batch, T, J, V, activation, input_lengths, labels, label_lengths, max_label_len, blank, NULL, NULL, NULL)) return -1;
    if (batch == 0) return 0;
    if (rnnt_check_ptr(who, "d_enc", d_enc, 4) || rnnt_check_ptr(who, "d_pred", d_pred, 4) || rnnt_check_ptr(who, "d_out", d_out, 4) ||
        rnnt_check_ptr(who, "d_workspace", d_workspace, 16) ||
        align_check_outputs(who, d_label_frames, d_frame_labels, d_label_logp, d_frame_logp, d_scores)) return -1;
    const size_t f = sizeof(float), nl = (size_t)batch * max_label_len * f, nt = (size_t)batch * T * f;
    const fused_span sp[] = {{"d_label_frames", (uintptr_t)d_label_frames, nl}, {"d_frame_labels", (uintptr_t)d_frame_labels, nt},
                             {"d_label_logp", (uintptr_t)d_label_logp, nl}, {"d_frame_logp", (uintptr_t)d_frame_logp, nt},
                             {"d_scores", (uintptr_t)d_scores, (size_t)batch * f},
                             {"d_enc", (uintptr_t)d_enc, (size_t)batch * T * J * f},
                             {"d_pred", (uintptr_t)d_pred, (size_t)batch * (max_label_len + 1) * J * f},
                             {"d_out", (uintptr_t)d_out, ((size_t)J + 1) * V * f},
                             {"d_workspace", (uintptr_t)d_workspace,
                              nntk_shim_rnnt_fused_align_workspace_floats(batch, T, max_label_len, J, V) * f}};
    if (align_overlap(who, sp, 5, 9)) return -1;
    int *len = (int *)malloc((size_t)batch * sizeof(int));
    if (!len) NNTK_FAIL("out of host memory");
    for (int b = 0; b < batch; ++b) len[b] = input_lengths ? input_lengths[b] : T;
    int rc = nntk_shim_rnnt_fused_align(d_enc, d_pred, d_out, batch, T, J, V, activation, len, labels, label_lengths, max_label_len, blank,
                                        d_label_frames, d_frame_labels, d_label_logp, d_frame_logp, d_scores, d_workspace);
    free(len);
    return rc;
}

int nntk_rnnt_fused_align(const float *enc, const float *pred, const float *out, int batch, int T, int J, int V, int activation,
                          const int *input_lengths, const int *labels, const int *label_lengths, int max_label_len, int blank,
                          int *label_frames, int *frame_labels, float *label_logp, float *frame_logp, float *scores) {
    static const char who[] = "nntk_rnnt_fused_align";
    nntk_shim_clear_error();
    if (fused_check(who, batch, T, J, V, activation, input_lengths, labels, label_lengths, max_label_len, blank, NULL, NULL, NULL)) return -1;
    if (batch == 0) return 0;
    if (rnnt_check_ptr(who, "enc", enc, 4) || rnnt_check_ptr(who, "pred", pred, 4) || rnnt_check_ptr(who, "out", out, 4) ||
        align_check_outputs(who, label_frames, frame_labels, label_logp, frame_logp, scores)) return -1;
    const size_t up = 3, U1 = (size_t)max_label_len + 1;
    const size_t ne = ((size_t)batch * T * J + up) & ~up, npd = ((size_t)batch * U1 * J + up) & ~up, nw = (((size_t)J + 1) * V + up) & ~up;
    const align_out o = align_out_layout(batch, T, max_label_len, label_frames, frame_labels, label_logp, frame_logp);
    float *d_in = nntk_devbuf_reserve(&t_a, ne + npd + nw + 4);
    float *d_o = nntk_devbuf_reserve(&t_b, o.total + 4);
    float *d_ws = nntk_devbuf_reserve(&t_c, nntk_shim_rnnt_fused_align_workspace_floats(batch, T, max_label_len, J, V));
    if (!d_in || !d_o || !d_ws) return -1;
    float *d_enc = d_in, *d_pred = d_in + ne, *d_out = d_pred + npd;
    if (nntk_shim_upload(d_enc, enc, (size_t)batch * T * J * sizeof(float)) || nntk_shim_upload(d_pred, pred, (size_t)batch * U1 * J * sizeof(float)) ||
        nntk_shim_upload(d_out, out, ((size_t)J + 1) * V * sizeof(float))) return -1;
    if (nntk_rnnt_fused_align_device(d_enc, d_pred, d_out, batch, T, J, V, activation, input_lengths, labels, label_lengths, max_label_len, blank,
                                     label_frames ? (int *)(d_o + o.lf) : NULL, frame_labels ? (int *)(d_o + o.fl) : NULL,
                                     label_logp ? d_o + o.ll : NULL, frame_logp ? d_o + o.fp : NULL, d_o + o.sc, d_ws)) return -1;
    return align_download(&o, d_o, batch, T, max_label_len, label_frames, frame_labels, label_logp, frame_logp, scores);
}
