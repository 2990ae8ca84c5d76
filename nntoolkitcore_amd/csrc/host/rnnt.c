/*
 * rnnt.c -- host layer of the RNN-Transducer calls (csrc/hip/rnnt.hip): the loss over the [batch][T][max_label_len + 1][V] lattice of
 * unnormalised scores with its gradient, and the joiner with its backward.  Every host array, shape, limit and pointer is checked
 * here, before anything is enqueued or allocated: a refusal needs no device.  Every call has a device-pointer form and a host-pointer
 * form (upload, device call, download); the two alignment calls -- on stored scores and on the joiner's inputs -- are one device body
 * and one host body that take the score source (nntk_shim_rnnt_src).  The pruned training loss (csrc/hip/rnnt_pruned.hip) -- simple
 * loss, prune ranges, banded joiner, banded loss -- is checked here too, with the same helpers.
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

/* the first `outputs` spans each against everything after it; a span at 0 is a pointer not given */
typedef struct { const char *name; uintptr_t at; size_t bytes; } rnnt_span;
static int rnnt_overlap(const char *who, const rnnt_span *sp, int outputs, int n) {
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

/* every row's frame count for the shim, which takes no NULL: input_lengths, or T; the caller frees it.  NULL: out of host memory */
static int *rnnt_lengths(const int *input_lengths, int batch, int T) {
    int *len = (int *)malloc((size_t)batch * sizeof(int));
    if (!len) { nntk_set_error("out of host memory"); return NULL; }
    for (int b = 0; b < batch; ++b) len[b] = input_lengths ? input_lengths[b] : T;
    return len;
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
    const rnnt_span sp[] = {{"d_dlogits", (uintptr_t)d_dlogits, bytes}, {"d_logits", (uintptr_t)d_logits, bytes}};
    if (rnnt_overlap(who, sp, 1, 2)) return -1;
    int *len = rnnt_lengths(input_lengths, batch, T);
    int rc = len ? nntk_shim_rnnt_loss(d_logits, batch, T, V, len, labels, label_lengths, max_label_len, blank, d_loss_rows, d_dlogits, d_workspace)
                 : -1;
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

/* the joiner's inputs of both fused host forms in one device block: enc | pred | out, each part rounded up to 16 bytes, then `extra`
 * floats for the caller */
typedef struct { size_t ne, npd, nw; float *d_enc, *d_pred, *d_out; } fused_in;
static int fused_stage(fused_in *s, const float *enc, const float *pred, const float *out, int batch, int T, int max_label_len, int J, int V,
                       size_t extra) {
    const size_t up = 3, re = (size_t)batch * T * J, rp = (size_t)batch * (max_label_len + 1) * J, rw = ((size_t)J + 1) * V;
    s->ne = (re + up) & ~up;
    s->npd = (rp + up) & ~up;
    s->nw = (rw + up) & ~up;
    s->d_enc = nntk_devbuf_reserve(&t_a, s->ne + s->npd + s->nw + extra + 4);
    if (!s->d_enc) return -1;
    s->d_pred = s->d_enc + s->ne;
    s->d_out = s->d_pred + s->npd;
    return nntk_shim_upload(s->d_enc, enc, re * sizeof(float)) || nntk_shim_upload(s->d_pred, pred, rp * sizeof(float)) ||
           nntk_shim_upload(s->d_out, out, rw * sizeof(float)) ? -1 : 0;
}

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
    /* outputs first */
    const rnnt_span sp[] = {{"d_loss_rows", (uintptr_t)d_loss_rows, (size_t)batch * f}, {"d_denc", (uintptr_t)d_denc, ne * f},
                            {"d_dpred", (uintptr_t)d_dpred, npd * f}, {"d_dout", (uintptr_t)d_dout, nw * f},
                            {"d_enc", (uintptr_t)d_enc, ne * f}, {"d_pred", (uintptr_t)d_pred, npd * f}, {"d_out", (uintptr_t)d_out, nw * f},
                            {"d_workspace", (uintptr_t)d_workspace,
                             nntk_shim_rnnt_fused_workspace_floats(batch, T, max_label_len, J, V, d_denc != NULL) * f}};
    if (rnnt_overlap(who, sp, 4, 8)) return -1;
    int *len = rnnt_lengths(input_lengths, batch, T);
    int rc = len ? nntk_shim_rnnt_fused_loss(d_enc, d_pred, d_out, batch, T, J, V, activation, len, labels, label_lengths, max_label_len, blank,
                                             d_loss_rows, d_denc, d_dpred, d_dout, d_workspace) : -1;
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
    /* inputs | loss rows in one block, the gradients in a second, the workspace in a third */
    fused_in s;
    if (fused_stage(&s, enc, pred, out, batch, T, max_label_len, J, V, ((size_t)batch + 3) & ~(size_t)3)) return -1;
    float *d_g = denc ? nntk_devbuf_reserve(&t_b, s.ne + s.npd + s.nw + 4) : NULL;
    float *d_ws = nntk_devbuf_reserve(&t_c, nntk_shim_rnnt_fused_workspace_floats(batch, T, max_label_len, J, V, denc != NULL));
    if ((denc && !d_g) || !d_ws) return -1;
    float *d_loss = s.d_out + s.nw;
    if (nntk_rnnt_fused_loss_device(s.d_enc, s.d_pred, s.d_out, batch, T, J, V, activation, input_lengths, labels, label_lengths, max_label_len,
                                    blank, d_loss, d_g, d_g ? d_g + s.ne : NULL, d_g ? d_g + s.ne + s.npd : NULL, d_ws)) return -1;
    if (nntk_shim_download(loss_rows, d_loss, (size_t)batch * sizeof(float))) return -1;
    if (!denc) return 0;
    if (nntk_shim_download(denc, d_g, (size_t)batch * T * J * sizeof(float)) ||
        nntk_shim_download(dpred, d_g + s.ne, (size_t)batch * (max_label_len + 1) * J * sizeof(float))) return -1;
    return nntk_shim_download(dout, d_g + s.ne + s.npd, ((size_t)J + 1) * V * sizeof(float));
}

/* ---- forced alignment (csrc/hip/rnnt_align.hip): the best single path, on stored scores and on the joiner's inputs.  One device
 *      body and one host body take the score source; in the host body its pointers are host memory ---- */
static int align_check(const char *who, const nntk_shim_rnnt_src *src, int batch, int T, int V, const int *input_lengths, const int *labels,
                       const int *label_lengths, int max_label_len, int blank) {
    if (!src->fused) return rnnt_check(who, batch, T, V, input_lengths, labels, label_lengths, max_label_len, blank);
    return fused_check(who, batch, T, src->J, V, src->kind, input_lengths, labels, label_lengths, max_label_len, blank, NULL, NULL, NULL);
}

/* the source's pointers, under the names of the device form (the stored scores 16-byte aligned) or of the host form */
static int align_check_src(const char *who, const nntk_shim_rnnt_src *src, int dev) {
    if (!src->fused) return rnnt_check_ptr(who, dev ? "d_logits" : "logits", src->d_logits, dev ? 16 : 4);
    return rnnt_check_ptr(who, dev ? "d_enc" : "enc", src->d_enc, 4) || rnnt_check_ptr(who, dev ? "d_pred" : "pred", src->d_pred, 4) ||
           rnnt_check_ptr(who, dev ? "d_out" : "out", src->d_out, 4);
}

static int align_check_outputs(const char *who, const nntk_shim_rnnt_path *p) {
    return rnnt_check_ptr(who, "scores", p->scores, 4) || (p->label_frames && rnnt_check_ptr(who, "label_frames", p->label_frames, 4)) ||
           (p->frame_labels && rnnt_check_ptr(who, "frame_labels", p->frame_labels, 4)) ||
           (p->label_logp && rnnt_check_ptr(who, "label_logp", p->label_logp, 4)) ||
           (p->frame_logp && rnnt_check_ptr(who, "frame_logp", p->frame_logp, 4));
}

static int align_device(const char *who, const nntk_shim_rnnt_src *src, int batch, int T, int V, const int *input_lengths, const int *labels,
                        const int *label_lengths, int max_label_len, int blank, const nntk_shim_rnnt_path *p, float *d_workspace) {
    nntk_shim_clear_error();
    if (align_check(who, src, batch, T, V, input_lengths, labels, label_lengths, max_label_len, blank)) return -1;
    if (batch == 0) return 0;
    if (align_check_src(who, src, 1) || rnnt_check_ptr(who, "d_workspace", d_workspace, 16) || align_check_outputs(who, p)) return -1;
    const size_t f = sizeof(float), nl = (size_t)batch * max_label_len * f, nt = (size_t)batch * T * f, U1 = (size_t)max_label_len + 1;
    /* outputs first; of the source's four spans those of the other source are at 0 */
    const rnnt_span sp[] = {{"d_label_frames", (uintptr_t)p->label_frames, nl}, {"d_frame_labels", (uintptr_t)p->frame_labels, nt},
                            {"d_label_logp", (uintptr_t)p->label_logp, nl}, {"d_frame_logp", (uintptr_t)p->frame_logp, nt},
                            {"d_scores", (uintptr_t)p->scores, (size_t)batch * f},
                            {"d_logits", (uintptr_t)src->d_logits, (size_t)batch * T * U1 * V * f},
                            {"d_enc", (uintptr_t)src->d_enc, (size_t)batch * T * src->J * f},
                            {"d_pred", (uintptr_t)src->d_pred, (size_t)batch * U1 * src->J * f},
                            {"d_out", (uintptr_t)src->d_out, ((size_t)src->J + 1) * V * f},
                            {"d_workspace", (uintptr_t)d_workspace,
                             nntk_shim_rnnt_align_workspace_floats(src, batch, T, V, max_label_len) * f}};
    if (rnnt_overlap(who, sp, 5, 10)) return -1;
    int *len = rnnt_lengths(input_lengths, batch, T);
    int rc = len ? nntk_shim_rnnt_align(src, batch, T, V, len, labels, label_lengths, max_label_len, blank, p, d_workspace) : -1;
    free(len);
    return rc;
}

/* who_dev: the device form's name, under which the device body speaks.  The outputs live in one device block: label_frames |
 * frame_labels | label_logp | frame_logp | scores, a part that is not asked for taking no room */
static int align_host(const char *who, const char *who_dev, const nntk_shim_rnnt_src *h, int batch, int T, int V, const int *input_lengths,
                      const int *labels, const int *label_lengths, int max_label_len, int blank, const nntk_shim_rnnt_path *p) {
    nntk_shim_clear_error();
    if (align_check(who, h, batch, T, V, input_lengths, labels, label_lengths, max_label_len, blank)) return -1;
    if (batch == 0) return 0;
    if (align_check_src(who, h, 0) || align_check_outputs(who, p)) return -1;
    const size_t nl = (size_t)batch * max_label_len, nt = (size_t)batch * T;
    const size_t fl = p->label_frames ? nl : 0, ll = fl + (p->frame_labels ? nt : 0), fp = ll + (p->label_logp ? nl : 0);
    const size_t sc = fp + (p->frame_logp ? nt : 0);
    nntk_shim_rnnt_src d = *h;
    if (h->fused) {
        fused_in s;
        if (fused_stage(&s, h->d_enc, h->d_pred, h->d_out, batch, T, max_label_len, h->J, V, 0)) return -1;
        d.d_enc = s.d_enc; d.d_pred = s.d_pred; d.d_out = s.d_out;
    } else {
        const size_t n = nt * (max_label_len + 1) * V;
        float *d_x = nntk_devbuf_reserve(&t_a, n + 4);
        if (!d_x || nntk_shim_upload(d_x, h->d_logits, n * sizeof(float))) return -1;
        d.d_logits = d_x;
    }
    float *d_o = nntk_devbuf_reserve(&t_b, sc + (size_t)batch + 4);
    float *d_ws = nntk_devbuf_reserve(&t_c, nntk_shim_rnnt_align_workspace_floats(h, batch, T, V, max_label_len));
    if (!d_o || !d_ws) return -1;
    const nntk_shim_rnnt_path dp = {.label_frames = p->label_frames ? (int *)d_o : NULL, .frame_labels = p->frame_labels ? (int *)(d_o + fl) : NULL,
                                    .label_logp = p->label_logp ? d_o + ll : NULL, .frame_logp = p->frame_logp ? d_o + fp : NULL, .scores = d_o + sc};
    if (align_device(who_dev, &d, batch, T, V, input_lengths, labels, label_lengths, max_label_len, blank, &dp, d_ws)) return -1;
    const size_t f = sizeof(float);
    if (p->label_frames && nl && nntk_shim_download(p->label_frames, dp.label_frames, nl * f)) return -1;
    if (p->frame_labels && nntk_shim_download(p->frame_labels, dp.frame_labels, nt * f)) return -1;
    if (p->label_logp && nl && nntk_shim_download(p->label_logp, dp.label_logp, nl * f)) return -1;
    if (p->frame_logp && nntk_shim_download(p->frame_logp, dp.frame_logp, nt * f)) return -1;
    return nntk_shim_download(p->scores, dp.scores, (size_t)batch * f);
}

#define ALIGN_STORED(x) (&(nntk_shim_rnnt_src){.fused = 0, .d_logits = (x)})
#define ALIGN_FUSED(e, p, o, j, k) (&(nntk_shim_rnnt_src){.fused = 1, .d_enc = (e), .d_pred = (p), .d_out = (o), .J = (j), .kind = (k)})
#define ALIGN_PATH(lf, fl, lp, fp, sc) \
    (&(nntk_shim_rnnt_path){.label_frames = (lf), .frame_labels = (fl), .label_logp = (lp), .frame_logp = (fp), .scores = (sc)})

size_t nntk_rnnt_align_workspace_floats(int batch, int T, int max_label_len) {
    return nntk_shim_rnnt_align_workspace_floats(ALIGN_STORED(NULL), batch, T, 0, max_label_len);
}

int nntk_rnnt_align_device(const float *d_logits, int batch, int T, int V, const int *input_lengths, const int *labels,
                           const int *label_lengths, int max_label_len, int blank, int *d_label_frames, int *d_frame_labels,
                           float *d_label_logp, float *d_frame_logp, float *d_scores, float *d_workspace) {
    return align_device("nntk_rnnt_align_device", ALIGN_STORED(d_logits), batch, T, V, input_lengths, labels, label_lengths, max_label_len,
                        blank, ALIGN_PATH(d_label_frames, d_frame_labels, d_label_logp, d_frame_logp, d_scores), d_workspace);
}

int nntk_rnnt_align(const float *logits, int batch, int T, int V, const int *input_lengths, const int *labels, const int *label_lengths,
                    int max_label_len, int blank, int *label_frames, int *frame_labels, float *label_logp, float *frame_logp,
                    float *scores) {
    return align_host("nntk_rnnt_align", "nntk_rnnt_align_device", ALIGN_STORED(logits), batch, T, V, input_lengths, labels, label_lengths,
                      max_label_len, blank, ALIGN_PATH(label_frames, frame_labels, label_logp, frame_logp, scores));
}

size_t nntk_rnnt_fused_align_workspace_floats(int batch, int T, int max_label_len, int J, int V) {
    return nntk_shim_rnnt_align_workspace_floats(ALIGN_FUSED(NULL, NULL, NULL, J, 0), batch, T, V, max_label_len);
}

int nntk_rnnt_fused_align_device(const float *d_enc, const float *d_pred, const float *d_out, int batch, int T, int J, int V, int activation,
                                 const int *input_lengths, const int *labels, const int *label_lengths, int max_label_len, int blank,
                                 int *d_label_frames, int *d_frame_labels, float *d_label_logp, float *d_frame_logp, float *d_scores,
                                 float *d_workspace) {
    return align_device("nntk_rnnt_fused_align_device", ALIGN_FUSED(d_enc, d_pred, d_out, J, activation), batch, T, V, input_lengths, labels,
                        label_lengths, max_label_len, blank, ALIGN_PATH(d_label_frames, d_frame_labels, d_label_logp, d_frame_logp, d_scores),
                        d_workspace);
}

int nntk_rnnt_fused_align(const float *enc, const float *pred, const float *out, int batch, int T, int J, int V, int activation,
                          const int *input_lengths, const int *labels, const int *label_lengths, int max_label_len, int blank,
                          int *label_frames, int *frame_labels, float *label_logp, float *frame_logp, float *scores) {
    return align_host("nntk_rnnt_fused_align", "nntk_rnnt_fused_align_device", ALIGN_FUSED(enc, pred, out, J, activation), batch, T, V,
                      input_lengths, labels, label_lengths, max_label_len, blank,
                      ALIGN_PATH(label_frames, frame_labels, label_logp, frame_logp, scores));
}

/* ---- the pruned training loss (csrc/hip/rnnt_pruned.hip): simple loss, prune ranges, banded joiner, banded loss.  d_ranges is device
 *      memory the host cannot check: the kernels clamp it ---- */
static int pruned_check_s(const char *who, int S, int U1) {
    if (S < 1 || S > U1) return rnnt_fail(who, "S %d is outside [1, %d]", S, U1, 0);
    return 0;
}

/* S, and every row's band: (T_b - 1)(S - 1) >= U_b + 1 - S, or no connected band runs from (0, 0) to (T_b - 1, U_b) */
static int prune_check(const char *who, int batch, int T, const int *input_lengths, const int *label_lengths, int max_label_len, int S) {
    if (batch < 0 || T < 0 || max_label_len < 0)
        return rnnt_fail(who, "batch %d, T %d, max_label_len %d: none may be negative", batch, T, max_label_len);
    if (max_label_len > NNTK_RNNT_MAX_LABELS)
        return rnnt_fail(who, "max_label_len %d is beyond what one workgroup's LDS holds (%d)", max_label_len, NNTK_RNNT_MAX_LABELS, 0);
    if ((long long)T + max_label_len > NNTK_RNNT_MAX_DIAGONALS)
        return rnnt_fail(who, "T + max_label_len = %d is more than %d lattice diagonals", T + max_label_len, NNTK_RNNT_MAX_DIAGONALS, 0);
    if (pruned_check_s(who, S, max_label_len + 1)) return -1;
    if (batch > 0 && !label_lengths) return rnnt_fail(who, "NULL label_lengths", 0, 0, 0);
    if (batch > 0 && T < 1) return rnnt_fail(who, "T %d < 1", T, 0, 0);
    for (int b = 0; b < batch; ++b) {
        const int Tb = input_lengths ? input_lengths[b] : T, Ub = label_lengths[b];
        if (Tb < 1 || Tb > T) return rnnt_fail(who, "input_lengths[%d] = %d is outside [1, %d]", b, Tb, T);
        if (Ub < 0 || Ub > max_label_len) return rnnt_fail(who, "label_lengths[%d] = %d is outside [0, %d]", b, Ub, max_label_len);
        if ((long long)(Tb - 1) * (S - 1) < (long long)Ub + 1 - S)
            return rnnt_fail(who, "row %d: %d frames cannot carry a connected band of %d positions across its labels (infeasible)", b, Tb, S);
    }
    return 0;
}

size_t nntk_rnnt_simple_workspace_floats(int batch, int T, int max_label_len, int want_grad) {
    return nntk_shim_rnnt_simple_workspace_floats(batch, T, max_label_len, want_grad != 0);
}

static int simple_check(const char *who, int batch, int T, int V, const int *input_lengths, const int *labels, const int *label_lengths,
                        int max_label_len, int blank, const void *dam, const void *dlm) {
    if (rnnt_check(who, batch, T, V, input_lengths, labels, label_lengths, max_label_len, blank)) return -1;
    const int given = (dam != NULL) + (dlm != NULL);
    if (given == 1) return rnnt_fail(who, "the gradient outputs d_dam, d_dlm are all NULL or all given (%d of 2 are)", given, 0, 0);
    return 0;
}

int nntk_rnnt_simple_loss_device(const float *d_am, const float *d_lm, int batch, int T, int V, const int *input_lengths, const int *labels,
                                 const int *label_lengths, int max_label_len, int blank, float *d_loss_rows, float *d_dam, float *d_dlm,
                                 float *d_occ, float *d_workspace) {
    static const char who[] = "nntk_rnnt_simple_loss_device";
    nntk_shim_clear_error();
    if (simple_check(who, batch, T, V, input_lengths, labels, label_lengths, max_label_len, blank, d_dam, d_dlm)) return -1;
    if (batch == 0) return 0;
    if (rnnt_check_ptr(who, "d_am", d_am, 16) || rnnt_check_ptr(who, "d_lm", d_lm, 16) || rnnt_check_ptr(who, "d_loss_rows", d_loss_rows, 4) ||
        rnnt_check_ptr(who, "d_workspace", d_workspace, 16) ||
        (d_dam && (rnnt_check_ptr(who, "d_dam", d_dam, 4) || rnnt_check_ptr(who, "d_dlm", d_dlm, 4))) ||
        (d_occ && rnnt_check_ptr(who, "d_occ", d_occ, 4))) return -1;
    const size_t U1 = (size_t)max_label_len + 1, f = sizeof(float), na = (size_t)batch * T * V * f, nl = (size_t)batch * U1 * V * f;
    /* outputs first */
    const rnnt_span sp[] = {{"d_loss_rows", (uintptr_t)d_loss_rows, (size_t)batch * f}, {"d_dam", (uintptr_t)d_dam, na}, {"d_dlm", (uintptr_t)d_dlm, nl},
                            {"d_occ", (uintptr_t)d_occ, (size_t)batch * T * U1 * f}, {"d_am", (uintptr_t)d_am, na}, {"d_lm", (uintptr_t)d_lm, nl},
                            {"d_workspace", (uintptr_t)d_workspace,
                             nntk_shim_rnnt_simple_workspace_floats(batch, T, max_label_len, d_dam != NULL || d_occ != NULL) * f}};
    if (rnnt_overlap(who, sp, 4, 7)) return -1;
    int *len = rnnt_lengths(input_lengths, batch, T);
    int rc = len ? nntk_shim_rnnt_simple_loss(d_am, d_lm, batch, T, V, len, labels, label_lengths, max_label_len, blank, d_loss_rows, d_dam,
                                              d_dlm, d_occ, d_workspace) : -1;
    free(len);
    return rc;
}

int nntk_rnnt_simple_loss(const float *am, const float *lm, int batch, int T, int V, const int *input_lengths, const int *labels,
                          const int *label_lengths, int max_label_len, int blank, float *loss_rows, float *dam, float *dlm, float *occ) {
    static const char who[] = "nntk_rnnt_simple_loss";
    nntk_shim_clear_error();
    if (simple_check(who, batch, T, V, input_lengths, labels, label_lengths, max_label_len, blank, dam, dlm)) return -1;
    if (batch == 0) return 0;
    if (rnnt_check_ptr(who, "am", am, 4) || rnnt_check_ptr(who, "lm", lm, 4) || rnnt_check_ptr(who, "loss_rows", loss_rows, 4) ||
        (dam && (rnnt_check_ptr(who, "dam", dam, 4) || rnnt_check_ptr(who, "dlm", dlm, 4))) || (occ && rnnt_check_ptr(who, "occ", occ, 4)))
        return -1;
    /* am | lm | loss rows in one block, dam | dlm | occ in a second (each part rounded up to 16 bytes), the workspace in a third */
    const size_t up = 3, U1 = (size_t)max_label_len + 1, ra = (size_t)batch * T * V, rl = (size_t)batch * U1 * V, ro = (size_t)batch * T * U1;
    const size_t na = (ra + up) & ~up, nl = (rl + up) & ~up, no = (ro + up) & ~up;
    float *d_in = nntk_devbuf_reserve(&t_a, na + nl + (size_t)batch + 4);
    float *d_g = (dam || occ) ? nntk_devbuf_reserve(&t_b, na + nl + no + 4) : NULL;
    float *d_ws = nntk_devbuf_reserve(&t_c, nntk_shim_rnnt_simple_workspace_floats(batch, T, max_label_len, dam != NULL || occ != NULL));
    if (!d_in || ((dam || occ) && !d_g) || !d_ws) return -1;
    float *d_loss = d_in + na + nl;
    if (nntk_shim_upload(d_in, am, ra * sizeof(float)) || nntk_shim_upload(d_in + na, lm, rl * sizeof(float))) return -1;
    if (nntk_rnnt_simple_loss_device(d_in, d_in + na, batch, T, V, input_lengths, labels, label_lengths, max_label_len, blank, d_loss,
                                     dam ? d_g : NULL, dam ? d_g + na : NULL, occ ? d_g + na + nl : NULL, d_ws)) return -1;
    if (nntk_shim_download(loss_rows, d_loss, (size_t)batch * sizeof(float))) return -1;
    if (dam && (nntk_shim_download(dam, d_g, ra * sizeof(float)) || nntk_shim_download(dlm, d_g + na, rl * sizeof(float)))) return -1;
    return occ ? nntk_shim_download(occ, d_g + na + nl, ro * sizeof(float)) : 0;
}

size_t nntk_rnnt_prune_workspace_floats(int batch) { return nntk_shim_rnnt_prune_workspace_floats(batch); }

int nntk_rnnt_prune_ranges_device(const float *d_occ, int batch, int T, const int *input_lengths, const int *label_lengths,
                                  int max_label_len, int S, int *d_ranges, float *d_workspace) {
    static const char who[] = "nntk_rnnt_prune_ranges_device";
    nntk_shim_clear_error();
    if (prune_check(who, batch, T, input_lengths, label_lengths, max_label_len, S)) return -1;
    if (batch == 0) return 0;
    if (rnnt_check_ptr(who, "d_occ", d_occ, 4) || rnnt_check_ptr(who, "d_ranges", d_ranges, 4) ||
        rnnt_check_ptr(who, "d_workspace", d_workspace, 4)) return -1;
    const size_t f = sizeof(float);
    const rnnt_span sp[] = {{"d_ranges", (uintptr_t)d_ranges, (size_t)batch * T * f},
                            {"d_occ", (uintptr_t)d_occ, (size_t)batch * T * ((size_t)max_label_len + 1) * f},
                            {"d_workspace", (uintptr_t)d_workspace, nntk_shim_rnnt_prune_workspace_floats(batch) * f}};
    if (rnnt_overlap(who, sp, 1, 3)) return -1;
    int *len = rnnt_lengths(input_lengths, batch, T);
    int rc = len ? nntk_shim_rnnt_prune_ranges(d_occ, batch, T, max_label_len + 1, len, label_lengths, S, d_ranges, d_workspace) : -1;
    free(len);
    return rc;
}

int nntk_rnnt_prune_ranges(const float *occ, int batch, int T, const int *input_lengths, const int *label_lengths, int max_label_len, int S,
                           int *ranges) {
    static const char who[] = "nntk_rnnt_prune_ranges";
    nntk_shim_clear_error();
    if (prune_check(who, batch, T, input_lengths, label_lengths, max_label_len, S)) return -1;
    if (batch == 0) return 0;
    if (rnnt_check_ptr(who, "occ", occ, 4) || rnnt_check_ptr(who, "ranges", ranges, 4)) return -1;
    const size_t n = (size_t)batch * T * ((size_t)max_label_len + 1), nu = (n + 3) & ~(size_t)3;
    float *d_occ = nntk_devbuf_reserve(&t_a, nu + (size_t)batch * T + 4);
    float *d_ws = nntk_devbuf_reserve(&t_c, nntk_shim_rnnt_prune_workspace_floats(batch));
    if (!d_occ || !d_ws || nntk_shim_upload(d_occ, occ, n * sizeof(float))) return -1;
    if (nntk_rnnt_prune_ranges_device(d_occ, batch, T, input_lengths, label_lengths, max_label_len, S, (int *)(d_occ + nu), d_ws)) return -1;
    return nntk_shim_download(ranges, d_occ + nu, (size_t)batch * T * sizeof(int));
}

static int pruned_joint_check(const char *who, int batch, int T, int U1, int S, int J, int activation) {
    if (joint_check(who, batch, T, U1, J, activation)) return -1;
    return (size_t)batch * T * U1 * J == 0 ? 0 : pruned_check_s(who, S, U1);      /* an empty tensor is not an error */
}

int nntk_rnnt_pruned_joint_device(const float *d_enc, const float *d_pred, const int *d_ranges, int batch, int T, int U1, int S, int J,
                                  int activation, float *d_out) {
    static const char who[] = "nntk_rnnt_pruned_joint_device";
    nntk_shim_clear_error();
    if (pruned_joint_check(who, batch, T, U1, S, J, activation)) return -1;
    if ((size_t)batch * T * U1 * J == 0) return 0;
    if (rnnt_check_ptr(who, "d_enc", d_enc, 4) || rnnt_check_ptr(who, "d_pred", d_pred, 4) || rnnt_check_ptr(who, "d_ranges", d_ranges, 4) ||
        rnnt_check_ptr(who, "d_out", d_out, 4)) return -1;
    const size_t f = sizeof(float);
    const rnnt_span sp[] = {{"d_out", (uintptr_t)d_out, (size_t)batch * T * S * J * f}, {"d_enc", (uintptr_t)d_enc, (size_t)batch * T * J * f},
                            {"d_pred", (uintptr_t)d_pred, (size_t)batch * U1 * J * f}, {"d_ranges", (uintptr_t)d_ranges, (size_t)batch * T * f}};
    if (rnnt_overlap(who, sp, 1, 4)) return -1;
    return nntk_shim_rnnt_pruned_joint(d_enc, d_pred, d_ranges, batch, T, U1, S, J, activation, d_out);
}

int nntk_rnnt_pruned_joint_backward_device(const float *d_out_fwd, const float *d_dout, const int *d_ranges, int batch, int T, int U1, int S,
                                           int J, int activation, float *d_denc, float *d_dpred) {
    static const char who[] = "nntk_rnnt_pruned_joint_backward_device";
    nntk_shim_clear_error();
    if (pruned_joint_check(who, batch, T, U1, S, J, activation)) return -1;
    if ((size_t)batch * T * U1 * J == 0) return 0;
    if ((activation != 0 && rnnt_check_ptr(who, "d_out_fwd", d_out_fwd, 4)) || rnnt_check_ptr(who, "d_dout", d_dout, 4) ||
        rnnt_check_ptr(who, "d_ranges", d_ranges, 4) || rnnt_check_ptr(who, "d_denc", d_denc, 4) || rnnt_check_ptr(who, "d_dpred", d_dpred, 4))
        return -1;
    const size_t f = sizeof(float), band = (size_t)batch * T * S * J * f;
    const rnnt_span sp[] = {{"d_denc", (uintptr_t)d_denc, (size_t)batch * T * J * f}, {"d_dpred", (uintptr_t)d_dpred, (size_t)batch * U1 * J * f},
                            {"d_out_fwd", (uintptr_t)(activation ? d_out_fwd : NULL), band}, {"d_dout", (uintptr_t)d_dout, band},
                            {"d_ranges", (uintptr_t)d_ranges, (size_t)batch * T * f}};
    if (rnnt_overlap(who, sp, 2, 5)) return -1;
    return nntk_shim_rnnt_pruned_joint_backward(d_out_fwd, d_dout, d_ranges, batch, T, U1, S, J, activation, d_denc, d_dpred);
}

size_t nntk_rnnt_pruned_workspace_floats(int batch, int T, int max_label_len, int want_grad) {
    return nntk_shim_rnnt_workspace_floats(batch, T, max_label_len, want_grad != 0);
}

int nntk_rnnt_pruned_loss_device(const float *d_logits, const int *d_ranges, int batch, int T, int S, int V, const int *input_lengths,
                                 const int *labels, const int *label_lengths, int max_label_len, int blank, float *d_loss_rows,
                                 float *d_dlogits, float *d_workspace) {
    static const char who[] = "nntk_rnnt_pruned_loss_device";
    nntk_shim_clear_error();
    if (rnnt_check(who, batch, T, V, input_lengths, labels, label_lengths, max_label_len, blank) ||
        pruned_check_s(who, S, max_label_len + 1)) return -1;
    if (batch == 0) return 0;
    if (rnnt_check_ptr(who, "d_logits", d_logits, 16) || rnnt_check_ptr(who, "d_ranges", d_ranges, 4) ||
        rnnt_check_ptr(who, "d_loss_rows", d_loss_rows, 4) || rnnt_check_ptr(who, "d_workspace", d_workspace, 16) ||
        (d_dlogits && rnnt_check_ptr(who, "d_dlogits", d_dlogits, 16))) return -1;
    const size_t f = sizeof(float), bytes = (size_t)batch * T * S * V * f;
    const rnnt_span sp[] = {{"d_dlogits", (uintptr_t)d_dlogits, bytes}, {"d_loss_rows", (uintptr_t)d_loss_rows, (size_t)batch * f},
                            {"d_logits", (uintptr_t)d_logits, bytes}, {"d_ranges", (uintptr_t)d_ranges, (size_t)batch * T * f},
                            {"d_workspace", (uintptr_t)d_workspace,
                             nntk_shim_rnnt_workspace_floats(batch, T, max_label_len, d_dlogits != NULL) * f}};
    if (rnnt_overlap(who, sp, 2, 5)) return -1;
    int *len = rnnt_lengths(input_lengths, batch, T);
    int rc = len ? nntk_shim_rnnt_pruned_loss(d_logits, d_ranges, batch, T, S, V, len, labels, label_lengths, max_label_len, blank, d_loss_rows,
                                              d_dlogits, d_workspace) : -1;
    free(len);
    return rc;
}

int nntk_rnnt_pruned_loss(const float *logits, const int *ranges, int batch, int T, int S, int V, const int *input_lengths, const int *labels,
                          const int *label_lengths, int max_label_len, int blank, float *loss_rows, float *dlogits) {
    static const char who[] = "nntk_rnnt_pruned_loss";
    nntk_shim_clear_error();
    if (rnnt_check(who, batch, T, V, input_lengths, labels, label_lengths, max_label_len, blank) ||
        pruned_check_s(who, S, max_label_len + 1)) return -1;
    if (batch == 0) return 0;
    if (rnnt_check_ptr(who, "logits", logits, 4) || rnnt_check_ptr(who, "ranges", ranges, 4) || rnnt_check_ptr(who, "loss_rows", loss_rows, 4) ||
        (dlogits && rnnt_check_ptr(who, "dlogits", dlogits, 4))) return -1;
    /* logits | ranges | loss rows in one block (each part rounded up to 16 bytes), the gradient in a second, the workspace in a third */
    const size_t up = 3, n = (size_t)batch * T * S * V, nu = (n + up) & ~up, nr = ((size_t)batch * T + up) & ~up;
    float *d_x = nntk_devbuf_reserve(&t_a, nu + nr + (size_t)batch + 4);
    float *d_g = dlogits ? nntk_devbuf_reserve(&t_b, n + 4) : NULL;
    float *d_ws = nntk_devbuf_reserve(&t_c, nntk_shim_rnnt_workspace_floats(batch, T, max_label_len, dlogits != NULL));
    if (!d_x || (dlogits && !d_g) || !d_ws) return -1;
    float *d_loss = d_x + nu + nr;
    if (nntk_shim_upload(d_x, logits, n * sizeof(float)) || nntk_shim_upload(d_x + nu, ranges, (size_t)batch * T * sizeof(int))) return -1;
    if (nntk_rnnt_pruned_loss_device(d_x, (const int *)(d_x + nu), batch, T, S, V, input_lengths, labels, label_lengths, max_label_len, blank,
                                     d_loss, d_g, d_ws)) return -1;
    if (nntk_shim_download(loss_rows, d_loss, (size_t)batch * sizeof(float))) return -1;
    return dlogits ? nntk_shim_download(dlogits, d_g, n * sizeof(float)) : 0;
}
