/*
 * ctc.c -- host layer of the CTC calls: loss and gradient, best-path decoding (csrc/hip/ctc.hip), prefix beam search on acoustic scores
 * alone or fused with an n-gram model (ngram_lm.c), in one shot or pushed chunk by chunk (csrc/hip/ctc_beam.hip), and forced alignment
 * (csrc/hip/ctc_align.hip).  Every host array is checked here, before anything is enqueued or allocated.  Each call has a
 * device-pointer form and a host-pointer form (upload, device call, download).
 */
#include <stdio.h>
#include <stdint.h>
#include <stdlib.h>
#include "nntk_internal.h"

/* scratch for the host-pointer forms: per thread and device, freed at thread exit (nntk_thread_scratch, runtime.c) */
#define t_a (*nntk_thread_scratch(NNTK_TS_A))
#define t_b (*nntk_thread_scratch(NNTK_TS_B))
#define t_c (*nntk_thread_scratch(NNTK_TS_C))

static int ctc_fail(const char *who, const char *fmt, int a, int b, int c) {
    char msg[200];
    int n = snprintf(msg, sizeof msg, "%s: ", who);
    snprintf(msg + n, sizeof msg - (size_t)n, fmt, a, b, c);
    nntk_set_error(msg);
    return -1;
}
static int ctc_check_shape(const char *who, int batch, int T, int C, int blank) {
    if (batch < 0 || T < 0 || C <= 0) return ctc_fail(who, "batch %d, T %d, C %d: batch and T must be >= 0, C > 0", batch, T, C);
    if (blank < 0 || blank >= C) return ctc_fail(who, "blank %d is outside [0, %d)", blank, C, 0);
    return 0;
}
static int ctc_check_labels(const char *who, int batch, int C, const int *labels, const int *label_lengths, int max_label_len, int blank) {
    if (max_label_len < 0) return ctc_fail(who, "max_label_len %d < 0", max_label_len, 0, 0);
    if (batch > 0 && (!label_lengths || (max_label_len > 0 && !labels))) NNTK_FAIL("nntk_ctc_loss: NULL labels / label_lengths");
    for (int b = 0; b < batch; ++b) {
        const int L = label_lengths[b];
        if (L < 0 || L > max_label_len) return ctc_fail(who, "label_lengths[%d] = %d is outside [0, %d]", b, L, max_label_len);
        for (int i = 0; i < L; ++i) {
            const int k = labels[(size_t)b * max_label_len + i];
            if (k < 0 || k >= C) return ctc_fail(who, "labels[%d][%d] = %d is not a class", b, i, k);
            if (k == blank) return ctc_fail(who, "labels[%d][%d] is the blank (%d)", b, i, k);
        }
    }
    return 0;
}
/* the input lengths the kernels read: the caller's, or T for every row; NULL = out of host memory */
static int *ctc_lengths(const int *input_lengths, int batch, int T) {
    int *len = (int *)malloc((size_t)(batch > 0 ? batch : 1) * sizeof(int));
    if (!len) { nntk_set_error("out of host memory"); return NULL; }
    for (int b = 0; b < batch; ++b) len[b] = input_lengths ? input_lengths[b] : T;
    return len;
}

/* ---- loss, gradient and best-path decoding (csrc/hip/ctc.hip) ---- */
size_t nntk_ctc_workspace_floats(int batch, int T, int max_label_len) {
    return nntk_shim_ctc_workspace_floats(batch, T, max_label_len);
}

int nntk_ctc_loss_device(const float *d_probs, int batch, int T, int C, const int *input_lengths, const int *labels,
                         const int *label_lengths, int max_label_len, int blank, float *d_loss_rows, float *d_dprobs,
                         float *d_workspace) {
    static const char who[] = "nntk_ctc_loss_device";
    nntk_shim_clear_error();
    if (ctc_check_shape(who, batch, T, C, blank) || nntk_check_lengths(who, input_lengths, batch, T, NULL, NULL) ||
        ctc_check_labels(who, batch, C, labels, label_lengths, max_label_len, blank)) return -1;
    if (batch == 0) return 0;
    if (!d_loss_rows || !d_workspace || (!d_probs && T > 0)) NNTK_FAIL("nntk_ctc_loss_device: NULL tensor");
    int *len = ctc_lengths(input_lengths, batch, T);
    if (!len) return -1;
    int rc = nntk_shim_ctc_loss(d_probs, batch, T, C, len, labels, label_lengths, max_label_len, blank, d_loss_rows, d_dprobs, d_workspace);
    free(len);
    return rc;
}

int nntk_ctc_greedy_decode_device(const float *d_probs, int batch, int T, int C, const int *input_lengths, int blank,
                                  int *d_labels_out, int *d_out_lengths) {
    static const char who[] = "nntk_ctc_greedy_decode_device";
    nntk_shim_clear_error();
    if (ctc_check_shape(who, batch, T, C, blank) || nntk_check_lengths(who, input_lengths, batch, T, NULL, NULL)) return -1;
    if (batch == 0) return 0;
    if (!d_out_lengths || ((!d_probs || !d_labels_out) && T > 0)) NNTK_FAIL("nntk_ctc_greedy_decode_device: NULL tensor");
    int *len = ctc_lengths(input_lengths, batch, T);
    if (!len) return -1;
    int rc = nntk_shim_ctc_greedy_decode(d_probs, batch, T, C, len, blank, d_labels_out, d_out_lengths);
    free(len);
    return rc;
}

int nntk_ctc_loss(const float *probs, int batch, int T, int C, const int *input_lengths, const int *labels, const int *label_lengths,
                  int max_label_len, int blank, float *loss_rows, float *dprobs) {
    static const char who[] = "nntk_ctc_loss";
    nntk_shim_clear_error();
    if (ctc_check_shape(who, batch, T, C, blank) || nntk_check_lengths(who, input_lengths, batch, T, NULL, NULL) ||
        ctc_check_labels(who, batch, C, labels, label_lengths, max_label_len, blank)) return -1;
    if (batch == 0) return 0;
    if (!loss_rows || (!probs && T > 0)) NNTK_FAIL("nntk_ctc_loss: NULL array");
    const size_t n = (size_t)batch * T * C;
    float *d_p = nntk_devbuf_reserve(&t_a, n + (size_t)batch + 4);
    float *d_g = dprobs ? nntk_devbuf_reserve(&t_b, n + 4) : NULL;
    float *d_ws = nntk_devbuf_reserve(&t_c, nntk_shim_ctc_workspace_floats(batch, dprobs ? T : 0, max_label_len));
    if (!d_p || (dprobs && !d_g) || !d_ws) return -1;
    float *d_loss = d_p + n;
    if (n && nntk_shim_upload(d_p, probs, n * sizeof(float))) return -1;
    if (nntk_ctc_loss_device(d_p, batch, T, C, input_lengths, labels, label_lengths, max_label_len, blank, d_loss, d_g, d_ws)) return -1;
    if (nntk_shim_download(loss_rows, d_loss, (size_t)batch * sizeof(float))) return -1;
    return dprobs && n ? nntk_shim_download(dprobs, d_g, n * sizeof(float)) : 0;
}

int nntk_ctc_greedy_decode(const float *probs, int batch, int T, int C, const int *input_lengths, int blank, int *labels_out,
                           int *out_lengths) {
    static const char who[] = "nntk_ctc_greedy_decode";
    nntk_shim_clear_error();
    if (ctc_check_shape(who, batch, T, C, blank) || nntk_check_lengths(who, input_lengths, batch, T, NULL, NULL)) return -1;
    if (batch == 0) return 0;
    if (!out_lengths || ((!probs || !labels_out) && T > 0)) NNTK_FAIL("nntk_ctc_greedy_decode: NULL array");
    const size_t n = (size_t)batch * T * C, nl = (size_t)batch * T;
    float *d_p = nntk_devbuf_reserve(&t_a, n + 4);
    int *d_o = (int *)nntk_devbuf_reserve(&t_b, nl + (size_t)batch + 4);
    if (!d_p || !d_o) return -1;
    if (n && nntk_shim_upload(d_p, probs, n * sizeof(float))) return -1;
    if (nntk_ctc_greedy_decode_device(d_p, batch, T, C, input_lengths, blank, d_o, d_o + nl)) return -1;
    if (nl && nntk_shim_download(labels_out, d_o, nl * sizeof(int))) return -1;
    return nntk_shim_download(out_lengths, d_o + nl, (size_t)batch * sizeof(int));
}

/* ---- prefix beam search (csrc/hip/ctc_beam.hip), with an n-gram handle (ngram_lm.c; INTEGRATION.md "CTC prefix beam search",
 *      Language-model fusion) or, lm NULL, on acoustic scores alone ---- */
static int ctc_beam_check(const char *who, int batch, int T, int C, const int *input_lengths, int blank, int beam_width,
                          int cutoff_top_n, int nbest) {
    if (ctc_check_shape(who, batch, T, C, blank) || nntk_check_lengths(who, input_lengths, batch, T, NULL, NULL)) return -1;
    if (beam_width < 1 || beam_width > NNTK_CTC_BEAM_MAX_W)
        return ctc_fail(who, "beam_width %d is outside [1, %d]", beam_width, NNTK_CTC_BEAM_MAX_W, 0);
    if (nbest < 1 || nbest > beam_width) return ctc_fail(who, "nbest %d is outside [1, beam_width = %d]", nbest, beam_width, 0);
    if (cutoff_top_n < 0) return ctc_fail(who, "cutoff_top_n %d < 0", cutoff_top_n, 0, 0);
    const int n = cutoff_top_n == 0 || cutoff_top_n >= C - 1 ? C - 1 : cutoff_top_n;      /* expanded classes per frame */
    if ((long long)beam_width * (n + 1) > NNTK_CTC_BEAM_MAX_CELLS)
        return ctc_fail(who, "beam_width %d x (%d expanded classes + 1) is more than %d candidate cells: lower beam_width or set cutoff_top_n",
                        beam_width, n, NNTK_CTC_BEAM_MAX_CELLS);
    if (T > NNTK_CTC_BEAM_MAX_T) return ctc_fail(who, "T %d is not below %d frames", T, NNTK_CTC_BEAM_MAX_T + 1, 0);
    return 0;
}
static int ctc_beam_lm_check(const char *who, NntkNgramLm lm, int C, int blank) {
    if (lm && !nntk_ngram_lm_matches(lm, C, blank))
        return ctc_fail(who, "the language model was built for another class count or blank than C = %d, blank = %d", C, blank, 0);
    return 0;
}

/* the detail outputs (label frames / log-probabilities, nl elements each; INTEGRATION.md "Label timestamps and confidences") of a device
 * call: 4-byte aligned, and apart from each other, from the other outputs and from what the kernels read while they write them */
typedef struct { const void *p; size_t bytes; const char *name; } beam_span;
static int beam_detail_check(const char *who, const int *d_frames, const float *d_logps, size_t nl, const beam_span *other, int n_other) {
    const beam_span det[2] = { { d_frames, nl * sizeof(int), "d_label_frames" }, { d_logps, nl * sizeof(float), "d_label_logps" } };
    char msg[200];
    for (int i = 0; i < 2; ++i) {
        if (!det[i].p) continue;
        if ((uintptr_t)det[i].p & 3) {
            snprintf(msg, sizeof msg, "%s: %s is not 4-byte aligned", who, det[i].name);
            nntk_set_error(msg);
            return -1;
        }
        for (int k = i + 1; k < 2 + n_other; ++k) {
            const beam_span *q = k < 2 ? &det[k] : &other[k - 2];
            const char *a = (const char *)det[i].p, *b = (const char *)q->p;
            if (b && det[i].bytes && q->bytes && a < b + q->bytes && b < a + det[i].bytes) {
                snprintf(msg, sizeof msg, "%s: %s overlaps %s", who, det[i].name, q->name);
                nntk_set_error(msg);
                return -1;
            }
        }
    }
    return 0;
}

size_t nntk_ctc_beam_workspace_floats(int batch, int T, int C, int beam_width, int cutoff_top_n) {
    return nntk_shim_ctc_beam_workspace_floats(batch, T, C, beam_width, cutoff_top_n, 0);
}
size_t nntk_ctc_beam_lm_workspace_floats(int batch, int T, int C, int beam_width, int cutoff_top_n) {
    return nntk_shim_ctc_beam_workspace_floats(batch, T, C, beam_width, cutoff_top_n, 1);
}
/* the detail outputs are written by the backtrack from what the search keeps anyway: no words of their own */
size_t nntk_ctc_beam_opt_workspace_floats(int batch, int T, int C, int beam_width, int cutoff_top_n, const NntkCtcBeamOptions *o) {
    return nntk_shim_ctc_beam_workspace_floats(batch, T, C, beam_width, cutoff_top_n, o && o->lm);
}

/* the device-pointer search under the name of the entry that was called */
static int beam_decode_device(const char *who, const float *d_probs, int batch, int T, int C, const int *input_lengths, int blank,
                              int beam_width, int cutoff_top_n, int nbest, NntkNgramLm lm, int *d_labels_out, int *d_out_lengths,
                              float *d_scores, int *d_label_frames, float *d_label_logps, float *d_workspace) {
    nntk_shim_clear_error();
    if (ctc_beam_check(who, batch, T, C, input_lengths, blank, beam_width, cutoff_top_n, nbest) || ctc_beam_lm_check(who, lm, C, blank))
        return -1;
    if (batch == 0) return 0;
    if (!d_out_lengths || !d_scores || !d_workspace || ((!d_probs || !d_labels_out) && T > 0)) return ctc_fail(who, "NULL tensor", 0, 0, 0);
    if (d_label_frames || d_label_logps) {
        const size_t nh = (size_t)batch * nbest, nl = nh * T;
        const beam_span other[5] = {
            { d_labels_out, nl * sizeof(int), "d_labels_out" }, { d_out_lengths, nh * sizeof(int), "d_out_lengths" },
            { d_scores, nh * sizeof(float), "d_scores" }, { d_probs, (size_t)batch * T * C * sizeof(float), "d_probs" },
            { d_workspace, sizeof(float) * nntk_shim_ctc_beam_workspace_floats(batch, T, C, beam_width, cutoff_top_n, lm != NULL),
              "d_workspace" } };
        if (beam_detail_check(who, d_label_frames, d_label_logps, nl, other, 5)) return -1;
    }
    nntk_shim_lm tab;
    if (lm && nntk_ngram_lm_device(lm, &tab)) return -1;
    int *len = ctc_lengths(input_lengths, batch, T);
    if (!len) return -1;
    int rc = nntk_shim_ctc_beam_decode(d_probs, batch, T, C, len, blank, beam_width, cutoff_top_n, nbest, lm ? &tab : NULL, d_labels_out,
                                       d_out_lengths, d_scores, d_label_frames, d_label_logps, d_workspace);
    free(len);
    return rc;
}

int nntk_ctc_beam_decode_device(const float *d_probs, int batch, int T, int C, const int *input_lengths, int blank, int beam_width,
                                int cutoff_top_n, int nbest, int *d_labels_out, int *d_out_lengths, float *d_scores,
                                float *d_workspace) {
    return beam_decode_device("nntk_ctc_beam_decode_device", d_probs, batch, T, C, input_lengths, blank, beam_width, cutoff_top_n, nbest,
                              NULL, d_labels_out, d_out_lengths, d_scores, NULL, NULL, d_workspace);
}
/* lm NULL: the call above itself, under its name */
int nntk_ctc_beam_decode_lm_device(const float *d_probs, int batch, int T, int C, const int *input_lengths, int blank, int beam_width,
                                   int cutoff_top_n, int nbest, NntkNgramLm lm, int *d_labels_out, int *d_out_lengths, float *d_scores,
                                   float *d_workspace) {
    return beam_decode_device(lm ? "nntk_ctc_beam_decode_lm_device" : "nntk_ctc_beam_decode_device", d_probs, batch, T, C, input_lengths,
                              blank, beam_width, cutoff_top_n, nbest, lm, d_labels_out, d_out_lengths, d_scores, NULL, NULL, d_workspace);
}
/* o NULL or all off: nntk_ctc_beam_decode_device itself; lm alone: the _lm_ call itself -- under their names */
int nntk_ctc_beam_decode_opt_device(const float *d_probs, int batch, int T, int C, const int *input_lengths, int blank, int beam_width,
                                    int cutoff_top_n, int nbest, const NntkCtcBeamOptions *o, int *d_labels_out, int *d_out_lengths,
                                    float *d_scores, float *d_workspace) {
    const char *who = o && (o->label_frames || o->label_logps) ? "nntk_ctc_beam_decode_opt_device"
                      : o && o->lm ? "nntk_ctc_beam_decode_lm_device" : "nntk_ctc_beam_decode_device";
    return beam_decode_device(who, d_probs, batch, T, C, input_lengths, blank, beam_width, cutoff_top_n, nbest, o ? o->lm : NULL,
                              d_labels_out, d_out_lengths, d_scores, o ? o->label_frames : NULL, o ? o->label_logps : NULL, d_workspace);
}

/* the results of a host-pointer search or push, packed at d_o: labels [nl] | lengths [nh] | scores [nh] | label frames [nl] |
 * label log-probabilities [nl]; the last two only where the caller asked (either may be NULL) */
static int beam_download(const int *d_o, size_t nl, size_t nh, int *labels_out, int *out_lengths, float *scores, int *label_frames,
                         float *label_logps) {
    if (nl && nntk_shim_download(labels_out, d_o, nl * sizeof(int))) return -1;
    if (nntk_shim_download(out_lengths, d_o + nl, nh * sizeof(int))) return -1;
    if (nntk_shim_download(scores, d_o + nl + nh, nh * sizeof(float))) return -1;
    if (nl && label_frames && nntk_shim_download(label_frames, d_o + nl + 2 * nh, nl * sizeof(int))) return -1;
    if (nl && label_logps && nntk_shim_download(label_logps, d_o + 2 * nl + 2 * nh, nl * sizeof(float))) return -1;
    return 0;
}

static int beam_decode_host(const char *who, const float *probs, int batch, int T, int C, const int *input_lengths, int blank,
                            int beam_width, int cutoff_top_n, int nbest, NntkNgramLm lm, int *labels_out, int *out_lengths,
                            float *scores, int *label_frames, float *label_logps) {
    nntk_shim_clear_error();
    if (ctc_beam_check(who, batch, T, C, input_lengths, blank, beam_width, cutoff_top_n, nbest) || ctc_beam_lm_check(who, lm, C, blank))
        return -1;
    if (batch == 0) return 0;
    if (!out_lengths || !scores || ((!probs || !labels_out) && T > 0)) return ctc_fail(who, "NULL array", 0, 0, 0);
    const size_t n = (size_t)batch * T * C, nh = (size_t)batch * nbest, nl = nh * T;
    float *d_p = nntk_devbuf_reserve(&t_a, n + 4);
    const int detail = label_frames || label_logps;
    int *d_o = (int *)nntk_devbuf_reserve(&t_b, nl + 2 * nh + (detail ? 2 * nl : 0) + 4);   /* beam_download's packing */
    float *d_ws = nntk_devbuf_reserve(&t_c, nntk_shim_ctc_beam_workspace_floats(batch, T, C, beam_width, cutoff_top_n, lm != NULL));
    if (!d_p || !d_o || !d_ws) return -1;
    if (n && nntk_shim_upload(d_p, probs, n * sizeof(float))) return -1;
    const NntkCtcBeamOptions dev = { lm, label_frames ? d_o + nl + 2 * nh : NULL, label_logps ? (float *)(d_o + 2 * nl + 2 * nh) : NULL };
    if (nntk_ctc_beam_decode_opt_device(d_p, batch, T, C, input_lengths, blank, beam_width, cutoff_top_n, nbest, &dev, d_o, d_o + nl,
                                        (float *)(d_o + nl + nh), d_ws)) return -1;
    return beam_download(d_o, nl, nh, labels_out, out_lengths, scores, label_frames, label_logps);
}

int nntk_ctc_beam_decode(const float *probs, int batch, int T, int C, const int *input_lengths, int blank, int beam_width,
                         int cutoff_top_n, int nbest, int *labels_out, int *out_lengths, float *scores) {
    return beam_decode_host("nntk_ctc_beam_decode", probs, batch, T, C, input_lengths, blank, beam_width, cutoff_top_n, nbest, NULL,
                            labels_out, out_lengths, scores, NULL, NULL);
}
int nntk_ctc_beam_decode_lm(const float *probs, int batch, int T, int C, const int *input_lengths, int blank, int beam_width,
                            int cutoff_top_n, int nbest, NntkNgramLm lm, int *labels_out, int *out_lengths, float *scores) {
    return beam_decode_host("nntk_ctc_beam_decode_lm", probs, batch, T, C, input_lengths, blank, beam_width, cutoff_top_n, nbest, lm,
                            labels_out, out_lengths, scores, NULL, NULL);
}
int nntk_ctc_beam_decode_opt(const float *probs, int batch, int T, int C, const int *input_lengths, int blank, int beam_width,
                             int cutoff_top_n, int nbest, const NntkCtcBeamOptions *o, int *labels_out, int *out_lengths, float *scores) {
    return beam_decode_host("nntk_ctc_beam_decode_opt", probs, batch, T, C, input_lengths, blank, beam_width, cutoff_top_n, nbest,
                            o ? o->lm : NULL, labels_out, out_lengths, scores, o ? o->label_frames : NULL, o ? o->label_logps : NULL);
}

/* ---- streaming CTC decoding (INTEGRATION.md "CTC prefix beam search", Streaming).  The beam lives in the handle's device buffer; which
 *      rows are new, how many frames each has seen and which half of its label strings is current is host bookkeeping, uploaded with
 *      every push: a reset touches no device memory ---- */
struct NntkCtcBeamStreamStruct {
    int batch, max_frames, C, blank, beam_width, cutoff_top_n, nbest, max_labels;
    int *frames;                    /* [batch] frames since the row's reset */
    int *half;                      /* [batch] the current half of the row's label strings */
    int *ctl;                       /* [4][batch] staging of one push */
    NntkNgramLm lm;                 /* NULL: acoustic scores only.  Not owned: it outlives the stream */
    int detail;                     /* the rows also carry their labels' frames and log-probabilities */
    nntk_devbuf d_buf;              /* nntk_shim_ctc_beam_stream_floats words, reserved by the first push */
    nntk_devbuf d_io;               /* the host-pointer push: probabilities | labels | lengths | scores */
};

size_t nntk_ctc_beam_stream_state_bytes(int batch, int max_frames, int C, int beam_width, int cutoff_top_n, int max_labels) {
    return sizeof(float) * nntk_shim_ctc_beam_stream_floats(batch, max_frames, C, beam_width, cutoff_top_n, max_labels, 0, 0);
}
size_t nntk_ctc_beam_stream_state_bytes_lm(int batch, int max_frames, int C, int beam_width, int cutoff_top_n, int max_labels) {
    return sizeof(float) * nntk_shim_ctc_beam_stream_floats(batch, max_frames, C, beam_width, cutoff_top_n, max_labels, 1, 0);
}
size_t nntk_ctc_beam_stream_state_bytes_opt(int batch, int max_frames, int C, int beam_width, int cutoff_top_n, int max_labels, int with_lm,
                                            int with_detail) {
    return sizeof(float) * nntk_shim_ctc_beam_stream_floats(batch, max_frames, C, beam_width, cutoff_top_n, max_labels, with_lm != 0,
                                                            with_detail != 0);
}

static NntkCtcBeamStream beam_stream_create(int batch, int max_frames, int C, int blank, int beam_width, int cutoff_top_n, int nbest,
                                            int max_labels, NntkNgramLm lm, int detail) {
    static const char who[] = "nntk_ctc_beam_stream_create";
    nntk_shim_clear_error();
    if (ctc_beam_check(who, batch, 0, C, NULL, blank, beam_width, cutoff_top_n, nbest)) return NULL;
    if (max_frames < 1) { ctc_fail(who, "max_frames %d < 1", max_frames, 0, 0); return NULL; }
    if (max_labels < 1) { ctc_fail(who, "max_labels %d < 1", max_labels, 0, 0); return NULL; }
    if (ctc_beam_lm_check(who, lm, C, blank)) return NULL;
    if (nntk_shim_ctc_beam_stream_check(C, beam_width, cutoff_top_n, lm != NULL)) return NULL;
    NntkCtcBeamStream s = (NntkCtcBeamStream)calloc(1, sizeof *s);
    const size_t rows = (size_t)(batch > 0 ? batch : 1);
    if (s) {
        s->frames = (int *)calloc(rows, sizeof(int));
        s->half = (int *)calloc(rows, sizeof(int));
        s->ctl = (int *)calloc(4 * rows, sizeof(int));
    }
    if (!s || !s->frames || !s->half || !s->ctl) {
        nntk_ctc_beam_stream_destroy(s);
        nntk_set_error("out of host memory");
        return NULL;
    }
    s->batch = batch; s->max_frames = max_frames; s->C = C; s->blank = blank;
    s->beam_width = beam_width; s->cutoff_top_n = cutoff_top_n; s->nbest = nbest; s->max_labels = max_labels;
    s->lm = lm;
    s->detail = detail != 0;
    return s;
}

NntkCtcBeamStream nntk_ctc_beam_stream_create(int batch, int max_frames, int C, int blank, int beam_width, int cutoff_top_n, int nbest,
                                              int max_labels) {
    return beam_stream_create(batch, max_frames, C, blank, beam_width, cutoff_top_n, nbest, max_labels, NULL, 0);
}
NntkCtcBeamStream nntk_ctc_beam_stream_create_lm(int batch, int max_frames, int C, int blank, int beam_width, int cutoff_top_n, int nbest,
                                                 int max_labels, NntkNgramLm lm) {
    return beam_stream_create(batch, max_frames, C, blank, beam_width, cutoff_top_n, nbest, max_labels, lm, 0);
}
NntkCtcBeamStream nntk_ctc_beam_stream_create_opt(int batch, int max_frames, int C, int blank, int beam_width, int cutoff_top_n, int nbest,
                                                  int max_labels, NntkNgramLm lm, int with_detail) {
    return beam_stream_create(batch, max_frames, C, blank, beam_width, cutoff_top_n, nbest, max_labels, lm, with_detail);
}

void nntk_ctc_beam_stream_destroy(NntkCtcBeamStream s) {
    if (!s) return;
    nntk_devbuf_free(&s->d_buf);
    nntk_devbuf_free(&s->d_io);
    free(s->frames);
    free(s->half);
    free(s->ctl);
    free(s);
}

int nntk_ctc_beam_stream_reset(NntkCtcBeamStream s, const int *rows, int n_rows) {
    static const char who[] = "nntk_ctc_beam_stream_reset";
    nntk_shim_clear_error();
    if (!s) NNTK_FAIL("nntk_ctc_beam_stream_reset: NULL handle");
    if (n_rows < 0) return ctc_fail(who, "n_rows %d < 0", n_rows, 0, 0);
    if (n_rows > 0 && !rows) NNTK_FAIL("nntk_ctc_beam_stream_reset: NULL rows");
    for (int i = 0; i < n_rows; ++i)
        if (rows[i] < 0 || rows[i] >= s->batch) return ctc_fail(who, "rows[%d] = %d is outside [0, %d)", i, rows[i], s->batch);
    for (int i = 0; i < n_rows; ++i) s->frames[rows[i]] = 0;        /* the next push starts the row from the empty prefix */
    return 0;
}

/* every check of a push; nothing is enqueued and nothing in the handle changes */
static int beam_stream_check_push(const char *who, NntkCtcBeamStream s, const void *probs, const int *n_frames, const void *labels,
                                  const void *lengths, const void *scores) {
    if (!n_frames || !probs || !labels || !lengths || !scores) return ctc_fail(who, "NULL argument", 0, 0, 0);
    for (int b = 0; b < s->batch; ++b) {
        if (n_frames[b] < 0 || n_frames[b] > s->max_frames)
            return ctc_fail(who, "n_frames[%d] = %d is outside [0, max_frames = %d]", b, n_frames[b], s->max_frames);
        if (n_frames[b] > NNTK_CTC_BEAM_MAX_T - s->frames[b])
            return ctc_fail(who, "row %d would pass %d frames since its reset", b, NNTK_CTC_BEAM_MAX_T, 0);
    }
    return 0;
}

/* which push a handle takes: one created with detail only the _opt pushes (opt), one created without it no detail pointer */
static int beam_stream_check_detail(const char *who, NntkCtcBeamStream s, int opt, const void *frames, const void *logps) {
    if (s->detail && !opt)
        return ctc_fail(who, "the stream was created with detail: push it through the _opt call", 0, 0, 0);
    if (!s->detail && (frames || logps))
        return ctc_fail(who, "the stream was created without detail: it holds no label frames or log-probabilities", 0, 0, 0);
    return 0;
}

static int beam_stream_push_device(const char *who, int opt, NntkCtcBeamStream s, const float *d_probs, const int *n_frames,
                                   const int *final, int *d_labels_out, int *d_out_lengths, float *d_scores, int *d_label_frames,
                                   float *d_label_logps) {
    nntk_shim_clear_error();
    if (!s) return ctc_fail(who, "NULL handle", 0, 0, 0);
    if (s->batch == 0) return 0;
    if (beam_stream_check_push(who, s, d_probs, n_frames, d_labels_out, d_out_lengths, d_scores) ||
        beam_stream_check_detail(who, s, opt, d_label_frames, d_label_logps)) return -1;
    if (d_label_frames || d_label_logps) {
        const size_t nh = (size_t)s->batch * s->nbest, nl = nh * s->max_labels;
        const beam_span other[4] = {
            { d_labels_out, nl * sizeof(int), "d_labels_out" }, { d_out_lengths, nh * sizeof(int), "d_out_lengths" },
            { d_scores, nh * sizeof(float), "d_scores" }, { d_probs, (size_t)s->batch * s->max_frames * s->C * sizeof(float), "d_probs" } };
        if (beam_detail_check(who, d_label_frames, d_label_logps, nl, other, 4)) return -1;
    }
    const int B = s->batch;
    nntk_shim_lm tab;
    if (s->lm && nntk_ngram_lm_device(s->lm, &tab)) return -1;
    float *d_buf = nntk_devbuf_reserve(&s->d_buf, nntk_shim_ctc_beam_stream_floats(B, s->max_frames, s->C, s->beam_width, s->cutoff_top_n,
                                                                                   s->max_labels, s->lm != NULL, s->detail));
    if (!d_buf) return -1;
    int any = 0;
    for (int b = 0; b < B; ++b) {
        s->ctl[b] = n_frames[b];
        s->ctl[B + b] = s->frames[b];
        s->ctl[2 * B + b] = s->half[b];
        s->ctl[3 * B + b] = 0;
        any |= n_frames[b] > 0;
    }
    if (nntk_shim_ctc_beam_stream_push(d_probs, B, s->max_frames, s->C, s->ctl, any, s->blank, s->beam_width, s->cutoff_top_n, s->nbest,
                                       s->max_labels, s->lm ? &tab : NULL, s->detail, d_labels_out, d_out_lengths, d_scores, d_label_frames,
                                       d_label_logps, d_buf)) return -1;
    for (int b = 0; b < B; ++b) {
        if (n_frames[b] > 0) { s->frames[b] += n_frames[b]; s->half[b] ^= 1; }
        if (final && final[b]) s->frames[b] = 0;
    }
    return 0;
}

int nntk_ctc_beam_stream_push_device(NntkCtcBeamStream s, const float *d_probs, const int *n_frames, const int *final,
                                     int *d_labels_out, int *d_out_lengths, float *d_scores) {
    return beam_stream_push_device("nntk_ctc_beam_stream_push_device", 0, s, d_probs, n_frames, final, d_labels_out, d_out_lengths,
                                   d_scores, NULL, NULL);
}
int nntk_ctc_beam_stream_push_opt_device(NntkCtcBeamStream s, const float *d_probs, const int *n_frames, const int *final,
                                         int *d_labels_out, int *d_out_lengths, float *d_scores, int *d_label_frames,
                                         float *d_label_logps) {
    return beam_stream_push_device("nntk_ctc_beam_stream_push_opt_device", 1, s, d_probs, n_frames, final, d_labels_out, d_out_lengths,
                                   d_scores, d_label_frames, d_label_logps);
}

static int beam_stream_push_host(const char *who, int opt, NntkCtcBeamStream s, const float *probs, const int *n_frames, const int *final,
                                 int *labels_out, int *out_lengths, float *scores, int *label_frames, float *label_logps) {
    nntk_shim_clear_error();
    if (!s) return ctc_fail(who, "NULL handle", 0, 0, 0);
    if (s->batch == 0) return 0;
    if (beam_stream_check_push(who, s, probs, n_frames, labels_out, out_lengths, scores) ||
        beam_stream_check_detail(who, s, opt, label_frames, label_logps)) return -1;
    const size_t n = (size_t)s->batch * s->max_frames * s->C, nh = (size_t)s->batch * s->nbest, nl = nh * s->max_labels;
    float *d_p = nntk_devbuf_reserve(&s->d_io, n + nl + 2 * nh + (s->detail ? 2 * nl : 0) + 4);
    if (!d_p) return -1;
    int *d_o = (int *)(d_p + n);
    if (nntk_shim_upload(d_p, probs, n * sizeof(float))) return -1;
    if (beam_stream_push_device(who, opt, s, d_p, n_frames, final, d_o, d_o + nl, (float *)(d_o + nl + nh),
                                label_frames ? d_o + nl + 2 * nh : NULL, label_logps ? (float *)(d_o + 2 * nl + 2 * nh) : NULL)) return -1;
    return beam_download(d_o, nl, nh, labels_out, out_lengths, scores, label_frames, label_logps);
}

int nntk_ctc_beam_stream_push(NntkCtcBeamStream s, const float *probs, const int *n_frames, const int *final, int *labels_out,
                              int *out_lengths, float *scores) {
    return beam_stream_push_host("nntk_ctc_beam_stream_push", 0, s, probs, n_frames, final, labels_out, out_lengths, scores, NULL, NULL);
}
int nntk_ctc_beam_stream_push_opt(NntkCtcBeamStream s, const float *probs, const int *n_frames, const int *final, int *labels_out,
                                  int *out_lengths, float *scores, int *label_frames, float *label_logps) {
    return beam_stream_push_host("nntk_ctc_beam_stream_push_opt", 1, s, probs, n_frames, final, labels_out, out_lengths, scores,
                                 label_frames, label_logps);
}

int nntk_ctc_greedy_decode_stream_device(const float *d_probs, int batch, int T, int C, const int *n_frames, int blank, int *d_prev,
                                         int *d_labels_out, int *d_out_lengths) {
    static const char who[] = "nntk_ctc_greedy_decode_stream_device";
    nntk_shim_clear_error();
    if (ctc_check_shape(who, batch, T, C, blank)) return -1;
    if (batch > 0 && !n_frames) NNTK_FAIL("nntk_ctc_greedy_decode_stream_device: NULL n_frames");
    if (nntk_check_lengths(who, n_frames, batch, T, NULL, NULL)) return -1;
    if (batch == 0) return 0;
    if (!d_prev || !d_out_lengths || ((!d_probs || !d_labels_out) && T > 0)) NNTK_FAIL("nntk_ctc_greedy_decode_stream_device: NULL tensor");
    return nntk_shim_ctc_greedy_decode_stream(d_probs, batch, T, C, n_frames, blank, d_prev, d_labels_out, d_out_lengths);
}

/* ---- CTC forced alignment (csrc/hip/ctc_align.hip) ---- */
static int ctc_align_check(const char *who, int batch, int T, int C, const int *input_lengths, const int *labels, const int *label_lengths,
                           int max_label_len, int blank) {
    if (ctc_check_shape(who, batch, T, C, blank) || nntk_check_lengths(who, input_lengths, batch, T, NULL, NULL)) return -1;
    if (max_label_len > NNTK_CTC_ALIGN_MAX_LABELS)
        return ctc_fail(who, "max_label_len %d is more than %d (the extended states of a row live in one workgroup's LDS)", max_label_len,
                        NNTK_CTC_ALIGN_MAX_LABELS, 0);
    return ctc_check_labels(who, batch, C, labels, label_lengths, max_label_len, blank);
}

size_t nntk_ctc_align_workspace_floats(int batch, int T, int max_label_len) {
    return nntk_shim_ctc_align_workspace_floats(batch, T, max_label_len);
}

int nntk_ctc_align_device(const float *d_probs, int batch, int T, int C, const int *input_lengths, const int *labels,
                          const int *label_lengths, int max_label_len, int blank, int *d_states, int *d_spans, float *d_scores,
                          float *d_workspace) {
    static const char who[] = "nntk_ctc_align_device";
    nntk_shim_clear_error();
    if (ctc_align_check(who, batch, T, C, input_lengths, labels, label_lengths, max_label_len, blank)) return -1;
    if (batch == 0) return 0;
    if (!d_scores || !d_workspace || (!d_probs && T > 0)) NNTK_FAIL("nntk_ctc_align_device: NULL tensor");
    int *len = ctc_lengths(input_lengths, batch, T);
    if (!len) return -1;
    int rc = nntk_shim_ctc_align(d_probs, batch, T, C, len, labels, label_lengths, max_label_len, blank, d_states, d_spans, d_scores,
                                 d_workspace);
    free(len);
    return rc;
}

int nntk_ctc_align(const float *probs, int batch, int T, int C, const int *input_lengths, const int *labels, const int *label_lengths,
                   int max_label_len, int blank, int *states, int *spans, float *scores) {
    static const char who[] = "nntk_ctc_align";
    nntk_shim_clear_error();
    if (ctc_align_check(who, batch, T, C, input_lengths, labels, label_lengths, max_label_len, blank)) return -1;
    if (batch == 0) return 0;
    if (!scores || (!probs && T > 0)) NNTK_FAIL("nntk_ctc_align: NULL array");
    const size_t n = (size_t)batch * T * C, ns = states ? (size_t)batch * T : 0, np = spans ? 2 * (size_t)batch * max_label_len : 0;
    float *d_p = nntk_devbuf_reserve(&t_a, n + 4);
    int *d_o = (int *)nntk_devbuf_reserve(&t_b, ns + np + (size_t)batch + 4);           /* states | spans | scores */
    float *d_ws = nntk_devbuf_reserve(&t_c, nntk_shim_ctc_align_workspace_floats(batch, T, max_label_len));
    if (!d_p || !d_o || !d_ws) return -1;
    if (n && nntk_shim_upload(d_p, probs, n * sizeof(float))) return -1;
    if (nntk_ctc_align_device(d_p, batch, T, C, input_lengths, labels, label_lengths, max_label_len, blank, ns ? d_o : NULL,
                              np ? d_o + ns : NULL, (float *)(d_o + ns + np), d_ws)) return -1;
    if (ns && nntk_shim_download(states, d_o, ns * sizeof(int))) return -1;
    if (np && nntk_shim_download(spans, d_o + ns, np * sizeof(int))) return -1;
    return nntk_shim_download(scores, d_o + ns + np, (size_t)batch * sizeof(float));
}
