/*
 * train.c -- host layer of the training path's second slice: the reference's train/loss.{h,c},
 * train/optimizers.{h,c} and ActivationFunctionCalculateGradient (layers/activation.c:47-54), under their own names
 * and host-pointer signatures, plus device-pointer forms for callers that keep tensors in HBM.  The kernels
 * (csrc/hip/train.hip) follow the reference's operation order.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "nntk_internal.h"

/* scratch for the host-pointer forms: per thread and device, freed at thread exit (nntk_thread_scratch, runtime.c) */
#define t_a (*nntk_thread_scratch(NNTK_TS_A))
#define t_b (*nntk_thread_scratch(NNTK_TS_B))
#define t_c (*nntk_thread_scratch(NNTK_TS_C))

/* ---- the three large products of every gradient: VALU kernels in the reference's order for small shapes, the MFMA GEMM
 *      (csrc/hip/train.hip "MFMA forms") once rows * I * K passes 2^27 multiply-adds ---- */
#define t_at (*nntk_thread_scratch(NNTK_TS_AT))
#define t_bt (*nntk_thread_scratch(NNTK_TS_BT))
#define t_pack (*nntk_thread_scratch(NNTK_TS_PACK))
#define t_tmp (*nntk_thread_scratch(NNTK_TS_TMP))
#define t_scr (*nntk_thread_scratch(NNTK_TS_SCR))
#define NNTK_TRAIN_MFMA_MACS ((double)(1 << 27))

/* C [I][K] += A [rows][I]^T B [rows][K];  c [K] += column sums of B.  a_shift_T > 0: A is h [B][T][I], row (b,t) uses h_{t-1} */
int nntk_train_outer_accumulate(const float *d_A, const float *d_B, float *d_C, float *d_c, long rows, int I, int K, int a_shift_T) {
    if (rows <= 0 || K <= 0) return 0;
    /* large products take the row-sliced MFMA form inside the call (train.hip outer_mfma_kernel), small ones the VALU dots */
    float *scr = nntk_devbuf_reserve(&t_scr, nntk_shim_outer_scratch_floats(I, K));
    if (!scr) return -1;
    return nntk_shim_outer_accumulate(d_A, d_B, d_C, d_c, scr, rows, I, K, a_shift_T);
}
/* out [rows][I] = d [rows][K] M [I][K]^T */
int nntk_train_rows_times_rowmat(const float *d_d, const float *d_M, float *d_out, long rows, int I, int K) {
    if (rows <= 0 || I <= 0) return 0;
    const int mfma = (double)rows * I * K >= NNTK_TRAIN_MFMA_MACS && K >= 16 && I >= 32;
    if (!mfma) return nntk_shim_rows_times_rowmat(d_d, d_M, d_out, rows, I, K);
    float *pack = nntk_devbuf_reserve(&t_pack, nntk_shim_gemm_nt_scratch_floats(I, K));
    if (!pack) return -1;
    return nntk_shim_gemm_nt(d_d, d_M, d_out, pack, NULL, rows, I, K, 0);
}

/* ---- activation gradient (activation.c:47-54): cached derivative on `a` when there is one, else derivative on z ---- */
int ActivationFunctionCalculateGradientDevice(ActivationFunction filter, const float *d_z, const float *d_a,
                                              const float *d_dout, float *d_output, int size) {
    nntk_shim_clear_error();
    if (!filter) NNTK_FAIL("ActivationFunctionCalculateGradientDevice: NULL handle");
    long n = size > 0 ? size : filter->input_size;
    int vpc = 1;
    if (filter->kind == NNTK_ACT_SOFTMAX) { vpc = filter->input_size; n *= filter->vector_size; }
    /* ReLU and identity have no cached derivative in the reference (activation_default.c:106, :138): z is used */
    return nntk_shim_activation_grad(filter->kind, filter->vector_size, vpc, d_z, d_a, d_dout, d_output, n);
}

void ActivationFunctionCalculateGradient(ActivationFunction filter, const float *z, const float *a, const float *d_out,
                                         float *output) {
    nntk_shim_clear_error();
    if (!filter) { nntk_set_error("ActivationFunctionCalculateGradient: NULL handle"); return; }
    if (filter->kind == NNTK_ACT_CUSTOM) {          /* the caller's own host functions */
        if (filter->cached_derivative == NULL || a == NULL) {
            if (filter->derivative) filter->derivative(filter->implementer, z, d_out, output, filter->input_size);
        } else {
            filter->cached_derivative(filter->implementer, a, d_out, output, filter->input_size);
        }
        return;
    }
    long n = filter->kind == NNTK_ACT_SOFTMAX ? (long)filter->input_size * filter->vector_size : filter->input_size;
    if (n <= 0) return;
    if ((filter->kind == NNTK_ACT_RELU || filter->kind == NNTK_ACT_IDENTITY) && !z && filter->kind == NNTK_ACT_RELU) {
        nntk_set_error("ActivationFunctionCalculateGradient: ReLU needs z"); return;
    }
    float *d = nntk_devbuf_reserve(&t_a, (size_t)4 * n);
    if (!d) return;
    float *dz = d, *da = d + n, *dd = d + 2 * n, *dout = d + 3 * n;
    /* softmax without a cached output: recompute it from z first (activation_default.c:187-190) */
    const int need_fwd = filter->kind == NNTK_ACT_SOFTMAX && !a;
    if (z && nntk_shim_upload(dz, z, (size_t)n * sizeof(float))) return;
    if (a && nntk_shim_upload(da, a, (size_t)n * sizeof(float))) return;
    if (need_fwd) {
        if (!z) { nntk_set_error("ActivationFunctionCalculateGradient: softmax needs z or a"); return; }
        if (nntk_shim_activation(NNTK_ACT_SOFTMAX, 1.f, filter->vector_size, dz, da, n)) return;
    }
    if (nntk_shim_upload(dd, d_out, (size_t)n * sizeof(float))) return;
    if (nntk_shim_activation_grad(filter->kind, filter->vector_size, filter->input_size, z ? dz : NULL,
                                  (a || need_fwd) ? da : NULL, dd, dout, n)) return;
    nntk_shim_download(output, dout, (size_t)n * sizeof(float));
}

/* ---- losses (train/loss.c) ---- */
static int loss_value(int kind, const float *d_y, const float *d_pred, int size, int batch, float *loss) {
    *loss = 0.0f;
    if (size <= 0 || batch <= 0) return 0;
    float *d_rows = nntk_devbuf_reserve(&t_c, (size_t)batch);
    if (!d_rows) return -1;
    if (nntk_shim_loss_rows(kind, d_y, d_pred, d_rows, size, batch)) return -1;
    float *rows = (float *)malloc((size_t)batch * sizeof(float));
    if (!rows) NNTK_FAIL("out of host memory");
    if (nntk_shim_download(rows, d_rows, (size_t)batch * sizeof(float))) { free(rows); return -1; }
    float acc = 0.0f;
    for (int b = 0; b < batch; ++b) acc += rows[b];          /* loss.c:15-22 / :36-44: summed over the batch in order */
    free(rows);
    *loss = acc / (float)batch;
    return 0;
}
int nntk_mean_squared_error_device(const float *d_y, const float *d_pred, int size, int batch, float *loss) {
    nntk_shim_clear_error();
    return loss_value(0, d_y, d_pred, size, batch, loss);
}
int nntk_categorical_crossentropy_device(const float *d_y, const float *d_pred, int c, int batch, float *loss) {
    nntk_shim_clear_error();
    return loss_value(1, d_y, d_pred, c, batch, loss);
}
int nntk_mean_squared_error_derivative_device(const float *d_y, const float *d_pred, float *d_out, int size, int batch) {
    nntk_shim_clear_error();
    return nntk_shim_loss_grad(0, d_y, d_pred, d_out, size, batch);
}
int nntk_categorical_crossentropy_derivative_device(const float *d_y, const float *d_pred, float *d_out, int c, int batch) {
    nntk_shim_clear_error();
    return nntk_shim_loss_grad(1, d_y, d_pred, d_out, c, batch);
}

static int stage2(const float *y, const float *p, size_t n, float **dy, float **dp) {
    float *d = nntk_devbuf_reserve(&t_a, 2 * n);
    if (!d) return -1;
    *dy = d; *dp = d + n;
    if (nntk_shim_upload(*dy, y, n * sizeof(float))) return -1;
    return nntk_shim_upload(*dp, p, n * sizeof(float));
}
float mean_squared_error(float *y, float *y_pred, int size, int batch) {
    nntk_shim_clear_error();
    float *dy, *dp, loss = 0.0f;
    if ((size_t)size * batch == 0 || stage2(y, y_pred, (size_t)size * batch, &dy, &dp)) return 0.0f;
    loss_value(0, dy, dp, size, batch, &loss);
    return loss;
}
float categorical_crossentropy(float *y, float *y_pred, int c, int batch) {
    nntk_shim_clear_error();
    float *dy, *dp, loss = 0.0f;
    if ((size_t)c * batch == 0 || stage2(y, y_pred, (size_t)c * batch, &dy, &dp)) return 0.0f;
    loss_value(1, dy, dp, c, batch, &loss);
    return loss;
}
static void loss_grad_host(int kind, float *y, float *y_pred, float *d_y_pred, int size, int batch) {
    nntk_shim_clear_error();
    size_t n = (size_t)size * batch;
    float *dy, *dp;
    if (n == 0 || stage2(y, y_pred, n, &dy, &dp)) return;
    float *dd = nntk_devbuf_reserve(&t_b, n);
    if (!dd || nntk_shim_loss_grad(kind, dy, dp, dd, size, batch)) return;
    nntk_shim_download(d_y_pred, dd, n * sizeof(float));
}
void mean_squared_error_derivative(float *y, float *y_pred, float *d_y_pred, int size, int batch) {
    loss_grad_host(0, y, y_pred, d_y_pred, size, batch);
}
void categorical_crossentropy_derivative(float *y, float *y_pred, float *d_y_pred, int c, int batch) {
    loss_grad_host(1, y, y_pred, d_y_pred, c, batch);
}

/* ---- CTC (csrc/hip/ctc.hip): every host array is checked here, before anything is enqueued or allocated ---- */
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

/* host-pointer forms: upload, device call, download */
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

/* ---- CTC prefix beam search (csrc/hip/ctc_beam.hip) ---- */
#define CTC_BEAM_MAX_W 128
#define CTC_BEAM_MAX_CELLS 16384
static int ctc_beam_check(const char *who, int batch, int T, int C, const int *input_lengths, int blank, int beam_width,
                          int cutoff_top_n, int nbest) {
    if (ctc_check_shape(who, batch, T, C, blank) || nntk_check_lengths(who, input_lengths, batch, T, NULL, NULL)) return -1;
    if (beam_width < 1 || beam_width > CTC_BEAM_MAX_W)
        return ctc_fail(who, "beam_width %d is outside [1, %d]", beam_width, CTC_BEAM_MAX_W, 0);
    if (nbest < 1 || nbest > beam_width) return ctc_fail(who, "nbest %d is outside [1, beam_width = %d]", nbest, beam_width, 0);
    if (cutoff_top_n < 0) return ctc_fail(who, "cutoff_top_n %d < 0", cutoff_top_n, 0, 0);
    const int n = cutoff_top_n == 0 || cutoff_top_n >= C - 1 ? C - 1 : cutoff_top_n;      /* expanded classes per frame */
    if ((long long)beam_width * (n + 1) > CTC_BEAM_MAX_CELLS)
        return ctc_fail(who, "beam_width %d x (%d expanded classes + 1) is more than %d candidate cells: lower beam_width or set cutoff_top_n",
                        beam_width, n, CTC_BEAM_MAX_CELLS);
    if (T >= (1 << 23)) return ctc_fail(who, "T %d is not below %d frames", T, 1 << 23, 0);
    return 0;
}

size_t nntk_ctc_beam_workspace_floats(int batch, int T, int C, int beam_width, int cutoff_top_n) {
    return nntk_shim_ctc_beam_workspace_floats(batch, T, C, beam_width, cutoff_top_n);
}

int nntk_ctc_beam_decode_device(const float *d_probs, int batch, int T, int C, const int *input_lengths, int blank, int beam_width,
                                int cutoff_top_n, int nbest, int *d_labels_out, int *d_out_lengths, float *d_scores,
                                float *d_workspace) {
    static const char who[] = "nntk_ctc_beam_decode_device";
    nntk_shim_clear_error();
    if (ctc_beam_check(who, batch, T, C, input_lengths, blank, beam_width, cutoff_top_n, nbest)) return -1;
    if (batch == 0) return 0;
    if (!d_out_lengths || !d_scores || !d_workspace || ((!d_probs || !d_labels_out) && T > 0))
        NNTK_FAIL("nntk_ctc_beam_decode_device: NULL tensor");
    int *len = ctc_lengths(input_lengths, batch, T);
    if (!len) return -1;
    int rc = nntk_shim_ctc_beam_decode(d_probs, batch, T, C, len, blank, beam_width, cutoff_top_n, nbest, d_labels_out, d_out_lengths,
                                       d_scores, d_workspace);
    free(len);
    return rc;
}

int nntk_ctc_beam_decode(const float *probs, int batch, int T, int C, const int *input_lengths, int blank, int beam_width,
                         int cutoff_top_n, int nbest, int *labels_out, int *out_lengths, float *scores) {
    static const char who[] = "nntk_ctc_beam_decode";
    nntk_shim_clear_error();
    if (ctc_beam_check(who, batch, T, C, input_lengths, blank, beam_width, cutoff_top_n, nbest)) return -1;
    if (batch == 0) return 0;
    if (!out_lengths || !scores || ((!probs || !labels_out) && T > 0)) NNTK_FAIL("nntk_ctc_beam_decode: NULL array");
    const size_t n = (size_t)batch * T * C, nh = (size_t)batch * nbest, nl = nh * T;
    float *d_p = nntk_devbuf_reserve(&t_a, n + 4);
    int *d_o = (int *)nntk_devbuf_reserve(&t_b, nl + 2 * nh + 4);             /* labels | lengths | scores */
    float *d_ws = nntk_devbuf_reserve(&t_c, nntk_shim_ctc_beam_workspace_floats(batch, T, C, beam_width, cutoff_top_n));
    if (!d_p || !d_o || !d_ws) return -1;
    if (n && nntk_shim_upload(d_p, probs, n * sizeof(float))) return -1;
    if (nntk_ctc_beam_decode_device(d_p, batch, T, C, input_lengths, blank, beam_width, cutoff_top_n, nbest, d_o, d_o + nl,
                                    (float *)(d_o + nl + nh), d_ws)) return -1;
    if (nl && nntk_shim_download(labels_out, d_o, nl * sizeof(int))) return -1;
    if (nntk_shim_download(out_lengths, d_o + nl, nh * sizeof(int))) return -1;
    return nntk_shim_download(scores, d_o + nl + nh, nh * sizeof(float));
}

/* ---- language-model fusion (INTEGRATION.md "CTC prefix beam search", Language-model fusion): the calls above with an n-gram handle
 *      (ngram_lm.c); lm NULL: the calls above themselves ---- */
size_t nntk_ctc_beam_lm_workspace_floats(int batch, int T, int C, int beam_width, int cutoff_top_n) {
    return nntk_shim_ctc_beam_lm_workspace_floats(batch, T, C, beam_width, cutoff_top_n);
}

static int ctc_beam_lm_check(const char *who, NntkNgramLm lm, int C, int blank) {
    if (lm && !nntk_ngram_lm_matches(lm, C, blank))
        return ctc_fail(who, "the language model was built for another class count or blank than C = %d, blank = %d", C, blank, 0);
    return 0;
}

int nntk_ctc_beam_decode_lm_device(const float *d_probs, int batch, int T, int C, const int *input_lengths, int blank, int beam_width,
                                   int cutoff_top_n, int nbest, NntkNgramLm lm, int *d_labels_out, int *d_out_lengths, float *d_scores,
                                   float *d_workspace) {
    static const char who[] = "nntk_ctc_beam_decode_lm_device";
    if (!lm)
        return nntk_ctc_beam_decode_device(d_probs, batch, T, C, input_lengths, blank, beam_width, cutoff_top_n, nbest, d_labels_out,
                                           d_out_lengths, d_scores, d_workspace);
    nntk_shim_clear_error();
    if (ctc_beam_check(who, batch, T, C, input_lengths, blank, beam_width, cutoff_top_n, nbest) || ctc_beam_lm_check(who, lm, C, blank))
        return -1;
    if (batch == 0) return 0;
    if (!d_out_lengths || !d_scores || !d_workspace || ((!d_probs || !d_labels_out) && T > 0))
        NNTK_FAIL("nntk_ctc_beam_decode_lm_device: NULL tensor");
    nntk_shim_lm tab;
    if (nntk_ngram_lm_device(lm, &tab)) return -1;
    int *len = ctc_lengths(input_lengths, batch, T);
    if (!len) return -1;
    int rc = nntk_shim_ctc_beam_decode_lm(d_probs, batch, T, C, len, blank, beam_width, cutoff_top_n, nbest, &tab, d_labels_out,
                                          d_out_lengths, d_scores, d_workspace);
    free(len);
    return rc;
}

int nntk_ctc_beam_decode_lm(const float *probs, int batch, int T, int C, const int *input_lengths, int blank, int beam_width,
                            int cutoff_top_n, int nbest, NntkNgramLm lm, int *labels_out, int *out_lengths, float *scores) {
    static const char who[] = "nntk_ctc_beam_decode_lm";
    nntk_shim_clear_error();
    if (ctc_beam_check(who, batch, T, C, input_lengths, blank, beam_width, cutoff_top_n, nbest) || ctc_beam_lm_check(who, lm, C, blank))
        return -1;
    if (batch == 0) return 0;
    if (!out_lengths || !scores || ((!probs || !labels_out) && T > 0)) NNTK_FAIL("nntk_ctc_beam_decode_lm: NULL array");
    const size_t n = (size_t)batch * T * C, nh = (size_t)batch * nbest, nl = nh * T;
    float *d_p = nntk_devbuf_reserve(&t_a, n + 4);
    int *d_o = (int *)nntk_devbuf_reserve(&t_b, nl + 2 * nh + 4);             /* labels | lengths | scores */
    float *d_ws = nntk_devbuf_reserve(&t_c, nntk_shim_ctc_beam_lm_workspace_floats(batch, T, C, beam_width, cutoff_top_n));
    if (!d_p || !d_o || !d_ws) return -1;
    if (n && nntk_shim_upload(d_p, probs, n * sizeof(float))) return -1;
    if (nntk_ctc_beam_decode_lm_device(d_p, batch, T, C, input_lengths, blank, beam_width, cutoff_top_n, nbest, lm, d_o, d_o + nl,
                                       (float *)(d_o + nl + nh), d_ws)) return -1;
    if (nl && nntk_shim_download(labels_out, d_o, nl * sizeof(int))) return -1;
    if (nntk_shim_download(out_lengths, d_o + nl, nh * sizeof(int))) return -1;
    return nntk_shim_download(scores, d_o + nl + nh, nh * sizeof(float));
}

/* ---- streaming CTC decoding (INTEGRATION.md "CTC prefix beam search", Streaming).  The beam lives in the handle's device buffer; which
 *      rows are new, how many frames each has seen and which half of its label strings is current is host bookkeeping, uploaded with
 *      every push: a reset touches no device memory ---- */
#define CTC_BEAM_MAX_T ((1 << 23) - 1)
struct NntkCtcBeamStreamStruct {
    int batch, max_frames, C, blank, beam_width, cutoff_top_n, nbest, max_labels;
    int *frames;                    /* [batch] frames since the row's reset */
    int *half;                      /* [batch] the current half of the row's label strings */
    int *ctl;                       /* [4][batch] staging of one push */
    NntkNgramLm lm;                 /* NULL: acoustic scores only.  Not owned: it outlives the stream */
    nntk_devbuf d_buf;              /* nntk_shim_ctc_beam_stream_floats words, reserved by the first push */
    nntk_devbuf d_io;               /* the host-pointer push: probabilities | labels | lengths | scores */
};

size_t nntk_ctc_beam_stream_state_bytes(int batch, int max_frames, int C, int beam_width, int cutoff_top_n, int max_labels) {
    return sizeof(float) * nntk_shim_ctc_beam_stream_floats(batch, max_frames, C, beam_width, cutoff_top_n, max_labels);
}

size_t nntk_ctc_beam_stream_state_bytes_lm(int batch, int max_frames, int C, int beam_width, int cutoff_top_n, int max_labels) {
    return sizeof(float) * nntk_shim_ctc_beam_stream_lm_floats(batch, max_frames, C, beam_width, cutoff_top_n, max_labels);
}

NntkCtcBeamStream nntk_ctc_beam_stream_create(int batch, int max_frames, int C, int blank, int beam_width, int cutoff_top_n, int nbest,
                                              int max_labels) {
    return nntk_ctc_beam_stream_create_lm(batch, max_frames, C, blank, beam_width, cutoff_top_n, nbest, max_labels, NULL);
}

NntkCtcBeamStream nntk_ctc_beam_stream_create_lm(int batch, int max_frames, int C, int blank, int beam_width, int cutoff_top_n, int nbest,
                                                 int max_labels, NntkNgramLm lm) {
    static const char who[] = "nntk_ctc_beam_stream_create";
    nntk_shim_clear_error();
    if (ctc_beam_check(who, batch, 0, C, NULL, blank, beam_width, cutoff_top_n, nbest)) return NULL;
    if (max_frames < 1) { ctc_fail(who, "max_frames %d < 1", max_frames, 0, 0); return NULL; }
    if (max_labels < 1) { ctc_fail(who, "max_labels %d < 1", max_labels, 0, 0); return NULL; }
    if (ctc_beam_lm_check(who, lm, C, blank)) return NULL;
    if (lm ? nntk_shim_ctc_beam_stream_check_lm(C, beam_width, cutoff_top_n) : nntk_shim_ctc_beam_stream_check(C, beam_width, cutoff_top_n))
        return NULL;
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
    return s;
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
        if (n_frames[b] > CTC_BEAM_MAX_T - s->frames[b])
            return ctc_fail(who, "row %d would pass %d frames since its reset", b, CTC_BEAM_MAX_T, 0);
    }
    return 0;
}

int nntk_ctc_beam_stream_push_device(NntkCtcBeamStream s, const float *d_probs, const int *n_frames, const int *final,
                                     int *d_labels_out, int *d_out_lengths, float *d_scores) {
    static const char who[] = "nntk_ctc_beam_stream_push_device";
    nntk_shim_clear_error();
    if (!s) NNTK_FAIL("nntk_ctc_beam_stream_push_device: NULL handle");
    if (s->batch == 0) return 0;
    if (beam_stream_check_push(who, s, d_probs, n_frames, d_labels_out, d_out_lengths, d_scores)) return -1;
    const int B = s->batch;
    nntk_shim_lm tab;
    if (s->lm && nntk_ngram_lm_device(s->lm, &tab)) return -1;
    float *d_buf = nntk_devbuf_reserve(&s->d_buf, (s->lm ? nntk_shim_ctc_beam_stream_lm_floats : nntk_shim_ctc_beam_stream_floats)(
                                                      B, s->max_frames, s->C, s->beam_width, s->cutoff_top_n, s->max_labels));
    if (!d_buf) return -1;
    int any = 0;
    for (int b = 0; b < B; ++b) {
        s->ctl[b] = n_frames[b];
        s->ctl[B + b] = s->frames[b];
        s->ctl[2 * B + b] = s->half[b];
        s->ctl[3 * B + b] = 0;
        any |= n_frames[b] > 0;
    }
    if (s->lm ? nntk_shim_ctc_beam_stream_push_lm(d_probs, B, s->max_frames, s->C, s->ctl, any, s->blank, s->beam_width, s->cutoff_top_n,
                                                  s->nbest, s->max_labels, &tab, d_labels_out, d_out_lengths, d_scores, d_buf)
              : nntk_shim_ctc_beam_stream_push(d_probs, B, s->max_frames, s->C, s->ctl, any, s->blank, s->beam_width, s->cutoff_top_n,
                                               s->nbest, s->max_labels, d_labels_out, d_out_lengths, d_scores, d_buf)) return -1;
    for (int b = 0; b < B; ++b) {
        if (n_frames[b] > 0) { s->frames[b] += n_frames[b]; s->half[b] ^= 1; }
        if (final && final[b]) s->frames[b] = 0;
    }
    return 0;
}

int nntk_ctc_beam_stream_push(NntkCtcBeamStream s, const float *probs, const int *n_frames, const int *final, int *labels_out,
                              int *out_lengths, float *scores) {
    static const char who[] = "nntk_ctc_beam_stream_push";
    nntk_shim_clear_error();
    if (!s) NNTK_FAIL("nntk_ctc_beam_stream_push: NULL handle");
    if (s->batch == 0) return 0;
    if (beam_stream_check_push(who, s, probs, n_frames, labels_out, out_lengths, scores)) return -1;
    const size_t n = (size_t)s->batch * s->max_frames * s->C, nh = (size_t)s->batch * s->nbest, nl = nh * s->max_labels;
    float *d_p = nntk_devbuf_reserve(&s->d_io, n + nl + 2 * nh + 4);
    if (!d_p) return -1;
    int *d_o = (int *)(d_p + n);
    if (nntk_shim_upload(d_p, probs, n * sizeof(float))) return -1;
    if (nntk_ctc_beam_stream_push_device(s, d_p, n_frames, final, d_o, d_o + nl, (float *)(d_o + nl + nh))) return -1;
    if (nntk_shim_download(labels_out, d_o, nl * sizeof(int))) return -1;
    if (nntk_shim_download(out_lengths, d_o + nl, nh * sizeof(int))) return -1;
    return nntk_shim_download(scores, d_o + nl + nh, nh * sizeof(float));
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
#define CTC_ALIGN_MAX_LABELS 4000
static int ctc_align_check(const char *who, int batch, int T, int C, const int *input_lengths, const int *labels, const int *label_lengths,
                           int max_label_len, int blank) {
    if (ctc_check_shape(who, batch, T, C, blank) || nntk_check_lengths(who, input_lengths, batch, T, NULL, NULL)) return -1;
    if (max_label_len > CTC_ALIGN_MAX_LABELS)
        return ctc_fail(who, "max_label_len %d is more than %d (the extended states of a row live in one workgroup's LDS)", max_label_len,
                        CTC_ALIGN_MAX_LABELS, 0);
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

/* ---- SGD (train/optimizers.c:13-19) ---- */
int nntk_sgd_optimize_device(SGD optimizer, const float *d_gradient, float *d_weights, long size) {
    nntk_shim_clear_error();
    return nntk_shim_sgd(optimizer.learning_rate, d_gradient, d_weights, size);
}
int sgd_optimize(SGD optimizer, float *gradient, float *weights, int size) {
    nntk_shim_clear_error();
    if (size <= 0) return 0;
    float *dg, *dw;
    if (stage2(gradient, weights, (size_t)size, &dg, &dw)) return -1;
    if (nntk_shim_sgd(optimizer.learning_rate, dg, dw, size)) return -1;
    return nntk_shim_download(weights, dw, (size_t)size * sizeof(float));
}

/* ---- the multi-tensor optimizer (csrc/hip/optim.hip): every argument is checked here, before anything is allocated or enqueued ---- */
struct NntkOptimizerStruct {
    nntk_optim_plan plan;
    nntk_optim_block *blocks;       /* host copy of the table: the moment pointers nntk_optimizer_state_device hands out */
    nntk_optim_block *d_blocks;
    float *d_state;                 /* the moments of every block */
    float *d_scalars;               /* the control block [8], then the partial sums [n_chunks] */
};

static void *opt_fail(const char *fmt, long a) {
    char msg[200];
    int n = snprintf(msg, sizeof msg, "nntk_optimizer_create: ");
    snprintf(msg + n, sizeof msg - (size_t)n, fmt, a);
    nntk_set_error(msg);
    return NULL;
}
static void *opt_fail_value(const char *name, double v, const char *rule) {
    char msg[200];
    snprintf(msg, sizeof msg, "nntk_optimizer_create: %s = %g %s", name, v, rule);
    nntk_set_error(msg);
    return NULL;
}

NntkOptimizer nntk_optimizer_create(NntkOptimizerConfig cfg, int n_blocks, float *const *d_weights, float *const *d_grads, const long *sizes) {
    nntk_shim_clear_error();
    if (cfg.kind < 0 || cfg.kind > 2) return opt_fail("unknown kind %ld (0 SGD, 1 momentum SGD, 2 Adam)", cfg.kind);
    if (n_blocks < 0) return opt_fail("n_blocks %ld < 0", n_blocks);
    if (!(cfg.beta1 >= 0.0f && cfg.beta1 < 1.0f)) return opt_fail_value("beta1", cfg.beta1, "is outside [0, 1)");
    if (!(cfg.beta2 >= 0.0f && cfg.beta2 < 1.0f)) return opt_fail_value("beta2", cfg.beta2, "is outside [0, 1)");
    if (!(cfg.epsilon >= 0.0f)) return opt_fail_value("epsilon", cfg.epsilon, "is negative");
    if (!(cfg.clip_norm >= 0.0f)) return opt_fail_value("clip_norm", cfg.clip_norm, "is negative");
    if (!(cfg.weight_decay >= 0.0f)) return opt_fail_value("weight_decay", cfg.weight_decay, "is negative");
    if (!(cfg.momentum >= 0.0f)) return opt_fail_value("momentum", cfg.momentum, "is negative");
    if (n_blocks > 0 && (!d_weights || !d_grads || !sizes)) return opt_fail("NULL pointer table for %ld blocks", n_blocks);
    long total = 0;
    for (int b = 0; b < n_blocks; ++b) {
        if (sizes[b] < 0) return opt_fail("block %ld has a negative size", b);
        if (sizes[b] == 0) continue;
        if (!d_weights[b] || !d_grads[b]) return opt_fail("block %ld has a NULL weights or gradient pointer", b);
        if (((size_t)d_weights[b] | (size_t)d_grads[b]) & 3) return opt_fail("block %ld is not 4-byte aligned", b);
        if (sizes[b] > (1L << 60) - total) return opt_fail("block %ld: the total size overflows", b);
        total += sizes[b];
    }

    NntkOptimizer o = (NntkOptimizer)calloc(1, sizeof *o);
    nntk_optim_block *blk = (nntk_optim_block *)calloc((size_t)n_blocks + 1, sizeof *blk);
    if (!o || !blk) { free(o); free(blk); nntk_set_error("nntk_optimizer_create: out of host memory"); return NULL; }
    o->blocks = blk;
    nntk_optim_plan *p = &o->plan;
    p->kind = cfg.kind; p->nesterov = cfg.nesterov != 0; p->decoupled = cfg.decoupled != 0; p->zero_gradients = cfg.zero_gradients != 0;
    p->momentum = cfg.momentum; p->beta1 = cfg.beta1; p->beta2 = cfg.beta2; p->epsilon = cfg.epsilon;
    p->weight_decay = cfg.weight_decay; p->grad_scale = cfg.grad_scale == 0.0f ? 1.0f : cfg.grad_scale; p->clip_norm = cfg.clip_norm;
    p->n_blocks = n_blocks;
    p->chunk_floats = nntk_shim_optim_chunk_floats(total);
    /* the chunk list and the layout of the moments: block b's moments start `phase` floats into a 16-byte-aligned region of its own */
    const int n_mom = cfg.kind == 2 ? 2 : cfg.kind == 1 ? 1 : 0;
    size_t region = 0;
    for (int b = 0; b < n_blocks; ++b) {
        blk[b].n = sizes[b];
        blk[b].chunk0 = p->n_chunks;
        if (sizes[b] == 0) continue;
        blk[b].w = d_weights[b]; blk[b].g = d_grads[b];
        blk[b].phase = (int)(((size_t)d_weights[b] >> 2) & 3);
        blk[b].g_vec = (int)(((size_t)d_grads[b] >> 2) & 3) == blk[b].phase;
        p->n_chunks += (blk[b].phase + sizes[b] + p->chunk_floats - 1) / p->chunk_floats;
        region += ((size_t)blk[b].phase + (size_t)sizes[b] + 3) & ~(size_t)3;
    }
    o->d_blocks = (nntk_optim_block *)nntk_shim_malloc(((size_t)n_blocks + 1) * sizeof *blk);
    o->d_scalars = (float *)nntk_shim_malloc((8 + (size_t)p->n_chunks) * sizeof(float));
    if (n_mom) o->d_state = (float *)nntk_shim_malloc((size_t)n_mom * region * sizeof(float));
    if (!o->d_blocks || !o->d_scalars || (n_mom && !o->d_state)) { nntk_optimizer_destroy(o); return NULL; }
    size_t off = 0;
    for (int b = 0; b < n_blocks && n_mom; ++b) {
        if (sizes[b] == 0) continue;
        blk[b].m = o->d_state + off + blk[b].phase;
        if (n_mom == 2) blk[b].v = o->d_state + region + off + blk[b].phase;
        off += ((size_t)blk[b].phase + (size_t)sizes[b] + 3) & ~(size_t)3;
    }
    p->d_blocks = o->d_blocks;
    p->d_ctl = o->d_scalars;
    p->d_partial = o->d_scalars + 8;
    const float ctl[8] = { 0.0f, 1.0f, 0.0f, 0.0f, cfg.learning_rate, 0.0f, 0.0f, 0.0f };       /* (the two step counters: integer zero) */
    if (nntk_shim_upload(o->d_blocks, blk, ((size_t)n_blocks + 1) * sizeof *blk) || nntk_shim_upload(o->d_scalars, ctl, sizeof ctl) ||
        (n_mom && nntk_shim_memset(o->d_state, 0, (size_t)n_mom * region * sizeof(float))) || nntk_shim_synchronize()) {
        nntk_optimizer_destroy(o);
        return NULL;
    }
    return o;
}

void nntk_optimizer_destroy(NntkOptimizer opt) {
    if (!opt) return;
    if (opt->d_blocks || opt->d_scalars || opt->d_state) nntk_shim_synchronize();
    nntk_shim_free(opt->d_blocks);
    nntk_shim_free(opt->d_scalars);
    nntk_shim_free(opt->d_state);
    free(opt->blocks);
    free(opt);
}

int nntk_optimizer_step_device(NntkOptimizer opt) {
    nntk_shim_clear_error();
    if (!opt) NNTK_FAIL("nntk_optimizer_step_device: NULL handle");
    return nntk_shim_optim_step(&opt->plan);
}

int nntk_optimizer_set_learning_rate(NntkOptimizer opt, float lr) {
    nntk_shim_clear_error();
    if (!opt) NNTK_FAIL("nntk_optimizer_set_learning_rate: NULL handle");
    return nntk_shim_optim_set_lr(opt->plan.d_ctl, lr);
}

const float *nntk_optimizer_info_device(NntkOptimizer opt) {
    nntk_shim_clear_error();
    if (!opt) { nntk_set_error("nntk_optimizer_info_device: NULL handle"); return NULL; }
    return opt->plan.d_ctl;
}

int nntk_optimizer_state_device(NntkOptimizer opt, int block, float **d_m, float **d_v) {
    nntk_shim_clear_error();
    if (!opt) NNTK_FAIL("nntk_optimizer_state_device: NULL handle");
    if (block < 0 || block >= opt->plan.n_blocks) NNTK_FAIL("nntk_optimizer_state_device: no such block");
    if (d_m) *d_m = opt->blocks[block].m;
    if (d_v) *d_v = opt->blocks[block].v;
    return 0;
}
