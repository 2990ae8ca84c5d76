/*
 * rnnt_decode.c -- host layer of RNN-Transducer decoding: the decoder handle with its own device copy of the weights; greedy search
 * (csrc/hip/rnnt_decode.hip) and, below it, beam search (csrc/hip/rnnt_beam.hip), each with the per-row state of a stream and the
 * decode call in its device-pointer and host-pointer forms; the beam search's plain, _lm and _opt entries share one body a form and the
 * workspace of nntk_shim_rnnt_beam_workspace_floats.  Every argument is checked here, before anything is allocated, uploaded or
 * enqueued: a refusal needs no device and writes nothing.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include "nntk_internal.h"

#define t_a (*nntk_thread_scratch(NNTK_TS_A))
#define t_b (*nntk_thread_scratch(NNTK_TS_B))
#define DEC_STR_(x) #x
#define DEC_STR(x) DEC_STR_(x)

struct NntkRnntDecoderStruct {
    NntkRnntDecoderConfig cfg;
    float *d_table, *d_U, *d_proj, *d_out;      /* the decoder's own blocks (d_proj NULL: identity) */
};

struct NntkRnntDecodeStateStruct {
    NntkRnntDecoder dec;
    int batch;
    float *d_f;                                 /* [batch][2H + J] */
    double *d_score;                            /* [batch] */
    int *d_i;                                   /* [batch][4], then [batch]: the rows of a reset */
};

static int dec_fail(const char *who, const char *fmt, long a, long b, long c) {
    char msg[240];
    int n = snprintf(msg, sizeof msg, "%s: ", who);
    snprintf(msg + n, sizeof msg - (size_t)n, fmt, a, b, c);
    nntk_set_error(msg);
    return -1;
}

static int dec_named_ptr(const char *who, const char *name, const void *p) {
    char msg[240];
    if (p && ((uintptr_t)p & 3) == 0) return 0;
    snprintf(msg, sizeof msg, p ? "%s: %s is not 4-byte aligned" : "%s: %s is NULL", who, name);
    nntk_set_error(msg);
    return -1;
}

static int dec_check_blocks(const char *who, const NntkRnntDecoderConfig *c, const float *d_embed, const float *d_lstm,
                            const float *d_pred_proj, const float *d_out) {
    if (dec_named_ptr(who, "d_embed", d_embed) || dec_named_ptr(who, "d_lstm", d_lstm) || dec_named_ptr(who, "d_out", d_out)) return -1;
    if (d_pred_proj && dec_named_ptr(who, "d_pred_proj", d_pred_proj)) return -1;
    if (!d_pred_proj && c->H != c->J)
        return dec_fail(who, "d_pred_proj is NULL (identity) but H %ld != J %ld", c->H, c->J, 0);
    return 0;
}

static int dec_check_config(const char *who, const NntkRnntDecoderConfig *c) {
    if (c->V < 2) return dec_fail(who, "V %ld < 2: a transducer has the blank and at least one label", c->V, 0, 0);
    if (c->V > NNTK_RNNT_DEC_MAX_V) return dec_fail(who, "V %ld is above the limit %ld", c->V, NNTK_RNNT_DEC_MAX_V, 0);
    if (c->blank < 0 || c->blank >= c->V) return dec_fail(who, "blank %ld is outside [0, %ld)", c->blank, c->V, 0);
    if (c->E < 1 || c->H < 1 || c->J < 1) return dec_fail(who, "E %ld, H %ld, J %ld: each must be at least 1", c->E, c->H, c->J);
    if (c->E > NNTK_RNNT_DEC_MAX_WIDTH || c->H > NNTK_RNNT_DEC_MAX_WIDTH || c->J > NNTK_RNNT_DEC_MAX_WIDTH)
        return dec_fail(who, "E %ld, H %ld, J %ld: one is above the limit " DEC_STR(NNTK_RNNT_DEC_MAX_WIDTH), c->E, c->H, c->J);
    if (c->joint_activation < 0 || c->joint_activation > 2)
        return dec_fail(who, "joint_activation %ld is none of 0 (identity), 1 (tanh), 2 (relu)", c->joint_activation, 0, 0);
    if (c->max_symbols_per_frame < 1) return dec_fail(who, "max_symbols_per_frame %ld < 1", c->max_symbols_per_frame, 0, 0);
    return 0;
}

/* the device work of create and load: copies of U, the projection and the vocabulary Dense, and the folded table embed W + b_i + b_h */
static int dec_load(NntkRnntDecoder d, const float *d_embed, const float *d_lstm, const float *d_pred_proj, const float *d_out) {
    const NntkRnntDecoderConfig *c = &d->cfg;
    const size_t G = 4 * (size_t)c->H;
    if (nntk_shim_rnnt_dec_table(d_embed, d_lstm, c->V, c->E, c->H, d->d_table)) return -1;
    if (nntk_shim_copy_d2d(d->d_U, d_lstm + (size_t)c->E * G, (size_t)c->H * G * sizeof(float))) return -1;
    if (d_pred_proj && nntk_shim_copy_d2d(d->d_proj, d_pred_proj, ((size_t)c->H + 1) * c->J * sizeof(float))) return -1;
    if (nntk_shim_copy_d2d(d->d_out, d_out, ((size_t)c->J + 1) * c->V * sizeof(float))) return -1;
    return nntk_shim_synchronize();             /* the caller's blocks are free for reuse on return */
}

NntkRnntDecoder nntk_rnnt_decoder_create(NntkRnntDecoderConfig cfg, const float *d_embed, const float *d_lstm, const float *d_pred_proj,
                                         const float *d_out) {
    static const char who[] = "nntk_rnnt_decoder_create";
    nntk_shim_clear_error();
    if (dec_check_config(who, &cfg) || dec_check_blocks(who, &cfg, d_embed, d_lstm, d_pred_proj, d_out)) return NULL;
    NntkRnntDecoder d = (NntkRnntDecoder)calloc(1, sizeof *d);
    if (!d) { nntk_set_error("nntk_rnnt_decoder_create: out of host memory"); return NULL; }
    d->cfg = cfg;
    const size_t G = 4 * (size_t)cfg.H;
    d->d_table = (float *)nntk_shim_malloc((size_t)cfg.V * G * sizeof(float));
    d->d_U = d->d_table ? (float *)nntk_shim_malloc((size_t)cfg.H * G * sizeof(float)) : NULL;
    d->d_out = d->d_U ? (float *)nntk_shim_malloc(((size_t)cfg.J + 1) * cfg.V * sizeof(float)) : NULL;
    if (d->d_out && d_pred_proj) d->d_proj = (float *)nntk_shim_malloc(((size_t)cfg.H + 1) * cfg.J * sizeof(float));
    if (!d->d_table || !d->d_U || !d->d_out || (d_pred_proj && !d->d_proj) || dec_load(d, d_embed, d_lstm, d_pred_proj, d_out)) {
        nntk_rnnt_decoder_destroy(d);
        return NULL;
    }
    return d;
}

int nntk_rnnt_decoder_load_weights_device(NntkRnntDecoder d, const float *d_embed, const float *d_lstm, const float *d_pred_proj,
                                          const float *d_out) {
    static const char who[] = "nntk_rnnt_decoder_load_weights_device";
    nntk_shim_clear_error();
    if (!d) return dec_fail(who, "NULL handle", 0, 0, 0);
    if (dec_check_blocks(who, &d->cfg, d_embed, d_lstm, d_pred_proj, d_out)) return -1;
    if ((d_pred_proj != NULL) != (d->d_proj != NULL))
        return dec_fail(who, "d_pred_proj must be given exactly when the decoder was created with one", 0, 0, 0);
    return dec_load(d, d_embed, d_lstm, d_pred_proj, d_out);
}

void nntk_rnnt_decoder_destroy(NntkRnntDecoder d) {
    if (!d) return;
    if (d->d_table) nntk_shim_synchronize();
    nntk_shim_free(d->d_table);
    nntk_shim_free(d->d_U);
    nntk_shim_free(d->d_proj);
    nntk_shim_free(d->d_out);
    free(d);
}

NntkRnntDecodeState nntk_rnnt_decode_state_create(NntkRnntDecoder d, int batch) {
    nntk_shim_clear_error();
    if (!d) { nntk_set_error("nntk_rnnt_decode_state_create: NULL decoder"); return NULL; }
    if (batch < 1) { dec_fail("nntk_rnnt_decode_state_create", "batch %ld < 1", batch, 0, 0); return NULL; }
    NntkRnntDecodeState s = (NntkRnntDecodeState)calloc(1, sizeof *s);
    if (!s) { nntk_set_error("nntk_rnnt_decode_state_create: out of host memory"); return NULL; }
    s->dec = d;
    s->batch = batch;
    s->d_f = (float *)nntk_shim_malloc((size_t)batch * (2 * (size_t)d->cfg.H + d->cfg.J) * sizeof(float));
    s->d_score = s->d_f ? (double *)nntk_shim_malloc((size_t)batch * sizeof(double)) : NULL;
    s->d_i = s->d_score ? (int *)nntk_shim_malloc((size_t)batch * 5 * sizeof(int)) : NULL;
    if (!s->d_i || nntk_shim_memset(s->d_i, 0, (size_t)batch * 5 * sizeof(int))) {
        nntk_rnnt_decode_state_destroy(s);
        return NULL;
    }
    return s;
}

/* the reset of a greedy or a beam state, d_i its [batch][4] (word 0 of a row: started) with [batch] for the rows behind; NULL: no state */
static int dec_state_reset(const char *who, int batch, int *d_i, const int *rows, int n_rows) {
    nntk_shim_clear_error();
    if (!d_i) return dec_fail(who, "NULL state", 0, 0, 0);
    if (n_rows < 0 || n_rows > batch) return dec_fail(who, "n_rows %ld is outside [0, %ld]", n_rows, batch, 0);
    if (!rows && n_rows > 0) return dec_fail(who, "rows is NULL with n_rows %ld", n_rows, 0, 0);
    if (!rows) return nntk_shim_memset(d_i, 0, (size_t)batch * 4 * sizeof(int));
    for (int i = 0; i < n_rows; ++i)
        if (rows[i] < 0 || rows[i] >= batch) return dec_fail(who, "rows[%ld] = %ld is outside [0, %ld)", i, rows[i], batch);
    if (n_rows == 0) return 0;
    int *d_rows = d_i + 4 * (size_t)batch;
    if (nntk_shim_upload_ints(d_rows, rows, n_rows)) return -1;
    return nntk_shim_rnnt_dec_reset(d_i, d_rows, n_rows);
}

int nntk_rnnt_decode_state_reset(NntkRnntDecodeState s, const int *rows, int n_rows) {
    return dec_state_reset("nntk_rnnt_decode_state_reset", s ? s->batch : 0, s ? s->d_i : NULL, rows, n_rows);
}

void nntk_rnnt_decode_state_destroy(NntkRnntDecodeState s) {
    if (!s) return;
    if (s->d_f) nntk_shim_synchronize();
    nntk_shim_free(s->d_f);
    nntk_shim_free(s->d_score);
    nntk_shim_free(s->d_i);
    free(s);
}

static int dec_overlap(const void *a, size_t na, const void *b, size_t nb) {
    return a && b && na && nb && (uintptr_t)a < (uintptr_t)b + nb && (uintptr_t)b < (uintptr_t)a + na;
}

/* no output (the first n_out blocks) may overlap another block of the call */
static int dec_check_overlaps(const char *who, int n_out, int n_all, const void *const *p, const size_t *n, const char *const *name) {
    for (int i = 0; i < n_out; ++i)
        for (int j = i + 1; j < n_all; ++j)
            if (dec_overlap(p[i], n[i], p[j], n[j])) {
                char msg[240];
                snprintf(msg, sizeof msg, "%s: %s overlaps %s", who, name[i], name[j]);
                nntk_set_error(msg);
                return -1;
            }
    return 0;
}

/* everything a decode call can be refused for; tensors = 1: the device form's pointers (alignment, overlap) */
static int dec_check_call(const char *who, NntkRnntDecoder d, NntkRnntDecodeState state, const float *enc, int batch, int T,
                          const int *n_frames, int max_labels, const int *labels_out, const int *label_frames, const int *out_lengths,
                          const float *scores) {
    if (!d) return dec_fail(who, "NULL decoder", 0, 0, 0);
    if (batch < 0 || T < 0) return dec_fail(who, "batch %ld, T %ld: neither may be negative", batch, T, 0);
    if (max_labels < 1) return dec_fail(who, "max_labels %ld < 1", max_labels, 0, 0);
    if (state && state->dec != d) return dec_fail(who, "the state belongs to another decoder", 0, 0, 0);
    if (state && state->batch != batch) return dec_fail(who, "batch %ld differs from the state's %ld", batch, state->batch, 0);
    if (batch == 0) return 0;
    for (int b = 0; n_frames && b < batch; ++b)
        if (n_frames[b] < 0 || n_frames[b] > T) return dec_fail(who, "n_frames[%ld] = %ld is outside [0, %ld]", b, n_frames[b], T);
    if (T > 0 && dec_named_ptr(who, "enc", enc)) return -1;
    if (dec_named_ptr(who, "labels_out", labels_out) || dec_named_ptr(who, "out_lengths", out_lengths)) return -1;
    if (label_frames && dec_named_ptr(who, "label_frames", label_frames)) return -1;
    if (scores && dec_named_ptr(who, "scores", scores)) return -1;
    const size_t nl = (size_t)batch * max_labels * sizeof(int), nb = (size_t)batch * sizeof(int);
    const size_t ne = (size_t)batch * T * d->cfg.J * sizeof(float);
    const void *p[5] = { labels_out, label_frames, out_lengths, scores, enc };
    const size_t n[5] = { nl, nl, nb, nb, ne };
    static const char *const name[5] = { "labels_out", "label_frames", "out_lengths", "scores", "enc" };
    return dec_check_overlaps(who, 5, 5, p, n, name);
}

/* the decoder as the launchers take it */
static nntk_shim_rnnt_dec dec_model(NntkRnntDecoder d) {
    return (nntk_shim_rnnt_dec){ d->d_table, d->d_U, d->d_proj, d->d_out, d->cfg.V, d->cfg.blank, d->cfg.E, d->cfg.H, d->cfg.J,
                                 d->cfg.joint_activation, d->cfg.max_symbols_per_frame };
}

/* every row's frame count, n_frames NULL: T; the caller frees it.  NULL: out of host memory, oom the error */
static int *dec_row_frames(const char *oom, const int *n_frames, int batch, int T) {
    int *len = (int *)malloc((size_t)batch * sizeof(int));
    if (!len) { nntk_set_error(oom); return NULL; }
    for (int b = 0; b < batch; ++b) len[b] = n_frames ? n_frames[b] : T;
    return len;
}

int nntk_rnnt_greedy_decode_device(NntkRnntDecoder d, NntkRnntDecodeState state, const float *d_enc, int batch, int T, const int *n_frames,
                                   int max_labels, int *d_labels_out, int *d_label_frames, int *d_out_lengths, float *d_scores) {
    static const char who[] = "nntk_rnnt_greedy_decode_device";
    nntk_shim_clear_error();
    if (dec_check_call(who, d, state, d_enc, batch, T, n_frames, max_labels, d_labels_out, d_label_frames, d_out_lengths, d_scores)) return -1;
    if (batch == 0) return 0;
    const nntk_shim_rnnt_dec m = dec_model(d);
    int *len = dec_row_frames("nntk_rnnt_greedy_decode_device: out of host memory", n_frames, batch, T);
    if (!len) return -1;
    int rc = nntk_shim_rnnt_greedy(&m, d_enc, batch, T, len, max_labels, state ? state->d_f : NULL, state ? state->d_score : NULL,
                                   state ? state->d_i : NULL, d_labels_out, d_label_frames, d_out_lengths, d_scores);
    free(len);
    return rc;
}

int nntk_rnnt_greedy_decode(NntkRnntDecoder d, NntkRnntDecodeState state, const float *enc, int batch, int T, const int *n_frames,
                            int max_labels, int *labels_out, int *label_frames, int *out_lengths, float *scores) {
    static const char who[] = "nntk_rnnt_greedy_decode";
    nntk_shim_clear_error();
    if (dec_check_call(who, d, state, enc, batch, T, n_frames, max_labels, labels_out, label_frames, out_lengths, scores)) return -1;
    if (batch == 0) return 0;
    const size_t ne = (size_t)batch * T * d->cfg.J, nl = (size_t)batch * max_labels;
    float *d_enc = nntk_devbuf_reserve(&t_a, ne + 4);
    int *d_lab = (int *)nntk_devbuf_reserve(&t_b, 2 * nl + 2 * (size_t)batch + 4);
    if (!d_enc || !d_lab) return -1;
    int *d_fr = d_lab + nl, *d_len = d_fr + nl;
    float *d_sc = (float *)(d_len + batch);
    if (ne && nntk_shim_upload(d_enc, enc, ne * sizeof(float))) return -1;
    if (state) {                                /* a push appends to what the caller's buffers hold */
        if (nntk_shim_upload(d_lab, labels_out, nl * sizeof(int))) return -1;
        if (label_frames && nntk_shim_upload(d_fr, label_frames, nl * sizeof(int))) return -1;
    }
    if (nntk_rnnt_greedy_decode_device(d, state, d_enc, batch, T, n_frames, max_labels, d_lab, label_frames ? d_fr : NULL, d_len,
                                       scores ? d_sc : NULL)) return -1;
    if (nntk_shim_download(labels_out, d_lab, nl * sizeof(int))) return -1;
    if (label_frames && nntk_shim_download(label_frames, d_fr, nl * sizeof(int))) return -1;
    if (nntk_shim_download(out_lengths, d_len, (size_t)batch * sizeof(int))) return -1;
    return scores ? nntk_shim_download(scores, d_sc, (size_t)batch * sizeof(float)) : 0;
}

/* ---- beam search (csrc/hip/rnnt_beam.hip) on the same decoder handle ---- */

struct NntkRnntBeamStateStruct {
    NntkRnntDecoder dec;
    int batch, width, max_labels;
    nntk_shim_rnnt_beam_state d;                /* d.i: [batch][4], then [batch]: the rows of a reset */
    NntkNgramLm lm;                             /* the model the stream was created with (NULL: none), and */
    int *d_q;                                   /* [batch][width]: each hypothesis's state in it */
    int detail;                                 /* created with detail: the label frames and log-probabilities are carried, in */
    int *d_fr;                                  /* [batch][width][max_labels] and */
    float *d_lp;                                /* the same shape; the frames a row has consumed ride in d.i */
};

static int beam_check_sizes(const char *who, NntkRnntDecoder d, int beam_width, int max_labels) {
    if (!d) return dec_fail(who, "NULL decoder", 0, 0, 0);
    if (beam_width < 1 || beam_width > NNTK_RNNT_BEAM_MAX_W)
        return dec_fail(who, "beam_width %ld is outside [1, %ld]", beam_width, NNTK_RNNT_BEAM_MAX_W, 0);
    if (max_labels < 1) return dec_fail(who, "max_labels %ld < 1", max_labels, 0, 0);
    return 0;
}

static int beam_sizes_ok(NntkRnntDecoder d, int batch, int beam_width, int max_labels) {
    return d && batch > 0 && beam_width >= 1 && beam_width <= NNTK_RNNT_BEAM_MAX_W && max_labels >= 1;
}

/* the six public sizes: the bytes of a stream's state (state = 1) or the floats of a call's workspace; 0 where a call would be refused */
static size_t beam_size(NntkRnntDecoder d, int batch, int beam_width, int max_labels, int with_lm, int with_detail, int state) {
    if (!beam_sizes_ok(d, batch, beam_width, max_labels)) return 0;
    if (!state)
        return nntk_shim_rnnt_beam_workspace_floats(batch, d->cfg.H, d->cfg.J, d->cfg.V, d->cfg.max_symbols_per_frame, beam_width, max_labels,
                                                    with_lm, with_detail);
    const size_t per_hyp = sizeof(double) + (2 * (size_t)d->cfg.H + d->cfg.J) * sizeof(float) + ((size_t)max_labels + 2) * sizeof(int) +
                           (with_lm ? sizeof(int) : 0) + (with_detail ? max_labels * (sizeof(int) + sizeof(float)) : 0);
    return (size_t)batch * (beam_width * per_hyp + 5 * sizeof(int));
}

static int beam_opt_detail(const NntkRnntBeamOptions *o) { return o && (o->label_frames || o->label_logps); }

/* the kernels with detail also rank the report, so length normalisation alone takes them and their workspace */
static int beam_opt_kernel(const NntkRnntBeamOptions *o) { return beam_opt_detail(o) || (o && o->length_norm); }

size_t nntk_rnnt_beam_workspace_floats(NntkRnntDecoder d, int batch, int beam_width, int max_labels) {
    return beam_size(d, batch, beam_width, max_labels, 0, 0, 0);
}
size_t nntk_rnnt_beam_lm_workspace_floats(NntkRnntDecoder d, int batch, int beam_width, int max_labels) {
    return beam_size(d, batch, beam_width, max_labels, 1, 0, 0);
}
size_t nntk_rnnt_beam_opt_workspace_floats(NntkRnntDecoder d, int batch, int beam_width, int max_labels, const NntkRnntBeamOptions *o) {
    return beam_size(d, batch, beam_width, max_labels, o && o->lm, beam_opt_kernel(o), 0);
}

size_t nntk_rnnt_beam_state_bytes(NntkRnntDecoder d, int batch, int beam_width, int max_labels) {
    return beam_size(d, batch, beam_width, max_labels, 0, 0, 1);
}
size_t nntk_rnnt_beam_state_bytes_lm(NntkRnntDecoder d, int batch, int beam_width, int max_labels) {
    return beam_size(d, batch, beam_width, max_labels, 1, 0, 1);
}
size_t nntk_rnnt_beam_state_bytes_opt(NntkRnntDecoder d, int batch, int beam_width, int max_labels, int with_lm, int with_detail) {
    return beam_size(d, batch, beam_width, max_labels, with_lm, with_detail, 1);
}

static int beam_check_lm(const char *who, NntkRnntDecoder d, NntkNgramLm lm) {
    if (lm && !nntk_ngram_lm_matches(lm, d->cfg.V, d->cfg.blank))
        return dec_fail(who, "the language model was built for another class count or blank than V %ld, blank %ld", d->cfg.V, d->cfg.blank, 0);
    return 0;
}

static NntkRnntBeamState beam_state_create(const char *who, NntkRnntDecoder d, int batch, int beam_width, int max_labels, NntkNgramLm lm,
                                           int detail) {
    nntk_shim_clear_error();
    if (beam_check_sizes(who, d, beam_width, max_labels)) return NULL;
    if (batch < 1) { dec_fail(who, "batch %ld < 1", batch, 0, 0); return NULL; }
    if (beam_check_lm(who, d, lm)) return NULL;
    NntkRnntBeamState s = (NntkRnntBeamState)calloc(1, sizeof *s);
    if (!s) { nntk_set_error("nntk_rnnt_beam_state_create: out of host memory"); return NULL; }
    s->dec = d; s->batch = batch; s->width = beam_width; s->max_labels = max_labels; s->lm = lm; s->detail = detail != 0;
    const size_t hyps = (size_t)batch * beam_width;
    s->d.score = (double *)nntk_shim_malloc(hyps * sizeof(double));
    s->d.f = s->d.score ? (float *)nntk_shim_malloc(hyps * (2 * (size_t)d->cfg.H + d->cfg.J) * sizeof(float)) : NULL;
    s->d.lab = s->d.f ? (int *)nntk_shim_malloc(hyps * max_labels * sizeof(int)) : NULL;
    s->d.meta = s->d.lab ? (int *)nntk_shim_malloc(hyps * 2 * sizeof(int)) : NULL;
    s->d.i = s->d.meta ? (int *)nntk_shim_malloc((size_t)batch * 5 * sizeof(int)) : NULL;
    s->d_q = s->d.i && lm ? (int *)nntk_shim_malloc(hyps * sizeof(int)) : NULL;
    s->d_fr = s->d.i && detail ? (int *)nntk_shim_malloc(hyps * max_labels * sizeof(int)) : NULL;
    s->d_lp = s->d_fr ? (float *)nntk_shim_malloc(hyps * max_labels * sizeof(float)) : NULL;
    if (!s->d.i || (lm && !s->d_q) || (detail && !s->d_lp) || nntk_shim_memset(s->d.i, 0, (size_t)batch * 5 * sizeof(int))) {
        nntk_rnnt_beam_state_destroy(s);
        return NULL;
    }
    return s;
}

NntkRnntBeamState nntk_rnnt_beam_state_create(NntkRnntDecoder d, int batch, int beam_width, int max_labels) {
    return beam_state_create("nntk_rnnt_beam_state_create", d, batch, beam_width, max_labels, NULL, 0);
}

NntkRnntBeamState nntk_rnnt_beam_state_create_lm(NntkRnntDecoder d, int batch, int beam_width, int max_labels, NntkNgramLm lm) {
    return beam_state_create("nntk_rnnt_beam_state_create_lm", d, batch, beam_width, max_labels, lm, 0);
}

NntkRnntBeamState nntk_rnnt_beam_state_create_opt(NntkRnntDecoder d, int batch, int beam_width, int max_labels, NntkNgramLm lm, int with_detail) {
    return beam_state_create("nntk_rnnt_beam_state_create_opt", d, batch, beam_width, max_labels, lm, with_detail);
}

int nntk_rnnt_beam_state_reset(NntkRnntBeamState s, const int *rows, int n_rows) {
    return dec_state_reset("nntk_rnnt_beam_state_reset", s ? s->batch : 0, s ? s->d.i : NULL, rows, n_rows);
}

void nntk_rnnt_beam_state_destroy(NntkRnntBeamState s) {
    if (!s) return;
    if (s->d.score) nntk_shim_synchronize();
    nntk_shim_free(s->d.score);
    nntk_shim_free(s->d.f);
    nntk_shim_free(s->d.lab);
    nntk_shim_free(s->d.meta);
    nntk_shim_free(s->d.i);
    nntk_shim_free(s->d_q);
    nntk_shim_free(s->d_fr);
    nntk_shim_free(s->d_lp);
    free(s);
}

/* everything a beam call can be refused for; ws NULL: the host-pointer form, which owns its workspace; o NULL or o->lm NULL: the
 * acoustic search */
static int beam_check_call(const char *who, NntkRnntDecoder d, NntkRnntBeamState state, const float *enc, int batch, int T,
                           const int *n_frames, int beam_width, int nbest, int max_labels, const NntkRnntBeamOptions *o, const int *labels_out,
                           const int *out_lengths, const float *scores, const float *ws, int device_form) {
    NntkNgramLm lm = o ? o->lm : NULL;
    const int detail = beam_opt_detail(o);
    if (!d) return dec_fail(who, "NULL decoder", 0, 0, 0);
    if (o && o->length_norm != 0 && o->length_norm != 1) return dec_fail(who, "length_norm %ld is neither 0 nor 1", o->length_norm, 0, 0);
    if (state && state->detail != detail)
        return dec_fail(who, state->detail ? "the state was created with detail, the call asks for none"
                                           : "the state was created without detail, the call asks for it", 0, 0, 0);
    if (beam_check_lm(who, d, lm)) return -1;
    if (state && state->lm != lm)
        return dec_fail(who, !state->lm ? "the state was created without a language model" :
                             !lm ? "the state was created with a language model" : "the state was created with another language model", 0, 0, 0);
    if (batch < 0 || T < 0) return dec_fail(who, "batch %ld, T %ld: neither may be negative", batch, T, 0);
    if (beam_width < 1 || beam_width > NNTK_RNNT_BEAM_MAX_W)
        return dec_fail(who, "beam_width %ld is outside [1, %ld]", beam_width, NNTK_RNNT_BEAM_MAX_W, 0);
    if (nbest < 1 || nbest > beam_width) return dec_fail(who, "nbest %ld is outside [1, beam_width %ld]", nbest, beam_width, 0);
    if (max_labels < 1) return dec_fail(who, "max_labels %ld < 1", max_labels, 0, 0);
    if (state && state->dec != d) return dec_fail(who, "the state belongs to another decoder", 0, 0, 0);
    if (state && state->batch != batch) return dec_fail(who, "batch %ld differs from the state's %ld", batch, state->batch, 0);
    if (state && state->width != beam_width)
        return dec_fail(who, "beam_width %ld differs from the state's %ld", beam_width, state->width, 0);
    if (state && state->max_labels != max_labels)
        return dec_fail(who, "max_labels %ld differs from the state's %ld", max_labels, state->max_labels, 0);
    if (batch == 0) return 0;
    for (int b = 0; n_frames && b < batch; ++b)
        if (n_frames[b] < 0 || n_frames[b] > T) return dec_fail(who, "n_frames[%ld] = %ld is outside [0, %ld]", b, n_frames[b], T);
    if (T > 0 && dec_named_ptr(who, "enc", enc)) return -1;
    if (dec_named_ptr(who, "labels_out", labels_out) || dec_named_ptr(who, "out_lengths", out_lengths) ||
        dec_named_ptr(who, "scores", scores)) return -1;
    if (o && o->label_frames && dec_named_ptr(who, "label_frames", o->label_frames)) return -1;
    if (o && o->label_logps && dec_named_ptr(who, "label_logps", o->label_logps)) return -1;
    if (device_form && (!ws || ((uintptr_t)ws & 15)))
        return dec_fail(who, ws ? "workspace is not 16-byte aligned" : "workspace is NULL", 0, 0, 0);
    const size_t nh = (size_t)batch * nbest;
    const void *p[7] = { labels_out, out_lengths, scores, o ? o->label_frames : NULL, o ? o->label_logps : NULL, enc, ws };
    const size_t n[7] = { nh * max_labels * sizeof(int), nh * sizeof(int), nh * sizeof(float), nh * max_labels * sizeof(int),
                          nh * max_labels * sizeof(float), (size_t)batch * T * d->cfg.J * sizeof(float),
                          !device_form ? 0 : nntk_rnnt_beam_opt_workspace_floats(d, batch, beam_width, max_labels, o) * sizeof(float) };
    static const char *const name[7] = { "labels_out", "out_lengths", "scores", "label_frames", "label_logps", "enc", "workspace" };
    if (dec_check_overlaps(who, 5, 7, p, n, name)) return -1;
    if (!nntk_shim_rnnt_beam_fits(d->cfg.H, d->cfg.J, d->cfg.V))
        return dec_fail(who, "the model (H %ld, J %ld, V %ld) is beyond the beam kernel's LDS", d->cfg.H, d->cfg.J, d->cfg.V);
    return 0;
}

static int beam_decode_device(const char *who, NntkRnntDecoder d, NntkRnntBeamState state, const float *d_enc, int batch, int T,
                              const int *n_frames, int beam_width, int nbest, int max_labels, const NntkRnntBeamOptions *o, int *d_labels_out,
                              int *d_out_lengths, float *d_scores, float *d_workspace) {
    nntk_shim_clear_error();
    if (beam_check_call(who, d, state, d_enc, batch, T, n_frames, beam_width, nbest, max_labels, o, d_labels_out, d_out_lengths, d_scores,
                        d_workspace, 1)) return -1;
    if (batch == 0) return 0;
    NntkNgramLm lm = o ? o->lm : NULL;
    nntk_shim_rnnt_lm tab;
    if (lm && nntk_ngram_lm_rnnt_device(lm, &tab)) return -1;
    int *len = dec_row_frames("nntk_rnnt_beam_decode_device: out of host memory", n_frames, batch, T);
    if (!len) return -1;
    const nntk_shim_rnnt_dec m = dec_model(d);
    const nntk_shim_rnnt_beam_detail dt = { o ? o->label_frames : NULL, o ? o->label_logps : NULL, state ? state->d_fr : NULL,
                                            state ? state->d_lp : NULL, o ? o->length_norm : 0 };
    int rc = nntk_shim_rnnt_beam(&m, d_enc, batch, T, len, beam_width, nbest, max_labels, state ? &state->d : NULL, lm ? &tab : NULL,
                                 state && lm ? state->d_q : NULL, beam_opt_kernel(o) ? &dt : NULL, d_labels_out, d_out_lengths, d_scores,
                                 d_workspace);
    free(len);
    return rc;
}

int nntk_rnnt_beam_decode_device(NntkRnntDecoder d, NntkRnntBeamState state, const float *d_enc, int batch, int T, const int *n_frames,
                                 int beam_width, int nbest, int max_labels, int *d_labels_out, int *d_out_lengths, float *d_scores,
                                 float *d_workspace) {
    return beam_decode_device("nntk_rnnt_beam_decode_device", d, state, d_enc, batch, T, n_frames, beam_width, nbest, max_labels, NULL,
                              d_labels_out, d_out_lengths, d_scores, d_workspace);
}

int nntk_rnnt_beam_decode_opt_device(NntkRnntDecoder d, NntkRnntBeamState state, const float *d_enc, int batch, int T, const int *n_frames,
                                     int beam_width, int nbest, int max_labels, const NntkRnntBeamOptions *o, int *d_labels_out,
                                     int *d_out_lengths, float *d_scores, float *d_workspace) {
    return beam_decode_device("nntk_rnnt_beam_decode_opt_device", d, state, d_enc, batch, T, n_frames, beam_width, nbest, max_labels, o,
                              d_labels_out, d_out_lengths, d_scores, d_workspace);
}

int nntk_rnnt_beam_decode_lm_device(NntkRnntDecoder d, NntkRnntBeamState state, const float *d_enc, int batch, int T, const int *n_frames,
                                    int beam_width, int nbest, int max_labels, NntkNgramLm lm, int *d_labels_out, int *d_out_lengths,
                                    float *d_scores, float *d_workspace) {
    const NntkRnntBeamOptions o = { lm, 0, NULL, NULL };
    return beam_decode_device("nntk_rnnt_beam_decode_lm_device", d, state, d_enc, batch, T, n_frames, beam_width, nbest, max_labels, &o,
                              d_labels_out, d_out_lengths, d_scores, d_workspace);
}

static int beam_decode_host(const char *who, NntkRnntDecoder d, NntkRnntBeamState state, const float *enc, int batch, int T,
                            const int *n_frames, int beam_width, int nbest, int max_labels, const NntkRnntBeamOptions *o, int *labels_out,
                            int *out_lengths, float *scores) {
    nntk_shim_clear_error();
    if (beam_check_call(who, d, state, enc, batch, T, n_frames, beam_width, nbest, max_labels, o, labels_out, out_lengths, scores, NULL, 0))
        return -1;
    if (batch == 0) return 0;
    const size_t ne = (size_t)batch * T * d->cfg.J, nh = (size_t)batch * nbest, nl = nh * max_labels;
    const int detail = beam_opt_detail(o);
    float *d_enc = nntk_devbuf_reserve(&t_a, ne + 4);
    int *d_lab = (int *)nntk_devbuf_reserve(&t_b, (detail ? 3 : 1) * nl + 2 * nh + 4);
    float *d_ws = nntk_devbuf_reserve(nntk_thread_scratch(NNTK_TS_C), nntk_rnnt_beam_opt_workspace_floats(d, batch, beam_width, max_labels, o));
    if (!d_enc || !d_lab || !d_ws) return -1;
    int *d_len = d_lab + nl;
    float *d_sc = (float *)(d_len + nh);
    NntkRnntBeamOptions dev = { NULL, 0, NULL, NULL };                /* o with the detail outputs in device memory, behind the scores */
    if (o) dev = *o;
    if (detail) {
        dev.label_frames = o->label_frames ? (int *)(d_sc + nh) : NULL;
        dev.label_logps = o->label_logps ? d_sc + nh + nl : NULL;
    }
    if (ne && nntk_shim_upload(d_enc, enc, ne * sizeof(float))) return -1;
    if (beam_decode_device(who, d, state, d_enc, batch, T, n_frames, beam_width, nbest, max_labels, o ? &dev : NULL, d_lab, d_len, d_sc, d_ws))
        return -1;
    if (nntk_shim_download(labels_out, d_lab, nl * sizeof(int))) return -1;
    if (nntk_shim_download(out_lengths, d_len, nh * sizeof(int))) return -1;
    if (dev.label_frames && nntk_shim_download(o->label_frames, dev.label_frames, nl * sizeof(int))) return -1;
    if (dev.label_logps && nntk_shim_download(o->label_logps, dev.label_logps, nl * sizeof(float))) return -1;
    return nntk_shim_download(scores, d_sc, nh * sizeof(float));
}

int nntk_rnnt_beam_decode_opt(NntkRnntDecoder d, NntkRnntBeamState state, const float *enc, int batch, int T, const int *n_frames,
                              int beam_width, int nbest, int max_labels, const NntkRnntBeamOptions *o, int *labels_out, int *out_lengths,
                              float *scores) {
    return beam_decode_host("nntk_rnnt_beam_decode_opt", d, state, enc, batch, T, n_frames, beam_width, nbest, max_labels, o, labels_out,
                            out_lengths, scores);
}

int nntk_rnnt_beam_decode(NntkRnntDecoder d, NntkRnntBeamState state, const float *enc, int batch, int T, const int *n_frames,
                          int beam_width, int nbest, int max_labels, int *labels_out, int *out_lengths, float *scores) {
    return beam_decode_host("nntk_rnnt_beam_decode", d, state, enc, batch, T, n_frames, beam_width, nbest, max_labels, NULL, labels_out,
                            out_lengths, scores);
}

int nntk_rnnt_beam_decode_lm(NntkRnntDecoder d, NntkRnntBeamState state, const float *enc, int batch, int T, const int *n_frames,
                             int beam_width, int nbest, int max_labels, NntkNgramLm lm, int *labels_out, int *out_lengths, float *scores) {
    const NntkRnntBeamOptions o = { lm, 0, NULL, NULL };
    return beam_decode_host("nntk_rnnt_beam_decode_lm", d, state, enc, batch, T, n_frames, beam_width, nbest, max_labels, &o, labels_out,
                            out_lengths, scores);
}
