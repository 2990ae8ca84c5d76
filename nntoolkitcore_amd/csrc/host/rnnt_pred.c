/*
 * rnnt_pred.c -- host layer of the transducer's prediction network in training: the label embedding (csrc/hip/rnnt_pred.hip: lookup and
 * table gradient) and the predictor handle, which composes the lookup, a training-mode LSTM and a training-mode TimeDistributedDense
 * from the library's own calls and adds nothing to their arithmetic.  Every argument is checked here, before anything is allocated,
 * uploaded or enqueued: a refusal needs no device and writes nothing.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "nntk_internal.h"

#define PRED_STR_(x) #x
#define PRED_STR(x) PRED_STR_(x)
#define PRED_MAX_WIDTH NNTK_RNNT_DEC_MAX_WIDTH      /* E, H, J: the decoder's limits */
#define PRED_MAX_V NNTK_RNNT_DEC_MAX_V

static int pred_fail(const char *who, const char *fmt, long a, long b, long c) {
    char msg[240];
    int n = snprintf(msg, sizeof msg, "%s: ", who);
    snprintf(msg + n, sizeof msg - (size_t)n, fmt, a, b, c);
    nntk_set_error(msg);
    return -1;
}

static int pred_ptr(const char *who, const char *name, const void *p, unsigned align) {
    char msg[240];
    if (p && ((uintptr_t)p & (align - 1)) == 0) return 0;
    if (p) snprintf(msg, sizeof msg, "%s: %s is not %u-byte aligned", who, name, align);
    else snprintf(msg, sizeof msg, "%s: %s is NULL", who, name);
    nntk_set_error(msg);
    return -1;
}

static int pred_overlap(const void *a, size_t na, const void *b, size_t nb) {
    return a && b && na && nb && (uintptr_t)a < (uintptr_t)b + nb && (uintptr_t)b < (uintptr_t)a + na;
}

/* ---- the embedding ---- */
static int embed_check(const char *who, int V, int E, int rows, const int *ids) {
    if (V < 1) return pred_fail(who, "V %ld < 1", V, 0, 0);
    if (E < 1 || E > PRED_MAX_WIDTH) return pred_fail(who, "E %ld is outside [1, " PRED_STR(NNTK_RNNT_DEC_MAX_WIDTH) "]", E, 0, 0);
    if (rows < 0) return pred_fail(who, "rows %ld < 0", rows, 0, 0);
    if (rows > 0 && !ids) return pred_fail(who, "ids is NULL", 0, 0, 0);
    for (int r = 0; r < rows; ++r)
        if (ids[r] < -1 || ids[r] >= V) return pred_fail(who, "ids[%ld] = %ld is outside [-1, %ld)", r, ids[r], V);
    return 0;
}

int nntk_embedding_lookup_device(const float *d_table, int V, int E, const int *ids, int rows, float *d_out) {
    static const char who[] = "nntk_embedding_lookup_device";
    nntk_shim_clear_error();
    if (embed_check(who, V, E, rows, ids)) return -1;
    if (rows == 0) return 0;
    if (pred_ptr(who, "d_table", d_table, 4) || pred_ptr(who, "d_out", d_out, 4)) return -1;
    if (pred_overlap(d_table, (size_t)V * E * sizeof(float), d_out, (size_t)rows * E * sizeof(float)))
        return pred_fail(who, "d_out overlaps d_table", 0, 0, 0);
    return nntk_shim_rows_select(d_table, E, ids, rows, d_out);
}

size_t nntk_embedding_workspace_floats(int rows, int V, int E) { return nntk_shim_embedding_workspace_floats(rows, V, E); }

/* Stable counting sort of the row numbers by id, O(rows + V): offsets [V + 1], the rows of id v are sorted_rows[offsets[v] ..
 * offsets[v + 1]) in ascending order; rows with id -1 are in no list.  Returns offsets[V], the rows listed, or -1. */
int nntk_embedding_sort_ids(const int *ids, int rows, int V, int *offsets, int *sorted_rows) {
    static const char who[] = "nntk_embedding_sort_ids";
    nntk_shim_clear_error();
    if (V < 1) return pred_fail(who, "V %ld < 1", V, 0, 0);
    if (rows < 0) return pred_fail(who, "rows %ld < 0", rows, 0, 0);
    if (!offsets || (rows > 0 && (!ids || !sorted_rows))) return pred_fail(who, "a NULL array", 0, 0, 0);
    for (int r = 0; r < rows; ++r)
        if (ids[r] < -1 || ids[r] >= V) return pred_fail(who, "ids[%ld] = %ld is outside [-1, %ld)", r, ids[r], V);
    memset(offsets, 0, ((size_t)V + 1) * sizeof(int));
    for (int r = 0; r < rows; ++r)
        if (ids[r] >= 0) ++offsets[ids[r] + 1];
    for (int v = 0; v < V; ++v) offsets[v + 1] += offsets[v];
    /* offsets[v] serves as the cursor of id v, then moves back by the id's count */
    for (int r = 0; r < rows; ++r)
        if (ids[r] >= 0) sorted_rows[offsets[ids[r]]++] = r;
    for (int v = V; v > 0; --v) offsets[v] = offsets[v - 1];
    offsets[0] = 0;
    return offsets[V];
}

int nntk_embedding_gradient_device(const float *d_dout, const int *ids, int rows, int V, int E, float *d_dtable, float *d_workspace) {
    static const char who[] = "nntk_embedding_gradient_device";
    nntk_shim_clear_error();
    if (embed_check(who, V, E, rows, ids)) return -1;
    if (pred_ptr(who, "d_dtable", d_dtable, 4) || pred_ptr(who, "d_workspace", d_workspace, 16)) return -1;
    if (rows > 0 && pred_ptr(who, "d_dout", d_dout, 4)) return -1;
    const size_t nt = (size_t)V * E * sizeof(float), nd = (size_t)rows * E * sizeof(float);
    const size_t nw = nntk_shim_embedding_workspace_floats(rows, V, E) * sizeof(float);
    if (pred_overlap(d_dtable, nt, d_dout, nd)) return pred_fail(who, "d_dtable overlaps d_dout", 0, 0, 0);
    if (pred_overlap(d_workspace, nw, d_dtable, nt) || pred_overlap(d_workspace, nw, d_dout, nd))
        return pred_fail(who, "d_workspace overlaps d_dtable or d_dout", 0, 0, 0);
    /* the plan: offsets | sorted rows | heavy chunks (id, chunk) | heavy ids (id, first partial slot), nntk_shim.h */
    /* an id of n > C rows has ceil(n / C) <= n / 16 chunks, and at most rows / (C + 1) ids are heavy */
    const size_t cap = (size_t)V + 1 + (size_t)rows + 2 * ((size_t)rows / 16 + 1) + 2 * ((size_t)rows / (NNTK_EMBED_CHUNK + 1) + 1);
    int *plan = (int *)malloc(cap * sizeof(int));
    if (!plan) return pred_fail(who, "out of host memory", 0, 0, 0);
    int *offsets = plan, *sorted = plan + V + 1;
    const int n_sorted = nntk_embedding_sort_ids(ids, rows, V, offsets, sorted);
    long n_items = 0, n_heavy = 0;
    for (int v = 0; v < V; ++v)
        if (offsets[v + 1] - offsets[v] > NNTK_EMBED_CHUNK) {
            n_items += (offsets[v + 1] - offsets[v] + NNTK_EMBED_CHUNK - 1) / NNTK_EMBED_CHUNK;
            ++n_heavy;
        }
    int *items = sorted + n_sorted, *heavy = items + 2 * n_items;
    long slot = 0;
    for (int v = 0; v < V; ++v) {
        const int n = offsets[v + 1] - offsets[v];
        if (n <= NNTK_EMBED_CHUNK) continue;
        *heavy++ = v;
        *heavy++ = (int)slot;
        for (int c = 0; c * NNTK_EMBED_CHUNK < n; ++c, ++slot) {
            items[2 * slot] = v;
            items[2 * slot + 1] = c;
        }
    }
    int rc = nntk_shim_embedding_grad(d_dout, V, E, plan, n_sorted, n_items, n_heavy, d_dtable, d_workspace);
    free(plan);
    return rc;
}

/* ---- the predictor handle ---- */
struct NntkRnntPredictorStruct {
    NntkRnntPredictorConfig cfg;
    LSTMActivations acts;
    LSTM lstm;
    TimeDistributedDense proj;                  /* NULL: identity */
    float *d_embed;                             /* [V][E], the handle's copy */
    float *d_x, *d_dx;                          /* [batch][U1][E] */
    float *d_h, *d_dh;                          /* [batch][U1][H], with a projection */
    float *d_dpm;                               /* [batch][U1][J]: d_dpred with the padding rows zeroed, with a projection */
    float *d_ws;                                /* nntk_embedding_workspace_floats(batch U1, V, E) */
    int *ids, *live, *lens;                     /* host: [batch][U1] input token or -1; row number or -1; [batch] U_b + 1 */
    size_t bytes;
    int loaded, forward_done;
};

static int pred_check_config(const char *who, const NntkRnntPredictorConfig *c) {
    if (c->V < 2) return pred_fail(who, "V %ld < 2: a transducer has the blank and at least one label", c->V, 0, 0);
    if (c->V > PRED_MAX_V) return pred_fail(who, "V %ld is above the limit %ld", c->V, PRED_MAX_V, 0);
    if (c->blank < 0 || c->blank >= c->V) return pred_fail(who, "blank %ld is outside [0, %ld)", c->blank, c->V, 0);
    if (c->E < 1 || c->H < 1 || c->J < 1) return pred_fail(who, "E %ld, H %ld, J %ld: each must be at least 1", c->E, c->H, c->J);
    if (c->E > PRED_MAX_WIDTH || c->H > PRED_MAX_WIDTH || c->J > PRED_MAX_WIDTH)
        return pred_fail(who, "E %ld, H %ld, J %ld: one is above the limit " PRED_STR(NNTK_RNNT_DEC_MAX_WIDTH), c->E, c->H, c->J);
    if (c->has_proj != 0 && c->has_proj != 1) return pred_fail(who, "has_proj %ld is neither 0 nor 1", c->has_proj, 0, 0);
    if (!c->has_proj && c->H != c->J) return pred_fail(who, "no projection (identity) but H %ld != J %ld", c->H, c->J, 0);
    if (c->batch < 1) return pred_fail(who, "batch %ld < 1", c->batch, 0, 0);
    if (c->max_label_len < 0) return pred_fail(who, "max_label_len %ld < 0", c->max_label_len, 0, 0);
    if ((long long)c->batch * (c->max_label_len + 1LL) > INT32_MAX / PRED_MAX_WIDTH)
        return pred_fail(who, "batch %ld x (max_label_len %ld + 1) rows are beyond 32-bit tensor sizes", c->batch, c->max_label_len, 0);
    return 0;
}

static float *pred_dev(NntkRnntPredictor p, size_t n_floats) {
    float *d = (float *)nntk_shim_malloc(n_floats * sizeof(float));
    if (d) p->bytes += n_floats * sizeof(float);
    return d;
}

NntkRnntPredictor nntk_rnnt_predictor_create(NntkRnntPredictorConfig cfg) {
    static const char who[] = "nntk_rnnt_predictor_create";
    nntk_shim_clear_error();
    if (pred_check_config(who, &cfg)) return NULL;
    NntkRnntPredictor p = (NntkRnntPredictor)calloc(1, sizeof *p);
    if (!p) { nntk_set_error("nntk_rnnt_predictor_create: out of host memory"); return NULL; }
    p->cfg = cfg;
    const int U1 = cfg.max_label_len + 1;
    const size_t rows = (size_t)cfg.batch * U1;
    const DefaultTrainingConfig tc = { cfg.batch };
    p->acts = LSTMActivationsCreateDefault(cfg.H);
    p->lstm = LSTMCreateForTraining(LSTMConfigCreate(cfg.E, cfg.H, true, U1, true, p->acts), tc);
    if (p->lstm && cfg.has_proj)
        p->proj = TimeDistributedDenseCreateForTraining(TimeDistributedDenseConfigCreate(U1, DenseConfigCreate(cfg.H, cfg.J, NULL)), tc);
    p->ids = (int *)malloc(rows * sizeof(int));
    p->live = (int *)malloc(rows * sizeof(int));
    p->lens = (int *)malloc((size_t)cfg.batch * sizeof(int));
    if (!p->lstm || (cfg.has_proj && !p->proj)) goto fail;             /* the layer's own message stands */
    if (!p->ids || !p->live || !p->lens) { nntk_set_error("nntk_rnnt_predictor_create: out of host memory"); goto fail; }
    if (!(p->d_embed = pred_dev(p, (size_t)cfg.V * cfg.E)) || !(p->d_x = pred_dev(p, rows * cfg.E)) || !(p->d_dx = pred_dev(p, rows * cfg.E)) ||
        !(p->d_ws = pred_dev(p, nntk_shim_embedding_workspace_floats((long)rows, cfg.V, cfg.E)))) goto fail;
    if (cfg.has_proj && (!(p->d_h = pred_dev(p, rows * cfg.H)) || !(p->d_dh = pred_dev(p, rows * cfg.H)) || !(p->d_dpm = pred_dev(p, rows * cfg.J))))
        goto fail;
    return p;
fail:
    nntk_rnnt_predictor_destroy(p);
    return NULL;
}

size_t nntk_rnnt_predictor_device_bytes(NntkRnntPredictor p) { return p ? p->bytes : 0; }

void nntk_rnnt_predictor_destroy(NntkRnntPredictor p) {
    if (!p) return;
    if (p->d_embed) nntk_shim_synchronize();
    if (p->proj) TimeDistributedDenseDestroy(p->proj);
    if (p->lstm) LSTMDestroy(p->lstm);
    LSTMActivationsDestroy(p->acts);
    nntk_shim_free(p->d_embed);
    nntk_shim_free(p->d_x);
    nntk_shim_free(p->d_dx);
    nntk_shim_free(p->d_h);
    nntk_shim_free(p->d_dh);
    nntk_shim_free(p->d_dpm);
    nntk_shim_free(p->d_ws);
    free(p->ids);
    free(p->live);
    free(p->lens);
    free(p);
}

/* the projection pointer of a call is given exactly when the handle has a projection */
static int pred_check_proj(const char *who, NntkRnntPredictor p, const char *name, const void *ptr) {
    char msg[240];
    if ((ptr != NULL) == (p->cfg.has_proj != 0)) return ptr ? pred_ptr(who, name, ptr, 4) : 0;
    snprintf(msg, sizeof msg, "%s: %s must be given exactly when the predictor has a projection (has_proj %d)", who, name, p->cfg.has_proj);
    nntk_set_error(msg);
    return -1;
}

int nntk_rnnt_predictor_load_weights_device(NntkRnntPredictor p, const float *d_embed, const float *d_lstm, const float *d_pred_proj) {
    static const char who[] = "nntk_rnnt_predictor_load_weights_device";
    nntk_shim_clear_error();
    if (!p) return pred_fail(who, "NULL handle", 0, 0, 0);
    if (pred_ptr(who, "d_embed", d_embed, 4) || pred_ptr(who, "d_lstm", d_lstm, 4) || pred_check_proj(who, p, "d_pred_proj", d_pred_proj)) return -1;
    if (nntk_shim_copy_d2d(p->d_embed, d_embed, (size_t)p->cfg.V * p->cfg.E * sizeof(float))) return -1;
    /* the layers' loads wait for the stream: the caller's blocks are free for reuse on return */
    if (LSTMLoadWeightsDevice(p->lstm, d_lstm)) return -1;
    if (p->proj && TimeDistributedDenseLoadWeightsDevice(p->proj, d_pred_proj)) return -1;
    p->loaded = 1;
    return 0;
}

int nntk_rnnt_predictor_forward_device(NntkRnntPredictor p, const int *labels, const int *label_lengths, float *d_pred) {
    static const char who[] = "nntk_rnnt_predictor_forward_device";
    nntk_shim_clear_error();
    if (!p) return pred_fail(who, "NULL handle", 0, 0, 0);
    const NntkRnntPredictorConfig *c = &p->cfg;
    const int B = c->batch, maxL = c->max_label_len, U1 = maxL + 1;
    if (!p->loaded) return pred_fail(who, "no weights: call nntk_rnnt_predictor_load_weights_device first", 0, 0, 0);
    if (maxL > 0 && !labels) return pred_fail(who, "labels is NULL", 0, 0, 0);
    if (pred_ptr(who, "d_pred", d_pred, 4)) return -1;
    for (int b = 0; b < B; ++b) {
        const int L = label_lengths ? label_lengths[b] : maxL;
        if (L < 0 || L > maxL) return pred_fail(who, "label_lengths[%ld] = %ld is outside [0, %ld]", b, L, maxL);
        for (int i = 0; i < L; ++i) {
            const int k = labels[(size_t)b * maxL + i];
            if (k < 0 || k >= c->V) return pred_fail(who, "labels[%ld][%ld] = %ld is not a class", b, i, k);
            if (k == c->blank) return pred_fail(who, "labels[%ld][%ld] is the blank (%ld)", b, i, k);
        }
    }
    /* nothing of the last forward is overwritten before this point: a refused call leaves the handle's backward intact */
    p->forward_done = 0;
    for (int b = 0; b < B; ++b) {
        const int L = label_lengths ? label_lengths[b] : maxL;
        int *ids = p->ids + (size_t)b * U1, *live = p->live + (size_t)b * U1;
        p->lens[b] = L + 1;
        for (int u = 0; u < U1; ++u) {
            ids[u] = u == 0 ? c->blank : u <= L ? labels[(size_t)b * maxL + u - 1] : -1;
            live[u] = u <= L ? b * U1 + u : -1;
        }
    }
    if (nntk_embedding_lookup_device(p->d_embed, c->V, c->E, p->ids, B * U1, p->d_x)) return -1;
    if (LSTMApplyTrainingBatchDeviceVarLen(p->lstm, p->d_x, p->proj ? p->d_h : d_pred, p->lens, NULL, NULL, NULL, NULL)) return -1;
    if (p->proj && TimeDistributedDenseApplyTrainingBatchDevice(p->proj, p->d_h, d_pred)) return -1;
    p->forward_done = 1;
    return 0;
}

int nntk_rnnt_predictor_backward_device(NntkRnntPredictor p, const float *d_dpred, float *d_dembed, float *d_dlstm, float *d_dproj) {
    static const char who[] = "nntk_rnnt_predictor_backward_device";
    nntk_shim_clear_error();
    if (!p) return pred_fail(who, "NULL handle", 0, 0, 0);
    const NntkRnntPredictorConfig *c = &p->cfg;
    const int rows = c->batch * (c->max_label_len + 1);
    if (!p->forward_done) return pred_fail(who, "no forward pass to differentiate: call nntk_rnnt_predictor_forward_device first", 0, 0, 0);
    if (pred_ptr(who, "d_dpred", d_dpred, 4) || pred_ptr(who, "d_dembed", d_dembed, 4) || pred_ptr(who, "d_dlstm", d_dlstm, 4) ||
        pred_check_proj(who, p, "d_dproj", d_dproj)) return -1;
    const size_t n_lstm = 4 * (size_t)c->H * ((size_t)c->E + c->H + 2), n_proj = ((size_t)c->H + 1) * c->J;
    const float *d_dh = d_dpred;
    if (p->proj) {
        /* the Dense gradient sums over every row: the padding rows of d_dpred (they may hold NaN) become exact zeros first */
        if (nntk_shim_rows_select(d_dpred, c->J, p->live, rows, p->d_dpm)) return -1;
        if (nntk_shim_memset(d_dproj, 0, n_proj * sizeof(float))) return -1;
        if (TimeDistributedDenseCalculateGradientDevice(p->proj, d_dproj, p->d_dh, p->d_dpm)) return -1;
        d_dh = p->d_dh;
    }
    if (nntk_shim_memset(d_dlstm, 0, n_lstm * sizeof(float))) return -1;
    if (LSTMCalculateGradientDeviceVarLen(p->lstm, d_dlstm, p->d_dx, d_dh, NULL, NULL, NULL, NULL)) return -1;
    return nntk_embedding_gradient_device(p->d_dx, p->ids, rows, c->V, c->E, d_dembed, p->d_ws);
}
