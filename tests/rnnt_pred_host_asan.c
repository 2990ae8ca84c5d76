/*
 * A stand-alone program over the host side of csrc/host/rnnt_pred.c, for -fsanitize=address,undefined on the CPU
 * (tests/test_rnnt_predictor_host.py compiles it together with that file and runs it).  Everything below the host layer is a stub: the
 * stub of the gradient launcher walks the whole plan the host built, at its exact malloc'd size, and checks it against the ids.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "nntk_internal.h"

static char g_err[256];
void nntk_set_error(const char *msg) { snprintf(g_err, sizeof g_err, "%s", msg); }
void nntk_shim_clear_error(void) { g_err[0] = 0; }
void *nntk_shim_malloc(size_t bytes) { return NULL; }
void nntk_shim_free(void *p) {}
int nntk_shim_synchronize(void) { return 0; }
int nntk_shim_copy_d2d(void *d, const void *s, size_t n) { return 0; }
int nntk_shim_memset(void *d, int v, size_t n) { return 0; }
int nntk_shim_rows_select(const float *s, int w, const int *idx, long rows, float *o) { return 0; }
size_t nntk_shim_embedding_workspace_floats(long rows, int V, int E) { return 16; }
LSTMActivations LSTMActivationsCreateDefault(int size) { LSTMActivations a; memset(&a, 0, sizeof a); return a; }
void LSTMActivationsDestroy(LSTMActivations a) {}
LSTMConfig LSTMConfigCreate(int i, int o, bool rs, int t, bool v2, LSTMActivations a) { LSTMConfig c; memset(&c, 0, sizeof c); return c; }
LSTM LSTMCreateForTraining(LSTMConfig c, LSTMTrainingConfig t) { return NULL; }
void LSTMDestroy(LSTM f) {}
int LSTMLoadWeightsDevice(LSTM f, const float *b) { return 0; }
int LSTMApplyTrainingBatchDeviceVarLen(LSTM f, const float *x, float *o, const int *l, const float *h0, const float *c0, float *hT, float *cT) { return 0; }
int LSTMCalculateGradientDeviceVarLen(LSTM f, float *g, float *dx, const float *d, const float *a, const float *b, float *c, float *e) { return 0; }
DenseConfig DenseConfigCreate(int i, int o, ActivationFunction a) { DenseConfig c; memset(&c, 0, sizeof c); return c; }
TimeDistributedDenseConfig TimeDistributedDenseConfigCreate(int ts, DenseConfig d) { TimeDistributedDenseConfig c; memset(&c, 0, sizeof c); return c; }
TimeDistributedDense TimeDistributedDenseCreateForTraining(TimeDistributedDenseConfig c, TimeDistributedDenseTrainingConfig t) { return NULL; }
void TimeDistributedDenseDestroy(TimeDistributedDense f) {}
int TimeDistributedDenseLoadWeightsDevice(TimeDistributedDense f, const float *b) { return 0; }
int TimeDistributedDenseApplyTrainingBatchDevice(TimeDistributedDense f, const float *x, float *o) { return 0; }
int TimeDistributedDenseCalculateGradientDevice(TimeDistributedDense f, float *g, float *dx, const float *d) { return 0; }

static const int *g_ids;
static int g_rows, g_plans;

#define REQUIRE(c) do { if (!(c)) { fprintf(stderr, "line %d: %s\n", __LINE__, #c); exit(1); } } while (0)

int nntk_shim_embedding_grad(const float *d_dout, int V, int E, const int *plan, long n_sorted, long n_items, long n_heavy, float *d_dtable,
                             float *d_ws) {
    const int *off = plan, *sorted = plan + V + 1, *items = sorted + n_sorted, *heavy = items + 2 * n_items;
    long live = 0, slot = 0, h = 0;
    for (int r = 0; r < g_rows; ++r) live += g_ids[r] >= 0;
    REQUIRE(off[0] == 0 && off[V] == n_sorted && n_sorted == live);
    for (int v = 0; v < V; ++v) {
        const int n = off[v + 1] - off[v];
        REQUIRE(n >= 0);
        for (int i = off[v]; i < off[v + 1]; ++i) {
            REQUIRE(sorted[i] >= 0 && sorted[i] < g_rows && g_ids[sorted[i]] == v);
            REQUIRE(i == off[v] || sorted[i - 1] < sorted[i]);
        }
        if (n <= NNTK_EMBED_CHUNK) continue;
        REQUIRE(h < n_heavy && heavy[2 * h] == v && heavy[2 * h + 1] == slot);
        ++h;
        for (int c = 0; c * NNTK_EMBED_CHUNK < n; ++c, ++slot) REQUIRE(slot < n_items && items[2 * slot] == v && items[2 * slot + 1] == c);
    }
    REQUIRE(h == n_heavy && slot == n_items && n_items <= g_rows / 16);
    ++g_plans;
    return 0;
}

static unsigned g_seed = 12345;
static int rnd(int n) { g_seed = g_seed * 1664525u + 1013904223u; return (int)((g_seed >> 8) % (unsigned)n); }

int main(void) {
    float *table = (float *)0x100000, *out = (float *)0x200000, *ws = (float *)0x300000;
    /* the plan of the gradient call, on id distributions from all-padding to one id taking every row */
    const int shapes[][3] = { {0, 1, 0}, {1, 1, 0}, {33, 1, 0}, {300, 8, 10}, {2624, 1024, 5}, {2624, 4096, 0}, {64, 2, 0}, {65, 3, 100}, {4097, 2, 1} };
    for (size_t s = 0; s < sizeof shapes / sizeof shapes[0]; ++s) {
        const int rows = shapes[s][0], V = shapes[s][1], pad = shapes[s][2];
        int *ids = (int *)malloc((size_t)(rows ? rows : 1) * sizeof(int));
        for (int r = 0; r < rows; ++r) ids[r] = rnd(100) < pad ? -1 : (r % 3 == 0 ? 0 : rnd(V));
        g_ids = ids; g_rows = rows;
        REQUIRE(nntk_embedding_gradient_device(rows ? table : NULL, ids, rows, V, 4, out, ws) == 0);
        int *off = (int *)malloc(((size_t)V + 1) * sizeof(int)), *srt = (int *)malloc((size_t)(rows ? rows : 1) * sizeof(int));
        REQUIRE(nntk_embedding_sort_ids(ids, rows, V, off, srt) == off[V]);
        free(off); free(srt); free(ids);
    }
    REQUIRE(g_plans == (int)(sizeof shapes / sizeof shapes[0]));
    /* refusals: none reaches a stub that would count a plan */
    int ids[3] = { 0, 4, -1 }, bad[3] = { 0, 5, 1 };
    REQUIRE(nntk_embedding_lookup_device(table, 5, 8, ids, 3, out) == 0);
    REQUIRE(nntk_embedding_lookup_device(table, 5, 8, bad, 3, out) == -1 && strstr(g_err, "ids[1] = 5"));
    REQUIRE(nntk_embedding_lookup_device(NULL, 5, 8, ids, 3, out) == -1 && strstr(g_err, "NULL"));
    REQUIRE(nntk_embedding_gradient_device(table, bad, 3, 5, 8, out, ws) == -1 && nntk_embedding_gradient_device(table, ids, 3, 5, 8, out, ws + 1) == -1);
    REQUIRE(nntk_embedding_gradient_device(table, ids, 3, 5, 8, table + 8, ws) == -1 && strstr(g_err, "overlaps"));
    NntkRnntPredictorConfig cfg = { 5, 7, 12, 20, 0, 0, 3, 4 };
    REQUIRE(!nntk_rnnt_predictor_create(cfg) && strstr(g_err, "H 12 != J 20"));
    cfg.has_proj = 1;
    REQUIRE(!nntk_rnnt_predictor_create(cfg));              /* the stubbed layer gives no handle: create unwinds what it had allocated */
    REQUIRE(nntk_rnnt_predictor_forward_device(NULL, ids, ids, out) == -1 && nntk_rnnt_predictor_backward_device(NULL, out, out, out, out) == -1);
    nntk_rnnt_predictor_destroy(NULL);
    puts("rnnt_pred host checks: ok");
    return 0;
}
