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
