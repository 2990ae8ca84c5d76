/*
 * recurrent.c -- GRU, LSTM and RNN host layer.  Reference: layers/recurrent.{h,c},
 * layers/private/recurrent_private.c:29-36 (one block W | U | b_i | b_h),
 * layers/gru.c (forward :13-19, :51-61, :110-204), layers/lstm.c (forward
 * :17-26, :55-65, :110-268), layers/rnn.c.
 *
 * Device plan per Apply:
 *   1. xW + b_i for all timesteps: one MFMA GEMM, written time-major [T, B, G*H]
 *   2. T fused step kernels (csrc/hip/recurrent.hip) carrying h (and c)
 * or, for the shapes they take, one launch of the register-resident kernels (recurrent_rr.hip, recurrent_fk.hip).
 * The single-sequence API is stateful exactly like the reference (gru.c:201, lstm.c:264-265): h/c persist in the handle
 * between calls.  The batched forms start every sequence from zeros (gru.c:260, lstm.c:439); their *VarLen forms take
 * per-row lengths and the caller's initial / final state.
 *
 * The three cells share one layer object (rec_layer) and everything written against it; the file goes: shared core,
 * kernel router, inference forms, training, bidirectional, then the three cells' entry points.
 */
#include <stdarg.h>
#include <stdio.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include "nntk_internal.h"

/* single-sequence calls of at most this many timesteps take the streaming kernels (one small launch per step, no
 * projection GEMM, no copies); longer ones amortise the batch path's fixed costs */
#define NNTK_STREAM_MAX_T 32

/* recurrent.c:7-19 */
RecurrentConfig RecurrentConfigCreate(int input_feature_channels, int output_feature_channels,
                                      bool return_sequences, int timesteps) {
    RecurrentConfig c;
    memset(&c, 0, sizeof(c));
    c.input_feature_channels = input_feature_channels;
    c.output_feature_channels = output_feature_channels;
    c.return_sequences = return_sequences;
    c.timesteps = timesteps;
    return c;
}

/* ============================== shared core =============================== */

typedef struct {
    int G;                      /* 1 (RNN), 3 (GRU) or 4 (LSTM) */
    int in, H, T;
    bool return_sequences;
    RecurrentWeights *weights;
    nntk_wblock wb;
    float *d_wp, *d_bi, *d_ut, *d_bh;
    float *d_wt;                /* W^T packed like U^T (only when in == H): layer-2 operand of the fused two-layer GRU */
    int wt_valid;
    int rr_exact_only;          /* W or U holds a value the bf16 split cannot represent (non-finite, > 3.39e38, denormal): exact kernels only */
    float *d_rr4;               /* the same weights as images of the full-K kernels (recurrent_fk.hip), packed with d_rr */
    float *d_rr;                /* weight images of the register-resident split-bf16 kernel (recurrent_rr.hip), made on first use */
    int rr_valid;
    float *d_rr_hf;             /* LSTM, H > 256: the images of the HF instantiation (h.U on two f16 images), packed on first use */
    int rr_hf_valid;
    float hf_wscale;            /* ... the scale W's images (and therefore Z) carry: 2^15 * (U's scale); 0: the form does not hold these weights */
    float *d_b4, *d_b4_train;   /* GRU on those kernels: the four-slot bias vector (gru_rr_build_image; the training forward's copy) */
    float *d_rr_train;          /* ... and the training forward's own copy, re-packed every mini-batch from the raw block */
    /* persistent single-sequence state [H], double-buffered: a stateful call reads state[cur] and writes
     * state[cur ^ 1]; cur flips only once the call is known to be good, so a call that has to be repeated
     * (persistent-kernel fault, see host_round_trip) still finds its initial state intact */
    float *d_h[2], *d_c[2];
    int cur;
    /* streaming path: pinned host staging the kernels read / write directly, a device counter of finished workgroups
     * and the pinned word the last one raises */
    float *pin_in, *pin_out;
    size_t pin_in_n, pin_out_n;
    unsigned *d_done;
    volatile unsigned *flag;
    unsigned seq;
    nntk_devbuf d_in, d_out, d_xw, d_work, d_work_rr, d_rr_stage;
    nntk_devbuf d_h2;           /* the fused LSTM -> TimeDistributedDense call: the sequence output in FRAG2H form */
    nntk_devbuf d_hseq;         /* register-resident kernels: their T-deep hand-off = the layer output in frag3 form (when the caller supplies no buffer) */
    nntk_devbuf d_xf3;          /* ... and the input packed into frag3 form (when the call packs it) */
    nntk_devbuf d_len;          /* *VarLen calls: the row lengths, then the 64-row batch tiles' maxima (ints) */
    nntk_devbuf d_bd, d_bd_len; /* bidirectional calls (on the forward handle): the composed route's tensors / the sum merge's backward half; row lengths */
} rec_core;

/* training state shared by the recurrent layers (gru.c:85-108): the mini-batch input and the forward caches on the device.
 * d_Zg = the gate cache (GRU [B][T][6H], LSTM zifgo [B][T][8H], RNN [B][T][H]); d_hU = GRU h.U_h, LSTM the cell state c, [B][T][H] */
typedef struct {
    int on, mini_batch, have_batch;
    const float *d_x_cur;        /* the mini-batch input of the last forward: d_x below (host-pointer calls) or the caller's device tensor */
    nntk_devbuf d_x, d_h, d_Zg, d_hU, d_dxW, d_dhU, d_work, d_raw, d_grad, d_scr, d_dout, d_dX;
    /* the *VarLen training calls: what the last forward ran with (row lengths on the device, the caller's initial state), remembered for
     * the gradient call; all NULL after a fixed-length, zero-state forward */
    nntk_train_vl vl;
    nntk_devbuf d_len, d_xm;     /* the lengths; the input with its padding steps cleared (what d_W's product reads) */
    nntk_devbuf d_s0;            /* step 0's recurrent gate gradients [B][G H] (+ [G H] unused column sums): d_U's h0 term */
    nntk_devbuf d_st;            /* host-memory forms: h0 | c0 | hT | cT | d_hT | d_cT | d_h0 | d_c0, [B][H] each */
    nntk_devbuf d_yo;            /* host-memory forms: the forward output */
    float *want_hT, *want_cT;    /* the forward call's final-state tensors, for a forward kernel that writes them itself (cleared when it did) */
    /* the bidirectional training calls: what this handle was in the last forward (0: none or a unidirectional forward since; 1 the forward,
     * 2 the backward direction), the other direction's handle and -- on the forward handle -- the merge */
    int bd_role, bd_merge;
    const void *bd_peer;
    nntk_devbuf d_bd_o, d_bd_do, d_bd_dx;      /* this direction's output, its output gradient, its input gradient */
    nntk_devbuf d_bd_g;          /* this direction's weight gradient of one call (W | U | b_i | b_h), before it is added onto the caller's block */
    nntk_devbuf d_bd_xr;         /* backward handle: the input reversed per row, kept for the gradient call */
    nntk_devbuf d_bd_host;       /* forward handle, host-memory forms: the merged output; d_dout | d_dX */
} rec_train;

/* One recurrent layer of any cell: what every internal routine takes.  The three public handle types are this layout. */
typedef struct {
    rec_core core;              /* core.G tells the cell */
    rec_train train;
    int use_bh;                 /* the config's v2: the step adds b_h (GRU: always) */
    int n_act;                  /* 3 / 5 / 1 */
    ActivationFunction act[5];  /* the caller's handles, in the kernels' order -- GRU: z, h, r; LSTM: input, forget, candidate, output gate, output */
    /* their kinds and ReLU scales as layer_acts found them at the START OF THE CALL IN PROGRESS: the handles stay with the caller, who may
     * change them between calls, so nothing here outlives a call */
    int acts[5];
    float scales[5];
} rec_layer;
struct GRUStruct { rec_layer l; };
struct LSTMStruct { rec_layer l; };
struct RNNStruct { rec_layer l; };

/* every public call starts with this: a clean error slot and its handle(s) */
#define REC_ENTER(who, handles_ok) do { nntk_shim_clear_error(); if (!(handles_ok)) NNTK_FAIL(who ": NULL handle"); } while (0)

/* sets "<who>: <formatted>" as the error; -1 */
__attribute__((format(printf, 2, 3))) static int rec_fail(const char *who, const char *fmt, ...) {
    char msg[256];
    int n = snprintf(msg, sizeof msg, "%s: ", who);
    if (n < 0 || n >= (int)sizeof msg) n = 0;
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(msg + n, sizeof msg - (size_t)n, fmt, ap);
    va_end(ap);
    nntk_set_error(msg);
    return -1;
}

int nntk_check_lengths(const char *who, const int *lengths, int B, int T, int *min_len, int *max_len) {
    int lo = T, hi = lengths ? 0 : T;
    for (int b = 0; lengths && b < B; ++b) {
        if (lengths[b] < 0 || lengths[b] > T) return rec_fail(who, "lengths[%d] = %d is outside [0, %d]", b, lengths[b], T);
        if (lengths[b] > hi) hi = lengths[b];
        if (lengths[b] < lo) lo = lengths[b];
    }
    if (min_len) *min_len = lo;
    if (max_len) *max_len = hi;
    return 0;
}

/* The device form of a batch's lengths (nntk_shim_rec_varlen's layout): one int per row (lengths NULL: every row T), then the 64-row
 * tiles' maxima; built in host memory and copied into buf in stream order.  bd: the bidirectional calls' virtual batch instead -- the B
 * rows padded to whole tiles (padding: 0) for the forward direction, the same again for the backward one.  NULL = error. */
static int *stage_lengths(nntk_devbuf *buf, const int *lengths, int B, int T, int bd) {
    const int Bp = 64 * ((B + 63) / 64), rows = bd ? 2 * Bp : B, tiles = (rows + 63) / 64;
    int *hl = (int *)calloc((size_t)rows + tiles, sizeof(int));
    if (!hl) { nntk_set_error("out of host memory"); return NULL; }
    for (int v = 0; v < rows; ++v) {
        const int r = bd ? v % Bp : v;
        hl[v] = r < B ? (lengths ? lengths[r] : T) : 0;
        if (hl[v] > hl[rows + v / 64]) hl[rows + v / 64] = hl[v];
    }
    int *d_len = (int *)nntk_devbuf_reserve(buf, (size_t)rows + tiles);
    if (d_len && nntk_shim_upload_ints(d_len, hl, (long)rows + tiles)) d_len = NULL;
    free(hl);
    return d_len;
}

/* 1 if the block holds a value the split-bf16 x 3 contraction cannot represent exactly: non-finite, above bf16's largest finite
 * value (bf16(x) = inf, and inf - inf = NaN in the split), or denormal (the bf16 MFMA flushes it).  The reference's f32 chain
 * (core/default_ops.cc:224-231) saturates or carries such values; the register-resident kernels would turn them into NaN, so a
 * flagged block keeps the exact-f32 kernels -- the same rule conv / dense / mel weights follow (runtime.c).  Branch-free so that
 * gcc vectorises it: the training forwards run it on every mini-batch. */
__attribute__((optimize("O3"))) static int rr_unsplittable(const float *v, size_t n) {
    const unsigned *u = (const unsigned *)v;
    unsigned bad = 0;
    for (size_t i = 0; i < n; ++i) {
        const unsigned a = u[i] & 0x7fffffffu;
        bad |= (unsigned)(a > 0x7f7f0000u) | (unsigned)(a - 1u < 0x007fffffu);
    }
    return bad != 0;
}

static int core_init(rec_core *c, int G, RecurrentConfig base) {
    memset(c, 0, sizeof(*c));
    c->G = G;
    c->in = base.input_feature_channels;
    c->H = base.output_feature_channels;
    c->T = base.timesteps;
    c->return_sequences = base.return_sequences;
    size_t w = (size_t)c->in * G * c->H, u = (size_t)c->H * G * c->H, b = (size_t)G * c->H;
    if (nntk_wblock_init(&c->wb, w + u + 2 * b)) return -1;
    c->weights = (RecurrentWeights *)malloc(sizeof(RecurrentWeights));
    c->weights->W = c->wb.host;
    c->weights->U = c->weights->W + w;
    c->weights->b_i = c->weights->U + u;
    c->weights->b_h = c->weights->b_i + b;
    /* one allocation: h[0] | h[1] | c[0] | c[1], each padded to 64 floats */
    size_t hs = ((size_t)c->H + 63) & ~(size_t)63;
    float *st = (float *)nntk_shim_malloc(4 * hs * sizeof(float));
    if (!st) return -1;
    c->d_h[0] = st; c->d_h[1] = st + hs; c->d_c[0] = st + 2 * hs; c->d_c[1] = st + 3 * hs;
    c->cur = 0;
    if (nntk_shim_memset(st, 0, 4 * hs * sizeof(float))) return -1;
    return 0;
}

static void core_free(rec_core *c) {
    nntk_shim_synchronize();
    nntk_shim_free(c->d_wp); nntk_shim_free(c->d_bi); nntk_shim_free(c->d_ut); nntk_shim_free(c->d_bh); nntk_shim_free(c->d_wt);
    nntk_shim_free(c->d_rr_hf);
    nntk_shim_free(c->d_rr); nntk_shim_free(c->d_rr4); nntk_shim_free(c->d_rr_train); nntk_shim_free(c->d_b4); nntk_shim_free(c->d_b4_train);
    nntk_shim_free(c->d_h[0]);
    nntk_shim_host_free(c->pin_in); nntk_shim_host_free(c->pin_out); nntk_shim_host_free((void *)c->flag);
    nntk_shim_free(c->d_done);
    nntk_devbuf_free(&c->d_in); nntk_devbuf_free(&c->d_out); nntk_devbuf_free(&c->d_xw); nntk_devbuf_free(&c->d_work); nntk_devbuf_free(&c->d_work_rr); nntk_devbuf_free(&c->d_rr_stage);
    nntk_devbuf_free(&c->d_hseq); nntk_devbuf_free(&c->d_xf3); nntk_devbuf_free(&c->d_h2);
    nntk_devbuf_free(&c->d_len);
    nntk_devbuf_free(&c->d_bd); nntk_devbuf_free(&c->d_bd_len);
    nntk_wblock_free(&c->wb);
    free(c->weights);
}

static void train_free(rec_train *t) {
    nntk_devbuf_free(&t->d_x); nntk_devbuf_free(&t->d_h); nntk_devbuf_free(&t->d_Zg); nntk_devbuf_free(&t->d_hU);
    nntk_devbuf_free(&t->d_dxW); nntk_devbuf_free(&t->d_dhU); nntk_devbuf_free(&t->d_work); nntk_devbuf_free(&t->d_raw);
    nntk_devbuf_free(&t->d_grad); nntk_devbuf_free(&t->d_scr); nntk_devbuf_free(&t->d_dout); nntk_devbuf_free(&t->d_dX);
    nntk_devbuf_free(&t->d_len); nntk_devbuf_free(&t->d_xm); nntk_devbuf_free(&t->d_s0); nntk_devbuf_free(&t->d_st);
    nntk_devbuf_free(&t->d_yo);
    nntk_devbuf_free(&t->d_bd_o); nntk_devbuf_free(&t->d_bd_do); nntk_devbuf_free(&t->d_bd_dx); nntk_devbuf_free(&t->d_bd_xr);
    nntk_devbuf_free(&t->d_bd_host); nntk_devbuf_free(&t->d_bd_g);
}

/* a handle of G gates over the caller's n_act activation handles (which stay the caller's: gru.c:116-126); NULL = error */
static rec_layer *layer_create(int G, RecurrentConfig base, int use_bh, const ActivationFunction *act, int n_act) {
    nntk_shim_clear_error();
    rec_layer *l = (rec_layer *)calloc(1, sizeof(rec_layer));
    if (!l) return NULL;
    l->use_bh = use_bh;
    l->n_act = n_act;
    memcpy(l->act, act, (size_t)n_act * sizeof(*act));
    if (core_init(&l->core, G, base)) { free(l); return NULL; }
    return l;
}
static void layer_train_on(rec_layer *l, RecurrentTrainingConfig training_config) {
    l->train.on = 1;
    l->train.mini_batch = training_config.mini_batch_size;
}
static void layer_destroy(rec_layer *l) {
    if (!l) return;
    core_free(&l->core);
    train_free(&l->train);
    free(l);
}

/* one [H][G*H] matrix transposed per gate into the step kernels' operand layout [G][Hj_p][Hk_p], so that each output column's K
 * vector is contiguous; the caller frees it.  NULL = out of host memory (error set) */
static float *pack_gate_transposed(const float *src, int G, int H, size_t *n) {
    const int Hj_p = (H + 15) & ~15, Hk_p = (H + 31) & ~31;
    *n = (size_t)G * Hj_p * Hk_p;
    float *tmp = (float *)calloc(*n, sizeof(float));
    if (!tmp) { nntk_set_error("out of host memory while packing recurrent weights"); return NULL; }
    for (int k = 0; k < H; ++k)
        for (int g = 0; g < G; ++g)
            for (int j = 0; j < H; ++j)
                tmp[((size_t)g * Hj_p + j) * Hk_p + k] = src[(size_t)k * G * H + (size_t)g * H + j];
    return tmp;
}

/* W [in, G*H] is already the GEMM's [K, N]; U [H, G*H] goes up as U^T per gate (pack_gate_transposed) */
static int core_upload(rec_core *c) {
    int G = c->G, H = c->H;
    if (nntk_upload_gemm_weights(&c->d_wp, c->weights->W, c->in, G * H)) return -1;
    if (nntk_upload_floats(&c->d_bi, c->weights->b_i, (size_t)G * H)) return -1;
    if (nntk_upload_floats(&c->d_bh, c->weights->b_h, (size_t)G * H)) return -1;
    size_t n;
    float *tmp = pack_gate_transposed(c->weights->U, G, H, &n);
    if (!tmp) return -1;
    int rc = nntk_upload_floats(&c->d_ut, tmp, n);
    free(tmp);
    if (rc) return rc;
    c->wt_valid = 0;
    c->rr_valid = 0;
    c->rr_hf_valid = 0;
    c->rr_exact_only = rr_unsplittable(c->weights->W, (size_t)c->in * G * H + (size_t)H * G * H);      /* W | U are contiguous */
    nntk_wblock_mark_uploaded(&c->wb);
    return 0;
}

/* W [in = H, G*H] in the U^T layout */
static int core_ensure_wt(rec_core *c) {
    if (c->wt_valid) return 0;
    if (c->in != c->H) NNTK_FAIL("fused GRU stack: layer 2's input size must equal its hidden size");
    size_t n;
    float *tmp = pack_gate_transposed(c->weights->W, c->G, c->H, &n);
    if (!tmp) return -1;
    int rc = nntk_upload_floats(&c->d_wt, tmp, n);
    free(tmp);
    if (rc) return rc;
    c->wt_valid = 1;
    return 0;
}

static int core_ensure(rec_core *c, int check_edits) {
    if (nntk_wblock_dirty(&c->wb, check_edits)) return core_upload(c);
    return 0;
}

static int core_reset_state(rec_core *c) {
    size_t hs = ((size_t)c->H + 63) & ~(size_t)63;
    c->cur = 0;
    return nntk_shim_memset(c->d_h[0], 0, 4 * hs * sizeof(float));
}

static int core_broadcast(rec_core *c, int root) {
    if (nntk_shim_dist_broadcast_host(c->wb.host, c->wb.n, root)) return -1;
    return core_upload(c);
}
static int core_sync(rec_core *c) {
    nntk_shim_synchronize();
    return core_upload(c);
}
/* the weight block W | U | b_i | b_h from device memory: staged through the pinned host block (the master copy every repack reads) */
static int core_load_device(rec_core *c, const char *who, const float *d_block) {
    if (!d_block) return rec_fail(who, "NULL block");
    if (nntk_shim_download(c->wb.host, d_block, c->wb.n * sizeof(float))) return -1;
    return core_upload(c);
}

/* kind + ReLU's output scale (activation_default.c:123-129) of one gate activation */
static int gate_kind(ActivationFunction a, int *kind, float *scale) {
    if (!a) NNTK_FAIL("recurrent layer: NULL gate activation");
    if (!nntk_act_fusable(a))
        NNTK_FAIL("recurrent layer: gate activations must be built-in identity/sigmoid/tanh/relu "
                  "(custom host callbacks and softmax cannot run inside the device step kernel)");
    *kind = a->kind;
    *scale = a->kind == NNTK_ACT_RELU ? a->relu_a : 1.0f;
    return 0;
}
/* reads the caller's activation handles for this call (l->acts, l->scales) */
static int layer_acts(rec_layer *l) {
    for (int i = 0; i < l->n_act; ++i)
        if (gate_kind(l->act[i], &l->acts[i], &l->scales[i])) return -1;
    return 0;
}
/* the activations the register-resident kernels are written for (the RNN cell has no such kernel) */
static int layer_std_acts(const rec_layer *l) {
    const int *a = l->acts;
    if (l->core.G == 4)
        return a[0] == NNTK_ACT_SIGMOID && a[1] == NNTK_ACT_SIGMOID && a[2] == NNTK_ACT_TANH && a[3] == NNTK_ACT_SIGMOID && a[4] == NNTK_ACT_TANH;
    return l->core.G == 3 && a[0] == NNTK_ACT_SIGMOID && a[1] == NNTK_ACT_TANH && a[2] == NNTK_ACT_SIGMOID;      /* z, h, r */
}

/* ============================== kernel router ============================== */
/* Which recurrent kernel a call takes depends on the layer's SHAPE, its activations and the FORM of the call -- never on the
 * number of sequences in it: a row's bits must not change with the batch (or shard) it arrives in (round 3 had a
 * B >= 32 threshold here, which made a 130-utterance batch sharded over 8 GPUs differ from the single-GPU run).
 *   zero-state batch forms ([B, T, in]: *ApplyInferenceBatch, *ApplyDevice, GRUStack2Apply*, the training forwards), qualifying
 *     shape, standard activations, splittable weights  ->  the register-resident split-bf16 kernels (recurrent_rr.hip), any B;
 *   the reference's stateful single-sequence call (*ApplyInference: carried h / c)  ->  the exact-f32 kernels, whose chain the
 *     streaming kernel (T <= 32) reproduces bit for bit, so cutting a stream into calls of any length gives the same bits.
 * Option rec_rr = 1 takes the register-resident kernels for the stateful call too; 0 never takes them. */

static int rr_option(void) {
    int on = -1;
    (void)nntk_shim_get_option("rec_rr", &on);
    return on;
}

/* THE test whether a layer takes the register-resident kernels: NULL when it does, else the reason (KernelPlan prints it).  Reads l->acts.
 * The callers say what differs between them: exact_only -- the weights hold a value the bf16 split cannot (the inference forms read
 * core.rr_exact_only, KernelPlan only once there was an upload, the training forwards scan the live block themselves); shape_ok -- the
 * kernel form in question takes this H x in (frag3-input form: nntk_shim_rr_image_floats_xf; f32-input form, which the training forwards
 * run: nntk_shim_lstm_rr_image_floats; the HF form: nntk_shim_lstm_rr_hf_ok). */
static const char *rr_why_not(const rec_layer *l, int exact_only, int shape_ok) {
    const rec_core *c = &l->core;
    if (c->G == 1) return "the RNN cell has no register-resident kernel";
    if (rr_option() == 0) return "option rec_rr = 0";
    if (!layer_std_acts(l)) return "non-default gate activations";
    if (exact_only) return "a weight the bf16 split cannot hold (non-finite, > 3.39e38 or denormal)";
    if (!shape_ok) return (c->H % 16) ? "H % 16 != 0" : (c->H < 64 || c->H > 512) ? "H outside 64..512" : "input wider than 128 (256 when H <= 256)";
    return NULL;
}
/* ... for the zero-state inference forms */
static int layer_takes_rr(const rec_layer *l) {
    return !rr_why_not(l, l->core.rr_exact_only, nntk_shim_rr_image_floats_xf(l->core.H, l->core.in) != 0);
}

/* How a call on the register-resident kernels takes its input and hands over its output.  The kernels' hand-off buffer is T-deep and
 * in FRAG3 form (frag3.hip: three bf16 images in MFMA fragment order), so the layer output exists in that form anyway; a consumer that
 * reads frag3 (the next layer of a stack, the dense GEMM) takes it from there and d_out may be NULL. */
typedef struct {
    const float *d_in;      /* f32 [B][T][in], or NULL when d_in_f3 is given */
    const float *d_in_f3;   /* the input in frag3 form, or NULL */
    float *d_out;           /* f32 output, or NULL */
    float *d_out_f3;        /* frag3 output [B][T][H] (nntk_frag3_floats), or NULL: handle scratch */
    float *d_out_h2;        /* LSTM only: the sequence output as a FRAG2H tensor (nntk_frag2h_floats) instead of d_out (which must be NULL), or NULL */
    /* the *VarLen calls: row lengths + tile maxima (device, stage_lengths) and the caller's state, or d_len NULL */
    const int *d_len;
    const float *d_h0, *d_c0;
    float *d_hT, *d_cT;
} rr_io;

/* decides the x form and provides it: 0 = f32 rows, 1 = frag3 (*xf3 set; packed here when the caller passed f32), 2 = shape not taken */
static int rr_input(rec_core *c, const rr_io *io, int B, const float **xf3) {
    *xf3 = io->d_in_f3;
    /* (a misaligned f32 pointer cannot take the 16-byte row requests: it is packed like a shape the f32 form does not take, so the kernel
     * family -- and the bits -- do not depend on the caller's pointer alignment) */
    const int f32_ok = io->d_in && (((size_t)io->d_in) & 15) == 0 && nntk_shim_lstm_rr_image_floats(c->H, c->in) != 0;
    const int xf_ok = nntk_shim_rr_image_floats_xf(c->H, c->in) != 0;
    if (io->d_in_f3) return xf_ok ? 1 : 2;
    int mode = -1;
    (void)nntk_shim_get_option("rec_xf", &mode);
    /* 1: always pack (one extra pass over x, then coalesced requests and no split inside the step); 0: only when the f32 path cannot
     * take the shape (in % 8 != 0); auto: pack once the call is big enough for the pass to pay (measured at the stack's LSTM, 512 x 996
     * x 128: 6.50 -> 6.16 ms including the pack).  The two x forms give the same bits (the split is exact and the kernels sum the same
     * products in the same order -- tests/test_gpu_frag3.py), so this is a speed choice that may depend on the size of the call. */
    /* a shape the full-K family takes (recurrent_fk.hip) runs on it at EVERY size -- it sums in another order than the split-K family, so
     * the choice must not depend on the call -- and that family reads frag3 only */
    const int fk = nntk_shim_fk_image_floats(c->H, c->in) != 0;
    if (f32_ok && !fk && (mode == 0 || (mode < 0 && (long)B * c->T < 8192))) return 0;
    if (!xf_ok || !io->d_in) return 2;
    float *buf = nntk_devbuf_reserve(&c->d_xf3, nntk_shim_frag3_floats(B, c->T, c->in));
    if (!buf) return -1;
    if (nntk_shim_frag3_pack(io->d_in, buf, B, c->T, c->in)) return -1;
    *xf3 = buf;
    return 1;
}

/* the LSTM's weight images of the register-resident (and, for the shapes that family takes, the full-K) kernels */
static int lstm_rr_images(rec_core *c) {
    const size_t img = nntk_shim_rr_image_floats_xf(c->H, c->in);
    if (!c->d_rr && !(c->d_rr = (float *)nntk_shim_malloc(img * sizeof(float)))) return -1;
    if (nntk_shim_lstm_rr_pack(c->d_ut, c->d_wp, c->d_rr, c->H, c->in)) return -1;
    const size_t img4 = nntk_shim_fk_image_floats(c->H, c->in);
    if (img4) {
        if (!c->d_rr4 && !(c->d_rr4 = (float *)nntk_shim_malloc(img4 * sizeof(float)))) return -1;
        if (nntk_shim_fk_pack(c->d_ut, c->d_wp, c->d_rr4, c->H, c->in)) return -1;
    }
    return 0;
}

/* GRU on the register-resident split-bf16 kernels (recurrent_rr.hip gru_rr_kernel).  The three gates ride in four slots,
 * z | r | h.U_h | x.W_h: the image is packed from [U_z | U_r | U_h | 0] and [W_z | W_r | 0 | W_h], the bias vector is
 * b_i,z + b_h,z | b_i,r + b_h,r | b_h,h | b_i,h (gru.c:144-186: the reset gate multiplies h.U_h + b_h,h only).
 * Packs *d_img (allocated on first use, `img` floats) and *d_b4 from the caller-layout weights W [in][3H], U [H][3H], b_i, b_h */
static int gru_rr_build_image(int in, int H, const float *W, const float *U, const float *bi, const float *bh,
                              float **d_img, size_t img, float **d_b4, nntk_devbuf *stage, float **d_img4) {
    const size_t nW = (size_t)in * 4 * H, nU = (size_t)H * 4 * H;
    float *tmp = (float *)calloc(nW + nU + 4 * (size_t)H, sizeof(float));
    if (!tmp) NNTK_FAIL("out of host memory while packing GRU weights");
    float *W4 = tmp, *U4 = tmp + nW, *b4 = U4 + nU;
    for (int k = 0; k < in; ++k) {
        memcpy(W4 + (size_t)k * 4 * H, W + (size_t)k * 3 * H, 2 * (size_t)H * sizeof(float));                 /* W_z | W_r */
        memcpy(W4 + (size_t)k * 4 * H + 3 * (size_t)H, W + (size_t)k * 3 * H + 2 * (size_t)H, (size_t)H * sizeof(float));   /* slot 3: W_h */
    }
    for (int k = 0; k < H; ++k) memcpy(U4 + (size_t)k * 4 * H, U + (size_t)k * 3 * H, 3 * (size_t)H * sizeof(float));      /* U_z | U_r | U_h | 0 */
    for (int j = 0; j < H; ++j) {
        b4[j] = bi[j] + bh[j];
        b4[H + j] = bi[H + j] + bh[H + j];
        b4[2 * H + j] = bh[2 * H + j];
        b4[3 * H + j] = bi[2 * H + j];
    }
    int rc = 0;
    float *d_tmp = nntk_devbuf_reserve(stage, nW + nU);        /* kept with the handle: stream order protects it, no synchronisation */
    if (!d_tmp) rc = -1;
    if (!rc && !*d_img && !(*d_img = (float *)nntk_shim_malloc(img * sizeof(float)))) rc = -1;
    if (!rc && !*d_b4 && !(*d_b4 = (float *)nntk_shim_malloc(4 * (size_t)H * sizeof(float)))) rc = -1;
    if (!rc) rc = nntk_shim_upload(d_tmp, tmp, (nW + nU) * sizeof(float));
    if (!rc) rc = nntk_shim_upload(*d_b4, b4, 4 * (size_t)H * sizeof(float));
    if (!rc) rc = nntk_shim_lstm_rr_pack_raw(d_tmp + nW, d_tmp, *d_img, H, in);
    const size_t img4 = d_img4 ? nntk_shim_fk_image_floats(H, in) : 0;        /* the full-K family's images of the same matrices */
    if (!rc && img4) {
        if (!*d_img4 && !(*d_img4 = (float *)nntk_shim_malloc(img4 * sizeof(float)))) rc = -1;
        if (!rc) rc = nntk_shim_fk_pack_raw(d_tmp + nW, d_tmp, *d_img4, H, in);
    }
    free(tmp);                                              /* (nntk_shim_upload has copied it) */
    return rc ? -1 : 0;
}
/* the GRU's images and four-slot bias of those kernels */
static int gru_rr_images(rec_core *c) {
    const int H = c->H, in = c->in;
    /* from the SHADOW, i.e. the weight version core_upload packed d_wp / d_ut from: the device-pointer calls do not look for
     * host edits (SyncWeights is their contract), and an un-synced edit must not reach this kernel alone */
    const float *sW = c->wb.shadow, *sU = sW + (size_t)in * 3 * H, *sbi = sU + (size_t)H * 3 * H, *sbh = sbi + 3 * (size_t)H;
    return gru_rr_build_image(in, H, sW, sU, sbi, sbh, &c->d_rr, nntk_shim_rr_image_floats_xf(H, in), &c->d_b4, &c->d_rr_stage, &c->d_rr4);
}
/* the layer's weight images of the register-resident kernels (d_rr, d_rr4; GRU: d_b4), packed on first use after an upload */
static int layer_rr_images(rec_layer *l) {
    rec_core *c = &l->core;
    if (nntk_shim_fk_image_floats(c->H, c->in) && !c->d_rr4) c->rr_valid = 0;      /* (option rec_fk switched on after the images were packed) */
    if (c->rr_valid) return 0;
    if (c->G == 4 ? lstm_rr_images(c) : gru_rr_images(c)) return -1;
    c->rr_valid = 1;
    return 0;
}

/* Runs the call on the register-resident kernels when the layer takes them: 0 = ran; 1 = not taken, and nothing enqueued that matters;
 * -1 = error.  stateful: the single-sequence call on the handle's own state, which takes these kernels only with option rec_rr = 1. */
static int core_try_rr(rec_layer *l, const rr_io *io, int B, int stateful) {
    rec_core *c = &l->core;
    if (stateful && rr_option() != 1) return 1;
    if (!layer_takes_rr(l)) return 1;
    const float *xf3 = NULL;
    const int xm = rr_input(c, io, B, &xf3);
    if (xm < 0) return -1;
    if (xm == 2) return 1;
    if (layer_rr_images(l)) return -1;
    float *d_work = nntk_devbuf_reserve(&c->d_work_rr, nntk_shim_lstm_rr_work_floats(B, c->H));
    float *d_hseq = io->d_out_f3 ? io->d_out_f3 : nntk_devbuf_reserve(&c->d_hseq, nntk_shim_rr_hseq_floats(B, c->T, c->H));
    if (!d_work || !d_hseq) return -1;
    const int gru = c->G == 3;
    const float *x = xm ? NULL : io->d_in, *xf = xm ? xf3 : NULL;
    const float *bi = gru ? c->d_b4 : c->d_bi, *bh = !gru && l->use_bh ? c->d_bh : NULL;       /* (the GRU's four-slot bias holds b_h) */
    if (io->d_len)
        return nntk_shim_rr_varlen(gru, x, xf, c->d_rr, c->d_rr4, bi, bh, io->d_h0, io->d_c0, io->d_out, d_hseq, io->d_hT, io->d_cT, d_work,
                                   io->d_len, B, c->T, c->in, c->H, c->return_sequences);
    const float *h0 = stateful ? c->d_h[c->cur] : NULL, *c0 = stateful ? c->d_c[c->cur] : NULL;
    float *hT = stateful ? c->d_h[c->cur ^ 1] : NULL, *cT = stateful ? c->d_c[c->cur ^ 1] : NULL;
    if (gru)
        return nntk_shim_gru_rr(x, xf, c->d_rr, c->d_rr4, bi, h0, io->d_out, d_hseq, hT, d_work, B, c->T, c->in, c->H, c->return_sequences, 0, 0);
    return nntk_shim_lstm_rr(x, xf, c->d_rr, c->d_rr4, bi, bh, h0, c0, io->d_out, io->d_out_h2, d_hseq, hT, cT, d_work, B, c->T, c->in, c->H,
                             c->return_sequences);
}

/* Which kernel family the zero-state batch forms of a layer will take, and why not the fast one when they will not: a caller can see a
 * performance cliff (a shape outside the register-resident kernels runs 1.3-1.8x slower) before it measures one.  The answer depends on
 * the layer only -- shape, activations, weights -- never on the batch (see the comment above rr_option). */
static const char *core_plan(rec_layer *l, char *buf, size_t n) {
    const rec_core *c = &l->core;
    const char *cell = c->G == 4 ? "lstm" : c->G == 3 ? "gru" : "rnn";
    if (layer_acts(l)) return c->G == 4 ? "lstm: invalid gate activations" : "gru: invalid gate activations";
    const char *why = rr_why_not(l, c->wb.uploaded && c->rr_exact_only, nntk_shim_rr_image_floats_xf(c->H, c->in) != 0);
    if (why)
        snprintf(buf, n, "%s: exact-f32 kernels (projection GEMM + rec_persistent_kernel, per-timestep kernels when that does not fit) -- %s", cell, why);
    else if (nntk_shim_fk_image_floats(c->H, c->in) != 0)       /* (option rec_fk = 1 and a shape that family takes) */
        snprintf(buf, n, "%s: %s_fk_kernel<16,%d,%d> (register-resident split-bf16 x 3 without split-K, input projection fused; the input is packed into frag3 form first); the stateful single-sequence call keeps the exact-f32 kernels",
                 cell, cell, c->in <= 128 ? 8 : 16, 4);
    else
        snprintf(buf, n, "%s: %s_rr_kernel<%d,%d> (register-resident split-bf16 x 3, input projection fused)%s; the stateful single-sequence call keeps the exact-f32 kernels",
                 cell, cell, c->H <= 256 ? 4 : 8, c->in <= 64 ? 1 : c->in <= 128 ? 2 : 4,
                 nntk_shim_lstm_rr_image_floats(c->H, c->in) != 0 ? "" : "; in % 8 != 0: the input is packed into frag3 form first");
    return buf;
}

/* ============================= inference forms ============================= */
/* (all of them read the activations of the call in progress from l->acts / l->scales: the entry point has run layer_acts) */

/* stateful != 0: continue from / store into the handle's state (B must be 1) */
static int core_apply_device(rec_layer *l, const float *d_in, float *d_out, int B, int stateful) {
    rec_core *c = &l->core;
    int G = c->G, H = c->H, T = c->T;
    if (B <= 0 || T <= 0) return 0;
    const rr_io io = { .d_in = d_in, .d_out = d_out };
    int rc = core_try_rr(l, &io, B, stateful);
    if (rc <= 0) return rc;
    float *d_xw = nntk_devbuf_reserve(&c->d_xw, (size_t)T * B * G * H);
    float *d_work = nntk_devbuf_reserve(&c->d_work, nntk_shim_recurrent_work_floats(B, H));
    if (!d_xw || !d_work) return -1;
    /* input projection, rows (b, t) written at time-major row t*B + b */
    if (nntk_shim_conv1d(d_in, c->d_wp, c->d_bi, NULL, 0.f, NNTK_ACT_IDENTITY, 1.f, d_xw,
                         B, T, c->in, G * H, 1, 1, T, 1))
        return -1;
    const float *bh = l->use_bh ? c->d_bh : NULL;
    const float *h0 = stateful ? c->d_h[c->cur] : NULL, *c0 = stateful ? c->d_c[c->cur] : NULL;
    float *hT = stateful ? c->d_h[c->cur ^ 1] : NULL, *cT = stateful ? c->d_c[c->cur ^ 1] : NULL;
    if (G == 1)
        return nntk_shim_rnn(d_xw, c->d_ut, bh, h0, d_out, hT, d_work, B, T, H, c->return_sequences, l->acts[0], l->scales[0]);
    if (G == 4)
        return nntk_shim_lstm(d_xw, c->d_ut, bh, h0, c0, d_out, hT, cT, d_work, B, T, H, c->return_sequences, l->acts, l->scales);
    return nntk_shim_gru(d_xw, c->d_ut, bh, h0, d_out, hT, d_work, B, T, H, c->return_sequences, l->acts, l->scales);
}

/* Ragged batches with carried state (the *VarLen calls): row b runs its first lengths[b] steps from h0[b] (c0[b]); hT / cT and the
 * output of a layer without sequences are the state after those steps, sequence outputs past them are zeros.  lengths is host memory
 * (NULL: every row T), checked before anything is enqueued and copied to the handle in stream order.  The call takes the kernel
 * family the layer's zero-state batch calls take -- the same router (core_try_rr, then the exact-f32 kernels), so a row's bits for
 * the steps it runs are those of *ApplyDevice.  c0 / cT: LSTM only (ignored for the other cells). */
static int core_apply_device_vl(rec_layer *l, const char *who, const float *d_in, float *d_out, int B, const int *lengths,
                                const float *d_h0, const float *d_c0, float *d_hT, float *d_cT) {
    rec_core *c = &l->core;
    const int G = c->G, H = c->H, T = c->T;
    if (B < 0) return rec_fail(who, "batch %d < 0", B);
    int T_min, T_max;
    if (nntk_check_lengths(who, lengths, B, T, &T_min, &T_max)) return -1;
    if (B == 0 || T <= 0) return 0;
    const int *d_len = stage_lengths(&c->d_len, lengths, B, T, 0);
    if (!d_len) return -1;
    if (G != 4) d_c0 = NULL, d_cT = NULL;
    const int zero_pad = c->return_sequences && T_min < T;
    const rr_io io = { .d_in = d_in, .d_out = d_out, .d_len = d_len, .d_h0 = d_h0, .d_c0 = d_c0, .d_hT = d_hT, .d_cT = d_cT };
    const int rc = core_try_rr(l, &io, B, 0);
    if (rc < 0) return -1;
    if (rc == 0) return zero_pad ? nntk_shim_varlen_zero_pad(d_out, d_len, B, T, H) : 0;
    float *d_xw = nntk_devbuf_reserve(&c->d_xw, (size_t)T * B * G * H);
    float *d_work = nntk_devbuf_reserve(&c->d_work, nntk_shim_recurrent_work_floats(B, H));
    if (!d_xw || !d_work) return -1;
    if (T_max > 0 && nntk_shim_conv1d(d_in, c->d_wp, c->d_bi, NULL, 0.f, NNTK_ACT_IDENTITY, 1.f, d_xw, B, T, c->in, G * H, 1, 1, T, 1))
        return -1;
    if (nntk_shim_rec_varlen(G, d_xw, c->d_ut, l->use_bh ? c->d_bh : NULL, d_h0, d_c0, d_out, d_hT, d_cT,
                             d_work, B, T, H, c->return_sequences, l->acts, l->scales, d_len, T_max))
        return -1;
    return zero_pad ? nntk_shim_varlen_zero_pad(d_out, d_len, B, T, H) : 0;
}

/* Device call with frag3 tensors on either side (additive API: <Layer>ApplyDeviceFrag3).  Zero state per sequence.  The
 * register-resident kernels take and produce the format natively; every other kernel goes through f32 scratch tensors (frag3 is
 * exact: unpack(pack(x)) == x), so the call works for every shape and the results do not depend on the route. */
static int core_apply_device_f3(rec_layer *l, const float *d_in, const float *d_in_f3, float *d_out, float *d_out_f3, int B) {
    rec_core *c = &l->core;
    if (B <= 0 || c->T <= 0) return 0;
    if (!d_in && !d_in_f3) NNTK_FAIL("ApplyDeviceFrag3: no input tensor");
    if (!d_out && !d_out_f3) NNTK_FAIL("ApplyDeviceFrag3: no output tensor");
    if (d_out_f3 && !c->return_sequences) NNTK_FAIL("ApplyDeviceFrag3: a frag3 output needs return_sequences");
    const rr_io io = { .d_in = d_in, .d_in_f3 = d_in_f3, .d_out = d_out, .d_out_f3 = d_out_f3 };
    const int rc = core_try_rr(l, &io, B, 0);
    if (rc <= 0) return rc;
    const float *x = d_in;
    if (!x) {
        float *xs = nntk_devbuf_reserve(&c->d_in, (size_t)B * c->T * c->in);
        if (!xs || nntk_shim_frag3_unpack(d_in_f3, xs, B, c->T, c->in)) return -1;
        x = xs;
    }
    float *o = d_out;
    if (!o && !(o = nntk_devbuf_reserve(&c->d_out, (size_t)B * c->T * c->H))) return -1;
    if (core_apply_device(l, x, o, B, 0)) return -1;
    return d_out_f3 ? nntk_shim_frag3_pack(o, d_out_f3, B, c->T, c->H) : 0;
}

/* The reference's own call shape -- one sequence, carried state, a handful of timesteps -- is latency, not throughput: T launches
 * of the streaming step kernel, x_t read from and h_t written to pinned host memory by the kernels themselves, and the host waits
 * on a pinned word the last workgroup raises (a stream synchronisation alone costs more than the kernels).  Same bits as the batch
 * path (recurrent.hip). */
#if defined(__x86_64__) || defined(__i386__)
#define NNTK_CPU_RELAX() __builtin_ia32_pause()
#elif defined(__aarch64__)
#define NNTK_CPU_RELAX() __asm__ __volatile__("yield")
#else
#define NNTK_CPU_RELAX() ((void)0)
#endif
static int core_apply_stream(rec_layer *l, const float *input, float *output) {
    rec_core *c = &l->core;
    const size_t n_in = (size_t)c->T * c->in, n_out = c->return_sequences ? (size_t)c->T * c->H : (size_t)c->H;
    if (c->pin_in_n < n_in) {
        nntk_shim_synchronize();
        nntk_shim_host_free(c->pin_in);
        c->pin_in = (float *)nntk_shim_host_alloc(n_in * sizeof(float));
        c->pin_in_n = c->pin_in ? n_in : 0;
    }
    if (c->pin_out_n < n_out) {
        nntk_shim_synchronize();
        nntk_shim_host_free(c->pin_out);
        c->pin_out = (float *)nntk_shim_host_alloc(n_out * sizeof(float));
        c->pin_out_n = c->pin_out ? n_out : 0;
    }
    if (!c->flag) {
        c->flag = (volatile unsigned *)nntk_shim_host_alloc(64);
        c->d_done = (unsigned *)nntk_shim_malloc(64);
        if (c->d_done && nntk_shim_memset(c->d_done, 0, 64)) return -1;
    }
    if (!c->pin_in || !c->pin_out || !c->flag || !c->d_done) return -1;
    memcpy(c->pin_in, input, n_in * sizeof(float));
    const unsigned seq = ++c->seq ? c->seq : ++c->seq;         /* never 0: the word's initial value */
    if (nntk_shim_rec_stream(c->G, c->G == 4, c->pin_in, c->d_wp, c->d_bi, c->d_ut, l->use_bh ? c->d_bh : NULL,
                             c->d_h[0], c->d_h[1], c->d_c[0], c->d_c[1], c->cur, c->pin_out, c->T, c->in, c->H,
                             c->return_sequences, l->acts, l->scales, c->d_done, (unsigned *)c->flag, seq))
        return -1;
    /* spin on the pinned word; after 5 ms fall back to a stream synchronisation (which also surfaces launch errors) */
    struct timespec t0, t1;
    clock_gettime(CLOCK_MONOTONIC, &t0);
    for (unsigned spins = 0; *c->flag != seq; ++spins) {
        if ((spins & 1023) == 1023) {
            clock_gettime(CLOCK_MONOTONIC, &t1);
            if ((t1.tv_sec - t0.tv_sec) * 1000000000L + (t1.tv_nsec - t0.tv_nsec) > 5000000L) {
                /* error paths: the last launch may not have counted every workgroup in, and only the workgroup that
                 * counts in last resets the counter -- clear it here, or every later call on this handle would wait
                 * for a count that is never reached */
                if (nntk_shim_synchronize()) { (void)nntk_shim_memset(c->d_done, 0, 64); return -1; }
                if (*c->flag != seq) {
                    (void)nntk_shim_memset(c->d_done, 0, 64);
                    (void)nntk_shim_synchronize();
                    NNTK_FAIL("streaming recurrent kernel did not complete");
                }
                break;
            }
        }
        NNTK_CPU_RELAX();
    }
    memcpy(output, c->pin_out, n_out * sizeof(float));
    c->cur = (c->cur + c->T) & 1;
    return 0;
}

/* ---- host-pointer forms: upload, the device form, download ---- */

/* one device-form call as the host forms run it (twice, when the first try has to be repeated) */
typedef struct dev_call {
    int (*run)(const struct dev_call *k, const float *d_in, float *d_out);
    rec_layer *l, *l2;          /* the layer; the second layer of a stack / the backward direction */
    const char *who;
    int B, stateful, merge;
    const int *lengths;
    const float *d_h0, *d_c0;
    float *d_hT, *d_cT;
} dev_call;
typedef struct { const float *host; float *dev; size_t n; } host_input;      /* (host NULL: not given, skipped) */

/* Uploads the inputs, runs the device form and downloads its output WITHOUT looking for errors, then asks whether a persistent kernel
 * gave up during the call: its workgroups were not all resident (another process held the CUs), and the library has switched to the
 * per-timestep kernels, which need no co-residency and produce the same bits.  Then the call is repeated once on those; a stateful
 * call's initial state is still intact (double-buffered, see rec_core).  strict: the repeat is examined like the first try, and a
 * second give-up is the error "recurrent kernel fault"; otherwise the repeat's download is the checking one. */
static int host_round_trip(const dev_call *k, const host_input *in, int n_inputs, float *d_out, float *output, size_t n_out, int strict) {
    for (int i = 0; i < n_inputs; ++i)
        if (in[i].host && nntk_shim_upload(in[i].dev, in[i].host, in[i].n * sizeof(float))) return -1;
    if (k->run(k, in[0].dev, d_out)) return -1;
    if (nntk_shim_download_nocheck(output, d_out, n_out * sizeof(float))) return -1;
    if (!nntk_shim_take_fault()) return 0;
    if (k->run(k, in[0].dev, d_out)) return -1;
    if (!strict) return nntk_shim_download(output, d_out, n_out * sizeof(float));
    if (nntk_shim_download_nocheck(output, d_out, n_out * sizeof(float))) return -1;
    if (nntk_shim_take_fault()) NNTK_FAIL("recurrent kernel fault");
    return 0;
}

static int run_apply(const dev_call *k, const float *d_in, float *d_out) { return core_apply_device(k->l, d_in, d_out, k->B, k->stateful); }
static int core_apply_host(rec_layer *l, const float *input, float *output, int B, int stateful) {
    rec_core *c = &l->core;
    if (B <= 0) return 0;
    if (stateful && B == 1 && c->T >= 1 && c->T <= NNTK_STREAM_MAX_T) {
        int on = -1;
        (void)nntk_shim_get_option("rec_stream", &on);
        if (on != 0) {
            if (core_ensure(c, 2)) return -1;          /* latency path: sampled edit check (runtime.c) */
            return core_apply_stream(l, input, output);
        }
    }
    if (core_ensure(c, 1)) return -1;
    size_t n_in = (size_t)B * c->T * c->in;
    size_t n_out = c->return_sequences ? (size_t)B * c->T * c->H : (size_t)B * c->H;
    float *d_in = nntk_devbuf_reserve(&c->d_in, n_in);
    float *d_out = nntk_devbuf_reserve(&c->d_out, n_out);
    if (!d_in || !d_out) return -1;
    const dev_call k = { .run = run_apply, .l = l, .B = B, .stateful = stateful };
    const host_input in = { input, d_in, n_in };
    if (host_round_trip(&k, &in, 1, d_out, output, n_out, 0)) return -1;
    if (stateful) c->cur ^= 1;
    return 0;
}

static int run_apply_vl(const dev_call *k, const float *d_in, float *d_out) {
    return core_apply_device_vl(k->l, k->who, d_in, d_out, k->B, k->lengths, k->d_h0, k->d_c0, k->d_hT, k->d_cT);
}
/* (the initial state goes up only when given, the final state comes down only when asked for) */
static int core_apply_host_vl(rec_layer *l, const char *who, const float *input, float *output, int B, const int *lengths,
                              const float *h0, const float *c0, float *hT, float *cT) {
    rec_core *c = &l->core;
    if (B <= 0) return core_apply_device_vl(l, who, NULL, NULL, B, lengths, NULL, NULL, NULL, NULL);
    if (core_ensure(c, 1)) return -1;
    const size_t n_in = (size_t)B * c->T * c->in, n_out = c->return_sequences ? (size_t)B * c->T * c->H : (size_t)B * c->H;
    const size_t BH = (size_t)B * c->H;
    const int lstm = c->G == 4;
    float *d_in = nntk_devbuf_reserve(&c->d_in, n_in);
    /* out | h0 | c0 | hT | cT */
    float *d_out = nntk_devbuf_reserve(&c->d_out, n_out + (2 + 2 * lstm) * BH);
    if (!d_in || !d_out) return -1;
    float *d_h0 = h0 ? d_out + n_out : NULL, *d_c0 = (lstm && c0) ? d_out + n_out + BH : NULL;
    float *d_hT = hT ? d_out + n_out + (1 + lstm) * BH : NULL, *d_cT = (lstm && cT) ? d_out + n_out + (2 + lstm) * BH : NULL;
    const dev_call k = { .run = run_apply_vl, .l = l, .who = who, .B = B, .lengths = lengths, .d_h0 = d_h0, .d_c0 = d_c0, .d_hT = d_hT, .d_cT = d_cT };
    const host_input in[3] = { { input, d_in, n_in }, { d_h0 ? h0 : NULL, d_h0, BH }, { d_c0 ? c0 : NULL, d_c0, BH } };
    if (host_round_trip(&k, in, 3, d_out, output, n_out, 1)) return -1;
    if (d_hT && nntk_shim_download(hT, d_hT, BH * sizeof(float))) return -1;
    if (d_cT && nntk_shim_download(cT, d_cT, BH * sizeof(float))) return -1;
    return 0;
}

/* ================================ training ================================= */
/* SURVEY 8(f)-4.  gru.c:246-293 / lstm.c:418-475 / rnn.c:249-291: the forward keeps its caches (rec_train); gru.c:295-512 /
 * lstm.c:294-416 + :477-556 / rnn.c:184-221 + :293-351: BPTT.  Default activations: one launch of the register-resident kernel's TRAIN
 * instantiation; otherwise one launch per timestep and direction, VALU dots in the reference's operation order: correct and
 * deterministic, not tuned (csrc/hip/train.hip).  The *VarLen forms train on ragged batches with carried state (INTEGRATION.md
 * "Training on ragged batches and long streams"). */

/* ONE zeroed block d_W | d_U | d_b_i | d_b_h | d_X (recurrent_private.c:10-22) */
static RecurrentGradient *gradient_create(int G, RecurrentConfig base, RecurrentTrainingConfig training_config) {
    RecurrentGradient *g = (RecurrentGradient *)malloc(sizeof(RecurrentGradient));
    if (!g) return NULL;
    size_t in = (size_t)base.input_feature_channels, H = (size_t)base.output_feature_channels;
    size_t w = in * G * H, u = H * G * H, b = G * H;
    size_t x = (size_t)training_config.mini_batch_size * in * base.timesteps;
    g->d_W = (float *)calloc(w + u + 2 * b + x + 1, sizeof(float));
    if (!g->d_W) { free(g); return NULL; }
    g->d_U = g->d_W + w;
    g->d_b_i = g->d_U + u;
    g->d_b_h = g->d_b_i + b;
    g->d_X = g->d_b_h + b;
    return g;
}
void RecurrentGradientDestroy(RecurrentGradient *gradient) {
    if (!gradient) return;
    free(gradient->d_W);
    free(gradient);
}

/* a ragged or carried-state forward (such a call always brings lengths: the *VarLen entry points fill them in) */
static int train_vl_active(const nntk_train_vl *vl) { return vl && (vl->d_len || vl->d_h0 || vl->d_c0); }
/* remembers what the forward ran with and gives the tensor the forward and d_W's product read: x itself, or -- ragged -- its copy with
 * the padding steps cleared (they may hold NaN) */
static const float *train_vl_begin(rec_train *t, const nntk_train_vl *vl, const float *d_x, int B, int T, int in) {
    t->have_batch = 0;           /* until this forward has been enqueued whole: a gradient call must not pair new lengths with old caches */
    t->bd_role = 0;              /* (a bidirectional forward sets it again once both directions are enqueued) */
    memset(&t->vl, 0, sizeof t->vl);
    if (!vl) return d_x;
    t->vl.d_len = vl->d_len; t->vl.max_len = vl->max_len; t->vl.d_h0 = vl->d_h0; t->vl.d_c0 = vl->d_c0;
    if (!vl->d_len) return d_x;
    float *d_xm = nntk_devbuf_reserve(&t->d_xm, (size_t)B * T * in);
    if (!d_xm || nntk_shim_train_mask_rows(d_x, vl->d_len, d_xm, B, T, in)) return NULL;
    return d_xm;
}
/* d_U += h0^T d_hU_0: the step-0 rows of the recurrent gate gradients d_G [B][T][K] against the carried-in state (the time-shifted product
 * reads zeros there) */
static int train_vl_dU_h0(rec_train *t, const float *d_G, float *d_dU, int B, int T, int H, int K) {
    if (!t->vl.d_h0) return 0;
    float *s0 = nntk_devbuf_reserve(&t->d_s0, (size_t)B * K + K);
    if (!s0) return -1;
    if (nntk_shim_copy_rows_d2d(s0, d_G, (size_t)T * K * sizeof(float), (size_t)K * sizeof(float), (size_t)B)) return -1;
    if (nntk_shim_memset(s0 + (size_t)B * K, 0, (size_t)K * sizeof(float))) return -1;
    return nntk_train_outer_accumulate(t->vl.d_h0, s0, d_dU, s0 + (size_t)B * K, (long)B, H, K, 0);
}

/* the raw block W | U | b_i | b_h on the device (caller layout), as the training kernels read it */
typedef struct { const float *W, *U, *bi, *bh; } raw_block;

/* The forward on the register-resident kernels' TRAIN instantiation (GRU, LSTM; standard activations, any mini-batch): ONE launch, the
 * caches written from the kernel's gate phase.  Its weight images are re-packed from the live weights every call (they change with every
 * optimiser step), so the test is made on the live host block, not on what core_upload saw, and the kernels run the f32-input form.
 * 0 = ran; 1 = not taken; -1 = error */
static int train_forward_rr(rec_layer *l, const float *d_x, const raw_block *raw, const nntk_train_vl *vl) {
    rec_core *c = &l->core;
    rec_train *t = &l->train;
    const int B = t->mini_batch, T = c->T, in = c->in, H = c->H, G = c->G, gru = G == 3;
    const size_t img = nntk_shim_lstm_rr_image_floats(H, in);
    if (rr_why_not(l, 0, img != 0) || rr_unsplittable(c->wb.host, (size_t)in * G * H + (size_t)H * G * H)) return 1;
    if (!gru && !c->d_rr_train && !(c->d_rr_train = (float *)nntk_shim_malloc(img * sizeof(float)))) return -1;       /* (the GRU's: its image builder) */
    float *d_wk = nntk_devbuf_reserve(&c->d_work_rr, nntk_shim_lstm_rr_work_floats(B, H));
    if (!d_wk) return -1;
    const float *bi = raw->bi, *bh = l->use_bh ? raw->bh : NULL;
    if (gru) {      /* packed on the host (four slots), its bias vector holds b_h */
        if (gru_rr_build_image(in, H, c->weights->W, c->weights->U, c->weights->b_i, c->weights->b_h, &c->d_rr_train, img, &c->d_b4_train, &c->d_rr_stage, NULL)) return -1;
        bi = c->d_b4_train, bh = NULL;
    } else if (nntk_shim_lstm_rr_pack_raw(raw->U, raw->W, c->d_rr_train, H, in))        /* packed on the device from the block just uploaded */
        return -1;
    float *d_hs = nntk_devbuf_reserve(&c->d_hseq, nntk_shim_rr_hseq_floats(B, T, H));
    if (!d_hs) return -1;
    float *d_h = t->d_h.p, *d_Zg = t->d_Zg.p, *d_hU = t->d_hU.p;
    if (!train_vl_active(vl))
        return gru ? nntk_shim_gru_rr_train_forward(d_x, c->d_rr_train, bi, d_h, d_hU, d_Zg, d_hs, d_wk, B, T, in, H)
                   : nntk_shim_lstm_rr_train_forward(d_x, c->d_rr_train, bi, bh, d_h, d_hU, d_Zg, d_hs, d_wk, B, T, in, H);
    /* the same kernel's TRAIN + VL instantiation: lengths, h0 (c0) in, hT (cT) out */
    const int rc = nntk_shim_rr_train_forward_vl(gru, d_x, c->d_rr_train, bi, bh, vl->d_h0, vl->d_c0, d_h, d_hU, d_Zg, t->want_hT, t->want_cT,
                                                 d_hs, d_wk, vl->d_len, B, T, in, H);
    if (rc == 0 && nntk_shim_varlen_zero_pad(d_h, vl->d_len, B, T, H)) return -1;
    if (rc == 0) t->want_hT = t->want_cT = NULL;
    return rc;
}

/* forward over the mini-batch with the caches kept for the gradient; d_x is a device tensor that stays valid until the gradient call */
static int layer_train_forward(rec_layer *l, const float *d_x, const nntk_train_vl *vl) {
    if (layer_acts(l)) return -1;
    rec_core *c = &l->core;
    rec_train *t = &l->train;
    const int B = t->mini_batch, T = c->T, in = c->in, H = c->H, G = c->G;
    const size_t w = (size_t)in * G * H, u = (size_t)H * G * H, b = (size_t)G * H, rows = (size_t)B * T;
    float *d_h = nntk_devbuf_reserve(&t->d_h, rows * H);
    float *d_Zg = nntk_devbuf_reserve(&t->d_Zg, rows * (G == 1 ? 1 : 2 * G) * H);
    float *d_hU = G == 1 ? d_h : nntk_devbuf_reserve(&t->d_hU, rows * H);          /* (the RNN keeps no second cache) */
    float *d_raw = nntk_devbuf_reserve(&t->d_raw, w + u + 2 * b);
    if (!d_h || !d_Zg || !d_hU || !d_raw) return -1;
    if (nntk_shim_upload(d_raw, c->wb.host, (w + u + 2 * b) * sizeof(float))) return -1;
    const raw_block raw = { d_raw, d_raw + w, d_raw + w + u, d_raw + w + u + b };
    if (!(d_x = train_vl_begin(t, vl, d_x, B, T, in))) return -1;
    int rc = G == 1 ? 1 : train_forward_rr(l, d_x, &raw, vl);
    if (rc < 0) return -1;
    if (rc) {
        if (nntk_shim_rec_train_forward(G, d_x, raw.W, raw.U, raw.bi, raw.bh, d_h, d_Zg, d_hU, B, T, in, H, l->use_bh ? 1 : 0, l->acts, l->scales,
                                        train_vl_active(vl) ? vl : NULL))
            return -1;
    }
    t->d_x_cur = d_x;
    t->have_batch = 1;
    return 0;
}

/* d_W, d_U, d_b_i, d_b_h are ADDED onto the caller's block d_grad = W [in][G H] | U [H][G H] | b_i [G H] | b_h [G H]
 * (recurrent_gradient_sum per (b, t), gru.c:508; lstm.c:412-415), d_dX [B][T][in] is overwritten; d_dout [B][T][H] or [B][H] */
static int layer_train_gradient(rec_layer *l, const float *d_dout, float *d_grad, float *d_dX, const nntk_train_vl *vl) {
    rec_core *c = &l->core;
    rec_train *t = &l->train;
    if (layer_acts(l)) return -1;
    const int B = t->mini_batch, T = c->T, in = c->in, H = c->H, G = c->G, K = G * H, rs = c->return_sequences ? 1 : 0;
    const size_t w = (size_t)in * K, u = (size_t)H * K, rows = (size_t)B * T;
    /* the gate gradients [B][T][K]: the GRU's differ between the input side (d_xW) and the recurrent side (d_hU), the other cells have one */
    float *d_dxW = nntk_devbuf_reserve(&t->d_dxW, rows * K);
    float *d_dhU = G == 3 ? nntk_devbuf_reserve(&t->d_dhU, rows * K) : d_dxW;
    float *d_work = nntk_devbuf_reserve(&t->d_work, nntk_shim_rec_train_work_floats(G, B, H));
    float *d_UT = nntk_devbuf_reserve(&t->d_scr, u);
    if (!d_dxW || !d_dhU || !d_work || !d_UT) return -1;
    const float *dW = t->d_raw.p, *dU = dW + w;
    if (nntk_shim_transpose(dU, d_UT, H, K, 0)) return -1;                  /* U^T [K][H]: coalesced per-step product */
    if (nntk_shim_rec_train_backward(G, d_dout, d_UT, t->d_h.p, t->d_Zg.p, t->d_hU.p, d_dxW, d_dhU, d_work, B, T, H, rs, l->acts, l->scales, vl)) return -1;
    /* d_W += x^T d_xW, d_b_i += colsum d_xW;  d_U += h_prev^T d_hU, d_b_h += colsum d_hU;  d_X = d_xW W^T */
    if (nntk_train_outer_accumulate(t->d_x_cur, d_dxW, d_grad, d_grad + w + u, (long)rows, in, K, 0)) return -1;
    if (nntk_train_outer_accumulate(t->d_h.p, d_dhU, d_grad + w, d_grad + w + u + K, (long)rows, H, K, T)) return -1;
    if (vl && train_vl_dU_h0(t, d_dhU, d_grad + w, B, T, H, K)) return -1;
    return nntk_train_rows_times_rowmat(d_dxW, dW, d_dX, (long)rows, in, K);
}
/* what the last forward ran with, for a gradient call that brings no state gradients of its own */
static const nntk_train_vl *train_last_vl(const rec_train *t) { return train_vl_active(&t->vl) ? &t->vl : NULL; }

/* runs the forward and hands out what the call asked for from the h (c) cache: the output (d_output NULL: none), the final state.
 * vl NULL: the fixed-length, zero-state call */
static int train_forward_out(rec_layer *l, const float *d_input, float *d_output, const nntk_train_vl *vl, float *d_hT, float *d_cT) {
    rec_core *c = &l->core;
    rec_train *t = &l->train;
    const int B = t->mini_batch, T = c->T, H = c->H;
    const int *d_len = vl ? vl->d_len : NULL;
    t->want_hT = d_hT; t->want_cT = d_cT;
    const int frc = layer_train_forward(l, d_input, vl);
    d_hT = t->want_hT; d_cT = t->want_cT;       /* NULL again when the forward kernel wrote them itself */
    t->want_hT = t->want_cT = NULL;
    if (frc) return -1;
    const float *d_h = t->d_h.p;
    if (d_output) {
        int rc;
        if (c->return_sequences) rc = nntk_shim_copy_d2d(d_output, d_h, (size_t)B * T * H * sizeof(float));      /* rows past a length: zeros */
        else if (d_len) rc = nntk_shim_train_final_state(d_h, d_len, vl->d_h0, d_output, B, T, H);
        /* the last step of every sequence (gru.c:286-291, lstm.c:466-471, rnn.c:283-288): one strided copy */
        else rc = nntk_shim_copy_rows_d2d(d_output, d_h + (size_t)(T - 1) * H, (size_t)T * H * sizeof(float), (size_t)H * sizeof(float), (size_t)B);
        if (rc) return -1;
    }
    if (d_hT && nntk_shim_train_final_state(d_h, d_len, vl->d_h0, d_hT, B, T, H)) return -1;
    if (d_cT && nntk_shim_train_final_state(t->d_hU.p, d_len, vl->d_c0, d_cT, B, T, H)) return -1;
    return 0;
}

/* ---- the fixed-length calls: every row T steps from zero state ---- */
/* device-pointer form: d_input [B][T][in] must stay valid until the gradient call; d_output [B][T][H] or [B][H], or NULL */
static int train_apply_dev(rec_layer *l, const char *who, const float *d_input, float *d_output) {
    if (!l->train.on) return rec_fail(who, "the handle was created for inference");      /* gru.c:247-249, lstm.c:419-421, rnn.c:250-252 */
    if (l->train.mini_batch <= 0 || l->core.T <= 0) return 0;
    return train_forward_out(l, d_input, d_output, NULL, NULL, NULL);
}
static int train_apply_host(rec_layer *l, const char *who, const float *input, float *output) {
    rec_core *c = &l->core;
    rec_train *t = &l->train;
    if (!t->on) return rec_fail(who, "the handle was created for inference");
    const int B = t->mini_batch, T = c->T, in = c->in, H = c->H;
    if (B <= 0 || T <= 0) return 0;
    float *d_x = nntk_devbuf_reserve(&t->d_x, (size_t)B * T * in);
    if (!d_x) return -1;
    if (nntk_shim_upload(d_x, input, (size_t)B * T * in * sizeof(float))) return -1;
    if (train_forward_out(l, d_x, NULL, NULL, NULL, NULL)) return -1;
    const float *d_h = t->d_h.p;
    if (c->return_sequences) return nntk_shim_download(output, d_h, (size_t)B * T * H * sizeof(float));
    return nntk_shim_download_rows(output, d_h + (size_t)(T - 1) * H, (size_t)T * H * sizeof(float), (size_t)H * sizeof(float), (size_t)B);
}
/* Enqueued on the calling thread's stream (the forward call that precedes it synchronised that stream once for its weight upload).
 * cell: "GRU" / "LSTM" / "RNN", for the message */
static int train_gradient_dev(rec_layer *l, const char *who, const char *cell, float *d_grad, float *d_dX, const float *d_dout) {
    if (!d_grad || !d_dX || !d_dout) return rec_fail(who, "NULL argument");
    if (!l->train.on || !l->train.have_batch) return rec_fail(who, "run %sApplyTrainingBatch[Device] on a training handle first", cell);
    return layer_train_gradient(l, d_dout, d_grad, d_dX, train_last_vl(&l->train));
}
/* void in the reference; errors through nntk_last_error() */
static void train_gradient_host(rec_layer *l, const char *who, const char *cell, RecurrentGradient *gradient, const float *d_out) {
    rec_core *c = &l->core;
    rec_train *t = &l->train;
    if (!t->on || !t->have_batch) { (void)rec_fail(who, "run %sApplyTrainingBatch on a training handle first", cell); return; }
    const int B = t->mini_batch, T = c->T, in = c->in, H = c->H, G = c->G;
    const size_t nblk = (size_t)in * G * H + (size_t)H * G * H + 2 * (size_t)G * H, rows = (size_t)B * T;
    const size_t n_do = c->return_sequences ? rows * H : (size_t)B * H;
    float *d_dout = nntk_devbuf_reserve(&t->d_dout, n_do);
    float *d_grad = nntk_devbuf_reserve(&t->d_grad, nblk);
    float *d_dX = nntk_devbuf_reserve(&t->d_dX, rows * in);
    if (!d_dout || !d_grad || !d_dX) return;
    if (nntk_shim_upload(d_dout, d_out, n_do * sizeof(float))) return;
    if (nntk_shim_upload(d_grad, gradient->d_W, nblk * sizeof(float))) return;       /* the block is contiguous */
    if (layer_train_gradient(l, d_dout, d_grad, d_dX, train_last_vl(t))) return;
    if (nntk_shim_download(gradient->d_W, d_grad, nblk * sizeof(float))) return;
    nntk_shim_download(gradient->d_X, d_dX, rows * in * sizeof(float));
}
/* (the entry points of the void call check all three of their arguments at once) */
#define REC_ENTER_GRADIENT(who, args_ok) do { nntk_shim_clear_error(); if (!(args_ok)) { nntk_set_error(who ": NULL argument"); return; } } while (0)

/* ---- the *VarLen calls: lengths (host memory; NULL: every row T) and carried state; c0 / cT and their gradients: LSTM only ---- */
static int train_apply_vl_dev(rec_layer *l, const char *who, const float *d_input, float *d_output, const int *lengths,
                              const float *d_h0, const float *d_c0, float *d_hT, float *d_cT) {
    rec_core *c = &l->core;
    rec_train *t = &l->train;
    if (!t->on) return rec_fail(who, "the handle was created for inference");
    const int B = t->mini_batch, T = c->T, lstm = c->G == 4;
    nntk_train_vl vl;
    memset(&vl, 0, sizeof vl);
    if (nntk_check_lengths(who, lengths, B, T, NULL, &vl.max_len)) return -1;
    if (B <= 0 || T <= 0) return 0;
    if (!d_input) return rec_fail(who, "NULL input");
    vl.d_h0 = d_h0;
    vl.d_c0 = lstm ? d_c0 : NULL;
    /* (a carried-in state alone: every row T) */
    if ((lengths || vl.d_h0 || vl.d_c0) && !(vl.d_len = stage_lengths(&t->d_len, lengths, B, T, 0))) return -1;
    return train_forward_out(l, d_input, d_output, &vl, d_hT, lstm ? d_cT : NULL);
}
static int train_gradient_vl_dev(rec_layer *l, const char *who, float *d_grad, float *d_dX, const float *d_dout,
                                 const float *d_dhT, const float *d_dcT, float *d_dh0, float *d_dc0) {
    rec_train *t = &l->train;
    const int lstm = l->core.G == 4;
    if (!d_grad || !d_dX || !d_dout) return rec_fail(who, "NULL argument");
    if (!t->on || !t->have_batch) return rec_fail(who, "run the forward call on a training handle first");
    nntk_train_vl vl = t->vl;
    vl.d_dhT = d_dhT; vl.d_dh0 = d_dh0;
    vl.d_dcT = lstm ? d_dcT : NULL; vl.d_dc0 = lstm ? d_dc0 : NULL;
    return layer_train_gradient(l, d_dout, d_grad, d_dX, &vl);
}
/* host-memory forms: upload, device call, download; the state tensors live in the handle (h0 / c0 until the gradient call) */
static int train_apply_vl_host(rec_layer *l, const char *who, const float *input, float *output, const int *lengths,
                               const float *h0, const float *c0, float *hT, float *cT) {
    rec_core *c = &l->core;
    rec_train *t = &l->train;
    if (!t->on) return rec_fail(who, "the handle was created for inference");
    const int B = t->mini_batch, T = c->T, in = c->in, H = c->H, lstm = c->G == 4;
    if (nntk_check_lengths(who, lengths, B, T, NULL, NULL)) return -1;
    if (B <= 0 || T <= 0) return 0;
    if (!input || !output) return rec_fail(who, "NULL argument");
    const size_t BH = (size_t)B * H, n_out = c->return_sequences ? (size_t)B * T * H : BH;
    float *d_x = nntk_devbuf_reserve(&t->d_x, (size_t)B * T * in);
    float *d_st = nntk_devbuf_reserve(&t->d_st, 8 * BH);
    float *d_out = nntk_devbuf_reserve(&t->d_yo, n_out);
    if (!d_x || !d_st || !d_out) return -1;
    float *d_h0 = h0 ? d_st : NULL, *d_c0 = (lstm && c0) ? d_st + BH : NULL;
    float *d_hT = hT ? d_st + 2 * BH : NULL, *d_cT = (lstm && cT) ? d_st + 3 * BH : NULL;
    if (nntk_shim_upload(d_x, input, (size_t)B * T * in * sizeof(float))) return -1;
    if (d_h0 && nntk_shim_upload(d_h0, h0, BH * sizeof(float))) return -1;
    if (d_c0 && nntk_shim_upload(d_c0, c0, BH * sizeof(float))) return -1;
    if (train_apply_vl_dev(l, who, d_x, d_out, lengths, d_h0, d_c0, d_hT, d_cT)) return -1;
    if (d_hT && nntk_shim_download(hT, d_hT, BH * sizeof(float))) return -1;
    if (d_cT && nntk_shim_download(cT, d_cT, BH * sizeof(float))) return -1;
    return nntk_shim_download(output, d_out, n_out * sizeof(float));
}
static int train_gradient_vl_host(rec_layer *l, const char *who, RecurrentGradient *gradient, const float *d_out,
                                  const float *hT_grad, const float *cT_grad, float *h0_grad, float *c0_grad) {
    rec_core *c = &l->core;
    rec_train *t = &l->train;
    if (!gradient || !d_out) return rec_fail(who, "NULL argument");
    if (!t->on || !t->have_batch) return rec_fail(who, "run the forward call on a training handle first");
    const int B = t->mini_batch, T = c->T, in = c->in, H = c->H, G = c->G, lstm = G == 4;
    const size_t nblk = (size_t)in * G * H + (size_t)H * G * H + 2 * (size_t)G * H, rows = (size_t)B * T, BH = (size_t)B * H;
    const size_t n_do = c->return_sequences ? rows * H : BH;
    float *d_dout = nntk_devbuf_reserve(&t->d_dout, n_do);
    float *d_grad = nntk_devbuf_reserve(&t->d_grad, nblk);
    float *d_dX = nntk_devbuf_reserve(&t->d_dX, rows * in);
    float *d_st = nntk_devbuf_reserve(&t->d_st, 8 * BH);      /* (already this size when the forward went through the host form: h0 / c0 stay) */
    if (!d_dout || !d_grad || !d_dX || !d_st) return -1;
    float *d_dhT = hT_grad ? d_st + 4 * BH : NULL, *d_dcT = (lstm && cT_grad) ? d_st + 5 * BH : NULL;
    float *d_dh0 = h0_grad ? d_st + 6 * BH : NULL, *d_dc0 = (lstm && c0_grad) ? d_st + 7 * BH : NULL;
    if (nntk_shim_upload(d_dout, d_out, n_do * sizeof(float))) return -1;
    if (nntk_shim_upload(d_grad, gradient->d_W, nblk * sizeof(float))) return -1;       /* the block is contiguous */
    if (d_dhT && nntk_shim_upload(d_dhT, hT_grad, BH * sizeof(float))) return -1;
    if (d_dcT && nntk_shim_upload(d_dcT, cT_grad, BH * sizeof(float))) return -1;
    if (train_gradient_vl_dev(l, who, d_grad, d_dX, d_dout, d_dhT, d_dcT, d_dh0, d_dc0)) return -1;
    if (nntk_shim_download(gradient->d_W, d_grad, nblk * sizeof(float))) return -1;
    if (d_dh0 && nntk_shim_download(h0_grad, d_dh0, BH * sizeof(float))) return -1;
    if (d_dc0 && nntk_shim_download(c0_grad, d_dc0, BH * sizeof(float))) return -1;
    return nntk_shim_download(gradient->d_X, d_dX, rows * in * sizeof(float));
}

/* ============================ bidirectional helpers ======================== */
/* layers/bidirectional.c forward helpers.  The device forms are the product; the host-pointer forms keep the
 * reference's signatures (void, caller-owned host buffers) and stage through device scratch. */

/* scratch of the host-pointer helpers: per calling thread (they have no handle to own it) */
#define g_bd_a (*nntk_thread_scratch(NNTK_TS_BD_A))
#define g_bd_b (*nntk_thread_scratch(NNTK_TS_BD_B))
#define g_bd_out (*nntk_thread_scratch(NNTK_TS_BD_OUT))
#define g_bd_len (*nntk_thread_scratch(NNTK_TS_BD_LEN))

int bd_reverse_input_batch_device(const float *d_input, float *d_output, RecurrentConfig config, int batch) {
    nntk_shim_clear_error();
    return nntk_shim_reverse_time(d_input, d_output, batch, config.timesteps, config.input_feature_channels);
}
int bd_reverse_backward_batch_device(const float *d_input, float *d_output, RecurrentConfig config, int batch) {
    nntk_shim_clear_error();
    return nntk_shim_reverse_time(d_input, d_output, batch, config.timesteps, config.output_feature_channels);
}
/* ragged rows: reverse each row's first lengths[b] steps, zeros after (lengths: host memory, as the *VarLen calls) */
static int bd_reverse_varlen(const char *who, const float *d_in, float *d_out, int T, int F, int batch, const int *lengths) {
    nntk_shim_clear_error();
    if (batch < 0) return rec_fail(who, "batch %d < 0", batch);
    if (!lengths) NNTK_FAIL("bd_reverse_*_varlen_device: NULL lengths");
    if (nntk_check_lengths(who, lengths, batch, T, NULL, NULL)) return -1;
    if (batch == 0 || T <= 0 || F <= 0) return 0;
    int *d_len = (int *)nntk_devbuf_reserve(&g_bd_len, (size_t)batch);
    if (!d_len || nntk_shim_upload_ints(d_len, lengths, batch)) return -1;
    return nntk_shim_reverse_time_varlen(d_in, d_out, d_len, batch, T, F);
}
int bd_reverse_input_batch_varlen_device(const float *d_input, float *d_output, RecurrentConfig config, int batch, const int *lengths) {
    return bd_reverse_varlen("bd_reverse_input_batch_varlen_device", d_input, d_output, config.timesteps, config.input_feature_channels,
                             batch, lengths);
}
int bd_reverse_backward_batch_varlen_device(const float *d_input, float *d_output, RecurrentConfig config, int batch, const int *lengths) {
    return bd_reverse_varlen("bd_reverse_backward_batch_varlen_device", d_input, d_output, config.timesteps, config.output_feature_channels,
                             batch, lengths);
}
int bd_merge_concat_device(const float *d_forward, const float *d_backward, float *d_output, RecurrentConfig config, int batch) {
    nntk_shim_clear_error();
    long rows = (long)batch * (config.return_sequences ? config.timesteps : 1);
    return nntk_shim_concat2(d_forward, d_backward, d_output, rows, config.output_feature_channels);
}
int bd_merge_sum_device(const float *d_forward, const float *d_backward, float *d_output, RecurrentConfig config, int batch) {
    nntk_shim_clear_error();
    long rows = (long)batch * (config.return_sequences ? config.timesteps : 1);
    return nntk_shim_add2(d_forward, d_backward, d_output, rows * config.output_feature_channels);
}

static void bd_reverse_host(const float *input, float *output, int batch, int T, int F) {
    nntk_shim_clear_error();
    size_t n = (size_t)batch * T * F;
    if (!n) return;
    float *d_in = nntk_devbuf_reserve(&g_bd_a, n), *d_out = nntk_devbuf_reserve(&g_bd_out, n);
    if (!d_in || !d_out) return;
    if (nntk_shim_upload(d_in, input, n * sizeof(float))) return;
    if (nntk_shim_reverse_time(d_in, d_out, batch, T, F)) return;
    (void)nntk_shim_download(output, d_out, n * sizeof(float));
}
/* bidirectional.c:25-35 */
void bd_reverse_input_batch(const float *input, float *output, RecurrentConfig config, int batch) {
    bd_reverse_host(input, output, batch, config.timesteps, config.input_feature_channels);
}
void bd_reverse_backward_batch(const float *input, float *output, RecurrentConfig config, int batch) {
    bd_reverse_host(input, output, batch, config.timesteps, config.output_feature_channels);
}
/* bidirectional.c:37-40 */
int bd_merge_concat_buffer_size(RecurrentConfig config) {
    int rows = config.return_sequences ? config.timesteps : 1;
    return 2 * rows * config.output_feature_channels;
}
static void bd_merge_host(const float *fwd, const float *bwd, float *output, RecurrentConfig config, int batch, int concat) {
    nntk_shim_clear_error();
    size_t n = (size_t)batch * (config.return_sequences ? config.timesteps : 1) * config.output_feature_channels;
    if (!n) return;
    float *d_a = nntk_devbuf_reserve(&g_bd_a, n), *d_b = nntk_devbuf_reserve(&g_bd_b, n);
    float *d_out = nntk_devbuf_reserve(&g_bd_out, concat ? 2 * n : n);
    if (!d_a || !d_b || !d_out) return;
    if (nntk_shim_upload(d_a, fwd, n * sizeof(float)) || nntk_shim_upload(d_b, bwd, n * sizeof(float))) return;
    int rc = concat ? bd_merge_concat_device(d_a, d_b, d_out, config, batch) : bd_merge_sum_device(d_a, d_b, d_out, config, batch);
    if (rc) return;
    (void)nntk_shim_download(output, d_out, (concat ? 2 * n : n) * sizeof(float));
}
/* bidirectional.c:42-58: per sequence, [rows, out] | [rows, out] -> [rows, 2*out] (the reference does it with three transposes) */
void bd_merge_concat(const float *forward_result, const float *backward_result, float *output,
                     RecurrentConfig config, int batch, float *buffer) {
    (void)buffer;
    bd_merge_host(forward_result, backward_result, output, config, batch, 1);
}
/* ---- gradient helpers (bidirectional.c:58-74, :87-108): pure data movement, as their forward counterparts ---- */
void bd_merge_concat_gradient(const float *d_out, float *d_forward_out, float *d_backward_out, RecurrentConfig config,
                              int batch, float *buffer) {
    (void)buffer;
    nntk_shim_clear_error();
    int rows = config.return_sequences ? config.timesteps : 1, C = config.output_feature_channels;
    size_t n = (size_t)batch * rows * C;
    if (!n) return;
    float *d_in = nntk_devbuf_reserve(&g_bd_out, 2 * n);
    float *d_a = nntk_devbuf_reserve(&g_bd_a, n), *d_b = nntk_devbuf_reserve(&g_bd_b, n);
    if (!d_in || !d_a || !d_b) return;
    if (nntk_shim_upload(d_in, d_out, 2 * n * sizeof(float))) return;
    if (nntk_shim_split2(d_in, d_a, d_b, (long)batch * rows, C)) return;
    if (nntk_shim_download(d_forward_out, d_a, n * sizeof(float))) return;
    (void)nntk_shim_download(d_backward_out, d_b, n * sizeof(float));
}
void bd_merge_sum_gradient(const float *d_out, float *d_forward_out, float *d_backward_out, RecurrentConfig config, int batch) {
    size_t n = (size_t)batch * (config.return_sequences ? config.timesteps : 1) * config.output_feature_channels;
    memcpy(d_forward_out, d_out, n * sizeof(float));        /* f_copy twice (bidirectional.c:95-96): no arithmetic */
    memcpy(d_backward_out, d_out, n * sizeof(float));
}
/* output = forward_dx + time-reversed backward_dx (bidirectional.c:99-108) */
void bd_accumulate_d_x(const float *forward_dx, const float *backward_dx, float *output, RecurrentConfig config, int batch) {
    nntk_shim_clear_error();
    size_t n = (size_t)batch * config.timesteps * config.input_feature_channels;
    if (!n) return;
    float *d_a = nntk_devbuf_reserve(&g_bd_a, n), *d_b = nntk_devbuf_reserve(&g_bd_b, n), *d_o = nntk_devbuf_reserve(&g_bd_out, n);
    if (!d_a || !d_b || !d_o) return;
    if (nntk_shim_upload(d_a, forward_dx, n * sizeof(float)) || nntk_shim_upload(d_b, backward_dx, n * sizeof(float))) return;
    if (nntk_shim_reverse_time(d_b, d_o, batch, config.timesteps, config.input_feature_channels)) return;
    if (nntk_shim_add2(d_a, d_o, d_o, (long)n)) return;
    (void)nntk_shim_download(output, d_o, n * sizeof(float));
}
/* bidirectional.c:76-85 */
void bd_merge_sum(const float *forward_result, const float *backward_result, float *output,
                  RecurrentConfig config, int batch) {
    bd_merge_host(forward_result, backward_result, output, config, batch, 0);
}

/* ---- device forms of the gradient helpers: thin wrappers over bd_train.hip.  The fixed-length ones keep the reference's contract
 * (d_backward is NOT reversed: bidirectional.c:58-74, :87-97; the reversal happens in bd_accumulate_d_x, :99-108) and return the bits of
 * the host forms above; the varlen ones serve ragged rows (lengths: host memory, NULL = every row T) and hand the backward direction its
 * gradient already reversed per row, zeros past a row's length. ---- */
static int bd_grad_args(const char *who, const void *a, const void *b, const void *c, int batch) {
    nntk_shim_clear_error();
    if (batch < 0) return rec_fail(who, "batch %d < 0", batch);
    if (batch > 0 && (!a || !b || !c)) return rec_fail(who, "NULL argument");
    return 0;
}
/* the row lengths on the device, in the calling thread's scratch: 0 and *d_len (NULL without lengths), or -1 */
static int bd_stage_lengths(const char *who, const int *lengths, int batch, int T, const int **d_len) {
    *d_len = NULL;
    if (nntk_check_lengths(who, lengths, batch, T, NULL, NULL)) return -1;
    if (!lengths || batch == 0) return 0;
    int *d = (int *)nntk_devbuf_reserve(&g_bd_len, (size_t)batch);
    if (!d || nntk_shim_upload_ints(d, lengths, batch)) return -1;
    *d_len = d;
    return 0;
}
int bd_merge_concat_gradient_device(const float *d_dout, float *d_forward, float *d_backward, RecurrentConfig config, int batch) {
    if (bd_grad_args("bd_merge_concat_gradient_device", d_dout, d_forward, d_backward, batch)) return -1;
    return nntk_shim_bd_scatter(d_dout, d_forward, d_backward, NULL, batch, config.timesteps, config.output_feature_channels,
                                config.return_sequences ? 1 : 0, 1, 0);
}
int bd_merge_sum_gradient_device(const float *d_dout, float *d_forward, float *d_backward, RecurrentConfig config, int batch) {
    if (bd_grad_args("bd_merge_sum_gradient_device", d_dout, d_forward, d_backward, batch)) return -1;
    return nntk_shim_bd_scatter(d_dout, d_forward, d_backward, NULL, batch, config.timesteps, config.output_feature_channels,
                                config.return_sequences ? 1 : 0, 0, 0);
}
int bd_accumulate_d_x_device(const float *d_forward_dx, const float *d_backward_dx, float *d_output, RecurrentConfig config, int batch) {
    if (bd_grad_args("bd_accumulate_d_x_device", d_forward_dx, d_backward_dx, d_output, batch)) return -1;
    return nntk_shim_bd_accumulate(d_forward_dx, d_backward_dx, d_output, NULL, batch, config.timesteps, config.input_feature_channels);
}
int bd_merge_gradient_varlen_device(const float *d_dout, float *d_forward, float *d_backward_reversed, RecurrentConfig config, int batch,
                                    const int *lengths, int merge) {
    const char *who = "bd_merge_gradient_varlen_device";
    if (bd_grad_args(who, d_dout, d_forward, d_backward_reversed, batch)) return -1;
    if (merge != NNTK_BD_MERGE_CONCAT && merge != NNTK_BD_MERGE_SUM)
        return rec_fail(who, "merge %d is neither NNTK_BD_MERGE_CONCAT nor NNTK_BD_MERGE_SUM", merge);
    const int *d_len;
    if (bd_stage_lengths(who, lengths, batch, config.timesteps, &d_len)) return -1;
    return nntk_shim_bd_scatter(d_dout, d_forward, d_backward_reversed, d_len, batch, config.timesteps, config.output_feature_channels,
                                config.return_sequences ? 1 : 0, merge == NNTK_BD_MERGE_CONCAT, 1);
}
int bd_accumulate_d_x_varlen_device(const float *d_forward_dx, const float *d_backward_dx, float *d_output, RecurrentConfig config, int batch,
                                    const int *lengths) {
    const char *who = "bd_accumulate_d_x_varlen_device";
    if (bd_grad_args(who, d_forward_dx, d_backward_dx, d_output, batch)) return -1;
    const int *d_len;
    if (bd_stage_lengths(who, lengths, batch, config.timesteps, &d_len)) return -1;
    return nntk_shim_bd_accumulate(d_forward_dx, d_backward_dx, d_output, d_len, batch, config.timesteps, config.input_feature_channels);
}

/* ============================ bidirectional layers in one call ======================== */
/* *BidirectionalApplyDevice (include/nntoolkitcore_hip.h): the result of the composed recipe -- reverse x per row, run each direction from
 * zero state, reverse the backward sequence output per row, merge -- bit for bit, on one of two routes:
 *   fused: both directions take the register-resident / full-K kernels (layer_takes_rr, the decision core_try_rr makes) ->
 *     one pack pass (x and x reversed per row into one frag3 tensor of 2 Bpad virtual rows) and ONE launch of the BD instantiations, which
 *     write the merged layout themselves (the sum merge: the backward half to scratch, then one add);
 *   composed: everything else (RNN, non-default activations, shapes those kernels do not take, option rec_rr = 0 or rec_bd = 0, weights the
 *     bf16 split cannot hold) -> the recipe itself, on the handles' own calls and scratch.
 * Both routes work on the FORWARD handle's scratch. */

/* everything that can fail is checked here, before anything is enqueued (dev: in / out are device pointers that must not overlap) */
static int bd_check(const rec_core *f, const rec_core *b, const char *who, const float *d_in, const float *d_out, int B, const int *lengths,
                    int merge, int dev, int *T_min) {
    if (f->in != b->in || f->H != b->H || f->T != b->T || f->return_sequences != b->return_sequences)
        return rec_fail(who, "the two directions differ in input size, hidden size, timesteps or return_sequences");
    if (merge != NNTK_BD_MERGE_CONCAT && merge != NNTK_BD_MERGE_SUM)
        return rec_fail(who, "merge %d is neither NNTK_BD_MERGE_CONCAT nor NNTK_BD_MERGE_SUM", merge);
    if (B < 0) return rec_fail(who, "batch %d < 0", B);
    const int T = f->T;
    if (nntk_check_lengths(who, lengths, B, T, T_min, NULL)) return -1;
    if (B == 0 || T <= 0) return 0;
    if (!d_in || !d_out) return rec_fail(who, "NULL input or output");
    const size_t W = merge == NNTK_BD_MERGE_CONCAT ? 2 * (size_t)f->H : (size_t)f->H;
    const size_t n_in = (size_t)B * T * f->in, n_out = (size_t)B * (f->return_sequences ? (size_t)T : 1) * W;
    if (dev && (const char *)d_in < (const char *)(d_out + n_out) && (const char *)d_out < (const char *)(d_in + n_in))
        return rec_fail(who, "the output buffer overlaps the input");
    return 0;
}

/* the fused route: 0 = ran; 1 = not taken (nothing that matters enqueued); -1 = error */
static int bd_fused(rec_layer *lf, rec_layer *lb, const float *d_in, float *d_out, int B, const int *lengths, int merge, int T_min) {
    rec_core *f = &lf->core, *b = &lb->core;
    int bd = -1;
    (void)nntk_shim_get_option("rec_bd", &bd);
    if (bd == 0 || !layer_takes_rr(lf) || !layer_takes_rr(lb)) return 1;
    const int H = f->H, T = f->T, in = f->in, gru = f->G == 3;
    const int rs = f->return_sequences, concat = merge == NNTK_BD_MERGE_CONCAT;
    /* (the concat merge's rows are 2H wide: a tile of them may pass the kernels' 32-bit offsets where one direction's rows do not) */
    if (!nntk_shim_rr_bd_fits(T, in, concat ? 2 * H : H)) return 1;
    if (layer_rr_images(lf) || layer_rr_images(lb)) return -1;
    /* the virtual batch: forward rows [0, Bp), backward rows [Bp, 2 Bp) */
    const int Bv = 2 * 64 * ((B + 63) / 64);
    const int *d_len = stage_lengths(&f->d_len, lengths, B, T, 1);
    if (!d_len) return -1;
    const size_t n_dir = (size_t)B * (rs ? (size_t)T : 1) * H;
    float *xf3 = nntk_devbuf_reserve(&f->d_xf3, nntk_shim_frag3_floats(Bv, T, in));
    float *d_work = nntk_devbuf_reserve(&f->d_work_rr, nntk_shim_lstm_rr_work_floats(Bv, H));
    float *d_hseq = nntk_devbuf_reserve(&f->d_hseq, nntk_shim_rr_hseq_floats(Bv, T, H));
    float *d_bwd = concat ? d_out + H : nntk_devbuf_reserve(&f->d_bd, n_dir);
    if (!xf3 || !d_work || !d_hseq || !d_bwd) return -1;
    if (nntk_shim_frag3_pack_bd(d_in, d_len, xf3, B, T, in)) return -1;            /* (d_len's first B entries: the forward rows = the call's lengths) */
    const float *bi_f = gru ? f->d_b4 : f->d_bi, *bi_b = gru ? b->d_b4 : b->d_bi;
    const float *bh_f = !gru && lf->use_bh ? f->d_bh : NULL, *bh_b = !gru && lb->use_bh ? b->d_bh : NULL;
    const int rc = nntk_shim_rr_bd(gru, xf3, f->d_rr, f->d_rr4, bi_f, bh_f, b->d_rr, b->d_rr4, bi_b, bh_b, d_out, d_bwd,
                                   concat ? 2 * H : H, d_hseq, d_work, d_len, B, T, in, H, rs);
    /* 1: the launcher declined after all (the persistent kernels disabled after a fault, too few resident workgroups) -- the pack pass and
     * the uploads above were wasted but harmless, and the caller runs the composed route */
    if (rc) return rc;
    if (!concat && nntk_shim_add2(d_out, d_bwd, d_out, (long)n_dir)) return -1;
    return rs && T_min < T ? nntk_shim_varlen_zero_pad(d_out, d_len, B, T, concat ? 2 * H : H) : 0;
}

/* the composed route: the recipe of bd_reverse_*[_varlen]_device, *ApplyDevice[VarLen] twice and bd_merge_*_device */
static int bd_composed(rec_layer *lf, rec_layer *lb, const char *who, const float *d_in, float *d_out, int B, const int *lengths, int merge) {
    rec_core *f = &lf->core;
    const int H = f->H, T = f->T, in = f->in, rs = f->return_sequences;
    const size_t n_in = (size_t)B * T * in, n_dir = (size_t)B * (rs ? (size_t)T : 1) * H;
    float *xr = nntk_devbuf_reserve(&f->d_bd, n_in + 3 * n_dir);
    if (!xr) return -1;
    float *of = xr + n_in, *obr = of + n_dir, *ob = obr + n_dir;
    int *d_len = NULL;
    if (lengths) {
        d_len = (int *)nntk_devbuf_reserve(&f->d_bd_len, (size_t)B);
        if (!d_len || nntk_shim_upload_ints(d_len, lengths, B)) return -1;
    }
    if (d_len ? nntk_shim_reverse_time_varlen(d_in, xr, d_len, B, T, in) : nntk_shim_reverse_time(d_in, xr, B, T, in)) return -1;
    if (lengths) {
        if (core_apply_device_vl(lf, who, d_in, of, B, lengths, NULL, NULL, NULL, NULL)) return -1;
        if (core_apply_device_vl(lb, who, xr, obr, B, lengths, NULL, NULL, NULL, NULL)) return -1;
    } else {
        if (core_apply_device(lf, d_in, of, B, 0)) return -1;
        if (core_apply_device(lb, xr, obr, B, 0)) return -1;
    }
    if (!rs) ob = obr;          /* the final states: no second reversal */
    else if (d_len ? nntk_shim_reverse_time_varlen(obr, ob, d_len, B, T, H) : nntk_shim_reverse_time(obr, ob, B, T, H)) return -1;
    return merge == NNTK_BD_MERGE_CONCAT ? nntk_shim_concat2(of, ob, d_out, (long)B * (rs ? T : 1), H) : nntk_shim_add2(of, ob, d_out, (long)n_dir);
}

static int core_apply_bd(rec_layer *lf, rec_layer *lb, const char *who, const float *d_in, float *d_out, int B, const int *lengths, int merge) {
    int T_min;
    if (bd_check(&lf->core, &lb->core, who, d_in, d_out, B, lengths, merge, 1, &T_min)) return -1;
    if (B == 0 || lf->core.T <= 0) return 0;
    if (core_ensure(&lf->core, 0) || core_ensure(&lb->core, 0)) return -1;
    const int rc = bd_fused(lf, lb, d_in, d_out, B, lengths, merge, T_min);
    if (rc <= 0) return rc;
    return bd_composed(lf, lb, who, d_in, d_out, B, lengths, merge);
}
static int run_apply_bd(const dev_call *k, const float *d_in, float *d_out) {
    return core_apply_bd(k->l, k->l2, k->who, d_in, d_out, k->B, k->lengths, k->merge);
}
static int core_apply_bd_host(rec_layer *lf, rec_layer *lb, const char *who, const float *input, float *output, int B, const int *lengths, int merge) {
    rec_core *f = &lf->core;
    int T_min;
    if (bd_check(f, &lb->core, who, input, output, B, lengths, merge, 0, &T_min)) return -1;
    if (B == 0 || f->T <= 0) return 0;
    if (core_ensure(f, 1) || core_ensure(&lb->core, 1)) return -1;
    const size_t W = merge == NNTK_BD_MERGE_CONCAT ? 2 * (size_t)f->H : (size_t)f->H;
    const size_t n_in = (size_t)B * f->T * f->in, n_out = (size_t)B * (f->return_sequences ? (size_t)f->T : 1) * W;
    float *d_in = nntk_devbuf_reserve(&f->d_in, n_in), *d_out = nntk_devbuf_reserve(&f->d_out, n_out);
    if (!d_in || !d_out) return -1;
    const dev_call k = { .run = run_apply_bd, .l = lf, .l2 = lb, .who = who, .B = B, .lengths = lengths, .merge = merge };
    const host_input in = { input, d_in, n_in };
    return host_round_trip(&k, &in, 1, d_out, output, n_out, 1);
}

/* ============================ bidirectional layers: training ======================== */
/* *BidirectionalApplyTrainingBatch[Device] / *BidirectionalCalculateGradient[Device] (include/nntoolkitcore_hip.h): the composed recipe on
 * two *CreateForTraining handles, bit for bit -- each direction IS its unidirectional *VarLen training call from zero state (train_apply_vl_dev
 * / train_gradient_vl_dev: same router, same kernels, same caches), and what lies around them is one pass each of bd_train.hip: the merge
 * with the backward output's reversal folded in, the scatter of d_out into both directions' output gradients, the sum of their input
 * gradients.  Each handle owns its direction's scratch (rec_train d_bd_*); the backward handle keeps x reversed per row, which its
 * gradient call reads.  Everything that can fail is checked before anything is enqueued or remembered. */

/* the pair itself: two different training handles of one shape */
static int bd_train_pair(const rec_layer *lf, const rec_layer *lb, const char *who) {
    const rec_core *f = &lf->core, *b = &lb->core;
    if (lf == lb) return rec_fail(who, "the same handle was passed for both directions (one handle holds one set of training caches)");
    if (!lf->train.on || !lb->train.on) return rec_fail(who, "the %s handle was created for inference", lf->train.on ? "backward" : "forward");
    if (f->G != b->G || f->in != b->in || f->H != b->H || f->T != b->T || f->return_sequences != b->return_sequences ||
        lf->train.mini_batch != lb->train.mini_batch)
        return rec_fail(who, "the two directions differ in input size, hidden size, timesteps, return_sequences or mini_batch_size");
    return 0;
}
static int bd_train_forward_check(rec_layer *lf, rec_layer *lb, const char *who, const float *in, const float *out, const int *lengths,
                                  int merge, int dev) {
    if (bd_train_pair(lf, lb, who)) return -1;
    if (merge != NNTK_BD_MERGE_CONCAT && merge != NNTK_BD_MERGE_SUM)
        return rec_fail(who, "merge %d is neither NNTK_BD_MERGE_CONCAT nor NNTK_BD_MERGE_SUM", merge);
    const rec_core *f = &lf->core;
    const int B = lf->train.mini_batch, T = f->T;
    if (nntk_check_lengths(who, lengths, B, T, NULL, NULL)) return -1;
    if (B <= 0 || T <= 0) return 0;
    if (!in || !out) return rec_fail(who, "NULL input or output");
    const size_t W = merge == NNTK_BD_MERGE_CONCAT ? 2 * (size_t)f->H : (size_t)f->H;
    const size_t n_in = (size_t)B * T * f->in, n_out = (size_t)B * (f->return_sequences ? (size_t)T : 1) * W;
    if (dev && (const char *)in < (const char *)(out + n_out) && (const char *)out < (const char *)(in + n_in))
        return rec_fail(who, "the output buffer overlaps the input");
    return layer_acts(lf) || layer_acts(lb) ? -1 : 0;
}
/* (after bd_train_forward_check) */
static int bd_train_forward_run(rec_layer *lf, rec_layer *lb, const char *who, const float *d_in, float *d_out, const int *lengths, int merge) {
    rec_core *f = &lf->core;
    rec_train *tf = &lf->train, *tb = &lb->train;
    const int B = tf->mini_batch, T = f->T, in = f->in, H = f->H, rs = f->return_sequences ? 1 : 0;
    if (B <= 0 || T <= 0) return 0;
    const size_t n_in = (size_t)B * T * in, n_dir = (size_t)B * (rs ? (size_t)T : 1) * H;
    float *of = nntk_devbuf_reserve(&tf->d_bd_o, n_dir), *obr = nntk_devbuf_reserve(&tb->d_bd_o, n_dir);
    float *xr = nntk_devbuf_reserve(&tb->d_bd_xr, n_in);
    if (!of || !obr || !xr) return -1;
    /* the forward direction first: it stages the lengths on the device, which the reversal and the merge read as well */
    if (train_apply_vl_dev(lf, who, d_in, of, lengths, NULL, NULL, NULL, NULL)) return -1;
    const int *d_len = tf->vl.d_len;
    if (d_len ? nntk_shim_reverse_time_varlen(d_in, xr, d_len, B, T, in) : nntk_shim_reverse_time(d_in, xr, B, T, in)) return -1;
    if (train_apply_vl_dev(lb, who, xr, obr, lengths, NULL, NULL, NULL, NULL)) return -1;
    if (nntk_shim_bd_merge(of, obr, d_out, d_len, B, T, H, rs, merge == NNTK_BD_MERGE_CONCAT)) return -1;
    tf->bd_role = 1; tf->bd_peer = lb; tf->bd_merge = merge;
    tb->bd_role = 2; tb->bd_peer = lf;
    return 0;
}
static int bd_train_forward_dev(rec_layer *lf, rec_layer *lb, const char *who, const float *d_in, float *d_out, const int *lengths, int merge) {
    if (bd_train_forward_check(lf, lb, who, d_in, d_out, lengths, merge, 1)) return -1;
    return bd_train_forward_run(lf, lb, who, d_in, d_out, lengths, merge);
}
static int bd_train_forward_host(rec_layer *lf, rec_layer *lb, const char *who, const float *input, float *output, const int *lengths, int merge) {
    if (bd_train_forward_check(lf, lb, who, input, output, lengths, merge, 0)) return -1;
    rec_core *f = &lf->core;
    const int B = lf->train.mini_batch, T = f->T;
    if (B <= 0 || T <= 0) return 0;
    const size_t W = merge == NNTK_BD_MERGE_CONCAT ? 2 * (size_t)f->H : (size_t)f->H;
    const size_t n_in = (size_t)B * T * f->in, n_out = (size_t)B * (f->return_sequences ? (size_t)T : 1) * W;
    float *d_x = nntk_devbuf_reserve(&lf->train.d_x, n_in), *d_out = nntk_devbuf_reserve(&lf->train.d_bd_host, n_out);
    if (!d_x || !d_out) return -1;
    if (nntk_shim_upload(d_x, input, n_in * sizeof(float))) return -1;
    if (bd_train_forward_run(lf, lb, who, d_x, d_out, lengths, merge)) return -1;
    return nntk_shim_download(output, d_out, n_out * sizeof(float));
}

/* the gradient call's pair: the handles of the last bidirectional forward, in its order, neither used for another forward since */
static int bd_train_gradient_check(rec_layer *lf, rec_layer *lb, const char *who) {
    if (bd_train_pair(lf, lb, who)) return -1;
    const rec_train *tf = &lf->train, *tb = &lb->train;
    if (!tf->have_batch || !tb->have_batch || tf->bd_role != 1 || tb->bd_role != 2 || tf->bd_peer != lb || tb->bd_peer != lf)
        return rec_fail(who, "run the bidirectional forward call on this pair of handles (forward, backward) first");
    return layer_acts(lf) || layer_acts(lb) ? -1 : 0;
}
/* d_gf / d_gb: the directions' blocks W | U | b_i | b_h, ADDED to; d_dX [B][T][in] written; d_dout in the forward call's output layout */
static int bd_train_gradient_run(rec_layer *lf, rec_layer *lb, const char *who, float *d_gf, float *d_gb, float *d_dX, const float *d_dout) {
    rec_core *f = &lf->core;
    rec_train *tf = &lf->train, *tb = &lb->train;
    const int B = tf->mini_batch, T = f->T, in = f->in, H = f->H, rs = f->return_sequences ? 1 : 0;
    if (B <= 0 || T <= 0) return 0;
    const size_t n_in = (size_t)B * T * in, n_dir = (size_t)B * (rs ? (size_t)T : 1) * H;
    float *dof = nntk_devbuf_reserve(&tf->d_bd_do, n_dir), *dob = nntk_devbuf_reserve(&tb->d_bd_do, n_dir);
    float *dxf = nntk_devbuf_reserve(&tf->d_bd_dx, n_in), *dxb = nntk_devbuf_reserve(&tb->d_bd_dx, n_in);
    if (!dof || !dob || !dxf || !dxb) return -1;
    /* Each direction's gradient is summed into a zeroed block of the handle's own and reaches the caller's block in ONE f32 add per element:
     * onto a zeroed block that is, bit for bit, what *CalculateGradientDeviceVarLen leaves there (it adds its row slices one by one onto
     * the block: zero + the same slices in the same order), and a second call onto the same block gives exactly twice the first. */
    const size_t nblk = (size_t)in * f->G * H + (size_t)H * f->G * H + 2 * (size_t)f->G * H;
    float *gf = nntk_devbuf_reserve(&tf->d_bd_g, nblk), *gb = nntk_devbuf_reserve(&tb->d_bd_g, nblk);
    if (!gf || !gb) return -1;
    const int *d_len = tf->vl.d_len;
    if (nntk_shim_bd_scatter(d_dout, dof, dob, d_len, B, T, H, rs, tf->bd_merge == NNTK_BD_MERGE_CONCAT, 1)) return -1;
    if (nntk_shim_memset(gf, 0, nblk * sizeof(float)) || nntk_shim_memset(gb, 0, nblk * sizeof(float))) return -1;
    if (train_gradient_vl_dev(lf, who, gf, dxf, dof, NULL, NULL, NULL, NULL)) return -1;
    if (train_gradient_vl_dev(lb, who, gb, dxb, dob, NULL, NULL, NULL, NULL)) return -1;
    if (nntk_shim_add_into(d_gf, gf, (long)nblk) || nntk_shim_add_into(d_gb, gb, (long)nblk)) return -1;
    return nntk_shim_bd_accumulate(dxf, dxb, d_dX, d_len, B, T, in);
}
static int bd_train_gradient_dev(rec_layer *lf, rec_layer *lb, const char *who, float *d_gf, float *d_gb, float *d_dX, const float *d_dout) {
    if (bd_train_gradient_check(lf, lb, who)) return -1;
    if (!d_gf || !d_gb || !d_dX || !d_dout) return rec_fail(who, "NULL argument");
    /* the two blocks and d_dX are written by different kernels of the call: one tensor in two roles would be added to twice or overwritten */
    const rec_core *f = &lf->core;
    const size_t nblk = (size_t)f->in * f->G * f->H + (size_t)f->H * f->G * f->H + 2 * (size_t)f->G * f->H;
    const size_t n_in = (size_t)(lf->train.mini_batch > 0 ? lf->train.mini_batch : 0) * (f->T > 0 ? f->T : 0) * f->in;
    if ((d_gf < d_gb + nblk && d_gb < d_gf + nblk) || (d_dX < d_gf + nblk && d_gf < d_dX + n_in) || (d_dX < d_gb + nblk && d_gb < d_dX + n_in))
        return rec_fail(who, "the gradient blocks and d_dX overlap");
    return bd_train_gradient_run(lf, lb, who, d_gf, d_gb, d_dX, d_dout);
}
/* host-memory form: the two gradient blocks go up, are added to and come down as *CalculateGradient's does; the layer's d_X [B][T][in] is
 * the caller's tensor (the blocks' own d_X fields are not written) */
static int bd_train_gradient_host(rec_layer *lf, rec_layer *lb, const char *who, RecurrentGradient *gf, RecurrentGradient *gb, float *d_X,
                                  const float *d_out) {
    if (bd_train_gradient_check(lf, lb, who)) return -1;
    if (!gf || !gb || !d_X || !d_out) return rec_fail(who, "NULL argument");
    rec_core *f = &lf->core;
    rec_train *tf = &lf->train, *tb = &lb->train;
    const int B = tf->mini_batch, T = f->T, in = f->in, H = f->H, G = f->G;
    if (B <= 0 || T <= 0) return 0;
    const size_t nblk = (size_t)in * G * H + (size_t)H * G * H + 2 * (size_t)G * H, n_in = (size_t)B * T * in;
    const size_t n_do = (size_t)B * (f->return_sequences ? (size_t)T : 1) * (tf->bd_merge == NNTK_BD_MERGE_CONCAT ? 2 * (size_t)H : (size_t)H);
    const size_t n_do4 = (n_do + 3) & ~(size_t)3;           /* d_dX behind it stays 16-byte aligned */
    float *d_dout = nntk_devbuf_reserve(&tf->d_bd_host, n_do4 + n_in);
    float *d_gf = nntk_devbuf_reserve(&tf->d_grad, nblk), *d_gb = nntk_devbuf_reserve(&tb->d_grad, nblk);
    if (!d_dout || !d_gf || !d_gb) return -1;
    float *d_dX = d_dout + n_do4;
    if (nntk_shim_upload(d_dout, d_out, n_do * sizeof(float))) return -1;
    if (nntk_shim_upload(d_gf, gf->d_W, nblk * sizeof(float)) || nntk_shim_upload(d_gb, gb->d_W, nblk * sizeof(float))) return -1;   /* contiguous blocks */
    if (bd_train_gradient_run(lf, lb, who, d_gf, d_gb, d_dX, d_dout)) return -1;
    if (nntk_shim_download(gf->d_W, d_gf, nblk * sizeof(float)) || nntk_shim_download(gb->d_W, d_gb, nblk * sizeof(float))) return -1;
    return nntk_shim_download(d_X, d_dX, n_in * sizeof(float));
}

/* ======================= entry-point bodies of all cells ==================== */
/* What remains of a public call once REC_ENTER has checked its handle: read the activations, look for weight edits the way the call's
 * form does (host-pointer forms: compare, core_apply_host*; device-pointer forms: core_ensure(.., 0) -- SyncWeights is their contract),
 * run the shared routine. */
static int layer_apply_inference(rec_layer *l, const char *who, const float *input, float *output) {
    if (l->train.on) return rec_fail(who, "the handle was created for training");           /* gru.c:190-192, lstm.c:242-244, rnn.c:223-225 */
    if (layer_acts(l)) return -1;
    return core_apply_host(l, input, output, 1, 1);
}
static int layer_apply_batch(rec_layer *l, const float *input, float *output, int batch) {
    if (layer_acts(l)) return -1;
    return core_apply_host(l, input, output, batch, 0);
}
static int layer_apply_device(rec_layer *l, const float *d_input, float *d_output, int batch) {
    if (layer_acts(l) || core_ensure(&l->core, 0)) return -1;
    return core_apply_device(l, d_input, d_output, batch, 0);
}
static int layer_apply_device_vl(rec_layer *l, const char *who, const float *d_input, float *d_output, int batch, const int *lengths,
                                 const float *d_h0, const float *d_c0, float *d_hT, float *d_cT) {
    if (layer_acts(l) || core_ensure(&l->core, 0)) return -1;
    return core_apply_device_vl(l, who, d_input, d_output, batch, lengths, d_h0, d_c0, d_hT, d_cT);
}
static int layer_apply_host_vl(rec_layer *l, const char *who, const float *input, float *output, int batch, const int *lengths,
                               const float *h0, const float *c0, float *hT, float *cT) {
    if (layer_acts(l)) return -1;
    return core_apply_host_vl(l, who, input, output, batch, lengths, h0, c0, hT, cT);
}
static int layer_apply_device_f3(rec_layer *l, const float *d_input, const float *d_input_frag3, float *d_output, float *d_output_frag3, int batch) {
    if (layer_acts(l) || core_ensure(&l->core, 0)) return -1;
    return core_apply_device_f3(l, d_input, d_input_frag3, d_output, d_output_frag3, batch);
}
static int layer_apply_bd(rec_layer *lf, rec_layer *lb, const char *who, const float *d_input, float *d_output, int batch, const int *lengths, int merge) {
    if (layer_acts(lf) || layer_acts(lb)) return -1;
    return core_apply_bd(lf, lb, who, d_input, d_output, batch, lengths, merge);
}
static int layer_apply_bd_host(rec_layer *lf, rec_layer *lb, const char *who, const float *input, float *output, int batch, const int *lengths, int merge) {
    if (layer_acts(lf) || layer_acts(lb)) return -1;
    return core_apply_bd_host(lf, lb, who, input, output, batch, lengths, merge);
}

/* ================================= GRU ==================================== */

/* gru.c:13-19 */
GRUConfig GRUConfigCreate(int input_feature_channels, int output_feature_channels, bool return_sequences,
                          int timesteps, GRUActivations activations) {
    GRUConfig c;
    memset(&c, 0, sizeof(c));
    c.base = RecurrentConfigCreate(input_feature_channels, output_feature_channels, return_sequences, timesteps);
    c.activations = activations;
    return c;
}

/* gru.c:206-212 */
GRUActivations GRUActivationsCreateDefault(int size) {
    GRUActivations a;
    a.z_gate_activation = ActivationFunctionCreateSigmoid(size);
    a.r_gate_activation = ActivationFunctionCreateSigmoid(size);
    a.h_gate_activation = ActivationFunctionCreateTanh(size);
    return a;
}
/* gru.c:220-230: argument order is (z, h, r) */
GRUActivations GRUActivationsCreate(ActivationFunction z_gate_activation, ActivationFunction h_gate_activation,
                                    ActivationFunction r_gate_activation) {
    GRUActivations a;
    a.z_gate_activation = z_gate_activation;
    a.h_gate_activation = h_gate_activation;
    a.r_gate_activation = r_gate_activation;
    return a;
}
void GRUActivationsDestroy(GRUActivations activations) {
    ActivationFunctionDestroy(activations.z_gate_activation);
    ActivationFunctionDestroy(activations.r_gate_activation);
    ActivationFunctionDestroy(activations.h_gate_activation);
}

GRU GRUCreateForInference(GRUConfig config) {
    const ActivationFunction act[3] = { config.activations.z_gate_activation, config.activations.h_gate_activation, config.activations.r_gate_activation };
    return (GRU)layer_create(3, config.base, 1, act, 3);
}
/* gru.c:232-244 */
GRU GRUCreateForTraining(GRUConfig config, GRUTrainingConfig training_config) {
    GRU f = GRUCreateForInference(config);
    if (f) layer_train_on(&f->l, training_config);
    return f;
}
GRUGradient *GRUGradientCreate(GRUConfig config, GRUTrainingConfig training_config) { return gradient_create(3, config.base, training_config); }
GRUWeights *GRUGetWeights(GRU filter) { return filter->l.core.weights; }
void GRUDestroy(GRU filter) { layer_destroy((rec_layer *)filter); }

int GRUBroadcastWeights(GRU filter, int root) {
    REC_ENTER("GRUBroadcastWeights", filter);
    return core_broadcast(&filter->l.core, root);
}
int GRULoadWeightsDevice(GRU filter, const float *d_block) {
    REC_ENTER("GRULoadWeightsDevice", filter);
    return core_load_device(&filter->l.core, "GRULoadWeightsDevice", d_block);
}
int GRUSyncWeights(GRU filter) {
    REC_ENTER("GRUSyncWeights", filter);
    return core_sync(&filter->l.core);
}
int GRUResetState(GRU filter) {
    REC_ENTER("GRUResetState", filter);
    return core_reset_state(&filter->l.core);
}
int GRUGetState(GRU filter, float *h_host) {
    REC_ENTER("GRUGetState", filter);
    return nntk_shim_download(h_host, filter->l.core.d_h[filter->l.core.cur], (size_t)filter->l.core.H * sizeof(float));
}
const char *GRUKernelPlan(GRU filter) {
    static _Thread_local char buf[320];
    return filter ? core_plan(&filter->l, buf, sizeof buf) : "";
}

int GRUApplyInference(GRU filter, const float *input, float *output) {
    REC_ENTER("GRUApplyInference", filter);
    return layer_apply_inference(&filter->l, "GRUApplyInference", input, output);
}
/* gru.c:246-293 forward semantics */
int GRUApplyInferenceBatch(GRU filter, const float *input, float *output, int batch) {
    REC_ENTER("GRUApplyInferenceBatch", filter);
    return layer_apply_batch(&filter->l, input, output, batch);
}
int GRUApplyDevice(GRU filter, const float *d_input, float *d_output, int batch) {
    REC_ENTER("GRUApplyDevice", filter);
    return layer_apply_device(&filter->l, d_input, d_output, batch);
}
int GRUApplyDeviceVarLen(GRU filter, const float *d_input, float *d_output, int batch, const int *lengths,
                         const float *d_h0, float *d_hT) {
    REC_ENTER("GRUApplyDeviceVarLen", filter);
    return layer_apply_device_vl(&filter->l, "GRUApplyDeviceVarLen", d_input, d_output, batch, lengths, d_h0, NULL, d_hT, NULL);
}
int GRUApplyInferenceBatchVarLen(GRU filter, const float *input, float *output, int batch, const int *lengths,
                                 const float *h0, float *hT) {
    REC_ENTER("GRUApplyInferenceBatchVarLen", filter);
    return layer_apply_host_vl(&filter->l, "GRUApplyInferenceBatchVarLen", input, output, batch, lengths, h0, NULL, hT, NULL);
}
int GRUApplyDeviceFrag3(GRU filter, const float *d_input, const float *d_input_frag3, float *d_output, float *d_output_frag3, int batch) {
    REC_ENTER("GRUApplyDeviceFrag3", filter);
    return layer_apply_device_f3(&filter->l, d_input, d_input_frag3, d_output, d_output_frag3, batch);
}
int GRUBidirectionalApplyDevice(GRU forward, GRU backward, const float *d_input, float *d_output, int batch, const int *lengths, int merge) {
    REC_ENTER("GRUBidirectionalApplyDevice", forward && backward);
    return layer_apply_bd(&forward->l, &backward->l, "GRUBidirectionalApplyDevice", d_input, d_output, batch, lengths, merge);
}
int GRUBidirectionalApplyInferenceBatch(GRU forward, GRU backward, const float *input, float *output, int batch, const int *lengths, int merge) {
    REC_ENTER("GRUBidirectionalApplyInferenceBatch", forward && backward);
    return layer_apply_bd_host(&forward->l, &backward->l, "GRUBidirectionalApplyInferenceBatch", input, output, batch, lengths, merge);
}

int GRUApplyTrainingBatch(GRU filter, const float *input, float *output) {
    REC_ENTER("GRUApplyTrainingBatch", filter);
    return train_apply_host(&filter->l, "GRUApplyTrainingBatch", input, output);
}
int GRUApplyTrainingBatchDevice(GRU filter, const float *d_input, float *d_output) {
    REC_ENTER("GRUApplyTrainingBatchDevice", filter);
    return train_apply_dev(&filter->l, "GRUApplyTrainingBatchDevice", d_input, d_output);
}
void GRUCalculateGradient(GRU filter, GRUGradient *gradient, float *d_out) {
    REC_ENTER_GRADIENT("GRUCalculateGradient", filter && gradient && d_out);
    train_gradient_host(&filter->l, "GRUCalculateGradient", "GRU", gradient, d_out);
}
int GRUCalculateGradientDevice(GRU filter, float *d_grad, float *d_dX, const float *d_dout) {
    nntk_shim_clear_error();
    if (!filter) NNTK_FAIL("GRUCalculateGradientDevice: NULL argument");
    return train_gradient_dev(&filter->l, "GRUCalculateGradientDevice", "GRU", d_grad, d_dX, d_dout);
}
int GRUApplyTrainingBatchDeviceVarLen(GRU filter, const float *d_input, float *d_output, const int *lengths, const float *d_h0, float *d_hT) {
    REC_ENTER("GRUApplyTrainingBatchDeviceVarLen", filter);
    return train_apply_vl_dev(&filter->l, "GRUApplyTrainingBatchDeviceVarLen", d_input, d_output, lengths, d_h0, NULL, d_hT, NULL);
}
int GRUCalculateGradientDeviceVarLen(GRU filter, float *d_grad, float *d_dX, const float *d_dout, const float *d_dhT, float *d_dh0) {
    REC_ENTER("GRUCalculateGradientDeviceVarLen", filter);
    return train_gradient_vl_dev(&filter->l, "GRUCalculateGradientDeviceVarLen", d_grad, d_dX, d_dout, d_dhT, NULL, d_dh0, NULL);
}
int GRUApplyTrainingBatchVarLen(GRU filter, const float *input, float *output, const int *lengths, const float *h0, float *hT) {
    REC_ENTER("GRUApplyTrainingBatchVarLen", filter);
    return train_apply_vl_host(&filter->l, "GRUApplyTrainingBatchVarLen", input, output, lengths, h0, NULL, hT, NULL);
}
int GRUCalculateGradientVarLen(GRU filter, GRUGradient *gradient, const float *d_out, const float *d_hT_grad, float *d_h0_grad) {
    REC_ENTER("GRUCalculateGradientVarLen", filter);
    return train_gradient_vl_host(&filter->l, "GRUCalculateGradientVarLen", gradient, d_out, d_hT_grad, NULL, d_h0_grad, NULL);
}
/* the bidirectional training calls (bd_train_*): forward / backward are two different GRUCreateForTraining handles of one shape */
int GRUBidirectionalApplyTrainingBatchDevice(GRU forward, GRU backward, const float *d_input, float *d_output, const int *lengths, int merge) {
    REC_ENTER("GRUBidirectionalApplyTrainingBatchDevice", forward && backward);
    return bd_train_forward_dev(&forward->l, &backward->l, "GRUBidirectionalApplyTrainingBatchDevice", d_input, d_output, lengths, merge);
}
int GRUBidirectionalCalculateGradientDevice(GRU forward, GRU backward, float *d_grad_forward, float *d_grad_backward, float *d_dX, const float *d_dout) {
    REC_ENTER("GRUBidirectionalCalculateGradientDevice", forward && backward);
    return bd_train_gradient_dev(&forward->l, &backward->l, "GRUBidirectionalCalculateGradientDevice", d_grad_forward, d_grad_backward, d_dX, d_dout);
}
int GRUBidirectionalApplyTrainingBatch(GRU forward, GRU backward, const float *input, float *output, const int *lengths, int merge) {
    REC_ENTER("GRUBidirectionalApplyTrainingBatch", forward && backward);
    return bd_train_forward_host(&forward->l, &backward->l, "GRUBidirectionalApplyTrainingBatch", input, output, lengths, merge);
}
int GRUBidirectionalCalculateGradient(GRU forward, GRU backward, GRUGradient *grad_forward, GRUGradient *grad_backward, float *d_X, const float *d_out) {
    REC_ENTER("GRUBidirectionalCalculateGradient", forward && backward);
    return bd_train_gradient_host(&forward->l, &backward->l, "GRUBidirectionalCalculateGradient", grad_forward, grad_backward, d_X, d_out);
}

/* ---- two stacked GRU layers in one persistent launch (BASELINE configs[3]; recurrent.hip gru2_persistent_kernel) ----
 * Same results as GRUApplyDevice(l1) followed by GRUApplyDevice(l2) on zero initial state (layer 1 bit for bit, layer 2
 * within the layer tolerance: its input projection is summed in another order); falls back to exactly those two calls
 * for shapes / activations the fused kernel does not take. */
int GRUStack2ApplyDevice(GRU l1, GRU l2, const float *d_input, float *d_output, int batch) {
    REC_ENTER("GRUStack2ApplyDevice", l1 && l2);
    rec_core *c1 = &l1->l.core, *c2 = &l2->l.core;
    if (!c1->return_sequences || c2->in != c1->H || c2->T != c1->T)
        NNTK_FAIL("GRUStack2ApplyDevice: layer 1 must return sequences and feed layer 2 (in2 = H1, same timesteps)");
    if (batch <= 0) return 0;
    if (core_ensure(c1, 0) || core_ensure(c2, 0)) return -1;
    const int H = c1->H, T = c1->T, B = batch;
    if (layer_acts(&l1->l) || layer_acts(&l2->l)) return -1;
    const int std_pair = layer_std_acts(&l1->l) && layer_std_acts(&l2->l);
    /* both layers on the register-resident split-bf16 kernels (gru_rr_kernel, one launch per layer, projections fused) when they take
     * them: measured faster than the fused exact-f32 kernel below (DESIGN K4b); rec_fused2 = 1 forces the fused kernel */
    int fused_on = -1;
    (void)nntk_shim_get_option("rec_fused2", &fused_on);
    const int rr_pair = layer_takes_rr(&l1->l) && layer_takes_rr(&l2->l);
    if (std_pair && c2->H == H && !(rr_pair && fused_on != 1)) {
        if (core_ensure_wt(c2)) return -1;
        float *d_xw = nntk_devbuf_reserve(&c1->d_xw, (size_t)T * B * 3 * H);
        float *d_work = nntk_devbuf_reserve(&c1->d_work, nntk_shim_gru2_work_floats(B, H) > nntk_shim_recurrent_work_floats(B, H)
                                                           ? nntk_shim_gru2_work_floats(B, H) : nntk_shim_recurrent_work_floats(B, H));
        if (!d_xw || !d_work) return -1;
        if (nntk_shim_conv1d(d_input, c1->d_wp, c1->d_bi, NULL, 0.f, NNTK_ACT_IDENTITY, 1.f, d_xw, B, T, c1->in, 3 * H, 1, 1, T, 1))
            return -1;
        int rc = nntk_shim_gru2(d_xw, c1->d_ut, c1->d_bh, c2->d_wt, c2->d_bi, c2->d_ut, c2->d_bh, d_output, NULL, d_work,
                                B, T, H, c2->return_sequences);
        if (rc <= 0) return rc;
    }
    /* the register-resident pair: layer 1 publishes h1_t ALREADY SPLIT, in layer 2's operand order, into a T-deep buffer -- its own
     * hand-off, so not one store more than a single layer issues -- and layer 2 reads that buffer as its x operand: 12 coalesced 1 KB
     * requests per half-step, no f32 inter-layer tensor, no split in the consumer (DESIGN K4b).  The values are the f32 h1_t exactly
     * (hi + mid + lo), so the result equals GRUApplyDevice(l1) then GRUApplyDevice(l2) bit for bit. */
    if (rr_pair) {
        float *d_h1 = nntk_devbuf_reserve(&c1->d_hseq, nntk_shim_rr_hseq_floats(B, T, H));
        if (!d_h1) return -1;
        const rr_io io1 = { .d_in = d_input, .d_out_f3 = d_h1 };
        int rc = core_try_rr(&l1->l, &io1, B, 0);
        if (rc < 0) return -1;
        if (rc == 0) {
            const rr_io io2 = { .d_in_f3 = d_h1, .d_out = d_output };
            rc = core_try_rr(&l2->l, &io2, B, 0);
            if (rc <= 0) return rc;
            /* layer 2 not taken after all (cannot happen for a pair that qualified): both layers again, through an f32 tensor */
        }
    }
    float *d_mid = nntk_devbuf_reserve(&c1->d_out, (size_t)B * T * H);         /* (layer 1's scratch holds the middle tensor) */
    if (!d_mid) return -1;
    if (GRUApplyDevice(l1, d_input, d_mid, batch)) return -1;
    return GRUApplyDevice(l2, d_mid, d_output, batch);
}
static int run_stack2(const dev_call *k, const float *d_in, float *d_out) { return GRUStack2ApplyDevice((GRU)k->l, (GRU)k->l2, d_in, d_out, k->B); }
int GRUStack2ApplyInferenceBatch(GRU l1, GRU l2, const float *input, float *output, int batch) {
    REC_ENTER("GRUStack2ApplyInferenceBatch", l1 && l2);
    if (batch <= 0) return 0;
    rec_core *c1 = &l1->l.core, *c2 = &l2->l.core;
    if (core_ensure(c1, 1) || core_ensure(c2, 1)) return -1;
    size_t n_in = (size_t)batch * c1->T * c1->in;
    size_t n_out = c2->return_sequences ? (size_t)batch * c2->T * c2->H : (size_t)batch * c2->H;
    float *d_in = nntk_devbuf_reserve(&c1->d_in, n_in);
    float *d_out = nntk_devbuf_reserve(&c2->d_out, n_out);
    if (!d_in || !d_out) return -1;
    const dev_call k = { .run = run_stack2, .l = &l1->l, .l2 = &l2->l, .B = batch };
    const host_input in = { input, d_in, n_in };
    return host_round_trip(&k, &in, 1, d_out, output, n_out, 0);
}

/* ================================= LSTM =================================== */

/* lstm.c:17-26: argument order (input, forget, candidate, output_gate, output) */
LSTMActivations LSTMActivationsCreate(ActivationFunction input_gate_activation,
                                      ActivationFunction forget_gate_activation,
                                      ActivationFunction candidate_gate_activation,
                                      ActivationFunction output_gate_activation,
                                      ActivationFunction output_activation) {
    LSTMActivations a;
    a.candidate_gate_activation = candidate_gate_activation;
    a.input_gate_activation = input_gate_activation;
    a.forget_gate_activation = forget_gate_activation;
    a.output_gate_activation = output_gate_activation;
    a.output_activation = output_activation;
    return a;
}
/* lstm.c:110-118 */
LSTMActivations LSTMActivationsCreateDefault(int size) {
    return LSTMActivationsCreate(ActivationFunctionCreateSigmoid(size), ActivationFunctionCreateSigmoid(size),
                                 ActivationFunctionCreateTanh(size), ActivationFunctionCreateSigmoid(size),
                                 ActivationFunctionCreateTanh(size));
}
void LSTMActivationsDestroy(LSTMActivations activations) {
    ActivationFunctionDestroy(activations.input_gate_activation);
    ActivationFunctionDestroy(activations.forget_gate_activation);
    ActivationFunctionDestroy(activations.candidate_gate_activation);
    ActivationFunctionDestroy(activations.output_gate_activation);
    ActivationFunctionDestroy(activations.output_activation);
}
/* lstm.c:132-138 */
LSTMConfig LSTMConfigCreate(int input_feature_channels, int output_feature_channels, bool return_sequences,
                            int timesteps, bool v2, LSTMActivations activations) {
    LSTMConfig c;
    memset(&c, 0, sizeof(c));
    c.base = RecurrentConfigCreate(input_feature_channels, output_feature_channels, return_sequences, timesteps);
    c.v2 = v2;
    c.activations = activations;
    return c;
}

LSTM LSTMCreateForInference(LSTMConfig config) {
    const LSTMActivations *a = &config.activations;
    const ActivationFunction act[5] = { a->input_gate_activation, a->forget_gate_activation, a->candidate_gate_activation,
                                        a->output_gate_activation, a->output_activation };
    return (LSTM)layer_create(4, config.base, config.v2, act, 5);
}
LSTM LSTMCreateForTraining(LSTMConfig config, LSTMTrainingConfig training_config) {
    LSTM f = LSTMCreateForInference(config);
    if (f) layer_train_on(&f->l, training_config);
    return f;
}
LSTMGradient *LSTMGradientCreate(LSTMConfig config, LSTMTrainingConfig training_config) { return gradient_create(4, config.base, training_config); }
LSTMWeights *LSTMGetWeights(LSTM filter) { return filter->l.core.weights; }
void LSTMDestroy(LSTM filter) { layer_destroy((rec_layer *)filter); }

int LSTMBroadcastWeights(LSTM filter, int root) {
    REC_ENTER("LSTMBroadcastWeights", filter);
    return core_broadcast(&filter->l.core, root);
}
int LSTMLoadWeightsDevice(LSTM filter, const float *d_block) {
    REC_ENTER("LSTMLoadWeightsDevice", filter);
    return core_load_device(&filter->l.core, "LSTMLoadWeightsDevice", d_block);
}
int LSTMSyncWeights(LSTM filter) {
    REC_ENTER("LSTMSyncWeights", filter);
    return core_sync(&filter->l.core);
}
/* lstm.c:270-274 (lstm_zero_state) */
int LSTMResetState(LSTM filter) {
    REC_ENTER("LSTMResetState", filter);
    return core_reset_state(&filter->l.core);
}
int LSTMGetState(LSTM filter, float *h_host, float *c_host) {
    REC_ENTER("LSTMGetState", filter);
    const rec_core *c = &filter->l.core;
    if (h_host && nntk_shim_download(h_host, c->d_h[c->cur], (size_t)c->H * sizeof(float))) return -1;
    if (c_host && nntk_shim_download(c_host, c->d_c[c->cur], (size_t)c->H * sizeof(float))) return -1;
    return 0;
}
const char *LSTMKernelPlan(LSTM filter) {
    static _Thread_local char buf[320];
    return filter ? core_plan(&filter->l, buf, sizeof buf) : "";
}

int LSTMApplyInference(LSTM filter, const float *input, float *output) {
    REC_ENTER("LSTMApplyInference", filter);
    return layer_apply_inference(&filter->l, "LSTMApplyInference", input, output);
}
/* lstm.c:426-475 forward semantics */
int LSTMApplyInferenceBatch(LSTM filter, const float *input, float *output, int batch) {
    REC_ENTER("LSTMApplyInferenceBatch", filter);
    return layer_apply_batch(&filter->l, input, output, batch);
}
int LSTMApplyDevice(LSTM filter, const float *d_input, float *d_output, int batch) {
    REC_ENTER("LSTMApplyDevice", filter);
    return layer_apply_device(&filter->l, d_input, d_output, batch);
}
int LSTMApplyDeviceVarLen(LSTM filter, const float *d_input, float *d_output, int batch, const int *lengths,
                          const float *d_h0, const float *d_c0, float *d_hT, float *d_cT) {
    REC_ENTER("LSTMApplyDeviceVarLen", filter);
    return layer_apply_device_vl(&filter->l, "LSTMApplyDeviceVarLen", d_input, d_output, batch, lengths, d_h0, d_c0, d_hT, d_cT);
}
int LSTMApplyInferenceBatchVarLen(LSTM filter, const float *input, float *output, int batch, const int *lengths,
                                  const float *h0, const float *c0, float *hT, float *cT) {
    REC_ENTER("LSTMApplyInferenceBatchVarLen", filter);
    return layer_apply_host_vl(&filter->l, "LSTMApplyInferenceBatchVarLen", input, output, batch, lengths, h0, c0, hT, cT);
}
int LSTMApplyDeviceFrag3(LSTM filter, const float *d_input, const float *d_input_frag3, float *d_output, float *d_output_frag3, int batch) {
    REC_ENTER("LSTMApplyDeviceFrag3", filter);
    return layer_apply_device_f3(&filter->l, d_input, d_input_frag3, d_output, d_output_frag3, batch);
}
int LSTMBidirectionalApplyDevice(LSTM forward, LSTM backward, const float *d_input, float *d_output, int batch, const int *lengths, int merge) {
    REC_ENTER("LSTMBidirectionalApplyDevice", forward && backward);
    return layer_apply_bd(&forward->l, &backward->l, "LSTMBidirectionalApplyDevice", d_input, d_output, batch, lengths, merge);
}
int LSTMBidirectionalApplyInferenceBatch(LSTM forward, LSTM backward, const float *input, float *output, int batch, const int *lengths, int merge) {
    REC_ENTER("LSTMBidirectionalApplyInferenceBatch", forward && backward);
    return layer_apply_bd_host(&forward->l, &backward->l, "LSTMBidirectionalApplyInferenceBatch", input, output, batch, lengths, merge);
}

/* The HF instantiation of the register-resident kernel (H > 256): its recurrence itself runs on two f16 images of h (three products per
 * k step), and its hand-off buffer IS the FRAG2H output.  Another contraction than the bf16 x 3 kernels' (same tolerance): the choice
 * depends on the layer only (shape, weights, option rec_hf), never on the call.  0 = ran; 1 = not taken; -1 = error */
static int lstm_try_rr_hf(rec_layer *l, const float *d_in, const float *d_in_f3, float *d_out_h2, int B) {
    rec_core *c = &l->core;
    if (rr_why_not(l, c->rr_exact_only, nntk_shim_lstm_rr_hf_ok(c->H, c->in))) return 1;
    if (!c->rr_hf_valid) {
        const size_t nW = (size_t)c->in * 4 * c->H, nU = (size_t)c->H * 4 * c->H;
        float us = nntk_f16_scale(c->weights->U, nU), mw = 0.f;
        for (size_t i = 0; i < nW; ++i) { float a = fabsf(c->weights->W[i]); if (a > mw) mw = a; }
        /* W's bf16 images are packed times 2^15 us: they must stay inside bf16's range (and the sums inside f32's) */
        c->hf_wscale = (us > 0.f && us < 1e15f && us > 1e-15f && mw * 32768.f * us < 1e30f) ? 32768.f * us : 0.f;
        if (c->hf_wscale > 0.f) {
            size_t img = nntk_shim_lstm_rr_hf_image_floats(c->H, c->in);
            if (!c->d_rr_hf && !(c->d_rr_hf = (float *)nntk_shim_malloc(img * sizeof(float)))) return -1;
            if (nntk_shim_lstm_rr_pack_hf(c->d_ut, c->d_wp, c->d_rr_hf, c->H, c->in, us, c->hf_wscale)) return -1;
        }
        c->rr_hf_valid = 1;
    }
    if (!(c->hf_wscale > 0.f)) return 1;
    const float *xf3 = d_in_f3;
    if (!xf3) {
        float *buf = nntk_devbuf_reserve(&c->d_xf3, nntk_shim_frag3_floats(B, c->T, c->in));
        if (!buf || nntk_shim_frag3_pack(d_in, buf, B, c->T, c->in)) return -1;
        xf3 = buf;
    }
    float *d_work = nntk_devbuf_reserve(&c->d_work_rr, nntk_shim_lstm_rr_work_floats(B, c->H));
    if (!d_work) return -1;
    return nntk_shim_lstm_rr_hf(xf3, c->d_rr_hf, c->d_bi, l->use_bh ? c->d_bh : NULL, d_out_h2, d_work, B, c->T, c->in, c->H, 1.f / c->hf_wscale);
}
/* The sequence output as a FRAG2H tensor (frag3.hip: two f16 images of h * 2^15 -- the dense GEMM's three-product operand form).  The form
 * holds magnitudes below 2, so it exists for the standard activations only (|h| = |o tanh(c)| < 1).  The split-K register-resident kernels
 * write it themselves (the wave that would write the f32 rows); every other kernel goes through an f32 scratch tensor and the pack pass:
 * the same bits, because the form is a function of the f32 value.  0 = done; 1 = not available for this layer; -1 = error. */
static int lstm_apply_device_h2(LSTM filter, const float *d_in, const float *d_in_f3, float *d_out_h2, int B) {
    rec_layer *l = &filter->l;
    rec_core *c = &l->core;
    if (layer_acts(l)) return -1;
    if (!layer_std_acts(l) || !c->return_sequences) return 1;
    if (B <= 0 || c->T <= 0) return 0;
    if (core_ensure(c, 0)) return -1;
    int rc = lstm_try_rr_hf(l, d_in, d_in_f3, d_out_h2, B);
    if (rc <= 0) return rc;
    if (!nntk_shim_fk_image_floats(c->H, c->in)) {       /* (the full-K family has no FRAG2H store; its shapes take the f32 way below) */
        const rr_io io = { .d_in = d_in, .d_in_f3 = d_in_f3, .d_out_h2 = d_out_h2 };
        rc = core_try_rr(l, &io, B, 0);
        if (rc <= 0) return rc;
    }
    float *o = nntk_devbuf_reserve(&c->d_out, (size_t)B * c->T * c->H);
    if (!o) return -1;
    if (core_apply_device_f3(l, d_in, d_in_f3, o, NULL, B)) return -1;
    return nntk_shim_frag2h_pack(o, d_out_h2, B, c->T, c->H);
}
int LSTMApplyDeviceFrag2h(LSTM filter, const float *d_input, const float *d_input_frag3, float *d_output_frag2h, int batch) {
    nntk_shim_clear_error();
    if (!filter || (!d_input && !d_input_frag3) || !d_output_frag2h) NNTK_FAIL("LSTMApplyDeviceFrag2h: NULL argument");
    int rc = lstm_apply_device_h2(filter, d_input, d_input_frag3, d_output_frag2h, batch);
    if (rc == 1) NNTK_FAIL("LSTMApplyDeviceFrag2h: the frag2h form holds |h| < 2 -- standard activations and return_sequences only");
    return rc;
}
/* for the fused LSTM -> TimeDistributedDense call (dense.c) */
int nntk_lstm_apply_device_h2(LSTM filter, const float *d_in, const float *d_in_f3, float *d_out_h2, int B) {
    return lstm_apply_device_h2(filter, d_in, d_in_f3, d_out_h2, B);
}
float *nntk_lstm_frag2h_scratch(LSTM f, int batch) {
    return nntk_devbuf_reserve(&f->l.core.d_h2, nntk_shim_frag2h_floats(batch, f->l.core.T, f->l.core.H));
}
void nntk_lstm_dims(LSTM f, int *T, int *in, int *H, int *return_sequences) {
    const rec_core *c = &f->l.core;
    *T = c->T; *in = c->in; *H = c->H; *return_sequences = c->return_sequences ? 1 : 0;
}
float *nntk_lstm_frag3_scratch(LSTM f, int batch) {
    /* the register-resident kernels' hand-off size counts H / 16 k steps (they take H % 16 == 0 only); a layer they do not take writes a
     * frag3 tensor of ceil(H / 16) k steps into this buffer through the pack pass: the larger of the two (found by the FRAG2H soak: for
     * H % 16 != 0 the fused LSTM -> dense call wrote one k step per row block past the end of the smaller one) */
    rec_core *c = &f->l.core;
    size_t a = nntk_shim_rr_hseq_floats(batch, c->T, c->H), b = nntk_shim_frag3_floats(batch, c->T, c->H);
    return nntk_devbuf_reserve(&c->d_hseq, a > b ? a : b);
}

int LSTMApplyTrainingBatch(LSTM filter, const float *input, float *output) {
    REC_ENTER("LSTMApplyTrainingBatch", filter);
    return train_apply_host(&filter->l, "LSTMApplyTrainingBatch", input, output);
}
int LSTMApplyTrainingBatchDevice(LSTM filter, const float *d_input, float *d_output) {
    REC_ENTER("LSTMApplyTrainingBatchDevice", filter);
    return train_apply_dev(&filter->l, "LSTMApplyTrainingBatchDevice", d_input, d_output);
}
void LSTMCalculateGradient(LSTM filter, LSTMGradient *gradient, float *d_out) {
    REC_ENTER_GRADIENT("LSTMCalculateGradient", filter && gradient && d_out);
    train_gradient_host(&filter->l, "LSTMCalculateGradient", "LSTM", gradient, d_out);
}
int LSTMCalculateGradientDevice(LSTM filter, float *d_grad, float *d_dX, const float *d_dout) {
    nntk_shim_clear_error();
    if (!filter) NNTK_FAIL("LSTMCalculateGradientDevice: NULL argument");
    return train_gradient_dev(&filter->l, "LSTMCalculateGradientDevice", "LSTM", d_grad, d_dX, d_dout);
}
int LSTMApplyTrainingBatchDeviceVarLen(LSTM filter, const float *d_input, float *d_output, const int *lengths,
                                       const float *d_h0, const float *d_c0, float *d_hT, float *d_cT) {
    REC_ENTER("LSTMApplyTrainingBatchDeviceVarLen", filter);
    return train_apply_vl_dev(&filter->l, "LSTMApplyTrainingBatchDeviceVarLen", d_input, d_output, lengths, d_h0, d_c0, d_hT, d_cT);
}
int LSTMCalculateGradientDeviceVarLen(LSTM filter, float *d_grad, float *d_dX, const float *d_dout,
                                      const float *d_dhT, const float *d_dcT, float *d_dh0, float *d_dc0) {
    REC_ENTER("LSTMCalculateGradientDeviceVarLen", filter);
    return train_gradient_vl_dev(&filter->l, "LSTMCalculateGradientDeviceVarLen", d_grad, d_dX, d_dout, d_dhT, d_dcT, d_dh0, d_dc0);
}
int LSTMApplyTrainingBatchVarLen(LSTM filter, const float *input, float *output, const int *lengths,
                                 const float *h0, const float *c0, float *hT, float *cT) {
    REC_ENTER("LSTMApplyTrainingBatchVarLen", filter);
    return train_apply_vl_host(&filter->l, "LSTMApplyTrainingBatchVarLen", input, output, lengths, h0, c0, hT, cT);
}
int LSTMCalculateGradientVarLen(LSTM filter, LSTMGradient *gradient, const float *d_out, const float *d_hT_grad, const float *d_cT_grad,
                                float *d_h0_grad, float *d_c0_grad) {
    REC_ENTER("LSTMCalculateGradientVarLen", filter);
    return train_gradient_vl_host(&filter->l, "LSTMCalculateGradientVarLen", gradient, d_out, d_hT_grad, d_cT_grad, d_h0_grad, d_c0_grad);
}
/* the bidirectional training calls (bd_train_*): forward / backward are two different LSTMCreateForTraining handles of one shape */
int LSTMBidirectionalApplyTrainingBatchDevice(LSTM forward, LSTM backward, const float *d_input, float *d_output, const int *lengths, int merge) {
    REC_ENTER("LSTMBidirectionalApplyTrainingBatchDevice", forward && backward);
    return bd_train_forward_dev(&forward->l, &backward->l, "LSTMBidirectionalApplyTrainingBatchDevice", d_input, d_output, lengths, merge);
}
int LSTMBidirectionalCalculateGradientDevice(LSTM forward, LSTM backward, float *d_grad_forward, float *d_grad_backward, float *d_dX, const float *d_dout) {
    REC_ENTER("LSTMBidirectionalCalculateGradientDevice", forward && backward);
    return bd_train_gradient_dev(&forward->l, &backward->l, "LSTMBidirectionalCalculateGradientDevice", d_grad_forward, d_grad_backward, d_dX, d_dout);
}
int LSTMBidirectionalApplyTrainingBatch(LSTM forward, LSTM backward, const float *input, float *output, const int *lengths, int merge) {
    REC_ENTER("LSTMBidirectionalApplyTrainingBatch", forward && backward);
    return bd_train_forward_host(&forward->l, &backward->l, "LSTMBidirectionalApplyTrainingBatch", input, output, lengths, merge);
}
int LSTMBidirectionalCalculateGradient(LSTM forward, LSTM backward, LSTMGradient *grad_forward, LSTMGradient *grad_backward, float *d_X, const float *d_out) {
    REC_ENTER("LSTMBidirectionalCalculateGradient", forward && backward);
    return bd_train_gradient_host(&forward->l, &backward->l, "LSTMBidirectionalCalculateGradient", grad_forward, grad_backward, d_X, d_out);
}

/* ================================= RNN ==================================== */
/* layers/rnn.c.  One gate; the activation is the layer's single ActivationFunction (rnn.h:20-24), which must be
 * one of the built-ins to run inside the step kernel. */

/* rnn.c:48-61 */
RNNConfig RNNConfigCreate(int input_feature_channels, int output_feature_channels, bool return_sequences,
                          int timesteps, bool v2, ActivationFunction activation) {
    RNNConfig c;
    memset(&c, 0, sizeof(c));
    c.base = RecurrentConfigCreate(input_feature_channels, output_feature_channels, return_sequences, timesteps);
    c.v2 = v2;
    c.activation = activation;
    return c;
}

RNN RNNCreateForInference(RNNConfig config) { return (RNN)layer_create(1, config.base, config.v2, &config.activation, 1); }
RNN RNNCreateForTraining(RNNConfig config, RNNTrainingConfig training_config) {
    RNN f = RNNCreateForInference(config);
    if (f) layer_train_on(&f->l, training_config);
    return f;
}
RNNGradient *RNNGradientCreate(RNNConfig config, RNNTrainingConfig training_config) { return gradient_create(1, config.base, training_config); }
RNNWeights *RNNGetWeights(RNN filter) { return filter->l.core.weights; }
void RNNDestroy(RNN filter) { layer_destroy((rec_layer *)filter); }

int RNNBroadcastWeights(RNN filter, int root) {
    REC_ENTER("RNNBroadcastWeights", filter);
    return core_broadcast(&filter->l.core, root);
}
int RNNLoadWeightsDevice(RNN filter, const float *d_block) {
    REC_ENTER("RNNLoadWeightsDevice", filter);
    return core_load_device(&filter->l.core, "RNNLoadWeightsDevice", d_block);
}
int RNNSyncWeights(RNN filter) {
    REC_ENTER("RNNSyncWeights", filter);
    return core_sync(&filter->l.core);
}
int RNNResetState(RNN filter) {
    REC_ENTER("RNNResetState", filter);
    return core_reset_state(&filter->l.core);
}
int RNNGetState(RNN filter, float *h_host) {
    REC_ENTER("RNNGetState", filter);
    return nntk_shim_download(h_host, filter->l.core.d_h[filter->l.core.cur], (size_t)filter->l.core.H * sizeof(float));
}

int RNNApplyInference(RNN filter, const float *input, float *output) {
    REC_ENTER("RNNApplyInference", filter);
    return layer_apply_inference(&filter->l, "RNNApplyInference", input, output);
}
/* rnn.c:249-291 forward semantics */
int RNNApplyInferenceBatch(RNN filter, const float *input, float *output, int batch) {
    REC_ENTER("RNNApplyInferenceBatch", filter);
    return layer_apply_batch(&filter->l, input, output, batch);
}
int RNNApplyDevice(RNN filter, const float *d_input, float *d_output, int batch) {
    REC_ENTER("RNNApplyDevice", filter);
    return layer_apply_device(&filter->l, d_input, d_output, batch);
}
int RNNApplyDeviceVarLen(RNN filter, const float *d_input, float *d_output, int batch, const int *lengths,
                         const float *d_h0, float *d_hT) {
    REC_ENTER("RNNApplyDeviceVarLen", filter);
    return layer_apply_device_vl(&filter->l, "RNNApplyDeviceVarLen", d_input, d_output, batch, lengths, d_h0, NULL, d_hT, NULL);
}
int RNNApplyInferenceBatchVarLen(RNN filter, const float *input, float *output, int batch, const int *lengths,
                                 const float *h0, float *hT) {
    REC_ENTER("RNNApplyInferenceBatchVarLen", filter);
    return layer_apply_host_vl(&filter->l, "RNNApplyInferenceBatchVarLen", input, output, batch, lengths, h0, NULL, hT, NULL);
}
int RNNBidirectionalApplyDevice(RNN forward, RNN backward, const float *d_input, float *d_output, int batch, const int *lengths, int merge) {
    REC_ENTER("RNNBidirectionalApplyDevice", forward && backward);
    return layer_apply_bd(&forward->l, &backward->l, "RNNBidirectionalApplyDevice", d_input, d_output, batch, lengths, merge);
}
int RNNBidirectionalApplyInferenceBatch(RNN forward, RNN backward, const float *input, float *output, int batch, const int *lengths, int merge) {
    REC_ENTER("RNNBidirectionalApplyInferenceBatch", forward && backward);
    return layer_apply_bd_host(&forward->l, &backward->l, "RNNBidirectionalApplyInferenceBatch", input, output, batch, lengths, merge);
}

int RNNApplyTrainingBatch(RNN filter, const float *input, float *output) {
    REC_ENTER("RNNApplyTrainingBatch", filter);
    return train_apply_host(&filter->l, "RNNApplyTrainingBatch", input, output);
}
int RNNApplyTrainingBatchDevice(RNN filter, const float *d_input, float *d_output) {
    REC_ENTER("RNNApplyTrainingBatchDevice", filter);
    return train_apply_dev(&filter->l, "RNNApplyTrainingBatchDevice", d_input, d_output);
}
void RNNCalculateGradient(RNN filter, RNNGradient *gradient, float *d_out) {
    REC_ENTER_GRADIENT("RNNCalculateGradient", filter && gradient && d_out);
    train_gradient_host(&filter->l, "RNNCalculateGradient", "RNN", gradient, d_out);
}
int RNNCalculateGradientDevice(RNN filter, float *d_grad, float *d_dX, const float *d_dout) {
    nntk_shim_clear_error();
    if (!filter) NNTK_FAIL("RNNCalculateGradientDevice: NULL argument");
    return train_gradient_dev(&filter->l, "RNNCalculateGradientDevice", "RNN", d_grad, d_dX, d_dout);
}
int RNNApplyTrainingBatchDeviceVarLen(RNN filter, const float *d_input, float *d_output, const int *lengths, const float *d_h0, float *d_hT) {
    REC_ENTER("RNNApplyTrainingBatchDeviceVarLen", filter);
    return train_apply_vl_dev(&filter->l, "RNNApplyTrainingBatchDeviceVarLen", d_input, d_output, lengths, d_h0, NULL, d_hT, NULL);
}
int RNNCalculateGradientDeviceVarLen(RNN filter, float *d_grad, float *d_dX, const float *d_dout, const float *d_dhT, float *d_dh0) {
    REC_ENTER("RNNCalculateGradientDeviceVarLen", filter);
    return train_gradient_vl_dev(&filter->l, "RNNCalculateGradientDeviceVarLen", d_grad, d_dX, d_dout, d_dhT, NULL, d_dh0, NULL);
}
int RNNApplyTrainingBatchVarLen(RNN filter, const float *input, float *output, const int *lengths, const float *h0, float *hT) {
    REC_ENTER("RNNApplyTrainingBatchVarLen", filter);
    return train_apply_vl_host(&filter->l, "RNNApplyTrainingBatchVarLen", input, output, lengths, h0, NULL, hT, NULL);
}
int RNNCalculateGradientVarLen(RNN filter, RNNGradient *gradient, const float *d_out, const float *d_hT_grad, float *d_h0_grad) {
    REC_ENTER("RNNCalculateGradientVarLen", filter);
    return train_gradient_vl_host(&filter->l, "RNNCalculateGradientVarLen", gradient, d_out, d_hT_grad, NULL, d_h0_grad, NULL);
}
/* the bidirectional training calls (bd_train_*): forward / backward are two different RNNCreateForTraining handles of one shape */
int RNNBidirectionalApplyTrainingBatchDevice(RNN forward, RNN backward, const float *d_input, float *d_output, const int *lengths, int merge) {
    REC_ENTER("RNNBidirectionalApplyTrainingBatchDevice", forward && backward);
    return bd_train_forward_dev(&forward->l, &backward->l, "RNNBidirectionalApplyTrainingBatchDevice", d_input, d_output, lengths, merge);
}
int RNNBidirectionalCalculateGradientDevice(RNN forward, RNN backward, float *d_grad_forward, float *d_grad_backward, float *d_dX, const float *d_dout) {
    REC_ENTER("RNNBidirectionalCalculateGradientDevice", forward && backward);
    return bd_train_gradient_dev(&forward->l, &backward->l, "RNNBidirectionalCalculateGradientDevice", d_grad_forward, d_grad_backward, d_dX, d_dout);
}
int RNNBidirectionalApplyTrainingBatch(RNN forward, RNN backward, const float *input, float *output, const int *lengths, int merge) {
    REC_ENTER("RNNBidirectionalApplyTrainingBatch", forward && backward);
    return bd_train_forward_host(&forward->l, &backward->l, "RNNBidirectionalApplyTrainingBatch", input, output, lengths, merge);
}
int RNNBidirectionalCalculateGradient(RNN forward, RNN backward, RNNGradient *grad_forward, RNNGradient *grad_backward, float *d_X, const float *d_out) {
    REC_ENTER("RNNBidirectionalCalculateGradient", forward && backward);
    return bd_train_gradient_host(&forward->l, &backward->l, "RNNBidirectionalCalculateGradient", grad_forward, grad_backward, d_X, d_out);
}
