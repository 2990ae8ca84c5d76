/*
 * nntk_shim.h -- the thin C-ABI between the C host layer (csrc/host) and the
 * hand-written HIP kernels (csrc/hip).  Plain pointers and ints only; no
 * HIP types.  All `d_` pointers are device addresses.  Every launcher enqueues on
 * the current stream (nntk_shim_stream) and returns 0, or -1 after recording a
 * message retrievable with nntk_shim_error().
 */
#ifndef NNTK_SHIM_H
#define NNTK_SHIM_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* activation kinds understood by the device code */
enum {
    NNTK_ACT_NONE     = -1,   /* no activation handle (dense.c:127-133 copy branch) */
    NNTK_ACT_IDENTITY = 0,
    NNTK_ACT_SIGMOID  = 1,
    NNTK_ACT_TANH     = 2,
    NNTK_ACT_RELU     = 3,
    NNTK_ACT_SOFTMAX  = 4,
    NNTK_ACT_LOG_EPS  = 5,    /* log(x + a): log-mel epilogue (log_mel_spectrogram.c:34-35); a rides in relu_a */
    NNTK_ACT_CUSTOM   = 100   /* host callback: not runnable on the device */
};

/* ---- runtime --------------------------------------------------------------- */
int         nntk_shim_device_count(void);
int         nntk_shim_set_device(int device);
int         nntk_shim_get_device(void);            /* the calling thread's current device, -1 without one */
void        nntk_shim_set_stream(void *stream);
void       *nntk_shim_get_stream(void);
int         nntk_shim_synchronize(void);
const char *nntk_shim_error(void);
void        nntk_shim_set_error(const char *msg);
void        nntk_shim_clear_error(void);

/* tuning / diagnostics knobs by name ("rec_persistent", "rec_pingpong", "gemm_tm_batch", ...; value "auto" restores
 * the default).  Environment variables NNTK_<NAME> give the initial values, read once. */
int nntk_shim_set_option(const char *name, const char *value);
int nntk_shim_get_option(const char *name, int *value);
/* sticky fault word of the persistent recurrent kernel (see runtime.hip) */
int nntk_shim_take_fault(void);            /* after a stream sync: 1 = a launch faulted (cleared, per-step kernels from now on) */
int nntk_shim_persistent_disabled(void);
const char *nntk_shim_last_conv_kernel(void);  /* ... of the Conv1d / dense GEMM kernel ("conv1d_mfma_bf16x3_kernel<frag3>", ...) */
const char *nntk_shim_last_rec_kernel(void);   /* name of the recurrent kernel this thread launched last ("" before the first) */
int nntk_shim_device_status(void);         /* non-blocking: 1 = a completed recurrent launch has faulted */

/* HIP-event spans around the recurrent step launches (off by default) */
void nntk_shim_profile_enable(int on);
int  nntk_shim_profile_get(const char *name, double *total_ms, long *launches, long *timesteps);

void *nntk_shim_malloc(size_t bytes);
void  nntk_shim_free(void *d_ptr);
void *nntk_shim_host_alloc(size_t bytes);              /* pinned, zero-filled */
void  nntk_shim_host_free(void *ptr);
int   nntk_shim_upload(void *d_dst, const void *h_src, size_t bytes);     /* blocking */
int   nntk_shim_upload_async(void *d_dst, const void *h_src, size_t bytes);        /* async on stream (pinned source) */
int   nntk_shim_download(void *h_dst, const void *d_src, size_t bytes);   /* blocking; -1 if a recurrent launch faulted */
int   nntk_shim_download_nocheck(void *h_dst, const void *d_src, size_t bytes);    /* blocking; leaves a fault for nntk_shim_take_fault */
int   nntk_shim_download_rows(void *h_dst, const void *d_src, size_t spitch, size_t width, size_t height);   /* strided rows, packed at the destination */
int   nntk_shim_copy_d2d(void *d_dst, const void *d_src, size_t bytes);   /* async on stream */
int   nntk_shim_copy_rows_d2d(void *d_dst, const void *d_src, size_t spitch, size_t width, size_t height);   /* strided rows -> packed, async */
int   nntk_shim_memset(void *d_ptr, int value, size_t bytes);             /* async on stream */

/* ---- K2/K3: implicit-GEMM conv1d / dense on f32 MFMA with fused epilogue ----
 * out[b, x, o] = act( bn( bias[o] + sum_{kk,i} in[b, x*stride+kk, i] * Wp[(kk*Cin_p + i), o] ) )
 *   d_in   [B, T, Cin]           channels-last
 *   d_wp   packed weights [Cout_p][k*Cin_p], K-contiguous, zero padded (see nntk_shim_conv_pack_sizes)
 *   d_bias [Cout]
 *   d_bn   NULL or 6*Cout floats: gamma | beta | mean | variance (batch_norm.c:79-84 order) | sd | 1/sd, the last
 *          two written by nntk_shim_bn_derive(d_bn, eps, Cout) after an upload of the first four
 *   out_mode 0: out[b, x, :] at row b*Tout + x;  1: time-major row x*B + b (for recurrent input projections)
 * Dense / TimeDistributedDense / input projection = the k=1, stride=1 case with T = rows.
 */
void nntk_shim_conv_pack_sizes(int Cin, int Cout, int k, int *Cin_p, int *Cout_p);
/* d_wp of nntk_shim_conv1d is the packed f32 matrix [Cout_p][k * Cin_p] FOLLOWED BY its three bf16 split images
 * (hi | mid | lo, each Cout_p * k * Cin_p bf16 in MFMA fragment order) written by
 * nntk_shim_split_bf16x3(d_wp, d_wp + n, Cout_p, k * Cin_p); the images are read only by the split-bf16 kernel */
int  nntk_shim_bn_derive(float *d_block, float eps, int C);
int  nntk_shim_split_bf16x3(const float *d_src, void *d_dst, int rows, int ktot);
/* on = 1: this packed weight block holds a non-finite, > 3.39e38 or denormal value, which the bf16 split cannot represent
 * exactly -- the "auto" contraction takes the exact-f32 kernel for it.  on = 0 (re-upload of clean weights, free) clears. */
void nntk_shim_weights_exact_only(const void *d_wp, int on);
int  nntk_shim_conv1d(const float *d_in, const float *d_wp, const float *d_bias, const float *d_bn,
                      float bn_eps, int act_kind, float relu_a, float *d_out,
                      int B, int T, int Cin, int Cout, int k, int stride, int Tout, int out_mode);

/* ---- training, first slice: Conv1dCalculateGradient (conv_1d.c:185-245); untuned VALU kernels, deterministic ---- */
/* Conv1d (+ BatchNorm + activation) with a frag3 tensor as output (conv1d.hip conv_epilogue_frag3); 1 = this form does not take the call */
int  nntk_shim_conv1d_frag3(const float *d_in, const float *d_wp, const float *d_bias, const float *d_bn,
                            float bn_eps, int act_kind, float relu_a, float *d_out_f3,
                            int B, int T, int Cin, int Cout, int k, int stride, int Tout);
/* flat-K split convolution (conv1d_flatk.hip; stride 1, Cin % 8 == 0, Cin % 16 != 0): d_wpf = [Cout_p][Kf_p] with K = tap * Cin + channel,
 * Kf_p = k * Cin rounded up to 16, followed by its split images (nntk_upload_packed_weights).  Returns 1 when not taken. */
int nntk_shim_conv1d_flatk(const float *d_in, const float *d_wpf, const float *d_bias, const float *d_bn,
                           float bn_eps, int act_kind, float relu_a, float *d_out,
                           int B, int T, int Cin, int Cout, int k, int Tout);
size_t nntk_shim_conv1d_grad_scratch_floats(int Cin, int Cout, int k);
int nntk_shim_conv1d_grad(const float *d_in, const float *d_W, const float *d_dout, float *d_dW, float *d_db,
                          float *d_dX, float *d_scratch, int B, int T, int Cin, int Cout, int k, int stride, int Tout);

/* ---- standalone BatchNorm (batch_norm.c:140-163 op order) and activations -- */
int nntk_shim_batch_norm(const float *d_in, const float *d_bn /*gamma|beta|mean|var*/, float eps,
                         float *d_out, long rows, int C);
int nntk_shim_activation(int kind, float relu_a, int softmax_vector_size,
                         const float *d_in, float *d_out, long n_elems);

/* ---- bidirectional helpers (layers/bidirectional.c): rows of [B, T, F] in reverse time order; row-wise
 *      concatenation [rows, C] | [rows, C] -> [rows, 2C]; elementwise sum */
int nntk_shim_reverse_time(const float *d_in, float *d_out, long B, int T, int F);
/* ragged rows: out[b][t] = in[b][len[b] - 1 - t] for t < len[b], zeros for t >= len[b] (d_len [B], device) */
int nntk_shim_reverse_time_varlen(const float *d_in, float *d_out, const int *d_len, long B, int T, int F);
/* n ints from host memory to the device, ordered on the stream; the host array may be reused when the call returns */
int nntk_shim_upload_ints(int *d_dst, const int *h_src, long n);
/* ---- streaming calls (INTEGRATION.md "Streaming a whole stack") ----
 * d_cnt = [4][B] ints on the device: emitted frames / outputs | steps in the assembled row (m) | old state steps | new state steps.
 * stream_gather: d_seq [B][state_rows + in_rows][C] = state ++ new input ++ zeros per row, then the state rows take the row's last
 * (new state) steps, in place.  spectrogram_rows: K1 on assembled rows with per-row sample and frame counts (spectrogram.hip ST
 * instantiations); rows past a row's frames are not written; 1 = the fused mel form does not take this nfft (nothing launched). */
int nntk_shim_stream_gather(const float *d_in, float *d_state, float *d_seq, const int *d_cnt, int B, int in_rows, int state_rows, int C);
int nntk_shim_spectrogram_rows(const float *d_in, const float *d_window, const float *d_twiddle, float *d_out,
                               int B, int row_stride, int nfft, int window_size, int step, int nfreq, int max_frames,
                               float fft_norm, int mode, float scale, const int *d_cnt,
                               const int *d_mel_tab, const float *d_mel_w, int n_mels, float eps, int do_log);
/* ---- training, second slice (train.hip): reference operation order throughout ---- */
int nntk_shim_activation_grad(int kind, int vector_size, int vectors_per_call, const float *d_z, const float *d_a,
                              const float *d_dout, float *d_out, long n);
int nntk_shim_dense_grad(const float *d_x, const float *d_W /*[in,out] caller layout*/, const float *d_dz, float *d_gW,
                         float *d_gb, float *d_dX, int B, int in, int out);
int nntk_shim_loss_rows(int kind /*0 mse, 1 categorical ce*/, const float *d_y, const float *d_pred, float *d_per_row, int size, int batch);
int nntk_shim_loss_grad(int kind, const float *d_y, const float *d_pred, float *d_out, int size, int batch);
int nntk_shim_sgd(float lr, const float *d_grad, float *d_w, long n);
/* ---- the multi-tensor optimizer step (optim.hip): two launches per step for any number of blocks.  The host (train.c) has checked every
 *      argument and built the tables; all pointers are device memory.
 *      d_blocks [n_blocks]: w, g the caller's pointers; m, v the moments (NULL where the kind has none), laid out with the 16-byte phase of
 *      w (phase = (address of w / 4) & 3, so w - phase, m - phase, v - phase are 16-byte aligned); g_vec = g has that phase too; chunk0 =
 *      the block's first chunk in the flat chunk list, a block taking ceil((phase + n) / chunk_floats) chunks.
 *      d_partial [n_chunks]; d_ctl [8] = norm | clip factor | skipped | steps taken | learning rate | steps (uint, read) | steps (uint,
 *      written) | unused ---- */
typedef struct { float *w, *g, *m, *v; long n; long chunk0; int phase, g_vec; } nntk_optim_block;
typedef struct {
    int kind, nesterov, decoupled, zero_gradients;
    float momentum, beta1, beta2, epsilon, weight_decay, grad_scale, clip_norm;
    int n_blocks, chunk_floats;
    long n_chunks;
    const nntk_optim_block *d_blocks;
    float *d_partial, *d_ctl;
} nntk_optim_plan;
int nntk_shim_optim_chunk_floats(long total_floats);
int nntk_shim_optim_step(const nntk_optim_plan *plan);
int nntk_shim_optim_set_lr(float *d_ctl, float lr);        /* in stream order */
/* the CTC kernels' limits, stated here once for the host's checks (ctc.c) and the launchers */
#define NNTK_CTC_BEAM_MAX_W 128
#define NNTK_CTC_BEAM_MAX_CELLS 16384           /* beam_width x (expanded classes + 1) cells of 8 bytes: 128 KiB of the 160 KiB of LDS */
#define NNTK_CTC_BEAM_MAX_T ((1 << 23) - 1)     /* frames of a row, or of a stream's row since its reset: length << 8 < 2^31 in the records */
#define NNTK_CTC_ALIGN_MAX_LABELS 4000          /* max_label_len of the alignment and the loss: a row's extended states live in LDS */
/* ---- CTC (ctc.hip): loss rows, gradient with respect to the probabilities, best-path decoding.  The int arrays are HOST memory,
 *      already checked by the caller (ctc.c), never NULL, copied in stream order; d_dprobs NULL = loss only; d_ws 16-byte aligned,
 *      nntk_shim_ctc_workspace_floats words (loss only: the int arrays and 2 words per row at its start are all that is touched) ---- */
size_t nntk_shim_ctc_workspace_floats(int batch, int T, int max_label_len);
int nntk_shim_ctc_loss(const float *d_probs, int B, int T, int C, const int *h_input_lengths, const int *h_labels,
                       const int *h_label_lengths, int max_label_len, int blank, float *d_loss_rows, float *d_dprobs, float *d_ws);
int nntk_shim_ctc_greedy_decode(const float *d_probs, int B, int T, int C, const int *h_input_lengths, int blank, int *d_labels_out,
                                int *d_out_lengths);
/* the chunk's labels only: d_prev [B] device, in/out, the argmax of each row's last frame seen (-1: none) */
int nntk_shim_ctc_greedy_decode_stream(const float *d_probs, int B, int T, int C, const int *h_input_lengths, int blank, int *d_prev,
                                       int *d_labels_out, int *d_out_lengths);
/* Language-model fusion (INTEGRATION.md "CTC prefix beam search", Language-model fusion): the device tables of an n-gram handle, 16-byte
 * records -- arcs {label, next state, factor mantissa, factor exponent}, states {first arc, arcs, backoff state, 0} and per-state factors
 * {backoff m, e, final m, e}.  depth = the longest backoff chain: the walk's loop count. */
typedef struct {
    const int *d_arcs, *d_states, *d_factors;
    int n_states, start_state, depth, unk_m, unk_e;
} nntk_shim_lm;
/* ---- CTC prefix beam search (ctc_beam.hip): the n-best prefixes of every row with their log-probabilities.  lm NULL (the sizes and the
 *      check: lm 0): acoustic scores only, on kernels compiled without the model.  h_input_lengths is HOST memory, checked by the caller
 *      (ctc.c), never NULL; d_ws 16-byte aligned, nntk_shim_ctc_beam_workspace_floats words.  d_label_frames / d_label_logps
 *      ([B][nbest][T], either or both NULL): the labels' frames and log-probabilities; both NULL: the kernels compiled without them ---- */
size_t nntk_shim_ctc_beam_workspace_floats(int batch, int T, int C, int beam_width, int cutoff_top_n, int lm);
int nntk_shim_ctc_beam_decode(const float *d_probs, int B, int T, int C, const int *h_input_lengths, int blank, int beam_width,
                              int cutoff_top_n, int nbest, const nntk_shim_lm *lm, int *d_labels_out, int *d_out_lengths,
                              float *d_scores, int *d_label_frames, float *d_label_logps, float *d_ws);
/* streaming form: d_buf = the handle's buffer, nntk_shim_ctc_beam_stream_floats words, 16-byte aligned, kept from push to push (the
 * carried beam, both halves of the label strings, the records and cut pairs of one push).  h_ctl HOST [4][B], built by ctc.c:
 * frames in this push | frames the row had seen before it | the current half of its label strings | 0.  any_frames 0: no row brings
 * a frame, only the outputs are rewritten.  _check: the launch-time limits, without a device.  detail: the handle also carries both
 * halves of the labels' frame and log-probability strings; d_label_frames / d_label_logps ([B][nbest][max_labels], either may be NULL)
 * report them and are NULL without it. */
size_t nntk_shim_ctc_beam_stream_floats(int batch, int max_frames, int C, int beam_width, int cutoff_top_n, int max_labels, int lm,
                                        int detail);
int nntk_shim_ctc_beam_stream_check(int C, int beam_width, int cutoff_top_n, int lm);
int nntk_shim_ctc_beam_stream_push(const float *d_probs, int B, int max_frames, int C, const int *h_ctl, int any_frames, int blank,
                                   int beam_width, int cutoff_top_n, int nbest, int max_labels, const nntk_shim_lm *lm, int detail,
                                   int *d_labels_out, int *d_out_lengths, float *d_scores, int *d_label_frames, float *d_label_logps,
                                   float *d_buf);
/* ---- CTC forced alignment (ctc_align.hip): the best single alignment of every row to its labels -- the state of every frame, the
 *      frame span of every label, ln of the path's probability.  The int arrays are HOST memory, already checked by the caller
 *      (ctc.c), never NULL; d_states / d_spans may be NULL; d_ws 16-byte aligned, nntk_shim_ctc_align_workspace_floats words ---- */
size_t nntk_shim_ctc_align_workspace_floats(int batch, int T, int max_label_len);
int nntk_shim_ctc_align(const float *d_probs, int B, int T, int C, const int *h_input_lengths, const int *h_labels,
                        const int *h_label_lengths, int max_label_len, int blank, int *d_states, int *d_spans, float *d_scores,
                        float *d_ws);
/* ---- Error counts and the MWER risk (edit_distance.hip).  d_hyp [B][n_hyp][max_hyp_len] / d_hyp_len [B][n_hyp] device, as the decoders
 *      write them; h_refs [B][max_ref_len] / h_ref_len [B] HOST memory, already checked by the caller (metrics.c), never NULL, copied in
 *      stream order; sep < 0 units, sep >= 0 words; d_counts [B][n_hyp][4]; d_ref_units [B] or NULL; d_ws 16-byte aligned,
 *      nntk_shim_edit_distance_workspace_floats words ---- */
#define NNTK_EDIT_MAX_HYP_LEN 32767             /* every count of a cell fits 16 bits */
#define NNTK_EDIT_MAX_REF_LEN NNTK_CTC_ALIGN_MAX_LABELS   /* the loss calls' limit: three diagonals of max_ref_len + 1 cells, 8 bytes each, live in LDS */
size_t nntk_shim_edit_distance_workspace_floats(int batch, int n_hyp, int max_hyp_len, int max_ref_len);
int nntk_shim_edit_distance(const int *d_hyp, const int *d_hyp_len, int B, int n_hyp, int max_hyp_len, const int *h_refs,
                            const int *h_ref_len, int max_ref_len, int sep, int *d_counts, int *d_ref_units, float *d_ws);
/* d_err read at d_err[(b * n_hyp + k) * err_stride]; d_risk_rows [B] / d_dlogp [B][n_hyp], either may be NULL */
int nntk_shim_mwer(const float *d_logp, const int *d_err, int err_stride, int B, int n_hyp, float *d_risk_rows, float *d_dlogp);
int nntk_shim_row_scale(const float *d_x, const float *d_scale, long rows, long row_floats, float *d_out);      /* d_out may be d_x */
/* the transducer kernels' limits, stated here once for the host's checks (rnnt.c) and the launcher */
#define NNTK_RNNT_MAX_LABELS 4000               /* max_label_len: two diagonals of max_label_len + 1 cells, 16 bytes each, live in LDS */
#define NNTK_RNNT_MAX_DIAGONALS 65536           /* T + max_label_len: the exponents of that many emissions (each >= -4000) sum inside 2^28 */
/* ---- RNN-Transducer (rnnt.hip): loss rows and the gradient with respect to the unnormalised scores [B][T][max_label_len + 1][V]; the
 *      joiner and its backward.  The int arrays are HOST memory, already checked by the caller (rnnt.c), never NULL, copied in stream
 *      order; d_dlogits NULL = loss only; the tensors and d_ws 16-byte aligned, nntk_shim_rnnt_workspace_floats words ---- */
size_t nntk_shim_rnnt_workspace_floats(int batch, int T, int max_label_len, int want_grad);
int nntk_shim_rnnt_loss(const float *d_logits, int B, int T, int V, const int *h_input_lengths, const int *h_labels,
                        const int *h_label_lengths, int max_label_len, int blank, float *d_loss_rows, float *d_dlogits, float *d_ws);
int nntk_shim_rnnt_joint(const float *d_enc, const float *d_pred, int B, int T, int U1, int J, int kind, float *d_out);
int nntk_shim_rnnt_joint_backward(const float *d_out_fwd, const float *d_dout, int B, int T, int U1, int J, int kind, float *d_denc,
                                  float *d_dpred);
/* ---- the fused transducer training loss (rnnt_fused.hip): joiner, vocabulary projection and loss from enc [B][T][J], pred [B][U1][J] and
 *      the Dense block W [J,V] | b [V]; the three gradient pointers all NULL = loss only.  Host int arrays as for nntk_shim_rnnt_loss,
 *      already checked by the caller (rnnt.c).  The limits: a tile's 32 rows of z (J floats each) and a group of g columns share one
 *      workgroup's LDS; V only bounds the partial blocks of d W. ---- */
#define NNTK_RNNT_FUSED_MAX_J 1024
#define NNTK_RNNT_FUSED_MAX_V 8192
size_t nntk_shim_rnnt_fused_workspace_floats(int batch, int T, int max_label_len, int J, int V, int want_grad);
int nntk_shim_rnnt_fused_loss(const float *d_enc, const float *d_pred, const float *d_out, int B, int T, int J, int V, int kind,
                              const int *h_input_lengths, const int *h_labels, const int *h_label_lengths, int max_label_len, int blank,
                              float *d_loss_rows, float *d_denc, float *d_dpred, float *d_dout, float *d_ws);
/* ---- the pruned transducer training loss (rnnt_pruned.hip).  Host int arrays as for nntk_shim_rnnt_loss, already checked by the caller
 *      (rnnt.c), never NULL; d_ranges [B][T] is DEVICE memory and clamped into [0, U1 - S] by every kernel that reads it.
 *      simple_loss: scores am [B][T][V] + lm [B][U1][V], both 16-byte aligned; d_dam and d_dlm both NULL or both given; d_occ
 *      [B][T][U1] may be NULL; the workspace with want_grad = a gradient or the occupancies are asked.
 *      prune_ranges: d_ws takes the two length arrays.  pruned_loss: d_logits [B][T][S][V] and d_dlogits (NULL = loss only) 16-byte
 *      aligned; its workspace is nntk_shim_rnnt_workspace_floats ---- */
size_t nntk_shim_rnnt_simple_workspace_floats(int batch, int T, int max_label_len, int want_grad);
int nntk_shim_rnnt_simple_loss(const float *d_am, const float *d_lm, int B, int T, int V, const int *h_input_lengths, const int *h_labels,
                               const int *h_label_lengths, int max_label_len, int blank, float *d_loss_rows, float *d_dam, float *d_dlm,
                               float *d_occ, float *d_ws);
size_t nntk_shim_rnnt_prune_workspace_floats(int batch);
int nntk_shim_rnnt_prune_ranges(const float *d_occ, int B, int T, int U1, const int *h_input_lengths, const int *h_label_lengths, int S,
                                int *d_ranges, float *d_ws);
int nntk_shim_rnnt_pruned_joint(const float *d_enc, const float *d_pred, const int *d_ranges, int B, int T, int U1, int S, int J, int kind,
                                float *d_out);
int nntk_shim_rnnt_pruned_joint_backward(const float *d_out_fwd, const float *d_dout, const int *d_ranges, int B, int T, int U1, int S, int J,
                                         int kind, float *d_denc, float *d_dpred);
int nntk_shim_rnnt_pruned_loss(const float *d_logits, const int *d_ranges, int B, int T, int S, int V, const int *h_input_lengths,
                               const int *h_labels, const int *h_label_lengths, int max_label_len, int blank, float *d_loss_rows,
                               float *d_dlogits, float *d_ws);
/* ---- transducer forced alignment (rnnt_align.hip): the best single path of every row through its lattice, on the emissions of
 *      either score source: stored scores (rnnt.hip's writer) or the joiner's inputs (rnnt_fused.hip's).  Host int arrays as for
 *      nntk_shim_rnnt_loss, already checked by the caller (rnnt.c), never NULL; the four path outputs may be NULL; d_ws 16-byte
 *      aligned: the source's loss-only workspace, then one backpointer byte per cell of batch * (T + max_label_len) diagonals of
 *      min(T, max_label_len + 1) cells ---- */
typedef struct {
    int fused;                              /* 0: d_logits [B][T][max_label_len + 1][V], 16-byte aligned; 1: the joiner's inputs below */
    const float *d_logits;
    const float *d_enc, *d_pred, *d_out;    /* [B][T][J], [B][max_label_len + 1][J], W [J,V] | b [V] */
    int J, kind;
} nntk_shim_rnnt_src;
typedef struct { int *label_frames, *frame_labels; float *label_logp, *frame_logp, *scores; } nntk_shim_rnnt_path;   /* the outputs */
size_t nntk_shim_rnnt_align_workspace_floats(const nntk_shim_rnnt_src *src, int batch, int T, int V, int max_label_len);
int nntk_shim_rnnt_align(const nntk_shim_rnnt_src *src, int B, int T, int V, const int *h_input_lengths, const int *h_labels,
                         const int *h_label_lengths, int max_label_len, int blank, const nntk_shim_rnnt_path *out, float *d_ws);
/* ---- greedy transducer decoding (rnnt_decode.hip).  The limits, stated once for the host's checks (rnnt_decode.c) and the launcher: a
 *      row's h, c, g, joiner output and max(4H, V) logits / gate pre-activations live in one workgroup's LDS (48 KiB at the limits), and
 *      the folded input table is V x 4H floats (128 MiB at the limits).  Batches above NNTK_RNNT_DEC_GROUP_BATCH rows put
 *      NNTK_RNNT_DEC_GROUP rows into a workgroup where their LDS fits (nntk_shim_rnnt_dec_rows_per_group); the bits do not depend on it. ---- */
#define NNTK_RNNT_DEC_MAX_WIDTH 1024            /* E, H, J */
#define NNTK_RNNT_DEC_MAX_V 8192
#define NNTK_RNNT_DEC_GROUP 4
#define NNTK_RNNT_DEC_GROUP_BATCH 512
/* the decoder's own device blocks: d_table [V][4H] = embed W + b_i + b_h, d_U [H][4H], d_proj [H][J] | b [J] or NULL, d_out [J][V] | b [V] */
typedef struct {
    const float *d_table, *d_U, *d_proj, *d_out;
    int V, blank, E, H, J, activation, max_symbols_per_frame;
} nntk_shim_rnnt_dec;
int nntk_shim_rnnt_dec_rows_per_group(int batch, int H, int J, int V);
int nntk_shim_rnnt_dec_table(const float *d_embed, const float *d_lstm, int V, int E, int H, float *d_table);
int nntk_shim_rnnt_dec_reset(int *d_st_i, const int *d_rows, int n_rows);      /* the listed rows start anew; in stream order */
/* h_n_frames HOST [batch], checked by the caller, copied in stream order (it rides in d_lengths).  State: d_st_f [batch][2H + J] (h | c |
 * g), d_st_score [batch] doubles, d_st_i [batch][4] (started | symbols in the frame | labels | frames consumed), or three NULLs: every
 * row from the start.  d_frames, d_scores may be NULL. */
int nntk_shim_rnnt_greedy(const nntk_shim_rnnt_dec *m, const float *d_enc, int batch, int T, const int *h_n_frames, int max_labels,
                          float *d_st_f, double *d_st_score, int *d_st_i, int *d_labels, int *d_frames, int *d_lengths, float *d_scores);
/* ---- transducer beam search (rnnt_beam.hip) on the greedy decoder's blocks.  One workgroup runs a row's whole search; the hypotheses
 *      of a depth share passes over the matrices in groups of NNTK_RNNT_DEC_GROUP where the group's LDS fits, else one by one
 *      (nntk_shim_rnnt_beam_group; nntk_shim_rnnt_beam_set_group(1 or NNTK_RNNT_DEC_GROUP) pins it for tests and timing, 0 = automatic;
 *      the bits do not depend on it).  The workspace, nntk_shim_rnnt_beam_workspace_floats words, holds the rows' frame counts, then per
 *      row three parts, each behind the one before so that an absent one moves nothing, S' = min(max_symbols_per_frame, max_labels):
 *        acoustic       (S' + 2) beam_width hypothesis slots (h | c | g, the labels, length and hash), beam_width V logits and the
 *                       frame's list B of beam_width (S' + 1) finished hypotheses;
 *        with_lm        an int per hypothesis slot (its LM state) and beam_width V doubles;
 *        with_detail    two words per hypothesis slot and label (frame, log-probability) and three per entry of B. ---- */
#define NNTK_RNNT_BEAM_MAX_W 32
size_t nntk_shim_rnnt_beam_workspace_floats(int batch, int H, int J, int V, int max_sym, int beam_width, int max_labels, int with_lm,
                                            int with_detail);
int nntk_shim_rnnt_beam_fits(int H, int J, int V);                             /* the kernel's LDS at one hypothesis a pass */
int nntk_shim_rnnt_beam_group(int beam_width, int H, int J, int V);
void nntk_shim_rnnt_beam_set_group(int group);
/* a stream's rows: score [batch][W] doubles, f [batch][W][2H + J], lab [batch][W][max_labels], meta [batch][W][2] (length | hash),
 * i [batch][4] (started | hypotheses | frames consumed, with detail | -); all NULL: every row from the start, nothing kept */
typedef struct {
    double *score;
    float *f;
    int *lab, *meta, *i;
} nntk_shim_rnnt_beam_state;
/* Language-model fusion (INTEGRATION.md "RNN-Transducer: beam search", Language-model fusion).  The search adds natural logs in double, so
 * next to the lookup records of nntk_shim_lm (d_arcs {label, next state, -, -}, d_states {first arc, arcs, backoff state, 0}) it reads
 * tables of its own: d_arc_ln [arcs] = ln G, d_state_ln [states][2] = ln B | ln E, and ln U. */
typedef struct {
    const int *d_arcs, *d_states;
    const double *d_arc_ln, *d_state_ln;
    double unk_ln;
    int start_state;
} nntk_shim_rnnt_lm;
/* Label timestamps, confidences and length normalisation (include/nntoolkitcore_hip.h, "Label timestamps" under the beam search).
 * d_frames, d_logps [batch][nbest][max_labels], each may be NULL.  d_st_fr, d_st_lp [batch][W][max_labels]: the arrays of a stream's
 * rows, both or neither (neither: the arrays are not carried); the frames a row has consumed ride in word 2 of the state's i, read only
 * while the row's started word is set, so a reset row counts from 0 again. */
typedef struct {
    int *d_frames;
    float *d_logps;
    int *d_st_fr;
    float *d_st_lp;
    int length_norm;
} nntk_shim_rnnt_beam_detail;
/* h_n_frames HOST [batch], checked by the caller, copied in stream order into the workspace; d_ws 16-byte aligned, sized with the flags
 * lm != NULL and dt != NULL.  st NULL: one-shot.  lm NULL: the acoustic search; with st and lm, d_st_q [batch][W] carries each
 * hypothesis's LM state.  dt NULL: no detail, the report in the search's own order (by score + ln E with lm); the same search either way. */
int nntk_shim_rnnt_beam(const nntk_shim_rnnt_dec *m, const float *d_enc, int batch, int T, const int *h_n_frames, int beam_width, int nbest,
                        int max_labels, const nntk_shim_rnnt_beam_state *st, const nntk_shim_rnnt_lm *lm, int *d_st_q,
                        const nntk_shim_rnnt_beam_detail *dt, int *d_labels, int *d_lengths, float *d_scores, float *d_ws);
/* ---- the prediction network's label embedding, for training (rnnt_pred.hip).  rows_select: d_out [rows][width] = d_src[h_idx[r]][:], exact
 *      zeros for h_idx[r] < 0; h_idx HOST memory, checked by the caller, carried in the kernel arguments.  embedding_grad: d_dtable [V][E],
 *      every element written, from the caller's plan (rnnt_pred.c), HOST ints laid out offsets [V + 1] | sorted rows [n_sorted] | heavy
 *      chunks [n_items][2] (id, chunk) | heavy ids [n_heavy][2] (id, first partial slot), uploaded in stream order into d_ws (16-byte
 *      aligned, nntk_shim_embedding_workspace_floats(rows >= n_sorted, V, E) floats); an id is heavy above NNTK_EMBED_CHUNK rows ---- */
#define NNTK_EMBED_CHUNK 32
int nntk_shim_rows_select(const float *d_src, int width, const int *h_idx, long rows, float *d_out);
size_t nntk_shim_embedding_workspace_floats(long rows, int V, int E);
int nntk_shim_embedding_grad(const float *d_dout, int V, int E, const int *h_plan, long n_sorted, long n_items, long n_heavy, float *d_dtable,
                             float *d_ws);
/* BatchNorm training (batch_norm.c:191-386): x, d_out [N, F]; d_block = gamma | beta | ...; d_stats [8][F] = mean | variance |
 * var_eps | sqrt_var | d_beta | d_gamma | d_var | d_mu; d_partial [slices][3][F] with slices from nntk_shim_bn_train_slices */
/* Ragged batches and carried state for the recurrent training launchers below (the *VarLen training calls; a NULL pointer to it = the
 * fixed-length, zero-state pass on the same kernels).  All pointers are device memory and may be NULL. */
typedef struct {
    const int *d_len;            /* [B] row lengths in [0, T], then the 64-row tiles' maxima (nntk_shim_rr_varlen's layout); NULL: every row T */
    int max_len;                 /* the longest row (read only with d_len) */
    const float *d_h0, *d_c0;    /* [B][H] initial state (zeros) */
    const float *d_dhT, *d_dcT;  /* [B][H] gradient arriving at the final state (zeros) */
    float *d_dh0, *d_dc0;        /* [B][H] gradient with respect to the initial state (not computed) */
} nntk_train_vl;
/* Recurrent training, one pair of calls for the three cells: G = gates per hidden unit, 1 RNN (rnn.c:144-221, :249-351), 3 GRU
 * (gru.c:246-512), 4 LSTM (lstm.c:185-239, :294-556).  Caller-layout weights W [in][G H], U [H][G H]; acts / scales in the order z, h, r
 * (GRU) | i, f, g, o, out (LSTM) | the one (RNN); the GRU always adds b_h, the others with use_bh.  Caches per (b, t): d_h [H];
 * d_Zg: GRU Z_gates [6H], LSTM zifgo [8H], RNN the pre-activation [H]; d_c [H]: GRU h_prev U_h + b_hh, LSTM the cell state, RNN unused.
 * backward: d_UT = U transposed [G H][H]; d_dG [B][T][G H] the recurrent side's gate gradients, d_dxW the input side's (the GRU's differ,
 * the other cells pass one buffer twice); d_work: nntk_shim_rec_train_work_floats. */
int nntk_shim_rec_train_forward(int G, const float *d_x, const float *d_W, const float *d_U, const float *d_bi, const float *d_bh,
                                float *d_h, float *d_Zg, float *d_c, int B, int T, int in, int H, int use_bh,
                                const int *acts, const float *scales, const nntk_train_vl *vl);
size_t nntk_shim_rec_train_work_floats(int G, int B, int H);
int nntk_shim_rec_train_backward(int G, const float *d_dout, const float *d_UT, const float *d_h, const float *d_Zg, const float *d_c,
                                 float *d_dxW, float *d_dG, float *d_work, int B, int T, int H, int return_sequences,
                                 const int *acts, const float *scales, const nntk_train_vl *vl);
/* the same forward pass on the register-resident kernels (recurrent_rr.hip, TRAIN + VL): one launch, h0 / c0 in, hT / cT out (may be NULL),
 * the caches of every step a row runs; d_h rows past a row's length are unspecified until nntk_shim_varlen_zero_pad clears them.  cell 0
 * LSTM, 1 GRU (d_bi = the four-slot bias, d_bh NULL, d_c = the h.U_h + b_h cache).  0 launched, 1 shape / configuration not taken, -1 error */
int nntk_shim_rr_train_forward_vl(int cell, const float *d_x, const float *d_img, const float *d_bi, const float *d_bh,
                                  const float *d_h0, const float *d_c0, float *d_h, float *d_c, float *d_z, float *d_hT, float *d_cT,
                                  float *d_hseq, float *d_work, const int *d_len, int B, int T, int in, int H);
/* d_sT [B][H] = d_seq [B][T][H] at each row's last step, or d_s0 (zeros) for an empty row */
int nntk_shim_train_final_state(const float *d_seq, const int *d_len, const float *d_s0, float *d_sT, int B, int T, int H);
/* d_xm = d_x [B][T][F] with exact zeros at t >= d_len[b] */
int nntk_shim_train_mask_rows(const float *d_x, const int *d_len, float *d_xm, int B, int T, int F);
/* MFMA forms of the large training products: C [M][N] (+)= A [M][K] x Bw [N][K]^T through the inference GEMM kernel (Bw is
 * packed per call into d_pack >= nntk_shim_gemm_nt_scratch_floats(N, K) floats; accumulate uses d_tmp [M][N]) */
size_t nntk_shim_gemm_nt_scratch_floats(int N, int K);
int nntk_shim_gemm_nt(const float *d_A, const float *d_Bw, float *d_C, float *d_pack, float *d_tmp, long M, int N, int K, int accumulate);
int nntk_shim_transpose(const float *d_src, float *d_dst, long R, int C, int shift_T);
/* MFMA form of the Conv1d input gradient (stride 1): the forward kernel on zero-padded d_out with flipped weights (train.hip) */
size_t nntk_shim_conv_dx_pack_floats(int Cin, int Cout, int k);
int nntk_shim_conv_dx_mfma(const float *d_dout, const float *d_W, float *d_dX, float *d_pad, float *d_wpack,
                           int B, int T, int Cin, int Cout, int k, int Tout);
/* C [I][K] += A^T B over `rows` rows, c [K] += column sums of B (a_shift_T > 0: A is h [B][T][I] and row (b,t) uses h_{t-1}) */
size_t nntk_shim_outer_scratch_floats(int I, int K);
int nntk_shim_outer_accumulate(const float *d_A, const float *d_B, float *d_C, float *d_c, float *d_scratch, long rows, int I, int K, int a_shift_T);
/* out [rows][I] = d [rows][K] times M [I][K]^T, k-ordered */
int nntk_shim_rows_times_rowmat(const float *d_d, const float *d_M, float *d_out, long rows, int I, int K);
int nntk_shim_bn_train_slices(long N, int *rows_per_slice);
int nntk_shim_bn_train_forward(const float *d_x, const float *d_block, float eps, float *d_stats, float *d_partial, float *d_out, long N, int F);
int nntk_shim_bn_train_backward(const float *d_x, const float *d_dout, const float *d_block, float *d_stats, float *d_partial, float *d_dx, long N, int F);
int nntk_shim_concat2(const float *d_a, const float *d_b, float *d_out, long rows, int C);
int nntk_shim_add2(const float *d_a, const float *d_b, float *d_out, long n);
/* signal/dft.h: complex DFT of any size n (direct, double accumulation); d_tw = 2n floats from nntk_shim_dft_twiddles */
int nntk_shim_dft_twiddles(float *d_tw, int n);
int nntk_shim_dft(const float *d_re, const float *d_im, const float *d_tw, float *d_ore, float *d_oim, int n, int inverse);
int nntk_shim_split2(const float *d_in, float *d_a, float *d_b, long rows, int C);
/* ---- bidirectional training (bd_train.hip): the merge, the output-gradient scatter and the input-gradient sum, each with the per-row time
 *      reversal folded in.  d_len [B] on the device or NULL (every row T); L = its entry.  Rows t >= L are written as exact zeros whatever
 *      the inputs hold there.  Without return_sequences a row is one step and nothing is reversed.  -1 when an output overlaps an input.
 *      merge:      out[b][t] = merge(of[b][t], obr[b][L-1-t]); concat: [.., 2H], forward in [0, H); else of + obr, [.., H]
 *      scatter:    d_of[b][t] = dout[b][t][forward part], d_ob[b][t] = dout[b][reverse ? L-1-t : t][backward part] (sum merge: both whole rows)
 *      accumulate: dx[b][t] = dxf[b][t] + dxbr[b][L-1-t]   (d_dx may be d_dxf) ---- */
int nntk_shim_bd_merge(const float *d_of, const float *d_obr, float *d_out, const int *d_len, long B, int T, int H,
                       int return_sequences, int concat);
int nntk_shim_bd_scatter(const float *d_dout, float *d_of, float *d_ob, const int *d_len, long B, int T, int H,
                         int return_sequences, int concat, int reverse);
int nntk_shim_bd_accumulate(const float *d_dxf, const float *d_dxbr, float *d_dx, const int *d_len, long B, int T, int F);

/* ---- K4: recurrent layers -------------------------------------------------
 * d_xw   [T, B, G*H] time-major input projections INCLUDING b_i (from nntk_shim_conv1d out_mode 1)
 * d_ut   packed recurrent weights U^T: [G*H, H] (row n = column n of U)
 * d_bh   [G*H] recurrent bias (NULL = none; LSTM v2=false)
 * d_h0 / d_c0  [B, H] initial state or NULL for zeros
 * d_out  [B, T, H] if return_sequences else [B, H]
 * d_hT / d_cT  [B, H] final state (may be NULL)
 * d_work scratch >= nntk_shim_recurrent_work_floats(B, H) floats
 * acts   GRU: {z, h, r};  LSTM: {i, f, g, o, out}
 * act_scales  parallel to acts: ReLU's output scale `a` (activation_default.c:123-129), ignored for other kinds; NULL = 1
 */
/* simple RNN cell (rnn.c:144-166): one gate, h' = act(xW + hU + b); same buffers as nntk_shim_gru */
int nntk_shim_rnn(const float *d_xw, const float *d_ut, const float *d_bh, const float *d_h0,
                  float *d_out, float *d_hT, float *d_work, int B, int T, int H,
                  int return_sequences, int act, float act_scale);
size_t nntk_shim_recurrent_work_floats(int B, int H);
/* per-row lengths on the exact-f32 kernels (the *VarLen calls; G = 1 RNN, 3 GRU, 4 LSTM): d_len = [B] lengths then [ceil(B / 64)]
 * the maxima of the 64-row batch tiles, device memory; T_max = the largest length.  A row follows its first d_len[b] steps and
 * then keeps its state (d_hT / d_cT, and d_out without sequences, = the state after d_len[b] steps); sequence outputs at
 * t >= d_len[b] are unspecified until nntk_shim_varlen_zero_pad clears them. */
int nntk_shim_rec_varlen(int G, const float *d_xw, const float *d_ut, const float *d_bh, const float *d_h0,
                         const float *d_c0, float *d_out, float *d_hT, float *d_cT, float *d_work, int B, int T, int H,
                         int return_sequences, const int *acts, const float *act_scales, const int *d_len, int T_max);
int nntk_shim_varlen_zero_pad(float *d_out, const int *d_len, int B, int T, int H);
int nntk_shim_gru(const float *d_xw, const float *d_ut, const float *d_bh,
                  const float *d_h0, float *d_out, float *d_hT, float *d_work,
                  int B, int T, int H, int return_sequences, const int acts[3], const float act_scales[3]);
int nntk_shim_lstm(const float *d_xw, const float *d_ut, const float *d_bh,
                   const float *d_h0, const float *d_c0, float *d_out, float *d_hT, float *d_cT,
                   float *d_work, int B, int T, int H, int return_sequences, const int acts[5], const float act_scales[5]);

/* Register-resident split-bf16 recurrent kernels with the input projection fused into the step (recurrent_rr.hip): standard
 * activations, H % 16 == 0, 64 <= H <= 512, in <= 128 (in <= 256 when H <= 256); f32 input: in % 8 == 0; frag3 input: any in.
 * d_x [B][T][in] f32 -- or NULL with d_xf3 = the same tensor in frag3 form (frag3.hip); d_img = weight images made by
 * nntk_shim_lstm_rr_pack from the per-gate U^T (d_ut) and the packed W^T (d_wp); d_bh NULL for the one-bias form.
 * d_hseq (nntk_shim_rr_hseq_floats) receives the layer output of every step in frag3 form -- it is the kernels' hand-off buffer;
 * d_out (f32) may be NULL when the caller consumes d_hseq.  d_work: nntk_shim_lstm_rr_work_floats.
 * nntk_shim_lstm_rr / nntk_shim_gru_rr return 1 when the shape / configuration is not taken (nothing launched). */
size_t nntk_shim_lstm_rr_image_floats(int H, int in);           /* 0: shape not taken (f32 input) */
size_t nntk_shim_rr_image_floats_xf(int H, int in);             /* 0: shape not taken (frag3 input) */
size_t nntk_shim_lstm_rr_work_floats(int B, int H);
size_t nntk_shim_rr_hseq_floats(int B, int T, int H);
int nntk_shim_lstm_rr_pack(const float *d_ut, const float *d_wp, float *d_img, int H, int in);
int nntk_shim_lstm_rr_pack_raw(const float *d_U /*[H][4H]*/, const float *d_W /*[in][4H]*/, float *d_img, int H, int in);
/* GRU on the same kernels (gru_rr_kernel): image from the four-slot matrices, d_b4 [4H]; see recurrent_rr.hip */
/* full-K family (recurrent_fk.hip: no split-K; H <= 256, frag3 input): own weight images d_img4 (NULL: family not used).  A shape this
 * family takes ALWAYS runs on it (the host packs an f32 input into frag3 form first), so a row's bits never depend on the call's size */
size_t nntk_shim_fk_image_floats(int H, int in);                /* 0: shape not taken (or option rec_fk = 0) */
int nntk_shim_fk_pack(const float *d_ut, const float *d_wp, float *d_img4, int H, int in);
int nntk_shim_fk_pack_raw(const float *d_U /*[H][4H]*/, const float *d_W /*[in][4H]*/, float *d_img4, int H, int in);
int nntk_shim_gru_rr(const float *d_x, const void *d_xf3, const float *d_img, const float *d_img4, const float *d_b4, const float *d_h0, float *d_out,
                     float *d_hseq, float *d_hT, float *d_work, int B, int T, int in, int H, int return_sequences, int x_tm, int out_tm);
int nntk_shim_gru_rr_train_forward(const float *d_x, const float *d_img, const float *d_b4, float *d_h, float *d_hU, float *d_Zg,
                                   float *d_hseq, float *d_work, int B, int T, int in, int H);
int nntk_shim_lstm_rr_train_forward(const float *d_x, const float *d_img, const float *d_bi, const float *d_bh,
                                    float *d_h, float *d_c, float *d_zifgo, float *d_hseq, float *d_work, int B, int T, int in, int H);
int nntk_shim_lstm_rr(const float *d_x, const void *d_xf3, const float *d_img, const float *d_img4, const float *d_bi, const float *d_bh,
                      const float *d_h0, const float *d_c0, float *d_out, float *d_out_h2 /* frag2h form of the sequence output, or NULL; needs d_out == NULL */,
                      float *d_hseq, float *d_hT, float *d_cT, float *d_work, int B, int T, int in, int H, int return_sequences);

/* per-row lengths on the same kernels (the *VarLen calls; cell 0 LSTM, 1 GRU with d_bi = d_b4 and d_bh NULL): d_len as nntk_shim_rec_varlen's;
 * row b runs its first d_len[b] steps and keeps its state after them; same family choice and bits as nntk_shim_lstm_rr / _gru_rr for every
 * step a row runs; 1 = not taken (nothing launched) */
int nntk_shim_rr_varlen(int cell, const float *d_x, const void *d_xf3, const float *d_img, const float *d_img4, const float *d_bi,
                        const float *d_bh, const float *d_h0, const float *d_c0, float *d_out, float *d_hseq, float *d_hT, float *d_cT,
                        float *d_work, const int *d_len, int B, int T, int in, int H, int return_sequences);

/* both directions of a bidirectional layer in one launch (the BD instantiations; the *BidirectionalApplyDevice calls): a virtual batch of
 * 2 Bpad rows, Bpad = 64 ceil(B / 64), forward in [0, Bpad) on d_img / d_img4 / d_bi / d_bh, backward in [Bpad, 2 Bpad) on the _b ones.
 * d_xf3: nntk_shim_frag3_pack_bd's tensor; d_len: [2 Bpad] virtual-row lengths (padding rows 0) then [2 Bpad / 64] the tiles' maxima;
 * d_hseq / d_work sized for 2 Bpad rows.  Forward row b writes d_out + b rowpitch + t ldo, backward row b d_out_b + b rowpitch +
 * (L_b - 1 - t) ldo, rowpitch = T ldo (sequences) or ldo; sequence outputs at t >= L_b are not written.  1 = not taken (nothing launched). */
int nntk_shim_rr_bd(int cell, const void *d_xf3, const float *d_img, const float *d_img4, const float *d_bi, const float *d_bh,
                    const float *d_img_b, const float *d_img4_b, const float *d_bi_b, const float *d_bh_b, float *d_out, float *d_out_b,
                    int ldo, float *d_hseq, float *d_work, const int *d_len, int B, int T, int in, int H, int return_sequences);
int nntk_shim_rr_bd_fits(int T, int in, int ldo);               /* 0: a 64-row tile of x or of the ldo-wide output rows is past 32-bit offsets (not taken) */

/* The HF instantiations of lstm_rr_kernel (H > 256): the h part of Z on two f16 images (three products per k step), the hand-off = the layer's
 * sequence output as a FRAG2H tensor (d_h2: nntk_shim_frag2h_floats(B, T, H) floats).  Zero initial state, x as a frag3 tensor.  Images:
 * nntk_shim_lstm_rr_pack_hf with uscale = a power of two with max |U| uscale <= 32768 and wscale = 32768 uscale; z_scale = 1 / wscale. */
int nntk_shim_lstm_rr_hf_ok(int H, int in);                     /* 256 < H <= 512, H % 16 == 0, in <= 256 (U has no LDS image: a 256-wide W fits), option rec_hf */
size_t nntk_shim_lstm_rr_hf_image_floats(int H, int in);
int nntk_shim_lstm_rr_pack_hf(const float *d_ut, const float *d_wp, float *d_img, int H, int in, float uscale, float wscale);
int nntk_shim_lstm_rr_hf(const void *d_xf3, const float *d_img, const float *d_bi, const float *d_bh, float *d_h2, float *d_work,
                         int B, int T, int in, int H, float z_scale);

/* ---- frag3 tensors (frag3.hip): a [B][T][C] f32 tensor as three bf16 images (x = hi + mid + lo exactly) in MFMA fragment order,
 * [T][2 ceil(B / 64)][ceil(C / 16)][3] blocks of 1 KB.  nntk_shim_dense_frag3: out [B][T][N] = act(h . W + b) with h in frag3 form and
 * d_wp the packed weights of a Dense layer; returns 1 when the shape is not taken. */
size_t nntk_shim_frag3_floats(int B, int T, int C);
int nntk_shim_frag3_pack(const float *d_x, void *d_frag, int B, int T, int C);
/* a bidirectional call's x operand: frag3 of 2 Bpad virtual rows, x then x reversed per row (d_len: [B] lengths, device), zeros elsewhere */
int nntk_shim_frag3_pack_bd(const float *d_x, const int *d_len, void *d_frag, int B, int T, int C);
int nntk_shim_frag3_unpack(const void *d_frag, float *d_x, int B, int T, int C);
/* FRAG2H (frag3.hip): the same tensor as two f16 images of x * 2^15 (|x| < 2), [T][2 ceil(B / 64)][ceil(C / 16)][2] blocks of 1 KB; the
 * dense GEMM on that form sums three products per k step.  d_wh2: the two f16 images of W * w_scale made by nntk_shim_split_f16x2 from the
 * packed f32 matrix ([N_p][K_p], nntk_shim_conv_pack_sizes; 2 * N_p * K_p halves), w_scale a power of two with max |W| w_scale <= 32768.
 * nntk_shim_dense_frag2h returns 1 when the shape / configuration is not taken (probe = 1: asks only, launches nothing). */
size_t nntk_shim_frag2h_floats(int B, int T, int C);
int nntk_shim_frag2h_pack(const float *d_x, void *d_frag, int B, int T, int C);
int nntk_shim_frag2h_unpack(const void *d_frag, float *d_x, int B, int T, int C);
int nntk_shim_split_f16x2(const float *d_src, void *d_dst, int rows, int ktot, float scale);
int nntk_shim_dense_frag2h(const void *d_frag, const void *d_wh2, float w_scale, const float *d_bias, int act_kind, float relu_a,
                           float *d_out, int B, int T, int K, int N, int probe);
int nntk_shim_dense_frag3(const void *d_frag, const float *d_wp, const float *d_bias, int act_kind, float relu_a,
                          float *d_out, int B, int T, int K, int N);

/* fused two-layer GRU (standard activations, zero initial state, both layers H units): layer 2's input projection and
 * recurrence run inside layer 1's persistent launch, one step behind.  d_wt2 = W2^T packed like U^T.  Returns 1 when
 * the shape is not taken (nothing launched). */
size_t nntk_shim_gru2_work_floats(int B, int H);
int nntk_shim_gru2(const float *d_xw1, const float *d_ut1, const float *d_bh1, const float *d_wt2,
                   const float *d_bi2, const float *d_ut2, const float *d_bh2, float *d_out, float *d_out1,
                   float *d_work, int B, int T, int H, int return_sequences);

/* streaming form: ONE sequence, T small; x [T, in] and out ([T, H] or [H]) may be pinned host memory (read / written by
 * the kernel directly, no copies); state h[cur] (c[cur]) -> h[(cur + T) & 1]; the last launch stores `seq` to *flag (a
 * pinned host word) once all outputs are visible to the host.  Bit-compatible with nntk_shim_gru / _lstm / _rnn. */
int nntk_shim_rec_stream(int G, int is_lstm, const float *x, const float *d_wp, const float *d_bi,
                         const float *d_ut, const float *d_bh, float *d_h0, float *d_h1, float *d_c0, float *d_c1,
                         int cur, float *out, int T, int in, int H, int return_sequences,
                         const int *acts, const float *scales, unsigned *d_done, unsigned *flag, unsigned seq);

/* ---- multi-GPU: one RCCL communicator per process, weight-block broadcast at start-up (dist.hip) ---- */
int nntk_shim_dist_unique_id(unsigned char *id128);
int nntk_shim_dist_init(const unsigned char *id128, int rank, int world);
int nntk_shim_dist_rank(void);
int nntk_shim_dist_world(void);
int nntk_shim_dist_broadcast_host(float *block, size_t n, int root);
int nntk_shim_add_into(float *d_dst, const float *d_src, long n);      /* dst += src, async */
int nntk_shim_dist_barrier(void);
int nntk_shim_dist_allreduce_device(float *d_block, size_t n);    /* in-place sum over the ranks, async on the stream */
int nntk_shim_dist_allreduce_host(float *block, size_t n);          /* staged, blocking */
int nntk_shim_dist_finalize(void);

/* ---- K1: framed STFT magnitude / PSD ---------------------------------------
 * d_in [B, input_size], d_window [window_size], d_out [B, nts, nfreq]
 * d_twiddle [nfft] complex interleaved: exp(-2*pi*i*m/nfft), evaluated in double on the host
 * mode 0: sqrt(re^2+im^2)/scale   mode 1: psd (spectrogram.c:41-47)
 */
int nntk_shim_spectrogram(const float *d_in, const float *d_window, const float *d_twiddle, float *d_out,
                          int B, int input_size, int nfft, int window_size, int step,
                          int nfreq, int nts, float fft_norm, int mode, float scale);

/* K1 with the mel projection (+ optional log(x + eps)) fused into its output stage; returns 1 when the configuration
 * is not taken by the fused kernel (nothing launched) */
int nntk_shim_spectrogram_mel(const float *d_in, const float *d_window, const float *d_twiddle, float *d_out,
                              int B, int input_size, int nfft, int window_size, int step,
                              int nfreq, int nts, float fft_norm, int mode, float scale,
                              const int *d_mel_tab, const float *d_mel_w, int n_mels, float eps, int do_log);

#ifdef __cplusplus
}
#endif
#endif
