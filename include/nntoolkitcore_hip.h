/*
 * nntoolkitcore_hip.h -- the drop-in C boundary of the MI355X-native
 * implementation of NNToolkitCore's time-series inference path
 *   Spectrogram -> Conv1d -> BatchNorm/Activation -> GRU/LSTM -> TimeDistributedDense.
 *
 * PART 1 re-declares the reference's own layer create/apply API for that path
 * (same symbol names, argument meaning, by-value struct layouts and 0 / -1 error
 * convention), so an application that includes the reference headers links
 * against libnntoolkitcore_hip.so unchanged.  Each block cites the reference
 * header it replaces.  The struct layouts are checked against the reference's
 * real headers by tests/test_abi_and_symbols.py (golden: tests/golden/ref_probe.json).
 *
 * PART 2 is ADDITIVE: batched [batch, time, feature] entry points, device-pointer
 * variants (so a stack chains on the GPU without host round trips), fused
 * Conv1d+BatchNorm+ReLU, weight re-sync, stream / device selection and an error
 * string for the void functions.  No HIP or torch type appears in any signature:
 * device buffers are plain `float *` holding device addresses, streams `void *`.
 *
 * Host code above this header stays C; the kernels are hand-written HIP for
 * gfx950 behind the thin shim in nntoolkitcore_amd/csrc/hip/nntk_shim.h.
 * There is NO CPU fallback: if the HIP runtime or a GPU is missing, Apply calls
 * fail (-1 / nntk_last_error()).
 */
#ifndef NNTOOLKITCORE_HIP_H
#define NNTOOLKITCORE_HIP_H

#include <stdbool.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ======================================================================= */
/* PART 1 -- reference API                                                   */
/* ======================================================================= */

/* ---- nntoolkitcore/layers/shared.h:12-34 ------------------------------- */
typedef struct { int mini_batch_size; } DefaultTrainingConfig;
typedef struct { int w; int b; int sum; } DefaultWeightsSize;
typedef struct { float *W; float *b; } DefaultWeights;

/* ---- nntoolkitcore/layers/activation.h:19-30 --------------------------- */
typedef void (*ActivationFunctionImpl)(void *, const float *, float *, int);
typedef void (*ActivationFunctionDerivative)(void *, const float *, const float *, float *, int);
typedef void (*ActivationImplementerDestroy)(void *);
typedef struct ActivationFunctionStruct *ActivationFunction;

/* Custom (host-callback) activations are accepted here for ABI compatibility
 * but cannot run on the device: a layer configured with one fails with -1. */
ActivationFunction ActivationFunctionCreate(int size, ActivationImplementerDestroy destroy_fn, void *implementer,
                                            ActivationFunctionImpl function, ActivationFunctionDerivative derivative,
                                            ActivationFunctionDerivative cached_derivative);
void ActivationFunctionDestroy(ActivationFunction filter);
/* host pointers; size fixed at create time (activation.c:23) */
void ActivationFunctionApply(ActivationFunction filter, const float *input, float *output);
/* activation.c:47-54: output = d_out * activation'(.) -- on the cached forward value `a` when the kind has a cached
 * derivative (sigmoid, tanh, softmax) and a != NULL, else on z.  Reference quirks kept: ReLU's derivative is
 * clamp(z, 0, 1) (activation_default.c:118-121), and inside ONE call every softmax vector reads d_out at the call's
 * base (activation_default.c:183).  The Device form takes device pointers; size <= 0 means the handle's size. */
void ActivationFunctionCalculateGradient(ActivationFunction filter, const float *z, const float *a, const float *d_out,
                                         float *output);
int  ActivationFunctionCalculateGradientDevice(ActivationFunction filter, const float *d_z, const float *d_a,
                                               const float *d_dout, float *d_output, int size);

/* ---- nntoolkitcore/layers/activation_default.h:19-27 ------------------- */
ActivationFunction ActivationFunctionCreateIdentity(int input_size);
ActivationFunction ActivationFunctionCreateSoftmax(int input_size, int vector_size);
ActivationFunction ActivationFunctionCreateSigmoid(int input_size);
ActivationFunction ActivationFunctionCreateReLU(int input_size, float a);
ActivationFunction ActivationFunctionCreateTanh(int input_size);

/* ---- nntoolkitcore/layers/conv_1d.h:22-55 ------------------------------ */
typedef struct {
    int input_feature_channels;
    int output_feature_channels;
    int kernel_size;
    int stride;
    int input_size;
    int output_size;
} Conv1dConfig;
typedef DefaultWeights ConvWeights;
typedef struct Conv1dStruct *Conv1d;

Conv1dConfig Conv1dConfigCreate(int input_feature_channels, int output_feature_channels, int kernel_size,
                                int stride, int inputSize);
Conv1d Conv1dCreateForInference(Conv1dConfig config);
ConvWeights *Conv1dGetWeights(Conv1d filter);            /* W [Cout][Cin][k] then b [Cout], one block */
int  Conv1dApplyInference(Conv1d filter, const float *input, float *output);   /* host, one sequence; -1 on a training handle */
void Conv1dDestroy(Conv1d filter);
/* training, first slice (layers/conv_1d.h:20, :43-51, shared.h:12-36): mini-batch forward that keeps its
 * input, and the gradient d_W / d_b (added to the block) / d_X (overwritten).  Deterministic, untuned. */
typedef DefaultTrainingConfig ConvTrainingConfig;
typedef struct { float *d_W; float *d_b; float *d_X; } DefaultGradient;      /* one zeroed block d_W | d_b | d_X */
typedef DefaultGradient ConvGradient;
Conv1d Conv1dCreateForTraining(Conv1dConfig config, ConvTrainingConfig training_config);
ConvGradient *Conv1dCreateGradient(Conv1dConfig config, ConvTrainingConfig training_config);
void ConvGradientDestroy(ConvGradient *gradient);
int  Conv1dApplyTrainingBatch(Conv1d filter, const float *input /*[mini_batch,T,Cin]*/, float *output);   /* -1 on an inference handle */
void Conv1dCalculateGradient(Conv1d filter, ConvGradient *gradient, const float *d_out /*[mini_batch,Tout,Cout]*/);
/* Additive device-pointer forms (tensors stay in HBM; enqueued on the calling thread's stream, but NOT asynchronous: each call
 * uploads the current weight block and waits for that copy, so it returns with the stream drained up to the upload; kernel-side
 * faults surface through nntk_hip_synchronize() / nntk_hip_device_status(); same kernels, same bits):
 * d_input must stay valid until the gradient call; d_grad_Wb = W [Cout][Cin][k] | b [Cout] is ADDED to, d_dX overwritten. */
int  Conv1dApplyTrainingBatchDevice(Conv1d filter, const float *d_input /*[mini_batch,T,Cin]*/, float *d_output);
int  Conv1dCalculateGradientDevice(Conv1d filter, float *d_grad_Wb, float *d_dX, const float *d_dout);

/* ---- nntoolkitcore/layers/batch_norm.h:19-66 --------------------------- */
typedef struct { float *gamma; float *beta; float *moving_mean; float *moving_variance; } BatchNormWeights;
typedef struct { int feature_channels; float epsilon; int count; } BatchNormConfig;
typedef struct BatchNormFilterStruct *BatchNorm;

BatchNormConfig BatchNormConfigCreate(int feature_channels, float epsilon, int count);
BatchNorm BatchNormCreateForInference(BatchNormConfig config);
BatchNormWeights *BatchNormGetWeights(BatchNorm filter);
int  BatchNormApplyInference(BatchNorm filter, const float *input, float *output);    /* -1 on a training-mode handle (batch_norm.c:167) */
void BatchNormDestroy(BatchNorm filter);
/* training (batch_norm.h:27-62, batch_norm.c:96-126, :191-386): forward over N = count * mini_batch rows with the batch's
 * own mean / biased variance, moving statistics updated in the weight block with `momentum`; the gradient OVERWRITES
 * d_beta, d_gamma [feature_channels] and d_x [N, feature_channels]. */
typedef struct { float momentum; int mini_batch_size; } BatchNormTrainingConfig;
typedef struct { float *d_gamma; float *d_beta; float *d_x; } BatchNormGradient;        /* block order: d_beta | d_gamma | d_x */
BatchNormTrainingConfig BatchNormTrainingConfigCreate(float momentum, int mini_batch_size);
BatchNorm BatchNormCreateForTraining(BatchNormConfig config, BatchNormTrainingConfig training_config);
BatchNormGradient *BatchNormGradientCreate(BatchNormConfig config, BatchNormTrainingConfig training_config);
void BatchNormGradientDestroy(BatchNormGradient *grad);
int  BatchNormApplyTrainingBatch(BatchNorm filter, const float *input, float *output);   /* -1 on an inference-mode handle */
void BatchNormCalculateGradient(BatchNorm filter, BatchNormGradient *gradient, float *d_out);
/* additive device-pointer forms of the two calls above (the host forms move the whole mini-batch over PCIe twice per call):
 * d_input must stay valid and unchanged until the matching gradient call; d_dbeta / d_dgamma [feature_channels] and d_dx are
 * overwritten like the host form's gradient block.  0 ok, -1 error. */
int  BatchNormApplyTrainingBatchDevice(BatchNorm filter, const float *d_input, float *d_output);
int  BatchNormCalculateGradientDevice(BatchNorm filter, float *d_dbeta, float *d_dgamma, float *d_dx, const float *d_dout);

/* ---- nntoolkitcore/layers/recurrent.h:17-56 ---------------------------- */
typedef struct { int w; int u; int b_i; int b_h; int sum; } RecurrentWeightsSize;
typedef struct { float *W; float *U; float *b_i; float *b_h; } RecurrentWeights;
typedef struct {
    int input_feature_channels;
    int output_feature_channels;
    bool return_sequences;
    int timesteps;
} RecurrentConfig;
RecurrentConfig RecurrentConfigCreate(int input_feature_channels, int output_feature_channels,
                                      bool return_sequences, int timesteps);

/* ---- nntoolkitcore/layers/gru.h:22-71 ---------------------------------- */
typedef RecurrentWeights GRUWeights;
typedef struct {
    ActivationFunction z_gate_activation;
    ActivationFunction h_gate_activation;
    ActivationFunction r_gate_activation;
} GRUActivations;
typedef struct { RecurrentConfig base; GRUActivations activations; } GRUConfig;
typedef struct GRUStruct *GRU;

GRUActivations GRUActivationsCreate(ActivationFunction z_gate_activation, ActivationFunction h_gate_activation,
                                    ActivationFunction r_gate_activation);
GRUActivations GRUActivationsCreateDefault(int size);
void GRUActivationsDestroy(GRUActivations activations);
GRUConfig GRUConfigCreate(int input_feature_channels, int output_feature_channels, bool return_sequences,
                          int timesteps, GRUActivations activations);
GRUWeights *GRUGetWeights(GRU filter);                   /* W [in,3H] | U [H,3H] | b_i [3H] | b_h [3H]; gates z,r,h */
/* training (gru.h:23-69, gru.c:232-512): forward over the mini-batch from a ZERO state per sequence keeping the gate
 * caches on the device, then back-propagation through time.  GRUCalculateGradient ADDS d_W, d_U, d_b_i, d_b_h onto the
 * block and overwrites d_X [mini_batch, timesteps, in]; d_out is [mini_batch, timesteps, out] if return_sequences else
 * [mini_batch, out].  Gate activations: built-in identity / sigmoid / tanh / ReLU. */
typedef struct { float *d_W; float *d_U; float *d_b_i; float *d_b_h; float *d_X; } RecurrentGradient;   /* one block, this order */
typedef DefaultTrainingConfig RecurrentTrainingConfig;
typedef RecurrentGradient GRUGradient;
typedef RecurrentTrainingConfig GRUTrainingConfig;
void RecurrentGradientDestroy(RecurrentGradient *gradient);
GRU  GRUCreateForTraining(GRUConfig config, GRUTrainingConfig training_config);
GRUGradient *GRUGradientCreate(GRUConfig config, GRUTrainingConfig training_config);
int  GRUApplyTrainingBatch(GRU filter, const float *input, float *output);      /* -1 on an inference-mode handle (gru.c:247) */
void GRUCalculateGradient(GRU filter, GRUGradient *gradients, float *d_out);
/* Additive device-pointer forms (tensors stay in HBM; enqueued on the calling thread's stream -- each call synchronises the stream
 * once for its weight upload, see Conv1dApplyTrainingBatchDevice; poll nntk_hip_device_status() for faults): d_input [B][T][in] must
 * stay valid until the gradient call; d_grad = W [in][3H] | U [H][3H] | b_i [3H] | b_h [3H] (the layout of the gradient block)
 * is ADDED to, d_dX [B][T][in] is overwritten.  Same kernels as the host-pointer forms: bit-identical results. */
int  GRUApplyTrainingBatchDevice(GRU filter, const float *d_input, float *d_output);
int  GRUCalculateGradientDevice(GRU filter, float *d_grad, float *d_dX, const float *d_dout);
GRU  GRUCreateForInference(GRUConfig config);
int  GRUApplyInference(GRU filter, const float *input, float *output);  /* host, one sequence, STATEFUL */
void GRUDestroy(GRU filter);

/* ---- nntoolkitcore/layers/lstm.h:20-75 --------------------------------- */
typedef RecurrentWeights LSTMWeights;
typedef struct {
    ActivationFunction candidate_gate_activation;
    ActivationFunction input_gate_activation;
    ActivationFunction forget_gate_activation;
    ActivationFunction output_gate_activation;
    ActivationFunction output_activation;
} LSTMActivations;
typedef struct { RecurrentConfig base; bool v2; LSTMActivations activations; } LSTMConfig;
typedef struct LSTMStruct *LSTM;

LSTMActivations LSTMActivationsCreate(ActivationFunction input_gate_activation,
                                      ActivationFunction forget_gate_activation,
                                      ActivationFunction candidate_gate_activation,
                                      ActivationFunction output_gate_activation,
                                      ActivationFunction output_activation);
LSTMActivations LSTMActivationsCreateDefault(int size);
void LSTMActivationsDestroy(LSTMActivations activations);
LSTMConfig LSTMConfigCreate(int input_feature_channels, int output_feature_channels, bool return_sequences,
                            int timesteps, bool v2, LSTMActivations activations);
LSTMWeights *LSTMGetWeights(LSTM filter);                /* W [in,4H] | U [H,4H] | b_i | b_h; gates i,f,g,o */
/* training (lstm.h:21-73, lstm.c:294-556): as for the GRU -- zero state per sequence, caches on the device, BPTT;
 * LSTMCalculateGradient ADDS d_W, d_U, d_b_i, d_b_h onto the block and overwrites d_X */
typedef RecurrentGradient LSTMGradient;
typedef RecurrentTrainingConfig LSTMTrainingConfig;
LSTM LSTMCreateForTraining(LSTMConfig config, LSTMTrainingConfig training_config);
LSTMGradient *LSTMGradientCreate(LSTMConfig config, LSTMTrainingConfig training_config);
int  LSTMApplyTrainingBatch(LSTM filter, const float *input, float *output);     /* -1 on an inference-mode handle (lstm.c:419) */
void LSTMCalculateGradient(LSTM filter, LSTMGradient *gradient, float *d_out);
/* device-pointer forms, as for the GRU (gate width 4H) */
int  LSTMApplyTrainingBatchDevice(LSTM filter, const float *d_input, float *d_output);
int  LSTMCalculateGradientDevice(LSTM filter, float *d_grad, float *d_dX, const float *d_dout);
LSTM LSTMCreateForInference(LSTMConfig config);
int  LSTMApplyInference(LSTM filter, const float *input, float *output); /* host, one sequence, STATEFUL */
void LSTMDestroy(LSTM filter);

/* ---- nntoolkitcore/layers/rnn.h:15-52 ------------ */
/* One-gate recurrent cell (rnn.c:144-166): h' = act((x W + b_i) + (h U [+ b_h if v2])).
 * W [in,out], U [out,out], b_i [out], b_h [out] in one block (rnn.c:36-46). */
typedef RecurrentWeights RNNWeights;
typedef struct { RecurrentConfig base; bool v2; ActivationFunction activation; } RNNConfig;
typedef struct RNNStruct *RNN;

RNNConfig RNNConfigCreate(int input_feature_channels, int output_feature_channels, bool return_sequences,
                          int timesteps, bool v2, ActivationFunction activation);
RNNWeights *RNNGetWeights(RNN filter);
/* training (rnn.h:16-48, rnn.c:184-221, :249-351): as for GRU / LSTM */
typedef RecurrentGradient RNNGradient;
typedef RecurrentTrainingConfig RNNTrainingConfig;
RNN  RNNCreateForTraining(RNNConfig config, RNNTrainingConfig training_config);
RNNGradient *RNNGradientCreate(RNNConfig config, RNNTrainingConfig training_config);
int  RNNApplyTrainingBatch(RNN filter, const float *input, float *output);
void RNNCalculateGradient(RNN filter, RNNGradient *gradients, float *d_out);
RNN  RNNCreateForInference(RNNConfig config);
/* host, one sequence, STATEFUL: T cells from the handle's h, output [T,out] or the last [out].  The
 * reference's loop (rnn.c:228-247) addresses its output at i * (i * out) and reloads h from the wrong row;
 * this is the layer its own batch forward pass (rnn.c:249-291) computes, not that indexing slip. */
int  RNNApplyInference(RNN filter, const float *input, float *output);
void RNNDestroy(RNN filter);

/* ---- nntoolkitcore/layers/bidirectional.h:15-46 (forward helpers) ------- */
/* host pointers, like the reference; the *_device forms below take device pointers */
void bd_reverse_input_batch(const float *input, float *output, RecurrentConfig config, int batch);    /* [B,T,in]  rows in reverse time order */
void bd_reverse_backward_batch(const float *input, float *output, RecurrentConfig config, int batch); /* [B,T,out] likewise */
int  bd_merge_concat_buffer_size(RecurrentConfig config);
/* output [B, rows, 2*out] = forward row | backward row (rows = timesteps if return_sequences else 1); buffer unused */
void bd_merge_concat(const float *forward_result, const float *backward_result, float *output,
                     RecurrentConfig config, int batch, float *buffer);
void bd_merge_sum(const float *forward_result, const float *backward_result, float *output,
                  RecurrentConfig config, int batch);
/* gradient helpers (bidirectional.h, bidirectional.c:58-74, :87-108); buffer unused */
void bd_merge_concat_gradient(const float *d_out, float *d_forward_out, float *d_backward_out, RecurrentConfig config,
                              int batch, float *buffer);
void bd_merge_sum_gradient(const float *d_out, float *d_forward_out, float *d_backward_out, RecurrentConfig config, int batch);
void bd_accumulate_d_x(const float *forward_dx, const float *backward_dx, float *output, RecurrentConfig config, int batch);

/* ---- nntoolkitcore/layers/dense.h:21-55 -------------------------------- */
typedef DefaultWeights DenseWeights;
typedef struct { int input_size; int output_size; ActivationFunction activation; } DenseConfig;
typedef struct DenseStruct *Dense;

DenseConfig DenseConfigCreate(int input_size, int output_size, ActivationFunction activation);
Dense DenseCreateForInference(DenseConfig config);
DenseWeights *DenseGetWeights(Dense filter);             /* W [in,out] row-major then b [out] */
int  DenseApplyInference(Dense filter, const float *input, float *output);     /* -1 on a training-mode handle (dense.c:136) */
void DenseDestroy(Dense filter);

/* training, second slice (dense.h:23-51, dense.c:85-119, :144-185): forward over the mini-batch keeping x, z, a on the
 * device; DenseCalculateGradient ADDS d_W, d_b onto the block in mini-batch order and overwrites d_X [mini_batch, in].
 * The activation must be built-in and sized to output_size (softmax: input_size * vector_size == output_size). */
typedef DefaultGradient DenseGradient;
typedef DefaultTrainingConfig DenseTrainingConfig;
Dense DenseCreateForTraining(DenseConfig config, DenseTrainingConfig training_config);
int  DenseApplyTrainingBatch(Dense filter, const float *input, float *output);  /* -1 on an inference-mode handle (dense.c:145) */
DenseGradient *DenseGradientCreate(DenseConfig config, DenseTrainingConfig training_config);
DenseGradient *DenseGradientCreateFromFilter(Dense dense);                      /* NULL on an inference-mode handle */
void DenseGradientDestroy(DenseGradient *gradient);
void DenseCalculateGradient(Dense filter, DenseGradient *gradient, float *d_out /*[mini_batch, out]*/);
/* additive device-pointer forms: d_input [mini_batch, in] must stay valid until the gradient call (it is the cached x);
 * d_grad_Wb = device [in * out + out] floats (d_W | d_b), ACCUMULATED onto like the host form; d_dX overwritten. */
int  DenseApplyTrainingBatchDevice(Dense filter, const float *d_input, float *d_output);
int  DenseCalculateGradientDevice(Dense filter, float *d_grad_Wb, float *d_dX, const float *d_dout);

/* ---- nntoolkitcore/layers/time_distributed_dense.h:19-45 --------------- */
typedef struct { DenseConfig dense; int ts; } TimeDistributedDenseConfig;
typedef struct TimeDistributedDenseStruct *TimeDistributedDense;

TimeDistributedDenseConfig TimeDistributedDenseConfigCreate(int ts, DenseConfig dense);
TimeDistributedDense TimeDistributedDenseCreateForInference(TimeDistributedDenseConfig config);
DenseWeights *TimeDistributedDenseGetWeights(TimeDistributedDense filter);
int  TimeDistributedDenseApplyInference(TimeDistributedDense filter, const float *input, float *output);
/* training (time_distributed_dense.h:24-43): a Dense trained on mini_batch * ts rows */
typedef DefaultTrainingConfig TimeDistributedDenseTrainingConfig;
TimeDistributedDense TimeDistributedDenseCreateForTraining(TimeDistributedDenseConfig config,
                                                           TimeDistributedDenseTrainingConfig training_config);
DenseGradient *TimeDistributedDenseGradientCreate(TimeDistributedDense filter);
int  TimeDistributedDenseApplyTrainingBatch(TimeDistributedDense filter, const float *input, float *output);
void TimeDistributedDenseCalculateGradient(TimeDistributedDense filter, DenseGradient *gradient, float *d_out);
int  TimeDistributedDenseApplyTrainingBatchDevice(TimeDistributedDense filter, const float *d_input, float *d_output);
int  TimeDistributedDenseCalculateGradientDevice(TimeDistributedDense filter, float *d_grad_Wb, float *d_dX, const float *d_dout);
void TimeDistributedDenseDestroy(TimeDistributedDense filter);

/* ---- nntoolkitcore/signal/dft.h:15-47 ---------------------------------- */
/* One complex DFT of any size on host split-complex buffers (un-normalised; forward = exp(-2 pi i k j / n)); the
 * reference runs kissfft (dft.c:34-47), here a direct transform with double accumulation on the device.  The
 * spectrogram kernels do not go through it. */
typedef struct DFTSetupStruct *DFTSetup;
typedef struct { int nfft; bool forward; bool complex; } DFTConfig;
typedef struct { float real; float imag; } ComplexFloat;
typedef struct { float *real_p; float *imag_p; } ComplexFloatSplit;
DFTConfig DFTConfigCreate(int nfft, bool forward, bool complex);
DFTSetup DFTSetupCreate(DFTConfig config);
void DFTPerform(DFTSetup setup, ComplexFloatSplit *input, ComplexFloatSplit *output);
void DFTSetupDestroy(DFTSetup setup);
void split_complex(const ComplexFloat *complex, ComplexFloatSplit *split, int size);
void join_complex_split(const ComplexFloatSplit *split, ComplexFloat *complex, int size);

/* ---- nntoolkitcore/signal/window.h:17-29 ------------------------------- */
typedef void (*window_fn)(float *, int);
void hamming_window(float *vector, int size);
void hann_window(float *vector, int size);
void ones(float *vector, int size);
void periodic_hamming_window(float *vector, int size);
void periodic_hann_window(float *vector, int size);
void blackman_window(float *vector, int size);

/* ---- nntoolkitcore/signal/spectrogram.h:20-44 -------------------------- */
typedef struct {
    int nfft;
    int window_size;
    int noverlap;
    int step;
    int input_size;
    int nfreq;
    int ntime_series;
    float fft_normalization_factor;
} SpectrogramConfig;
typedef struct SpectrogramStruct *Spectrogram;

SpectrogramConfig SpectrogramConfigCreate(int nfft, int window_size, int noverlap, int input_size,
                                          float fft_normalization_factor);
Spectrogram SpectrogramCreatePSD(SpectrogramConfig config, int fs);
Spectrogram SpectrogramCreateMagnitude(SpectrogramConfig config);
SpectrogramConfig SpectrogramGetConfig(Spectrogram filter);
void SpectrogramSetWindowFunc(Spectrogram filter, window_fn fn);
void SpectrogramSetScaleFactor(Spectrogram filter, float factor);
void SpectrogramApply(Spectrogram filter, const float *input, float *output);  /* host; errors via nntk_last_error() */
void SpectrogramDestroy(Spectrogram filter);

/* ---- nntoolkitcore/signal/mel_filterbank.h:14-41, log_mel_spectrogram.h:12-18 ----
 * (the first "next" row: 257 spectrogram bins -> n_mels features) */
typedef struct {
    int n_mels;
    int n_fft;
    int sample_rate;
    float lower_hz;
    float upper_hz;
} MelFilterBankConfig;
typedef struct MelFilterBankStruct *MelFilterBank;
typedef struct LogMelSpectrogramStruct *LogMelSpectrogram;

MelFilterBankConfig MelFilterBankConfigCreate(int n_mels, int n_fft, int sample_rate, float lower_hz, float upper_hz);
MelFilterBank MelFilterBankCreate(MelFilterBankConfig config);
void MelFilterBankApply(MelFilterBank filter_bank, const float *spectrogram, float *mel_spectrogram, int timesteps);
void MelFilterBankDestroy(MelFilterBank filter_bank);
LogMelSpectrogram LogMelSpectrogramCreate(Spectrogram spectrogram, MelFilterBankConfig mel_filter_bank_config);
void LogMelSpectrogramApply(LogMelSpectrogram filter, const float *input, float *output);   /* log(mel + 1.5849e-13) */
void LogMelSpectrogramDestroy(LogMelSpectrogram filter);

/* ======================================================================= */
/* PART 2 -- additive MI355X entry points                                    */
/* ======================================================================= */

/* ---- runtime ----------------------------------------------------------- */
int         nntk_hip_device_count(void);
int         nntk_hip_set_device(int device);          /* 0 ok, -1 error */
void        nntk_hip_set_stream(void *hip_stream);    /* all later launches OF THE CALLING THREAD use it; NULL = default stream */
void       *nntk_hip_get_stream(void);
int         nntk_hip_synchronize(void);               /* waits for the calling thread's current stream; -1 if a recurrent
                                                         launch faulted since the last check (see below) */
const char *nntk_last_error(void);                    /* "" when the last call succeeded */
const char *nntk_version(void);
const char *nntk_build_source_hash(void);        /* sha256/16 of the sources THIS binary was built from (nntoolkitcore_amd/_build.py) */
/* Threading (as the reference: distinct handles are independent, a handle is not re-entrant -- conv_1d.c:41,
 * gru.c:86, lstm.c:97): the current stream and the error string are per host thread; two threads may drive two
 * handles on two streams at the same time.  One handle is used by one thread and on one stream at a time
 * (nntk_hip_synchronize() before moving it to another stream).
 *
 * Tuning / diagnostics knobs by name; environment variables NNTK_<NAME> give the initial values (read once).
 *   "gemm_split_bf16" contraction of Conv1d / Dense / TimeDistributedDense / mel: auto = split-bf16 x 3 (every f32 operand as
 *                    three bf16 terms, six bf16 MFMA products accumulated in f32: f32 accuracy, not the k-ordered f32 chain),
 *                    0 = the exact-f32 chain everywhere, 1 = split also for the recurrent input projection.  EDGE VALUES under
 *                    auto: a non-finite input, or one above 3.39e38, gives NaN (where the chain gives +-inf) in exactly the outputs
 *                    whose window holds it; inputs below 1.18e-38 count as zero; a WEIGHT block holding such a value is detected
 *                    at upload and runs on the exact kernel.  INTEGRATION.md section 6 has the table, tests/test_gpu_edges.py pins it.
 *   "rec_rr"         GRU / LSTM batches: 0 = never the register-resident split-bf16 kernels (recurrent_rr.hip lstm_rr_kernel /
 *                    gru_rr_kernel; x W fused into the step, f32-accuracy contraction, not the exact-f32 chain), 1 = also below 32
 *                    sequences, auto = from 32.  Shapes: H 64..512 (multiple of 16), in <= 128, or in <= 256 when H <= 256; default
 *                    gate activations.  GRUStack2Apply* runs two such launches when both layers qualify ("rec_fused2" = 1: the fused
 *                    exact-f32 two-layer kernel instead)
 *   "train_bptt"     0 = GRU / LSTM gradients walk time with two launches per step instead of the persistent BPTT kernel
 *   "rec_persistent" 0 = per-timestep recurrent kernels only     "rec_pingpong" 0/1 = ping-pong halves off/on
 *   "rec_spin_us"    budget of the persistent kernel's spins     "gemm_tm_batch" 0/1
 *   "weights_check"  host-pointer calls look for in-place edits of the weight block before they launch:
 *                    1 (default) = the whole block is compared with the uploaded copy on every call, except the
 *                    single-sequence streaming GRU/LSTM/RNNApplyInference (T <= 32), which checks 257 probes of 64 B;
 *                    2 = the whole block everywhere, 0 = never (use <Layer>SyncWeights)
 * value "auto" restores the default.  0 ok, -1 unknown option. */
int         nntk_hip_set_option(const char *name, const char *value);
int         nntk_hip_get_option(const char *name, int *value);
/* The persistent GRU/LSTM kernel needs all its workgroups resident; if another process's kernel holds the CUs its
 * bounded spins give up and raise a sticky fault word.  Host-pointer recurrent calls notice it themselves and repeat
 * the call on the per-timestep kernels (same bits); device-pointer callers see it as -1 from nntk_hip_synchronize(),
 * or poll it without blocking here (0 healthy, 1 a completed recurrent launch of this thread has faulted).  After a
 * fault the process keeps to the per-timestep kernels. */
int         nntk_hip_device_status(void);
/* Name of the recurrent kernel the calling thread launched last ("" before the first): "lstm_rr_kernel<8,2>" (register-
 * resident split-bf16 LSTM with the fused input projection), "rec_persistent_kernel<4,LSTM>", "gru2_persistent_kernel<8>",
 * "rec_step_kernel<3,GRU>", ...  Diagnostics: which of the paths described under "rec_rr" / "rec_persistent" a call took. */
const char *nntk_hip_last_recurrent_kernel(void);
/* The same for the Conv1d / Dense / TimeDistributedDense GEMM kernels: "conv1d_mfma_bf16x3_kernel", "conv1d_mfma_bf16x3_kernel<frag3>"
 * (the frag3 epilogue of Conv1dBatchNormActivationApplyDeviceFrag3), "conv1d_flatk_bf16x3_kernel", "conv1d_mfma_kernel" (exact f32),
 * "conv1d_valu_kernel". */
const char *nntk_hip_last_conv_kernel(void);
/* Optional HIP-event spans around the recurrent kernel launches (name "rec_step"): enable,
 * run, then read the summed milliseconds, the number of kernel launches and the timesteps they
 * covered (a persistent launch covers all T of a sequence).  Reading clears the spans. */
void        nntk_hip_profile_enable(int on);
int         nntk_hip_profile_get(const char *name, double *total_ms, long *launches, long *timesteps);

/* raw device memory helpers for C callers that chain layers on the GPU */
float *nntk_device_alloc(size_t n_floats);
void   nntk_device_free(float *ptr);
int    nntk_device_upload(float *dst_device, const float *src_host, size_t n_floats);
int    nntk_device_download(float *dst_host, const float *src_device, size_t n_floats);

/* Re-upload the host weight block after the caller edited it.  The host-pointer
 * Apply* functions of Part 1 detect edits themselves (they compare the block with
 * the last uploaded copy); the *Device functions below do not. */
int Conv1dSyncWeights(Conv1d filter);
int BatchNormSyncWeights(BatchNorm filter);
int GRUSyncWeights(GRU filter);
int LSTMSyncWeights(LSTM filter);
int RNNSyncWeights(RNN filter);
int DenseSyncWeights(Dense filter);
int TimeDistributedDenseSyncWeights(TimeDistributedDense filter);
/* The weight block from DEVICE memory: d_block holds the <Layer>GetWeights() block, same order and size (Conv1d / Dense /
 * TimeDistributedDense: W | b; BatchNorm: gamma | beta | moving_mean | moving_variance; GRU / LSTM / RNN: W | U | b_i | b_h).  It is
 * copied into the handle's host block in stream order, the call waits for that copy and then does what <Layer>SyncWeights does: afterwards
 * <Layer>GetWeights() shows the new values and every call on the handle -- host and device forms, inference and training -- uses them.
 * The sibling of <Layer>BroadcastWeights (same host block, filled from RCCL); the step after nntk_optimizer_step_device (below).  The copy
 * goes through the pinned host block on purpose: it is the library's master copy, from which every layer repacks. */
int Conv1dLoadWeightsDevice(Conv1d filter, const float *d_block);
int BatchNormLoadWeightsDevice(BatchNorm filter, const float *d_block);
int GRULoadWeightsDevice(GRU filter, const float *d_block);
int LSTMLoadWeightsDevice(LSTM filter, const float *d_block);
int RNNLoadWeightsDevice(RNN filter, const float *d_block);
int DenseLoadWeightsDevice(Dense filter, const float *d_block);
int TimeDistributedDenseLoadWeightsDevice(TimeDistributedDense filter, const float *d_block);

/* ---- multi-GPU: one process per GPU, utterances sharded, NO collective on the data path --------------------
 * (every utterance is independent: BatchNorm uses stored statistics, batch_norm.c:178-181; every sequence owns
 * its recurrent state).  The only communication is one RCCL broadcast of each layer's weight block from the root
 * at start-up, over xGMI.  RCCL is dlopen()ed at the first nntk_dist_* call; a single-GPU caller never loads it.
 *   rank 0:      nntk_dist_get_unique_id(id)  -> carry the 128 bytes to the other ranks (file, env, socket ...)
 *   every rank:  nntk_hip_set_device(local); nntk_dist_init(id, rank, world);
 *                <Layer>BroadcastWeights(handle, 0) for each layer;  nntk_dist_shard_range(B, world, rank, &lo, &hi);
 *                run utterances [lo, hi) with the *ApplyDevice / *ApplyInferenceBatch calls;  nntk_dist_finalize().
 * All return 0 / -1 (nntk_last_error()).  Without a communicator the broadcasts are no-ops. */
#define NNTK_DIST_ID_BYTES 128
int  nntk_dist_get_unique_id(unsigned char id[NNTK_DIST_ID_BYTES]);
int  nntk_dist_init(const unsigned char id[NNTK_DIST_ID_BYTES], int rank, int world_size);   /* collective */
int  nntk_dist_rank(void);
int  nntk_dist_world_size(void);
int  nntk_dist_broadcast(float *host_block, size_t n_floats, int root);      /* any host block, in place, blocking */
int  nntk_dist_barrier(void);
/* Data-parallel TRAINING: in-place SUM of a gradient block over the ranks (RCCL all-reduce over xGMI).  nntk_dist_allreduce: a host
 * block, staged, blocking.  nntk_dist_allreduce_device: a block in HBM (what <Layer>CalculateGradientDevice accumulates into),
 * asynchronous on the calling thread's stream.  Both are no-ops without a communicator (one rank). */
int  nntk_dist_allreduce(float *host_block, size_t n_floats);
int  nntk_dist_allreduce_device(float *d_block, size_t n_floats);
int  nntk_dist_finalize(void);
void nntk_dist_shard_range(int n_utterances, int world_size, int rank, int *lo, int *hi);
int Conv1dBroadcastWeights(Conv1d filter, int root);
int BatchNormBroadcastWeights(BatchNorm filter, int root);
int GRUBroadcastWeights(GRU filter, int root);
int LSTMBroadcastWeights(LSTM filter, int root);
int RNNBroadcastWeights(RNN filter, int root);
int DenseBroadcastWeights(Dense filter, int root);
int TimeDistributedDenseBroadcastWeights(TimeDistributedDense filter, int root);

/* ---- batched host-pointer forms: semantics of the reference's
 *      *ApplyTrainingBatch forward pass (conv_1d.c:167, gru.c:246, lstm.c:426,
 *      dense.c:144) without the training caches: input [batch, T, in],
 *      zero initial recurrent state per sequence. --------------------------- */
int Conv1dApplyInferenceBatch(Conv1d filter, const float *input, float *output, int batch);
int GRUApplyInferenceBatch(GRU filter, const float *input, float *output, int batch);
int LSTMApplyInferenceBatch(LSTM filter, const float *input, float *output, int batch);
int RNNApplyInferenceBatch(RNN filter, const float *input, float *output, int batch);   /* rnn.c:249-291 forward */
int TimeDistributedDenseApplyInferenceBatch(TimeDistributedDense filter, const float *input, float *output, int batch);
int SpectrogramApplyBatch(Spectrogram filter, const float *input, float *output, int batch);
int LogMelSpectrogramApplyBatch(LogMelSpectrogram filter, const float *input, float *output, int batch);

/* ---- device-pointer forms (all pointers are device addresses; asynchronous
 *      on the current stream; 0 ok, -1 error) ------------------------------ */
int SpectrogramApplyDevice(Spectrogram filter, const float *d_input /*[batch,input_size]*/,
                           float *d_output /*[batch,ntime_series,nfreq]*/, int batch);
int MelFilterBankApplyDevice(MelFilterBank filter_bank, const float *d_spectrogram /*[rows,nbins]*/,
                             float *d_mel /*[rows,n_mels]*/, int rows);
int LogMelSpectrogramApplyDevice(LogMelSpectrogram filter, const float *d_input /*[batch,input_size]*/,
                                 float *d_output /*[batch,ntime_series,n_mels]*/, int batch);
int Conv1dApplyDevice(Conv1d filter, const float *d_input /*[batch,T,Cin]*/,
                      float *d_output /*[batch,Tout,Cout]*/, int batch);
/* fused Conv1d -> BatchNorm(inference) -> activation in one kernel; bn and/or act may be NULL */
int Conv1dBatchNormActivationApplyDevice(Conv1d filter, BatchNorm bn, ActivationFunction act,
                                         const float *d_input, float *d_output, int batch);
int BatchNormApplyDevice(BatchNorm filter, const float *d_input, float *d_output, int rows);
int ActivationFunctionApplyDevice(ActivationFunction filter, const float *d_input, float *d_output, int size);
int GRUApplyDevice(GRU filter, const float *d_input /*[batch,T,in]*/, float *d_output, int batch);
int LSTMApplyDevice(LSTM filter, const float *d_input /*[batch,T,in]*/, float *d_output, int batch);
/* Two stacked GRU layers (layer 1 returns sequences and feeds layer 2) in ONE persistent launch: layer 2 runs one step
 * behind layer 1 inside the same kernel, so its input projection and the inter-layer [batch,T,H] tensor never reach HBM.
 * Results = GRUApplyDevice(l1) then GRUApplyDevice(l2) from zero state (gru.c:246-293 forward semantics), within the
 * layer tolerance; shapes or activations the fused kernel does not take run exactly those two calls. */
int GRUStack2ApplyDevice(GRU layer1, GRU layer2, const float *d_input /*[batch,T,in]*/, float *d_output, int batch);
int GRUStack2ApplyInferenceBatch(GRU layer1, GRU layer2, const float *input, float *output, int batch);
int RNNApplyDevice(RNN filter, const float *d_input /*[batch,T,in]*/, float *d_output, int batch);
int bd_reverse_input_batch_device(const float *d_input, float *d_output, RecurrentConfig config, int batch);
int bd_reverse_backward_batch_device(const float *d_input, float *d_output, RecurrentConfig config, int batch);
int bd_merge_concat_device(const float *d_forward, const float *d_backward, float *d_output, RecurrentConfig config, int batch);
int bd_merge_sum_device(const float *d_forward, const float *d_backward, float *d_output, RecurrentConfig config, int batch);
/* ---- ragged batches and carried state (INTEGRATION.md "Ragged batches and chunked streaming") -----------------------------------
 * T = the layer's timesteps, also the row stride of the [batch][T][in] input and the [batch][T][H] output.  Row b with L = lengths[b]
 * (0 <= L <= T) runs its first L steps from h0[b] (c0[b]): return_sequences: out[b][t] = h_t for t < L, zeros for t >= L (as PyTorch's
 * pad_packed_sequence); otherwise out[b] = h_L.  hT[b] = h_L, cT[b] = c_L (L = 0: h0[b] / c0[b], or zeros without them).  A row's result
 * equals the stateful single-sequence recurrence (gru.c:189-204, lstm.c:241-268, rnn.c:144-166) on x[b][:L] from that state.
 * lengths: HOST memory, [batch], or NULL for all T; checked before anything is enqueued (-1 and nntk_last_error() for a length outside
 * [0, T] or batch < 0) and copied in stream order, so the array may be reused when the call returns.  Every state pointer may be NULL
 * (zeros in, nothing out).  f32 only; device pointers and asynchrony as the *ApplyDevice calls.  Runs on the kernel family the layer's
 * *ApplyDevice call takes (*KernelPlan: lstm_rr_kernel / gru_rr_kernel, *_fk_kernel, rec_persistent_kernel or the per-timestep kernels),
 * with the same bits for every step a row runs.  Each 64-row batch tile runs to its own longest row. */
int GRUApplyDeviceVarLen(GRU filter, const float *d_input /*[batch,T,in]*/, float *d_output, int batch,
                         const int *lengths /*host [batch] or NULL*/, const float *d_h0 /*[batch,H] or NULL*/, float *d_hT /*[batch,H] or NULL*/);
int RNNApplyDeviceVarLen(RNN filter, const float *d_input, float *d_output, int batch, const int *lengths,
                         const float *d_h0, float *d_hT);
int LSTMApplyDeviceVarLen(LSTM filter, const float *d_input, float *d_output, int batch, const int *lengths,
                          const float *d_h0, const float *d_c0, float *d_hT, float *d_cT);
/* the same on host memory (upload, device call, download) */
int GRUApplyInferenceBatchVarLen(GRU filter, const float *input, float *output, int batch, const int *lengths,
                                 const float *h0, float *hT);
int RNNApplyInferenceBatchVarLen(RNN filter, const float *input, float *output, int batch, const int *lengths,
                                 const float *h0, float *hT);
int LSTMApplyInferenceBatchVarLen(LSTM filter, const float *input, float *output, int batch, const int *lengths,
                                  const float *h0, const float *c0, float *hT, float *cT);
/* ---- training on ragged batches with carried state (INTEGRATION.md "Training on ragged batches and long streams") -------------------
 * The training counterpart of the calls above, on a *CreateForTraining handle: B = its mini_batch_size, T = its timesteps (also the row
 * stride), H its hidden size.  lengths: HOST memory [B] or NULL (every row T), checked before anything is enqueued (-1 and
 * nntk_last_error() for a length outside [0, T]; nothing written) and copied in stream order.  Every state pointer may be NULL (zeros in /
 * nothing out).
 * Forward: row b runs steps 0 .. L-1 (L = lengths[b]) from h0[b] (c0[b]).  return_sequences: out[b][t] = h_t for t < L, exact zeros for
 * t >= L; otherwise out[b] = h_L.  hT[b] = h_L, cT[b] = c_L (L = 0: h0[b] / c0[b], zeros without them).  x[b][t >= L] influences nothing
 * (it may hold NaN).  The handle remembers the lengths and h0 / c0 for the gradient call: the state tensors must stay valid until then,
 * like d_input.
 * Gradient: d_dout[b][t >= L] is ignored (it may hold NaN); without return_sequences d_dout[b] enters at step L-1.  d_dhT[b] / d_dcT[b]
 * is the gradient arriving at h_L / c_L from outside (the next chunk's d_dh0 / d_dc0), added where the recurrence's own carry would be.
 * d_dh0[b] / d_dc0[b] is the gradient with respect to h0[b] / c0[b] (the zero state when none was given; L = 0: d_dhT[b] / d_dcT[b] passed
 * through, or zeros -- plus d_dout[b] in d_dh0[b] without return_sequences, where out[b] = h_L is h0[b] itself).  d_dX[b][t >= L] is exact zeros.  d_grad (W | U | b_i | b_h) is ADDED to; only steps t < L contribute, and step 0
 * contributes its h0 / c0 terms.
 * With lengths == NULL and every state pointer NULL the calls run the kernels of *ApplyTrainingBatchDevice / *CalculateGradientDevice and
 * return their bits.  Ragged and carried-state calls take the routes of the fixed-length ones: the forward pass runs the register-resident
 * kernel (its TRAIN instantiation with per-row lengths: each 64-row batch tile runs to its own longest row) wherever the fixed-length call
 * does (except a GRU with H <= 256 and in <= 64), the gradient the persistent BPTT kernel wherever the fixed-length call does (a row is idle until its own last step, every 16-row
 * batch tile starts at its own longest row); otherwise the per-timestep kernels.  nntk_hip_last_recurrent_kernel() names the kernel the last
 * call ran. */
int GRUApplyTrainingBatchDeviceVarLen(GRU filter, const float *d_input /*[B,T,in]*/, float *d_output, const int *lengths /*host [B] or NULL*/,
                                      const float *d_h0 /*[B,H] or NULL*/, float *d_hT /*[B,H] or NULL*/);
int RNNApplyTrainingBatchDeviceVarLen(RNN filter, const float *d_input, float *d_output, const int *lengths, const float *d_h0, float *d_hT);
int LSTMApplyTrainingBatchDeviceVarLen(LSTM filter, const float *d_input, float *d_output, const int *lengths,
                                       const float *d_h0, const float *d_c0, float *d_hT, float *d_cT);
int GRUCalculateGradientDeviceVarLen(GRU filter, float *d_grad, float *d_dX /*[B,T,in]*/, const float *d_dout,
                                     const float *d_dhT /*[B,H] or NULL*/, float *d_dh0 /*[B,H] or NULL*/);
int RNNCalculateGradientDeviceVarLen(RNN filter, float *d_grad, float *d_dX, const float *d_dout, const float *d_dhT, float *d_dh0);
int LSTMCalculateGradientDeviceVarLen(LSTM filter, float *d_grad, float *d_dX, const float *d_dout,
                                      const float *d_dhT, const float *d_dcT, float *d_dh0, float *d_dc0);
/* the same on host memory (upload, device call, download; the gradient block is accumulated as *CalculateGradient does).  int, not void:
 * -1 and nntk_last_error() on an error */
int GRUApplyTrainingBatchVarLen(GRU filter, const float *input, float *output, const int *lengths, const float *h0, float *hT);
int RNNApplyTrainingBatchVarLen(RNN filter, const float *input, float *output, const int *lengths, const float *h0, float *hT);
int LSTMApplyTrainingBatchVarLen(LSTM filter, const float *input, float *output, const int *lengths,
                                 const float *h0, const float *c0, float *hT, float *cT);
int GRUCalculateGradientVarLen(GRU filter, GRUGradient *gradient, const float *d_out, const float *d_hT_grad, float *d_h0_grad);
int RNNCalculateGradientVarLen(RNN filter, RNNGradient *gradient, const float *d_out, const float *d_hT_grad, float *d_h0_grad);
int LSTMCalculateGradientVarLen(LSTM filter, LSTMGradient *gradient, const float *d_out, const float *d_hT_grad, const float *d_cT_grad,
                                float *d_h0_grad, float *d_c0_grad);
/* the RNN's device-pointer training calls, in the shape of the GRU's (d_grad = W [in][H] | U [H][H] | b_i [H] | b_h [H], ADDED to) */
int RNNApplyTrainingBatchDevice(RNN filter, const float *d_input, float *d_output);
int RNNCalculateGradientDevice(RNN filter, float *d_grad, float *d_dX, const float *d_dout);
/* bidirectional helpers for ragged rows: out[b][t] = in[b][lengths[b] - 1 - t] for t < lengths[b], zeros after (lengths: host) */
int bd_reverse_input_batch_varlen_device(const float *d_input, float *d_output, RecurrentConfig config, int batch, const int *lengths);
int bd_reverse_backward_batch_varlen_device(const float *d_input, float *d_output, RecurrentConfig config, int batch, const int *lengths);
/* ---- streaming a whole stack (INTEGRATION.md "Streaming a whole stack") ------------------------------------------------------
 * Audio arrives in chunks, per row (user) and per call; every stage keeps what the next chunk needs in a device STATE buffer the caller
 * owns, updated in place (the call reads the old state before it writes the new one, in stream order: one buffer per stage).  The
 * handle's input_size is the most new samples (spectrogram) or new rows (conv) a row may bring per call, and the row stride of the chunk
 * input.  Counts are HOST arrays [batch], checked before anything is enqueued and copied in stream order; on -1 (nntk_last_error()) nothing
 * is enqueued and nothing is written, host arrays included.  final[b] != 0 (final may be NULL: none) ends row b's stream: its last frames
 * are released and its state emptied, so the slot can start a new stream.  n_new[b] = 0 leaves row b's state unchanged (a final still
 * releases).  out[b][j] is frame / output g_b + j of the one-shot call (SpectrogramApplyDevice, LogMelSpectrogramApplyDevice,
 * Conv1dBatchNormActivationApplyDevice) on the row's whole stream, g_b = what the row emitted before, BIT FOR BIT; rows j >= frames[b]
 * (n_out[b]) are zeros.
 * Spectrogram: row b's virtual sequence is tail ++ new, m = tail_len + n_new samples, F = m >= window_size ? (m - noverlap) / step : 0
 * complete frames; E = final ? F : F & ~1 are emitted (K1 transforms frames in pairs: an odd frame waits for its partner, one hop of
 * delay, 10 ms at step 160) and next_tail_len = final ? 0 : m - E * step <= window_size + step - 1.
 * Conv1d: m = hist_len + n_new rows, O = m >= k ? (m - k) / s + 1 : 0 outputs, next_hist_len = final ? 0 : m - O * s <= k - 1; requires
 * stride <= kernel_size.  The *_plan / *_sizes functions are that arithmetic (pure host code, no GPU): 0 ok, -1 invalid arguments. */
int nntk_spectrogram_stream_plan(SpectrogramConfig cfg, int tail_len, int n_new, int final, int *frames, int *next_tail_len);
int nntk_spectrogram_stream_sizes(SpectrogramConfig cfg, int *tail_floats /* window_size + step - 1 */,
                                  int *max_frames /* ceil(input_size / step) + 1: the output row stride */);
int nntk_conv1d_stream_plan(Conv1dConfig cfg, int hist_len, int n_new, int final, int *n_out, int *next_hist_len);
int nntk_conv1d_stream_sizes(Conv1dConfig cfg, int *hist_rows /* k - 1 */, int *max_outputs /* ceil(input_size / stride) */);
int SpectrogramApplyDeviceStream(Spectrogram filter, const float *d_input /*[B][input_size]*/, const int *n_new /*host [B]*/,
                                 const int *final /*host [B] or NULL*/, float *d_tail /*[B][tail_floats], in place*/,
                                 int *tail_len /*host [B], in/out*/, float *d_output /*[B][max_frames][nfreq]*/, int *frames /*host [B], out*/,
                                 int batch);
int LogMelSpectrogramApplyDeviceStream(LogMelSpectrogram filter, const float *d_input, const int *n_new, const int *final, float *d_tail,
                                       int *tail_len, float *d_output /*[B][max_frames][n_mels]*/, int *frames, int batch);
int Conv1dBatchNormActivationApplyDeviceStream(Conv1d filter, BatchNorm bn /*or NULL*/, ActivationFunction act /*or NULL*/,
                                               const float *d_input /*[B][input_size][Cin]*/, const int *n_new, const int *final,
                                               float *d_hist /*[B][k-1][Cin], in place*/, int *hist_len /*host [B], in/out*/,
                                               float *d_output /*[B][max_outputs][Cout]*/, int *n_out /*host [B], out*/, int batch);
/* rows t >= lengths[b] of the [B][ts][out] output are zeros, rows t < lengths[b] the bits of TimeDistributedDenseApplyDevice (lengths:
 * host [B] or NULL = all ts, checked and copied like the *VarLen calls' lengths) */
int TimeDistributedDenseApplyDeviceVarLen(TimeDistributedDense filter, const float *d_input, float *d_output, int batch,
                                          const int *lengths);
/* ---- bidirectional layers in one call (INTEGRATION.md "A bidirectional layer") ------------------------------------------------
 * forward / backward: two layers of one kind with equal input size, hidden size H, timesteps T and return_sequences (the same handle may
 * be passed twice).  d_input [batch][T][in]; lengths: HOST memory, [batch], or NULL for all T (copied in stream order, as the *VarLen calls).
 * The result is, bit for bit, that of the composed recipe
 *     bd_reverse_input_batch[_varlen]_device(x -> xr); *ApplyDevice[VarLen](forward, x -> of); *ApplyDevice[VarLen](backward, xr -> obr);
 *     return_sequences: bd_reverse_backward_batch[_varlen]_device(obr -> ob), else ob = obr;  bd_merge_{concat,sum}_device(of, ob)
 * i.e. both directions from zero state; with return_sequences out[b][t] is merge(h_fwd[t], h_bwd[L - 1 - t]) for t < L = lengths[b] and
 * zeros for t >= L; without, out[b] = merge(forward state after L steps, backward state after its L steps over the reversed prefix).
 * NNTK_BD_MERGE_CONCAT: output [batch][T][2H] (or [batch][2H]), forward in columns [0, H), backward in [H, 2H); NNTK_BD_MERGE_SUM: [batch][T][H]
 * (or [batch][H]), forward + backward.  Where both directions take the register-resident / full-K kernels (*KernelPlan) they run in ONE
 * launch over a virtual batch of both directions (nntk_hip_last_recurrent_kernel() then names the kernel with a ",bd" mark); elsewhere the
 * call runs the recipe itself.  -1 and nntk_last_error() -- before anything is enqueued, the output untouched -- when the two layers differ
 * in in / H / T / return_sequences, a length is outside [0, T], merge is not one of the two constants, batch < 0, or (device form) the
 * output overlaps the input.  Not stateful; f32; device pointers and asynchrony as the *ApplyDevice calls. */
#define NNTK_BD_MERGE_CONCAT 0
#define NNTK_BD_MERGE_SUM 1
int GRUBidirectionalApplyDevice(GRU forward, GRU backward, const float *d_input /*[B,T,in]*/, float *d_output, int batch,
                                const int *lengths /*host [B] or NULL*/, int merge);
int LSTMBidirectionalApplyDevice(LSTM forward, LSTM backward, const float *d_input, float *d_output, int batch, const int *lengths, int merge);
int RNNBidirectionalApplyDevice(RNN forward, RNN backward, const float *d_input, float *d_output, int batch, const int *lengths, int merge);
/* the same on host memory (upload, device call, download) */
int GRUBidirectionalApplyInferenceBatch(GRU forward, GRU backward, const float *input, float *output, int batch, const int *lengths, int merge);
int LSTMBidirectionalApplyInferenceBatch(LSTM forward, LSTM backward, const float *input, float *output, int batch, const int *lengths, int merge);
int RNNBidirectionalApplyInferenceBatch(RNN forward, RNN backward, const float *input, float *output, int batch, const int *lengths, int merge);
/* ---- training a bidirectional layer (INTEGRATION.md "Training a bidirectional layer") -------------------------------------------
 * Device forms of the reference's gradient helpers (bidirectional.c:58-108), thin wrappers over one-pass kernels.  The three fixed-length
 * forms return the bits of bd_merge_concat_gradient / bd_merge_sum_gradient / bd_accumulate_d_x; as there, d_backward is NOT reversed
 * (bd_accumulate_d_x reverses the backward direction's d_X within T).  The varlen forms are what a ragged bidirectional layer needs
 * (lengths: HOST memory [batch] or NULL = every row T, checked and copied like bd_reverse_*_varlen_device's; L = lengths[b]):
 *   bd_merge_gradient_varlen_device: d_forward[b][t] = d_dout[b][t][forward part], d_backward_reversed[b][t] = d_dout[b][L-1-t][backward part]
 *     for t < L, both exact zeros for t >= L whatever d_dout holds there; parts: columns [0, H) / [H, 2H) (NNTK_BD_MERGE_CONCAT) or the whole
 *     row twice (NNTK_BD_MERGE_SUM); without return_sequences the plain split / copy of [batch][2H] / [batch][H].
 *   bd_accumulate_d_x_varlen_device: d_output[b][t] = d_forward_dx[b][t] + d_backward_dx[b][L-1-t] for t < L (one f32 add), zeros for t >= L.
 * -1 and nntk_last_error() for batch < 0, a NULL pointer, a length outside [0, T], an unknown merge, or tensors that overlap (d_output may
 * be d_forward_dx). */
int bd_merge_concat_gradient_device(const float *d_dout, float *d_forward, float *d_backward, RecurrentConfig config, int batch);
int bd_merge_sum_gradient_device(const float *d_dout, float *d_forward, float *d_backward, RecurrentConfig config, int batch);
int bd_accumulate_d_x_device(const float *d_forward_dx, const float *d_backward_dx, float *d_output, RecurrentConfig config, int batch);
int bd_merge_gradient_varlen_device(const float *d_dout, float *d_forward, float *d_backward_reversed, RecurrentConfig config, int batch,
                                    const int *lengths, int merge);
int bd_accumulate_d_x_varlen_device(const float *d_forward_dx, const float *d_backward_dx, float *d_output, RecurrentConfig config, int batch,
                                    const int *lengths);
/* The layer in one call per pass.  forward / backward: two DIFFERENT *CreateForTraining handles of one kind with equal input size, H, T,
 * return_sequences and mini_batch_size (B; T is also the row stride); one handle holds one set of caches, so the same handle twice is an
 * error.  Both directions start from zero state (a bidirectional layer cannot be chunked in time: no h0 / hT).  lengths: HOST [B] or NULL.
 * Forward: bit for bit the recipe
 *     bd_reverse_input_batch[_varlen]_device(x -> xr); *ApplyTrainingBatchDeviceVarLen(forward, x -> of); *ApplyTrainingBatchDeviceVarLen(backward,
 *     xr -> obr), both with these lengths and no states; out[b][t] = merge(of[b][t], obr[b][L-1-t])
 * in the output layout of *BidirectionalApplyDevice: rows t >= L exact zeros, x[b][t >= L] influences nothing (it may hold NaN); without
 * return_sequences out[b] = merge(of[b], obr[b]).  Each direction takes the kernel its unidirectional call takes;
 * nntk_hip_last_recurrent_kernel() names the backward direction's (it ran last).  xr lives in the backward handle until its next forward call;
 * d_input must stay valid until the gradient call.  The forward handle remembers merge and the lengths.
 * Gradient: bit for bit bd_merge_gradient_varlen_device(d_dout -> d_of, d_obr), *CalculateGradientDeviceVarLen(forward, d_grad_forward, dXf,
 * d_of) and (backward, d_grad_backward, dXbr, d_obr) without state gradients, bd_accumulate_d_x_varlen_device(dXf, dXbr -> d_dX).
 * d_grad_* (W | U | b_i | b_h of each direction) are ADDED to, d_dX [B][T][in] is written (exact zeros for t >= L), d_dout[b][t >= L] is
 * ignored.  The blocks' bits are the recipe's for blocks that enter the call zeroed (what nntk_optimizer_step_device with zero_gradients
 * leaves).  Onto a block that is not zero the call adds its whole gradient in ONE f32 add per element -- a second call onto the same block
 * gives exactly twice the first -- where the unidirectional call adds its row slices one by one, so there the last bits may differ from
 * the recipe's.  All scratch lives in the two handles, reserved on first use.
 * -1 and nntk_last_error(), before anything is enqueued and with nothing written or remembered: a NULL handle or pointer, an inference
 * handle, the same handle twice, handles that differ in a size above, a length outside [0, T], an unknown merge, (device form) an output
 * that overlaps the input; for the gradient call also: (device form) d_grad_forward, d_grad_backward and d_dX overlapping one another; no bidirectional forward call on this pair, in this order, since either handle's
 * last forward call. */
int GRUBidirectionalApplyTrainingBatchDevice(GRU forward, GRU backward, const float *d_input /*[B,T,in]*/, float *d_output,
                                             const int *lengths /*host [B] or NULL*/, int merge);
int LSTMBidirectionalApplyTrainingBatchDevice(LSTM forward, LSTM backward, const float *d_input, float *d_output, const int *lengths, int merge);
int RNNBidirectionalApplyTrainingBatchDevice(RNN forward, RNN backward, const float *d_input, float *d_output, const int *lengths, int merge);
int GRUBidirectionalCalculateGradientDevice(GRU forward, GRU backward, float *d_grad_forward, float *d_grad_backward, float *d_dX /*[B,T,in]*/,
                                            const float *d_dout);
int LSTMBidirectionalCalculateGradientDevice(LSTM forward, LSTM backward, float *d_grad_forward, float *d_grad_backward, float *d_dX,
                                             const float *d_dout);
int RNNBidirectionalCalculateGradientDevice(RNN forward, RNN backward, float *d_grad_forward, float *d_grad_backward, float *d_dX,
                                            const float *d_dout);
/* the same on host memory (upload, device call, download).  The blocks d_W | d_U | d_b_i | d_b_h of the two gradients are accumulated as
 * *CalculateGradient does; the layer's input gradient goes to d_X [B][T][in] (the d_X fields of the two gradients are not written) */
int GRUBidirectionalApplyTrainingBatch(GRU forward, GRU backward, const float *input, float *output, const int *lengths, int merge);
int LSTMBidirectionalApplyTrainingBatch(LSTM forward, LSTM backward, const float *input, float *output, const int *lengths, int merge);
int RNNBidirectionalApplyTrainingBatch(RNN forward, RNN backward, const float *input, float *output, const int *lengths, int merge);
int GRUBidirectionalCalculateGradient(GRU forward, GRU backward, GRUGradient *grad_forward, GRUGradient *grad_backward, float *d_X,
                                      const float *d_out);
int LSTMBidirectionalCalculateGradient(LSTM forward, LSTM backward, LSTMGradient *grad_forward, LSTMGradient *grad_backward, float *d_X,
                                       const float *d_out);
int RNNBidirectionalCalculateGradient(RNN forward, RNN backward, RNNGradient *grad_forward, RNNGradient *grad_backward, float *d_X,
                                      const float *d_out);
/* ---- frag3 tensors: activations already split for the split-bf16 x 3 contraction ---------------------------------------------
 * The default contraction of conv / dense / recurrent layers multiplies every f32 operand as three bf16 terms (x = hi + mid + lo,
 * exactly).  A FRAG3 tensor is a [batch][T][C] f32 tensor stored as those three images in MFMA fragment order:
 * [T][2 ceil(batch / 64)][ceil(C / 16)][3] blocks of 1 KB, block = 32 batch rows x 16 channels, lane 32 kh + n of a wavefront holding
 * channels 16 ks + 8 kh .. + 7 of batch row 32 ht + n as 8 consecutive bf16.  Padding CHANNELS (past C) are zeros; padding ROWS (past the
 * batch, up to the next multiple of 64) are unspecified -- nntk_frag3_pack_device writes zeros there, the recurrent kernels write the
 * state of rows that computed on zero inputs, the conv epilogue (Conv1dBatchNormActivationApplyDeviceFrag3) does not write them at all:
 * a consumer must not let them reach a real row (every consumer here masks).  6 bytes per value
 * instead of 4; in exchange a consumer's operand fetch is a run of coalesced 1 KB loads straight into MFMA registers (no LDS
 * staging, no split, no per-row requests).  The register-resident GRU / LSTM kernels produce their output in this form for free
 * (it is their inter-workgroup hand-off) and read their input from it; the dense GEMM reads it as its A operand.
 * The format is exact for every value the three bf16 terms can represent -- unpack(pack(x)) == x for finite |x| <= 3.39e38 that are not
 * denormal (a larger |x| or +-inf gives NaN, a denormal 0: INTEGRATION.md section 6) -- so every *Frag3 call equals its f32 counterpart BIT FOR BIT.
 * Scratch: a layer on the register-resident kernels keeps its T-deep hand-off (= its output in frag3 form, 6 bytes per batch * T * H value,
 * 1.5 x the f32 output) in the handle when the caller passes no d_output_frag3 -- also for plain <GRU|LSTM>ApplyDevice calls.
 *   <GRU|LSTM>ApplyDeviceFrag3: input as f32 (d_input) or frag3 (d_input_frag3), one of them NULL; output as f32 (d_output), frag3
 *   (d_output_frag3, needs return_sequences) or both, unused ones NULL.  Zero initial state per sequence.  Shapes the register-resident
 *   kernels do not take run the other kernels through f32 scratch -- the call is valid for every layer.
 *   LSTMTimeDistributedDenseApplyDevice = LSTMApplyDevice then TimeDistributedDenseApplyDevice without the f32 tensor in between
 *   (on the FRAG2H form below by default; option dense_f16x2 = 0: on frag3, bit for bit the two f32 calls). */
size_t nntk_frag3_floats(int batch, int T, int C);                       /* size of a frag3 tensor, in floats */
int nntk_frag3_pack_device(const float *d_x /*[batch,T,C]*/, float *d_frag3, int batch, int T, int C);
int nntk_frag3_unpack_device(const float *d_frag3, float *d_x /*[batch,T,C]*/, int batch, int T, int C);
/* Which kernel family the batch forms of this layer take, and -- when it is not the register-resident one -- why (shape, activations,
 * weights, options): a human-readable line, valid until the calling thread's next call of the same function.  Depends on the layer
 * only, never on the batch size. */
const char *GRUKernelPlan(GRU filter);
const char *LSTMKernelPlan(LSTM filter);
int GRUApplyDeviceFrag3(GRU filter, const float *d_input, const float *d_input_frag3, float *d_output, float *d_output_frag3, int batch);
int LSTMApplyDeviceFrag3(LSTM filter, const float *d_input, const float *d_input_frag3, float *d_output, float *d_output_frag3, int batch);
int TimeDistributedDenseApplyDeviceFrag3(TimeDistributedDense filter, const float *d_input_frag3 /*[batch,ts,in]*/, float *d_output, int batch);
/* Conv1d -> BatchNorm -> activation (bn / act may be NULL) with the output as a frag3 tensor [batch][Tout][Cout]
 * (nntk_frag3_floats(batch, Tout, Cout) floats), written by the conv kernel's epilogue: the layer in front of a recurrent layer
 * hands over the operand form directly (reference seam: layers/conv_1d.c:122-147 -> layers/lstm.c:201).  Equals
 * Conv1dBatchNormActivationApplyDevice -> nntk_frag3_pack_device bit for bit; valid for every layer (shapes the epilogue does not take
 * -- stride != 1, kernel_size > 9 -- run those two calls through scratch in the handle). */
int Conv1dBatchNormActivationApplyDeviceFrag3(Conv1d filter, BatchNorm bn, ActivationFunction act,
                                              const float *d_input /*[batch,T,Cin]*/, float *d_output_frag3, int batch);
/* ---- FRAG2H tensors: a bounded activation tensor as two f16 images, for a three-product contraction ----------------------------
 * The same block structure as frag3 -- [T][2 ceil(batch / 64)][ceil(C / 16)][2] blocks of 1 KB, same lane order -- holding hi = f16(x 2^15)
 * and lo = f16(x 2^15 - hi): |x - (hi + lo) 2^-15| <= 2^-23 |x| (at worst one f32 ulp, 0.3 ulp rms; absolute 2^-40 below |x| ~ 2^-17), 4 bytes
 * per value.  f16 ends at 65 504, so the form is DEFINED FOR |x| < 2 ONLY (a larger value becomes inf): it is what a GRU / LSTM layer with
 * the standard activations produces (|h| < 1).  The dense GEMM on it (weights as two f16 images of W 2^q, q chosen at upload so that
 * max |W| 2^q <= 32 768; weights must be finite) sums three products hi.hi + hi.lo + lo.hi per k step instead of frag3's six at the same MFMA
 * rate, f32 accumulation, one exact multiplication by 2^-(15 + q) in the epilogue.  Measured against an f64 dot product of the same f32
 * operands the error is below the frag3 / f32-input GEMM's and below that of the reference's own f32 accumulation order
 * (profiles/r05_gemm_f16x2_micro.log; tests/test_gpu_frag2h.py) -- but the results are NOT bit-identical to those routes.
 *   LSTMApplyDeviceFrag2h: the layer's sequence output in this form; -1 for non-standard activations / return_sequences == false.
 *     For 256 < H <= 512 the call runs the HF instantiation of the register-resident kernel: the RECURRENCE ITSELF multiplies h -- the same
 *     bounded operand -- as two f16 images against two f16 images of U 2^q (three products per k step; the input projection x.W keeps its
 *     three bf16 images and six products), and the kernel's hand-off buffer IS the frag2h tensor.  Same tolerance against the reference as the
 *     six-product kernel (tests/test_gpu_frag2h.py: T = 996 against the oracle and float64), not the same bits; option rec_hf = 0 keeps the
 *     six-product recurrence (its output wave then writes the form).  Which kernel runs depends on the layer only, never on the call.
 *   TimeDistributedDenseApplyDeviceFrag2h: valid for every layer (shapes / weights the f16 kernel does not take unpack to f32).
 *   LSTMTimeDistributedDenseApplyDevice takes this route by default when it applies (option dense_f16x2 = 0: the frag3 route). */
size_t nntk_frag2h_floats(int batch, int T, int C);
int nntk_frag2h_pack_device(const float *d_x /*[batch,T,C], |x| < 2*/, float *d_frag2h, int batch, int T, int C);
int nntk_frag2h_unpack_device(const float *d_frag2h, float *d_x /*[batch,T,C]*/, int batch, int T, int C);
int LSTMApplyDeviceFrag2h(LSTM filter, const float *d_input, const float *d_input_frag3, float *d_output_frag2h, int batch);
int TimeDistributedDenseApplyDeviceFrag2h(TimeDistributedDense filter, const float *d_input_frag2h /*[batch,ts,in]*/, float *d_output, int batch);
int LSTMTimeDistributedDenseApplyDevice(LSTM lstm, TimeDistributedDense tdd, const float *d_input /*[batch,T,in]*/,
                                        float *d_output /*[batch,T,out]*/, int batch);
int DenseApplyDevice(Dense filter, const float *d_input /*[rows,in]*/, float *d_output /*[rows,out]*/, int rows);
int TimeDistributedDenseApplyDevice(TimeDistributedDense filter, const float *d_input, float *d_output, int batch);

/* recurrent state of the stateful single-sequence API (gru.c:201, lstm.c:264-265) */
int GRUResetState(GRU filter);
int LSTMResetState(LSTM filter);
int RNNResetState(RNN filter);
int GRUGetState(GRU filter, float *h_host);
int RNNGetState(RNN filter, float *h_host);
int LSTMGetState(LSTM filter, float *h_host, float *c_host);

/* ---- nntoolkitcore/train/loss.h:17-23, train/optimizers.h:12-16 ------- */
/* Host pointers, the reference's names and operation order (per-sample sums in order, batch sum in order).  One
 * documented difference: categorical_crossentropy_derivative writes EVERY row; the reference's loop (loss.c:47-52)
 * forgets the row offset and only ever writes row 0 (identical here). */
float mean_squared_error(float *y, float *y_pred, int size, int batch);
void  mean_squared_error_derivative(float *y, float *y_pred, float *d_y_pred, int size, int batch);
float categorical_crossentropy(float *y, float *y_pred, int c, int batch);
void  categorical_crossentropy_derivative(float *y, float *y_pred, float *d_y_pred, int c, int batch);
typedef struct { float learning_rate; } SGD;
int   sgd_optimize(SGD optimizer, float *gradient, float *weights, int size);    /* w -= g * lr, two roundings */
/* device-pointer forms */
int nntk_mean_squared_error_device(const float *d_y, const float *d_pred, int size, int batch, float *loss);
int nntk_categorical_crossentropy_device(const float *d_y, const float *d_pred, int c, int batch, float *loss);
int nntk_mean_squared_error_derivative_device(const float *d_y, const float *d_pred, float *d_out, int size, int batch);
int nntk_categorical_crossentropy_derivative_device(const float *d_y, const float *d_pred, float *d_out, int c, int batch);
int nntk_sgd_optimize_device(SGD optimizer, const float *d_gradient, float *d_weights, long size);

/* ---- a multi-tensor optimizer over caller-owned device blocks: SGD, momentum SGD, Adam / AdamW; gradient scaling, global-norm clipping,
 *      a non-finite guard and gradient zeroing in the same step (INTEGRATION.md "Optimizers") ------------------------------------------
 * One handle owns the list of (weights, gradient) blocks of a model -- any device pointers, 4-byte aligned, e.g. the d_grad blocks that
 * <Layer>CalculateGradientDevice adds into and device copies of the <Layer>GetWeights() blocks -- plus the moments.  A step is TWO kernel
 * launches whatever n_blocks is, on the calling thread's current stream, and the host reads nothing back: the norm, the clip factor, the
 * skip decision and the step count are produced and consumed on the device.
 * Semantics are PyTorch's (torch.optim.SGD / Adam / AdamW, torch.nn.utils.clip_grad_norm_), so hyper-parameters carry over:
 *   g = gradient * grad_scale;  norm = L2 norm of g over ALL blocks;  g *= min(1, clip_norm / (norm + 1e-6)) when clip_norm > 0
 *   weight_decay: g += weight_decay * w, or with `decoupled` w *= 1 - lr * weight_decay first (AdamW)
 *   kind 0: w -= lr * g        kind 1: buf = momentum * buf + g (buf = g on the first step); w -= lr * (nesterov ? g + momentum * buf : buf)
 *   kind 2: m += (1 - beta1)(g - m); v = beta2 v + (1 - beta2) g^2; w -= lr / (1 - beta1^t) * m / (sqrt(v) / sqrt(1 - beta2^t) + epsilon)
 * Non-finite guard: when the norm is not finite (a NaN or inf in any gradient, or a sum of squares past the float range) the step is
 *   SKIPPED: weights, moments and the step count keep their bits, info[2] reads 1; the gradients are still zeroed with zero_gradients.
 *   The norm is computed whether or not clip_norm is set.
 * Deterministic: no atomics; the same inputs give the same bits; a block's result does not depend on the order of the list (the
 *   per-chunk sums of squares are added exactly, as scaled integers); the summation tree inside a block is fixed by the total size.
 * nntk_optimizer_create checks its arguments before it allocates or enqueues anything and needs no GPU to refuse them: NULL and
 *   nntk_last_error() for an unknown kind, n_blocks < 0, a negative size, a NULL or misaligned pointer of a non-empty block, beta1 / beta2
 *   outside [0, 1), a negative epsilon, clip_norm, weight_decay or momentum.  Empty blocks and n_blocks == 0 are valid (the step touches
 *   no block).  The pointer / size table is uploaded once, here; the blocks must stay allocated while the handle lives.
 * nntk_optimizer_info_device: 4 floats on the device, valid after a step in stream order: the norm before clipping | the clip factor
 *   applied (0 on a skipped step) | 1.0 if the step was skipped | steps taken so far.
 * nntk_optimizer_state_device: the moments of one block for checkpoints (sizes[block] floats each): kind 1 d_m = the momentum buffer,
 *   kind 2 d_m / d_v = Adam's first / second moment; NULL where the kind has none or the block is empty.
 * nntk_optimizer_set_learning_rate takes effect at the next step enqueued after it, in stream order. */
typedef struct {
    int   kind;               /* 0 SGD, 1 SGD with momentum, 2 Adam */
    float learning_rate;
    float momentum; int nesterov;            /* kind 1 */
    float beta1, beta2, epsilon;             /* kind 2 */
    float weight_decay; int decoupled;       /* L2 added to the gradient, or (decoupled) w *= 1 - lr * wd first: AdamW */
    float grad_scale;         /* every gradient is multiplied by this first (1 / batch); 0 means 1 */
    float clip_norm;          /* global L2 norm over ALL blocks after grad_scale; 0 = no clipping */
    int   zero_gradients;     /* the step leaves every gradient block zeroed: replaces the caller's memsets */
} NntkOptimizerConfig;
typedef struct NntkOptimizerStruct *NntkOptimizer;
NntkOptimizer nntk_optimizer_create(NntkOptimizerConfig cfg, int n_blocks, float *const *d_weights, float *const *d_grads, const long *sizes);
int   nntk_optimizer_step_device(NntkOptimizer opt);
int   nntk_optimizer_set_learning_rate(NntkOptimizer opt, float lr);
const float *nntk_optimizer_info_device(NntkOptimizer opt);
int   nntk_optimizer_state_device(NntkOptimizer opt, int block, float **d_m, float **d_v);
void  nntk_optimizer_destroy(NntkOptimizer opt);

/* ---- CTC (Graves et al., 2006) on softmax probabilities: loss, gradient, best-path decoding; rows ragged --------
 * The loss of a frame-wise softmax trained on unsegmented label sequences, and the decoder that goes with it (INTEGRATION.md "CTC").
 *   d_probs [batch][T][C]: PROBABILITIES (a softmax TimeDistributedDense's output), not log-probabilities; frames t >= input_lengths[b]
 *     influence nothing and may hold anything, NaN included.
 *   input_lengths / labels [batch][max_label_len] / label_lengths: HOST memory (input_lengths NULL = every row T), checked before anything
 *     is enqueued -- -1, nntk_last_error() and nothing written for an input length outside [0, T], a label length outside
 *     [0, max_label_len], a label outside [0, C) or equal to blank, or blank outside [0, C) -- and copied in stream order.
 *   d_loss_rows [batch]: -log p(labels_b | probs_b), unreduced; +inf for a row no alignment produces (input_length < label_length + the
 *     number of adjacent equal labels, or zeros in d_probs on every path).  input_length 0: 0 for an empty label, +inf otherwise.
 *   d_dprobs [batch][T][C] or NULL: d loss_b / d probs[b][t][k] -- what TimeDistributedDenseCalculateGradientDevice of a softmax layer takes
 *     as d_dout.  Every element is written; exact zeros for t >= input_lengths[b], for a class no alignment passes through at (b, t)
 *     (every probs == 0 entry included), and for the whole row when its loss is +inf.
 *   d_workspace: nntk_ctc_workspace_floats(batch, T, max_label_len) floats, 16-byte aligned.  With d_dprobs == NULL only its first
 *     nntk_ctc_workspace_floats(batch, 0, max_label_len) floats are touched.  Limits: max_label_len <= 4000; with a gradient C <= 32768.
 * Deterministic: the same bits on every call, the same loss bits with and without a gradient, a row's bits independent of the other rows.
 * Greedy decode: per row and t < input_length, argmax over C (ties: the lowest index); frames equal to the previous frame's argmax and
 * blanks are dropped.  d_labels_out [batch][T]: the row's labels, then -1 up to T; d_out_lengths [batch].
 * The host-pointer forms upload, run the device form and download.  All run on the calling thread's current stream. */
size_t nntk_ctc_workspace_floats(int batch, int T, int max_label_len);
int nntk_ctc_loss_device(const float *d_probs, int batch, int T, int C, const int *input_lengths, const int *labels,
                         const int *label_lengths, int max_label_len, int blank, float *d_loss_rows, float *d_dprobs,
                         float *d_workspace);
int nntk_ctc_greedy_decode_device(const float *d_probs, int batch, int T, int C, const int *input_lengths, int blank,
                                  int *d_labels_out, int *d_out_lengths);
int nntk_ctc_loss(const float *probs, int batch, int T, int C, const int *input_lengths, const int *labels, const int *label_lengths,
                  int max_label_len, int blank, float *loss_rows, float *dprobs);
int nntk_ctc_greedy_decode(const float *probs, int batch, int T, int C, const int *input_lengths, int blank, int *labels_out,
                           int *out_lengths);

/* ---- CTC prefix beam search (csrc/hip/ctc_beam.hip; INTEGRATION.md "CTC prefix beam search") ----
 * Acoustic scores only (nntk_ctc_beam_decode_lm_device below fuses an n-gram language model): per row the beam_width most probable label prefixes are kept per frame, each with the summed mass of ALL its
 * alignments (ending in blank, p_b; ending in its last label, p_nb), and the nbest best after the row's last frame are returned.
 *   d_probs [batch][T][C] probabilities; input_lengths HOST int [batch] or NULL (= all T); frames t >= input_lengths[b] influence
 *     nothing and may hold NaN.  Host arrays are checked before anything is enqueued: -1, nntk_last_error(), nothing written.
 *   cutoff_top_n: 0, or >= C - 1, expands every non-blank class per frame; otherwise only the cutoff_top_n non-blank classes of highest
 *     probability (ties: the lower class).  The blank and the repeat of a prefix's last label are always processed.
 *   Per frame, beam entry i (rank order) gives the stay cell i * (C + 1) -- the same prefix, p_b' = (p_b + p_nb) p[blank],
 *     p_nb' = p_nb p[last] -- and for each expanded class c the extend cell i * (C + 1) + 1 + c -- prefix + c, p_b' = 0,
 *     p_nb' = p_b p[c] if c repeats the last label, else (p_b + p_nb) p[c].  A stay cell whose prefix is also an extend cell's prefix is
 *     merged into that cell (p_b' of the stay; p_nb' = stay + extension).  Totals p_b' + p_nb' of exactly 0 are dropped; the beam_width
 *     largest totals form the next beam in descending order, exact ties to the lower cell index.
 *   d_labels_out [batch][nbest][T]: hypothesis k's labels, then -1; d_out_lengths [batch][nbest]; d_scores [batch][nbest] =
 *     ln(p_b + p_nb).  A slot without a hypothesis: labels -1, length -1, score -inf.  input_length 0: the empty prefix, score 0, in
 *     slot 0.  Every element of the three outputs is written.
 *   d_workspace: nntk_ctc_beam_workspace_floats(batch, T, C, beam_width, cutoff_top_n) floats, 16-byte aligned (24 bytes per row,
 *     frame and beam entry, plus 8 per row, frame and expanded class when a class cut applies).
 * Limits: 1 <= nbest <= beam_width <= 128; beam_width * (expanded classes + 1) <= 16384 (the candidate cells of a frame live in one
 * workgroup's LDS); T < 2^23.  Deterministic: no atomics, the same bits on every call, a row's bits independent of the other rows,
 * cutoff_top_n >= C - 1 the bits of 0.  The device form runs on the calling thread's stream and reads nothing back. */
size_t nntk_ctc_beam_workspace_floats(int batch, int T, int C, int beam_width, int cutoff_top_n);
int nntk_ctc_beam_decode_device(const float *d_probs, int batch, int T, int C, const int *input_lengths, int blank, int beam_width,
                                int cutoff_top_n, int nbest, int *d_labels_out, int *d_out_lengths, float *d_scores,
                                float *d_workspace);
int nntk_ctc_beam_decode(const float *probs, int batch, int T, int C, const int *input_lengths, int blank, int beam_width,
                         int cutoff_top_n, int nbest, int *labels_out, int *out_lengths, float *scores);

/* ---- streaming CTC decoding (INTEGRATION.md "CTC prefix beam search", Streaming) ----
 * A handle is pushed chunk by chunk -- d_probs [batch][max_frames][C] and n_frames are what a streaming stack's push returns -- and
 * after every push row b's outputs are the nbest hypotheses nntk_ctc_beam_decode_device gives on the concatenation of the row's valid
 * frames since its last reset, with the same blank, beam_width, cutoff_top_n, nbest: labels, lengths and the score BITS, for every
 * way of cutting the stream into pushes (one frame per push and pushes with n_frames[b] == 0 included).  All semantics of that call
 * carry over: candidate cells, merging, the canonical-index tie rule, dropping exact-zero totals, -1 / -inf for empty slots.
 *   A row that has seen no frame reports the empty prefix in slot 0 (length 0, score 0.0).  n_frames[b] == 0 leaves the row's state
 *     as it is and rewrites its current n-best.  A row whose beam has died (a frame with zero mass on every candidate) holds no
 *     hypothesis -- every slot -1 / -1 / -inf -- until it is reset.  Frames t >= n_frames[b] influence nothing and may hold NaN.
 *   final (HOST int [batch] or NULL): final[b] != 0 makes this push's outputs the row's final result; after they are written the
 *     row is reset and starts a new stream on the next push.  nntk_ctc_beam_stream_reset does the same for the listed rows at any time.
 *   max_labels: the capacity of the stored and returned label strings.  A longer hypothesis keeps its first max_labels labels and
 *     d_out_lengths still reports its true length; scores, lengths and ranking are unaffected (no string is ever compared).
 *     d_labels_out [batch][nbest][max_labels]: labels at index >= min(length, max_labels) are -1.  Every output element is written
 *     on every push.
 *   Host checks: n_frames (0..max_frames each) and the pointers are checked before anything is enqueued; on a refusal -1,
 *     nntk_last_error(), nothing written, the state untouched.  The host arrays are copied in stream order and are free for reuse on
 *     return.  The handle counts each row's frames since its reset on the host and refuses a push that would take a row past
 *     2^23 - 1 frames (the prefix length shares a word with the parent rank).
 *   create checks every argument before touching a device (NULL + nntk_last_error() on refusal): the one-shot call's limits
 *     (1 <= nbest <= beam_width <= 128, the 16384-cell limit, LDS fit), max_frames >= 1, max_labels >= 1, batch >= 0.  batch == 0:
 *     every call returns 0 without a device.  The device memory (nntk_ctc_beam_stream_state_bytes: 40 bytes per row and beam entry,
 *     two label strings of max_labels ints per row and beam entry, and the scratch of one push -- 8 bytes per row, frame of a push
 *     and beam entry, 8 more per expanded class under a class cut) is allocated by the first push.
 *   Deterministic: no atomics, the same bits on every run, a row's bits independent of the other rows and of how THEY are chunked.
 *   The device push runs on the calling thread's stream and reads nothing back; pushes of one handle belong on one stream.  The
 *   host-pointer push uploads, runs the device push and downloads. */
typedef struct NntkCtcBeamStreamStruct *NntkCtcBeamStream;
NntkCtcBeamStream nntk_ctc_beam_stream_create(int batch, int max_frames, int C, int blank, int beam_width, int cutoff_top_n, int nbest,
                                              int max_labels);
size_t nntk_ctc_beam_stream_state_bytes(int batch, int max_frames, int C, int beam_width, int cutoff_top_n, int max_labels);
int nntk_ctc_beam_stream_push_device(NntkCtcBeamStream s, const float *d_probs, const int *n_frames, const int *final,
                                     int *d_labels_out, int *d_out_lengths, float *d_scores);
int nntk_ctc_beam_stream_reset(NntkCtcBeamStream s, const int *rows, int n_rows);
void nntk_ctc_beam_stream_destroy(NntkCtcBeamStream s);
int nntk_ctc_beam_stream_push(NntkCtcBeamStream s, const float *probs, const int *n_frames, const int *final, int *labels_out,
                              int *out_lengths, float *scores);
/* ---- language-model fusion (INTEGRATION.md "CTC prefix beam search", Language-model fusion) ----
 * A token-level n-gram model as a deterministic backoff automaton (the usual ARPA-to-automaton form).  State 0 is the empty context;
 * state s owns the arcs [arc_begin[s], arc_begin[s+1]), labels strictly ascending, in [0, n_classes), never blank; an arc carries a
 * natural-log conditional probability and the next state.  backoff_state[0] == -1 and 0 <= backoff_state[s] < s for s > 0 (shorter
 * contexts first); backoff_logw finite; final_logp [n_states] (may hold -inf) or NULL: the end-of-sentence log-probability from each
 * state, already backed off.  The walk from state s on label c takes backoffs until a state has an arc labelled c, or state 0 has none:
 *   F(s, c) = B(s_0) B(s_1) ... G(arc), next = arc_next;   or   F = B(s_0) ... U, next = 0      with
 *   G = exp(alpha arc_logp + beta), B(s) = exp(alpha backoff_logw[s]), U = exp(alpha unk_logp + beta), E(s) = exp(alpha final_logp[s])
 *   (E = 1 without final_logp).  Each factor is computed in double and rounded once to an f32 mantissa with an int exponent; the
 *   product runs from left to right.  alpha == 0 switches the model off (every G and U is exp(beta), every B and E is 1); alpha == 0
 *   and beta == 0 make every factor exactly 1.
 * create checks all of it before it allocates anything and never touches a device: NULL + nntk_last_error() for an arc_begin that does
 * not start at 0, is not monotone or reaches 2^31; labels out of range, unsorted or blank; arc_next / start_state / backoff_state out of
 * range; NaN or +inf anywhere, a non-finite backoff_logw; alpha < 0 or not finite, beta not finite; blank outside [0, n_classes); a
 * factor whose natural log lies outside [-65536, 65536].  The arrays are copied.  The device tables (nntk_ngram_lm_device_bytes: 16
 * bytes per arc, 32 per state) are uploaded by the first decode that uses the handle; one handle belongs to one device.
 * nntk_ngram_lm_score (host only): the sum of ln F along labels from start_state, plus ln E of the last state when with_final, in
 * double from the unrounded values: fused score - nntk_ngram_lm_score = the acoustic score.  NaN + nntk_last_error() for a bad label.
 *
 * nntk_ctc_beam_decode_lm_device: nntk_ctc_beam_decode_device with the model fused in.  Every beam entry carries an LM state (the
 * empty prefix: start_state); a stay keeps it; the extend cell (i, c) holds F(state_i, c) times the acoustic value above (one more
 * multiply) and its entry takes next(state_i, c).  After the row's last frame every total is multiplied by E(state), exact zeros are
 * dropped, the rest are ordered descending (ties: the lower rank of the last beam) and the first nbest are reported with
 * score = ln(product).  A row without frames reports the empty prefix with score ln E(start_state).  lm == NULL: the acoustic call's
 * bits.  -1, nothing written, when lm was built for another class count or blank.  Workspace: nntk_ctc_beam_lm_workspace_floats.
 * nntk_ctc_beam_stream_create_lm: the streaming handle with a model, which must outlive the stream (NULL: nntk_ctc_beam_stream_create);
 * after every push a row's outputs are the bits of nntk_ctc_beam_decode_lm_device on its frames since the reset -- the E step applies
 * to what is reported, never to the carried beam.  nntk_ctc_beam_stream_state_bytes_lm: 4 more bytes per row and beam entry. */
typedef struct NntkNgramLmStruct *NntkNgramLm;
NntkNgramLm nntk_ngram_lm_create(int n_classes, int blank, int n_states, const long *arc_begin, const int *arc_label, const float *arc_logp,
                                 const int *arc_next, const int *backoff_state, const float *backoff_logw, const float *final_logp,
                                 int start_state, float unk_logp, float alpha, float beta);
double nntk_ngram_lm_score(NntkNgramLm lm, const int *labels, int n, int with_final);
size_t nntk_ngram_lm_device_bytes(NntkNgramLm lm);
void nntk_ngram_lm_destroy(NntkNgramLm lm);
size_t nntk_ctc_beam_lm_workspace_floats(int batch, int T, int C, int beam_width, int cutoff_top_n);
int nntk_ctc_beam_decode_lm_device(const float *d_probs, int batch, int T, int C, const int *input_lengths, int blank, int beam_width,
                                   int cutoff_top_n, int nbest, NntkNgramLm lm, int *d_labels_out, int *d_out_lengths, float *d_scores,
                                   float *d_workspace);
int nntk_ctc_beam_decode_lm(const float *probs, int batch, int T, int C, const int *input_lengths, int blank, int beam_width,
                            int cutoff_top_n, int nbest, NntkNgramLm lm, int *labels_out, int *out_lengths, float *scores);
NntkCtcBeamStream nntk_ctc_beam_stream_create_lm(int batch, int max_frames, int C, int blank, int beam_width, int cutoff_top_n, int nbest,
                                                 int max_labels, NntkNgramLm lm);
size_t nntk_ctc_beam_stream_state_bytes_lm(int batch, int max_frames, int C, int beam_width, int cutoff_top_n, int max_labels);
/* ---- label timestamps and confidences (INTEGRATION.md "CTC prefix beam search", Label timestamps and confidences) ----
 * The option form of the search: lm as above (NULL: acoustic), and per reported label the frame it is timed at and the log of its
 * acoustic probability there.  o == NULL, or a struct with everything off, is nntk_ctc_beam_decode_device bit for bit; lm alone is
 * nntk_ctc_beam_decode_lm_device bit for bit.  Detail is on when either pointer is not NULL; either may be NULL.  Labels, lengths and
 * score bits never depend on it.
 *   The rule.  Every beam entry carries one frame per label.  A plain stay keeps them; a plain extension at frame t appends t (counted
 *     from the row's start; in a stream from the row's last reset).  When entry j's stay is merged into entry i's extend cell, the
 *     extension's p_nb' (the LM factor included) is compared with j's stay p_nb' in the search's own number form: extension > stay,
 *     strictly, replaces the LAST frame of j by t; otherwise (exact ties included) j's frames stay.  So a label's frame is the latest
 *     frame at which entering the label outweighed continuing it -- the usual rule of open CTC decoders, NOT the Viterbi alignment
 *     (nntk_ctc_align_device gives that).  Which frames an entry holds never influences a mass, the order, the cut or an LM state.
 *   label_logps[k] = (float) log((double) probs[b][label_frames[k]][labels[k]]): the acoustic posterior, never the LM factor; always
 *     finite (a zero-probability extension is dropped, and a merge takes a frame only when its extension is > 0).
 *   label_frames / label_logps [batch][nbest][T] (the one-shot calls) or [batch][nbest][max_labels] (a push): frames are followed by
 *     -1, log-probabilities by 0.0f; a slot without a hypothesis is -1 / 0.0f throughout; every element of an output that is asked
 *     for is written.  In the device forms they are device pointers, in the host forms host pointers.
 *   Refused before anything is enqueued (-1 / NULL, nntk_last_error(), nothing written): everything the plain calls refuse; a detail
 *     output that is not 4-byte aligned or overlaps the other detail output, d_labels_out, d_out_lengths, d_scores, d_probs or
 *     d_workspace; detail pointers pushed into a stream created without detail; a stream created with detail pushed through
 *     nntk_ctc_beam_stream_push[_device].
 *   Workspace: nntk_ctc_beam_opt_workspace_floats -- detail needs no words of its own.  A stream with detail carries two more
 *     double-buffered strings per row and beam entry, the frames and the log-probabilities of its labels (earlier pushes'
 *     probabilities are gone): nntk_ctc_beam_stream_state_bytes_opt is 16 * max_labels bytes more per row and beam entry, next to the
 *     40 (44 with a model) and the 8 * max_labels of the label strings.  A hypothesis longer than max_labels keeps the frames and
 *     log-probabilities of its first max_labels labels, as it keeps those labels.  After every push the five outputs have the bits
 *     of the one-shot call on the row's frames since its reset, for every chunking. */
typedef struct {
    NntkNgramLm lm;        /* NULL: acoustic scores only */
    int *label_frames;     /* [batch][nbest][T], or NULL */
    float *label_logps;    /* the same shape, or NULL */
} NntkCtcBeamOptions;
size_t nntk_ctc_beam_opt_workspace_floats(int batch, int T, int C, int beam_width, int cutoff_top_n, const NntkCtcBeamOptions *o);
int nntk_ctc_beam_decode_opt_device(const float *d_probs, int batch, int T, int C, const int *input_lengths, int blank, int beam_width,
                                    int cutoff_top_n, int nbest, const NntkCtcBeamOptions *o, int *d_labels_out, int *d_out_lengths,
                                    float *d_scores, float *d_workspace);
int nntk_ctc_beam_decode_opt(const float *probs, int batch, int T, int C, const int *input_lengths, int blank, int beam_width,
                             int cutoff_top_n, int nbest, const NntkCtcBeamOptions *o, int *labels_out, int *out_lengths, float *scores);
NntkCtcBeamStream nntk_ctc_beam_stream_create_opt(int batch, int max_frames, int C, int blank, int beam_width, int cutoff_top_n, int nbest,
                                                  int max_labels, NntkNgramLm lm, int with_detail);
size_t nntk_ctc_beam_stream_state_bytes_opt(int batch, int max_frames, int C, int beam_width, int cutoff_top_n, int max_labels, int with_lm,
                                            int with_detail);
int nntk_ctc_beam_stream_push_opt_device(NntkCtcBeamStream s, const float *d_probs, const int *n_frames, const int *final,
                                         int *d_labels_out, int *d_out_lengths, float *d_scores, int *d_label_frames,
                                         float *d_label_logps);
int nntk_ctc_beam_stream_push_opt(NntkCtcBeamStream s, const float *probs, const int *n_frames, const int *final, int *labels_out,
                                  int *out_lengths, float *scores, int *label_frames, float *label_logps);
/* Streaming best path: the labels THIS chunk adds.  d_probs [batch][T][C]; n_frames HOST int [batch], 0..T; d_prev [batch] device
 * int, in/out: the argmax of the row's last frame seen, -1 = a new stream (the caller resets a row by writing -1); unchanged where
 * n_frames[b] == 0.  A frame whose argmax equals the previous frame's (d_prev[b] for the chunk's first) is dropped, then blanks are.
 * d_labels_out [batch][T], -1 behind the labels; d_out_lengths [batch].  The concatenation of a row's chunk outputs equals
 * nntk_ctc_greedy_decode_device on the concatenated frames; argument checks and ties (lowest index) are that call's. */
int nntk_ctc_greedy_decode_stream_device(const float *d_probs, int batch, int T, int C, const int *n_frames, int blank, int *d_prev,
                                         int *d_labels_out, int *d_out_lengths);

/* ---- CTC forced alignment (csrc/hip/ctc_align.hip; INTEGRATION.md "CTC forced alignment") ----
 * Given a row's labels, its single most probable alignment (Viterbi): which frames belong to which label.
 *   d_probs, input_lengths, labels [batch][max_label_len], label_lengths: as for nntk_ctc_loss_device -- probabilities, HOST int arrays
 *     (input_lengths NULL = every row T) with the same checks, made before anything is enqueued: -1, nntk_last_error(), nothing
 *     written.  Frames t >= input_lengths[b] influence nothing and may hold NaN.
 *   Row b has L labels and the extended states s in [0, 2L]; cls(s) is the blank for even s, labels[(s - 1) / 2] for odd s.
 *     v_0(0) = p[0][blank], v_0(1) = p[0][cls(1)], every other v_0 is 0; v_t(s) = max(v_{t-1}(s), v_{t-1}(s-1), v_{t-1}(s-2)) p[t][cls(s)],
 *     the s - 2 term only for odd s >= 3 with cls(s) != cls(s - 2).  Values carry an int32 exponent of their own: no underflow.
 *   Ties: the candidates are taken in the order s, s - 1, s - 2 and a later one replaces the current one only if it is strictly
 *     greater.  The path ends in state 2L unless v(2L - 1) is strictly greater (L = 0: state 0).
 *   d_states [batch][T] or NULL: the best path's state for t < input_length, then -1.  Odd s: frame t emits label (s - 1) / 2; even: blank.
 *   d_spans [batch][max_label_len][2] or NULL: for label i < L the first frame in state 2i + 1 and one past the last such frame (they
 *     are contiguous); -1, -1 for i >= L.
 *   d_scores [batch]: ln of the best path's probability.  A row no alignment produces (input_length < label_length + the number of
 *     adjacent equal labels, or zeros in d_probs on every path): -inf, every state -1, every span -1.  input_length 0: 0 for an empty
 *     label, -inf otherwise.  Every element of every non-NULL output is written.
 *   d_workspace: nntk_ctc_align_workspace_floats(batch, T, max_label_len) floats, 16-byte aligned: 1 byte per row, frame and extended
 *     state (batch * T * (2 max_label_len + 1) bytes of backpointers), plus 4 (3 + max_label_len) bytes per row and 16.
 * Limit: max_label_len <= 4000.  Deterministic: no atomics, the same bits on every call, a row's bits independent of the other rows
 * and of max_label_len.  The host-pointer form uploads, runs the device form and downloads.  The device form runs on the calling
 * thread's stream and reads nothing back. */
size_t nntk_ctc_align_workspace_floats(int batch, int T, int max_label_len);
int nntk_ctc_align_device(const float *d_probs, int batch, int T, int C, const int *input_lengths, const int *labels,
                          const int *label_lengths, int max_label_len, int blank, int *d_states, int *d_spans, float *d_scores,
                          float *d_workspace);
int nntk_ctc_align(const float *probs, int batch, int T, int C, const int *input_lengths, const int *labels, const int *label_lengths,
                   int max_label_len, int blank, int *states, int *spans, float *scores);

/* ---- RNN-Transducer (Graves, 2012): loss, gradient and joiner (csrc/hip/rnnt.hip; INTEGRATION.md "RNN-Transducer: loss and joiner") ----
 *   d_logits [batch][T][max_label_len + 1][V]: UNNORMALISED scores (the vocabulary Dense on top of the joiner, identity activation); the
 *     log-softmax over V is fused into the call.  Write U_b = label_lengths[b], T_b = input_lengths[b], p = softmax over V, y_u the row's
 *     u-th label (1-based).  alpha(0, 0) = 1, alpha(t, u) = alpha(t-1, u) p_blank(t-1, u) + alpha(t, u-1) p_{y_u}(t, u-1);
 *     P_b = alpha(T_b-1, U_b) p_blank(T_b-1, U_b); beta symmetrically, beta(T_b-1, U_b) = p_blank(T_b-1, U_b).  Cells with t >= T_b or
 *     u > U_b influence nothing and may hold anything, NaN included.
 *   input_lengths / labels [batch][max_label_len] / label_lengths: HOST memory (input_lengths NULL = every row T), checked before anything
 *     is enqueued, as are the shape and the pointers -- -1, nntk_last_error() and nothing written for an input length outside [1, T], a
 *     label length outside [0, max_label_len], a label outside [0, V) or equal to blank, blank outside [0, V), V < 2, a NULL tensor, a
 *     d_logits / d_dlogits / d_workspace that is not 16-byte aligned, d_dlogits overlapping d_logits -- and copied in stream order.  A
 *     refusal needs no device.  Repeated labels need no special rule.
 *   d_loss_rows [batch]: -log P_b, unreduced.  Finite whenever the row's live scores are (the variables and the emissions carry an
 *     int32 exponent of their own; an emission below 2^-4000 of its cell's total counts as 2^-4000); +inf only through -inf scores.
 *     A -inf score is a zero emission (a masked class, a -inf bias of the projection) and has the gradient 0.  A live cell whose V
 *     scores are all -inf has two zero emissions: no path passes through it, its gradient row is exact zeros and never NaN, and the
 *     row's loss is finite as long as a path goes round the cell.  This holds for the stored, the fused, the simple and the banded loss.
 *   d_dlogits or NULL: d loss_b / d logits; per live cell
 *       alpha(t,u) / P ( p_v beta(t,u) - [v = blank] p_blank beta(t+1,u) - [v = y_{u+1}] p_y beta(t,u+1) ),
 *     beta(T_b, U_b) standing for 1 in the blank term of the last cell.  Every element is written: exact zeros for t >= T_b or u > U_b
 *     and for a row with P = 0.
 *   d_workspace: nntk_rnnt_workspace_floats(batch, T, max_label_len, want_grad) floats, 16-byte aligned: 16 bytes per cell of
 *     [batch][T][max_label_len + 1], 24 more with a gradient, plus 4 (4 + max_label_len) bytes per row and 16.
 * Limits: max_label_len <= 4000, T + max_label_len <= 65536.  Deterministic: no atomics, the same bits on every call, the same loss
 * bits with and without a gradient, a row's bits independent of the other rows and of the T / max_label_len padding.
 * The host-pointer form uploads, runs the device form and downloads.  All run on the calling thread's current stream.
 *
 * Joiner: d_out [batch][T][U1][J] = act(d_enc [batch][T][J] + d_pred [batch][U1][J]); activation 0 identity, 1 tanh (tanhf), 2 relu
 * (max(x, 0)), the formulas of activation_default.  Backward, from the forward OUTPUT (not read for the identity) and d_dout of the same
 * shape, overwriting both results: d_denc[b][t][:] = sum over u, ascending, of d_dout act'; d_dpred[b][u][:] = the sum over t, ascending;
 * one accumulator per element, no atomics.  The vocabulary projection on top is Dense / TimeDistributedDense with batch T U1 rows. */
size_t nntk_rnnt_workspace_floats(int batch, int T, int max_label_len, int want_grad);
int nntk_rnnt_loss_device(const float *d_logits, int batch, int T, int V, const int *input_lengths, const int *labels,
                          const int *label_lengths, int max_label_len, int blank, float *d_loss_rows, float *d_dlogits,
                          float *d_workspace);
int nntk_rnnt_loss(const float *logits, int batch, int T, int V, const int *input_lengths, const int *labels, const int *label_lengths,
                   int max_label_len, int blank, float *loss_rows, float *dlogits);
int nntk_rnnt_joint_device(const float *d_enc, const float *d_pred, int batch, int T, int U1, int J, int activation, float *d_out);
int nntk_rnnt_joint_backward_device(const float *d_out_fwd, const float *d_dout, int batch, int T, int U1, int J, int activation,
                                    float *d_denc, float *d_dpred);

/* ---- RNN-Transducer: fused training loss (csrc/hip/rnnt_fused.hip; INTEGRATION.md "RNN-Transducer: fused training loss") ----
 * Joiner, vocabulary projection and loss in one call: with logits[b][t][u] = act(d_enc[b][t] + d_pred[b][u]) W + b, d_loss_rows[b] is
 * what nntk_rnnt_loss_device defines on those logits -- which are never stored, and neither is their gradient.
 *   d_enc [batch][T][J], d_pred [batch][U1 = max_label_len + 1][J]; d_out: the Dense block W [J,V] row-major | b [V], the layout
 *     nntk_rnnt_decoder_create takes; activation 0 identity, 1 tanh, 2 relu, as in nntk_rnnt_joint_device.  Cells with t >= T_b or
 *     u > U_b influence nothing: enc / pred may hold NaN there, and none of it reaches any output.
 *   input_lengths / labels / label_lengths: HOST memory, exactly the checks of nntk_rnnt_loss_device.
 *   d_denc [batch][T][J], d_dpred [batch][U1][J], d_dout [J V + V] (laid out like d_out): all three NULL (loss only) or all three given;
 *     the gradients of the PLAIN SUM of the loss rows (no averaging), overwritten, every element written; exact zeros in d_denc for
 *     t >= T_b, in d_dpred for u > U_b, and from a row with P = 0.
 *   d_workspace: nntk_rnnt_fused_workspace_floats(batch, T, max_label_len, J, V, want_grad) floats, 16-byte aligned.  In floats, with
 *     cells = batch T U1: nntk_rnnt_workspace_floats(batch, T, max_label_len, want_grad) -- the per-cell scalars: 4 per cell, 6 more with a
 *     gradient, and the host arrays -- and, with a gradient only, cells J (d z act', the one tensor of the joiner's size) +
 *     J V (W transposed) + 32 (J + 1) V (32 partial blocks of d_dout, added in order: a constant number, whatever the batch, T and
 *     the labels).  Every part is rounded up to 16 bytes.  Nothing of
 *     batch T U1 V elements exists anywhere.
 * Refused on the host before anything is enqueued (-1, nntk_last_error(), nothing written, no device needed): everything
 * nntk_rnnt_loss_device and nntk_rnnt_joint_device refuse; J outside [1, 1024]; V above 8192; gradient pointers only partly given; a NULL
 * tensor; a workspace that is not 16-byte aligned; an output overlapping another output, an input or the workspace.
 * Deterministic: no atomics, the same bits on every call, the same loss bits with and without a gradient; a row's loss, d_denc and
 * d_dpred bits do not depend on the other rows, on the row's position in the batch or on the T / max_label_len padding.  The products
 * run on the exact-f32 MFMA (f32 inputs, one fmaf chain per element).  Runs on the calling thread's stream and reads nothing back; the
 * host-pointer form uploads, runs the device form and downloads. */
size_t nntk_rnnt_fused_workspace_floats(int batch, int T, int max_label_len, int J, int V, int want_grad);
int nntk_rnnt_fused_loss_device(const float *d_enc, const float *d_pred, const float *d_out, int batch, int T, int J, int V, int activation,
                                const int *input_lengths, const int *labels, const int *label_lengths, int max_label_len, int blank,
                                float *d_loss_rows, float *d_denc, float *d_dpred, float *d_dout, float *d_workspace);
int nntk_rnnt_fused_loss(const float *enc, const float *pred, const float *out, int batch, int T, int J, int V, int activation,
                         const int *input_lengths, const int *labels, const int *label_lengths, int max_label_len, int blank,
                         float *loss_rows, float *denc, float *dpred, float *dout);

/* ---- RNN-Transducer: pruned training loss (csrc/hip/rnnt_pruned.hip; INTEGRATION.md "RNN-Transducer: pruned training loss") ----
 * Kuang et al., "Pruned RNN-T for fast, memory-efficient ASR training" (2022), in three steps and a joiner that gathers the band.  The
 * conventions are those of nntk_rnnt_loss_device: U1 = max_label_len + 1, HOST input_lengths (NULL = every row T) / labels /
 * label_lengths with exactly its checks, padding (t >= T_b or u > U_b) never read -- NaN there is legal -- and given zero gradient.
 *
 * 1. Simple loss.  score(t, u, v) = d_am[b][t][v] + d_lm[b][u][v], an f32 sum rounded once; no [batch][T][U1][V] tensor exists.
 *   d_am [batch][T][V], d_lm [batch][U1][V]: 16-byte aligned.
 *   d_loss_rows [batch]: the bits nntk_rnnt_loss_device gives on the broadcast sum tensor.
 *   d_dam [batch][T][V], d_dlm [batch][U1][V]: both NULL or both given; the gradient of the plain sum of the loss rows: the stored loss's
 *     per-cell gradient g(t, u, v) summed over u (d_dam) and over t (d_dlm), the index ascending, in a double rounded once.  Every
 *     element is written; zeros on padding and from a row with P = 0.
 *   d_occ [batch][T][U1] or NULL: the occupancy alpha(t,u) beta(t,u) / P of every cell; 0 on padding and in rows with P = 0.
 *   d_workspace: nntk_rnnt_simple_workspace_floats(batch, T, max_label_len, want_grad) floats, 16-byte aligned; want_grad = a gradient or
 *     d_occ is asked: nntk_rnnt_workspace_floats of the same arguments plus, with want_grad, 4 per cell.
 * 2. Prune ranges.  From d_occ and S, d_ranges [batch][T] int on the DEVICE; nothing is read back.  With fin = max(0, U_b + 1 - S):
 *     w(t, s) = sum over u = s .. s + S - 1, ascending, in double, of occ(t, u), for s in [0, fin]; s0[t] = the lowest s that attains the
 *     maximum; then one forward pass, r[-1] = 0, lo[t] = max(0, fin - (T_b - 1 - t)(S - 1)), hi[t] = min(fin, t (S - 1)),
 *     r[t] = clamp(s0[t], max(lo[t], r[t-1]), min(hi[t], r[t-1] + S - 1)).  So r[0] = 0, r[T_b - 1] = fin, r never decreases and steps by
 *     at most S - 1: the band holds (0, 0) and (T_b - 1, U_b) and is connected.  Frames t >= T_b get fin.  Frames t >= T_b of d_occ
 *     are never read, nor is u > U_b in a row with U_b + 1 >= S.  A row with fewer positions than S (U_b + 1 < S) has the one window
 *     s = 0, whose sum does reach into u in (U_b, S): what those cells hold (NaN included) changes nothing, r[t] is 0 either way.
 *   Refused: S outside [1, U1]; a row with (T_b - 1)(S - 1) < U_b + 1 - S, which has no connected band.
 *   d_workspace: nntk_rnnt_prune_workspace_floats(batch) floats (the two length arrays), 4-byte aligned.
 * 3. Banded joiner.  d_out [batch][T][S][J] = act(d_enc[b][t][:] + d_pred[b][r[b][t] + s][:]), activations as nntk_rnnt_joint_device.
 *   Backward from the forward OUTPUT: d_denc[b][t] = the sum over s, ascending; d_dpred[b][u] = the sum over the frames t whose window
 *   holds u, t ascending, gathered per (b, u): one accumulator per element, no atomics, every element written.
 * 4. Banded loss.  d_logits [batch][T][S][V] (the vocabulary Dense on the banded joiner): cell (t, s) is lattice cell (t, u = r[t] + s),
 *   its label emission that of label u, padding where u > U_b.  d_loss_rows[b] = -log of the mass of the paths whose cells all lie in
 *   the band, never below the full loss; d_dlogits [batch][T][S][V] or NULL, every element written once.  A row whose band carries
 *   no mass behaves like a row with P = 0: loss +inf, zero gradient.  With S = U1 (all ranges 0) loss and gradient are the bits of
 *   nntk_rnnt_loss_device on the same tensor.  d_logits, d_dlogits and d_workspace -- nntk_rnnt_pruned_workspace_floats(batch, T,
 *   max_label_len, want_grad) = nntk_rnnt_workspace_floats: the per-cell scalars of the FULL lattice -- 16-byte aligned.
 * d_ranges is device data no host check can see: every kernel clamps each value into [0, U1 - S], so no content of it causes an access
 * outside the tensors (with the clamp r + s never exceeds U1 - 1).
 * Refused on the host before anything is enqueued (-1, nntk_last_error(), nothing written, no device needed): everything
 * nntk_rnnt_loss_device (and, for the joiner, nntk_rnnt_joint_device) refuses; S out of range; the infeasible row; d_dam / d_dlm only
 * partly given; NULL or misaligned tensors; an output overlapping another output, an input or the workspace.
 * Deterministic: no atomics, the same bits on every call, a row's bits independent of the other rows and of its position in the batch.
 * The host-pointer forms upload, run the device form and download.  All run on the calling thread's stream. */
size_t nntk_rnnt_simple_workspace_floats(int batch, int T, int max_label_len, int want_grad);
int nntk_rnnt_simple_loss_device(const float *d_am, const float *d_lm, int batch, int T, int V, const int *input_lengths, const int *labels,
                                 const int *label_lengths, int max_label_len, int blank, float *d_loss_rows, float *d_dam, float *d_dlm,
                                 float *d_occ, float *d_workspace);
int nntk_rnnt_simple_loss(const float *am, const float *lm, int batch, int T, int V, const int *input_lengths, const int *labels,
                          const int *label_lengths, int max_label_len, int blank, float *loss_rows, float *dam, float *dlm, float *occ);
size_t nntk_rnnt_prune_workspace_floats(int batch);
int nntk_rnnt_prune_ranges_device(const float *d_occ, int batch, int T, const int *input_lengths, const int *label_lengths,
                                  int max_label_len, int S, int *d_ranges, float *d_workspace);
int nntk_rnnt_prune_ranges(const float *occ, int batch, int T, const int *input_lengths, const int *label_lengths, int max_label_len, int S,
                           int *ranges);
int nntk_rnnt_pruned_joint_device(const float *d_enc, const float *d_pred, const int *d_ranges, int batch, int T, int U1, int S, int J,
                                  int activation, float *d_out);
int nntk_rnnt_pruned_joint_backward_device(const float *d_out_fwd, const float *d_dout, const int *d_ranges, int batch, int T, int U1, int S,
                                           int J, int activation, float *d_denc, float *d_dpred);
size_t nntk_rnnt_pruned_workspace_floats(int batch, int T, int max_label_len, int want_grad);
int nntk_rnnt_pruned_loss_device(const float *d_logits, const int *d_ranges, int batch, int T, int S, int V, const int *input_lengths,
                                 const int *labels, const int *label_lengths, int max_label_len, int blank, float *d_loss_rows,
                                 float *d_dlogits, float *d_workspace);
int nntk_rnnt_pruned_loss(const float *logits, const int *ranges, int batch, int T, int S, int V, const int *input_lengths, const int *labels,
                          const int *label_lengths, int max_label_len, int blank, float *loss_rows, float *dlogits);

/* ---- RNN-Transducer: forced alignment (csrc/hip/rnnt_align.hip; INTEGRATION.md "RNN-Transducer: forced alignment") ----
 * Given a row's labels, its single most probable path through the lattice (Viterbi): in which frame every label is emitted.
 *   d_logits, input_lengths, labels, label_lengths, blank: as for nntk_rnnt_loss_device, with exactly its checks, made before anything
 *     is enqueued: -1, nntk_last_error(), nothing written, no device needed.  The fused form takes d_enc, d_pred, d_out, J, V and
 *     activation as nntk_rnnt_fused_loss_device does, with that call's checks and its limits J <= 1024, V <= 8192; the scores are
 *     never stored.  Cells with t >= T_b or u > U_b influence nothing and may hold NaN.
 *   v(0, 0) = 1; into cell (t, u) the candidates are taken in the order v(t-1, u) p_blank(t-1, u) (the blank move), then
 *     v(t, u-1) p_{y_u}(t, u-1) (the label move), and the label move replaces the blank move only if it is strictly greater; the path's
 *     probability is v(T_b-1, U_b) p_blank(T_b-1, U_b).  Values and emissions carry an int32 exponent of their own: no underflow at
 *     any T + U.  As in the loss, an emission below 2^-4000 of its cell's total counts as 2^-4000.
 *   d_label_frames [batch][max_label_len] or NULL: the frame t in which label i < U_b is emitted (the move (t, i) -> (t, i + 1)),
 *     non-decreasing in i; -1 for i >= U_b.
 *   d_frame_labels [batch][T] or NULL: the number of labels emitted when frame t < T_b is left by its blank (the u of that blank move);
 *     -1 for t >= T_b.
 *   d_label_logp [batch][max_label_len] / d_frame_logp [batch][T], or NULL: ln of the label's emission and of the frame's blank
 *     emission on the path, from mantissa and exponent; 0 in the padding.  exp(label_logp) is a per-label confidence.
 *   d_scores [batch]: ln of the path's probability; the sum of the row's label_logp and frame_logp up to rounding.  A row whose every
 *     path holds a zero emission (-inf scores): -inf, label_frames and frame_labels -1, both logp arrays 0.
 *   Every element of every non-NULL output is written.  Outputs may not overlap one another, the inputs or the workspace.
 *   d_workspace, 16-byte aligned: nntk_rnnt_align_workspace_floats(batch, T, max_label_len) =
 *     nntk_rnnt_workspace_floats(batch, T, max_label_len, 0) rounded up to 4 floats, plus one backpointer byte per cell of
 *     batch (T + max_label_len) anti-diagonals, each min(T, max_label_len + 1) cells wide (rounded up to 16 bytes), plus 16 bytes;
 *     nntk_rnnt_fused_align_workspace_floats(batch, T, max_label_len, J, V): the same on top of
 *     nntk_rnnt_fused_workspace_floats(batch, T, max_label_len, J, V, 0).
 * Limits: max_label_len <= 4000, T + max_label_len <= 65536.  Deterministic: no atomics, the same bits on every call; a row's bits
 * do not depend on the other rows, on its position in the batch or on the T / max_label_len padding.  The device forms run on the
 * calling thread's stream and read nothing back; the host-pointer forms upload, run the device form and download. */
size_t nntk_rnnt_align_workspace_floats(int batch, int T, int max_label_len);
int nntk_rnnt_align_device(const float *d_logits, int batch, int T, int V, const int *input_lengths, const int *labels,
                           const int *label_lengths, int max_label_len, int blank, int *d_label_frames, int *d_frame_labels,
                           float *d_label_logp, float *d_frame_logp, float *d_scores, float *d_workspace);
int nntk_rnnt_align(const float *logits, int batch, int T, int V, const int *input_lengths, const int *labels, const int *label_lengths,
                    int max_label_len, int blank, int *label_frames, int *frame_labels, float *label_logp, float *frame_logp,
                    float *scores);
size_t nntk_rnnt_fused_align_workspace_floats(int batch, int T, int max_label_len, int J, int V);
int nntk_rnnt_fused_align_device(const float *d_enc, const float *d_pred, const float *d_out, int batch, int T, int J, int V, int activation,
                                 const int *input_lengths, const int *labels, const int *label_lengths, int max_label_len, int blank,
                                 int *d_label_frames, int *d_frame_labels, float *d_label_logp, float *d_frame_logp, float *d_scores,
                                 float *d_workspace);
int nntk_rnnt_fused_align(const float *enc, const float *pred, const float *out, int batch, int T, int J, int V, int activation,
                          const int *input_lengths, const int *labels, const int *label_lengths, int max_label_len, int blank,
                          int *label_frames, int *frame_labels, float *label_logp, float *frame_logp, float *scores);

/* ---- RNN-Transducer: greedy decoding (csrc/hip/rnnt_decode.hip; INTEGRATION.md "RNN-Transducer: greedy decoding") ----
 * The model: a one-layer LSTM prediction network over a label embedding, a linear projection to the joiner width, the joiner of
 * nntk_rnnt_joint_device and a vocabulary Dense.  V classes, embedding width E, hidden width H, joiner width J; caller-owned device blocks:
 *   d_embed [V][E] row-major; row `blank` is the start-of-sequence input
 *   d_lstm  the LSTMGetWeights block W [E,4H] | U [H,4H] | b_i [4H] | b_h [4H], gates i, f, g, o, the default activations
 *   d_pred_proj  Dense layout W [H,J] | b [J], or NULL: identity, which requires H == J
 *   d_out   Dense layout W [J,V] | b [V]
 * create / load_weights_device copy what the kernel reads into the decoder's own device memory -- U, the projection, the vocabulary
 * Dense, and the table embed W + b_i + b_h [V][4H] (one product, so an emission costs h U alone) -- and return after the copies are
 * done: the four blocks may be freed or rewritten at once.  load takes d_pred_proj exactly when create did.
 * Per row b, with n = n_frames[b] live frames of d_enc [batch][T][J]: (h, c) = 0, one LSTM step on embed[blank], g = proj(h); t = 0,
 * s = 0; while t < n: z = act(enc[b][t] + g), logits = z W_out + b_out, k = argmax (ties: the lowest index), lp = logits[k] -
 * logsumexp(logits), score += lp; k == blank: t += 1, s = 0; else label k is appended with frame t, an LSTM step on embed[k], g = proj(h),
 * s += 1, and when s == max_symbols_per_frame: t += 1, s = 0 (no blank is scored for that move).  A row that holds max_labels labels
 * stops for good.  Frames t >= n_frames[b] influence nothing and may hold NaN.
 *   d_labels_out [batch][max_labels]: the labels, then -1; d_label_frames (same shape, or NULL): the frame of each label, then -1;
 *   d_out_lengths [batch]; d_scores [batch] or NULL: the sum of lp over the row's decisions.  n_frames 0: length 0, score 0.
 * With a state (nntk_rnnt_decode_state_create: batch rows of h, c, g, s, the label count, the frames consumed and the score, 8 H + 4 J +
 * 28 bytes per row whatever the stream's length) the call continues every row where the last call left it: the caller passes the
 * same output buffers on every push, labels are appended, frames count from the start of the row's stream, lengths and scores are
 * rewritten, and any split of a row's frames into pushes gives the one-shot call's labels, frames, lengths and score bits.  reset
 * (rows NULL, 0: every row) puts rows back to the start, in stream order.  A state belongs to its decoder and must not outlive it.
 * Checks, all on the host before anything is enqueued (-1 / NULL, nntk_last_error(), nothing written): a NULL handle or required
 * pointer; V < 2 or > 8192; blank outside [0, V); E, H, J < 1 or > 1024; d_pred_proj NULL with H != J; joint_activation not 0 / 1 / 2;
 * max_symbols_per_frame < 1; max_labels < 1; n_frames[b] outside [0, T] (host array; NULL = every row T); batch different from the
 * state's; a tensor that is not 4-byte aligned; output arrays overlapping one another or d_enc.
 * Deterministic: no atomics, the same bits on every call; a row's labels, frames and score bits do not depend on the other rows, its
 * position in the batch, the T padding, or how many rows share a workgroup.  One launch on the calling thread's stream, nothing read
 * back.  The host-pointer form uploads, runs the device form and downloads (with a state it first uploads the label buffers). */
typedef struct { int V, blank, E, H, J, joint_activation, max_symbols_per_frame; } NntkRnntDecoderConfig;
typedef struct NntkRnntDecoderStruct *NntkRnntDecoder;
typedef struct NntkRnntDecodeStateStruct *NntkRnntDecodeState;
NntkRnntDecoder nntk_rnnt_decoder_create(NntkRnntDecoderConfig cfg, const float *d_embed, const float *d_lstm, const float *d_pred_proj,
                                         const float *d_out);
int nntk_rnnt_decoder_load_weights_device(NntkRnntDecoder d, const float *d_embed, const float *d_lstm, const float *d_pred_proj,
                                          const float *d_out);
void nntk_rnnt_decoder_destroy(NntkRnntDecoder d);
NntkRnntDecodeState nntk_rnnt_decode_state_create(NntkRnntDecoder d, int batch);
int nntk_rnnt_decode_state_reset(NntkRnntDecodeState s, const int *rows, int n_rows);
void nntk_rnnt_decode_state_destroy(NntkRnntDecodeState s);
int nntk_rnnt_greedy_decode_device(NntkRnntDecoder d, NntkRnntDecodeState state, const float *d_enc, int batch, int T, const int *n_frames,
                                   int max_labels, int *d_labels_out, int *d_label_frames, int *d_out_lengths, float *d_scores);
int nntk_rnnt_greedy_decode(NntkRnntDecoder d, NntkRnntDecodeState state, const float *enc, int batch, int T, const int *n_frames,
                            int max_labels, int *labels_out, int *label_frames, int *out_lengths, float *scores);

/* ---- RNN-Transducer: beam search (csrc/hip/rnnt_beam.hip; INTEGRATION.md "RNN-Transducer: beam search") ----
 * The model, the weight blocks, the decoder handle and max_symbols_per_frame (S below) are those of greedy decoding; W = beam_width.
 * A hypothesis is a label sequence y, a score (natural log of probability mass, carried in double) and the prediction-network state
 * (h, c, g) after blank, y_1 .. y_|y|.  logp(t, hyp)[v] = (logits[v] - max) - log(sum exp(logits - max)), the logits from
 * act(enc[b][t] + g) W_out + b_out with the greedy kernel's arithmetic (four interleaved fmaf chains, expf per element, the sum in
 * double in a fixed order); the difference is taken in float, the rest in double.  Per row b with n = n_frames[b] live frames:
 *   A = [ (y = (), score = 0, state = LSTM step on embed[blank] from zero) ]
 *   for t in 0 .. n-1:
 *       B = empty list                       hypotheses that have left frame t
 *       C = A                                rank order
 *       for depth in 0 .. S:                 depth = labels emitted inside frame t
 *           for i, hyp in enumerate(C):      position order
 *               cand = (hyp.y, hyp.score + logp(t, hyp)[blank])
 *               if cand.score == -inf: drop
 *               elif an entry of B has the same label sequence:
 *                   entry.score = logaddexp(entry.score, cand.score)      double; the entry keeps its insertion index and state
 *               else: append to B            insertion index = running count
 *           if depth == S: break
 *           cells = { (i, v) : C[i].score + logp(t, C[i])[v]  for v != blank, for C[i] with fewer than max_labels labels, score > -inf }
 *           C = the W best cells, score descending, exact ties to the lower i*V + v;
 *               each becomes (C[i].y + v, that score, LSTM step on embed[v] from C[i]'s state)
 *           if C is empty: break
 *       A = the W best of B, score descending, exact ties to the lower insertion index
 *   result: A[0 .. nbest-1]
 * Sequences that meet at different depths are merged only in B; p_blank depends only on (t, y), so this is the lattice sum: with no
 * pruning and S at least the label count, a hypothesis's final score is exactly ln P(y | x), minus the transducer loss.  "Same label
 * sequence" is decided exactly on the labels (a hash only pre-filters).  B holds at most W (S + 1) entries a frame.
 *   d_labels_out [batch][nbest][max_labels]: hypothesis k's labels, then -1; d_out_lengths [batch][nbest]; d_scores [batch][nbest]: the
 *   double score rounded to f32.  A slot without a hypothesis holds labels -1, length -1, score -inf.  n_frames[b] == 0: the empty
 *   hypothesis with score 0 in slot 0.  Every element of the three outputs is written.  Frames t >= n_frames[b] influence nothing and
 *   may hold NaN.  d_workspace: nntk_rnnt_beam_workspace_floats(d, batch, beam_width, max_labels) floats, 16-byte aligned.
 * state NULL: every row starts from the beginning and nothing is kept.  With a state (nntk_rnnt_beam_state_create: per row W label
 * sequences, double scores and (h, c, g); nntk_rnnt_beam_state_bytes bytes whatever the stream's length) the call continues every
 * row from the A the last push left, and the three outputs are rewritten with the n-best over all frames pushed so far: any split of
 * a row's frames into pushes gives the one-shot call's labels, lengths and score bits.  beam_width and max_labels must equal the
 * state's; a state belongs to its decoder and must not outlive it.  reset (rows NULL, 0: every row) puts rows back to the start.
 * Checks, all on the host before anything is enqueued (-1 / NULL, nntk_last_error(), nothing written): a NULL handle or required
 * pointer; beam_width outside [1, 32]; nbest outside [1, beam_width]; max_labels < 1; n_frames[b] outside [0, T] (host array; NULL =
 * every row T); batch, beam_width or max_labels different from the state's; an output that is not 4-byte aligned, a workspace that is
 * not 16-byte aligned; outputs overlapping one another, d_enc or the workspace; a model beyond the kernel's LDS.
 * Deterministic: no atomics, the same bits on every call; a row's bits do not depend on the other rows, its position in the batch,
 * the T padding, or how many hypotheses share a pass over a matrix.  One launch on the calling thread's stream.  The host-pointer
 * form uploads, runs the device form on a workspace of its own and downloads.  Language-model fusion, and label timestamps,
 * confidences and length normalisation: below. */
typedef struct NntkRnntBeamStateStruct *NntkRnntBeamState;
size_t nntk_rnnt_beam_workspace_floats(NntkRnntDecoder d, int batch, int beam_width, int max_labels);
int nntk_rnnt_beam_decode_device(NntkRnntDecoder d, NntkRnntBeamState state, const float *d_enc, int batch, int T, const int *n_frames,
                                 int beam_width, int nbest, int max_labels, int *d_labels_out, int *d_out_lengths, float *d_scores,
                                 float *d_workspace);
int nntk_rnnt_beam_decode(NntkRnntDecoder d, NntkRnntBeamState state, const float *enc, int batch, int T, const int *n_frames,
                          int beam_width, int nbest, int max_labels, int *labels_out, int *out_lengths, float *scores);
NntkRnntBeamState nntk_rnnt_beam_state_create(NntkRnntDecoder d, int batch, int beam_width, int max_labels);
size_t nntk_rnnt_beam_state_bytes(NntkRnntDecoder d, int batch, int beam_width, int max_labels);
int nntk_rnnt_beam_state_reset(NntkRnntBeamState s, const int *rows, int n_rows);
void nntk_rnnt_beam_state_destroy(NntkRnntBeamState s);
/* ---- language-model fusion (INTEGRATION.md "RNN-Transducer: beam search", Language-model fusion) ----
 * nntk_rnnt_beam_decode_lm_device: nntk_rnnt_beam_decode_device with an n-gram handle (NntkNgramLm, above) fused into the search, in
 * the same single launch.  Every hypothesis carries a state q of the automaton; the initial hypothesis has q = start_state.  In the
 * pseudo-code above:
 *   blank: cand = hyp.score + logp(t, hyp)[blank], q kept -- unchanged.  The automaton is deterministic, so hypotheses with the same
 *     labels have the same q and a merge in B needs no rule for it.
 *   label cell (i, v): score = (C[i].score + logp(t, C[i])[v]) + lnF(q_i, v), in double; the parenthesised part is the acoustic
 *     call's expression.  The new hypothesis takes q = next(q_i, v).  A cell whose score is -inf (an arc of log-probability -inf) is
 *     not a candidate.  The W best cells and the W best of B are chosen on these fused scores, with the tie rules above.
 *   lnF(s, v) is the walk of nntk_ngram_lm_score: from s, add ln B(s) and move to backoff_state[s] until a state has an arc labelled
 *     v, then add ln G(arc), next = arc_next; when state 0 has none, add ln U, next = 0.  lnF = ((0 + b_0) + b_1 ...) + g, from left to
 *     right in double, on the unrounded doubles nntk_ngram_lm_score sums (ln G = alpha arc_logp + beta, ln B = alpha backoff_logw,
 *     ln U = alpha unk_logp + beta, ln E = alpha final_logp; alpha == 0: beta, 0, beta, 0).  The device only adds them.
 *   report: every entry of the final A gets + ln E(q) (0 without final_logp); entries at -inf are dropped, the rest are ordered
 *     descending, exact ties to the lower rank in A, and the first nbest are written.  A row without frames (and without a carried
 *     beam) reports the empty hypothesis with score ln E(start_state).  With a state, the ln E term applies to what is reported after
 *     each push, never to the carried beam: any split of a row's frames into pushes gives the one-shot call's bits after every push.
 *   lm == NULL: the acoustic call, bit for bit.  alpha == 0, beta == 0 and no final_logp: every term is +0.0 and the bits are again the
 *     acoustic call's.  score - nntk_ngram_lm_score(lm, y, n, 1) is the acoustic log mass of y.
 * d_workspace: nntk_rnnt_beam_lm_workspace_floats floats with a model (the acoustic workspace, then per row 4 bytes per hypothesis
 * slot and 8 beam_width V bytes), nntk_rnnt_beam_workspace_floats without.  nntk_rnnt_beam_state_create_lm: a state for streams
 * decoded with lm (NULL: nntk_rnnt_beam_state_create), nntk_rnnt_beam_state_bytes_lm bytes: 4 more per row and beam entry, the
 * state q.  The lm must outlive the state; reset, destroy and the decode calls take the state as before.  The search reads the
 * lookup records of nntk_ngram_lm_device_bytes and doubles of its own -- nntk_ngram_lm_rnnt_device_bytes: 8 bytes per arc, 16 per
 * state -- which the first transducer decode that uses the handle uploads.
 * Refused on the host before anything is enqueued (-1 / NULL, nntk_last_error(), nothing written): everything the acoustic call
 * refuses; an lm built for another class count than V or another blank than the decoder's; a state created without an lm in a call
 * with one, a state created with an lm in a call without (nntk_rnnt_beam_decode_device included), a state created with another lm.
 * The guarantees of the acoustic call hold: no atomics, the same bits on every call, a row's bits independent of the other rows, its
 * batch position, the T padding (NaN there included) and how many hypotheses share a pass over a matrix. */
size_t nntk_ngram_lm_rnnt_device_bytes(NntkNgramLm lm);
size_t nntk_rnnt_beam_lm_workspace_floats(NntkRnntDecoder d, int batch, int beam_width, int max_labels);
int nntk_rnnt_beam_decode_lm_device(NntkRnntDecoder d, NntkRnntBeamState state, const float *d_enc, int batch, int T, const int *n_frames,
                                    int beam_width, int nbest, int max_labels, NntkNgramLm lm, int *d_labels_out, int *d_out_lengths,
                                    float *d_scores, float *d_workspace);
int nntk_rnnt_beam_decode_lm(NntkRnntDecoder d, NntkRnntBeamState state, const float *enc, int batch, int T, const int *n_frames,
                             int beam_width, int nbest, int max_labels, NntkNgramLm lm, int *labels_out, int *out_lengths, float *scores);
NntkRnntBeamState nntk_rnnt_beam_state_create_lm(NntkRnntDecoder d, int batch, int beam_width, int max_labels, NntkNgramLm lm);
size_t nntk_rnnt_beam_state_bytes_lm(NntkRnntDecoder d, int batch, int beam_width, int max_labels);
/* ---- label timestamps, confidences and length normalisation (INTEGRATION.md "RNN-Transducer: beam search", Label timestamps,
 *      confidences and length normalisation) ----
 * nntk_rnnt_beam_decode_opt_device: the beam search above with an options struct; o == NULL or a struct with everything off (lm NULL,
 * length_norm 0, both pointers NULL) is nntk_rnnt_beam_decode_device bit for bit, lm alone nntk_rnnt_beam_decode_lm_device.  "Detail"
 * is on when label_frames or label_logps is not NULL.  Every hypothesis then carries two arrays of length |y| next to its labels:
 * frames[j], the frame in which label j was emitted, counted from the start of the row's stream, and lps[j], the acoustic
 * log-probability of that emission.  In the pseudo-code above:
 *   label cell (i, v) at frame t: the new hypothesis takes C[i].frames + [t0 + t] and C[i].lps + [(float)((double)(logits[v] - max) -
 *     lse)]: t0 is the number of frames the row's stream consumed before this call (0 without a state or after a reset), the value is
 *     the double the selection already forms, rounded once to f32.  With a language model lnF is NOT part of it: lps is the acoustic
 *     confidence.
 *   entries of B also hold lead, a double, and the arrays they report.  Insert: lead = cand.score, the candidate's arrays.  Merge: the
 *     score is the logaddexp as before and the entry keeps its insertion index and state as before; if cand.score > lead (a double
 *     compare) then lead = cand.score and the entry takes the candidate's arrays; on an exact tie it keeps what it has.  A merged
 *     hypothesis so reports the alignment of its dominant contributor (not the Viterbi alignment: nntk_rnnt_align_device gives that).
 *     Which arrays are kept never influences a score, a cut or a state.
 *   frame end: A's entries take the arrays of their B entry.
 *   report: length_norm == 0: the order above.  length_norm == 1: the entries to be reported (with a model: after + ln E, the -inf
 *     entries dropped) are ranked by key = score / (double)(length + 1), the + 1 counting the initial blank, descending, exact ties to
 *     the lower rank in A, and the first nbest are written.  d_scores holds the plain score whatever the order, so with a model score -
 *     nntk_ngram_lm_score(...) stays the acoustic mass.  Normalisation touches only the report, never a cut and never the carried beam:
 *     any split of a stream into pushes gives the one-shot bits after every push, for all five outputs.
 * label_frames [batch][nbest][max_labels] int: hypothesis k's frames, then -1; label_logps, the same shape, float: the values, then
 * 0.0f.  A slot without a hypothesis holds -1 / 0.0f throughout; every element of an output that is asked for is written.  Either may
 * be NULL; in the _device form both are device pointers, in the host form host pointers.
 * d_workspace: nntk_rnnt_beam_opt_workspace_floats(d, batch, beam_width, max_labels, o) floats: what the call without the struct needs,
 * and with detail or length_norm per row 8 max_labels bytes per hypothesis slot and 12 bytes per entry of B behind it.
 * nntk_rnnt_beam_state_create_opt(.., lm, with_detail): a stream state; with_detail 0 it is nntk_rnnt_beam_state_create(_lm)'s.  With
 * detail it holds per row and beam entry max_labels ints and max_labels floats more (nntk_rnnt_beam_state_bytes_opt; whatever the
 * stream's length) and the row's count of consumed frames, which a reset of the row puts back to 0.
 * Refused on the host before anything is enqueued (-1 / NULL, nntk_last_error(), nothing written): everything the calls above refuse;
 * length_norm outside {0, 1}; a detail output that is not 4-byte aligned or overlaps another output, d_enc or the workspace; a state
 * created without detail in a call with detail and the reverse -- so a state created with detail is refused by
 * nntk_rnnt_beam_decode_device and nntk_rnnt_beam_decode_lm_device.
 * The guarantees above hold for the five outputs: no atomics, one launch, the same bits on every call, a row independent of the other
 * rows, its batch position, the T padding (NaN there included) and how many hypotheses share a pass over a matrix. */
typedef struct {
    NntkNgramLm lm;          /* NULL: the acoustic search */
    int length_norm;         /* 0 | 1 */
    int *label_frames;       /* [batch][nbest][max_labels] or NULL; a device pointer in the _device form */
    float *label_logps;      /* the same shape, or NULL */
} NntkRnntBeamOptions;
size_t nntk_rnnt_beam_opt_workspace_floats(NntkRnntDecoder d, int batch, int beam_width, int max_labels, const NntkRnntBeamOptions *o);
int nntk_rnnt_beam_decode_opt_device(NntkRnntDecoder d, NntkRnntBeamState state, const float *d_enc, int batch, int T, const int *n_frames,
                                     int beam_width, int nbest, int max_labels, const NntkRnntBeamOptions *o, int *d_labels_out,
                                     int *d_out_lengths, float *d_scores, float *d_workspace);
int nntk_rnnt_beam_decode_opt(NntkRnntDecoder d, NntkRnntBeamState state, const float *enc, int batch, int T, const int *n_frames,
                              int beam_width, int nbest, int max_labels, const NntkRnntBeamOptions *o, int *labels_out, int *out_lengths,
                              float *scores);
NntkRnntBeamState nntk_rnnt_beam_state_create_opt(NntkRnntDecoder d, int batch, int beam_width, int max_labels, NntkNgramLm lm,
                                                  int with_detail);
size_t nntk_rnnt_beam_state_bytes_opt(NntkRnntDecoder d, int batch, int beam_width, int max_labels, int with_lm, int with_detail);

/* ---- RNN-Transducer: training the prediction network (csrc/hip/rnnt_pred.hip, csrc/host/rnnt_pred.c; INTEGRATION.md "RNN-Transducer:
 *      training the prediction network") ----
 * Label embedding.  ids: HOST int arrays, like every label array of this library, checked on the host and copied in stream order (the
 * array is free on return).
 *   lookup: d_out [rows][E], d_out[r][:] = d_table[ids[r]][:], bit copies; ids[r] == -1: a row of exact zeros.  A table row that no id
 *     names is not read (it may hold NaN).  rows == 0 writes nothing.  16-byte accesses when E % 4 == 0 and both tensors are 16-byte
 *     aligned, one float per lane otherwise; the bits do not depend on it.
 *   gradient: d_dtable [V][E], d_dtable[v][:] = the sum over the rows r with ids[r] == v of d_dout[r][:]; EVERY element is written, exact
 *     zeros for an id that does not occur; rows with ids[r] == -1 are never read (they may hold NaN).  rows == 0 zeroes the table.
 *     d_workspace: nntk_embedding_workspace_floats(rows, V, E) floats, 16-byte aligned (V + 1 + rows ints of the sort, the lists of the
 *     heavy ids, and rows / 16 + 1 partial rows of E floats).
 *     No atomics.  The host counting-sorts the row numbers by id (nntk_embedding_sort_ids, O(rows + V)) and uploads the offsets and the
 *     sorted rows into the workspace.  The summation shape of an id with n rows r_0 < r_1 < .. is a function of n alone: chunks of
 *     32 consecutive list entries, each summed in ascending order in one f32 chain that starts from the chunk's first row (so one
 *     occurrence is a bit copy), then the chunk sums added in ascending chunk order.  An id with more than 32 rows -- the start symbol
 *     of a transducer batch -- has every chunk summed by a workgroup of its own.  Two calls return the same bits, and the bits of
 *     d_dtable[v] depend only on the ascending list of v's rows and their values: not on V, the other ids, or the grid.
 *   nntk_embedding_sort_ids: the stable counting sort itself, on host memory: offsets [V + 1], sorted_rows [rows]; the rows of id v
 *     are sorted_rows[offsets[v] .. offsets[v + 1]), ascending; id -1 is in no list.  Returns offsets[V], or -1.
 *   Refused on the host (-1, nntk_last_error(), nothing enqueued, no device needed): a NULL pointer; V < 1; E outside [1, 1024];
 *     rows < 0; an id outside [-1, V); a tensor that is not 4-byte aligned; a workspace that is not 16-byte aligned; d_dtable
 *     overlapping d_dout, d_out overlapping d_table, the workspace overlapping either tensor.
 * Predictor handle: exactly the decoder's prediction network (nntk_rnnt_decoder_create above) in training, on blocks of the decoder's
 * layouts: d_embed [V][E]; d_lstm, the LSTMGetWeights block W | U | b_i | b_h with the default activations; d_pred_proj, the Dense block
 * W [H,J] | b [J] -- with has_proj == 0 the projection is the identity, which requires H == J, and every projection pointer is NULL.
 * It composes the lookup above, a training-mode LSTM (batch x U1 steps, U1 = max_label_len + 1, return_sequences) through
 * LSTMLoadWeightsDevice / LSTMApplyTrainingBatchDeviceVarLen / LSTMCalculateGradientDeviceVarLen and a training-mode
 * TimeDistributedDense on batch U1 rows; d_pred, d_dlstm and d_dproj are the bits of that recipe with the lookup done on the host.
 *   load_weights_device copies the blocks into the handle (the embedding into a device copy of its own) and returns after the copies
 *     are done: the blocks may be rewritten at once, e.g. by the next optimizer step.
 *   forward: labels HOST [batch][max_label_len], label_lengths HOST [batch] or NULL (every row max_label_len).  With U_b =
 *     label_lengths[b], the input token of step u is blank for u == 0 and labels[b][u-1] for 1 <= u <= U_b; row b runs U_b + 1 LSTM steps
 *     from the zero state, d_pred[b][u] = proj(h_u): the decoder's g after blank, y_1 .. y_u.  For u > U_b, h is exact zeros, so
 *     d_pred[b][u] is the projection's bias (zeros without a projection).  labels[b][i >= U_b] are neither checked nor read.
 *   backward: belongs to the last forward (the handle remembers its ids and lengths).  d_dpred [batch][U1][J] is the gradient of any
 *     scalar with respect to d_pred; d_dpred[b][u > U_b] is ignored and may hold NaN (with a projection the handle copies d_dpred into
 *     its own scratch with those rows zeroed before the Dense gradient call; without one no copy is made, the LSTM call ignores them).
 *     d_dembed [V][E], d_dlstm (W | U | b_i | b_h) and d_dproj (W [H,J] | b [J]) are OVERWRITTEN with that scalar's gradients.
 *   device_bytes: the handle's own device buffers (the embedding copy, x, d x, and with a projection h, d h and the masked d pred, plus
 *     the embedding workspace); the two layer handles own theirs.
 * Refused on the host before anything is enqueued (-1 / NULL, nntk_last_error()): a NULL handle or pointer; V outside [2, 8192]; E, H, J
 * outside [1, 1024]; blank outside [0, V); has_proj == 0 with H != J; batch < 1; max_label_len < 0; whatever the LSTM training handle
 * refuses; a label outside [0, V) or equal to blank; a length outside [0, max_label_len]; forward before load_weights_device; backward
 * before a forward; a projection pointer that does not match has_proj.  Errors of the inner calls are passed through with their text.
 * Deterministic: no atomics in the new kernels, the same bits on every call.  Runs on the calling thread's stream, reads nothing back. */
int nntk_embedding_lookup_device(const float *d_table, int V, int E, const int *ids, int rows, float *d_out);
int nntk_embedding_gradient_device(const float *d_dout, const int *ids, int rows, int V, int E, float *d_dtable, float *d_workspace);
size_t nntk_embedding_workspace_floats(int rows, int V, int E);
int nntk_embedding_sort_ids(const int *ids, int rows, int V, int *offsets, int *sorted_rows);
typedef struct { int V, E, H, J, blank, has_proj, batch, max_label_len; } NntkRnntPredictorConfig;
typedef struct NntkRnntPredictorStruct *NntkRnntPredictor;
NntkRnntPredictor nntk_rnnt_predictor_create(NntkRnntPredictorConfig cfg);
int nntk_rnnt_predictor_load_weights_device(NntkRnntPredictor p, const float *d_embed, const float *d_lstm, const float *d_pred_proj);
int nntk_rnnt_predictor_forward_device(NntkRnntPredictor p, const int *labels, const int *label_lengths, float *d_pred);
int nntk_rnnt_predictor_backward_device(NntkRnntPredictor p, const float *d_dpred, float *d_dembed, float *d_dlstm, float *d_dproj);
size_t nntk_rnnt_predictor_device_bytes(NntkRnntPredictor p);
void nntk_rnnt_predictor_destroy(NntkRnntPredictor p);

/* ---- Error counts and MWER training (csrc/hip/edit_distance.hip; INTEGRATION.md "Error rates and MWER training") ----
 * Edit distance: how wrong every hypothesis of an n-best list is, split into substitutions, deletions and insertions.
 *   d_hyp [batch][n_hyp][max_hyp_len], d_hyp_lengths [batch][n_hyp]: DEVICE int, exactly as nntk_ctc_beam_decode_device /
 *     nntk_rnnt_beam_decode_device (max_hyp_len = T / max_labels) or the greedy decoders (n_hyp = 1) leave them.  What stands behind
 *     a hypothesis's length (the decoders write -1) is never read into the result.  A length < 0 is the decoders' "no hypothesis"
 *     slot and gives {-1, -1, -1, -1}; a length above max_hyp_len is read as max_hyp_len.
 *   refs [batch][max_ref_len], ref_lengths [batch]: HOST int, like the labels / label_lengths of the loss calls (the same arrays
 *     serve both), checked before anything is enqueued, then copied in stream order.
 *   sep < 0, unit mode: tokens are compared as ints, any value.  sep >= 0, word mode: both sequences are cut at tokens equal to sep
 *     (leading, trailing and repeated separators make no empty words) and the same dynamic program runs over words; two words are
 *     equal iff they have the same length and the same tokens (a hash pre-filters, the decision is exact).
 *   Definition, h_1..h_m the hypothesis's units and r_1..r_n the reference's: D[0][j] = j (all deletions), D[i][0] = i (all
 *     insertions); for i, j >= 1 a cell takes the smallest of (1) D[i-1][j-1] + (h_i != r_j), a hit or substitution, (2) D[i][j-1] + 1,
 *     a deletion (r_j has no counterpart), (3) D[i-1][j] + 1, an insertion; on an equal distance the earlier candidate in that order
 *     wins.  A cell's three counts are its chosen predecessor's counts plus the chosen operation; the result is cell (m, n) -- the
 *     counts of a backtrace from (m, n) that takes the first minimal predecessor in the same order.  Hits = n - S - D.
 *   d_counts [batch][n_hyp][4]: {distance = S + D + I, substitutions, deletions, insertions} of every pair.
 *   d_ref_units [batch] or NULL: the reference's units -- ref_lengths[b], in word mode its word count.
 *     Every element of both outputs is written.
 *   d_workspace: nntk_edit_distance_workspace_floats(batch, n_hyp, max_hyp_len, max_ref_len) floats, 16-byte aligned: the copy of
 *     the references and, for word mode, 8 bytes per possible word (every second token) of every sequence.
 * Refused on the host before anything is enqueued, without a device (-1, nntk_last_error(), nothing written): batch < 0, n_hyp < 1,
 * max_hyp_len outside [0, 32767] (every count fits 16 bits), max_ref_len outside [0, 4000] (the loss calls' limit: a pair's diagonals
 * live in one workgroup's LDS), a reference length outside [0, max_ref_len], a NULL pointer (d_ref_units apart), a workspace that is
 * not 16-byte aligned.  Deterministic: integer arithmetic, no atomics, the same bits on every call; a pair's counts depend on
 * nothing but the pair -- not on the other rows, the padding, max_hyp_len or max_ref_len.  The device form runs on the calling
 * thread's stream and reads nothing back; nntk_edit_distance takes every pointer in host memory: upload, device form, download.
 *
 * MWER (Prabhavalkar et al., 2018): the expected error over the renormalised n-best list and its gradient.  d_logp [batch][n_hyp]:
 * the hypotheses' log-probabilities, finite or -inf (minus the loss rows of a loss call run with the hypotheses as labels);
 * d_err: int, hypothesis k of row b at d_err[(b n_hyp + k) err_stride] -- err_stride 4 reads the distance column of d_counts in place.
 * A hypothesis is valid iff err >= 0.  Over the valid ones P_k = exp(logp_k - logsumexp(logp)), e = the plain mean of err;
 *   d_risk_rows [batch] = sum_k P_k (err_k - e),    d_dlogp [batch][n_hyp] = d risk / d logp_k = P_k ((err_k - e) - risk);
 * either output may be NULL.  Invalid slots get exact zeros; a row with no valid hypothesis, or whose valid logp are all -inf, gets
 * risk 0 and gradient 0: no NaN is ever written.  Accumulated in double in index order, rounded to f32 once; no atomics.
 *
 * Row scale: d_out[r][:] = d_x[r][:] d_scale[r] over [rows][row_floats], one f32 multiply per element; d_out may be d_x.  A
 * d_scale[r] of exactly 0 gives exact zeros whatever the row holds, inf and NaN included.  With d_scale = -d_dlogp it turns the
 * unreduced gradient of nntk_rnnt_loss_device / nntk_ctc_loss_device, run with the hypotheses as labels on batch n_hyp rows, into the
 * gradient of the risk; the rows of invalid hypotheses may hold anything. */
size_t nntk_edit_distance_workspace_floats(int batch, int n_hyp, int max_hyp_len, int max_ref_len);
int nntk_edit_distance_device(const int *d_hyp, const int *d_hyp_lengths, int batch, int n_hyp, int max_hyp_len, const int *refs,
                              const int *ref_lengths, int max_ref_len, int sep, int *d_counts, int *d_ref_units, float *d_workspace);
int nntk_edit_distance(const int *hyp, const int *hyp_lengths, int batch, int n_hyp, int max_hyp_len, const int *refs,
                       const int *ref_lengths, int max_ref_len, int sep, int *counts, int *ref_units);
int nntk_mwer_device(const float *d_logp, const int *d_err, int err_stride, int batch, int n_hyp, float *d_risk_rows, float *d_dlogp);
int nntk_row_scale_device(const float *d_x, const float *d_scale, long rows, long row_floats, float *d_out);

#ifdef __cplusplus
}
#endif
#endif /* NNTOOLKITCORE_HIP_H */
