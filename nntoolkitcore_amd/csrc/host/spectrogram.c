/*
 * spectrogram.c -- window generators and the Spectrogram host layer.  Reference:
 * signal/window.c:13-54, signal/spectrogram.c:36-140.  The window and the scale
 * factor are setup-time host work (kept in the reference's arithmetic: window in
 * double then rounded, scale factors as left-to-right fp32 sums); frames are
 * transformed on the GPU (csrc/hip/spectrogram.hip).
 */
#include <math.h>
#include <stdlib.h>
#include <stdio.h>
#include <string.h>
#include "nntk_internal.h"

#ifndef M_PI
#define M_PI 3.14159265358979323846
#endif

/* ------------------------------- windows ---------------------------------- */

/* window.c:13-17: alpha - (1 - alpha) * cos(2*pi*i / denominator), double math */
static void cosine_sum_window(float *v, int size, int denominator, float alpha) {
    for (int i = 0; i < size; ++i) v[i] = alpha - (1 - alpha) * cos(2 * M_PI * i / denominator);
}
void ones(float *vector, int size) { for (int i = 0; i < size; ++i) vector[i] = 1.0f; }
void hann_window(float *vector, int size) { cosine_sum_window(vector, size, size - 1, 0.5f); }
void hamming_window(float *vector, int size) { cosine_sum_window(vector, size, size - 1, 0.54f); }
void periodic_hann_window(float *vector, int size) { cosine_sum_window(vector, size, size, 0.5f); }
void periodic_hamming_window(float *vector, int size) { cosine_sum_window(vector, size, size, 0.54f); }
/* window.c:49-54: the angle is held in a float */
void blackman_window(float *vector, int size) {
    for (int i = 0; i < size; ++i) {
        float angle = 2.f * M_PI * i / size;
        vector[i] = .42f - .5 * cos(angle) + .08 * cos(2 * angle);
    }
}

/* ------------------------------ spectrogram ------------------------------- */

struct SpectrogramStruct {
    SpectrogramConfig config;
    int mode;                /* 0 magnitude, 1 psd */
    int fs;
    float *window;           /* host, [window_size] */
    float scale_factor;
    int window_dirty;
    float *d_window, *d_twiddle;
    nntk_devbuf d_in, d_out;
    nntk_devbuf d_seq, d_cnt;   /* the streaming calls: assembled rows (tail ++ new samples), per-row counts (ints) */
};

/* spectrogram.c:59-70 */
SpectrogramConfig SpectrogramConfigCreate(int nfft, int window_size, int noverlap, int input_size,
                                          float fft_normalization_factor) {
    SpectrogramConfig c;
    c.nfft = nfft;
    c.window_size = window_size;
    c.noverlap = noverlap;
    c.input_size = input_size;
    c.step = window_size - noverlap;
    c.nfreq = nfft / 2 + 1;
    c.ntime_series = (input_size - noverlap) / c.step;
    c.fft_normalization_factor = fft_normalization_factor;
    return c;
}

/* spectrogram.c:36-38 (sum w) and :49-57 (fs * sum w^2), fp32 left to right */
static void recompute_scale(Spectrogram f) {
    float s = 0.0f;
    if (f->mode == 0) {
        for (int i = 0; i < f->config.window_size; ++i) s += f->window[i];
        f->scale_factor = s;
    } else {
        for (int i = 0; i < f->config.window_size; ++i) {
            float p = f->window[i] * f->window[i];
            s += p;
        }
        f->scale_factor = s * f->fs;
    }
}

static Spectrogram spectrogram_create(SpectrogramConfig config, int mode, int fs) {
    nntk_shim_clear_error();
    Spectrogram f = (Spectrogram)calloc(1, sizeof(struct SpectrogramStruct));
    if (!f) return NULL;
    f->config = config;
    f->mode = mode;
    f->fs = fs;
    f->window = (float *)calloc((size_t)(config.window_size > 0 ? config.window_size : 1), sizeof(float));
    if (!f->window) { free(f); return NULL; }
    SpectrogramSetWindowFunc(f, ones);      /* spectrogram.c:88, :96 */
    return f;
}

Spectrogram SpectrogramCreatePSD(SpectrogramConfig config, int fs) { return spectrogram_create(config, 1, fs); }
Spectrogram SpectrogramCreateMagnitude(SpectrogramConfig config) { return spectrogram_create(config, 0, 0); }
SpectrogramConfig SpectrogramGetConfig(Spectrogram filter) { return filter->config; }

/* spectrogram.c:100-107 */
void SpectrogramSetScaleFactor(Spectrogram filter, float factor) { filter->scale_factor = factor; }
void SpectrogramSetWindowFunc(Spectrogram filter, window_fn fn) {
    fn(filter->window, filter->config.window_size);
    recompute_scale(filter);
    filter->window_dirty = 1;
}

void SpectrogramDestroy(Spectrogram filter) {
    if (!filter) return;
    nntk_shim_synchronize();
    nntk_shim_free(filter->d_window);
    nntk_shim_free(filter->d_twiddle);
    nntk_devbuf_free(&filter->d_in);
    nntk_devbuf_free(&filter->d_out);
    nntk_devbuf_free(&filter->d_seq);
    nntk_devbuf_free(&filter->d_cnt);
    free(filter->window);
    free(filter);
}

static int spectrogram_ensure(Spectrogram f) {
    if (!f->d_twiddle) {
        int n = f->config.nfft;
        float *tw = (float *)malloc(sizeof(float) * 2 * (size_t)n);
        if (!tw) NNTK_FAIL("out of host memory for the twiddle table");
        for (int m = 0; m < n; ++m) {
            double phase = -2.0 * M_PI * m / n;
            tw[2 * m] = (float)cos(phase);
            tw[2 * m + 1] = (float)sin(phase);
        }
        int rc = nntk_upload_floats(&f->d_twiddle, tw, 2 * (size_t)n);
        free(tw);
        if (rc) return rc;
    }
    if (f->window_dirty || !f->d_window) {
        if (f->d_window) nntk_shim_synchronize();
        if (nntk_upload_floats(&f->d_window, f->window, (size_t)f->config.window_size)) return -1;
        f->window_dirty = 0;
    }
    return 0;
}

int SpectrogramApplyDevice(Spectrogram filter, const float *d_input, float *d_output, int batch) {
    nntk_shim_clear_error();
    if (!filter) NNTK_FAIL("SpectrogramApplyDevice: NULL handle");
    if (spectrogram_ensure(filter)) return -1;
    const SpectrogramConfig *c = &filter->config;
    return nntk_shim_spectrogram(d_input, filter->d_window, filter->d_twiddle, d_output, batch, c->input_size, c->nfft,
                                 c->window_size, c->step, c->nfreq, c->ntime_series, c->fft_normalization_factor,
                                 filter->mode, filter->scale_factor);
}

/* K1 with the mel projection fused (mel.c); 1 = not taken for this configuration */
int nntk_spectrogram_apply_mel_device(Spectrogram filter, const float *d_input, float *d_output, int batch,
                                      const int *d_mel_tab, const float *d_mel_w, int n_mels, float eps, int do_log) {
    if (spectrogram_ensure(filter)) return -1;
    const SpectrogramConfig *c = &filter->config;
    return nntk_shim_spectrogram_mel(d_input, filter->d_window, filter->d_twiddle, d_output, batch, c->input_size, c->nfft,
                                     c->window_size, c->step, c->nfreq, c->ntime_series, c->fft_normalization_factor,
                                     filter->mode, filter->scale_factor, d_mel_tab, d_mel_w, n_mels, eps, do_log);
}

/* ------------------------------ streaming --------------------------------
 * Row b's virtual sequence is s = tail ++ new, m = tail_len + n_new samples; F = m >= window_size ? (m - noverlap) / step : 0 complete
 * frames; emitted E = final ? F : F & ~1 (whole pairs only: K1 transforms frames in pairs, so holding an odd frame back keeps every
 * pair the one-shot call forms); the next tail is s[E * step : m].  Pure host arithmetic on configs. */
static int spec_stream_cfg_ok(SpectrogramConfig cfg) {
    return cfg.window_size > 0 && cfg.step > 0 && cfg.noverlap >= 0 && cfg.input_size >= 0 && cfg.nfft >= cfg.window_size;
}
int nntk_spectrogram_stream_sizes(SpectrogramConfig cfg, int *tail_floats, int *max_frames) {
    nntk_shim_clear_error();
    if (!spec_stream_cfg_ok(cfg)) NNTK_FAIL("nntk_spectrogram_stream_sizes: invalid spectrogram config");
    if (tail_floats) *tail_floats = cfg.window_size + cfg.step - 1;
    if (max_frames) *max_frames = (cfg.input_size + cfg.step - 1) / cfg.step + 1;
    return 0;
}
int nntk_spectrogram_stream_plan(SpectrogramConfig cfg, int tail_len, int n_new, int final, int *frames, int *next_tail_len) {
    nntk_shim_clear_error();
    if (!spec_stream_cfg_ok(cfg)) NNTK_FAIL("nntk_spectrogram_stream_plan: invalid spectrogram config");
    if (tail_len < 0 || tail_len > cfg.window_size + cfg.step - 1 || n_new < 0 || n_new > cfg.input_size)
        NNTK_FAIL("nntk_spectrogram_stream_plan: tail_len outside [0, window_size + step - 1] or n_new outside [0, input_size]");
    const int m = tail_len + n_new;
    const int F = m >= cfg.window_size ? (m - cfg.noverlap) / cfg.step : 0;
    const int E = final ? F : (F & ~1);
    if (frames) *frames = E;
    if (next_tail_len) *next_tail_len = final ? 0 : m - E * cfg.step;
    return 0;
}

static int ranges_overlap(const void *a, size_t na, const void *b, size_t nb) {
    const char *x = (const char *)a, *y = (const char *)b;
    return na > 0 && nb > 0 && x < y + nb && y < x + na;
}

/* The one streaming path of SpectrogramApplyDeviceStream and LogMelSpectrogramApplyDeviceStream: validation (nothing enqueued, nothing
 * written on -1), per-row plans, one count upload, the row assembly (tail update in place), K1's ST instantiation on the assembled rows
 * and -- unless the caller zeroes its own output (*d_frames_out set: the unfused log-mel form pads after its GEMM) -- the padding rows.
 * d_mel_tab != NULL: the fused mel form (returns 1, nothing enqueued, when it does not take this nfft).  orow = floats per output row. */
int nntk_spectrogram_stream_device(Spectrogram f, const char *who, const float *d_input, const int *n_new, const int *final,
                                   float *d_tail, int *tail_len, float *d_output, int *frames, int batch, int orow,
                                   const int *d_mel_tab, const float *d_mel_w, int n_mels, const int **d_frames_out) {
    char msg[256];
    if (!f) { snprintf(msg, sizeof msg, "%s: NULL handle", who); NNTK_FAIL(msg); }
    const SpectrogramConfig *c = &f->config;
    if (batch < 0) { snprintf(msg, sizeof msg, "%s: batch %d < 0", who, batch); NNTK_FAIL(msg); }
    int tf, mf;
    if (nntk_spectrogram_stream_sizes(*c, &tf, &mf)) return -1;
    if (batch == 0) return 0;
    if (!d_input || !n_new || !d_tail || !tail_len || !d_output || !frames) { snprintf(msg, sizeof msg, "%s: NULL argument", who); NNTK_FAIL(msg); }
    for (int b = 0; b < batch; ++b) {
        if (n_new[b] < 0 || n_new[b] > c->input_size) {
            snprintf(msg, sizeof msg, "%s: n_new[%d] = %d is outside [0, %d]", who, b, n_new[b], c->input_size);
            NNTK_FAIL(msg);
        }
        if (tail_len[b] < 0 || tail_len[b] > tf) {
            snprintf(msg, sizeof msg, "%s: tail_len[%d] = %d is outside [0, %d]", who, b, tail_len[b], tf);
            NNTK_FAIL(msg);
        }
    }
    const size_t n_in = (size_t)batch * c->input_size, n_tail = (size_t)batch * tf, n_out = (size_t)batch * mf * orow;
    if (ranges_overlap(d_output, n_out * 4, d_input, n_in * 4) || ranges_overlap(d_output, n_out * 4, d_tail, n_tail * 4) ||
        ranges_overlap(d_tail, n_tail * 4, d_input, n_in * 4)) {
        snprintf(msg, sizeof msg, "%s: the output, the input and the tail buffer must not overlap", who);
        NNTK_FAIL(msg);
    }
    if (d_mel_tab && (c->nfft != 512 || n_mels > 257)) return 1;      /* (spectrogram_launch's own test for the fused form) */
    int *h = (int *)malloc((size_t)4 * batch * sizeof(int));
    if (!h) NNTK_FAIL("out of host memory");
    /* [4][B]: frames | samples in the assembled row | old tail | new tail (nntk_shim.h, streaming calls) */
    for (int b = 0; b < batch; ++b) {
        int E, nt;
        (void)nntk_spectrogram_stream_plan(*c, tail_len[b], n_new[b], final ? final[b] : 0, &E, &nt);
        h[b] = E; h[batch + b] = tail_len[b] + n_new[b]; h[2 * batch + b] = tail_len[b]; h[3 * batch + b] = nt;
    }
    const int S = tf + c->input_size;
    int *d_cnt = (int *)nntk_devbuf_reserve(&f->d_cnt, (size_t)4 * batch);
    float *d_seq = nntk_devbuf_reserve(&f->d_seq, (size_t)batch * S);
    int rc = (!d_cnt || !d_seq || spectrogram_ensure(f)) ? -1 : 0;
    if (!rc) rc = nntk_shim_upload_ints(d_cnt, h, 4L * batch);
    if (!rc) rc = nntk_shim_stream_gather(d_input, d_tail, d_seq, d_cnt, batch, c->input_size, tf, 1);
    if (!rc) rc = nntk_shim_spectrogram_rows(d_seq, f->d_window, f->d_twiddle, d_output, batch, S, c->nfft, c->window_size, c->step,
                                             c->nfreq, mf, c->fft_normalization_factor, f->mode, f->scale_factor, d_cnt,
                                             d_mel_tab, d_mel_w, n_mels, 1.5849e-13f, 1);
    if (!rc && !d_frames_out) rc = nntk_shim_varlen_zero_pad(d_output, d_cnt, batch, mf, orow);
    if (!rc) {
        for (int b = 0; b < batch; ++b) { frames[b] = h[b]; tail_len[b] = h[3 * batch + b]; }
        if (d_frames_out) *d_frames_out = d_cnt;
    }
    free(h);
    return rc < 0 ? -1 : 0;
}

int SpectrogramApplyDeviceStream(Spectrogram f, const float *d_input, const int *n_new, const int *final, float *d_tail, int *tail_len,
                                 float *d_output, int *frames, int batch) {
    nntk_shim_clear_error();
    if (!f) NNTK_FAIL("SpectrogramApplyDeviceStream: NULL handle");
    return nntk_spectrogram_stream_device(f, "SpectrogramApplyDeviceStream", d_input, n_new, final, d_tail, tail_len, d_output, frames,
                                          batch, f->config.nfreq, NULL, NULL, 0, NULL);
}

int SpectrogramApplyBatch(Spectrogram filter, const float *input, float *output, int batch) {
    nntk_shim_clear_error();
    if (!filter) NNTK_FAIL("SpectrogramApplyBatch: NULL handle");
    if (batch <= 0) return 0;
    const SpectrogramConfig *c = &filter->config;
    size_t n_in = (size_t)batch * c->input_size;
    size_t n_out = (size_t)batch * c->ntime_series * c->nfreq;
    float *d_in = nntk_devbuf_reserve(&filter->d_in, n_in);
    float *d_out = nntk_devbuf_reserve(&filter->d_out, n_out);
    if (!d_in || !d_out) return -1;
    if (nntk_shim_upload(d_in, input, n_in * sizeof(float))) return -1;
    if (SpectrogramApplyDevice(filter, d_in, d_out, batch)) return -1;
    return nntk_shim_download(output, d_out, n_out * sizeof(float));
}

/* spectrogram.c:113-135: void in the reference; failures are reported through
 * nntk_last_error() and leave `output` untouched. */
void SpectrogramApply(Spectrogram filter, const float *input, float *output) {
    (void)SpectrogramApplyBatch(filter, input, output, 1);
}


/* ============================== signal/dft.h ==============================
 * The reference's public complex DFT (dft.h:15-47, dft.c:23-92: kissfft of size nfft, un-normalised; `complex` is
 * carried in the config and not used there either).  Host split-complex buffers in and out, as the reference. */
struct DFTSetupStruct {
    DFTConfig config;
    float *d_tw;              /* [nfft] (cos, sin) */
    float *d_io;              /* re | im | out re | out im */
};
DFTConfig DFTConfigCreate(int nfft, bool forward, bool complex) {
    DFTConfig c;
    memset(&c, 0, sizeof(c));
    c.nfft = nfft;
    c.forward = forward;
    c.complex = complex;
    return c;
}
DFTSetup DFTSetupCreate(DFTConfig config) {
    nntk_shim_clear_error();
    if (config.nfft <= 0) { nntk_set_error("DFTSetupCreate: nfft must be positive"); return NULL; }
    DFTSetup s = (DFTSetup)calloc(1, sizeof(struct DFTSetupStruct));
    if (!s) return NULL;
    s->config = config;
    s->d_tw = (float *)nntk_shim_malloc((size_t)2 * config.nfft * sizeof(float));
    s->d_io = (float *)nntk_shim_malloc((size_t)4 * config.nfft * sizeof(float));
    if (!s->d_tw || !s->d_io || nntk_shim_dft_twiddles(s->d_tw, config.nfft)) { DFTSetupDestroy(s); return NULL; }
    return s;
}
void DFTSetupDestroy(DFTSetup setup) {
    if (!setup) return;
    nntk_shim_synchronize();
    nntk_shim_free(setup->d_tw);
    nntk_shim_free(setup->d_io);
    free(setup);
}
void DFTPerform(DFTSetup setup, ComplexFloatSplit *input, ComplexFloatSplit *output) {
    nntk_shim_clear_error();
    if (!setup || !input || !output) { nntk_set_error("DFTPerform: NULL argument"); return; }
    const size_t n = (size_t)setup->config.nfft;
    float *d = setup->d_io;
    if (nntk_shim_upload(d, input->real_p, n * sizeof(float)) || nntk_shim_upload(d + n, input->imag_p, n * sizeof(float))) return;
    if (nntk_shim_dft(d, d + n, setup->d_tw, d + 2 * n, d + 3 * n, (int)n, setup->config.forward ? 0 : 1)) return;
    if (nntk_shim_download(output->real_p, d + 2 * n, n * sizeof(float))) return;
    (void)nntk_shim_download(output->imag_p, d + 3 * n, n * sizeof(float));
}
/* dft.c:62-75, :85-92: pure data movement between the interleaved and the split layout */
void split_complex(const ComplexFloat *complex, ComplexFloatSplit *split, int size) {
    for (int i = 0; i < size; ++i) { split->real_p[i] = complex[i].real; split->imag_p[i] = complex[i].imag; }
}
void join_complex_split(const ComplexFloatSplit *split, ComplexFloat *complex, int size) {
    for (int i = 0; i < size; ++i) { complex[i].real = split->real_p[i]; complex[i].imag = split->imag_p[i]; }
}
