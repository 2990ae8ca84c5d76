/*
 * metrics.c -- host layer of the error counts: the edit distance of every hypothesis to its row's reference, the MWER risk over an
 * n-best list and the row scale that carries its gradient into a loss call (csrc/hip/edit_distance.hip).  Every host array and every
 * argument is checked here, before anything is enqueued or allocated: a refusal needs no device.
 */
#include <stdio.h>
#include <stdint.h>
#include "nntk_internal.h"

/* scratch for the host-pointer form: per thread and device, freed at thread exit (nntk_thread_scratch, runtime.c) */
#define t_a (*nntk_thread_scratch(NNTK_TS_A))
#define t_b (*nntk_thread_scratch(NNTK_TS_B))
#define t_c (*nntk_thread_scratch(NNTK_TS_C))

static int metrics_fail(const char *who, const char *fmt, long a, long b, long c) {
    char msg[200];
    int n = snprintf(msg, sizeof msg, "%s: ", who);
    snprintf(msg + n, sizeof msg - (size_t)n, fmt, a, b, c);
    nntk_set_error(msg);
    return -1;
}

/* the shape and the host arrays of an edit distance call */
static int edit_check(const char *who, int batch, int n_hyp, int max_hyp_len, const int *refs, const int *ref_lengths, int max_ref_len) {
    if (batch < 0 || n_hyp < 1) return metrics_fail(who, "batch %ld, n_hyp %ld: batch must be >= 0, n_hyp >= 1", batch, n_hyp, 0);
    if (max_hyp_len < 0 || max_hyp_len > NNTK_EDIT_MAX_HYP_LEN)
        return metrics_fail(who, "max_hyp_len %ld is outside [0, %ld] (a count is 16 bits)", max_hyp_len, NNTK_EDIT_MAX_HYP_LEN, 0);
    if (max_ref_len < 0 || max_ref_len > NNTK_EDIT_MAX_REF_LEN)
        return metrics_fail(who, "max_ref_len %ld is outside [0, %ld] (a pair's diagonals live in one workgroup's LDS)", max_ref_len,
                            NNTK_EDIT_MAX_REF_LEN, 0);
    if (batch > 0 && (!ref_lengths || (max_ref_len > 0 && !refs))) return metrics_fail(who, "NULL refs / ref_lengths", 0, 0, 0);
    for (int b = 0; b < batch; ++b)
        if (ref_lengths[b] < 0 || ref_lengths[b] > max_ref_len)
            return metrics_fail(who, "ref_lengths[%ld] = %ld is outside [0, %ld]", b, ref_lengths[b], max_ref_len);
    return 0;
}

size_t nntk_edit_distance_workspace_floats(int batch, int n_hyp, int max_hyp_len, int max_ref_len) {
    return nntk_shim_edit_distance_workspace_floats(batch, n_hyp, max_hyp_len, max_ref_len);
}

int nntk_edit_distance_device(const int *d_hyp, const int *d_hyp_lengths, int batch, int n_hyp, int max_hyp_len, const int *refs,
                              const int *ref_lengths, int max_ref_len, int sep, int *d_counts, int *d_ref_units, float *d_workspace) {
    static const char who[] = "nntk_edit_distance_device";
    nntk_shim_clear_error();
    if (edit_check(who, batch, n_hyp, max_hyp_len, refs, ref_lengths, max_ref_len)) return -1;
    if (batch == 0) return 0;
    if (!d_hyp_lengths || !d_counts || !d_workspace || (!d_hyp && max_hyp_len > 0)) return metrics_fail(who, "NULL tensor", 0, 0, 0);
    if ((uintptr_t)d_workspace & 15) return metrics_fail(who, "the workspace must be 16-byte aligned", 0, 0, 0);
    if (((uintptr_t)d_hyp | (uintptr_t)d_hyp_lengths | (uintptr_t)d_counts | (uintptr_t)d_ref_units) & 3)
        return metrics_fail(who, "an int tensor is not 4-byte aligned", 0, 0, 0);
    return nntk_shim_edit_distance(d_hyp, d_hyp_lengths, batch, n_hyp, max_hyp_len, refs, ref_lengths, max_ref_len, sep, d_counts,
                                   d_ref_units, d_workspace);
}

int nntk_edit_distance(const int *hyp, const int *hyp_lengths, int batch, int n_hyp, int max_hyp_len, const int *refs,
                       const int *ref_lengths, int max_ref_len, int sep, int *counts, int *ref_units) {
    static const char who[] = "nntk_edit_distance";
    nntk_shim_clear_error();
    if (edit_check(who, batch, n_hyp, max_hyp_len, refs, ref_lengths, max_ref_len)) return -1;
    if (batch == 0) return 0;
    if (!hyp_lengths || !counts || (!hyp && max_hyp_len > 0)) return metrics_fail(who, "NULL array", 0, 0, 0);
    const size_t np = (size_t)batch * n_hyp, nt = np * max_hyp_len;
    int *d_h = (int *)nntk_devbuf_reserve(&t_a, nt + np + 4);                         /* hypotheses | their lengths */
    int *d_o = (int *)nntk_devbuf_reserve(&t_b, 4 * np + (size_t)batch + 4);          /* counts | reference units */
    float *d_ws = nntk_devbuf_reserve(&t_c, nntk_shim_edit_distance_workspace_floats(batch, n_hyp, max_hyp_len, max_ref_len));
    if (!d_h || !d_o || !d_ws) return -1;
    if (nt && nntk_shim_upload(d_h, hyp, nt * sizeof(int))) return -1;
    if (nntk_shim_upload(d_h + nt, hyp_lengths, np * sizeof(int))) return -1;
    if (nntk_edit_distance_device(d_h, d_h + nt, batch, n_hyp, max_hyp_len, refs, ref_lengths, max_ref_len, sep, d_o, d_o + 4 * np, d_ws))
        return -1;
    if (nntk_shim_download(counts, d_o, 4 * np * sizeof(int))) return -1;
    return ref_units ? nntk_shim_download(ref_units, d_o + 4 * np, (size_t)batch * sizeof(int)) : 0;
}

int nntk_mwer_device(const float *d_logp, const int *d_err, int err_stride, int batch, int n_hyp, float *d_risk_rows, float *d_dlogp) {
    static const char who[] = "nntk_mwer_device";
    nntk_shim_clear_error();
    if (batch < 0 || n_hyp < 1) return metrics_fail(who, "batch %ld, n_hyp %ld: batch must be >= 0, n_hyp >= 1", batch, n_hyp, 0);
    if (err_stride < 1) return metrics_fail(who, "err_stride %ld < 1", err_stride, 0, 0);
    if (batch == 0) return 0;
    if (!d_logp || !d_err || (!d_risk_rows && !d_dlogp)) return metrics_fail(who, "NULL tensor", 0, 0, 0);
    if (((uintptr_t)d_logp | (uintptr_t)d_err | (uintptr_t)d_risk_rows | (uintptr_t)d_dlogp) & 3)
        return metrics_fail(who, "a tensor is not 4-byte aligned", 0, 0, 0);
    return nntk_shim_mwer(d_logp, d_err, err_stride, batch, n_hyp, d_risk_rows, d_dlogp);
}

int nntk_row_scale_device(const float *d_x, const float *d_scale, long rows, long row_floats, float *d_out) {
    static const char who[] = "nntk_row_scale_device";
    nntk_shim_clear_error();
    if (rows < 0 || row_floats < 0) return metrics_fail(who, "rows %ld, row_floats %ld: both must be >= 0", rows, row_floats, 0);
    if (rows == 0 || row_floats == 0) return 0;
    if (!d_x || !d_scale || !d_out) return metrics_fail(who, "NULL tensor", 0, 0, 0);
    if (((uintptr_t)d_x | (uintptr_t)d_scale | (uintptr_t)d_out) & 3) return metrics_fail(who, "a tensor is not 4-byte aligned", 0, 0, 0);
    return nntk_shim_row_scale(d_x, d_scale, rows, row_floats, d_out);
}
