/*
 * ngram_lm.c -- the token-level n-gram language model of the fused CTC beam search (INTEGRATION.md "CTC prefix beam search",
 * Language-model fusion): a deterministic backoff automaton, checked in full on the host, scored on the host in double, and laid out
 * as 16-byte records that the first decode using the handle uploads.  create, score and destroy never touch a device.  The fused
 * transducer beam search (rnnt_decode.c) adds the unrounded logs themselves: a second table of doubles, uploaded by its first decode.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "nntk_internal.h"

#define LM_EZERO (-(1 << 28))              /* ctc_xf.hpp: the exponent of a zero mass */
#define LM_MAX_LN 65536.0                  /* |ln factor| a table may hold: the exponents of a whole utterance stay inside an int */

struct NntkNgramLmStruct {
    int n_classes, blank, n_states, n_arcs, start_state, depth, have_final;
    double alpha, beta, unk_ln;            /* unk_ln = alpha * unk_logp + beta */
    long *arc_begin;
    int *arc_label, *arc_next, *backoff_state;
    double *arc_ln, *backoff_ln, *final_ln;    /* ln G, ln B, ln E: the unrounded values nntk_ngram_lm_score sums */
    int *tab;                              /* the device image: 4 words per arc, 8 per state; NULL once uploaded */
    int unk_m, unk_e;
    nntk_devbuf d_tab;
    int uploaded;
    nntk_devbuf d_ln;                      /* the transducer search's doubles: ln G per arc, then ln B | ln E per state */
    int ln_uploaded;
};

static void *lm_fail(const char *fmt, long a, long b, long c) {
    char msg[200];
    int n = snprintf(msg, sizeof msg, "nntk_ngram_lm_create: ");
    snprintf(msg + n, sizeof msg - (size_t)n, fmt, a, b, c);
    nntk_set_error(msg);
    return NULL;
}

/* exp(x) rounded once to an f32 mantissa in [0.5, 1) and an exponent; zero for x = -inf */
static void lm_xf(double x, int *m_bits, int *e) {
    float m = 0.0f;
    int ex = LM_EZERO;
    if (x == 0.0) {                        /* the unit factor, exactly: xf_one() */
        m = 0.5f;
        ex = 1;
    } else if (x != -INFINITY) {
        const double k = floor(x / 0.69314718055994530942) + 1.0;
        int e2;
        const double md = frexp(exp(x - k * 0.69314718055994530942), &e2);
        m = (float)md;
        ex = (int)k + e2;
        if (m == 1.0f) { m = 0.5f; ++ex; }
    }
    memcpy(m_bits, &m, sizeof m);
    *e = ex;
}

/* a log-probability of the table: no NaN, no +inf; finite_only: no -inf either.  The scaled value must stay in range. */
static int lm_bad_value(double v, double alpha, double beta, int finite_only) {
    if (isnan(v) || v == INFINITY) return 1;
    if (v == -INFINITY) return finite_only;
    return fabs(alpha * v + beta) > LM_MAX_LN;
}
static double lm_scaled(double v, double alpha, double beta) {
    /* alpha == 0 switches the model off whatever it holds: 0 * -inf is not a NaN here */
    return alpha == 0.0 ? beta : alpha * v + beta;
}

NntkNgramLm nntk_ngram_lm_create(int n_classes, int blank, int n_states, const long *arc_begin, const int *arc_label, const float *arc_logp,
                                 const int *arc_next, const int *backoff_state, const float *backoff_logw, const float *final_logp,
                                 int start_state, float unk_logp, float alpha, float beta) {
    nntk_shim_clear_error();
    if (n_classes < 1) return lm_fail("n_classes %ld < 1", n_classes, 0, 0);
    if (blank < 0 || blank >= n_classes) return lm_fail("blank %ld is outside [0, %ld)", blank, n_classes, 0);
    if (n_states < 1) return lm_fail("n_states %ld < 1", n_states, 0, 0);
    if (!arc_begin || !backoff_state || !backoff_logw) return lm_fail("NULL arc_begin, backoff_state or backoff_logw", 0, 0, 0);
    if (isnan(alpha) || alpha < 0.0f || alpha == INFINITY) return lm_fail("alpha must be finite and >= 0", 0, 0, 0);
    if (isnan(beta) || isinf(beta)) return lm_fail("beta must be finite", 0, 0, 0);
    if (start_state < 0 || start_state >= n_states) return lm_fail("start_state %ld is outside [0, %ld)", start_state, n_states, 0);
    if (arc_begin[0] != 0) return lm_fail("arc_begin[0] = %ld, not 0", arc_begin[0], 0, 0);
    for (int s = 0; s < n_states; ++s)
        if (arc_begin[s + 1] < arc_begin[s] || arc_begin[s + 1] > 0x7fffffffL)
            return lm_fail("arc_begin[%ld] = %ld: not monotone, or 2^31 arcs or more", s + 1, arc_begin[s + 1], 0);
    const long n_arcs = arc_begin[n_states];
    if (n_arcs > 0 && (!arc_label || !arc_logp || !arc_next)) return lm_fail("NULL arc_label, arc_logp or arc_next", 0, 0, 0);
    const double a = alpha, be = beta;
    for (int s = 0; s < n_states; ++s) {
        for (long q = arc_begin[s]; q < arc_begin[s + 1]; ++q) {
            if (arc_label[q] < 0 || arc_label[q] >= n_classes) return lm_fail("arc %ld: label %ld is not a class", q, arc_label[q], 0);
            if (arc_label[q] == blank) return lm_fail("arc %ld carries the blank (%ld)", q, blank, 0);
            if (q > arc_begin[s] && arc_label[q] <= arc_label[q - 1])
                return lm_fail("state %ld: arc labels are not strictly ascending at arc %ld", s, q, 0);
            if (arc_next[q] < 0 || arc_next[q] >= n_states) return lm_fail("arc %ld: next state %ld is outside [0, %ld)", q, arc_next[q], n_states);
            if (lm_bad_value(arc_logp[q], a, be, 0)) return lm_fail("arc %ld: arc_logp is NaN, +inf or out of range", q, 0, 0);
        }
        if (s == 0 ? backoff_state[0] != -1 : (backoff_state[s] < 0 || backoff_state[s] >= s))
            return lm_fail("backoff_state[%ld] = %ld: -1 for state 0, else a lower state", s, backoff_state[s], 0);
        if (lm_bad_value(backoff_logw[s], a, 0.0, 1)) return lm_fail("backoff_logw[%ld] is not finite or out of range", s, 0, 0);
        if (final_logp && lm_bad_value(final_logp[s], a, 0.0, 0)) return lm_fail("final_logp[%ld] is NaN, +inf or out of range", s, 0, 0);
    }
    if (lm_bad_value(unk_logp, a, be, 0)) return lm_fail("unk_logp is NaN, +inf or out of range", 0, 0, 0);

    NntkNgramLm lm = (NntkNgramLm)calloc(1, sizeof *lm);
    const size_t ns = (size_t)n_states, na = (size_t)n_arcs, na1 = na ? na : 1;
    if (lm) {
        lm->arc_begin = (long *)malloc((ns + 1) * sizeof(long));
        lm->arc_label = (int *)malloc(na1 * sizeof(int));
        lm->arc_next = (int *)malloc(na1 * sizeof(int));
        lm->backoff_state = (int *)malloc(ns * sizeof(int));
        lm->arc_ln = (double *)malloc(na1 * sizeof(double));
        lm->backoff_ln = (double *)malloc(ns * sizeof(double));
        lm->final_ln = (double *)malloc(ns * sizeof(double));
        lm->tab = (int *)calloc(4 * na + 8 * ns, sizeof(int));
    }
    if (!lm || !lm->arc_begin || !lm->arc_label || !lm->arc_next || !lm->backoff_state || !lm->arc_ln || !lm->backoff_ln || !lm->final_ln ||
        !lm->tab) {
        nntk_ngram_lm_destroy(lm);
        nntk_set_error("out of host memory");
        return NULL;
    }
    lm->n_classes = n_classes; lm->blank = blank; lm->n_states = n_states; lm->n_arcs = (int)n_arcs; lm->start_state = start_state;
    lm->have_final = final_logp != NULL; lm->alpha = a; lm->beta = be;
    lm->unk_ln = lm_scaled(unk_logp, a, be);
    lm_xf(lm->unk_ln, &lm->unk_m, &lm->unk_e);
    memcpy(lm->arc_begin, arc_begin, (ns + 1) * sizeof(long));
    if (na) { memcpy(lm->arc_label, arc_label, na * sizeof(int)); memcpy(lm->arc_next, arc_next, na * sizeof(int)); }
    memcpy(lm->backoff_state, backoff_state, ns * sizeof(int));
    /* device image: arcs {label, next, m, e} | states {arc_begin, arc_count, backoff_state, 0} | factors {B.m, B.e, E.m, E.e} */
    int *arc = lm->tab, *st = arc + 4 * na, *fac = st + 4 * ns;
    for (size_t q = 0; q < na; ++q) {
        lm->arc_ln[q] = lm_scaled(arc_logp[q], a, be);
        arc[4 * q] = arc_label[q];
        arc[4 * q + 1] = arc_next[q];
        lm_xf(lm->arc_ln[q], &arc[4 * q + 2], &arc[4 * q + 3]);
    }
    int *chain = (int *)fac;                                                   /* the backoff chain's length, before the factors land there */
    for (int s = 0; s < n_states; ++s) {
        chain[s] = s == 0 ? 0 : chain[backoff_state[s]] + 1;
        if (chain[s] > lm->depth) lm->depth = chain[s];
    }
    for (int s = 0; s < n_states; ++s) {
        lm->backoff_ln[s] = lm_scaled(backoff_logw[s], a, 0.0);
        lm->final_ln[s] = final_logp ? lm_scaled(final_logp[s], a, 0.0) : 0.0;
        st[4 * s] = (int)arc_begin[s];
        st[4 * s + 1] = (int)(arc_begin[s + 1] - arc_begin[s]);
        st[4 * s + 2] = backoff_state[s];
        st[4 * s + 3] = 0;
        lm_xf(lm->backoff_ln[s], &fac[4 * s], &fac[4 * s + 1]);
        lm_xf(lm->final_ln[s], &fac[4 * s + 2], &fac[4 * s + 3]);
    }
    return lm;
}

void nntk_ngram_lm_destroy(NntkNgramLm lm) {
    if (!lm) return;
    if (lm->d_tab.p) nntk_devbuf_free(&lm->d_tab);
    if (lm->d_ln.p) nntk_devbuf_free(&lm->d_ln);
    free(lm->arc_begin); free(lm->arc_label); free(lm->arc_next); free(lm->backoff_state);
    free(lm->arc_ln); free(lm->backoff_ln); free(lm->final_ln); free(lm->tab);
    free(lm);
}

size_t nntk_ngram_lm_device_bytes(NntkNgramLm lm) {
    return lm ? 16 * ((size_t)lm->n_arcs + 2 * (size_t)lm->n_states) : 0;
}

size_t nntk_ngram_lm_rnnt_device_bytes(NntkNgramLm lm) {
    return lm ? 8 * (size_t)lm->n_arcs + 16 * (size_t)lm->n_states : 0;
}

double nntk_ngram_lm_score(NntkNgramLm lm, const int *labels, int n, int with_final) {
    nntk_shim_clear_error();
    if (!lm || n < 0 || (n > 0 && !labels)) { nntk_set_error("nntk_ngram_lm_score: NULL handle or labels, or n < 0"); return NAN; }
    double sum = 0.0;
    int s = lm->start_state;
    for (int i = 0; i < n; ++i) {
        const int c = labels[i];
        if (c < 0 || c >= lm->n_classes || c == lm->blank) { nntk_set_error("nntk_ngram_lm_score: a label is not a non-blank class"); return NAN; }
        for (;;) {
            long lo = lm->arc_begin[s], hi = lm->arc_begin[s + 1] - 1, hit = -1;
            while (lo <= hi) {
                const long mid = lo + (hi - lo) / 2;
                if (lm->arc_label[mid] == c) { hit = mid; break; }
                if (lm->arc_label[mid] < c) lo = mid + 1; else hi = mid - 1;
            }
            if (hit >= 0) { sum += lm->arc_ln[hit]; s = lm->arc_next[hit]; break; }
            if (s == 0) { sum += lm->unk_ln; break; }
            sum += lm->backoff_ln[s];
            s = lm->backoff_state[s];
        }
    }
    if (with_final) sum += lm->final_ln[s];
    return sum;
}

/* ---- for the decoders (ctc.c, rnnt_decode.c) ---- */
int nntk_ngram_lm_matches(NntkNgramLm lm, int C, int blank) { return lm->n_classes == C && lm->blank == blank; }

int nntk_ngram_lm_device(NntkNgramLm lm, nntk_shim_lm *out) {
    const size_t words = 4 * (size_t)lm->n_arcs + 8 * (size_t)lm->n_states;
    if (!lm->uploaded) {
        float *d = nntk_devbuf_reserve(&lm->d_tab, words);
        if (!d || nntk_shim_upload(d, lm->tab, words * sizeof(int))) return -1;
        lm->uploaded = 1;
        free(lm->tab);
        lm->tab = NULL;
    }
    const int *d = (const int *)lm->d_tab.p;
    out->d_arcs = d;
    out->d_states = d + 4 * (size_t)lm->n_arcs;
    out->d_factors = d + 4 * (size_t)lm->n_arcs + 4 * (size_t)lm->n_states;
    out->n_states = lm->n_states;
    out->start_state = lm->start_state;
    out->depth = lm->depth;
    out->unk_m = lm->unk_m;
    out->unk_e = lm->unk_e;
    return 0;
}

/* the transducer beam search adds natural logs in double: the unrounded values nntk_ngram_lm_score sums, next to the lookup records */
int nntk_ngram_lm_rnnt_device(NntkNgramLm lm, nntk_shim_rnnt_lm *out) {
    nntk_shim_lm tab;
    if (nntk_ngram_lm_device(lm, &tab)) return -1;
    const size_t na = (size_t)lm->n_arcs, ns = (size_t)lm->n_states;
    if (!lm->ln_uploaded) {
        double *h = (double *)malloc((na + 2 * ns) * sizeof(double));
        if (!h) NNTK_FAIL("nntk_ngram_lm: out of host memory");
        memcpy(h, lm->arc_ln, na * sizeof(double));
        for (size_t s = 0; s < ns; ++s) { h[na + 2 * s] = lm->backoff_ln[s]; h[na + 2 * s + 1] = lm->final_ln[s]; }
        float *d = nntk_devbuf_reserve(&lm->d_ln, 2 * (na + 2 * ns));
        const int rc = d ? nntk_shim_upload(d, h, (na + 2 * ns) * sizeof(double)) : -1;
        free(h);
        if (rc) return -1;
        lm->ln_uploaded = 1;
    }
    out->d_arcs = tab.d_arcs;
    out->d_states = tab.d_states;
    out->d_arc_ln = (const double *)lm->d_ln.p;
    out->d_state_ln = out->d_arc_ln + na;
    out->unk_ln = lm->unk_ln;
    out->start_state = lm->start_state;
    return 0;
}
