// rnnt_beam.hip -- RNN-Transducer beam search with the network inside the search (the contract: include/nntoolkitcore_hip.h,
// "RNN-Transducer: beam search").  One launch runs every row's whole search.
//
// Work split.  One workgroup of RD_THREADS lanes owns a row and runs its frames, depths and hypotheses; rows never talk to each other:
// no flags, no spins, no atomics.  The hypotheses of a depth go through the joiner, the vocabulary Dense and h U in groups of R
// (NNTK_RNNT_DEC_GROUP where the group's LDS fits, else 1): one pass over W_out or U serves R hypotheses, with rd_matvec's bits whatever
// R.  A frame costs at most (S + 1) ceil(W / R) passes over W_out and S ceil(W / R) over U (and the projection).
//
// LDS.  RbShared (the reductions' scratch, the depth's hypotheses C: slot, score, length, hash, max and log-sum-exp of the logits; the
// selected cells), then per group row  h [Hp] | c [Hp] | z [Jp] | buf [max(4H, V)]  (buf: gate pre-activations or logits).
//
// Workspace (global, L2-resident at these sizes; rb_layout is the layout, nntk_shim_rnnt_beam_workspace_floats its size): the rows'
// frame counts, then per row the acoustic part, the LM part with a model and the detail part with detail, in that order, so that a part
// that is absent moves none of the others.  The acoustic part:
//   bscore [W (S' + 1)] doubles      the scores of B, the hypotheses that have left the frame, in insertion order
//   states [(S' + 2) W][2H + J]      h | c | g of every hypothesis slot: A (two buffers, swapped every frame), then one level per depth
//   labels [(S' + 2) W][max_labels]  each slot's label sequence
//   meta   [(S' + 2) W][2]           its length and hash (the hash only pre-filters; equality is decided on the labels)
//   logits [W][V]                    the depth's logits, for the selection
//   bslot  [W (S' + 1)]              the slot of each entry of B
// with S' = min(max_symbols_per_frame, max_labels): a depth d holds hypotheses of at least d labels, so no deeper level is ever filled.
//
// Selection.  The W best of the depth's cells (and of B at the end of a frame) are found by W rounds of a workgroup arg-max over
// (score descending, index ascending), each round restricted to what ranks behind the round before: exact and order-stable.  Scores,
// compares and logaddexp are in double.  The LSTM step of a selected cell runs after the selection: W steps a depth.
//
// Language-model fusion (the LM = true instantiations; include/nntoolkitcore_hip.h, "Language-model fusion" under the beam search).  Every
// slot carries the state q of a backoff automaton (lmq, behind the acoustic workspace, which does not move), and the row owns
// lmterm [W][V] doubles.  Once per depth the rows of lmterm are filled by scattering the backoff chains instead of V binary searches:
// every element is marked unset; level by level (q_i, backoff(q_i), ... 0, a workgroup barrier between levels) the lanes stride over
// the arcs of hypothesis i's state of that level and an unset label takes acc + ln G(arc), acc = ((b_0 + b_1) + ...) the backoffs
// taken so far; what is still unset after state 0 takes acc + ln U.  Labels within a state are distinct and rows belong to one
// hypothesis, so nothing races, and the cost is the chain's arcs + V per hypothesis.  The same pass that fills the unknown labels adds
// the acoustic cell, (base + logp) + lnF, so the W rounds of the selection read one double a cell; -inf (a zero-mass arc, the blank, a
// hypothesis that cannot be extended) is no candidate.  next(q_i, v) is looked up for the W selected cells only, by binary search
// along the chain.  The tables are global memory; no LDS is added.  At the end the entries of A take + ln E(q), the -inf ones are
// dropped and the rest are ranked (at most 32: every entry counts the entries ahead of it); the carried A stays as it was.
//
// Label timestamps, confidences and length normalisation (the DETAIL = true instantiations; include/nntoolkitcore_hip.h, "Label
// timestamps" under the beam search).  Behind the LM part of the row's block, so that nothing else moves: per slot frames [max_labels]
// ints and lps [max_labels] floats, copied wherever labs is copied with the same loops, and per entry of B lead (a double: the largest
// single contribution so far) and bfslot (the slot whose arrays the entry reports).  The lane that merges a candidate into B compares
// it with lead and, if it is larger, points bfslot at the candidate's slot; every slot a bfslot can name (the current A buffer, the
// depth levels) lives until the end of the frame, so nothing is moved at merge time.  At the end of a frame A's entries take the
// state and labels of bslot[e] as before and the arrays of bfslot[e].  The report ranks the entries by score or, with length_norm,
// by score / (length + 1), with the LM report's counting rank on sh.cand / sh.n_score / sh.found: no LDS is added.
#include <limits.h>
#include "rnnt_dec_common.hpp"

#define RB_MAX_W NNTK_RNNT_BEAM_MAX_W

struct RbLayout {                          // offsets in floats from the row's block, each a multiple of 4
    size_t bscore, states, labels, meta, logits, bslot, row;
    size_t lmq, lmterm;                    // with a language model only, behind the acoustic layout: [(S' + 2) W] ints | [W][V] doubles
    int nslots, nbmax, SF;
};

struct RbDetailLayout {                    // with detail only, behind both: [(S' + 2) W][max_labels] ints | the same, floats | [W (S' + 1)] doubles | ints
    size_t fr, lp, lead, bfslot;
};

static RbLayout rb_layout(int H, int J, int V, int max_sym, int W, int max_labels, bool lm = false, RbDetailLayout *detail = nullptr) {
    RbLayout l;
    const int depths = max_sym < max_labels ? max_sym : max_labels;
    l.nslots = (depths + 2) * W; l.nbmax = (depths + 1) * W; l.SF = 2 * H + J;
    size_t at = 0;
    auto take = [&at](size_t n) { const size_t a = at; at += (n + 3) & ~(size_t)3; return a; };
    l.bscore = take(2 * (size_t)l.nbmax);
    l.states = take((size_t)l.nslots * l.SF);
    l.labels = take((size_t)l.nslots * max_labels);
    l.meta = take(2 * (size_t)l.nslots);
    l.logits = take((size_t)W * V);
    l.bslot = take((size_t)l.nbmax);
    l.lmq = l.lmterm = at;
    if (lm) {
        l.lmq = take((size_t)l.nslots);
        l.lmterm = take(2 * (size_t)W * V);
    }
    if (detail) {
        detail->fr = take((size_t)l.nslots * max_labels);
        detail->lp = take((size_t)l.nslots * max_labels);
        detail->lead = take(2 * (size_t)l.nbmax);
        detail->bfslot = take((size_t)l.nbmax);
    }
    l.row = at;
    return l;
}

struct RnntBeamArgs {
    const float *enc;                      // [batch][T][J]
    const float *table, *U, *proj, *out;   // as in rnnt_decode.hip
    float *ws;
    nntk_shim_rnnt_beam_state st;          // all NULL: every row from the start, nothing kept
    int *labels, *lengths;                 // [batch][nbest][max_labels] | [batch][nbest]
    float *scores;
    RbLayout lay;
    size_t ws_head;                        // floats before the first row's block: the frame counts
    int batch, T, V, blank, H, J, act, max_sym, W, nbest, max_labels;
    nntk_shim_rnnt_lm lm;                  // the LM instantiations only
    int *st_q;                             // [batch][W]: the LM states of a stream's rows (with st)
    nntk_shim_rnnt_beam_detail dt;         // the DETAIL instantiations only, as is
    RbDetailLayout dlay;                   // their part of the row's block (lay.row counts it)
};

template <int R> struct RbShared {
    double red_sum[R][RD_WAVES];
    double red_s[RD_WAVES];
    double a_score[RB_MAX_W], c_score[RB_MAX_W], c_lse[RB_MAX_W], cand[RB_MAX_W], n_score[RB_MAX_W];
    double best_s;
    float red_max[R][RD_WAVES];
    float c_max[RB_MAX_W];
    int red_i[RD_WAVES];
    int c_slot[RB_MAX_W], c_len[RB_MAX_W], n_src[RB_MAX_W], n_lab[RB_MAX_W], found[RB_MAX_W];
    unsigned c_hash[RB_MAX_W];
    int best_i, nA, nC, nB, nSel;
};

static size_t rb_lds_bytes(int R, int H, int J, int V) {
    const size_t Hp = (size_t)(H + 3) & ~(size_t)3, Jp = (size_t)(J + 3) & ~(size_t)3;
    const size_t W = 4 * (size_t)H > (size_t)V ? 4 * (size_t)H : (size_t)V, Wp = (W + 3) & ~(size_t)3;
    const size_t fixed = R == 1 ? sizeof(RbShared<1>) : sizeof(RbShared<NNTK_RNNT_DEC_GROUP>);
    return ((fixed + 15) & ~(size_t)15) + (size_t)R * (2 * Hp + Jp + Wp) * sizeof(float);
}

__device__ __forceinline__ double rb_logaddexp(double x, double y) {         // both finite
    const double m = x > y ? x : y, d = x > y ? y - x : x - y;
    return m + log1p(exp(d));
}

// next(q, v): the first state along q's backoff chain with an arc labelled v gives the arc's next state; none, state 0 included: 0
__device__ static int rb_lm_next(const nntk_shim_rnnt_lm &lm, int s, int v) {
    for (;;) {
        int lo = lm.d_states[4 * s], hi = lo + lm.d_states[4 * s + 1] - 1;
        while (lo <= hi) {
            const int mid = lo + (hi - lo) / 2, c = lm.d_arcs[4 * (size_t)mid];
            if (c == v) return lm.d_arcs[4 * (size_t)mid + 1];
            if (c < v) lo = mid + 1; else hi = mid - 1;
        }
        if (s == 0) return 0;
        s = lm.d_states[4 * s + 2];
    }
}

template <int R, bool LM, bool DETAIL>
__global__ __launch_bounds__(RD_THREADS) void rnnt_beam_kernel(const RnntBeamArgs a) {
    extern __shared__ __align__(16) unsigned char rb_smem[];
    RbShared<R> &sh = *(RbShared<R> *)rb_smem;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int H = a.H, J = a.J, V = a.V, G = 4 * H, W = a.W, ML = a.max_labels, SF = a.lay.SF;
    const int Hp = (H + 3) & ~3, Jp = (J + 3) & ~3, Wp = ((G > V ? G : V) + 3) & ~3;
    float *sh_h = (float *)(rb_smem + ((sizeof(RbShared<R>) + 15) & ~(size_t)15));
    float *sh_c = sh_h + R * Hp, *sh_z = sh_c + R * Hp, *sh_buf = sh_z + R * Jp;
    const float *pbias = a.proj ? a.proj + (size_t)H * J : nullptr;
    const float *obias = a.out + (size_t)J * V;
    const int b = blockIdx.x;
    float *row = a.ws + a.ws_head + (size_t)b * a.lay.row;
    double *bscore = (double *)(row + a.lay.bscore);
    float *states = row + a.lay.states, *lg = row + a.lay.logits;
    int *labs = (int *)(row + a.lay.labels), *meta = (int *)(row + a.lay.meta), *bslot = (int *)(row + a.lay.bslot);
    int *lmq = (int *)(row + a.lay.lmq);                                     // LM only, as is lmterm
    double *lmterm = (double *)(row + a.lay.lmterm);
    int *fr = (int *)(row + a.dlay.fr), *bfslot = (int *)(row + a.dlay.bfslot);   // DETAIL only, as are lp and lead
    float *lp = row + a.dlay.lp;
    double *lead = (double *)(row + a.dlay.lead);
    const int n = ((const int *)a.ws)[b];
    const bool started = a.st.i && a.st.i[4 * b] != 0;
    int t0 = 0;                                                              // DETAIL: the frames the row's stream has consumed
    if constexpr (DETAIL) { if (started) t0 = a.st.i[4 * b + 2]; }

    // the workgroup's best (score descending, index ascending; INT_MAX: none) -> sh.best_s, sh.best_i
    auto block_best = [&](double s, int idx) {
        for (int off = 32; off > 0; off >>= 1) {
            const double os = __shfl_xor(s, off);
            const int oi = __shfl_xor(idx, off);
            if (oi != INT_MAX && (idx == INT_MAX || os > s || (os == s && oi < idx))) { s = os; idx = oi; }
        }
        if (lane == 0) { sh.red_s[wave] = s; sh.red_i[wave] = idx; }
        __syncthreads();
        if (tid == 0) {
            s = sh.red_s[0]; idx = sh.red_i[0];
            for (int w = 1; w < RD_WAVES; ++w) {
                const double os = sh.red_s[w];
                const int oi = sh.red_i[w];
                if (oi != INT_MAX && (idx == INT_MAX || os > s || (os == s && oi < idx))) { s = os; idx = oi; }
            }
            sh.best_s = s; sh.best_i = idx;
        }
        __syncthreads();
    };

    // the prediction network for the selected cells k0 .. k0 + cnt - 1: from slot n_src (-1: the zero state) on label n_lab into slot dst0 + k
    auto step_group = [&](int k0, int cnt, int dst0) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int src = r < cnt ? sh.n_src[k0 + r] : -1;
            const float *st = states + (size_t)(src < 0 ? 0 : src) * SF;
            for (int j = tid; j < H; j += RD_THREADS) {
                sh_h[r * Hp + j] = src >= 0 ? st[j] : 0.0f;
                sh_c[r * Hp + j] = src >= 0 ? st[H + j] : 0.0f;
            }
        }
        __syncthreads();
        for (int nn = tid; nn < G; nn += RD_THREADS) {
            float hu[R];
            rd_matvec<R>(a.U, H, G, nn, sh_h, Hp, hu);
#pragma unroll
            for (int r = 0; r < R; ++r)
                if (r < cnt) sh_buf[r * Wp + nn] = a.table[(size_t)sh.n_lab[k0 + r] * G + nn] + hu[r];
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < R; ++r) {
            if (r >= cnt) continue;
            const float *zg = sh_buf + r * Wp;
            float *st = states + (size_t)(dst0 + k0 + r) * SF;
            for (int j = tid; j < H; j += RD_THREADS) {
                const float gi = rd_sigmoid(zg[j]), gf = rd_sigmoid(zg[H + j]), gg = tanhf(zg[2 * H + j]), go = rd_sigmoid(zg[3 * H + j]);
                const float c = gf * sh_c[r * Hp + j] + gi * gg;
                const float h = go * tanhf(c);
                sh_h[r * Hp + j] = h;
                st[j] = h; st[H + j] = c;
            }
        }
        __syncthreads();
        for (int j = tid; j < J; j += RD_THREADS) {
            if (a.proj) {
                float ph[R];
                rd_matvec<R>(a.proj, H, J, j, sh_h, Hp, ph);
#pragma unroll
                for (int r = 0; r < R; ++r)
                    if (r < cnt) states[(size_t)(dst0 + k0 + r) * SF + 2 * H + j] = ph[r] + pbias[j];
            } else {
#pragma unroll
                for (int r = 0; r < R; ++r)
                    if (r < cnt) states[(size_t)(dst0 + k0 + r) * SF + 2 * H + j] = sh_h[r * Hp + j];
            }
        }
        __syncthreads();
    };

    // frame t for the hypotheses i0 .. i0 + cnt - 1 of C: the logits (kept in the workspace when cells will be selected), their max and
    // log-sum-exp, and the score of the hypothesis leaving the frame by a blank
    auto logits_group = [&](int i0, int cnt, int t, bool keep) {
        const float *e = a.enc + ((size_t)b * a.T + t) * J;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            if (r < cnt) {
                const float *g = states + (size_t)sh.c_slot[i0 + r] * SF + 2 * H;
                for (int j = tid; j < J; j += RD_THREADS) sh_z[r * Jp + j] = rd_act(a.act, e[j] + g[j]);
            } else {
                for (int j = tid; j < J; j += RD_THREADS) sh_z[r * Jp + j] = 0.0f;
            }
        }
        __syncthreads();
        float m[R];
#pragma unroll
        for (int r = 0; r < R; ++r) m[r] = -INFINITY;
        for (int nn = tid; nn < V; nn += RD_THREADS) {
            float x[R];
            rd_matvec<R>(a.out, J, V, nn, sh_z, Jp, x);
#pragma unroll
            for (int r = 0; r < R; ++r) {
                x[r] += obias[nn];
                sh_buf[r * Wp + nn] = x[r];
                if (x[r] > m[r]) m[r] = x[r];
                if (keep && r < cnt) lg[(size_t)(i0 + r) * V + nn] = x[r];
            }
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            for (int off = 32; off > 0; off >>= 1) {
                const float om = __shfl_xor(m[r], off);
                if (om > m[r]) m[r] = om;
            }
            if (lane == 0) sh.red_max[r][wave] = m[r];
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < R; ++r) {
            m[r] = sh.red_max[r][0];
            for (int w = 1; w < RD_WAVES; ++w) {
                const float om = sh.red_max[r][w];
                if (om > m[r]) m[r] = om;
            }
            const double sum = rd_wave_sum_exp(sh_buf + r * Wp, V, tid, m[r]);
            if (lane == 0) sh.red_sum[r][wave] = sum;
            if (tid == 0 && r < cnt) sh.c_max[i0 + r] = m[r];
        }
        __syncthreads();
        if (tid < cnt) {
            const int r = tid, i = i0 + r;
            double sum = 0.0;
            for (int w = 0; w < RD_WAVES; ++w) sum += sh.red_sum[r][w];
            const double lse = log(sum);
            sh.c_lse[i] = lse;
            sh.cand[i] = sh.c_score[i] + ((double)(sh_buf[r * Wp + a.blank] - sh.c_max[i]) - lse);
        }
        __syncthreads();
    };

    int cur = 0;                                                             // which of the two A buffers holds A
    for (int i = tid; i < R * (2 * Hp + Jp); i += RD_THREADS) sh_h[i] = 0.0f;
    if (started) {
        const int nA = a.st.i[4 * b + 1];
        const size_t at = (size_t)b * W;
        for (int i = tid; i < nA * SF; i += RD_THREADS) states[i] = a.st.f[at * SF + i];
        for (int k = 0; k < nA; ++k) {
            const int len = a.st.meta[2 * (at + k)];
            for (int j = tid; j < len; j += RD_THREADS) labs[(size_t)k * ML + j] = a.st.lab[(at + k) * ML + j];
            if constexpr (DETAIL) {
                if (a.dt.d_st_fr)
                    for (int j = tid; j < len; j += RD_THREADS) {
                        fr[(size_t)k * ML + j] = a.dt.d_st_fr[(at + k) * ML + j];
                        lp[(size_t)k * ML + j] = a.dt.d_st_lp[(at + k) * ML + j];
                    }
            }
        }
        if (tid < nA) {
            meta[2 * tid] = a.st.meta[2 * (at + tid)]; meta[2 * tid + 1] = a.st.meta[2 * (at + tid) + 1];
            sh.a_score[tid] = a.st.score[at + tid];
            if constexpr (LM) lmq[tid] = a.st_q[at + tid];
        }
        if (tid == 0) sh.nA = nA;
        __syncthreads();
    } else {
        if (tid == 0) { meta[0] = 0; meta[1] = 0; sh.a_score[0] = 0.0; sh.n_src[0] = -1; sh.n_lab[0] = a.blank; sh.nA = 1; }
        if constexpr (LM) { if (tid == 0) lmq[0] = a.lm.start_state; }
        __syncthreads();
        step_group(0, 1, 0);                                                 // the step on embed[blank] from the zero state
    }

    for (int t = 0; t < n; ++t) {
        const int nA = sh.nA;
        if (nA == 0) break;
        __syncthreads();
        if (tid < nA) {
            const int slot = cur * W + tid;
            sh.c_slot[tid] = slot; sh.c_score[tid] = sh.a_score[tid]; sh.c_len[tid] = meta[2 * slot]; sh.c_hash[tid] = (unsigned)meta[2 * slot + 1];
        }
        if (tid == 0) { sh.nC = nA; sh.nB = 0; }
        __syncthreads();
        for (int depth = 0;; ++depth) {
            const int nC = sh.nC, nB = sh.nB;
            const bool last = depth == a.max_sym;
            for (int i0 = 0; i0 < nC; i0 += R) logits_group(i0, nC - i0 < R ? nC - i0 : R, t, !last);
            // a hypothesis leaves the frame: the entry of B with its label sequence, if there is one (the depth's own are distinct)
            for (int i = wave; i < nC; i += RD_WAVES) {
                int f = -1;
                if (sh.cand[i] > -INFINITY) {
                    const int len = sh.c_len[i];
                    const int *q = labs + (size_t)sh.c_slot[i] * ML;
                    for (int e = lane; e < nB; e += 64) {
                        const int s = bslot[e];
                        if (meta[2 * s] != len || (unsigned)meta[2 * s + 1] != sh.c_hash[i]) continue;
                        const int *p = labs + (size_t)s * ML;
                        bool eq = true;
                        for (int j = 0; j < len; ++j)
                            if (p[j] != q[j]) { eq = false; break; }
                        if (eq) f = e;
                    }
                    for (int off = 32; off > 0; off >>= 1) {
                        const int of = __shfl_xor(f, off);
                        if (of > f) f = of;
                    }
                }
                if (lane == 0) sh.found[i] = f;
            }
            __syncthreads();
            if (tid == 0) {
                int nb = nB;
                for (int i = 0; i < nC; ++i) {
                    const double cs = sh.cand[i];
                    if (!(cs > -INFINITY)) continue;
                    const int f = sh.found[i];
                    if constexpr (DETAIL) {                                  // the dominant contributor's arrays; a tie keeps what is there
                        if (f >= 0) { if (cs > lead[f]) { lead[f] = cs; bfslot[f] = sh.c_slot[i]; } }
                        else if (nb < a.lay.nbmax) { lead[nb] = cs; bfslot[nb] = sh.c_slot[i]; }
                    }
                    if (f >= 0) bscore[f] = rb_logaddexp(bscore[f], cs);
                    else if (nb < a.lay.nbmax) { bslot[nb] = sh.c_slot[i]; bscore[nb] = cs; ++nb; }
                }
                sh.nB = nb;
            }
            __syncthreads();
            if (last) break;
            // the W best label cells (i, v), v != blank
            double prev_s = INFINITY;
            int prev_i = -1, nSel = 0;
            if constexpr (LM) {
                // lmterm[i][v] = ln F(q_i, v) by scattering q_i's backoff chain, then the fused score of the cell in its place
                for (int idx = tid; idx < nC * V; idx += RD_THREADS) lmterm[idx] = NAN;      // unset (no table value is a NaN)
                __syncthreads();
                for (int level = 0;; ++level) {
                    bool more = false;
                    for (int i = 0; i < nC; ++i) {
                        int s = lmq[sh.c_slot[i]], l = 0;
                        double acc = 0.0;
                        for (; l < level && s != 0; ++l) { acc += a.lm.d_state_ln[2 * s]; s = a.lm.d_states[4 * s + 2]; }
                        if (l < level) continue;                             // the chain ended at state 0, levels ago
                        more |= s != 0;
                        const int first = a.lm.d_states[4 * s], cnt = a.lm.d_states[4 * s + 1];
                        for (int q = tid; q < cnt; q += RD_THREADS) {
                            double *cell = lmterm + (size_t)i * V + a.lm.d_arcs[4 * (size_t)(first + q)];
                            if (*cell != *cell) *cell = acc + a.lm.d_arc_ln[first + q];
                        }
                    }
                    __syncthreads();
                    if (!more) break;
                }
                for (int i = 0; i < nC; ++i) {
                    const double base = sh.c_score[i], lse = sh.c_lse[i];
                    const bool open = sh.c_len[i] < ML && base > -INFINITY;
                    const float mx = sh.c_max[i];
                    double acc = 0.0;
                    for (int s = lmq[sh.c_slot[i]]; s != 0; s = a.lm.d_states[4 * s + 2]) acc += a.lm.d_state_ln[2 * s];
                    for (int v = tid; v < V; v += RD_THREADS) {
                        const double t = lmterm[(size_t)i * V + v];
                        const double f = (base + ((double)(lg[(size_t)i * V + v] - mx) - lse)) + (t != t ? acc + a.lm.unk_ln : t);
                        lmterm[(size_t)i * V + v] = open && v != a.blank ? f : -INFINITY;
                    }
                }
                __syncthreads();
            }
            for (int k = 0; k < W; ++k) {
                double bs = -INFINITY;
                int bi = INT_MAX;
                if constexpr (LM) {
                    for (int idx = tid; idx < nC * V; idx += RD_THREADS) {
                        const double s = lmterm[idx];
                        if (!(s > -INFINITY)) continue;                      // no candidate
                        if ((s < prev_s || (s == prev_s && idx > prev_i)) && (bi == INT_MAX || s > bs)) { bs = s; bi = idx; }
                    }
                } else {
                for (int i = 0; i < nC; ++i) {
                    const double base = sh.c_score[i], lse = sh.c_lse[i];
                    if (!(sh.c_len[i] < ML && base > -INFINITY)) continue;
                    const float mx = sh.c_max[i];
                    for (int v = tid; v < V; v += RD_THREADS) {
                        if (v == a.blank) continue;
                        const double s = base + ((double)(lg[(size_t)i * V + v] - mx) - lse);
                        const int idx = i * V + v;
                        if ((s < prev_s || (s == prev_s && idx > prev_i)) && (bi == INT_MAX || s > bs)) { bs = s; bi = idx; }
                    }
                }
                }
                block_best(bs, bi);
                if (sh.best_i == INT_MAX) break;
                prev_s = sh.best_s; prev_i = sh.best_i;
                if (tid == 0) { sh.n_src[k] = prev_i / V; sh.n_lab[k] = prev_i % V; sh.n_score[k] = prev_s; }
                ++nSel;
            }
            if (nSel == 0) break;
            __syncthreads();
            // the cells become the next depth's C, in the level of slots that belongs to this depth
            const int dst0 = (2 + depth) * W;
            int ss = 0, ol = 0;
            unsigned oh = 0;
            float nlp = 0.0f;                                                // DETAIL: the cell's acoustic log-probability
            if (tid < nSel) { const int i = sh.n_src[tid]; ss = sh.c_slot[i]; ol = sh.c_len[i]; oh = sh.c_hash[i]; }
            if constexpr (DETAIL) {
                if (tid < nSel) {
                    const int i = sh.n_src[tid];
                    nlp = (float)((double)(lg[(size_t)i * V + sh.n_lab[tid]] - sh.c_max[i]) - sh.c_lse[i]);
                }
            }
            __syncthreads();
            if (tid < nSel) {
                const unsigned nh = oh * 1000003u + (unsigned)(sh.n_lab[tid] + 1);
                sh.n_src[tid] = ss; sh.c_slot[tid] = dst0 + tid; sh.c_score[tid] = sh.n_score[tid]; sh.c_len[tid] = ol + 1; sh.c_hash[tid] = nh;
                meta[2 * (dst0 + tid)] = ol + 1; meta[2 * (dst0 + tid) + 1] = (int)nh;
                if constexpr (LM) lmq[dst0 + tid] = rb_lm_next(a.lm, lmq[ss], sh.n_lab[tid]);
            }
            if (tid == 0) sh.nC = nSel;
            __syncthreads();
            for (int k = 0; k < nSel; ++k) {
                const int L = sh.c_len[k] - 1;
                const int *p = labs + (size_t)sh.n_src[k] * ML;
                int *q = labs + (size_t)sh.c_slot[k] * ML;
                for (int j = tid; j < L; j += RD_THREADS) q[j] = p[j];
                if (tid == 0) q[L] = sh.n_lab[k];
                if constexpr (DETAIL) {
                    const size_t from = (size_t)sh.n_src[k] * ML, to = (size_t)sh.c_slot[k] * ML;
                    for (int j = tid; j < L; j += RD_THREADS) { fr[to + j] = fr[from + j]; lp[to + j] = lp[from + j]; }
                }
            }
            if constexpr (DETAIL) {
                if (tid < nSel) { fr[(size_t)(dst0 + tid) * ML + ol] = t0 + t; lp[(size_t)(dst0 + tid) * ML + ol] = nlp; }
            }
            for (int k0 = 0; k0 < nSel; k0 += R) step_group(k0, nSel - k0 < R ? nSel - k0 : R, dst0);
        }
        // A = the W best of B (score descending, insertion index ascending), into the other A buffer
        const int nB = sh.nB;
        double prev_s = INFINITY;
        int prev_i = -1, nNew = 0;
        for (int k = 0; k < W; ++k) {
            double bs = -INFINITY;
            int bi = INT_MAX;
            for (int e = tid; e < nB; e += RD_THREADS) {
                const double s = bscore[e];
                if ((s < prev_s || (s == prev_s && e > prev_i)) && (bi == INT_MAX || s > bs)) { bs = s; bi = e; }
            }
            block_best(bs, bi);
            if (sh.best_i == INT_MAX) break;
            prev_s = sh.best_s; prev_i = sh.best_i;
            if (tid == 0) { sh.n_src[k] = bslot[prev_i]; sh.a_score[k] = prev_s; }
            if constexpr (DETAIL) { if (tid == 0) sh.n_lab[k] = bfslot[prev_i]; }
            ++nNew;
        }
        __syncthreads();
        cur ^= 1;
        for (int k = 0; k < nNew; ++k) {
            const int src = sh.n_src[k], dst = cur * W + k, len = meta[2 * src];
            for (int j = tid; j < SF; j += RD_THREADS) states[(size_t)dst * SF + j] = states[(size_t)src * SF + j];
            for (int j = tid; j < len; j += RD_THREADS) labs[(size_t)dst * ML + j] = labs[(size_t)src * ML + j];
            if (tid == 0) { meta[2 * dst] = len; meta[2 * dst + 1] = meta[2 * src + 1]; }
            if constexpr (LM) { if (tid == 0) lmq[dst] = lmq[src]; }
            if constexpr (DETAIL) {
                const size_t from = (size_t)sh.n_lab[k] * ML;
                for (int j = tid; j < len; j += RD_THREADS) { fr[(size_t)dst * ML + j] = fr[from + j]; lp[(size_t)dst * ML + j] = lp[from + j]; }
            }
        }
        if (tid == 0) sh.nA = nNew;
        __syncthreads();
    }

    const int nA = sh.nA;
    if constexpr (DETAIL) {
        // the report: the score (with a model: + ln E(q), the -inf entries dropped) in sh.cand, the key it is ranked by in sh.n_score
        __syncthreads();
        if (tid < nA) {
            double s = sh.a_score[tid];
            if constexpr (LM) s += a.lm.d_state_ln[2 * lmq[cur * W + tid] + 1];
            sh.cand[tid] = s;
            sh.n_score[tid] = a.dt.length_norm ? s / (double)(meta[2 * (cur * W + tid)] + 1) : s;
        }
        __syncthreads();
        if (tid < nA) {
            const double s = sh.n_score[tid];
            int ahead = 0;
            for (int j = 0; j < nA; ++j) {
                const double o = sh.n_score[j];
                ahead += o > -INFINITY && (o > s || (o == s && j < tid));
            }
            if (s > -INFINITY) sh.found[ahead] = tid;
        }
        if (tid == 0) {
            int kept = 0;
            for (int j = 0; j < nA; ++j) kept += sh.n_score[j] > -INFINITY;
            sh.nSel = kept;
        }
        __syncthreads();
        const int kept = sh.nSel;
        for (int k = 0; k < a.nbest; ++k) {
            const size_t o = (size_t)b * a.nbest + k;
            const int src = k < kept ? sh.found[k] : 0, slot = cur * W + src, len = k < kept ? meta[2 * slot] : 0;
            for (int j = tid; j < ML; j += RD_THREADS) {
                a.labels[o * ML + j] = j < len ? labs[(size_t)slot * ML + j] : -1;
                if (a.dt.d_frames) a.dt.d_frames[o * ML + j] = j < len ? fr[(size_t)slot * ML + j] : -1;
                if (a.dt.d_logps) a.dt.d_logps[o * ML + j] = j < len ? lp[(size_t)slot * ML + j] : 0.0f;
            }
            if (tid == 0) {
                a.lengths[o] = k < kept ? len : -1;
                a.scores[o] = k < kept ? (float)sh.cand[src] : -INFINITY;
            }
        }
    } else if constexpr (LM) {
        // the report: + ln E(q), the -inf entries dropped, the rest ranked descending, ties to the lower rank in A; A itself stays
        __syncthreads();
        if (tid < nA) sh.cand[tid] = sh.a_score[tid] + a.lm.d_state_ln[2 * lmq[cur * W + tid] + 1];
        __syncthreads();
        if (tid < nA) {
            const double s = sh.cand[tid];
            int ahead = 0;
            for (int j = 0; j < nA; ++j) {
                const double o = sh.cand[j];
                ahead += o > -INFINITY && (o > s || (o == s && j < tid));
            }
            if (s > -INFINITY) sh.found[ahead] = tid;
        }
        if (tid == 0) {
            int kept = 0;
            for (int j = 0; j < nA; ++j) kept += sh.cand[j] > -INFINITY;
            sh.nSel = kept;
        }
        __syncthreads();
        const int kept = sh.nSel;
        for (int k = 0; k < a.nbest; ++k) {
            const size_t o = (size_t)b * a.nbest + k;
            const int src = k < kept ? sh.found[k] : 0, slot = cur * W + src, len = k < kept ? meta[2 * slot] : 0;
            for (int j = tid; j < ML; j += RD_THREADS) a.labels[o * ML + j] = j < len ? labs[(size_t)slot * ML + j] : -1;
            if (tid == 0) {
                a.lengths[o] = k < kept ? len : -1;
                a.scores[o] = k < kept ? (float)sh.cand[src] : -INFINITY;
            }
        }
    } else {
    for (int k = 0; k < a.nbest; ++k) {
        const size_t o = (size_t)b * a.nbest + k;
        const int slot = cur * W + k, len = k < nA ? meta[2 * slot] : 0;
        for (int j = tid; j < ML; j += RD_THREADS) a.labels[o * ML + j] = j < len ? labs[(size_t)slot * ML + j] : -1;
        if (tid == 0) {
            a.lengths[o] = k < nA ? len : -1;
            a.scores[o] = k < nA ? (float)sh.a_score[k] : -INFINITY;
        }
    }
    }
    if (a.st.i) {
        const size_t at = (size_t)b * W;
        for (int i = tid; i < nA * SF; i += RD_THREADS) a.st.f[at * SF + i] = states[(size_t)cur * W * SF + i];
        for (int k = 0; k < nA; ++k) {
            const int slot = cur * W + k, len = meta[2 * slot];
            for (int j = tid; j < len; j += RD_THREADS) a.st.lab[(at + k) * ML + j] = labs[(size_t)slot * ML + j];
            if constexpr (DETAIL) {
                if (a.dt.d_st_fr)
                    for (int j = tid; j < len; j += RD_THREADS) {
                        a.dt.d_st_fr[(at + k) * ML + j] = fr[(size_t)slot * ML + j];
                        a.dt.d_st_lp[(at + k) * ML + j] = lp[(size_t)slot * ML + j];
                    }
            }
        }
        if (tid < nA) {
            const int slot = cur * W + tid;
            a.st.meta[2 * (at + tid)] = meta[2 * slot]; a.st.meta[2 * (at + tid) + 1] = meta[2 * slot + 1];
            a.st.score[at + tid] = sh.a_score[tid];
            if constexpr (LM) a.st_q[at + tid] = lmq[slot];
        }
        if (tid == 0) { a.st.i[4 * b] = 1; a.st.i[4 * b + 1] = nA; }
        if constexpr (DETAIL) { if (tid == 0) a.st.i[4 * b + 2] = t0 + n; }
    }
}

typedef void (*RbKernel)(const RnntBeamArgs);

template <int R> static RbKernel rb_kernel(bool lm, bool detail) {
    static const RbKernel k[2][2] = { { rnnt_beam_kernel<R, false, false>, rnnt_beam_kernel<R, false, true> },
                                      { rnnt_beam_kernel<R, true, false>, rnnt_beam_kernel<R, true, true> } };
    return k[lm][detail];
}

static int rb_launch(RbKernel k, const RnntBeamArgs &a, size_t lds) {
    if (lds > 48 * 1024 && nntk_set_max_dynamic_lds((const void *)k, lds)) return -1;
    hipLaunchKernelGGL(k, dim3((unsigned)a.batch), dim3(RD_THREADS), lds, nntk_stream(), a);
    return 0;
}

static int rb_forced_group = 0;

extern "C" {

size_t nntk_shim_rnnt_beam_workspace_floats(int batch, int H, int J, int V, int max_sym, int beam_width, int max_labels, int with_lm,
                                            int with_detail) {
    if (batch <= 0) return 0;
    RbDetailLayout dl;
    return (((size_t)batch + 3) & ~(size_t)3) +
           (size_t)batch * rb_layout(H, J, V, max_sym, beam_width, max_labels, with_lm != 0, with_detail ? &dl : nullptr).row;
}

int nntk_shim_rnnt_beam_fits(int H, int J, int V) { return rb_lds_bytes(1, H, J, V) <= RD_LDS_MAX; }

int nntk_shim_rnnt_beam_group(int beam_width, int H, int J, int V) {
    const bool fits = rb_lds_bytes(NNTK_RNNT_DEC_GROUP, H, J, V) <= RD_LDS_MAX;
    if (rb_forced_group) return rb_forced_group == NNTK_RNNT_DEC_GROUP && fits ? NNTK_RNNT_DEC_GROUP : 1;
    return beam_width > 1 && fits ? NNTK_RNNT_DEC_GROUP : 1;
}

void nntk_shim_rnnt_beam_set_group(int group) { rb_forced_group = group == 1 || group == NNTK_RNNT_DEC_GROUP ? group : 0; }

int nntk_shim_rnnt_beam(const nntk_shim_rnnt_dec *m, const float *d_enc, int batch, int T, const int *h_n_frames, int beam_width, int nbest,
                        int max_labels, const nntk_shim_rnnt_beam_state *st, const nntk_shim_rnnt_lm *lm, int *d_st_q,
                        const nntk_shim_rnnt_beam_detail *dt, int *d_labels, int *d_lengths, float *d_scores, float *d_ws) {
    if (batch <= 0) return 0;
    const int depths = m->max_symbols_per_frame < max_labels ? m->max_symbols_per_frame : max_labels;
    if (m->E < 1 || m->H < 1 || m->J < 1 || m->V < 2 || m->H > NNTK_RNNT_DEC_MAX_WIDTH || m->J > NNTK_RNNT_DEC_MAX_WIDTH ||
        m->V > NNTK_RNNT_DEC_MAX_V || !nntk_shim_rnnt_beam_fits(m->H, m->J, m->V) || beam_width < 1 || beam_width > RB_MAX_W ||
        (size_t)(depths + 2) * beam_width > (size_t)INT_MAX / 4)
        return nntk_fail_msg("nntk_rnnt_beam_decode_device: the model is beyond the decoding kernel's limits");
    if (nntk_shim_upload_ints((int *)d_ws, h_n_frames, batch)) return -1;
    RnntBeamArgs a;
    a.enc = d_enc; a.table = m->d_table; a.U = m->d_U; a.proj = m->d_proj; a.out = m->d_out;
    a.ws = d_ws;
    a.st = st ? *st : nntk_shim_rnnt_beam_state();
    a.lm = lm ? *lm : nntk_shim_rnnt_lm();
    a.dt = dt ? *dt : nntk_shim_rnnt_beam_detail();
    a.st_q = st ? d_st_q : nullptr;            // what a stream carries besides st is dropped without one
    if (!st) a.dt.d_st_fr = nullptr, a.dt.d_st_lp = nullptr;
    a.labels = d_labels; a.lengths = d_lengths; a.scores = d_scores;
    a.dlay = RbDetailLayout();
    a.lay = rb_layout(m->H, m->J, m->V, m->max_symbols_per_frame, beam_width, max_labels, lm != nullptr, dt ? &a.dlay : nullptr);
    a.ws_head = ((size_t)batch + 3) & ~(size_t)3;
    a.batch = batch; a.T = T; a.V = m->V; a.blank = m->blank; a.H = m->H; a.J = m->J; a.act = m->activation;
    a.max_sym = m->max_symbols_per_frame; a.W = beam_width; a.nbest = nbest; a.max_labels = max_labels;
    const int R = nntk_shim_rnnt_beam_group(beam_width, m->H, m->J, m->V);
    const RbKernel k = R == 1 ? rb_kernel<1>(lm != nullptr, dt != nullptr) : rb_kernel<NNTK_RNNT_DEC_GROUP>(lm != nullptr, dt != nullptr);
    if (rb_launch(k, a, rb_lds_bytes(R, m->H, m->J, m->V))) return -1;
    NNTK_LAUNCH_CHECK("rnnt_beam_kernel");
    return 0;
}

}  // extern "C"
