// rnnt_tdt_beam.hip -- beam search for a token-and-duration transducer (TDT) with the network inside the search (the contract:
// include/nntoolkitcore_hip.h, "RNN-Transducer: token-and-duration beam search").  One launch runs every row's whole search.
//
// Why not rnnt_beam.hip on a [J][V + D] block.  The classic search is frame-synchronous: one set A enters frame t, one set B leaves it.
// Here a move carries a duration, so the hypotheses that leave frame t land on t + 1 .. t + Dmax, and a frame nobody lands on is never
// joined.  The search therefore keeps BUCKETS, one list of (score, slot) per future frame, instead of A and B.
//
// Work split.  One workgroup of RD_THREADS lanes owns a row and runs its frames, depths and hypotheses; rows never talk to each other:
// no flags, no spins, no atomics.  The hypotheses of a depth go through the joiner, the [J][V + D] block and h U in groups of R
// (NNTK_RNNT_DEC_GROUP where the group's LDS fits, else 1) with rd_matvec's bits whatever R.  A lane owns column n of [0, V + D), so both
// heads land in LDS in one pass; the token head's max and sum-exp cover [0, V) with the reductions of rnnt_dec_common.hpp, the duration
// head (at most 8 values) is reduced serially by one lane per hypothesis -- lane RD_THREADS - 1 - r, while the others sum the token
// head -- exactly as rnnt_tdt_decode.hip does, and leaves lp_dur [D] doubles in LDS.  These products are matrix-vector products for at
// most 4 hypotheses, bound to the greedy kernel's four fmaf chains: no matrix instructions.
//
// The ring.  A slot (h | c | g, labels, length, hash) written in frame t is referenced by buckets up to t + Dmax, so the slots form a
// ring of Dmax + 1 frames of (S' + 2) W slots, S' = min(max_symbols_per_frame, max_labels): level 0 the frame's C, one level per depth
// for the selected cells.  The buckets form a ring of Dmax + 1 lists; frame t uses position t mod (Dmax + 1) of both.  bucket[n] sits
// where n would: the clamp min(t + d, n) only redirects moves into it.  At the start of frame t the W best of bucket[t] are copied into
// frame t's level 0 from frames t - Dmax .. t - 1, which are other ring positions; the bucket is then empty for frame t + Dmax + 1.  An
// empty bucket[t] skips the frame before any barrier.  A bucket holds at most 2 W (S' + 1) Dmax entries: a source frame contributes at
// most W (S' + 1) blank entries (equal label sequences merge) and W (S' + 1) selected cells, and Dmax source frames reach one bucket.
// The initial hypothesis lives in the ring position of frame -1.
//
// Selection.  The W best of the W V D cells are found by W rounds of a workgroup arg-max over (score descending, index (i V + v) D + k
// ascending), each round restricted to what ranks behind the round before.  The score separates, base_i + (lp_tok[i][v] + lp_dur[i][k]):
// a lane reads its columns' logits from the workspace and the hypothesis's D values of lp_dur from LDS; no [W][V][D] array exists.  Two
// selected cells (i, v, k) and (i, v, k') are the same hypothesis up to score and landing frame: they share ONE slot and one LSTM step.
//
// Merging.  A move into a bucket looks for its label sequence there: one wavefront per candidate scans the bucket (length and hash
// pre-filter, equality on the labels), then lane 0 of the workgroup applies the candidates in order -- logaddexp into the entry found, or
// append.  Two candidates of one phase can only share a label sequence by sharing a slot (one hypothesis, two durations, both clamped to
// n); the applying lane finds that twin among the entries the phase appended to bucket[n].
//
// Barriers per depth, nC hypotheses in C, W' cells selected, U of them distinct steps: 4 ceil(nC / R) (z | max parts | sum parts and the
// duration head | lp ready) + 1 + 2 (blank moves: built | found | applied) + 2 a round, W' + 1 rounds at most, + 1 + 3 (twins | slots | lists) +
// 4 ceil(U / R) (the classic step) + 2 (label moves).  A joined frame adds 2 W + 3 for its C and its end; a skipped frame adds none.
//
// LDS.  TbShared (the reductions' scratch; C: slot, score, length, hash, max, log-sum-exp, lp_blank, lp_dur [W][8] doubles; the selected
// cells; the candidates of a phase, W * 8 of them; the buckets' counts), 10.8 KiB at R = 4, then per group row
// h [Hp] | c [Hp] | z [Jp] | buf [max(4H, V + D)]: the classic beam's layout with V + D in V's place.  H = J = 640, V = 1024, D = 5,
// R = 4: 10.8 + 4 * 17.5 = 80.8 KiB.
//
// Workspace (tb_layout; nntk_shim_rnnt_tdt_beam_workspace_floats): the rows' frame counts, two counters per row (frames joined | LSTM
// steps, for the timing tool), then per row  bscore [Dmax + 1][cap] doubles | bslot [Dmax + 1][cap] | states [slots][2H + J] |
// labels [slots][max_labels] | meta [slots][2] | logits [W][V],  cap = 2 W (S' + 1) Dmax, slots = (Dmax + 1)(S' + 2) W.
//
// Language-model fusion (the LM = true instantiations; include/nntoolkitcore_hip.h, the options under the TDT beam search).  The state q
// of the backoff automaton is one word per slot of the ring (lmq, behind the acoustic workspace, which does not move): a bucket entry's
// q is its slot's, and equal label sequences have equal q, so merging needs no rule.  The selection's score still separates,
// (base_i + (lp_tok[i][v] + lp_dur[i][k])) + lnF[i][v], and lnF does not depend on k: before the W rounds of a depth the row's
// lmterm [W][V] doubles are filled, one walk per (i, v) whatever D, by scattering q_i's backoff chain as rnnt_beam.hip does (every
// element marked unset; level by level, a barrier between levels, the lanes stride over the arcs of hypothesis i's state of that level
// and an unset label takes acc + ln G(arc); what is still unset after state 0 takes acc + ln U).  A round reads one more double per
// (i, v) and adds it last, in the header's order; a cell at -inf is no candidate, as before.  next(q_i, v) is looked up for the first
// selected cell of each (i, v) only, with its slot.  No LDS is added.
//
// Label frames, durations, confidences and length normalisation (the DETAIL = true instantiations).  Behind the LM part: per slot
// fr | du | lp [max_labels], copied wherever labs is copied; per bucket entry lead (the largest single contribution), bfslot (the slot
// whose arrays it reports: a reference, not a copy -- that slot was written at most Dmax frames before the bucket is consumed, so it is
// still on the ring) and bdur; per candidate of a phase cld.  Twins -- two selected cells (i, v, k), (i, v, k') -- share a slot and so
// fr and lp, but not the last label's duration: that one value rides with the candidate (cld) and the bucket entry (bdur), and reaches
// a slot's du only when the entry is copied into a frame's level 0 or reported.  A new slot's own last du is 0: what its hypothesis
// took if it joins the next C, which only a duration-0 cell does.  The lane that applies a candidate compares it with lead and, if
// it is larger, points bfslot and bdur at the candidate; the twin found in bucket[n] comes by the same lines.  The report (also the LM
// one) takes the W best of bucket[n] and ranks them by score or score / (length + 1), every entry counting the entries ahead of it, on
// arrays of TbShared that the frames have left free: no LDS is added, so tb_lds_bytes, fits and group hold for every instantiation.
//
// Streaming (the STREAM = true instantiations; include/nntoolkitcore_hip.h, "streamed" under the TDT beam search).  A push has seen N
// frames of its row and does not know the row's end, and a frame t with t + Dmax > N makes clamped moves into bucket[N], whose
// insertion order interleaves several source frames: carrying the ring alone cannot give the one-shot bits.  So the same frame loop runs
// twice.  The committed frames [c_old, c_new), c = max(0, N - Dmax + 1), have t + Dmax <= N: min(t + d, n) is t + d for every end
// n >= N, and what they write is what every longer one-shot call writes.  They run on the CARRIED block of the row (tb_layout's row
// block in the stream's state, ring positions t mod (Dmax + 1) on the absolute frame) between a restore and a save of sh.nb.  Then
// the workgroup copies the block into the call's workspace -- everything but logits and lmterm, which a depth fills before it reads
// them -- re-points its row pointers at the copy, and runs the at most Dmax - 1 tail frames [c_new, N) with the clamp n = N and the
// report there.  Every index in a block (slot, entry) is relative to it, so the copy is a search of its own; the carried block never
// sees a clamped move, and the next push runs the tail's frames again, committed or as its own tail.  Those frames' encoder vectors
// are held in the state, frame t at position t mod (Dmax - 1): a frame seen by an earlier push is read from there, a later one from
// the chunk, and the tail's new frames are copied in (as bits) between the two phases, when the committed phase has read what they
// replace.  The first push after create or reset sets up frame -1 and the blank step; the host sends that flag and the frames seen
// before in the two counter words of the row, which the kernel reads before it writes them.  No LDS is added, no atomics, one launch.
#include <limits.h>
#include <stdlib.h>
#include "rnnt_dec_common.hpp"

#define TB_MAX_W NNTK_RNNT_BEAM_MAX_W
#define TB_MAX_D NNTK_RNNT_TDT_MAX_DURATIONS
#define TB_MAX_RING (NNTK_RNNT_TDT_MAX_DURATION + 1)

struct TbLayout {                          // offsets in floats from the row's block, each a multiple of 4
    size_t bscore, bslot, states, labels, meta, logits, row;
    int frame_slots, cap, SF, depths;      // slots a frame, entries a bucket, floats of a state, S'
};

struct TbOptLayout {                       // behind the acoustic layout, which does not move; a part that is absent takes no room
    size_t lmq, lmterm;                    // with a language model: [slots] ints | [W][V] doubles
    size_t fr, du, lp;                     // with detail, per slot: [max_labels] ints | ints | floats
    size_t lead, bfslot, bdur;             // ... per bucket entry: [Dmax + 1][cap] doubles | ints | ints
    size_t cld;                            // ... per candidate of a phase: [W * 8] ints, its last label's duration
};

static TbLayout tb_layout(int H, int J, int V, int max_sym, int dmax, int W, int max_labels, bool lm = false, bool detail = false,
                          TbOptLayout *opt = nullptr) {
    TbLayout l;
    TbOptLayout o = TbOptLayout();
    l.depths = max_sym < max_labels ? max_sym : max_labels;
    l.frame_slots = (l.depths + 2) * W; l.cap = 2 * W * (l.depths + 1) * dmax; l.SF = 2 * H + J;
    const size_t ring = (size_t)dmax + 1, slots = ring * l.frame_slots;
    size_t at = 0;
    auto take = [&at](size_t n) { const size_t a = at; at += (n + 3) & ~(size_t)3; return a; };
    l.bscore = take(2 * ring * l.cap);
    l.bslot = take(ring * l.cap);
    l.states = take(slots * l.SF);
    l.labels = take(slots * max_labels);
    l.meta = take(2 * slots);
    l.logits = take((size_t)W * V);
    if (lm) {
        o.lmq = take(slots);
        o.lmterm = take(2 * (size_t)W * V);
    }
    if (detail) {
        o.fr = take(slots * max_labels);
        o.du = take(slots * max_labels);
        o.lp = take(slots * max_labels);
        o.lead = take(2 * ring * l.cap);
        o.bfslot = take(ring * l.cap);
        o.bdur = take(ring * l.cap);
        o.cld = take((size_t)W * TB_MAX_D);
    }
    l.row = at;
    if (opt) *opt = o;
    return l;
}

// the ring's slots and entries stay inside 2^29, so that every index is an int
static bool tb_sizes_ok(int max_sym, int dmax, int W, int max_labels) {
    const size_t depths = (size_t)(max_sym < max_labels ? max_sym : max_labels);
    return max_sym >= 1 && max_labels >= 1 && dmax >= 1 && W >= 1 && 2 * ((size_t)dmax + 1) * (depths + 2) * W * dmax <= (size_t)INT_MAX / 4;
}

static size_t tb_head(int batch) { return (((size_t)batch + 3) & ~(size_t)3) + ((2 * (size_t)batch + 3) & ~(size_t)3); }

struct TbArgs {
    const float *enc;                      // [batch][T][J]
    const float *table, *U, *proj, *out;   // as in rnnt_tdt_decode.hip: out [J][V + D] b[V + D]
    float *ws;
    int *labels, *lengths;                 // [batch][nbest][max_labels] | [batch][nbest]
    float *scores;
    TbLayout lay;
    size_t ws_head;
    int batch, T, V, blank, H, J, act, max_sym, W, nbest, max_labels;
    nntk_shim_rnnt_tdt_durs du;
    TbOptLayout opt;                       // the LM and DETAIL instantiations only, as is what follows (lay.row counts both parts)
    nntk_shim_rnnt_lm lm;
    nntk_shim_rnnt_tdt_beam_detail dt;
    float *st;                             // the STREAM instantiations only: the rows' carried state, st_row floats a row, each
    size_t st_row, st_nb, st_held;         // the row block | nb [Dmax + 1] ints | held [Dmax - 1][J] (offsets in floats)
};

template <int R> struct TbShared {
    double red_sum[R][RD_WAVES];
    double red_s[RD_WAVES];
    double c_score[TB_MAX_W], c_lse[TB_MAX_W], c_lpb[TB_MAX_W], n_score[TB_MAX_W];
    double lp_dur[TB_MAX_W][TB_MAX_D];
    double cd_s[TB_MAX_W * TB_MAX_D];
    double best_s;
    float red_max[R][RD_WAVES];
    float c_max[TB_MAX_W];
    int red_i[RD_WAVES];
    int c_slot[TB_MAX_W], c_len[TB_MAX_W], n_i[TB_MAX_W], n_v[TB_MAX_W], n_k[TB_MAX_W], n_slot[TB_MAX_W], n_par[TB_MAX_W], n_len[TB_MAX_W];
    int st_src[TB_MAX_W], st_lab[TB_MAX_W], st_dst[TB_MAX_W];
    unsigned c_hash[TB_MAX_W], n_hash[TB_MAX_W];
    int cd_slot[TB_MAX_W * TB_MAX_D], cd_f[TB_MAX_W * TB_MAX_D], cd_found[TB_MAX_W * TB_MAX_D];
    int nb[TB_MAX_RING];
    int best_i, nC, nStep, nCand;
};

static size_t tb_lds_bytes(int R, int H, int J, int VD) {
    const size_t Hp = (size_t)(H + 3) & ~(size_t)3, Jp = (size_t)(J + 3) & ~(size_t)3;
    const size_t W = 4 * (size_t)H > (size_t)VD ? 4 * (size_t)H : (size_t)VD, Wp = (W + 3) & ~(size_t)3;
    const size_t fixed = R == 1 ? sizeof(TbShared<1>) : sizeof(TbShared<NNTK_RNNT_DEC_GROUP>);
    return ((fixed + 15) & ~(size_t)15) + (size_t)R * (2 * Hp + Jp + Wp) * sizeof(float);
}

__device__ __forceinline__ double tb_logaddexp(double x, double y) {         // both finite
    const double m = x > y ? x : y, d = x > y ? y - x : x - y;
    return m + log1p(exp(d));
}

// durations[i] out of the kernel arguments: a select chain, so that the table stays in scalar registers
__device__ __forceinline__ int tb_duration(const nntk_shim_rnnt_tdt_durs &du, int i) {
    int d = du.dur[0];
#pragma unroll
    for (int j = 1; j < TB_MAX_D; ++j) d = i == j ? du.dur[j] : d;
    return d;
}

template <int R, bool LM, bool DETAIL, bool STREAM>
__global__ __launch_bounds__(RD_THREADS) void rnnt_tdt_beam_kernel(const TbArgs a) {
    extern __shared__ __align__(16) unsigned char tb_smem[];
    TbShared<R> &sh = *(TbShared<R> *)tb_smem;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int H = a.H, J = a.J, V = a.V, D = a.du.n, VD = V + D, G = 4 * H, W = a.W, ML = a.max_labels, SF = a.lay.SF;
    const int Hp = (H + 3) & ~3, Jp = (J + 3) & ~3, Wp = ((G > VD ? G : VD) + 3) & ~3;
    const int RING = tb_duration(a.du, D - 1) + 1, cap = a.lay.cap, Dp = __popc(a.du.pos_mask);
    float *sh_h = (float *)(tb_smem + ((sizeof(TbShared<R>) + 15) & ~(size_t)15));
    float *sh_c = sh_h + R * Hp, *sh_z = sh_c + R * Hp, *sh_buf = sh_z + R * Jp;
    const float *pbias = a.proj ? a.proj + (size_t)H * J : nullptr;
    const float *obias = a.out + (size_t)J * VD;
    const int b = blockIdx.x;
    float *const ws_row = a.ws + a.ws_head + (size_t)b * a.lay.row;
    float *row = STREAM ? a.st + (size_t)b * a.st_row : ws_row;              // a stream's committed frames run on the carried block
    double *bscore = (double *)(row + a.lay.bscore);
    float *states = row + a.lay.states, *lg = row + a.lay.logits;
    int *bslot = (int *)(row + a.lay.bslot), *labs = (int *)(row + a.lay.labels), *meta = (int *)(row + a.lay.meta);
    int *lmq = (int *)(row + a.opt.lmq);                                     // LM only, as is lmterm
    double *lmterm = (double *)(row + a.opt.lmterm);
    int *fr = (int *)(row + a.opt.fr), *du = (int *)(row + a.opt.du);        // DETAIL only, as are lp .. cld
    float *lp = row + a.opt.lp;
    double *lead = (double *)(row + a.opt.lead);
    int *bfslot = (int *)(row + a.opt.bfslot), *bdur = (int *)(row + a.opt.bdur), *cld = (int *)(row + a.opt.cld);
    const int n = ((const int *)a.ws)[b];                                    // STREAM: the frames seen with this push
    int *const stat = (int *)a.ws + (((size_t)a.batch + 3) & ~(size_t)3) + 2 * (size_t)b;
    // STREAM: the frames seen before (the host put them and the first-push flag where the counters go), what is committed before and
    // after this push, c = max(0, N - Dmax + 1), and the held encoder frames, frame t at t mod (Dmax - 1)
    const int n_old = STREAM ? stat[0] : 0, first = STREAM ? stat[1] : 1, HR = RING > 2 ? RING - 2 : 1;
    const int c_old = n_old - RING + 2 > 0 ? n_old - RING + 2 : 0, c_new = n - RING + 2 > c_old ? n - RING + 2 : c_old;
    float *const held = STREAM ? a.st + (size_t)b * a.st_row + a.st_held : nullptr;
    int *const st_nb = STREAM ? (int *)(a.st + (size_t)b * a.st_row + a.st_nb) : nullptr;
    int joined = 0, steps = 0;                                               // lane 0's counters, for the timing tool

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

    // the `count` best entries of ring position p's bucket (score descending, insertion index ascending) -> sh.n_slot, sh.n_score
    // (DETAIL: and the entry's index -> sh.n_par, for its lead's arrays)
    auto bucket_best = [&](int p, int count) {
        const int nB = sh.nb[p];
        double prev_s = INFINITY;
        int prev_i = -1, got = 0;
        for (int k = 0; k < count; ++k) {
            double bs = -INFINITY;
            int bi = INT_MAX;
            for (int e = tid; e < nB; e += RD_THREADS) {
                const double s = bscore[(size_t)p * cap + e];
                if ((s < prev_s || (s == prev_s && e > prev_i)) && (bi == INT_MAX || s > bs)) { bs = s; bi = e; }
            }
            block_best(bs, bi);
            if (sh.best_i == INT_MAX) break;
            prev_s = sh.best_s; prev_i = sh.best_i;
            if (tid == 0) { sh.n_slot[k] = bslot[(size_t)p * cap + prev_i]; sh.n_score[k] = prev_s; }
            if constexpr (DETAIL) { if (tid == 0) sh.n_par[k] = prev_i; }
            ++got;
        }
        __syncthreads();
        return got;
    };

    // the prediction network for the steps k0 .. k0 + cnt - 1 of the list: from slot st_src (-1: the zero state) on label st_lab into st_dst
    auto step_group = [&](int k0, int cnt) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int src = r < cnt ? sh.st_src[k0 + r] : -1;
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
                if (r < cnt) sh_buf[r * Wp + nn] = a.table[(size_t)sh.st_lab[k0 + r] * G + nn] + hu[r];
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < R; ++r) {
            if (r >= cnt) continue;
            const float *zg = sh_buf + r * Wp;
            float *st = states + (size_t)sh.st_dst[k0 + r] * SF;
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
                    if (r < cnt) states[(size_t)sh.st_dst[k0 + r] * SF + 2 * H + j] = ph[r] + pbias[j];
            } else {
#pragma unroll
                for (int r = 0; r < R; ++r)
                    if (r < cnt) states[(size_t)sh.st_dst[k0 + r] * SF + 2 * H + j] = sh_h[r * Hp + j];
            }
        }
        __syncthreads();
    };

    // frame t for the hypotheses i0 .. i0 + cnt - 1 of C, one pass over [J][V + D]: the token logits into the workspace, their max and
    // log-sum-exp, lp_tok[blank] and the duration head's lp_dur [D]
    auto heads_group = [&](int i0, int cnt, int t) {
        const float *e = STREAM ? (t < n_old ? held + (size_t)(t % HR) * J : a.enc + ((size_t)b * a.T + (t - n_old)) * J)
                                : a.enc + ((size_t)b * a.T + t) * J;
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
        for (int nn = tid; nn < VD; nn += RD_THREADS) {
            float x[R];
            rd_matvec<R>(a.out, J, VD, nn, sh_z, Jp, x);
#pragma unroll
            for (int r = 0; r < R; ++r) {
                x[r] += obias[nn];
                sh_buf[r * Wp + nn] = x[r];
                if (nn < V) {
                    if (x[r] > m[r]) m[r] = x[r];
                    if (r < cnt) lg[(size_t)(i0 + r) * V + nn] = x[r];
                }
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
            if (tid == RD_THREADS - 1 - r && r < cnt) {                      // the duration head, serially, i ascending
                const float *xd = sh_buf + r * Wp + V;
                float bm = xd[0];
                for (int i = 1; i < D; ++i)
                    if (xd[i] > bm) bm = xd[i];
                double ds = 0.0;
                for (int i = 0; i < D; ++i) ds += (double)expf(xd[i] - bm);
                const double ld = log(ds);
                for (int i = 0; i < D; ++i) sh.lp_dur[i0 + r][i] = ((double)xd[i] - (double)bm) - ld;
            }
        }
        __syncthreads();
        if (tid < cnt) {
            const int r = tid, i = i0 + r;
            double sum = 0.0;
            for (int w = 0; w < RD_WAVES; ++w) sum += sh.red_sum[r][w];
            const double lse = log(sum);
            sh.c_lse[i] = lse;
            sh.c_lpb[i] = (double)(sh_buf[r * Wp + a.blank] - sh.c_max[i]) - lse;
        }
        __syncthreads();
    };

    // the phase's candidates cd_s | cd_slot | cd_f (the landing frame, -1: dropped) move into their buckets, in order
    auto merge_phase = [&](int nCand) {
        for (int c = wave; c < nCand; c += RD_WAVES) {
            int f = -1;
            const int fr = sh.cd_f[c];
            if (fr >= 0) {
                const int p = fr % RING, cnt = sh.nb[p], slot = sh.cd_slot[c], len = meta[2 * slot], hs = meta[2 * slot + 1];
                const int *q = labs + (size_t)slot * ML;
                for (int e = lane; e < cnt; e += 64) {
                    const int s = bslot[(size_t)p * cap + e];
                    if (meta[2 * s] != len || meta[2 * s + 1] != hs) continue;
                    const int *pl = labs + (size_t)s * ML;
                    bool eq = true;
                    for (int j = 0; j < len; ++j)
                        if (pl[j] != q[j]) { eq = false; break; }
                    if (eq) f = e;
                }
                for (int off = 32; off > 0; off >>= 1) {
                    const int of = __shfl_xor(f, off);
                    if (of > f) f = of;
                }
            }
            if (lane == 0) sh.cd_found[c] = f;
        }
        __syncthreads();
        if (tid == 0) {
            const int pn = n % RING, start_n = sh.nb[pn];
            for (int c = 0; c < nCand; ++c) {
                const int fr = sh.cd_f[c];
                if (fr < 0) continue;
                const int p = fr % RING, nbp = sh.nb[p], slot = sh.cd_slot[c];
                const double s = sh.cd_s[c];
                int e = sh.cd_found[c];
                if (e < 0 && fr == n)                                        // its twin of this phase: the same slot, clamped as well
                    for (int e2 = start_n; e2 < nbp; ++e2)
                        if (bslot[(size_t)pn * cap + e2] == slot) { e = e2; break; }
                double *at = bscore + (size_t)p * cap;
                if constexpr (DETAIL) {                                      // the dominant contributor's arrays and last duration; a tie
                    const size_t en = (size_t)p * cap + (e >= 0 ? e : nbp);  // keeps what is there.  The twin of bucket[n] comes by here too
                    if (e >= 0 ? s > lead[en] : nbp < cap) { lead[en] = s; bfslot[en] = slot; bdur[en] = cld[c]; }
                }
                if (e >= 0) at[e] = tb_logaddexp(at[e], s);
                else if (nbp < cap) { bslot[(size_t)p * cap + nbp] = slot; at[nbp] = s; sh.nb[p] = nbp + 1; }
            }
        }
        __syncthreads();
    };

    for (int i = tid; i < R * (2 * Hp + Jp); i += RD_THREADS) sh_h[i] = 0.0f;
    const int slot0 = (RING - 1) * a.lay.frame_slots;                        // frame -1's ring position
    if (tid < RING) sh.nb[tid] = first ? tid == 0 : st_nb[tid];
    if (STREAM && !first) __syncthreads();                                   // a later push: the carried block is as the last one left it
    else {
    if (tid == 0) {
        meta[2 * slot0] = 0; meta[2 * slot0 + 1] = 0; bslot[0] = slot0; bscore[0] = 0.0;
        if constexpr (LM) lmq[slot0] = a.lm.start_state;
        if constexpr (DETAIL) { lead[0] = 0.0; bfslot[0] = slot0; bdur[0] = 0; }
        sh.st_src[0] = -1; sh.st_lab[0] = a.blank; sh.st_dst[0] = slot0;
    }
    __syncthreads();
    step_group(0, 1);                                                        // the step on embed[blank] from the zero state
    }

    // STREAM: phase 0 the committed frames [c_old, c_new), where min(t + d, n) is t + d for every later end, on the carried block;
    // phase 1 the tail [c_new, n) and the report on a copy of it in the workspace, which the next push runs again
    for (int phase = 0, t0 = STREAM ? c_old : 0, t1 = STREAM ? c_new : n;; ++phase) {
    for (int t = t0; t < t1; ++t) {
        const int p = t % RING;
        if (sh.nb[p] == 0) continue;                                         // nobody landed here: no barrier, no read of the frame
        const int nA = bucket_best(p, W), fb = p * a.lay.frame_slots;
        for (int k = 0; k < nA; ++k) {                                       // C = the W best, into the frame's level 0
            const int src = sh.n_slot[k], dst = fb + k, len = meta[2 * src];
            for (int j = tid; j < SF; j += RD_THREADS) states[(size_t)dst * SF + j] = states[(size_t)src * SF + j];
            for (int j = tid; j < len; j += RD_THREADS) labs[(size_t)dst * ML + j] = labs[(size_t)src * ML + j];
            if (tid == 0) { meta[2 * dst] = len; meta[2 * dst + 1] = meta[2 * src + 1]; }
            if constexpr (LM) { if (tid == 0) lmq[dst] = lmq[src]; }
            if constexpr (DETAIL) {                                          // the lead's arrays; the last duration is the entry's own
                const size_t en = (size_t)p * cap + sh.n_par[k], from = (size_t)bfslot[en] * ML, to = (size_t)dst * ML;
                for (int j = tid; j < len; j += RD_THREADS) {
                    fr[to + j] = fr[from + j]; lp[to + j] = lp[from + j]; du[to + j] = j == len - 1 ? bdur[en] : du[from + j];
                }
            }
        }
        if (tid < nA) {
            const int src = sh.n_slot[tid];
            sh.c_slot[tid] = fb + tid; sh.c_score[tid] = sh.n_score[tid]; sh.c_len[tid] = meta[2 * src]; sh.c_hash[tid] = (unsigned)meta[2 * src + 1];
        }
        if (tid == 0) { sh.nC = nA; sh.nb[p] = 0; ++joined; }
        __syncthreads();
        for (int depth = 0;; ++depth) {
            const int nC = sh.nC;
            const bool last = depth == a.max_sym;
            for (int i0 = 0; i0 < nC; i0 += R) heads_group(i0, nC - i0 < R ? nC - i0 : R, t);
            // the blanks: every hypothesis leaves the frame with every positive duration
            for (int idx = tid; idx < nC * D; idx += RD_THREADS) {
                const int i = idx / D, k = idx % D;
                if (!((a.du.pos_mask >> k) & 1)) continue;
                const int c = i * Dp + __popc(a.du.pos_mask & ((1u << k) - 1)), f = t + tb_duration(a.du, k);
                const double s = sh.c_score[i] + (sh.c_lpb[i] + sh.lp_dur[i][k]);
                sh.cd_s[c] = s; sh.cd_slot[c] = sh.c_slot[i]; sh.cd_f[c] = s > -INFINITY ? (f < n ? f : n) : -1;
                if constexpr (DETAIL) cld[c] = sh.c_len[i] ? du[(size_t)sh.c_slot[i] * ML + sh.c_len[i] - 1] : 0;
            }
            __syncthreads();
            merge_phase(nC * Dp);
            // the W best label cells (i, v, k), v != blank; the last depth takes no duration 0
            const unsigned kmask = depth > a.lay.depths ? 0u : last ? a.du.pos_mask : (1u << D) - 1;
            double prev_s = INFINITY;
            int prev_i = -1, nSel = 0;
            if constexpr (LM) {
                // lmterm[i][v] = ln F(q_i, v), one walk per (i, v) whatever the durations: q_i's backoff chain is scattered level by level
                // (the arcs of the level's state over the lanes, an unset label takes acc + ln G), what no level set takes acc + ln U
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
                    double acc = 0.0;
                    for (int s = lmq[sh.c_slot[i]]; s != 0; s = a.lm.d_states[4 * s + 2]) acc += a.lm.d_state_ln[2 * s];
                    for (int v = tid; v < V; v += RD_THREADS) {
                        const double x = lmterm[(size_t)i * V + v];
                        if (x != x) lmterm[(size_t)i * V + v] = acc + a.lm.unk_ln;
                    }
                }
                __syncthreads();
            }
            for (int k = 0; k < W; ++k) {
                double bs = -INFINITY;
                int bi = INT_MAX;
                for (int i = 0; i < nC; ++i) {
                    if (sh.c_len[i] >= ML) continue;
                    const double base = sh.c_score[i], lse = sh.c_lse[i];
                    const float mx = sh.c_max[i];
                    for (int v = tid; v < V; v += RD_THREADS) {
                        if (v == a.blank) continue;
                        const double lt = (double)(lg[(size_t)i * V + v] - mx) - lse;
                        const double lf = LM ? lmterm[(size_t)i * V + v] : 0.0;
                        for (int kk = 0; kk < D; ++kk) {
                            if (!((kmask >> kk) & 1)) continue;
                            const double s = LM ? (base + (lt + sh.lp_dur[i][kk])) + lf : base + (lt + sh.lp_dur[i][kk]);
                            const int idx = (i * V + v) * D + kk;
                            if (s > -INFINITY && (s < prev_s || (s == prev_s && idx > prev_i)) && (bi == INT_MAX || s > bs)) { bs = s; bi = idx; }
                        }
                    }
                }
                block_best(bs, bi);
                if (sh.best_i == INT_MAX) break;
                prev_s = sh.best_s; prev_i = sh.best_i;
                if (tid == 0) { sh.n_i[k] = prev_i / D / V; sh.n_v[k] = prev_i / D % V; sh.n_k[k] = prev_i % D; sh.n_score[k] = prev_s; }
                ++nSel;
            }
            if (nSel == 0) break;
            __syncthreads();
            // a cell's slot is that of the first selected cell with its (i, v): one hypothesis, one LSTM step
            const int dst0 = fb + (depth + 1) * W;
            int first = tid, ps = 0, ol = 0;
            unsigned oh = 0;
            float nlp = 0.0f;                                                // DETAIL: the token head's lp_tok[v], as the selection formed it
            if (tid < nSel) {
                const int i = sh.n_i[tid], v = sh.n_v[tid];
                for (int j = 0; j < tid; ++j)
                    if (sh.n_i[j] == i && sh.n_v[j] == v) { first = j; break; }
                ps = sh.c_slot[i]; ol = sh.c_len[i]; oh = sh.c_hash[i];
                if constexpr (DETAIL) nlp = (float)((double)(lg[(size_t)i * V + v] - sh.c_max[i]) - sh.c_lse[i]);
            }
            __syncthreads();
            if (tid < nSel) {
                const unsigned nh = oh * 1000003u + (unsigned)(sh.n_v[tid] + 1);
                sh.n_slot[tid] = dst0 + first; sh.n_par[tid] = ps; sh.n_len[tid] = ol + 1; sh.n_hash[tid] = nh;
                if (first == tid) { meta[2 * (dst0 + tid)] = ol + 1; meta[2 * (dst0 + tid) + 1] = (int)nh; }
                if constexpr (LM) { if (first == tid) lmq[dst0 + tid] = rd_lm_next(a.lm, lmq[ps], sh.n_v[tid]); }
                if constexpr (DETAIL) {                                      // duration 0: what the slot's own hypothesis (the next C) took;
                    const size_t at = (size_t)(dst0 + tid) * ML + ol;        // a twin's positive one rides with its candidate and entry
                    if (first == tid) { fr[at] = t; lp[at] = nlp; du[at] = 0; }
                }
            }
            __syncthreads();
            if (tid == 0) {                                                  // the steps to run, the next C (duration 0), the moves (the rest)
                int nStep = 0, nNext = 0, nCand = 0;
                for (int k = 0; k < nSel; ++k) {
                    const int slot = sh.n_slot[k], d = tb_duration(a.du, sh.n_k[k]);
                    if (slot == dst0 + k) { sh.st_src[nStep] = sh.n_par[k]; sh.st_lab[nStep] = sh.n_v[k]; sh.st_dst[nStep] = slot; ++nStep; }
                    if (d == 0) {
                        sh.c_slot[nNext] = slot; sh.c_score[nNext] = sh.n_score[k]; sh.c_len[nNext] = sh.n_len[k]; sh.c_hash[nNext] = sh.n_hash[k];
                        ++nNext;
                    } else {
                        sh.cd_s[nCand] = sh.n_score[k]; sh.cd_slot[nCand] = slot; sh.cd_f[nCand] = t + d < n ? t + d : n;
                        if constexpr (DETAIL) cld[nCand] = d;
                        ++nCand;
                    }
                }
                sh.nStep = nStep; sh.nC = nNext; sh.nCand = nCand;
                steps += nStep;
            }
            __syncthreads();
            const int nStep = sh.nStep;
            for (int k = 0; k < nStep; ++k) {
                const int L = meta[2 * sh.st_dst[k]] - 1;
                const int *pl = labs + (size_t)sh.st_src[k] * ML;
                int *q = labs + (size_t)sh.st_dst[k] * ML;
                for (int j = tid; j < L; j += RD_THREADS) q[j] = pl[j];
                if (tid == 0) q[L] = sh.st_lab[k];
                if constexpr (DETAIL) {
                    const size_t from = (size_t)sh.st_src[k] * ML, to = (size_t)sh.st_dst[k] * ML;
                    for (int j = tid; j < L; j += RD_THREADS) { fr[to + j] = fr[from + j]; lp[to + j] = lp[from + j]; du[to + j] = du[from + j]; }
                }
            }
            for (int k0 = 0; k0 < nStep; k0 += R) step_group(k0, nStep - k0 < R ? nStep - k0 : R);
            merge_phase(sh.nCand);
            if (last || sh.nC == 0) break;
        }
        __syncthreads();
    }
    if constexpr (STREAM) {
        if (phase == 1) break;
        if (tid < RING) st_nb[tid] = sh.nb[tid];
        if (c_new >= n) break;                                               // no tail: the report reads the carried block, and writes none of it
        for (int t = c_new > n_old ? c_new : n_old; t < n; ++t) {            // the tail's new frames are held for the next push: bit copies
            const unsigned *src = (const unsigned *)(a.enc + ((size_t)b * a.T + (t - n_old)) * J);
            unsigned *dst = (unsigned *)(held + (size_t)(t % HR) * J);
            for (int j = tid; j < J; j += RD_THREADS) dst[j] = src[j];
        }
        // the block without what a depth fills before it reads it (logits, lmterm); every part is a multiple of 4 floats
        const size_t end0 = a.lay.logits, beg1 = LM ? a.opt.lmq : DETAIL ? a.opt.fr : a.lay.row, end1 = LM ? a.opt.lmterm : a.lay.row;
        const size_t beg2 = LM && DETAIL ? a.opt.fr : a.lay.row;
        const float4 *src4 = (const float4 *)row;
        float4 *dst4 = (float4 *)ws_row;
        for (size_t i = tid; i < end0 / 4; i += RD_THREADS) dst4[i] = src4[i];
        for (size_t i = beg1 / 4 + tid; i < end1 / 4; i += RD_THREADS) dst4[i] = src4[i];
        for (size_t i = beg2 / 4 + tid; i < a.lay.row / 4; i += RD_THREADS) dst4[i] = src4[i];
        row = ws_row;
        bscore = (double *)(row + a.lay.bscore); states = row + a.lay.states; lg = row + a.lay.logits;
        bslot = (int *)(row + a.lay.bslot); labs = (int *)(row + a.lay.labels); meta = (int *)(row + a.lay.meta);
        lmq = (int *)(row + a.opt.lmq); lmterm = (double *)(row + a.opt.lmterm);
        fr = (int *)(row + a.opt.fr); du = (int *)(row + a.opt.du); lp = row + a.opt.lp;
        lead = (double *)(row + a.opt.lead);
        bfslot = (int *)(row + a.opt.bfslot); bdur = (int *)(row + a.opt.bdur); cld = (int *)(row + a.opt.cld);
        __syncthreads();
        t0 = c_new; t1 = n;
    } else break;
    }

    if constexpr (LM || DETAIL) {
        // the report: the W best of bucket[n], + ln E(q) with a model, the -inf ones dropped, ranked by score or score / (length + 1)
        // (every entry counts the entries ahead of it; ties to the lower rank).  On what the frames have left free: the score in
        // sh.c_score, the key in sh.c_lse, the order in sh.n_i, the kept count in sh.nCand
        const int pn = n % RING, nW = bucket_best(pn, W);
        if (tid < nW) {
            double s = sh.n_score[tid];
            if constexpr (LM) s += a.lm.d_state_ln[2 * lmq[sh.n_slot[tid]] + 1];
            sh.c_score[tid] = s;
            sh.c_lse[tid] = a.dt.length_norm ? s / (double)(meta[2 * sh.n_slot[tid]] + 1) : s;
        }
        __syncthreads();
        if (tid < nW) {
            const double s = sh.c_lse[tid];
            int ahead = 0;
            for (int j = 0; j < nW; ++j) {
                const double o = sh.c_lse[j];
                ahead += o > -INFINITY && (o > s || (o == s && j < tid));
            }
            if (s > -INFINITY) sh.n_i[ahead] = tid;
        }
        if (tid == 0) {
            int kept = 0;
            for (int j = 0; j < nW; ++j) kept += sh.c_lse[j] > -INFINITY;
            sh.nCand = kept;
        }
        __syncthreads();
        const int kept = sh.nCand;
        for (int k = 0; k < a.nbest; ++k) {
            const size_t o = (size_t)b * a.nbest + k;
            const int src = k < kept ? sh.n_i[k] : 0, slot = sh.n_slot[src], len = k < kept ? meta[2 * slot] : 0;
            size_t from = 0;
            int ld = 0;
            if constexpr (DETAIL) {
                if (k < kept) { const size_t en = (size_t)pn * cap + sh.n_par[src]; from = (size_t)bfslot[en] * ML; ld = bdur[en]; }
            }
            for (int j = tid; j < ML; j += RD_THREADS) {
                a.labels[o * ML + j] = j < len ? labs[(size_t)slot * ML + j] : -1;
                if constexpr (DETAIL) {
                    if (a.dt.d_frames) a.dt.d_frames[o * ML + j] = j < len ? fr[from + j] : -1;
                    if (a.dt.d_durations) a.dt.d_durations[o * ML + j] = j < len ? (j == len - 1 ? ld : du[from + j]) : -1;
                    if (a.dt.d_logps) a.dt.d_logps[o * ML + j] = j < len ? lp[from + j] : 0.0f;
                }
            }
            if (tid == 0) {
                a.lengths[o] = k < kept ? len : -1;
                a.scores[o] = k < kept ? (float)sh.c_score[src] : -INFINITY;
            }
        }
    } else {
    const int nOut = bucket_best(n % RING, a.nbest);
    for (int k = 0; k < a.nbest; ++k) {
        const size_t o = (size_t)b * a.nbest + k;
        const int slot = k < nOut ? sh.n_slot[k] : 0, len = k < nOut ? meta[2 * slot] : 0;
        for (int j = tid; j < ML; j += RD_THREADS) a.labels[o * ML + j] = j < len ? labs[(size_t)slot * ML + j] : -1;
        if (tid == 0) {
            a.lengths[o] = k < nOut ? len : -1;
            a.scores[o] = k < nOut ? (float)sh.n_score[k] : -INFINITY;
        }
    }
    }
    if (tid == 0) { stat[0] = joined; stat[1] = steps; }
}

typedef void (*TbKernel)(const TbArgs);

template <int R> static TbKernel tb_kernel(bool lm, bool detail, bool stream) {
    static const TbKernel k[2][2][2] = {
        { { rnnt_tdt_beam_kernel<R, false, false, false>, rnnt_tdt_beam_kernel<R, false, false, true> },
          { rnnt_tdt_beam_kernel<R, false, true, false>, rnnt_tdt_beam_kernel<R, false, true, true> } },
        { { rnnt_tdt_beam_kernel<R, true, false, false>, rnnt_tdt_beam_kernel<R, true, false, true> },
          { rnnt_tdt_beam_kernel<R, true, true, false>, rnnt_tdt_beam_kernel<R, true, true, true> } } };
    return k[lm][detail][stream];
}

static int tb_forced_group = 0;

// a stream's carried state, per row: the row block of tb_layout | nb [Dmax + 1] | held [Dmax - 1][J], each padded to 4 floats
static size_t tb_state_row(const TbLayout &l, int dmax, int J, size_t *nb = nullptr, size_t *held = nullptr) {
    const size_t at_nb = l.row, at_held = at_nb + (((size_t)dmax + 1 + 3) & ~(size_t)3);
    if (nb) *nb = at_nb;
    if (held) *held = at_held;
    return at_held + (((size_t)(dmax - 1) * J + 3) & ~(size_t)3);
}

extern "C" {

size_t nntk_shim_rnnt_tdt_beam_workspace_floats(int batch, int H, int J, int V, int max_sym, int dmax, int beam_width, int max_labels,
                                                int with_lm, int with_detail) {
    if (batch <= 0 || !tb_sizes_ok(max_sym, dmax, beam_width, max_labels)) return 0;
    return tb_head(batch) + (size_t)batch * tb_layout(H, J, V, max_sym, dmax, beam_width, max_labels, with_lm != 0, with_detail != 0).row;
}

int nntk_shim_rnnt_tdt_beam_fits(int H, int J, int V, int D) { return tb_lds_bytes(1, H, J, V + D) <= RD_LDS_MAX; }

int nntk_shim_rnnt_tdt_beam_group(int beam_width, int H, int J, int V, int D) {
    const bool fits = tb_lds_bytes(NNTK_RNNT_DEC_GROUP, H, J, V + D) <= RD_LDS_MAX;
    if (tb_forced_group) return tb_forced_group == NNTK_RNNT_DEC_GROUP && fits ? NNTK_RNNT_DEC_GROUP : 1;
    return beam_width > 1 && fits ? NNTK_RNNT_DEC_GROUP : 1;
}

void nntk_shim_rnnt_tdt_beam_set_group(int group) { tb_forced_group = group == 1 || group == NNTK_RNNT_DEC_GROUP ? group : 0; }

size_t nntk_shim_rnnt_tdt_beam_state_floats(int batch, int H, int J, int V, int max_sym, int dmax, int beam_width, int max_labels,
                                            int with_lm, int with_detail) {
    if (batch <= 0 || !tb_sizes_ok(max_sym, dmax, beam_width, max_labels)) return 0;
    return (size_t)batch * tb_state_row(tb_layout(H, J, V, max_sym, dmax, beam_width, max_labels, with_lm != 0, with_detail != 0), dmax, J);
}

// d_state NULL: one-shot, h_n_frames the rows' lengths.  Else a push: h_n_frames the frames seen with it, h_seen those seen before
static int tb_run(const nntk_shim_rnnt_dec *m, const nntk_shim_rnnt_tdt_durs *du, const float *d_enc, int batch, int T,
                  const int *h_n_frames, const int *h_seen, const int *h_first, float *d_state, int beam_width, int nbest, int max_labels,
                  const nntk_shim_rnnt_lm *lm, const nntk_shim_rnnt_tdt_beam_detail *dt, int *d_labels, int *d_lengths, float *d_scores,
                  float *d_ws) {
    if (batch <= 0) return 0;
    const int dmax = du->n >= 1 && du->n <= TB_MAX_D ? du->dur[du->n - 1] : 0;
    if (m->E < 1 || m->H < 1 || m->J < 1 || m->V < 2 || m->H > NNTK_RNNT_DEC_MAX_WIDTH || m->J > NNTK_RNNT_DEC_MAX_WIDTH ||
        m->V > NNTK_RNNT_DEC_MAX_V || dmax < 1 || dmax > NNTK_RNNT_TDT_MAX_DURATION || du->pos_mask == 0 ||
        !nntk_shim_rnnt_tdt_beam_fits(m->H, m->J, m->V, du->n) || beam_width < 1 || beam_width > TB_MAX_W || nbest < 1 || nbest > beam_width ||
        !tb_sizes_ok(m->max_symbols_per_frame, dmax, beam_width, max_labels))
        return nntk_fail_msg("nntk_rnnt_tdt_beam_decode_device: the model is beyond the decoding kernel's limits");
    if (!d_state) {
        if (nntk_shim_upload_ints((int *)d_ws, h_n_frames, batch)) return -1;
    } else {                                                                 // the head as the kernel reads it: n [batch] | (seen, first) a row
        const size_t at = ((size_t)batch + 3) & ~(size_t)3, words = at + 2 * (size_t)batch;
        int *head = (int *)calloc(words, sizeof(int));
        if (!head) return nntk_fail_msg("nntk_rnnt_tdt_beam_stream_push_device: out of host memory");
        for (int b = 0; b < batch; ++b) { head[b] = h_n_frames[b]; head[at + 2 * b] = h_seen[b]; head[at + 2 * b + 1] = h_first[b]; }
        const int rc = nntk_shim_upload_ints((int *)d_ws, head, (long)words);
        free(head);
        if (rc) return -1;
    }
    TbArgs a;
    a.enc = d_enc; a.table = m->d_table; a.U = m->d_U; a.proj = m->d_proj; a.out = m->d_out;
    a.ws = d_ws;
    a.labels = d_labels; a.lengths = d_lengths; a.scores = d_scores;
    a.lm = lm ? *lm : nntk_shim_rnnt_lm();
    a.dt = dt ? *dt : nntk_shim_rnnt_tdt_beam_detail();
    a.lay = tb_layout(m->H, m->J, m->V, m->max_symbols_per_frame, dmax, beam_width, max_labels, lm != nullptr, dt != nullptr, &a.opt);
    a.ws_head = tb_head(batch);
    a.st = d_state;
    a.st_row = tb_state_row(a.lay, dmax, m->J, &a.st_nb, &a.st_held);
    a.batch = batch; a.T = T; a.V = m->V; a.blank = m->blank; a.H = m->H; a.J = m->J; a.act = m->activation;
    a.max_sym = m->max_symbols_per_frame; a.W = beam_width; a.nbest = nbest; a.max_labels = max_labels;
    a.du = *du;
    const int R = nntk_shim_rnnt_tdt_beam_group(beam_width, m->H, m->J, m->V, du->n);
    const size_t lds = tb_lds_bytes(R, m->H, m->J, m->V + du->n);
    const bool st = d_state != nullptr;
    const TbKernel k = R == 1 ? tb_kernel<1>(lm != nullptr, dt != nullptr, st) : tb_kernel<NNTK_RNNT_DEC_GROUP>(lm != nullptr, dt != nullptr, st);
    if (lds > 48 * 1024 && nntk_set_max_dynamic_lds((const void *)k, lds)) return -1;
    hipLaunchKernelGGL(k, dim3((unsigned)batch), dim3(RD_THREADS), lds, nntk_stream(), a);
    NNTK_LAUNCH_CHECK("rnnt_tdt_beam_kernel");
    return 0;
}

int nntk_shim_rnnt_tdt_beam(const nntk_shim_rnnt_dec *m, const nntk_shim_rnnt_tdt_durs *du, const float *d_enc, int batch, int T,
                            const int *h_n_frames, int beam_width, int nbest, int max_labels, const nntk_shim_rnnt_lm *lm,
                            const nntk_shim_rnnt_tdt_beam_detail *dt, int *d_labels, int *d_lengths, float *d_scores, float *d_ws) {
    return tb_run(m, du, d_enc, batch, T, h_n_frames, nullptr, nullptr, nullptr, beam_width, nbest, max_labels, lm, dt, d_labels, d_lengths,
                  d_scores, d_ws);
}

int nntk_shim_rnnt_tdt_beam_stream(const nntk_shim_rnnt_dec *m, const nntk_shim_rnnt_tdt_durs *du, const float *d_enc, int batch, int T,
                                   const int *h_seen_now, const int *h_seen, const int *h_first, float *d_state, int beam_width, int nbest,
                                   int max_labels, const nntk_shim_rnnt_lm *lm, const nntk_shim_rnnt_tdt_beam_detail *dt, int *d_labels,
                                   int *d_lengths, float *d_scores, float *d_ws) {
    return tb_run(m, du, d_enc, batch, T, h_seen_now, h_seen, h_first, d_state, beam_width, nbest, max_labels, lm, dt, d_labels, d_lengths,
                  d_scores, d_ws);
}

}  // extern "C"
