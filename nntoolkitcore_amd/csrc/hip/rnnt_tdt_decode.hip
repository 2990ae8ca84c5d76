// rnnt_tdt_decode.hip -- greedy decoding of a token-and-duration transducer (TDT, Xu et al. 2023; the loss is rnnt_tdt.hip): one launch
// runs every row's whole decision loop.  A decision scores the V tokens and the D durations of one (frame, prediction-network state) with
// ONE pass over the [J][V + D] block, picks a token and a duration, and moves on by that many frames: a frame that is jumped over is never
// joined or projected, so a row makes fewer passes over the matrix than it has frames.
//
// Work split.  As rnnt_decode.hip: a workgroup of RD_THREADS lanes owns R rows (R = 1 or NNTK_RNNT_DEC_GROUP, the launcher's choice,
// never visible in the bits) and steps them together; the rows of a group sit at different t, a row that is done (or only pays owed
// frames) is parked with an all-zero z, its logits computed and ignored.  A lane owns column n of [0, V + D): the logits of both heads land
// in the row's max(4H, V + D) LDS buffer in the same pass.  The token head's argmax and sum-exp cover [0, V) with the reductions of
// rnnt_dec_common.hpp.  The duration head (at most 8 values, in LDS by then) is reduced by ONE lane per row -- lane RD_THREADS - 1 - r, in
// the last wavefront, while the others finish the token sum-exp -- in a fixed serial order, i ascending: one scan yields the best
// duration overall and the best positive one, a second the sum exp(x - best) in double.  Which of the two winners counts is a select
// after the token argmax (a blank never takes duration 0), not a second pass.  The duration table and the mask of its positive entries
// ride in the kernel arguments: no global read for them, no atomics, no flags, rows never talk to each other.
//
// Barriers.  A decision: 4 __syncthreads (z ready | the wavefronts' argmax parts ready | the sum parts and the duration head ready | the
// row's move made) -- the classic kernel's count, the duration head lives inside phases three and four.  An emission step: 3 (gate
// pre-activations | h, c | g), again the classic kernel's.
//
// Bits.  The contract of rnnt_dec_common.hpp for the matrix-vector products, the token maximum and its sum-exp.  Duration head: the
// maximum is exact, ties to the lowest index (strict > over ascending i); sum exp(x_i - max), expf per element, added in double, i
// ascending; lp_dur = (x_i - max) - log(sum), the difference and the rest in double.  score += lp_tok + lp_dur in double, rounded to f32
// only in the output, so a stream's chunks add up exactly as the one-shot call does -- whatever R, the batch, T or the chunking.
//
// Streaming.  The classic state (h, c, g; started | s | labels | frames consumed; the score) plus one int per row: the frames the last
// jump went past the chunk's end.  A started row enters at t = owed; where that is at or beyond the chunk's frames the row decides
// nothing and the rest stays owed.  A fresh row never reads the word, so the classic reset serves.
#include "rnnt_dec_common.hpp"

struct TdArgs {
    const float *enc;                      // [batch][T][J]
    const float *table, *U, *proj, *out;   // [V][4H] | [H][4H] | [H][J] b[J] or NULL | [J][V + D] b[V + D]
    float *st_f;                           // per row h [H] | c [H] | g [J], or NULL: every row from the start, nothing kept
    double *st_score;                      // [batch]
    int *st_i, *st_owed;                   // [batch][4]: started | s | labels | frames consumed; [batch]: frames owed
    int *labels, *frames, *durs, *lengths; // lengths holds the call's n_frames on entry
    float *scores;
    int batch, T, V, blank, H, J, act, max_sym, max_labels;
    nntk_shim_rnnt_tdt_durs du;
};

// fixed part of the LDS, then the float arrays: h [R][Hp] | c [R][Hp] | g [R][Jp] | z [R][Jp] | buf [R][Wp]
template <int R> struct TdShared {
    double red_sum[R][RD_WAVES];
    double score[R > 1 ? R : 2];
    double dur_sum[R > 1 ? R : 2];
    float red_max[R][RD_WAVES];
    int red_idx[R][RD_WAVES];
    int t[4], s[4], count[4], n[4], base[4], emit[4], row[4], fresh[4], best[4], live[4], dur_all[4], dur_pos[4];
};

static size_t td_lds_bytes(int R, int H, int J, int VD) {
    const size_t Hp = (size_t)(H + 3) & ~(size_t)3, Jp = (size_t)(J + 3) & ~(size_t)3;
    const size_t W = 4 * (size_t)H > (size_t)VD ? 4 * (size_t)H : (size_t)VD, Wp = (W + 3) & ~(size_t)3;
    const size_t fixed = R == 1 ? sizeof(TdShared<1>) : sizeof(TdShared<NNTK_RNNT_DEC_GROUP>);
    return ((fixed + 15) & ~(size_t)15) + (size_t)R * (2 * Hp + 2 * Jp + Wp) * sizeof(float);
}

// durations[i] out of the kernel arguments: a select chain, so that the table stays in scalar registers
__device__ __forceinline__ int td_duration(const nntk_shim_rnnt_tdt_durs &du, int i) {
    int d = du.dur[0];
#pragma unroll
    for (int j = 1; j < NNTK_RNNT_TDT_MAX_DURATIONS; ++j) d = i == j ? du.dur[j] : d;
    return d;
}

template <int R>
__global__ __launch_bounds__(RD_THREADS) void rnnt_tdt_greedy_kernel(const TdArgs a) {
    extern __shared__ __align__(16) unsigned char td_smem[];
    TdShared<R> &sh = *(TdShared<R> *)td_smem;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int H = a.H, J = a.J, V = a.V, D = a.du.n, VD = V + D, G = 4 * H;
    const int Hp = (H + 3) & ~3, Jp = (J + 3) & ~3, Wp = ((G > VD ? G : VD) + 3) & ~3;
    float *sh_h = (float *)(td_smem + ((sizeof(TdShared<R>) + 15) & ~(size_t)15));
    float *sh_c = sh_h + R * Hp, *sh_g = sh_c + R * Hp, *sh_z = sh_g + R * Jp, *sh_buf = sh_z + R * Jp;
    const float *pbias = a.proj ? a.proj + (size_t)H * J : nullptr;
    const float *obias = a.out + (size_t)J * VD;

    if (tid < R) {
        const int r = tid, b = blockIdx.x * R + r;
        const bool valid = b < a.batch;
        const bool started = valid && a.st_i && a.st_i[4 * b] != 0;
        sh.row[r] = valid ? b : -1;
        sh.n[r] = valid ? a.lengths[b] : 0;
        sh.t[r] = started ? a.st_owed[b] : 0;                                 // the frames a jump of the last push went past its end
        sh.s[r] = started ? a.st_i[4 * b + 1] : 0;
        sh.count[r] = started ? a.st_i[4 * b + 2] : 0;
        sh.base[r] = started ? a.st_i[4 * b + 3] : 0;
        sh.score[r] = started ? a.st_score[b] : 0.0;
        sh.fresh[r] = valid && !started;
        sh.emit[r] = valid && !started ? a.blank : -1;                     // a new row: the step on embed[blank] from the zero state
    }
    for (int i = tid; i < R * (2 * Hp + 2 * Jp); i += RD_THREADS) sh_h[i] = 0.0f;   // h, c, g, z: the padding columns stay zero
    __syncthreads();
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int b = sh.row[r];
        if (b >= 0 && !sh.fresh[r]) {
            const float *st = a.st_f + (size_t)b * (2 * H + J);
            for (int j = tid; j < H; j += RD_THREADS) { sh_h[r * Hp + j] = st[j]; sh_c[r * Hp + j] = st[H + j]; }
            for (int j = tid; j < J; j += RD_THREADS) sh_g[r * Jp + j] = st[2 * H + j];
        }
    }
    __syncthreads();

    bool step = false;
#pragma unroll
    for (int r = 0; r < R; ++r) step |= sh.emit[r] >= 0;
    for (;;) {
        if (step) {                                                            // the prediction network, for the rows that emitted
            for (int n = tid; n < G; n += RD_THREADS) {
                float hu[R];
                rd_matvec<R>(a.U, H, G, n, sh_h, Hp, hu);
#pragma unroll
                for (int r = 0; r < R; ++r)
                    if (sh.emit[r] >= 0) sh_buf[r * Wp + n] = a.table[(size_t)sh.emit[r] * G + n] + hu[r];
            }
            __syncthreads();
#pragma unroll
            for (int r = 0; r < R; ++r) {
                if (sh.emit[r] < 0) continue;
                const float *zg = sh_buf + r * Wp;
                for (int j = tid; j < H; j += RD_THREADS) {
                    const float gi = rd_sigmoid(zg[j]), gf = rd_sigmoid(zg[H + j]), gg = tanhf(zg[2 * H + j]), go = rd_sigmoid(zg[3 * H + j]);
                    const float c = gf * sh_c[r * Hp + j] + gi * gg;
                    sh_c[r * Hp + j] = c;
                    sh_h[r * Hp + j] = go * tanhf(c);
                }
            }
            __syncthreads();
            for (int j = tid; j < J; j += RD_THREADS) {
                if (a.proj) {
                    float ph[R];
                    rd_matvec<R>(a.proj, H, J, j, sh_h, Hp, ph);
#pragma unroll
                    for (int r = 0; r < R; ++r)
                        if (sh.emit[r] >= 0) sh_g[r * Jp + j] = ph[r] + pbias[j];
                } else {
#pragma unroll
                    for (int r = 0; r < R; ++r)
                        if (sh.emit[r] >= 0) sh_g[r * Jp + j] = sh_h[r * Hp + j];
                }
            }
            __syncthreads();
        }
        bool act[R], any = false;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            act[r] = sh.row[r] >= 0 && sh.t[r] < sh.n[r] && sh.count[r] < a.max_labels;
            any |= act[r];
        }
        if (!any) break;
        // the joiner at each row's own t; a parked row keeps an all-zero z (its logits are computed and ignored)
#pragma unroll
        for (int r = 0; r < R; ++r) {
            if (act[r]) {
                const float *e = a.enc + ((size_t)sh.row[r] * a.T + sh.t[r]) * J;
                for (int j = tid; j < J; j += RD_THREADS) sh_z[r * Jp + j] = rd_act(a.act, e[j] + sh_g[r * Jp + j]);
            } else {
                for (int j = tid; j < J; j += RD_THREADS) sh_z[r * Jp + j] = 0.0f;
            }
        }
        __syncthreads();
        // one pass over [J][V + D] for both heads; each lane's part of the TOKEN argmax (columns below V)
        float m[R];
        int mi[R];
#pragma unroll
        for (int r = 0; r < R; ++r) { m[r] = -INFINITY; mi[r] = V; }
        for (int n = tid; n < VD; n += RD_THREADS) {
            float x[R];
            rd_matvec<R>(a.out, J, VD, n, sh_z, Jp, x);
#pragma unroll
            for (int r = 0; r < R; ++r) {
                x[r] += obias[n];
                sh_buf[r * Wp + n] = x[r];
                if (n < V && (x[r] > m[r] || (x[r] == m[r] && n < mi[r]))) { m[r] = x[r]; mi[r] = n; }
            }
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            rd_wave_argmax(m[r], mi[r]);
            if (lane == 0) { sh.red_max[r][wave] = m[r]; sh.red_idx[r][wave] = mi[r]; }
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < R; ++r) {
            m[r] = sh.red_max[r][0]; mi[r] = sh.red_idx[r][0];
            for (int w = 1; w < RD_WAVES; ++w) {
                const float om = sh.red_max[r][w];
                const int oi = sh.red_idx[r][w];
                if (om > m[r] || (om == m[r] && oi < mi[r])) { m[r] = om; mi[r] = oi; }
            }
            const double sum = rd_wave_sum_exp(sh_buf + r * Wp, V, tid, m[r]);
            if (lane == 0) sh.red_sum[r][wave] = sum;
            if (tid == 0) { sh.best[r] = mi[r]; sh.live[r] = act[r]; }
            if (tid == RD_THREADS - 1 - r) {                                   // the duration head: both winners in one serial scan
                const float *xd = sh_buf + r * Wp + V;
                float bm = xd[0], pm = -INFINITY;
                int bi = 0, pi = __ffs(a.du.pos_mask) - 1;                     // (NaN scores: stay on a valid, a positive, duration)
                for (int i = 0; i < D; ++i) {
                    const float x = xd[i];
                    if (x > bm) { bm = x; bi = i; }
                    if (((a.du.pos_mask >> i) & 1) && x > pm) { pm = x; pi = i; }
                }
                double ds = 0.0;
                for (int i = 0; i < D; ++i) ds += (double)expf(xd[i] - bm);
                sh.dur_all[r] = bi; sh.dur_pos[r] = pi; sh.dur_sum[r] = ds;
            }
        }
        __syncthreads();
        if (tid < R && sh.live[tid]) {
            const int r = tid, b = sh.row[r];
            double sum = 0.0;
            for (int w = 0; w < RD_WAVES; ++w) sum += sh.red_sum[r][w];
            const int k = sh.best[r] < V ? sh.best[r] : a.blank;               // (no finite or infinite maximum: NaN weights; stay in bounds)
            const bool is_blank = k == a.blank;
            const int i = is_blank ? sh.dur_pos[r] : sh.dur_all[r];            // a blank never takes duration 0
            const float *xd = sh_buf + r * Wp + V;
            const double lp_tok = -log(sum);                                   // x[k] - max - log(sum), x[k] = max
            const double lp_dur = ((double)xd[i] - (double)xd[sh.dur_all[r]]) - log(sh.dur_sum[r]);
            sh.score[r] += lp_tok + lp_dur;
            const int d = td_duration(a.du, i);
            if (is_blank) {
                sh.t[r] += d; sh.s[r] = 0; sh.emit[r] = -1;
            } else {
                const size_t at = (size_t)b * a.max_labels + sh.count[r];
                a.labels[at] = k;
                if (a.frames) a.frames[at] = sh.base[r] + sh.t[r];
                if (a.durs) a.durs[at] = d;
                sh.count[r] += 1; sh.emit[r] = k;
                if (d > 0) { sh.t[r] += d; sh.s[r] = 0; }
                else if (++sh.s[r] == a.max_sym) { sh.t[r] += 1; sh.s[r] = 0; } // the cap moves on without scoring anything
            }
        } else if (tid < R) {
            sh.emit[tid] = -1;
        }
        __syncthreads();
        step = false;
#pragma unroll
        for (int r = 0; r < R; ++r) step |= sh.emit[r] >= 0;
    }

#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int b = sh.row[r];
        if (b < 0) continue;
        if (a.st_f) {
            float *st = a.st_f + (size_t)b * (2 * H + J);
            for (int j = tid; j < H; j += RD_THREADS) { st[j] = sh_h[r * Hp + j]; st[H + j] = sh_c[r * Hp + j]; }
            for (int j = tid; j < J; j += RD_THREADS) st[2 * H + j] = sh_g[r * Jp + j];
        }
        const int cnt = sh.count[r];
        for (int i = cnt + tid; i < a.max_labels; i += RD_THREADS) {
            const size_t at = (size_t)b * a.max_labels + i;
            a.labels[at] = -1;
            if (a.frames) a.frames[at] = -1;
            if (a.durs) a.durs[at] = -1;
        }
        if (tid == 0) {
            if (a.st_i) {
                const int used = sh.t[r] < sh.n[r] ? sh.t[r] : sh.n[r];        // beyond the chunk's frames: owed to the next pushes
                a.st_i[4 * b] = 1; a.st_i[4 * b + 1] = sh.s[r]; a.st_i[4 * b + 2] = cnt; a.st_i[4 * b + 3] = sh.base[r] + used;
                a.st_owed[b] = sh.t[r] - used;
                a.st_score[b] = sh.score[r];
            }
            a.lengths[b] = cnt;
            if (a.scores) a.scores[b] = (float)sh.score[r];
        }
    }
}

extern "C" {

int nntk_shim_rnnt_tdt_dec_rows_per_group(int batch, int H, int J, int V, int D) {
    return batch > NNTK_RNNT_DEC_GROUP_BATCH && td_lds_bytes(NNTK_RNNT_DEC_GROUP, H, J, V + D) <= RD_LDS_MAX ? NNTK_RNNT_DEC_GROUP : 1;
}

int nntk_shim_rnnt_tdt_greedy(const nntk_shim_rnnt_dec *m, const nntk_shim_rnnt_tdt_durs *du, const float *d_enc, int batch, int T,
                              const int *h_n_frames, int max_labels, float *d_st_f, double *d_st_score, int *d_st_i, int *d_st_owed,
                              int *d_labels, int *d_frames, int *d_durations, int *d_lengths, float *d_scores) {
    if (batch <= 0) return 0;
    if (m->E < 1 || m->H < 1 || m->J < 1 || m->V < 2 || m->H > NNTK_RNNT_DEC_MAX_WIDTH || m->J > NNTK_RNNT_DEC_MAX_WIDTH ||
        m->V > NNTK_RNNT_DEC_MAX_V || du->n < 1 || du->n > NNTK_RNNT_TDT_MAX_DURATIONS || du->pos_mask == 0 ||
        td_lds_bytes(1, m->H, m->J, m->V + du->n) > RD_LDS_MAX)
        return nntk_fail_msg("nntk_rnnt_tdt_greedy_decode_device: the model is beyond the decoding kernel's limits");
    if (nntk_shim_upload_ints(d_lengths, h_n_frames, batch)) return -1;          // the frame counts ride in the output until the row is done
    TdArgs a;
    a.enc = d_enc; a.table = m->d_table; a.U = m->d_U; a.proj = m->d_proj; a.out = m->d_out;
    a.st_f = d_st_f; a.st_score = d_st_score; a.st_i = d_st_i; a.st_owed = d_st_owed;
    a.labels = d_labels; a.frames = d_frames; a.durs = d_durations; a.lengths = d_lengths; a.scores = d_scores;
    a.batch = batch; a.T = T; a.V = m->V; a.blank = m->blank; a.H = m->H; a.J = m->J; a.act = m->activation;
    a.max_sym = m->max_symbols_per_frame; a.max_labels = max_labels;
    a.du = *du;
    const int R = nntk_shim_rnnt_tdt_dec_rows_per_group(batch, m->H, m->J, m->V, du->n);
    const size_t lds = td_lds_bytes(R, m->H, m->J, m->V + du->n);
    const dim3 grid((unsigned)((batch + R - 1) / R));
    if (R == 1) {
        if (lds > 48 * 1024 && nntk_set_max_dynamic_lds((const void *)rnnt_tdt_greedy_kernel<1>, lds)) return -1;
        hipLaunchKernelGGL(rnnt_tdt_greedy_kernel<1>, grid, dim3(RD_THREADS), lds, nntk_stream(), a);
    } else {
        if (lds > 48 * 1024 && nntk_set_max_dynamic_lds((const void *)rnnt_tdt_greedy_kernel<NNTK_RNNT_DEC_GROUP>, lds)) return -1;
        hipLaunchKernelGGL(rnnt_tdt_greedy_kernel<NNTK_RNNT_DEC_GROUP>, grid, dim3(RD_THREADS), lds, nntk_stream(), a);
    }
    NNTK_LAUNCH_CHECK("rnnt_tdt_greedy_kernel");
    return 0;
}

}  // extern "C"
