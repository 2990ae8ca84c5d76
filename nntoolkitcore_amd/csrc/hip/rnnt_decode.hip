// rnnt_decode.hip -- greedy RNN-Transducer decoding with the network inside the search: one launch runs every row's whole decision loop
// (joiner -> vocabulary projection -> argmax / log-sum-exp -> on a label, the prediction network's LSTM step and its projection).
//
// Work split.  A workgroup of RD_THREADS lanes owns R rows (R = 1 or NNTK_RNNT_DEC_GROUP; the launcher's choice, never visible in the bits) and
// steps them together: one pass over the vocabulary matrix serves the R rows' decisions, one pass over U the rows that emitted (the step
// is skipped when none did).  h, c, g, the joiner output and the logits / gate pre-activations live in LDS; the weights are read through
// L2, every matrix in the caller's own [K][N] layout: a lane owns output column n, so a wavefront's load of row k is 256 contiguous bytes.
// Rows never talk to each other: no flags, no spins, no atomics; a workgroup whose rows are done leaves.
//
// Bits.  Every output element of a matrix-vector product is  ((p0 + p1) + (p2 + p3)) + bias  with p_i the fmaf chain over k = i mod 4,
// ascending -- whatever R, the batch, T or the chunking.  The maximum is exact; ties go to the lowest index in the lane scan, the
// butterfly and the scan over the wavefronts.  sum exp(x - max): expf per element, added in double in a fixed order (a lane's elements
// ascending, the xor butterfly, the wavefronts ascending); lp = -log(sum) in double; the score is carried in double and rounded to f32
// only in the output, so a stream's chunks add up exactly as the one-shot call does.
//
// Precomputed at create / load time (rnnt_dec_table_kernel): table[v][:] = embed[v] W + b_i + b_h, so an emission costs h U alone.
#include "rnnt_dec_common.hpp"                // rd_matvec, rd_act, rd_sigmoid, the reduction butterflies: shared with rnnt_beam.hip

struct RnntDecArgs {
    const float *enc;                      // [batch][T][J]
    const float *table, *U, *proj, *out;   // [V][4H] | [H][4H] | [H][J] b[J] or NULL | [J][V] b[V]
    float *st_f;                           // per row h [H] | c [H] | g [J], or NULL: every row from the start, nothing kept
    double *st_score;                      // [batch]
    int *st_i;                             // [batch][4]: started | s | labels | frames consumed
    int *labels, *frames, *lengths;        // lengths holds the call's n_frames on entry
    float *scores;
    int batch, T, V, blank, H, J, act, max_sym, max_labels;
};

// fixed part of the LDS, then the float arrays: h [R][Hp] | c [R][Hp] | g [R][Jp] | z [R][Jp] | buf [R][Wp]
template <int R> struct RdShared {
    double red_sum[R][RD_WAVES];
    double score[R > 1 ? R : 2];
    float red_max[R][RD_WAVES];
    int red_idx[R][RD_WAVES];
    int t[4], s[4], count[4], n[4], base[4], emit[4], row[4], fresh[4], best[4], live[4];
};

static size_t rd_lds_bytes(int R, int H, int J, int V) {
    const size_t Hp = (size_t)(H + 3) & ~(size_t)3, Jp = (size_t)(J + 3) & ~(size_t)3;
    const size_t W = 4 * (size_t)H > (size_t)V ? 4 * (size_t)H : (size_t)V, Wp = (W + 3) & ~(size_t)3;
    const size_t fixed = R == 1 ? sizeof(RdShared<1>) : sizeof(RdShared<NNTK_RNNT_DEC_GROUP>);
    return ((fixed + 15) & ~(size_t)15) + (size_t)R * (2 * Hp + 2 * Jp + Wp) * sizeof(float);
}

template <int R>
__global__ __launch_bounds__(RD_THREADS) void rnnt_greedy_kernel(const RnntDecArgs a) {
    extern __shared__ __align__(16) unsigned char rd_smem[];
    RdShared<R> &sh = *(RdShared<R> *)rd_smem;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int H = a.H, J = a.J, V = a.V, G = 4 * H;
    const int Hp = (H + 3) & ~3, Jp = (J + 3) & ~3, Wp = ((G > V ? G : V) + 3) & ~3;
    float *sh_h = (float *)(rd_smem + ((sizeof(RdShared<R>) + 15) & ~(size_t)15));
    float *sh_c = sh_h + R * Hp, *sh_g = sh_c + R * Hp, *sh_z = sh_g + R * Jp, *sh_buf = sh_z + R * Jp;
    const float *pbias = a.proj ? a.proj + (size_t)H * J : nullptr;
    const float *obias = a.out + (size_t)J * V;

    if (tid < R) {
        const int r = tid, b = blockIdx.x * R + r;
        const bool valid = b < a.batch;
        const bool started = valid && a.st_i && a.st_i[4 * b] != 0;
        sh.row[r] = valid ? b : -1;
        sh.n[r] = valid ? a.lengths[b] : 0;
        sh.t[r] = 0;
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
        // the joiner; a row that is done keeps an all-zero z (its logits are computed and ignored)
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
        // the vocabulary projection, then each lane's part of the argmax
        float m[R];
        int mi[R];
#pragma unroll
        for (int r = 0; r < R; ++r) { m[r] = -INFINITY; mi[r] = V; }
        for (int n = tid; n < V; n += RD_THREADS) {
            float x[R];
            rd_matvec<R>(a.out, J, V, n, sh_z, Jp, x);
#pragma unroll
            for (int r = 0; r < R; ++r) {
                x[r] += obias[n];
                sh_buf[r * Wp + n] = x[r];
                if (x[r] > m[r] || (x[r] == m[r] && n < mi[r])) { m[r] = x[r]; mi[r] = n; }
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
        }
        __syncthreads();
        if (tid < R && sh.live[tid]) {
            const int r = tid, b = sh.row[r];
            double sum = 0.0;
            for (int w = 0; w < RD_WAVES; ++w) sum += sh.red_sum[r][w];
            const int k = sh.best[r] < V ? sh.best[r] : a.blank;               // (no finite or infinite maximum: NaN weights; stay in bounds)
            sh.score[r] -= log(sum);                                           // lp = x[k] - max - log(sum), x[k] = max
            if (k == a.blank) {
                sh.t[r] += 1; sh.s[r] = 0; sh.emit[r] = -1;
            } else {
                const size_t at = (size_t)b * a.max_labels + sh.count[r];
                a.labels[at] = k;
                if (a.frames) a.frames[at] = sh.base[r] + sh.t[r];
                sh.count[r] += 1; sh.emit[r] = k;
                if (++sh.s[r] == a.max_sym) { sh.t[r] += 1; sh.s[r] = 0; }     // the cap moves on without scoring a blank
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
            a.labels[(size_t)b * a.max_labels + i] = -1;
            if (a.frames) a.frames[(size_t)b * a.max_labels + i] = -1;
        }
        if (tid == 0) {
            if (a.st_i) {
                a.st_i[4 * b] = 1; a.st_i[4 * b + 1] = sh.s[r]; a.st_i[4 * b + 2] = cnt; a.st_i[4 * b + 3] = sh.base[r] + sh.t[r];
                a.st_score[b] = sh.score[r];
            }
            a.lengths[b] = cnt;
            if (a.scores) a.scores[b] = (float)sh.score[r];
        }
    }
}

// table[v][n] = (sum over e, ascending, of embed[v][e] W[e][n]) + b_i[n] + b_h[n]
__global__ __launch_bounds__(256) void rnnt_dec_table_kernel(const float *__restrict__ embed, const float *__restrict__ lstm, int E, int H,
                                                             float *__restrict__ table) {
    const int G = 4 * H, v = blockIdx.y;
    const float *W = lstm, *bi = lstm + (size_t)(E + H) * G, *bh = bi + G;
    const float *x = embed + (size_t)v * E;
    for (int n = blockIdx.x * 256 + threadIdx.x; n < G; n += gridDim.x * 256) {
        float acc = 0.0f;
        for (int e = 0; e < E; ++e) acc = fmaf(x[e], W[(size_t)e * G + n], acc);
        table[(size_t)v * G + n] = (acc + bi[n]) + bh[n];
    }
}

__global__ void rnnt_dec_reset_kernel(int *st_i, const int *rows, int n_rows) {
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n_rows; i += gridDim.x * 256) st_i[4 * rows[i]] = 0;
}

extern "C" {

int nntk_shim_rnnt_dec_rows_per_group(int batch, int H, int J, int V) {
    return batch > NNTK_RNNT_DEC_GROUP_BATCH && rd_lds_bytes(NNTK_RNNT_DEC_GROUP, H, J, V) <= RD_LDS_MAX ? NNTK_RNNT_DEC_GROUP : 1;
}

int nntk_shim_rnnt_dec_table(const float *d_embed, const float *d_lstm, int V, int E, int H, float *d_table) {
    const int gx = (4 * H + 255) / 256;
    hipLaunchKernelGGL(rnnt_dec_table_kernel, dim3((unsigned)(gx > 16 ? 16 : gx), (unsigned)V), dim3(256), 0, nntk_stream(), d_embed, d_lstm,
                       E, H, d_table);
    NNTK_LAUNCH_CHECK("rnnt_dec_table_kernel");
    return 0;
}

int nntk_shim_rnnt_dec_reset(int *d_st_i, const int *d_rows, int n_rows) {
    if (n_rows <= 0) return 0;
    hipLaunchKernelGGL(rnnt_dec_reset_kernel, dim3((unsigned)((n_rows + 255) / 256)), dim3(256), 0, nntk_stream(), d_st_i, d_rows, n_rows);
    NNTK_LAUNCH_CHECK("rnnt_dec_reset_kernel");
    return 0;
}

int nntk_shim_rnnt_greedy(const nntk_shim_rnnt_dec *m, const float *d_enc, int batch, int T, const int *h_n_frames, int max_labels,
                          float *d_st_f, double *d_st_score, int *d_st_i, int *d_labels, int *d_frames, int *d_lengths, float *d_scores) {
    if (batch <= 0) return 0;
    if (m->E < 1 || m->H < 1 || m->J < 1 || m->V < 2 || m->H > NNTK_RNNT_DEC_MAX_WIDTH || m->J > NNTK_RNNT_DEC_MAX_WIDTH ||
        m->V > NNTK_RNNT_DEC_MAX_V || rd_lds_bytes(1, m->H, m->J, m->V) > RD_LDS_MAX)
        return nntk_fail_msg("nntk_rnnt_greedy_decode_device: the model is beyond the decoding kernel's limits");
    if (nntk_shim_upload_ints(d_lengths, h_n_frames, batch)) return -1;          // the frame counts ride in the output until the row is done
    RnntDecArgs a;
    a.enc = d_enc; a.table = m->d_table; a.U = m->d_U; a.proj = m->d_proj; a.out = m->d_out;
    a.st_f = d_st_f; a.st_score = d_st_score; a.st_i = d_st_i;
    a.labels = d_labels; a.frames = d_frames; a.lengths = d_lengths; a.scores = d_scores;
    a.batch = batch; a.T = T; a.V = m->V; a.blank = m->blank; a.H = m->H; a.J = m->J; a.act = m->activation;
    a.max_sym = m->max_symbols_per_frame; a.max_labels = max_labels;
    const int R = nntk_shim_rnnt_dec_rows_per_group(batch, m->H, m->J, m->V);
    const size_t lds = rd_lds_bytes(R, m->H, m->J, m->V);
    const dim3 grid((unsigned)((batch + R - 1) / R));
    if (R == 1) {
        if (lds > 48 * 1024 && nntk_set_max_dynamic_lds((const void *)rnnt_greedy_kernel<1>, lds)) return -1;
        hipLaunchKernelGGL(rnnt_greedy_kernel<1>, grid, dim3(RD_THREADS), lds, nntk_stream(), a);
    } else {
        if (lds > 48 * 1024 && nntk_set_max_dynamic_lds((const void *)rnnt_greedy_kernel<NNTK_RNNT_DEC_GROUP>, lds)) return -1;
        hipLaunchKernelGGL(rnnt_greedy_kernel<NNTK_RNNT_DEC_GROUP>, grid, dim3(RD_THREADS), lds, nntk_stream(), a);
    }
    NNTK_LAUNCH_CHECK("rnnt_greedy_kernel");
    return 0;
}

}  // extern "C"
