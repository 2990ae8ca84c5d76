// edit_distance.hip -- how wrong a hypothesis is: the Levenshtein distance of every hypothesis [B][n_hyp][max_hyp_len] (as the decoders
// leave them in device memory) to its row's reference, split into substitutions, deletions and insertions; the minimum word error
// rate (MWER) risk over an n-best list with its gradient; and the row scale that carries that gradient into a loss call.
//
// Definition.  h_1..h_m the hypothesis, r_1..r_n the reference.  D[0][j] = j (all deletions), D[i][0] = i (all insertions); for
// i, j >= 1 a cell takes the smallest of (1) D[i-1][j-1] + (h_i != r_j), a hit or substitution, (2) D[i][j-1] + 1, a deletion (r_j has
// no counterpart), (3) D[i-1][j] + 1, an insertion; on an equal distance the earlier candidate in that order wins.  A cell's three
// counts are its chosen predecessor's counts plus the chosen operation; the result is cell (m, n).  That is what a backtrace from
// (m, n) counts when it takes the first minimal predecessor in the same order.  Hits = n - S - D, distance = S + D + I.
//
// A cell is 8 bytes: distance | S << 16 | D << 32 | I << 48 (every count <= 32767), so an operation is one 64-bit add and the
// candidates are compared on the low 16 bits only: the tie-break is by candidate order, never by a count's value.
//
// Work split.  The dependency runs along anti-diagonals d = i + j.  Three rotating diagonals live in LDS, indexed along the pair's
// shorter side (at most min(m, n) + 1 cells), lanes over the cells of the diagonal, one synchronisation per diagonal.  A workgroup
// of four wavefronts owns four consecutive pairs and chooses from the lengths it reads (the hypothesis lengths are device memory):
// a pair with at most ED_WAVE_UNITS units on either side is swept by one wavefront -- the four of them side by side, synchronised
// by wavefront-scope fences only -- and a longer pair by the whole workgroup with a barrier per diagonal, after the short ones.
// The pair's units are staged in LDS once: all of them for a short pair and for the reference; of a long hypothesis as many as
// the 160 KiB leave room for (the rest is read from global memory).
//
// Word mode (sep >= 0).  edit_words_kernel first cuts every sequence at tokens equal to sep -- one workgroup per sequence, a word
// starts where a non-separator follows a separator or the start, its index is a ballot prefix count -- into records
// {start | length << 16, FNV-1a hash of the tokens}.  The same sweep then runs over records; two words are equal iff length and
// hash agree AND the tokens do: the hash only pre-filters, the decision is exact.
//
// No atomics: every output element has one writer.  The same bits on every call; a pair's result depends on nothing but the pair.
#include <stdint.h>
#include <type_traits>
#include "nntk_common.hpp"

#define ED_THREADS 256
#define ED_WAVES 4                        // wavefronts, and pairs, per workgroup
#define ED_WAVE_UNITS 256                 // a pair with at most this many units on either side is one wavefront's
#define ED_LDS_LIMIT (160 * 1024)

#define ED_WAVE_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); \
                            __builtin_amdgcn_wave_barrier();                        \
                            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); } while (0)

typedef unsigned long long ed_cell;
#define ED_SUB ((ed_cell)1 | ((ed_cell)1 << 16))
#define ED_DEL ((ed_cell)1 | ((ed_cell)1 << 32))
#define ED_INS ((ed_cell)1 | ((ed_cell)1 << 48))

// workspace, in 4-byte words: [reference lengths B | references B*maxR | reference word counts B | hypothesis word counts P]
// [reference word records B * ceil(maxR / 2), 8 bytes each] [hypothesis word records P * ceil(maxH / 2)]; the records start on
// 16-byte boundaries and are touched in word mode only
struct EdWs { size_t rcnt, hcnt, rrec, hrec, total; int rp, hp; };
static EdWs ed_ws(int B, int n_hyp, int maxH, int maxR) {
    EdWs l;
    const size_t b = B > 0 ? (size_t)B : 0, p = b * (size_t)(n_hyp > 0 ? n_hyp : 0);
    const size_t mh = maxH > 0 ? (size_t)maxH : 0, mr = maxR > 0 ? (size_t)maxR : 0;
    auto up = [](size_t x) { return (x + 3) & ~(size_t)3; };
    l.rp = (int)((mr + 1) / 2);
    l.hp = (int)((mh + 1) / 2);
    l.rcnt = b + b * mr;
    l.hcnt = l.rcnt + b;
    l.rrec = up(l.hcnt + p);
    l.hrec = l.rrec + up(2 * b * (size_t)l.rp);
    l.total = l.hrec + up(2 * p * (size_t)l.hp) + 4;
    return l;
}

// LDS of the sweep, in units and bytes.  A wavefront's slice: three diagonals of w_diag cells, then w_ru reference and w_hu
// hypothesis units.  The workgroup's form (only where a pair can be longer than ED_WAVE_UNITS): three diagonals of g_diag cells,
// all g_ru reference units, the first g_hu hypothesis units.
struct EdLds { int w_diag, w_ru, w_hu, w_slice, g_diag, g_ru, g_hu; size_t total; };
static EdLds ed_lds(int UH, int UR, int usz) {
    EdLds l;
    const int K = UH < UR ? UH : UR, big = UH > UR ? UH : UR;
    auto up = [](size_t x) { return (x + 15) & ~(size_t)15; };
    l.w_diag = (K < ED_WAVE_UNITS ? K : ED_WAVE_UNITS) + 1;
    l.w_ru = UR < ED_WAVE_UNITS ? UR : ED_WAVE_UNITS;
    l.w_hu = UH < ED_WAVE_UNITS ? UH : ED_WAVE_UNITS;
    l.w_slice = (int)up((size_t)3 * l.w_diag * sizeof(ed_cell) + (size_t)(l.w_ru + l.w_hu) * usz);
    l.total = (size_t)ED_WAVES * l.w_slice;
    l.g_diag = l.g_ru = l.g_hu = 0;
    if (big > ED_WAVE_UNITS) {
        l.g_diag = K + 1;
        l.g_ru = UR;
        const size_t fixed = (size_t)3 * l.g_diag * sizeof(ed_cell) + (size_t)UR * usz;     // <= 96 024 + 16 000 bytes
        const size_t room = (ED_LDS_LIMIT - fixed) / usz;
        l.g_hu = (size_t)UH < room ? UH : (int)room;
        const size_t g = up(fixed + (size_t)l.g_hu * usz);
        if (g > l.total) l.total = g;
    }
    return l;
}

// ---- word mode: cut every sequence into word records.  Sequence s < P is hypothesis s, s >= P reference s - P ----
__global__ __launch_bounds__(ED_THREADS) void edit_words_kernel(const int *__restrict__ hyp, const int *__restrict__ hyp_len, long P, int maxH,
                                                                const int *__restrict__ refs, const int *__restrict__ ref_len, int maxR,
                                                                int sep, int *hcnt, uint2 *hrec, int hp, int *rcnt, uint2 *rrec, int rp) {
    __shared__ int wave_tot[ED_WAVES];
    const long s = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const bool is_hyp = s < P;
    const int *tok = is_hyp ? hyp + s * maxH : refs + (s - P) * maxR;
    int len = is_hyp ? hyp_len[s] : ref_len[s - P];
    const int cap = is_hyp ? maxH : maxR;
    len = len < 0 ? 0 : len > cap ? cap : len;
    uint2 *rec = is_hyp ? hrec + s * hp : rrec + (s - P) * rp;
    int base = 0;
    for (int c0 = 0; c0 < len; c0 += ED_THREADS) {
        const int i = c0 + tid;
        const bool start = i < len && tok[i] != sep && (i == 0 || tok[i - 1] == sep);
        const unsigned long long bal = __ballot(start);
        if (lane == 0) wave_tot[w] = __popcll(bal);
        __syncthreads();
        int off = base, total = 0;
        for (int k = 0; k < ED_WAVES; ++k) {
            if (k < w) off += wave_tot[k];
            total += wave_tot[k];
        }
        if (start) {
            unsigned h = 2166136261u;
            int k = i;
            for (; k < len && tok[k] != sep; ++k) h = (h ^ (unsigned)tok[k]) * 16777619u;
            rec[off + __popcll(bal & ((1ull << lane) - 1))] = make_uint2((unsigned)i | ((unsigned)(k - i) << 16), h);
        }
        base += total;
        __syncthreads();
    }
    if (tid == 0) *(is_hyp ? hcnt + s : rcnt + (s - P)) = base;
}

// one side of a pair: its units (tokens, or word records) in LDS up to `staged`, in global memory behind; tok: the tokens a word
// record points into
template <bool WORD> struct EdSide {
    typedef typename std::conditional<WORD, uint2, int>::type unit;
    const unit *lds, *glob;
    const int *tok;
    int staged;
    __device__ __forceinline__ unit at(int i) const { return i < staged ? lds[i] : glob[i]; }
};

template <bool WORD>
__device__ __forceinline__ bool ed_differ(const EdSide<WORD> &H, int i, const EdSide<WORD> &R, int j) {
    if constexpr (!WORD) {
        return H.at(i) != R.at(j);
    } else {
        const uint2 a = H.at(i), b = R.at(j);
        if (a.y != b.y || (a.x >> 16) != (b.x >> 16)) return true;
        const int *x = H.tok + (a.x & 0xffffu), *y = R.tok + (b.x & 0xffffu);
        const int len = (int)(a.x >> 16);
        for (int k = 0; k < len; ++k)
            if (x[k] != y[k]) return true;
        return false;
    }
}

// G lanes (a wavefront, or the workgroup) sweep the (m + 1) x (n + 1) table of one pair; lane t of them.  diag: 3 x pitch cells.
// Leaves {distance, S, D, I} at out.  The callers synchronise the group before diag is written here and after it was read.
template <bool WORD, int G>
__device__ __forceinline__ void ed_sweep(int t, int m, int n, const EdSide<WORD> &H, const EdSide<WORD> &R, ed_cell *diag, int pitch,
                                         int *out) {
    const bool by_hyp = m <= n;                           // a cell's place in its diagonal: i when the hypothesis is the shorter side, else j
    const int o_del = by_hyp ? 0 : 1, o_ins = by_hyp ? 1 : 0;
    ed_cell *cur = diag, *p1 = diag + pitch, *p2 = diag + 2 * pitch;      // diagonals d, d - 1, d - 2
    for (int d = 0; d <= m + n; ++d) {
        const int lo = d > n ? d - n : 0, hi = d < m ? d : m;
        for (int i = lo + t; i <= hi; i += G) {
            const int j = d - i, p = by_hyp ? i : j;
            ed_cell c;
            if (i == 0) c = (ed_cell)j * ED_DEL;
            else if (j == 0) c = (ed_cell)i * ED_INS;
            else {
                c = p2[p - 1] + (ed_differ<WORD>(H, i - 1, R, j - 1) ? ED_SUB : 0);
                const ed_cell del = p1[p - o_del] + ED_DEL, ins = p1[p - o_ins] + ED_INS;
                if ((del & 0xffffu) < (c & 0xffffu)) c = del;
                if ((ins & 0xffffu) < (c & 0xffffu)) c = ins;
            }
            cur[p] = c;
        }
        if (G == 64) ED_WAVE_SYNC(); else __syncthreads();
        ed_cell *const r = p2;
        p2 = p1; p1 = cur; cur = r;
    }
    if (t < 4) out[t] = (int)((p1[by_hyp ? m : n] >> (16 * t)) & 0xffffu);      // p1: the last diagonal written
}

// the unit counts of pair q: m < 0 = the decoders' "no hypothesis" slot
template <bool WORD>
__device__ __forceinline__ void ed_dims(long q, int n_hyp, int maxH, const int *hyp_len, const int *ref_len, const int *hcnt, const int *rcnt,
                                        int &m, int &n) {
    const long b = q / n_hyp;
    const int hl = hyp_len[q];
    if constexpr (WORD) { m = hl < 0 ? -1 : hcnt[q]; n = rcnt[b]; }
    else { m = hl < 0 ? -1 : hl > maxH ? maxH : hl; n = ref_len[b]; }
}

template <bool WORD>
__global__ __launch_bounds__(ED_THREADS) void edit_distance_kernel(const int *__restrict__ hyp, const int *__restrict__ hyp_len, long P,
                                                                   int n_hyp, int maxH, const int *__restrict__ ws_ints, int maxR, EdWs wl,
                                                                   EdLds ll, int *counts, int *ref_units) {
    typedef typename EdSide<WORD>::unit unit;
    extern __shared__ __align__(16) unsigned char ed_smem[];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const long q0 = (long)blockIdx.x * ED_WAVES;
    const int *ref_len = ws_ints, *refs = ws_ints + (P / n_hyp), *rcnt = ws_ints + wl.rcnt, *hcnt = ws_ints + wl.hcnt;
    const uint2 *rrec = (const uint2 *)(ws_ints + wl.rrec), *hrec = (const uint2 *)(ws_ints + wl.hrec);

    // one side's units in global memory
    auto side = [&](long q, bool is_hyp, const unit *lds, int staged) {
        EdSide<WORD> s;
        const long b = q / n_hyp;
        s.tok = is_hyp ? hyp + q * maxH : refs + b * maxR;
        if constexpr (WORD) s.glob = is_hyp ? hrec + q * wl.hp : rrec + b * wl.rp;
        else s.glob = s.tok;
        s.lds = lds;
        s.staged = staged;
        return s;
    };

    // short pairs: wavefront w sweeps pair q0 + w in its own slice
    {
        const long q = q0 + w;
        if (q < P) {
            int m, n;
            ed_dims<WORD>(q, n_hyp, maxH, hyp_len, ref_len, hcnt, rcnt, m, n);
            if (ref_units && q % n_hyp == 0 && lane == 0) ref_units[q / n_hyp] = n;
            if (m < 0) {
                if (lane < 4) counts[q * 4 + lane] = -1;
            } else if (m <= ED_WAVE_UNITS && n <= ED_WAVE_UNITS) {
                unsigned char *slice = ed_smem + (size_t)w * ll.w_slice;
                ed_cell *diag = (ed_cell *)slice;
                unit *ru = (unit *)(slice + (size_t)3 * ll.w_diag * sizeof(ed_cell)), *hu = ru + ll.w_ru;
                const EdSide<WORD> H = side(q, true, hu, m), R = side(q, false, ru, n);
                for (int k = lane; k < m; k += 64) hu[k] = H.glob[k];
                for (int k = lane; k < n; k += 64) ru[k] = R.glob[k];
                ED_WAVE_SYNC();
                ed_sweep<WORD, 64>(lane, m, n, H, R, diag, ll.w_diag, counts + q * 4);
            }
        }
    }
    // long pairs: the whole workgroup, one after the other (every lane reads the same lengths: the branch is uniform)
    if (ll.g_diag == 0) return;
    for (int k = 0; k < ED_WAVES; ++k) {
        const long q = q0 + k;
        if (q >= P) break;
        int m, n;
        ed_dims<WORD>(q, n_hyp, maxH, hyp_len, ref_len, hcnt, rcnt, m, n);
        if (m < 0 || (m <= ED_WAVE_UNITS && n <= ED_WAVE_UNITS)) continue;
        ed_cell *diag = (ed_cell *)ed_smem;
        unit *ru = (unit *)(ed_smem + (size_t)3 * ll.g_diag * sizeof(ed_cell)), *hu = ru + ll.g_ru;
        const int hs = m < ll.g_hu ? m : ll.g_hu;
        const EdSide<WORD> H = side(q, true, hu, hs), R = side(q, false, ru, n);
        __syncthreads();                                  // the slices, or the pair before, are done with
        for (int i = tid; i < hs; i += ED_THREADS) hu[i] = H.glob[i];
        for (int i = tid; i < n; i += ED_THREADS) ru[i] = R.glob[i];
        __syncthreads();
        ed_sweep<WORD, ED_THREADS>(tid, m, n, H, R, diag, ll.g_diag, counts + q * 4);
    }
}

// ---- MWER: one lane per row, the row's n_hyp slots in index order, in double, rounded to f32 once ----
__global__ __launch_bounds__(256) void mwer_kernel(const float *__restrict__ logp, const int *__restrict__ err, int err_stride, int B,
                                                   int n_hyp, float *risk_rows, float *dlogp) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const float *lp = logp + (long)b * n_hyp;
    const int *e = err + (long)b * n_hyp * err_stride;
    float *g = dlogp ? dlogp + (long)b * n_hyp : nullptr;
    double mx = -INFINITY, esum = 0.0;
    int valid = 0;
    for (int k = 0; k < n_hyp; ++k) {
        const int ek = e[(long)k * err_stride];
        if (ek < 0) continue;
        ++valid;
        esum += (double)ek;
        const double v = (double)lp[k];
        if (v > mx) mx = v;
    }
    double risk = 0.0;
    const bool live = valid > 0 && mx > -INFINITY && mx < INFINITY;       // else: nothing to renormalise, risk 0 and gradient 0
    double z = 0.0, mean = 0.0;
    if (live) {
        mean = esum / (double)valid;
        for (int k = 0; k < n_hyp; ++k)
            if (e[(long)k * err_stride] >= 0) z += exp((double)lp[k] - mx);
        for (int k = 0; k < n_hyp; ++k) {
            const int ek = e[(long)k * err_stride];
            if (ek >= 0) risk += exp((double)lp[k] - mx) / z * ((double)ek - mean);
        }
    }
    if (risk_rows) risk_rows[b] = (float)risk;
    if (g)
        for (int k = 0; k < n_hyp; ++k) {
            const int ek = e[(long)k * err_stride];
            g[k] = live && ek >= 0 ? (float)(exp((double)lp[k] - mx) / z * (((double)ek - mean) - risk)) : 0.0f;
        }
}

// ---- out[r][:] = x[r][:] * scale[r]; a scale of exactly 0 gives zeros whatever the row holds.  V4: rows of whole, aligned float4 ----
template <bool V4>
__global__ __launch_bounds__(256) void row_scale_kernel(const float *__restrict__ x, const float *__restrict__ scale, long rows,
                                                        long row_floats, float *out) {
    const long n = V4 ? row_floats / 4 : row_floats;
    for (long r = blockIdx.y; r < rows; r += gridDim.y) {
        const float s = scale[r];
        for (long c = (long)blockIdx.x * blockDim.x + threadIdx.x; c < n; c += (long)gridDim.x * blockDim.x) {
            if constexpr (V4) {
                float4 v = ((const float4 *)(x + r * row_floats))[c];
                v = s == 0.0f ? make_float4(0.0f, 0.0f, 0.0f, 0.0f) : make_float4(v.x * s, v.y * s, v.z * s, v.w * s);
                ((float4 *)(out + r * row_floats))[c] = v;
            } else {
                const float v = x[r * row_floats + c];
                out[r * row_floats + c] = s == 0.0f ? 0.0f : v * s;
            }
        }
    }
}

extern "C" {

size_t nntk_shim_edit_distance_workspace_floats(int batch, int n_hyp, int max_hyp_len, int max_ref_len) {
    return ed_ws(batch, n_hyp, max_hyp_len, max_ref_len).total;
}

int nntk_shim_edit_distance(const int *d_hyp, const int *d_hyp_len, int B, int n_hyp, int maxH, const int *h_refs, const int *h_ref_len,
                            int maxR, int sep, int *d_counts, int *d_ref_units, float *d_ws) {
    if (B <= 0 || n_hyp <= 0) return 0;
    if (maxH > NNTK_EDIT_MAX_HYP_LEN || maxR > NNTK_EDIT_MAX_REF_LEN)
        return nntk_fail_msg("nntk_edit_distance_device: a length limit is beyond what the cells and one workgroup's LDS hold");
    const EdWs wl = ed_ws(B, n_hyp, maxH, maxR);
    const long P = (long)B * n_hyp;
    int *d_ints = (int *)d_ws;
    if (nntk_shim_upload_ints(d_ints, h_ref_len, B)) return -1;
    if (maxR > 0 && nntk_shim_upload_ints(d_ints + B, h_refs, (long)B * maxR)) return -1;
    const bool word = sep >= 0;
    if (word) {
        hipLaunchKernelGGL(edit_words_kernel, dim3((unsigned)(P + B)), dim3(ED_THREADS), 0, nntk_stream(), d_hyp, d_hyp_len, P, maxH,
                           d_ints + B, d_ints, maxR, sep, d_ints + wl.hcnt, (uint2 *)(d_ints + wl.hrec), wl.hp, d_ints + wl.rcnt,
                           (uint2 *)(d_ints + wl.rrec), wl.rp);
        NNTK_LAUNCH_CHECK("edit_words_kernel");
    }
    const EdLds ll = word ? ed_lds(wl.hp, wl.rp, (int)sizeof(uint2)) : ed_lds(maxH, maxR, (int)sizeof(int));
    if (ll.total > ED_LDS_LIMIT) return nntk_fail_msg("nntk_edit_distance_device: the pair's diagonals do not fit one workgroup's LDS");
    const unsigned grid = (unsigned)((P + ED_WAVES - 1) / ED_WAVES);
#define ED_LAUNCH(WORD)                                                                                                          \
    do {                                                                                                                         \
        if (ll.total > 48 * 1024 && nntk_set_max_dynamic_lds((const void *)edit_distance_kernel<WORD>, ll.total)) return -1;      \
        hipLaunchKernelGGL(edit_distance_kernel<WORD>, dim3(grid), dim3(ED_THREADS), ll.total, nntk_stream(), d_hyp, d_hyp_len, P,  \
                           n_hyp, maxH, d_ints, maxR, wl, ll, d_counts, d_ref_units);                                            \
    } while (0)
    if (word) ED_LAUNCH(true);
    else ED_LAUNCH(false);
#undef ED_LAUNCH
    NNTK_LAUNCH_CHECK("edit_distance_kernel");
    return 0;
}

int nntk_shim_mwer(const float *d_logp, const int *d_err, int err_stride, int B, int n_hyp, float *d_risk_rows, float *d_dlogp) {
    if (B <= 0) return 0;
    hipLaunchKernelGGL(mwer_kernel, dim3((unsigned)nntk_cdiv(B, 256)), dim3(256), 0, nntk_stream(), d_logp, d_err, err_stride, B, n_hyp,
                       d_risk_rows, d_dlogp);
    NNTK_LAUNCH_CHECK("mwer_kernel");
    return 0;
}

int nntk_shim_row_scale(const float *d_x, const float *d_scale, long rows, long row_floats, float *d_out) {
    if (rows <= 0 || row_floats <= 0) return 0;
    const bool v4 = row_floats % 4 == 0 && (((uintptr_t)d_x | (uintptr_t)d_out) & 15) == 0;
    const long n = v4 ? row_floats / 4 : row_floats;
    const long bx = (n + 255) / 256;
    const dim3 grid((unsigned)(bx < 4096 ? bx : 4096), (unsigned)(rows < 65535 ? rows : 65535));
    if (v4) hipLaunchKernelGGL(row_scale_kernel<true>, grid, dim3(256), 0, nntk_stream(), d_x, d_scale, rows, row_floats, d_out);
    else hipLaunchKernelGGL(row_scale_kernel<false>, grid, dim3(256), 0, nntk_stream(), d_x, d_scale, rows, row_floats, d_out);
    NNTK_LAUNCH_CHECK("row_scale_kernel");
    return 0;
}

}  // extern "C"
