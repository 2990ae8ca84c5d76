// ctc_beam.hip -- CTC prefix beam search (Graves 2012; Hannun et al. 2014) on softmax probabilities [B][T][C], rows ragged, on acoustic
// scores alone or fused with a token-level n-gram language model (the LM instantiations; "Language model" below): per row the W best label prefixes per frame, each with the mass of its alignments ending in blank (p_b) and in its last
// label (p_nb), and after the last frame an n-best list with log-probabilities.  INTEGRATION.md "CTC prefix beam search" fixes the
// semantics (candidate cells, merging, the canonical-index tie rule) exactly; this file follows them cell by cell.
//
// Range.  Prefix masses fall like C^-T: every mass is an "xf" (ctc_xf.hpp), and the beam is ordered by a 64-bit integer key that is
// monotone in (exponent, mantissa), zero for a zero mass.
//
// Work split.  ctc_beam_cut_kernel (only when a class cut applies): a wavefront per frame finds the cutoff_top_n-th largest non-blank
// probability by bisection on the float bits and writes the frame's (class, probability) pairs in ascending class order -- parallel
// over B*T, off the serial chain.  ctc_beam_kernel: one 256-lane workgroup per row, the beam resident in LDS for all frames.  A frame
// is: stays and merge detection (lanes over beam entries / entry pairs), the W x (n + 1) cell matrix (lanes over cells), the at most
// W merges, the selection, the new beam.  Selection: one reduction gives the largest and smallest non-zero key; a bisection between
// them stops as soon as W <= count(key >= theta) <= 256 (or at a single key value, when more than 256 cells tie there); the survivors
// are compacted in cell order and ranked against each other by counting, which yields the descending order and the lower-index tie
// rule at once.  No atomics anywhere: every count is a ballot.  The next frame's probabilities are loaded before the frame's first
// barrier (the barriers wait for LDS only) and land in the other half of a double buffer at its end.  Per entry and frame one
// (parent rank | prefix length, class or -1) record and the (p_b, p_nb) pair go to the workspace: the only global stores of the loop.
// ctc_beam_backtrack_kernel: a workgroup per row stages the records of a block of frames in LDS and a lane per hypothesis walks them
// from the last frame, writing labels in forward order, then the -1 padding, the lengths and the scores.  ctc_beam_commit_kernel (a
// stream's push) does the same per surviving entry for the frames of the push and appends to the strings the handle carries.
//
// Shared pieces, each written once.  beam_walk_records: the staged walk of the records, with a visitor per label (backtrack: write at
// the position counted down; commit: write at the position the record names).  beam_final_rank: the end-of-sentence ranking, for the
// one-shot call's tail and the commit.  The commit's `put` / slot_of / entry_of: one body for "entry k is hypothesis k" and for the
// ranking's order.  beam_pad: what stands behind a hypothesis.  beam_dispatch: the host's runtime bools as template arguments.
//
// Prefix identity.  No label string is compared in the frame loop.  A prefix is known by a 64-bit hash chained over its labels
// (splitmix64 finaliser), its length and its last class; an entry also carries its parent prefix's hash.  Entry j merges into the
// extend cell (i, c) when j's parent hash is i's hash, j is one label longer than i and j's last class is c.  Unlike a parent RANK,
// this also recognises a prefix that left the beam and came back while its child stayed.  Two different prefixes of one length are
// taken for one with probability 2^-64 per compared pair.
//
// Language model (LM instantiations only; the others are compiled without any of it).  Every beam entry carries the state of a
// deterministic backoff automaton (one more int in the LDS state block, and in the carry of a stream).  The extend cell (i, c) is
// multiplied by F(state_i, c): beam_lm_walk takes the state's backoffs until a state has an arc labelled c -- a binary search over the
// state's sorted 16-byte arc records per step -- multiplying the backoff factors and the arc's factor from left to right, or the
// unknown-label factor when state 0 has no such arc.  The walk is bounded by the table's longest backoff chain as a loop count as well
// as by reaching state 0.  Cells stay 8 bytes: the next state is looked up again for the at most W surviving extend cells.  After the
// row's last frame every total is multiplied by the end-of-sentence factor of its state and the entries are ranked again; the
// backtrack (or the commit of a stream) reports in that order, and a stream carries the beam as it was before it.
//
// Label timestamps (DETAIL instantiations only; INTEGRATION.md "Label timestamps and confidences").  A label's frame is the latest frame
// at which entering the label outweighed continuing it.  The records already say where a label entered (class >= 0, at the length it
// made).  The one new bit: when a stay is merged into an extend cell, the merging lane compares extension and stay by their keys just
// before it sums them, and a merge with extension > stay is recorded with class -2 instead of -1.  A walker going backwards gives
// position len - 1 the frame of the first extension-or-(-2) record it meets at length len and ignores the earlier ones; `r.y >= 0`
// walkers never see the mark.  Confidence: ln of the acoustic probability of the label at that frame, gathered by the walker.
#include <stdint.h>
#include <limits.h>
#include <type_traits>
#include "nntk_common.hpp"
#include "ctc_xf.hpp"

#define BEAM_MAX_W NNTK_CTC_BEAM_MAX_W    // (the three limits the host layer checks too: nntk_shim.h)
#define BEAM_MAX_CELLS NNTK_CTC_BEAM_MAX_CELLS  // W * (n + 1) cells of 8 bytes: 128 KiB of the 160 KiB of LDS
#define BEAM_LIST 256                     // survivors ranked against each other
#define BEAM_PF 4                         // staged words a lane carries in registers across the selection
#define BEAM_BT_RECORDS 8192              // backtrack: records staged per block of frames (64 KiB)
#define BEAM_MAX_T NNTK_CTC_BEAM_MAX_T    // the prefix length shares a signed word with the parent rank: length << 8 < 2^31

typedef unsigned long long u64;

// workspace, in 4-byte words: [ints: input lengths B | final beam size B] [records: B*T*W int2] [masses: B*T*W float4]
// [class cut: B*T*ncut (class, prob) pairs] [LM only: final order B*W ints | final masses B*W float4]; every part starts on a 16-byte
// boundary
struct BeamLayout { size_t ints, hist, mass, cut, forder, fmass, total; };
static BeamLayout beam_layout(int B, int T, int W, int ncut, bool lm = false) {
    BeamLayout l;
    const size_t b = B > 0 ? (size_t)B : 0, t = T > 0 ? (size_t)T : 0, w = W > 0 ? (size_t)W : 0, n = ncut > 0 ? (size_t)ncut : 0;
    auto up = [](size_t x) { return (x + 3) & ~(size_t)3; };
    l.ints = 0;
    l.hist = up(2 * b);
    l.mass = l.hist + up(2 * b * t * w);
    l.cut = l.mass + 4 * b * t * w;
    l.forder = l.cut + up(2 * b * t * n);
    l.fmass = l.forder + (lm ? up(b * w) : 0);
    l.total = l.fmass + (lm ? 4 * b * w : 0) + 4;
    return l;
}
// 0: every non-blank class is expanded
static int beam_ncut(int C, int cutoff_top_n) { return cutoff_top_n <= 0 || cutoff_top_n >= C - 1 ? 0 : cutoff_top_n; }

// LDS of ctc_beam_kernel, byte offsets; every part 16-byte aligned
struct BeamLds { unsigned cells, stage, state, frame, sel, lkey, lidx, cnt, red, total; };
__host__ __device__ static inline BeamLds beam_lds(int W, int n, int C, bool cut, bool stage, bool lm = false) {
    BeamLds l;
    auto up = [](unsigned x) { return (x + 15u) & ~15u; };
    l.cells = 0;
    l.stage = up(8u * (unsigned)W * (unsigned)(n + 1));
    l.state = l.stage + (stage ? up(cut ? 16u * (unsigned)n : 8u * (unsigned)C) : 0u);
    // [2] x { p_b, p_nb, hash, parent hash : 8 bytes; last, len, home : 4 bytes; LM: the LM state, 4 bytes } [W]
    l.frame = l.state + up(2u * (lm ? 48u : 44u) * (unsigned)W);
    l.sel = l.frame + up(32u * (unsigned)W);            // stay p_b', stay p_nb', p_b + p_nb, record: 8 bytes each [W]
    l.lkey = l.sel + up(4u * (unsigned)W);
    l.lidx = l.lkey + 8u * BEAM_LIST;
    l.cnt = l.lidx + 4u * BEAM_LIST;
    l.red = l.cnt + 2u * 16u * (BEAM_MAX_CELLS / CTC_THREADS);
    l.total = l.red + 128u;
    return l;
}

__device__ __forceinline__ u64 beam_key(float2 w) {
    const unsigned mb = __float_as_uint(w.x);
    return mb == 0u ? 0ull : ((u64)(unsigned)(__float_as_int(w.y) - CTC_EZERO) << 23) | (u64)(mb & 0x7fffffu);
}
__device__ __forceinline__ u64 beam_hash(u64 h, int c) {
    u64 x = h + (u64)(unsigned)(c + 1) * 0x9E3779B97F4A7C15ull;
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27; x *= 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
__device__ __forceinline__ xf xf_add2(xf a, xf b) { return xf_add3(a, b, xf_zero()); }
// ln(p_b + p_nb) of a final entry, once per hypothesis: double, libm log.  One expression for the one-shot and the streaming form.
__device__ __forceinline__ float beam_score(float4 m) {
    xf pb, pnb;
    pb.m = m.x; pb.e = __float_as_int(m.y);
    pnb.m = m.z; pnb.e = __float_as_int(m.w);
    const xf s = xf_add2(pb, pnb);
    return (float)((double)s.e * 0.69314718055994530942 + log((double)s.m));
}
// a label's confidence: ln of its acoustic probability at its reported frame, in double, rounded once.  One expression for both forms.
__device__ __forceinline__ float beam_logp(float p) { return (float)log((double)p); }
// The end-of-sentence ranking over the nb finalised keys in LDS (the caller stored them and passed a barrier): rank = the place of entry
// tid in descending order, ties to the lower entry, or -1 for an exact zero or no entry; alive = the entries that are not zero.  One
// expression for the one-shot call's tail and the stream's commit.
struct BeamFinalRank { int rank, alive; };
__device__ __forceinline__ BeamFinalRank beam_final_rank(const u64 *keys, int nb, int tid) {
    const u64 k = tid < nb ? keys[tid] : 0ull;
    int rank = 0, alive = 0;
    for (int u = 0; u < nb; ++u) {
        const u64 ku = keys[u];
        rank += (ku > k || (ku == k && u < tid)) ? 1 : 0;
        alive += ku != 0ull ? 1 : 0;
    }
    return {k != 0ull ? rank : -1, alive};
}

// ---- language model: F(state, c) and next(state, c) of INTEGRATION.md "Language-model fusion" ----
__device__ __forceinline__ xf xf_mul(xf a, xf b) { return xf_norm(a.m * b.m, a.e + b.e); }
__device__ __forceinline__ xf beam_lm_xf(int m, int e) { xf r; r.m = __int_as_float(m); r.e = e; return r; }
__device__ static xf beam_lm_walk(const nntk_shim_lm &lm, int s, int c, int &next) {
    const int4 *arcs = (const int4 *)lm.d_arcs, *states = (const int4 *)lm.d_states, *fac = (const int4 *)lm.d_factors;
    xf f = xf_one();
    s = min(max(s, 0), lm.n_states - 1);
    for (int d = 0; d <= lm.depth; ++d) {                                      // at most depth backoffs: depth + 1 states
        const int4 st = states[s];
        int a = st.x, z = st.x + st.y - 1;
        while (a <= z) {
            const int mid = a + ((z - a) >> 1);
            const int4 arc = arcs[mid];
            if (arc.x == c) { next = arc.y; return xf_mul(f, beam_lm_xf(arc.z, arc.w)); }
            if (arc.x < c) a = mid + 1; else z = mid - 1;
        }
        if (s == 0) break;
        const int4 bf = fac[s];
        f = xf_mul(f, beam_lm_xf(bf.x, bf.y));
        s = min(max(st.z, 0), s - 1);                                          // shorter contexts first: a walk only descends
    }
    next = 0;
    return xf_mul(f, beam_lm_xf(lm.unk_m, lm.unk_e));
}
__device__ __forceinline__ xf beam_lm_final(const nntk_shim_lm &lm, int s) {
    const int4 f = ((const int4 *)lm.d_factors)[s];
    return beam_lm_xf(f.z, f.w);
}

// ---- streaming: the beam a row carries from one push to the next (INTEGRATION.md "CTC prefix beam search", Streaming).  Plain global
// memory, a slot per row: written once per push with ordinary stores by the row's workgroup, read back by the same row's workgroup of
// the next launch on the stream.  ctl = [4][B] ints the host uploads per push: frames in this push | frames the row had seen before it
// (0: the row starts from the empty prefix and its slot is not read) | which half of the label strings is current | unused.
struct BeamCarry {
    float4 *mass;                         // [B][W] p_b, p_nb (mantissa, exponent each)
    u64 *h, *ph;                          // [B][W] prefix hash, parent prefix hash
    int2 *tail;                           // [B][W] last class, length
    int *nb;                              // [B] entries; 0: the beam has died
    int *lm;                              // [B][W] LM state (LM instantiations; else NULL)
    const int *seen;                      // ctl + B
};
// buffer of a streaming handle, in 4-byte words; every part starts on a 16-byte boundary
struct BeamStreamLayout { size_t ctl, nb, mass, h, ph, tail, str, hist, cut, lm, fstr, lstr, total; };
static BeamStreamLayout beam_stream_layout(int B, int T, int W, int ncut, int L, bool lm = false, bool detail = false) {
    BeamStreamLayout l;
    const size_t b = B > 0 ? (size_t)B : 0, t = T > 0 ? (size_t)T : 0, w = W > 0 ? (size_t)W : 0, n = ncut > 0 ? (size_t)ncut : 0;
    const size_t ml = L > 0 ? (size_t)L : 0;
    auto up = [](size_t x) { return (x + 3) & ~(size_t)3; };
    l.ctl = 0;
    l.nb = up(4 * b);
    l.mass = l.nb + up(b);
    l.h = l.mass + 4 * b * w;
    l.ph = l.h + up(2 * b * w);
    l.tail = l.ph + up(2 * b * w);
    l.str = l.tail + up(2 * b * w);
    l.hist = l.str + up(2 * b * w * ml);
    l.cut = l.hist + up(2 * b * t * w);
    l.lm = l.cut + up(2 * b * t * n);                                          // the carried LM states, behind everything else
    l.fstr = l.lm + (lm ? up(b * w) : 0);                                      // detail: both halves of the frame strings, then of the
    l.lstr = l.fstr + (detail ? up(2 * b * w * ml) : 0);                       // log-probability strings: 16 * L bytes per row and entry
    l.total = l.lstr + (detail ? up(2 * b * w * ml) : 0) + 4;
    return l;
}

// ---- class cut: the n non-blank classes of highest probability (ties: the lower class), ascending class order ----
__global__ __launch_bounds__(CTC_THREADS) void ctc_beam_cut_kernel(const float *__restrict__ probs, int T, int C, int blank, int n,
                                                                   const int *__restrict__ lens, float2 *__restrict__ pairs, long frames) {
    const int lane = threadIdx.x & 63;
    const u64 lt = (1ull << lane) - 1;
    for (long f = blockIdx.x * 4L + (threadIdx.x >> 6); f < frames; f += gridDim.x * 4L) {
        const int b = (int)(f / T), t = (int)(f % T);
        if (t >= lens[b]) continue;
        const float *row = probs + f * C;
        float2 *out = pairs + f * n;
        // the largest lo with count(bits >= lo) >= n: probabilities are non-negative, their bits order like their values
        unsigned lo = 0u, hi = 0x7f800001u;
        while (hi - lo > 1u) {
            const unsigned mid = lo + (hi - lo) / 2u;
            int cnt = 0;
            for (int k0 = 0; k0 < C; k0 += 64) {
                const int k = k0 + lane;
                const bool in = k < C && k != blank && __float_as_uint(row[k]) >= mid;
                cnt += __popcll(__ballot(in));
            }
            if (cnt >= n) lo = mid; else hi = mid;
        }
        int above = 0;
        for (int k0 = 0; k0 < C; k0 += 64) {
            const int k = k0 + lane;
            above += __popcll(__ballot(k < C && k != blank && __float_as_uint(row[k]) > lo));
        }
        int need = n - above, pos = 0;                                       // classes equal to the threshold still to take, lowest first
        for (int k0 = 0; k0 < C; k0 += 64) {
            const int k = k0 + lane;
            const bool in = k < C && k != blank;
            const float v = in ? row[k] : 0.0f;
            const unsigned vb = __float_as_uint(v);
            const u64 eqm = __ballot(in && vb == lo);
            const bool take = in && (vb > lo || (vb == lo && __popcll(eqm & lt) < need));
            const u64 tm = __ballot(take);
            if (take) {
                const int p = pos + __popcll(tm & lt);
                if (p < n) out[p] = make_float2(__int_as_float(k), v);
            }
            pos += __popcll(tm);
            need -= min(need, (int)__popcll(eqm));
        }
    }
}

// ---- the beam: one workgroup per row ----
// STREAM: T is the capacity of a push and lens its frame counts; the beam starts from the row's slot of `cs` (or the empty prefix, for
// a row that has seen no frame) and ends there; the masses of the frames in between are not kept.
// LM: every extension is weighted by the language model `lm`; !STREAM: the final ranking goes to forder / fmass ([B][W] each: the entry
// of the last beam that hypothesis k is, and its finalised total as (m, e, 0, zero's exponent)) and its size to nfin.
// DETAIL (label timestamps; "Label timestamps" below): a merge whose extension outweighs the stay it is summed with writes its record's
// class as -2 instead of -1.  Nothing else changes: no mass, key, cut, hash or LM state depends on it.
template <bool CUT, bool STAGE, bool STREAM, bool LM, bool DETAIL>
__global__ __launch_bounds__(CTC_THREADS) void ctc_beam_kernel(const float *__restrict__ probs, int T, int C, int blank, int W, int n,
                                                               unsigned magic, const int *__restrict__ lens, int *__restrict__ nfin,
                                                               int2 *__restrict__ hist, float4 *__restrict__ mass,
                                                               const float2 *__restrict__ pairs, BeamCarry cs, nntk_shim_lm lm,
                                                               int *__restrict__ forder, float4 *__restrict__ fmass) {
    extern __shared__ __align__(16) unsigned char beam_smem[];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const u64 lt = (1ull << lane) - 1;
    const int Tb = lens[b], n1 = n + 1;
    const BeamLds L = beam_lds(W, n, C, CUT, STAGE, LM);
    float2 *cell = (float2 *)(beam_smem + L.cells);
    float *srow = (float *)(beam_smem + L.stage);                              // !CUT: [2][C] probabilities
    float2 *spair = (float2 *)(beam_smem + L.stage);                           // CUT: [2][n] (class, probability)
    unsigned char *st = beam_smem + L.state;
    float2 *s_pb = (float2 *)st, *s_pnb = s_pb + 2 * W;
    u64 *s_h = (u64 *)(s_pnb + 2 * W), *s_ph = s_h + 2 * W;
    int *s_last = (int *)(s_ph + 2 * W), *s_len = s_last + 2 * W, *s_home = s_len + 2 * W;
    int *s_lm = s_home + 2 * W;                                                // LM only
    float2 *f_spb = (float2 *)(beam_smem + L.frame), *f_spnb = f_spb + W, *f_sum = f_spnb + W;
    int2 *f_rec = (int2 *)(f_sum + W);
    int *sel = (int *)(beam_smem + L.sel);
    u64 *lkey = (u64 *)(beam_smem + L.lkey);
    int *lidx = (int *)(beam_smem + L.lidx);
    int4 *cnt1 = (int4 *)(beam_smem + L.cnt), *cnt2 = cnt1 + BEAM_MAX_CELLS / CTC_THREADS;
    u64 *r_max = (u64 *)(beam_smem + L.red), *r_min = r_max + 4;
    int *r_nz = (int *)(r_min + 4), *r_bis = r_nz + 4;                         // r_bis [2][4]

    const float *prow = probs + (long)b * T * C;
    const float2 *crow = CUT ? pairs + (long)b * T * n : nullptr;
    int2 *hrow = hist + (long)b * T * W;
    float4 *mrow = mass + (long)b * T * W;
    const int M = CUT ? n : C;                                                 // staged elements per frame
    const bool in_regs = STAGE && M <= BEAM_PF * CTC_THREADS;

    auto div_n1 = [&](int idx) { return n1 == 1 ? idx : (int)__umulhi((unsigned)idx, magic); };

    // the row's beam: the carried one, or the empty prefix
    const bool carried = STREAM && cs.seen[b] > 0;
    int nb = 1, cur = 0;
    if (STREAM) {
        if (Tb == 0) return;                                                   // uniform: nothing to do, the slot stays as it is
        if (carried) nb = min(max(cs.nb[b], 0), W);
        if (nb == 0) return;                                                   // a dead beam stays dead
    }
    if (carried) {
        if (tid < nb) {
            const long q = (long)b * W + tid;
            const float4 m = cs.mass[q];
            const int2 tl = cs.tail[q];
            s_pb[tid] = make_float2(m.x, m.y);
            s_pnb[tid] = make_float2(m.z, m.w);
            s_h[tid] = cs.h[q];
            s_ph[tid] = cs.ph[q];
            s_last[tid] = tl.x;
            s_len[tid] = tl.y;
            s_home[tid] = -1;
            if (LM) s_lm[tid] = cs.lm[q];
        }
    } else if (tid == 0) {
        s_pb[0] = xf_pack(xf_one());
        s_pnb[0] = xf_pack(xf_zero());
        s_h[0] = 0x243F6A8885A308D3ull;
        s_ph[0] = 0ull;
        s_last[0] = -1;
        s_len[0] = 0;
        s_home[0] = -1;
        if (LM) s_lm[0] = lm.start_state;
    }
    if (STAGE && Tb > 0) {
        if (CUT) for (int k = tid; k < M; k += CTC_THREADS) spair[k] = crow[k];
        else for (int k = tid; k < M; k += CTC_THREADS) srow[k] = prow[k];
    }
    __syncthreads();                                                           // the slot's words are in LDS: the stores needed them

    for (int t = 0; t < Tb; ++t) {
        const int o = cur * W, on = (cur ^ 1) * W;                             // this frame's beam, the next one's
        const float *grow = prow + (long)t * C;
        const float2 *gpair = CUT ? crow + (long)t * n : nullptr;
        const float *sr = srow + cur * M;
        const float2 *sp = spair + cur * M;
        // the next frame's staged words: in flight across every barrier of this frame
        float pre[BEAM_PF];
        float2 pre2[BEAM_PF];
        if (in_regs && t + 1 < Tb) {
#pragma unroll
            for (int q = 0; q < BEAM_PF; ++q) {
                const int k = tid + CTC_THREADS * q;
                if (CUT) pre2[q] = k < M ? gpair[n + k] : make_float2(0.0f, 0.0f);
                else pre[q] = k < M ? grow[C + k] : 0.0f;
            }
        }
        auto prob_of = [&](int c) { return (!CUT && STAGE) ? sr[c] : grow[c]; };
        auto cell_class = [&](int k, int &c, float &p) {
            if (CUT) {
                const float2 v = STAGE ? sp[k] : gpair[k];
                c = __float_as_int(v.x);
                p = v.y;
            } else {
                c = k + (k >= blank ? 1 : 0);
                p = prob_of(c);
            }
        };

        // ---- stays; which entry's prefix is another entry's prefix plus one expanded class ----
        if (tid < nb) {
            const xf pb = xf_unpack(s_pb[o + tid]), pnb = xf_unpack(s_pnb[o + tid]);
            const xf s = xf_add2(pb, pnb);
            f_sum[tid] = xf_pack(s);
            f_spb[tid] = xf_pack(xf_times_prob(s, prob_of(blank)));
            f_spnb[tid] = xf_pack(s_len[o + tid] > 0 ? xf_times_prob(pnb, prob_of(s_last[o + tid])) : xf_zero());
        }
        {
            int sh = 0;
            while ((1 << sh) < nb) ++sh;
            const int pairs_n = nb << sh;
            for (int p = tid; p < pairs_n; p += CTC_THREADS) {
                const int j = p & ((1 << sh) - 1), i = p >> sh;                // consecutive lanes: consecutive j
                if (j >= nb) continue;
                if (s_len[o + j] != s_len[o + i] + 1 || s_ph[o + j] != s_h[o + i]) continue;
                const int c = s_last[o + j];
                int k = -1;
                if (CUT) {
                    int a = 0, z = n - 1;
                    while (a <= z) {
                        const int mid = (a + z) >> 1;
                        const int cm = __float_as_int(STAGE ? sp[mid].x : gpair[mid].x);
                        if (cm == c) { k = mid; break; }
                        if (cm < c) a = mid + 1; else z = mid - 1;
                    }
                } else {
                    k = c - (c > blank ? 1 : 0);
                }
                if (k >= 0) s_home[o + j] = i * n1 + 1 + k;
            }
        }
        CTC_LDS_BARRIER();

        // ---- the cell matrix: cell i * (n + 1) is entry i's stay, cell i * (n + 1) + 1 + k its extension by the k-th expanded class ----
        const int N = nb * n1;
        for (int idx = tid; idx < N; idx += CTC_THREADS) {
            const int i = div_n1(idx), kk = idx - i * n1;
            xf v;
            if (kk == 0) {
                v = s_home[o + i] < 0 ? xf_add2(xf_unpack(f_spb[i]), xf_unpack(f_spnb[i])) : xf_zero();
            } else {
                int c;
                float p;
                cell_class(kk - 1, c, p);
                v = xf_times_prob(xf_unpack(c == s_last[o + i] ? s_pb[o + i] : f_sum[i]), p);
                if (LM) {
                    int nx;
                    v = xf_mul(v, beam_lm_walk(lm, s_lm[o + i], c, nx));
                }
            }
            cell[idx] = xf_pack(v);
        }
        CTC_LDS_BARRIER();
        // ---- merges: p_nb' = stay + extension, in that order; the cell holds the candidate's total ----
        bool moved = false;                                                    // DETAIL: this lane's merge takes the frame (same lane below)
        if (tid < nb && s_home[o + tid] >= 0) {
            const int hc = s_home[o + tid];
            if (DETAIL) moved = beam_key(cell[hc]) > beam_key(f_spnb[tid]);       // extension > stay, strictly, as (exponent, mantissa)
            const xf mnb = xf_add2(xf_unpack(f_spnb[tid]), xf_unpack(cell[hc]));
            f_spnb[tid] = xf_pack(mnb);
            cell[hc] = xf_pack(xf_add2(xf_unpack(f_spb[tid]), mnb));
        }
        CTC_LDS_BARRIER();

        // ---- selection ----
        const int R = (N + CTC_THREADS - 1) / CTC_THREADS;
        {
            u64 mx = 0ull, mn = ~0ull;
            int nz = 0;
            for (int r = 0; r < R; ++r) {
                const int idx = r * CTC_THREADS + tid;
                const u64 k = idx < N ? beam_key(cell[idx]) : 0ull;
                if (k) { mx = k > mx ? k : mx; mn = k < mn ? k : mn; ++nz; }
            }
            for (int off = 32; off > 0; off >>= 1) {
                const u64 omx = __shfl_xor(mx, off), omn = __shfl_xor(mn, off);
                mx = omx > mx ? omx : mx;
                mn = omn < mn ? omn : mn;
                nz += __shfl_xor(nz, off);
            }
            if (lane == 0) { r_max[wave] = mx; r_min[wave] = mn; r_nz[wave] = nz; }
        }
        CTC_LDS_BARRIER();
        u64 lo = ~0ull, hi = 0ull;
        int clo = 0;
        for (int w = 0; w < 4; ++w) {
            lo = r_min[w] < lo ? r_min[w] : lo;
            hi = r_max[w] > hi ? r_max[w] : hi;
            clo += r_nz[w];
        }
        const int Wt = min(W, clo);                                           // candidates with total exactly 0 are dropped
        if (Wt == 0) { nb = 0; break; }                                       // uniform: every lane read the same words
        hi += 1ull;
        // count(key >= lo) = clo >= Wt always; count(key >= hi) < Wt always
        for (int it = 0; clo > BEAM_LIST && hi - lo > 1ull; ++it) {
            const u64 mid = lo + (hi - lo) / 2ull;
            int c = 0;
            for (int r = 0; r < R; ++r) {
                const int idx = r * CTC_THREADS + tid;
                c += __popcll(__ballot(idx < N && beam_key(cell[idx]) >= mid));
            }
            int *slot = r_bis + (it & 1) * 4;
            if (lane == 0) slot[wave] = c;
            CTC_LDS_BARRIER();
            c = slot[0] + slot[1] + slot[2] + slot[3];
            if (c >= Wt) { lo = mid; clo = c; } else { hi = mid; }
        }
        // survivors in cell order: every key above lo, then the first of those equal to lo, BEAM_LIST in all
        for (int r = 0; r < R; ++r) {
            const int idx = r * CTC_THREADS + tid;
            const u64 k = idx < N ? beam_key(cell[idx]) : 0ull;
            const int c1 = __popcll(__ballot(k > lo)), c2 = __popcll(__ballot(k == lo));
            if (lane == 0) { ((int *)(cnt1 + r))[wave] = c1; ((int *)(cnt2 + r))[wave] = c2; }
        }
        CTC_LDS_BARRIER();
        int tot1 = 0, tot2 = 0;
        for (int r = 0; r < R; ++r) {
            const int4 a = cnt1[r], e = cnt2[r];
            tot1 += a.x + a.y + a.z + a.w;
            tot2 += e.x + e.y + e.z + e.w;
        }
        {
            int run1 = 0, run2 = tot1;
            for (int r = 0; r < R; ++r) {
                const int idx = r * CTC_THREADS + tid;
                const u64 k = idx < N ? beam_key(cell[idx]) : 0ull;
                const bool g = k > lo, e = k == lo;
                const u64 m1 = __ballot(g), m2 = __ballot(e);
                const int4 a = cnt1[r], q = cnt2[r];
                const int p1 = run1 + (wave > 0 ? a.x : 0) + (wave > 1 ? a.y : 0) + (wave > 2 ? a.z : 0) + __popcll(m1 & lt);
                const int p2 = run2 + (wave > 0 ? q.x : 0) + (wave > 1 ? q.y : 0) + (wave > 2 ? q.z : 0) + __popcll(m2 & lt);
                if (g && p1 < BEAM_LIST) { lkey[p1] = k; lidx[p1] = idx; }
                if (e && p2 < BEAM_LIST) { lkey[p2] = k; lidx[p2] = idx; }
                run1 += a.x + a.y + a.z + a.w;
                run2 += q.x + q.y + q.z + q.w;
            }
        }
        const int nl = min(BEAM_LIST, tot1 + tot2);
        CTC_LDS_BARRIER();
        if (tid < nl) {
            const u64 k = lkey[tid];
            const int idx = lidx[tid];
            int rank = 0;
            for (int u = 0; u < nl; ++u) {
                const u64 ku = lkey[u];
                rank += (ku > k || (ku == k && lidx[u] < idx)) ? 1 : 0;
            }
            if (rank < Wt) sel[rank] = idx;
        }
        CTC_LDS_BARRIER();

        // ---- the new beam: rank r as a plain stay or extension first; a merged cell is taken over by the entry whose stay it holds ----
        if (tid < Wt) {
            const int idx = sel[tid];
            const int i = div_n1(idx), kk = idx - i * n1;
            if (kk == 0) {
                s_pb[on + tid] = f_spb[i];
                s_pnb[on + tid] = f_spnb[i];
                s_h[on + tid] = s_h[o + i];
                s_ph[on + tid] = s_ph[o + i];
                s_last[on + tid] = s_last[o + i];
                s_len[on + tid] = s_len[o + i];
                if (LM) s_lm[on + tid] = s_lm[o + i];
                f_rec[tid] = make_int2(i | (s_len[o + i] << 8), -1);
            } else {
                int c;
                float p;
                cell_class(kk - 1, c, p);
                const u64 h = s_h[o + i];
                s_pb[on + tid] = xf_pack(xf_zero());
                s_pnb[on + tid] = cell[idx];
                s_h[on + tid] = beam_hash(h, c);
                s_ph[on + tid] = h;
                s_last[on + tid] = c;
                s_len[on + tid] = s_len[o + i] + 1;
                if (LM) {
                    int nx;
                    beam_lm_walk(lm, s_lm[o + i], c, nx);
                    s_lm[on + tid] = nx;
                }
                f_rec[tid] = make_int2(i | ((s_len[o + i] + 1) << 8), c);
                cell[idx].x = __uint_as_float(0x80000000u | (unsigned)tid);    // no mantissa has the sign bit: "selected, rank tid"
            }
            s_home[on + tid] = -1;
        }
        CTC_LDS_BARRIER();
        if (tid < nb && s_home[o + tid] >= 0) {
            const unsigned m = __float_as_uint(cell[s_home[o + tid]].x);
            if (m & 0x80000000u) {
                const int r = (int)(m & 0xffffu);
                s_pb[on + r] = f_spb[tid];
                s_pnb[on + r] = f_spnb[tid];
                s_h[on + r] = s_h[o + tid];
                s_ph[on + r] = s_ph[o + tid];
                s_last[on + r] = s_last[o + tid];
                s_len[on + r] = s_len[o + tid];
                if (LM) s_lm[on + r] = s_lm[o + tid];
                f_rec[r] = make_int2(tid | (s_len[o + tid] << 8), DETAIL && moved ? -2 : -1);
            }
        }
        if (STAGE && t + 1 < Tb) {
            if (in_regs) {
#pragma unroll
                for (int q = 0; q < BEAM_PF; ++q) {
                    const int k = tid + CTC_THREADS * q;
                    if (k < M) {
                        if (CUT) spair[(cur ^ 1) * M + k] = pre2[q];
                        else srow[(cur ^ 1) * M + k] = pre[q];
                    }
                }
            } else if (CUT) {
                for (int k = tid; k < M; k += CTC_THREADS) spair[(cur ^ 1) * M + k] = gpair[n + k];
            } else {
                for (int k = tid; k < M; k += CTC_THREADS) srow[(cur ^ 1) * M + k] = grow[C + k];
            }
        }
        CTC_LDS_BARRIER();
        if (tid < Wt) {
            const float2 pb = s_pb[on + tid], pnb = s_pnb[on + tid];
            hrow[(long)t * W + tid] = f_rec[tid];
            if (!STREAM) mrow[(long)t * W + tid] = make_float4(pb.x, pb.y, pnb.x, pnb.y);
        }
        nb = Wt;
        cur ^= 1;
    }
    if (STREAM) {
        // the beam this push leaves (written in LDS before the loop's last barrier)
        if (tid < nb) {
            const int o = cur * W + tid;
            const long q = (long)b * W + tid;
            const float2 pb = s_pb[o], pnb = s_pnb[o];
            cs.mass[q] = make_float4(pb.x, pb.y, pnb.x, pnb.y);
            cs.h[q] = s_h[o];
            cs.ph[q] = s_ph[o];
            cs.tail[q] = make_int2(s_last[o], s_len[o]);
            if (LM) cs.lm[q] = s_lm[o];
        }
        if (tid == 0) cs.nb[b] = nb;
    } else if (LM) {
        // the end of the row: every total times the end-of-sentence factor of its state, exact zeros dropped, the rest in descending
        // order, ties to the lower rank in the last beam (the beam's words were written before the loop's last barrier)
        __syncthreads();
        xf v = xf_zero();
        if (tid < nb) {
            const int o = cur * W + tid;
            v = xf_mul(xf_add2(xf_unpack(s_pb[o]), xf_unpack(s_pnb[o])), beam_lm_final(lm, s_lm[o]));
            lkey[tid] = beam_key(xf_pack(v));
        }
        __syncthreads();
        const BeamFinalRank fin = beam_final_rank(lkey, nb, tid);
        if (fin.rank >= 0) {
            forder[(long)b * W + fin.rank] = tid;
            fmass[(long)b * W + fin.rank] = make_float4(v.m, __int_as_float(v.e), 0.0f, __int_as_float(CTC_EZERO));
        }
        if (tid == 0) nfin[b] = fin.alive;
    } else if (tid == 0) {
        nfin[b] = nb;
    }
}

// ---- what the backtrack and the stream's commit share ----

// The record walk: the row's Tb frames of records are staged in LDS in blocks of BEAM_BT_RECORDS / W frames, the last block first, and
// an `active` lane walks its entry's line of descent from `rank` in the last frame to the first frame.  Every record that made a label
// (class >= 0) goes to visit(t, f, record): t its frame, f the frame the label reports -- under DETAIL the latest -2 record met since
// the previous label (`ft`: a register of the lane, so it crosses the blocks' edges), else t.  Every lane of the workgroup must call:
// the two barriers of a block are the workgroup's.  Returns the rank the line has before the first frame, and a pending `ft`.
struct BeamWalkEnd { int rank, ft; };
template <bool DETAIL, class Visit>
__device__ __forceinline__ BeamWalkEnd beam_walk_records(int2 *rec, const int2 *__restrict__ hrow, int Tb, int W, int tid, bool active,
                                                         int rank, Visit visit) {
    int ft = -1;
    const int TC = max(1, BEAM_BT_RECORDS / W);
    for (int t1 = Tb; t1 > 0; t1 -= TC) {
        const int t0 = max(0, t1 - TC);
        const long base = (long)t0 * W;
        const int cnt = (t1 - t0) * W;
        __syncthreads();
        for (int q = tid; q < cnt; q += CTC_THREADS) rec[q] = hrow[base + q];
        __syncthreads();
        if (active) {
            for (int t = t1 - 1; t >= t0; --t) {
                const int2 r = rec[(t - t0) * W + rank];
                if (DETAIL && r.y == -2 && ft < 0) ft = t;                     // the latest merge that took this position's frame
                if (r.y >= 0) {
                    visit(t, ft >= 0 ? ft : t, r);
                    ft = -1;
                }
                rank = r.x & 0xff;
            }
        }
    }
    return {rank, ft};
}

// behind a hypothesis: label -1, frame -1, log-probability 0.0 (fr, lp: null where that output is not asked for)
template <bool DETAIL>
__device__ __forceinline__ void beam_pad(long q, int *lab, int *fr, float *lp) {
    lab[q] = -1;
    if (DETAIL && fr) fr[q] = -1;
    if (DETAIL && lp) lp[q] = 0.0f;
}

// ---- backtrack: hypothesis k of a row is entry k of its last frame; FIN (the LM calls): entry forder[k], with the total fmass[k] ----
// DETAIL: the walking lane also writes frames / logps ([B][nbest][T] each, either may be null; "Label timestamps" above).
template <bool FIN, bool DETAIL>
__global__ __launch_bounds__(CTC_THREADS) void ctc_beam_backtrack_kernel(int T, int W, int nbest, const int *__restrict__ lens,
                                                                         const int *__restrict__ nfin, const int2 *__restrict__ hist,
                                                                         const float4 *__restrict__ mass, const int *__restrict__ forder,
                                                                         const float4 *__restrict__ fmass, int *__restrict__ labels,
                                                                         int *__restrict__ out_len, float *__restrict__ scores,
                                                                         const float *__restrict__ probs, int C, int *__restrict__ frames,
                                                                         float *__restrict__ logps) {
    extern __shared__ __align__(16) unsigned char beam_smem[];
    __shared__ int s_hlen[BEAM_MAX_W];
    int2 *rec = (int2 *)beam_smem;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int Tb = lens[b];
    const int nh = (!FIN && Tb == 0) ? 1 : min(nbest, nfin[b]);               // hypotheses this row has
    const int2 *hrow = hist + (long)b * T * W;
    const float4 *mrow = mass + (long)b * T * W;
    int *lab = labels + (long)b * nbest * T;
    const float *prow = DETAIL ? probs + (long)b * T * C : nullptr;
    int *fr = DETAIL && frames ? frames + (long)b * nbest * T : nullptr;
    float *lp = DETAIL && logps ? logps + (long)b * nbest * T : nullptr;
    int rank = tid, len = -1, pos = -1;
    if (tid < nbest) {
        float score = -INFINITY;
        if (tid < nh) {
            if (FIN) rank = forder[(long)b * W + tid];
            if (Tb == 0) {
                len = 0;
                score = FIN ? beam_score(fmass[(long)b * W + tid]) : 0.0f;
            } else {
                len = hrow[(long)(Tb - 1) * W + rank].x >> 8;
                score = FIN ? beam_score(fmass[(long)b * W + tid]) : beam_score(mrow[(long)(Tb - 1) * W + tid]);
            }
        }
        pos = len - 1;
        s_hlen[tid] = len;
        out_len[(long)b * nbest + tid] = len;
        scores[(long)b * nbest + tid] = score;
    }
    // the labels in forward order: the walk meets the last one first
    beam_walk_records<DETAIL>(rec, hrow, Tb, W, tid, tid < nh, rank, [&](int, int f, int2 r) {
        if (pos < 0) return;
        if (DETAIL) {
            if (fr) fr[(long)tid * T + pos] = f;
            if (lp) lp[(long)tid * T + pos] = beam_logp(prow[(long)f * C + r.y]);
        }
        lab[(long)tid * T + pos--] = r.y;
    });
    __syncthreads();
    const long cells = (long)nbest * T;
    for (long q = tid; q < cells; q += CTC_THREADS)
        if ((int)(q % T) >= s_hlen[(int)(q / T)]) beam_pad<DETAIL>(q, lab, fr, lp);
}

// ---- streaming commit: a workgroup per row, a lane per surviving entry.  The lane walks the push's records from its last frame to its
// first, which gives the labels the entry gained inside the push (a record carries the length after it, so each label knows its
// place) and the rank it descends from at the push's start; the entry's string = that ancestor's stored string + those labels goes
// to the other half of the double-buffered store, cut at L labels, and the first nbest entries go to the outputs as well.  A row
// without frames in this push only rewrites its outputs from what it holds.  FIN (a stream with a language model): what is REPORTED is
// the beam after the end-of-sentence factors -- entry tid goes to output slot `slot` (its rank among the finalised totals, or none) --
// while the carried beam and its strings stay in entry order, unfinalised.
// DETAIL: every entry also carries the frame and the log-probability of each of its labels (fstrs / lstrs, laid out and double-buffered
// like strs): earlier pushes' probabilities are gone, so the values travel.  A label gained in this push takes `seen` + its frame and
// this push's probability; a -2 record that no extension of this push answers moves the LAST element the ancestor held (s_mvt: the
// push's frame, or -1), frame and log-probability, if that position is stored at all.  oframes / ologps ([B][nbest][L], either may be
// null) report like labels.
template <bool FIN, bool DETAIL>
__global__ __launch_bounds__(CTC_THREADS) void ctc_beam_commit_kernel(int B, int T, int W, int nbest, int L, const int *__restrict__ ctl,
                                                                      BeamCarry cs, const int2 *__restrict__ hist, int *__restrict__ strs,
                                                                      int *__restrict__ labels, int *__restrict__ out_len,
                                                                      float *__restrict__ scores, nntk_shim_lm lm,
                                                                      const float *__restrict__ probs, int C, int *__restrict__ fstrs,
                                                                      float *__restrict__ lstrs, int *__restrict__ oframes,
                                                                      float *__restrict__ ologps) {
    extern __shared__ __align__(16) unsigned char beam_smem[];
    __shared__ int s_hlen[BEAM_MAX_W], s_anc[BEAM_MAX_W], s_alen[BEAM_MAX_W];
    __shared__ int s_mvt[DETAIL ? BEAM_MAX_W : 1];
    __shared__ int s_slot[FIN ? BEAM_MAX_W : 1], s_ord[FIN ? BEAM_MAX_W : 1];
    __shared__ u64 s_key[FIN ? BEAM_MAX_W : 1];
    int2 *rec = (int2 *)beam_smem;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int Tb = ctl[b], seen = ctl[B + b], par = ctl[2 * B + b] & 1;
    const bool fresh = seen == 0 && Tb == 0;                                   // no frame since the reset: the empty prefix alone
    const int nb = fresh ? 1 : min(max(cs.nb[b], 0), W);
    int nh = min(nbest, nb);
    const int *src = strs + ((long)par * B + b) * W * L;
    int *dst = strs + ((long)(par ^ 1) * B + b) * W * L;
    const int2 *hrow = hist + (long)b * T * W;
    int *lab = labels + (long)b * nbest * L;
    const int *fsrc = DETAIL ? fstrs + ((long)par * B + b) * W * L : nullptr;
    int *fdst = DETAIL ? fstrs + ((long)(par ^ 1) * B + b) * W * L : nullptr;
    const float *lsrc = DETAIL ? lstrs + ((long)par * B + b) * W * L : nullptr;
    float *ldst = DETAIL ? lstrs + ((long)(par ^ 1) * B + b) * W * L : nullptr;
    const float *prow = DETAIL ? probs + (long)b * T * C : nullptr;
    int *ofr = DETAIL && oframes ? oframes + (long)b * nbest * L : nullptr;
    float *olp = DETAIL && ologps ? ologps + (long)b * nbest * L : nullptr;
    int len = -1;
    if (tid < nb) len = fresh ? 0 : cs.tail[(long)b * W + tid].y;
    int slot = tid < nh ? tid : -1;                                            // the output slot that reports entry tid
    if (FIN) {
        xf v = xf_zero();
        if (tid < nb) {
            xf tot = xf_one();
            int st = lm.start_state;
            if (!fresh) {
                const float4 m = cs.mass[(long)b * W + tid];
                tot = xf_add2(xf_unpack(make_float2(m.x, m.y)), xf_unpack(make_float2(m.z, m.w)));
                st = min(max(cs.lm[(long)b * W + tid], 0), lm.n_states - 1);
            }
            v = xf_mul(tot, beam_lm_final(lm, st));
            s_key[tid] = beam_key(xf_pack(v));
        }
        __syncthreads();
        const BeamFinalRank fin = beam_final_rank(s_key, nb, tid);
        nh = min(nbest, fin.alive);
        slot = fin.rank < nbest ? fin.rank : -1;
        if (tid < W) s_slot[tid] = slot;
        if (slot >= 0) {
            s_ord[slot] = tid;
            out_len[(long)b * nbest + slot] = len;
            scores[(long)b * nbest + slot] = beam_score(make_float4(v.m, __int_as_float(v.e), 0.0f, __int_as_float(CTC_EZERO)));
        }
        if (tid < nbest && tid >= nh) {
            out_len[(long)b * nbest + tid] = -1;
            scores[(long)b * nbest + tid] = -INFINITY;
        }
    } else if (tid < nbest) {
        float score = -INFINITY;
        if (tid < nh) score = fresh ? 0.0f : beam_score(cs.mass[(long)b * W + tid]);
        out_len[(long)b * nbest + tid] = tid < nh ? len : -1;
        scores[(long)b * nbest + tid] = score;
    }
    if (tid < W) s_hlen[tid] = len;
    // who reports whom.  FIN: by the ranking above; else entry k is hypothesis k
    auto slot_of = [&](int k) { return FIN ? s_slot[k] : (k < nbest ? k : -1); };     // the output slot of entry k (< nb), or -1
    auto entry_of = [&](int k) { return FIN ? s_ord[k] : k; };                       // the entry that output slot k (< nh) reports
    // element p of entry k: stored, and told if an output slot s >= 0 reports the entry
    auto put = [&](int k, int s, int p, int v, int f, float lg) {
        const long at = (long)k * L + p, to = FIN ? (long)s * L + p : at;             // !FIN: a reported entry's slot is its own index
        dst[at] = v;
        if (s >= 0) lab[to] = v;
        if (DETAIL) {
            fdst[at] = f;
            ldst[at] = lg;
            if (s >= 0 && ofr) ofr[to] = f;
            if (s >= 0 && olp) olp[to] = lg;
        }
    };
    const long cells_out = (long)nbest * L;
    if (Tb == 0 || nb == 0) {
        __syncthreads();
        for (long q = tid; q < cells_out; q += CTC_THREADS) {
            const int k = (int)(q / L), p = (int)(q % L);
            const int e = k < nh ? entry_of(k) : 0;
            if (k < nh && p < min(s_hlen[e], L)) {
                lab[q] = src[(long)e * L + p];
                if (DETAIL && ofr) ofr[q] = fsrc[(long)e * L + p];
                if (DETAIL && olp) olp[q] = lsrc[(long)e * L + p];
            } else {
                beam_pad<DETAIL>(q, lab, ofr, olp);
            }
        }
        return;
    }
    int gained = 0;
    const BeamWalkEnd end = beam_walk_records<DETAIL>(rec, hrow, Tb, W, tid, tid < nb, tid, [&](int, int f, int2 r) {
        const int pos = (r.x >> 8) - 1;
        if (pos < L) put(tid, slot, pos, r.y, seen + f, DETAIL ? beam_logp(prow[(long)f * C + r.y]) : 0.0f);
        ++gained;
    });
    if (tid < nb) {
        s_anc[tid] = end.rank;
        s_alen[tid] = len - gained;
        if (DETAIL) s_mvt[tid] = end.ft;
    }
    __syncthreads();
    // the ancestors' strings, and the padding behind every reported hypothesis; the places in between were written above.  A k is looked
    // at twice: as an entry, and as an output slot.  The places are disjoint whoever reports whom: a copy ends below s_alen <= s_hlen of
    // the entry, the padding of the slot that reports it starts at s_hlen; and `k >= nh ||` keeps entry_of from an unreported slot
    const long cells = (long)max(nb, nbest) * L;
    for (long q = tid; q < cells; q += CTC_THREADS) {
        const int k = (int)(q / L), p = (int)(q % L);
        if (k < nb && p < min(s_alen[k], L)) {
            const int a = s_anc[k], v = src[(long)a * L + p];
            int f = 0;
            float lg = 0.0f;
            if (DETAIL) {
                // the ancestor's element, moved when this push took the ancestor's last frame
                f = fsrc[(long)a * L + p];
                lg = lsrc[(long)a * L + p];
                if (p == s_alen[k] - 1 && s_mvt[k] >= 0) {
                    f = seen + s_mvt[k];
                    lg = beam_logp(prow[(long)s_mvt[k] * C + min(max(v, 0), C - 1)]);
                }
            }
            put(k, slot_of(k), p, v, f, lg);
        }
        if (k < nbest && (k >= nh || p >= min(s_hlen[entry_of(k)], L))) beam_pad<DETAIL>(q, lab, ofr, olp);
    }
}

// ---- host section.  lm NULL: the acoustic-only kernels, exactly ----

// runtime bools -> template arguments: beam_dispatch(f, b0, b1, ...) calls the generic lambda f with one std::bool_constant per bool
template <class F>
static int beam_dispatch(F f) { return f(); }
template <class F, class... Bools>
static int beam_dispatch(F f, bool b, Bools... rest) {
    return b ? beam_dispatch([&](auto... c) { return f(std::true_type(), c...); }, rest...)
             : beam_dispatch([&](auto... c) { return f(std::false_type(), c...); }, rest...);
}

// The class cut (when one applies) and the beam kernel.  One-shot call (STREAM false): lens = the rows' lengths, nfin / mass / forder /
// fmass the workspace's, an empty carry.  Push (STREAM true): lens = the control block, cs = the handle's beam, those four null.
// detail: the instantiations that mark the merges which take a label's frame.
template <bool STREAM>
static int beam_launch(const float *d_probs, int B, int T, int C, int blank, int W, int ncut, const nntk_shim_lm *lm, bool detail,
                       const int *d_lens, int *d_nfin, int2 *d_hist, float4 *d_mass, float2 *d_pairs, const BeamCarry &cs, int *d_forder, float4 *d_fmass) {
    const int n = ncut ? ncut : C - 1;
    const long frames = (long)B * T;
    if (ncut && frames > 0) {
        long g = (frames + 3) / 4;
        if (g > 16384) g = 16384;
        hipLaunchKernelGGL(ctc_beam_cut_kernel, dim3((unsigned)g), dim3(CTC_THREADS), 0, nntk_stream(), d_probs, T, C, blank, n, d_lens,
                           d_pairs, frames);
        NNTK_LAUNCH_CHECK("ctc_beam_cut_kernel");
    }
    // the frame's probabilities (or its cut pairs) double-buffered in LDS where they fit beside the cells
    const bool stage = beam_lds(W, n, C, ncut != 0, true, lm != nullptr).total <= CTC_LDS_LIMIT;
    const size_t lds = beam_lds(W, n, C, ncut != 0, stage, lm != nullptr).total;
    if (lds > CTC_LDS_LIMIT)
        return nntk_fail_msg(STREAM ? "nntk_ctc_beam_stream_push_device: the beam does not fit one workgroup's LDS"
                                    : "nntk_ctc_beam_decode_device: the beam does not fit one workgroup's LDS");
    const unsigned magic = n + 1 > 1 ? (unsigned)(0x100000000ull / (unsigned)(n + 1)) + 1u : 0u;
    const nntk_shim_lm lmv = lm ? *lm : nntk_shim_lm();
    if (beam_dispatch([&](auto cut, auto stg, auto lmc, auto det) {
            const auto kern = ctc_beam_kernel<cut.value, stg.value, STREAM, lmc.value, det.value>;
            if (lds > 48 * 1024 && nntk_set_max_dynamic_lds((const void *)kern, lds)) return -1;
            hipLaunchKernelGGL(kern, dim3((unsigned)B), dim3(CTC_THREADS), lds, nntk_stream(), d_probs, T, C, blank, W, n, magic, d_lens,
                               d_nfin, d_hist, d_mass, d_pairs, cs, lmv, d_forder, d_fmass);
            return 0;
        }, ncut != 0, stage, lm != nullptr, detail)) return -1;
    NNTK_LAUNCH_CHECK("ctc_beam_kernel");
    return 0;
}

extern "C" {

size_t nntk_shim_ctc_beam_workspace_floats(int batch, int T, int C, int beam_width, int cutoff_top_n, int lm) {
    return beam_layout(batch, T, beam_width, beam_ncut(C, cutoff_top_n), lm != 0).total;
}

int nntk_shim_ctc_beam_decode(const float *d_probs, int B, int T, int C, const int *h_input_lengths, int blank, int W, int cutoff_top_n,
                              int nbest, const nntk_shim_lm *lm, int *d_labels_out, int *d_out_lengths, float *d_scores,
                              int *d_label_frames, float *d_label_logps, float *d_ws) {
    if (B <= 0) return 0;
    const bool detail = d_label_frames || d_label_logps;
    if (((uintptr_t)d_ws & 15) != 0) return nntk_fail_msg("nntk_ctc_beam_decode_device: the workspace must be 16-byte aligned");
    const int ncut = beam_ncut(C, cutoff_top_n), n = ncut ? ncut : C - 1;
    if (W < 1 || W > BEAM_MAX_W || nbest < 1 || nbest > W || (long)W * (n + 1) > BEAM_MAX_CELLS || T > BEAM_MAX_T)
        return nntk_fail_msg("nntk_ctc_beam_decode_device: beam_width, nbest or beam_width * (classes + 1) beyond the kernel's limits");
    const BeamLayout lay = beam_layout(B, T, W, ncut, lm != nullptr);
    int *d_lens = (int *)d_ws, *d_nfin = d_lens + B;
    int *d_forder = (int *)(d_ws + lay.forder);
    float4 *d_fmass = (float4 *)(d_ws + lay.fmass);
    int2 *d_hist = (int2 *)(d_ws + lay.hist);
    float4 *d_mass = (float4 *)(d_ws + lay.mass);
    if (nntk_shim_upload_ints(d_lens, h_input_lengths, B)) return -1;
    if (beam_launch<false>(d_probs, B, T, C, blank, W, ncut, lm, detail, d_lens, d_nfin, d_hist, d_mass, (float2 *)(d_ws + lay.cut), BeamCarry(),
                           d_forder, d_fmass)) return -1;
    const size_t blds = (size_t)BEAM_BT_RECORDS * sizeof(int2);
    if (beam_dispatch([&](auto fin, auto det) {
            const auto kern = ctc_beam_backtrack_kernel<fin.value, det.value>;
            if (nntk_set_max_dynamic_lds((const void *)kern, blds)) return -1;
            hipLaunchKernelGGL(kern, dim3((unsigned)B), dim3(CTC_THREADS), blds, nntk_stream(), T, W, nbest, d_lens, d_nfin, d_hist, d_mass,
                               d_forder, d_fmass, d_labels_out, d_out_lengths, d_scores, d_probs, C, d_label_frames, d_label_logps);
            return 0;
        }, lm != nullptr, detail)) return -1;
    NNTK_LAUNCH_CHECK("ctc_beam_backtrack_kernel");
    return 0;
}

// ---- streaming form: the handle's buffer (beam_stream_layout), one push ----
size_t nntk_shim_ctc_beam_stream_floats(int batch, int max_frames, int C, int beam_width, int cutoff_top_n, int max_labels, int lm,
                                        int detail) {
    return beam_stream_layout(batch, max_frames, beam_width, beam_ncut(C, cutoff_top_n), max_labels, lm != 0, detail != 0).total;
}

// the limits of the kernel that only the launch knows in the one-shot call; no device is touched.  lm: with the per-entry LM state in the
// LDS state block
int nntk_shim_ctc_beam_stream_check(int C, int W, int cutoff_top_n, int lm) {
    const int ncut = beam_ncut(C, cutoff_top_n), n = ncut ? ncut : C - 1;
    if (W < 1 || W > BEAM_MAX_W || (long)W * (n + 1) > BEAM_MAX_CELLS)
        return nntk_fail_msg("nntk_ctc_beam_stream_create: beam_width or beam_width * (classes + 1) beyond the kernel's limits");
    if (beam_lds(W, n, C, ncut != 0, false, lm != 0).total > CTC_LDS_LIMIT)
        return nntk_fail_msg("nntk_ctc_beam_stream_create: the beam does not fit one workgroup's LDS");
    return 0;
}

int nntk_shim_ctc_beam_stream_push(const float *d_probs, int B, int T, int C, const int *h_ctl, int any_frames, int blank, int W,
                                   int cutoff_top_n, int nbest, int L, const nntk_shim_lm *lm, int detail, int *d_labels_out,
                                   int *d_out_lengths, float *d_scores, int *d_label_frames, float *d_label_logps, float *d_buf) {
    if (B <= 0) return 0;
    if (((uintptr_t)d_buf & 15) != 0) return nntk_fail_msg("nntk_ctc_beam_stream_push_device: the handle's buffer is not 16-byte aligned");
    const int ncut = beam_ncut(C, cutoff_top_n);
    const BeamStreamLayout lay = beam_stream_layout(B, T, W, ncut, L, lm != nullptr, detail != 0);
    int *d_ctl = (int *)d_buf;
    BeamCarry cs;
    cs.nb = (int *)(d_buf + lay.nb);
    cs.mass = (float4 *)(d_buf + lay.mass);
    cs.h = (u64 *)(d_buf + lay.h);
    cs.ph = (u64 *)(d_buf + lay.ph);
    cs.tail = (int2 *)(d_buf + lay.tail);
    cs.lm = lm ? (int *)(d_buf + lay.lm) : nullptr;
    cs.seen = d_ctl + B;
    int *d_strs = (int *)(d_buf + lay.str);
    int *d_fstrs = (int *)(d_buf + lay.fstr);
    float *d_lstrs = d_buf + lay.lstr;
    int2 *d_hist = (int2 *)(d_buf + lay.hist);
    const nntk_shim_lm lmv = lm ? *lm : nntk_shim_lm();
    if (nntk_shim_upload_ints(d_ctl, h_ctl, 4L * B)) return -1;
    if (any_frames && beam_launch<true>(d_probs, B, T, C, blank, W, ncut, lm, detail != 0, d_ctl, nullptr, d_hist, nullptr, (float2 *)(d_buf + lay.cut),
                                        cs, nullptr, nullptr)) return -1;
    const size_t blds = (size_t)BEAM_BT_RECORDS * sizeof(int2);
    if (beam_dispatch([&](auto fin, auto det) {
            const auto kern = ctc_beam_commit_kernel<fin.value, det.value>;
            if (nntk_set_max_dynamic_lds((const void *)kern, blds)) return -1;
            hipLaunchKernelGGL(kern, dim3((unsigned)B), dim3(CTC_THREADS), blds, nntk_stream(), B, T, W, nbest, L, d_ctl, cs, d_hist, d_strs,
                               d_labels_out, d_out_lengths, d_scores, lmv, d_probs, C, d_fstrs, d_lstrs, d_label_frames, d_label_logps);
            return 0;
        }, lm != nullptr, detail != 0)) return -1;
    NNTK_LAUNCH_CHECK("ctc_beam_commit_kernel");
    return 0;
}

}  // extern "C"
