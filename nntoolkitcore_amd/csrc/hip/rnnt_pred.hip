// rnnt_pred.hip -- the label embedding of the transducer's prediction network, for training (csrc/host/rnnt_pred.c; INTEGRATION.md
// "RNN-Transducer: training the prediction network"): the row lookup and the gradient with respect to the table.  No atomics anywhere.
//
// Row select (rows_select_kernel): out[r][:] = src[idx[r]][:], or exact zeros for idx[r] < 0.  No arithmetic touches a value, so the rows
// are bit copies (NaN payloads included).  The indices are host memory and ride in the kernel arguments, 960 rows a launch: nothing is
// staged and the host array is free on return.  It is the embedding lookup (src = the table) and the mask of the predictor's backward
// (src = d_dpred, idx[r] = r for a live row).  16-byte accesses when the width is a multiple of 4 and both pointers are 16-byte aligned,
// else one float per lane: the bits are the same.
//
// Table gradient: d_dtable[v][:] = sum of d_dout[r][:] over the rows r with ids[r] == v.  The host (rnnt_pred.c) counting-sorts the row
// numbers by id -- ascending r inside an id -- and uploads one int plan in stream order into the workspace:
//     offsets [V + 1] | sorted rows [n_sorted] | heavy chunks [n_items][2] = (id, chunk) | heavy ids [n_heavy][2] = (id, first slot)
// THE SUMMATION SHAPE of an id with n occurrences r_0 < r_1 < .. depends on n alone.  With C = NNTK_EMBED_CHUNK = 32:
//     chunk c holds r_{cC} .. r_{min(n, (c+1)C) - 1};  partial_c = ((x[r_{cC}] + x[r_{cC+1}]) + x[r_{cC+2}]) + ..   (ascending, one f32 chain
//     per element, starting FROM the first row: one occurrence is a bit copy);   result = ((partial_0 + partial_1) + partial_2) + ..
// n == 0: exact zeros.  n <= C is a single chunk, summed by the workgroup that owns table row v and stored there.  n > C (a "heavy" id --
// in transducer use the start symbol, once per batch row): every chunk is summed by a workgroup of its own into a partial row of the
// workspace (embedding_grad_kernel, the same launch as the light ids), and a second launch adds an id's partials in chunk order
// (embedding_combine_kernel).  So a heavy id is ceil(n / C) parallel chains of C rows and one of ceil(n / C) partials, never one chain
// of n rows on one wavefront.  Neither V, nor the other ids, nor the grid enter an id's sum: the bits of d_dtable[v] are a function of
// the ascending row list of v and those rows' values.  Rows with id -1 are in no list and are never read.
#include <stdint.h>
#include <string.h>
#include "nntk_common.hpp"

#define PRED_THREADS 256
#define PRED_IDX_PER_LAUNCH 960
static_assert(NNTK_EMBED_CHUNK == 32, "the documented summation shape");

struct PredIdxChunk { int v[PRED_IDX_PER_LAUNCH]; };

// lpr lanes (a power of two, <= 256) walk one row; a workgroup holds 256 / lpr rows
template <bool VEC>
__global__ __launch_bounds__(PRED_THREADS) void rows_select_kernel(const float *__restrict__ src, PredIdxChunk idx, int rows, int width,
                                                                    int lpr, float *__restrict__ out) {
    const int r = blockIdx.x * (PRED_THREADS / lpr) + (int)threadIdx.x / lpr;
    const int lane = (int)threadIdx.x & (lpr - 1);
    if (r >= rows) return;
    const int s = idx.v[r];
    if (VEC) {
        const f32x4 *sp = (const f32x4 *)(src + (size_t)(s < 0 ? 0 : s) * width);
        f32x4 *op = (f32x4 *)(out + (size_t)r * width);
        const f32x4 zero = { 0.0f, 0.0f, 0.0f, 0.0f };
        for (int u = lane; u < width / 4; u += lpr) op[u] = s < 0 ? zero : sp[u];
    } else {
        const float *sp = src + (size_t)(s < 0 ? 0 : s) * width;
        float *op = out + (size_t)r * width;
        for (int u = lane; u < width; u += lpr) op[u] = s < 0 ? 0.0f : sp[u];
    }
}

static bool pred_vec_ok(int width, const void *a, const void *b, const void *c) {
    return width % 4 == 0 && (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15) == 0;
}

// the lanes a row of `units` accesses takes: the next power of two, at most the workgroup
static int pred_lanes(int units) {
    int l = 1;
    while (l < units && l < PRED_THREADS) l <<= 1;
    return l;
}

int nntk_shim_rows_select(const float *d_src, int width, const int *h_idx, long rows, float *d_out) {
    if (rows <= 0 || width <= 0) return 0;
    const bool vec = pred_vec_ok(width, d_src, d_out, NULL);
    const int lpr = pred_lanes(vec ? width / 4 : width), rpb = PRED_THREADS / lpr;
    for (long r0 = 0; r0 < rows; r0 += PRED_IDX_PER_LAUNCH) {
        const int m = rows - r0 < PRED_IDX_PER_LAUNCH ? (int)(rows - r0) : PRED_IDX_PER_LAUNCH;
        PredIdxChunk c;
        memcpy(c.v, h_idx + r0, (size_t)m * sizeof(int));
        float *out = d_out + (size_t)r0 * width;
        if (vec)
            hipLaunchKernelGGL(rows_select_kernel<true>, dim3((unsigned)nntk_cdiv(m, rpb)), dim3(PRED_THREADS), 0, nntk_stream(), d_src, c, m,
                               width, lpr, out);
        else
            hipLaunchKernelGGL(rows_select_kernel<false>, dim3((unsigned)nntk_cdiv(m, rpb)), dim3(PRED_THREADS), 0, nntk_stream(), d_src, c, m,
                               width, lpr, out);
    }
    NNTK_LAUNCH_CHECK("rows_select_kernel");
    return 0;
}

// ---- the table gradient ----
template <bool VEC> struct PredVal { typedef float type; };
template <> struct PredVal<true> { typedef f32x4 type; };

// x[rows[0]] + x[rows[1]] + .. in that order, one chain per element; the loads of eight rows are in flight at a time
template <bool VEC>
__device__ __forceinline__ typename PredVal<VEC>::type pred_chain(const float *__restrict__ x, const int *__restrict__ rows, int n, int E,
                                                                   int u) {
    typedef typename PredVal<VEC>::type val;
    val acc = ((const val *)(x + (size_t)rows[0] * E))[u];
    for (int i0 = 1; i0 < n; i0 += 8) {
        val t[8];
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (i0 + k < n) t[k] = ((const val *)(x + (size_t)rows[i0 + k] * E))[u];
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (i0 + k < n) acc += t[k];
    }
    return acc;
}

// workgroups [0, V): table row v when it has at most one chunk (zeros when it has none); workgroups V + i: heavy chunk i into partial row i
template <bool VEC>
__global__ __launch_bounds__(PRED_THREADS) void embedding_grad_kernel(const float *__restrict__ dout, const int *__restrict__ offsets,
                                                                       const int *__restrict__ sorted, const int *__restrict__ items, int V,
                                                                       int E, float *__restrict__ dtable, float *__restrict__ partial) {
    typedef typename PredVal<VEC>::type val;
    const int b = blockIdx.x, units = VEC ? E / 4 : E;
    int begin, n;
    val *dst;
    if (b < V) {
        begin = offsets[b];
        n = offsets[b + 1] - begin;
        if (n > NNTK_EMBED_CHUNK) return;                       // a heavy id: its chunks are items, its row is the combine kernel's
        dst = (val *)(dtable + (size_t)b * E);
    } else {
        const int v = items[2 * (b - V)], c = items[2 * (b - V) + 1];
        begin = offsets[v] + c * NNTK_EMBED_CHUNK;
        n = min(NNTK_EMBED_CHUNK, offsets[v + 1] - begin);
        dst = (val *)(partial + (size_t)(b - V) * E);
    }
    for (int u = threadIdx.x; u < units; u += blockDim.x) {
        val acc = val();
        if (n > 0) acc = pred_chain<VEC>(dout, sorted + begin, n, E, u);
        dst[u] = acc;
    }
}

// table row of heavy id h = its partial rows added in chunk order
template <bool VEC>
__global__ __launch_bounds__(PRED_THREADS) void embedding_combine_kernel(const float *__restrict__ partial, const int *__restrict__ offsets,
                                                                          const int *__restrict__ heavy, int E, float *__restrict__ dtable) {
    typedef typename PredVal<VEC>::type val;
    const int v = heavy[2 * blockIdx.x], slot = heavy[2 * blockIdx.x + 1], units = VEC ? E / 4 : E;
    const int chunks = (offsets[v + 1] - offsets[v] + NNTK_EMBED_CHUNK - 1) / NNTK_EMBED_CHUNK;
    val *dst = (val *)(dtable + (size_t)v * E);
    for (int u = threadIdx.x; u < units; u += blockDim.x) {
        val acc = ((const val *)(partial + (size_t)slot * E))[u];
        for (int c = 1; c < chunks; ++c) acc += ((const val *)(partial + (size_t)(slot + c) * E))[u];
        dst[u] = acc;
    }
}

// the most chunks of heavy ids that `rows` rows can make: an id with n > C rows has ceil(n / C) <= n / 16 of them
static size_t pred_max_items(long rows) { return (size_t)(rows / 16) + 1; }
static size_t pred_max_heavy(long rows) { return (size_t)(rows / (NNTK_EMBED_CHUNK + 1)) + 1; }
static size_t pred_round4(size_t n) { return (n + 3) & ~(size_t)3; }

size_t nntk_shim_embedding_workspace_floats(long rows, int V, int E) {
    if (rows < 0 || V < 0 || E < 0) return 0;
    const size_t ints = (size_t)V + 1 + (size_t)rows + 2 * pred_max_items(rows) + 2 * pred_max_heavy(rows);
    return pred_round4(ints) + pred_max_items(rows) * (size_t)E + 4;
}

int nntk_shim_embedding_grad(const float *d_dout, int V, int E, const int *h_plan, long n_sorted, long n_items, long n_heavy, float *d_dtable,
                             float *d_ws) {
    if ((size_t)n_items > pred_max_items(n_sorted) || (size_t)n_heavy > pred_max_heavy(n_sorted))
        return nntk_fail_msg("nntk_shim_embedding_grad: the plan is larger than the workspace");
    const size_t n_ints = (size_t)V + 1 + (size_t)n_sorted + 2 * (size_t)n_items + 2 * (size_t)n_heavy;
    int *d_plan = (int *)d_ws;
    if (nntk_shim_upload_ints(d_plan, h_plan, (long)n_ints)) return -1;
    const int *d_off = d_plan, *d_sorted = d_off + V + 1, *d_items = d_sorted + n_sorted, *d_heavy = d_items + 2 * n_items;
    float *d_partial = d_ws + pred_round4(n_ints);
    const bool vec = pred_vec_ok(E, d_dout, d_dtable, d_partial);
    const int units = vec ? E / 4 : E;
    const int threads = 64 * nntk_cdiv(units < PRED_THREADS ? units : PRED_THREADS, 64);
    const dim3 grid((unsigned)((long)V + n_items));
    if (vec)
        hipLaunchKernelGGL(embedding_grad_kernel<true>, grid, dim3(threads), 0, nntk_stream(), d_dout, d_off, d_sorted, d_items, V, E, d_dtable,
                           d_partial);
    else
        hipLaunchKernelGGL(embedding_grad_kernel<false>, grid, dim3(threads), 0, nntk_stream(), d_dout, d_off, d_sorted, d_items, V, E, d_dtable,
                           d_partial);
    NNTK_LAUNCH_CHECK("embedding_grad_kernel");
    if (n_heavy == 0) return 0;
    if (vec)
        hipLaunchKernelGGL(embedding_combine_kernel<true>, dim3((unsigned)n_heavy), dim3(threads), 0, nntk_stream(), d_partial, d_off, d_heavy, E,
                           d_dtable);
    else
        hipLaunchKernelGGL(embedding_combine_kernel<false>, dim3((unsigned)n_heavy), dim3(threads), 0, nntk_stream(), d_partial, d_off, d_heavy,
                           E, d_dtable);
    NNTK_LAUNCH_CHECK("embedding_combine_kernel");
    return 0;
}
