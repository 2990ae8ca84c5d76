// bd_train.hip -- data movement of the bidirectional TRAINING calls (*BidirectionalApplyTrainingBatchDevice /
// *BidirectionalCalculateGradientDevice, the bd_*_gradient*_device helpers): the forward merge, the scatter of the output gradient to the
// two directions and the sum of their input gradients, each with the per-row time reversal folded in.  The recurrences themselves are the
// unidirectional training kernels (train.hip, recurrent_rr.hip), untouched.
//
// All f32, one pass with no arithmetic beyond the index split and at most one add (built to be memory-bound): every tensor read and written once (the sum merge's scatter reads d_out twice: both directions take
// the whole row).  A lane moves V = 4 floats (16 bytes) where the feature widths are multiples of 4 and the pointers 16-byte aligned, else
// V = 1; a row's reversal moves whole feature vectors, so the two forms give the same bits.  Plain stores only.
// Throughout L = len ? len[b] : T.  Rows t >= L are written as exact zeros, whatever the inputs hold there.
#include "nntk_common.hpp"

namespace {

template <int V> struct Vec;
template <> struct Vec<1> { typedef float type; };
template <> struct Vec<4> { typedef float4 type; };

template <int V> __device__ __forceinline__ typename Vec<V>::type vzero();
template <> __device__ __forceinline__ float vzero<1>() { return 0.0f; }
template <> __device__ __forceinline__ float4 vzero<4>() { return make_float4(0.0f, 0.0f, 0.0f, 0.0f); }
__device__ __forceinline__ float vadd(float a, float b) { return a + b; }
__device__ __forceinline__ float4 vadd(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

// unit e of a [B][R][Wv] tensor of V-float vectors -> (b, t, c).  I: the index type, 32 bits wherever the tensor's unit count fits (the
// 64-bit divisions are emulated on the GPU and would cost more than the memory access they serve)
template <typename I> struct Pos { I b; int t, c; };
template <typename I> __device__ __forceinline__ Pos<I> pos_of(I e, int R, int Wv) {
    Pos<I> p;
    const I r = e / (I)Wv;
    p.c = (int)(e - r * (I)Wv);
    p.b = r / (I)R;
    p.t = (int)(r - p.b * (I)R);
    return p;
}

// out[b][t] = merge(of[b][t], obr[b][L-1-t]) for t < L, zeros for t >= L (seq); out[b] = merge(of[b], obr[b]) (R = 1, seq = 0).
// concat: forward in columns [0, H), backward in [H, 2H); else one add, forward operand first.  Hv = H / V.
template <int V, typename I>
__global__ __launch_bounds__(256) void bd_merge_kernel(const typename Vec<V>::type *__restrict__ of, const typename Vec<V>::type *__restrict__ obr,
                                                       typename Vec<V>::type *__restrict__ out, const int *__restrict__ len,
                                                       long B, int R, int Hv, int seq, int concat) {
    typedef typename Vec<V>::type vec;
    const int Wv = concat ? 2 * Hv : Hv;
    const I total = (I)B * R * Wv;
    for (I e = blockIdx.x * (I)blockDim.x + threadIdx.x; e < total; e += (I)gridDim.x * blockDim.x) {
        const Pos<I> p = pos_of<I>(e, R, Wv);
        const int L = seq ? (len ? len[p.b] : R) : 1;
        vec v = vzero<V>();
        if (p.t < L) {
            const I rf = p.b * R + p.t, rb = p.b * R + (seq ? L - 1 - p.t : 0);
            if (!concat) v = vadd(of[rf * Hv + p.c], obr[rb * Hv + p.c]);
            else v = p.c < Hv ? of[rf * Hv + p.c] : obr[rb * Hv + (p.c - Hv)];
        }
        out[e] = v;
    }
}

// d_of[b][t] = dout[b][t][forward part], d_ob[b][t] = dout[b][rev ? L-1-t : t][backward part] for t < L, both zeros for t >= L (seq);
// R = 1, seq = 0: the plain split / copy.  concat: the parts are columns [0, H) and [H, 2H) of 2H-wide rows; else both are the whole row.
template <int V, typename I>
__global__ __launch_bounds__(256) void bd_scatter_kernel(const typename Vec<V>::type *__restrict__ dout, typename Vec<V>::type *__restrict__ d_of,
                                                         typename Vec<V>::type *__restrict__ d_ob, const int *__restrict__ len,
                                                         long B, int R, int Hv, int seq, int concat, int rev) {
    typedef typename Vec<V>::type vec;
    const int Wv = concat ? 2 * Hv : Hv, boff = concat ? Hv : 0;
    const I total = (I)B * R * Hv;
    for (I e = blockIdx.x * (I)blockDim.x + threadIdx.x; e < total; e += (I)gridDim.x * blockDim.x) {
        const Pos<I> p = pos_of<I>(e, R, Hv);
        const int L = seq ? (len ? len[p.b] : R) : 1;
        vec f = vzero<V>(), b = vzero<V>();
        if (p.t < L) {
            const I rf = p.b * R + p.t, rb = p.b * R + (rev && seq ? L - 1 - p.t : p.t);
            f = dout[rf * Wv + p.c];
            b = dout[rb * Wv + boff + p.c];
        }
        d_of[e] = f;
        d_ob[e] = b;
    }
}

// dx[b][t] = dxf[b][t] + dxbr[b][L-1-t] for t < L (one add, forward operand first), zeros for t >= L
template <int V, typename I>
__global__ __launch_bounds__(256) void bd_accumulate_kernel(const typename Vec<V>::type *__restrict__ dxf, const typename Vec<V>::type *__restrict__ dxbr,
                                                            typename Vec<V>::type *__restrict__ dx, const int *__restrict__ len,
                                                            long B, int T, int Fv) {
    typedef typename Vec<V>::type vec;
    const I total = (I)B * T * Fv;
    for (I e = blockIdx.x * (I)blockDim.x + threadIdx.x; e < total; e += (I)gridDim.x * blockDim.x) {
        const Pos<I> p = pos_of<I>(e, T, Fv);
        const int L = len ? len[p.b] : T;
        vec v = vzero<V>();
        if (p.t < L) v = vadd(dxf[e], dxbr[(p.b * T + (L - 1 - p.t)) * Fv + p.c]);
        dx[e] = v;
    }
}

int grid_for(long work_items) {
    long g = (work_items + 255) / 256;
    if (g < 1) g = 1;
    if (g > 2048) g = 2048;   // 256 CUs x 8 blocks; grid-stride beyond
    return (int)g;
}

bool aligned16(const void *a, const void *b, const void *c) { return (((size_t)a | (size_t)b | (size_t)c) & 15) == 0; }
bool overlap(const float *a, long na, const float *b, long nb) { return a < b + nb && b < a + na; }

// the kernel's index type: 32 bits while the largest tensor of the call stays below 2^31 floats (so that no index, the grid stride added,
// wraps), 64 bits beyond
#define BD_LAUNCH(kernel, V, floats, units, ...)                                                                                  \
    do {                                                                                                                        \
        if ((floats) < (1L << 31))                                                                                              \
            hipLaunchKernelGGL((kernel<V, unsigned>), dim3(grid_for(units)), dim3(256), 0, nntk_stream(), __VA_ARGS__);         \
        else                                                                                                                    \
            hipLaunchKernelGGL((kernel<V, long>), dim3(grid_for(units)), dim3(256), 0, nntk_stream(), __VA_ARGS__);             \
    } while (0)

}  // namespace

extern "C" {

int nntk_shim_bd_merge(const float *d_of, const float *d_obr, float *d_out, const int *d_len, long B, int T, int H,
                       int return_sequences, int concat) {
    const int R = return_sequences ? T : 1;
    if (B <= 0 || R <= 0 || H <= 0) return 0;
    const long n = B * R * H;
    const long no = concat ? 2 * n : n;
    if (overlap(d_out, no, d_of, n) || overlap(d_out, no, d_obr, n))
        return nntk_fail_msg("bd_merge: the output overlaps an input");
    if (H % 4 == 0 && aligned16(d_of, d_obr, d_out))
        BD_LAUNCH(bd_merge_kernel, 4, no, no / 4, (const float4 *)d_of, (const float4 *)d_obr, (float4 *)d_out, d_len, B, R, H / 4,
                  return_sequences, concat);
    else
        BD_LAUNCH(bd_merge_kernel, 1, no, no, d_of, d_obr, d_out, d_len, B, R, H, return_sequences, concat);
    NNTK_LAUNCH_CHECK("bd_merge_kernel");
    return 0;
}

int nntk_shim_bd_scatter(const float *d_dout, float *d_of, float *d_ob, const int *d_len, long B, int T, int H,
                         int return_sequences, int concat, int reverse) {
    const int R = return_sequences ? T : 1;
    if (B <= 0 || R <= 0 || H <= 0) return 0;
    const long n = B * R * H;
    if (overlap(d_dout, concat ? 2 * n : n, d_of, n) || overlap(d_dout, concat ? 2 * n : n, d_ob, n) || overlap(d_of, n, d_ob, n))
        return nntk_fail_msg("bd_scatter: the tensors overlap");
    if (H % 4 == 0 && aligned16(d_dout, d_of, d_ob))
        BD_LAUNCH(bd_scatter_kernel, 4, concat ? 2 * n : n, n / 4, (const float4 *)d_dout, (float4 *)d_of, (float4 *)d_ob, d_len, B, R, H / 4,
                  return_sequences, concat, reverse);
    else
        BD_LAUNCH(bd_scatter_kernel, 1, concat ? 2 * n : n, n, d_dout, d_of, d_ob, d_len, B, R, H, return_sequences, concat, reverse);
    NNTK_LAUNCH_CHECK("bd_scatter_kernel");
    return 0;
}

int nntk_shim_bd_accumulate(const float *d_dxf, const float *d_dxbr, float *d_dx, const int *d_len, long B, int T, int F) {
    if (B <= 0 || T <= 0 || F <= 0) return 0;
    const long n = B * T * F;
    // (d_dx == d_dxf is fine: a lane reads the element it writes; any other overlap is not)
    if (overlap(d_dx, n, d_dxbr, n) || (d_dx != d_dxf && overlap(d_dx, n, d_dxf, n)))
        return nntk_fail_msg("bd_accumulate: the output overlaps an input");
    if (F % 4 == 0 && aligned16(d_dxf, d_dxbr, d_dx))
        BD_LAUNCH(bd_accumulate_kernel, 4, n, n / 4, (const float4 *)d_dxf, (const float4 *)d_dxbr, (float4 *)d_dx, d_len, B, T, F / 4);
    else
        BD_LAUNCH(bd_accumulate_kernel, 1, n, n, d_dxf, d_dxbr, d_dx, d_len, B, T, F);
    NNTK_LAUNCH_CHECK("bd_accumulate_kernel");
    return 0;
}

}  // extern "C"
