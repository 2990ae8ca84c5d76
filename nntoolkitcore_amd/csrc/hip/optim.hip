// optim.hip -- the device-side optimizer step (nntk_optimizer_*): SGD, momentum SGD and Adam / AdamW over any number of caller-owned
// (weights, gradient) blocks, with gradient scaling, global-norm clipping, a non-finite guard and gradient zeroing, in TWO launches per step
// whatever the number of blocks, with no atomics and nothing read back by the host.
//
// Index space.  Every block is cut into chunks of `chunk` floats (a multiple of 1024, fixed by the TOTAL size: optim_chunk_floats) of its
// VIRTUAL range: virtual index j = i + phase, phase = (address of w / 4) & 3, so that virtual quad q = [4 q, 4 q + 4) of a block is one
// 16-byte-aligned float4 of w -- and of the moments, which the host lays out with the same phase.  A quad that lies inside the block moves
// as one 16-byte access per array (the gradient too when its pointer has the phase of w; 4-byte accesses otherwise); the one or two quads
// that straddle a block's ends are the scalar head and tail.  The chunks of all blocks form one flat list (d_blocks[b].chunk0 = the first
// chunk of block b; a workgroup finds its block by bisection) that the grid strides over: forty small blocks and one large block load the
// machine alike.
//
// Pass 1 (optim_norm_kernel): partial[c] = sum of (g * grad_scale)^2 over chunk c -- per thread in quad order, then a fixed xor tree over
//   the wavefront, then the four wavefronts in order.  A chunk's sum depends on that block's values, size and phase alone.
// Pass 2 (optim_step_kernel): EVERY workgroup re-adds all partials itself.  Floating-point sums depend on their order, and the order of
//   the chunks is the order in which the caller listed the blocks; so the partials are added EXACTLY: scaled by a power of two taken from
//   their maximum, truncated to 64-bit integers and summed as integers, which is associative.  The norm is therefore one value for every
//   workgroup and every listing order.  Then: skip = the norm is not finite (a NaN or inf anywhere); clip = min(1, clip_norm / (norm + 1e-6));
//   the update of the workgroup's chunks; with zero_gradients +0.0 into every gradient element, skipped step or not.
// Control block d_ctl [8]: 0 norm | 1 clip factor (0 on a skipped step) | 2 skipped | 3 steps taken | 4 learning rate | 5 steps, read by
//   pass 2 | 6 steps, written by pass 2.  Pass 1 copies word 6 to word 5, so no workgroup of pass 2 reads a word another one writes, and a
//   replayed launch sequence counts on.  Words 5 and 6 hold an unsigned integer.
#include "nntk_common.hpp"

// every operation rounds separately (no a * b + c contraction): kind 0 without scale, clip and decay is then train.hip's sgd_kernel bit for bit
#pragma clang fp contract(off)

#define OPT_THREADS 256
#define OPT_MAX_GRID 2048          // 256 CUs x 8 workgroups: the grid strides over the remaining chunks

static __device__ __forceinline__ int optim_find_block(const nntk_optim_block *__restrict__ blocks, int n_blocks, long c) {
    int lo = 0, hi = n_blocks - 1;             // the last block with chunk0 <= c (empty blocks share their successor's chunk0 and are passed over)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (blocks[mid].chunk0 <= c) lo = mid; else hi = mid - 1;
    }
    return lo;
}

static __device__ __forceinline__ float wave_sum_f32(float s) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
    return s;
}

__global__ __launch_bounds__(OPT_THREADS) void optim_norm_kernel(nntk_optim_plan p) {
    __shared__ float wsum[OPT_THREADS / 64];
    unsigned *ctl_u = reinterpret_cast<unsigned *>(p.d_ctl);
    if (blockIdx.x == 0 && threadIdx.x == 0) ctl_u[5] = ctl_u[6];
    const int quads = p.chunk_floats / 4;
    const float gs = p.grad_scale;
    for (long c = blockIdx.x; c < p.n_chunks; c += gridDim.x) {
        const nntk_optim_block b = p.d_blocks[optim_find_block(p.d_blocks, p.n_blocks, c)];
        const long j0 = (c - b.chunk0) * p.chunk_floats, lo = b.phase, hi = b.phase + b.n;
        const float *gv = b.g - b.phase;                   // virtual index -> address (dereferenced inside [lo, hi) only)
        float s = 0.0f;
        for (int q = threadIdx.x; q < quads; q += OPT_THREADS) {
            const long j = j0 + 4L * q;
            if (j >= hi) break;
            float x0 = 0.f, x1 = 0.f, x2 = 0.f, x3 = 0.f;
            if (b.g_vec && j >= lo && j + 4 <= hi) {
                const float4 v = *reinterpret_cast<const float4 *>(gv + j);
                x0 = v.x; x1 = v.y; x2 = v.z; x3 = v.w;
            } else {
                if (j >= lo) x0 = gv[j];
                if (j + 1 >= lo && j + 1 < hi) x1 = gv[j + 1];
                if (j + 2 >= lo && j + 2 < hi) x2 = gv[j + 2];
                if (j + 3 >= lo && j + 3 < hi) x3 = gv[j + 3];
            }
            x0 *= gs; x1 *= gs; x2 *= gs; x3 *= gs;
            s += (x0 * x0 + x1 * x1) + (x2 * x2 + x3 * x3);
        }
        s = wave_sum_f32(s);
        if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = s;
        __syncthreads();
        if (threadIdx.x == 0) p.d_partial[c] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
        __syncthreads();
    }
}

struct OptStep {                  // what every workgroup of pass 2 derives for itself
    float clip, lr, step_size, bc2_sqrt, decay_mul, one_m_b1, one_m_b2;     // (the scalars are formed in double and rounded once, as PyTorch forms them)
    int skip;
};

// the element update: PyTorch's SGD / Adam / AdamW (foreach-free, single tensor) formulas, one rounding per operation
static __device__ __forceinline__ void optim_update(const nntk_optim_plan &p, const OptStep &s, float g, float &w, float &m, float &v) {
    g = (g * p.grad_scale) * s.clip;
    if (p.weight_decay != 0.0f) {
        if (p.decoupled) w = w * s.decay_mul;
        else g = g + p.weight_decay * w;
    }
    if (p.kind == 0) {
        w = w - g * s.lr;
    } else if (p.kind == 1) {
        m = p.momentum * m + g;                             // the buffer starts at zero: the first step leaves it equal to g
        if (p.nesterov) g = g + p.momentum * m; else g = m;
        w = w - g * s.lr;
    } else {
        m = m + s.one_m_b1 * (g - m);                       // lerp
        v = p.beta2 * v + (s.one_m_b2 * g) * g;
        const float denom = sqrtf(v) / s.bc2_sqrt + p.epsilon;
        w = w - (s.step_size * m) / denom;
    }
}

__global__ __launch_bounds__(OPT_THREADS) void optim_step_kernel(nntk_optim_plan p) {
    __shared__ float wmax[OPT_THREADS / 64];
    __shared__ int wbad[OPT_THREADS / 64];
    __shared__ unsigned long long wacc[OPT_THREADS / 64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    // ---- the global norm from the partials: maximum and a non-finite flag, then the exact integer sum ----
    float mx = 0.0f;
    int bad = 0;
    for (long i = threadIdx.x; i < p.n_chunks; i += OPT_THREADS) {
        const float x = p.d_partial[i];
        if (!(x <= 3.402823466e38f)) bad = 1;               // NaN or +inf (the partials are sums of squares)
        else mx = fmaxf(mx, x);
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { mx = fmaxf(mx, __shfl_xor(mx, o, 64)); bad |= __shfl_xor(bad, o, 64); }
    if (lane == 0) { wmax[wv] = mx; wbad[wv] = bad; }
    __syncthreads();
    mx = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
    bad = wbad[0] | wbad[1] | wbad[2] | wbad[3];
    double sumsq = 0.0;
    if (!bad && mx > 0.0f) {
        int e;
        (void)frexpf(mx, &e);                               // mx < 2^e
        int bits = 1;
        while ((1L << bits) < p.n_chunks + 1) ++bits;
        const int sh = 62 - bits - e;                       // every scaled partial < 2^(62 - bits): n_chunks of them stay below 2^62
        unsigned long long acc = 0;
        for (long i = threadIdx.x; i < p.n_chunks; i += OPT_THREADS) acc += (unsigned long long)ldexp((double)p.d_partial[i], sh);
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            const unsigned lo_ = __shfl_xor((unsigned)acc, o, 64), hi_ = __shfl_xor((unsigned)(acc >> 32), o, 64);
            acc += ((unsigned long long)hi_ << 32) | lo_;
        }
        if (lane == 0) wacc[wv] = acc;
        __syncthreads();
        sumsq = ldexp((double)(wacc[0] + wacc[1] + wacc[2] + wacc[3]), -sh);
    }
    const float norm = bad ? __builtin_nanf("") : (float)sqrt(sumsq);
    OptStep s;
    s.skip = bad || !(norm <= 3.402823466e38f);
    s.clip = 1.0f;
    if (p.clip_norm > 0.0f && !s.skip) s.clip = fminf(1.0f, p.clip_norm / (norm + 1e-6f));
    s.lr = p.d_ctl[4];
    const unsigned steps = reinterpret_cast<const unsigned *>(p.d_ctl)[5];
    const double t = (double)steps + 1.0;
    s.step_size = s.lr;
    s.bc2_sqrt = 1.0f;
    if (p.kind == 2) {
        s.step_size = (float)((double)s.lr / (1.0 - pow((double)p.beta1, t)));
        s.bc2_sqrt = (float)sqrt(1.0 - pow((double)p.beta2, t));
    }
    s.decay_mul = (float)(1.0 - (double)s.lr * (double)p.weight_decay);
    s.one_m_b1 = (float)(1.0 - (double)p.beta1);
    s.one_m_b2 = (float)(1.0 - (double)p.beta2);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const unsigned after = steps + (s.skip ? 0u : 1u);
        p.d_ctl[0] = norm;
        p.d_ctl[1] = s.skip ? 0.0f : s.clip;
        p.d_ctl[2] = s.skip ? 1.0f : 0.0f;
        p.d_ctl[3] = (float)after;
        reinterpret_cast<unsigned *>(p.d_ctl)[6] = after;
    }
    if (s.skip && !p.zero_gradients) return;

    // ---- the update ----
    const int quads = p.chunk_floats / 4;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    for (long c = blockIdx.x; c < p.n_chunks; c += gridDim.x) {
        const nntk_optim_block b = p.d_blocks[optim_find_block(p.d_blocks, p.n_blocks, c)];
        const long j0 = (c - b.chunk0) * p.chunk_floats, lo = b.phase, hi = b.phase + b.n;
        float *gv = b.g - b.phase, *wp = b.w - b.phase;
        float *mp = p.kind >= 1 ? b.m - b.phase : nullptr, *vp = p.kind == 2 ? b.v - b.phase : nullptr;
        for (int q = threadIdx.x; q < quads; q += OPT_THREADS) {
            const long j = j0 + 4L * q;
            if (j >= hi) break;
            if (j >= lo && j + 4 <= hi) {                   // a whole quad: 16-byte accesses
                if (!s.skip) {
                    float4 g4;
                    if (b.g_vec) g4 = *reinterpret_cast<const float4 *>(gv + j);
                    else { g4.x = gv[j]; g4.y = gv[j + 1]; g4.z = gv[j + 2]; g4.w = gv[j + 3]; }
                    float4 w4 = *reinterpret_cast<const float4 *>(wp + j), m4 = zero4, v4 = zero4;
                    if (mp) m4 = *reinterpret_cast<const float4 *>(mp + j);
                    if (vp) v4 = *reinterpret_cast<const float4 *>(vp + j);
                    optim_update(p, s, g4.x, w4.x, m4.x, v4.x);
                    optim_update(p, s, g4.y, w4.y, m4.y, v4.y);
                    optim_update(p, s, g4.z, w4.z, m4.z, v4.z);
                    optim_update(p, s, g4.w, w4.w, m4.w, v4.w);
                    *reinterpret_cast<float4 *>(wp + j) = w4;
                    if (mp) *reinterpret_cast<float4 *>(mp + j) = m4;
                    if (vp) *reinterpret_cast<float4 *>(vp + j) = v4;
                }
                if (p.zero_gradients) {
                    if (b.g_vec) *reinterpret_cast<float4 *>(gv + j) = zero4;
                    else { gv[j] = 0.f; gv[j + 1] = 0.f; gv[j + 2] = 0.f; gv[j + 3] = 0.f; }
                }
            } else {                                        // the block's head or tail: element by element, inside [lo, hi)
                for (long i = j < lo ? lo : j; i < j + 4 && i < hi; ++i) {
                    if (!s.skip) {
                        float w = wp[i], m = mp ? mp[i] : 0.f, v = vp ? vp[i] : 0.f;
                        optim_update(p, s, gv[i], w, m, v);
                        wp[i] = w;
                        if (mp) mp[i] = m;
                        if (vp) vp[i] = v;
                    }
                    if (p.zero_gradients) gv[i] = 0.f;
                }
            }
        }
    }
}

__global__ void optim_set_kernel(float *dst, float value) { *dst = value; }

// the chunk length for a total of `total` floats: 4096, doubled until at most ~16 K chunks remain (pass 2 re-reads every partial in every
// workgroup).  It fixes the summation tree of the norm, and depends on the total alone.
extern "C" int nntk_shim_optim_chunk_floats(long total) {
    long ch = 4096;
    while (total / ch > 16384 && ch < (1L << 30)) ch *= 2;
    return (int)ch;
}

extern "C" int nntk_shim_optim_set_lr(float *d_ctl, float lr) {
    hipLaunchKernelGGL(optim_set_kernel, dim3(1), dim3(1), 0, nntk_stream(), d_ctl + 4, lr);
    NNTK_LAUNCH_CHECK("optim_set_kernel");
    return 0;
}

extern "C" int nntk_shim_optim_step(const nntk_optim_plan *plan) {
    const unsigned grid = (unsigned)(plan->n_chunks < 1 ? 1 : plan->n_chunks > OPT_MAX_GRID ? OPT_MAX_GRID : plan->n_chunks);
    hipLaunchKernelGGL(optim_norm_kernel, dim3(grid), dim3(OPT_THREADS), 0, nntk_stream(), *plan);
    NNTK_LAUNCH_CHECK("optim_norm_kernel");
    hipLaunchKernelGGL(optim_step_kernel, dim3(grid), dim3(OPT_THREADS), 0, nntk_stream(), *plan);
    NNTK_LAUNCH_CHECK("optim_step_kernel");
    return 0;
}
