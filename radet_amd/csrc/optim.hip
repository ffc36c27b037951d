// Optimiser step on flat fp32 arenas (HBM-streaming, 16-byte accesses):
//   global L2 norm (two-stage deterministic reduction) -> clip coefficient -> AdamW update, fused.
// Replaces torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW as driven by mmcv's OptimizerHook
// (configs/base/default_runtime.py:1-19; radet/apis/train.py:87-126 in the reference).
#include "common.h"
#include "../../include/radet_hip.h"

__global__ __launch_bounds__(256) void sqnorm_kernel(const float* __restrict__ g, size_t n, float* __restrict__ partials) {
    double acc = 0.0;
    const size_t n4 = n / 4;
    const float4* g4 = reinterpret_cast<const float4*>(g);
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
        const float4 v = g4[i];
        acc += (double)((v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w));
    }
    if (blockIdx.x == 0)
        for (size_t i = n4 * 4 + threadIdx.x; i < n; i += 256) acc += (double)(g[i] * g[i]);
    __shared__ double red[4];
    acc = wave_sum_d(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partials[blockIdx.x] = (float)((red[0] + red[1]) + (red[2] + red[3]));
}

extern "C" int radet_sqnorm_partials(const float* g, size_t n, float* partials, int npartials, void* stream) {
    if (npartials < 1 || npartials > 4096) return RADET_ERR_ARG;
    hipLaunchKernelGGL(sqnorm_kernel, dim3(npartials), dim3(256), 0, (hipStream_t)stream, g, n, partials);
    return radet_check_launch();
}

// Every block of an optimiser kernel: sum of sqnorm_kernel's partials -> global norm -> clip coefficient with the mean
// (1 / grad_div) folded in; block 0 also reports the norm.  Ends in a barrier.
__device__ __forceinline__ float clip_coef(float max_norm, float grad_div, const float* __restrict__ partials, int npartials,
                                           float* __restrict__ grad_norm_out) {
    __shared__ float s_coef;
    if (threadIdx.x < 64) {
        double a = 0.0;
        for (int k = threadIdx.x; k < npartials; k += 64) a += (double)partials[k];
        a = wave_sum_d(a);
        if (threadIdx.x == 0) {
            const float norm = (float)sqrt(a) / grad_div;
            float coef = 1.f;
            if (max_norm > 0.f) {
                coef = max_norm / (norm + 1e-6f);
                if (coef > 1.f) coef = 1.f;
            }
            s_coef = coef / grad_div;
            if (blockIdx.x == 0 && grad_norm_out) *grad_norm_out = norm;
        }
    }
    __syncthreads();
    return s_coef;
}

__global__ __launch_bounds__(256) void adamw_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                    float* __restrict__ m, float* __restrict__ v, size_t n, float lr,
                                                    float b1, float b2, float eps, float wd, float bc1, float bc2_sqrt,
                                                    float max_norm, float grad_div, const float* __restrict__ partials,
                                                    int npartials, float* __restrict__ grad_norm_out) {
    const float coef = clip_coef(max_norm, grad_div, partials, npartials, grad_norm_out);
    const float step = lr / bc1;
    const float decay = 1.f - lr * wd;
    const size_t n4 = n / 4;
    float4* p4 = reinterpret_cast<float4*>(p);
    const float4* g4 = reinterpret_cast<const float4*>(g);
    float4* m4 = reinterpret_cast<float4*>(m);
    float4* v4 = reinterpret_cast<float4*>(v);
#define ADAMW_ONE(P, G, M, V)                                 \
    {                                                         \
        const float gg = (G) * coef;                          \
        (M) = b1 * (M) + (1.f - b1) * gg;                     \
        (V) = b2 * (V) + (1.f - b2) * gg * gg;                \
        const float den = sqrtf(V) / bc2_sqrt + eps;          \
        (P) = (P) * decay - step * ((M) / den);               \
    }
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
        float4 pp = p4[i], mm = m4[i], vv = v4[i];
        const float4 gq = g4[i];
        ADAMW_ONE(pp.x, gq.x, mm.x, vv.x)
        ADAMW_ONE(pp.y, gq.y, mm.y, vv.y)
        ADAMW_ONE(pp.z, gq.z, mm.z, vv.z)
        ADAMW_ONE(pp.w, gq.w, mm.w, vv.w)
        p4[i] = pp; m4[i] = mm; v4[i] = vv;
    }
    if (blockIdx.x == 0)
        for (size_t i = n4 * 4 + threadIdx.x; i < n; i += 256) {
            float pp = p[i], mm = m[i], vv = v[i];
            ADAMW_ONE(pp, g[i], mm, vv)
            p[i] = pp; m[i] = mm; v[i] = vv;
        }
}

extern "C" int radet_adamw_step(float* p, const float* g, float* m, float* v, size_t n, float lr, float beta1,
                                float beta2, float eps, float weight_decay, int step, float max_norm, float grad_div,
                                const float* partials, int npartials, float* grad_norm_out, void* stream) {
    if (step < 1 || grad_div <= 0.f) return RADET_ERR_ARG;
    const float bc1 = 1.f - powf(beta1, (float)step);
    const float bc2 = 1.f - powf(beta2, (float)step);
    const size_t n4 = n / 4;
    int blocks = (int)((n4 + 255) / 256);
    if (blocks > 2048) blocks = 2048;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(adamw_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, p, g, m, v, n, lr, beta1, beta2, eps,
                       weight_decay, bc1, sqrtf(bc2), max_norm, grad_div, partials, npartials, grad_norm_out);
    return radet_check_launch();
}

// ---------------------------------------------------------------------------------------------------------------------
// Parameter groups as a run table (RadetOptRun, include/radet_hip.h).  Each block stages the table into LDS once; a
// 16-byte group finds its run in two steps: a binary search for the first element of its WAVE's 256-element span (the
// same address in every lane: broadcast LDS reads, no divergence), then a walk over the runs that begin inside the span --
// none for all but the few spans that hold a boundary.  A group that a boundary cuts resolves each element on its own.
struct RunTable {
    uint32_t begin[RADET_OPT_MAX_RUNS], end[RADET_OPT_MAX_RUNS];
    float lr_mult[RADET_OPT_MAX_RUNS], decay_mult[RADET_OPT_MAX_RUNS];
};

__device__ __forceinline__ void stage_runs(RunTable& t, const RadetOptRun* __restrict__ runs, int nruns) {
    for (int r = threadIdx.x; r < nruns; r += 256) {
        const RadetOptRun u = runs[r];
        t.begin[r] = u.begin; t.end[r] = u.end; t.lr_mult[r] = u.lr_mult; t.decay_mult[r] = u.decay_mult;
    }
    __syncthreads();
}

// the last run that begins at or before element e (indices stay inside [0, nruns) whatever the table holds)
__device__ __forceinline__ int find_run(const RunTable& t, int nruns, uint32_t e) {
    int lo = 0, hi = nruns - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (t.begin[mid] <= e) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ int next_run(const RunTable& t, int nruns, int r, uint32_t e) {
    while (e >= t.end[r] && r + 1 < nruns) ++r;
    return r;
}

// run of the 16-byte group that starts at element e0 (group index i4 = e0 / 4 of a lane-consecutive grid-stride loop)
__device__ __forceinline__ int group_run(const RunTable& t, int nruns, uint32_t e0) {
    const uint32_t span0 = e0 - 4u * (threadIdx.x & 63);
    return next_run(t, nruns, find_run(t, nruns, span0), e0);
}

__global__ __launch_bounds__(256) void adamw_runs_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                         float* __restrict__ m, float* __restrict__ v, size_t n, float lr,
                                                         float b1, float b2, float eps, float wd, float bc1, float bc2_sqrt,
                                                         float max_norm, float grad_div, const float* __restrict__ partials,
                                                         int npartials, float* __restrict__ grad_norm_out,
                                                         const RadetOptRun* __restrict__ runs, int nruns) {
    __shared__ RunTable t;
    stage_runs(t, runs, nruns);
    const float coef = clip_coef(max_norm, grad_div, partials, npartials, grad_norm_out);
    const size_t n4 = n / 4;
    float4* p4 = reinterpret_cast<float4*>(p);
    const float4* g4 = reinterpret_cast<const float4*>(g);
    float4* m4 = reinterpret_cast<float4*>(m);
    float4* v4 = reinterpret_cast<float4*>(v);
#define ADAMW_RUN(R, P, G, M, V)                                              \
    {                                                                         \
        const float lr_r = lr * t.lr_mult[R];                                 \
        const float step = lr_r / bc1;                                        \
        const float decay = 1.f - lr_r * (wd * t.decay_mult[R]);              \
        ADAMW_ONE(P, G, M, V)                                                 \
    }
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
        const uint32_t e0 = (uint32_t)(i * 4);
        int r = group_run(t, nruns, e0);
        float4 pp = p4[i], mm = m4[i], vv = v4[i];
        const float4 gq = g4[i];
        if (e0 + 3 < t.end[r] || r + 1 >= nruns) {          // the whole group lies in run r
            const float lr_r = lr * t.lr_mult[r];
            const float step = lr_r / bc1;
            const float decay = 1.f - lr_r * (wd * t.decay_mult[r]);
            ADAMW_ONE(pp.x, gq.x, mm.x, vv.x)
            ADAMW_ONE(pp.y, gq.y, mm.y, vv.y)
            ADAMW_ONE(pp.z, gq.z, mm.z, vv.z)
            ADAMW_ONE(pp.w, gq.w, mm.w, vv.w)
        } else {                                            // a boundary inside the 16 bytes
            ADAMW_RUN(r, pp.x, gq.x, mm.x, vv.x)
            r = next_run(t, nruns, r, e0 + 1);
            ADAMW_RUN(r, pp.y, gq.y, mm.y, vv.y)
            r = next_run(t, nruns, r, e0 + 2);
            ADAMW_RUN(r, pp.z, gq.z, mm.z, vv.z)
            r = next_run(t, nruns, r, e0 + 3);
            ADAMW_RUN(r, pp.w, gq.w, mm.w, vv.w)
        }
        p4[i] = pp; m4[i] = mm; v4[i] = vv;
    }
    if (blockIdx.x == 0)
        for (size_t i = n4 * 4 + threadIdx.x; i < n; i += 256) {
            const int r = next_run(t, nruns, find_run(t, nruns, (uint32_t)i), (uint32_t)i);
            float pp = p[i], mm = m[i], vv = v[i];
            ADAMW_RUN(r, pp, g[i], mm, vv)
            p[i] = pp; m[i] = mm; v[i] = vv;
        }
#undef ADAMW_RUN
}

static int optim_blocks(size_t n) {
    size_t blocks = (n / 4 + 255) / 256;
    return blocks > 2048 ? 2048 : blocks < 1 ? 1 : (int)blocks;
}

extern "C" int radet_adamw_step_runs(float* p, const float* g, float* m, float* v, size_t n, float lr, float beta1,
                                     float beta2, float eps, float weight_decay, int step, float max_norm, float grad_div,
                                     const float* partials, int npartials, float* grad_norm_out, const RadetOptRun* runs,
                                     int nruns, void* stream) {
    if (step < 1 || grad_div <= 0.f || runs == nullptr || nruns < 1 || nruns > RADET_OPT_MAX_RUNS || n >= ((size_t)1 << 32))
        return RADET_ERR_ARG;
    const float bc1 = 1.f - powf(beta1, (float)step);
    const float bc2 = 1.f - powf(beta2, (float)step);
    hipLaunchKernelGGL(adamw_runs_kernel, dim3(optim_blocks(n)), dim3(256), 0, (hipStream_t)stream, p, g, m, v, n, lr, beta1,
                       beta2, eps, weight_decay, bc1, sqrtf(bc2), max_norm, grad_div, partials, npartials, grad_norm_out, runs,
                       nruns);
    return radet_check_launch();
}

// torch.optim.SGD (torch/optim/sgd.py:_single_tensor_sgd), in its order.  MOM: momentum != 0 (buf exists); nruns == 0: no table.
template <bool MOM>
__global__ __launch_bounds__(256) void sgd_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf,
                                                  size_t n, float lr, float momentum, float dampening, float wd, int nesterov,
                                                  int first, float max_norm, float grad_div,
                                                  const float* __restrict__ partials, int npartials,
                                                  float* __restrict__ grad_norm_out, const RadetOptRun* __restrict__ runs,
                                                  int nruns) {
    __shared__ RunTable t;
    if (nruns > 0) stage_runs(t, runs, nruns);
    const float coef = clip_coef(max_norm, grad_div, partials, npartials, grad_norm_out);
    const float keep = 1.f - dampening;
    const size_t n4 = n / 4;
    float4* p4 = reinterpret_cast<float4*>(p);
    const float4* g4 = reinterpret_cast<const float4*>(g);
    float4* b4 = reinterpret_cast<float4*>(buf);
#define SGD_ONE(P, G, B, LR, WD)                                              \
    {                                                                         \
        float d = (G) * coef + (WD) * (P);                                    \
        if (MOM) {                                                            \
            (B) = first ? d : momentum * (B) + keep * d;                      \
            d = nesterov ? d + momentum * (B) : (B);                          \
        }                                                                     \
        (P) = (P) - (LR) * d;                                                 \
    }
#define SGD_RUN(R, P, G, B) SGD_ONE(P, G, B, lr * t.lr_mult[R], wd * t.decay_mult[R])
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
        const uint32_t e0 = (uint32_t)(i * 4);
        int r = nruns > 0 ? group_run(t, nruns, e0) : 0;
        float4 pp = p4[i], bb = make_float4(0.f, 0.f, 0.f, 0.f);
        const float4 gq = g4[i];
        if (MOM) bb = b4[i];
        if (nruns == 0 || e0 + 3 < t.end[r] || r + 1 >= nruns) {
            const float lr_r = nruns > 0 ? lr * t.lr_mult[r] : lr;
            const float wd_r = nruns > 0 ? wd * t.decay_mult[r] : wd;
            SGD_ONE(pp.x, gq.x, bb.x, lr_r, wd_r)
            SGD_ONE(pp.y, gq.y, bb.y, lr_r, wd_r)
            SGD_ONE(pp.z, gq.z, bb.z, lr_r, wd_r)
            SGD_ONE(pp.w, gq.w, bb.w, lr_r, wd_r)
        } else {
            SGD_RUN(r, pp.x, gq.x, bb.x)
            r = next_run(t, nruns, r, e0 + 1);
            SGD_RUN(r, pp.y, gq.y, bb.y)
            r = next_run(t, nruns, r, e0 + 2);
            SGD_RUN(r, pp.z, gq.z, bb.z)
            r = next_run(t, nruns, r, e0 + 3);
            SGD_RUN(r, pp.w, gq.w, bb.w)
        }
        p4[i] = pp;
        if (MOM) b4[i] = bb;
    }
    if (blockIdx.x == 0)
        for (size_t i = n4 * 4 + threadIdx.x; i < n; i += 256) {
            float pp = p[i], bb = MOM ? buf[i] : 0.f;
            if (nruns > 0) {
                const int r = next_run(t, nruns, find_run(t, nruns, (uint32_t)i), (uint32_t)i);
                SGD_RUN(r, pp, g[i], bb)
            } else {
                SGD_ONE(pp, g[i], bb, lr, wd)
            }
            p[i] = pp;
            if (MOM) buf[i] = bb;
        }
#undef SGD_RUN
#undef SGD_ONE
}

extern "C" int radet_sgd_step(float* p, const float* g, float* buf, size_t n, float lr, float momentum, float dampening,
                              float weight_decay, int nesterov, int step, float max_norm, float grad_div, const float* partials,
                              int npartials, float* grad_norm_out, const RadetOptRun* runs, int nruns, void* stream) {
    if (step < 1 || grad_div <= 0.f || n >= ((size_t)1 << 32)) return RADET_ERR_ARG;
    if ((runs == nullptr) != (nruns == 0) || nruns < 0 || nruns > RADET_OPT_MAX_RUNS) return RADET_ERR_ARG;
    if (nesterov && (dampening != 0.f || momentum == 0.f)) return RADET_ERR_ARG;
    if (momentum != 0.f && buf == nullptr) return RADET_ERR_ARG;
    auto kernel = momentum != 0.f ? sgd_kernel<true> : sgd_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3(optim_blocks(n)), dim3(256), 0, (hipStream_t)stream, p, g, buf, n, lr, momentum, dampening,
                       weight_decay, nesterov, (int)(step == 1), max_norm, grad_div, partials, npartials, grad_norm_out, runs,
                       nruns);
    return radet_check_launch();
}

// MODE 0: acc = g;  1: acc += g;  2: g = acc + g
template <int MODE>
__global__ __launch_bounds__(256) void grad_accumulate_kernel(float* __restrict__ acc, float* __restrict__ g, size_t n) {
    const size_t n4 = n / 4;
    float4* a4 = reinterpret_cast<float4*>(acc);
    float4* g4 = reinterpret_cast<float4*>(g);
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
        const float4 y = g4[i];
        if (MODE == 0) {
            a4[i] = y;
        } else {
            const float4 x = a4[i];
            const float4 s = make_float4(x.x + y.x, x.y + y.y, x.z + y.z, x.w + y.w);
            if (MODE == 1) a4[i] = s; else g4[i] = s;
        }
    }
    if (blockIdx.x == 0)
        for (size_t i = n4 * 4 + threadIdx.x; i < n; i += 256) {
            if (MODE == 0) acc[i] = g[i];
            else if (MODE == 1) acc[i] = acc[i] + g[i];
            else g[i] = acc[i] + g[i];
        }
}

extern "C" int radet_grad_accumulate(float* acc, float* g, size_t n, int mode, void* stream) {
    if (mode < 0 || mode > 2) return RADET_ERR_ARG;
    auto kernel = mode == 0 ? grad_accumulate_kernel<0> : mode == 1 ? grad_accumulate_kernel<1> : grad_accumulate_kernel<2>;
    hipLaunchKernelGGL(kernel, dim3(optim_blocks(n)), dim3(256), 0, (hipStream_t)stream, acc, g, n);
    return radet_check_launch();
}

// ---------------------------------------------------------------------------------------------------------------------
// Weight EMA over the trainable arena (mmcv's EMAHook: ema.mul_(1 - m).add_(param, alpha=m)) and the exchange of two arenas.
// torch's CPU ops round twice: t = fl(ema * (1 - m)), then ONE fused multiply-add fl(m * p + t); the intrinsics pin exactly
// that whatever -ffp-contract says.  Both kernels are shaped like grad_accumulate_kernel -- 16-byte accesses, a grid-stride
// loop -- but take any base pointer a float may have: the host peels `head` elements so that the 16-byte body is aligned
// (both pointers share their offset inside a 16-byte line), or makes everything head when they do not.  The peeled head
// and the tail behind the last whole group are spread over the whole grid, one element per thread and trip.
__device__ __forceinline__ float ema_one(float e, float p, float m, float om) { return __fmaf_rn(m, p, __fmul_rn(e, om)); }

__global__ __launch_bounds__(256) void ema_update_kernel(float* __restrict__ ema, const float* __restrict__ p, size_t n,
                                                         size_t head, float m, float om) {
    const size_t n4 = (n - head) / 4;
    float4* e4 = reinterpret_cast<float4*>(ema + head);
    const float4* p4 = reinterpret_cast<const float4*>(p + head);
    const size_t tid = (size_t)blockIdx.x * 256 + threadIdx.x, stride = (size_t)gridDim.x * 256;
    for (size_t i = tid; i < n4; i += stride) {
        float4 e = e4[i];
        const float4 q = p4[i];
        e.x = ema_one(e.x, q.x, m, om); e.y = ema_one(e.y, q.y, m, om);
        e.z = ema_one(e.z, q.z, m, om); e.w = ema_one(e.w, q.w, m, om);
        e4[i] = e;
    }
    const size_t body_end = head + n4 * 4, rest = n - n4 * 4;       // scalar elements: [0, head) and [body_end, n)
    for (size_t k = tid; k < rest; k += stride) {
        const size_t i = k < head ? k : body_end + (k - head);
        ema[i] = ema_one(ema[i], p[i], m, om);
    }
}

__global__ __launch_bounds__(256) void ema_swap_kernel(float* __restrict__ a, float* __restrict__ b, size_t n, size_t head) {
    const size_t n4 = (n - head) / 4;
    float4* a4 = reinterpret_cast<float4*>(a + head);
    float4* b4 = reinterpret_cast<float4*>(b + head);
    const size_t tid = (size_t)blockIdx.x * 256 + threadIdx.x, stride = (size_t)gridDim.x * 256;
    for (size_t i = tid; i < n4; i += stride) {
        const float4 x = a4[i], y = b4[i];
        a4[i] = y; b4[i] = x;
    }
    const size_t body_end = head + n4 * 4, rest = n - n4 * 4;
    for (size_t k = tid; k < rest; k += stride) {
        const size_t i = k < head ? k : body_end + (k - head);
        const float x = a[i], y = b[i];
        a[i] = y; b[i] = x;
    }
}

// elements to peel in front of the 16-byte body of two float arrays: 0-3 when they share their offset inside a 16-byte
// line, n (no body: the scalar path) when they do not
static size_t ema_head(const void* a, const void* b, size_t n) {
    const uintptr_t ua = (uintptr_t)a, ub = (uintptr_t)b;
    if ((ua & 15) != (ub & 15)) return n;
    const size_t head = ((16 - (ua & 15)) & 15) / 4;
    return head < n ? head : n;
}

static bool ema_bad_pair(const void* a, const void* b, size_t n) {
    const uintptr_t ua = (uintptr_t)a, ub = (uintptr_t)b;
    if (a == nullptr || b == nullptr || ((ua | ub) & 3)) return true;
    return ua < ub ? ub - ua < 4 * n : ua - ub < 4 * n;             // (the kernels' __restrict__: the arrays are disjoint)
}

extern "C" int radet_ema_update(float* ema, const float* p, size_t n, float momentum, float one_minus, void* stream) {
    if (n == 0) return RADET_OK;
    if (ema_bad_pair(ema, p, n)) return RADET_ERR_ARG;
    hipLaunchKernelGGL(ema_update_kernel, dim3(optim_blocks(n)), dim3(256), 0, (hipStream_t)stream, ema, p, n,
                       ema_head(ema, p, n), momentum, one_minus);
    return radet_check_launch();
}

extern "C" int radet_ema_swap(float* a, float* b, size_t n, void* stream) {
    if (n == 0) return RADET_OK;
    if (ema_bad_pair(a, b, n)) return RADET_ERR_ARG;
    hipLaunchKernelGGL(ema_swap_kernel, dim3(optim_blocks(n)), dim3(256), 0, (hipStream_t)stream, a, b, n, ema_head(a, b, n));
    return radet_check_launch();
}
