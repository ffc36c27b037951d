// Soft-NMS (mmcv.ops.batched_nms with nms.type = 'soft_nms', reached from radet_head.py:159-163): sequential,
// score-dependent picks with naive / linear / gaussian score decay.  gfx950 / CDNA4 only.
//
//  soft_nms_kernel : one workgroup (1024 threads) per image runs the GLOBAL loop over all classes on the class-offset
//                    boxes, i.e. the literal order of mmcv's softnms_cpu: no sort, no label segments, no merge.
//                    Cross-class IoU on offset boxes is exactly 0, so other classes only see a multiply by 1.0f.
//    per pick: block-wide argmax on the 64-bit key (order-preserving score bits, ~index) = highest score, lowest input
//    index: 6 wave shuffles, one LDS exchange of 16 keys, ONE barrier (the exchange slots alternate between rounds);
//    every lane then decays and prunes its own boxes against the picked box.  Picks are staged in LDS (index, score) and
//    written out 1024 at a time, so the register-resident loop holds no global memory access at all: a barrier waits
//    for a wave's outstanding stores, which would put the output rows on every round's critical path.
//    n <= SOFT_NMS_REG_CAP (8192 = 1024 lanes x SOFT_NMS_KREG 8): boxes, scores and alive bits live in registers, the
//    picked box is a broadcast read of the offset boxes staged in LDS (16 B per box, <= 128 KiB).
//    n >  SOFT_NMS_REG_CAP: the same loop through the caller's workspace (offset boxes, scores, alive flags: 24 B per
//    candidate), same results.
//  A pick loop ends after min(max_out, n) picks or when nothing is left: the detector path (max_per_img = 100) runs at
//  most 100 rounds whatever the candidate count.
//
// Arithmetic: fp32, unfused (-ffp-contract=off for the whole library); the gaussian weight is exp in DOUBLE of the fp32
// argument, rounded once to fp32.  A NaN IoU (two zero-area boxes) gives weight 1 under every method.  Candidates with a
// NaN score are never picked.
#include "common.h"
#include "radet_hip.h"

#define SOFT_NMS_THREADS 1024
#define SOFT_NMS_KREG 8
#define SOFT_NMS_REG_CAP (SOFT_NMS_THREADS * SOFT_NMS_KREG)
#define SOFT_NMS_MAX_CAP 65536
#define SOFT_NMS_PICKBUF 1024   // picks staged in LDS between two flushes to the outputs

// (score, index) -> key whose unsigned maximum is the highest score, ties to the lowest index; 0 = no candidate
__device__ __forceinline__ unsigned long long snms_key(float s, int idx) {
    unsigned u = __float_as_uint(s + 0.0f);                 // -0 -> +0: equal scores, equal bits
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ((unsigned long long)u << 32) | (unsigned long long)(~(unsigned)idx);
}

__device__ __forceinline__ unsigned long long snms_wave_max(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long w = __shfl_xor(v, o, 64);
        v = w > v ? w : v;
    }
    return v;
}

// block-wide maximum of the lanes' keys; `par` alternates between rounds so that one barrier per round is enough
__device__ __forceinline__ unsigned long long snms_block_max(unsigned long long key, unsigned long long (*s_red)[16],
                                                             int par, int lane, int wave) {
    key = snms_wave_max(key);
    if (lane == 0) s_red[par][wave] = key;
    __syncthreads();
    unsigned long long best = s_red[par][0];
#pragma unroll
    for (int w = 1; w < SOFT_NMS_THREADS / 64; ++w) {
        const unsigned long long k = s_red[par][w];
        best = k > best ? k : best;
    }
    return best;
}

// picks [base, base + cnt) (cnt <= SOFT_NMS_PICKBUF) from the LDS stage to the outputs, one lane each; between barriers
__device__ __forceinline__ void snms_flush(const int* s_pidx, const float* s_psc, int base, int cnt, int tid,
                                           const float4* bsrc, const int64_t* lsrc, float* ob, float* os, int64_t* ol,
                                           int64_t* ok) {
    if (tid < cnt) {
        const int pi = s_pidx[tid];
        *reinterpret_cast<float4*>(ob + (size_t)(base + tid) * 4) = bsrc[pi];
        os[base + tid] = s_psc[tid];
        ol[base + tid] = lsrc[pi];
        ok[base + tid] = pi;
    }
}

// decayed score of box p after box i was picked (softnms_cpu's inner loop with offset 0)
__device__ __forceinline__ float snms_decay(float s, const float4 bi, float area_i, const float4 bp, int method, float thr,
                                            float sigma) {
    const float xx1 = fmaxf(bi.x, bp.x), yy1 = fmaxf(bi.y, bp.y);
    const float xx2 = fminf(bi.z, bp.z), yy2 = fminf(bi.w, bp.w);
    const float w = fmaxf(0.f, xx2 - xx1), h = fmaxf(0.f, yy2 - yy1);
    const float inter = w * h;
    // no intersection (every box of another class, most of the same): ovr is +-0 or NaN, the weight exactly 1 unless a
    // threshold <= 0 makes 0 >= thr hold -- skip the division, s * 1.0f == s
    if (inter == 0.f && (method == RADET_SOFT_NMS_GAUSSIAN || thr > 0.f)) return s;
    const float area_p = (bp.z - bp.x) * (bp.w - bp.y);
    const float ovr = inter / (area_i + area_p - inter);
    float weight = 1.0f;
    if (method == RADET_SOFT_NMS_GAUSSIAN) {
        if (ovr == ovr && ovr != 0.f) weight = (float)exp((double)(-(ovr * ovr) / sigma));   // exp(-0) is exactly 1
    } else if (ovr >= thr) {
        weight = method == RADET_SOFT_NMS_LINEAR ? 1.0f - ovr : 0.0f;
    }
    return s * weight;
}

__global__ __launch_bounds__(SOFT_NMS_THREADS) void soft_nms_kernel(
    const float* __restrict__ boxes, const float* __restrict__ scores, const int64_t* __restrict__ labels,
    const int* __restrict__ counts, int cap, int method, float thr, float sigma, float min_score, int class_agnostic,
    int max_out, float* __restrict__ out_boxes, float* __restrict__ out_scores, int64_t* __restrict__ out_labels,
    int64_t* __restrict__ out_keep, int* __restrict__ out_count, char* __restrict__ ws_all, size_t ws_per_image) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float4* lbox = reinterpret_cast<float4*>(smem);              // [min(cap, SOFT_NMS_REG_CAP)] offset boxes
    __shared__ unsigned long long s_red[2][16];
    __shared__ float s_mx[16];
    __shared__ int s_pidx[SOFT_NMS_PICKBUF];
    __shared__ float s_psc[SOFT_NMS_PICKBUF];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int n = counts[b];
    n = n < 0 ? 0 : (n > cap ? cap : n);
    const float4* bsrc = reinterpret_cast<const float4*>(boxes) + (size_t)b * cap;
    const float* ssrc = scores + (size_t)b * cap;
    const int64_t* lsrc = labels + (size_t)b * cap;
    float* ob = out_boxes + (size_t)b * max_out * 4;
    float* os = out_scores + (size_t)b * max_out;
    int64_t* ol = out_labels + (size_t)b * max_out;
    int64_t* ok = out_keep + (size_t)b * max_out;

    // class offset = label * (largest coordinate of the valid candidates + 1), as mode 3 of radet_nms
    float unit = 0.f;
    if (!class_agnostic) {
        float mx = -INFINITY;
        for (int i = tid; i < n * 4; i += SOFT_NMS_THREADS) mx = fmaxf(mx, boxes[(size_t)b * cap * 4 + i]);
        mx = wave_max(mx);
        if (lane == 0) s_mx[wave] = mx;
        __syncthreads();
        mx = s_mx[0];
#pragma unroll
        for (int i = 1; i < 16; ++i) mx = fmaxf(mx, s_mx[i]);
        unit = mx + 1.0f;
    }
    const int lim = max_out < n ? max_out : n;
    int picks = 0, par = 0;

    if (n <= SOFT_NMS_REG_CAP) {
        // ---- register-resident: lane tid holds the boxes k * 1024 + tid
        float4 X[SOFT_NMS_KREG];
        float S[SOFT_NMS_KREG];
        unsigned alive = 0;
        const int kmax = (n + SOFT_NMS_THREADS - 1) / SOFT_NMS_THREADS;   // uniform
#pragma unroll
        for (int k = 0; k < SOFT_NMS_KREG; ++k) {
            const int i = k * SOFT_NMS_THREADS + tid;
            X[k] = make_float4(0.f, 0.f, 0.f, 0.f);
            S[k] = 0.f;
            if (i < n) {
                const float4 bb = bsrc[i];
                const float off = class_agnostic ? 0.f : (float)(int)lsrc[i] * unit;
                X[k] = make_float4(bb.x + off, bb.y + off, bb.z + off, bb.w + off);
                S[k] = ssrc[i];
                if (S[k] == S[k]) alive |= 1u << k;
                lbox[i] = X[k];
            }
        }
        __syncthreads();
        while (picks < lim) {
            unsigned long long key = 0;
#pragma unroll
            for (int k = 0; k < SOFT_NMS_KREG; ++k)
                if (k < kmax && ((alive >> k) & 1u)) {
                    const unsigned long long c = snms_key(S[k], k * SOFT_NMS_THREADS + tid);
                    key = c > key ? c : key;
                }
            const unsigned long long best = snms_block_max(key, s_red, par, lane, wave);
            par ^= 1;
            if (best == 0) break;                                         // uniform: nothing left
            const int pi = __builtin_amdgcn_readfirstlane((int)~(unsigned)(best & 0xFFFFFFFFull));
            const int pk = pi / SOFT_NMS_THREADS;
            const float4 bi = lbox[pi];
            const float area_i = (bi.z - bi.x) * (bi.w - bi.y);
            if (tid == (pi & (SOFT_NMS_THREADS - 1))) {
                float sp = S[0];
#pragma unroll
                for (int k = 1; k < SOFT_NMS_KREG; ++k)
                    if (k == pk) sp = S[k];
                alive &= ~(1u << pk);
                s_pidx[picks & (SOFT_NMS_PICKBUF - 1)] = pi;
                s_psc[picks & (SOFT_NMS_PICKBUF - 1)] = sp;
            }
#pragma unroll
            for (int k = 0; k < SOFT_NMS_KREG; ++k)
                if (k < kmax && ((alive >> k) & 1u)) {
                    S[k] = snms_decay(S[k], bi, area_i, X[k], method, thr, sigma);
                    if (S[k] < min_score) alive &= ~(1u << k);
                }
            ++picks;
            if ((picks & (SOFT_NMS_PICKBUF - 1)) == 0) {                  // uniform: the stage is full
                __syncthreads();
                snms_flush(s_pidx, s_psc, picks - SOFT_NMS_PICKBUF, SOFT_NMS_PICKBUF, tid, bsrc, lsrc, ob, os, ol, ok);
                __syncthreads();
            }
        }
    } else {
        // ---- general pass through the workspace: lane tid owns the boxes i = tid (mod 1024)
        char* w = ws_all + (size_t)b * ws_per_image;
        float4* gbox = reinterpret_cast<float4*>(w);
        float* gs = reinterpret_cast<float*>(w + (size_t)cap * 16);
        int* galive = reinterpret_cast<int*>(w + (size_t)cap * 20);
        for (int i = tid; i < n; i += SOFT_NMS_THREADS) {
            const float4 bb = bsrc[i];
            const float off = class_agnostic ? 0.f : (float)(int)lsrc[i] * unit;
            gbox[i] = make_float4(bb.x + off, bb.y + off, bb.z + off, bb.w + off);
            const float s = ssrc[i];
            gs[i] = s;
            galive[i] = s == s;
        }
        __threadfence_block();
        __syncthreads();
        while (picks < lim) {
            unsigned long long key = 0;
            for (int i = tid; i < n; i += SOFT_NMS_THREADS)
                if (galive[i]) {
                    const unsigned long long c = snms_key(gs[i], i);
                    key = c > key ? c : key;
                }
            const unsigned long long best = snms_block_max(key, s_red, par, lane, wave);
            par ^= 1;
            if (best == 0) break;
            const int pi = __builtin_amdgcn_readfirstlane((int)~(unsigned)(best & 0xFFFFFFFFull));
            const float4 bi = gbox[pi];
            const float area_i = (bi.z - bi.x) * (bi.w - bi.y);
            if (tid == (pi & (SOFT_NMS_THREADS - 1))) {
                galive[pi] = 0;
                s_pidx[picks & (SOFT_NMS_PICKBUF - 1)] = pi;
                s_psc[picks & (SOFT_NMS_PICKBUF - 1)] = gs[pi];
            }
            for (int i = tid; i < n; i += SOFT_NMS_THREADS)
                if (galive[i]) {
                    const float s = snms_decay(gs[i], bi, area_i, gbox[i], method, thr, sigma);
                    gs[i] = s;
                    if (s < min_score) galive[i] = 0;
                }
            ++picks;
            if ((picks & (SOFT_NMS_PICKBUF - 1)) == 0) {                  // uniform: the stage is full
                __syncthreads();
                snms_flush(s_pidx, s_psc, picks - SOFT_NMS_PICKBUF, SOFT_NMS_PICKBUF, tid, bsrc, lsrc, ob, os, ol, ok);
                __syncthreads();
            }
        }
    }
    __syncthreads();
    snms_flush(s_pidx, s_psc, picks & ~(SOFT_NMS_PICKBUF - 1), picks & (SOFT_NMS_PICKBUF - 1), tid, bsrc, lsrc, ob, os, ol, ok);
    if (tid == 0) out_count[b] = picks;
}

static size_t soft_nms_ws_per_image(int cap) { return ((size_t)cap * 24 + 255) / 256 * 256; }

extern "C" size_t radet_soft_nms_ws_bytes(int B, int cap) {
    if (B < 1 || cap < 1) return 0;
    return (size_t)B * soft_nms_ws_per_image(cap);
}

extern "C" int radet_soft_nms(const float* boxes, const float* scores, const int64_t* labels, const int* counts, int B,
                              int cap, int method, float iou_thr, float sigma, float min_score, int class_agnostic,
                              int max_out, float* out_boxes, float* out_scores, int64_t* out_labels, int64_t* out_keep,
                              int* out_count, void* ws, void* stream) {
    if (B < 1 || cap < 1 || cap > SOFT_NMS_MAX_CAP || max_out <= 0) return RADET_ERR_ARG;
    if (method != RADET_SOFT_NMS_NAIVE && method != RADET_SOFT_NMS_LINEAR && method != RADET_SOFT_NMS_GAUSSIAN)
        return RADET_ERR_ARG;
    if (method == RADET_SOFT_NMS_GAUSSIAN && !(sigma > 0.f)) return RADET_ERR_ARG;
    const size_t smem = (size_t)(cap < SOFT_NMS_REG_CAP ? cap : SOFT_NMS_REG_CAP) * 16;
    static bool attr_set = false;
    if (!attr_set) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(soft_nms_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                SOFT_NMS_REG_CAP * 16) != hipSuccess)
            return RADET_ERR_LAUNCH;
        attr_set = true;
    }
    hipLaunchKernelGGL(soft_nms_kernel, dim3(B), dim3(SOFT_NMS_THREADS), smem, (hipStream_t)stream, boxes, scores, labels,
                       counts, cap, method, iou_thr, sigma, min_score, class_agnostic, max_out, out_boxes, out_scores,
                       out_labels, out_keep, out_count, (char*)ws, soft_nms_ws_per_image(cap));
    return radet_check_launch();
}
