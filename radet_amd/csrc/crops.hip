// Detections -> a packed batch of RoI crops for a downstream pose network, with no host round trip: the NMS outputs
// (boxes [B,K,4], scores [B,K], counts [B], as radet_nms / radet_soft_nms leave them) and the frames of the batch (the
// PREP_DESC_INTS rows of radet_preprocess_frames: mixed sizes, views into larger device tensors) are on the device when NMS
// finishes; two launches turn them into [cap, ...] crops of one fixed size.
//
//   radet_crop_plan    one workgroup: validity, ordered compaction, one window of the output's aspect ratio per kept
//                      detection (CROP_ROW_INTS ints), the counters {n_out, n_total, where each frame's rows end}
//   radet_crop_frames  grid (pixel tiles / CROP_TILES, cap): a block whose slot is at or beyond n_out (read from device
//                      memory) exits before any other load or store; otherwise "paste the frame on a filled canvas, slice
//                      the window, resize to Ho x Wo" with the view arithmetic of resize_u8_kernel (pixel_ops.h: lin_taps_u8
//                      with the edge clamp at the window's border, lin_blend_u8), every tap read from the frame in place or
//                      the fill colour, then either norm_store (f32 NCHW) or the raw BGR bytes (u8 NHWC)
//
// The window rule is fp32 with one rounding per operation (the explicit _rn intrinsics below; the file is also built with
// contraction off), so a NumPy float32 restatement agrees to the bit.  Memory-bound like preprocess_frames_kernel: 12 source
// bytes per output pixel (mostly shared with the neighbouring lanes), 12 or 3 bytes stored.  No LDS in the pixel kernel, no
// scratch.
#include "common.h"
#include "pixel_ops.h"
#include "radet_hip.h"

#define CROP_GLOBAL __attribute__((address_space(1)))

#define CROP_TILES 4                  // 256-pixel tiles per block of the pixel kernel

struct CropWindow { int wx0, wy0, ww, wh; };

// a side in pixels: ceil, clamped to [1, CROP_MAX_SIDE] (the comparison first: an infinite side never reaches the cast)
__device__ __forceinline__ int crop_side(float s) {
    if (!(s < (float)CROP_MAX_SIDE)) return CROP_MAX_SIDE;
    const int v = (int)ceilf(s);
    return v < 1 ? 1 : v;
}

__device__ __forceinline__ bool crop_window(float x1, float y1, float x2, float y2, float score, float a, float scale,
                                            float score_thr, CropWindow* o) {
    if (!(isfinite(x1) && isfinite(y1) && isfinite(x2) && isfinite(y2))) return false;
    const float w = __fsub_rn(x2, x1), h = __fsub_rn(y2, y1);
    const float cx = __fmul_rn(__fadd_rn(x1, x2), 0.5f), cy = __fmul_rn(__fadd_rn(y1, y2), 0.5f);
    if (!(w > 0.f && h > 0.f && fabsf(cx) < 1048576.f && fabsf(cy) < 1048576.f && score >= score_thr)) return false;
    const float hs = __fmul_rn(fmaxf(h, __fdiv_rn(w, a)), scale), ws = __fmul_rn(hs, a);
    o->wh = crop_side(hs);
    o->ww = crop_side(ws);
    o->wx0 = (int)floorf(__fsub_rn(cx, __fmul_rn(0.5f, (float)o->ww)));
    o->wy0 = (int)floorf(__fsub_rn(cy, __fmul_rn(0.5f, (float)o->wh)));
    return true;
}

// Ordered stream compaction by one workgroup, as threshold_compact_kernel (boxops.hip): ballot prefix inside a wavefront of
// 64 lanes, running offsets across the 16 wavefronts, no atomics -- so the rows come out image-major, then by rank.
__global__ __launch_bounds__(1024) void crop_plan_kernel(const float* __restrict__ boxes, const float* __restrict__ scores,
                                                         const int* __restrict__ counts, int B, int K, float a, float scale,
                                                         float score_thr, int cap, int* __restrict__ rows,
                                                         int* __restrict__ counters) {
    __shared__ int wcnt[16];
    __shared__ int base_s;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int n = B * K;                                        // (< 2^31: checked by the host)
    if (tid == 0) base_s = 0;
    __syncthreads();
    for (int c0 = 0; c0 < n; c0 += 1024) {
        const int i = c0 + tid;
        bool sel = false;
        int b = 0, j = 0;
        CropWindow win = {0, 0, 1, 1};
        if (i < n && i >= 0) {
            b = i / K;
            j = i - b * K;
            if (j < counts[b]) {
                const float4 bx = reinterpret_cast<const float4*>(boxes)[i];
                sel = crop_window(bx.x, bx.y, bx.z, bx.w, scores[i], a, scale, score_thr, &win);
            }
        }
        const unsigned long long m = __ballot(sel);
        if (lane == 0) wcnt[wv] = __popcll(m);
        __syncthreads();
        int off = base_s;
        for (int k = 0; k < wv; ++k) off += wcnt[k];
        off += __popcll(m & ((1ull << lane) - 1ull));
        if (sel && off < cap) {
            int* r = rows + (size_t)off * CROP_ROW_INTS;
            r[0] = b; r[1] = j; r[2] = win.wx0; r[3] = win.wy0; r[4] = win.ww; r[5] = win.wh;
        }
        __syncthreads();
        if (tid == 0) {
            int t = 0;
            for (int k = 0; k < 16; ++k) t += wcnt[k];
            base_s += t;
        }
        __syncthreads();
    }
    const int n_out = base_s < cap ? base_s : cap;
    if (tid == 0) {
        counters[0] = n_out;
        counters[1] = base_s;
    }
    // counters[2 + b] = the number of kept rows of the frames 0 .. b: the rows are image-major, so frame b's are
    // [counters[1 + b] (0 for b == 0), counters[2 + b]) and a host that has the counters splits the batch without reading a
    // row.  The rows are this workgroup's own stores, ordered before these loads by the barrier that ends the loop.
    for (int b = tid; b < B; b += 1024) {
        int lo = 0, hi = n_out;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (rows[(size_t)mid * CROP_ROW_INTS] <= b) lo = mid + 1; else hi = mid;
        }
        counters[2 + b] = lo;
    }
}

// F32: out f32 [cap,3,Ho,Wo] through norm_store; else out u8 [cap,Ho,Wo,3], the blended BGR bytes.  PACK (u8 only, Ho * Wo a
// multiple of 4 so that every slot and every group of four pixels starts on a dword): the four lanes of a group hold 12
// consecutive bytes, which three of them store as dwords -- 48 contiguous dwords per wavefront instead of 192 byte stores.
template <bool F32, bool PACK>
__global__ __launch_bounds__(256) void crop_frames_kernel(const int* __restrict__ rows, const int* __restrict__ counters,
                                                          const int* __restrict__ desc, int B, void* __restrict__ out, int Ho,
                                                          int Wo, int to_rgb, unsigned fill, float m0, float m1, float m2,
                                                          float s0, float s1, float s2) {
    const int n = blockIdx.y;
    if (n >= counters[0]) return;                               // slots at or beyond n_out: nothing is loaded or stored
    const int plane = Ho * Wo;
    const int* r = rows + (size_t)n * CROP_ROW_INTS;
    const int b = r[0], wx0 = r[2], wy0 = r[3], ww = r[4], wh = r[5];
    // (rows a caller made up: nothing outside the descriptor table or beyond the int range is touched)
    if ((unsigned)b >= (unsigned)B || ww < 1 || wh < 1 || ww > CROP_MAX_SIDE || wh > CROP_MAX_SIDE ||
        wx0 < -(1 << 30) || wx0 > (1 << 30) || wy0 < -(1 << 30) || wy0 > (1 << 30))
        return;
    const int* d = desc + (size_t)PREP_DESC_INTS * b;
    const CROP_GLOBAL uint8_t* src = (const CROP_GLOBAL uint8_t*)(((uint64_t)(uint32_t)d[1] << 32) | (uint64_t)(uint32_t)d[0]);
    const size_t stride = (size_t)(uint32_t)d[2];
    const int sh = d[3] > 0 ? d[3] : 0, sw = d[4] > 0 ? d[4] : 0;
    // CROP_TILES tiles of 256 pixels per block, one pixel per thread and trip: a quarter of the blocks (what a slot beyond
    // n_out costs is its blocks' launch) and four independent pixels' loads per thread for the compiler to overlap
#pragma unroll
    for (int it = 0; it < CROP_TILES; ++it) {
        const int p = (blockIdx.x * CROP_TILES + it) * 256 + threadIdx.x;
        if (p >= plane) return;
        const int y = p / Wo, x = p - y * Wo;
        const LinTaps t = lin_taps_u8(y, x, wh, ww, Ho, Wo);
        const int y0 = wy0 + t.y0, y1 = wy0 + t.y1, x0 = wx0 + t.sx, x1 = wx0 + t.x1;
        const bool iy0 = (unsigned)y0 < (unsigned)sh, iy1 = (unsigned)y1 < (unsigned)sh;
        const bool ix0 = (unsigned)x0 < (unsigned)sw, ix1 = (unsigned)x1 < (unsigned)sw;
        const CROP_GLOBAL uint8_t* r0 = src + (size_t)(iy0 ? y0 : 0) * stride;
        const CROP_GLOBAL uint8_t* r1 = src + (size_t)(iy1 ? y1 : 0) * stride;
        const size_t c0 = (size_t)(ix0 ? x0 : 0) * 3, c1 = (size_t)(ix1 ? x1 : 0) * 3;
        int v[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int f = (int)((fill >> (8 * c)) & 0xFFu);
            const int p00 = iy0 && ix0 ? r0[c0 + c] : f, p01 = iy0 && ix1 ? r0[c1 + c] : f;
            const int p10 = iy1 && ix0 ? r1[c0 + c] : f, p11 = iy1 && ix1 ? r1[c1 + c] : f;
            v[c] = lin_blend_u8(p00, p01, p10, p11, t);
        }
        if (F32) {
            norm_store((float*)out + (size_t)n * 3 * plane + p, (size_t)plane, v, to_rgb != 0, m0, m1, m2, s0, s1, s2);
        } else if (PACK) {
            // bytes of the group: p0 p0 p0 p1 | p1 p1 p2 p2 | p2 p3 p3 p3; lane k < 3 stores dword k, from its pixel and the next
            const unsigned px = (unsigned)v[0] | (unsigned)v[1] << 8 | (unsigned)v[2] << 16;
            const unsigned nx = (unsigned)__shfl_down((int)px, 1, 64);
            const int k = p & 3;
            if (k < 3) ((unsigned*)out)[((size_t)n * plane + (p - k)) * 3 / 4 + k] = (px >> (8 * k)) | (nx << (24 - 8 * k));
        } else {
            uint8_t* o = (uint8_t*)out + ((size_t)n * plane + p) * 3;
            o[0] = (uint8_t)v[0]; o[1] = (uint8_t)v[1]; o[2] = (uint8_t)v[2];
        }
    }
}

extern "C" int radet_crop_plan(const float* boxes, const float* scores, const int* counts, int B, int K, int Ho, int Wo,
                               float scale, float score_thr, int cap, int* rows, int* counters, void* stream) {
    if (B < 0 || K < 0 || cap < 0 || cap > 65535 || Ho < 1 || Ho > 4096 || Wo < 1 || Wo > 4096) return RADET_ERR_ARG;
    if (!(scale > 0.f) || !std::isfinite(scale) || (long long)B * K >= 0x80000000ll) return RADET_ERR_ARG;
    if (B == 0 || cap == 0) return RADET_OK;
    if (K == 0 || !boxes || !scores || !counts || !rows || !counters || ((uintptr_t)boxes & 15)) return RADET_ERR_ARG;
    hipLaunchKernelGGL(crop_plan_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, boxes, scores, counts, B, K,
                       (float)Wo / (float)Ho, scale, score_thr, cap, rows, counters);
    return radet_check_launch();
}

extern "C" int radet_crop_frames(const int* rows, const int* counters, const int* desc, int B, int cap, int Ho, int Wo, int flags,
                                 unsigned fill, float m0, float m1, float m2, float s0, float s1, float s2, void* out,
                                 void* stream) {
    if (B < 0 || cap < 0 || cap > 65535 || Ho < 1 || Ho > 4096 || Wo < 1 || Wo > 4096 || (flags & ~(CROP_TO_RGB | CROP_F32)))
        return RADET_ERR_ARG;
    if (B == 0 || cap == 0) return RADET_OK;
    if (!rows || !counters || !desc || !out || ((uintptr_t)out & 3)) return RADET_ERR_ARG;
    const dim3 grid((Ho * Wo + 256 * CROP_TILES - 1) / (256 * CROP_TILES), cap), block(256);
    hipStream_t st = (hipStream_t)stream;
    const int rgb = flags & CROP_TO_RGB;
    if (flags & CROP_F32)
        hipLaunchKernelGGL((crop_frames_kernel<true, false>), grid, block, 0, st, rows, counters, desc, B, out, Ho, Wo, rgb, fill,
                           m0, m1, m2, s0, s1, s2);
    else if ((Ho * Wo) % 4 == 0)
        hipLaunchKernelGGL((crop_frames_kernel<false, true>), grid, block, 0, st, rows, counters, desc, B, out, Ho, Wo, rgb, fill,
                           m0, m1, m2, s0, s1, s2);
    else
        hipLaunchKernelGGL((crop_frames_kernel<false, false>), grid, block, 0, st, rows, counters, desc, B, out, Ho, Wo, rgb, fill,
                           m0, m1, m2, s0, s1, s2);
    return radet_check_launch();
}
