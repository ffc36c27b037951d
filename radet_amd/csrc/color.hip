// The colour stages of AutoAugment (radet/datasets/pipelines/auto_augment.py:709-890: ColorTransform, EqualizeTransform,
// BrightnessTransform, ContrastTransform, i.e. mmcv.adjust_color / imequalize / adjust_brightness / adjust_contrast) for a
// batch of packed u8 HWC BGR images, in place, in two launches: radet_color_stats_u8 counts the per-image histograms of B,
// G, R and gray that Equalize and Contrast need, radet_color_apply_u8 builds each row's 3 x 256-byte map from its
// descriptor and histogram and maps the image (Brightness, Contrast, Equalize) or blends every pixel with its gray (Color).
// The pixel rules are written out in include/radet_hip.h.
//
// One row of COLOR_DESC_INTS ints per image; grid (ceil(largest image / COLOR_CHUNK_PX), images): a workgroup of 256
// threads takes one chunk of COLOR_CHUNK_PX pixels of one image.  An image starts at byte 3 * offset of the buffer, at any
// alignment, and its neighbours in the buffer belong to other images, so a chunk is staged through LDS at its own 16-byte
// phase: whole aligned 16-byte words where they lie inside the chunk, single bytes at its unaligned head and tail; no byte
// outside the chunk is read or written.  Both kernels are memory-bound (12 KB in, and for apply 12 KB out, per workgroup).
// Statistics: integer LDS atomics into one histogram copy per wave (a flat region then serialises a wave on one
// address, not the workgroup), then one integer global atomic per non-zero bin: integer sums do not depend on the order
// of arrival, so the histograms and everything built from them are bit-reproducible.  No float atomics, no scratch.
#include "common.h"
#include "../../include/radet_hip.h"

constexpr int CHUNK_BYTES = 3 * COLOR_CHUNK_PX;
constexpr int STAGE_BYTES = CHUNK_BYTES + 16;      // (the chunk behind up to 15 bytes of phase, in whole words)

struct ColorChunk { size_t b0; int npx, total, kind; };   // first byte in the buffer, pixels of the chunk, pixels of the image

// chunk blockIdx.x of the image of row d; false for a row that is not run (skipped, no such kind, no pixels, an image
// that leaves the buffer) and behind the image's last chunk
__device__ __forceinline__ bool color_chunk(const int* __restrict__ d, long long img_px, ColorChunk* c) {
    const int off = d[COLOR_DESC_OFF], h = d[COLOR_DESC_H], w = d[COLOR_DESC_W], kind = d[COLOR_DESC_KIND];
    if ((d[COLOR_DESC_FLAGS] & COLOR_SKIP) || kind < COLOR_BRIGHTNESS || kind > COLOR_EQUALIZE) return false;
    if (h <= 0 || w <= 0 || off < 0) return false;
    const long long n = (long long)h * w;
    if ((long long)off + n > img_px) return false;                  // (img_px < 2^31: n fits an int from here on)
    const long long p0 = (long long)blockIdx.x * COLOR_CHUNK_PX;
    if (p0 >= n) return false;
    c->b0 = ((size_t)off + (size_t)p0) * 3;
    c->npx = (int)min((long long)COLOR_CHUNK_PX, n - p0);
    c->total = (int)n;
    c->kind = kind;
    return true;
}

// bytes [b0, b0 + nbytes) of img <-> stage[phase ..), phase = the address of the first byte mod 16; returns the phase
template <bool OUT>
__device__ __forceinline__ int stage_copy(uint8_t* img, size_t b0, int nbytes, uint8_t* stage) {
    const int phase = (int)((uintptr_t)(img + b0) & 15);
    uint8_t* base = img + b0 - phase;                                // (16-byte aligned; the bytes before b0 are not touched)
    const int end = phase + nbytes;
    for (int j = threadIdx.x; j * 16 < end; j += 256) {
        const int lo = j * 16, hi = lo + 16;
        if (lo >= phase && hi <= end) {
            if (OUT) *reinterpret_cast<uint4*>(base + lo) = *reinterpret_cast<const uint4*>(stage + lo);
            else *reinterpret_cast<uint4*>(stage + lo) = *reinterpret_cast<const uint4*>(base + lo);
        } else {
            for (int k = max(lo, phase); k < min(hi, end); ++k) {
                if (OUT) base[k] = stage[k];
                else stage[k] = base[k];
            }
        }
    }
    return phase;
}

__device__ __forceinline__ int bgr2gray(int b, int g, int r) { return (3735 * b + 19235 * g + 9798 * r + 16384) >> 15; }

__global__ __launch_bounds__(256) void color_stats_kernel(const uint8_t* __restrict__ img, long long img_px, const int* __restrict__ desc,
                                                          unsigned* __restrict__ hist) {
    __shared__ __attribute__((aligned(16))) uint8_t stage[STAGE_BYTES];
    __shared__ unsigned wh[4][4][256];                              // [wave][B, G, R, gray][value]
    ColorChunk c;
    if (!color_chunk(desc + (size_t)COLOR_DESC_INTS * blockIdx.y, img_px, &c)) return;
    if (c.kind != COLOR_EQUALIZE && c.kind != COLOR_CONTRAST) return;
    for (int i = threadIdx.x; i < 4 * 4 * 256; i += 256) (&wh[0][0][0])[i] = 0u;
    const int phase = stage_copy<false>(const_cast<uint8_t*>(img), c.b0, 3 * c.npx, stage);
    __syncthreads();
    unsigned (*mine)[256] = wh[threadIdx.x >> 6];
    // a thread's pixels (p, p + 256, ...) counted as runs of equal values: on a flat region the 64 lanes of a wave would
    // otherwise meet on one LDS address at every pixel; a run costs one atomic whatever its length
    int held[4] = {-1, -1, -1, -1};
    unsigned run[4] = {0u, 0u, 0u, 0u};
    for (int p = threadIdx.x; p < c.npx; p += 256) {
        const uint8_t* q = stage + phase + 3 * p;
        const int b = q[0], g = q[1], r = q[2];
        const int v[4] = {b, g, r, bgr2gray(b, g, r)};
#pragma unroll
        for (int ch = 0; ch < 4; ++ch) {
            if (v[ch] == held[ch]) { ++run[ch]; continue; }
            if (run[ch]) atomicAdd(&mine[ch][held[ch]], run[ch]);
            held[ch] = v[ch];
            run[ch] = 1u;
        }
    }
#pragma unroll
    for (int ch = 0; ch < 4; ++ch)
        if (run[ch]) atomicAdd(&mine[ch][held[ch]], run[ch]);
    __syncthreads();
    unsigned* out = hist + (size_t)blockIdx.y * 4 * 256;
    for (int ch = 0; ch < 4; ++ch) {
        const unsigned s = wh[0][ch][threadIdx.x] + wh[1][ch][threadIdx.x] + wh[2][ch][threadIdx.x] + wh[3][ch][threadIdx.x];
        if (s) atomicAdd(out + ch * 256 + threadIdx.x, s);
    }
}

// inclusive prefix sum over the workgroup's 256 threads (thread t holds bin t); part: 4 words of LDS
__device__ __forceinline__ unsigned scan256(unsigned v, unsigned* part) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned t = __shfl_up(v, d, 64);
        if (lane >= d) v += t;
    }
    if (lane == 63) part[wave] = v;
    __syncthreads();
    for (int k = 0; k < wave; ++k) v += part[k];
    __syncthreads();
    return v;
}

// fp32 -> byte as `np.clip(t, 0, 255).astype(np.uint8)`: clipped, then truncated
__device__ __forceinline__ uint8_t clip_trunc(float t) { return (uint8_t)(int)fminf(fmaxf(t, 0.f), 255.f); }

__global__ __launch_bounds__(256) void color_apply_kernel(uint8_t* __restrict__ img, long long img_px, const int* __restrict__ desc,
                                                          const unsigned* __restrict__ hist) {
    __shared__ __attribute__((aligned(16))) uint8_t stage[STAGE_BYTES];
    __shared__ uint8_t lut[3][256];
    __shared__ unsigned part[4], step[3];
    __shared__ unsigned long long part64[4];
    const int* d = desc + (size_t)COLOR_DESC_INTS * blockIdx.y;
    ColorChunk c;
    if (!color_chunk(d, img_px, &c)) return;
    if ((c.kind == COLOR_EQUALIZE || c.kind == COLOR_CONTRAST) && !hist) return;
    const float alpha = __int_as_float(d[COLOR_DESC_ALPHA]), beta = __int_as_float(d[COLOR_DESC_BETA]);
    const int v = threadIdx.x;
    if (c.kind == COLOR_BRIGHTNESS) {
        lut[0][v] = lut[1][v] = lut[2][v] = clip_trunc(__fmul_rn((float)v, alpha));
    } else if (c.kind == COLOR_CONTRAST) {
        const unsigned* hrow = hist + (size_t)blockIdx.y * 4 * 256;      // (hist is not NULL here: checked above)
        // mean = round half to even of sum(v * ghist[v]) / N, in integers
        unsigned long long s = (unsigned long long)v * hrow[3 * 256 + v];
        for (int m = 32; m; m >>= 1) s += __shfl_xor(s, m, 64);
        if ((v & 63) == 0) part64[v >> 6] = s;
        __syncthreads();
        s = part64[0] + part64[1] + part64[2] + part64[3];
        const unsigned long long n = (unsigned long long)c.total, r = s % n;
        unsigned long long mean = s / n;
        mean += (2 * r > n || (2 * r == n && (mean & 1))) ? 1 : 0;
        const float m = __fmul_rn((float)mean, beta);
        lut[0][v] = lut[1][v] = lut[2][v] = clip_trunc(__fmaf_rn((float)v, alpha, m));
    } else if (c.kind == COLOR_EQUALIZE) {
        const unsigned* hrow = hist + (size_t)blockIdx.y * 4 * 256;
        if (v < 3) step[v] = 0u;
        __syncthreads();
        for (int ch = 0; ch < 3; ++ch) {
            const unsigned hv = hrow[ch * 256 + v], incl = scan256(hv, part);
            // the highest value present is where the running count reaches N: step = (N - its count) / 255
            if (hv && incl == (unsigned)c.total) step[ch] = ((unsigned)c.total - hv) / 255u;
            __syncthreads();
            const unsigned st = step[ch];
            lut[ch][v] = st ? (uint8_t)min(255u, (incl - hv + st / 2) / st) : (uint8_t)v;
        }
    }
    const int phase = stage_copy<false>(img, c.b0, 3 * c.npx, stage);
    __syncthreads();
    for (int p = threadIdx.x; p < c.npx; p += 256) {
        uint8_t* q = stage + phase + 3 * p;
        if (c.kind == COLOR_COLOR) {
            // per channel fma(x, alpha, fl32(gray * beta)), rounded half to even, saturated: the product rounds on its own
            const int b = q[0], g = q[1], r = q[2];
            const float gb = __fmul_rn((float)bgr2gray(b, g, r), beta);
            q[0] = (uint8_t)(int)fminf(fmaxf(rintf(__fmaf_rn((float)b, alpha, gb)), 0.f), 255.f);
            q[1] = (uint8_t)(int)fminf(fmaxf(rintf(__fmaf_rn((float)g, alpha, gb)), 0.f), 255.f);
            q[2] = (uint8_t)(int)fminf(fmaxf(rintf(__fmaf_rn((float)r, alpha, gb)), 0.f), 255.f);
        } else {
            q[0] = lut[0][q[0]];
            q[1] = lut[1][q[1]];
            q[2] = lut[2][q[2]];
        }
    }
    __syncthreads();
    stage_copy<true>(img, c.b0, 3 * c.npx, stage);
}

static int color_args(const void* img, size_t img_px, const int* desc, int nimg, int max_px, int channels) {
    if (channels != 3 || nimg < 0 || max_px < 0 || nimg > 65535 || max_px > 0x7FFFFFFF - COLOR_CHUNK_PX) return RADET_ERR_ARG;
    if (nimg == 0 || max_px == 0) return RADET_OK;
    if (!img || !desc || ((uintptr_t)desc & 3) || img_px > 0x7FFFFFFFull) return RADET_ERR_ARG;   // (pixel offsets are ints)
    return 1;                                                       // (launch)
}

extern "C" int radet_color_stats_u8(const uint8_t* img, size_t img_px, const int* desc, int nimg, int max_px, unsigned* hist,
                                    int channels, void* stream) {
    const int rc = color_args(img, img_px, desc, nimg, max_px, channels);
    if (rc != 1) return rc;
    if (!hist || ((uintptr_t)hist & 3)) return RADET_ERR_ARG;
    hipLaunchKernelGGL(color_stats_kernel, dim3((max_px + COLOR_CHUNK_PX - 1) / COLOR_CHUNK_PX, nimg), dim3(256), 0,
                       (hipStream_t)stream, img, (long long)img_px, desc, hist);
    return radet_check_launch();
}

extern "C" int radet_color_apply_u8(uint8_t* img, size_t img_px, const int* desc, int nimg, int max_px, const unsigned* hist,
                                    int channels, void* stream) {
    const int rc = color_args(img, img_px, desc, nimg, max_px, channels);
    if (rc != 1) return rc;
    if ((uintptr_t)hist & 3) return RADET_ERR_ARG;
    hipLaunchKernelGGL(color_apply_kernel, dim3((max_px + COLOR_CHUNK_PX - 1) / COLOR_CHUNK_PX, nimg), dim3(256), 0,
                       (hipStream_t)stream, img, (long long)img_px, desc, hist);
    return radet_check_launch();
}
