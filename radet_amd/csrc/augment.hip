// Photometric training augmentation of the BOP pipeline (RandomBackground + CosyPoseAug's five Pillow stages +
// RandomFlip / Normalize / Pad), batched over images of differing sizes: four launches per batch, whatever B is.
//
// Images are packed u8 HWC BGR arrays, back to back; every intermediate buffer has the same packing.  One row of
// AUG_PARAM_INTS ints per image (include/radet_hip.h) says where its pixels are and which stages are on; a stage that is
// off passes the image through unchanged.  The kernels restate Pillow's integer / float32 arithmetic (libImaging
// BoxBlur.c, Filter.c, Blend.c, Convert.c): tests/_augment_ref.py is the NumPy restatement, pinned bit for bit to Pillow.
//   merge + hblur : background pixel where no instance mask equals 1; then 3 horizontal box passes (GaussianBlur(k))
//   vblur         : 3 vertical box passes (Pillow blurs all rows first, then all columns)
//   sharp         : SMOOTH 3x3 (1 1 1 / 1 5 1 / 1 1 1, /13, float), border pixels kept, blended with the image; the
//                   image's luma sum for Contrast (u64 atomics: integer, order-independent)
//   finish        : Contrast, Brightness, Color blends, horizontal flip, BGR->RGB, Normalize, zero pad -> f32[B,3,Hp,Wp]
#include "common.h"
#include "../../include/radet_hip.h"

enum {
    AUG_MERGE = 1, AUG_BLUR = 2, AUG_SHARP = 4, AUG_CONTRAST = 8, AUG_BRIGHT = 16, AUG_COLOR = 32, AUG_FLIP = 64, AUG_TO_RGB = 128
};

struct AugImg {
    int off, h, w, flags, bg_off, nmask;
    const uint8_t* masks;
    int r;
    unsigned ww, fw;
    float f_sharp, f_contrast, f_bright, f_color;
};

__device__ __forceinline__ AugImg load_img(const int* params, int n) {
    const int* p = params + AUG_PARAM_INTS * n;
    AugImg a;
    a.off = p[0]; a.h = p[1]; a.w = p[2]; a.flags = p[3]; a.bg_off = p[4]; a.nmask = p[5];
    a.masks = (const uint8_t*)(((uint64_t)(uint32_t)p[7] << 32) | (uint64_t)(uint32_t)p[6]);
    a.r = p[8]; a.ww = (unsigned)p[9]; a.fw = (unsigned)p[10];
    a.f_sharp = __int_as_float(p[11]); a.f_contrast = __int_as_float(p[12]);
    a.f_bright = __int_as_float(p[13]); a.f_color = __int_as_float(p[14]);
    return a;
}

// Image.blend(in1, in2, alpha) per byte: in1 + alpha * (in2 - in1) in float32, truncated; clipped outside [0, 1]
__device__ __forceinline__ int pil_blend(int in1, int in2, float alpha) {
    const float t = (float)in1 + alpha * (float)(in2 - in1);
    if (alpha >= 0.f && alpha <= 1.f) return (int)t;
    if (t <= 0.f) return 0;
    if (t >= 255.f) return 255;
    return (int)t;
}

// convert("L"): ITU-R 601-2 luma in 16-bit fixed point; bgr = the pixel's bytes in BGR order
__device__ __forceinline__ int pil_luma(int b, int g, int r) { return (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16; }

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// one box pass of ImagingHorizontalBoxBlur over n samples spaced `stride` apart (channel interleave):
// out[x] = (sum in[clamp(x-r .. x+r)] * ww + (in[clamp(x-r-1)] + in[clamp(x+r+1)]) * fw + 2^23) >> 24
__device__ __forceinline__ uint8_t box_tap(const uint8_t* in, int x, int n, int stride, int r, unsigned ww, unsigned fw) {
    unsigned s = 0;
    for (int k = -r; k <= r; ++k) s += in[clampi(x + k, 0, n - 1) * stride];
    const unsigned far = (unsigned)in[clampi(x - r - 1, 0, n - 1) * stride] + (unsigned)in[clampi(x + r + 1, 0, n - 1) * stride];
    return (uint8_t)((s * ww + far * fw + (1u << 23)) >> 24);
}

// grid (max_h, nimg): one row per workgroup; LDS = 2 x (3 * max_w) bytes
__global__ __launch_bounds__(256) void aug_merge_hblur_kernel(const uint8_t* __restrict__ src, const uint8_t* __restrict__ bg,
                                                              const int* __restrict__ params, uint8_t* __restrict__ dst) {
    extern __shared__ uint8_t lds[];
    const AugImg a = load_img(params, blockIdx.y);
    const int y = blockIdx.x;
    if (y >= a.h) return;
    const int n = a.w * 3;
    uint8_t* A = lds;
    uint8_t* B = lds + n;
    const size_t row = (size_t)a.off + (size_t)y * a.w;
    const size_t plane = (size_t)a.h * a.w;
    for (int i = threadIdx.x; i < n; i += 256) {
        uint8_t v = src[row * 3 + i];
        if (a.flags & AUG_MERGE) {
            const int x = i / 3;
            bool fg = false;
            for (int g = 0; g < a.nmask && !fg; ++g) fg = a.masks[g * plane + (size_t)y * a.w + x] == 1;
            if (!fg) v = bg[((size_t)a.bg_off + (size_t)y * a.w) * 3 + i];
        }
        A[i] = v;
    }
    if (a.flags & AUG_BLUR) {
        for (int pass = 0; pass < 3; ++pass) {
            __syncthreads();
            for (int i = threadIdx.x; i < n; i += 256) {
                const int x = i / 3, c = i - 3 * x;
                B[i] = box_tap(A + c, x, a.w, 3, a.r, a.ww, a.fw);
            }
            uint8_t* t = A; A = B; B = t;
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += 256) dst[row * 3 + i] = A[i];
}

// grid (ceil(max_w / cols), nimg): a strip of `cols` columns per workgroup; LDS = 2 x (3 * cols * max_h) bytes
__global__ __launch_bounds__(256) void aug_vblur_kernel(const uint8_t* __restrict__ src, const int* __restrict__ params,
                                                        uint8_t* __restrict__ dst, int cols) {
    extern __shared__ uint8_t lds[];
    const AugImg a = load_img(params, blockIdx.y);
    const int x0 = blockIdx.x * cols;
    if (x0 >= a.w) return;
    const int nc = min(cols, a.w - x0) * 3;              // bytes per strip row
    const int n = nc * a.h;
    if (!(a.flags & AUG_BLUR)) {
        for (int i = threadIdx.x; i < n; i += 256) {
            const int y = i / nc, j = i - y * nc;
            const size_t o = ((size_t)a.off + (size_t)y * a.w + x0) * 3 + j;
            dst[o] = src[o];
        }
        return;
    }
    uint8_t* A = lds;
    uint8_t* B = lds + n;
    for (int i = threadIdx.x; i < n; i += 256) {
        const int y = i / nc, j = i - y * nc;
        A[i] = src[((size_t)a.off + (size_t)y * a.w + x0) * 3 + j];
    }
    for (int pass = 0; pass < 3; ++pass) {
        __syncthreads();
        for (int i = threadIdx.x; i < n; i += 256) {
            const int y = i / nc, j = i - y * nc;
            B[i] = box_tap(A + j, y, a.h, nc, a.r, a.ww, a.fw);
        }
        uint8_t* t = A; A = B; B = t;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += 256) {
        const int y = i / nc, j = i - y * nc;
        dst[((size_t)a.off + (size_t)y * a.w + x0) * 3 + j] = A[i];
    }
}

__device__ __forceinline__ int pil_clip8(float v) {
    if (v <= 0.f) return 0;
    if (v >= 255.f) return 255;
    return (int)((double)v + 0.5);                   // (Filter.c's clip8 adds a double 0.5)
}

// grid (ceil(max_px / 256), nimg): one pixel per thread
__global__ __launch_bounds__(256) void aug_sharp_kernel(const uint8_t* __restrict__ src, const int* __restrict__ params,
                                                        uint8_t* __restrict__ dst, unsigned long long* __restrict__ lsum) {
    __shared__ unsigned long long part[4];
    const AugImg a = load_img(params, blockIdx.y);
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (blockIdx.x * 256 >= a.h * a.w) return;            // (uniform over the workgroup)
    unsigned l = 0;
    if (p < a.h * a.w) {
        const int y = p / a.w, x = p - y * a.w;
        const uint8_t* s = src + ((size_t)a.off + p) * 3;
        int v[3] = {s[0], s[1], s[2]};
        if ((a.flags & AUG_SHARP) && y > 0 && y < a.h - 1 && x > 0 && x < a.w - 1) {
            const float k1 = 1.f / 13.f, k5 = 5.f / 13.f;
            const int st = a.w * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const uint8_t* dn = s + st + c;                  // Pillow's in1 (row y + 1) takes kernel[0..2] ...
                const uint8_t* md = s + c;
                const uint8_t* up = s - st + c;                  // ... and in_1 (row y - 1) kernel[6..8]
                float ss = 0.f;
                ss += (float)dn[-3] * k1 + (float)dn[0] * k1 + (float)dn[3] * k1;
                ss += (float)md[-3] * k1 + (float)md[0] * k5 + (float)md[3] * k1;
                ss += (float)up[-3] * k1 + (float)up[0] * k1 + (float)up[3] * k1;
                v[c] = pil_blend(pil_clip8(ss), v[c], a.f_sharp);
            }
        }
        uint8_t* d = dst + ((size_t)a.off + p) * 3;
        d[0] = (uint8_t)v[0]; d[1] = (uint8_t)v[1]; d[2] = (uint8_t)v[2];
        l = (unsigned)pil_luma(v[0], v[1], v[2]);
    }
    if (!(a.flags & AUG_CONTRAST)) return;
    unsigned long long t = l;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = t;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(lsum + blockIdx.y, part[0] + part[1] + part[2] + part[3]);
}

// grid (ceil(Hp * Wp / 256), nimg): one output pixel (3 planes) per thread
__global__ __launch_bounds__(256) void aug_finish_kernel(const uint8_t* __restrict__ src, const unsigned long long* __restrict__ lsum,
                                                         const int* __restrict__ params, float* __restrict__ out, int Hp, int Wp,
                                                         float m0, float m1, float m2, float s0, float s1, float s2) {
    const AugImg a = load_img(params, blockIdx.y);
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= Hp * Wp) return;
    const int y = p / Wp, x = p - y * Wp;
    float* o = out + (size_t)blockIdx.y * 3 * Hp * Wp + p;
    const size_t plane = (size_t)Hp * Wp;
    if (y >= a.h || x >= a.w) {
        o[0] = 0.f; o[plane] = 0.f; o[2 * plane] = 0.f;
        return;
    }
    const int sx = (a.flags & AUG_FLIP) ? a.w - 1 - x : x;
    const uint8_t* s = src + ((size_t)a.off + (size_t)y * a.w + sx) * 3;
    int v[3] = {s[0], s[1], s[2]};
    if (a.flags & AUG_CONTRAST) {
        const int mean = (int)((double)lsum[blockIdx.y] / (double)((long long)a.h * a.w) + 0.5);
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = pil_blend(mean, v[c], a.f_contrast);
    }
    if (a.flags & AUG_BRIGHT) {
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = pil_blend(0, v[c], a.f_bright);
    }
    if (a.flags & AUG_COLOR) {
        const int l = pil_luma(v[0], v[1], v[2]);
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = pil_blend(l, v[c], a.f_color);
    }
    const bool rgb = a.flags & AUG_TO_RGB;
    const float q0 = (float)(rgb ? v[2] : v[0]), q1 = (float)v[1], q2 = (float)(rgb ? v[0] : v[2]);
    o[0] = (q0 - m0) * s0;
    o[plane] = (q1 - m1) * s1;
    o[2 * plane] = (q2 - m2) * s2;
}

extern "C" int radet_augment_merge_hblur(const uint8_t* src, const uint8_t* bg, const int* params, uint8_t* dst, int nimg,
                                         int max_h, int max_w, void* stream) {
    if (nimg < 0 || max_h < 0 || max_w < 0 || max_w > AUG_MAX_W) return RADET_ERR_ARG;
    if (nimg == 0 || max_h == 0 || max_w == 0) return RADET_OK;
    hipLaunchKernelGGL(aug_merge_hblur_kernel, dim3(max_h, nimg), dim3(256), 6 * max_w, (hipStream_t)stream, src, bg, params, dst);
    return radet_check_launch();
}

static int vblur_cols(int max_h) { return min(64, (6 * AUG_MAX_W) / (6 * max_h)); }

extern "C" int radet_augment_vblur(const uint8_t* src, const int* params, uint8_t* dst, int nimg, int max_h, int max_w,
                                   void* stream) {
    if (nimg < 0 || max_h < 0 || max_w < 0 || max_h > AUG_MAX_W) return RADET_ERR_ARG;
    if (nimg == 0 || max_h == 0 || max_w == 0) return RADET_OK;
    const int cols = vblur_cols(max_h);
    hipLaunchKernelGGL(aug_vblur_kernel, dim3((max_w + cols - 1) / cols, nimg), dim3(256), 6 * cols * max_h, (hipStream_t)stream,
                       src, params, dst, cols);
    return radet_check_launch();
}

extern "C" int radet_augment_sharp(const uint8_t* src, const int* params, uint8_t* dst, unsigned long long* lsum, int nimg,
                                   int max_px, void* stream) {
    if (nimg < 0 || max_px < 0) return RADET_ERR_ARG;
    if (nimg == 0) return RADET_OK;
    if (hipMemsetAsync(lsum, 0, sizeof(unsigned long long) * nimg, (hipStream_t)stream) != hipSuccess) return RADET_ERR_LAUNCH;
    if (max_px == 0) return RADET_OK;
    hipLaunchKernelGGL(aug_sharp_kernel, dim3((max_px + 255) / 256, nimg), dim3(256), 0, (hipStream_t)stream, src, params, dst, lsum);
    return radet_check_launch();
}

extern "C" int radet_augment_finish(const uint8_t* src, const unsigned long long* lsum, const int* params, float* out, int nimg,
                                    int Hp, int Wp, float m0, float m1, float m2, float s0, float s1, float s2, void* stream) {
    if (nimg < 0 || Hp < 0 || Wp < 0) return RADET_ERR_ARG;
    if (nimg == 0 || Hp == 0 || Wp == 0) return RADET_OK;
    hipLaunchKernelGGL(aug_finish_kernel, dim3((Hp * Wp + 255) / 256, nimg), dim3(256), 0, (hipStream_t)stream, src, lsum, params,
                       out, Hp, Wp, m0, m1, m2, s0, s1, s2);
    return radet_check_launch();
}
