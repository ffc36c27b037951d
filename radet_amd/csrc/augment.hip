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
#include "pixel_ops.h"
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
    // the masks are u8 [G,h,w], or (mask pitch word Hm << 16 | Wm) the top-left h x w of u8 [G,Hm,Wm]; a pitch that does
    // not hold the image counts as no masks
    const int pitch = params[AUG_PARAM_INTS * blockIdx.y + 15];
    const int mh = pitch ? pitch >> 16 : a.h, mw = pitch ? pitch & 0xFFFF : a.w;
    const int nmask = (mh >= a.h && mw >= a.w) ? a.nmask : 0;
    const size_t mplane = (size_t)mh * mw;
    for (int i = threadIdx.x; i < n; i += 256) {
        uint8_t v = src[row * 3 + i];
        if (a.flags & AUG_MERGE) {
            const int x = i / 3;
            bool fg = false;
            for (int g = 0; g < nmask && !fg; ++g) fg = a.masks[g * mplane + (size_t)y * mw + x] == 1;
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

// The u8 BGR pixel (y, x) of image n after the last photometric stage and the flip: what the reference's image holds when
// Normalize (and the mask-free GenerateDistanceMap) read it.  src = the output of sharp (or of box in a mix pipeline).
__device__ __forceinline__ void aug_final_bgr(const uint8_t* __restrict__ src, const unsigned long long* __restrict__ lsum,
                                              const AugImg& a, int n, int y, int x, int v[3]) {
    const int sx = (a.flags & AUG_FLIP) ? a.w - 1 - x : x;
    const uint8_t* s = src + ((size_t)a.off + (size_t)y * a.w + sx) * 3;
    v[0] = s[0]; v[1] = s[1]; v[2] = s[2];
    if (a.flags & AUG_CONTRAST) {
        const int mean = (int)((double)lsum[n] / (double)((long long)a.h * a.w) + 0.5);
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
        zero_store(o, plane);
        return;
    }
    int v[3];
    aug_final_bgr(src, lsum, a, blockIdx.y, y, x, v);
    norm_store(o, plane, v, a.flags & AUG_TO_RGB, m0, m1, m2, s0, s1, s2);
}

// The padded box crops of the mask-free sampler (GenerateDistanceMap(with_gt_mask=False)): one descriptor row per box
// (include/radet_hip.h, CROP_DESC_INTS); canvases are packed u8 HWC arrays, back to back.
struct CropBox { int img, wx, wy, cw, ch, sx0, sy0, sx1, sy1, fill, out; };

__device__ __forceinline__ CropBox load_crop_box(const int* desc, int n) {
    const int* d = desc + CROP_DESC_INTS * n;
    CropBox b;
    b.img = d[0]; b.wx = d[1]; b.wy = d[2]; b.cw = d[3]; b.ch = d[4];
    b.sx0 = d[5]; b.sy0 = d[6]; b.sx1 = d[7]; b.sy1 = d[8]; b.fill = d[9]; b.out = d[10];
    return b;
}

// canvas pixel p as b | g << 8 | r << 16: the image pixel under it inside the source rectangle (already intersected with
// the image by the caller: no address is formed from a coordinate outside it), the fill colour elsewhere
__device__ __forceinline__ uint32_t canvas_pixel(const uint8_t* __restrict__ src, const unsigned long long* __restrict__ lsum,
                                                 const AugImg& a, const CropBox& b, int p) {
    const int cy = p / b.cw, cx = p - cy * b.cw;
    const int x = b.wx + cx, y = b.wy + cy;
    if (x < b.sx0 || x >= b.sx1 || y < b.sy0 || y >= b.sy1) return (uint32_t)b.fill & 0xFFFFFFu;
    int v[3];
    aug_final_bgr(src, lsum, a, b.img, y, x, v);
    return (uint32_t)v[0] | ((uint32_t)v[1] << 8) | ((uint32_t)v[2] << 16);
}

// grid (ceil((3 * max_px / 4 + 2) / 256), ncanvas): one aligned dword of the packed output per thread.  A dword holds
// bytes of at most two pixels; it is stored whole where all four bytes belong to this canvas, byte by byte at the two
// ends (the neighbouring canvases own the other bytes of those dwords).
__global__ __launch_bounds__(256) void crop_canvases_kernel(const uint8_t* __restrict__ src, const unsigned long long* __restrict__ lsum,
                                                            const int* __restrict__ params, int nimg, const int* __restrict__ desc,
                                                            uint8_t* __restrict__ dst, long long total_px, long long src_bytes) {
    CropBox b = load_crop_box(desc, blockIdx.y);
    if (b.img < 0 || b.img >= nimg || b.cw <= 0 || b.ch <= 0 || b.out < 0) return;          // (uniform over the workgroup)
    const long long npx = (long long)b.cw * b.ch;
    if ((long long)b.out + npx > total_px) return;
    const AugImg a = load_img(params, b.img);
    if (a.off < 0 || a.h <= 0 || a.w <= 0 || 3 * ((long long)a.off + (long long)a.h * a.w) > src_bytes) return;
    b.sx0 = max(b.sx0, 0); b.sy0 = max(b.sy0, 0); b.sx1 = min(b.sx1, a.w); b.sy1 = min(b.sy1, a.h);
    const long long gs = 3ll * b.out, ge = gs + 3 * npx;           // this canvas's bytes of dst
    const long long G = (gs & ~3ll) + 4ll * ((long long)blockIdx.x * 256 + threadIdx.x);
    if (G >= ge) return;
    const long long k0 = G - gs;                                   // canvas byte of the dword's first byte (-3 .. at the head)
    const int p0 = (int)((k0 < 0 ? 0 : k0) / 3);
    const int r0 = (int)(k0 - 3ll * p0);                           // byte of pixel p0 the dword starts at (negative at the head)
    // bytes r0 .. r0 + 3 of the 6-byte string (pixel p0, pixel p0 + 1)
    uint64_t two = canvas_pixel(src, lsum, a, b, p0);
    if (r0 + 3 > 2 && p0 + 1 < npx) two |= (uint64_t)canvas_pixel(src, lsum, a, b, p0 + 1) << 24;
    if (r0 >= 0 && G + 4 <= ge) {
        *(uint32_t*)(dst + G) = (uint32_t)(two >> (8 * r0));
    } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int r = r0 + q;                                   // byte of the string
            if (r >= 0 && G + q < ge) dst[G + q] = (uint8_t)(two >> (8 * r));
        }
    }
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

extern "C" int radet_crop_canvases(const uint8_t* src, size_t src_bytes, const unsigned long long* lsum, const int* params, int nimg,
                                   const int* desc, int ncanvas, int max_px, uint8_t* dst, size_t total_px, void* stream) {
    if (nimg < 0 || ncanvas < 0 || max_px < 0 || ((uintptr_t)dst & 3)) return RADET_ERR_ARG;
    if (nimg == 0 || ncanvas == 0 || max_px == 0) return RADET_OK;
    const long long dwords = (3ll * max_px + 3) / 4 + 1;          // an unaligned canvas touches one dword more
    hipLaunchKernelGGL(crop_canvases_kernel, dim3((unsigned)((dwords + 255) / 256), ncanvas), dim3(256), 0, (hipStream_t)stream, src,
                       lsum, params, nimg, desc, dst, (long long)total_px, (long long)src_bytes);
    return radet_check_launch();
}

// ---------------------------------------------------------------------------------------------------------------------
// The mixpbr stages between RandomBackground and RandomFlip (RandomHSV, RandomNoise, RandomSmooth), two more launches per
// batch over the same packed layout.  Their per-image parameters live in a second table of AUG2_PARAM_INTS ints per image
// (include/radet_hip.h); tests/_mixaug_ref.py is the NumPy restatement the kernels equal bit for bit (the noise up to the
// last ulp of ocml's fp64 log / sin / cos against the host's).
//   hsv_noise : BGR->HSV (OpenCV RGB2HSV_b, 12-bit fixed point), float32 channel scales with the reference's clip and
//               truncation, HSV->BGR (HSV2RGB_b's float path), then img + (sigma z) 255 in fp64, z from Box-Muller on a
//               Philox-4x64-10 stream (element e = (y w + x) 3 + c; pair e >> 1 uses words 2p, 2p + 1; block b counter b + 1)
//   box       : cv2.blur k x k (k = 1, 3, 5, 7), BORDER_REFLECT_101, (window sum + (k^2 - 1) / 2) / k^2
enum { AUG2_HSV = 1, AUG2_NOISE = 2, AUG2_BOX = 4 };

struct Aug2Img {
    int off, h, w, flags;
    float fa, fb, fc;
    int lt;                       // bit 0 / 1 / 2: the (double) h / s / v factor is < 1 (no clip)
    double sigma;
    uint64_t k0, k1;
    int k;
};

__device__ __forceinline__ Aug2Img load_img2(const int* params, int n) {
    const int* p = params + AUG2_PARAM_INTS * n;
    Aug2Img a;
    a.off = p[0]; a.h = p[1]; a.w = p[2]; a.flags = p[3];
    a.fa = __int_as_float(p[4]); a.fb = __int_as_float(p[5]); a.fc = __int_as_float(p[6]); a.lt = p[7];
    a.sigma = __longlong_as_double((long long)(((uint64_t)(uint32_t)p[9] << 32) | (uint32_t)p[8]));
    a.k0 = ((uint64_t)(uint32_t)p[11] << 32) | (uint32_t)p[10];
    a.k1 = ((uint64_t)(uint32_t)p[13] << 32) | (uint32_t)p[12];
    a.k = p[14];
    return a;
}

// Philox-4x64-10 (Salmon et al. 2011; numpy.random.Philox) of the counter (c0, 0, 0, 0)
__device__ __forceinline__ void philox4x64_10(uint64_t c0, uint64_t k0, uint64_t k1, uint64_t out[4]) {
    uint64_t x0 = c0, x1 = 0, x2 = 0, x3 = 0;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        if (r) { k0 += 0x9E3779B97F4A7C15ull; k1 += 0xBB67AE8584CAA73Bull; }
        const uint64_t lo0 = 0xD2E7470EE14C6C93ull * x0, hi0 = __umul64hi(0xD2E7470EE14C6C93ull, x0);
        const uint64_t lo1 = 0xCA5A826395121157ull * x2, hi1 = __umul64hi(0xCA5A826395121157ull, x2);
        x0 = hi1 ^ x1 ^ k0; x1 = lo1; x2 = hi0 ^ x3 ^ k1; x3 = lo0;
    }
    out[0] = x0; out[1] = x1; out[2] = x2; out[3] = x3;
}

// Box-Muller on one pair of words (fp64; -ffp-contract=off keeps every product and sum rounded on its own)
__device__ __forceinline__ void box_muller(uint64_t w0, uint64_t w1, double& z0, double& z1) {
    const double u1 = (double)((w0 >> 11) + 1) * 0x1.0p-53;
    const double u2 = (double)(w1 >> 11) * 0x1.0p-53;
    const double r = sqrt(-2.0 * log(u1));
    const double t = 6.283185307179586 * u2;
    z0 = r * cos(t);
    z1 = r * sin(t);
}

__device__ __forceinline__ int noise_byte(int v, double sigma, double z) {
    double x = (double)v + (sigma * z) * 255.0;
    x = x > 255.0 ? 255.0 : (x < 0.0 ? 0.0 : x);
    return (int)x;
}

// cv2 BGR2HSV (u8) -> scale -> HSV2BGR (u8) of one pixel, in place; sdiv / hdiv: OpenCV's tables (in LDS)
__device__ __forceinline__ void hsv_pixel(int& b, int& g, int& r, const Aug2Img& a, const int* sdiv, const int* hdiv) {
    const int v = max(max(b, g), r), vmin = min(min(b, g), r), diff = v - vmin;
    const int s = (diff * sdiv[v] + (1 << 11)) >> 12;
    int h = v == r ? g - b : (v == g ? b - r + 2 * diff : r - g + 4 * diff);
    h = (h * hdiv[diff] + (1 << 11)) >> 12;
    h += h < 0 ? 180 : 0;
    float hf = (float)h * a.fa, sf = (float)s * a.fb, vf = (float)v * a.fc;
    if (!(a.lt & 1)) hf = fminf(hf, 179.f);
    if (!(a.lt & 2)) sf = fminf(sf, 255.f);
    if (!(a.lt & 4)) vf = fminf(vf, 255.f);
    const float H = (float)(int)hf * (6.f / 180.f), S = (float)(int)sf * (1.f / 255.f), V = (float)(int)vf * (1.f / 255.f);
    float fb = V, fg = V, fr = V;
    if (S != 0.f) {
        float hh = fmodf(H, 6.f);
        int sector = (int)floorf(hh);
        hh -= (float)sector;
        if ((unsigned)sector >= 6u) { sector = 0; hh = 0.f; }
        const float t1 = V * (1.f - S), t2 = V * (1.f - S * hh), t3 = V * (1.f - S * (1.f - hh));
        // sector -> (b, g, r) = tab[{1,3,0}, {1,0,2}, {3,0,1}, {0,2,1}, {0,1,3}, {2,1,0}], tab = (V, t1, t2, t3); selects,
        // not an indexed array (a runtime-indexed array would go to scratch)
        fb = sector <= 1 ? t1 : (sector == 2 ? t3 : (sector == 5 ? t2 : V));
        fg = sector == 0 ? t3 : (sector <= 2 ? V : (sector == 3 ? t2 : t1));
        fr = sector == 0 || sector == 5 ? V : (sector == 1 ? t2 : (sector == 4 ? t3 : t1));
    }
    b = clampi((int)rintf(fb * 255.f), 0, 255);
    g = clampi((int)rintf(fg * 255.f), 0, 255);
    r = clampi((int)rintf(fr * 255.f), 0, 255);
}

// grid (ceil(ceil(max_px / 4) / 256), nimg): 4 pixels = 12 bytes = 3 Philox blocks per thread
__global__ __launch_bounds__(256) void aug_hsv_noise_kernel(const uint8_t* __restrict__ src, const int* __restrict__ params2,
                                                            uint8_t* __restrict__ dst) {
    __shared__ int sdiv[256], hdiv[256];
    const Aug2Img a = load_img2(params2, blockIdx.y);
    const int npx = a.h * a.w;
    if ((int)blockIdx.x * 256 * 4 >= npx) return;          // (uniform over the workgroup)
    {
        const int i = threadIdx.x;                         // round(255 * 2^12 / i), round(180 * 2^12 / (6 i)): no ties
        sdiv[i] = i ? (2 * (255 << 12) + i) / (2 * i) : 0;
        hdiv[i] = i ? (2 * (30 << 12) + i) / (2 * i) : 0;
    }
    __syncthreads();
    const int g = blockIdx.x * 256 + threadIdx.x;
    const int nb = min(12, 3 * (npx - 4 * g));             // bytes of this group
    if (nb <= 0) return;
    const size_t base = (size_t)a.off * 3 + (size_t)g * 12;
    int v[12];
    const bool wide = nb == 12 && ((a.off * 3) & 3) == 0;
    if (wide) {
        const uint32_t* s4 = (const uint32_t*)(src + base);
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const uint32_t u = s4[j];
            v[4 * j] = u & 255; v[4 * j + 1] = (u >> 8) & 255; v[4 * j + 2] = (u >> 16) & 255; v[4 * j + 3] = u >> 24;
        }
    } else {
#pragma unroll
        for (int j = 0; j < 12; ++j) v[j] = j < nb ? src[base + j] : 0;
    }
    if (a.flags & AUG2_HSV) {
#pragma unroll
        for (int p = 0; p < 4; ++p) hsv_pixel(v[3 * p], v[3 * p + 1], v[3 * p + 2], a, sdiv, hdiv);
    }
    if (a.flags & AUG2_NOISE) {
#pragma unroll
        for (int blk = 0; blk < 3; ++blk) {
            uint64_t wd[4];
            philox4x64_10((uint64_t)g * 3 + blk + 1, a.k0, a.k1, wd);
            double z0, z1, z2, z3;
            box_muller(wd[0], wd[1], z0, z1);
            box_muller(wd[2], wd[3], z2, z3);
            v[4 * blk] = noise_byte(v[4 * blk], a.sigma, z0);
            v[4 * blk + 1] = noise_byte(v[4 * blk + 1], a.sigma, z1);
            v[4 * blk + 2] = noise_byte(v[4 * blk + 2], a.sigma, z2);
            v[4 * blk + 3] = noise_byte(v[4 * blk + 3], a.sigma, z3);
        }
    }
    if (wide) {
        uint32_t* d4 = (uint32_t*)(dst + base);
#pragma unroll
        for (int j = 0; j < 3; ++j)
            d4[j] = (uint32_t)v[4 * j] | ((uint32_t)v[4 * j + 1] << 8) | ((uint32_t)v[4 * j + 2] << 16) | ((uint32_t)v[4 * j + 3] << 24);
    } else {
#pragma unroll
        for (int j = 0; j < 12; ++j)
            if (j < nb) dst[base + j] = (uint8_t)v[j];
    }
}

// cv2.borderInterpolate(p, n, BORDER_REFLECT_101)
__device__ __forceinline__ int reflect101(int p, int n) {
    if (n == 1) return 0;
    while ((unsigned)p >= (unsigned)n) p = p < 0 ? -p : 2 * (n - 1) - p;
    return p;
}

#define BOX_TW 64                                          // output pixels per tile row
#define BOX_TH 16                                          // output rows per tile
#define BOX_R 3                                            // the largest radius (k = 7)
#define BOX_IN_ROWS (BOX_TH + 2 * BOX_R)
#define BOX_IN_STRIDE 216                                  // >= 3 (lead) + 3 * (BOX_TW + 2 * BOX_R) + 3, a multiple of 4
#define BOX_OUT_B (3 * BOX_TW)

// grid (ceil(max_w / 64), ceil(max_h / 16), nimg).  The input rows of a tile (window rows reflected) go to LDS as aligned
// dwords of the packed buffer (byte loads only where a dword would leave [0, nbytes)), reflected border columns after them
// as bytes; separable integer sums (running windows) in LDS; the tile is written back as aligned dwords (bytes at the
// ends of each row segment).
__global__ __launch_bounds__(256) void aug_box_kernel(const uint8_t* __restrict__ src, const int* __restrict__ params2,
                                                      uint8_t* __restrict__ dst, long long nbytes) {
    __shared__ uint32_t in4[BOX_IN_ROWS * BOX_IN_STRIDE / 4];
    __shared__ uint16_t hs[BOX_IN_ROWS * BOX_OUT_B];
    __shared__ uint32_t out4[BOX_TH * BOX_OUT_B / 4 + 1];
    __shared__ int lead[BOX_IN_ROWS];
    uint8_t* in = (uint8_t*)in4;
    uint8_t* ob = (uint8_t*)out4;
    const Aug2Img a = load_img2(params2, blockIdx.z);
    const int x0 = blockIdx.x * BOX_TW, y0 = blockIdx.y * BOX_TH;
    if (x0 >= a.w || y0 >= a.h) return;                    // (uniform over the workgroup)
    const int tw = min(BOX_TW, a.w - x0), th = min(BOX_TH, a.h - y0);
    const int k = (a.flags & AUG2_BOX) ? a.k : 1, r = k >> 1;
    const int nrow = th + 2 * r, ncol = tw + 2 * r;
    const int xa = max(x0 - r, 0), xb = min(x0 + tw + r, a.w);   // columns inside the image
    const int t = threadIdx.x;

    // 1. rows y0 - r .. y0 + th + r - 1 (reflected), columns xa .. xb - 1: LDS byte (x - (x0 - r)) * 3 + c + lead[i]
    if (t < nrow) {
        const long long gv = ((long long)a.off + (long long)reflect101(y0 - r + t, a.h) * a.w + (x0 - r)) * 3;
        lead[t] = (int)(gv - (gv & ~3ll));
    }
    {
        const int nd = (3 * (xb - xa) + 6 + 3) >> 2;           // dwords per row, an upper bound
        for (int i = t; i < nrow * nd; i += 256) {
            const int row = i / nd, j = i - row * nd;
            const long long rb = ((long long)a.off + (long long)reflect101(y0 - r + row, a.h) * a.w) * 3;
            const long long gv = rb + (long long)(x0 - r) * 3, g0 = (rb + 3ll * xa) & ~3ll, g1 = rb + 3ll * xb;
            const long long G = g0 + 4ll * j;
            if (G >= g1) continue;
            const int pos = row * BOX_IN_STRIDE + (int)(G - (gv & ~3ll));
            if (G + 4 <= nbytes) {
                in4[pos >> 2] = *(const uint32_t*)(src + G);
            } else {
                for (int q = 0; q < 4 && G + q < nbytes; ++q) in[pos + q] = src[G + q];
            }
        }
    }
    __syncthreads();
    if (r) {                                                // columns outside the image: reflect-101
        for (int i = t; i < nrow * 2 * r * 3; i += 256) {
            const int row = i / (6 * r), rest = i - row * 6 * r, q0 = rest / 3, c = rest - q0 * 3;
            const int q = q0 < r ? q0 : ncol - 2 * r + q0;     // (left r columns, then right r columns)
            const int x = x0 - r + q;
            if (x >= 0 && x < a.w) continue;
            const long long rb = ((long long)a.off + (long long)reflect101(y0 - r + row, a.h) * a.w) * 3;
            in[row * BOX_IN_STRIDE + lead[row] + q * 3 + c] = src[rb + 3ll * reflect101(x, a.w) + c];
        }
        __syncthreads();
    }

    // 2. horizontal window sums: one (row, channel, run of 16 pixels) per task
    for (int i = t; i < nrow * 3 * (BOX_TW / 16); i += 256) {
        const int row = i / (3 * (BOX_TW / 16)), rest = i - row * 3 * (BOX_TW / 16), c = rest >> 2, p0 = (rest & 3) * 16;
        if (p0 >= tw) continue;
        const uint8_t* s = in + row * BOX_IN_STRIDE + lead[row] + c;
        uint16_t* h = hs + row * BOX_OUT_B + c;
        int sum = 0;
        for (int d = 0; d <= 2 * r; ++d) sum += s[(p0 + d) * 3];
        const int p1 = min(p0 + 16, tw);
        for (int p = p0; p < p1; ++p) {
            h[p * 3] = (uint16_t)sum;
            if (p + 1 < p1) sum += (int)s[(p + 2 * r + 1) * 3] - (int)s[p * 3];
        }
    }
    __syncthreads();

    // 3. vertical window sums and the rounded mean: one output byte column per task
    const int kk = k * k, half = (kk - 1) >> 1;
    for (int j = t; j < 3 * tw; j += 256) {
        int sum = 0;
        for (int d = 0; d <= 2 * r; ++d) sum += hs[d * BOX_OUT_B + j];
        for (int y = 0; y < th; ++y) {
            ob[y * BOX_OUT_B + j] = (uint8_t)((unsigned)(sum + half) / (unsigned)kk);
            if (y + 1 < th) sum += (int)hs[(y + 2 * r + 1) * BOX_OUT_B + j] - (int)hs[y * BOX_OUT_B + j];
        }
    }
    __syncthreads();

    // 4. store: aligned dwords inside each row segment, single bytes at its ends
    for (int i = t; i < th * (BOX_OUT_B / 4 + 2); i += 256) {
        const int y = i / (BOX_OUT_B / 4 + 2), j = i - y * (BOX_OUT_B / 4 + 2);
        const long long gs = ((long long)a.off + (long long)(y0 + y) * a.w + x0) * 3, ge = gs + 3 * tw;
        const long long G = (gs & ~3ll) + 4ll * j;
        if (G >= ge) continue;
        const int o = (int)(G - gs);                            // LDS byte of global byte G (may be -1 .. -3 at the head)
        if (G >= gs && G + 4 <= ge) {
            const int w0 = y * (BOX_OUT_B / 4) + (o >> 2), sh = o & 3;
            const uint32_t lo = out4[w0], hi = out4[w0 + 1];
            *(uint32_t*)(dst + G) = sh ? (uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * sh)) : lo;
        } else {
            for (int q = 0; q < 4; ++q)
                if (G + q >= gs && G + q < ge) dst[G + q] = ob[y * BOX_OUT_B + o + q];
        }
    }
}

extern "C" int radet_augment_hsv_noise(const uint8_t* src, const int* params2, uint8_t* dst, int nimg, int max_px, void* stream) {
    if (nimg < 0 || max_px < 0 || ((uintptr_t)src & 3) || ((uintptr_t)dst & 3)) return RADET_ERR_ARG;
    if (nimg == 0 || max_px == 0) return RADET_OK;
    const int groups = (max_px + 3) / 4;
    hipLaunchKernelGGL(aug_hsv_noise_kernel, dim3((groups + 255) / 256, nimg), dim3(256), 0, (hipStream_t)stream, src, params2, dst);
    return radet_check_launch();
}

extern "C" int radet_augment_box(const uint8_t* src, const int* params2, uint8_t* dst, size_t nbytes, int nimg, int max_h, int max_w,
                                 void* stream) {
    if (nimg < 0 || max_h < 0 || max_w < 0 || max_h > AUG_MAX_W || max_w > AUG_MAX_W || ((uintptr_t)src & 3) || ((uintptr_t)dst & 3))
        return RADET_ERR_ARG;
    if (nimg == 0 || max_h == 0 || max_w == 0) return RADET_OK;
    hipLaunchKernelGGL(aug_box_kernel, dim3((max_w + BOX_TW - 1) / BOX_TW, (max_h + BOX_TH - 1) / BOX_TH, nimg), dim3(256), 0,
                       (hipStream_t)stream, src, params2, dst, (long long)nbytes);
    return radet_check_launch();
}
