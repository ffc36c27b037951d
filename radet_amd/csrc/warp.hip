// Affine augmentation (Rotate / Shear / Translate of radet/datasets/pipelines/auto_augment.py: mmcv.imrotate / imshear /
// imtranslate -> cv2.warpAffine, INTER_LINEAR, BORDER_CONSTANT) for a batch of packed u8 images of mixed sizes, and for the
// instance masks that go with them (one channel, fill 0), in ONE launch per entry rank.
//
// cv2 is neither in the reference tree nor in this image, so this restates OpenCV's classic fixed-point path
// (imgwarp.cpp: warpAffine's coordinate tables + remapBilinear): PARITY UNPINNED against cv2 itself -- newer OpenCV
// releases ship a float SIMD warpAffine whose results differ; the arithmetic is pinned by tests/_affine_ref.py (integer
// NumPy, same formulas).  With the inverse matrix M (the host inverts the forward one in double, as cv2 does), AB = 1024:
//      X0 = round((M1 * y + M2) * AB) + 16,  Y0 = round((M4 * y + M5) * AB) + 16        (round: half to even, cvRound)
//      X = (X0 + round(M0 * x * AB)) >> 5,   Y = (Y0 + round(M3 * x * AB)) >> 5
//      sx = X >> 5, sy = Y >> 5, fx = X & 31, fy = Y & 31
//      dst = ((32 - fx)(32 - fy) p00 + fx (32 - fy) p01 + (32 - fx) fy p10 + fx fy p11 + 512) >> 10  per channel,
// a tap outside the image being the fill byte of its channel (cv2's 15-bit weight table is these products times 32, so
// its fix-up step never fires and (sum * 32 + 2^14) >> 15 is the line above).  Every double product and sum is rounded on
// its own (__dmul_rn / __dadd_rn; the Makefile also compiles with -ffp-contract=off).  The host refuses matrices whose
// coordinates leave 32 bits (ImagePipeline); here the sums are formed in 64 bits, so a row that breaks that reads fill
// or wrong pixels but never outside the image.
//
// One row of WARP_DESC_INTS ints per image (include/radet_hip.h).  grid (ceil(max h * w / 256), rows): one output pixel
// (all channels) per thread, as resize_u8_kernel; byte stores of the packed pixels.  A gather, memory-bound: 4 taps of C
// bytes, mostly shared with the neighbouring lanes, and C stored bytes per pixel.  No LDS, no scratch.
#include "common.h"
#include "../../include/radet_hip.h"

__device__ __forceinline__ double warp_desc_f64(const int* d, int k) {
    const unsigned long long lo = (unsigned)d[WARP_DESC_MATRIX + 2 * k], hi = (unsigned)d[WARP_DESC_MATRIX + 2 * k + 1];
    return __longlong_as_double((long long)(lo | hi << 32));
}

template <int C>
__global__ __launch_bounds__(256) void warp_affine_u8_kernel(const uint8_t* __restrict__ src, long long src_px,
                                                             uint8_t* __restrict__ dst, long long dst_px,
                                                             const int* __restrict__ desc) {
    const int* d = desc + (size_t)WARP_DESC_INTS * blockIdx.y;
    const int so = d[WARP_DESC_SRC], dof = d[WARP_DESC_DST], h = d[WARP_DESC_H], w = d[WARP_DESC_W];
    if (h <= 0 || w <= 0 || so < 0 || dof < 0 || d[WARP_DESC_CHANNELS] != C) return;
    const long long px = (long long)h * w;
    if (so + px > src_px || dof + px > dst_px) return;              // (a row that leaves its buffer is not touched)
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p >= px) return;
    const uint8_t* s = src + (size_t)so * C;
    uint8_t* o = dst + ((size_t)dof + (size_t)p) * C;
    if (d[WARP_DESC_FLAGS] & WARP_SKIP) {
#pragma unroll
        for (int c = 0; c < C; ++c) o[c] = s[(size_t)p * C + c];
        return;
    }
    const int y = (int)(p / w), x = (int)(p - (long long)y * w);
    const double AB = 1024.0;
    const double m0 = warp_desc_f64(d, 0), m1 = warp_desc_f64(d, 1), m2 = warp_desc_f64(d, 2);
    const double m3 = warp_desc_f64(d, 3), m4 = warp_desc_f64(d, 4), m5 = warp_desc_f64(d, 5);
    const long long X0 = (long long)__double2int_rn(__dmul_rn(__dadd_rn(__dmul_rn(m1, (double)y), m2), AB)) + 16;
    const long long Y0 = (long long)__double2int_rn(__dmul_rn(__dadd_rn(__dmul_rn(m4, (double)y), m5), AB)) + 16;
    const long long X = (X0 + (long long)__double2int_rn(__dmul_rn(__dmul_rn(m0, (double)x), AB))) >> 5;
    const long long Y = (Y0 + (long long)__double2int_rn(__dmul_rn(__dmul_rn(m3, (double)x), AB))) >> 5;
    const long long sx = X >> 5, sy = Y >> 5;
    const int fx = (int)(X & 31), fy = (int)(Y & 31);
    const int w00 = (32 - fx) * (32 - fy), w01 = fx * (32 - fy), w10 = (32 - fx) * fy, w11 = fx * fy;
    const bool iy0 = sy >= 0 && sy < h, iy1 = sy + 1 >= 0 && sy + 1 < h;
    const bool ix0 = sx >= 0 && sx < w, ix1 = sx + 1 >= 0 && sx + 1 < w;
    const uint8_t* r0 = s + (size_t)(iy0 ? sy : 0) * w * C;
    const uint8_t* r1 = s + (size_t)(iy1 ? sy + 1 : 0) * w * C;
    const size_t c0 = (size_t)(ix0 ? sx : 0) * C, c1 = (size_t)(ix1 ? sx + 1 : 0) * C;
    const unsigned fill = (unsigned)d[WARP_DESC_FILL];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const int f = (int)((fill >> (8 * c)) & 0xFFu);
        const int p00 = iy0 && ix0 ? r0[c0 + c] : f, p01 = iy0 && ix1 ? r0[c1 + c] : f;
        const int p10 = iy1 && ix0 ? r1[c0 + c] : f, p11 = iy1 && ix1 ? r1[c1 + c] : f;
        o[c] = (uint8_t)((w00 * p00 + w01 * p01 + w10 * p10 + w11 * p11 + 512) >> 10);
    }
}

extern "C" int radet_warp_affine_u8(const uint8_t* src, size_t src_px, uint8_t* dst, size_t dst_px, const int* desc, int nimg,
                                    int max_px, int channels, void* stream) {
    if (nimg < 0 || max_px < 0 || (channels != 1 && channels != 3) || nimg > 65535) return RADET_ERR_ARG;
    if (nimg == 0 || max_px == 0) return RADET_OK;
    if (!src || !dst || !desc || src == dst || ((uintptr_t)desc & 3) || max_px > 0x7FFFFFFF - 255) return RADET_ERR_ARG;
    if (src_px > 0x7FFFFFFFull || dst_px > 0x7FFFFFFFull) return RADET_ERR_ARG;      // (pixel offsets are ints)
    const dim3 grid((max_px + 255) / 256, nimg);
    if (channels == 3)
        hipLaunchKernelGGL(warp_affine_u8_kernel<3>, grid, dim3(256), 0, (hipStream_t)stream, src, (long long)src_px, dst,
                           (long long)dst_px, desc);
    else
        hipLaunchKernelGGL(warp_affine_u8_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, src, (long long)src_px, dst,
                           (long long)dst_px, desc);
    return radet_check_launch();
}
