// Per-pixel device helpers shared by imgproc.hip (radet_resize_linear_u8 / _f), augment.hip (radet_augment_finish) and
// preprocess.hip (radet_preprocess_frames): one definition of the 8-bit INTER_LINEAR arithmetic and of the Normalize / pad
// store, so that the one-launch frame preparation equals resize -> finish bit for bit by construction; and the view row
// that imgproc.hip and masks.hip share.
#pragma once
#include "common.h"
#include "../../include/radet_hip.h"

// source index + fraction of destination index d (cv::resize, INTER_LINEAR): f = (d + 0.5) * scale - 0.5 in float
__device__ __forceinline__ void lin_coord(int d, double scale, int n, bool clamp_frac, int* s, float* f) {
    float fx = (float)(((double)d + 0.5) * scale - 0.5);
    int sx = (int)floorf(fx);
    fx -= (float)sx;
    if (clamp_frac) {                                           // x direction: coefficients are reset at the borders
        if (sx < 0) { fx = 0.f; sx = 0; }
        if (sx >= n - 1) { fx = 0.f; sx = n - 1; }
    }
    *s = sx;
    *f = fx;
}

__device__ __forceinline__ int clip_row(int y, int n) { return y < 0 ? 0 : (y < n ? y : n - 1); }

__device__ __forceinline__ int coef_fix(float c) {             // saturate_cast<short>(c * 2048): round to nearest even
    int v = __float2int_rn(c * 2048.f);
    return v > 32767 ? 32767 : (v < -32768 ? -32768 : v);
}

// the four taps of destination pixel (dy, dx) of an sh x sw -> dh x dw resize: columns sx / x1, rows y0 / y1 (all inside
// the source) and their 11-bit fixed-point coefficients
struct LinTaps { int sx, x1, y0, y1, a0, a1, b0, b1; };

__device__ __forceinline__ LinTaps lin_taps_u8(int dy, int dx, int sh, int sw, int dh, int dw) {
    const double scale_x = 1.0 / ((double)dw / (double)sw), scale_y = 1.0 / ((double)dh / (double)sh);
    LinTaps t;
    int sy;
    float fx, fy;
    lin_coord(dx, scale_x, sw, true, &t.sx, &fx);
    lin_coord(dy, scale_y, sh, false, &sy, &fy);
    t.a0 = coef_fix(1.f - fx); t.a1 = coef_fix(fx); t.b0 = coef_fix(1.f - fy); t.b1 = coef_fix(fy);
    t.y0 = clip_row(sy, sh); t.y1 = clip_row(sy + 1, sh);
    t.x1 = t.sx + 1 < sw ? t.sx + 1 : t.sx;                     // a1 == 0 whenever sx is the last column
    return t;
}

// one channel from its four source bytes (p00 p01 = row y0 at sx, x1; p10 p11 = row y1): the horizontal pass kept as
// integers, the vertical pass ((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2, saturated to 8 bits
__device__ __forceinline__ int lin_blend_u8(int p00, int p01, int p10, int p11, const LinTaps& t) {
    const int h0 = p00 * t.a0 + p01 * t.a1;
    const int h1 = p10 * t.a0 + p11 * t.a1;
    const int v = (((t.b0 * (h0 >> 4)) >> 16) + ((t.b1 * (h1 >> 4)) >> 16) + 2) >> 2;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// One view row (include/radet_hip.h RADET_VIEW_INTS): the wh x ww window at (wy0, wx0) of the source, resized to a virtual
// Hr x Wr, of which the h x w window at (oy, ox) is written.  load_view is false for a row with bad geometry.
struct View { int Hr, Wr, wy0, wx0, wh, ww, oy, ox, h, w, flip; unsigned fill; };

__device__ __forceinline__ bool load_view(const int* __restrict__ rows, size_t n, View* v) {
    const int* d = rows + n * RADET_VIEW_INTS;
    *v = {d[0], d[1], d[2], d[3], d[4], d[5], d[6], d[7], d[8], d[9], d[10], (unsigned)d[11]};
    return v->Hr > 0 && v->Wr > 0 && v->wh > 0 && v->ww > 0 && (long long)v->wy0 + v->wh <= 0x7FFFFFFFLL &&
           (long long)v->wx0 + v->ww <= 0x7FFFFFFFLL && v->oy >= 0 && v->ox >= 0 && v->h >= 0 && v->w >= 0 &&
           v->oy <= v->Hr - v->h && v->ox <= v->Wr - v->w;
}

// Normalize of one u8 BGR pixel v into the three planes at o (optional BGR->RGB, (q - mean) * stdinv in fp32), and Pad's zeros
__device__ __forceinline__ void norm_store(float* __restrict__ o, size_t plane, const int v[3], bool rgb, float m0, float m1,
                                           float m2, float s0, float s1, float s2) {
    const float q0 = (float)(rgb ? v[2] : v[0]), q1 = (float)v[1], q2 = (float)(rgb ? v[0] : v[2]);
    o[0] = (q0 - m0) * s0;
    o[plane] = (q1 - m1) * s1;
    o[2 * plane] = (q2 - m2) * s2;
}

__device__ __forceinline__ void zero_store(float* __restrict__ o, size_t plane) {
    o[0] = 0.f; o[plane] = 0.f; o[2 * plane] = 0.f;
}
