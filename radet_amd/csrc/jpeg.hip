// Baseline JPEG decoding of a batch on the device, byte for byte what libjpeg's default decompressor gives (slow-integer
// IDCT, fancy chroma upsampling, 16-bit fixed-point YCbCr -> RGB): three launches whatever the batch size.
//   jpeg_entropy   one lane per index segment (radet_jpeg_index wrote the entry points): Huffman symbols -> int16
//                  coefficients in natural order, [block][64], every block written once
//   jpeg_idct      one lane per 8x8 block: dequantise, jidctint's two passes, level shift, range limit -> u8 planes
//                  padded to whole MCUs
//   jpeg_convert   four pixels per lane: h2v1 / h2v2 triangle upsampling over the component's real size, colour
//                  conversion, B G R bytes into the packed source buffer of radet_resize_linear_u8
// Descriptors: include/radet_hip.h.  Plain C++ and vector stores only.
#include "common.h"
#include "jpeg_common.h"
#include "radet_hip.h"

namespace {

__constant__ const uint8_t kNatural[64] = RJ_ZIGZAG;
constexpr int kLanes = 64;           // one wave per workgroup: the lanes of a workgroup share an image's tables
constexpr int kBlkStride = 33;       // dwords per lane's block in LDS (32 + 1: lanes on distinct banks)

struct Img {
    int file_off, scan_hi, W, H, ncomp, hs, vs, mcux, mcuy, coef_off[3], plane_off[3], dst_off, row0, nrows;
};

__device__ inline Img load_img(const int* d) {
    Img g;
    g.file_off = d[0]; g.scan_hi = d[1]; g.W = d[2]; g.H = d[3]; g.ncomp = d[4]; g.hs = d[5]; g.vs = d[6]; g.mcux = d[7]; g.mcuy = d[8];
    for (int c = 0; c < 3; ++c) { g.coef_off[c] = d[9 + c]; g.plane_off[c] = d[12 + c]; }
    g.dst_off = d[15]; g.row0 = d[16]; g.nrows = d[17];
    return g;
}

__global__ __launch_bounds__(kLanes) void jpeg_entropy_kernel(const uint8_t* __restrict__ files, const int* __restrict__ desc,
                                                              const int* __restrict__ wgs, const uint4* __restrict__ huff,
                                                              const int* __restrict__ rows, int n_rows, uint4* __restrict__ coef,
                                                              int* __restrict__ err) {
    __shared__ __attribute__((aligned(16))) RjHuff sh[6];
    __shared__ uint32_t blk[kLanes * kBlkStride];
    const int tid = threadIdx.x, img = wgs[2 * blockIdx.x], first = wgs[2 * blockIdx.x + 1];
    const Img g = load_img(desc + (size_t)img * JPEG_DESC_INTS);
    {
        constexpr int per = RJ_HUFF_BYTES / 16;
        const uint4* src = huff + (size_t)img * 6 * per;
        uint4* dst = reinterpret_cast<uint4*>(sh);
        for (int i = tid; i < 2 * g.ncomp * per; i += kLanes) dst[i] = src[i];
    }
    uint32_t* mine = blk + tid * kBlkStride;
    for (int i = 0; i < 32; ++i) mine[i] = 0;
    __syncthreads();
    const int r = first + tid;
    if (r >= g.row0 + g.nrows || r >= n_rows || g.ncomp < 1 || g.ncomp > 3) return;
    const int* row = rows + (size_t)r * RJ_ROW_INTS;
    const int total = g.mcux * g.mcuy;
    const int m0 = row[RJ_MCU0], nm = row[RJ_NMCU];
    if (row[RJ_OFF] < 0 || row[RJ_OFF] > g.scan_hi || m0 < 0 || nm < 0 || m0 + nm > total) { atomicOr(err + img, RJ_E_COUNT); return; }
    RjBits b;
    rj_start(&b, files + g.file_off, row[RJ_OFF], g.scan_hi);
    rj_fill(&b);
    b.n -= row[RJ_BIT] & 7;
    int pred[3] = {row[RJ_PRED], row[RJ_PRED + 1], row[RJ_PRED + 2]};
    int bad = 0;
    for (int m = m0; m < m0 + nm && !bad; ++m) {
        const int mx = m % g.mcux, my = m / g.mcux;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (c >= g.ncomp) break;
            const int h = c ? 1 : g.hs, v = c ? 1 : g.vs;
            for (int k = 0; k < h * v && !bad; ++k) {
                rj_fill(&b);
                int s = rj_symbol(&b, &sh[2 * c]);
                if (s < 0 || s > 15) { bad = RJ_E_CODE; break; }
                pred[c] += rj_extend(rj_take(&b, s), s);
                reinterpret_cast<int16_t*>(mine)[0] = (int16_t)pred[c];
                for (int i = 1; i < 64;) {
                    rj_fill(&b);
                    const int rs = rj_symbol(&b, &sh[2 * c + 1]);
                    if (rs < 0) { bad = RJ_E_CODE; break; }
                    s = rs & 15;
                    if (s == 0) {
                        if ((rs >> 4) != 15) break;
                        i += 16;
                        continue;
                    }
                    i += rs >> 4;
                    if (i > 63) { bad = RJ_E_INDEX; break; }
                    reinterpret_cast<int16_t*>(mine)[kNatural[i]] = (int16_t)rj_extend(rj_take(&b, s), s);
                    ++i;
                }
                if (b.n < b.fake) bad = RJ_E_EARLY;
                // the block leaves the lane once, zeros included; the LDS copy is cleared for the next one
                const int by = my * v + k / h, bx = mx * h + k % h;
                uint4* out = coef + ((size_t)g.coef_off[c] + (size_t)by * (g.mcux * h) + bx) * 8;
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    out[q] = make_uint4(mine[4 * q], mine[4 * q + 1], mine[4 * q + 2], mine[4 * q + 3]);
                    mine[4 * q] = mine[4 * q + 1] = mine[4 * q + 2] = mine[4 * q + 3] = 0;
                }
            }
            if (bad) break;
        }
    }
    if (!bad && rj_position(&b) != row[RJ_END]) bad = RJ_E_END;
    if (bad) atomicOr(err + img, bad);
}

// jidctint.c's 1-D pass over eight values; `shift` is CONST_BITS - PASS1_BITS (columns) or CONST_BITS + PASS1_BITS + 3 (rows).
// The sums are 64 bits wide, as libjpeg's (INT32 = long): a coefficient is an int16 and a quantiser at most 255, so no
// stream, however extreme, overflows them; the workspace between the passes is int, as libjpeg's.
__device__ inline void idct8(int& v0, int& v1, int& v2, int& v3, int& v4, int& v5, int& v6, int& v7, int shift) {
    typedef long long L;
    L z1 = ((L)v2 + v6) * 4433;
    L tmp2 = z1 + (L)v6 * -15137, tmp3 = z1 + (L)v2 * 6270;
    L tmp0 = ((L)v0 + v4) * 8192, tmp1 = ((L)v0 - v4) * 8192;
    const L tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = v7; tmp1 = v5; tmp2 = v3; tmp3 = v1;
    z1 = tmp0 + tmp3;
    L z2 = tmp1 + tmp2, z3 = tmp0 + tmp2, z4 = tmp1 + tmp3;
    const L z5 = (z3 + z4) * 9633;
    tmp0 *= 2446; tmp1 *= 16819; tmp2 *= 25172; tmp3 *= 12299;
    z1 *= -7373; z2 *= -20995; z3 *= -16069; z4 *= -3196;
    z3 += z5; z4 += z5;
    tmp0 += z1 + z3; tmp1 += z2 + z4; tmp2 += z2 + z3; tmp3 += z1 + z4;
    const L rnd = 1LL << (shift - 1);
    v0 = (int)((tmp10 + tmp3 + rnd) >> shift); v7 = (int)((tmp10 - tmp3 + rnd) >> shift);
    v1 = (int)((tmp11 + tmp2 + rnd) >> shift); v6 = (int)((tmp11 - tmp2 + rnd) >> shift);
    v2 = (int)((tmp12 + tmp1 + rnd) >> shift); v5 = (int)((tmp12 - tmp1 + rnd) >> shift);
    v3 = (int)((tmp13 + tmp0 + rnd) >> shift); v4 = (int)((tmp13 - tmp0 + rnd) >> shift);
}

// libjpeg's range_limit table after the level shift: exact also where it wraps
__device__ inline unsigned range_limit(int v) {
    v &= 1023;
    return v < 128 ? v + 128 : v < 512 ? 255 : v < 896 ? 0 : v - 896;
}

__global__ __launch_bounds__(256) void jpeg_idct_kernel(const int* __restrict__ desc, const uint16_t* __restrict__ quant,
                                                        const uint4* __restrict__ coef, uint8_t* __restrict__ planes) {
    const int img = blockIdx.y / 3, c = blockIdx.y % 3;
    const Img g = load_img(desc + (size_t)img * JPEG_DESC_INTS);
    if (c >= g.ncomp) return;
    const int bw = g.mcux * (c ? 1 : g.hs), bh = g.mcuy * (c ? 1 : g.vs);
    const int blkid = blockIdx.x * 256 + threadIdx.x;
    if (blkid >= bw * bh) return;
    const uint4* in = coef + ((size_t)g.coef_off[c] + blkid) * 8;
    const uint4* q = reinterpret_cast<const uint4*>(quant + ((size_t)img * 3 + c) * 64);
    int ws[64];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const uint4 a = in[r], b = q[r];
        const uint32_t aw[4] = {a.x, a.y, a.z, a.w}, bw_[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            ws[8 * r + 2 * j] = (int)(int16_t)(aw[j] & 0xFFFF) * (int)(bw_[j] & 0xFFFF);
            ws[8 * r + 2 * j + 1] = (int)(int16_t)(aw[j] >> 16) * (int)(bw_[j] >> 16);
        }
    }
#pragma unroll
    for (int x = 0; x < 8; ++x)
        idct8(ws[x], ws[8 + x], ws[16 + x], ws[24 + x], ws[32 + x], ws[40 + x], ws[48 + x], ws[56 + x], 11);
    const int pw = bw * 8;
    uint8_t* out = planes + g.plane_off[c] + (size_t)(blkid / bw) * 8 * pw + (blkid % bw) * 8;
#pragma unroll
    for (int y = 0; y < 8; ++y) {
        idct8(ws[8 * y], ws[8 * y + 1], ws[8 * y + 2], ws[8 * y + 3], ws[8 * y + 4], ws[8 * y + 5], ws[8 * y + 6], ws[8 * y + 7], 18);
        uint2 o;
        o.x = range_limit(ws[8 * y]) | range_limit(ws[8 * y + 1]) << 8 | range_limit(ws[8 * y + 2]) << 16 | range_limit(ws[8 * y + 3]) << 24;
        o.y = range_limit(ws[8 * y + 4]) | range_limit(ws[8 * y + 5]) << 8 | range_limit(ws[8 * y + 6]) << 16 | range_limit(ws[8 * y + 7]) << 24;
        *reinterpret_cast<uint2*>(out + (size_t)y * pw) = o;
    }
}

// one chroma sample at full resolution (jdsample.c: fullsize copy, h2v1_fancy_upsample, h2v2_fancy_upsample); cw x ch is the
// component's real downsampled size, pw its padded row length
__device__ inline int chroma_at(const uint8_t* __restrict__ p, int pw, int cw, int ch, int y, int x, int hs, int vs) {
    if (hs == 1) return p[(size_t)y * pw + x];
    const int i = x >> 1;
    if (vs == 1) {
        const uint8_t* in = p + (size_t)y * pw;
        if (x & 1) return i == cw - 1 ? in[i] : (3 * in[i] + in[i + 1] + 2) >> 2;
        return i == 0 ? in[0] : (3 * in[i] + in[i - 1] + 1) >> 2;
    }
    const int r = y >> 1;
    const int f = min(max((y & 1) ? r + 1 : r - 1, 0), ch - 1);
    const uint8_t* nr = p + (size_t)r * pw;
    const uint8_t* fr = p + (size_t)f * pw;
    const int s = 3 * nr[i] + fr[i];
    if (x & 1) return i == cw - 1 ? (4 * s + 7) >> 4 : (3 * s + 3 * nr[i + 1] + fr[i + 1] + 7) >> 4;
    return i == 0 ? (4 * s + 8) >> 4 : (3 * s + 3 * nr[i - 1] + fr[i - 1] + 8) >> 4;
}

__device__ inline unsigned clamp255(int v) { return (unsigned)min(max(v, 0), 255); }

__global__ __launch_bounds__(256) void jpeg_convert_kernel(const int* __restrict__ desc, const uint8_t* __restrict__ planes,
                                                           uint8_t* __restrict__ dst) {
    const int img = blockIdx.y;
    const Img g = load_img(desc + (size_t)img * JPEG_DESC_INTS);
    const int npx = g.W * g.H, p0 = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (p0 >= npx) return;
    const int pw0 = g.mcux * g.hs * 8, pwc = g.mcux * 8;
    const int cw = (g.W + g.hs - 1) / g.hs, ch = (g.H + g.vs - 1) / g.vs;
    const uint8_t* Y = planes + g.plane_off[0];
    uint8_t px[12];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int p = min(p0 + j, npx - 1), y = p / g.W, x = p % g.W;
        const int yy = Y[(size_t)y * pw0 + x];
        int cb = 0, cr = 0;
        if (g.ncomp == 3) {
            cb = chroma_at(planes + g.plane_off[1], pwc, cw, ch, y, x, g.hs, g.vs) - 128;
            cr = chroma_at(planes + g.plane_off[2], pwc, cw, ch, y, x, g.hs, g.vs) - 128;
        }
        px[3 * j] = (uint8_t)clamp255(yy + ((116130 * cb + 32768) >> 16));
        px[3 * j + 1] = (uint8_t)clamp255(yy + ((-22554 * cb + 32768 - 46802 * cr) >> 16));
        px[3 * j + 2] = (uint8_t)clamp255(yy + ((91881 * cr + 32768) >> 16));
    }
    uint8_t* out = dst + ((size_t)g.dst_off + p0) * 3;
    if (p0 + 4 <= npx && (g.dst_off & 3) == 0) {
        // twelve bytes at a multiple of twelve from a dword-aligned buffer: three aligned dwords
        uint32_t* o = reinterpret_cast<uint32_t*>(out);
#pragma unroll
        for (int k = 0; k < 3; ++k)
            o[k] = px[4 * k] | (uint32_t)px[4 * k + 1] << 8 | (uint32_t)px[4 * k + 2] << 16 | (uint32_t)px[4 * k + 3] << 24;
    } else {
        const int n = min(4, npx - p0) * 3;
#pragma unroll
        for (int k = 0; k < 12; ++k)
            if (k < n) out[k] = px[k];
    }
}

}  // namespace

extern "C" int radet_jpeg_decode(const uint8_t* files, const int* desc, int nimg, const int* wgs, int n_wg, const void* huff,
                                 const uint16_t* quant, const int* rows, int n_rows, int16_t* coef, uint8_t* planes, uint8_t* dst,
                                 int* err, int max_blocks, int max_px, int stages, void* stream) {
    if (nimg <= 0) return 0;
    if (!files || !desc || !wgs || !huff || !quant || !rows || !coef || !planes || !dst || !err || n_wg <= 0 || n_rows <= 0 ||
        max_blocks <= 0 || max_px <= 0 || nimg > 21845)
        return -1;
    if ((reinterpret_cast<uintptr_t>(huff) | reinterpret_cast<uintptr_t>(quant) | reinterpret_cast<uintptr_t>(coef)) & 15) return -1;
    if ((reinterpret_cast<uintptr_t>(planes) & 7) | (reinterpret_cast<uintptr_t>(dst) & 3)) return -1;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (stages & 1)
        hipLaunchKernelGGL(jpeg_entropy_kernel, dim3(n_wg), dim3(kLanes), 0, s, files, desc, wgs, static_cast<const uint4*>(huff), rows,
                           n_rows, reinterpret_cast<uint4*>(coef), err);
    if (stages & 2)
        hipLaunchKernelGGL(jpeg_idct_kernel, dim3((max_blocks + 255) / 256, nimg * 3), dim3(256), 0, s, desc, quant,
                           reinterpret_cast<const uint4*>(coef), planes);
    if (stages & 4)
        hipLaunchKernelGGL(jpeg_convert_kernel, dim3((max_px / 4 + 256) / 256, nimg), dim3(256), 0, s, desc, planes, dst);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}
