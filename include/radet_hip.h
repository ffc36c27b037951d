/* radet_hip.h -- C ABI of libradet_hip.so, the MI355X (gfx950) implementation of RADet's detector hot path.
 *
 * Every entry point: plain pointers (DEVICE memory unless stated "host"), sizes, and a `void* stream`
 * (hipStream_t; NULL = default stream).  Stream-ordered, no allocation, no host synchronisation
 * inside; workspaces are supplied by the caller.  Return value: 0 = ok, -1 = bad argument, -2 = launch
 * failure.  Activations are NHWC fp32, several pyramid levels concatenated row-wise ("multi-level
 * buffer"): level l holds B images of Ho_l x Wo_l pixels starting at row out_row_off_l.
 *
 * seg_desc (host): nseg x 6 ints {Hi, Wi, Ho, Wo, in_row_off, out_row_off} per level.
 *
 * Each function names the reference interface it replaces (paths relative to /root/reference).
 */
#ifndef RADET_HIP_H
#define RADET_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- convolution stack: replaces torch.nn.Conv2d/BatchNorm2d(eval)/ReLU/residual-add behind
 *      radet/models/backbones/resnet.py:260-299,622-637, necks/fpn.py:170-221,
 *      dense_heads/atss_head.py:118-145 (cuDNN in the reference) ------------------------------- */

/* One convolution's parameter bundle for the batched fold / unfold kernels (device pointers). */
typedef struct RadetConvDesc {
    const float* w;        /* [Cout][Cin][KH][KW]  parameter (OIHW, state-dict layout) */
    const float* bias;     /* [Cout] conv bias or NULL */
    const float* bn_gamma; /* [Cout] or NULL (no BN) */
    const float* bn_beta;
    const float* bn_mean;
    const float* bn_var;
    float* wf;             /* [Cout][KH*KW][Cin]   folded weights (OHWI) for forward */
    float* wft;            /* [Cin][KH*KW][Cout]   transposed copy for dgrad, or NULL */
    float* bias_f;         /* [Cout] folded bias (BN shift or conv bias or 0) */
    const float* dwf_slabs;      /* [nsplit][Cout][KH*KW][Cin] wgrad partial slabs */
    const float* dbias_partials; /* [nsplit][Cout] or NULL */
    float* dw;             /* [Cout][Cin][KH][KW] gradient (OIHW) or NULL (frozen) */
    float* dbias;          /* [Cout] or NULL */
    float* dgamma;         /* [Cout] or NULL */
    float* dbeta;          /* [Cout] or NULL */
    int cout, cin, kh, kw;
    int nsplit;
    float eps;
    int wft_ld;            /* row stride of wft's last dim (>= Cout; zero-padded K for small heads), 0 = Cout */
    int wft_off;           /* column offset inside that padded row */
    int w16;               /* 1: wf / wft are bf16 buffers (bf16-storage mode); 2: bf16 plane triples (rows [3][Cin] resp.
                              [3][wft_ld], see "planes" below); 3: fp16 plane pairs (rows [2][Cin] resp. [2][wft_ld], see
                              "plane pairs" below; needs w_amax); bias_f stays fp32 */
    float* w_amax;         /* 64 words or NULL: amax slot (see RadetScales) of the folded weights, largest |wf|; zeroed and raised
                              by radet_fold_weights -- the weight operand's scale in the fp16 hi / lo arithmetic */
    float* wfq;            /* optional: a second copy of wf as fp16 plane pairs (rows [2][Cin], scaled by w_amax's power of two),
                              the weight operand of forward launches whose x arrives as plane pairs; or NULL */
    float* w_l1;           /* amax-style slot or NULL: largest L1 norm of a folded output channel, max_o sum |wf[o][.][.]| --
                              |conv output| <= amax(x) * it (+ |bias| + |addend|): the bound RadetScales.yq is scaled with */
    float* bias_amax;      /* amax-style slot or NULL: largest |bias_f| */
    float* w_l1t;          /* amax-style slot or NULL (round 6): largest L1 norm of a folded INPUT channel, max_c sum_{o,t} |wf[o][t][c]|
                              -- |dgrad output| <= amax(dy) * it: the bound a dgrad launch scales its pair output with */
} RadetConvDesc;

/* ---- amax slots (round 5, "fp16 hi / lo arithmetic").  The default fp32 conv arithmetic forms fp32-accurate products
 * from TWO fp16 numbers per operand element: t = x 2^e, hi = fp16(t), lo = fp16((t - hi) 2^11), and
 * x x' = 2^-(e + e') (hi hi' + 2^-11 (hi lo' + lo hi')) -- three v_mfma_f32_32x32x16_f16 per K = 16 step instead of the six
 * bf16 plane products of RADET_TILE_X3 (the dropped lo lo' term is <= 2^-24 relative; x = 2^-e (hi + 2^-11 lo) to 2^-23
 * relative for every element within 2^-27 of the tensor's largest).  fp16 has 5 exponent bits, so every operand tensor is
 * scaled by an exact power of two 2^e that puts its largest magnitude into [2^14, 2^15).  e comes from the tensor's "amax
 * slot": RADET_AMAX_WORDS = 64 32-bit words, 128 bytes apart (radet_amax_slot_words() = 2048 words = 8 KiB per slot, the
 * rest unused), of device memory whose LARGEST word is the bit pattern of a
 * non-negative float that is >= every |element| (the largest magnitude, or any bound on it), e = 141 - biased_exponent(slot)
 * (0 for a zero slot).  Slots are maintained by the kernels that WRITE a tensor: they raise one of the 64 words (chosen by
 * workgroup and wave: thousands of waves raising ONE address serialise) with atomicMax on the bit pattern -- order
 * independent, hence deterministic -- in conv epilogues (RadetScales.y_amax), the y_amax / dst_amax / dx_amax arguments of the
 * elementwise layer kernels and radet_absmax; or they store a bound they can derive before writing into word 0 (GroupNorm:
 * planes_amax of radet_gn_relu_fwd / _bwd with RADET_LAYER_PAIRS, radet_split_pairs; the other words must be zero).  The caller zeroes a slot before the first kernel of a step that
 * raises it.  Host struct of device pointers (each to a 64-word slot): */
#define RADET_AMAX_WORDS 64
typedef struct RadetScales {
    const void* x_amax;    /* slot of the GEMM's x operand (dgrad: dy; wgrad: dy) */
    const void* w_amax;    /* slot of the w operand (RadetConvDesc.w_amax; wgrad: the slot of x) */
    void* y_amax;          /* slot raised to the largest |y| stored, or NULL (works with every arithmetic) */
    const void* x1_amax;   /* the same for the second problem of a pair launch */
    const void* w1_amax;
    void* y1_amax;
    /* optional pair copy of the output (first problem only; fp32 y, Cout % 32 == 0): yq = y once more as fp16 plane pairs
     * (rows [2][Cout]), scaled by the power of two of the bound  amax(x) * L1max(w) + max|bias| + amax(addend)  -- complete
     * before the launch starts, unlike y's own largest magnitude -- which is stored to yq_amax.  x_true_amax: the slot x's
     * producer RAISED (for a plane-pair x: not the bound its pairs were scaled with, or the bounds of consecutive layers would
     * multiply); w_l1: RadetConvDesc.w_l1; bias_amax / addend_amax: NULL when the launch has no bias / addend.  The next
     * conv reads yq as its x operand (RADET_TILE_P3 | RADET_TILE_H2) and needs no operand split in its K loop. */
    void* yq;
    void* yq_amax;
    const void* x_true_amax;
    const void* w_l1;
    const void* bias_amax;
    const void* addend_amax;
} RadetScales;

/* Gather table of one conv geometry: table[tap][Mp] = input row feeding (output row m, tap) or -1 (padding /
 * stride hole); Mp = radet_gather_table_rows(M).  Forward / wgrad: (so, sr, off, div) = (stride, 1, -pad, 1) with
 * seg_desc rows = conv outputs.  dgrad: (1, -1, pad, stride) with input/output roles of seg_desc swapped.
 * Built once per (B, H, W); removes every integer division from the GEMM main loops. */
int radet_gather_table_rows(int M);
int radet_build_gather_table(int* table, int B, int KH, int KW, int so, int sr, int off, int div, const int* seg_desc,
                             int nseg, void* stream);
/* Implicit-GEMM conv on MFMA: y[m,n] = sum_{tap,c} x[table[tap][m], c] * w[n][tap][c].  Forward: w = wf.
 * dgrad: x = dy, w = wft (Cin/Cout swapped, dgrad table).
 * Epilogue: y = acc + bias[n] (+ addend[m,n]) ; relu ; then y = mask[m,n] > 0 ? y : 0.
 * tile_override: a packed word, RADET_TILE_* below.  splitk_ws (may be NULL): workspace of splitk_ws_floats floats whose
 * first 16384 words are arrival tickets that must be ZERO before the first launch (every launch leaves them zero); when
 * given, launches with too few tiles for 256 CUs split the K loop (<= 8 ways, or only the left-over tiles of the last
 * round) and the workgroup that arrives last at a tile sums the partial tiles in split order and applies the epilogue --
 * one launch, deterministic.  One workspace per stream: concurrent launches must not share it. */
enum {
    RADET_TILE_ID_MASK = 0xFF,         /* block tile: 0 = launcher heuristic, 1 = 128 x 128, 2 = 128 x 64, 3 = 64 x 64, 4 = 128 x 32
                                          (4 waves); 5 = 128 x 128, 6 = 256 x 128 (8 waves, P3 only); 7 / 8 = 64 x 64 whose four
                                          waves divide a 64- / 32-channel K step and add their partial tiles through LDS */
    RADET_TILE_SYMBOL = 0x100,         /* tagged kernel symbol (profiling) */
    RADET_TILE_BK32 = 0x200,           /* K step 32 instead of 16 channels (ignored with P3) */
    RADET_TILE_MATH_BF16 = 0x400,      /* bf16 math: fp32 tensors, operands rounded RNE to bf16 between LDS and the matrix core */
    RADET_TILE_STORE_BF16 = 0x800,     /* bf16 storage: x, w, addend, mask and y are bf16 tensors */
    RADET_TILE_SPLITK = 0x1000,        /* * n (bits 12-15): forced split-K factor n = 1..15 (0 = the launcher's choice) */
    RADET_TILE_SPLITK_MASK = 0xF000,
    RADET_TILE_OUT_F32 = 0x10000,      /* with STORE_BF16: y is fp32 */
    RADET_TILE_STAGES3 = 0x20000,      /* 3 LDS stages (fp32 tensors, launches that run alone on the device) */
    RADET_TILE_STAGES4 = 0x40000,      /* 4 LDS stages (tile 8 with H2) */
    RADET_TILE_ROWPAIRS = 0x80000,     /* with P3 | H2, tiles 5 / 6: a tile load fetches both planes of a row (128 bytes) */
    RADET_TILE_STREAMK = 0x100000,     /* * w (bits 20-22): stream-K schedule with w = 1..7 persistent workgroups per CU */
    RADET_TILE_STREAMK_MASK = 0x700000,
    RADET_TILE_X3 = 0x1000000,         /* fp32 tensors, products from three bf16 planes per operand, split in registers */
    RADET_TILE_P3 = 0x2000000,         /* x and w ARRIVE as planes (bf16 triples; fp16 pairs with H2); y, addend, mask, bias fp32 */
    RADET_TILE_H2 = 0x8000000,         /* with X3 or P3: fp16 hi / lo arithmetic (RadetScales; the _s entry points) */
    RADET_TILE_MASKQ = 0x10000000      /* `mask` is an fp16 plane-pair tensor (rows [2][Cout]; fp32 tensors, Cout % 32 == 0) */
};
/* MATH_BF16 is the arithmetic of mmcv's fp16 wrapper, `apis/train.py:113-117`, in bf16.  STORE_BF16 and P3 need
 * Cin % 32 == 0 (-1 otherwise).  X3: x = hi + mid + lo exactly, 8 significand bits each; 6 of the 9 plane products --
 * everything above 2^-24 relative -- through v_mfma_f32_32x32x16_bf16, fp32 accumulate; ignored (native fp32 MFMA) with
 * MATH_BF16, STORE_BF16 or Cin % 32 != 0.  P3: x rows [3][Cin] bf16, w [Cout][taps][3][Cin] bf16 ("planes" below), no
 * operand split in the K loop, K step 32 channels.  Stream-K: fp32 math, untagged symbol, tiles 2-4; the K stages of the
 * whole launch are shared evenly, tiles cut by a share boundary are reduced inside the launch in K order (deterministic);
 * plain launch when there is less than one K stage per workgroup; ignored with X3 / P3.  Refused with -1: tiles 5 / 6
 * without P3; tiles 7 / 8 without X3 (7 also runs with P3 | H2, one problem per launch), with stream-K bits, or when
 * Cin does not divide by their K step; ROWPAIRS when Cin % 32 != 0; MASKQ with STORE_BF16 or a pair launch. */
int radet_conv2d_igemm(const float* x, const float* w, const float* bias, const float* addend, const float* mask,
                       float* y, const int* gather_table, int M, int Cin, int Cout, int KH, int KW, int relu,
                       int tile_override, float* splitk_ws, size_t splitk_ws_floats, void* stream);
/* Two independent convolutions of identical geometry (cls / reg tower layers of the shared head) in ONE launch */
/* ... with amax slots: RADET_TILE_H2 (together with X3: fp32 tensors split in registers, tiles 1-4, 7, 8; or with P3:
 * operands arrive as fp16 plane pairs, tiles 1-3, 5-7) selects the fp16 hi / lo arithmetic described at RadetScales; x_amax
 * and w_amax are required then.  y_amax alone may be used with any arithmetic. */
int radet_conv2d_igemm_s(const float* x, const float* w, const float* bias, const float* addend, const float* mask,
                         float* y, const int* gather_table, int M, int Cin, int Cout, int KH, int KW, int relu,
                         int tile_override, float* splitk_ws, size_t splitk_ws_floats, void* stream, const RadetScales* sc);
int radet_conv2d_igemm_pair_s(const float* x0, const float* w0, const float* bias0, const float* addend0,
                              const float* mask0, float* y0, const float* x1, const float* w1, const float* bias1,
                              const float* addend1, const float* mask1, float* y1, const int* gather_table, int M,
                              int Cin, int Cout, int KH, int KW, int relu, int tile_override, float* splitk_ws,
                              size_t splitk_ws_floats, void* stream, const RadetScales* sc);
int radet_conv2d_igemm_taps_s(const float* x, const float* w, const float* addend, const float* mask, float* y,
                              const int* gather_table, const int* out_rows, const int* tap_ids_host, int ntaps, int kt_w,
                              int M, int Cin, int Cout, int tile_override, float* splitk_ws, size_t splitk_ws_floats,
                              void* stream, const RadetScales* sc);
int radet_conv2d_igemm_classes_s(const float* x, const float* w, const float* addend, const float* mask, float* y,
                                 const int* gather_table, const int* out_rows, const int* tap_ids_host,
                                 const int* cls_ntaps, const int* cls_start, int ncls, int kt_w, int M, int Cin, int Cout,
                                 int tile_override, float* splitk_ws, size_t splitk_ws_floats, void* stream,
                                 const RadetScales* sc);
int radet_conv2d_igemm_pair(const float* x0, const float* w0, const float* bias0, const float* addend0,
                            const float* mask0, float* y0, const float* x1, const float* w1, const float* bias1,
                            const float* addend1, const float* mask1, float* y1, const int* gather_table, int M, int Cin,
                            int Cout, int KH, int KW, int relu, int tile_override, float* splitk_ws,
                            size_t splitk_ws_floats, void* stream);
/* Tap-subset variant for the dgrad of strided convs: GEMM row m writes output row out_rows[m]; only `ntaps` taps
 * (tap_ids_host[t] = tap index inside the weight's kt_w taps) contribute; gather_table is [ntaps][Mp]. One launch
 * per stride-parity class performs only the non-zero multiply-adds (no bias / relu; addend + mask supported). */
int radet_conv2d_igemm_taps(const float* x, const float* w, const float* addend, const float* mask, float* y,
                            const int* gather_table, const int* out_rows, const int* tap_ids_host, int ntaps, int kt_w,
                            int M, int Cin, int Cout, int tile_override, float* splitk_ws, size_t splitk_ws_floats,
                            void* stream);
/* Class variant: ALL stride-parity classes of a strided dgrad in ONE launch (replaces one radet_conv2d_igemm_taps
 * launch per class; reference: the dgrad torch autograd runs for the stride-2 convs of mmdet ResNet / FPN extra levels).
 * GEMM rows = output rows sorted by class, each class padded to a multiple of 128 rows (out_rows = -1 and table = -1 on
 * the pad rows); class c owns rows [cls_start[c], cls_start[c+1]) (cls_start[0] = 0, the last class ends at M, M % 128
 * == 0), runs cls_ntaps[c] <= 4 taps, its tap t reads weight tap tap_ids_host[4c + t]; gather_table is
 * [max ntaps][radet_gather_table_rows(M)].  Order the classes by taps, most first (the grid keeps that order). */
int radet_conv2d_igemm_classes(const float* x, const float* w, const float* addend, const float* mask, float* y,
                               const int* gather_table, const int* out_rows, const int* tap_ids_host, const int* cls_ntaps,
                               const int* cls_start, int ncls, int kt_w, int M, int Cin, int Cout, int tile_override,
                               float* splitk_ws, size_t splitk_ws_floats, void* stream);
/* Predictor head convs (3x3, stride 1, pad 1, <= 32 output channels; reference: atss_cls / atss_reg / atss_iou of
 * radet/models/dense_heads/radet_head.py:_init_layers, applied per level in forward_single) as a direct convolution from an
 * LDS patch: x [rows][Cin] fp32 over all pyramid levels (rows of (level, image) contiguous, row-major H x W), w OHWI
 * [c][9][Cin], y [rows][c].  tiles_dev: ntiles x {base_row, H, W, (tile_y << 16) | tile_x} (int32), one 8 x 16 block of
 * output pixels each.  A second conv on the same input may share the launch (w1 / bias1 / y1 / c1; c0 + c1 <= 32).
 * Arithmetic: fp32 products from three bf16 planes per operand (as RADET_TILE_X3).  Cin % 16 == 0. */
int radet_pred3x3_patch(const float* x, int Cin, const int* tiles_dev, int ntiles, const float* w0, const float* bias0,
                        float* y0, int c0, const float* w1, const float* bias1, float* y1, int c1, void* stream);
/* wgrad: slabs[s][o][tap][c] = sum over pixel split s of dy[m,o] * x[table[tap][m],c];
 * optional dbias_partials[s][o] = column sums of dy.  S from radet_conv2d_wgrad_splits.
 * flags: a packed word, RADET_WGRAD_* below (its bits are NOT those of tile_override). */
enum {
    RADET_WGRAD_MATH_BF16 = 0x1,       /* bf16 math (as RADET_TILE_MATH_BF16) */
    RADET_WGRAD_STORE_BF16 = 0x2,      /* bf16 storage: dy and x are bf16 tensors (ld_dy / Cin in elements, multiples of 8); slabs fp32 */
    RADET_WGRAD_TILE = 0x10,           /* * t (bits 4-5): tile of the one-tap kernel, Cout x Cin = 1: 128 x 128, 2: 64 x 64,
                                          3: 128 x 64 (X3 / H2 only); 0 = the launcher's choice.  S is then the caller's choice */
    RADET_WGRAD_TILE_MASK = 0x30,
    RADET_WGRAD_ONE_TAP = 0x40,        /* never use the all-taps kernel */
    RADET_WGRAD_PX32 = 0x80,           /* 32 instead of 16 pixels per LDS stage (one-tap kernel, fp32 tensors, not bf16 math) */
    RADET_WGRAD_X3 = 0x100,            /* fp32 products from three bf16 planes per operand (as RADET_TILE_X3) */
    RADET_WGRAD_P3 = 0x200,            /* dy and x arrive as planes: bf16 triples (dy rows [3][ld_dy], x rows [3][Cin]), fp16 pairs with H2 */
    RADET_WGRAD_KDIV4 = 0x400,         /* X3 / H2, 64 x 64 tile: the four waves divide a 64-pixel stage four ways ... */
    RADET_WGRAD_KDIV2 = 0x800,         /* ... a 32-pixel stage two ways, and share the operand splits */
    RADET_WGRAD_H2 = 0x1000,           /* fp16 hi / lo arithmetic (radet_conv2d_wgrad_s: both amax slots required) */
    RADET_WGRAD_DEEP = 0x2000,         /* P3 | H2, 3 x 3: conv_wgrad9d_kernel (five stage buffers, loads four stages ahead) */
    RADET_WGRAD_WINDOWS = 0x4000       /* P3 | H2, 3 x 3 (an experiment): conv_wgrad9r_kernel (shifted windows of row segments) */
};
/* P3 without H2: 3 x 3 convs with Cin % 32 == 0 and ld_dy % 32 == 0, no MATH_BF16 / STORE_BF16 (-1 otherwise). */
int radet_conv2d_wgrad_splits(int M, int Cin, int Cout, int KH, int KW);
int radet_conv2d_wgrad(const float* dy, const float* x, float* slabs, float* dbias_partials, const int* gather_table,
                       int M, int Cin, int Cout, int ld_dy, int KH, int KW, int S, int flags, void* stream);
/* ... with amax slots: RADET_WGRAD_H2 (see RadetScales; sc->x_amax = the slot of dy, sc->w_amax = the slot of x; no MATH_BF16 /
 * STORE_BF16): fp32 tensors split in registers with the one-tap tiles (TILE, PX32, KDIV4 / KDIV2 as for X3), or, with P3, dy
 * rows [2][ld_dy] / x rows [2][Cin] fp16 plane pairs (Cin % 32 == 0, ld_dy % 32 == 0): 3 x 3 convs run conv_wgrad9q_kernel (128
 * output x 32 input channels x 9 taps per workgroup) unless ONE_TAP is set; every other kernel size, and ONE_TAP, the one-tap
 * pair kernel (TILE = 1: 128 x 128, otherwise 64 x 64).  DEEP and WINDOWS need the gather table of a unit-stride conv with
 * padding 1 -- tap (r, q) of pixel m reads what tap (r, 1) of pixel m + q - 1 reads, or padding: row - pixel fits 16 bits;
 * DEEP copies the table rows of a pixel split to LDS (splits of more than 1664 pixels fall back to conv_wgrad9q_kernel).  All
 * three all-taps kernels form the same sums in the same order: bit-identical results. */
int radet_conv2d_wgrad_s(const float* dy, const float* x, float* slabs, float* dbias_partials, const int* gather_table,
                         int M, int Cin, int Cout, int ld_dy, int KH, int KW, int S, int flags, void* stream,
                         const RadetScales* sc);
/* Grouped wgrad: up to 32 independent weight-gradient GEMMs (one-tap kernel) in ONE launch -- the convs of a backbone
 * stage / of the neck, whose individual grids are too short to fill 256 CUs.  Each job = the arguments of
 * radet_conv2d_wgrad (host array; Cout and Cin multiples of the tile).  flags: only RADET_WGRAD_MATH_BF16 and
 * RADET_WGRAD_TILE are read (TILE = 1: 128 x 128 tiles, otherwise 64 x 64). */
typedef struct RadetWgradJob {
    const float* dy;
    const float* x;
    float* slabs;
    float* dbias_partials;
    const int* gather_table;
    int M, Cin, Cout, ld_dy, KH, KW, S;
} RadetWgradJob;
int radet_conv2d_wgrad_group(const RadetWgradJob* jobs, int njobs, int flags, void* stream);
int radet_fold_weights(const RadetConvDesc* table_dev, int nconv, void* stream);
int radet_unfold_grads(const RadetConvDesc* table_dev, int nconv, int max_cout, void* stream);
/* ---- the memory-bound layers: stem, max-pool, GroupNorm + ReLU forward / backward, upsample-add forward / backward, ReLU
 * backward -- one entry point each.  `flags` is a packed word, RADET_LAYER_* below; any other bit is refused with -1.  The
 * `*_amax` arguments are amax slots (see RadetScales) and may be NULL; a slot that a kernel RAISES to the largest magnitude it
 * stores is not reset here.  Every argument check precedes the first HIP call. */
enum {
    RADET_LAYER_BF16 = 0x1,    /* bf16 storage: the activation tensors are bf16, not fp32 (parameters, statistics and workspaces
                                  stay fp32).  Refused together with a plane output, an amax slot or RADET_LAYER_PAIRS. */
    RADET_LAYER_PAIRS = 0x2    /* the optional plane output holds fp16 plane pairs (scaled; its amax slot is required), not bf16
                                  plane triples.  Max-pool and GroupNorm only. */
};
/* stem: 7x7/2 conv (3->64) + folded BN + ReLU, NCHW fp32 image in, NHWC out (resnet.py:558-570,627-629); y_amax is raised */
int radet_stem_conv_bn_relu(const float* img_nchw, const float* wf_ohwi, const float* bias, void* y_nhwc, int B, int H, int W,
                            int flags, void* y_amax, void* stream);
/* max-pool 3x3 / 2 (resnet.py:570,630), C % 4 == 0; y_amax is raised.  yq (may be NULL; needs RADET_LAYER_PAIRS, C % 32 == 0,
 * yq_amax and x_amax): the output once more as fp16 plane pairs, scaled by x's amax slot x_amax, whose bits go to yq_amax */
int radet_maxpool3x3s2(const void* x, void* y, int B, int H, int W, int C, int flags, void* y_amax, void* yq, void* yq_amax,
                       const void* x_amax, void* stream);
/* Trainable stem (ResNet(frozen_stages=-1): conv1 / bn1 get gradients, resnet.py:572-588).  Backward of the max-pool fused with
 * the stem's ReLU: ds = [s > 0] * (dpool routed to the first maximum of each 3x3 / 2 window in row-major order -- the element
 * torch's MaxPool2d backward picks); s = stem output [B,H,W,C], dpool [B,Ho,Wo,C], fp32, C % 4 == 0. */
int radet_maxpool3x3s2_bwd_relu(const float* s, const float* dpool, float* ds, int B, int H, int W, int C, void* stream);
/* Weight gradient of the 7x7 / 2 stem conv from the NCHW image: slabs[S][64][49][3] (pixel splits, the layout radet_unfold_grads
 * reduces) and dbias_partials[S][64] (column sums of ds, may be NULL); ds = gradient w.r.t. the stem's pre-activation
 * [B*Ho*Wo, 64].  S from radet_stem_wgrad_splits (or any S >= 1). */
int radet_stem_wgrad_splits(int B, int H, int W);
int radet_stem_wgrad(const float* img_nchw, const float* ds, float* slabs, float* dbias_partials, int B, int H, int W, int S,
                     void* stream);

/* ---- GroupNorm(32, 256) + ReLU over a multi-level buffer (atss_head.py:32,60-76 via mmcv ConvModule) */
int radet_gn_workspace_floats(int B, const int* seg_desc, int nseg);
/* forward of one tensor (z1 == NULL) or of two tensors of one geometry (cls_convs[i].gn / reg_convs[i].gn) in one pair of
 * launches.  Per tensor: z in; y (z's type, may be NULL) and / or planes (may be NULL, fp32 z only) out -- bf16 plane triples, or
 * with RADET_LAYER_PAIRS fp16 plane pairs scaled by the power of two of a bound on |y| that needs no pass over the data
 * (max|gamma| sqrt(n - 1) + max|beta| for the n values of a group), which is stored to planes_amax; stats [nseg*B][32][2];
 * y_amax is raised to y's largest magnitude, zhat_amax to the largest normalised magnitude.  C == 256, groups == 32. */
int radet_gn_relu_fwd(const void* z0, const float* gamma0, const float* beta0, void* y0, void* planes0, float* stats0,
                      float* partial_ws0, void* y_amax0, void* planes_amax0, void* zhat_amax0, const void* z1,
                      const float* gamma1, const float* beta1, void* y1, void* planes1, float* stats1, float* partial_ws1,
                      void* y_amax1, void* planes_amax1, void* zhat_amax1, int B, int C, int groups, float eps, int relu,
                      int flags, const int* seg_desc, int nseg, void* stream);
/* backward: dz in dy's type (may be NULL) and / or as planes (may be NULL, fp32 only) -- bf16 plane triples, or with
 * RADET_LAYER_PAIRS fp16 plane pairs scaled by the bound rstd_max max|gamma| dy_amax (2 + zhat_max), stored to planes_amax;
 * dy_amax = the amax slot of dy (required with pairs), zhat_amax from the forward call (NULL: sqrt(n - 1)). */
int radet_gn_relu_bwd(const void* dy, const void* z, const float* stats, const float* gamma, const float* beta, void* dz,
                      void* planes, float* dgamma, float* dbeta, float* partial_ws, int B, int C, int groups, int relu,
                      int flags, const int* seg_desc, int nseg, void* stream, const void* dy_amax, const void* zhat_amax,
                      void* planes_amax);

/* ---- FPN top-down: dst += nearest_upsample(src) and its adjoint (fpn.py:182-191); C % 4 == 0; the written tensor's slot
 * (dst_amax / dsrc_amax) is raised */
int radet_upsample_add(void* dst, const void* src, int B, int Ho, int Wo, int Hi, int Wi, int C, int flags, void* dst_amax,
                       void* stream);
int radet_upsample_add_bwd(void* dsrc, const void* ddst, int B, int Ho, int Wo, int Hi, int Wi, int C, int flags,
                           void* dsrc_amax, void* stream);
/* ReLU backward for a junction with no producing GEMM: dx = (dy + addend?) * [act > 0]; n % 4 == 0; dx_amax is raised */
int radet_relu_bwd(const void* dy, const void* addend, const void* act, void* dx, size_t n, int flags, void* dx_amax,
                   void* stream);
/* the row converter used at the fp32 boundaries of the bf16-storage mode (loss gradients, module outputs) */
int radet_convert_rows(const void* src, void* dst, size_t rows, int ncols, int src_ld, int src_off, int dst_ld,
                       int dst_off, int to_bf16, void* stream);
/* ---- bf16 plane triples ("planes"): the operand format of the default fp32 arithmetic's conv GEMMs.  An fp32 value x is
 * stored as three bf16 numbers hi + mid + lo == x exactly (8 significand bits each, truncation); a row of C channels is
 * [3][C] bf16 = hi | mid | lo, rows back to back (6 bytes per element).  The producers of a tensor that only conv GEMMs read
 * (GroupNorm+ReLU outputs of the head towers, their gradients, folded weights with RadetConvDesc.w16 = 2) write planes once;
 * radet_conv2d_igemm (RADET_TILE_P3) and radet_conv2d_wgrad (RADET_WGRAD_P3) multiply them on the bf16 matrix cores with fp32
 * accumulation (6 of the 9 plane products, as RADET_TILE_X3) -- same results as splitting the fp32 operands inside the GEMM,
 * without the per-use VALU work.  Replaces nothing in the reference by itself: it is the storage format behind the convs of
 * resnet.py:260-299 / fpn.py:170-221 / atss_head.py:118-145.  C % 8 == 0, row strides in floats, % 4 == 0. */
int radet_split_planes(const float* src, void* dst_planes, size_t rows, int C, int src_ld, void* stream);
int radet_merge_planes(const void* src_planes, float* dst, size_t rows, int C, int dst_ld, void* stream);
/* ---- fp16 plane pairs ("plane pairs"): the operand format of the fp16 hi / lo arithmetic for tensors that only conv GEMMs
 * read.  A row of C channels (C % 32 == 0) is C / 32 groups of 128 bytes [hi x 32 | lo x 32] fp16 -- 4 bytes per element,
 * one cache line per 32-channel K stage and row -- holding x 2^e split as described at RadetScales, e from the tensor's amax
 * slot.  radet_split_pairs scales by the slot of src and copies the slot's bits to dst_amax; radet_merge_pairs is the
 * inverse (tests / API boundary).  radet_conv2d_igemm_s (RADET_TILE_H2 | P3) and radet_conv2d_wgrad_s (RADET_WGRAD_H2 | P3)
 * multiply them with three v_mfma_f32_32x32x16_f16 per K = 16 step and no operand work in their K loops. */
int radet_split_pairs(const float* src, void* dst_pairs, size_t rows, int C, int src_ld, const void* src_amax, void* dst_amax,
                      void* stream);
int radet_merge_pairs(const void* src_pairs, float* dst, size_t rows, int C, int dst_ld, const void* amax, void* stream);
/* A stand-alone amax pass for tensors whose producer raises no slot (any n). */
int radet_absmax(const float* x, size_t n, void* amax, void* stream);
int radet_amax_slot_words(void);   /* 32-bit words to allocate (and zero) per amax slot */
int radet_nchw_to_nhwc(const float* x, float* y, int B, int C, int H, int W, void* stream);
int radet_nhwc_to_nchw(const float* x, float* y, int B, int C, int H, int W, void* stream);

/* ---- head loss: targets + sigmoid focal + GIoU + IoU-BCE, forward and gradients in one pass.
 *      Replaces RADetHead.get_targets/_get_target_single/loss (dense_heads/radet_head.py:173-392),
 *      TBLRBBoxCoder.encode/decode (core/bbox/coder/tblr_bbox_coder.py:71-172), bbox_overlaps aligned
 *      (core/bbox/iou_calculators/iou2d_calculator.py:116-158), FocalLoss/GIoULoss/CrossEntropyLoss
 *      (models/losses/{focal,iou,cross_entropy}_loss.py) and mmcv.ops.sigmoid_focal_loss.
 *  Rows are level-major: level l rows [off_l, off_l + B*h_l*w_l), image-major inside, row-major pixels.
 *  cls [R,C] logits; reg_u [R,4] = atss_reg output BEFORE Scale/ReLU; iou [R] logits; scales [nlvl].
 *  gt_boxes [sumG,4], gt_labels i64 [sumG], gt_off i32 [B+1]; p2g i64 [B,N], pw f32 [B,N] (N = points/img).
 *  level_desc (host): nlvl x 3 ints {h, w, stride}.  grad_scale: 3 device floats (upstream grads) or NULL.
 *  Outputs: losses[3] = {loss_cls, loss_bbox, loss_iou}; dcls [R,dcls_ld]; dreg_u [R,dreg_ld]; diou [R,diou_ld]
 *  (row strides let the gradients land in zero-padded buffers that the dgrad GEMM consumes directly; the
 *  sparse dreg_u / diou rows of non-positive points are zero-filled here); dscales [nlvl];
 *  optional dumps (may be NULL): labels_out i64 [R], bbox_targets_out [R,4].
 *  flags = RADET_HEAD_LOSS_POSTACT (bit 0) | kind << RADET_HEAD_LOSS_KIND_SHIFT (bits 1-3):
 *    POSTACT: reg_u holds the head's bbox_pred AFTER Scale + ReLU (the tensor `RADetHead.loss` receives,
 *    radet_head.py:173-181; pass scales = 1): dreg_u is then the gradient w.r.t. that tensor (no ReLU mask).
 *    kind: the `loss_bbox` module, one of RADET_BOX_LOSS_* (0 = GIoU, so flags 0 / 1 keep their earlier meaning);
 *    a value without a kernel returns RADET_ERR_ARG before anything is launched.  giou_eps is that module's `eps`
 *    whatever the kind.  The IoU branch does not depend on the kind: its target is bbox_overlaps' I / max(U, 1e-6)
 *    (radet_head.py:267), the box weight max(iou, 1e-12) * pw.  (Kind GIoU shares that union with its loss, as it
 *    always did: there the bound is giou_eps, the same number at GIoULoss' default.)
 *  ws: int32 workspace of radet_head_loss_ws_ints(R) ints. */
#define RADET_HEAD_LOSS_POSTACT 1
#define RADET_HEAD_LOSS_KIND_SHIFT 1
#define RADET_HEAD_LOSS_KIND_MASK (7 << RADET_HEAD_LOSS_KIND_SHIFT)
/* box regression losses (radet/models/losses/iou_loss.py): GIoULoss, IoULoss(linear=False) = -log(iou),
 * IoULoss(linear=True) = 1 - iou, DIoULoss, CIoULoss */
#define RADET_BOX_LOSS_GIOU 0
#define RADET_BOX_LOSS_IOU 1
#define RADET_BOX_LOSS_IOU_LINEAR 2
#define RADET_BOX_LOSS_DIOU 3
#define RADET_BOX_LOSS_CIOU 4
#define RADET_BOX_LOSS_KINDS 5
int radet_head_loss_ws_ints(int R);
int radet_head_loss(const float* cls, const float* reg_u, const float* iou, const float* scales,
                    const float* gt_boxes, const int64_t* gt_labels, const int* gt_off, const int64_t* p2g,
                    const float* pw, const int* level_desc, int nlvl, int B, int num_classes, float alpha,
                    float gamma, float loss_bbox_weight, float giou_eps, const float* grad_scale, float* losses,
                    float* dcls, int dcls_ld, float* dreg_u, int dreg_ld, float* diou, int diou_ld, float* dscales,
                    int64_t* labels_out, float* bbox_targets_out, int flags, int* ws, void* stream);
/* bbox_pred = relu(reg_u * scale_level) materialised for the module API (atss_head.py:143, radet_head.py:29) */
int radet_scale_relu(const float* reg_u, const float* scales, float* out, const int* level_desc, int nlvl, int B,
                     void* stream);

/* ---- inference: threshold / per-level top-k / TBLR decode (radet_head.py:55-146, atss_head.py:325-387) */
/* For each image b: candidates written to cand_* [B, cap] (cap = nlvl * nms_pre), count in cand_count[b].
 * Per level: scores = sigmoid(cls) > score_thr, top nms_pre by score (ties: lower flat index first),
 * boxes decoded with clamp to (img_h, img_w) and divided by scale_factor[b] (4 floats per image). */
size_t radet_decode_ws_bytes(int B, int nlvl, int nms_pre);
int radet_decode_candidates(const float* cls, const float* reg_u, const float* iou, const float* scales,
                            const int* level_desc, int nlvl, int B, int num_classes, float score_thr, int nms_pre,
                            const float* img_hw /*[B,2]*/, const float* scale_factor /*[B,4] or NULL*/,
                            float* cand_boxes, float* cand_scores, float* cand_ctr, int64_t* cand_labels,
                            int* cand_count, void* ws, void* stream);

/* ---- NMS family (radet/ops/vote/vote_ext.cpp:70-353, radet/ops/cluster/cluster_ext.cpp:4-87,
 *      mmcv.ops.batched_nms as used at radet_head.py:160). Batched over images: inputs [B, cap] with
 *      counts[b] valid entries.  mode: 0 vote, 1 global_vote, 2 cluster (ids), 3 hard batched NMS.
 *      Outputs (capacity max_out per image, heads in descending cluster score):
 *        out_boxes [B,max_out,4], out_scores [B,max_out], out_labels i64 [B,max_out], out_count [B];
 *      mode 2: instance_id i64 [B,cap], cluster_num i64 [B,cap]; mode 3: keep i64 [B,max_out] (input index).
 *      ws: workspace of radet_nms_ws_bytes(B, cap) bytes.  cap <= 65536: up to 8192 candidates per image the sorts run in
 *      LDS and a crowded label's greedy pass out of registers; above, the sorts run in global memory and label segments
 *      longer than 8192 boxes take a general pass (same results; the reference ops have no size limit,
 *      cluster_ext.cpp:4-87 / vote_ext.cpp:70-207). */
size_t radet_nms_ws_bytes(int B, int cap);
int radet_nms(const float* boxes, const float* cluster_scores, const float* vote_scores, const int64_t* labels,
              const int* counts, int B, int cap, int mode, float iou_thr, int iou_enable, float sigma, int max_out,
              float* out_boxes, float* out_scores, int64_t* out_labels, int* out_count, int64_t* aux0, int64_t* aux1,
              void* ws, void* stream);

/* ---- Soft-NMS (mmcv.ops.batched_nms with nms.type = 'soft_nms', reached from radet_head.py:159-163; mmcv 1.3.18's
 *      softnms_cpu restated -- mmcv is not available to the tests, so parity with it is UNPINNED; the tests pin a NumPy
 *      restatement bit for bit).  Batched over images like radet_nms: inputs [B, cap] with counts[b] valid entries,
 *      cap <= 65536.  Per image: boxes + float(label) * (largest valid coordinate + 1) in fp32 (class_agnostic: no
 *      offset); then repeatedly pick the highest current score among the boxes neither picked nor pruned (ties: lowest
 *      input index -- this project's rule, mmcv's depends on its swap history) and multiply every remaining score by
 *        naive:    ovr >= iou_thr ? 0 : 1          linear: ovr >= iou_thr ? 1 - ovr : 1
 *        gaussian: exp(-(ovr * ovr) / sigma), argument in fp32, exp in DOUBLE rounded once to fp32 (not glibc expf)
 *      with ovr = inter / (area_i + area_p - inter), all fp32 and unfused; a NaN ovr (two zero-area boxes) gives weight 1
 *      under every method (mmcv's gaussian branch would write NaN scores).  After each multiply a box with score <
 *      min_score is removed for good; the picked box is never checked, so an image's first pick survives whatever its
 *      score.  Candidates with a NaN score are never picked.
 *      Outputs in pick order (scores non-increasing), the first max_out (> 0) of the sequence: out_boxes [B,max_out,4] the
 *      original boxes, out_scores the decayed scores, out_labels, out_keep i64 [B,max_out] input indices, out_count [B].
 *      One workgroup per image runs the global loop: up to 8192 candidates (1024 lanes x 8) from registers and LDS,
 *      above through ws (radet_soft_nms_ws_bytes: 24 B per candidate, no dense mask); same results.  No host
 *      synchronisation, no allocation.  RADET_ERR_ARG before any launch: method not 0..2, sigma <= 0 with gaussian,
 *      max_out <= 0, cap outside 1..65536. */
#define RADET_SOFT_NMS_NAIVE 0
#define RADET_SOFT_NMS_LINEAR 1
#define RADET_SOFT_NMS_GAUSSIAN 2
size_t radet_soft_nms_ws_bytes(int B, int cap);
int radet_soft_nms(const float* boxes, const float* scores, const int64_t* labels, const int* counts, int B, int cap,
                   int method, float iou_thr, float sigma, float min_score, int class_agnostic, int max_out,
                   float* out_boxes, float* out_scores, int64_t* out_labels, int64_t* out_keep, int* out_count,
                   void* ws, void* stream);

/* ---- detections tracked across frames (csrc/track.hip), one launch per batch of consecutive frames.  The reference has no
 *      tracker: these are this project's OWN rules (parity: UNPINNED), pinned bit for bit to the NumPy restatement
 *      tests/_track_ref.py.  The default parameters (Python: ops/track.py) are starting points nobody has evaluated.
 *   A SEQUENCE (one camera) holds TRACK_MAX_TRACKS = 256 slots; a zero-filled state is the empty tracker.  Ids start at 1;
 *   id 0 means "no track".  State of sequence s: TRACK_STATE_BYTES bytes at state + s * TRACK_STATE_BYTES (16-byte aligned):
 *        box f32 [256,4] (the current estimate) | vel f32 [256,4] (per-frame displacement of the four coordinates) |
 *        label i32 [256] | id i32 [256] (0: the slot is free) | misses i32 [256] | hits i32 [256] | score f32 [256] |
 *        next_id i32 (the last id handed out), frames i32, refused i32, one i32 of padding
 *   Inputs as radet_nms emits them: boxes [nseq,B,cap,4], scores [nseq,B,cap], labels i64, counts [nseq,B] (clamped to
 *   [0, cap]); the B frames of a sequence are consecutive in time and run one after the other.  Per frame, in this order --
 *   all arithmetic fp32, every operation rounded once, min(a, b) = a < b ? a : b, max(a, b) = a > b ? a : b,
 *   area = (x2 - x1) * (y2 - y1):
 *   1. predict: for every slot pred = box + vel, one add per coordinate (motion TRACK_MOTION_NONE: pred = box; vel is then
 *      neither read nor written, except that a new track's is zeroed).
 *   2. the detections are visited in the order given (rank order).  ELIGIBLE: four finite coordinates, a finite score,
 *      score >= track_thr, 0 <= label < 2^31.  An ineligible detection gets id 0 and touches nothing.
 *   3. match: candidate slots are live (id != 0), not yet matched in this frame, of index < max_tracks and -- with class_aware
 *      -- of the detection's label.  IoU of pred (a) against the detection (b): iw = max(min(x2a, x2b) - max(x1a, x1b), 0), ih
 *      likewise, inter = iw * ih, union = (area_a + area_b) - inter, iou = inter / union.  A slot qualifies with iou >=
 *      iou_thr (a NaN IoU -- two zero-area boxes -- never does); the highest IoU wins, equal IoUs go to the lower slot.  On a
 *      match: vel = det - box (one subtraction per coordinate against the estimate of one frame ago, observed or coasted; no
 *      division), box = det, score = the detection's, misses = 0, hits += 1; the detection's id is the slot's.
 *   4. start: an unmatched eligible detection with score >= new_thr takes the lowest slot below max_tracks that is free AT
 *      THIS MOMENT (slots that expire in step 5 of this frame are free from the next frame on): id = ++next_id, box = det,
 *      vel = 0, label, score, hits = 1, misses = 0, and the slot counts as matched for the rest of the frame.  No free slot:
 *      id 0 and refused += 1.  Below new_thr: id 0.
 *   5. age: every live slot not matched in this frame gets misses += 1; with misses > max_age it is freed (id = 0, its other
 *      fields stay as they are), otherwise box = pred (the track coasts, vel unchanged).
 *   6. frames += 1.
 *   Outputs [nseq,B,cap]: ids i32 (0: none), hits i32 (the track's hits after the update, 0 where the id is 0); slots at or
 *   beyond a frame's count are written as 0.  One wave per sequence: the 256 slots live in registers, four per lane (slot =
 *   4 * lane + j), detections are read 64 at a time and broadcast from registers; no LDS, no barriers, no atomics, no host
 *   synchronisation, no allocation.
 *   RADET_ERR_ARG before any launch: nseq, B or cap < 1, cap > TRACK_MAX_DETS, max_tracks outside [1, TRACK_MAX_TRACKS],
 *   iou_thr outside (0, 1], max_age < 0, a non-finite threshold, an unknown motion, class_aware not 0 / 1, a NULL or
 *   misaligned (boxes, state: 16 bytes) pointer. */
#define TRACK_MAX_TRACKS 256
#define TRACK_MAX_DETS 4096
#define TRACK_STATE_BYTES 13328          /* 256 * (16 + 16 + 5 * 4) + 16 */
#define TRACK_MOTION_NONE 0
#define TRACK_MOTION_CONSTANT 1
size_t radet_track_state_bytes(int nseq);
int radet_track_update(const float* boxes, const float* scores, const int64_t* labels, const int* counts, int nseq, int B,
                       int cap, void* state, float iou_thr, float track_thr, float new_thr, int max_age, int max_tracks,
                       int motion, int class_aware, int* ids, int* hits, void* stream);

/* ---- visibility-guided positive-sample assigner (radet/datasets/pipelines/label_assignment.py:57-201).
 *      One image per workgroup.  masks u8 [sumG, H, W]; rng_words u32 [B, U] = the next U raw 32-bit outputs of the image's
 *      RandomState (MT19937; a random_sample() is two words); out p2g i64 [B,N], pw f32 [B,N], used i32 [B] (words
 *      consumed; -1 = stream exhausted, -2 = more than 256 gts, -3 = an adapted positive_num above 64).
 *      flags: bit 0 balance_sample, bit 1 multiply_samplepro_for_weight, bit 2 adapt_positive_num, bit 3 NOT
 *      random_sample_by_distance (uniform integer draws: randint / permutation) -- the constructor arguments of
 *      label_assignment.py:30-46; the BOP configs use flags = 1.  ws: radet_assign_ws_bytes(B, N) bytes. */
size_t radet_assign_ws_bytes(int B, int N);
int radet_assign_points(const float* gt_boxes, const int* gt_off, const uint8_t* masks, int H, int W,
                        const uint32_t* rng_words, int U, const int* level_desc, const float* regress_ranges /*host, nlvl x 2*/,
                        int nlvl, int B, int positive_num, int flags, float neg_threshold, int64_t* p2g, float* pw, int* used,
                        void* ws, void* stream);

/* same with float per-box distance maps f32 [sumG, H, W] (mask-free sampler: MBD / GDT output mapped into the image,
 * radet/datasets/pipelines/loading.py:586-645, read as np.float32 by label_assignment.py:85-92) */
int radet_assign_points_f(const float* gt_boxes, const int* gt_off, const float* distance_maps, int H, int W,
                          const uint32_t* rng_words, int U, const int* level_desc, const float* regress_ranges /*host, nlvl x 2*/,
                          int nlvl, int B, int positive_num, int flags, float neg_threshold, int64_t* p2g, float* pw, int* used,
                          void* ws, void* stream);

/* ---- box-to-distance transforms of the mask-free sampler (GenerateDistanceMap(with_gt_mask=False)):
 *      pybind ops bbox2distance_ext.{MBD, GDT} (radet/ops/bbox2distance/bbox2distance_ext.cpp:127-133, 225-236), batched
 *      over box crops.  img_desc_dev[n][5] = (pixel offset of the crop in the packed arrays, h, w, first seed, seeds);
 *      images u8 [px][3] (HWC), dmap f64 [px], cost / dist f32 [px]; seeds as int32.  Bit-identical to the
 *      reference's sequential raster scans. */
size_t radet_mbd_ws_bytes(size_t total_px);
int radet_mbd(const uint8_t* images, const int* img_desc_dev, int nimg, const int* seeds_x, const int* seeds_y, float alpha,
              int niter, int base_size, double* dmap, size_t total_px, void* ws, void* stream);
int radet_gdt(const float* cost, const int* img_desc_dev, int nimg, const int* seeds_x, const int* seeds_y, float* dist,
              void* ws_labels /* int32 [px] */, void* stream);

/* ---- image processing around those transforms (radet/ops/bbox2distance/bbox2distance_wrapper.py:80-93, 118-130,
 *      170-181: cv2.resize / cv2.GaussianBlur / cv2.cvtColor / cv2.Sobel / cv2.addWeighted), batched over packed crops:
 *      *_desc (device) = ncrop x 3 ints {pixel offset, height, width}; max_*_px = the largest crop's pixel count (grid).
 *      OpenCV's generic algorithms restated (cv2 is absent: parity unpinned against cv2, pinned by oracle/imgproc.py):
 *      8-bit INTER_LINEAR with 11-bit fixed-point coefficients, float / double INTER_LINEAR, 9x9 Gaussian (sigma 1.7,
 *      kernel5 (host) = centre tap + 4 taps, BORDER_REFLECT_101, round to nearest even; tmp = 3 floats per pixel), and
 *      the Sobel edge map (3x3 Gaussian, RGB2GRAY, |0.5 d/dx + 0.5 d/dy| / max; gray_ws 1 byte per pixel, max_ws
 *      one word per crop). */
int radet_resize_linear_u8(const uint8_t* src, const int* src_desc, uint8_t* dst, const int* dst_desc, const int* view_desc,
                           int ncrop, int max_dst_px, int channels, void* stream);
int radet_resize_linear_f(const void* src, const int* src_desc, void* dst, const int* dst_desc, int ncrop, int max_dst_px,
                          int is_f64, void* stream);
/* The view row: per-image / per-mask geometry of radet_resize_linear_u8, radet_mask_transform and radet_rle_masks.
 * view_desc (device, may be NULL) = one row per image or mask of RADET_VIEW_INTS ints
 *      {Hr, Wr, wy0, wx0, wh, ww, oy, ox, h, w, flip, fill}:
 * take the wh x ww window at (wy0, wx0) of the source, in the source's own coordinates (it may overhang the source or miss
 * it; what lies outside reads as the fill for images, as 0 for masks), resize it to a virtual Hr x Wr, and write the h x w
 * window at (oy, ox) of that.  view_desc == NULL is the whole source to the whole output, from the scalar arguments.
 * Resize + RandomCrop sets (oy, ox, h, w); Expand / MinIoURandomCrop + Resize set (wy0, wx0, wh, ww, fill); no canvas and
 * no full-size resized image is ever made.  fill = c0 | c1 << 8 | c2 << 16 in the source's channel order (images only),
 * flip as radet_mask_transform's (bitmap masks only).
 *   images: taps and coefficients are those of a wh x ww image resized to Hr x Wr at output pixel (oy + y, ox + x) (the
 *      edge clamp is at the window's border); each tap is read at (wy0 + ty, wx0 + tx) of the source or is the fill: bit
 *      for bit "paste the source on the filled canvas, slice, radet_resize_linear_u8, slice".  dst_desc stays {pixel
 *      offset, h, w}, max_dst_px the largest h * w.
 *   masks: dst[g][y][x] = y < h && x < w ? norm(S(wy0 + nn(oy + flip_y(y)), wx0 + nn(ox + flip_x(x)))) : pad_val, nn over
 *      the wh x ww grid resized to Hr x Wr, S = src[g] inside the Hs x Ws source and 0 outside it, the flip inside the
 *      h x w window (it follows the crop), norm_max still the maximum of the whole source mask.
 *   A bad row has Hr, Wr, wh or ww <= 0, wy0 + wh or wx0 + ww beyond int, an output window that is not inside Hr x Wr, or
 *      (masks) h > Hd or w > Wd, or (images) h, w other than its dst_desc row's or an empty source.  An image with a bad
 *      row is not written; a mask with a bad row is pad_val only. */
#define RADET_VIEW_INTS 12
int radet_gaussian_blur9_u8(const uint8_t* src, const int* desc, uint8_t* dst, float* tmp, const float* kernel5, int ncrop,
                            int max_px, void* stream);
int radet_sobel_edge(const uint8_t* src, const int* desc, float* edge, uint8_t* gray_ws, uint32_t* max_ws, int ncrop,
                     int max_px, void* stream);

/* ---- instance-mask path feeding the assigner: BitmapMasks.rescale / resize / flip / pad
 *      (core/mask/structures.py:253-303: mmcv.imresize = cv2.INTER_NEAREST, np.flip, np.pad per mask) fused into one
 *      pass over a [G,Hs,Ws] u8 stack, and LoadAnnotations._load_bop_masks' normalisation (loading.py:419-422).
 *      dst[g][y][x] = y < Hr && x < Wr ? norm(src[g][nn(flip_y(y))][nn(flip_x(x))]) : pad_val, dst is [G,Hd,Wd];
 *      flip: 0 none, 1 horizontal, 2 vertical, 3 diagonal; norm_max (from radet_mask_max) or NULL = no normalisation */
int radet_mask_max(const uint8_t* masks, uint32_t* maxes /* [G] */, int G, size_t hw, void* stream);
int radet_mask_transform(const uint8_t* src, uint8_t* dst, const uint32_t* norm_max, const int* view_desc, int G, int Hs, int Ws,
                         int Hr, int Wr, int Hd, int Wd, int flip, int pad_val, void* stream);
/* view_desc (i32 [G][RADET_VIEW_INTS], see above) replaces Hr, Wr and flip by one geometry per mask */

/* ---- the same masks from run-length annotations (COCO RLE / rasterised polygons, radet/datasets/pipelines/loading.py:313-380
 *      `_poly2mask`), without a bitmap on the host or in HBM: one launch per group of masks of one destination geometry.
 *      A mask is the union of its parts; a part is a COCO run list over the source image in column-major order (first run
 *      zeros).  run_ends u32 [n_ends]: the inclusive prefix sums of every part's counts, part after part (a part's last
 *      entry is Hs * Ws < 2^32).  part_desc i32 [n_parts][RLE_PART_INTS] = {offset into run_ends, runs};
 *      mask_desc i32 [G][RLE_MASK_INTS] = {first part, parts, Hs, Ws, flip (bit 0: horizontal)}.
 *      dst u8 [G,Hd,Wd]: what radet_mask_transform writes for the decoded 0 / 1 bitmap with the mask's own flip:
 *      dst[g][y][x] = y < Hr && x < Wr ? OR over parts of (index of the run that holds nn(flip_x(x)) * Hs + nn(y)) & 1 : pad_val.
 *      dst_plain (may be NULL) u8 [G,Hd,Wd]: the unflipped mask, written ONLY for masks whose flip bit is set (for the
 *      others dst already is that mask): both orientations from one lookup.  Rows that point outside the tables decode as
 *      empty.  Wd <= 8192, G <= 65535.  view_desc (i32 [G][RADET_VIEW_INTS], see above; may be NULL) replaces Hr, Wr: the
 *      same window of what is decoded -- a sample outside the source is 0, not a lookup in a neighbouring column's runs;
 *      the flip stays mask_desc's (the flip word of view_desc is not read) and acts inside the h x w window. */
#define RLE_MASK_INTS 5
#define RLE_PART_INTS 2
int radet_rle_masks(const uint32_t* run_ends, int n_ends, const int* part_desc, int n_parts, const int* mask_desc,
                    const int* view_desc, int G, uint8_t* dst, uint8_t* dst_plain, int Hr, int Wr, int Hd, int Wd, int pad_val,
                    void* stream);

/* ---- baseline JPEG files decoded on the device (csrc/jpeg.hip, csrc/jpeg_index.c, radet_amd/core/jpeg.py): what libjpeg's
 *      default decompressor gives for them byte for byte (slow-integer IDCT, fancy upsampling, fixed-point YCbCr -> RGB),
 *      stored B, G, R.  Supported: one interleaved Huffman scan, 8 bits, 1 component or YCbCr with luma sampling 1x1, 2x1
 *      or 2x2 and chroma 1x1.
 *      radet_jpeg_index (host only, no device is touched): one walk over the scan file[scan_lo, scan_hi) that writes an
 *      entry point every seg_mcus MCUs of a restart interval and at every restart marker, rows of JPEG_ROW_INTS ints
 *      {raw byte offset, bit in that byte, first MCU, MCUs, DC predictor x 3, end offset * 8 + end bit}.  comp_blocks[c] =
 *      blocks of component c per MCU; huff = 2 * ncomp table records of JPEG_HUFF_BYTES (DC, AC per component; layout:
 *      csrc/jpeg_common.h, built by core/jpeg.py).  Returns the number of rows, or minus an error bit: 1 undefined code,
 *      2 coefficient index past 63, 4 the stream ends early, 8 restart marker out of sequence, 16 MCU count / arguments,
 *      64 more than max_rows rows.
 *      radet_jpeg_decode: three launches for nimg images (entropy decode, IDCT, upsample + convert; `stages` bits 1 | 2 | 4
 *      select them, 7 = all).  files: the files' bytes; desc i32 [nimg][JPEG_DESC_INTS] = {file offset, scan end (relative),
 *      W, H, components, luma h, luma v, MCUs per row, MCU rows, first block of component 0..2 in coef, byte offset of plane
 *      0..2 in planes (multiples of 8), destination pixel offset in dst, first index row, index rows, 0...};
 *      wgs i32 [n_wg][2] = {image, first index row} per workgroup of 64 segments; huff [nimg][6] records; quant u16
 *      [nimg][3][64] in natural order; rows: the index rows of all images; coef i16 [blocks][64] and planes u8: scratch
 *      (planes are padded to whole MCUs); dst: packed u8 BGR pixels; err i32 [nimg], zero on entry: error bits per image
 *      (the walker's, and 32: a segment did not end where its index row says).  huff, quant, coef 16-byte aligned. */
#define JPEG_ROW_INTS 8
#define JPEG_DESC_INTS 20
#define JPEG_HUFF_BYTES 1424
int radet_jpeg_index(const uint8_t* file, int scan_lo, int scan_hi, int ncomp, const int* comp_blocks, const void* huff,
                     int n_mcus, int restart_interval, int seg_mcus, int* rows, int max_rows);
int radet_jpeg_decode(const uint8_t* files, const int* desc, int nimg, const int* wgs, int n_wg, const void* huff,
                      const uint16_t* quant, const int* rows, int n_rows, int16_t* coef, uint8_t* planes, uint8_t* dst,
                      int* err, int max_blocks, int max_px, int stages, void* stream);

/* ---- BOP training-image augmentation (csrc/augment.hip): RandomBackground merge, CosyPoseAug's PillowBlur /
 *      PillowSharpness / PillowContrast / PillowBrightness / PillowColor, RandomFlip, Normalize, Pad, batched over packed
 *      u8 HWC BGR images (every buffer packed alike).  params (device) = nimg rows of AUG_PARAM_INTS ints:
 *      {pixel offset, h, w, flags, background pixel offset, mask count, mask address lo, hi (u8 [G,h,w]), blur radius,
 *       blur ww, blur fw, f32 bits of the sharpness / contrast / brightness / color factors, mask pitch};
 *      mask pitch: 0, or Hm << 16 | Wm when the masks are the top-left h x w of u8 [G,Hm,Wm] (Hm >= h, Wm >= w; the
 *      assigner's zero-padded masks of a sample smaller than a fixed pad size serve the merge as they are);
 *      flags: 1 merge, 2 blur, 4 sharpness, 8 contrast, 16 brightness, 32 color, 64 horizontal flip, 128 BGR->RGB.
 *      Four launches per batch in this order; lsum = one u64 luma sum per image (sharp -> finish); out = f32 [nimg,3,Hp,Wp]
 *      with out = (x - m) * s per channel and zeros beyond each image.  Widths and heights up to AUG_MAX_W. */
#define AUG_PARAM_INTS 16
#define AUG_MAX_W 8192
int radet_augment_merge_hblur(const uint8_t* src, const uint8_t* bg, const int* params, uint8_t* dst, int nimg, int max_h,
                              int max_w, void* stream);
int radet_augment_vblur(const uint8_t* src, const int* params, uint8_t* dst, int nimg, int max_h, int max_w, void* stream);
int radet_augment_sharp(const uint8_t* src, const int* params, uint8_t* dst, unsigned long long* lsum, int nimg, int max_px,
                        void* stream);
int radet_augment_finish(const uint8_t* src, const unsigned long long* lsum, const int* params, float* out, int nimg, int Hp,
                         int Wp, float m0, float m1, float m2, float s0, float s1, float s2, void* stream);

/* ---- the mixpbr stages RandomHSV / RandomNoise / RandomSmooth (csrc/augment.hip) on the same packed u8 HWC BGR layout,
 *      between radet_augment_merge_hblur and radet_augment_finish.  params2 (device) = nimg rows of AUG2_PARAM_INTS ints:
 *      {pixel offset, h, w, flags, f32 bits of the h / s / v factors, lt (bit 0 / 1 / 2: that factor is < 1, no clip),
 *       f64 bits of the noise sigma (lo, hi), Philox key word 0 (lo, hi), key word 1 (lo, hi), box size k (1, 3, 5, 7), 0};
 *      flags: 1 HSV, 2 noise, 4 box.  hsv_noise: cv2 BGR2HSV, scale, HSV2BGR, then + N(0, sigma) * 255 from Box-Muller on
 *      Philox-4x64-10 (key, counter = block + 1); box: cv2.blur k x k, reflect-101.  src / dst 4-byte aligned; nbytes =
 *      the size of box's src buffer (its loads stay inside it); max_px = the largest h * w. */
#define AUG2_PARAM_INTS 16
int radet_augment_hsv_noise(const uint8_t* src, const int* params2, uint8_t* dst, int nimg, int max_px, void* stream);
int radet_augment_box(const uint8_t* src, const int* params2, uint8_t* dst, size_t nbytes, int nimg, int max_h, int max_w,
                      void* stream);

/* ---- the mask-free sampler inside the image pipeline (GenerateDistanceMap(with_gt_mask=False), loading.py:596-645): the
 *      padded box crops cut from the augmented u8 BGR image, and the distance maps pasted for the assigner.
 *      radet_crop_canvases (csrc/augment.hip): src / lsum / params = what radet_augment_finish reads; a canvas pixel inside
 *      its box's clipped source rectangle is the u8 BGR value radet_augment_finish normalises (contrast / brightness / color
 *      blends, the mirrored column of a flipped image), every other canvas pixel the box's fill colour.  desc (device) =
 *      ncanvas rows of CROP_DESC_INTS ints, coordinates in the (flipped) image:
 *      {image index, window x0, y0 (image position of canvas pixel (0, 0), may be negative), canvas width, height,
 *       source rectangle x0, y0, x1, y1 (exclusive; the kernel intersects it with the image), fill b | g << 8 | r << 16,
 *       output pixel offset, 0};
 *      dst = the u8 HWC canvases back to back ({offset, h, w} rows of the crop kernels above), total_px pixels (a canvas
 *      that would leave it is not written); src_bytes = the size of src; src / dst 4-byte aligned; max_px = largest canvas.
 *      radet_paste_maps (csrc/imgproc.hip): out f32 [nbox, H, W] = per box the map value inside the truncated box rectangle
 *      (f32 as is, f64 rounded to f32), 1 there for a disabled box, 0 elsewhere; every element is written.  desc (device) =
 *      nbox rows of PASTE_DESC_INTS ints: {map pixel offset, map height, map width, region x0, y0 inside the map, box x0,
 *      y0, x1, y1 in the image (exclusive), enabled}; map_px = the size of maps in elements (reads stay inside it). */
#define CROP_DESC_INTS 12
#define PASTE_DESC_INTS 10
int radet_crop_canvases(const uint8_t* src, size_t src_bytes, const unsigned long long* lsum, const int* params, int nimg,
                        const int* desc, int ncanvas, int max_px, uint8_t* dst, size_t total_px, void* stream);
int radet_paste_maps(const void* maps, size_t map_px, int is_f64, const int* desc, int nbox, int H, int W, float* out,
                     void* stream);

/* ---- affine augmentation (csrc/warp.hip): Rotate / Shear / Translate of radet/datasets/pipelines/auto_augment.py, i.e.
 *      cv2.warpAffine(INTER_LINEAR, BORDER_CONSTANT, output size = input size) in its classic fixed-point form, for nimg
 *      packed u8 HWC images of mixed sizes (channels == 3) or single planes such as instance masks (channels == 1) in one
 *      launch.  desc (device) = nimg rows of WARP_DESC_INTS ints:
 *      [WARP_DESC_SRC] pixel offset of the image in src, [WARP_DESC_DST] pixel offset of the output in dst, [WARP_DESC_H],
 *      [WARP_DESC_W], [WARP_DESC_CHANNELS] (must equal `channels`), [WARP_DESC_FILL] fill = c0 | c1 << 8 | c2 << 16 in the
 *      image's channel order, [WARP_DESC_FLAGS] (WARP_SKIP: the image is copied unchanged), one spare word, then from
 *      [WARP_DESC_MATRIX] the INVERSE 2 x 3 matrix {M0 .. M5} as 6 doubles (low word first): the host inverts the forward
 *      matrix in double exactly as cv2 does.  Per output pixel (x, y), AB = 1024, round = half to even:
 *          X0 = round((M1 y + M2) AB) + 16, Y0 = round((M4 y + M5) AB) + 16,
 *          X = (X0 + round(M0 x AB)) >> 5, Y = (Y0 + round(M3 x AB)) >> 5, sx = X >> 5, sy = Y >> 5, fx = X & 31, fy = Y & 31,
 *          dst = (sum of the four taps at (sx, sy) .. (sx + 1, sy + 1) times (32 - fx | fx)(32 - fy | fy) + 512) >> 10,
 *      every double product and sum rounded on its own; a tap outside the image is the fill byte of its channel.
 *      src_px / dst_px: the sizes of src / dst in pixels (< 2^31); a row that does not lie inside them, or with h, w <= 0 or
 *      another channel count, is not written.  src != dst.  max_px = the largest image's pixel count; nimg <= 65535.
 *      The caller keeps |M0| w + |M1| h + |M2| (and the second row's) below 2^21 so that the coordinates fit 32 bits. */
#define WARP_DESC_INTS 20
#define WARP_DESC_SRC 0
#define WARP_DESC_DST 1
#define WARP_DESC_H 2
#define WARP_DESC_W 3
#define WARP_DESC_CHANNELS 4
#define WARP_DESC_FILL 5
#define WARP_DESC_FLAGS 6
#define WARP_DESC_MATRIX 8
#define WARP_SKIP 1
int radet_warp_affine_u8(const uint8_t* src, size_t src_px, uint8_t* dst, size_t dst_px, const int* desc, int nimg, int max_px,
                         int channels, void* stream);

/* ---- CutOut (csrc/cutout.hip; radet/datasets/pipelines/transforms.py:1734-1804): the holes of nimg images filled in place
 *      in one launch.  desc (device) = nimg rows of CUTOUT_DESC_INTS ints:
 *      [CUTOUT_DESC_OFF] radet_cutout_u8: pixel offset of the image in the packed u8 HWC buffer; radet_cutout_f32: index of
 *      the image in out f32 [nbatch,3,Hp,Wp], [CUTOUT_DESC_H], [CUTOUT_DESC_W], [CUTOUT_DESC_FILL] fill = c0 | c1 << 8 |
 *      c2 << 16 in the u8 image's channel order (BGR), [CUTOUT_DESC_FIRST] the image's first row of `holes`,
 *      [CUTOUT_DESC_COUNT] the number of its rows, [CUTOUT_DESC_FLAGS] (CUTOUT_SKIP: the image is left alone; f32 only:
 *      CUTOUT_FLIP the sample is flipped horizontally, CUTOUT_TO_RGB the planes are RGB), one spare word.
 *      holes (device) = nholes rows {x1, y1, x2, y2}: half-open rectangles in the coordinates of the unflipped image, of
 *      any values; each is clipped to the image.  max_holes = the largest count, max_area = the largest hole's pixels.
 *      radet_cutout_u8 stores the fill bytes; radet_cutout_f32 stores per plane what radet_augment_finish writes for a u8
 *      pixel equal to the fill with no blend flag set ((q - m) * s in fp32), at columns w - x2 .. w - x1 - 1 of a flipped
 *      sample.  Nothing outside the holes is written.  A row whose image does not lie inside the buffer (img_px pixels;
 *      nbatch images of Hp x Wp) or whose holes do not lie inside the table is not written.  channels must be 3;
 *      nimg, max_holes <= 65535. */
#define CUTOUT_DESC_INTS 8
#define CUTOUT_DESC_OFF 0
#define CUTOUT_DESC_H 1
#define CUTOUT_DESC_W 2
#define CUTOUT_DESC_FILL 3
#define CUTOUT_DESC_FIRST 4
#define CUTOUT_DESC_COUNT 5
#define CUTOUT_DESC_FLAGS 6
#define CUTOUT_SKIP 1
#define CUTOUT_FLIP 2
#define CUTOUT_TO_RGB 4
int radet_cutout_u8(uint8_t* img, size_t img_px, const int* desc, int nimg, const int* holes, int nholes, int max_holes,
                    int max_area, int channels, void* stream);
int radet_cutout_f32(float* out, int nbatch, int Hp, int Wp, const int* desc, int nimg, const int* holes, int nholes, int max_holes,
                     int max_area, float m0, float m1, float m2, float s0, float s1, float s2, void* stream);

/* ---- AutoAugment's colour stages (csrc/color.hip; radet/datasets/pipelines/auto_augment.py:709-890: ColorTransform,
 *      EqualizeTransform, BrightnessTransform, ContrastTransform) on nimg packed u8 HWC BGR images, in place, two launches.
 *      desc (device) = nimg rows of COLOR_DESC_INTS ints: [COLOR_DESC_OFF] pixel offset of the image in the packed buffer
 *      (byte 3 * offset: any alignment), [COLOR_DESC_H], [COLOR_DESC_W], [COLOR_DESC_KIND] (COLOR_BRIGHTNESS, COLOR_CONTRAST,
 *      COLOR_COLOR, COLOR_EQUALIZE; any other value: the row is not run), [COLOR_DESC_ALPHA] / [COLOR_DESC_BETA] the fp32
 *      bits of alpha = fl32(factor) and beta = fl32(1 - factor) (1 - factor formed in double; fl32 = one rounding to
 *      nearest even), [COLOR_DESC_FLAGS] (COLOR_SKIP: the image is left alone), one spare word.
 *      The pixel rules are this project's restatement of mmcv 1.3.18 (adjust_brightness / adjust_contrast / adjust_color /
 *      imequalize) on OpenCV 4; neither is installed where this is developed, so parity with their PIXELS is unpinned (as
 *      for radet_warp_affine_u8), the stages' planning is pinned to the reference.  x = a channel byte, N = h * w,
 *          gray(b, g, r) = (3735 b + 19235 g + 9798 r + 16384) >> 15                 (OpenCV 4's u8 BGR2GRAY)
 *          hist[c][v] = the number of pixels with value v in channel c (B, G, R), ghist[v] the same of the gray image
 *      Brightness: t = fl32(x * alpha), clipped to [0, 255], truncated: one 256-entry map for the three channels.
 *      Contrast:   mean = sum(v * ghist[v]) / N rounded half to even, in integers (= Python's round(float64(S) / N) for
 *                  every image up to 8192 x 8192); m = fl32(mean * beta), rounded on its own; t = fma(x, alpha, m), clipped,
 *                  truncated: one 256-entry map.
 *      Color:      per pixel g = gray(pixel); per channel t = fma(x, alpha, fl32(g * beta)), rounded half to even,
 *                  saturated to [0, 255].
 *      Equalize:   per channel c: last = the highest v with hist[c][v] > 0, step = (N - hist[c][last]) / 255 (integer);
 *                  step == 0: the channel is unchanged; else lut[v] = min(255, (sum_{u < v} hist[c][u] + step / 2) / step).
 *      The fused multiply-add (one rounding of x * alpha + m) is this project's choice where OpenCV's scalar and SIMD paths
 *      of addWeighted may differ; the product g * beta / mean * beta is never contracted into it.
 *      radet_color_stats_u8: hist u32 [nimg, 4, 256] = hist of B, G, R and ghist of every row whose kind is COLOR_EQUALIZE or
 *      COLOR_CONTRAST, ADDED to what hist holds (integer atomics: bit-reproducible): the caller zeroes it.  Other rows are
 *      not read.  radet_color_apply_u8: every row's image mapped in place; hist is read for COLOR_EQUALIZE / COLOR_CONTRAST
 *      rows (NULL: those rows are not run).  A workgroup takes COLOR_CHUNK_PX pixels of one image; no byte outside the rows'
 *      images is read or written.  A row with h, w <= 0 or whose image does not lie inside the buffer (img_px pixels,
 *      < 2^31) is not run.  max_px = the largest image's pixel count; channels must be 3; nimg <= 65535; images up to 8192 a
 *      side (counts fit 32 bits). */
#define COLOR_DESC_INTS 8
#define COLOR_DESC_OFF 0
#define COLOR_DESC_H 1
#define COLOR_DESC_W 2
#define COLOR_DESC_KIND 3
#define COLOR_DESC_ALPHA 4
#define COLOR_DESC_BETA 5
#define COLOR_DESC_FLAGS 6
#define COLOR_SKIP 1
#define COLOR_BRIGHTNESS 1
#define COLOR_CONTRAST 2
#define COLOR_COLOR 3
#define COLOR_EQUALIZE 4
#define COLOR_CHUNK_PX 4096
int radet_color_stats_u8(const uint8_t* img, size_t img_px, const int* desc, int nimg, int max_px, unsigned* hist, int channels,
                         void* stream);
int radet_color_apply_u8(uint8_t* img, size_t img_px, const int* desc, int nimg, int max_px, const unsigned* hist, int channels,
                         void* stream);

/* ---- in-memory frames through the test pipeline in one launch (csrc/preprocess.hip): LoadImageFromWebcam -> Resize ->
 *      Normalize -> Pad (radet/datasets/pipelines/loading.py:88 as radet/apis/inference.py:97-102 uses it).  nimg u8 HWC BGR
 *      frames of any, mixed sizes -> out f32 [nimg,3,Hp,Wp]: what radet_resize_linear_u8 followed by radet_augment_finish
 *      (no augmentation flag set) writes for the same pixels, bit for bit; every element of out is written.
 *      desc (device) = nimg rows of PREP_DESC_INTS ints:
 *      {source byte address lo, hi, source row stride in bytes (unsigned), source h, w, destination (resized) h, w, flags};
 *      a pixel is 3 consecutive bytes, pixels of a row are contiguous; any address alignment (byte loads), so a frame may
 *      be a view into a larger device tensor.  flags: PREP_TO_RGB | PREP_FLIP_H | PREP_FLIP_V.  Pixels beyond the
 *      destination h x w are zero; a row with source h or w <= 0 is all zeros.  nimg <= 65535, Hp * Wp < 2^31.
 *      PREP_FLIP_H / PREP_FLIP_V (both: diagonal) are the views of test-time augmentation, mmcv.imflip of the RESIZED image
 *      in front of Normalize and Pad: inside the destination h x w, pixel (y, x) of a flipped row is what the unflipped row
 *      writes at (y, w - 1 - x), at (h - 1 - y, x), or at both mirrored; the padding stays on the right and at the bottom.
 *      A row without these flags writes the bits it wrote before they existed. */
#define PREP_DESC_INTS 8
#define PREP_TO_RGB 1
#define PREP_FLIP_H 2
#define PREP_FLIP_V 4
int radet_preprocess_frames(const int* desc, int nimg, int Hp, int Wp, float m0, float m1, float m2, float s0, float s1,
                            float s2, float* out, void* stream);

/* ---- test-time augmentation: the views' candidates back in the frame, packed per image (csrc/tta.hip), one launch.
 *      Input: the candidate lists of V * B (view, image) rows, row r = v * B + b, as radet_decode_candidates writes them in
 *      VIEW coordinates (scale_factor = NULL) into ONE pool: pool_boxes f32 [pool, 4] (16-byte aligned), pool_scores /
 *      pool_ctr f32 [pool], pool_labels i64 [pool], counts i32 [V * B].  Views of different scales may have different
 *      capacities: nothing but its descriptor row says where a row's list lies, so every decode launch (one per group of
 *      views that ran as one forward batch) writes its own [rows, cap] block of the pool.
 *      desc = V * B rows of MERGE_DESC_INTS 32-bit words:
 *        {h, w (the view's img_shape, f32 bits), sx, sy, sx, sy (its scale_factor, f32 bits), flip code (0 none, 1
 *         horizontal, 2 vertical, 3 diagonal), start (the pool index of the row's first candidate), cap (the row's capacity)};
 *      it is passed twice: desc_host (host memory, read during the call only, never by the device) is what the argument
 *      checks read, desc (device) the same words for the kernel -- uploading them is the caller's.
 *      Output, per image b: out_* [B, cap_out] hold view 0's counts[0 * B + b] candidates, then view 1's, ...; inside a
 *      view the order is kept and nothing is dropped (the reference's torch.cat order of aug_test_bboxes; every NMS here
 *      breaks ties by input index); out_count[b] = the sum of the counts (a count above its row's cap counts as cap).
 *      Slots at and beyond out_count[b] are not written.  Scores, centerness and labels are copied; boxes are
 *      bbox_mapping_back (radet/core/bbox/transforms.py:46-55), fp32, every operation rounded once, a true IEEE division:
 *        horizontal: x1' = w - x2, x2' = w - x1;  vertical: y1' = h - y2, y2' = h - y1;  diagonal: both;
 *        then x1' / sx, y1' / sy, x2' / sx(word 4), y2' / sy(word 5).
 *      grid (ceil(cap_out / 256), B), one output slot per thread, 16-byte loads and stores for the boxes.  No host
 *      synchronisation, no allocation, capturable.  RADET_ERR_ARG before any launch: V outside 1..TTA_MAX_VIEWS, B < 0 or
 *      > 65535, cap_out outside 1..65536, a NULL pointer with B > 0, and from desc_host: a flip code outside 0..3, a cap < 0,
 *      a row whose [start, start + cap) leaves [0, pool), an image whose caps do not add up to at most cap_out.  B == 0:
 *      RADET_OK, no launch. */
#define TTA_MAX_VIEWS 16
#define MERGE_DESC_INTS 9
int radet_merge_views(const int* desc_host, const int* desc, int V, int B, size_t pool, const float* pool_boxes,
                      const float* pool_scores, const float* pool_ctr, const int64_t* pool_labels, const int* counts,
                      int cap_out, float* out_boxes, float* out_scores, float* out_ctr, int64_t* out_labels, int* out_count,
                      void* stream);

/* ---- tiled inference: the rows' candidates filtered at the tile borders, back in the frame, packed per image
 *      (csrc/tiles.hip), one launch.  A batch of B frames has R = row_start[B] rows, image-major: image b's rows are
 *      [row_start[b], row_start[b + 1]) -- its full-frame row, if it has one, then its tiles -- 1..TILE_MAX_ROWS of them.
 *      Input: the rows' candidate lists as radet_decode_candidates writes them in ROW coordinates (scale_factor = NULL, boxes
 *      clamped to the row's img_shape) into ONE pool, laid out as for radet_merge_views; counts i32 [R].
 *      desc = R rows of TILE_DESC_INTS 32-bit words:
 *        {h, w (the row's img_shape, f32 bits), sx, sy, sx, sy (its scale_factor, f32 bits), x0, y0 (where the row's source
 *         rectangle starts in the frame, the integers as f32 bits), edge mask (TILE_EDGE_L | _T | _R | _B: that side of the
 *         row is a cut through the frame, not a side of the frame), start (pool index of the row's first candidate), cap};
 *      the full-frame row has x0 = y0 = 0 and mask 0.  desc and row_start are passed twice, as radet_merge_views' desc is:
 *      *_host (host memory, read during the call only) for the argument checks, the device copies for the kernel.
 *      A candidate (x1, y1, x2, y2) of a row is DROPPED if  L and x1 <= m,  or T and y1 <= m,  or R and x2 >= w - m,  or
 *      B and y2 >= h - m  (m = edge_margin; w - m, h - m in fp32, rounded once; comparisons with a NaN are false).  With
 *      m = 0 these are exactly the boxes the decode clamped onto a cut: the object reaches past the tile, and a neighbouring
 *      tile or the full-frame row sees it whole.  A kept box is mapped back as  x / sx + x0  (a true IEEE division, then one
 *      add, each rounded once; x2 and y2 use words 4 and 5); scores, centerness and labels are copied.
 *      Output, per image b: out_* [B, cap_out] hold the kept candidates in row order, inside a row in candidate order (a
 *      stable compaction; a count below 0 counts as 0, one above its row's cap as cap); out_count[b] = the number kept,
 *      out_dropped[b] = the number dropped, together the sum of the image's clamped counts.  Slots at and beyond out_count[b]
 *      are not written.  grid B: one workgroup of 512 threads per image, ballot + popcount ranks, no atomics, so the order
 *      does not depend on scheduling.  No host synchronisation, no allocation, capturable.  RADET_ERR_ARG before any launch:
 *      B < 0 or > 65535, cap_out outside 1..65536, an edge_margin that is negative or not finite, a NULL pointer with B > 0,
 *      and from the host copies: row_start[0] != 0, an image with no row or more than TILE_MAX_ROWS, an edge mask outside
 *      0..15, a cap < 0, a row whose [start, start + cap) leaves [0, pool), an image whose caps add up to more than cap_out.
 *      B == 0: RADET_OK, no launch. */
#define TILE_MAX_ROWS 64
#define TILE_DESC_INTS 11
#define TILE_EDGE_L 1
#define TILE_EDGE_T 2
#define TILE_EDGE_R 4
#define TILE_EDGE_B 8
int radet_merge_tiles(const int* desc_host, const int* desc, const int* row_start_host, const int* row_start, int B, size_t pool,
                      const float* pool_boxes, const float* pool_scores, const float* pool_ctr, const int64_t* pool_labels,
                      const int* counts, float edge_margin, int cap_out, float* out_boxes, float* out_scores, float* out_ctr,
                      int64_t* out_labels, int* out_count, int* out_dropped, void* stream);

/* ---- detections -> a packed batch of RoI crops (csrc/crops.hip), two launches, nothing read back to the host.
 * radet_crop_plan (one workgroup): boxes f32 [B,K,4] (16-byte aligned), scores f32 [B,K], counts i32 [B] -- the NMS outputs
 *      as they are -- walked image-major, then by rank j < counts[b].  A detection is valid if its four coordinates are
 *      finite, w = x2 - x1 > 0, h = y2 - y1 > 0, |cx|, |cy| < 2^20 and score >= score_thr; the valid ones are compacted in
 *      order (stable).  counters i32 [2 + B]: counters[0] = n_out = min(n_total, cap), counters[1] = n_total = the number
 *      of valid detections, counters[2 + b] = the number of rows of the frames 0 .. b (frame b's rows end there: a host
 *      that copies the counters splits the batch per frame without reading a row);
 *      rows i32 [cap][CROP_ROW_INTS] = {b, j, wx0, wy0, ww, wh} for the first n_out of them, rows beyond are not written.
 *      The window has the output's aspect ratio (no distortion) and may overhang the frame or miss it; fp32, every
 *      operation rounded once:
 *          a  = (float)Wo / (float)Ho
 *          hs = fmaxf(h, w / a) * scale                       ws = hs * a
 *          wh = clamp((int)ceilf(hs), 1, CROP_MAX_SIDE)       ww = clamp((int)ceilf(ws), 1, CROP_MAX_SIDE)
 *          cx = (x1 + x2) * 0.5f                              cy = (y1 + y2) * 0.5f
 *          wx0 = (int)floorf(cx - 0.5f * (float)ww)           wy0 = (int)floorf(cy - 0.5f * (float)wh)
 * radet_crop_frames (grid: pixel tiles x cap): slot n < n_out (read from counters on the device; the other blocks exit
 *      before any load or store) = the wh x ww window at (wy0, wx0) of frame b resized to Ho x Wo: taps and coefficients of
 *      a wh x ww image (the edge clamp is at the window's border), each tap read at (wy0 + ty, wx0 + tx) of the frame or
 *      the fill colour outside it -- bit for bit radet_resize_linear_u8 with the view row {Ho, Wo, wy0, wx0, wh, ww, 0, 0,
 *      Ho, Wo, 0, fill}.  desc = B rows of PREP_DESC_INTS ints as above (address, row stride, source h, w; the other
 *      fields are not read); fill = c0 | c1 << 8 | c2 << 16 in the frame's channel order.  flags: CROP_F32: out f32
 *      [cap,3,Ho,Wo] = (q - mean) * stdinv per plane, with CROP_TO_RGB after the BGR->RGB swap (radet_augment_finish's
 *      Normalize); without CROP_F32: out u8 [cap,Ho,Wo,3], the raw BGR bytes (4-byte aligned).  A row whose b is not in
 *      [0, B) or whose window is not one the plan writes is skipped.
 * RADET_ERR_ARG before any launch: B, K or cap < 0, K == 0 or a NULL pointer with B and cap > 0, Ho or Wo outside
 *      [1, 4096], cap > 65535, B * K >= 2^31, scale not finite or <= 0, unknown flags.  B == 0 or cap == 0: RADET_OK, no
 *      launch. */
#define CROP_ROW_INTS 6
#define CROP_MAX_SIDE 16384
#define CROP_TO_RGB 1
#define CROP_F32 2
int radet_crop_plan(const float* boxes, const float* scores, const int* counts, int B, int K, int Ho, int Wo, float scale,
                    float score_thr, int cap, int* rows, int* counters, void* stream);
int radet_crop_frames(const int* rows, const int* counters, const int* desc, int B, int cap, int Ho, int Wo, int flags,
                      unsigned fill, float m0, float m1, float m2, float s0, float s1, float s2, void* out, void* stream);

/* ---- detections drawn on frames (csrc/draw.hip), one launch: box outlines and "name|score" labels.  These are this
 *      project's own pixel rules (the reference draws with matplotlib / mmcv / cv2; parity with them is unpinned), pinned bit
 *      for bit to the NumPy restatement tests/_draw_ref.py.
 *      src_desc / dst_desc (device) = B rows of PREP_DESC_INTS ints as above (address, row stride, h, w; the other fields are
 *      not read): any byte alignment, frames may be views into larger tensors.  A destination row names the same h x w as
 *      its source row (a frame whose rows disagree is skipped).  Out of place every byte of the h x w x 3 pixels of every
 *      destination frame is written (copy + overlay in one pass); with DRAW_INPLACE dst_desc == src_desc and a pixel tile
 *      that nothing covers stores nothing (without the flag, a frame whose destination row names its source row's address and
 *      stride is in place likewise: one table may mix both).  Bytes between the rows of a view are never touched.  max_h / max_w: the largest
 *      h / w of the table (the grid; pixels beyond them are not visited).  Frames with h or w <= 0 draw nothing.
 *      Detections in the padded NMS layout: boxes f32 [B,K,4] (16-byte aligned), scores f32 [B,K], labels i64 [B,K],
 *      counts i32 [B].
 *   Which are drawn.  Detection j < min(counts[b], K) is VALID when its four coordinates and its score are finite,
 *      score > score_thr (strict), 0 <= label < (n_names > 0 ? n_names : 100000) (and < n_palette when box_colour < 0), and
 *      x2i >= x1i, y2i >= y1i where  vi = (int)clamp(v, -2^20, 2^20)  (truncation toward zero: numpy's astype(int32)).
 *      The first max_dets (<= DRAW_MAX_DETS) valid detections in rank order are DRAWN; r = their rank among the drawn.
 *   Outline.  t = thickness >= 1, lo = t / 2, hi = (t - 1) / 2.  Pixel (x, y) is on detection r's outline when it is inside
 *      [x1i - lo, x2i + hi] x [y1i - lo, y2i + hi] and not strictly inside (x1i + hi, x2i - lo) x (y1i + hi, y2i - lo).
 *      Opaque; the lowest r whose outline covers a pixel gives its colour: box_colour = b | g << 8 | r << 16, or with
 *      box_colour < 0 the three bytes palette[label] (u8 [n_palette,3], BGR).
 *   Label (Hc > 0).  atlas u8 [S,Hc,Wa] holds one strip of coverage per row-block, strip s being widths[s] (i32 [S], clamped
 *      to [0, Wa]) columns wide: strips 0-9 the digits, 10 '.', 11 '|', 12 'class ', 13 + c the name of class c.  The text is
 *      with n_names > 0 the strips {13 + label, 11, d, 10, d, d}, else {12, the label's decimal digits, 11, d, 10, d, d};
 *      d.dd shows  cents = clamp((int)floor((double)score * 100.0 + 0.5), 0, 100)  -- ties round UP (0.125 -> 0.13), where
 *      Python's ':.02f' rounds half to even.  Wt = the sum of the strips' widths (at most DRAW_MAX_TEXT_W), p = pad, the
 *      label rectangle is lw x lh = (Wt + 2p) x (Hc + 2p) at  lx = max(0, min(x1i, w - lw)),  ly = max(0, min(y1i, h - lh)).
 *      Blend, exact in integers, per channel, a in [0, 65025]:  out = (colour * a + pixel * (65025 - a) + 32512) / 65025.
 *      Above ALL outlines the labels are composited from the last drawn rank down to rank 0, each as: the rectangle in black
 *      with a = a_bg * 255 (a_bg in [0, 255]), then the text in text_colour with a = 255 * coverage at text pixel
 *      (x - lx - p, y - ly - p) inside [0, Wt) x [0, Hc).  Hc == 0 draws no labels (atlas, widths may be NULL).
 *   Gather form: one workgroup per 128 x 8 pixel tile and frame derives the frame's drawn detections, culls them against its
 *      tile into LDS in rank order (ballot + popcount across its wavefronts) and every pixel is computed and stored by
 *      exactly one thread: no atomics, no workspace, no host synchronisation, capturable, the same bytes on every run.
 *   RADET_ERR_ARG before any launch: B outside [0, 65535], K < 0, thickness outside [1, DRAW_MAX_THICKNESS], max_dets outside
 *      [0, DRAW_MAX_DETS], a_bg outside [0, 255], a colour above 0xFFFFFF, box_colour < 0 without a palette, pad outside
 *      [0, DRAW_MAX_PAD], Hc outside [0, DRAW_MAX_GLYPH_H], with Hc > 0 a NULL atlas / widths, Wa outside [1, DRAW_MAX_TEXT_W]
 *      or S < 13 + n_names, a NaN score_thr, unknown flags, max_h > 65535 * 8, a NULL table or boxes not 16-byte aligned with
 *      something to do.  B == 0 or max_h == 0 or max_w == 0: RADET_OK, no launch. */
#define DRAW_MAX_DETS 256
#define DRAW_MAX_THICKNESS 255
#define DRAW_MAX_TEXT_W 4096
#define DRAW_MAX_GLYPH_H 256
#define DRAW_MAX_PAD 64
#define DRAW_INPLACE 1
int radet_draw_detections(const int* src_desc, const int* dst_desc, int B, int max_h, int max_w, const float* boxes,
                          const float* scores, const int64_t* labels, const int* counts, int K, int thickness, int box_colour,
                          const uint8_t* palette, int n_palette, int text_colour, int a_bg, float score_thr, int max_dets,
                          int n_names, int pad, int flags, const uint8_t* atlas, const int* widths, int S, int Hc, int Wa,
                          void* stream);

/* ---- stand-alone box / loss operators behind the registered classes (used on their own; inside the detector the same
 *      arithmetic runs fused in radet_head_loss / radet_decode_candidates) ------------------------------------------ */
/* bbox_overlaps / BboxOverlaps2D (radet/core/bbox/iou_calculators/iou2d_calculator.py:43-159): boxes [batch, M, 4] and
 * [batch, N, 4]; mode 0 iou, 1 iof, 2 giou; aligned: out [batch, M] (M == N) else the M x N matrix out [batch, M, N].
 * Operation order = the reference's PyTorch expressions, results equal PyTorch-CPU fp32 bit for bit. */
int radet_bbox_overlaps(const float* bboxes1, const float* bboxes2, float* out, int batch, int M, int N, int mode,
                        int aligned, float eps, void* stream);
/* TBLRBBoxCoder.encode / decode = bboxes2tblr / tblr2bboxes (radet/core/bbox/coder/tblr_bbox_coder.py:71-172).
 * normalizer4 (host): the 4 normalisation factors (a scalar normalizer repeated); decode clamps to
 * [0, max_w] x [0, max_h] when clip != 0 (clip_border and max_shape given). */
int radet_tblr_encode(const float* priors, const float* gts, float* out, int n, const float* normalizer4,
                      int normalize_by_wh, void* stream);
int radet_tblr_decode(const float* priors, const float* tblr, float* out, int n, const float* normalizer4,
                      int normalize_by_wh, float max_h, float max_w, int clip, void* stream);
/* Elementwise losses with `weight_reduce_loss` semantics (radet/models/losses/utils.py:24-51).  Forward: optional
 * loss_elem = loss * weight * elem_scale per element, optional partials[radet_loss_partials(n_elem)] = per-workgroup sums that
 * radet_loss_finalize adds in a fixed order: out[0] = sum / avg_factor[0] (device scalar, may be NULL) * scale.
 * weight_cols: 0 none, 1 per row, C per element.  Backward: d(input) = dloss/dinput * weight * g with
 * g = grad_elem[i] * scale (reduction 'none') or grad_scalar[0] * scale / avg_factor[0] (reduced); grad_elem,
 * grad_scalar, avg_factor may each be NULL.
 *   sigmoid focal  : mmcv.ops.sigmoid_focal_loss as wrapped by radet/models/losses/focal_loss.py:44-86 (target = class
 *                    index per row, anything outside [0, C) = background)
 *   bce with logits: radet/models/losses/cross_entropy_loss.py:57-92 (use_sigmoid=True), float targets [N, C]
 *   giou           : radet/models/losses/iou_loss.py:82-98, boxes [N, 4], weight [N] or NULL, gradient w.r.t. pred */
int radet_loss_partials(size_t n_elem);
int radet_loss_finalize(const float* partials, int npartials, const float* avg_factor, float scale, float* out,
                        void* stream);
int radet_sigmoid_focal_loss(const float* logits, const int64_t* target, const float* weight, int weight_cols, size_t N,
                             int C, float gamma, float alpha, float* loss_elem, float elem_scale, float* partials,
                             void* stream);
int radet_sigmoid_focal_loss_bwd(const float* logits, const int64_t* target, const float* weight, int weight_cols, size_t N,
                                 int C, float gamma, float alpha, const float* grad_elem, const float* grad_scalar,
                                 const float* avg_factor, float scale, float* dlogits, void* stream);
int radet_bce_logits_loss(const float* logits, const float* target, const float* weight, int weight_cols, size_t N, int C,
                          float* loss_elem, float elem_scale, float* partials, void* stream);
int radet_bce_logits_loss_bwd(const float* logits, const float* target, const float* weight, int weight_cols, size_t N,
                              int C, const float* grad_elem, const float* grad_scalar, const float* avg_factor, float scale,
                              float* dlogits, void* stream);
int radet_giou_loss(const float* pred, const float* target, const float* weight, size_t N, float eps, float* loss_elem,
                    float elem_scale, float* partials, void* stream);
int radet_giou_loss_bwd(const float* pred, const float* target, const float* weight, size_t N, float eps,
                        const float* grad_elem, const float* grad_scalar, const float* avg_factor, float scale, float* dpred,
                        void* stream);
/* The box regression losses by kind (RADET_BOX_LOSS_*; iou_loss.py:11-34,82-213), same argument layout, partial sums and
 * gradient contract as the giou pair; kind GIoU runs the giou kernels themselves.  eps = the module's `eps` (IoU: the
 * clamp below the log, on top of bbox_overlaps' own 1e-6; DIoU / CIoU: added to the union, c^2 and the heights);
 * hp1 is a spare hyper-parameter, pass 0.  An unknown kind returns RADET_ERR_ARG before any launch. */
int radet_box_loss(int kind, const float* pred, const float* target, const float* weight, size_t N, float eps, float hp1,
                   float* loss_elem, float elem_scale, float* partials, void* stream);
int radet_box_loss_bwd(int kind, const float* pred, const float* target, const float* weight, size_t N, float eps, float hp1,
                       const float* grad_elem, const float* grad_scalar, const float* avg_factor, float scale, float* dpred,
                       void* stream);
/* multiclass_nms' score filter (radet/core/post_processing/bbox_nms.py:54-56): idx[0..count) = ascending indices i
 * with scores[i] > thr (torch.nonzero order); one workgroup, ordered ballot-prefix compaction. */
int radet_threshold_compact(const float* scores, size_t n, float thr, int64_t* idx, int* count, void* stream);

/* ---- anchors (core/anchor/anchor_generator.py:206-271): [sum h*w, 4], centre (j*stride, i*stride), side 8*stride */
int radet_grid_anchors(float* out, const int* level_desc, int nlvl, int octave_base_scale, void* stream);

/* ---- optimiser step on flat arenas: global L2 grad-norm clip + AdamW (torch.optim.AdamW +
 *      clip_grad_norm_ as driven by mmcv OptimizerHook; configs/base/default_runtime.py:1-19) */
int radet_sqnorm_partials(const float* g, size_t n, float* partials, int npartials, void* stream);
int radet_adamw_step(float* p, const float* g, float* m, float* v, size_t n, float lr, float beta1, float beta2,
                     float eps, float weight_decay, int step, float max_norm, float grad_div,
                     const float* partials, int npartials, float* grad_norm_out, void* stream);
/* Parameter groups (mmcv's paramwise_cfg) as a RUN TABLE over the trainable arena: run r scales the learning rate of the
 * elements [begin, end) by lr_mult and their weight decay by decay_mult.  Runs are sorted, disjoint and cover [0, n); a
 * boundary may fall anywhere (inside a 16-byte access too) and a run may be one element long.  The table is a DEVICE array
 * (a replayed launch tape sees a stable pointer) of at most RADET_OPT_MAX_RUNS runs: each block stages it into 16 KiB of LDS.
 * The kernels trust its order and coverage -- radet_amd/runtime.py:build_opt_runs validates them -- and cannot be led out of
 * bounds by a bad one (it only selects multipliers). */
#define RADET_OPT_MAX_RUNS 1024
typedef struct { uint32_t begin, end; float lr_mult, decay_mult; } RadetOptRun;
/* radet_adamw_step per run: lr_r = lr * lr_mult, decay = 1 - lr_r * (weight_decay * decay_mult), step size lr_r / bc1; the
 * clip coefficient is the global one (all runs, as clip_grad_norm_ over all parameters).  lr_mult = 0 leaves p untouched and
 * still updates m and v.  One run (0, n, 1, 1) is bit-identical to radet_adamw_step.  Arguments 0-15 are radet_adamw_step's.
 * RADET_ERR_ARG: nruns outside [1, RADET_OPT_MAX_RUNS], runs == NULL, n >= 2^32, step < 1, grad_div <= 0. */
int radet_adamw_step_runs(float* p, const float* g, float* m, float* v, size_t n, float lr, float beta1, float beta2,
                          float eps, float weight_decay, int step, float max_norm, float grad_div,
                          const float* partials, int npartials, float* grad_norm_out, const RadetOptRun* runs, int nruns,
                          void* stream);
/* torch.optim.SGD behind the same fused clip: d = g * coef + (weight_decay * decay_mult) * p; with momentum != 0:
 * buf = d at step 1, else momentum * buf + (1 - dampening) * d, and d = d + momentum * buf (nesterov) or buf; then
 * p -= (lr * lr_mult) * d.  buf is read and written only with momentum != 0 (may be NULL otherwise).  runs may be NULL with
 * nruns = 0: every multiplier is 1.
 * RADET_ERR_ARG: nesterov with dampening != 0 or momentum == 0 (torch raises), runs == NULL with nruns != 0 or the reverse,
 * nruns > RADET_OPT_MAX_RUNS, n >= 2^32, step < 1, grad_div <= 0, momentum != 0 with buf == NULL. */
int radet_sgd_step(float* p, const float* g, float* buf, size_t n, float lr, float momentum, float dampening,
                   float weight_decay, int nesterov, int step, float max_norm, float grad_div, const float* partials,
                   int npartials, float* grad_norm_out, const RadetOptRun* runs, int nruns, void* stream);
/* Gradient accumulation beside the gradient arena (which every backward pass overwrites): mode 0 acc = g, mode 1 acc += g,
 * mode 2 g = acc + g with acc left as it is (the last micro-step: clip and optimizer then run on g unchanged).
 * RADET_ERR_ARG for any other mode. */
int radet_grad_accumulate(float* acc, float* g, size_t n, int mode, void* stream);
/* Weight EMA (mmcv's EMAHook, `ema.mul_(1 - m).add_(param, alpha=m)`): per element t = fl32(ema * one_minus), then
 * ema = fma(momentum, p, t) with its single rounding -- torch's CPU arithmetic bit for bit.  momentum and one_minus are m and
 * 1 - m, each formed in double by the caller and rounded once to fp32.  p is only read.  Moves 12 bytes per element, like
 * radet_grad_accumulate's mode 1.
 * radet_ema_swap exchanges a and b exactly (evaluation and checkpoints see the EMA weights, then they are swapped back).
 * Both take any n (64-bit index math) and any float-aligned base: 16-byte accesses over the aligned body when the two
 * pointers share their offset inside a 16-byte line (up to 3 head elements are peeled), element accesses otherwise.
 * n == 0 launches nothing and returns 0.  RADET_ERR_ARG with n > 0: a NULL or not 4-byte-aligned pointer, arrays that
 * overlap. */
int radet_ema_update(float* ema, const float* p, size_t n, float momentum, float one_minus, void* stream);
int radet_ema_swap(float* a, float* b, size_t n, void* stream);

/* ---- COCO-protocol box evaluation (radet_amd/datasets/cocoeval.py:COCOeval, the yardstick: both entry points equal it bit
 *      for bit; IEEE fp64 + - * / and comparisons only).
 *      A segment is one (category, image) pair, numbered category * n_images + image in the evaluator's (sorted) id order --
 *      one per image with useCats = 0.  Ground truths [gt_off[s], gt_off[s+1]) and detections [dt_off[s], dt_off[s+1]) belong
 *      to segment s; detections of a segment are in descending-score order (stable), cut to maxDets[-1].
 *      A segment may hold at most RADET_COCO_MAX_GT ground truths (the IoU row and the visiting orders live in LDS):
 *      max_seg_gt above it makes radet_coco_match return RADET_ERR_COCO_OVERSIZE before anything is launched or written.
 *      Also required: n_area <= 8 and n_area * n_thr <= 64 (one lane per pair), else -1. */
#define RADET_COCO_MAX_GT 512
#define RADET_ERR_COCO_OVERSIZE -3
/* dt_xyxy f32[D,4]: the detector's corners (x, y, w = x2 - x1, h = y2 - y1, area = w * h are formed in fp64);
 * gt_xywh f64[G,4], gt_area f64[G] (the annotation's `area`), gt_flags u8[G]: bit 0 iscrowd, bit 1 "annotation id is 0" (which
 * the host evaluator reads as unmatched); iou_thrs f64[n_thr]; area_rng f64[n_area,2] (closed ranges).
 * Outputs, with c = a * n_thr + t: dt_match i32[D, n_area*n_thr] index of the matched gt inside its segment (-1: none),
 * dt_flag u8[D, n_area*n_thr] bit 0 matched, bit 1 dtIgnore; gt_match i32[G, n_area*n_thr] rank of the matching detection
 * inside its segment (the caller pre-fills -1); gt_ignore u8[G, n_area]. */
int radet_coco_match(const float* dt_xyxy, const int* dt_off, const double* gt_xywh, const double* gt_area,
                     const uint8_t* gt_flags, const int* gt_off, int nseg, int max_seg_gt, const double* iou_thrs, int n_thr,
                     const double* area_rng, int n_area, int* dt_match, uint8_t* dt_flag, int* gt_match, uint8_t* gt_ignore,
                     void* stream);
/* The detections of category k are rows [dt_cat_off[k], dt_cat_off[k+1]) of dt_flag_sorted u8[D, A*T] / dt_rank_sorted i32[D]
 * (rank inside the segment) / dt_score_sorted f32[D], stable-sorted by descending score over all images; its ground truths are
 * rows [gt_cat_off[k], gt_cat_off[k+1]) of gt_ignore.  Writes precision f64[T,R,K,A,M], recall f64[T,K,A,M] and scores
 * f64[T,R,K,A,M] where the host evaluator writes them; the caller pre-fills -1. */
int radet_coco_accumulate(const uint8_t* dt_flag_sorted, const int* dt_rank_sorted, const float* dt_score_sorted,
                          const int* dt_cat_off, const uint8_t* gt_ignore, const int* gt_cat_off, const int* max_dets,
                          const double* rec_thrs, int T, int R, int K, int A, int M, double* precision, double* recall,
                          double* scores, void* stream);

/* ---- launch tape (round 6): the host side of a steady-state train step as ONE call.  The reference drives its step from
 *      Python, one autograd node and one cuDNN / ATen launch at a time (mmcv's EpochBasedRunner.train -> model.train_step ->
 *      radet/models/detectors/base.py:218-253 -> optimizer hook); here a step is ~250 C-ABI calls on four HIP streams, and
 *      issuing them from Python costs ~19 us each -- 4.5-4.9 ms of host time per step, which bounds the bf16-storage step and
 *      would bound every step on a node whose ranks share the host.  A tape is a host array of RadetTapeOp recorded from one
 *      eager step (radet_amd/tape.py): every entry point of this header that was called, with its argument values, and the
 *      event record / wait operations between the streams.  radet_tape_replay issues ops [first, last) in order -- exactly the
 *      calls the eager step made, so results are bit-identical -- without re-entering Python.  Arguments that change from step
 *      to step (input / target pointers, learning rate, step number) are patched in the array by the owner before the call.
 *      Not a hipGraph: the launches stay ordinary stream-ordered launches (graphs measured slower here), the
 *      gradient exchange stays in Python between two replayed segments. */
typedef struct RadetTapeOp {
    int32_t kind;        /* 0: call thunk `fn` with args; 1: hipEventRecord(event, stream); 2: hipStreamWaitEvent(stream, event) */
    int32_t fn;          /* kind 0: index returned by radet_tape_fn_index */
    void* stream;        /* kind 1 / 2 (host handle: hipStream_t) */
    void* event;         /* kind 1 / 2 (host handle: hipEvent_t) */
    uint64_t args[32];   /* kind 0: one 64-bit word per argument in declaration order: pointers / size_t as is, int sign-extended,
                            float as its bit pattern in the low 32 bits */
} RadetTapeOp;
int radet_tape_fn_index(const char* name);    /* index of an `int radet_*(...)` entry point of this header, -1 if unknown (host) */
/* issues ops[first .. last); stops at the first op that fails: returns its code and stores its index in *failed (host, may be
 * NULL); 0 when all were issued */
int radet_tape_replay(const RadetTapeOp* ops, int first, int last, int* failed);
/* stream-ordered helpers a taped step uses instead of torch's fill / copy (hipMemsetAsync / hipMemcpyAsync device to device) */
int radet_fill_zero(void* dst, size_t nbytes, void* stream);
/* a HIP stream whose kernels may only run on the compute units whose bit is set in cu_mask (host array of nwords 32-bit words, bit i
 * of word w = CU 32 w + i; hipExtStreamCreateWithCUMask): the engine's weight-gradient streams can be kept off a share of the CUs
 * so that the dependent dgrad chain always finds free ones (experiment switch RADET_WGRAD_CU_MASK).  *stream_out: hipStream_t (host) */
int radet_stream_create_cumask(const uint32_t* cu_mask, int nwords, void** stream_out);
int radet_copy_d2d(void* dst, const void* src, size_t nbytes, void* stream);

/* ---- segmented copy between arbitrary device byte addresses (csrc/copy.hip): the sample cache's gather (HBM arena -> a
 *      batch's packed source buffer) and insert (buffer -> arena), one launch for a whole table.
 *      desc (device) = n rows of COPY_DESC_INTS ints: {source address lo, hi, destination address lo, hi, bytes, first tile}.
 *      A row owns ((destination & 15) + bytes + COPY_TILE_BYTES - 1) / COPY_TILE_BYTES tiles (none for bytes <= 0);
 *      `first tile` is the exclusive prefix sum of those counts over the rows and n_tiles their total (one workgroup per
 *      tile, so rows of very different sizes share the device evenly).  Any source / destination alignment; rows may not
 *      overlap each other's destinations.  Only bytes of [source, source + bytes) are read and only bytes of
 *      [destination, destination + bytes) are written, whatever the tile column holds.
 *      Returns RADET_ERR_ARG for n < 0, n_tiles < 0 or a NULL table with n > 0; n = 0 launches nothing. */
#define COPY_DESC_INTS 6
#define COPY_TILE_BYTES 16384
int radet_copy_segments(const int* desc, int n, int n_tiles, void* stream);

#ifdef __cplusplus
}
#endif
#endif
