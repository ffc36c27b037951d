// Baseline-JPEG entropy reading shared by the host walker (jpeg_index.c, plain C) and the device decoder (jpeg.hip): the
// Huffman table record, the bit reader and the symbol decode.  Both sides run the SAME statements, so a position the walker
// writes into an index row is a position the device reader reproduces.
//
// A position in the entropy-coded data is (raw byte offset into the file, bit 0..7 inside that byte, MSB first).  The raw
// offset is the offset of a DATA byte: the 00 stuffed after an FF is never one.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define RJ_FN __device__ __host__ static inline
#else
#define RJ_FN static inline
#endif

#define RJ_LOOK_BITS 9
#define RJ_HUFF_BYTES 1424
// one Huffman table (built by radet_amd/core/jpeg.py:huff_record from a DHT segment)
typedef struct {
    uint16_t look[1 << RJ_LOOK_BITS];   // first 9 bits of the stream -> (length << 8) | symbol; 0: the code is longer
    int32_t maxcode[18];                // [l] largest code of length l (1..16), -1: none
    int32_t valoff[18];                 // [l] index into vals of code c of length l = c + valoff[l]
    uint8_t vals[256];
} RjHuff;

// index row (int32 x RJ_ROW_INTS): where a segment starts, what it covers, the DC predictors, where it must end
#define RJ_ROW_INTS 8
enum { RJ_OFF = 0, RJ_BIT = 1, RJ_MCU0 = 2, RJ_NMCU = 3, RJ_PRED = 4, RJ_END = 7 };   // RJ_END = end offset * 8 + end bit

// error bits (walker: return value -(bit); device: OR-ed into the image's error word)
enum { RJ_E_CODE = 1, RJ_E_INDEX = 2, RJ_E_EARLY = 4, RJ_E_RESTART = 8, RJ_E_COUNT = 16, RJ_E_END = 32, RJ_E_ROWS = 64 };

typedef struct {
    const uint8_t* p;   // the file
    int pos, end;       // next raw byte to load; one past the last byte that may be read
    uint64_t buf;       // the low n bits are the unread bits
    int n;
    int fake;           // how many of them (the lowest) are zeros fed after a marker or the end
    uint64_t adv;       // per loaded byte, newest in the low 8 bits: by how much loading it advanced pos (0 fake, 1, 2 stuffed)
} RjBits;

RJ_FN void rj_start(RjBits* b, const uint8_t* p, int pos, int end) {
    b->p = p; b->pos = pos; b->end = end; b->buf = 0; b->n = 0; b->fake = 0; b->adv = 0;
}

// load bytes until more than 56 bits are there; an FF 00 pair is one FF, any other FF xx (a marker) and the end feed zeros
RJ_FN void rj_fill(RjBits* b) {
    while (b->n <= 56) {
        unsigned v = 0, a = 0;
        if (b->pos < b->end) {
            v = b->p[b->pos];
            a = 1;
            if (v == 0xFF) {
                if (b->pos + 1 < b->end && b->p[b->pos + 1] == 0) a = 2;
                else { v = 0; a = 0; }
            }
        }
        b->pos += (int)a;
        if (a == 0) b->fake += 8;
        b->buf = (b->buf << 8) | v;
        b->adv = (b->adv << 8) | a;
        b->n += 8;
    }
}

RJ_FN unsigned rj_peek16(const RjBits* b) { return (unsigned)(b->buf >> (b->n - 16)) & 0xFFFFu; }

RJ_FN unsigned rj_take(RjBits* b, int k) {        // k <= 16 bits, k = 0 -> 0
    b->n -= k;
    return (unsigned)(b->buf >> b->n) & ((1u << k) - 1u);
}

// the position of the next unread bit, as offset * 8 + bit
RJ_FN int rj_position(const RjBits* b) {
    int k = (b->n + 7) >> 3, off = b->pos;
    uint64_t a = b->adv;
    for (int j = 0; j < k; ++j) { off -= (int)(a & 0xFF); a >>= 8; }
    return off * 8 + ((8 - (b->n & 7)) & 7);
}

// one Huffman symbol (rj_fill first); -1: no code of up to 16 bits matches
RJ_FN int rj_symbol(RjBits* b, const RjHuff* h) {
    unsigned c = rj_peek16(b);
    unsigned e = h->look[c >> (16 - RJ_LOOK_BITS)];
    if (e) { b->n -= (int)(e >> 8); return (int)(e & 0xFF); }
    for (int l = RJ_LOOK_BITS + 1; l <= 16; ++l) {
        int code = (int)(c >> (16 - l));
        if (code <= h->maxcode[l]) { b->n -= l; return h->vals[(code + h->valoff[l]) & 255]; }
    }
    return -1;
}

// HUFF_EXTEND: the s-bit magnitude v as a signed value
RJ_FN int rj_extend(unsigned v, int s) { return s && v < (1u << (s - 1)) ? (int)v - (1 << s) + 1 : (int)v; }

// zigzag position -> natural position
#define RJ_ZIGZAG {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, \
                   28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, \
                   54, 47, 55, 62, 63}
