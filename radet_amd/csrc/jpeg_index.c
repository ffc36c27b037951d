/* radet_jpeg_index: the serial seam of device JPEG decoding.  One walk over the entropy-coded data of a baseline scan that
 * decodes every symbol (no arithmetic on coefficients beyond the DC sums) and writes an entry point every seg_mcus MCUs and
 * at every restart marker.  It is also the validator: a stream it accepts is one the device decoder cannot run off.
 * Plain C, host only. */
#include <stddef.h>
#include "jpeg_common.h"
#include "radet_hip.h"

int radet_jpeg_index(const uint8_t* file, int scan_lo, int scan_hi, int ncomp, const int* comp_blocks, const void* huff,
                     int n_mcus, int restart_interval, int seg_mcus, int* rows, int max_rows) {
    const RjHuff* H = (const RjHuff*)huff;
    if (!file || !comp_blocks || !huff || !rows || ncomp < 1 || ncomp > 3 || n_mcus < 1 || seg_mcus < 1 || scan_lo < 0 ||
        scan_hi < scan_lo || restart_interval < 0)
        return -RJ_E_COUNT;
    RjBits b;
    rj_start(&b, file, scan_lo, scan_hi);
    int pred[3] = {0, 0, 0}, nrows = 0, in_interval = 0, next_rst = 0;
    int* row = NULL;
    for (int m = 0; m < n_mcus; ++m) {
        if (restart_interval && m && in_interval == restart_interval) {
            /* whole bytes only, nothing real left in the reader, then FF.. Dn */
            b.n -= b.n & 7;
            if (b.n != b.fake) return -RJ_E_RESTART;
            int p = b.pos;
            while (p + 1 < scan_hi && file[p] == 0xFF && file[p + 1] == 0xFF) ++p;
            if (p + 1 >= scan_hi) return -RJ_E_EARLY;
            if (file[p] != 0xFF || file[p + 1] != 0xD0 + (next_rst & 7)) return -RJ_E_RESTART;
            next_rst++;
            rj_start(&b, file, p + 2, scan_hi);
            pred[0] = pred[1] = pred[2] = 0;
            in_interval = 0;
        }
        if (in_interval % seg_mcus == 0) {
            if (nrows == max_rows) return -RJ_E_ROWS;
            rj_fill(&b);
            int pos = rj_position(&b);
            row =rows + (size_t)nrows++ * RJ_ROW_INTS;
            row[RJ_OFF] = pos >> 3; row[RJ_BIT] = pos & 7; row[RJ_MCU0] = m; row[RJ_NMCU] = 0;
            row[RJ_PRED] = pred[0]; row[RJ_PRED + 1] = pred[1]; row[RJ_PRED + 2] = pred[2];
            row[RJ_END] = 0;
        }
        for (int c = 0; c < ncomp; ++c)
            for (int k = 0; k < comp_blocks[c]; ++k) {
                rj_fill(&b);
                int s = rj_symbol(&b, H + 2 * c);
                if (s < 0 || s > 15) return -RJ_E_CODE;
                pred[c] += rj_extend(rj_take(&b, s), s);
                if (b.n < b.fake) return -RJ_E_EARLY;
                for (int i = 1; i < 64;) {
                    rj_fill(&b);
                    int rs = rj_symbol(&b, H + 2 * c + 1);
                    if (rs < 0) return -RJ_E_CODE;
                    int r = rs >> 4;
                    s = rs & 15;
                    if (s == 0) {
                        if (b.n < b.fake) return -RJ_E_EARLY;
                        if (r != 15) break;
                        i += 16;
                        if (i > 64) return -RJ_E_INDEX;
                        continue;
                    }
                    i += r;
                    if (i > 63) return -RJ_E_INDEX;
                    rj_take(&b, s);
                    if (b.n < b.fake) return -RJ_E_EARLY;
                    ++i;
                }
            }
        row[RJ_NMCU]++;
        in_interval++;
        /* the segment's end: before a restart marker or the end of the scan it is where the last MCU stopped */
        row[RJ_END] = rj_position(&b);
    }
    /* more restart intervals than the frame has MCUs */
    {
        int p = b.pos;
        b.n -= b.n & 7;
        if (b.n == b.fake && p + 1 < scan_hi && file[p] == 0xFF && file[p + 1] >= 0xD0 && file[p + 1] <= 0xD7) return -RJ_E_COUNT;
    }
    return nrows;
}
