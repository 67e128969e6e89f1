/* jpeg_entropy.h -- the serial half of a baseline JPEG decode: marker parse + Huffman pass of ONE tile stream -> quantised coefficients.
 *
 * Internal (not part of any installed ABI): C99 that is also valid C++, `static` functions only, no global state, no allocation.  Included by
 * jpeg_kernels.hip (the host threads of cerb_jpeg_read_tiles) and by tests/tools/jpeg_entropy_main.c (a stand-alone program the suite compiles with
 * the host sanitizers).  Everything after this pass -- dequantisation, inverse DCT, chroma up-sampling, colour conversion, placement -- is per-block /
 * per-pixel integer arithmetic and runs on the device (jpeg_kernels.hip; the arithmetic is stated in include/cerberus_hip.h).
 *
 * Input: a tile's byte stream and, optionally, the page's JPEGTables stream (TIFF tag 347).  The reader splices "tables minus EOI" + "tile minus
 * SOI" for libjpeg; parsing the two streams one after the other into the same table state is the same thing.
 *
 * Accepted: SOF0 / SOF1, 8-bit precision, Huffman coding, ONE interleaved scan of 3 components with sampling (1x1 | 2x1 | 2x2, 1x1, 1x1), DRI / RSTn,
 * 8- and 16-bit quantisation tables, any APPn / COM.  Everything else a JPEG may be (progressive, arithmetic, lossless, 12-bit, 1 or 4 components,
 * other sampling factors, several scans) is CERB_JPEG_UNSUPPORTED: not an error, the caller decodes such a tile another way.  A truncated stream, a
 * bad Huffman table or code, a coefficient index past 63, a missing table, a marker (or the end) where entropy-coded data was expected are
 * CERB_JPEG_CORRUPT.  Never reads past n_src, never writes past coef_cap.
 *
 * Output: cerb_jpeg_hdr (size, sampling, the three quantisation tables de-zigzagged, the colour decision, the MCU grid) and the QUANTISED
 * coefficients as int16 in natural (row-major 8 x 8) order: component 0's raster of (mcu_rows * v0) x (mcu_cols * h0) blocks of 64, then component
 * 1's, then component 2's.  A DC prediction that leaves int16 wraps (only hostile streams get there).
 *
 * Colour decision = what libjpeg decides for the stream the reader hands it today (reader.TiffReader._decode):
 *   page photometric 2 -> none (the reader forces it with an Adobe transform-0 segment); else a JFIF APP0 seen -> YCbCr; else an Adobe APP14 seen ->
 *   its transform byte (0 none, anything else YCbCr); else component ids 1, 2, 3 -> YCbCr, 'R', 'G', 'B' -> none, anything else -> YCbCr. */
#ifndef CERB_JPEG_ENTROPY_H
#define CERB_JPEG_ENTROPY_H
#include <stdint.h>
#include <string.h>

#define CERB_JPEG_OK 0
#define CERB_JPEG_UNSUPPORTED 1
#define CERB_JPEG_CORRUPT (-1)
#define CERB_JPEG_TOO_LARGE (-2) /* the coefficients do not fit coef_cap: nothing was written */

typedef struct cerb_jpeg_hdr {
    int32_t status;             /* CERB_JPEG_OK / _UNSUPPORTED / _CORRUPT: the device kernels skip every tile whose status is not 0 */
    int32_t width, height;
    int32_t h[3], v[3];         /* sampling factors */
    int32_t transform;          /* 1: the components are Y, Cb, Cr and are converted; 0: they are R, G, B */
    int32_t mcu_cols, mcu_rows;
    int32_t gx0, gy0;           /* where the tile lies in its level (filled in by the window call) */
    int32_t reserved[4];         /* (keeps q on a 16-byte boundary: the device loads its rows as vectors) */
    int64_t coef_off;           /* first coefficient of the tile in the window's coefficient buffer, in int16 units (filled in by the window call);
                                   the tile's component planes start at the same offset, in bytes, in the device scratch */
    uint16_t q[3][64];          /* per component, natural order */
} cerb_jpeg_hdr;

typedef struct cerb_jpeg_huff {
    int32_t maxcode[17];        /* largest code of length l, -1 when there is none */
    int32_t delta[17];          /* index of the first symbol of length l minus its code */
    uint16_t look[512];         /* next 9 bits -> (length << 8) | symbol, 0 when the code is longer */
    int16_t fast_ac[512];       /* AC tables: next 9 bits -> (value << 8) | (run << 4) | (code + value bits) when both fit in them, else 0 */
    uint8_t vals[256];
    int32_t defined;
} cerb_jpeg_huff;

typedef struct cerb_jpeg_state {
    cerb_jpeg_huff dc[4], ac[4];
    uint16_t q[4][64];
    int32_t q_defined[4];
    int32_t saw_jfif, saw_adobe, adobe_transform;
    int32_t have_sof, width, height;
    int32_t cid[3], h[3], v[3], tq[3], td[3], ta[3];
    int32_t restart;
} cerb_jpeg_state;

static const uint8_t cerb_jpeg_zigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                             41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                             30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

static int cerb_jpeg_build_huff(cerb_jpeg_huff* t, const uint8_t* bits /* [16] */, const uint8_t* vals, int n_vals, int is_dc) {
    int32_t code = 0, k = 0;
    memset(t->look, 0, sizeof(t->look));
    memset(t->vals, 0, sizeof(t->vals));
    for (int i = 0; i < n_vals; ++i) {
        if (is_dc && vals[i] > 15) return CERB_JPEG_CORRUPT;
        t->vals[i] = vals[i];
    }
    t->maxcode[0] = -1;
    t->delta[0] = 0;
    for (int l = 1; l <= 16; ++l) {
        const int32_t cnt = bits[l - 1];
        t->delta[l] = k - code;
        if (code + cnt > ((int32_t)1 << l)) return CERB_JPEG_CORRUPT; /* more codes of this length than the prefix leaves room for */
        if (l <= 9) {
            for (int32_t c = 0; c < cnt; ++c) {
                const uint16_t e = (uint16_t)((l << 8) | t->vals[k + c]);
                const int32_t first = (code + c) << (9 - l);
                for (int32_t f = 0; f < ((int32_t)1 << (9 - l)); ++f) t->look[first + f] = e;
            }
        }
        code += cnt;
        k += cnt;
        t->maxcode[l] = cnt ? code - 1 : -1;
        code <<= 1;
    }
    memset(t->fast_ac, 0, sizeof(t->fast_ac));
    if (!is_dc) {
        for (int32_t i = 0; i < 512; ++i) {
            const int l = t->look[i] >> 8, run = (t->look[i] >> 4) & 15, sz = t->look[i] & 15;
            if (!t->look[i] || !sz || l + sz > 9) continue;
            int32_t v = ((i << l) & 511) >> (9 - sz);
            if (v < ((int32_t)1 << (sz - 1))) v -= ((int32_t)1 << sz) - 1;
            if (v >= -128 && v <= 127) t->fast_ac[i] = (int16_t)(v * 256 + run * 16 + l + sz);
        }
    }
    t->defined = 1;
    return CERB_JPEG_OK;
}

static void cerb_jpeg_state_init(cerb_jpeg_state* s) { memset(s, 0, sizeof(*s)); }

/* Marker segments of one stream from its SOI on.  tables_only: a JPEGTables stream (ends at EOI or at the end of the bytes).  Otherwise the parse
 * stops behind the SOS header and *scan_pos is where the entropy-coded data starts. */
static int cerb_jpeg_parse(cerb_jpeg_state* s, const uint8_t* src, int64_t n, int tables_only, int64_t* scan_pos) {
    int64_t p = 2;
    if (n < 2 || src[0] != 0xFF || src[1] != 0xD8) return CERB_JPEG_CORRUPT;
    for (;;) {
        if (p >= n) return tables_only ? CERB_JPEG_OK : CERB_JPEG_CORRUPT;
        if (src[p] != 0xFF) return CERB_JPEG_CORRUPT;
        while (p < n && src[p] == 0xFF) ++p;
        if (p >= n) return CERB_JPEG_CORRUPT;
        const int m = src[p++];
        if (m == 0xD9) return tables_only ? CERB_JPEG_OK : CERB_JPEG_CORRUPT; /* EOI before any scan */
        if (m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;                  /* TEM / a stray RSTn: no parameters */
        if (m == 0x00 || m == 0xD8) return CERB_JPEG_CORRUPT;
        if (p + 2 > n) return CERB_JPEG_CORRUPT;
        const int64_t len = ((int64_t)src[p] << 8) | src[p + 1];
        if (len < 2 || p + len > n) return CERB_JPEG_CORRUPT;
        const uint8_t* seg = src + p + 2;
        int64_t sl = len - 2;
        p += len;
        if (m == 0xC0 || m == 0xC1) {
            if (s->have_sof || sl < 6) return CERB_JPEG_CORRUPT;
            if (seg[0] != 8) return CERB_JPEG_UNSUPPORTED; /* 12-bit */
            s->height = (seg[1] << 8) | seg[2];
            s->width = (seg[3] << 8) | seg[4];
            const int nf = seg[5];
            if (sl < 6 + 3 * (int64_t)nf) return CERB_JPEG_CORRUPT;
            if (nf != 3 || s->height == 0 || s->width == 0) return CERB_JPEG_UNSUPPORTED; /* grey / CMYK; a height left to a DNL segment */
            for (int i = 0; i < 3; ++i) {
                s->cid[i] = seg[6 + 3 * i];
                s->h[i] = seg[7 + 3 * i] >> 4;
                s->v[i] = seg[7 + 3 * i] & 15;
                s->tq[i] = seg[8 + 3 * i];
                if (s->tq[i] > 3 || s->h[i] < 1 || s->h[i] > 4 || s->v[i] < 1 || s->v[i] > 4) return CERB_JPEG_CORRUPT;
            }
            if (s->h[1] != 1 || s->v[1] != 1 || s->h[2] != 1 || s->v[2] != 1 ||
                !((s->h[0] == 1 && s->v[0] == 1) || (s->h[0] == 2 && s->v[0] == 1) || (s->h[0] == 2 && s->v[0] == 2)))
                return CERB_JPEG_UNSUPPORTED;
            s->have_sof = 1;
        } else if ((m >= 0xC2 && m <= 0xCF && m != 0xC4) || m == 0xDE || m == 0xDF) {
            return CERB_JPEG_UNSUPPORTED; /* progressive, lossless, differential, arithmetic (SOFn, JPG, DAC), hierarchical (DHP, EXP) */
        } else if (m == 0xC4) {
            while (sl > 0) {
                if (sl < 17) return CERB_JPEG_CORRUPT;
                const int tc = seg[0] >> 4, th = seg[0] & 15;
                int cnt = 0;
                for (int i = 1; i <= 16; ++i) cnt += seg[i];
                if (tc > 1 || th > 3 || cnt > 256 || sl < 17 + cnt) return CERB_JPEG_CORRUPT;
                if (cerb_jpeg_build_huff(tc ? &s->ac[th] : &s->dc[th], seg + 1, seg + 17, cnt, tc == 0) != CERB_JPEG_OK) return CERB_JPEG_CORRUPT;
                seg += 17 + cnt;
                sl -= 17 + cnt;
            }
        } else if (m == 0xDB) {
            while (sl > 0) {
                const int pq = seg[0] >> 4, tq = seg[0] & 15;
                if (pq > 1 || tq > 3 || sl < 1 + 64 * (pq + 1)) return CERB_JPEG_CORRUPT;
                for (int k = 0; k < 64; ++k)
                    s->q[tq][cerb_jpeg_zigzag[k]] = pq ? (uint16_t)((seg[1 + 2 * k] << 8) | seg[2 + 2 * k]) : (uint16_t)seg[1 + k];
                s->q_defined[tq] = 1;
                seg += 1 + 64 * (pq + 1);
                sl -= 1 + 64 * (pq + 1);
            }
        } else if (m == 0xDD) {
            if (sl < 2) return CERB_JPEG_CORRUPT;
            s->restart = (seg[0] << 8) | seg[1];
        } else if (m == 0xE0) {
            if (sl >= 14 && memcmp(seg, "JFIF\0", 5) == 0) s->saw_jfif = 1;
        } else if (m == 0xEE) {
            if (sl >= 12 && memcmp(seg, "Adobe", 5) == 0) {
                s->saw_adobe = 1;
                s->adobe_transform = seg[11];
            }
        } else if (m == 0xDA) {
            if (tables_only || !s->have_sof || sl < 1) return CERB_JPEG_CORRUPT;
            const int ns = seg[0];
            if (ns < 1 || ns > 4 || sl < 4 + 2 * (int64_t)ns) return CERB_JPEG_CORRUPT;
            if (ns != 3) return CERB_JPEG_UNSUPPORTED; /* one scan per component */
            for (int i = 0; i < 3; ++i) {
                if (seg[1 + 2 * i] != s->cid[i]) return CERB_JPEG_UNSUPPORTED;
                s->td[i] = seg[2 + 2 * i] >> 4;
                s->ta[i] = seg[2 + 2 * i] & 15;
                if (s->td[i] > 3 || s->ta[i] > 3) return CERB_JPEG_CORRUPT;
                if (!s->dc[s->td[i]].defined || !s->ac[s->ta[i]].defined || !s->q_defined[s->tq[i]]) return CERB_JPEG_CORRUPT; /* a missing table */
            }
            if (seg[7] != 0 || seg[8] != 63 || seg[9] != 0) return CERB_JPEG_UNSUPPORTED;
            *scan_pos = p;
            return CERB_JPEG_OK;
        }
        /* every other segment (APPn, COM, DNL, ...) is skipped */
    }
}

/* The header of a parsed stream; returns the number of coefficients (int16) its scan holds. */
static int64_t cerb_jpeg_fill_hdr(const cerb_jpeg_state* s, int photometric_rgb, cerb_jpeg_hdr* hdr) {
    memset(hdr, 0, sizeof(*hdr));
    hdr->width = s->width;
    hdr->height = s->height;
    int64_t blocks = 0;
    hdr->mcu_cols = (s->width + 8 * s->h[0] - 1) / (8 * s->h[0]);
    hdr->mcu_rows = (s->height + 8 * s->v[0] - 1) / (8 * s->v[0]);
    for (int i = 0; i < 3; ++i) {
        hdr->h[i] = s->h[i];
        hdr->v[i] = s->v[i];
        memcpy(hdr->q[i], s->q[s->tq[i]], sizeof(hdr->q[i]));
        blocks += (int64_t)hdr->mcu_cols * hdr->mcu_rows * s->h[i] * s->v[i];
    }
    if (photometric_rgb) hdr->transform = 0;
    else if (s->saw_jfif) hdr->transform = 1;
    else if (s->saw_adobe) hdr->transform = s->adobe_transform != 0;
    else hdr->transform = !(s->cid[0] == 'R' && s->cid[1] == 'G' && s->cid[2] == 'B');
    return blocks * 64;
}

typedef struct cerb_jpeg_bits {
    const uint8_t* src;
    int64_t p, n;
    uint64_t acc; /* the low cnt bits are valid */
    int cnt, stop;
} cerb_jpeg_bits;

/* Top the bit buffer up to more than 56 bits; stops for good at a marker, at a lone 0xFF at the end and at the end of the bytes. */
static void cerb_jpeg_fill(cerb_jpeg_bits* b) {
    if (b->cnt <= 32 && !b->stop && b->p + 4 <= b->n) { /* four plain bytes at once */
        const uint8_t* q = b->src + b->p;
        if (q[0] != 0xFF && q[1] != 0xFF && q[2] != 0xFF && q[3] != 0xFF) {
            b->acc = (b->acc << 32) | ((uint32_t)q[0] << 24) | ((uint32_t)q[1] << 16) | ((uint32_t)q[2] << 8) | q[3];
            b->cnt += 32;
            b->p += 4;
        }
    }
    while (b->cnt <= 56 && !b->stop) {
        if (b->p >= b->n) {
            b->stop = 1;
            break;
        }
        const uint8_t x = b->src[b->p];
        if (x == 0xFF) {
            if (b->p + 1 >= b->n || b->src[b->p + 1] != 0) {
                b->stop = 1;
                break;
            }
            b->p += 2;
        } else {
            b->p += 1;
        }
        b->acc = (b->acc << 8) | x;
        b->cnt += 8;
    }
}

/* the next k (1 .. 16) bits without consuming them, zero-padded where the data ends */
static uint32_t cerb_jpeg_peek(const cerb_jpeg_bits* b, int k) {
    const uint64_t v = b->cnt >= k ? b->acc >> (b->cnt - k) : b->acc << (k - b->cnt);
    return (uint32_t)(v & (((uint64_t)1 << k) - 1));
}

/* one Huffman symbol, or -1 (no such code, or the data ended inside it) */
static int cerb_jpeg_symbol(cerb_jpeg_bits* b, const cerb_jpeg_huff* t) {
    const uint16_t e = t->look[cerb_jpeg_peek(b, 9)];
    if (e) {
        const int l = e >> 8;
        if (l > b->cnt) return -1;
        b->cnt -= l;
        return e & 255;
    }
    for (int l = 10; l <= 16; ++l) {
        const int32_t c = (int32_t)cerb_jpeg_peek(b, l);
        if (c <= t->maxcode[l]) {
            if (l > b->cnt) return -1;
            b->cnt -= l;
            return t->vals[(c + t->delta[l]) & 255];
        }
    }
    return -1;
}

/* s (1 .. 15) bits as the signed value of magnitude category s; *ok = 0 when the data ended */
static int32_t cerb_jpeg_receive(cerb_jpeg_bits* b, int s, int* ok) {
    if (s > b->cnt) {
        *ok = 0;
        return 0;
    }
    const int32_t v = (int32_t)cerb_jpeg_peek(b, s);
    b->cnt -= s;
    return v < ((int32_t)1 << (s - 1)) ? v - (((int32_t)1 << s) - 1) : v;
}

/* The scan of a parsed stream: coefs must hold what cerb_jpeg_fill_hdr returned. */
static int cerb_jpeg_scan(const cerb_jpeg_state* s, const cerb_jpeg_hdr* hdr, const uint8_t* src, int64_t n, int64_t scan_pos, int16_t* coefs) {
    cerb_jpeg_bits b;
    b.src = src; b.p = scan_pos; b.n = n; b.acc = 0; b.cnt = 0; b.stop = 0;
    int16_t* base[3];
    int64_t across[3];
    {
        int64_t off = 0;
        for (int i = 0; i < 3; ++i) {
            base[i] = coefs + off;
            across[i] = (int64_t)hdr->mcu_cols * s->h[i];
            off += across[i] * hdr->mcu_rows * s->v[i] * 64;
        }
        memset(coefs, 0, (size_t)off * sizeof(int16_t));
    }
    int32_t pred[3] = {0, 0, 0};
    int64_t done = 0;
    int next_rst = 0;
    for (int my = 0; my < hdr->mcu_rows; ++my) {
        for (int mx = 0; mx < hdr->mcu_cols; ++mx, ++done) {
            if (s->restart && done && done % s->restart == 0) {
                /* the bits left over are padding; fill() never went past the marker */
                int64_t p = b.p;
                if (p >= n || src[p] != 0xFF) return CERB_JPEG_CORRUPT;
                while (p < n && src[p] == 0xFF) ++p;
                if (p >= n || src[p] != 0xD0 + next_rst) return CERB_JPEG_CORRUPT;
                next_rst = (next_rst + 1) & 7;
                b.p = p + 1; b.acc = 0; b.cnt = 0; b.stop = 0;
                pred[0] = pred[1] = pred[2] = 0;
            }
            for (int ci = 0; ci < 3; ++ci) {
                const cerb_jpeg_huff* dc = &s->dc[s->td[ci]];
                const cerb_jpeg_huff* ac = &s->ac[s->ta[ci]];
                for (int by = 0; by < s->v[ci]; ++by) {
                    for (int bx = 0; bx < s->h[ci]; ++bx) {
                        int16_t* blk = base[ci] + (((int64_t)my * s->v[ci] + by) * across[ci] + (int64_t)mx * s->h[ci] + bx) * 64;
                        int ok = 1;
                        if (b.cnt < 32) cerb_jpeg_fill(&b); /* a code and its value take 31 bits at most */
                        int sym = cerb_jpeg_symbol(&b, dc);
                        if (sym < 0) return CERB_JPEG_CORRUPT;
                        if (sym) pred[ci] = (int16_t)(pred[ci] + cerb_jpeg_receive(&b, sym, &ok));
                        if (!ok) return CERB_JPEG_CORRUPT;
                        blk[0] = (int16_t)pred[ci];
                        for (int k = 1; k < 64;) {
                            if (b.cnt < 32) cerb_jpeg_fill(&b);
                            const int32_t fa = ac->fast_ac[cerb_jpeg_peek(&b, 9)];
                            if (fa) { /* run, size and a small value out of one look-up */
                                if ((fa & 15) > b.cnt) return CERB_JPEG_CORRUPT;
                                k += (fa >> 4) & 15;
                                if (k > 63) return CERB_JPEG_CORRUPT;
                                b.cnt -= fa & 15;
                                blk[cerb_jpeg_zigzag[k++]] = (int16_t)(fa >> 8);
                                continue;
                            }
                            sym = cerb_jpeg_symbol(&b, ac);
                            if (sym < 0) return CERB_JPEG_CORRUPT;
                            const int r = sym >> 4, sz = sym & 15;
                            if (sz == 0) {
                                if (r != 15) break; /* end of block */
                                k += 16;
                                continue;
                            }
                            k += r;
                            if (k > 63) return CERB_JPEG_CORRUPT; /* a coefficient index past 63 */
                            blk[cerb_jpeg_zigzag[k]] = (int16_t)cerb_jpeg_receive(&b, sz, &ok);
                            if (!ok) return CERB_JPEG_CORRUPT;
                            ++k;
                        }
                    }
                }
            }
        }
    }
    return CERB_JPEG_OK;
}

/* Both streams' segments into one state: 0, or the status that ends the decode.  *scan_pos: the tile's entropy-coded data. */
static int cerb_jpeg_parse_tile(cerb_jpeg_state* s, const uint8_t* tables, int64_t n_tables, const uint8_t* src, int64_t n_src, int64_t* scan_pos) {
    cerb_jpeg_state_init(s);
    if (tables && n_tables > 0) {
        const int rc = cerb_jpeg_parse(s, tables, n_tables, 1, scan_pos);
        if (rc != CERB_JPEG_OK) return rc;
    }
    return cerb_jpeg_parse(s, src, n_src, 0, scan_pos);
}

/* One tile, start to end.  hdr->status is the return value; *coef_used: the coefficients written (int16 units). */
static int cerb_jpeg_entropy_decode(const uint8_t* tables, int64_t n_tables, const uint8_t* src, int64_t n_src, int photometric_rgb,
                                    cerb_jpeg_hdr* hdr, int16_t* coefs, int64_t coef_cap, int64_t* coef_used) {
    cerb_jpeg_state s;
    int64_t scan_pos = 0;
    if (coef_used) *coef_used = 0;
    memset(hdr, 0, sizeof(*hdr));
    int rc = cerb_jpeg_parse_tile(&s, tables, n_tables, src, n_src, &scan_pos);
    if (rc == CERB_JPEG_OK) {
        const int64_t need = cerb_jpeg_fill_hdr(&s, photometric_rgb, hdr);
        if (need > coef_cap) rc = CERB_JPEG_TOO_LARGE;
        else {
            rc = cerb_jpeg_scan(&s, hdr, src, n_src, scan_pos, coefs);
            if (rc == CERB_JPEG_OK && coef_used) *coef_used = need;
        }
    }
    hdr->status = rc;
    return rc;
}

#endif /* CERB_JPEG_ENTROPY_H */
