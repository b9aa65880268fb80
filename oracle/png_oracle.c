/*
 * png_oracle.c -- CPU ORACLE for the lossless PNG row of the hot path.
 *
 * TEST INFRASTRUCTURE ONLY (tests/, __graft_entry__.smoke(), tools/): nothing under caesium-clt_amd/ links or calls this.
 *
 * PARITY UNPINNED.  The reference reaches this path through `caesium::compress_in_memory` with `png.optimize = true`
 * (/root/reference/src/compressor.rs:305, parameters :427-429, level :64 of src/options.rs), which runs oxipng 9.1.5 +
 * libdeflate 1.25.2 (Cargo.lock:1161, :917-932).  Neither is in /root/reference nor in this image, and the reference's
 * tests hold no PNG golden bytes, so byte parity with the real tool cannot be established here.  What this
 * file pins instead:
 *   - decode (chunk walk, RFC 1950/1951 inflate, PNG unfilter): pixel-exact against libpng via Pillow
 *     (tests/test_oracle_png.py), on every colour type / bit depth Pillow can write;
 *   - the output is a valid PNG whose pixels equal the input's (Pillow decodes both), and a valid zlib stream (zlib
 *     inflates it);
 *   - the row-filter strategies follow the numbering oxipng documents (0-4 fixed, 5 MinSum, 6 Entropy, 7 Bigrams,
 *     8 BigEnt, 9 Brute) and the trial sets of its presets (-o3: filters 0,7,8,9) [UPSTREAM-RECALL]; their scoring is
 *     restated from the published heuristics (LodePNG's, which oxipng adopted): see filter_scores();
 *   - the DEFLATE coder is THIS PROJECT'S OWN (a chunk-parallel LZ77 + dynamic Huffman coder laid out for the GPU,
 *     deflate_chunk()), not libdeflate's near-optimal parser: sizes differ from the reference's by a few percent, the
 *     decoded pixels do not.  The device path (k_png_*.hip) must equal this file byte for byte.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "png_oracle.h"
#include "webp_oracle.h"
#include "../include/png_quality_table.h"

/* ------------------------------------------------------------------------------------------------ checksums */
static uint32_t crc_table[256];
static void crc_init(void) {
    if (crc_table[1]) return;
    for (uint32_t n = 0; n < 256; n++) {
        uint32_t c = n;
        for (int k = 0; k < 8; k++) c = (c & 1) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
        crc_table[n] = c;
    }
}
uint32_t cso_crc32(uint32_t crc, const uint8_t *p, size_t n) {
    crc_init();
    crc = ~crc;
    for (size_t i = 0; i < n; i++) crc = crc_table[(crc ^ p[i]) & 255] ^ (crc >> 8);
    return ~crc;
}
uint32_t cso_adler32(const uint8_t *p, size_t n) {
    uint32_t a = 1, b = 0;
    for (size_t i = 0; i < n; i++) { a = (a + p[i]) % 65521u; b = (b + a) % 65521u; }
    return (b << 16) | a;
}
static uint32_t be32(const uint8_t *p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }
static void put_be32(uint8_t *p, uint32_t v) { p[0] = (uint8_t)(v >> 24); p[1] = (uint8_t)(v >> 16); p[2] = (uint8_t)(v >> 8); p[3] = (uint8_t)v; }

/* ------------------------------------------------------------------------------------------------ inflate (RFC 1951) */
typedef struct { const uint8_t *in; size_t n, pos; uint32_t bitbuf; int bitcnt; int err; } ibits;
static uint32_t need(ibits *s, int n) {
    uint32_t v = s->bitbuf;
    while (s->bitcnt < n) {
        if (s->pos >= s->n) { s->err = 1; return 0; }
        v |= (uint32_t)s->in[s->pos++] << s->bitcnt;
        s->bitcnt += 8;
    }
    s->bitbuf = n < 32 ? v >> n : 0;
    s->bitcnt -= n;
    return v & ((n < 32 ? (1u << n) : 0u) - 1u);
}
typedef struct { uint16_t count[16], symbol[288]; } hcode;
/* canonical code from lengths; returns 0 complete, >0 incomplete, <0 over-subscribed */
static int hbuild(hcode *h, const uint8_t *len, int n) {
    uint16_t offs[16];
    memset(h->count, 0, sizeof h->count);
    for (int i = 0; i < n; i++) h->count[len[i]]++;
    if (h->count[0] == n) return 0;
    int left = 1;
    for (int l = 1; l < 16; l++) { left <<= 1; left -= h->count[l]; if (left < 0) return left; }
    offs[1] = 0;
    for (int l = 1; l < 15; l++) offs[l + 1] = offs[l] + h->count[l];
    for (int i = 0; i < n; i++) if (len[i]) h->symbol[offs[len[i]]++] = (uint16_t)i;
    return left;
}
static int hdecode(ibits *s, const hcode *h) {
    int code = 0, first = 0, index = 0;
    for (int l = 1; l < 16; l++) {
        code |= (int)need(s, 1);
        if (s->err) return -1;
        int count = h->count[l];
        if (code - count < first) return h->symbol[index + (code - first)];
        index += count; first += count; first <<= 1; code <<= 1;
    }
    return -1;
}
static const uint16_t LEN_BASE[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
static const uint8_t LEN_EXTRA[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
static const uint16_t DIST_BASE[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
static const uint8_t DIST_EXTRA[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
static const uint8_t CL_ORDER[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

/* raw deflate -> out (capacity cap).  Stops at the final block, or as soon as cap bytes exist (a PNG decoder needs no
   more: libpng's "too much image data" is a warning).  Returns 0, or a negative error. */
static int inflate_raw(ibits *s, uint8_t *out, size_t cap, size_t *produced) {
    size_t o = 0;
    int last;
    do {
        last = (int)need(s, 1);
        int type = (int)need(s, 2);
        if (s->err) return -1;
        if (type == 0) {
            s->bitbuf = 0; s->bitcnt = 0;
            if (s->pos + 4 > s->n) return -1;
            unsigned len = s->in[s->pos] | (s->in[s->pos + 1] << 8), nlen = s->in[s->pos + 2] | (s->in[s->pos + 3] << 8);
            s->pos += 4;
            if ((len ^ 0xFFFFu) != nlen) return -2;
            if (s->pos + len > s->n) return -1;
            size_t take = len; if (take > cap - o) take = cap - o;
            memcpy(out + o, s->in + s->pos, take);
            o += take; s->pos += len;
            if (o >= cap) break;
            continue;
        }
        if (type == 3) return -3;
        hcode lc, dc;
        uint8_t lens[320];
        if (type == 1) {
            int i = 0;
            for (; i < 144; i++) lens[i] = 8;
            for (; i < 256; i++) lens[i] = 9;
            for (; i < 280; i++) lens[i] = 7;
            for (; i < 288; i++) lens[i] = 8;
            hbuild(&lc, lens, 288);
            for (i = 0; i < 30; i++) lens[i] = 5;
            hbuild(&dc, lens, 30);
        } else {
            int nlen = (int)need(s, 5) + 257, ndist = (int)need(s, 5) + 1, ncode = (int)need(s, 4) + 4;
            if (s->err) return -1;
            if (nlen > 286 || ndist > 30) return -4;
            uint8_t cl[19]; memset(cl, 0, sizeof cl);
            for (int i = 0; i < ncode; i++) cl[CL_ORDER[i]] = (uint8_t)need(s, 3);
            if (s->err) return -1;
            hcode cc;
            if (hbuild(&cc, cl, 19) != 0) return -5;   /* zlib: the code-length code must be complete */
            int idx = 0;
            while (idx < nlen + ndist) {
                int sym = hdecode(s, &cc);
                if (sym < 0) return -6;
                if (sym < 16) lens[idx++] = (uint8_t)sym;
                else {
                    int rep, val = 0;
                    if (sym == 16) { if (idx == 0) return -7; val = lens[idx - 1]; rep = 3 + (int)need(s, 2); }
                    else if (sym == 17) rep = 3 + (int)need(s, 3);
                    else rep = 11 + (int)need(s, 7);
                    if (s->err) return -1;
                    if (idx + rep > nlen + ndist) return -8;
                    while (rep--) lens[idx++] = (uint8_t)val;
                }
            }
            if (lens[256] == 0) return -9;
            /* an incomplete code only as a single codeword of length 1 (zlib inflate_table's "max != 1", libdeflate) */
            int r = hbuild(&lc, lens, nlen);
            if (r < 0 || (r > 0 && (nlen - lc.count[0] != 1 || lc.count[1] != 1))) return -10;
            r = hbuild(&dc, lens + nlen, ndist);
            if (r < 0 || (r > 0 && (ndist - dc.count[0] != 1 || dc.count[1] != 1))) return -11;
        }
        for (;;) {
            int sym = hdecode(s, &lc);
            if (sym < 0) return -12;
            if (sym < 256) { if (o < cap) out[o] = (uint8_t)sym; o++; if (o >= cap) break; continue; }
            if (sym == 256) break;
            sym -= 257;
            if (sym >= 29) return -13;
            unsigned len = LEN_BASE[sym] + need(s, LEN_EXTRA[sym]);
            int ds = hdecode(s, &dc);
            if (ds < 0 || ds >= 30) return -14;
            unsigned dist = DIST_BASE[ds] + need(s, DIST_EXTRA[ds]);
            if (s->err) return -1;
            if (dist > o) return -15;
            while (len-- && o < cap) { out[o] = out[o - dist]; o++; }
            if (o >= cap) break;
        }
        if (o >= cap) break;
    } while (!last);
    *produced = o;
    return 0;
}
int cso_inflate_zlib(const uint8_t *in, size_t n, uint8_t *out, size_t cap, size_t *produced) {
    if (n < 2) return -20;
    unsigned cmf = in[0], flg = in[1];
    if ((cmf & 15) != 8 || (cmf >> 4) > 7 || ((cmf << 8) | flg) % 31 || (flg & 0x20)) return -21;
    ibits s; memset(&s, 0, sizeof s);
    s.in = in; s.n = n; s.pos = 2;
    *produced = 0;
    return inflate_raw(&s, out, cap, produced);
}

/* ------------------------------------------------------------------------------------------------ PNG parse + unfilter */
static const uint8_t PNG_SIG[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1A, '\n'};
static int kept_when_stripping(const uint8_t *type) {   /* oxipng StripChunks::Safe keeps these ancillary chunks [UPSTREAM-RECALL] */
    static const char *keep[] = {"cICP", "iCCP", "sRGB", "pHYs", "tRNS"};   /* tRNS is image data, never stripped */
    for (size_t i = 0; i < sizeof keep / sizeof *keep; i++) if (!memcmp(type, keep[i], 4)) return 1;
    return 0;
}
static int paeth(int a, int b, int c) {
    int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}
void cso_png_free(cso_png *p) {
    if (!p) return;
    free(p->pix); free(p->chunks); free(p);
}
int cso_png_decode(const uint8_t *in, size_t n, int keep_metadata, cso_png **out) {
    *out = NULL;
    if (n < 8 + 25 || memcmp(in, PNG_SIG, 8)) return CSO_PNG_BAD;
    cso_png *P = (cso_png *)calloc(1, sizeof *P);
    uint8_t *idat = (uint8_t *)malloc(n);
    size_t nidat = 0, pos = 8;
    int seen_ihdr = 0, seen_idat = 0, seen_iend = 0, rc = 0;
    P->chunks = (uint8_t *)malloc(n); P->chunks_len = 0; P->idat_at = (size_t)-1;
    while (pos + 12 <= n && !seen_iend) {
        uint32_t len = be32(in + pos);
        const uint8_t *type = in + pos + 4;
        if (len > 0x7FFFFFFFu || pos + 12 + (size_t)len > n) { rc = CSO_PNG_BAD; break; }
        const uint8_t *d = in + pos + 8;
        if (!seen_ihdr) {
            if (memcmp(type, "IHDR", 4) || len != 13) { rc = CSO_PNG_BAD; break; }
            if (cso_crc32(0, type, 4 + 13) != be32(d + 13)) { rc = CSO_PNG_BAD; break; }
            P->width = be32(d); P->height = be32(d + 4); P->depth = d[8]; P->ctype = d[9]; P->interlace = d[12];
            if (!P->width || !P->height || P->width > 0x7FFFFFFFu || P->height > 0x7FFFFFFFu || d[10] || d[11] || d[12] > 1) { rc = CSO_PNG_BAD; break; }
            static const int chans[7] = {1, 0, 3, 1, 2, 0, 4};
            int okd = 0;
            switch (P->ctype) {
            case 0: okd = P->depth == 1 || P->depth == 2 || P->depth == 4 || P->depth == 8 || P->depth == 16; break;
            case 3: okd = P->depth == 1 || P->depth == 2 || P->depth == 4 || P->depth == 8; break;
            case 2: case 4: case 6: okd = P->depth == 8 || P->depth == 16; break;
            }
            if (!okd) { rc = CSO_PNG_BAD; break; }
            P->channels = chans[P->ctype];
            int bits = P->channels * P->depth;
            P->bpp = bits >= 8 ? bits / 8 : 1;
            P->rowbytes = ((size_t)P->width * (size_t)bits + 7) / 8;
            seen_ihdr = 1;
        } else if (!memcmp(type, "IDAT", 4)) {
            if (P->idat_at == (size_t)-1) P->idat_at = P->chunks_len;
            memcpy(idat + nidat, d, len); nidat += len; seen_idat = 1;
        } else if (!memcmp(type, "IEND", 4)) {
            seen_iend = 1;
        } else {
            if (!memcmp(type, "acTL", 4)) { rc = CSO_PNG_UNSUPPORTED; break; }   /* animated PNG */
            if (!memcmp(type, "PLTE", 4)) { if (len % 3 || len > 768) { rc = CSO_PNG_BAD; break; } P->nplte = (int)(len / 3); }
            int critical = !(type[0] & 0x20);
            if (critical || keep_metadata || kept_when_stripping(type)) {
                if (!memcmp(type, "tRNS", 4) || !memcmp(type, "bKGD", 4) || !memcmp(type, "sBIT", 4)) P->no_reduce = 1;
                if (!memcmp(type, "bKGD", 4) || !memcmp(type, "sBIT", 4) || !memcmp(type, "hIST", 4)) P->pal_tied = 1;
                memcpy(P->chunks + P->chunks_len, in + pos, 12 + (size_t)len);
                P->chunks_len += 12 + (size_t)len;
            }
        }
        pos += 12 + (size_t)len;
    }
    if (!rc && (!seen_ihdr || !seen_idat || !seen_iend)) rc = CSO_PNG_BAD;
    if (!rc && P->ctype == 3 && !P->nplte) rc = CSO_PNG_BAD;
    if (rc) { free(idat); cso_png_free(P); return rc; }
    /* the passes of the stream: one for a plain image, up to seven reduced images for Adam7 (PNG spec section 8.2); every pass is
       filtered on its own; the output is never interlaced */
    static const int XS[7] = {0, 4, 0, 2, 0, 1, 0}, YS[7] = {0, 0, 4, 0, 2, 0, 1}, DX[7] = {8, 8, 4, 4, 2, 2, 1}, DY[7] = {8, 8, 8, 4, 4, 2, 2};
    const int bits = P->channels * P->depth, npass = P->interlace ? 7 : 1;
    size_t raw_len = 0;
    for (int p = 0; p < npass; p++) {
        const uint32_t pw = P->interlace ? (P->width + DX[p] - 1 - XS[p]) / DX[p] : P->width, ph = P->interlace ? (P->height + DY[p] - 1 - YS[p]) / DY[p] : P->height;
        if (pw && ph) raw_len += (size_t)ph * (1 + ((size_t)pw * bits + 7) / 8);
    }
    size_t got = 0;
    uint8_t *raw = (uint8_t *)malloc(raw_len);
    rc = cso_inflate_zlib(idat, nidat, raw, raw_len, &got);
    free(idat);
    if (rc || got < raw_len) { free(raw); cso_png_free(P); return CSO_PNG_BAD; }
    P->pix = (uint8_t *)calloc(P->rowbytes, P->height);
    const int bpp = P->bpp;
    const uint8_t *f = raw;
    for (int p = 0; p < npass && !rc; p++) {
        const uint32_t pw = P->interlace ? (P->width + DX[p] - 1 - XS[p]) / DX[p] : P->width, ph = P->interlace ? (P->height + DY[p] - 1 - YS[p]) / DY[p] : P->height;
        if (!pw || !ph) continue;
        const size_t prb = ((size_t)pw * bits + 7) / 8;
        uint8_t *tmp = P->interlace ? (uint8_t *)malloc(prb * ph) : P->pix;
        for (uint32_t y = 0; y < ph && !rc; y++, f += 1 + prb) {
            uint8_t *cur = tmp + y * prb;
            const uint8_t *up = y ? cur - prb : NULL;
            int ft = f[0];
            if (ft > 4) { rc = CSO_PNG_BAD; break; }
            for (size_t x = 0; x < prb; x++) {
                int a = x >= (size_t)bpp ? cur[x - bpp] : 0, b = up ? up[x] : 0, c = (up && x >= (size_t)bpp) ? up[x - bpp] : 0, v = f[1 + x];
                switch (ft) {
                case 1: v += a; break;
                case 2: v += b; break;
                case 3: v += (a + b) >> 1; break;
                case 4: v += paeth(a, b, c); break;
                }
                cur[x] = (uint8_t)v;
            }
        }
        if (P->interlace) {
            if (!rc)
                for (uint32_t y = 0; y < ph; y++)
                    for (uint32_t x = 0; x < pw; x++) {
                        const uint32_t oy = YS[p] + y * DY[p], ox = XS[p] + x * DX[p];
                        if (bits >= 8) memcpy(P->pix + (size_t)oy * P->rowbytes + (size_t)ox * (bits / 8), tmp + (size_t)y * prb + (size_t)x * (bits / 8), (size_t)bits / 8);
                        else {   /* sub-byte samples: most significant bits first */
                            const size_t sb = (size_t)x * bits, db = (size_t)ox * bits;
                            const int v = (tmp[(size_t)y * prb + sb / 8] >> (8 - bits - (sb & 7))) & ((1 << bits) - 1);
                            P->pix[(size_t)oy * P->rowbytes + db / 8] |= (uint8_t)(v << (8 - bits - (db & 7)));
                        }
                    }
            free(tmp);
        }
    }
    free(raw);
    if (rc) { cso_png_free(P); return rc; }
    *out = P;
    return 0;
}

/* ------------------------------------------------------------------------------------------------ P2: reductions
 * The subset of oxipng's reductions that needs no palette: 16 -> 8 bits when every sample's two bytes are equal; alpha
 * dropped when every pixel is opaque; colour -> grey when r == g == b everywhere.  Applied in that order, always (oxipng
 * evaluates both variants and keeps the smaller; for these three the reduced image practically always wins), and never
 * when a carried chunk is tied to the colour type (tRNS, bKGD, sBIT).  Then colour -> palette (to_palette) and 8-bit grey -> 4 / 2 / 1 bit
 * (grey_depth).  An 8-bit indexed image that does not use its whole palette loses the unused entries and the depth they cost (index_depth);
 * palettes are not re-ordered, duplicate entries not merged. */
/* colour -> palette: an 8-bit RGB / RGBA image with at most 256 distinct pixels becomes an indexed one (entries sorted by
   alpha, then red, green, blue, so that the translucent ones come first and tRNS stops at the last of them; index depth 1, 2, 4
   or 8 by their number) when the indexed rows plus the PLTE / tRNS chunks are smaller than the rows were.  Returns 8 or 0. */
static int cmp_u32(const void *a, const void *b) { uint32_t x = *(const uint32_t *)a, y = *(const uint32_t *)b; return x < y ? -1 : x > y; }
static int to_palette(cso_png *P) {
    if (P->depth != 8 || (P->ctype != 2 && P->ctype != 6) || P->nplte) return 0;
    const int ch = P->channels;
    uint32_t pal[257];
    int n = 0;
    for (uint32_t y = 0; y < P->height && n <= 256; y++) {
        const uint8_t *r = P->pix + (size_t)y * P->rowbytes;
        for (uint32_t x = 0; x < P->width && n <= 256; x++) {
            const uint8_t *px = r + (size_t)x * ch;
            const uint32_t key = ((uint32_t)(ch == 4 ? px[3] : 255) << 24) | ((uint32_t)px[0] << 16) | ((uint32_t)px[1] << 8) | px[2];
            int k = 0;
            while (k < n && pal[k] != key) k++;
            if (k == n) pal[n++] = key;
        }
    }
    if (n > 256) return 0;
    qsort(pal, (size_t)n, sizeof pal[0], cmp_u32);
    int ntr = 0;
    for (int k = 0; k < n; k++) if ((pal[k] >> 24) != 255) ntr = k + 1;
    const int d = n <= 2 ? 1 : n <= 4 ? 2 : n <= 16 ? 4 : 8;
    const size_t nrb = ((size_t)P->width * d + 7) / 8;
    const size_t extra = 12 + 3 * (size_t)n + (ntr ? 12 + (size_t)ntr : 0);
    if ((size_t)P->height * (1 + nrb) + extra >= (size_t)P->height * (1 + P->rowbytes)) return 0;
    uint8_t *np = (uint8_t *)calloc(nrb, P->height);
    for (uint32_t y = 0; y < P->height; y++)
        for (uint32_t x = 0; x < P->width; x++) {
            const uint8_t *px = P->pix + (size_t)y * P->rowbytes + (size_t)x * ch;
            const uint32_t key = ((uint32_t)(ch == 4 ? px[3] : 255) << 24) | ((uint32_t)px[0] << 16) | ((uint32_t)px[1] << 8) | px[2];
            int k = 0;
            while (pal[k] != key) k++;
            const size_t bit = (size_t)x * d;
            np[(size_t)y * nrb + bit / 8] |= (uint8_t)(k << (8 - d - (bit & 7)));
        }
    free(P->pix);
    P->pix = np; P->rowbytes = nrb; P->channels = 1; P->depth = d; P->bpp = 1; P->ctype = 3; P->nplte = n;
    /* PLTE and tRNS go in front of where the first IDAT stood */
    uint8_t *ins = (uint8_t *)malloc(extra), *w = ins;
    put_be32(w, (uint32_t)(3 * n)); memcpy(w + 4, "PLTE", 4);
    for (int k = 0; k < n; k++) { w[8 + 3 * k] = (uint8_t)(pal[k] >> 16); w[9 + 3 * k] = (uint8_t)(pal[k] >> 8); w[10 + 3 * k] = (uint8_t)pal[k]; }
    put_be32(w + 8 + 3 * n, cso_crc32(0, w + 4, 4 + 3 * (size_t)n)); w += 12 + 3 * n;
    if (ntr) {
        put_be32(w, (uint32_t)ntr); memcpy(w + 4, "tRNS", 4);
        for (int k = 0; k < ntr; k++) w[8 + k] = (uint8_t)(pal[k] >> 24);
        put_be32(w + 8 + ntr, cso_crc32(0, w + 4, 4 + (size_t)ntr)); w += 12 + ntr;
    }
    uint8_t *nc = (uint8_t *)malloc(P->chunks_len + extra);
    memcpy(nc, P->chunks, P->idat_at); memcpy(nc + P->idat_at, ins, extra); memcpy(nc + P->idat_at + extra, P->chunks + P->idat_at, P->chunks_len - P->idat_at);
    free(P->chunks); free(ins);
    P->chunks = nc; P->chunks_len += extra; P->idat_at += extra;
    return 8;
}
/* 8-bit grey -> 4, 2 or 1 bit when every sample is a multiple of 17, 85 or 255 (the values those depths can express).  Returns 32 or 0. */
static int grey_depth(cso_png *P) {
    if (P->ctype != 0 || P->depth != 8) return 0;
    int ok4 = 1, ok2 = 1, ok1 = 1;
    for (uint32_t y = 0; y < P->height; y++)
        for (uint32_t x = 0; x < P->width; x++) {
            const int v = P->pix[(size_t)y * P->rowbytes + x];
            if (v % 17) ok4 = 0;
            if (v % 85) ok2 = 0;
            if (v % 255) ok1 = 0;
        }
    const int d = ok1 ? 1 : ok2 ? 2 : ok4 ? 4 : 0;
    if (!d) return 0;
    const size_t nrb = ((size_t)P->width * d + 7) / 8;
    uint8_t *np = (uint8_t *)calloc(nrb, P->height);
    const int div = 255 / ((1 << d) - 1);
    for (uint32_t y = 0; y < P->height; y++)
        for (uint32_t x = 0; x < P->width; x++) {
            const size_t bit = (size_t)x * d;
            np[(size_t)y * nrb + bit / 8] |= (uint8_t)((P->pix[(size_t)y * P->rowbytes + x] / div) << (8 - d - (bit & 7)));
        }
    free(P->pix);
    P->pix = np; P->rowbytes = nrb; P->depth = d; P->bpp = 1;
    return 32;
}
/* an 8-bit indexed image that does not use its whole palette, or lists a colour twice: the entries no pixel points at are dropped, duplicates (same red,
   green, blue and alpha) merged into their first, the entries that are not opaque moved in front of the opaque ones (round 4; oxipng's reduced_palette /
   alpha-first ordering in spirit, not its luma sort), the indices renumbered and packed at the smallest depth that holds the entries left (1, 2, 4 or 8 bits), PLTE and tRNS written again for them (a tRNS that ends up
   all opaque goes).  Not when a carried chunk counts on the palette as it is (bKGD, sBIT, hIST), nor when a pixel points past the palette.
   Returns 64 or 0. */
static int index_depth(cso_png *P) {
    if (P->ctype != 3 || P->depth != 8 || P->pal_tied) return 0;
    int used[256], map[256], n = 0;
    memset(used, 0, sizeof used);
    for (uint32_t y = 0; y < P->height; y++)
        for (uint32_t x = 0; x < P->width; x++) used[P->pix[(size_t)y * P->rowbytes + x]] = 1;
    for (int i = 0; i < 256; i++) if (used[i] && i >= P->nplte) return 0;
    /* the entries that stay: one per distinct colour (red, green, blue, alpha) among the used ones -- a later duplicate points at the first --, those that are
       not opaque in front of the opaque ones (each group in the old order), so that tRNS stops at the last of them */
    const uint8_t *plte0 = NULL, *trns0 = NULL;
    uint32_t ntrns0 = 0;
    for (size_t pos = 0; pos + 12 <= P->chunks_len; pos += 12 + (size_t)be32(P->chunks + pos)) {
        if (!memcmp(P->chunks + pos + 4, "PLTE", 4)) plte0 = P->chunks + pos + 8;
        if (!memcmp(P->chunks + pos + 4, "tRNS", 4)) { trns0 = P->chunks + pos + 8; ntrns0 = be32(P->chunks + pos); }
    }
    if (!plte0) return 0;
    int first_of[256], order[256], nuniq = 0;
    uint32_t col[256];
    for (int i = 0; i < 256; i++) {
        first_of[i] = -1;
        if (!used[i]) continue;
        col[i] = ((uint32_t)((trns0 && (uint32_t)i < ntrns0) ? trns0[i] : 255) << 24) | ((uint32_t)plte0[3 * i] << 16) | ((uint32_t)plte0[3 * i + 1] << 8) | plte0[3 * i + 2];
        first_of[i] = i;
        for (int k = 0; k < i; k++) if (used[k] && first_of[k] == k && col[k] == col[i]) { first_of[i] = k; break; }
        if (first_of[i] == i) nuniq++;
    }
    for (int pass = 0; pass < 2; pass++)
        for (int i = 0; i < 256; i++)
            if (used[i] && first_of[i] == i && ((col[i] >> 24) != 255) == (pass == 0)) { map[i] = n; order[n++] = i; }
    for (int i = 0; i < 256; i++) if (used[i] && first_of[i] != i) map[i] = map[first_of[i]];
    (void)nuniq;
    const int d = n <= 2 ? 1 : n <= 4 ? 2 : n <= 16 ? 4 : 8;
    if (d == 8 && n == P->nplte) return 0;
    const size_t nrb = ((size_t)P->width * d + 7) / 8;
    uint8_t *np = (uint8_t *)calloc(nrb, P->height);
    for (uint32_t y = 0; y < P->height; y++)
        for (uint32_t x = 0; x < P->width; x++) {
            const size_t bit = (size_t)x * d;
            np[(size_t)y * nrb + bit / 8] |= (uint8_t)(map[P->pix[(size_t)y * P->rowbytes + x]] << (8 - d - (bit & 7)));
        }
    free(P->pix);
    P->pix = np; P->rowbytes = nrb; P->depth = d; P->bpp = 1;
    /* the carried chunks again: PLTE and tRNS of the entries that are left */
    const uint8_t *plte = NULL, *trns = NULL;
    uint32_t ntrns = 0;
    for (size_t pos = 0; pos + 12 <= P->chunks_len; pos += 12 + (size_t)be32(P->chunks + pos)) {
        if (!memcmp(P->chunks + pos + 4, "PLTE", 4)) plte = P->chunks + pos + 8;
        if (!memcmp(P->chunks + pos + 4, "tRNS", 4)) { trns = P->chunks + pos + 8; ntrns = be32(P->chunks + pos); }
    }
    uint8_t npl[768], ntr[256];
    int nt = 0;
    for (int k = 0; k < n; k++) {
        const int i = order[k];
        memcpy(npl + 3 * k, plte + 3 * i, 3);
        ntr[k] = (trns && (uint32_t)i < ntrns) ? trns[i] : 255;
        if (ntr[k] != 255) nt = k + 1;
    }
    uint8_t *nc = (uint8_t *)malloc(P->chunks_len + 16), *w = nc;
    size_t new_idat_at = P->idat_at;
    for (size_t pos = 0; pos + 12 <= P->chunks_len;) {
        const uint32_t len = be32(P->chunks + pos);
        const uint8_t *type = P->chunks + pos + 4;
        const uint8_t *data = P->chunks + pos + 8;
        uint32_t nlen = len;
        int drop = 0;
        if (!memcmp(type, "PLTE", 4)) { nlen = (uint32_t)(3 * n); data = npl; }
        else if (!memcmp(type, "tRNS", 4)) { nlen = (uint32_t)nt; data = ntr; drop = nt == 0; }
        if (!drop) {
            put_be32(w, nlen); memcpy(w + 4, type, 4); memcpy(w + 8, data, nlen);
            put_be32(w + 8 + nlen, cso_crc32(0, w + 4, 4 + (size_t)nlen));
            w += 12 + nlen;
        }
        if (pos < P->idat_at) new_idat_at -= (12 + (size_t)len) - (drop ? 0 : 12 + (size_t)nlen);
        pos += 12 + (size_t)len;
    }
    free(P->chunks);
    P->chunks = nc; P->chunks_len = (size_t)(w - nc); P->idat_at = new_idat_at; P->nplte = n;
    return 64;
}
int cso_png_reduce(cso_png *P) {
    if (P->ctype == 3) return index_depth(P);
    if (P->no_reduce || P->ctype == 3 || P->depth < 8) return 0;
    const int bps = P->depth / 8, ch = P->channels;
    const size_t npx = (size_t)P->width * P->height;
    int narrow = bps == 2, opaque = (ch == 2 || ch == 4), grey = ch >= 3;
    for (uint32_t y = 0; y < P->height; y++) {
        const uint8_t *r = P->pix + (size_t)y * P->rowbytes;
        for (uint32_t x = 0; x < P->width; x++) {
            const uint8_t *px = r + (size_t)x * ch * bps;
            if (narrow) for (int k = 0; k < ch; k++) if (px[2 * k] != px[2 * k + 1]) narrow = 0;
            if (opaque) for (int b = 0; b < bps; b++) if (px[(ch - 1) * bps + b] != 0xFF) opaque = 0;
            if (grey) for (int b = 0; b < bps; b++) if (px[b] != px[bps + b] || px[b] != px[2 * bps + b]) grey = 0;
        }
    }
    (void)npx;
    if (!narrow && !opaque && !grey) return to_palette(P) | grey_depth(P);
    const int nbps = narrow ? 1 : bps;
    int keep[4], nk = 0;   /* source channels that survive */
    for (int k = 0; k < ch; k++) {
        if (opaque && k == ch - 1) continue;
        if (grey && (k == 1 || k == 2)) continue;
        keep[nk++] = k;
    }
    const size_t nrow = (size_t)P->width * nk * nbps;
    uint8_t *np = (uint8_t *)malloc(nrow * P->height);
    for (uint32_t y = 0; y < P->height; y++)
        for (uint32_t x = 0; x < P->width; x++)
            for (int k = 0; k < nk; k++)
                for (int b = 0; b < nbps; b++)
                    np[(size_t)y * nrow + ((size_t)x * nk + k) * nbps + b] = P->pix[(size_t)y * P->rowbytes + ((size_t)x * ch + keep[k]) * bps + b];
    free(P->pix);
    P->pix = np; P->rowbytes = nrow; P->channels = nk; P->depth = nbps * 8; P->bpp = nk * nbps;
    P->ctype = nk == 1 ? 0 : nk == 2 ? 4 : nk == 3 ? 2 : 6;
    return (narrow ? 1 : 0) | (opaque ? 2 : 0) | (grey ? 4 : 0) | to_palette(P) | grey_depth(P);
}

/* ------------------------------------------------------------------------------------------------ lossy PNG: colour quantisation
 * `-q` on a PNG (png.optimize = false): libcaesium quantises with imagequant 4.4.1 (dithering 1.0) and writes a palette PNG with
 * lodepng (Cargo.lock:735, :972).  Neither is available and their output cannot be pinned; this is a plain, deterministic,
 * integer MEDIAN CUT laid out for the GPU, without dithering -- coarser than imagequant on gradients, stated as such:
 *   1. pixels -> (a, r, g, b) of 8 bits (high bytes of 16-bit samples); bins of 4 + 5 + 5 + 5 bits hold count and channel sums;
 *   2. boxes over the non-empty bins (ascending bin id): the most populous splittable box is cut along the channel with the
 *      largest spread of bin means (ties: r, g, b, a) at the weighted median, until 256 boxes -- or, from two boxes on, until the
 *      palette is good enough for the quality asked for (png_quality_table.h);
 *   3. palette = rounded mean of each box, sorted by (a, r, g, b), duplicates merged; every pixel takes the nearest entry
 *      (squared distance over the four channels; ties: the lower index).
 * Applied to truecolour images that still have more than 256 colours after the lossless reductions; everything else (grey,
 * indexed, few colours) goes through unchanged, which is already exact. */
typedef struct { uint32_t id, cnt, s[4]; } qbin;   /* s: sums of r, g, b, a */
typedef struct { int lo, hi; uint64_t cnt; } qbox;  /* bins ord[lo, hi) */
static const qbin *g_bins; static int g_axis;
static int bin_mean(const qbin *b, int c) { return (int)(b->s[c] / b->cnt); }
static int cmp_axis(const void *x, const void *y) {
    const qbin *a = g_bins + *(const int *)x, *b = g_bins + *(const int *)y;
    int ma = bin_mean(a, g_axis), mb = bin_mean(b, g_axis);
    if (ma != mb) return ma < mb ? -1 : 1;
    return a->id < b->id ? -1 : a->id > b->id;
}
static int box_axis(const qbin *bins, const int *ord, const qbox *bx, int *range) {
    int best = 0, br = -1;
    for (int c = 0; c < 4; c++) {
        int mn = 255, mx = 0;
        for (int i = bx->lo; i < bx->hi; i++) { int m = bin_mean(bins + ord[i], c); if (m < mn) mn = m; if (m > mx) mx = m; }
        if (mx - mn > br) { br = mx - mn; best = c; }
    }
    *range = br;
    return best;
}
/* error of the palette entry box k would give: every bin mean against the rounded box mean */
static uint64_t box_error(const qbin *bins, const int *ord, const qbox *bx) {
    uint64_t sum[4] = {0, 0, 0, 0}, cnt = 0, err = 0;
    for (int i = bx->lo; i < bx->hi; i++) { const qbin *b = bins + ord[i]; cnt += b->cnt; for (int c = 0; c < 4; c++) sum[c] += b->s[c]; }
    for (int i = bx->lo; i < bx->hi; i++) {
        const qbin *b = bins + ord[i];
        uint64_t d2 = 0;
        for (int c = 0; c < 4; c++) { const int64_t d = (int64_t)bin_mean(b, c) - (int64_t)((2 * sum[c] + cnt) / (2 * cnt)); d2 += (uint64_t)(d * d); }
        err += d2 * b->cnt;
    }
    return err;
}
static int median_cut(const qbin *bins, int nbins, int quality, uint32_t *pal) {
    int *ord = (int *)malloc(sizeof(int) * (size_t)nbins);
    for (int i = 0; i < nbins; i++) ord[i] = i;
    qbox box[256];
    int nbox = 1;
    box[0].lo = 0; box[0].hi = nbins; box[0].cnt = 0;
    for (int i = 0; i < nbins; i++) box[0].cnt += bins[i].cnt;
    uint8_t dead[256]; memset(dead, 0, sizeof dead);
    const uint64_t pixels = box[0].cnt;
    uint64_t berr[256], total_err;
    berr[0] = total_err = box_error(bins, ord, &box[0]);
    quality = quality < 0 ? 0 : quality > 100 ? 100 : quality;
    while (nbox < 256) {
        if (nbox >= 2 && (quality == 0 || total_err * 1024 <= kQualityBound[quality] * pixels)) break;   /* good enough for this -q */
        int pick = -1;
        for (int k = 0; k < nbox; k++) if (!dead[k] && box[k].hi - box[k].lo > 1 && (pick < 0 || box[k].cnt > box[pick].cnt)) pick = k;
        if (pick < 0) break;
        int range, axis = box_axis(bins, ord, &box[pick], &range);
        if (range == 0) { dead[pick] = 1; continue; }
        g_bins = bins; g_axis = axis;
        qsort(ord + box[pick].lo, (size_t)(box[pick].hi - box[pick].lo), sizeof(int), cmp_axis);
        uint64_t cum = 0;
        int s = box[pick].lo;
        while (s < box[pick].hi - 1) { cum += bins[ord[s]].cnt; s++; if (2 * cum >= box[pick].cnt) break; }
        box[nbox].lo = s; box[nbox].hi = box[pick].hi; box[nbox].cnt = box[pick].cnt - cum;
        box[pick].hi = s; box[pick].cnt = cum;
        total_err -= berr[pick];
        berr[pick] = box_error(bins, ord, &box[pick]); berr[nbox] = box_error(bins, ord, &box[nbox]);
        total_err += berr[pick] + berr[nbox];
        nbox++;
    }
    int n = 0;
    for (int k = 0; k < nbox; k++) {
        uint64_t sum[4] = {0, 0, 0, 0}, cnt = 0;
        for (int i = box[k].lo; i < box[k].hi; i++) { const qbin *b = bins + ord[i]; cnt += b->cnt; for (int c = 0; c < 4; c++) sum[c] += b->s[c]; }
        uint32_t v[4];
        for (int c = 0; c < 4; c++) v[c] = (uint32_t)((2 * sum[c] + cnt) / (2 * cnt));
        pal[n++] = (v[3] << 24) | (v[0] << 16) | (v[1] << 8) | v[2];
    }
    free(ord);
    qsort(pal, (size_t)n, sizeof pal[0], cmp_u32);
    int m = 0;
    for (int k = 0; k < n; k++) if (!m || pal[k] != pal[m - 1]) pal[m++] = pal[k];
    return m;
}
/* truecolour (8 or 16 bit) with more than 256 colours -> an 8-bit indexed image; returns 16 when applied */
static int quantize(cso_png *P, int quality) {
    if (P->no_reduce || (P->ctype != 2 && P->ctype != 6) || P->nplte) return 0;
    const int ch = P->channels, bps = P->depth / 8;
    const size_t npx = (size_t)P->width * P->height;
    {   /* at most 256 distinct pixels (high bytes): nothing to quantise, the image stays as the lossless reductions left it */
        uint32_t seen[257];
        int ns = 0;
        for (uint32_t y = 0; y < P->height && ns <= 256; y++)
            for (uint32_t x = 0; x < P->width && ns <= 256; x++) {
                const uint8_t *px = P->pix + (size_t)y * P->rowbytes + (size_t)x * ch * bps;
                const uint32_t key = ((uint32_t)(ch == 4 ? px[3 * bps] : 255) << 24) | ((uint32_t)px[0] << 16) | ((uint32_t)px[bps] << 8) | px[2 * bps];
                int k = 0;
                while (k < ns && seen[k] != key) k++;
                if (k == ns) seen[ns++] = key;
            }
        if (ns <= 256) return 0;
    }
    qbin *all = (qbin *)calloc(1u << 19, sizeof(qbin));
    for (uint32_t y = 0; y < P->height; y++)
        for (uint32_t x = 0; x < P->width; x++) {
            const uint8_t *px = P->pix + (size_t)y * P->rowbytes + (size_t)x * ch * bps;
            const uint32_t r = px[0], g = px[bps], b = px[2 * bps], a = ch == 4 ? px[3 * bps] : 255u;
            qbin *q = all + (((a >> 4) << 15) | ((r >> 3) << 10) | ((g >> 3) << 5) | (b >> 3));
            q->cnt++; q->s[0] += r; q->s[1] += g; q->s[2] += b; q->s[3] += a;
        }
    int nbins = 0;
    for (uint32_t i = 0; i < (1u << 19); i++) if (all[i].cnt) { all[nbins] = all[i]; all[nbins].id = i; nbins++; }
    uint32_t pal[256];
    const int n = median_cut(all, nbins, quality, pal);
    free(all);
    (void)npx;
    int ntr = 0;
    for (int k = 0; k < n; k++) if ((pal[k] >> 24) != 255) ntr = k + 1;
    const int d = n <= 2 ? 1 : n <= 4 ? 2 : n <= 16 ? 4 : 8;
    const size_t nrb = ((size_t)P->width * d + 7) / 8;
    uint8_t *np = (uint8_t *)calloc(nrb, P->height);
    /* every pixel its palette entry, with Floyd-Steinberg error diffusion (libcaesium runs imagequant at dithering level 1.0; this is the plain
       integer form, every row left to right -- so that on the GPU a row can follow the one above it two pixels behind --, not imagequant's): the pixel plus
       the error that reached it (sixteenths: 7 from the left, 3 / 5 / 1 from the row above's x+1 / x / x-1), clamped to 0..255 per channel, goes to
       its nearest entry (squared distance over a, r, g, b; ties: the lower index); what is left goes on */
    int (*below)[4] = (int (*)[4])calloc((size_t)P->width + 2, sizeof(int[4])), (*next)[4] = (int (*)[4])calloc((size_t)P->width + 2, sizeof(int[4]));   /* index x + 1 */
    for (uint32_t y = 0; y < P->height; y++) {
        int left[4] = {0, 0, 0, 0};
        memset(next, 0, ((size_t)P->width + 2) * sizeof(int[4]));
        for (uint32_t x = 0; x < P->width; x++) {
            const uint8_t *px = P->pix + (size_t)y * P->rowbytes + (size_t)x * ch * bps;
            const int src[4] = {px[0], px[bps], px[2 * bps], ch == 4 ? px[3 * bps] : 255};   /* r g b a */
            int want[4];
            for (int c = 0; c < 4; c++) { int v = src[c] + ((7 * left[c] + below[x + 1][c] + 8) >> 4); want[c] = v < 0 ? 0 : v > 255 ? 255 : v; }
            int best = 0; uint32_t bd = ~0u;
            for (int k = 0; k < n; k++) {
                const int dr = want[0] - (int)((pal[k] >> 16) & 255), dg = want[1] - (int)((pal[k] >> 8) & 255), db = want[2] - (int)(pal[k] & 255), da = want[3] - (int)(pal[k] >> 24);
                const uint32_t dist = (uint32_t)(dr * dr + dg * dg + db * db + da * da);
                if (dist < bd) { bd = dist; best = k; }
            }
            const int got[4] = {(int)((pal[best] >> 16) & 255), (int)((pal[best] >> 8) & 255), (int)(pal[best] & 255), (int)(pal[best] >> 24)};
            for (int c = 0; c < 4; c++) {
                const int e = want[c] - got[c];
                left[c] = e;
                next[x][c] += 3 * e; next[x + 1][c] += 5 * e; next[x + 2][c] += e;   /* (x - 1, x, x + 1 of the row below) */
            }
            const size_t bit = (size_t)x * d;
            np[(size_t)y * nrb + bit / 8] |= (uint8_t)(best << (8 - d - (bit & 7)));
        }
        int (*t)[4] = below; below = next; next = t;
    }
    free(below); free(next);
    free(P->pix);
    P->pix = np; P->rowbytes = nrb; P->channels = 1; P->depth = d; P->bpp = 1; P->ctype = 3; P->nplte = n;
    const size_t extra = 12 + 3 * (size_t)n + (ntr ? 12 + (size_t)ntr : 0);
    uint8_t *ins = (uint8_t *)malloc(extra), *w = ins;
    put_be32(w, (uint32_t)(3 * n)); memcpy(w + 4, "PLTE", 4);
    for (int k = 0; k < n; k++) { w[8 + 3 * k] = (uint8_t)(pal[k] >> 16); w[9 + 3 * k] = (uint8_t)(pal[k] >> 8); w[10 + 3 * k] = (uint8_t)pal[k]; }
    put_be32(w + 8 + 3 * n, cso_crc32(0, w + 4, 4 + 3 * (size_t)n)); w += 12 + 3 * n;
    if (ntr) {
        put_be32(w, (uint32_t)ntr); memcpy(w + 4, "tRNS", 4);
        for (int k = 0; k < ntr; k++) w[8 + k] = (uint8_t)(pal[k] >> 24);
        put_be32(w + 8 + ntr, cso_crc32(0, w + 4, 4 + (size_t)ntr)); w += 12 + ntr;
    }
    uint8_t *nc = (uint8_t *)malloc(P->chunks_len + extra);
    memcpy(nc, P->chunks, P->idat_at); memcpy(nc + P->idat_at, ins, extra); memcpy(nc + P->idat_at + extra, P->chunks + P->idat_at, P->chunks_len - P->idat_at);
    free(P->chunks); free(ins);
    P->chunks = nc; P->chunks_len += extra; P->idat_at += extra;
    return 16;
}
int cso_png_quantize(cso_png *P, int quality) { return quantize(P, quality); }

/* ------------------------------------------------------------------------------------------------ row filters */
static void filter_row(int ft, const uint8_t *cur, const uint8_t *up, size_t n, int bpp, uint8_t *dst) {
    dst[0] = (uint8_t)ft;
    for (size_t x = 0; x < n; x++) {
        int a = x >= (size_t)bpp ? cur[x - bpp] : 0, b = up ? up[x] : 0, c = (up && x >= (size_t)bpp) ? up[x - bpp] : 0, v = cur[x];
        switch (ft) {
        case 1: v -= a; break;
        case 2: v -= b; break;
        case 3: v -= (a + b) >> 1; break;
        case 4: v -= paeth(a, b, c); break;
        }
        dst[1 + x] = (uint8_t)v;
    }
}
/* i * log2(i) in integers: LodePNG's ilog2i (floor(log2) plus a linear fraction) */
static uint64_t ilog2i(uint64_t i) {
    if (!i) return 0;
    int l = 63 - __builtin_clzll(i);
    return i * (uint64_t)l + ((i - (1ull << l)) << 1);
}
static uint64_t fixed_cost_row(const uint8_t *row, size_t n, int bpp);
/* scores of one candidate row (type byte + n filtered bytes):
     [0] MinSum: sum of |signed byte| over the data bytes            (least wins)
     [1] Entropy: sum ilog2i(count) over the byte histogram, type byte included   (most wins)
     [2] Bigrams: number of distinct byte pairs, type byte included  (least wins)
     [3] BigEnt: sum ilog2i(count) over the pair histogram           (most wins)
     [4] Brute: estimated bits of the row under this project's tokenizer and a code of its own (least wins).  oxipng's
         Brute deflates the candidate together with the previously chosen rows at a fast libdeflate level, which makes the
         rows depend on each other; this statement scores every row on its own so that all rows are independent. */
static void filter_scores(const uint8_t *row, size_t n, int bpp, uint64_t sc[5]) {
    uint64_t ms = 0;
    uint32_t cnt[256]; memset(cnt, 0, sizeof cnt);
    for (size_t i = 1; i <= n; i++) { uint8_t b = row[i]; ms += b < 128 ? b : 256 - b; }
    for (size_t i = 0; i <= n; i++) cnt[row[i]]++;
    uint64_t ent = 0;
    for (int i = 0; i < 256; i++) ent += ilog2i(cnt[i]);
    static uint32_t pc[65536];
    uint64_t distinct = 0, bent = 0;
    for (size_t i = 0; i < n; i++) { uint32_t k = ((uint32_t)row[i] << 8) | row[i + 1]; if (!pc[k]++) distinct++; }
    for (size_t i = 0; i < n; i++) { uint32_t k = ((uint32_t)row[i] << 8) | row[i + 1]; if (pc[k]) { bent += ilog2i(pc[k]); pc[k] = 0; } }
    sc[0] = ms; sc[1] = ent; sc[2] = distinct; sc[3] = bent;
    sc[4] = fixed_cost_row(row, n + 1, bpp);
}
/* scores of every (row, filter): out[height][5][5] */
int cso_png_scores(const cso_png *P, uint64_t *out) {
    const size_t n = P->rowbytes, stride = 1 + n;
    uint8_t *cand = (uint8_t *)malloc(stride);
    for (uint32_t y = 0; y < P->height; y++) {
        const uint8_t *cur = P->pix + (size_t)y * n, *up = y ? cur - n : NULL;
        for (int f = 0; f < 5; f++) { filter_row(f, cur, up, n, P->bpp, cand); filter_scores(cand, n, P->bpp, out + ((size_t)y * 5 + f) * 5); }
    }
    free(cand);
    return 0;
}
/* strategy 0..4: that filter on every row; 5..9: per row, the candidate with the best score (ties: the lower filter) */
int cso_png_filter(const cso_png *P, int strategy, uint8_t *out, uint8_t *choice) {
    if (strategy < 0 || strategy > 9) return -1;
    const size_t n = P->rowbytes, stride = 1 + n;
    uint8_t *cand = (uint8_t *)malloc(stride * 5);
    for (uint32_t y = 0; y < P->height; y++) {
        const uint8_t *cur = P->pix + (size_t)y * n, *up = y ? cur - n : NULL;
        int pick = strategy;
        if (strategy >= 5) {
            uint64_t best = 0;
            pick = 0;
            for (int f = 0; f < 5; f++) {
                uint64_t sc[5];
                filter_row(f, cur, up, n, P->bpp, cand + f * stride);
                filter_scores(cand + f * stride, n, P->bpp, sc);
                uint64_t v = sc[strategy - 5];
                int more_wins = strategy == 6 || strategy == 8;
                if (f == 0 || (more_wins ? v > best : v < best)) { best = v; pick = f; }
            }
            memcpy(out + (size_t)y * stride, cand + pick * stride, stride);
        } else
            filter_row(pick, cur, up, n, P->bpp, out + (size_t)y * stride);
        if (choice) choice[y] = (uint8_t)pick;
    }
    free(cand);
    return 0;
}

/* ------------------------------------------------------------------------------------------------ deflate (this project's coder)
 * The stream is cut into CHUNKs of 32 KiB of input; every chunk becomes one dynamic-Huffman block followed -- except
 * after the last one -- by an empty stored block, which byte-aligns it (the "sync flush" pigz uses for the same
 * purpose), so chunks are coded independently and concatenated as bytes.
 * Tokenizer, per TILE of 64 consecutive positions (one GPU wave takes a tile per step):
 *   candidates of position p:  (a) up to four earlier positions q < tile start whose 4 bytes hash like p's: a table of
 *   2048 buckets x 4 entries, seeded with the 32 KiB in front of the chunk and refreshed after each tile (per hash, the
 *   tile's last position is pushed in);  (b) the fixed distances 1,2,3,4,6,8 (pixel strides of filtered PNG data), of
 *   which the one with the longest match inside the first 8 bytes (ties: the smaller distance) is extended if all 8
 *   agree.  The longest wins (ties: (b), then the nearer); length 3 is only taken at distance <= 8.  Matches end at the
 *   chunk end; their sources may lie in front of the chunk (the deflate window spans blocks).
 *   parse: greedy with one step of lazy evaluation inside a tile (a match at p yields to a longer one at p+1 unless p is
 *   the last position of its tile).
 * Code lengths: Huffman by repeated merge of the two least frequent (ties: the larger index first), limited to 15 (7 for
 * the code-length code) by the bit-count adjustment of T.81 K.2 / libjpeg; at least two symbols are coded in every
 * alphabet (zlib's rule, which keeps every code complete).
 */
#define CHUNK 32768u
#define HASH_BITS 9   /* the greedy table: 512 buckets (what it has to tell apart is chunks with matches from chunks without; the parse has its own tables) */
#define WAYS 4
static int len_code(int len) { int c = 28; while (LEN_BASE[c] > len) c--; return c; }
static int dist_code(int d) { int c = 29; while (DIST_BASE[c] > d) c--; return c; }
static size_t lcp(const uint8_t *a, const uint8_t *b, size_t max) { size_t l = 0; while (l < max && a[l] == b[l]) l++; return l; }
static const int FIXED_DIST[6] = {1, 2, 3, 4, 6, 8};
static uint32_t hash4(const uint8_t *d, int bits) {
    uint32_t v = d[0] | ((uint32_t)d[1] << 8) | ((uint32_t)d[2] << 16) | ((uint32_t)d[3] << 24);
    return (v * 0x9E3779B1u) >> (32 - bits);
}
/* after a tile: of the tile's positions with one hash only the LAST enters the bucket, pushing the older entries back */
static void insert_tile(uint16_t (*table)[WAYS], int bits, const uint8_t *data, size_t total, size_t base_rel, size_t t0, size_t t1) {
    /* positions are stored as 16-bit offsets from (chunk start - 32768): rel = p + base_rel */
    size_t lastpos[1 << 11];   /* only the slots of this tile's hashes are read (bits <= 11) */
    for (size_t p = t0; p < t1 && p + 4 <= total; p++) lastpos[hash4(data + p, bits)] = p;
    for (size_t p = t0; p < t1 && p + 4 <= total; p++) {
        uint32_t h = hash4(data + p, bits);
        size_t rel = p + base_rel;
        if (lastpos[h] != p || rel == 0xFFFF) continue;
        for (int w = WAYS - 1; w > 0; w--) table[h][w] = table[h][w - 1];
        table[h][0] = (uint16_t)rel;
    }
}

/* What a literal costs in this chunk, in 1/16 bit: log2(total / count) in integer arithmetic (exponent + the top four bits of the
   mantissa, i.e. a piecewise-linear log2), at least one bit, at most fifteen.  A short match is taken only if the literals it replaces
   cost more than it does: on filtered photographic data a byte costs 5-6 bits, and a three-byte match at a row's distance (a length
   code, a distance code and 11 extra bits) is a loss -- zlib and a greedy parse take it anyway, an optimal parser (libdeflate, zopfli)
   does not. */
static void literal_costs(const uint8_t *data, size_t start, size_t end, uint16_t cost16[256]) {
    uint32_t cnt[256];
    memset(cnt, 0, sizeof cnt);
    for (size_t p = start; p < end; p++) cnt[data[p]]++;
    const uint64_t total = end - start;
    for (int b = 0; b < 256; b++) {
        uint32_t c = 240;
        if (cnt[b]) {
            const uint64_t q = (total << 8) / cnt[b];   /* >= 256 */
            int e = 63; while (!((q >> e) & 1)) e--;
            c = 16u * (uint32_t)(e - 8) + (uint32_t)(((q << 4) >> e) & 15u);
            if (c < 16) c = 16; if (c > 240) c = 240;
        }
        cost16[b] = (uint16_t)c;
    }
}
#define MATCH_BASE16 320   /* what the two symbols of a match cost before their extra bits, in 1/16 bit (tuned on the synthetic set) */
#define MATCH_RULE_MAXLEN 8   /* longer matches always pay */
typedef struct { uint16_t len, dist; } token;   /* len 0: literal */
/* tokens of data[start, end) (one chunk of a stream of `total` bytes; tiles are aligned to multiples of 64 of the stream).
   tok[i] describes position start+i; taken[i] = the parse visits it. */
static void tokenize(const uint8_t *data, size_t total, size_t start, size_t end, token *tok, uint8_t *taken) {
    uint16_t table[1 << HASH_BITS][WAYS];
    memset(table, 0xFF, sizeof table);
    const size_t seed0 = start > 32768 ? start - 32768 : 0;
    const size_t base_rel = 32768 - start;   /* modulo 2^64: rel = p - start + 32768 */
    for (size_t t0 = seed0; t0 < start; t0 += 64) insert_tile(table, HASH_BITS, data, total, base_rel, t0, t0 + 64);
    size_t carry = start;   /* next position the parse visits */
    uint16_t cost16[256];
    literal_costs(data, start, end, cost16);
    for (size_t t0 = start; t0 < end; t0 += 64) {
        size_t t1 = t0 + 64 < end ? t0 + 64 : end;
        for (size_t p = t0; p < t1; p++) {
            size_t maxlen = end - p < 258 ? end - p : 258;
            size_t bl = 0, bd = 0;
            size_t l8best = 0, dbest = 0;
            for (int k = 0; k < 6; k++) {
                size_t d = (size_t)FIXED_DIST[k];
                if (d > p) continue;
                size_t l8 = lcp(data + p, data + p - d, maxlen < 8 ? maxlen : 8);
                if (l8 > l8best) { l8best = l8; dbest = d; }
            }
            if (l8best) { bl = l8best; bd = dbest; if (l8best == 8 && maxlen > 8) bl = lcp(data + p, data + p - dbest, maxlen); }
            if (p + 4 <= total) {
                uint32_t h = hash4(data + p, HASH_BITS);
                for (int w = 0; w < WAYS; w++) {   /* most recent first; a longer match wins, a tie keeps the nearer */
                    if (table[h][w] == 0xFFFF) break;
                    size_t d = (p + base_rel) - table[h][w];
                    if (d > 32768) break;
                    size_t l = lcp(data + p, data + p - d, maxlen);
                    if (l > bl) { bl = l; bd = d; }
                }
            }
            if (bl < 3 || (bl == 3 && bd > 8)) { bl = 0; bd = 0; }
            if (bl && bl <= MATCH_RULE_MAXLEN) {   /* lengths 3..8 have no extra bits */
                uint32_t lit = 0;
                for (size_t k = 0; k < bl; k++) lit += cost16[data[p + k]];
                if (lit < MATCH_BASE16 + 16u * (uint32_t)DIST_EXTRA[dist_code((int)bd)]) { bl = 0; bd = 0; }
            }
            tok[p - start].len = (uint16_t)bl; tok[p - start].dist = (uint16_t)bd;
        }
        insert_tile(table, HASH_BITS, data, total, base_rel, t0, t1);
        for (size_t p = t0; p < t1; p++) {
            size_t i = p - start;
            taken[i] = 0;
            if (p != carry) continue;
            taken[i] = 1;
            int lazy = tok[i].len && p + 1 < t1 && tok[i + 1].len > tok[i].len;
            if (lazy) tok[i].len = 0;
            carry = p + (tok[i].len ? tok[i].len : 1);
        }
    }
}
/* ------------------------------------------------------------------------------------------------ the min-cost-path parse
 * What libdeflate's levels 10-12 (oxipng -o3 / -o4 call 11 / 12) and zopfli do in their own ways: find, per position, a few candidate
 * matches, give every symbol a cost from the statistics of the previous parse, take the cheapest path through the chunk, and repeat.
 * Restated for the GPU's shape (k_png_parse.hip runs the same steps; every rule below is order-independent or tie-broken explicitly):
 *   WHICH CHUNKS: a chunk whose greedy parse (tokenize) made at least one token in DEEP_DIV (512) a match.  Photographic chunks have next to
 *   no matches and nothing to choose between: they keep the greedy parse (and its speed).
 *   CANDIDATES of position p: distances from (a) the fixed set 1,2,3,4,6,8 -- of these f0 = the nearest whose first 8 bytes agree in
 *   >= 3, f1 = the one that agrees longest inside 8 bytes (ties: the nearer; extended when all 8 agree); (b) the four 4-byte-hash
 *   entries of tokenize's table; (c) the DEEP_WAYS8 entries of a second table keyed by 8 bytes (2048 buckets), which is where the long matches far back
 *   come from.  Both tables are refreshed in tokenize's way but every DEEP_TILE positions: of a tile's positions with one hash the last enters.  Kept per position: c0 = the nearest candidate that matches
 *   >= 3 bytes, c1 = the longest (ties: the nearer), if longer than c0.  Lengths up to c0's use c0's distance, longer ones c1's.
 *   COSTS in 1/16 bit: 16 log2(total / count) (literal_costs' integer log2) per literal / length / distance symbol from the
 *   previous parse's counts, a symbol that did not occur costs as if it had occurred half a time; plus the extra bits.
 *   PATH: the chunk is cut into DEEP_SEG-byte segments (one per GPU lane); per segment, backwards, cost[i] = min over: the literal,
 *   c0 at lengths 3..min(len0, DEEP_CAP) and len0, c1 at lengths len0+1..min(len1, DEEP_CAP) and len1 (lengths above DEEP_CAP only in
 *   full: the cost window of a lane is DEEP_CAP wide).  Ties: the literal, then the shorter length (key = cost << 9 | length).
 *   Matches end at their segment's end.
 *   ITERATIONS: DEEP_ITERS passes, each from the counts of the one before; the first prices literals by the chunk's byte counts and both symbols of
 *   a match at DEEP_START / 16 bits (+ extra bits); --zopfli: DEEP_ITERS_ZOPFLI. */
#define DEEP_DIV 512
#define DEEP_HASH4_BITS 11
#define DEEP_HASH8_BITS 11
#define DEEP_WAYS8 8
#define DEEP_TILE 256   /* positions whose candidates come out of one state of the tables (the GPU wave takes four per lane: independent work in flight together) */
#define DEEP_SEG 512
#define DEEP_CAP 16
#define DEEP_ITERS 5
#define DEEP_START 64   /* 1/16 bit */
#define DEEP_LIVE_NUM 9   /* a trial takes the parse when its greedy stream is within NUM / DEN of the smallest greedy stream of the picture */
#define DEEP_LIVE_DEN 8
#define DEEP_ITERS_ZOPFLI 15
static int deep_div_override = 0;   /* tools only (tools/png_parse_gap.py sweeps it): 0 = DEEP_DIV */
void cso_png_deep_div(int v) { deep_div_override = v; }
static uint32_t hash8(const uint8_t *d) {
    uint32_t lo = d[0] | ((uint32_t)d[1] << 8) | ((uint32_t)d[2] << 16) | ((uint32_t)d[3] << 24);
    uint32_t hi = d[4] | ((uint32_t)d[5] << 8) | ((uint32_t)d[6] << 16) | ((uint32_t)d[7] << 24);
    return ((lo * 0x9E3779B1u) ^ (hi * 0x85EBCA6Bu)) >> (32 - DEEP_HASH8_BITS);
}
static void insert_tile8(uint16_t (*table)[DEEP_WAYS8], const uint8_t *data, size_t total, size_t base_rel, size_t t0, size_t t1) {
    size_t lastpos[1 << DEEP_HASH8_BITS];
    for (size_t p = t0; p < t1 && p + 8 <= total; p++) lastpos[hash8(data + p)] = p;
    for (size_t p = t0; p < t1 && p + 8 <= total; p++) {
        uint32_t h = hash8(data + p);
        size_t rel = p + base_rel;
        if (lastpos[h] != p || rel == 0xFFFF) continue;
        for (int w = DEEP_WAYS8 - 1; w > 0; w--) table[h][w] = table[h][w - 1];
        table[h][0] = (uint16_t)rel;
    }
}
static uint32_t cost16_of(uint32_t c, uint32_t total) {   /* 16 log2(total / c), 1 .. 240; c >= 1, total >= c, total < 2^23 */
    const uint32_t q = (total << 8) / c;
    int e = 31; while (!((q >> e) & 1)) e--;
    uint32_t v = 16u * (uint32_t)(e - 8) + (((q << 4) >> e) & 15u);
    return v < 1 ? 1 : v > 240 ? 240 : v;
}
typedef struct { uint16_t len0, d0, len1, d1; } deep_cand;
static void deep_costs(const uint32_t *lf, const uint32_t *df, uint32_t *lit_cost, uint32_t *len_cost, uint32_t *dist_cost) {
    uint32_t tl = 0, td = 0;
    for (int i = 0; i < 286; i++) tl += lf[i];
    for (int i = 0; i < 30; i++) td += df[i];
    for (int i = 0; i < 256; i++) lit_cost[i] = lf[i] ? cost16_of(lf[i], tl) : cost16_of(1, 2 * tl);
    for (int l = 3; l <= 258; l++) { int c = len_code(l); len_cost[l] = (lf[257 + c] ? cost16_of(lf[257 + c], tl) : cost16_of(1, 2 * tl)) + 16u * (uint32_t)LEN_EXTRA[c]; }
    for (int c = 0; c < 30; c++) dist_cost[c] = (td == 0 ? 80u : df[c] ? cost16_of(df[c], td) : cost16_of(1, 2 * td)) + 16u * (uint32_t)DIST_EXTRA[c];
}
/* what a block with these counts takes, in 1/16 bit: the entropy of its two alphabets + the extra bits */
static uint64_t deep_estimate(const uint32_t *lf, const uint32_t *df) {
    uint32_t tl = 0, td = 0;
    uint64_t e = 0;
    for (int i = 0; i < 286; i++) tl += lf[i];
    for (int i = 0; i < 30; i++) td += df[i];
    for (int i = 0; i < 286; i++) if (lf[i]) e += (uint64_t)lf[i] * (cost16_of(lf[i], tl) + 16u * (uint32_t)(i > 256 ? LEN_EXTRA[i - 257] : 0));
    for (int i = 0; i < 30; i++) if (df[i]) e += (uint64_t)df[i] * (cost16_of(df[i], td) + 16u * (uint32_t)DIST_EXTRA[i]);
    return e;
}
/* tok / taken: out, as tokenize() */
static void deep_parse(const uint8_t *data, size_t total, size_t start, size_t end, int iters, token *tok, uint8_t *taken) {
    const size_t n = end - start;
    deep_cand *cand = (deep_cand *)malloc(sizeof(deep_cand) * n);
    {
        uint16_t table[1 << DEEP_HASH4_BITS][WAYS];
        static uint16_t table8[1 << DEEP_HASH8_BITS][DEEP_WAYS8];
        memset(table, 0xFF, sizeof table);
        memset(table8, 0xFF, sizeof table8);
        const size_t seed0 = start > 32768 ? start - 32768 : 0;
        const size_t base_rel = 32768 - start;
        for (size_t t0 = seed0; t0 < start; t0 += DEEP_TILE) { insert_tile(table, DEEP_HASH4_BITS, data, total, base_rel, t0, t0 + DEEP_TILE); insert_tile8(table8, data, total, base_rel, t0, t0 + DEEP_TILE); }
        for (size_t t0 = start; t0 < end; t0 += DEEP_TILE) {
            size_t t1 = t0 + DEEP_TILE < end ? t0 + DEEP_TILE : end;
            for (size_t p = t0; p < t1; p++) {
                const size_t maxlen = end - p < 258 ? end - p : 258;
                size_t len0 = 0, d0 = 0, len1 = 0, d1 = 0;   /* c0: nearest with >= 3; c1: longest, ties nearer */
#define DEEP_OFFER(L_, D_) do { size_t L__ = (L_), D__ = (D_); if (L__ >= 3 && (!d0 || D__ < d0)) { len0 = L__; d0 = D__; } if (L__ > len1 || (L__ == len1 && L__ && D__ < d1)) { len1 = L__; d1 = D__; } } while (0)
                {
                    size_t l8best = 0, dbest = 0, f0l = 0, f0d = 0;
                    for (int k = 0; k < 6; k++) {
                        size_t d = (size_t)FIXED_DIST[k];
                        if (d > p) continue;
                        size_t l8 = lcp(data + p, data + p - d, maxlen < 8 ? maxlen : 8);
                        if (l8 > l8best) { l8best = l8; dbest = d; }
                        if (l8 >= 3 && !f0d) { f0l = l8; f0d = d; }
                    }
                    if (l8best) {
                        size_t l = l8best;
                        if (l8best == 8 && maxlen > 8) l = lcp(data + p, data + p - dbest, maxlen);
                        if (f0d && f0d != dbest) DEEP_OFFER(f0l, f0d);
                        DEEP_OFFER(l, dbest);
                    }
                }
                if (p + 4 <= total) {
                    uint32_t h = hash4(data + p, DEEP_HASH4_BITS);
                    for (int w = 0; w < WAYS; w++) {
                        if (table[h][w] == 0xFFFF) break;
                        size_t d = (p + base_rel) - table[h][w];
                        if (d > 32768) break;
                        DEEP_OFFER(lcp(data + p, data + p - d, maxlen), d);
                    }
                }
                if (p + 8 <= total) {
                    uint32_t h = hash8(data + p);
                    for (int w = 0; w < DEEP_WAYS8; w++) {
                        if (table8[h][w] == 0xFFFF) break;
                        size_t d = (p + base_rel) - table8[h][w];
                        if (d > 32768) break;
                        DEEP_OFFER(lcp(data + p, data + p - d, maxlen), d);
                    }
                }
#undef DEEP_OFFER
                if (len1 <= len0) { len1 = 0; d1 = 0; }
                deep_cand *c = &cand[p - start];
                c->len0 = (uint16_t)len0; c->d0 = (uint16_t)(d0 & 0xFFFF); c->len1 = (uint16_t)len1; c->d1 = (uint16_t)(d1 & 0xFFFF);   /* 32768 is kept as 32768 */
            }
            insert_tile(table, DEEP_HASH4_BITS, data, total, base_rel, t0, t1);
            insert_tile8(table8, data, total, base_rel, t0, t1);
        }
    }
    uint32_t lf[286], df[30];   /* the first pass's counts: every byte of the chunk a literal (its matches: DEEP_START) */
    memset(lf, 0, sizeof lf); memset(df, 0, sizeof df);
    for (size_t p = start; p < end; p++) lf[data[p]]++;
    uint32_t *cost = (uint32_t *)malloc(sizeof(uint32_t) * (DEEP_SEG + 1));
    uint16_t *choice = (uint16_t *)malloc(sizeof(uint16_t) * n);
    for (int it = 0; it < iters; it++) {
        uint32_t lit_cost[256], len_cost[259], dist_cost[30];
        deep_costs(lf, df, lit_cost, len_cost, dist_cost);
        if (it == 0) {   /* no parse yet: start as if a match's two symbols cost DEEP_START / 16 bits each */
            for (int l = 3; l <= 258; l++) len_cost[l] = DEEP_START + 16u * (uint32_t)LEN_EXTRA[len_code(l)];
            for (int c = 0; c < 30; c++) dist_cost[c] = DEEP_START + 16u * (uint32_t)DIST_EXTRA[c];
        }
        memset(lf, 0, sizeof lf); memset(df, 0, sizeof df);
        for (size_t s0 = 0; s0 < n; s0 += DEEP_SEG) {
            const size_t ns = n - s0 < DEEP_SEG ? n - s0 : DEEP_SEG;
            cost[ns] = 0;
            for (size_t i = ns; i-- > 0;) {
                const deep_cand *c = &cand[s0 + i];
                const size_t avail = ns - i;
                const size_t l0 = c->len0 < avail ? c->len0 : avail, l1 = c->len1 < avail ? c->len1 : avail;
                uint32_t best = ((cost[i + 1] + lit_cost[data[start + s0 + i]]) << 9) | 1u;
                if (l0 >= 3) {
                    const uint32_t dc0 = dist_cost[dist_code(c->d0 ? c->d0 : 1)];
                    const size_t top = l0 < DEEP_CAP ? l0 : DEEP_CAP;
                    for (size_t l = 3; l <= top; l++) { uint32_t k = ((cost[i + l] + len_cost[l] + dc0) << 9) | (uint32_t)l; if (k < best) best = k; }
                    if (l0 > DEEP_CAP) { uint32_t k = ((cost[i + l0] + len_cost[l0] + dc0) << 9) | (uint32_t)l0; if (k < best) best = k; }
                    if (l1 > l0) {
                        const uint32_t dc1 = dist_cost[dist_code(c->d1)];
                        const size_t top1 = l1 < DEEP_CAP ? l1 : DEEP_CAP;
                        for (size_t l = l0 + 1; l <= top1; l++) { uint32_t k = ((cost[i + l] + len_cost[l] + dc1) << 9) | (uint32_t)l; if (k < best) best = k; }
                        if (l1 > DEEP_CAP) { uint32_t k = ((cost[i + l1] + len_cost[l1] + dc1) << 9) | (uint32_t)l1; if (k < best) best = k; }
                    }
                }
                cost[i] = best >> 9;
                choice[s0 + i] = (uint16_t)(best & 511u);
            }
            for (size_t i = 0; i < ns;) {
                const deep_cand *c = &cand[s0 + i];
                const size_t avail = ns - i, l = choice[s0 + i];
                if (l == 1) { lf[data[start + s0 + i]]++; i++; continue; }
                const size_t l0 = c->len0 < avail ? c->len0 : avail;
                const size_t d = l <= l0 ? c->d0 : c->d1;
                lf[257 + len_code((int)l)]++; df[dist_code((int)d)]++;
                i += l;
            }
        }
        lf[256] = 1;
    }
    memset(taken, 0, n);
    for (size_t s0 = 0; s0 < n; s0 += DEEP_SEG) {
        const size_t ns = n - s0 < DEEP_SEG ? n - s0 : DEEP_SEG;
        for (size_t i = 0; i < ns;) {
            const deep_cand *c = &cand[s0 + i];
            const size_t avail = ns - i, l = choice[s0 + i];
            taken[s0 + i] = 1;
            if (l == 1) { tok[s0 + i].len = 0; tok[s0 + i].dist = 0; i++; continue; }
            const size_t l0 = c->len0 < avail ? c->len0 : avail;
            tok[s0 + i].len = (uint16_t)l; tok[s0 + i].dist = (uint16_t)(l <= l0 ? c->d0 : c->d1);
            i += l;
        }
    }
    free(cand); free(cost); free(choice);
}
/* code lengths for freq[0..n): Huffman, then limited to `limit` bits */
static void code_lengths(const uint32_t *freq_in, int n, int limit, uint8_t *len_out) {
    uint32_t freq[288]; int codesize[288], others[288], idx[288], m = 0;
    uint32_t f2[288];
    memcpy(f2, freq_in, sizeof(uint32_t) * (size_t)n);
    int used = 0;
    for (int i = 0; i < n; i++) used += f2[i] != 0;
    for (int i = 0; i < n && used < 2; i++) if (!f2[i]) { f2[i] = 1; used++; }   /* zlib: force at least two codes */
    for (int i = 0; i < n; i++) { len_out[i] = 0; if (f2[i]) { freq[m] = f2[i]; idx[m] = i; codesize[m] = 0; others[m] = -1; m++; } }
    for (;;) {
        int c1 = -1, c2 = -1;
        uint64_t v = ~0ull;
        for (int i = 0; i < m; i++) if (freq[i] && freq[i] <= v) { v = freq[i]; c1 = i; }
        v = ~0ull;
        for (int i = 0; i < m; i++) if (freq[i] && freq[i] <= v && i != c1) { v = freq[i]; c2 = i; }
        if (c2 < 0) break;
        freq[c1] += freq[c2]; freq[c2] = 0;
        codesize[c1]++; while (others[c1] >= 0) { c1 = others[c1]; codesize[c1]++; }
        others[c1] = c2;
        codesize[c2]++; while (others[c2] >= 0) { c2 = others[c2]; codesize[c2]++; }
    }
    int bits[64]; memset(bits, 0, sizeof bits);
    for (int i = 0; i < m; i++) bits[codesize[i] > 63 ? 63 : codesize[i]]++;
    for (int i = 63; i > limit; i--)
        while (bits[i] > 0) {
            int j = i - 2; while (bits[j] == 0) j--;
            bits[i] -= 2; bits[i - 1]++; bits[j + 1] += 2; bits[j]--;
        }
    /* symbols in order of (unlimited) code size, then of symbol, take the limited lengths shortest first */
    int l = 1;
    for (int cs = 1; cs < 64; cs++)
        for (int i = 0; i < m; i++)
            if ((codesize[i] > 63 ? 63 : codesize[i]) == cs) { while (bits[l] == 0) l++; bits[l]--; len_out[idx[i]] = (uint8_t)l; }
}
static void canonical(const uint8_t *len, int n, uint16_t *code) {   /* bit-reversed canonical codes, as deflate packs them */
    int count[16] = {0}, next[16];
    for (int i = 0; i < n; i++) count[len[i]]++;
    count[0] = 0;
    int c = 0;
    for (int l = 1; l < 16; l++) { c = (c + count[l - 1]) << 1; next[l] = c; }
    for (int i = 0; i < n; i++) {
        code[i] = 0;
        if (!len[i]) continue;
        int v = next[len[i]]++, r = 0;
        for (int b = 0; b < len[i]; b++) r |= ((v >> b) & 1) << (len[i] - 1 - b);
        code[i] = (uint16_t)r;
    }
}
typedef struct { uint8_t *p; size_t n, cap; uint64_t acc; int nb; } obits;
static void put(obits *o, uint32_t v, int n) {
    o->acc |= (uint64_t)v << o->nb; o->nb += n;
    while (o->nb >= 8) {
        if (o->n == o->cap) { o->cap = o->cap * 2 + 64; o->p = (uint8_t *)realloc(o->p, o->cap); }
        o->p[o->n++] = (uint8_t)o->acc; o->acc >>= 8; o->nb -= 8;
    }
}
static void align(obits *o) { if (o->nb) put(o, 0, 8 - o->nb); }

/* the code-length sequence of a block header: run-length symbols over the concatenated litlen + dist lengths */
static int header_symbols(const uint8_t *seq, int n, uint8_t *sym, uint8_t *extra) {
    int m = 0;
    for (int i = 0; i < n;) {
        int v = seq[i], r = 1;
        while (i + r < n && seq[i + r] == v) r++;
        i += r;
        if (v == 0) {
            while (r >= 11) { int t = r > 138 ? 138 : r; sym[m] = 18; extra[m++] = (uint8_t)(t - 11); r -= t; }
            if (r >= 3) { sym[m] = 17; extra[m++] = (uint8_t)(r - 3); r = 0; }
            while (r--) { sym[m] = 0; extra[m++] = 0; }
        } else {
            sym[m] = (uint8_t)v; extra[m++] = 0; r--;
            while (r >= 3) { int t = r > 6 ? 6 : r; sym[m] = 16; extra[m++] = (uint8_t)(t - 3); r -= t; }
            while (r--) { sym[m] = (uint8_t)v; extra[m++] = 0; }
        }
    }
    return m;
}
static void deflate_chunk(const uint8_t *data, size_t total, size_t start, size_t end, int last, int iters, obits *o) {
    size_t n = end - start;
    token *tok = (token *)malloc(sizeof(token) * n);
    uint8_t *taken = (uint8_t *)malloc(n);
    tokenize(data, total, start, end, tok, taken);
    uint32_t lf[286], df[30];
    memset(lf, 0, sizeof lf); memset(df, 0, sizeof df);
    for (size_t i = 0; i < n; i++) {
        if (!taken[i]) continue;
        if (tok[i].len) { lf[257 + len_code(tok[i].len)]++; df[dist_code(tok[i].dist)]++; } else lf[data[start + i]]++;
    }
    lf[256] = 1;
    {
        uint32_t nm = 0, nt = 0;
        for (int i = 0; i < 286; i++) if (i != 256) nt += lf[i];
        for (int i = 257; i < 286; i++) nm += lf[i];
        if (iters > 0 && nm * (uint32_t)(deep_div_override ? deep_div_override : DEEP_DIV) >= nt) {
            const uint64_t est_greedy = deep_estimate(lf, df);
            token *gtok = (token *)malloc(sizeof(token) * n); uint8_t *gtaken = (uint8_t *)malloc(n);
            memcpy(gtok, tok, sizeof(token) * n); memcpy(gtaken, taken, n);
            double ent0 = 0; uint64_t avgl = 0;
            if (getenv("CSO_DEEP_REPORT")) { uint16_t c16[256]; literal_costs(data, start, end, c16); for (size_t i = start; i < end; i++) avgl += c16[data[i]]; avgl /= n;
                uint32_t T = 0, TD = 0; for (int i = 0; i < 286; i++) T += lf[i]; for (int i = 0; i < 30; i++) TD += df[i];
                for (int i = 0; i < 286; i++) if (lf[i]) ent0 += lf[i] * (double)cost16_of(lf[i], T) / 16 + (i > 256 ? lf[i] * LEN_EXTRA[i - 257] : 0);
                for (int i = 0; i < 30; i++) if (df[i]) ent0 += df[i] * (double)cost16_of(df[i], TD) / 16 + df[i] * DIST_EXTRA[i]; }
            deep_parse(data, total, start, end, iters, tok, taken);
            memset(lf, 0, sizeof lf); memset(df, 0, sizeof df);
            for (size_t i = 0; i < n; i++) {
                if (!taken[i]) continue;
                if (tok[i].len) { lf[257 + len_code(tok[i].len)]++; df[dist_code(tok[i].dist)]++; } else lf[data[start + i]]++;
            }
            lf[256] = 1;
            if (deep_estimate(lf, df) >= est_greedy) {   /* the parse must promise a smaller block (segment ends cut long runs: a flat chunk can lose) */
                memcpy(tok, gtok, sizeof(token) * n); memcpy(taken, gtaken, n);
                memset(lf, 0, sizeof lf); memset(df, 0, sizeof df);
                for (size_t i = 0; i < n; i++) {
                    if (!taken[i]) continue;
                    if (tok[i].len) { lf[257 + len_code(tok[i].len)]++; df[dist_code(tok[i].dist)]++; } else lf[data[start + i]]++;
                }
                lf[256] = 1;
            }
            free(gtok); free(gtaken);
            if (getenv("CSO_DEEP_REPORT")) { double ent1 = 0;
                uint32_t T = 0, TD = 0; for (int i = 0; i < 286; i++) T += lf[i]; for (int i = 0; i < 30; i++) TD += df[i];
                for (int i = 0; i < 286; i++) if (lf[i]) ent1 += lf[i] * (double)cost16_of(lf[i], T) / 16 + (i > 256 ? lf[i] * LEN_EXTRA[i - 257] : 0);
                for (int i = 0; i < 30; i++) if (df[i]) ent1 += df[i] * (double)cost16_of(df[i], TD) / 16 + df[i] * DIST_EXTRA[i];
                fprintf(stderr, "chunk %zu avglit16 %llu nm %u nt %u greedy %.0f deep %.0f gain %.2f%%\n", start / CHUNK, (unsigned long long)avgl, nm, nt, ent0 / 8, ent1 / 8, 100 * (ent0 - ent1) / ent0); }
        }
    }
    uint8_t ll[286], dl[30];
    uint16_t lc[286], dc[30];
    code_lengths(lf, 286, 15, ll);
    code_lengths(df, 30, 15, dl);
    canonical(ll, 286, lc); canonical(dl, 30, dc);
    int nl = 286, nd = 30;
    while (nl > 257 && !ll[nl - 1]) nl--;
    while (nd > 1 && !dl[nd - 1]) nd--;
    uint8_t seq[316], sym[316], extra[316];
    memcpy(seq, ll, (size_t)nl); memcpy(seq + nl, dl, (size_t)nd);
    int m = header_symbols(seq, nl + nd, sym, extra);
    uint32_t cf[19]; memset(cf, 0, sizeof cf);
    for (int i = 0; i < m; i++) cf[sym[i]]++;
    uint8_t cl[19]; uint16_t cc[19];
    code_lengths(cf, 19, 7, cl);
    canonical(cl, 19, cc);
    int ncl = 19;
    while (ncl > 4 && !cl[CL_ORDER[ncl - 1]]) ncl--;
    put(o, last ? 1 : 0, 1); put(o, 2, 2);
    put(o, (uint32_t)(nl - 257), 5); put(o, (uint32_t)(nd - 1), 5); put(o, (uint32_t)(ncl - 4), 4);
    for (int i = 0; i < ncl; i++) put(o, cl[CL_ORDER[i]], 3);
    for (int i = 0; i < m; i++) {
        put(o, cc[sym[i]], cl[sym[i]]);
        if (sym[i] == 16) put(o, extra[i], 2); else if (sym[i] == 17) put(o, extra[i], 3); else if (sym[i] == 18) put(o, extra[i], 7);
    }
    for (size_t i = 0; i < n; i++) {
        if (!taken[i]) continue;
        if (tok[i].len) {
            int c = len_code(tok[i].len), d = dist_code(tok[i].dist);
            put(o, lc[257 + c], ll[257 + c]); put(o, (uint32_t)(tok[i].len - LEN_BASE[c]), LEN_EXTRA[c]);
            put(o, dc[d], dl[d]); put(o, (uint32_t)(tok[i].dist - DIST_BASE[d]), DIST_EXTRA[d]);
        } else
            put(o, lc[data[start + i]], ll[data[start + i]]);
    }
    put(o, lc[256], ll[256]);
    if (last) align(o);
    else { put(o, 0, 3); align(o); put(o, 0, 16); put(o, 0xFFFF, 16); }
    free(tok); free(taken);
}
/* Brute score: estimated bits of one candidate row (type byte first) coded as a chunk of its own with a dynamic code:
   n*log2(n) - sum c*log2(c) over the literal/length and the distance histograms of its tokens (ilog2i), plus the extra
   bits.  Rows longer than a chunk are scored on their first CHUNK bytes. */
static uint64_t fixed_cost_row(const uint8_t *row, size_t n, int bpp) {
    (void)bpp;
    if (n > CHUNK) n = CHUNK;
    token *tok = (token *)malloc(sizeof(token) * n);
    uint8_t *taken = (uint8_t *)malloc(n);
    tokenize(row, n, 0, n, tok, taken);
    uint32_t lf[286], df[30];
    memset(lf, 0, sizeof lf); memset(df, 0, sizeof df);
    uint64_t extra = 0, nl = 0, nd = 0;
    for (size_t i = 0; i < n; i++) {
        if (!taken[i]) continue;
        nl++;
        if (tok[i].len) { int c = len_code(tok[i].len), d = dist_code(tok[i].dist); lf[257 + c]++; df[d]++; nd++; extra += (uint64_t)(LEN_EXTRA[c] + DIST_EXTRA[d]); }
        else lf[row[i]]++;
    }
    uint64_t bits = ilog2i(nl) + ilog2i(nd) + extra, sub = 0;
    for (int i = 0; i < 286; i++) sub += ilog2i(lf[i]);
    for (int i = 0; i < 30; i++) sub += ilog2i(df[i]);
    free(tok); free(taken);
    return bits - sub;
}
int cso_deflate_zlib_iters(const uint8_t *data, size_t n, int iters, uint8_t **out, size_t *out_len);
int cso_deflate_zlib(const uint8_t *data, size_t n, uint8_t **out, size_t *out_len) { return cso_deflate_zlib_iters(data, n, DEEP_ITERS, out, out_len); }
/* iters: passes of the min-cost-path parse over the chunks that qualify (0: greedy parse everywhere; DEEP_ITERS; --zopfli: DEEP_ITERS_ZOPFLI) */
int cso_deflate_zlib_iters(const uint8_t *data, size_t n, int iters, uint8_t **out, size_t *out_len) {
    obits o; memset(&o, 0, sizeof o);
    put(&o, 0x78, 8); put(&o, 0xDA, 8);
    if (n == 0) { put(&o, 1, 1); put(&o, 1, 2); put(&o, 0, 7); align(&o); }
    for (size_t s = 0; s < n; s += CHUNK) {
        size_t e = s + CHUNK < n ? s + CHUNK : n;
        deflate_chunk(data, n, s, e, e == n, iters, &o);
    }
    uint32_t ad = cso_adler32(data, n);
    put(&o, ad >> 24, 8); put(&o, (ad >> 16) & 255, 8); put(&o, (ad >> 8) & 255, 8); put(&o, ad & 255, 8);
    *out = o.p; *out_len = o.n;
    return 0;
}

/* ------------------------------------------------------------------------------------------------ the whole row: optimise
 * trial sets per --png-opt-level, after oxipng's presets [UPSTREAM-RECALL]: 0,1 -> {5}; 2 -> {0,1,6,7}; 3,4 -> {0,7,8,9};
 * 5 -> {0,1,2,5,6,7,8,9}; 6 -> {0..9}.  (The presets' libdeflate levels have no counterpart: one coder here.)  The
 * smallest stream wins (ties: the earlier trial); when the new file is not smaller than the input, the input is
 * returned unchanged (oxipng: "file already optimized"). */
int cso_png_trials(int level, int *set) {
    static const int s01[] = {5}, s2[] = {0, 1, 6, 7}, s34[] = {0, 7, 8, 9}, s5[] = {0, 1, 2, 5, 6, 7, 8, 9}, s6[] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9};
    const int *s; int n;
    if (level <= 1) { s = s01; n = 1; } else if (level == 2) { s = s2; n = 4; } else if (level <= 4) { s = s34; n = 4; } else if (level == 5) { s = s5; n = 8; } else { s = s6; n = 10; }
    memcpy(set, s, sizeof(int) * (size_t)n);
    return n;
}
static int png_recode(const uint8_t *in, size_t n, int level, int keep_metadata, int lossy, int quality, int iters, uint8_t **out, size_t *out_len, int *chosen) {
    cso_png *P = NULL;
    int rc = cso_png_decode(in, n, keep_metadata, &P);
    if (rc) return rc;
    cso_png_reduce(P);
    if (lossy) quantize(P, quality);
    size_t raw_len = (1 + P->rowbytes) * (size_t)P->height;
    uint8_t *filt = (uint8_t *)malloc(raw_len), *best = NULL;
    size_t best_len = 0;
    int set[10], ns = cso_png_trials(level, set), best_s = -1;
    /* every trial with the greedy parse first; the min-cost-path parse then only for the trials within an eighth of the smallest (it gains a few
       percent: a trial further behind cannot win -- on photographs that is filter None, the one stream full of matches) */
    uint8_t *zt[10]; size_t zn[10], smallest = 0;
    for (int t = 0; t < ns; t++) {
        cso_png_filter(P, set[t], filt, NULL);
        cso_deflate_zlib_iters(filt, raw_len, 0, &zt[t], &zn[t]);
        if (t == 0 || zn[t] < smallest) smallest = zn[t];
    }
    for (int t = 0; t < ns; t++) {
        uint8_t *z = zt[t]; size_t zl = zn[t];
        if (iters > 0 && (uint64_t)zn[t] * DEEP_LIVE_DEN <= (uint64_t)smallest * DEEP_LIVE_NUM) {
            free(z);
            cso_png_filter(P, set[t], filt, NULL);
            cso_deflate_zlib_iters(filt, raw_len, iters, &z, &zl);
        }
        if (!best || zl < best_len) { free(best); best = z; best_len = zl; best_s = set[t]; } else free(z);
    }
    free(filt);
    /* signature, IHDR, the kept chunks in their order with the one new IDAT where the first IDAT stood, IEND */
    size_t cap = 8 + 25 + P->chunks_len + 12 + best_len + 12;
    uint8_t *o = (uint8_t *)malloc(cap), *w = o;
    memcpy(w, PNG_SIG, 8); w += 8;
    put_be32(w, 13); memcpy(w + 4, "IHDR", 4); put_be32(w + 8, P->width); put_be32(w + 12, P->height);
    w[16] = (uint8_t)P->depth; w[17] = (uint8_t)P->ctype; w[18] = 0; w[19] = 0; w[20] = 0;
    put_be32(w + 21, cso_crc32(0, w + 4, 17)); w += 25;
    memcpy(w, P->chunks, P->idat_at); w += P->idat_at;
    put_be32(w, (uint32_t)best_len); memcpy(w + 4, "IDAT", 4); memcpy(w + 8, best, best_len);
    put_be32(w + 8 + best_len, cso_crc32(0, w + 4, 4 + best_len)); w += 12 + best_len;
    memcpy(w, P->chunks + P->idat_at, P->chunks_len - P->idat_at); w += P->chunks_len - P->idat_at;
    put_be32(w, 0); memcpy(w + 4, "IEND", 4); put_be32(w + 8, 0xAE426082u); w += 12;
    size_t total = (size_t)(w - o);
    free(best);
    cso_png_free(P);
    if (chosen) *chosen = best_s;
    if (!lossy && total >= n) { free(o); o = (uint8_t *)malloc(n); memcpy(o, in, n); total = n; if (chosen) *chosen = -1; }   /* oxipng: "already optimised" */
    *out = o; *out_len = total;
    return 0;
}
int cso_png_optimize(const uint8_t *in, size_t n, int level, int keep_metadata, uint8_t **out, size_t *out_len, int *chosen) {
    return png_recode(in, n, level, keep_metadata, 0, 0, DEEP_ITERS, out, out_len, chosen);
}
/* png.force_zopfli (--zopfli): the same coder with DEEP_ITERS_ZOPFLI passes of the cost model */
int cso_png_optimize_zopfli(const uint8_t *in, size_t n, int level, int keep_metadata, uint8_t **out, size_t *out_len, int *chosen) {
    return png_recode(in, n, level, keep_metadata, 0, 0, DEEP_ITERS_ZOPFLI, out, out_len, chosen);
}
/* tools: any number of passes (0 = the greedy parse everywhere) */
int cso_png_optimize_iters(const uint8_t *in, size_t n, int level, int iters, uint8_t **out, size_t *out_len) {
    return png_recode(in, n, level, 0, 0, 0, iters, out, out_len, NULL);
}
/* `-q` on a PNG: the reductions, the quantiser, then the same filter trials and coder; the result is returned whatever its size */
int cso_png_lossy(const uint8_t *in, size_t n, int level, int keep_metadata, int quality, uint8_t **out, size_t *out_len) {
    return png_recode(in, n, level, keep_metadata, 1, quality, DEEP_ITERS, out, out_len, NULL);
}

/* ---- PNG -> WebP (caesium::convert_in_memory with a PNG source, /root/reference/src/compressor.rs:289-299): the decoded pixels as the
   8-bit RGB the VP8 encoder imports.  Opaque formats only (the device build refuses transparency).  16-bit samples round as
   image-rs converts them, (v + 128) / 257 [UPSTREAM-RECALL]; sub-byte grey scales to the full range; an index past the PLTE is black */
int cso_png_to_rgb(const cso_png *P, uint8_t *rgb) {
    const uint8_t *plte = NULL;
    int npal = 0;
    for (size_t pos = 0; pos + 12 <= P->chunks_len;) {
        const uint32_t len = be32(P->chunks + pos);
        if (!memcmp(P->chunks + pos + 4, "PLTE", 4)) { plte = P->chunks + pos + 8; npal = (int)(len / 3); }
        if (!memcmp(P->chunks + pos + 4, "tRNS", 4)) return CSO_PNG_UNSUPPORTED;
        pos += 12 + (size_t)len;
    }
    if (P->ctype == 4 || P->ctype == 6) return CSO_PNG_UNSUPPORTED;
    for (uint32_t y = 0; y < P->height; y++) {
        const uint8_t *r = P->pix + (size_t)y * P->rowbytes;
        uint8_t *o = rgb + (size_t)y * P->width * 3;
        for (uint32_t x = 0; x < P->width; x++, o += 3) {
            if (P->ctype == 2) {
                for (int c = 0; c < 3; c++)
                    o[c] = P->depth == 16 ? (uint8_t)(((((uint32_t)r[6 * (size_t)x + 2 * c] << 8) | r[6 * (size_t)x + 2 * c + 1]) + 128u) / 257u) : r[3 * (size_t)x + c];
                continue;
            }
            uint32_t v;
            if (P->depth == 16) v = ((((uint32_t)r[2 * (size_t)x] << 8) | r[2 * (size_t)x + 1]) + 128u) / 257u;
            else if (P->depth == 8) v = r[x];
            else {
                const uint32_t per = 8u / (uint32_t)P->depth, k = x % per;
                v = ((uint32_t)r[x / per] >> (8u - (uint32_t)P->depth - k * (uint32_t)P->depth)) & ((1u << P->depth) - 1u);
                if (P->ctype == 0) v *= 255u / ((1u << P->depth) - 1u);
            }
            if (P->ctype == 3) {
                if ((int)v < npal) { o[0] = plte[3 * v]; o[1] = plte[3 * v + 1]; o[2] = plte[3 * v + 2]; } else { o[0] = o[1] = o[2] = 0; }
            } else o[0] = o[1] = o[2] = (uint8_t)v;
        }
    }
    return 0;
}
int cso_png_to_webp(const uint8_t *in, size_t n, int quality, uint8_t **out, size_t *out_len) {
    cso_png *P = NULL;
    int rc = cso_png_decode(in, n, 0, &P);
    if (rc) return rc;
    uint8_t *rgb = (uint8_t *)malloc((size_t)P->width * P->height * 3 + 1);
    rc = cso_png_to_rgb(P, rgb);
    if (!rc && cso_webp_encode_rgb(rgb, (int)P->width, (int)P->height, quality, out, out_len)) rc = CSO_PNG_UNSUPPORTED;
    free(rgb);
    cso_png_free(P);
    return rc;
}

/* ------------------------------------------------------------------------------------------------------------------------------------
 * Lossless WebP OUTPUT (VP8L), the statement the device coder (caesium-clt_amd/csrc/k_vp8l_enc.hip) is compared with byte for byte.
 * Replaces, for webp.lossless, libwebp's lossless coder as libcaesium calls it (/root/reference/src/compressor.rs:427-429, call sites
 * :289-305).  NOT libwebp's bytes -- "parity unpinned": the stream uses the format's data-parallel tools only (subtract-green, the
 * spatial predictor with the best of the 14 modes per 16 x 16 block by the sum of absolute residuals, every mode predicting from ORIGINAL
 * neighbours, one group of prefix codes limited to 15 bits); what is pinned is the format (WebP Lossless Bitstream Specification,
 * sections 4.1 "predictor transform", 4.3 "subtract green", 6.2 "details of decoding prefix codes"): libwebp decodes the file to the
 * source pixels (tests/test_webp_lossless_emul.py).  Lives in this file because it shares code_lengths() / canonical() with DEFLATE.
 * px: `channels` (1 grey, 2 grey + alpha, 3 RGB, 4 RGBA) bytes per pixel.  Returns 0, *out malloc'ed. */
static uint32_t l_avg(uint32_t a, uint32_t b) {
    uint32_t r = 0;
    for (int s = 0; s < 32; s += 8) r |= ((((a >> s) & 255u) + ((b >> s) & 255u)) >> 1) << s;
    return r;
}
static uint32_t l_clip(int v) { return v < 0 ? 0u : v > 255 ? 255u : (uint32_t)v; }
static uint32_t l_predict(int mode, uint32_t L, uint32_t T, uint32_t TR, uint32_t TL) {
    uint32_t r = 0;
    switch (mode) {
    case 0: return 0xFF000000u;
    case 1: return L;
    case 2: return T;
    case 3: return TR;
    case 4: return TL;
    case 5: return l_avg(l_avg(L, TR), T);
    case 6: return l_avg(L, TL);
    case 7: return l_avg(L, T);
    case 8: return l_avg(TL, T);
    case 9: return l_avg(T, TR);
    case 10: return l_avg(l_avg(L, TL), l_avg(T, TR));
    case 11: {   /* Select: the neighbour nearer to the gradient estimate L + T - TL (Manhattan distance over the four channels) */
        int pl = 0, pt = 0;
        for (int s = 0; s < 32; s += 8) {
            const int l = (int)((L >> s) & 255u), t = (int)((T >> s) & 255u), tl = (int)((TL >> s) & 255u);
            pl += abs(t - tl);   /* |(l + t - tl) - l| */
            pt += abs(l - tl);   /* |(l + t - tl) - t| */
        }
        return pl < pt ? L : T;
    }
    case 12:
        for (int s = 0; s < 32; s += 8) r |= l_clip((int)((L >> s) & 255u) + (int)((T >> s) & 255u) - (int)((TL >> s) & 255u)) << s;
        return r;
    case 13: {
        const uint32_t a = l_avg(L, T);
        for (int s = 0; s < 32; s += 8) { const int x = (int)((a >> s) & 255u), y = (int)((TL >> s) & 255u); r |= l_clip(x + (x - y) / 2) << s; }
        return r;
    }
    default: return 0xFF000000u;
    }
}
static uint32_t l_sub(uint32_t a, uint32_t b) {   /* per channel, modulo 256 */
    uint32_t r = 0;
    for (int s = 0; s < 32; s += 8) r |= ((((a >> s) & 255u) - ((b >> s) & 255u)) & 255u) << s;
    return r;
}
static uint32_t l_sg(const uint8_t *px, int w, int channels, int x, int y) {   /* ARGB after the subtract-green transform */
    const uint8_t *p = px + ((size_t)y * (size_t)w + (size_t)x) * (size_t)channels;
    if (channels <= 2) return (channels == 2 ? (uint32_t)p[1] << 24 : 0xFF000000u) | ((uint32_t)p[0] << 8);
    const uint32_t r = p[0], g = p[1], b = p[2];
    return (channels == 4 ? (uint32_t)p[3] << 24 : 0xFF000000u) | (((r - g) & 255u) << 16) | (g << 8) | ((b - g) & 255u);
}
static uint32_t l_pred_at(const uint8_t *px, int w, int channels, int x, int y, int mode) {   /* the frame's rules: first pixel black, first row left, first column top */
    if (y == 0) return x == 0 ? 0xFF000000u : l_sg(px, w, channels, x - 1, 0);
    if (x == 0) return l_sg(px, w, channels, 0, y - 1);
    const uint32_t TR = x + 1 < w ? l_sg(px, w, channels, x + 1, y - 1) : l_sg(px, w, channels, 0, y);   /* one past the row above = the row's own first pixel */
    return l_predict(mode, l_sg(px, w, channels, x - 1, y), l_sg(px, w, channels, x, y - 1), TR, l_sg(px, w, channels, x - 1, y - 1));
}
typedef struct { uint8_t len[288]; uint16_t code[288]; int used, s0, s1, last; } lcode;
static void l_make_code(lcode *c, const uint32_t *f, int n) {
    code_lengths(f, n, 15, c->len);
    c->used = 0; c->s0 = c->s1 = c->last = 0;
    for (int i = 0; i < n; i++) if (f[i]) { if (c->used == 0) c->s0 = i; else if (c->used == 1) c->s1 = i; c->used++; c->last = i; }
    if (c->used <= 1) memset(c->len, 0, (size_t)n);   /* a code with one symbol costs no bits */
    canonical(c->len, n, c->code);
}
static void l_put_code(obits *o, const lcode *c) {
    if (c->used <= 2) {   /* a simple code: one or two symbols, the first in a 1-bit field when that is enough */
        const int two = c->used == 2, wide = c->s0 > 1, w0 = wide ? 8 : 1;
        put(o, 1, 1); put(o, (uint32_t)two, 1); put(o, (uint32_t)wide, 1); put(o, (uint32_t)c->s0, w0);
        if (two) put(o, (uint32_t)c->s1, 8);
        return;
    }
    /* a normal code the long way: the code-length code gives the sixteen lengths 0..15 four bits each (so length v is the 4-bit code v, written
       MSB first as prefix codes are) and the run-length symbols 16, 17, 18 none; the lengths are cut behind the last symbol in use */
    static const int kOrder[19] = {17, 18, 0, 1, 2, 3, 4, 5, 16, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15};   /* the format's order of the code-length code lengths */
    put(o, 0, 1);
    put(o, 15, 4);                              /* 4 + 15 = 19 code-length code lengths follow */
    for (int i = 0; i < 19; i++) put(o, kOrder[i] <= 15 ? 4u : 0u, 3);
    const int n = c->last + 1;
    put(o, 1, 1);                               /* max_symbol is given: */
    put(o, 4, 3);                               /*   in a field of 2 + 2 * 4 = 10 bits */
    put(o, (uint32_t)(n - 2), 10);
    for (int i = 0; i < n; i++) { const int v = c->len[i]; put(o, (uint32_t)(((v & 1) << 3) | ((v & 2) << 1) | ((v & 4) >> 1) | ((v & 8) >> 3)), 4); }
}
static void l_put_single(obits *o) { put(o, 1, 1); put(o, 0, 1); put(o, 0, 1); put(o, 0, 1); }   /* simple code, one symbol, 1-bit field, symbol 0 */
int cso_vp8l_encode(const uint8_t *px, int width, int height, int channels, uint8_t **out, size_t *out_len) {
    if (width < 1 || height < 1 || width > 16384 || height > 16384 || channels < 1 || channels > 4) return CSO_PNG_UNSUPPORTED;
    const int bw = (width + 15) / 16, bh = (height + 15) / 16;
    uint8_t *modes = (uint8_t *)malloc((size_t)bw * (size_t)bh);
    uint32_t *res = (uint32_t *)malloc(sizeof(uint32_t) * (size_t)width * (size_t)height);
    for (int by = 0; by < bh; by++)
        for (int bx = 0; bx < bw; bx++) {
            uint64_t cost[14] = {0};
            for (int y = by * 16; y < by * 16 + 16 && y < height; y++)
                for (int x = bx * 16; x < bx * 16 + 16 && x < width; x++) {
                    if (!x || !y) continue;   /* the frame's first row and column are predicted the same way whatever the mode */
                    const uint32_t me = l_sg(px, width, channels, x, y);
                    for (int m = 0; m < 14; m++) {
                        const uint32_t r = l_sub(me, l_pred_at(px, width, channels, x, y, m));
                        for (int s = 0; s < 32; s += 8) { const uint32_t v = (r >> s) & 255u; cost[m] += v < 128u ? v : 256u - v; }
                    }
                }
            int best = 0;
            for (int m = 1; m < 14; m++) if (cost[m] < cost[best]) best = m;
            modes[by * bw + bx] = (uint8_t)best;
        }
    uint32_t hist[4][288]; uint32_t mh[288];
    memset(hist, 0, sizeof hist); memset(mh, 0, sizeof mh);
    for (int y = 0; y < height; y++)
        for (int x = 0; x < width; x++) {
            const uint32_t v = l_sub(l_sg(px, width, channels, x, y), l_pred_at(px, width, channels, x, y, modes[(y / 16) * bw + x / 16]));
            res[(size_t)y * (size_t)width + (size_t)x] = v;
            hist[0][(v >> 8) & 255u]++; hist[1][(v >> 16) & 255u]++; hist[2][v & 255u]++; hist[3][v >> 24]++;
        }
    for (int b = 0; b < bw * bh; b++) mh[modes[b]]++;
    lcode cg, cr, cb, ca, cm;
    l_make_code(&cg, hist[0], 280); l_make_code(&cr, hist[1], 256); l_make_code(&cb, hist[2], 256); l_make_code(&ca, hist[3], 256); l_make_code(&cm, mh, 280);
    obits o; memset(&o, 0, sizeof o);
    put(&o, 0x2F, 8);
    put(&o, (uint32_t)(width - 1), 14); put(&o, (uint32_t)(height - 1), 14); put(&o, (channels == 2 || channels == 4) ? 1u : 0u, 1); put(&o, 0, 3);
    put(&o, 1, 1); put(&o, 2, 2);                    /* a transform: subtract green */
    put(&o, 1, 1); put(&o, 0, 2); put(&o, 2, 3);     /* a transform: predictor, blocks of 1 << (2 + 2) pixels */
    put(&o, 0, 1);                                   /* its mode image (a sub-resolution image: no meta prefix bit): no colour cache */
    l_put_code(&o, &cm); l_put_single(&o); l_put_single(&o); l_put_single(&o); l_put_single(&o);   /* the mode sits in the green channel */
    for (int b = 0; b < bw * bh; b++) put(&o, cm.code[modes[b]], cm.len[modes[b]]);
    put(&o, 0, 1);                                   /* no further transform */
    put(&o, 0, 1);                                   /* the picture: no colour cache */
    put(&o, 0, 1);                                   /* no meta prefix image */
    l_put_code(&o, &cg); l_put_code(&o, &cr); l_put_code(&o, &cb); l_put_code(&o, &ca); l_put_single(&o);   /* green, red, blue, alpha, distance */
    for (size_t i = 0; i < (size_t)width * (size_t)height; i++) {
        const uint32_t v = res[i], g = (v >> 8) & 255u, r = (v >> 16) & 255u, b = v & 255u, a = v >> 24;
        put(&o, cg.code[g], cg.len[g]); put(&o, cr.code[r], cr.len[r]); put(&o, cb.code[b], cb.len[b]); put(&o, ca.code[a], ca.len[a]);
    }
    align(&o);
    const size_t payload = o.n, padded = payload + (payload & 1u), total = 20 + padded;
    uint8_t *f = (uint8_t *)calloc(total, 1);
    memcpy(f, "RIFF", 4); f[4] = (uint8_t)(total - 8); f[5] = (uint8_t)((total - 8) >> 8); f[6] = (uint8_t)((total - 8) >> 16); f[7] = (uint8_t)((total - 8) >> 24);
    memcpy(f + 8, "WEBPVP8L", 8); f[16] = (uint8_t)payload; f[17] = (uint8_t)(payload >> 8); f[18] = (uint8_t)(payload >> 16); f[19] = (uint8_t)(payload >> 24);
    memcpy(f + 20, o.p, payload);
    free(o.p); free(modes); free(res);
    *out = f; *out_len = total;
    return 0;
}
