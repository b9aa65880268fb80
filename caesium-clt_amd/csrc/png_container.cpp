// png_container.cpp -- the PNG container on the host: the chunk walk and the carried-chunk policy of the lossless PNG row (what oxipng's
// decode does in front of the pixels), the chunks the host writes itself, and oxipng's filter presets.  No device work here.
// Statement of every stage: oracle/png_oracle.c.
#include <cstring>

#include "png_batch.hpp"

namespace csp {
namespace {

void put_be32(uint8_t *p, uint32_t v) { p[0] = uint8_t(v >> 24); p[1] = uint8_t(v >> 16); p[2] = uint8_t(v >> 8); p[3] = uint8_t(v); }
uint32_t crc32_host(const uint8_t *p, size_t n) {
    struct Table {   // built once, thread-safe (the boundary is called from several host threads)
        uint32_t t[256];
        Table() { for (uint32_t i = 0; i < 256; i++) { uint32_t c = i; for (int k = 0; k < 8; k++) c = (c & 1) ? 0xEDB88320u ^ (c >> 1) : c >> 1; t[i] = c; } }
    };
    static const Table table;
    uint32_t crc = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; i++) crc = table.t[(crc ^ p[i]) & 255] ^ (crc >> 8);
    return ~crc;
}
const uint8_t kSig[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1A, '\n'};
// a prefix starts with the signature and the IHDR chunk: its type at 12, its 13 payload bytes at 16 (depth at +8, colour type at +9, interlace
// method at +12), its CRC at 29
enum { IHDR_TYPE = 12, IHDR_DATA = 16, IHDR_CRC = 29 };

// oxipng StripChunks::Safe keeps these ancillary chunks [UPSTREAM-RECALL]; tRNS is image data
bool kept_when_stripping(const uint8_t *type) {
    static const char *keep[] = {"cICP", "iCCP", "sRGB", "pHYs", "tRNS"};
    for (const char *k : keep) if (!memcmp(type, k, 4)) return true;
    return false;
}

}  // namespace

uint32_t be32(const uint8_t *p) { return (uint32_t(p[0]) << 24) | (uint32_t(p[1]) << 16) | (uint32_t(p[2]) << 8) | p[3]; }

void append_chunk(std::vector<uint8_t> &dst, const char type[4], const uint8_t *data, uint32_t len) {
    const size_t at = dst.size();
    dst.resize(at + 12 + len);
    put_be32(&dst[at], len); memcpy(&dst[at + 4], type, 4); if (len) memcpy(&dst[at + 8], data, len);
    put_be32(&dst[at + 8 + len], crc32_host(&dst[at + 4], 4 + len));
}

void set_ihdr_format(std::vector<uint8_t> &prefix, uint32_t depth, uint32_t ctype) {
    prefix[IHDR_DATA + 8] = uint8_t(depth); prefix[IHDR_DATA + 9] = uint8_t(ctype);
    put_be32(&prefix[IHDR_CRC], crc32_host(&prefix[IHDR_TYPE], 17));
}

uint32_t palette_depth(uint32_t n) { return n <= 2 ? 1u : n <= 4 ? 2u : n <= 16 ? 4u : 8u; }

uint32_t leading_transparent(const std::vector<uint32_t> &pal) {
    uint32_t ntr = 0;
    for (uint32_t k = 0; k < uint32_t(pal.size()); k++) if ((pal[k] >> 24) != 255) ntr = k + 1;
    return ntr;
}

// the IHDR of a file: geometry and format checks, and the output's IHDR (never interlaced) as the start of the prefix
static void parse_ihdr(const uint8_t *chunk, PngItem &it) {
    auto fail = [&](int code, const char *msg) { it.code = code; it.msg = msg; };
    const uint8_t *d = chunk + 8;
    if (crc32_host(chunk + 4, 17) != be32(d + 13)) return fail(CS_ERR_BAD_PNG, "IHDR checksum");
    const int depth = d[8], ctype = d[9];
    it.width = be32(d); it.height = be32(d + 4);
    if (!it.width || !it.height || it.width > 0x7FFFFFFFu || it.height > 0x7FFFFFFFu || d[10] || d[11] || d[12] > 1) return fail(CS_ERR_BAD_PNG, "bad IHDR");
    static const int chans[7] = {1, 0, 3, 1, 2, 0, 4};
    bool ok = false;
    switch (ctype) {
    case 0: ok = depth == 1 || depth == 2 || depth == 4 || depth == 8 || depth == 16; break;
    case 3: ok = depth == 1 || depth == 2 || depth == 4 || depth == 8; break;
    case 2: case 4: case 6: ok = depth == 8 || depth == 16; break;
    }
    if (!ok) return fail(CS_ERR_BAD_PNG, "bad colour type / bit depth");
    it.interlace = d[12] != 0;
    const uint64_t bits = uint64_t(chans[ctype]) * uint64_t(depth);
    it.bpp = bits >= 8 ? uint32_t(bits / 8) : 1u;
    it.channels = uint32_t(chans[ctype]); it.depth = uint32_t(depth); it.ctype = uint32_t(ctype);
    const uint64_t rb = (uint64_t(it.width) * bits + 7) / 8;
    if (rb > 0x7FFFFFF0u) return fail(CS_ERR_UNSUPPORTED, "PNG row too long");
    it.rowbytes = uint32_t(rb);
    it.prefix.assign(kSig, kSig + 8);
    it.prefix.insert(it.prefix.end(), chunk, chunk + 25);
    it.prefix[IHDR_DATA + 12] = 0;   // interlace method of the output
    set_ihdr_format(it.prefix, it.depth, it.ctype);
}

// the chunk walk (oracle: cso_png_decode, first half)
void parse_png(const uint8_t *in, size_t n, bool keep_metadata, PngItem &it) {
    auto fail = [&](int code, const char *msg) { it.code = code; it.msg = msg; };
    it.file_size = n;
    if (n < 8 + 25 || memcmp(in, kSig, 8)) return fail(CS_ERR_BAD_PNG, "not a PNG");
    size_t pos = 8;
    bool seen_ihdr = false, seen_idat = false, seen_iend = false;
    int nplte = 0;
    while (pos + 12 <= n && !seen_iend) {
        const uint32_t len = be32(in + pos);
        const uint8_t *type = in + pos + 4, *d = in + pos + 8;
        if (len > 0x7FFFFFFFu || pos + 12 + size_t(len) > n) return fail(CS_ERR_BAD_PNG, "truncated PNG chunk");
        if (!seen_ihdr) {
            if (memcmp(type, "IHDR", 4) || len != 13) return fail(CS_ERR_BAD_PNG, "PNG does not start with IHDR");
            parse_ihdr(in + pos, it);
            if (it.code) return;
            seen_ihdr = true;
        } else if (!memcmp(type, "IDAT", 4)) {
            it.idat.emplace_back(pos + 8, size_t(len)); it.idat_len += len; seen_idat = true;
        } else if (!memcmp(type, "IEND", 4)) {
            seen_iend = true;
        } else {
            if (!memcmp(type, "acTL", 4)) return fail(CS_ERR_UNSUPPORTED, "animated PNG has no device path in this build");
            if (!memcmp(type, "PLTE", 4)) { if (len % 3 || len > 768) return fail(CS_ERR_BAD_PNG, "bad PLTE"); nplte = int(len / 3); it.has_plte = true; it.plte.assign(d, d + len); }
            if (!memcmp(type, "tRNS", 4)) { it.has_trns = true; it.trns.assign(d, d + len); }
            const bool critical = !(type[0] & 0x20);
            if (critical || keep_metadata || kept_when_stripping(type)) {
                if (!memcmp(type, "tRNS", 4) || !memcmp(type, "bKGD", 4) || !memcmp(type, "sBIT", 4)) it.no_reduce = true;
                if (!memcmp(type, "bKGD", 4) || !memcmp(type, "sBIT", 4) || !memcmp(type, "hIST", 4)) it.pal_tied = true;
                std::vector<uint8_t> &dst = seen_idat ? it.suffix : it.prefix;
                dst.insert(dst.end(), in + pos, in + pos + 12 + size_t(len));
            }
        }
        pos += 12 + size_t(len);
    }
    if (!seen_ihdr || !seen_idat || !seen_iend) return fail(CS_ERR_BAD_PNG, "PNG without IHDR / IDAT / IEND");
    if (it.ctype == 3 && !nplte) return fail(CS_ERR_BAD_PNG, "palette PNG without PLTE");
    append_chunk(it.suffix, "IEND", nullptr, 0);
    // the two zlib header bytes (oracle: cso_inflate_zlib)
    uint8_t z[2]; size_t got = 0;
    for (auto &r : it.idat) for (size_t k = 0; k < r.second && got < 2; k++) z[got++] = in[r.first + k];
    if (got < 2 || (z[0] & 15) != 8 || (z[0] >> 4) > 7 || ((unsigned(z[0]) << 8) | z[1]) % 31 || (z[1] & 0x20)) return fail(CS_ERR_BAD_PNG, "bad zlib header in IDAT");
    if (it.idat_len > 0xFFFFFFF0u) return fail(CS_ERR_UNSUPPORTED, "IDAT stream too long");
}

// a source that is pixels already (csp_batch_create_pixels): the item a PNG file of that image would parse to
void pixels_item(const csp_pixels &src, uint32_t bits, PngItem &it) {
    const uint32_t bps = bits / 8;
    static const uint8_t ctype_of[5] = {0, 0, 4, 2, 6};
    if (!src.device_pixels || !src.width || !src.height || src.channels < 1 || src.channels > 4 || src.width > 0x7FFFFFFFu || src.height > 0x7FFFFFFFu ||
        uint64_t(src.width) * src.channels * bps > 0x7FFFFFF0u) { it.code = CS_ERR_UNSUPPORTED; it.msg = "bad pixel source"; return; }
    it.width = src.width; it.height = src.height; it.depth = bits; it.ctype = ctype_of[src.channels]; it.channels = src.channels; it.bpp = src.channels * bps;
    it.rowbytes = src.width * src.channels * bps;
    uint8_t ihdr[13] = {};   // compression, filter and interlace method 0
    put_be32(ihdr, src.width); put_be32(ihdr + 4, src.height); ihdr[8] = uint8_t(bits); ihdr[9] = ctype_of[src.channels];
    it.prefix.assign(kSig, kSig + 8);
    append_chunk(it.prefix, "IHDR", ihdr, 13);
    it.suffix.clear();
    append_chunk(it.suffix, "IEND", nullptr, 0);
}

// oxipng's presets [UPSTREAM-RECALL]: filters tried per --png-opt-level (oracle: cso_png_trials)
int trial_set(int level, int *set) {
    static const int s01[] = {5}, s2[] = {0, 1, 6, 7}, s34[] = {0, 7, 8, 9}, s5[] = {0, 1, 2, 5, 6, 7, 8, 9}, s6[] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9};
    const int *s; int n;
    if (level <= 1) { s = s01; n = 1; } else if (level == 2) { s = s2; n = 4; } else if (level <= 4) { s = s34; n = 4; } else if (level == 5) { s = s5; n = 8; } else { s = s6; n = 10; }
    memcpy(set, s, sizeof(int) * size_t(n));
    return n;
}

}  // namespace csp
