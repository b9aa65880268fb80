// gif_container.cpp -- the GIF container on the host (GIF87a / GIF89a): the logical screen descriptor and the global colour table, graphic control extensions
// (delay, disposal, transparent index), image descriptors (rectangle, local table, interlace flag), the LZW minimum code size and the data sub-blocks -- joined
// per frame into one stream for upload --, the NETSCAPE2.0 loop extension, comment and other application extensions; and the same blocks written again around
// the frames the device coded.  A malformed file gets CS_ERR_BAD_GIF for itself alone.
#include <cstring>

#include "gif_batch.hpp"

static inline uint32_t rd16(const uint8_t *p) { return uint32_t(p[0]) | (uint32_t(p[1]) << 8); }
static inline void wr16(std::vector<uint8_t> &o, uint32_t v) { o.push_back(uint8_t(v)); o.push_back(uint8_t(v >> 8)); }

// the sub-blocks from i on, up to and with their terminator; false if the file ends first
static bool walk_sub_blocks(const uint8_t *d, size_t n, size_t &i, std::vector<uint8_t> *join) {
    for (;;) {
        if (i >= n) return false;
        const size_t len = d[i++];
        if (!len) return true;
        if (i + len > n) return false;
        if (join) join->insert(join->end(), d + i, d + i + len);
        i += len;
    }
}

int csg_parse(const uint8_t *d, size_t n, csg_file &f, std::string &msg) {
    auto bad = [&](const char *m) { msg = m; return int(CS_ERR_BAD_GIF); };
    if (n < 13 || (memcmp(d, "GIF87a", 6) && memcmp(d, "GIF89a", 6))) return bad("truncated GIF header");
    f.cw = rd16(d + 6); f.ch = rd16(d + 8);
    memcpy(f.lsd, d + 6, 7);
    size_t i = 13;
    if (f.lsd[4] & 0x80) {
        f.gct.off = i; f.gct.len = size_t(3) << ((f.lsd[4] & 7) + 1);
        if (i + f.gct.len > n) return bad("truncated global colour table");
        i += f.gct.len;
    }
    if (!f.cw || !f.ch) return bad("a GIF canvas without pixels");
    uint32_t disposal = 0, delay = 0;
    int transparent = -1;
    for (;;) {
        if (i >= n) return bad("no trailer before the end of the GIF file");
        const uint8_t b = d[i++];
        if (b == 0x3B) break;
        if (b == 0x21) {
            if (i >= n) return bad("truncated GIF extension block");
            const size_t start = i - 1;
            const uint8_t label = d[i++];
            if (label == 0xF9 && i + 5 <= n && d[i] == 4) {
                disposal = (d[i + 1] >> 2) & 7; delay = rd16(d + i + 2); transparent = (d[i + 1] & 1) ? int(d[i + 4]) : -1;
                if (disposal > 3) disposal = 0;   // reserved values: nothing is disposed of
                i += 5;
                if (!walk_sub_blocks(d, n, i, nullptr)) return bad("truncated graphic control extension");
                continue;
            }
            const size_t first = i;
            if (!walk_sub_blocks(d, n, i, nullptr)) return bad("truncated GIF extension block");
            if (label == 0x01) f.plain_text = true;
            else if (label == 0xFF && d[first] == 11 && !memcmp(d + first + 1, "NETSCAPE2.0", 11)) { if (!f.loop.len) { f.loop.off = start; f.loop.len = i - start; } }
            else if (label == 0xFF || label == 0xFE) f.meta.push_back(csg_range{start, i - start});
            continue;
        }
        if (b != 0x2C) return bad("a block that is neither an extension nor an image nor the trailer");
        if (i + 9 > n) return bad("truncated image descriptor");
        csg_frame_src s;
        s.x = rd16(d + i); s.y = rd16(d + i + 2); s.w = rd16(d + i + 4); s.h = rd16(d + i + 6);
        const uint8_t packed = d[i + 8];
        i += 9;
        s.interlaced = (packed & 0x40) != 0;
        if (packed & 0x80) {
            s.lct.off = i; s.lct.len = size_t(3) << ((packed & 7) + 1);
            if (i + s.lct.len > n) return bad("truncated local colour table");
            i += s.lct.len;
        }
        if (i >= n) return bad("truncated image data");
        s.mcs = d[i++];
        if (!walk_sub_blocks(d, n, i, &s.data)) return bad("truncated image data");
        if (!s.w || !s.h || s.x + s.w > f.cw || s.y + s.h > f.ch) return bad("a frame's rectangle is empty or leaves the canvas");
        if (s.mcs < 2 || s.mcs > 8) return bad("LZW minimum code size outside 2..8");   // (1 is refused: no decoder agrees with another on it)
        if (!s.lct.len && !f.gct.len) return bad("a frame without a colour table");
        s.disposal = disposal; s.delay = delay; s.transparent = transparent;
        disposal = delay = 0; transparent = -1;
        f.frames.push_back(std::move(s));
    }
    if (f.frames.empty()) return bad("a GIF file without a frame");
    return 0;
}

uint64_t csg_declared_pixels(const uint8_t *d, size_t n) {
    if (n < 13) return 0;
    const uint64_t canvas = uint64_t(rd16(d + 6)) * rd16(d + 8);
    uint64_t frames = 0;
    size_t i = 13 + ((d[10] & 0x80) ? (size_t(3) << ((d[10] & 7) + 1)) : 0);
    while (i < n && d[i] != 0x3B) {
        const uint8_t b = d[i++];
        if (b == 0x21) i++;
        else if (b == 0x2C) { if (i + 9 > n) break; i += 9 + ((d[i + 8] & 0x80) ? (size_t(3) << ((d[i + 8] & 7) + 1)) : 0) + 1; frames++; }
        else break;
        if (!walk_sub_blocks(d, n, i, nullptr)) break;
    }
    return canvas * (frames ? frames : 1);
}

void csg_write_file_head(const uint8_t *d, const csg_file &f, bool keep_metadata, std::vector<uint8_t> &out) {
    out.insert(out.end(), {'G', 'I', 'F', '8', '9', 'a'});
    out.insert(out.end(), f.lsd, f.lsd + 7);
    out.insert(out.end(), d + f.gct.off, d + f.gct.off + f.gct.len);
    out.insert(out.end(), d + f.loop.off, d + f.loop.off + f.loop.len);
    if (keep_metadata) for (const csg_range &r : f.meta) out.insert(out.end(), d + r.off, d + r.off + r.len);
}

void csg_write_frame_head(const uint8_t *d, const csg_frame_src &s, const csg::GifFrame &g, std::vector<uint8_t> &out) {
    out.insert(out.end(), {0x21, 0xF9, 0x04, uint8_t((g.odisposal << 2) | (s.transparent >= 0 ? 1 : 0))});
    wr16(out, s.delay);
    out.push_back(uint8_t(s.transparent >= 0 ? s.transparent : 0)); out.push_back(0);
    out.push_back(0x2C);
    wr16(out, g.ox); wr16(out, g.oy); wr16(out, g.ow); wr16(out, g.oh);
    uint8_t packed = 0;
    if (s.lct.len) { uint32_t bits = 0; while ((size_t(3) << (bits + 1)) < s.lct.len) bits++; packed = uint8_t(0x80 | bits); }
    out.push_back(packed);
    out.insert(out.end(), d + s.lct.off, d + s.lct.off + s.lct.len);
    out.push_back(uint8_t(g.omcs));
}
