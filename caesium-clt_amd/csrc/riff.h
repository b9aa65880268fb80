// riff.h -- the RIFF / WEBP container as the host sources read and write it: little-endian fields, the chunk walk, the metadata chunks, VP8X (host only)
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

namespace riff {

inline uint32_t rd24(const uint8_t *d) { return uint32_t(d[0]) | (uint32_t(d[1]) << 8) | (uint32_t(d[2]) << 16); }
inline uint32_t rd32(const uint8_t *d) { return rd24(d) | (uint32_t(d[3]) << 24); }
inline void wr24(uint8_t *q, uint32_t v) { q[0] = uint8_t(v); q[1] = uint8_t(v >> 8); q[2] = uint8_t(v >> 16); }
inline void wr32(uint8_t *q, uint32_t v) { wr24(q, v); q[3] = uint8_t(v >> 24); }

// where the chunks of a file of n bytes end: what the RIFF header says, or the file's end (libwebp tolerates a RIFF size past it as long as the chunks are there)
inline size_t declared_end(const uint8_t *d, size_t n) { const size_t end = size_t(rd32(d + 4)) + 8; return end > n ? n : end; }

// The chunks between `start` and `end` of d[0, n): for (Chunks c(d, n, end); c.next();) -- c.at is the chunk header's offset, c.len the payload's length as the
// header states it.  A chunk whose payload runs past n is still handed out, with c.truncated set, and is the last one.
struct Chunks {
    const uint8_t *d;
    size_t n, end, nxt, at = 0, len = 0;
    bool truncated = false;
    Chunks(const uint8_t *d_, size_t n_, size_t end_, size_t start = 12) : d(d_), n(n_), end(end_), nxt(start) {}
    bool next() {
        if (nxt + 8 > end) return false;
        at = nxt; len = rd32(d + at + 4);
        truncated = at + 8 + len > n;
        nxt = at + 8 + len + (len & 1);
        return true;
    }
    bool is(const char *id) const { return !memcmp(d + at, id, 4); }
    const uint8_t *payload() const { return d + at + 8; }
};

// the first ICCP and the first EXIF chunk of a file (what img-parts reads for libcaesium's keep_metadata; XMP is not carried)
struct Metadata {
    const uint8_t *icc = nullptr, *exif = nullptr;
    size_t icc_len = 0, exif_len = 0;
    bool any() const { return icc || exif; }
    uint8_t vp8x_flags() const { return uint8_t((icc ? 0x20 : 0) | (exif ? 0x08 : 0)); }
    size_t bytes() const { return (icc ? 8 + icc_len + (icc_len & 1) : 0) + (exif ? 8 + exif_len + (exif_len & 1) : 0); }   // as chunks, padded
};
inline Metadata find_metadata(const uint8_t *d, size_t n) {
    Metadata m;
    for (Chunks c(d, n, n); c.next() && !c.truncated;) {
        if (c.is("ICCP") && !m.icc) { m.icc = c.payload(); m.icc_len = c.len; }
        if (c.is("EXIF") && !m.exif) { m.exif = c.payload(); m.exif_len = c.len; }
    }
    return m;
}

// the writers return the byte behind what they wrote
inline uint8_t *write_header(uint8_t *dst, size_t total) { memcpy(dst, "RIFF", 4); wr32(dst + 4, uint32_t(total - 8)); memcpy(dst + 8, "WEBP", 4); return dst + 12; }
inline uint8_t *write_vp8x(uint8_t *dst, uint8_t flags, uint32_t canvas_w, uint32_t canvas_h) {
    memcpy(dst, "VP8X", 4); wr32(dst + 4, 10);
    dst[8] = flags; dst[9] = dst[10] = dst[11] = 0;
    wr24(dst + 12, canvas_w - 1); wr24(dst + 15, canvas_h - 1);
    return dst + 18;
}
inline uint8_t *append_chunk(uint8_t *dst, const char *id, const uint8_t *payload, size_t len) {   // pads to even
    memcpy(dst, id, 4); wr32(dst + 4, uint32_t(len)); memcpy(dst + 8, payload, len);
    dst += 8 + len;
    if (len & 1) *dst++ = 0;
    return dst;
}

}  // namespace riff
