// route_webp.cpp -- WebP inputs (libcaesium: libwebp decodes, then webp::compress / convert_in_memory, compressor.rs:289-305): the device decodes the
// key frame (cswd_batch), the RGB stays in HBM and goes to the encoder of the target: the WebP encoder at webp.quality (`compress`
// on a WebP file), the JPEG or the PNG row (conversions).  A size, if given, is applied by the JPEG row's Lanczos branch on the way.
// webp_inputs at the bottom reads top to bottom: group, decode, collect_pictures, encode_stills (one of to_png / to_lossless_webp / to_lossy_webp / to_jpeg), the animated files.
#include "riff.h"
#include "routes.hpp"

namespace route {
namespace {

// the device batches of one step, released together when the step is over
struct Handles {
    cswd_batch *wb = nullptr;
    csh_batch *jb = nullptr, *rb = nullptr, *rb2 = nullptr;
    csp_batch *pb = nullptr;
    std::vector<cswd_rgba *> joined;
    ~Handles() { csp_batch_destroy(pb); csh_batch_destroy(jb); csh_batch_destroy(rb); csh_batch_destroy(rb2); for (cswd_rgba *jn : joined) cswd_rgba_destroy(jn); cswd_batch_destroy(wb); }
};

// the decoded files of one group
struct Pictures {
    std::vector<csp_pixels> px;            // per still picture: what the target's coder takes (RGB; RGBA for a picture with transparency towards PNG / lossless WebP)
    std::vector<const uint8_t *> aplane;   // its alpha plane in device memory where it becomes an ALPH chunk (lossy WebP), or null
    std::vector<csp_pixels> rgb3;          // its RGB whatever its transparency ...
    std::vector<const uint8_t *> rplane;   // ... and the plane of a picture the RGBA consumers get: what a resize works on
    std::vector<size_t> at;                // its place in the call
    std::vector<size_t> anim_at;           // the animated files of the group (indices into it)
};

// groups by what the decoder reserves, not by file bytes: per declared pixel 3 B of RGB, 5 B of alpha room and 8 B of VP8L work area
// (+ 4 MiB + 16 x the file), so ~20 B per pixel of the canvas the header declares -- a tiny file may declare 16383 x 16383.  A group
// that still fails for want of memory is halved and tried again (as the JPEG row does), so that one oversized header fails alone.
// An animated file counts every frame (webp_declared_pixels): its frames are pictures of the batch, coded again by cswd_batch_encode_anim -- for target
// WebP without a size; an animation whose frames alone exceed the cap is refused before anything is reserved for it.
const uint64_t POOL_CAP = uint64_t(64) << 30;
uint64_t pool_estimate(const CByteArray &in) { return webp_declared_pixels(in.data, in.length) * 20 + 16 * uint64_t(in.length) + (uint64_t(4) << 20); }
bool animated(const CByteArray &in) { return in.length >= 30 && !memcmp(in.data, "RIFF", 4) && !memcmp(in.data + 8, "WEBPVP8X", 8) && (in.data[20] & 0x02); }

// What the decode left of the files [g0, g0 + n): an animated file goes to pic.anim_at where there is a path for it (WebP output at the canvas' size), a still
// picture into pic, a file that failed gets its result.  Returns the failures.
int collect_pictures(cswd_batch *wb, size_t g0, size_t n, const CCSParameters *p, uint32_t target, Pictures &pic, CCSResult *results) {
    int failed = 0;
    for (size_t k = 0; k < n; k++) {
        uint32_t nframes = 0, cw = 0, ch = 0;
        if (!cswd_batch_frames(wb, k, &nframes, &cw, &ch) && nframes) {
            const char *why = target != CS_TYPE_WEBP ? "an animated WebP file converts to no JPEG / PNG in this build (it is compressed as animated WebP)"
                              : (p->width || p->height) ? "resizing an animated WebP file has no path in this build" : nullptr;
            if (!why) pic.anim_at.push_back(k);
            else { results[g0 + k] = make_result(CS_ERR_UNSUPPORTED, why); failed++; }
            continue;
        }
        csp_pixels s; const char *msg = "";
        const int code = cswd_batch_pixels(wb, k, &s.device_pixels, &s.width, &s.height, &s.channels, &msg);
        if (code) { results[g0 + k] = make_result(code, msg); failed++; continue; }
        const uint8_t *rgba = nullptr, *plane = nullptr;
        cswd_batch_alpha(wb, k, &rgba, &plane);
        // a picture with transparency: the PNG coder and the lossless WebP coder take its RGBA; the lossy WebP encoder its RGB, the plane becomes the
        // ALPH chunk afterwards; a JPEG drops the plane (as image-rs does)
        const bool wants_rgba = plane && (target == CS_TYPE_PNG || (target == CS_TYPE_WEBP && p->webp_lossless));
        pic.rgb3.push_back(s); pic.rplane.push_back(wants_rgba ? plane : nullptr);
        if (wants_rgba) { s.device_pixels = rgba; s.channels = 4; }
        pic.px.push_back(s); pic.aplane.push_back((plane && target == CS_TYPE_WEBP && !p->webp_lossless) ? plane : nullptr); pic.at.push_back(g0 + k);
    }
    return failed;
}

// pictures through the JPEG row's Lanczos branch, stopped behind its RGB: px[k] is replaced by picture k at the size asked for (in device memory that b owns)
int resize_batch(std::vector<csp_pixels> &px, const std::vector<csp_pixels> &from, const CCSParameters *p, int device, csh_batch *&b) {
    int r = csh_batch_create_from_pixels_rgb(from.data(), from.size(), p, device, &b);
    if (r == 0) r = csh_batch_run(b, nullptr);
    for (size_t k = 0; k < from.size() && r == 0; k++) { const char *m = ""; if (csh_batch_pixels(b, k, &px[k].device_pixels, &px[k].width, &px[k].height, &px[k].channels, &m)) r = CS_ERR_NO_DEVICE; }
    return r;
}

// the pictures at the size asked for, for the PNG / lossless WebP coders: every picture's RGB through the Lanczos branch, the alpha planes of the
// pictures with transparency through it as grey pictures (image-rs resamples the four channels alike), and the two halves joined again
int resize_pictures(const Pictures &pic, const CCSParameters *p, int device, Handles &h, std::vector<csp_pixels> &src) {
    int r = resize_batch(src, pic.rgb3, p, device, h.rb);
    std::vector<csp_pixels> planes;
    std::vector<size_t> whose;
    for (size_t k = 0; k < pic.rgb3.size(); k++) if (pic.rplane[k]) { planes.push_back(csp_pixels{pic.rplane[k], pic.rgb3[k].width, pic.rgb3[k].height, 1}); whose.push_back(k); }
    if (r || planes.empty()) return r;
    const std::vector<csp_pixels> full = planes;
    r = resize_batch(planes, full, p, device, h.rb2);
    for (size_t j = 0; j < planes.size() && r == 0; j++) {
        const csp_pixels &a = planes[j];
        csp_pixels &c = src[whose[j]];
        if (a.width != c.width || a.height != c.height || a.channels != 1 || c.channels != 3) return CS_ERR_NO_DEVICE;
        cswd_rgba *jn = nullptr;
        if (cswd_rgba_join(c.device_pixels, a.device_pixels, c.width, c.height, device, &jn, &c.device_pixels)) return CS_ERR_NO_DEVICE;
        h.joined.push_back(jn); c.channels = 4;
    }
    return r;
}

// One function per target.  Each codes pic.px into out / res, sets failed to the files that failed (below 0: the fetch itself failed) and returns 0 or the
// code that fails every picture; the batches it made stay in h.
int to_png(const Pictures &pic, const CCSParameters *p, int device, Handles &h, CByteArray *out, CCSResult *res, int &failed) {
    std::vector<csp_pixels> src = pic.px;
    int rc = (p->width || p->height) ? resize_pictures(pic, p, device, h, src) : 0;
    if (rc == 0) rc = csp_batch_create_pixels(src.data(), src.size(), p, device, &h.pb);
    if (rc == 0) rc = csp_batch_run(h.pb, nullptr);
    if (rc == 0) failed = csp_batch_fetch(h.pb, out, res);
    return rc;
}
int to_lossless_webp(const Pictures &pic, const CCSParameters *p, int device, Handles &h, CByteArray *out, CCSResult *res, int &failed) {   // webp.lossless: the VP8L coder
    std::vector<csp_pixels> src = pic.px;
    const int rc = (p->width || p->height) ? resize_pictures(pic, p, device, h, src) : 0;
    if (rc == 0) failed = csl_encode_pixels(src.data(), src.size(), device, out, res);
    return rc;
}
int to_jpeg(const Pictures &pic, const CCSParameters *p, int device, Handles &h, CByteArray *out, CCSResult *res, int &failed) {   // the size is the JPEG row's own business
    int rc = csh_batch_create_from_pixels(pic.px.data(), pic.px.size(), p, device, &h.jb);
    if (rc == 0) rc = csh_batch_run(h.jb, nullptr);
    if (rc == 0) failed = csh_batch_fetch(h.jb, out, res);
    return rc;
}
int to_lossy_webp(const Pictures &pic, const CCSParameters *p, int device, Handles &h, CByteArray *out, CCSResult *res, int &failed) {
    int rc = csh_batch_create_webp_from_pixels(pic.px.data(), pic.px.size(), p, device, &h.jb);
    if (rc == 0) rc = csh_batch_run(h.jb, nullptr);
    if (rc == 0) failed = csh_batch_fetch(h.jb, out, res);
    if (rc || failed < 0) return rc;
    // the alpha planes of the pictures that have one: through the same Lanczos branch as the colour, as grey pictures (image-rs resamples the four channels
    // alike), then the VP8L coder over each plane and VP8X + ALPH + VP8
    std::vector<csp_pixels> apx;
    std::vector<size_t> aat;
    for (size_t k = 0; k < pic.px.size(); k++)
        if (pic.aplane[k] && out[k].data) { apx.push_back(csp_pixels{pic.aplane[k], pic.px[k].width, pic.px[k].height, 1}); aat.push_back(k); }
    if (apx.empty()) return 0;
    if (p->width || p->height) { const std::vector<csp_pixels> full = apx; rc = resize_batch(apx, full, p, device, h.rb); }
    if (rc == 0) failed += attach_alpha_planes(apx, aat, out, res, device);
    return rc;
}

// keep_metadata on WebP -> WebP (libcaesium's webp::compress: ICC profile and EXIF of the SOURCE read with img-parts and set on the encoded
// file, which turns it into the extended format): RIFF { VP8X(flags, canvas), ICCP?, VP8, EXIF? }.  XMP is not carried (img-parts' API
// sets profile and EXIF only).  The chunk walk is the container's: host work, like the JPEG row's marker copy.
void carry_metadata(const CByteArray &src, CByteArray &out) {
    const bool extended = out.data && out.length >= 38 && !memcmp(out.data + 12, "VP8X", 4);   // made here: VP8X, ALPH, VP8 (a picture with transparency)
    const bool lossless = out.data && out.length >= 26 && !memcmp(out.data + 12, "VP8L", 4) && out.data[20] == 0x2F;   // webp.lossless: a bare VP8L stream
    if (src.length < 20 || !out.data || out.length < 26 || (memcmp(out.data + 12, "VP8 ", 4) && !extended && !lossless)) return;
    const riff::Metadata md = riff::find_metadata(src.data, src.length);
    if (!md.any()) return;
    const uint8_t *f = out.data + 20;   // VP8 frame header: tag (3), start code (3), 14-bit width and height -- or the VP8X chunk's flags and canvas size
    // a VP8L stream says its size (14 + 14 bits, each minus one) and whether its alpha is in use right behind the signature byte
    const uint32_t lbits = lossless ? riff::rd32(f + 1) : 0u;
    const uint32_t w = lossless ? (lbits & 0x3FFFu) + 1 : extended ? riff::rd24(f + 4) + 1 : (uint32_t(f[6]) | (uint32_t(f[7]) << 8)) & 0x3FFFu;
    const uint32_t h = lossless ? ((lbits >> 14) & 0x3FFFu) + 1 : extended ? riff::rd24(f + 7) + 1 : (uint32_t(f[8]) | (uint32_t(f[9]) << 8)) & 0x3FFFu;
    const uint8_t flags0 = lossless ? uint8_t(((lbits >> 28) & 1u) ? 0x10 : 0) : extended ? f[0] : 0;   // VP8X alpha flag from the stream's alpha_is_used bit
    const size_t body0 = extended ? 30 : 12, body = out.length - body0;   // the chunks behind the file header (and behind VP8X), with their padding
    const size_t total = 12 + 18 + md.bytes() + body;
    uint8_t *o = static_cast<uint8_t *>(malloc(total));
    if (!o) return;
    uint8_t *q = riff::write_vp8x(riff::write_header(o, total), uint8_t(flags0 | md.vp8x_flags()), w, h);
    if (md.icc) q = riff::append_chunk(q, "ICCP", md.icc, md.icc_len);
    memcpy(q, out.data + body0, body); q += body;
    if (md.exif) riff::append_chunk(q, "EXIF", md.exif, md.exif_len);
    free(out.data);
    out.data = o; out.length = total;
}

// the still pictures of a group through the target's coder, and what comes out into their places
int encode_stills(const CByteArray *inputs, const Pictures &pic, const CCSParameters *p, uint32_t target, int device, CByteArray *outputs, CCSResult *results) {
    const size_t m = pic.px.size();
    if (!m) return 0;
    std::vector<CByteArray> out(m);
    std::vector<CCSResult> res(m);
    Handles h;
    int failed = -1;
    const auto coder = target == CS_TYPE_PNG ? to_png : target != CS_TYPE_WEBP ? to_jpeg : p->webp_lossless ? to_lossless_webp : to_lossy_webp;
    const int rc = coder(pic, p, device, h, out.data(), res.data(), failed);
    if (rc || failed < 0) {
        for (size_t k = 0; k < m; k++) { cs_free_bytes(&out[k]); cs_free_result(&res[k]); results[pic.at[k]] = make_result(rc ? rc : CS_ERR_NO_DEVICE, csh_last_error()); }
        return int(m);
    }
    for (size_t k = 0; k < m; k++) {
        if (target == CS_TYPE_WEBP && p->keep_metadata && out[k].data) carry_metadata(inputs[pic.at[k]], out[k]);
        outputs[pic.at[k]] = out[k]; results[pic.at[k]] = res[k];
    }
    return failed;
}

}  // namespace

int webp_inputs(const CByteArray *inputs, size_t count, const CCSParameters *p, uint32_t target, int device, CByteArray *outputs, CCSResult *results) {
    int failed_total = 0;
    size_t limit = 512;
    for (size_t g0 = 0, n = 0; g0 < count; g0 += n) {
        n = group_extent(inputs + g0, count - g0, limit, uint64_t(256) << 20, POOL_CAP, pool_estimate);
        if (n == 1 && pool_estimate(inputs[g0]) > POOL_CAP && animated(inputs[g0])) {
            results[g0] = make_result(CS_ERR_UNSUPPORTED, "animated WebP: the frames of this file exceed the device pools of one batch");
            failed_total++;
            continue;
        }
        Handles decoded;
        int rc = cswd_batch_create(inputs + g0, n, device, &decoded.wb);
        if (rc == 0) rc = cswd_batch_run(decoded.wb);
        if (rc != 0 && n > 1 && (rc == CS_ERR_NO_DEVICE || rc == CS_ERR_POOL_OVERFLOW) && csh_device_count() > device) { limit = (n + 1) / 2; n = 0; continue; }   // same files again, in smaller groups
        limit = 512;
        if (rc) { for (size_t k = 0; k < n; k++) results[g0 + k] = make_result(rc, csh_last_error()); failed_total += int(n); continue; }
        Pictures pic;
        failed_total += collect_pictures(decoded.wb, g0, n, p, target, pic, results);
        failed_total += encode_stills(inputs, pic, p, target, device, outputs, results);
        // the animated files of the group (indices into it, so every array starts at the group): their frames are coded again, each file gets its result
        failed_total += cswd_batch_encode_anim(decoded.wb, inputs + g0, pic.anim_at.data(), pic.anim_at.size(), p, device, outputs + g0, results + g0);
    }
    return failed_total;
}

}  // namespace route
