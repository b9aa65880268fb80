// capi.cpp -- the libcaesium-shaped entry points on top of the device batch queue: what a call's files are, and which route (routes.hpp) takes them.
// Reference semantics: /root/reference/src/compressor.rs:287-306 (call shapes), :411-446 (parameters).
#include <algorithm>
#include <atomic>
#include <functional>
#include <thread>
#include <vector>

#include "riff.h"
#include "routes.hpp"

namespace route {
// declared pixel count of a JPEG / PNG / WebP (0 when the header does not say): what a file will occupy on the device is known before
// anything is decoded
// canvas of a WebP file from its first chunk: VP8X (24-bit width-1 / height-1), a bare VP8 key frame (14-bit sizes behind the start
// code) or a bare VP8L stream (14 + 14 bits behind the signature); 0 when the header does not say
uint64_t webp_declared_pixels(const uint8_t *d, size_t n) {
    if (n < 30 || memcmp(d, "RIFF", 4) || memcmp(d + 8, "WEBP", 4)) return 0;
    const uint8_t *f = d + 20;
    if (!memcmp(d + 12, "VP8X", 4)) {
        const uint64_t canvas = (uint64_t(riff::rd24(f + 4)) + 1) * (uint64_t(riff::rd24(f + 7)) + 1);
        if (!(f[0] & 0x02)) return canvas;
        // an animated file: every ANMF frame is a picture of its own on the device (its 24-bit width - 1 / height - 1 at bytes 6 and 9 of the chunk), so the frames
        // count, not the canvas
        uint64_t frames = 0;
        for (riff::Chunks c(d, n, n); c.next();)
            if (c.is("ANMF") && c.at + 8 + 16 <= n) frames += (uint64_t(riff::rd24(c.payload() + 6)) + 1) * (uint64_t(riff::rd24(c.payload() + 9)) + 1);
        return std::max(canvas, frames);
    }
    if (!memcmp(d + 12, "VP8 ", 4)) return (f[3] == 0x9D && f[4] == 0x01 && f[5] == 0x2A) ? uint64_t((f[6] | (f[7] << 8)) & 0x3FFF) * uint64_t((f[8] | (f[9] << 8)) & 0x3FFF) : 0;
    if (!memcmp(d + 12, "VP8L", 4) && f[0] == 0x2F) { const uint32_t b = riff::rd32(f + 1); return uint64_t((b & 0x3FFF) + 1) * uint64_t(((b >> 14) & 0x3FFF) + 1); }
    return 0;
}
}  // namespace route

static uint64_t declared_pixels(const uint8_t *d, size_t n) {
    if (n >= 30 && !memcmp(d, "RIFF", 4)) return route::webp_declared_pixels(d, n);
    if (n >= 24 && !memcmp(d, "\x89PNG\r\n\x1a\n", 8)) return route::png_declared_pixels(d);
    if (n >= 13 && !memcmp(d, "GIF8", 4)) return csg_declared_pixels(d, n);
    if (n < 4 || d[0] != 0xFF || d[1] != 0xD8) return 0;
    for (size_t i = 2; i + 4 <= n;) {
        if (d[i] != 0xFF) { i++; continue; }
        const int m = d[i + 1];
        if (m == 0xFF) { i++; continue; }
        if (m == 0xD8 || m == 0x01 || (m >= 0xD0 && m <= 0xD7)) { i += 2; continue; }
        const size_t L = (size_t(d[i + 2]) << 8) | d[i + 3];
        if (L < 2 || i + 2 + L > n) break;
        if (m >= 0xC0 && m <= 0xCF && m != 0xC4 && m != 0xC8 && m != 0xCC && L >= 7) return (uint64_t((d[i + 5] << 8) | d[i + 6])) * uint64_t((d[i + 7] << 8) | d[i + 8]);
        if (m == 0xDA) break;
        i += 2 + L;
    }
    return 0;
}

// GIF and TIFF files (libcaesium: gifski / the tiff crate; SURVEY.md 2 rows 9-10: outside the north-star's JPEG / PNG / WebP scope, "CPU
// passthrough") are passed through: the file comes back as it is, with Success -- as for a PNG that oxipng cannot make smaller.  A tree
// that holds such files (configs[4], /root/reference/src/compressor.rs:774 hands the engine a .tif) then completes without error lines; the
// caller's overwrite / min-savings policy sees equal sizes and acts on that.  A resize or a conversion of such a file is still refused.
// A GIF file leaves this path under CSH_GIF=device (read on every call; unset, empty or "pass": here as before): route::gif_compress optimises it, pixel-exact
// (DESIGN.md 8.3), and under CSH_GIF=lossy with the bounded-error coder at gif_quality; its resize is still answered here, and any other value of the variable
// fails the call's GIF files with CS_ERR_UNSUPPORTED.
// A TIFF file leaves it when CSH_TIFF is set (tiff_mode below; read on every call): route::tiff_compress decodes its strips and tiles and codes them again;
// its resize is still answered here.
static CCSResult passthrough(const CByteArray &in, const CCSParameters *p, CByteArray *out) {
    out->data = nullptr; out->length = 0;
    if (p->width || p->height) return make_result(CS_ERR_UNSUPPORTED, "resizing a GIF / TIFF file has no path in this build (the file itself is passed through without a size)");
    out->data = static_cast<uint8_t *>(malloc(in.length ? in.length : 1));
    if (!out->data) return make_result(CS_ERR_NO_DEVICE, "out of memory");
    memcpy(out->data, in.data, in.length); out->length = in.length;
    return make_result(0, nullptr);
}
static const char *const BAD_CSH_GIF = "CSH_GIF names no GIF path (unset, empty or \"pass\": the file is passed through; \"device\": the pixel-exact optimiser; \"lossy\": the same with the bounded-error coder at gif_quality)";
static const char *const BAD_CSH_TIFF = "CSH_TIFF names no TIFF path (unset, empty or \"pass\": the file is passed through; \"device\": re-coded with the compression tiff_compression names; \"lzw\", \"packbits\", \"none\": re-coded with that compression)";
static const char *const NO_TIFF_DEFLATE = "the TIFF route's Deflate coder is not built (tiff_compression 2 under CSH_TIFF=device): LZW (1), PackBits (3) and uncompressed output are";
// CSH_GIF: 0 pass the file through, 1 the device route, 2 the device route with the lossy coder at gif_quality, -1 a value that names none of them
static int gif_mode() {
    const char *e = getenv("CSH_GIF");
    if (!e || !*e || !strcmp(e, "pass")) return 0;
    return !strcmp(e, "device") ? 1 : !strcmp(e, "lossy") ? 2 : -1;
}
// CSH_TIFF: TIFF_PASS the file is passed through; a CST_OUT_* value: the device route with that output compression ("device": what tiff_compression names -- 1 LZW,
// 3 PackBits, 2 Deflate, which the route does not write: TIFF_NO_DEFLATE; anything else uncompressed); TIFF_JUNK: a value that names none of them
enum { TIFF_PASS = -1, TIFF_JUNK = -2, TIFF_NO_DEFLATE = -3 };
static int tiff_mode(const CCSParameters *p) {
    const char *e = getenv("CSH_TIFF");
    if (!e || !*e || !strcmp(e, "pass")) return TIFF_PASS;
    if (!strcmp(e, "lzw")) return CST_OUT_LZW;
    if (!strcmp(e, "packbits")) return CST_OUT_PACKBITS;
    if (!strcmp(e, "none")) return CST_OUT_NONE;
    if (strcmp(e, "device")) return TIFF_JUNK;
    return p->tiff_compression == 1 ? int(CST_OUT_LZW) : p->tiff_compression == 3 ? int(CST_OUT_PACKBITS) : p->tiff_compression == 2 ? int(TIFF_NO_DEFLATE) : int(CST_OUT_NONE);
}
// the files of a compress call by the row that takes them; a TIFF file without CSH_TIFF, and a GIF file outside CSH_GIF=device, is answered on the spot, by pass(i) -- or by
// refuse(i, message) under a value of CSH_GIF / CSH_TIFF that means nothing (and for a TIFF file under CSH_TIFF=device with tiff_compression 2)
struct Rows { std::vector<size_t> png, webp, gif, tiff, other; bool any_pass = false, gif_lossy = false; int tiff_out = 0; };
template <class Pass, class Refuse>
static Rows sort_rows(const CByteArray *inputs, size_t count, const CCSParameters *p, Pass pass, Refuse refuse) {
    Rows r;
    const int gif = gif_mode(), tiff = tiff_mode(p);
    r.gif_lossy = gif == 2; r.tiff_out = tiff;
    for (size_t i = 0; i < count; i++) {
        const int t = sniff(inputs[i].data, inputs[i].length);
        if (t == CS_TYPE_GIF && gif < 0) { refuse(i, BAD_CSH_GIF); r.any_pass = true; }
        else if (t == CS_TYPE_TIFF && (tiff == TIFF_JUNK || tiff == TIFF_NO_DEFLATE) && !p->width && !p->height) { refuse(i, tiff == TIFF_JUNK ? BAD_CSH_TIFF : NO_TIFF_DEFLATE); r.any_pass = true; }
        else if (t == CS_TYPE_TIFF && tiff >= 0 && !p->width && !p->height) r.tiff.push_back(i);
        else if (t == CS_TYPE_GIF && gif > 0 && !p->width && !p->height) r.gif.push_back(i);
        else if (t == CS_TYPE_GIF || t == CS_TYPE_TIFF) { pass(i); r.any_pass = true; }
        else (t == CS_TYPE_PNG ? r.png : t == CS_TYPE_WEBP ? r.webp : r.other).push_back(i);
    }
    return r;
}

// A caller may pass no results array: the routes always write one, so such a call gets an array of its own here, released when the call returns
struct Results {
    std::vector<CCSResult> own;
    CCSResult *r;
    Results(CCSResult *given, size_t count) : own(given ? 0 : count, make_result(0, nullptr)), r(given ? given : own.data()) {}
    ~Results() { for (CCSResult &x : own) cs_free_result(&x); }
};

// the *_in_memory forms: one file as a batch of one on device 0
static CByteArray one_file(const uint8_t *in, size_t n, CByteArray *out) { out->data = nullptr; out->length = 0; return CByteArray{const_cast<uint8_t *>(in), n}; }

// where cs_batch_convert sends a file, in the order the routes run
enum Convert { JPEG_TO_WEBP, FROM_WEBP, JPEG_TO_LOSSLESS_WEBP, JPEG_TO_PNG, PNG_TO_JPEG, PNG_TO_LOSSLESS_WEBP, PNG_TO_WEBP, NCONVERT, REFUSED = -1 };
// convert: JPEG -> WebP (the JPEG path's decode and resize, then the VP8 encoder), opaque PNG -> WebP (the PNG path's decode, then
// the same encoder), JPEG -> PNG and PNG -> JPEG (csp_png_to_jpeg) run on the device; every other pair of formats has no device path
static int classify_convert(int src, uint32_t format, bool webp_lossless, int *code, const char **msg) {
    if (src == CS_TYPE_UNKN) { *code = CS_ERR_UNKNOWN_TYPE; *msg = "unknown file type"; return REFUSED; }
    if (uint32_t(src) == format) { *code = CS_ERR_SAME_FORMAT; *msg = "cannot convert to the same format"; return REFUSED; }
    if (src == CS_TYPE_JPEG && format == CS_TYPE_PNG) return JPEG_TO_PNG;
    if (src == CS_TYPE_PNG && format == CS_TYPE_JPEG) return PNG_TO_JPEG;
    if (src == CS_TYPE_WEBP && (format == CS_TYPE_JPEG || format == CS_TYPE_PNG)) return FROM_WEBP;
    if ((src != CS_TYPE_JPEG && src != CS_TYPE_PNG) || format != CS_TYPE_WEBP) {
        *code = CS_ERR_UNSUPPORTED; *msg = "this format conversion has no device path in this build (built: JPEG / PNG -> WebP, JPEG <-> PNG, WebP -> JPEG / PNG)";
        return REFUSED;
    }
    if (webp_lossless) return src == CS_TYPE_JPEG ? JPEG_TO_LOSSLESS_WEBP : PNG_TO_LOSSLESS_WEBP;
    return src == CS_TYPE_PNG ? PNG_TO_WEBP : JPEG_TO_WEBP;
}
static int run_convert(int r, const CByteArray *in, size_t n, const CCSParameters *p, uint32_t format, int device, CByteArray *out, CCSResult *res) {
    switch (r) {
    case JPEG_TO_WEBP: return route::jpeg_to_webp(in, n, p, device, out, res);
    case FROM_WEBP: return route::webp_inputs(in, n, p, format, device, out, res);
    case JPEG_TO_LOSSLESS_WEBP: return route::jpeg_to_pixels(in, n, p, device, out, res, true);
    case JPEG_TO_PNG: return route::jpeg_to_pixels(in, n, p, device, out, res, false);
    case PNG_TO_JPEG: return route::png_convert(in, n, p, device, out, res, false);
    case PNG_TO_LOSSLESS_WEBP: return route::png_convert(in, n, p, device, out, res, true);
    default: return route::png_compress(in, n, p, device, out, res, true);
    }
}

extern "C" {

void cs_default_parameters(CCSParameters *p) {
    memset(p, 0, sizeof *p);
    p->jpeg_quality = 80; p->jpeg_chroma_subsampling = 0; p->jpeg_progressive = true; p->jpeg_optimize = false; p->jpeg_preserve_icc = true;
    p->png_quality = 80; p->png_optimization_level = 3; p->gif_quality = 80; p->webp_quality = 80;
    p->tiff_deflate_level = 6;
}

// one device batch = at most CS_GROUP files: launch grids index (image, scan) pairs in gridDim.y (<= 65535), and a group
// of 2048 1080p files already occupies ~40 GB of HBM and tens of thousands of workgroups per launch (the JPEG row
// cuts its groups further into spans of CS_SPAN files -- CSH_GROUP overrides that span, see route::jpeg_compress)
enum { CS_GROUP = 2048 };
size_t cs_batch_extent(const CByteArray *inputs, size_t count) {
    // ~25 bytes of pools per pixel on the JPEG path (coefficients both ways, planes, per-unit arrays), 4 x the file for the streams
    return route::group_extent(inputs, count, CS_GROUP, uint64_t(2) << 30, uint64_t(96) << 30,
                               [](const CByteArray &f) { return declared_pixels(f.data, f.length) * 25 + 4 * uint64_t(f.length) + (1u << 20); });
}

// one call, mixed inputs: PNG files go to the PNG pipeline, WebP files to theirs, everything else to the JPEG pipeline (which
// answers per file for what it has no device path for); results keep the order of the inputs
int cs_batch_compress(const CByteArray *inputs, size_t count, const CCSParameters *p, int device, CByteArray *outputs, CCSResult *results_or_null) {
    Results own(results_or_null, count);
    CCSResult *results = own.r;
    int passed_failed = 0;
    const Rows r = sort_rows(inputs, count, p, [&](size_t i) { results[i] = passthrough(inputs[i], p, &outputs[i]); if (!results[i].success) passed_failed++; },
                             [&](size_t i, const char *msg) { outputs[i].data = nullptr; outputs[i].length = 0; results[i] = make_result(CS_ERR_UNSUPPORTED, msg); passed_failed++; });
    const std::vector<size_t> &png = r.png, &webp = r.webp, &gif = r.gif, &tiff = r.tiff, &other = r.other;   // PNG files: lossless under png.optimize, else the lossy (quantising) form of the same pipeline
    if (png.empty() && webp.empty() && gif.empty() && tiff.empty() && !r.any_pass) return route::jpeg_compress(inputs, count, p, device, outputs, results);
    std::atomic<int> failed{0};
    auto run = [&](const std::vector<size_t> &idx, int kind) {
        failed += route::for_subset(inputs, idx, outputs, results, [&](const CByteArray *in, size_t n, CByteArray *out, CCSResult *res) {
            return kind == 1 ? route::png_compress(in, n, p, device, out, res, false) : kind == 2 ? route::webp_inputs(in, n, p, CS_TYPE_WEBP, device, out, res) :
                   kind == 3 ? route::gif_compress(in, n, p, device, out, res, r.gif_lossy) : kind == 4 ? route::tiff_compress(in, n, p, device, out, res, r.tiff_out) :
                   route::jpeg_compress(in, n, p, device, out, res);
        });
    };
    // the rows side by side (each batch keeps to its own stream; their outputs are disjoint): a tree of all three kinds waits for its slowest row only
    std::vector<std::thread> rows;
    if (!png.empty() && (!webp.empty() || !other.empty())) rows.emplace_back(run, std::cref(png), 1); else run(png, 1);
    if (!webp.empty() && !other.empty()) rows.emplace_back(run, std::cref(webp), 2); else run(webp, 2);
    if (!gif.empty() && !other.empty()) rows.emplace_back(run, std::cref(gif), 3); else run(gif, 3);
    if (!tiff.empty() && !other.empty()) rows.emplace_back(run, std::cref(tiff), 4); else run(tiff, 4);
    run(other, 0);
    for (std::thread &t : rows) t.join();
    return failed.load() + passed_failed;
}
CCSResult cs_compress_in_memory(const uint8_t *in, size_t n, const CCSParameters *p, CByteArray *out) {
    const CByteArray input = one_file(in, n, out);
    CCSResult r = {false, 0, nullptr};
    cs_batch_compress(&input, 1, p, 0, out, &r);
    return r;
}

// size-targeting (size_walk.h): JPEG files walk over the retained DCT of one batch, PNG and WebP files run their route again per try
int cs_batch_compress_to_size(const CByteArray *inputs, size_t count, CCSParameters *p, size_t max_output_size, bool return_smallest, int device,
                              CByteArray *outputs, CCSResult *results_or_null) {
    Results own(results_or_null, count);
    CCSResult *results = own.r;
    int failed = 0;
    // libcaesium's size walk returns its smallest try when asked to, and fails otherwise: a file that cannot be made smaller
    // and is larger than the target is a failure unless return_smallest
    auto hold_to_target = [&](size_t i, const char *msg) {
        if (results[i].success && outputs[i].length > max_output_size && !return_smallest) { cs_free_bytes(&outputs[i]); results[i] = make_result(CS_ERR_TOO_BIG, msg); failed++; }
    };
    const Rows rows = sort_rows(inputs, count, p, [&](size_t i) {   // passed through as it is (see passthrough()): there is no quality to walk
        results[i] = passthrough(inputs[i], p, &outputs[i]);
        if (!results[i].success) failed++;
        hold_to_target(i, "the file is passed through as it is (GIF / TIFF have no device path) and is larger than the target size");
    }, [&](size_t i, const char *msg) { outputs[i].data = nullptr; outputs[i].length = 0; results[i] = make_result(CS_ERR_UNSUPPORTED, msg); failed++; });
    // a GIF file under CSH_GIF=device / lossy: one run of its route (the optimiser is pixel-exact, and the lossy coder runs at the quality given: no quality is walked), then the same rule
    failed += route::for_subset(inputs, rows.gif, outputs, results, [&](const CByteArray *in, size_t n, CByteArray *out, CCSResult *res) { return route::gif_compress(in, n, p, device, out, res, rows.gif_lossy); });
    for (size_t i : rows.gif) hold_to_target(i, rows.gif_lossy ? "the GIF route runs once, at the quality given, and walks no quality: its one result is larger than the target size"
                                                               : "the GIF optimiser is pixel-exact and has no quality to walk: its one result is larger than the target size");
    // a TIFF file with CSH_TIFF set: one run of its route (lossless: there is no quality to walk), then the same rule
    failed += route::for_subset(inputs, rows.tiff, outputs, results, [&](const CByteArray *in, size_t n, CByteArray *out, CCSResult *res) { return route::tiff_compress(in, n, p, device, out, res, rows.tiff_out); });
    for (size_t i : rows.tiff) hold_to_target(i, "the TIFF route is lossless and has no quality to walk: its one result is larger than the target size");
    if (rows.png.empty() && rows.webp.empty() && rows.gif.empty() && rows.tiff.empty() && !rows.any_pass) return route::jpeg_compress_to_size(inputs, count, p, max_output_size, return_smallest, device, outputs, results);
    // the JPEG walk leaves its last quality in the caller's parameters, as the reference's &mut does
    failed += route::for_subset(inputs, rows.other, outputs, results, [&](const CByteArray *in, size_t n, CByteArray *out, CCSResult *res) {
        return route::jpeg_compress_to_size(in, n, p, max_output_size, return_smallest, device, out, res);
    });
    for (int webp_files = 0; webp_files < 2; webp_files++)
        failed += route::for_subset(inputs, webp_files ? rows.webp : rows.png, outputs, results, [&](const CByteArray *in, size_t n, CByteArray *out, CCSResult *res) {
            return route::rerun_to_size(in, n, p, max_output_size, return_smallest, device, out, res, webp_files != 0);
        });
    return failed;
}
CCSResult cs_compress_to_size_in_memory(const uint8_t *in, size_t n, CCSParameters *p, size_t max_output_size, bool return_smallest, CByteArray *out) {
    const CByteArray input = one_file(in, n, out);
    CCSResult r = make_result(0, nullptr);
    cs_batch_compress_to_size(&input, 1, p, max_output_size, return_smallest, 0, out, &r);
    return r;
}

int cs_batch_convert(const CByteArray *inputs, size_t count, const CCSParameters *p, uint32_t format, int device, CByteArray *outputs, CCSResult *results_or_null) {
    Results own(results_or_null, count);
    CCSResult *results = own.r;
    int failed_total = 0;
    std::vector<size_t> idx[NCONVERT];
    for (size_t i = 0; i < count; i++) {
        outputs[i].data = nullptr; outputs[i].length = 0;
        int code = 0; const char *msg = nullptr;
        const int r = classify_convert(sniff(inputs[i].data, inputs[i].length), format, p->webp_lossless, &code, &msg);
        if (r == REFUSED) { results[i] = make_result(code, msg); failed_total++; } else idx[r].push_back(i);
    }
    for (int r = 0; r < NCONVERT; r++)
        failed_total += route::for_subset(inputs, idx[r], outputs, results, [&](const CByteArray *in, size_t n, CByteArray *out, CCSResult *res) {
            return run_convert(r, in, n, p, format, device, out, res);
        });
    return failed_total;
}
CCSResult cs_convert_in_memory(const uint8_t *in, size_t n, const CCSParameters *p, uint32_t format, CByteArray *out) {
    const CByteArray input = one_file(in, n, out);
    CCSResult r = {false, 0, nullptr};
    cs_batch_convert(&input, 1, p, format, 0, out, &r);
    return r;
}

void cs_free_bytes(CByteArray *b) { if (b && b->data) { free(b->data); b->data = nullptr; b->length = 0; } }
void cs_free_result(CCSResult *r) { if (r && r->error_message) { free(const_cast<char *>(r->error_message)); r->error_message = nullptr; } }

}  // extern "C"
