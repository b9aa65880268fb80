// png_convert.cpp -- the PNG sources that go through pixels: width / height on a PNG (decode, Lanczos3, encode again) and the converters
// PNG -> JPEG and PNG -> lossless WebP.  All of them start with a decode-only batch and expand its pixels with k_png_rgb; what they share is
// here once: decode_to_pixels, add_rgb_job / Expansion, ResizePlan, collect_results.
#include <cstring>

#include "png_batch.hpp"
#include "resize_host.h"

namespace csp {

using csh::DevBuf;

uint32_t rgb_channels(const PngItem &it, bool keep_alpha) {
    return ((it.ctype == 2 || it.ctype == 6 || it.ctype == 3) ? 3u : 1u) + ((keep_alpha && it.transparent()) ? 1u : 0u);
}

RgbJob add_rgb_job(const PngItem &it, uint32_t out_nc, uint64_t src_off, uint64_t dst_off, std::vector<uint8_t> &tables) {
    RgbJob e{};
    e.image = uint32_t(it.image); e.width = it.width; e.height = it.height; e.rowbytes = it.rowbytes; e.ctype = it.ctype; e.depth = it.depth; e.out_nc = out_nc;
    e.plte_off = uint32_t(tables.size()); e.npal = uint32_t(it.plte.size() / 3);
    tables.insert(tables.end(), it.plte.begin(), it.plte.end());
    e.trns_off = uint32_t(tables.size()); e.ntrns = uint32_t(it.trns.size());
    tables.insert(tables.end(), it.trns.begin(), it.trns.end());
    e.src_off = src_off; e.dst_off = dst_off;
    return e;
}

namespace {

// a decode-only batch of the files, run, and the status words of its images
int decode_to_pixels(const CByteArray *inputs, size_t count, const CCSParameters *p, int device, int mode, std::unique_ptr<csp_batch> &a, std::vector<uint32_t> &status) {
    csp_batch *raw = nullptr;
    int rc = png_create(inputs, nullptr, count, p, device, mode, &raw);
    a.reset(raw);
    if (rc == 0) rc = csp_batch_run(a.get(), nullptr);
    if (rc) return rc;
    if (read_status_and_lengths(a.get(), status, nullptr)) { csh_set_error("download failed"); return CS_ERR_NO_DEVICE; }
    return 0;
}

// the pixels of a decode-only batch as the png crate's EXPAND transformation hands them on (k_png_rgb), image behind image in d_src
struct Expansion {
    std::vector<RgbJob> ejobs;
    std::vector<uint8_t> tables = std::vector<uint8_t>(1, 0);   // PLTE and tRNS payloads
    uint64_t src_bytes = 0;
    uint32_t max_h = 0;
    DevBuf<RgbJob> d_ejobs;
    DevBuf<uint8_t> d_tables, d_src;
    // the job of one image and its place in d_src (bps: bytes per sample there); the caller pushes it, or fills the place some other way
    RgbJob next(const PngItem &it, uint32_t nc, uint32_t bps, uint64_t pix_off) {
        const RgbJob e = add_rgb_job(it, nc, pix_off, src_bytes, tables);
        src_bytes += (uint64_t(it.width) * it.height * nc * bps + 255) & ~uint64_t(255);
        return e;
    }
    void push(const RgbJob &e) { max_h = std::max(max_h, e.height); ejobs.push_back(e); }
    int upload(hipStream_t st) { return (d_ejobs.upload(ejobs, st) || d_tables.upload(tables, st) || d_src.alloc(src_bytes + 256)) ? -1 : 0; }
    void launch(hipStream_t st, csp_batch *a) { launch_png_rgb(st, d_ejobs.p, int(ejobs.size()), max_h, d_tables.p, a->d_work.p, d_src.p, a->d_status.p); }
};

// the two Lanczos passes of k_png_resize.hip over interleaved samples: jobs, taps and buffers
struct ResizePlan {
    std::vector<PngResize> jobs;
    std::vector<csh::ResizeTap> taps;
    std::vector<float> weights;
    uint64_t tmp_floats = 0, dst_bytes = 0, max_tmp = 0, max_dst = 0;
    DevBuf<PngResize> d_jobs;
    DevBuf<csh::ResizeTap> d_taps;
    DevBuf<float> d_weights, d_tmp;
    DevBuf<uint8_t> d_dst;
    // one picture (its samples at src_off of the source buffer) towards the size p asks for.  false: too large for one device batch -- one lane per
    // sample, a launch holds 2^32 of them.  guard_source_row: the caller's guard covers the source row too
    bool add(uint32_t width, uint32_t height, uint32_t nc, uint32_t bps, uint64_t src_off, const CCSParameters *p, bool guard_source_row) {
        int nw = 0, nh = 0;
        csh_compute_dimensions(int(width), int(height), int(p->width), int(p->height), nw, nh);
        const uint64_t tmpn = uint64_t(nh) * width * nc, dstn = uint64_t(nw) * nh * nc;
        if (uint64_t(nw) * nc * bps > 0x7FFFFFF0u || (guard_source_row && uint64_t(width) * nc * bps > 0x7FFFFFF0u) || tmpn > 0xFFFFFF00u || dstn > 0xFFFFFF00u / bps) return false;
        PngResize j{};
        j.width = width; j.height = height; j.nc = nc; j.nw = uint32_t(nw); j.nh = uint32_t(nh); j.bps = bps;
        j.src_off = src_off; j.tmp_off = tmp_floats; j.dst_off = dst_bytes;
        const bool same = uint32_t(nw) == width && uint32_t(nh) == height;   // image-rs copies instead of resampling
        j.vtap_base = uint32_t(taps.size()); csh_lanczos_axis(int(height), nh, same, taps, weights);
        j.htap_base = uint32_t(taps.size()); csh_lanczos_axis(int(width), nw, same, taps, weights);
        tmp_floats += (tmpn + 63) & ~uint64_t(63); dst_bytes += (dstn * bps + 255) & ~uint64_t(255);
        max_tmp = std::max(max_tmp, tmpn); max_dst = std::max(max_dst, dstn);
        jobs.push_back(j);
        return true;
    }
    int upload(hipStream_t st) {
        return (d_jobs.upload(jobs, st) || d_taps.upload(taps, st) || d_weights.upload(weights, st) || d_tmp.alloc((png_resize_is_fused(jobs.data(), int(jobs.size())) ? 0 : tmp_floats) + 64) ||
                d_dst.alloc(dst_bytes + 256)) ? -1 : 0;
    }
    int launch(hipStream_t st, const uint8_t *src) {   // (waits)
        launch_png_resize(st, d_jobs.p, jobs.data(), int(jobs.size()), d_taps.p, d_weights.p, src, d_tmp.p, d_dst.p, max_tmp, max_dst);
        if (hipStreamSynchronize(st) != hipSuccess || hipGetLastError() != hipSuccess) { csh_set_error("PNG resize kernels failed"); return -1; }
        return 0;
    }
    uint8_t *resized(size_t k) const { return d_dst.p + jobs[k].dst_off; }
};

// what an encoder made of pictures at[k] of the caller's files: nfailed < 0: the call itself failed (rc, or no code: the device).  Returns the failures
int collect_results(const std::vector<size_t> &at, std::vector<CByteArray> &out, std::vector<CCSResult> &res, int nfailed, int rc, CByteArray *outputs, CCSResult *results) {
    for (size_t k = 0; k < at.size(); k++) {
        if (nfailed < 0) { if (results) results[at[k]] = png_result(rc ? rc : CS_ERR_NO_DEVICE, csh_last_error()); continue; }
        outputs[at[k]] = out[k];
        if (results) results[at[k]] = res[k]; else cs_free_result(&res[k]);
    }
    return nfailed < 0 ? int(at.size()) : nfailed;
}

// lossless WebP with a size.  Opaque pictures (grey, RGB): the JPEG row's resize branch, stopped behind its pixels (*rb keeps them); pictures with
// transparency (grey + alpha, RGBA): the PNG row's own two Lanczos passes over the interleaved samples (k_png_resize.hip, the same arithmetic; image-rs
// resamples the channels alike).  src: the pictures, resized
int resize_for_webp(const CCSParameters *p, int device, hipStream_t st, const std::vector<csp_pixels> &px, const Expansion &X, ResizePlan &R, csh_batch **rb, std::vector<csp_pixels> &src) {
    std::vector<csp_pixels> opaque;
    std::vector<size_t> opaque_at, job_at;
    for (size_t k = 0; k < px.size(); k++) {
        if (px[k].channels == 1 || px[k].channels == 3) { opaque.push_back(px[k]); opaque_at.push_back(k); continue; }
        if (!R.add(px[k].width, px[k].height, px[k].channels, 1, X.ejobs[k].dst_off, p, false)) { csh_set_error("resized PNG too large for one device batch"); return CS_ERR_UNSUPPORTED; }
        src[k].width = R.jobs.back().nw; src[k].height = R.jobs.back().nh;
        job_at.push_back(k);
    }
    if (!opaque.empty()) {
        int rc = csh_batch_create_from_pixels_rgb(opaque.data(), opaque.size(), p, device, rb);
        if (rc == 0) rc = csh_batch_run(*rb, nullptr);
        for (size_t j = 0; j < opaque.size() && rc == 0; j++) { const char *m = ""; csp_pixels &d = src[opaque_at[j]]; if (csh_batch_pixels(*rb, j, &d.device_pixels, &d.width, &d.height, &d.channels, &m)) rc = CS_ERR_NO_DEVICE; }
        if (rc) return rc;
    }
    if (!R.jobs.empty()) {
        if (R.upload(st) || R.launch(st, X.d_src.p)) return CS_ERR_NO_DEVICE;
        for (size_t j = 0; j < R.jobs.size(); j++) src[job_at[j]].device_pixels = R.resized(j);
    }
    return 0;
}

// PNG -> JPEG (convert_in_memory to JPEG): a decode-only batch, the pixels as 8-bit grey or RGB (k_png_rgb: palette looked up, 16-bit narrowed,
// sub-byte grey scaled; an alpha channel or tRNS is dropped, as image-rs's JPEG encoder does [UPSTREAM-RECALL]), then the JPEG batch object from
// those pixels (csh_batch_create_from_pixels: its resize honours width / height, its encoder p's JPEG parameters).  Device to device; results in input order.
// PNG -> lossless WebP shares everything up to the pixels.  It keeps an alpha channel / tRNS chunk as the picture's alpha (grey + alpha / RGBA pixels)
// and sends the pixels -- resized first when a size is given -- to the VP8L coder (csl_encode_pixels).
int png_to_pixels_then(const CByteArray *inputs, size_t count, const CCSParameters *p, int device, CByteArray *outputs, CCSResult *results, bool lossless_webp) {
    for (size_t i = 0; i < count; i++) { outputs[i].data = nullptr; outputs[i].length = 0; }
    auto fail_all = [&](int rc) { for (size_t i = 0; i < count; i++) if (results) results[i] = png_result(rc, csh_last_error()); return int(count); };
    CCSParameters q = *p;
    q.width = 0; q.height = 0;
    std::unique_ptr<csp_batch> a;
    std::vector<uint32_t> status;
    if (int rc = decode_to_pixels(inputs, count, &q, device, MODE_DECODE_ANY, a, status)) return fail_all(rc);
    hipStream_t st = a->stream;
    Expansion X;
    std::vector<size_t> at;
    std::vector<csp_pixels> px;
    int failed = 0;
    for (size_t i = 0; i < count; i++) {
        const PngItem &it = a->items[i];
        int code = it.code;
        const char *msg = it.msg.c_str();
        if (!code && status[it.image]) { code = int(status[it.image]); msg = "malformed PNG data"; }
        if (!code && !lossless_webp && (it.width > 65535 || it.height > 65535)) { code = CS_ERR_UNSUPPORTED; msg = "image too large for a JPEG"; }
        if (!code && lossless_webp && (it.width > 16384 || it.height > 16384)) { code = CS_ERR_UNSUPPORTED; msg = "image too large for a WebP"; }
        if (code) { if (results) results[i] = png_result(code, msg); failed++; continue; }
        const uint32_t nc = rgb_channels(it, lossless_webp);   // a JPEG drops the alpha; a lossless WebP keeps it
        X.push(X.next(it, nc, 1, a->imgs[it.image].pix_off));
        px.push_back(csp_pixels{nullptr, it.width, it.height, nc});   // the pointer is known once the buffer is
        at.push_back(i);
    }
    if (px.empty()) return failed;
    auto fail_rest = [&](int code) { for (size_t k : at) if (results) results[k] = png_result(code, csh_last_error()); return failed + int(at.size()); };   // the files that were still good
    if (X.upload(st)) return fail_rest(CS_ERR_NO_DEVICE);
    X.launch(st, a.get());
    if (hipStreamSynchronize(st) != hipSuccess || hipGetLastError() != hipSuccess) { csh_set_error("PNG kernels failed"); return fail_rest(CS_ERR_NO_DEVICE); }
    for (size_t k = 0; k < px.size(); k++) px[k].device_pixels = X.d_src.p + X.ejobs[k].dst_off;
    std::vector<CByteArray> out(px.size());
    std::vector<CCSResult> res(px.size());
    csh_batch *jb = nullptr;   // to JPEG: the encoder; to lossless WebP: the resize branch of the opaque pictures
    ResizePlan R;
    std::vector<csp_pixels> src = px;
    int rc = 0, nfailed;
    if (lossless_webp) {
        if (p->width || p->height) rc = resize_for_webp(p, device, st, px, X, R, &jb, src);
        nfailed = rc ? -1 : csl_encode_pixels(src.data(), src.size(), device, out.data(), res.data());
    } else {
        rc = csh_batch_create_from_pixels(px.data(), px.size(), p, device, &jb);
        if (rc == 0) rc = csh_batch_run(jb, nullptr);
        nfailed = rc ? -1 : csh_batch_fetch(jb, out.data(), res.data());
    }
    failed += collect_results(at, out, res, nfailed, rc, outputs, results);
    csh_batch_destroy(jb);
    return failed;
}

}  // namespace

// width / height on PNG sources (libcaesium png::compress with a size: decode, image-rs resize_exact Lanczos3, encode): a decode-only
// batch, the two Lanczos passes over its pixels, then the coder -- or, on the way to WebP, the VP8 encoder -- over the resized pixels
// (device to device, as for JPEG -> PNG).
// The pixels are expanded first as the png crate does for image-rs (palette looked up, sub-byte grey scaled, tRNS as an alpha channel:
// k_png_rgb); 16-bit sources keep their 16 bits (a tRNS chunk becomes a 16-bit alpha sample).
int png_create_resized(const CByteArray *inputs, size_t count, const CCSParameters *p, int device, int mode, csp_batch **out) {
    *out = nullptr;
    std::unique_ptr<csp_batch> a;
    std::vector<uint32_t> status;
    if (int rc = decode_to_pixels(inputs, count, p, device, MODE_DECODE, a, status)) return rc;
    hipStream_t st = a->stream;
    std::vector<PreFail> pre(count);
    std::vector<csp_pixels> px(count);
    Expansion X;
    ResizePlan R;
    std::vector<size_t> job_item;
    struct RawCopy { uint64_t dst, src, bytes; };
    std::vector<RawCopy> copies;
    std::vector<uint8_t> bits(count, 8);
    for (size_t i = 0; i < count; i++) {
        const PngItem &it = a->items[i];
        px[i] = csp_pixels{nullptr, 0, 0, 0};
        if (it.code) { pre[i] = PreFail{it.code, it.msg}; continue; }
        if (status[it.image]) { pre[i] = PreFail{int(status[it.image]), "malformed PNG data"}; continue; }
        // what the png crate's EXPAND transformation hands image-rs: 8-bit samples, palette looked up, tRNS as an alpha channel
        // (16-bit images stay as they are: image-rs resamples L16 / La16 / Rgb16 / Rgba16 at 16 bits)
        const bool wide = it.depth == 16;
        if (wide && it.has_trns && mode != MODE_PNG) { pre[i] = PreFail{CS_ERR_UNSUPPORTED, "resizing a 16-bit PNG with a tRNS chunk on the way to another format has no device path in this build"}; continue; }
        const uint32_t nc = rgb_channels(it, true), bps = wide ? 2u : 1u;
        if (!R.add(it.width, it.height, nc, bps, X.src_bytes, p, true)) { pre[i] = PreFail{CS_ERR_UNSUPPORTED, "resized PNG too large for one device batch"}; continue; }
        RgbJob e = X.next(it, nc, bps, a->imgs[it.image].pix_off);
        e.wide = wide && it.has_trns && (it.ctype == 0 || it.ctype == 2) ? 1u : 0u;   // the colour key becomes a 16-bit alpha sample
        if (wide && !e.wide) copies.push_back(RawCopy{e.dst_off, e.src_off, uint64_t(it.height) * it.rowbytes});   // nothing to expand
        else X.push(e);
        bits[i] = uint8_t(8 * bps);
        px[i].width = R.jobs.back().nw; px[i].height = R.jobs.back().nh; px[i].channels = nc;
        job_item.push_back(i);
    }
    if (!R.jobs.empty()) {
        if (R.upload(st) || X.upload(st)) return CS_ERR_NO_DEVICE;
        X.launch(st, a.get());
        for (const RawCopy &c : copies)
            if (hipMemcpyAsync(X.d_src.p + c.dst, a->d_work.p + c.src, c.bytes, hipMemcpyDeviceToDevice, st) != hipSuccess) { csh_set_error("pixel copy failed"); return CS_ERR_NO_DEVICE; }
        if (R.launch(st, X.d_src.p)) return CS_ERR_NO_DEVICE;
        for (size_t k = 0; k < R.jobs.size(); k++) px[job_item[k]].device_pixels = R.resized(k);
    }
    CCSParameters q = *p;
    q.width = 0; q.height = 0;
    return png_create(nullptr, px.data(), count, &q, device, mode, out, &pre, &bits);   // copies the pixels before the resized ones go out of scope
}

}  // namespace csp

using namespace csp;

extern "C" int csp_batch_create(const CByteArray *inputs, size_t count, const CCSParameters *p, int device, csp_batch **out) {
    return (p->width || p->height) ? png_create_resized(inputs, count, p, device, MODE_PNG, out) : png_create(inputs, nullptr, count, p, device, MODE_PNG, out);
}
extern "C" int csp_batch_create_webp(const CByteArray *inputs, size_t count, const CCSParameters *p, int device, csp_batch **out) {
    return (p->width || p->height) ? png_create_resized(inputs, count, p, device, MODE_WEBP, out) : png_create(inputs, nullptr, count, p, device, MODE_WEBP, out);
}
extern "C" int csp_batch_create_pixels(const csp_pixels *sources, size_t count, const CCSParameters *p, int device, csp_batch **out) { return png_create(nullptr, sources, count, p, device, MODE_PNG, out); }
extern "C" int csp_png_to_jpeg(const CByteArray *inputs, size_t count, const CCSParameters *p, int device, CByteArray *outputs, CCSResult *results) {
    return png_to_pixels_then(inputs, count, p, device, outputs, results, false);
}
extern "C" int csp_png_to_lossless_webp(const CByteArray *inputs, size_t count, const CCSParameters *p, int device, CByteArray *outputs, CCSResult *results) {
    return png_to_pixels_then(inputs, count, p, device, outputs, results, true);
}
