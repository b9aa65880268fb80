// webp_anim.cpp -- animated WebP inputs (libcaesium decodes them with libwebp's AnimDecoder and codes the frames again): the container on the host (VP8X, ANIM,
// every ANMF; the muxer of the output), the canvases and the change search on the device (k_webp_anim.hip), the frames' rectangles through the encoders the
// still pictures take (the lossy WebP encoder with csl_encode_pixels for an ALPH chunk, or csl_encode_pixels alone under webp.lossless).
// The output keeps the canvas, the frame count, every duration, the loop count and the background colour.  Frame 0 is the whole canvas; frame k > 0 the bounding
// box of the pixels that differ from canvas k - 1, its left and top edge rounded down to even (1 x 1 at the origin when nothing changed); every frame disposes
// to none.  Lossy frames do not blend.  A lossless frame is written in blend form -- an unchanged pixel as 0x00000000 -- when every changed pixel is opaque and the
// rectangle holds an unchanged pixel at all, else it does not blend either.
#include <algorithm>
#include <cstring>

#include "riff.h"
#include "routes.hpp"
#include "webp_anim.hpp"

using namespace csh;
using riff::rd24; using riff::rd32; using riff::wr24; using riff::wr32;

// AnimDecoder's key frames: the first; a frame that covers the canvas and does not blend; a frame behind one that disposed to the background and either covered
// the canvas or was a key frame itself (nothing of an older canvas is left then)
static void anim_key_frames(cswd_anim &a) {
    bool prev_key = false, prev_full = false, prev_dispose = false;
    for (size_t k = 0; k < a.frames.size(); k++) {
        csw::AnimFrame &f = a.frames[k];
        const bool full = f.x == 0 && f.y == 0 && f.w == a.cw && f.h == a.ch;
        const bool key = k == 0 || (full && (f.flags & csw::ANIM_NO_BLEND)) || (prev_dispose && (prev_full || prev_key));
        if (key) f.flags |= csw::ANIM_KEY;
        prev_key = key; prev_full = full; prev_dispose = (f.flags & csw::ANIM_DISPOSE) != 0;
    }
}

int cswd_parse_anim(const uint8_t *d, size_t n, cswd_anim &a, std::vector<cswd_frame_src> &src, std::string &msg) {
    bool have_canvas = false, have_anim = false;
    for (riff::Chunks c(d, n, riff::declared_end(d, n)); c.next();) {
        if (c.truncated) { msg = "truncated WebP chunk"; return CS_ERR_BAD_WEBP; }
        const uint8_t *p = c.payload();
        const size_t cl = c.len;
        if (c.is("VP8X") && cl >= 10) { a.cw = rd24(p + 4) + 1; a.ch = rd24(p + 7) + 1; have_canvas = true; }
        else if (c.is("ANIM") && cl >= 6) { a.background = rd32(p); a.loops = uint32_t(p[4]) | (uint32_t(p[5]) << 8); have_anim = true; }
        else if (c.is("ANMF")) {
            if (!have_canvas || !have_anim || cl < 16) { msg = "ANMF chunk without VP8X and ANIM in front of it, or shorter than its header"; return CS_ERR_BAD_WEBP; }
            csw::AnimFrame f;
            memset(&f, 0, sizeof f);
            f.x = 2 * rd24(p); f.y = 2 * rd24(p + 3); f.w = rd24(p + 6) + 1; f.h = rd24(p + 9) + 1;
            f.flags = ((p[15] & 0x01) ? csw::ANIM_DISPOSE : 0u) | ((p[15] & 0x02) ? csw::ANIM_NO_BLEND : 0u);
            if (uint64_t(f.x) + f.w > a.cw || uint64_t(f.y) + f.h > a.ch) { msg = "an animation frame leaves the canvas"; return CS_ERR_BAD_WEBP; }
            cswd_frame_src s;
            for (riff::Chunks in(p, cl, cl, 16); !s.len && in.next();) {   // ALPH in front of VP8, or VP8L; anything else is passed by
                if (in.truncated) { msg = "truncated chunk inside an ANMF chunk"; return CS_ERR_BAD_WEBP; }
                const size_t off = c.at + 8 + in.at + 8;
                if (in.is("ALPH")) { if (!s.alph_len) { s.alph_off = off; s.alph_len = in.len; } }
                else if (in.is("VP8 ")) { s.off = off; s.len = in.len; }
                else if (in.is("VP8L")) { s.off = off; s.len = in.len; s.lossless = true; }
            }
            if (!s.len) { msg = "an ANMF chunk holds no VP8 / VP8L bitstream"; return CS_ERR_BAD_WEBP; }
            f.image = uint32_t(a.frames.size());
            a.frames.push_back(f); a.duration.push_back(rd24(p + 12)); src.push_back(s);
        }
    }
    if (a.frames.empty()) { msg = "an animated WebP file without frames"; return CS_ERR_BAD_WEBP; }
    if (uint64_t(a.cw) * a.ch > (uint64_t(1) << 30)) { msg = "animated WebP: a canvas of more than 2^30 pixels has no device path"; return CS_ERR_UNSUPPORTED; }
    anim_key_frames(a);
    return 0;
}

extern "C" int cswd_batch_frames(cswd_batch *b, size_t file, uint32_t *nframes, uint32_t *canvas_w, uint32_t *canvas_h) {
    *nframes = *canvas_w = *canvas_h = 0;
    if (file >= b->items.size()) { csh_set_error("cswd_batch_frames: index out of range"); return -1; }
    const cswd_batch::Item &it = b->items[file];
    if (it.code) return it.code;
    if (it.anim < 0) return 0;
    const cswd_anim &a = b->anims[size_t(it.anim)];
    *nframes = uint32_t(a.frames.size()); *canvas_w = a.cw; *canvas_h = a.ch;
    return 0;
}

extern "C" int cswd_batch_read_canvas(cswd_batch *b, size_t file, uint32_t frame, uint8_t *dst) {
    if (!b->ran || file >= b->items.size()) { csh_set_error("cswd_batch_read_canvas: batch not run / index out of range"); return -1; }
    const cswd_batch::Item &it = b->items[file];
    if (it.code) return it.code;
    if (it.anim < 0 || frame >= b->anims[size_t(it.anim)].frames.size()) { csh_set_error("cswd_batch_read_canvas: not an animated file / no such frame"); return -1; }
    if (hipSetDevice(b->device) != hipSuccess) { csh_set_error("hipSetDevice failed"); return CS_ERR_NO_DEVICE; }
    const cswd_anim &a = b->anims[size_t(it.anim)];
    const std::vector<csw::AnimFile> files = {csw::AnimFile{0, uint32_t(a.frames.size()), a.cw, a.ch}};
    const uint64_t npx = uint64_t(a.cw) * a.ch;
    DevBuf<csw::AnimFile> d_files;
    DevBuf<csw::AnimFrame> d_frames;
    DevBuf<uint8_t> d_canvas;
    if (d_files.upload(files, b->stream) || d_frames.upload(a.frames, b->stream) || d_canvas.alloc(size_t(npx) * 4)) return CS_ERR_NO_DEVICE;
    csw::launch_webp_anim(b->stream, csw::ANIM_WALK_CANVAS, d_files.p, 1, npx, d_frames.p, b->d_imgs.p, b->d_rgb.p, nullptr, d_canvas.p, frame);
    if (csh_copy_wait(dst, d_canvas.p, size_t(npx) * 4, hipMemcpyDeviceToHost, b->stream) != hipSuccess || hipGetLastError() != hipSuccess) { csh_set_error("canvas walk failed on the device"); return CS_ERR_NO_DEVICE; }
    return 0;
}

namespace {
struct Chunks {   // a frame's coded chunks as they go into its ANMF: [ALPH,] VP8 -- or VP8L
    std::vector<uint8_t> bytes;
    bool alpha = false;
};
}

// files[j] of the batch -> outputs / results at the same index as the file has in `sources` (the array cswd_batch_create was given)
extern "C" int cswd_batch_encode_anim(cswd_batch *b, const CByteArray *sources, const size_t *files, size_t nfiles, const CCSParameters *p, int device, CByteArray *outputs, CCSResult *results) {
    if (!nfiles) return 0;
    auto fail_all = [&](int code, const char *msg) { for (size_t j = 0; j < nfiles; j++) { outputs[files[j]].data = nullptr; outputs[files[j]].length = 0; results[files[j]] = make_result(uint32_t(code), msg); } return int(nfiles); };
    if (!b->ran) return fail_all(-1, "cswd_batch_encode_anim: batch not run");
    if (hipSetDevice(b->device) != hipSuccess) return fail_all(CS_ERR_NO_DEVICE, "hipSetDevice failed");
    const bool lossless = p->webp_lossless;
    // the files' frames in one array, the statistics beside it
    std::vector<csw::AnimFile> afiles;
    std::vector<csw::AnimFrame> frames;
    uint64_t max_px = 0;
    for (size_t j = 0; j < nfiles; j++) {
        const cswd_batch::Item &it = b->items[files[j]];
        if (it.code || it.anim < 0) return fail_all(-1, "cswd_batch_encode_anim: not an animated file of this batch");
        const cswd_anim &a = b->anims[size_t(it.anim)];
        afiles.push_back(csw::AnimFile{uint32_t(frames.size()), uint32_t(a.frames.size()), a.cw, a.ch});
        frames.insert(frames.end(), a.frames.begin(), a.frames.end());
        max_px = std::max(max_px, uint64_t(a.cw) * a.ch);
    }
    std::vector<uint32_t> stats(frames.size() * csw::ANIM_STAT, 0u);
    for (size_t k = 0; k < frames.size(); k++) stats[k * csw::ANIM_STAT] = stats[k * csw::ANIM_STAT + 1] = 0xFFFFFFFFu;
    DevBuf<csw::AnimFile> d_files;
    DevBuf<csw::AnimFrame> d_frames;
    DevBuf<uint32_t> d_stats;
    DevBuf<uint8_t> d_rects;
    if (d_files.upload(afiles, b->stream) || d_frames.upload(frames, b->stream) || d_stats.upload(stats, b->stream)) return fail_all(CS_ERR_NO_DEVICE, csh_last_error());
    csw::launch_webp_anim(b->stream, csw::ANIM_WALK_STATS, d_files.p, int(afiles.size()), max_px, d_frames.p, b->d_imgs.p, b->d_rgb.p, d_stats.p, nullptr, 0);
    if (csh_copy_wait(stats.data(), d_stats.p, stats.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, b->stream) != hipSuccess || hipGetLastError() != hipSuccess)
        return fail_all(CS_ERR_NO_DEVICE, "the change search failed on the device");
    // the rectangles, their form and their place in the pool
    uint64_t pool_bytes = 0;
    for (const csw::AnimFile &F : afiles)
        for (uint32_t k = 0; k < F.nframes; k++) {
            csw::AnimFrame &f = frames[F.first + k];
            const uint32_t *s = &stats[size_t(F.first + k) * csw::ANIM_STAT];
            if (k == 0) { f.ox = f.oy = 0; f.ow = F.cw; f.oh = F.ch; }
            else if (!s[4]) { f.ox = f.oy = 0; f.ow = f.oh = 1; }
            else { f.ox = s[0] & ~1u; f.oy = s[1] & ~1u; f.ow = s[2] + 1 - f.ox; f.oh = s[3] + 1 - f.oy; }
            if (lossless && k > 0 && !s[5] && uint64_t(s[4]) < uint64_t(f.ow) * f.oh) f.flags |= csw::ANIM_HOLES;
            const uint64_t npx = uint64_t(f.ow) * f.oh;
            f.split = lossless ? 0u : 1u;
            f.out_off = pool_bytes; pool_bytes += ((lossless ? 4 : 3) * npx + 63) & ~uint64_t(63);
            f.a_off = pool_bytes; if (!lossless) pool_bytes += (npx + 63) & ~uint64_t(63);
        }
    if (d_frames.upload(frames, b->stream) || d_rects.alloc(size_t(pool_bytes) + 64)) return fail_all(CS_ERR_NO_DEVICE, csh_last_error());
    csw::launch_webp_anim(b->stream, csw::ANIM_WALK_PACK, d_files.p, int(afiles.size()), max_px, d_frames.p, b->d_imgs.p, b->d_rgb.p, d_stats.p, d_rects.p, 0);
    if (csh_copy_wait(stats.data(), d_stats.p, stats.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, b->stream) != hipSuccess || hipGetLastError() != hipSuccess)
        return fail_all(CS_ERR_NO_DEVICE, "packing the frames' rectangles failed on the device");
    // the encoders the still pictures take, over every frame of every file (in runs: a device batch holds a few thousand pictures)
    const size_t nfr = frames.size(), run = 1024;
    std::vector<Chunks> coded(nfr);
    std::vector<int> code(nfr, 0);
    std::vector<std::string> why(nfr);
    for (size_t r0 = 0; r0 < nfr; r0 += run) {
        const size_t rn = std::min(run, nfr - r0);
        std::vector<csp_pixels> px(rn);
        std::vector<CByteArray> out(rn);
        std::vector<CCSResult> res(rn);
        for (size_t k = 0; k < rn; k++) { const csw::AnimFrame &f = frames[r0 + k]; px[k] = csp_pixels{d_rects.p + f.out_off, f.ow, f.oh, lossless ? 4u : 3u}; out[k].data = nullptr; out[k].length = 0; res[k] = make_result(0, nullptr); }
        if (lossless) csl_encode_pixels(px.data(), rn, device, out.data(), res.data());
        else {
            csh_batch *jb = nullptr;
            int rc = csh_batch_create_webp_from_pixels(px.data(), rn, p, device, &jb);
            if (rc == 0) rc = csh_batch_run(jb, nullptr);
            if (rc == 0 && csh_batch_fetch(jb, out.data(), res.data()) < 0) rc = CS_ERR_NO_DEVICE;
            csh_batch_destroy(jb);
            if (rc) for (size_t k = 0; k < rn; k++) { cs_free_bytes(&out[k]); cs_free_result(&res[k]); res[k] = make_result(uint32_t(rc), csh_last_error()); }
            // the alpha plane of a rectangle that is not opaque: the VP8L coder over it as a grey picture, into an ALPH chunk in front of the frame
            std::vector<csp_pixels> apx;
            std::vector<size_t> aat;
            for (size_t k = 0; k < rn; k++)
                if (out[k].data && stats[(r0 + k) * csw::ANIM_STAT + 6]) { const csw::AnimFrame &f = frames[r0 + k]; apx.push_back(csp_pixels{d_rects.p + f.a_off, f.ow, f.oh, 1}); aat.push_back(k); }
            if (!apx.empty()) route::attach_alpha_planes(apx, aat, out.data(), res.data(), device);   // (a frame that fails here fails its file below)
        }
        for (size_t k = 0; k < rn; k++) {
            Chunks &c = coded[r0 + k];
            if (!out[k].data || out[k].length < 20) { code[r0 + k] = res[k].code ? int(res[k].code) : CS_ERR_NO_DEVICE; why[r0 + k] = res[k].error_message ? res[k].error_message : "frame coder failed"; }
            else {   // the file's chunks behind its RIFF header (and behind the VP8X chunk csl_attach_alpha puts in front of ALPH)
                const size_t skip = !memcmp(out[k].data + 12, "VP8X", 4) ? 30 : 12;
                c.bytes.assign(out[k].data + skip, out[k].data + out[k].length);
                if (c.bytes.size() & 1) c.bytes.push_back(0);
                c.alpha = stats[(r0 + k) * csw::ANIM_STAT + 6] != 0;
            }
            cs_free_bytes(&out[k]); cs_free_result(&res[k]);
        }
    }
    // the files: RIFF, VP8X, [ICCP], ANIM, the ANMF chunks, [EXIF]
    int failed = 0;
    for (size_t j = 0; j < nfiles; j++) {
        const size_t at = files[j];
        const cswd_anim &a = b->anims[size_t(b->items[at].anim)];
        const csw::AnimFile &F = afiles[j];
        outputs[at].data = nullptr; outputs[at].length = 0;
        int bad = 0;
        const char *bad_msg = "";
        bool alpha = false;
        size_t total = 12 + 18 + 14;
        for (uint32_t k = 0; k < F.nframes; k++) {
            if (code[F.first + k] && !bad) { bad = code[F.first + k]; bad_msg = why[F.first + k].c_str(); }
            alpha |= coded[F.first + k].alpha;
            total += 8 + 16 + coded[F.first + k].bytes.size();
        }
        if (bad) { results[at] = make_result(uint32_t(bad), bad_msg); failed++; continue; }
        // what a still picture keeps under keep_metadata (route_webp.cpp): the source's ICC profile and EXIF, not its XMP
        const riff::Metadata md = p->keep_metadata ? riff::find_metadata(sources[at].data, sources[at].length) : riff::Metadata();
        total += md.bytes();
        if (total > 0xFFFFFFF0ull) { results[at] = make_result(CS_ERR_UNSUPPORTED, "animated WebP output beyond the RIFF size field"); failed++; continue; }
        uint8_t *o = static_cast<uint8_t *>(malloc(total));
        if (!o) { results[at] = make_result(CS_ERR_NO_DEVICE, "out of memory"); failed++; continue; }
        uint8_t *w = riff::write_vp8x(riff::write_header(o, total), uint8_t(0x02 | (alpha ? 0x10 : 0) | md.vp8x_flags()), a.cw, a.ch);
        if (md.icc) w = riff::append_chunk(w, "ICCP", md.icc, md.icc_len);
        memcpy(w, "ANIM", 4); wr32(w + 4, 6); wr32(w + 8, a.background); w[12] = uint8_t(a.loops); w[13] = uint8_t(a.loops >> 8); w += 14;
        for (uint32_t k = 0; k < F.nframes; k++) {
            const csw::AnimFrame &f = frames[F.first + k];
            const std::vector<uint8_t> &c = coded[F.first + k].bytes;   // whole chunks, padded to even
            memcpy(w, "ANMF", 4); wr32(w + 4, uint32_t(16 + c.size()));
            wr24(w + 8, f.ox / 2); wr24(w + 11, f.oy / 2); wr24(w + 14, f.ow - 1); wr24(w + 17, f.oh - 1); wr24(w + 20, a.duration[k]);
            w[23] = (f.flags & csw::ANIM_HOLES) ? 0x00 : 0x02;   // blend only in the blend form; dispose to none
            memcpy(w + 24, c.data(), c.size());
            w += 24 + c.size();
        }
        if (md.exif) riff::append_chunk(w, "EXIF", md.exif, md.exif_len);
        outputs[at].data = o; outputs[at].length = total;
        results[at] = make_result(0, nullptr);
    }
    return failed;
}
