// vp8l_encode.cpp -- lossless WebP OUTPUT of the batch queue (webp.lossless; libcaesium's webp::compress with libwebp's lossless coder,
// /root/reference/src/compressor.rs:427-429 and 289-305): pixels that are already in device memory -> one VP8L file each
// (k_vp8l_enc.hip).  Sources are the decoders of this library (WebP inputs: webp_decode.cpp; JPEG inputs: the pixel tap of the JPEG row).
#include <cstring>
#include <vector>

#include "devmem.hpp"
#include "riff.h"
#include "routes.hpp"
#include "webp_kernels.h"

using namespace csh;

extern "C" int csl_encode_pixels(const csp_pixels *px, size_t count, int device, CByteArray *outputs, CCSResult *results) {
    for (size_t i = 0; i < count; i++) { outputs[i].data = nullptr; outputs[i].length = 0; }
    if (csh_device_count() <= device || hipSetDevice(device) != hipSuccess) {
        for (size_t i = 0; i < count; i++) results[i] = make_result(CS_ERR_NO_DEVICE, "no HIP device available (libcaesium_hip has no CPU path)");
        return int(count);
    }
    // the coder, read on every call: unset / empty / "plain" = literals only (the bytes oracle/png_oracle.c cso_vp8l_encode states), "refs" = backward
    // references and a colour cache (k_vp8l_refs.hip), "palette" = refs, and for a picture of at most 256 colours the colour-indexing transform where that is
    // smaller (k_vp8l_palette.hip), "groups" = palette, and for every picture of more than one tile its refs stream with a set of codes per group of tiles where that
    // is smaller (k_vp8l_groups.hip), "far" = groups, and for every record a second token set from a match finder over the whole window where that is smaller
    // (k_vp8l_far.hip)
    const char *mode = getenv("CSH_VP8L");
    const bool far = mode && !strcmp(mode, "far");
    const bool groups = far || (mode && !strcmp(mode, "groups"));
    const bool palette = groups || (mode && !strcmp(mode, "palette"));
    const bool refs = palette || (mode && !strcmp(mode, "refs"));
    if (mode && *mode && !refs && strcmp(mode, "plain")) {
        for (size_t i = 0; i < count; i++) results[i] = make_result(CS_ERR_UNSUPPORTED, "CSH_VP8L names no lossless WebP coder (plain, refs, palette, groups, far)");
        return int(count);
    }
    int failed = 0;
    std::vector<csw::Vp8lImg> imgs;
    std::vector<size_t> at;
    uint64_t work = 0, modes = 0, out = 0, max_px = 0, cst = 0;
    uint32_t max_blocks = 0;
    for (size_t i = 0; i < count; i++) {
        const uint32_t ch = px[i].channels;
        if (!((ch >= 1 && ch <= 4) || ch == csw::VP8L_ALPHA_OF + 2 || ch == csw::VP8L_ALPHA_OF + 4) || !px[i].width || !px[i].height || px[i].width > 16384 || px[i].height > 16384) {
            results[i] = make_result(CS_ERR_UNSUPPORTED, "lossless WebP output takes 8-bit grey / RGB pictures, with or without alpha, of at most 16384 x 16384"); failed++; continue;
        }
        csw::Vp8lImg im;
        memset(&im, 0, sizeof im);
        im.rgb = px[i].device_pixels; im.width = px[i].width; im.height = px[i].height; im.channels = px[i].channels;
        im.bw = (im.width + 15) / 16; im.bh = (im.height + 15) / 16;
        const uint64_t npx = uint64_t(im.width) * im.height;
        im.res_off = work; work += (npx + 63) & ~uint64_t(63);
        im.mode_off = modes; modes += (uint64_t(im.bw) * im.bh + 63) & ~uint64_t(63);
        const uint64_t cap = 8 * npx + 2 * uint64_t(im.bw) * im.bh + 8192;   // four codes of at most 15 bits per pixel, the mode image, the code descriptions
        if (cap > 0xFFFFFFF0ull) { results[i] = make_result(CS_ERR_UNSUPPORTED, "picture too large for one lossless WebP batch item"); failed++; continue; }
        im.out_off = out; im.out_cap = uint32_t(cap); out += (cap + 255) & ~uint64_t(255);   // (the refs stream is written only where it is the smaller one)
        if (refs) {
            im.nchunk = uint32_t((npx + csw::VP8L_CHUNK - 1) / csw::VP8L_CHUNK);
            im.tok_off = im.res_off; im.hit_off = im.res_off;   // one entry per pixel, like the residuals
            im.cst_off = cst; cst += uint64_t(im.nchunk) * csw::VP8L_CACHE_STATE;
        }
        max_px = std::max(max_px, npx); max_blocks = std::max(max_blocks, im.bw * im.bh);
        imgs.push_back(im); at.push_back(i);
    }
    if (imgs.empty()) return failed;
    hipStream_t st = 0;
    bool have_st = false;
    DevBuf<csw::Vp8lImg> d_imgs;
    DevBuf<uint32_t> d_work, d_hist, d_len, d_status;
    DevBuf<uint8_t> d_modes, d_out, d_hit, d_lens;
    DevBuf<uint64_t> d_tok, d_cst;
    DevBuf<uint32_t> d_rhist, d_pick, d_pcount, d_pal;
    DevBuf<unsigned long long> d_ptab, d_ginfo;
    DevBuf<csw::Vp8lGroupImg> d_gimg;
    DevBuf<uint32_t> d_feat, d_ghist;
    DevBuf<uint8_t> d_label, d_glens;
    DevBuf<uint64_t> d_tok2;
    DevBuf<uint32_t> d_pos0, d_pos1, d_prev, d_cnt, d_dtot, d_won, d_rhist2, d_pick2, d_feat2, d_ghist2;
    DevBuf<uint8_t> d_lens2, d_label2, d_glens2;
    DevBuf<unsigned long long> d_ginfo2;
    std::vector<uint32_t> len(imgs.size()), status(imgs.size());
    bool ok = hipStreamCreateWithFlags(&st, hipStreamNonBlocking) == hipSuccess;
    have_st = ok;
    // palette: the colours of every picture are counted first, and the one read-back of the counts (4 bytes per picture) decides which pictures get a candidate
    // record and pools of their own, behind the pictures'
    const size_t nparent = imgs.size();
    uint64_t max_packed = 0;
    if (ok && palette) {
        std::vector<uint32_t> pcount(nparent);
        ok = !d_imgs.upload(imgs, st) && !d_ptab.alloc(nparent * csw::VP8L_PAL_SLOTS + 8) && !d_ptab.zero(st) && !d_pcount.alloc(nparent + 1) && !d_pcount.zero(st);
        if (ok) {
            csw::launch_vp8l_pal_count(st, d_imgs.p, int(nparent), max_px, d_ptab.p, d_pcount.p);
            ok = csh_copy_wait(pcount.data(), d_pcount.p, nparent * sizeof(uint32_t), hipMemcpyDeviceToHost, st) == hipSuccess && hipGetLastError() == hipSuccess;
        }
        for (size_t k = 0; ok && k < nparent; k++) {
            if (pcount[k] < 1 || pcount[k] > csw::VP8L_PAL_MAX) continue;
            csw::Vp8lImg im = imgs[k];
            im.pal_n = pcount[k]; im.parent = uint32_t(k); im.src_width = im.width;
            im.width = (im.width + (1u << csw::vp8l_pal_bits(im.pal_n)) - 1) >> csw::vp8l_pal_bits(im.pal_n);
            im.bw = im.bh = 0; im.mode_off = 0;
            const uint64_t npx = uint64_t(im.width) * im.height;
            im.res_off = work; work += (npx + 63) & ~uint64_t(63);
            im.nchunk = uint32_t((npx + csw::VP8L_CHUNK - 1) / csw::VP8L_CHUNK);
            im.tok_off = im.res_off; im.hit_off = im.res_off;
            im.cst_off = cst; cst += uint64_t(im.nchunk) * csw::VP8L_CACHE_STATE;
            max_packed = std::max(max_packed, npx);
            imgs.push_back(im);
        }
        const size_t ncand = imgs.size() - nparent;
        ok = ok && !d_pal.alloc(ncand * csw::VP8L_PAL_BLOCK + 8);
        for (size_t k = 0; ok && k < ncand; k++) imgs[nparent + k].pal = d_pal.p + k * csw::VP8L_PAL_BLOCK;
    }
    ok = ok && !d_imgs.upload(imgs, st) && !d_work.alloc(work + 64) && !d_hist.alloc(imgs.size() * 1024 + 8) && !d_hist.zero(st) && !d_len.alloc(imgs.size() + 1) && !d_status.alloc(imgs.size() + 1) &&
         !d_modes.alloc(modes + 64) && !d_out.alloc(out + 256);
    if (ok && refs)
        ok = !d_tok.alloc(work + 64) && !d_hit.alloc(work + 64) && !d_cst.alloc(cst + 64) && !d_rhist.alloc(imgs.size() * csw::VP8L_NOPT * csw::VP8L_HIST + 8) && !d_rhist.zero(st) &&
             !d_lens.alloc(imgs.size() * csw::VP8L_LENS + 8) && !d_pick.alloc(imgs.size() * 4 + 4);
    // groups: the pictures' tiles (a picture of one tile has no grouped candidate) and the pools behind them, in this mode only
    uint32_t max_tiles = 0;
    uint64_t tiles = 0;
    if (ok && groups) {
        std::vector<csw::Vp8lGroupImg> gimgs(nparent);
        for (size_t k = 0; k < nparent; k++) {
            csw::Vp8lGroupImg &g = gimgs[k];
            const uint32_t b = csw::vp8l_group_bits(imgs[k].width, imgs[k].height);
            g.tw = (imgs[k].width + (1u << b) - 1) >> b; g.th = (imgs[k].height + (1u << b) - 1) >> b; g.ntile = g.tw * g.th;
            g.bits = g.ntile > 1 ? b : 0u;
            g.tile_off = tiles; tiles += (g.ntile + 63) & ~uint64_t(63);
            if (g.bits) max_tiles = std::max(max_tiles, g.ntile);
        }
        ok = !d_gimg.upload(gimgs, st) && !d_label.alloc(tiles + 64) && !d_feat.alloc(tiles * csw::VP8L_TILE_FEAT + 64) &&
             !d_ghist.alloc(nparent * csw::VP8L_MAX_GROUPS * csw::VP8L_HIST + 8) && !d_ghist.zero(st) && !d_glens.alloc(nparent * csw::VP8L_MAX_GROUPS * csw::VP8L_LENS + 8) &&
             !d_ginfo.alloc(nparent * csw::VP8L_GROUP_INFO + 8) && !d_ginfo.zero(st);
    }
    // far: the sort's two position arrays and the links (12 bytes per pixel), the digit counts (a word per 16 pixels), and a second set of every pool that depends
    // on tokens (8 bytes per pixel and the per-record tables), in this mode only
    if (ok && far)
        ok = !d_pos0.alloc(work + 64) && !d_pos1.alloc(work + 64) && !d_prev.alloc(work + 64) && !d_cnt.alloc(cst / csw::VP8L_CACHE_STATE * 256 + 256) &&
             !d_dtot.alloc(imgs.size() * csw::VP8L_FAR_TOT + 8) && !d_dtot.zero(st) && !d_won.alloc(imgs.size() + 1) && !d_tok2.alloc(work + 64) &&
             !d_rhist2.alloc(imgs.size() * csw::VP8L_NOPT * csw::VP8L_HIST + 8) && !d_rhist2.zero(st) && !d_lens2.alloc(imgs.size() * csw::VP8L_LENS + 8) && !d_pick2.alloc(imgs.size() * 4 + 4) &&
             !d_label2.alloc(tiles + 64) && !d_feat2.alloc(tiles * csw::VP8L_TILE_FEAT + 64) && !d_ghist2.alloc(nparent * csw::VP8L_MAX_GROUPS * csw::VP8L_HIST + 8) && !d_ghist2.zero(st) &&
             !d_glens2.alloc(nparent * csw::VP8L_MAX_GROUPS * csw::VP8L_LENS + 8) && !d_ginfo2.alloc(nparent * csw::VP8L_GROUP_INFO + 8) && !d_ginfo2.zero(st);
    if (ok) {
        const csw::Vp8lRefs pools = {d_tok.p, d_hit.p, d_cst.p, d_rhist.p, d_lens.p, d_pick.p, d_gimg.p, d_label.p, d_feat.p, d_ghist.p, d_glens.p, d_ginfo.p};
        if (far) {
            const csw::Vp8lFar fp = {{d_pos0.p, d_pos1.p}, d_prev.p, d_cnt.p, d_dtot.p, d_won.p,
                                     {d_tok2.p, d_hit.p, d_cst.p, d_rhist2.p, d_lens2.p, d_pick2.p, d_gimg.p, d_label2.p, d_feat2.p, d_ghist2.p, d_glens2.p, d_ginfo2.p}};
            csw::launch_vp8l_encode_far(st, d_imgs.p, int(nparent), int(imgs.size() - nparent), max_blocks, max_px, max_packed, max_tiles, d_ptab.p, d_pal.p, d_work.p, d_modes.p, d_hist.p, pools, fp,
                                        d_out.p, d_len.p, d_status.p);
        } else if (groups)
            csw::launch_vp8l_encode_groups(st, d_imgs.p, int(nparent), int(imgs.size() - nparent), max_blocks, max_px, max_packed, max_tiles, d_ptab.p, d_pal.p, d_work.p, d_modes.p, d_hist.p,
                                           pools, d_out.p, d_len.p, d_status.p);
        else if (palette)
            csw::launch_vp8l_encode_palette(st, d_imgs.p, int(nparent), int(imgs.size() - nparent), max_blocks, max_px, max_packed, d_ptab.p, d_pal.p, d_work.p, d_modes.p, d_hist.p, pools, d_out.p,
                                            d_len.p, d_status.p);
        else if (refs)
            csw::launch_vp8l_encode_refs(st, d_imgs.p, int(imgs.size()), max_blocks, max_px, d_work.p, d_modes.p, d_hist.p, pools, d_out.p, d_len.p, d_status.p);
        else
            csw::launch_vp8l_encode(st, d_imgs.p, int(imgs.size()), max_blocks, max_px, d_work.p, d_modes.p, d_hist.p, d_out.p, d_len.p, d_status.p);
        ok = hipMemcpyAsync(len.data(), d_len.p, len.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, st) == hipSuccess &&
             hipMemcpyAsync(status.data(), d_status.p, status.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, st) == hipSuccess && hipStreamSynchronize(st) == hipSuccess && hipGetLastError() == hipSuccess;
    }
    for (size_t k = 0; k < nparent; k++) {
        const size_t i = at[k];
        if (!ok) { results[i] = make_result(CS_ERR_NO_DEVICE, "lossless WebP coding failed on the device"); failed++; continue; }
        if (status[k] || !len[k]) { results[i] = make_result(CS_ERR_POOL_OVERFLOW, "lossless WebP output larger than its region"); failed++; continue; }
        outputs[i].data = static_cast<uint8_t *>(malloc(len[k]));
        if (!outputs[i].data || csh_copy_wait(outputs[i].data, d_out.p + imgs[k].out_off, len[k], hipMemcpyDeviceToHost, st) != hipSuccess) {
            free(outputs[i].data); outputs[i].data = nullptr; results[i] = make_result(CS_ERR_NO_DEVICE, "D2H failed"); failed++; continue;
        }
        outputs[i].length = len[k];
        results[i] = make_result(0, nullptr);
    }
    if (have_st) { (void)hipStreamSynchronize(st); (void)hipStreamDestroy(st); }   // nothing queued may outlive the device blocks
    return failed;
}

// A lossy file and its alpha plane as a VP8L file (csl_encode_pixels over the plane as a grey picture) -> the extended-format file libwebp writes for a picture with
// transparency: VP8X (alpha flag, canvas size), ALPH (one header byte: lossless compression, no filter, no pre-processing; then the VP8L stream without its five
// header bytes -- signature and sizes, which ALPH implies; its green channel is the alpha), the VP8 frame.  lossy is replaced; 0 ok.
extern "C" int csl_attach_alpha(CByteArray *lossy, const CByteArray *alpha_vp8l, uint32_t width, uint32_t height) {
    if (!lossy || !lossy->data || lossy->length < 30 || memcmp(lossy->data + 12, "VP8 ", 4) || !alpha_vp8l || !alpha_vp8l->data || alpha_vp8l->length < 26 || memcmp(alpha_vp8l->data + 12, "VP8L", 4)) return -1;
    const uint8_t *a = alpha_vp8l->data;
    const size_t pl = riff::rd32(a + 16);
    if (pl < 5 || 20 + pl > alpha_vp8l->length) return -1;
    const size_t vp8 = lossy->length - 12, apay = pl - 5, alph = 1 + apay, total = 12 + 18 + 8 + alph + (alph & 1) + vp8;
    uint8_t *o = static_cast<uint8_t *>(malloc(total));
    if (!o) return -1;
    uint8_t *w = riff::write_vp8x(riff::write_header(o, total), 0x10, width, height);
    memcpy(w, "ALPH", 4); riff::wr32(w + 4, uint32_t(alph)); w[8] = 0x01; memcpy(w + 9, a + 25, apay); w += 8 + alph;   // (no append_chunk: the payload is put together in place)
    if (alph & 1) *w++ = 0;
    memcpy(w, lossy->data + 12, vp8);
    free(lossy->data);
    lossy->data = o; lossy->length = total;
    return 0;
}

int route::attach_alpha_planes(const std::vector<csp_pixels> &planes, const std::vector<size_t> &whose, CByteArray *outs, CCSResult *results, int device) {
    std::vector<CByteArray> aout(planes.size());
    std::vector<CCSResult> ares(planes.size());
    csl_encode_pixels(planes.data(), planes.size(), device, aout.data(), ares.data());
    int failed = 0;
    for (size_t j = 0; j < planes.size(); j++) {
        const size_t k = whose[j];
        if (!aout[j].data || csl_attach_alpha(&outs[k], &aout[j], planes[j].width, planes[j].height)) {
            cs_free_bytes(&outs[k]); cs_free_result(&results[k]);
            results[k] = make_result(ares[j].code ? ares[j].code : CS_ERR_NO_DEVICE, "alpha plane coder failed"); failed++;
        }
        cs_free_bytes(&aout[j]); cs_free_result(&ares[j]);
    }
    return failed;
}
