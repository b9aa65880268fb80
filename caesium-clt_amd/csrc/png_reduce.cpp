// png_reduce.cpp -- P2 of the PNG batch: which reductions the pixels allow (device), the new geometry and IHDR (host), the repack (device).
// One host round trip per batch; afterwards every later stage sees the reduced image as if it had come in that way.
// Statement: oracle/png_oracle.c (to_palette, quantize, grey_depth, index_depth).
#include <algorithm>
#include <cstring>

#include "../../include/png_quality_table.h"
#include "png_batch.hpp"

namespace csp {
namespace {

using csh::DevBuf;

// what the analysis kernels found, per image
struct Analysis {
    std::vector<uint32_t> flags, status, counts, used;   // used: 8 words per image, one bit per palette index an indexed image uses
    explicit Analysis(int nimg) : flags(nimg), status(nimg), counts(nimg), used(size_t(nimg) * 8, 0) {}
};
typedef std::map<int, std::vector<uint32_t>> Palettes;   // image -> its sorted ARGB entries

// the device analysis and its read-back
int analyze(csp_batch *b, Analysis &A) {
    hipStream_t st = b->stream;
    const int nimg = int(b->imgs.size());
    if (b->d_keys.alloc(size_t(nimg) * CSP_PAL_SLOTS) || b->d_slot_index.alloc(size_t(nimg) * CSP_PAL_SLOTS) || b->d_counts.alloc(size_t(nimg) + 1) || b->d_cand.upload(b->cand0, st)) return -1;
    if (hipMemcpyAsync(b->d_flags.p, b->flags0.data(), sizeof(uint32_t) * nimg, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemsetAsync(b->d_keys.p, 0xFF, sizeof(unsigned long long) * size_t(nimg) * CSP_PAL_SLOTS, st) != hipSuccess || b->d_counts.zero(st)) return -1;
    launch_png_analyze(st, b->d_imgs.p, b->total_rows, b->d_row_image.p, b->d_work.p, b->d_flags.p, b->d_status.p);
    launch_png_colors(st, b->d_imgs.p, b->total_rows, b->d_row_image.p, b->d_work.p, b->d_cand.p, b->d_keys.p, b->d_counts.p, b->d_status.p);
    bool any_indexed = false;
    for (int i = 0; i < nimg; i++) any_indexed |= (b->flags0[i] & 64u) != 0;
    DevBuf<uint32_t> d_used;
    if (any_indexed) {
        if (d_used.alloc(size_t(nimg) * 8) || d_used.zero(st)) return -1;
        launch_png_used(st, b->d_imgs.p, b->total_rows, b->d_row_image.p, b->d_work.p, b->d_flags.p, d_used.p, b->d_status.p);
        if (hipMemcpyAsync(A.used.data(), d_used.p, sizeof(uint32_t) * A.used.size(), hipMemcpyDeviceToHost, st) != hipSuccess) return -1;
    }
    if (hipMemcpyAsync(A.flags.data(), b->d_flags.p, sizeof(uint32_t) * nimg, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipMemcpyAsync(A.counts.data(), b->d_counts.p, sizeof(uint32_t) * nimg, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipMemcpyAsync(A.status.data(), b->d_status.p, sizeof(uint32_t) * nimg, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
        csh_set_error("PNG analysis failed");
        return -1;
    }
    return 0;
}

// the median cut of one group of images (10 MB of bins each): bins counted and compacted, one workgroup per image over the non-empty bins
// (k_png_mediancut); the host only sorts the <= 256 entries and merges equal ones
int median_cut_group(csp_batch *b, std::vector<QuantJob> &part, uint32_t qmax_h, Palettes &qpal) {
    hipStream_t st = b->stream;
    const size_t gn = part.size();
    uint64_t lt = 0;
    for (size_t k = 0; k < gn; k++) { part[k].bins_off = uint64_t(k) * CSP_QBINS * 5; part[k].list_off = lt; lt += std::min<uint64_t>(uint64_t(part[k].width) * part[k].height, CSP_QBINS); }
    if (b->d_qbins.alloc(gn * size_t(CSP_QBINS) * 5) || b->d_qbins.zero(st) || b->d_qlist.alloc(lt + 1) || b->d_qn.alloc(gn + 1) || b->d_qn.zero(st) || b->d_qjobs.upload(part, st)) return -1;
    launch_png_qhist(st, b->d_qjobs.p, int(gn), qmax_h, b->d_work.p, b->d_qbins.p);
    launch_png_qcompact(st, b->d_qjobs.p, int(gn), b->d_qbins.p, b->d_qlist.p, b->d_qn.p);
    DevBuf<uint32_t> d_qord, d_cutpal, d_ncut;
    DevBuf<uint4> d_qrec;
    if (d_qrec.alloc(lt + 1) || d_qord.alloc(2 * (lt + 1)) || d_cutpal.alloc(gn * 256) || d_ncut.alloc(gn)) return -1;
    const int q = b->png_quality < 0 ? 0 : b->png_quality > 100 ? 100 : b->png_quality;
    launch_png_mediancut(st, b->d_qjobs.p, int(gn), b->d_qlist.p, b->d_qn.p, d_qrec.p, d_qord.p, lt + 1, q, kQualityBound[q], d_cutpal.p, d_ncut.p);
    std::vector<uint32_t> cutpal(gn * 256), ncut(gn);
    if (csh_copy_wait(cutpal.data(), d_cutpal.p, sizeof(uint32_t) * gn * 256, hipMemcpyDeviceToHost, st) != hipSuccess ||
        csh_copy_wait(ncut.data(), d_ncut.p, sizeof(uint32_t) * gn, hipMemcpyDeviceToHost, st) != hipSuccess || hipGetLastError() != hipSuccess) return -1;
    for (size_t k = 0; k < gn; k++) {
        std::vector<uint32_t> cut(cutpal.begin() + k * 256, cutpal.begin() + k * 256 + std::min<uint32_t>(ncut[k], 256));
        std::sort(cut.begin(), cut.end());
        cut.erase(std::unique(cut.begin(), cut.end()), cut.end());
        qpal[int(part[k].image)] = std::move(cut);
    }
    return 0;
}

// lossy: truecolour images that keep more than 256 colours after the lossless reductions get a palette from the median cut (a second round trip
// for the <= 256 palette entries, only for such images), a few images at a time
int lossy_palettes(csp_batch *b, const Analysis &A, Palettes &qpal) {
    std::vector<QuantJob> qjobs;
    uint32_t qmax_h = 0;
    for (int i = 0; i < int(b->imgs.size()); i++) {
        if (A.status[i] || !b->cand0[i] || (A.flags[i] & 4u) || A.counts[i] <= 256) continue;
        const PngImg &im = b->imgs[i];
        QuantJob q{};
        q.image = uint32_t(i); q.channels = im.channels; q.bps = im.bps; q.rowbytes = im.rowbytes; q.width = im.width; q.height = im.height; q.src_off = im.pix_off;
        qmax_h = std::max(qmax_h, im.height);
        qjobs.push_back(q);
    }
    for (size_t g0 = 0; g0 < qjobs.size(); g0 += 64) {
        std::vector<QuantJob> part(qjobs.begin() + g0, qjobs.begin() + g0 + std::min<size_t>(64, qjobs.size() - g0));
        if (median_cut_group(b, part, qmax_h, qpal)) return -1;
    }
    return 0;
}

// what the flags leave of an image's samples
struct Samples { uint32_t nk, nbps; bool grey; };   // channels, bytes per sample, colour -> grey

// colour -> palette (oracle: to_palette): at most 256 distinct pixels, and smaller rows even with the PLTE / tRNS chunks; lossy: what is still
// truecolour is quantised (oracle: quantize) with the palette the median cut made.  depth 0: stays as it is
struct ToPalette {
    uint32_t depth = 0, ntr = 0;
    bool nearest = false;                    // quantised: nearest entry with error diffusion, not an exact lookup
    std::vector<uint32_t> pal;               // sorted ARGB entries
    std::vector<unsigned long long> tab;     // the colour table of k_png_colors (exact lookup only)
};
int decide_palette(csp_batch *b, int i, const Analysis &A, const Samples &s, const Palettes &qpal, ToPalette &d) {
    const PngImg &im = b->imgs[i];
    if (b->cand0[i] && !s.grey && s.nbps == 1 && (s.nk == 3 || s.nk == 4) && A.counts[i] <= 256) {
        d.tab.resize(CSP_PAL_SLOTS);
        if (csh_copy_wait(d.tab.data(), b->d_keys.p + size_t(i) * CSP_PAL_SLOTS, sizeof(unsigned long long) * CSP_PAL_SLOTS, hipMemcpyDeviceToHost, b->stream) != hipSuccess) return -1;
        for (auto k : d.tab) if (k != ~0ull) d.pal.push_back(uint32_t(k));
        std::sort(d.pal.begin(), d.pal.end());
        const uint32_t n = uint32_t(d.pal.size());
        d.ntr = leading_transparent(d.pal);
        d.depth = palette_depth(n);
        const uint64_t nrb = (uint64_t(im.width) * d.depth + 7) / 8, extra = 12 + 3 * uint64_t(n) + (d.ntr ? 12 + d.ntr : 0);
        if (uint64_t(im.height) * (1 + nrb) + extra >= uint64_t(im.height) * (1 + uint64_t(im.width) * s.nk)) d.depth = 0;
    }
    const auto q = qpal.find(i);
    if (!d.depth && q != qpal.end()) {
        d.pal = q->second;
        d.ntr = leading_transparent(d.pal);
        d.depth = palette_depth(uint32_t(d.pal.size()));
        d.nearest = true;
    }
    return 0;
}

// 8-bit grey -> 4 / 2 / 1 bit (oracle: grey_depth): the result is a single 8-bit channel whose every level fits
uint32_t decide_grey_depth(uint32_t flags, const Samples &s) {
    if (s.nk != 1 || s.nbps != 1) return 0;
    return (flags & 32u) ? 1u : (flags & 16u) ? 2u : (flags & 8u) ? 4u : 0u;
}

// an 8-bit indexed image that does not use its whole palette: the unused entries go, the rest is renumbered and packed at the depth it needs
// (oracle: index_depth).  The entries that stay: one per distinct colour among the used ones, those that are not opaque in front of the opaque ones
struct IndexedRepack {
    uint32_t depth = 0, nused = 0;
    uint8_t imap[256], iorder[256];   // old index -> new; new index -> the old one it keeps
};
IndexedRepack decide_indexed(const PngItem &it, const uint32_t *used) {
    IndexedRepack d;
    const uint32_t npl = uint32_t(it.plte.size() / 3);
    bool ok = true;
    int first_of[256];
    uint32_t col[256];
    auto is_used = [&](uint32_t v) { return ((used[v >> 5] >> (v & 31u)) & 1u) != 0; };
    for (uint32_t v = 0; v < 256; v++) {
        first_of[v] = -1; d.imap[v] = 0;
        if (!is_used(v)) continue;
        if (v >= npl) { ok = false; continue; }
        col[v] = (uint32_t(v < it.trns.size() ? it.trns[v] : 255) << 24) | (uint32_t(it.plte[3 * v]) << 16) | (uint32_t(it.plte[3 * v + 1]) << 8) | it.plte[3 * v + 2];
        first_of[v] = int(v);
        for (uint32_t k = 0; k < v; k++) if (first_of[k] == int(k) && col[k] == col[v]) { first_of[v] = int(k); break; }
    }
    for (int pass = 0; pass < 2 && ok; pass++)
        for (uint32_t v = 0; v < 256; v++)
            if (first_of[v] == int(v) && ((col[v] >> 24) != 255) == (pass == 0)) { d.imap[v] = uint8_t(d.nused); d.iorder[d.nused++] = uint8_t(v); }
    for (uint32_t v = 0; v < 256 && ok; v++) if (first_of[v] >= 0 && first_of[v] != int(v)) d.imap[v] = d.imap[first_of[v]];
    d.depth = palette_depth(d.nused);
    if (!ok || !d.nused || (d.depth == 8 && d.nused == npl)) d.depth = 0;
    return d;
}

// the jobs and tables of the batch's reductions, in image order: the kernels index them
struct Reduction {
    std::vector<ReduceJob> jobs;
    std::vector<uint8_t> remaps;   // 256 bytes per indexed job: old palette index -> new
    std::vector<PaletteJob> pjobs;
    uint64_t dither_pixels = 0, dither_steps = 0;   // k_png_dither: line-buffer pixels of the quantised images, the longest image's steps
    std::vector<uint32_t> palettes;
    std::vector<uint16_t> slot_index;
    uint32_t max_height = 0;
    explicit Reduction(int nimg) : slot_index(size_t(nimg) * CSP_PAL_SLOTS, 0) {}
};

// an image becomes indexed: its job, its place in the palette tables, the new geometry, IHDR, PLTE and (if some entry is not opaque) tRNS
void apply_palette(int i, const ToPalette &d, PngImg &im, PngItem &it, Reduction &R) {
    PaletteJob j{};
    j.image = uint32_t(i); j.old_rowbytes = im.rowbytes; j.old_channels = im.channels; j.old_bps = im.bps; j.depth = d.depth; j.table = uint32_t(i);
    j.src_off = im.pix_off; j.dst_off = im.raw_off;
    j.nearest = d.nearest ? 2u : 0u; j.npal = uint32_t(d.pal.size()); j.pal_off = uint32_t(R.palettes.size());   // (2: with error diffusion, k_png_dither)
    if (d.nearest) {
        j.line_off = uint32_t(R.dither_pixels); R.dither_pixels += 2 * uint64_t(im.width);
        const uint64_t steps = uint64_t((im.height + CSP_DITHER_ROWS - 1) / CSP_DITHER_ROWS) * (uint64_t(im.width) + 2 * CSP_DITHER_ROWS);
        R.dither_steps = std::max(R.dither_steps, steps);
        R.palettes.insert(R.palettes.end(), d.pal.begin(), d.pal.end());
    }
    for (uint32_t sl = 0; sl < CSP_PAL_SLOTS && !d.nearest; sl++)
        if (d.tab[sl] != ~0ull) R.slot_index[size_t(i) * CSP_PAL_SLOTS + sl] = uint16_t(std::lower_bound(d.pal.begin(), d.pal.end(), uint32_t(d.tab[sl])) - d.pal.begin());
    im.channels = 1; im.bps = 0; im.bpp = 1; im.rowbytes = uint32_t((uint64_t(im.width) * d.depth + 7) / 8);
    set_ihdr_format(it.prefix, d.depth, 3);
    const uint32_t n = uint32_t(d.pal.size());
    std::vector<uint8_t> rgb(3 * size_t(n)), alpha(d.ntr);
    for (uint32_t k = 0; k < n; k++) { rgb[3 * k] = uint8_t(d.pal[k] >> 16); rgb[3 * k + 1] = uint8_t(d.pal[k] >> 8); rgb[3 * k + 2] = uint8_t(d.pal[k]); }
    for (uint32_t k = 0; k < d.ntr; k++) alpha[k] = uint8_t(d.pal[k] >> 24);
    append_chunk(it.prefix, "PLTE", rgb.data(), 3 * n);
    if (d.ntr) append_chunk(it.prefix, "tRNS", alpha.data(), d.ntr);
    R.pjobs.push_back(j);
}

// an indexed image is renumbered: its job and remap table, the new geometry and IHDR, and PLTE and tRNS of the entries that are left (a tRNS
// that ends up all opaque goes): the carried chunks behind IHDR, written again
void apply_indexed(int i, const IndexedRepack &d, PngImg &im, PngItem &it, Reduction &R) {
    ReduceJob j{};
    j.image = uint32_t(i); j.mask = 0; j.old_rowbytes = im.rowbytes; j.old_channels = 1; j.old_bps = 1;
    j.src_off = im.pix_off; j.dst_off = im.raw_off;
    j.gdepth = d.depth | 256u; j.remap = uint32_t(R.remaps.size() / 256);
    R.remaps.insert(R.remaps.end(), d.imap, d.imap + 256);
    im.bps = 0; im.bpp = 1; im.rowbytes = uint32_t((uint64_t(im.width) * d.depth + 7) / 8);
    std::vector<uint8_t> npl, ntr;
    uint32_t nt = 0;
    for (uint32_t k = 0; k < d.nused; k++) {
        const uint32_t v = d.iorder[k];
        npl.insert(npl.end(), it.plte.begin() + 3 * v, it.plte.begin() + 3 * v + 3);
        ntr.push_back(v < it.trns.size() ? it.trns[v] : uint8_t(255));
        if (ntr.back() != 255) nt = k + 1;
    }
    ntr.resize(nt);
    std::vector<uint8_t> np(it.prefix.begin(), it.prefix.begin() + 33);   // signature and IHDR
    for (size_t pos = 33; pos + 12 <= it.prefix.size();) {
        const uint32_t len = be32(&it.prefix[pos]);
        const char *type = reinterpret_cast<const char *>(&it.prefix[pos + 4]);
        if (!memcmp(type, "PLTE", 4)) append_chunk(np, type, npl.data(), uint32_t(npl.size()));
        else if (!memcmp(type, "tRNS", 4)) { if (nt) append_chunk(np, type, ntr.data(), nt); }
        else append_chunk(np, type, &it.prefix[pos + 8], len);
        pos += 12 + size_t(len);
    }
    it.prefix.swap(np);
    it.plte = npl; it.trns = ntr;
    set_ihdr_format(it.prefix, d.depth, 3);
    R.jobs.push_back(j);
}

// 16 -> 8 bits, alpha away, colour -> grey, grey depth: the job, the new geometry and IHDR
void apply_samples(int i, uint32_t mask, const Samples &s, uint32_t gdepth, PngImg &im, PngItem &it, Reduction &R) {
    ReduceJob j{};
    j.image = uint32_t(i); j.mask = mask; j.old_rowbytes = im.rowbytes; j.old_channels = im.channels; j.old_bps = im.bps;
    j.src_off = im.pix_off; j.dst_off = im.raw_off;   // the second region of the image takes the new pixels
    j.gdepth = gdepth;
    im.channels = s.nk; im.bps = s.nbps; im.bpp = s.nk * s.nbps; im.rowbytes = im.width * s.nk * s.nbps;
    if (gdepth) { im.bps = 0; im.bpp = 1; im.rowbytes = uint32_t((uint64_t(im.width) * gdepth + 7) / 8); }
    set_ihdr_format(it.prefix, gdepth ? gdepth : s.nbps * 8, s.nk == 1 ? 0 : s.nk == 2 ? 4 : s.nk == 3 ? 2 : 6);
    R.jobs.push_back(j);
}

// decides and applies the reduction of image i; *changed: the image has a job now
int reduce_image(csp_batch *b, int i, const Analysis &A, const Palettes &qpal, PngItem &it, Reduction &R, bool *changed) {
    PngImg &im = b->imgs[i];
    const uint32_t flags = A.flags[i];
    const bool narrow = flags & 1u, opaque = flags & 2u, grey = flags & 4u;
    const Samples s{im.channels - (opaque ? 1u : 0u) - (grey ? 2u : 0u), narrow ? 1u : im.bps, grey};
    ToPalette pal;
    if (decide_palette(b, i, A, s, qpal, pal)) return -1;
    const uint32_t gdepth = pal.depth ? 0u : decide_grey_depth(flags, s);
    const IndexedRepack idx = (flags & 64u) ? decide_indexed(it, &A.used[size_t(i) * 8]) : IndexedRepack();
    *changed = pal.depth || (flags & 7u) || gdepth || idx.depth;
    if (!*changed) return 0;
    if (pal.depth) apply_palette(i, pal, im, it, R);
    else if (idx.depth) apply_indexed(i, idx, im, it, R);
    else apply_samples(i, flags & 7u, s, gdepth, im, it, R);
    im.raw_len = uint64_t(im.height) * (uint64_t(im.rowbytes) + 1);
    im.nchunks = uint32_t((im.raw_len + CSP_CHUNK - 1) / CSP_CHUNK);
    std::swap(im.pix_off, im.raw_off);
    if (im.height > R.max_height) R.max_height = im.height;
    return 0;
}

// prefixes changed (IHDR, perhaps PLTE / tRNS): the carried bytes laid out again, everything uploaded, the repack kernels, the chunk index
int relayout_and_repack(csp_batch *b, const std::vector<size_t> &item_of, Reduction &R) {
    hipStream_t st = b->stream;
    const int nimg = int(b->imgs.size());
    b->n_reduced = uint32_t(R.jobs.size() + R.pjobs.size());
    b->raw_total = 0;
    b->fixed.clear();
    for (int i = 0; i < nimg; i++) {
        PngImg &im = b->imgs[i];
        const PngItem &it = b->items[item_of[i]];
        b->raw_total += im.raw_len;
        im.fix_off = b->fixed.size(); im.prefix_len = uint32_t(it.prefix.size()); im.suffix_len = uint32_t(it.suffix.size());
        b->fixed.insert(b->fixed.end(), it.prefix.begin(), it.prefix.end());
        b->fixed.insert(b->fixed.end(), it.suffix.begin(), it.suffix.end());
    }
    R.jobs.push_back(ReduceJob{}); R.pjobs.push_back(PaletteJob{});   // never empty uploads
    R.palettes.push_back(0);
    if (b->d_fixed.upload(b->fixed, st) || b->d_pjobs.upload(R.pjobs, st) || b->d_slot_index.upload(R.slot_index, st) || b->d_qpal.upload(R.palettes, st) ||
        hipMemcpyAsync(b->d_imgs.p, b->imgs.data(), sizeof(PngImg) * nimg, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemcpyAsync(b->d_jobs.p, R.jobs.data(), sizeof(ReduceJob) * R.jobs.size(), hipMemcpyHostToDevice, st) != hipSuccess) { csh_set_error("PNG reduction upload failed"); return -1; }
    R.remaps.resize(R.remaps.size() + 256, 0);   // never an empty upload
    DevBuf<uint8_t> d_remaps;
    if (d_remaps.upload(R.remaps, st)) return -1;
    launch_png_repack(st, b->d_imgs.p, b->d_jobs.p, int(R.jobs.size()) - 1, R.max_height, b->d_work.p, b->d_work.p, d_remaps.p);
    launch_png_indexed(st, b->d_imgs.p, b->d_pjobs.p, int(R.pjobs.size()) - 1, R.max_height, b->d_keys.p, b->d_slot_index.p, b->d_work.p, b->d_work.p);
    DevBuf<int16_t> d_lines;   // the error rows the bands of k_png_dither hand down (freed behind the synchronisation below)
    if (R.dither_steps) {
        if (R.dither_steps > 0x3FFFFFFFull || d_lines.alloc(size_t(R.dither_pixels) * 4 + 4)) { csh_set_error("PNG dither buffers failed"); return -1; }
        launch_png_dither(st, b->d_imgs.p, b->d_pjobs.p, int(R.pjobs.size()) - 1, int(R.dither_steps), b->d_qpal.p, b->d_work.p, b->d_work.p, d_lines.p);
    }
    return upload_chunk_index(b);   // synchronises: the job vectors may go out of scope
}

}  // namespace

int reduce_step(csp_batch *b) {
    const int nimg = int(b->imgs.size());
    b->reduced = true;
    bool any = false;
    for (int i = 0; i < nimg; i++) any |= b->flags0[i] != 0 || b->cand0[i] != 0;
    if (!any || !nimg) return 0;
    Analysis A(nimg);
    if (analyze(b, A)) return -1;
    std::vector<size_t> item_of(nimg, 0);
    for (size_t n = 0; n < b->items.size(); n++) if (b->items[n].image >= 0) item_of[b->items[n].image] = n;
    Palettes qpal;
    if (b->lossy && lossy_palettes(b, A, qpal)) return -1;
    Reduction R(nimg);
    bool changed = false;
    for (int i = 0; i < nimg; i++) {
        bool c = false;
        if (A.status[i]) continue;
        if (reduce_image(b, i, A, qpal, b->items[item_of[i]], R, &c)) return -1;
        changed |= c;
    }
    return changed ? relayout_and_repack(b, item_of, R) : 0;
}

}  // namespace csp
