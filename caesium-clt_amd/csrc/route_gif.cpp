// route_gif.cpp -- GIF inputs under CSH_GIF=device / lossy: the csg_batch (container walk on the host; LZW decode, canvas walk, LZW coder and the
// assembly of the files on the device) and the route that feeds it in groups.  The output renders what the input renders, canvas for canvas: frames shrink to what
// changed, unchanged pixels are written transparent, the LZW streams are coded afresh; a file that did not get smaller comes back as it is.
#include <algorithm>
#include <cstring>

#include "gif_batch.hpp"
#include "routes.hpp"

using namespace csh;
using namespace csg;

namespace {
enum { K_DECODE, K_STATS, K_PACK, K_ENCODE, K_LAYOUT, K_HEAD, K_MERGE, K_NEAR };   // (K_ENCODE times whichever coder the batch runs: it runs one)
const char *const KERNEL_NAMES[CSG_NKERNELS] = {"gif_lzw_decode", "gif_anim_stats", "gif_anim_pack", "gif_lzw_encode", "gif_layout", "gif_frame_head", "gif_merge", "gif_near"};

uint32_t chunk_pixels_from_env() {
    const char *e = getenv("CSH_GIF_CHUNK");
    if (!e || !*e) return 16384;
    char *end = nullptr;
    const unsigned long v = strtoul(e, &end, 10);
    return (*end || v < 1024 || v > 1048576) ? 16384u : uint32_t(v);   // anything else is not a chunk size: the default stands
}
template <class T> T align64(T v) { return (v + 63) & ~T(63); }

struct Box { uint32_t x0 = 0xFFFFFFFFu, y0 = 0xFFFFFFFFu, x1 = 0, y1 = 0; bool empty() const { return x0 > x1 || y0 > y1; } };
Box unite(const Box &a, const Box &b) {
    if (a.empty()) return b;
    if (b.empty()) return a;
    Box r; r.x0 = std::min(a.x0, b.x0); r.y0 = std::min(a.y0, b.y0); r.x1 = std::max(a.x1, b.x1); r.y1 = std::max(a.y1, b.y1);
    return r;
}
}  // namespace

extern "C" const char *csg_kernel_name(int slot) { return slot >= 0 && slot < CSG_NKERNELS ? KERNEL_NAMES[slot] : ""; }

// distance 0: the exact coder
static int batch_create(const CByteArray *inputs, size_t count, const CCSParameters *p, int device, uint32_t distance, csg_batch **out) {
    *out = nullptr;
    if (hipSetDevice(device) != hipSuccess) { csh_set_error("hipSetDevice failed"); return CS_ERR_NO_DEVICE; }
    csg_batch *b = new csg_batch;
    b->device = device; b->inputs = inputs; b->keep_metadata = p->keep_metadata; b->chunk_pixels = chunk_pixels_from_env(); b->distance = distance;
    memset(&b->timing, 0, sizeof b->timing);
    if (hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking) != hipSuccess) { delete b; csh_set_error("hipStreamCreate failed"); return CS_ERR_NO_DEVICE; }
    b->have_stream = true;
    b->items.resize(count); b->parsed.resize(count);
    for (size_t i = 0; i < count; i++) {
        csg_batch::Item &it = b->items[i];
        csg_file &f = b->parsed[i];
        it.code = csg_parse(inputs[i].data, inputs[i].length, f, it.msg);
        if (it.code) { f = csg_file(); continue; }
        if (f.plain_text) { it.pass = true; continue; }
        uint64_t px = 0;
        for (const csg_frame_src &s : f.frames) px += uint64_t(s.w) * s.h;
        if (uint64_t(f.cw) * f.ch > (uint64_t(1) << 28) || px > (uint64_t(1) << 31) || f.frames.size() > 65535) {
            it.code = CS_ERR_UNSUPPORTED; it.msg = "GIF: a canvas of more than 2^28 pixels, frames of more than 2^31 pixels together or more than 65535 frames have no device path";
            continue;
        }
        it.file = int(b->files.size());
        b->files.push_back(GifFile{uint32_t(b->frames.size()), uint32_t(f.frames.size()), f.cw, f.ch, 0});
        b->file_item.push_back(i);
    }
    *out = b;
    return 0;
}

extern "C" int csg_batch_create(const CByteArray *inputs, size_t count, const CCSParameters *p, int device, csg_batch **out) {
    return batch_create(inputs, count, p, device, 0, out);   // (gif_quality is not read: this batch is pixel-exact)
}
// D = 100 - quality, the quality held to 1..100 (0 counts as 1, as in libcaesium; --lossless sets 100)
extern "C" int csg_batch_create_lossy(const CByteArray *inputs, size_t count, const CCSParameters *p, int device, csg_batch **out) {
    return batch_create(inputs, count, p, device, 100u - std::min(100u, std::max(1u, p->gif_quality)), out);
}

extern "C" void csg_batch_destroy(csg_batch *b) { delete b; }

extern "C" int csg_batch_run(csg_batch *b, csg_timing *t) {
    if (hipSetDevice(b->device) != hipSuccess) { csh_set_error("hipSetDevice failed"); return CS_ERR_NO_DEVICE; }
    const hipStream_t st = b->stream;
    csg_timing &T = b->timing;
    memset(&T, 0, sizeof T);
    T.chunk_pixels = b->chunk_pixels; T.lossy_distance = b->distance; T.n_files = uint32_t(b->items.size());
    hipEvent_t ev[2 * CSG_NKERNELS + 2] = {};
    bool launched[CSG_NKERNELS] = {false};
    auto timed = [&](int slot, auto fn) { (void)hipEventRecord(ev[2 * slot], st); fn(); (void)hipEventRecord(ev[2 * slot + 1], st); launched[slot] = true; };
    auto done = [&](int rc) { for (hipEvent_t &e : ev) if (e) (void)hipEventDestroy(e); if (t) *t = T; return rc; };
    for (hipEvent_t &e : ev) if (hipEventCreate(&e) != hipSuccess) { e = nullptr; csh_set_error("hipEventCreate failed"); return done(CS_ERR_NO_DEVICE); }
    (void)hipEventRecord(ev[2 * CSG_NKERNELS], st);

    // ---- the frames, their colour tables and their streams
    std::vector<GifFrame> &frames = b->frames;
    frames.clear(); b->frame_file.clear();
    std::vector<uint32_t> tables, table_n;   // 256 words a table, and how many of them the file gave
    std::vector<uint8_t> canon, data;
    uint64_t idx_bytes = 0, max_px = 0;
    auto add_table = [&](const uint8_t *rgb, size_t len) {
        const uint32_t at = uint32_t(tables.size() / 256), n = uint32_t(len / 3);
        tables.resize(tables.size() + 256, 0xFF000000u); canon.resize(canon.size() + 256); table_n.push_back(n);
        uint32_t *tb = &tables[size_t(at) * 256];
        for (uint32_t i = 0; i < n; i++) tb[i] = uint32_t(rgb[3 * i]) | (uint32_t(rgb[3 * i + 1]) << 8) | (uint32_t(rgb[3 * i + 2]) << 16) | 0xFF000000u;
        for (uint32_t i = 0; i < 256; i++) { uint32_t j = 0; while (j < std::min(i, n) && tb[j] != tb[i]) j++; canon[size_t(at) * 256 + i] = uint8_t(j < std::min(i, n) ? j : i); }   // the lowest index of the same colour
        return at;
    };
    for (size_t fi = 0; fi < b->files.size(); fi++) {
        const size_t item = b->file_item[fi];
        const csg_file &f = b->parsed[item];
        const uint8_t *d = b->inputs[item].data;
        b->files[fi].first = uint32_t(frames.size());
        b->items[item].palette = b->items[item].not_smaller = false;
        max_px = std::max(max_px, uint64_t(f.cw) * f.ch);
        const uint32_t global = f.gct.len ? add_table(d + f.gct.off, f.gct.len) : 0u;
        for (const csg_frame_src &s : f.frames) {
            GifFrame g;
            memset(&g, 0, sizeof g);
            g.x = s.x; g.y = s.y; g.w = s.w; g.h = s.h; g.flags = s.interlaced ? GIF_INTERLACED : 0u; g.disposal = s.disposal; g.odisposal = 1;
            g.transparent = s.transparent >= 0 ? uint32_t(s.transparent) : GIF_NO_INDEX;
            g.mcs = s.mcs;
            g.pal = s.lct.len ? add_table(d + s.lct.off, s.lct.len) : global;
            g.pal_n = uint32_t((s.lct.len ? s.lct.len : f.gct.len) / 3);
            uint32_t bits = 1; while ((1u << bits) < g.pal_n) bits++;
            g.omcs = std::max(2u, bits);
            // the output's code size follows the table; a transparent index it cannot code (the extension may name any of 0..255) leaves the file as it is
            if (g.transparent != GIF_NO_INDEX && g.transparent >= (1u << g.omcs)) b->items[item].palette = true;
            g.data_off = data.size(); g.data_len = uint32_t(s.data.size());
            data.insert(data.end(), s.data.begin(), s.data.end());
            data.resize(align64(data.size()), 0);
            g.idx_off = idx_bytes; idx_bytes += align64(uint64_t(s.w) * s.h);
            frames.push_back(g); b->frame_file.push_back(uint32_t(fi));
            T.in_bytes += s.data.size();
        }
    }
    data.resize(data.size() + 64, 0);
    const uint32_t nframes = uint32_t(frames.size()), nfiles = uint32_t(b->files.size());
    T.n_frames = nframes;
    for (const csg_batch::Item &it : b->items) if (it.code) T.n_failed++;
    b->out.clear();
    if (!nframes) { b->ran = true; return done(0); }

    std::vector<uint32_t> status(nframes, 0u), stats(size_t(nframes) * GIF_STAT, 0u), file_flags(nfiles, 0u);
    for (uint32_t k = 0; k < nframes; k++) for (int q : {0, 1, 4, 5}) stats[size_t(k) * GIF_STAT + q] = 0xFFFFFFFFu;
    DevBuf<uint32_t> d_status, d_stats, d_flags, d_frame_file, d_cbits;
    DevBuf<uint64_t> d_cstart, d_file_bytes;
    DevBuf<GifPlace> d_place;
    DevBuf<GifChunk> d_chunks;
    DevBuf<uint8_t> d_pack, d_cbuf, d_heads, d_out;
    if (b->d_data.upload(data, st) || b->d_tables.upload(tables, st) || b->d_canon.upload(canon, st) || b->d_frames.upload(frames, st) || b->d_files.upload(b->files, st) || b->d_idx.alloc(size_t(idx_bytes) + 64) ||
        b->d_idx.zero(st) || d_status.upload(status, st) || d_stats.upload(stats, st) || d_flags.upload(file_flags, st) || d_frame_file.upload(b->frame_file, st))
        return done(CS_ERR_NO_DEVICE);
    timed(K_DECODE, [&] { launch_gif_lzw_decode(st, b->d_frames.p, nframes, b->d_data.p, b->d_idx.p, d_status.p); });
    timed(K_STATS, [&] { launch_gif_anim(st, GIF_WALK_STATS, b->d_files.p, nfiles, max_px, b->d_frames.p, b->d_idx.p, b->d_tables.p, b->d_canon.p, d_stats.p, d_flags.p, nullptr, 0); });
    if (csh_copy_wait(status.data(), d_status.p, status.size() * 4, hipMemcpyDeviceToHost, st) != hipSuccess || csh_copy_wait(stats.data(), d_stats.p, stats.size() * 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipGetLastError() != hipSuccess) { csh_set_error("GIF: the LZW decoder or the change search failed on the device"); return done(CS_ERR_NO_DEVICE); }
    b->ran = true;   // the taps read the decoded rectangles from here on

    // ---- the output rule: rectangles and disposals from the boxes, chunks, head bytes
    std::vector<GifChunk> chunks;
    std::vector<uint8_t> heads;
    uint64_t pack_bytes = 0, cbuf_bytes = 0, out_bytes = 0;
    std::vector<GifFile> coded = b->files;   // the files of the second half: one that failed to decode, or is passed through already, takes no part in it (no frames)
    for (uint32_t fi = 0; fi < nfiles; fi++) {
        GifFile &F = coded[fi];
        const size_t item = b->file_item[fi];
        const csg_file &f = b->parsed[item];
        const uint8_t *d = b->inputs[item].data;
        auto box = [&](uint32_t k, int which) { Box r; if (k < F.nframes) { const uint32_t *s = &stats[size_t(F.first + k) * GIF_STAT + 4 * which]; r.x0 = s[0]; r.y0 = s[1]; r.x1 = s[2]; r.y1 = s[3]; } return r; };
        for (uint32_t k = 0; k < F.nframes; k++) if (status[F.first + k] != GIF_OK && !b->items[item].code) {
            b->items[item].code = CS_ERR_BAD_GIF; T.n_failed++;
            b->items[item].msg = status[F.first + k] == GIF_BAD_CODE ? "GIF: an LZW code beyond the next free table entry" : "GIF: the LZW data ends before the frame's rectangle is full";
        }
        if (b->items[item].code || b->items[item].palette) F.nframes = 0;
        uint64_t cap = 1;
        Box prev;
        for (uint32_t k = 0; k < F.nframes; k++) {
            GifFrame &g = frames[F.first + k];
            g.odisposal = (k + 1 < F.nframes && !box(k + 1, 1).empty()) ? 2u : 1u;
            Box r;
            if (k == 0) { r.x0 = r.y0 = 0; r.x1 = F.cw - 1; r.y1 = F.ch - 1; }
            else {
                r = unite(box(k, 0), box(k + 1, 1));
                if (frames[F.first + k - 1].odisposal == 2u) r = unite(r, prev);
                if (r.empty()) { r.x0 = r.y0 = r.x1 = r.y1 = 0; }
            }
            prev = r;
            g.ox = r.x0; g.oy = r.y0; g.ow = r.x1 - r.x0 + 1; g.oh = r.y1 - r.y0 + 1;
            const uint64_t npx = uint64_t(g.ow) * g.oh;
            g.out_off = pack_bytes; pack_bytes += align64(npx);
            g.first_chunk = uint32_t(chunks.size()); g.nchunks = uint32_t((npx + b->chunk_pixels - 1) / b->chunk_pixels);
            uint64_t coded = 0;
            for (uint32_t c = 0; c < g.nchunks; c++) {
                const uint64_t n = std::min<uint64_t>(b->chunk_pixels, npx - uint64_t(c) * b->chunk_pixels);
                chunks.push_back(GifChunk{F.first + k, c, cbuf_bytes});
                cbuf_bytes += gif_chunk_cap(n); coded += gif_chunk_cap(n);
            }
            g.head_off = heads.size();
            if (k == 0) csg_write_file_head(d, f, b->keep_metadata, heads);
            csg_write_frame_head(d, f.frames[k], g, heads);
            g.head_len = uint32_t(heads.size() - g.head_off);
            cap += g.head_len + coded + coded / 255 + 2;
        }
        F.out_off = b->files[fi].out_off = out_bytes; out_bytes += align64(cap);
    }
    heads.resize(heads.size() + 64, 0);
    const uint32_t nchunks = uint32_t(chunks.size());
    DevBuf<GifFile> d_coded;
    if (b->d_frames.upload(frames, st) || d_coded.upload(coded, st) || d_chunks.upload(chunks, st) || d_heads.upload(heads, st) || d_pack.alloc(size_t(pack_bytes) + 64) || d_cbuf.alloc(size_t(cbuf_bytes) + 64) ||
        d_cbits.alloc(nchunks) || d_cstart.alloc(nchunks) || d_place.alloc(nframes) || d_file_bytes.alloc(nfiles) || d_out.alloc(size_t(out_bytes) + 64))
        return done(CS_ERR_NO_DEVICE);
    const bool lossy = b->distance > 0;   // else the launches are the exact route's
    b->ntables = lossy ? uint32_t(table_n.size()) : 0u;
    if (lossy) {
        if (b->d_table_n.upload(table_n, st) || b->d_cand.alloc(size_t(b->ntables) * 256 * GIF_NEAR_ROW) || b->d_cand.zero(st) || b->d_cand_n.alloc(size_t(b->ntables) * 256)) return done(CS_ERR_NO_DEVICE);
        timed(K_NEAR, [&] { launch_gif_near(st, b->d_tables.p, b->d_canon.p, b->d_table_n.p, b->ntables, b->distance, b->d_cand.p, b->d_cand_n.p); });
    }
    timed(K_PACK, [&] { launch_gif_anim(st, GIF_WALK_PACK, d_coded.p, nfiles, max_px, b->d_frames.p, b->d_idx.p, b->d_tables.p, b->d_canon.p, d_stats.p, d_flags.p, d_pack.p, 0); });
    timed(K_ENCODE, [&] {
        if (lossy) launch_gif_lzw_encode_lossy(st, b->d_frames.p, d_chunks.p, nchunks, d_pack.p, b->d_cand.p, b->d_cand_n.p, d_cbuf.p, d_cbits.p, b->chunk_pixels);
        else launch_gif_lzw_encode(st, b->d_frames.p, d_chunks.p, nchunks, d_pack.p, d_cbuf.p, d_cbits.p, b->chunk_pixels);
    });
    timed(K_LAYOUT, [&] { launch_gif_layout(st, d_coded.p, nfiles, b->d_frames.p, d_cbits.p, d_cstart.p, d_place.p, d_file_bytes.p); });
    timed(K_HEAD, [&] { launch_gif_frame_head(st, d_coded.p, b->d_frames.p, d_frame_file.p, nframes, d_heads.p, d_place.p, d_out.p); });
    timed(K_MERGE, [&] { launch_gif_merge(st, d_coded.p, b->d_frames.p, d_frame_file.p, d_chunks.p, nchunks, d_cbuf.p, d_cbits.p, d_cstart.p, d_place.p, d_out.p); });
    (void)hipEventRecord(ev[2 * CSG_NKERNELS + 1], st);
    // ---- sizes, flags, bytes
    std::vector<uint64_t> file_bytes(nfiles, 0);
    if (csh_copy_wait(file_bytes.data(), d_file_bytes.p, size_t(nfiles) * 8, hipMemcpyDeviceToHost, st) != hipSuccess || csh_copy_wait(file_flags.data(), d_flags.p, size_t(nfiles) * 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipGetLastError() != hipSuccess) { csh_set_error("GIF: the coder failed on the device"); return done(CS_ERR_NO_DEVICE); }
    b->out.resize(size_t(out_bytes));
    for (uint32_t fi = 0; fi < nfiles; fi++) {
        csg_batch::Item &it = b->items[b->file_item[fi]];
        if (it.code) continue;
        if (it.palette || file_flags[fi]) { it.palette = true; T.n_passed_palette++; continue; }
        it.out_bytes = file_bytes[fi];
        T.out_bytes += it.out_bytes;
        if (it.out_bytes >= b->inputs[b->file_item[fi]].length) { it.not_smaller = true; T.n_not_smaller++; continue; }
        if (hipMemcpyAsync(b->out.data() + coded[fi].out_off, d_out.p + coded[fi].out_off, size_t(it.out_bytes), hipMemcpyDeviceToHost, st) != hipSuccess) { csh_set_error("GIF: reading the files back failed"); return done(CS_ERR_NO_DEVICE); }
    }
    if (hipStreamSynchronize(st) != hipSuccess) { csh_set_error("GIF: reading the files back failed"); return done(CS_ERR_NO_DEVICE); }
    for (int s = 0; s < CSG_NKERNELS; s++) if (launched[s]) (void)hipEventElapsedTime(&T.kernel_ms[s], ev[2 * s], ev[2 * s + 1]);
    (void)hipEventElapsedTime(&T.total_ms, ev[2 * CSG_NKERNELS], ev[2 * CSG_NKERNELS + 1]);
    return done(0);
}

extern "C" int csg_batch_fetch(csg_batch *b, CByteArray *outputs, CCSResult *results) {
    if (!b->ran && !b->files.empty()) { csh_set_error("csg_batch_fetch: batch not run"); return -1; }
    int failed = 0;
    for (size_t i = 0; i < b->items.size(); i++) {
        const csg_batch::Item &it = b->items[i];
        outputs[i].data = nullptr; outputs[i].length = 0;
        if (it.code) { results[i] = make_result(it.code, it.msg.c_str()); failed++; continue; }
        const bool same = it.pass || it.palette || it.not_smaller;   // the input's bytes
        const uint8_t *src = same ? b->inputs[i].data : b->out.data() + b->files[size_t(it.file)].out_off;
        const size_t len = same ? b->inputs[i].length : size_t(it.out_bytes);
        outputs[i].data = static_cast<uint8_t *>(malloc(len ? len : 1));
        if (!outputs[i].data) { results[i] = make_result(CS_ERR_NO_DEVICE, "out of memory"); failed++; continue; }
        memcpy(outputs[i].data, src, len); outputs[i].length = len;
        results[i] = make_result(0, nullptr);
    }
    return failed;
}

// ---- the tests' taps
static const csg_batch::Item *tap_item(csg_batch *b, size_t file, const char *who) {
    if (file >= b->items.size()) { csh_set_error("%s: index out of range", who); return nullptr; }
    return &b->items[file];
}
extern "C" int csg_batch_frames(csg_batch *b, size_t file, uint32_t *nframes, uint32_t *canvas_w, uint32_t *canvas_h) {
    *nframes = *canvas_w = *canvas_h = 0;
    const csg_batch::Item *it = tap_item(b, file, "csg_batch_frames");
    if (!it) return -1;
    if (it->code) return it->code;
    const csg_file &f = b->parsed[file];
    *nframes = uint32_t(f.frames.size()); *canvas_w = f.cw; *canvas_h = f.ch;
    return 0;
}
extern "C" int csg_batch_read_indices(csg_batch *b, size_t file, uint32_t frame, uint8_t *dst) {
    const csg_batch::Item *it = tap_item(b, file, "csg_batch_read_indices");
    if (!it) return -1;
    if (it->code) return it->code;
    if (!b->ran || it->file < 0 || frame >= b->files[size_t(it->file)].nframes) { csh_set_error("csg_batch_read_indices: batch not run / a file that is passed through / no such frame"); return -1; }
    if (hipSetDevice(b->device) != hipSuccess) { csh_set_error("hipSetDevice failed"); return CS_ERR_NO_DEVICE; }
    const GifFrame &g = b->frames[b->files[size_t(it->file)].first + frame];
    if (csh_copy_wait(dst, b->d_idx.p + g.idx_off, size_t(g.w) * g.h, hipMemcpyDeviceToHost, b->stream) != hipSuccess) { csh_set_error("csg_batch_read_indices: copy failed"); return CS_ERR_NO_DEVICE; }
    return 0;
}
extern "C" int csg_batch_read_canvas(csg_batch *b, size_t file, uint32_t frame, uint8_t *dst) {
    const csg_batch::Item *it = tap_item(b, file, "csg_batch_read_canvas");
    if (!it) return -1;
    if (it->code) return it->code;
    if (!b->ran || it->file < 0 || frame >= b->files[size_t(it->file)].nframes) { csh_set_error("csg_batch_read_canvas: batch not run / a file that is passed through / no such frame"); return -1; }
    if (hipSetDevice(b->device) != hipSuccess) { csh_set_error("hipSetDevice failed"); return CS_ERR_NO_DEVICE; }
    const std::vector<GifFile> one = {b->files[size_t(it->file)]};
    const uint64_t npx = uint64_t(one[0].cw) * one[0].ch;
    DevBuf<GifFile> d_one;
    DevBuf<uint8_t> d_canvas;
    if (d_one.upload(one, b->stream) || d_canvas.alloc(size_t(npx) * 4)) return CS_ERR_NO_DEVICE;
    launch_gif_anim(b->stream, GIF_WALK_CANVAS, d_one.p, 1, npx, b->d_frames.p, b->d_idx.p, b->d_tables.p, b->d_canon.p, nullptr, nullptr, d_canvas.p, frame);
    if (csh_copy_wait(dst, d_canvas.p, size_t(npx) * 4, hipMemcpyDeviceToHost, b->stream) != hipSuccess || hipGetLastError() != hipSuccess) { csh_set_error("canvas walk failed on the device"); return CS_ERR_NO_DEVICE; }
    return 0;
}

extern "C" int csg_batch_read_near(csg_batch *b, size_t file, uint32_t frame, uint8_t *cand, uint8_t *count) {
    const csg_batch::Item *it = tap_item(b, file, "csg_batch_read_near");
    if (!it) return -1;
    if (it->code) return it->code;
    if (!b->ran || it->file < 0 || frame >= b->files[size_t(it->file)].nframes) { csh_set_error("csg_batch_read_near: batch not run / a file that is passed through / no such frame"); return -1; }
    const uint32_t pal = b->frames[b->files[size_t(it->file)].first + frame].pal;
    if (!b->distance || pal >= b->ntables) {   // no distance (or nothing was coded): every index stands alone
        memset(cand, 0, 256 * GIF_NEAR_ROW);
        for (uint32_t i = 0; i < 256; i++) { cand[i * GIF_NEAR_ROW] = uint8_t(i); count[i] = 1; }
        return 0;
    }
    if (hipSetDevice(b->device) != hipSuccess) { csh_set_error("hipSetDevice failed"); return CS_ERR_NO_DEVICE; }
    if (csh_copy_wait(cand, b->d_cand.p + size_t(pal) * 256 * GIF_NEAR_ROW, 256 * GIF_NEAR_ROW, hipMemcpyDeviceToHost, b->stream) != hipSuccess ||
        csh_copy_wait(count, b->d_cand_n.p + size_t(pal) * 256, 256, hipMemcpyDeviceToHost, b->stream) != hipSuccess) { csh_set_error("csg_batch_read_near: copy failed"); return CS_ERR_NO_DEVICE; }
    return 0;
}

namespace route {

// GIF -> GIF: groups of at most 1024 files, sized by what they hold on the device -- per pixel of every frame the decoded index, the output index, a byte and a
// half of chunk buffer and as much of output, beside the file itself
int gif_compress(const CByteArray *inputs, size_t count, const CCSParameters *p, int device, CByteArray *outputs, CCSResult *results, bool lossy) {
    int failed_total = 0;
    for (size_t g0 = 0, n = 0; g0 < count; g0 += n) {
        n = group_extent(inputs + g0, count - g0, 1024, uint64_t(2) << 30, uint64_t(96) << 30, [](const CByteArray &f) { return uint64_t(1 << 20) + 2 * uint64_t(f.length) + csg_declared_pixels(f.data, f.length) * 6; });
        csg_batch *b = nullptr;
        int rc = lossy ? csg_batch_create_lossy(inputs + g0, n, p, device, &b) : csg_batch_create(inputs + g0, n, p, device, &b);
        if (rc == 0) rc = csg_batch_run(b, nullptr);
        if (rc != 0) {
            for (size_t i = 0; i < n; i++) { outputs[g0 + i].data = nullptr; outputs[g0 + i].length = 0; results[g0 + i] = make_result(rc, csh_last_error()); }
            failed_total += int(n);
        } else {
            const int failed = csg_batch_fetch(b, outputs + g0, results + g0);
            failed_total += failed < 0 ? int(n) : failed;
        }
        csg_batch_destroy(b);
    }
    return failed_total;
}

}  // namespace route
