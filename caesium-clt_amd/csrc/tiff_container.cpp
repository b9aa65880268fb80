// tiff_container.cpp -- the walk over a classic TIFF file (magic 42, either byte order) for the TIFF route: every IFD of the main chain is a page;
// per page the tags that say how its strips or tiles are cut and coded, and every entry with the place of its value, checked to lie inside the file.  And the other
// direction: the values block and the IFD of an output page.  Host code only; nothing here interprets a sample.
#include <algorithm>
#include <cstring>
#include <unordered_set>

#include "tiff_batch.hpp"

using namespace cst;

namespace {
struct Rd {
    const uint8_t *d; size_t n; bool be;
    uint32_t u16(size_t at) const { return be ? (uint32_t(d[at]) << 8) | d[at + 1] : uint32_t(d[at]) | (uint32_t(d[at + 1]) << 8); }
    uint32_t u32(size_t at) const { return be ? (u16(at) << 16) | u16(at + 2) : u16(at) | (u16(at + 2) << 16); }
    // value k of an entry of BYTE / SHORT / LONG (or IFD) type; anything else reads as 0
    uint32_t val(const cst_entry &e, uint32_t k) const {
        if (k >= e.count) return 0;
        return e.type == 1 ? d[e.at + k] : e.type == 3 ? u16(e.at + 2 * size_t(k)) : (e.type == 4 || e.type == 13) ? u32(e.at + 4 * size_t(k)) : 0u;
    }
};
const uint32_t TYPE_SIZE[14] = {0, 1, 1, 2, 4, 8, 1, 1, 2, 4, 8, 4, 8, 4};
enum { READ_OK = 0, READ_BAD = 1, READ_PASS = 2 };

// the entries of the IFD at `off`; next: the offset behind them.  READ_PASS: a field type this walk cannot size
int read_ifd(const Rd &r, uint64_t off, std::vector<cst_entry> &out, uint32_t *next, std::string &msg) {
    if (off + 2 > r.n) { msg = "TIFF: an IFD offset outside the file"; return READ_BAD; }
    const uint32_t cnt = r.u16(size_t(off));
    if (off + 2 + 12 * uint64_t(cnt) + 4 > r.n) { msg = "TIFF: an IFD that ends behind the file"; return READ_BAD; }
    int rc = READ_OK;
    for (uint32_t k = 0; k < cnt; k++) {
        const size_t at = size_t(off) + 2 + 12 * size_t(k);
        cst_entry e;
        e.tag = uint16_t(r.u16(at)); e.type = uint16_t(r.u16(at + 2)); e.count = r.u32(at + 4);
        if (e.type == 0 || e.type > 13) { rc = READ_PASS; continue; }
        const uint64_t bytes = uint64_t(e.count) * TYPE_SIZE[e.type];
        uint64_t where = at + 8;
        if (bytes > 4) where = r.u32(at + 8);
        if (where + bytes > r.n) { msg = "TIFF: a value offset or count outside the file"; return READ_BAD; }
        e.at = size_t(where); e.bytes = size_t(bytes);
        out.push_back(e);
    }
    if (next) *next = r.u32(size_t(off) + 2 + 12 * size_t(cnt));
    return rc;
}
const cst_entry *find(const std::vector<cst_entry> &es, uint32_t tag) {
    for (const cst_entry &e : es) if (e.tag == tag) return &e;
    return nullptr;
}
bool dropped_without_metadata(uint32_t tag) {
    for (uint32_t t : {270u, 271u, 272u, 305u, 306u, 315u, 700u, 33432u, 33723u, 34377u, 34665u, 34853u}) if (t == tag) return true;
    return false;
}
}  // namespace

int cst_parse(const uint8_t *d, size_t n, bool keep_metadata, cst_file &f, std::string &msg) {
    f = cst_file();
    auto bad = [&](const char *m) { msg = m; return int(CS_ERR_BAD_TIFF); };
    if (n < 8 || (memcmp(d, "II", 2) && memcmp(d, "MM", 2))) return bad("TIFF: no header");
    f.big_endian = d[0] == 'M';
    const Rd r{d, n, f.big_endian};
    if (r.u16(2) != 42) return bad("TIFF: not a classic TIFF header (magic 42)");
    std::unordered_set<uint32_t> seen;
    uint64_t decoded = 0, units = 0;   // (units: rows and segments, which the kernels' grids count)
    for (uint32_t off = r.u32(4); off;) {
        if (!seen.insert(off).second) return bad("TIFF: the IFD chain loops");
        if (seen.size() > 65535) { f.pass = true; break; }
        cst_page_src s;
        uint32_t next = 0;
        const int rc = read_ifd(r, off, s.entries, &next, msg);
        if (rc == READ_BAD) return CS_ERR_BAD_TIFF;
        if (rc == READ_PASS) f.pass = true;
        off = next;
        const std::vector<cst_entry> &E = s.entries;
        auto num = [&](uint32_t tag, uint32_t dflt) { const cst_entry *e = find(E, tag); return e && e->count ? r.val(*e, 0) : dflt; };
        if (!find(E, 256) || !find(E, 257)) return bad("TIFF: a page without ImageWidth / ImageLength");
        s.width = num(256, 0); s.height = num(257, 0);
        if (!s.width || !s.height) return bad("TIFF: a page of zero width or height");
        s.spp = num(277, 1); s.comp = num(259, 1);
        if (!s.spp) return bad("TIFF: SamplesPerPixel is 0");
        if (s.spp > 65535) { f.pass = true; f.pages.push_back(s); continue; }   // (the tag is a SHORT by the text; the loop below runs once a sample)
        // BitsPerSample: the bits of a pixel are the samples' sum (a single value stands for every sample, as libtiff reads it)
        const cst_entry *bps = find(E, 258);
        uint64_t pixel_bits = 0;
        bool all8 = true, all16 = true;
        for (uint32_t k = 0; k < s.spp; k++) {
            const uint32_t b = bps ? r.val(*bps, bps->count == s.spp ? k : 0) : 1u;
            if (!b) return bad("TIFF: BitsPerSample is 0");
            pixel_bits += b; all8 = all8 && b == 8; all16 = all16 && b == 16;
            if (k == 0) s.bits = b;
        }
        if (pixel_bits > (1u << 20)) { f.pass = true; f.pages.push_back(s); continue; }   // (and a row's bits stay inside 64)
        s.pred_ok = s.spp > TIFF_PRED_MAX_SPP ? uint32_t(TIFF_PRED_NONE) : all8 ? uint32_t(TIFF_PRED_8) : all16 ? (f.big_endian ? uint32_t(TIFF_PRED_16BE) : uint32_t(TIFF_PRED_16LE)) : uint32_t(TIFF_PRED_NONE);
        const uint32_t predictor = num(317, 1);
        if (predictor == 2) { if (s.pred_ok == TIFF_PRED_NONE) f.pass = true; s.pred = s.pred_ok; }
        else if (predictor != 1) f.pass = true;
        if (s.comp != TIFF_C_NONE && s.comp != TIFF_C_LZW && s.comp != TIFF_C_DEFLATE && s.comp != TIFF_C_ADOBE_DEFLATE && s.comp != TIFF_C_PACKBITS) f.pass = true;
        if (num(284, 1) == 2 || num(266, 1) == 2 || find(E, 330)) f.pass = true;   // separate planes, bits from the low end, SubIFDs
        if (num(262, 0) == 6) {   // YCbCr: only without subsampling (the tag's default is 2 x 2)
            const cst_entry *ss = find(E, 530);
            if (!ss || ss->count < 2 || r.val(*ss, 0) != 1 || r.val(*ss, 1) != 1) f.pass = true;
        }
        s.tiled = find(E, 322) || find(E, 323) || find(E, 324) || find(E, 325);
        const cst_entry *offs = find(E, s.tiled ? 324 : 273), *cnts = find(E, s.tiled ? 325 : 279);
        if (!offs || !cnts || (s.tiled && (!find(E, 322) || !find(E, 323)))) return bad("TIFF: a page without its strip / tile offsets, byte counts or tile size");
        const uint64_t seg_w = s.tiled ? num(322, 0) : s.width;
        if (s.tiled) { s.tw = num(322, 0); s.tl = num(323, 0); if (!s.tw || !s.tl) return bad("TIFF: a tile of zero width or length"); }
        else { s.rps = num(278, 0xFFFFFFFFu); if (!s.rps) return bad("TIFF: RowsPerStrip is 0"); if (s.rps > s.height) s.rps = s.height; }
        const uint64_t rowbytes = (seg_w * pixel_bits + 7) / 8;
        s.seg_rows = s.tiled ? s.tl : s.rps;
        const uint64_t nseg = s.tiled ? uint64_t((s.width + s.tw - 1) / s.tw) * ((s.height + s.tl - 1) / s.tl) : (uint64_t(s.height) + s.rps - 1) / s.rps;
        const uint64_t rows = s.tiled ? nseg * s.tl : s.height;   // (a page too large for this route is passed through before its arrays are looked at)
        if (rowbytes > (uint64_t(1) << 31) || nseg > (1u << 20) || rows > (1u << 20) || rowbytes * rows > (uint64_t(1) << 31)) { f.pass = true; f.pages.push_back(s); continue; }
        if (offs->count != nseg || cnts->count != nseg) return bad("TIFF: strip / tile offsets or byte counts of the wrong length");
        s.rowbytes = uint32_t(rowbytes); s.nseg = uint32_t(nseg); s.decoded = rowbytes * rows;
        decoded += s.decoded; units += rows + nseg;
        if (!f.pass) {
            for (uint32_t k = 0; k < s.nseg; k++) {
                const uint64_t o = r.val(*offs, k), len = r.val(*cnts, k);
                if (o + len > n) return bad("TIFF: a strip / tile offset or byte count outside the file");
                if (s.comp == TIFF_C_LZW && len >= 2 && d[o] == 0 && (d[o + 1] & 1)) { f.pass = true; break; }   // old-style LZW (libtiff's test): codes from the low bit up
                if ((s.comp == TIFF_C_DEFLATE || s.comp == TIFF_C_ADOBE_DEFLATE) && (len < 2 || (d[o] & 0x0F) != 8 || (d[o] >> 4) > 7 || ((uint32_t(d[o]) << 8) | d[o + 1]) % 31 || (d[o + 1] & 0x20)))
                    return bad("TIFF: a Deflate strip / tile without a zlib header");
                s.seg_off.push_back(o); s.seg_len.push_back(len);
            }
        }
        if (keep_metadata && !f.pass) {
            for (int which = 0; which < 2; which++) {
                const cst_entry *p = find(E, which ? 34853 : 34665);
                if (!p || p->count != 1 || (p->type != 4 && p->type != 13)) continue;
                std::vector<cst_entry> &sub = which ? s.gps : s.exif;
                const int rs = read_ifd(r, r.val(*p, 0), sub, nullptr, msg);
                if (rs == READ_BAD) return CS_ERR_BAD_TIFF;
                if (rs == READ_PASS) f.pass = true;
                (which ? s.has_gps : s.has_exif) = true;
            }
        }
        f.pages.push_back(s);
    }
    if (f.pages.empty() && !f.pass) return bad("TIFF: no IFD");
    if (decoded > (uint64_t(1) << 31) || units > (1u << 25)) f.pass = true;
    return 0;
}

uint64_t cst_declared_bytes(const uint8_t *d, size_t n, uint64_t *units, bool *deflate) {
    cst_file f;
    std::string msg;
    if (units) *units = 0;
    if (deflate) *deflate = false;
    if (cst_parse(d, n, false, f, msg) || f.pass) return 0;
    uint64_t t = 0;
    for (const cst_page_src &s : f.pages) {
        t += s.decoded;
        if (units) *units += uint64_t(s.nseg) + (s.tiled ? uint64_t(s.nseg) * s.tl : s.height);
        if (deflate && (s.comp == TIFF_C_DEFLATE || s.comp == TIFF_C_ADOBE_DEFLATE)) *deflate = true;
    }
    return t;
}

void cst_write_head(const uint8_t *d, const cst_file &f, const cst_page_src &s, bool keep_metadata, uint32_t comp, bool with_pred, uint32_t nout, uint32_t rows_per_strip, std::vector<uint8_t> &heads,
                    std::vector<uint32_t> &relocs, TiffHead &H) {
    const bool be = f.big_endian;
    enum { CARRY, SHORT1, LONG1, SEG_OFF, SEG_CNT, SUB };
    struct Out { uint32_t tag; int kind; uint32_t imm; const cst_entry *src; const std::vector<cst_entry> *sub; uint32_t at; };
    std::vector<Out> es;
    for (const cst_entry &e : s.entries) {
        if (e.tag == 259 || e.tag == 273 || e.tag == 279 || e.tag == 278 || e.tag == 317 || e.tag == 324 || e.tag == 325) continue;
        if (!keep_metadata && dropped_without_metadata(e.tag)) continue;
        if (e.tag == 34665 || e.tag == 34853) {   // a private IFD is copied with what it points to; a pointer that is none is dropped
            if (e.tag == 34665 ? s.has_exif : s.has_gps) es.push_back(Out{e.tag, SUB, 0, &e, e.tag == 34665 ? &s.exif : &s.gps, 0});
            continue;
        }
        es.push_back(Out{e.tag, CARRY, 0, &e, nullptr, 0});
    }
    es.push_back(Out{259, SHORT1, comp, nullptr, nullptr, 0});
    es.push_back(Out{s.tiled ? 324u : 273u, SEG_OFF, 0, nullptr, nullptr, 0});
    es.push_back(Out{s.tiled ? 325u : 279u, SEG_CNT, 0, nullptr, nullptr, 0});
    if (!s.tiled) es.push_back(Out{278, LONG1, rows_per_strip, nullptr, nullptr, 0});
    if (with_pred) es.push_back(Out{317, SHORT1, 2, nullptr, nullptr, 0});
    std::stable_sort(es.begin(), es.end(), [](const Out &a, const Out &b) { return a.tag < b.tag; });

    std::vector<uint8_t> blob;
    std::vector<uint32_t> rel;
    auto even = [&]() { if (blob.size() & 1) blob.push_back(0); };
    auto p16 = [&](uint32_t v) { blob.push_back(uint8_t(be ? v >> 8 : v)); blob.push_back(uint8_t(be ? v : v >> 8)); };
    auto p32 = [&](uint32_t v) { if (be) { p16(v >> 16); p16(v & 0xFFFFu); } else { p16(v & 0xFFFFu); p16(v >> 16); } };
    auto offset32 = [&](uint32_t v) { rel.push_back(uint32_t(blob.size())); p32(v); };   // an offset into the blob: the blob's place is added on the device
    auto bytes = [&](const cst_entry &e) { even(); const uint32_t at = uint32_t(blob.size()); blob.insert(blob.end(), d + e.at, d + e.at + e.bytes); return at; };
    auto entry = [&](const cst_entry &e, uint32_t at) {   // a carried entry: its value in place, or the offset of its copy
        p16(e.tag); p16(e.type); p32(e.count);
        if (e.bytes > 4) offset32(at);
        else { for (size_t k = 0; k < 4; k++) blob.push_back(k < e.bytes ? d[e.at + k] : 0); }
    };
    memset(&H, 0, sizeof H);
    // the values, in tag order
    for (Out &o : es) {
        if (o.kind == CARRY && o.src->bytes > 4) o.at = bytes(*o.src);
        else if ((o.kind == SEG_OFF || o.kind == SEG_CNT) && nout > 1) { even(); o.at = uint32_t(blob.size()); blob.resize(blob.size() + 4 * size_t(nout), 0); }
        else if (o.kind == SUB) {   // the private IFD's values, then the private IFD (without its interoperability pointer, 40965)
            std::vector<uint32_t> at;
            for (const cst_entry &e : *o.sub) at.push_back(e.tag != 40965 && e.bytes > 4 ? bytes(e) : 0u);
            even();
            o.at = uint32_t(blob.size());
            uint32_t cnt = 0;
            for (const cst_entry &e : *o.sub) if (e.tag != 40965) cnt++;
            p16(cnt);
            for (size_t k = 0; k < o.sub->size(); k++) if ((*o.sub)[k].tag != 40965) entry((*o.sub)[k], at[k]);
            p32(0);
        }
    }
    even();
    H.ifd_pos = uint32_t(blob.size());
    p16(uint32_t(es.size()));
    for (const Out &o : es) {
        if (o.kind == CARRY) { entry(*o.src, o.at); continue; }
        p16(o.tag);
        if (o.kind == SHORT1) { p16(3); p32(1); p16(o.imm); p16(0); }
        else if (o.kind == LONG1) { p16(4); p32(1); p32(o.imm); }
        else if (o.kind == SUB) { p16(o.src->type); p32(1); offset32(o.at); }
        else {
            p16(4); p32(nout);
            (o.kind == SEG_OFF ? H.off_pos : H.cnt_pos) = nout > 1 ? o.at : uint32_t(blob.size());
            if (nout > 1) offset32(o.at); else p32(0);
        }
    }
    p32(0);
    heads.resize((heads.size() + 15) & ~size_t(15), 0);
    H.off = heads.size(); H.len = uint32_t(blob.size());
    H.reloc_first = uint32_t(relocs.size()); H.nreloc = uint32_t(rel.size());
    heads.insert(heads.end(), blob.begin(), blob.end());
    relocs.insert(relocs.end(), rel.begin(), rel.end());
}
