// scan_search.cpp -- the host half of the JPEG batch's scan search.
// The host side of mozjpeg's scan search (jcmaster.c select_scans [UPSTREAM-RECALL]; the statement the oracle is pinned with:
// oracle/jpeg_oracle.c cso_search_progression).  The device has coded a stage's candidate scans; their sizes (DHT + SOS + stuffed data)
// come back and the decisions are replayed per image in mozjpeg's own order -- which is also what decides whether an image needs a
// conditional stage at all:
//   after ST_1   luma Al 0, 1, 2 in turn (stop at the first that is not cheaper); chroma Al 0, 1, 2 likewise.  Al 2 cheaper than Al 1:
//                the image wants luma at Al 3 tried (ST_1B)
//   after ST_1B  luma Al 3.  Then the Al of the frequency-split candidates is known: their work items and token plans are patched
//   after ST_2   whole band, split at 2, split at 8 (= stage 1's band pair at the chosen Al: search_work), [stop if the whole band still
//                leads], split at 5, [stop unless the split at 8 leads]: luma and chroma apart.  Not stopped: the split at 12 (ST_2B)
//   after ST_2B  split at 12, [stop unless it leads].  Not stopped: the split at 18 (ST_2C)
//   after ST_2C  split at 18.  Then every file's list of scans.
// Candidate numbering: cso_search_progression's.

#include <algorithm>

#include "batch.hpp"

namespace csh {

enum { kLumaSplit0 = 12, kNLuma = 23, kChromaBase = 26, kChromaSplit0 = 42 };
// the work item that holds candidate `cand` of an image: its own, or -- the split at 8 -- stage 1's band scans at the chosen Al
static int search_work(const SearchImg &si, int cand) {
    if (cand == kLumaSplit0 + 3 || cand == kLumaSplit0 + 4) return si.cand_work[1 + 3 * si.Al_luma + (cand - (kLumaSplit0 + 3))];
    if (cand >= kChromaSplit0 + 6 && cand <= kChromaSplit0 + 9) return si.cand_work[kChromaBase + 6 * si.Al_chroma + (cand - (kChromaSplit0 + 6))];
    return si.cand_work[cand];
}
int search_costs(csh_batch *b, AsmCtx &a, int stage) {
    hipStream_t st = b->stream;
    const Stage &sg = b->enc.stage[stage];
    a.work0 = int(sg.work0); a.nwork_run = int(sg.nwork);
    launch_scan_cost(st, a);
    b->enc.h_cost.resize(b->enc.swork.size());
    CSH_CHECK(hipMemcpyAsync(b->enc.h_cost.data() + sg.work0, b->enc.d_scan_cost.p + sg.work0, size_t(sg.nwork) * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    CSH_CHECK(hipStreamSynchronize(st));
    return 0;
}
// marks the work items of `stage` of every image for which want(image's search) is non-zero (bit 0 luma, bit 1 chroma); returns how many images that is
uint32_t search_gate(csh_batch *b, int stage, int (*want)(const SearchImg &)) {
    const Stage &sg = b->enc.stage[stage];
    b->enc.work_active.resize(b->enc.swork.size());
    uint32_t nimg = 0;
    std::vector<char> on(size_t(b->nimg), 0);
    for (int i = 0; i < b->nimg; i++) { const int m = want(b->enc.simg[size_t(i)]); on[size_t(i)] = char(m); if (m) nimg++; }
    for (uint32_t wi = sg.work0; wi < sg.work0 + sg.nwork; wi++) {
        const ScanWork &w = b->enc.swork[wi];
        const int comp = b->enc.script[size_t(w.scan)].comp[0];
        b->enc.work_active[wi] = uint8_t((on[size_t(w.image)] & (comp == 0 ? 1 : 2)) ? 1 : 0);   // want: bit 0 luma, bit 1 chroma
    }
    return nimg;
}
int search_decide(csh_batch *b, int stage) {
    hipStream_t st = b->stream;
    for (int i = 0; i < b->nimg; i++) {
        SearchImg &si = b->enc.simg[size_t(i)];
        const ImgDesc &im = b->imgs[size_t(i)];
        if (si.fixed) continue;
        auto size = [&](int cand) -> uint64_t { return b->enc.h_cost[size_t(search_work(si, cand))]; };
        auto luma_split = [&](int idx) { return idx == 0 ? size(kLumaSplit0) : size(kLumaSplit0 + 2 * idx - 1) + size(kLumaSplit0 + 2 * idx); };
        auto chroma_split = [&](int idx) {
            if (idx == 0) return size(kChromaSplit0) + size(kChromaSplit0 + 1);
            uint64_t cost = 0;
            for (int k = 2; k <= 5; k++) cost += size(kChromaSplit0 + 4 * (idx - 1) + k);
            return cost;
        };
        // one step of the split loop (jcmaster.c): returns true when the search goes on to idx + 1
        auto split_step = [&](int idx, uint64_t cost, uint64_t &best, int &choice) {
            if (idx == 0) { best = cost; choice = 0; return true; }
            if (cost < best) { best = cost; choice = idx; }
            return !((idx == 2 && choice == 0) || (idx == 3 && choice != 2) || (idx == 4 && choice != 4) || idx == 5);
        };
        if (stage == EncodePlan::ST_1) {
            si.Al_luma = 0; si.Al_chroma = 0; si.luma_on = true; si.chroma_on = false;
            for (int Al = 0; Al <= 2 && si.luma_on; Al++) {   // candidates 1+3Al, 2+3Al: the two band scans at Al; 3+3k: the refinements that bring it back to 0
                uint64_t cost = size(1 + 3 * Al) + size(2 + 3 * Al);
                for (int k = 0; k < Al; k++) cost += size(3 + 3 * k);
                if (Al == 0 || cost < si.best_luma) { si.best_luma = cost; si.Al_luma = Al; } else si.luma_on = false;
            }
            if (im.ncomp == 3)
                for (int Al = 0; Al <= 2; Al++) {
                    uint64_t cost = 0;
                    for (int k = 0; k < 4; k++) cost += size(kChromaBase + 6 * Al + k);
                    for (int k = 0; k < Al; k++) cost += size(kChromaBase + 4 + 6 * k) + size(kChromaBase + 5 + 6 * k);
                    if (Al == 0 || cost < si.best_chroma) { si.best_chroma = cost; si.Al_chroma = Al; } else break;
                }
        } else if (stage == EncodePlan::ST_1B) {
            if (si.luma_on) {
                const uint64_t cost = size(10) + size(11) + size(3) + size(6) + size(9);
                if (cost < si.best_luma) { si.best_luma = cost; si.Al_luma = 3; }
                si.luma_on = false;
            }
        } else if (stage == EncodePlan::ST_2) {
            si.luma_on = true;
            for (int idx = 0; idx <= 3 && si.luma_on; idx++) si.luma_on = split_step(idx, luma_split(idx), si.best_luma, si.split_luma);
            si.chroma_on = im.ncomp == 3;
            for (int idx = 0; idx <= 3 && si.chroma_on; idx++) si.chroma_on = split_step(idx, chroma_split(idx), si.best_chroma, si.split_chroma);
        } else {
            const int idx = stage == EncodePlan::ST_2B ? 4 : 5;
            if (si.luma_on) si.luma_on = split_step(idx, luma_split(idx), si.best_luma, si.split_luma);
            if (si.chroma_on) si.chroma_on = split_step(idx, chroma_split(idx), si.best_chroma, si.split_chroma);
        }
    }
    if (stage == EncodePlan::ST_1 || stage == EncodePlan::ST_1B) {
        // once no image waits for ST_1B: the frequency-split stages are coded at the chosen Al -- their work items' scans, and the Al in their token plans
        bool pending = false;
        for (int i = 0; i < b->nimg && stage == EncodePlan::ST_1; i++) pending = pending || b->enc.simg[size_t(i)].luma_on;
        if (pending) return 0;
        for (int sid : {int(EncodePlan::ST_2), int(EncodePlan::ST_2B), int(EncodePlan::ST_2C)}) {
            const Stage &sg = b->enc.stage[sid];
            for (uint32_t wi = sg.work0; wi < sg.work0 + sg.nwork; wi++) {
                ScanWork &w = b->enc.swork[wi];
                const EncScan e = b->enc.script[size_t(w.scan)];
                const SearchImg &si = b->enc.simg[size_t(w.image)];
                const int Al = e.comp[0] == 0 ? si.Al_luma : si.Al_chroma;
                w.scan = b->enc.cand_script.at({e.comp[0], e.Ss, e.Se, 0, Al});
                w.list = b->enc.nzsets[size_t(b->enc.nzset_of[size_t(w.image) * CSH_MAX_COMPS + size_t(e.comp[0])])].list[Al];   // made by ST_1 (Al 0..2) or ST_1B (luma Al 3)
            }
            for (uint32_t pi = sg.plan0; pi < sg.plan0 + sg.nplans; pi++) {
                TokPlan &P = b->enc.plans[pi];
                const SearchImg &si = b->enc.simg[size_t(b->enc.plan_image[pi])];
                for (uint32_t k = 0; k < P.nslot; k++) P.s[k].Al = uint8_t(b->enc.plan_comp[pi] == 0 ? si.Al_luma : si.Al_chroma);
            }
            if (sg.nwork) CSH_CHECK(hipMemcpyAsync(b->enc.d_swork.p + sg.work0, b->enc.swork.data() + sg.work0, size_t(sg.nwork) * sizeof(ScanWork), hipMemcpyHostToDevice, st));
            launch_rebind_slots(st, b->enc.d_swork.p + sg.work0, sg.nwork, b->enc.d_nzlists.p, b->enc.d_slots.p);   // the slots name their list themselves (SlotRec::nzlist)
            if (sg.nplans) CSH_CHECK(hipMemcpyAsync(b->enc.d_plans.p + sg.plan0, b->enc.plans.data() + sg.plan0, size_t(sg.nplans) * sizeof(TokPlan), hipMemcpyHostToDevice, st));
        }
    }
    return 0;
}
// every file's list of scans: DC, luma bands, luma refinements down to the Al both share, chroma bands, chroma refinements down to it, then the
// shared refinements, luma first
int search_lists(csh_batch *b) {
    hipStream_t st = b->stream;
    for (int i = 0; i < b->nimg; i++) {
        const SearchImg &si = b->enc.simg[size_t(i)];
        const ImgDesc &im = b->imgs[size_t(i)];
        if (si.fixed) continue;   // its list was written with its work items (batch_plan.cpp output_scans)
        uint32_t *list = b->enc.img_list.data() + size_t(i) * CSH_LIST_MAX;
        uint32_t m = 0;
        auto put = [&](int cand) { list[m++] = uint32_t(search_work(si, cand)); };
        const int min_Al = im.ncomp == 3 ? std::min(si.Al_luma, si.Al_chroma) : si.Al_luma;
        put(0);
        if (si.split_luma == 0) put(kLumaSplit0); else { put(kLumaSplit0 + 2 * si.split_luma - 1); put(kLumaSplit0 + 2 * si.split_luma); }
        for (int Al = si.Al_luma - 1; Al >= min_Al; Al--) put(3 + 3 * Al);
        if (im.ncomp == 3) {
            if (si.split_chroma == 0) { put(kChromaSplit0); put(kChromaSplit0 + 1); }
            else for (int k = 2; k <= 5; k++) put(kChromaSplit0 + 4 * (si.split_chroma - 1) + k);
            for (int Al = si.Al_chroma - 1; Al >= min_Al; Al--) { put(kChromaBase + 6 * Al + 4); put(kChromaBase + 6 * Al + 5); }
        }
        for (int Al = min_Al - 1; Al >= 0; Al--) {
            put(3 + 3 * Al);
            if (im.ncomp == 3) { put(kChromaBase + 6 * Al + 4); put(kChromaBase + 6 * Al + 5); }
        }
        b->enc.img_nlist[size_t(i)] = m;
    }
    CSH_CHECK(hipMemcpyAsync(b->enc.d_img_list.p, b->enc.img_list.data(), b->enc.img_list.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    CSH_CHECK(hipMemcpyAsync(b->enc.d_img_nlist.p, b->enc.img_nlist.data(), b->enc.img_nlist.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    return 0;
}

}  // namespace csh
