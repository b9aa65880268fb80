// du_decode_par.cpp -- device unit over caesium-clt_amd/csrc/k_decode_par.hip: k_dec_mark_pending and k_dec_chain, the label chain that settles the
// block-in-MCU labels of the scans still on the relaxation list, through their launchers and on arrays the test makes up (no stream is decoded: the
// hypotheses k_dec_dense<3> would have written are an input).  Deterministic: one lane per scan, a scan's sub-sequences in order.  See du_common.h.
#include "../../caesium-clt_amd/csrc/k_decode_par.hip"
#include "du_common.h"
using namespace csh;

extern "C" {
// scans: [nps][6] = kind (types.h CSH_PS_*), image, nb_mcu, bits_len, clean_len, sub_base; the scan's index is its par_index, as the planner numbers them.
// state: [total_sub + nps] in and out (a scan's states start at sub_base + par_index); nblk: [total_sub] in and out; hyp: [total_sub][10];
// list: nlist entries scan << 32 | sub-sequence; scan_pending: [nps] out; need_seq: [nimg + CSH_DEC_NSTATS] in and out, the counters behind the images' words
int csdu_dec_chain(int nps, const int32_t *scans, int nimg, int total_sub, uint64_t *state, uint32_t *nblk, const uint16_t *hyp, const uint64_t *list, int nlist,
                   uint32_t *scan_pending, uint32_t *need_seq) {
    if (nps <= 0 || nimg <= 0 || total_sub <= 0 || nlist < 0 || nlist > total_sub) return -1;
    std::vector<ParScan> pss;
    pss.resize(size_t(nps));
    for (int i = 0; i < nps; i++) {
        const int32_t *s = scans + 6 * i;
        if (s[0] < 0 || s[0] > 4 || s[1] < 0 || s[1] >= nimg || s[2] < 1 || s[2] > 10 || s[3] < 0 || s[4] < 0 || s[5] < 0) return -1;
        const int64_t nsub = (int64_t(s[3]) + CSH_SUBSEQ_BYTES - 1) / CSH_SUBSEQ_BYTES;
        if (int64_t(s[5]) + nsub > total_sub) return -1;   // every sub-sequence the chain may visit has its row of hypotheses
        ParScan &ps = pss[size_t(i)];
        memset(&ps, 0, sizeof ps);
        ps.kind = s[0]; ps.image = s[1]; ps.nb_mcu = s[2]; ps.bits_len = uint32_t(s[3]); ps.clean_len = uint32_t(s[4]); ps.sub_base = uint32_t(s[5]); ps.par_index = uint32_t(i);
    }
    for (size_t i = 0; i < size_t(total_sub) * 10; i++) if (hyp[i] != 0xFFFF && (hyp[i] >> 12) >= 10) return -1;   // an exit label indexes the next row
    for (int i = 0; i < nlist; i++) if ((list[i] >> 32) >= uint64_t(nps)) return -1;
    DuBufs B;
    ParScan *d_pss;
    uint64_t *d_state, *d_list;
    uint32_t *d_nblk, *d_cnt, *d_pending, *d_need;
    uint16_t *d_hyp;
    const uint32_t cnt = uint32_t(nlist);
    const size_t nstate = size_t(total_sub) + size_t(nps);
    DU_TRY(B.upload(&d_pss, pss.data(), pss.size() * sizeof(ParScan)));
    DU_TRY(B.upload(&d_state, state, nstate * 8));
    DU_TRY(B.upload(&d_nblk, nblk, size_t(total_sub) * 4));
    DU_TRY(B.upload(&d_hyp, hyp, size_t(total_sub) * 10 * 2));
    DU_TRY(B.upload(&d_list, list, size_t(nlist) * 8));
    DU_TRY(B.upload(&d_cnt, &cnt, 4));
    DU_TRY(B.zeroed(&d_pending, size_t(nps) * 4));   // (as the run does in front of launch_dec_mark_pending)
    DU_TRY(B.upload(&d_need, need_seq, (size_t(nimg) + CSH_DEC_NSTATS) * 4));
    launch_dec_mark_pending(0, d_pss, uint32_t(total_sub), d_list, d_cnt, d_pending);
    launch_dec_chain(0, d_pss, nps, d_state, d_nblk, d_hyp, d_pending, d_need, d_need + nimg);
    DU_TRY(du_finish());
    DU_TRY(du_download(state, d_state, nstate * 8));
    DU_TRY(du_download(nblk, d_nblk, size_t(total_sub) * 4));
    DU_TRY(du_download(scan_pending, d_pending, size_t(nps) * 4));
    return du_download(need_seq, d_need, (size_t(nimg) + CSH_DEC_NSTATS) * 4);
}
}
