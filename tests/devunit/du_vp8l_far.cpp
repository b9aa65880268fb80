// du_vp8l_far.cpp -- device unit over caesium-clt_amd/csrc/k_vp8l_far.hip: the link stage (the three passes of the stable radix sort and k_vp8l_far_link) and
// k_vp8l_match_far, launched as the coder launches them (launch_vp8l_far_links, launch_vp8l_far_match), over a raw array of residual words of a given width;
// what comes back is prev[] and the candidates tok[] (bits 0-15 the length, from bit 16 the distance).  See du_common.h.
#include "../../caesium-clt_amd/csrc/k_vp8l_far.hip"
#include "du_common.h"
using namespace csw;

// the host symbol of another file that this one's launcher names (k_vp8l_groups.hip has it; launch_vp8l_token_stages comes with k_vp8l_refs.hip in
// du_vp8l_refs.cpp, which is linked into the same library); nothing here launches the coder
namespace csw {
void launch_vp8l_group_stages(hipStream_t, const Vp8lImg *, int, uint32_t, const uint32_t *, const Vp8lRefs &) {}
}  // namespace csw

extern "C" {
// refused: no words, a width that does not divide them, a picture the coder would refuse
int csdu_vp8l_far(const uint32_t *px, int n, int width, uint32_t *prev, uint64_t *tok) {
    if (n <= 0 || width <= 0 || width > 16384 || n % width || n / width > 16384) return -1;
    Vp8lImg im;
    memset(&im, 0, sizeof im);
    im.width = uint32_t(width); im.height = uint32_t(n / width);
    im.nchunk = (uint32_t(n) + VP8L_CHUNK - 1) / VP8L_CHUNK;
    DuBufs B;
    Vp8lImg *d_im;
    uint32_t *d_px;
    Vp8lFar F;
    memset(&F, 0, sizeof F);
    const size_t words = size_t(n) * 4;
    DU_TRY(B.upload(&d_im, &im, sizeof im));
    DU_TRY(B.upload(&d_px, px, words));
    DU_TRY(B.zeroed(&F.pos[0], words, 0x55));
    DU_TRY(B.zeroed(&F.pos[1], words, 0x55));
    DU_TRY(B.zeroed(&F.prev, words, 0x55));
    DU_TRY(B.zeroed(&F.cnt, size_t(im.nchunk) * 256 * 4, 0x55));
    DU_TRY(B.zeroed(&F.dtot, size_t(VP8L_FAR_TOT) * 4));
    DU_TRY(B.zeroed(&F.B.tok, size_t(n) * 8, 0x55));
    launch_vp8l_far_links(0, d_im, 1, uint64_t(n), d_px, F);
    launch_vp8l_far_match(0, d_im, 1, uint64_t(n), d_px, F);
    DU_TRY(du_finish());
    DU_TRY(du_download(prev, F.prev, words));
    return du_download(tok, F.B.tok, size_t(n) * 8);
}
}
