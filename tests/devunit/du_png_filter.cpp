// du_png_filter.cpp -- device unit over caesium-clt_amd/csrc/k_png_filter.hip: the squared distance of the dither's palette search, dpk_sub + ddot2 on
// packed halves exactly as k_png_dither composes them.  See du_common.h.
#include "../../caesium-clt_amd/csrc/k_png_filter.hip"
#include "du_common.h"
using namespace csp;

// thread i: the wanted colour (wrg = r | g << 16, wba = b | a << 16) against one palette entry in the same form (a padding entry: 0x40004000 twice)
__global__ void __launch_bounds__(256) k_du_dither_dist(int n, const uint32_t *__restrict__ wrg, const uint32_t *__restrict__ wba, const uint32_t *__restrict__ prg, const uint32_t *__restrict__ pba,
                                                        uint32_t *__restrict__ out) {
    const int i = int(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= n) return;
    const uint32_t drg = dpk_sub(wrg[i], prg[i]), dba = dpk_sub(wba[i], pba[i]);
    out[i] = uint32_t(ddot2(drg, drg, ddot2(dba, dba, 0)));
}

extern "C" {
int csdu_dither_dist(int n, const uint32_t *wrg, const uint32_t *wba, const uint32_t *prg, const uint32_t *pba, uint32_t *out) {
    if (n <= 0) return -1;
    DuBufs B;
    uint32_t *d[4], *d_o;
    const uint32_t *src[4] = {wrg, wba, prg, pba};
    for (int k = 0; k < 4; k++) DU_TRY(B.upload(&d[k], src[k], size_t(n) * 4));
    DU_TRY(B.zeroed(&d_o, size_t(n) * 4, 0x55));
    CSH_LAUNCH(k_du_dither_dist, dim3(unsigned((n + 255) / 256)), dim3(256), 0, n, d[0], d[1], d[2], d[3], d_o);
    DU_TRY(du_finish());
    return du_download(out, d_o, size_t(n) * 4);
}
}
