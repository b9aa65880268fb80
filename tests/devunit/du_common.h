// du_common.h -- what the device-unit translation units share (tests/devunit/README.md).  Each unit includes ONE kernel source and drives single
// functions of it: a small __global__ kernel calls the function on inputs from a buffer, one case per lane or per wave, and writes what came back; an
// extern "C" entry allocates, copies, launches, waits and copies back, and returns the HIP error code (0 = ran).  The library is built twice from these
// sources -- hipcc for gfx950 (tests/devunit/libcsh_devunit.so) and g++ -DCSH_EMUL (tests/emul/libcsh_devunit_emul.so) -- so that the two branches of
// every CSH_EMUL conditional in the functions under test meet the same inputs and the same expected values (tests/_devunit_cases.py).
// Test infrastructure: never linked into libcaesium_hip.so.
#pragma once
#include "../../caesium-clt_amd/csrc/gpu_rt.h"
#include "../../caesium-clt_amd/csrc/png_wave.h"

#define DU_TRY(expr) do { const int e_ = int(expr); if (e_ != 0) return e_; } while (0)

// device buffers of one entry: freed together, whatever happened
struct DuBufs {
    void *p[8];
    int n = 0;
    template <class T> int alloc(T **out, size_t bytes) {
        void *q = nullptr;
        const int e = int(hipMalloc(&q, bytes ? bytes : 4));
        if (e == 0) { p[n++] = q; *out = reinterpret_cast<T *>(q); }
        return e;
    }
    template <class T> int upload(T **out, const void *src, size_t bytes) {
        int e = alloc(out, bytes);
        if (e == 0 && bytes) e = int(hipMemcpy(*out, src, bytes, hipMemcpyHostToDevice));
        return e;
    }
    template <class T> int zeroed(T **out, size_t bytes, int fill = 0) {
        int e = alloc(out, bytes);
        if (e == 0 && bytes) e = int(hipMemsetAsync(*out, fill, bytes, 0));
        return e;
    }
    ~DuBufs() { for (int i = 0; i < n; i++) (void)hipFree(p[i]); }
};
static inline int du_finish() {
    int e = int(hipGetLastError());
    if (e == 0) e = int(hipDeviceSynchronize());
    return e;
}
static inline int du_download(void *dst, const void *src, size_t bytes) { return bytes ? int(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost)) : 0; }

// A "wave kernel" in the dual idiom: the device runs it with 64 threads a wave, the emulation with one thread that plays the wave (png_wave.h).
// wpb: waves per workgroup (1 or 4: workgroups of 64 and of 256 threads).
#define DU_WAVE_INDEX() (blockIdx.x * (blockDim.x / CSP_WAVE_THREADS) + threadIdx.x / CSP_WAVE_THREADS)
#define DU_WAVE_LAUNCH(kern, nwaves, wpb, ...) CSH_LAUNCH(kern, dim3(unsigned((nwaves) / (wpb))), dim3(unsigned((wpb) * CSP_WAVE_THREADS)), 0, __VA_ARGS__)
