// du_runtime.cpp -- what the kernel sources expect from the library they are normally part of, and the unit library's own two questions.  See du_common.h.
#include <cstdarg>

#include "du_common.h"

#ifdef CSH_EMUL
thread_local dim3 threadIdx, blockIdx, blockDim, gridDim;   // the emulation runtime's lane coordinates (pipeline.cpp defines them for the library)
thread_local int csh_emul_phase = 0;
int csh_emul_reverse = 0;
#endif
static char du_error[512];
void csh_set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(du_error, sizeof du_error, fmt, ap);
    va_end(ap);
}

extern "C" {
int csdu_is_emul() {
#ifdef CSH_EMUL
    return 1;
#else
    return 0;
#endif
}
// devices visible, or -(HIP error code)
int csdu_device_count() {
    int n = 0;
    const int e = int(hipGetDeviceCount(&n));
    return e ? -e : n;
}
const char *csdu_last_error() { return du_error; }
// the emulation runs the lanes of a launch in the other order (gpu_rt.h csh_emul_reverse): nothing here may depend on it
void csdu_set_reverse(int on) {
#ifdef CSH_EMUL
    csh_emul_reverse = on;
#else
    (void)on;
#endif
}
}
