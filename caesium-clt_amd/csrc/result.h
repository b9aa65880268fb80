// result.h -- the one maker of a CCSResult and the one reader of a file's magic bytes (host only)
#pragma once
#include <cstdlib>
#include <cstring>

#include "../../include/caesium_hip.h"

// success for code 0; any other code with a malloc'd copy of msg (cs_free_result releases it)
static inline CCSResult make_result(int code, const char *msg) {
    CCSResult r;
    r.success = code == 0; r.code = uint32_t(code); r.error_message = nullptr;
    if (code && msg) { size_t n = strlen(msg); char *m = static_cast<char *>(malloc(n + 1)); memcpy(m, msg, n + 1); r.error_message = m; }
    return r;
}

static inline int sniff(const uint8_t *d, size_t n) {
    if (n >= 3 && d[0] == 0xFF && d[1] == 0xD8 && d[2] == 0xFF) return CS_TYPE_JPEG;
    if (n >= 8 && !memcmp(d, "\x89PNG\r\n\x1a\n", 8)) return CS_TYPE_PNG;
    if (n >= 12 && !memcmp(d, "RIFF", 4) && !memcmp(d + 8, "WEBP", 4)) return CS_TYPE_WEBP;
    if (n >= 6 && (!memcmp(d, "GIF87a", 6) || !memcmp(d, "GIF89a", 6))) return CS_TYPE_GIF;
    if (n >= 4 && (!memcmp(d, "II*\0", 4) || !memcmp(d, "MM\0*", 4))) return CS_TYPE_TIFF;
    return CS_TYPE_UNKN;
}
